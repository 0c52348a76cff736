// Jumanji board puzzles (Game2048, Minesweeper, SlidingTilePuzzle, RubiksCube, Snake, Maze): batched reset /
// step kernel, one env per lane, bit-exact with the reference.
//
// Replaces, for the whole batch in one launch, XxxEnv::{Reset,Step,WriteState} of envpool/jumanji/*_env.h
// plus the runtime (async_envpool.h:118-132, env.h:184-256).  The env bodies are jumanji_env.hip.h (shared
// with the host harness of the tests); one kernel instantiation per puzzle, so the puzzle switch folds away.
//
// Data layout (HBM), see DESIGN.md "Jumanji":
//   state  jm::<Puzzle>State [N]  env-major, read and written in place by the env's lane (64 B Game2048,
//                                 200 B Minesweeper, 108 B SlidingTilePuzzle, 56 B RubiksCube, 160 B Snake,
//                                 104 B Maze): the runtime-indexed cells (flood fill, shuffle, snake body,
//                                 fruit / tile placement) are global accesses, never scratch
//   init   int32 [100]            the parsed initial-state key, uploaded once per pool
//   mt     CommonDev, tiled (envs reset at their own times)
// Episode limits: SlidingTilePuzzle, RubiksCube, Snake and Maze end at their own time limit (Cfg::time_limit)
// and report trunc against that limit + 1 (their CurrentMaxEpisodeSteps), i.e. never; Game2048 and
// Minesweeper against the config's max_episode_steps.  Snake's reset fruit loop is bounded by the engine key
// "snake_max_tries": an exhausted bound sets the pool's error word (Pool::EnableErrorWord).
// Render: jumanji_render.hip.h painted by render_kernel.hip.h, one workgroup per band of a frame.
#include <algorithm>
#include <string>

#include "device_common.hip.h"
#include "engine.h"
#include "jumanji_env.hip.h"
#include "jumanji_render.hip.h"
#include "render_kernel.hip.h"

namespace epa {
namespace {

using jm::Cfg;

constexpr int kBlock = 256;
constexpr int kMaxEnvKeys = 7;
constexpr unsigned kErrTries = 1;  // Snake: the reset's fruit placement ran out of tries
constexpr unsigned kErrState = 2;  // set_state put a position off the board

struct JmDev {
  void* state;       // jm::State<P>::T [N]
  const int* init;   // kInitWords
  unsigned* err;
  int key_bytes[kMaxEnvKeys];  // row bytes of each env state key
  int act_dim;
};

// The env's generator as jumanji_env.hip.h draws from it: Mt19937::UniformInt / Canonical and the pair draw
// of std::shuffle: std::__gen_two_uniform_ints(b0, b1, g) (bits/stl_algo.h:3704-3711) is ONE
// uniform_int_distribution<unsigned long>{0, b0 * b1 - 1} draw split as (x / b1, x % b1), which with
// mt19937's 32-bit range and b0 * b1 <= 2^31 takes the same Lemire path as UniformInt.
struct JmGen : Mt19937 {
  using Mt19937::Mt19937;
  __device__ void UniformPair(uint32_t b0, uint32_t b1, int* p0, int* p1) {
    const uint32_t x = (uint32_t)UniformInt(0, (int)(b0 * b1 - 1u));
    *p0 = (int)(x / b1);
    *p1 = (int)(x % b1);
  }
};

template <int P>
__global__ __launch_bounds__(kBlock) void JumanjiStepKernel(JmDev d, CommonDev cm, StepArgs a,
                                                            const int* __restrict__ action, OutPtrs out, Cfg c) {
  using T = typename jm::State<P>::T;
  const int row = blockIdx.x * kBlock + threadIdx.x;
  if (row >= a.k) return;
  const int e = a.ids ? a.ids[row] - a.id_offset : row;
  bool done = cm.done[e] != 0;
  int cur = cm.cur_step[e];
  const bool reset = a.force_reset || done;  // async_envpool.h:127
  float reward = 0.0f;
  JmGen g(cm, e);
  T& s = static_cast<T*>(d.state)[e];
  if (reset) {
    cur = 0;
    if (!jm::ResetP<P>(g, c, d.init, s, &done)) {
      *d.err = kErrTries;
      done = true;  // (resets again on its next step)
    }
  } else {
    ++cur;
    reward = jm::StepP<P>(g, c, s, action + (size_t)row * d.act_dim, cur, &done);
  }
  g.Commit();
  cm.done[e] = done ? 1 : 0;
  cm.cur_step[e] = cur;
  // CurrentMaxEpisodeSteps: the puzzle's own limit + 1 where it has one
  WriteCommon(out, row, e + a.id_offset, cur, done, reward, c.time_limit > 0 ? c.time_limit + 1 : a.max_episode_steps);
  void* o[kMaxEnvKeys];
#pragma unroll
  for (int j = 0; j < kMaxEnvKeys; ++j) o[j] = static_cast<char*>(out.p[kKeyEnv0 + j]) + (size_t)row * d.key_bytes[j];
  jm::ObsP<P>(c, s, cur, o);
}

// flat state per env: cur_step, done, then jm::HiddenP's words
template <int P>
__global__ void JumanjiGetState(JmDev d, CommonDev cm, Cfg c, const int* ids, int k, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int e = ids[i];
  double* o = out + (size_t)i * (2 + jm::HiddenWords(P));
  o[0] = cm.cur_step[e];
  o[1] = cm.done[e];
  jm::HiddenP<P>(c, static_cast<const typename jm::State<P>::T*>(d.state)[e], cm.cur_step[e], o + 2);
}

template <int P>
__global__ void JumanjiSetState(JmDev d, CommonDev cm, const int* ids, int k, const double* in) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int e = ids[i];
  const double* o = in + (size_t)i * (2 + jm::HiddenWords(P));
  bool done = o[1] != 0.0;
  if (!jm::SetHiddenP<P>(static_cast<typename jm::State<P>::T*>(d.state)[e], o + 2)) {
    *d.err = kErrState;
    done = true;  // such an env resets on its next step
  }
  cm.cur_step[e] = (int)o[0];
  cm.done[e] = done ? 1 : 0;
}

// the render kernel's painter of puzzle P (render_kernel.hip.h)
template <int P>
struct JmPainter {
  using State = typename jm::State<P>::T;
  static __device__ void Paint(render::Canvas& cv, const State& s) { jm::Render(cv, s); }
};

int PuzzleOf(const std::string& family) {
  if (family == "Game2048") return jm::kGame2048;
  if (family == "Minesweeper") return jm::kMinesweeper;
  if (family == "SlidingTilePuzzle") return jm::kSlidingTile;
  if (family == "RubiksCube") return jm::kRubiksCube;
  if (family == "Snake") return jm::kSnake;
  return jm::kMaze;
}

// the reference's StateSpec key order of each puzzle (after the common keys), and its action
FamilySpec Spec(int p) {
  const KeySpec action{"action", EPA_I32, {}};
  switch (p) {
    case jm::kGame2048:
      return {{{"obs:board", EPA_I32, {4, 4}}, {"obs:action_mask", EPA_BOOL, {4}}, {"info:highest_tile", EPA_I32, {}}},
              action};
    case jm::kMinesweeper:
      return {{{"obs:board", EPA_I32, {10, 10}}, {"obs:action_mask", EPA_BOOL, {10, 10}},
               {"obs:num_mines", EPA_I32, {}}, {"obs:step_count", EPA_I32, {}}},
              {"action", EPA_I32, {2}}};
    case jm::kSlidingTile:
      return {{{"obs:puzzle", EPA_I32, {5, 5}}, {"obs:empty_tile_position", EPA_I32, {2}},
               {"obs:action_mask", EPA_BOOL, {4}}, {"obs:step_count", EPA_I32, {}},
               {"info:prop_correctly_placed", EPA_F32, {}}},
              action};
    case jm::kRubiksCube:
      return {{{"obs:cube", EPA_I8, {6, 3, 3}}, {"obs:step_count", EPA_I32, {}}}, {"action", EPA_I32, {3}}};
    case jm::kSnake:
      return {{{"obs:grid", EPA_F32, {12, 12, 5}}, {"obs:step_count", EPA_I32, {}}, {"obs:action_mask", EPA_BOOL, {4}}},
              action};
    default:
      return {{{"obs:agent_position.row", EPA_I32, {}}, {"obs:agent_position.col", EPA_I32, {}},
               {"obs:target_position.row", EPA_I32, {}}, {"obs:target_position.col", EPA_I32, {}},
               {"obs:walls", EPA_BOOL, {10, 10}}, {"obs:step_count", EPA_I32, {}}, {"obs:action_mask", EPA_BOOL, {4}}},
              action};
  }
}

size_t StateBytes(int p) {
  switch (p) {
    case jm::kGame2048: return sizeof(jm::Game2048State);
    case jm::kMinesweeper: return sizeof(jm::MinesweeperState);
    case jm::kSlidingTile: return sizeof(jm::SlidingTileState);
    case jm::kRubiksCube: return sizeof(jm::RubiksCubeState);
    case jm::kSnake: return sizeof(jm::SnakeState);
    default: return sizeof(jm::MazeState);
  }
}

// Config -> Cfg (+ the initial state words), with the checks that keep every access of the kernel inside the
// env's own state: positions on the board, a mine count the board can hold.  envpool_amd/jumanji parses the
// reference's string keys into these numeric ones (engine_config); the defaults are each puzzle's default config.
Cfg MakeCfg(int p, const Config& cfg, std::vector<int>* init) {
  Cfg c{};
  c.puzzle = p;
  const int limits[6] = {0, 0, 500, 200, 4000, 100};
  c.time_limit = (int)cfg.Get("time_limit", limits[p]);
  c.use_init = cfg.Get("use_init", 0) != 0 ? 1 : 0;
  c.add_random_cell = cfg.Get("add_random_cell", 1) != 0 ? 1 : 0;
  c.num_scrambles = (int)cfg.Get("num_scrambles", 100);
  c.num_mines = (int)cfg.Get("num_mines", 10);
  // Snake: head (0, 0), fruit (0, 1); Maze: agent (0, 0), target (9, 9)
  const int dflt[4] = {0, 0, p == jm::kMaze ? 9 : 0, p == jm::kSnake ? 1 : p == jm::kMaze ? 9 : 0};
  const int side = p == jm::kSnake ? 12 : 10;
  for (int i = 0; i < 4; ++i) {
    c.pos[i] = (int)cfg.Get("pos" + std::to_string(i), dflt[i]);
    if (c.pos[i] < 0 || c.pos[i] >= side) {
      throw std::invalid_argument("Jumanji: positions must be on the board (the reference clamps them)");
    }
  }
  if (c.time_limit < 0) throw std::invalid_argument("Jumanji: time_limit must be >= 0");
  if (c.num_mines < 0 || c.num_mines > 100) throw std::invalid_argument("Minesweeper: num_mines must be in [0, 100]");
  const double tries = cfg.Get("snake_max_tries", 1 << 20);
  if (tries < 1 || tries > 2147483647.0) throw std::invalid_argument("snake_max_tries must be in [1, 2^31)");
  c.max_tries = (int)tries;
  init->assign(jm::kInitWords, 0);
  for (int i = 0; i < jm::kInitWords; ++i) (*init)[i] = (int)cfg.Get("init" + std::to_string(i), 0);
  return c;
}

class JumanjiPool : public Pool {
 public:
  bool ConcurrentSafe() const override { return true; }  // per-env state + the launch's own rows only
  JumanjiPool(int p, const Config& cfg) : Pool(cfg, Spec(p), /*needs_rng=*/true), p_(p) {
    std::vector<int> init;
    c_ = MakeCfg(p, cfg, &init);
    const size_t n = (size_t)cfg.num_envs;
    d_.state = DevAlloc<char>(StateBytes(p) * n);
    d_.init = DevUpload(init.data(), jm::kInitWords);
    const int nkeys = (int)keys_.size() - kNumCommonKeys;  // the puzzle's own keys follow the common ones
    for (int j = 0; j < kMaxEnvKeys; ++j) d_.key_bytes[j] = j < nkeys ? keys_[kNumCommonKeys + j].row_bytes() : 0;
    d_.act_dim = action_.row_elems();
    EnableErrorWord();
    d_.err = err_dev_;
    mt_tile_default_ = 16;  // envs reset at their own times
    InitCommon();
  }
  int StateDim() const override { return 2 + jm::HiddenWords(p_); }
  void GetState(const int* d_ids, int k, double* d_out) override {
    auto kernel = JumanjiGetState<jm::kGame2048>;
    switch (p_) {
      case jm::kMinesweeper: kernel = JumanjiGetState<jm::kMinesweeper>; break;
      case jm::kSlidingTile: kernel = JumanjiGetState<jm::kSlidingTile>; break;
      case jm::kRubiksCube: kernel = JumanjiGetState<jm::kRubiksCube>; break;
      case jm::kSnake: kernel = JumanjiGetState<jm::kSnake>; break;
      case jm::kMaze: kernel = JumanjiGetState<jm::kMaze>; break;
      default: break;
    }
    hipLaunchKernelGGL(kernel, dim3((k + 255) / 256), dim3(256), 0, stream_, d_, common_, c_, d_ids, k, d_out);
  }
  void SetState(const int* d_ids, int k, const double* d_in) override {
    auto kernel = JumanjiSetState<jm::kGame2048>;
    switch (p_) {
      case jm::kMinesweeper: kernel = JumanjiSetState<jm::kMinesweeper>; break;
      case jm::kSlidingTile: kernel = JumanjiSetState<jm::kSlidingTile>; break;
      case jm::kRubiksCube: kernel = JumanjiSetState<jm::kRubiksCube>; break;
      case jm::kSnake: kernel = JumanjiSetState<jm::kSnake>; break;
      case jm::kMaze: kernel = JumanjiSetState<jm::kMaze>; break;
      default: break;
    }
    hipLaunchKernelGGL(kernel, dim3((k + 255) / 256), dim3(256), 0, stream_, d_, common_, d_ids, k, d_in);
  }
  void RenderSize(int width, int height, int* w, int* h) const override { jm::RenderSize(width, height, w, h); }
  void Render(const int* d_ids, int k, int w, int h, int /*camera_id*/, void* d_rgb) override {
    switch (p_) {
      case jm::kGame2048: return RenderP<jm::kGame2048>(d_ids, k, w, h, d_rgb);
      case jm::kMinesweeper: return RenderP<jm::kMinesweeper>(d_ids, k, w, h, d_rgb);
      case jm::kSlidingTile: return RenderP<jm::kSlidingTile>(d_ids, k, w, h, d_rgb);
      case jm::kRubiksCube: return RenderP<jm::kRubiksCube>(d_ids, k, w, h, d_rgb);
      case jm::kSnake: return RenderP<jm::kSnake>(d_ids, k, w, h, d_rgb);
      default: return RenderP<jm::kMaze>(d_ids, k, w, h, d_rgb);
    }
  }
  std::string ErrorText(unsigned code) const override {
    if (code == kErrTries) {
      return "Snake: a reset's fruit placement ran out of tries (snake_max_tries = " + std::to_string(c_.max_tries) +
             "); the reference would spin here";
    }
    if (code == kErrState) return "Jumanji: an env state put a position off the board (set_state)";
    return Pool::ErrorText(code);
  }

 protected:
  void Launch(const int* d_ids, int k, const void* d_action, bool force_reset, const OutPtrs& out) override {
    StepArgs a{d_ids, k, force_reset ? 1 : 0, cfg_.max_episode_steps, cfg_.env_id_offset};
    const int blocks = (k + kBlock - 1) / kBlock;
    auto kernel = JumanjiStepKernel<jm::kGame2048>;
    switch (p_) {
      case jm::kMinesweeper: kernel = JumanjiStepKernel<jm::kMinesweeper>; break;
      case jm::kSlidingTile: kernel = JumanjiStepKernel<jm::kSlidingTile>; break;
      case jm::kRubiksCube: kernel = JumanjiStepKernel<jm::kRubiksCube>; break;
      case jm::kSnake: kernel = JumanjiStepKernel<jm::kSnake>; break;
      case jm::kMaze: kernel = JumanjiStepKernel<jm::kMaze>; break;
      default: break;
    }
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream_, d_, common_, a,
                       static_cast<const int*>(d_action), out, c_);
  }

 private:
  template <int P>
  void RenderP(const int* d_ids, int k, int w, int h, void* d_rgb) {
    render::LaunchRender<JmPainter<P>>(static_cast<const typename jm::State<P>::T*>(d_.state), d_ids, k, w, h, d_rgb,
                                       stream_);
  }
  int p_;
  Cfg c_{};
  JmDev d_{};
};

}  // namespace

FamilySpec DescribeJumanji(const std::string& name, const Config&) { return Spec(PuzzleOf(name)); }

Pool* MakeJumanji(const std::string& name, const Config& cfg) { return new JumanjiPool(PuzzleOf(name), cfg); }

}  // namespace epa
