// MiniGrid navigation family: batched reset / step kernel, one env per lane, bit-exact with the reference.
//
// Replaces, for the whole batch in one launch, MiniGridEnv::{Reset,Step,WriteState}
// (envpool/minigrid/impl/minigrid_env.cc:31-76) for env_name empty / doorkey / distshift / crossing /
// lava_gap / dynamic_obstacles / four_rooms, plus the runtime (async_envpool.h:118-132, env.h:184-256).
// The env bodies are minigrid_env.hip.h (shared with the host harness of the tests).
//
// Data layout (HBM), see DESIGN.md "MiniGrid":
//   grid   uint16 [N][W*H]  env-major: a lane's view window is 7 short runs inside its own <= 722 bytes,
//                           and a reset writes that block from one lane (cell-major would make every window
//                           read 49 scattered 2-byte accesses one sector apart)
//   agent  int32  [N]       x | y << 8 | dir << 16
//   carry  uint16 [N]       carried object's cell word
//   obst   uint64 [N]       DynamicObstacles positions, byte i = x | y << 4
//   mt     CommonDev, tiled (envs reset at their own times)
// Outputs: ~290 B per env-step, 147 B image + 96 B mission of them.  The images of a block's 256 rows are
// staged in LDS and stored as 16-byte words by the whole block (the block's rows are one contiguous run of
// the image section); the mission is one constant 96-byte row per pool, stored the same way.
// Every rejection loop is bounded by the engine key "minigrid_max_tries": an exhausted bound sets the
// pool's error word (Pool::EnableErrorWord), which recv turns into an error.
#include <algorithm>
#include <cstring>
#include <string>

#include "device_common.hip.h"
#include "engine.h"
#include "minigrid_env.hip.h"

namespace epa {
namespace {

using mg::EnvState;
using mg::GridRef;
using mg::TaskCfg;

constexpr int kBlock = 256;
constexpr unsigned kErrTries = 1;   // a reset's rejection sampling ran out of tries
constexpr unsigned kErrState = 2;   // an env state (set_state) with the agent or an obstacle off the grid

struct MgDev {
  uint16_t* grid;
  int* agent;
  uint16_t* carry;
  uint64_t* obst;  // [N]
  const uint4* mission;  // kMissionBytes / 16 words
  unsigned* err;
  int cells;
  int n;
};

__device__ inline void LoadState(const MgDev& d, int e, EnvState& s) {
  const int a = d.agent[e];
  s.ax = a & 255;
  s.ay = (a >> 8) & 255;
  s.dir = (a >> 16) & 3;
  s.carry = d.carry[e];
  s.obst = d.obst ? d.obst[e] : 0;
}
__device__ inline void StoreState(const MgDev& d, int e, const EnvState& s, int n_obst) {
  d.agent[e] = (s.ax & 255) | ((s.ay & 255) << 8) | (s.dir << 16);
  d.carry[e] = s.carry;
  if (n_obst > 0) d.obst[e] = s.obst;
}
// The step reads the cell in front of the agent and the 3 x 3 neighbourhoods of the obstacles: both must be
// on the grid (the reference CHECKs InBounds; a state from set_state may say otherwise)
__device__ inline bool Steppable(const TaskCfg& c, const EnvState& s) {
  if (s.ax < 1 || s.ax > c.width - 2 || s.ay < 1 || s.ay > c.height - 2) return false;
  for (int i = 0; i < c.n_obstacles; ++i) {
    if (mg::ObstX(s.obst, i) >= c.width || mg::ObstY(s.obst, i) >= c.height) return false;
  }
  return true;
}

// The env's generator as minigrid_env.hip.h draws from it: Mt19937::UniformInt (uniform_int_distribution<int>)
// and the pair draw of std::shuffle.
struct MgGen : Mt19937 {
  using Mt19937::Mt19937;
  // std::__gen_two_uniform_ints(b0, b1, g) (bits/stl_algo.h:3704-3711): ONE
  // uniform_int_distribution<unsigned long>{0, b0 * b1 - 1} draw split as (x / b1, x % b1).  With mt19937's
  // 32-bit range and b0 * b1 <= 2^31 that distribution takes the same Lemire path as UniformInt
  // (uniform_int_dist.h:310-317 -> _S_nd<uint64_t>, :243-268).
  __device__ void UniformPair(uint32_t b0, uint32_t b1, int* p0, int* p1) {
    const uint32_t x = (uint32_t)UniformInt(0, (int)(b0 * b1 - 1u));
    *p0 = (int)(x / b1);
    *p1 = (int)(x % b1);
  }
};

// one instantiation per task: the task's code alone (the task switch of ResetEnv / StepEnv folds away)
template <int TASK>
__global__ __launch_bounds__(kBlock) void MiniGridStepKernel(MgDev d, CommonDev cm, StepArgs a,
                                                             const int* __restrict__ action, OutPtrs out,
                                                             TaskCfg c_arg) {
  // the fields MakeTaskCfg derives from the task alone, restated here as compile-time constants through the
  // same helpers (minigrid_env.hip.h), so that the task switch and the loops over them fold away
  TaskCfg c = c_arg;
  c.task = TASK;
  c.see_through = mg::SeeThroughWalls(TASK);
  if (mg::HasFixedSide(TASK)) c.width = c.height = mg::kMaxSide;
  if (!mg::HasObstacles(TASK)) c.n_obstacles = 0;
  __shared__ uint4 sh4[kBlock * mg::kImageBytes / 16];
  uint8_t* sh = reinterpret_cast<uint8_t*>(sh4);
  {  // one block per 256 rows (a grid-stride loop kept the kernel arguments live across its back edge: 50-250
     // SGPR spills per instantiation; without it none, and no scratch)
    const int base = blockIdx.x * kBlock;
    const int row = base + threadIdx.x;
    if (row < a.k) {
      const int e = a.ids ? a.ids[row] - a.id_offset : row;
      bool done = cm.done[e] != 0;
      int cur = cm.cur_step[e];
      const bool reset = a.force_reset || done;  // async_envpool.h:127
      float reward = 0.0f;
      MgGen g(cm, e);
      GridRef gr{d.grid + (size_t)e * d.cells, c.width};
      EnvState s;
      if (reset) {
        cur = 0;
        done = false;
        if (!mg::ResetEnv(g, gr, c, s)) {
          *d.err = kErrTries;
          done = true;  // (resets again on its next step)
          s.ax = s.ay = 1;
        }
      } else {
        LoadState(d, e, s);
        ++cur;
        if (Steppable(c, s)) {
          reward = mg::StepEnv(g, gr, c, s, action[row], cur, &done);
        } else {
          *d.err = kErrState;
          done = true;
        }
      }
      g.Commit();
      StoreState(d, e, s, c.n_obstacles);
      cm.done[e] = done ? 1 : 0;
      cm.cur_step[e] = cur;
      WriteCommon(out, row, e + a.id_offset, cur, done, reward, a.max_episode_steps);
      ((int*)out.p[kKeyEnv0])[row] = s.dir;
      ((int*)out.p[kKeyEnv0 + 3])[2 * row] = s.ax;
      ((int*)out.p[kKeyEnv0 + 3])[2 * row + 1] = s.ay;
      ((int*)out.p[kKeyEnv0 + 4])[row] = 0;  // mission_id of every task here
      mg::GenImage(gr, c, s, sh + threadIdx.x * mg::kImageBytes);
    }
    __syncthreads();
    // the block's rows [base, base + rows) are one contiguous run of the image and mission sections
    const int rows = min(kBlock, a.k - base);
    uint8_t* img = (uint8_t*)out.p[kKeyEnv0 + 1] + (size_t)base * mg::kImageBytes;
    const int bytes = rows * mg::kImageBytes;
    if ((reinterpret_cast<uintptr_t>(img) & 15u) == 0) {
      uint4* img4 = reinterpret_cast<uint4*>(img);
      for (int i = threadIdx.x; i < bytes / 16; i += kBlock) img4[i] = sh4[i];
      for (int j = (bytes & ~15) + threadIdx.x; j < bytes; j += kBlock) img[j] = sh[j];
    } else {
      for (int j = threadIdx.x; j < bytes; j += kBlock) img[j] = sh[j];
    }
    uint8_t* mis = (uint8_t*)out.p[kKeyEnv0 + 2] + (size_t)base * mg::kMissionBytes;
    constexpr int kMis4 = mg::kMissionBytes / 16;
    if ((reinterpret_cast<uintptr_t>(mis) & 15u) == 0) {
      uint4* mis4 = reinterpret_cast<uint4*>(mis);
      for (int i = threadIdx.x; i < rows * kMis4; i += kBlock) mis4[i] = d.mission[i % kMis4];
    } else {
      const uint8_t* src = reinterpret_cast<const uint8_t*>(d.mission);
      for (int j = threadIdx.x; j < rows * mg::kMissionBytes; j += kBlock) mis[j] = src[j % mg::kMissionBytes];
    }
  }
}

// flat state per env: cur_step, done, x, y, dir, carried (type, colour, state), 8 obstacles (x, y) (-1: none),
// then the grid encoding in DebugState order ((x * height + y) * 3 + channel)
constexpr int kHead = 8 + 2 * mg::kMaxObstacles;

__global__ void MiniGridGetState(MgDev d, CommonDev cm, TaskCfg c, const int* ids, int k, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int e = ids[i];
  EnvState s;
  LoadState(d, e, s);
  double* o = out + (size_t)i * (kHead + 3 * d.cells);
  o[0] = cm.cur_step[e];
  o[1] = cm.done[e];
  o[2] = s.ax;
  o[3] = s.ay;
  o[4] = s.dir;
  o[5] = mg::TypeOf(s.carry);
  o[6] = mg::ColorOf(s.carry);
  o[7] = mg::StateOf(s.carry);
  for (int j = 0; j < mg::kMaxObstacles; ++j) {
    const bool has = j < c.n_obstacles;
    o[8 + 2 * j] = has ? mg::ObstX(s.obst, j) : -1;
    o[9 + 2 * j] = has ? mg::ObstY(s.obst, j) : -1;
  }
  const GridRef gr{d.grid + (size_t)e * d.cells, c.width};
  for (int x = 0; x < c.width; ++x) {
    for (int y = 0; y < c.height; ++y) {
      const uint16_t v = gr.Get(x, y);
      double* q = o + kHead + (x * c.height + y) * 3;
      q[0] = mg::TypeOf(v);
      q[1] = mg::ColorOf(v);
      q[2] = mg::StateOf(v);
    }
  }
}

__global__ void MiniGridSetState(MgDev d, CommonDev cm, TaskCfg c, const int* ids, int k, const double* in) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int e = ids[i];
  const double* o = in + (size_t)i * (kHead + 3 * d.cells);
  EnvState s;
  s.ax = (int)o[2];
  s.ay = (int)o[3];
  s.dir = ((int)o[4]) & 3;
  s.carry = mg::MakeCell((int)o[5] & 15, (int)o[6] & 7, (int)o[7] & 3);
  s.obst = 0;
  for (int j = 0; j < c.n_obstacles; ++j) s.obst = mg::SetObst(s.obst, j, (int)o[8 + 2 * j] & 15, (int)o[9 + 2 * j] & 15);
  bool done = o[1] != 0.0;
  if (!Steppable(c, s)) {  // keep the grid and positions consistent: such an env resets on its next step
    *d.err = kErrState;
    done = true;
    s.ax = s.ay = 1;
  }
  const GridRef gr{d.grid + (size_t)e * d.cells, c.width};
  for (int x = 0; x < c.width; ++x) {
    for (int y = 0; y < c.height; ++y) {
      const double* q = o + kHead + (x * c.height + y) * 3;
      gr.Set(x, y, mg::MakeCell((int)q[0] & 15, (int)q[1] & 7, (int)q[2] & 3));
    }
  }
  StoreState(d, e, s, c.n_obstacles);
  cm.cur_step[e] = (int)o[0];
  cm.done[e] = done ? 1 : 0;
}

FamilySpec Spec() {
  return {{{"obs:direction", EPA_I32, {}},
           {"obs:image", EPA_U8, {mg::kView, mg::kView, 3}},
           {"obs:mission", EPA_U8, {mg::kMissionBytes}},
           {"info:agent_pos", EPA_I32, {2}},
           {"info:mission_id", EPA_I32, {}}},
          {"action", EPA_I32, {}}};
}

// Config -> TaskCfg, with the checks that keep every grid access of the kernel inside the env's block
// (the reference's constructors and CHECKs, where it has them)
TaskCfg MakeTaskCfg(const Config& cfg) {
  TaskCfg c{};
  c.task = (int)cfg.Get("env_name_code", -1);
  if (c.task < mg::kTaskEmpty || c.task > mg::kTaskFourRooms) {
    throw std::invalid_argument("MiniGrid: env_name_code must name one of the 7 navigation tasks");
  }
  c.size = (int)cfg.Get("size", 8);
  c.width = c.height = c.size;
  if (c.task == mg::kTaskDistShift) {
    c.width = (int)cfg.Get("width", 9);
    c.height = (int)cfg.Get("height", 7);
  } else if (mg::HasFixedSide(c.task)) {
    c.width = c.height = mg::kMaxSide;
  }
  if (c.width < 5 || c.height < 5 || c.width > mg::kMaxSide || c.height > mg::kMaxSide) {
    throw std::invalid_argument("MiniGrid: the grid sides (size, or width and height of distshift) must be in [5, 19]");
  }
  c.start_x = (int)cfg.Get("start_x", 1);
  c.start_y = (int)cfg.Get("start_y", 1);
  c.start_dir = (int)cfg.Get("start_dir", 0);
  const bool fixed_start = c.task == mg::kTaskEmpty || c.task == mg::kTaskDistShift || c.task == mg::kTaskDynObs;
  if (fixed_start && c.start_x >= 0 &&
      (c.start_x < 1 || c.start_x > c.width - 2 || c.start_y < 1 || c.start_y > c.height - 2 || c.start_dir < 0 ||
       c.start_dir > 3)) {
    throw std::invalid_argument("MiniGrid: agent_start_pos must be inside the walls, agent_start_dir in [0, 3]");
  }
  c.num_crossings = (int)cfg.Get("num_crossings", 1);
  if (c.task == mg::kTaskCrossing) {
    if (c.size % 2 != 1) throw std::invalid_argument("MiniGrid crossing: size must be odd");
    const int rivers = 2 * ((c.size - 3) / 2);
    if (c.num_crossings < 1 || c.num_crossings > rivers) {
      throw std::invalid_argument("MiniGrid crossing: num_crossings must be in [1, " + std::to_string(rivers) + "]");
    }
  }
  c.obstacle = cfg.Get("obstacle_wall", 0) != 0 ? mg::kWallCell : mg::kLavaCell;
  c.strip2_row = (int)cfg.Get("strip2_row", 2);
  if (c.task == mg::kTaskDistShift && (c.strip2_row < 1 || c.strip2_row > c.height - 2)) {
    throw std::invalid_argument("MiniGrid distshift: strip2_row must be inside the walls");
  }
  c.n_obstacles = 0;
  if (mg::HasObstacles(c.task)) {  // DynamicObstaclesTask's constructor (minigrid_tasks.cc:200)
    const int n = (int)cfg.Get("n_obstacles", 4);
    c.n_obstacles = n <= c.size / 2 + 1 ? n : c.size / 2;
    if (c.n_obstacles < 0 || c.n_obstacles > mg::kMaxObstacles || c.size > 16) {
      throw std::invalid_argument("MiniGrid dynamic_obstacles: n_obstacles must be in [0, 8] after the clamp to size / 2, size at most 16");
    }
  }
  c.max_steps = cfg.max_episode_steps;
  const double tries = cfg.Get("minigrid_max_tries", 1 << 20);
  if (tries < 0 || tries > 2147483647.0) throw std::invalid_argument("minigrid_max_tries must be in [0, 2^31)");
  c.max_tries = (int)tries;
  c.see_through = mg::SeeThroughWalls(c.task);
  return c;
}

// SetMission of each task (minigrid_tasks.cc, minigrid_room_tasks.cc)
std::string MissionText(const TaskCfg& c) {
  switch (c.task) {
    case mg::kTaskDoorKey: return "use the key to open the door and then get to the goal";
    case mg::kTaskCrossing:
    case mg::kTaskLavaGap:
      return c.obstacle == mg::kLavaCell ? "avoid the lava and get to the green goal square"
                                         : "find the opening and get to the green goal square";
    case mg::kTaskFourRooms: return "reach the goal";
    default: return "get to the green goal square";
  }
}

class MiniGridPool : public Pool {
 public:
  bool ConcurrentSafe() const override { return true; }  // per-env state + the launch's own block only
  explicit MiniGridPool(const Config& cfg)
      : Pool(cfg, Spec(), /*needs_rng=*/true), c_(MakeTaskCfg(cfg)) {
    const size_t n = (size_t)cfg.num_envs;
    d_.n = cfg.num_envs;
    d_.cells = c_.width * c_.height;
    d_.grid = DevAlloc<uint16_t>(n * d_.cells);
    d_.agent = DevAlloc<int>(n);
    d_.carry = DevAlloc<uint16_t>(n);
    d_.obst = DevAlloc<uint64_t>(n);
    // WriteMission (minigrid_render.cc:371-376): the text, zero-padded, at most mission_bytes - 1 bytes
    char text[mg::kMissionBytes] = {};
    const std::string m = MissionText(c_);
    std::memcpy(text, m.data(), std::min<size_t>(m.size(), mg::kMissionBytes - 1));
    d_.mission = reinterpret_cast<const uint4*>(DevUpload(text, mg::kMissionBytes));
    EnableErrorWord();
    d_.err = err_dev_;
    mt_tile_default_ = 16;  // envs reset at their own times
    InitCommon();
  }
  int StateDim() const override { return kHead + 3 * d_.cells; }
  void GetState(const int* d_ids, int k, double* d_out) override {
    hipLaunchKernelGGL(MiniGridGetState, dim3((k + 255) / 256), dim3(256), 0, stream_, d_, common_, c_, d_ids, k,
                       d_out);
  }
  void SetState(const int* d_ids, int k, const double* d_in) override {
    hipLaunchKernelGGL(MiniGridSetState, dim3((k + 255) / 256), dim3(256), 0, stream_, d_, common_, c_, d_ids, k,
                       d_in);
  }
  std::string ErrorText(unsigned code) const override {
    if (code == kErrTries) {
      return "MiniGrid: a reset's rejection sampling ran out of tries (minigrid_max_tries = " +
             std::to_string(c_.max_tries) + "); the reference would throw or spin here";
    }
    if (code == kErrState) return "MiniGrid: an env state put the agent or an obstacle off the grid (set_state)";
    return Pool::ErrorText(code);
  }

 protected:
  void Launch(const int* d_ids, int k, const void* d_action, bool force_reset, const OutPtrs& out) override {
    StepArgs a{d_ids, k, force_reset ? 1 : 0, cfg_.max_episode_steps, cfg_.env_id_offset};
    const int blocks = (k + kBlock - 1) / kBlock;
    auto kernel = MiniGridStepKernel<mg::kTaskEmpty>;
    switch (c_.task) {
      case mg::kTaskDoorKey: kernel = MiniGridStepKernel<mg::kTaskDoorKey>; break;
      case mg::kTaskDistShift: kernel = MiniGridStepKernel<mg::kTaskDistShift>; break;
      case mg::kTaskCrossing: kernel = MiniGridStepKernel<mg::kTaskCrossing>; break;
      case mg::kTaskLavaGap: kernel = MiniGridStepKernel<mg::kTaskLavaGap>; break;
      case mg::kTaskDynObs: kernel = MiniGridStepKernel<mg::kTaskDynObs>; break;
      case mg::kTaskFourRooms: kernel = MiniGridStepKernel<mg::kTaskFourRooms>; break;
      default: break;
    }
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream_, d_, common_, a,
                       static_cast<const int*>(d_action), out, c_);
  }

 private:
  TaskCfg c_;
  MgDev d_{};
};

}  // namespace

FamilySpec DescribeMiniGrid(const std::string&, const Config&) { return Spec(); }

Pool* MakeMiniGrid(const std::string&, const Config& cfg) { return new MiniGridPool(cfg); }

}  // namespace epa
