// PGX two-player board games (TicTacToe, ConnectFour, Hex, Othello): batched reset / step kernel, one env per
// lane, bit-exact with the reference.
//
// Replaces, for the whole batch in one launch, XxxEnv::{Reset,Step,WriteState} of envpool/pgx/board_games.h
// plus the runtime (async_envpool.h:118-132, env.h:184-256) of a pool with max_num_players = 2.  The env bodies
// are pgx_env.hip.h (shared with the host harness of the tests); one kernel instantiation per game.
//
// Data layout (HBM), see DESIGN.md "PGX":
//   state  pgx::State [N]   64 B per env, env-major: three 128-bit cell sets (stones, legal mask) + four words,
//                           read once and written once by the env's lane
//   mt     CommonDev, tiled (envs reset at their own times; one draw per reset)
// Outputs: every env writes 2 player rows, kept together as the [2, ...] block of its batch row (the reference's
// env-major player rows).  They are most of the traffic (Hex: 1.6 KB per env-step, obs 968 B of it), so a lane does
// not store its own row: it leaves its `View` (state + common keys, 96 B) in LDS, and then the block writes each
// key's section -- one contiguous range for the block's rows -- in 16-byte words, every thread computing the
// elements of its words from the views (pgx::Elem).  A wave's stores are then 1 KB contiguous instead of 64 rows
// apart.
// Render: pgx_render.hip.h painted by render_kernel.hip.h, one workgroup per band of a frame.
// Playout: pgx_playout.hip.h, one (env, repeat) per lane, the whole game in registers (PgxPlayoutKernel).
#include <algorithm>
#include <string>

#include "device_common.hip.h"
#include "engine.h"
#include "pgx_env.hip.h"
#include "pgx_playout.hip.h"
#include "pgx_render.hip.h"
#include "render_kernel.hip.h"

namespace epa {
namespace {

constexpr int kBlock = 256;
constexpr unsigned kErrState = 1;  // set_state words that are no position of the game

// key K's section of rows [row0, row0 + nrows) of the launch, written by the whole block
template <int G, int K>
__device__ __forceinline__ void EmitKey(const OutPtrs& out, int row0, int nrows, const pgx::View* lv) {
  constexpr int re = pgx::RowElems<G>(K), eb = pgx::ElemBytes(K), per = 16 / eb;
  char* base = static_cast<char*>(out.p[K]) + (size_t)row0 * (re * eb);
  const int total = nrows * re;
  // head elements up to the first 16-byte boundary (a pipelined launch's second half may start anywhere)
  const int mis = (int)((uintptr_t)base & 15);
  const int head = std::min(total, mis == 0 ? 0 : (16 - mis) / eb);
  const int words = (total - head) / per;
  const int tail = head + words * per;
  auto one = [&](int i) {
    const int r = i / re;
    const uint32_t x = pgx::Elem<G>(lv[r], K, i - r * re);
    if (eb == 1) {
      base[i] = (char)x;
    } else {
      reinterpret_cast<uint32_t*>(base)[i] = x;
    }
  };
  for (int i = threadIdx.x; i < head; i += kBlock) one(i);
  for (int c = threadIdx.x; c < words; c += kBlock) {
    const int i0 = head + c * per;
    int r = i0 / re, e = i0 - r * re;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < per; ++j) {
      const uint32_t x = pgx::Elem<G>(lv[r], K, e);
      if (eb == 1) {
        w[j >> 2] |= (x & 0xffu) << (8 * (j & 3));
      } else {
        w[j] = x;
      }
      if (++e == re) {
        e = 0;
        ++r;
      }
    }
    *reinterpret_cast<uint4*>(base + (size_t)i0 * eb) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  for (int i = tail + threadIdx.x; i < total; i += kBlock) one(i);
}

template <int G, int... K>
__device__ __forceinline__ void EmitAll(const OutPtrs& out, int row0, int nrows, const pgx::View* lv,
                                        std::integer_sequence<int, K...>) {
  (EmitKey<G, K>(out, row0, nrows, lv), ...);
}

template <int G>
__global__ __launch_bounds__(kBlock) void PgxStepKernel(CommonDev cm, StepArgs a, pgx::State* st,
                                                        const int* __restrict__ action, OutPtrs out) {
  __shared__ pgx::View lv[kBlock];
  const int row0 = blockIdx.x * kBlock;
  const int row = row0 + threadIdx.x;
  if (row < a.k) {
    const int e = a.ids ? a.ids[row] - a.id_offset : row;
    pgx::State s = st[e];
    int cur = cm.cur_step[e];
    pgx::Rewards rw{{0.0f, 0.0f}};
    if (a.force_reset || cm.done[e] != 0) {  // async_envpool.h:127
      cur = 0;
      Mt19937 g(cm, e);
      pgx::Reset<G>(g, s);
      g.Commit();
    } else {
      ++cur;
      rw = pgx::Step<G>(s, action[row]);
    }
    st[e] = s;
    cm.done[e] = s.done ? 1 : 0;
    cm.cur_step[e] = cur;
    pgx::View v{};
    v.s = s;
    pgx::Finish(v, e + a.id_offset, cur, rw, a.max_episode_steps);
    lv[threadIdx.x] = v;
  }
  __syncthreads();
  if (row0 >= a.k) return;
  EmitAll<G>(out, row0, std::min(kBlock, a.k - row0), lv, std::make_integer_sequence<int, pgx::kNumKeys>());
}

// flat state per env: cur_step, done, then pgx::Hidden's words
template <int G>
__global__ void PgxGetState(CommonDev cm, const pgx::State* st, const int* ids, int k, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int e = ids[i];
  constexpr int W = pgx::HiddenWords<G>();
  double* o = out + (size_t)i * (2 + W);
  o[0] = cm.cur_step[e];
  o[1] = cm.done[e];
  int32_t w[W];
  pgx::Hidden<G>(st[e], w);
  for (int j = 0; j < W; ++j) o[2 + j] = w[j];
}

template <int G>
__global__ void PgxSetState(CommonDev cm, pgx::State* st, unsigned* err, const int* ids, int k, const double* in) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int e = ids[i];
  constexpr int W = pgx::HiddenWords<G>();
  const double* o = in + (size_t)i * (2 + W);
  int32_t w[W];
  for (int j = 0; j < W; ++j) w[j] = (int32_t)o[2 + j];
  pgx::State s{};
  bool done = o[1] != 0.0;
  if (!pgx::SetHidden<G>(s, w)) {
    *err = kErrState;
    done = true;  // such an env resets on its next step
  }
  s.done = done ? 1 : 0;
  st[e] = s;
  cm.cur_step[e] = (int)o[0];
  cm.done[e] = done ? 1 : 0;
}

// Random playouts (pgx_playout.hip.h): lane i plays repeat i % R of listed env i / R, so the repeats of one env sit
// in adjacent lanes -- they load the same 64-byte State (one sector for the group) and their games, from one position,
// are the likeliest to be of similar length -- and result i of each of the three arrays is lane i's, stored coalesced.
// No barrier, no memory traffic per ply and no LDS of its own (the compiler keeps Step's seat-indexed reward pairs in
// 16 bytes of LDS per lane): a block is one wave, which leaves its SIMD as soon as its own longest game is over.
// The loop is divergent per lane (a wave runs for its longest game, and Hex's flood fill for the lane with the
// largest group); lanes whose game is over idle until then.
// Commit (R == 1, ids that do not repeat: the engine checks both) also writes back what the plies' step launches
// would have: the State, done and cur_step.  An env that is over at the call -- cm.done, which an env before its first
// reset has set while its State is still all zeros -- plays nothing and is left as it is.
constexpr int kPlayoutBlock = 64;
static_assert(pgx::kPlayoutMaxPlies == EPA_PLAYOUT_MAX_PLIES && pgx::kPlayoutMaxRepeats == EPA_PLAYOUT_MAX_REPEATS,
              "the C ABI states the header's limits");

template <int G>
__global__ __launch_bounds__(kPlayoutBlock) void PgxPlayoutKernel(CommonDev cm, pgx::State* st,
                                                                  const int* __restrict__ ids, PlayoutArgs a,
                                                                  int id_offset) {
  const long long i = (long long)blockIdx.x * kPlayoutBlock + threadIdx.x;
  if (i >= (long long)a.k * a.repeats) return;
  const int row = (int)(i / a.repeats), r = (int)(i - (long long)row * a.repeats);
  const int e = ids[row];
  pgx::State s = st[e];
  const uint64_t h = pgx::PlayoutStream(a.seed, e + id_offset, r);
  const pgx::PlayoutResult res = pgx::Playout<G>(s, cm.done[e] != 0, h, pgx::PlayoutLimit(a.max_plies));
  reinterpret_cast<float2*>(a.returns)[i] = make_float2(res.ret[0], res.ret[1]);
  a.plies[i] = res.plies;
  a.status[i] = (unsigned char)res.status;
  if ((a.flags & EPA_PLAYOUT_COMMIT) != 0 && res.plies > 0) {
    st[e] = s;
    cm.done[e] = s.done ? 1 : 0;
    cm.cur_step[e] += res.plies;
  }
}

// the render kernel's painter of game G (render_kernel.hip.h)
template <int G>
struct PgxPainter {
  using State = pgx::State;
  static __device__ void Paint(render::Canvas& cv, const State& s) { pgx::Render<G>(cv, s); }
};

int GameOf(const std::string& family) {
  if (family == "TicTacToe") return pgx::kTicTacToe;
  if (family == "ConnectFour") return pgx::kConnectFour;
  if (family == "Hex") return pgx::kHex;
  return pgx::kOthello;
}

// the reference's StateSpec key order (after the common keys); "obs" and "info:players.id" are per player
template <int G>
FamilySpec Spec() {
  using D = pgx::Dims<G>;
  return {{{"obs", EPA_BOOL, {pgx::kPlayers, D::H, D::W, D::C}, pgx::kPlayers},
           {"info:board", EPA_I32, {D::H, D::W}},
           {"info:current_player", EPA_I32, {}},
           {"info:legal_action_mask", EPA_BOOL, {D::A}},
           {"info:players.id", EPA_I32, {pgx::kPlayers}, pgx::kPlayers}},
          {"action", EPA_I32, {}},
          pgx::kPlayers};
}

template <int G>
class PgxPool : public Pool {
 public:
  bool ConcurrentSafe() const override { return true; }  // per-env state + the launch's own rows only
  explicit PgxPool(const Config& cfg)
      : Pool(cfg, Spec<G>(), /*needs_rng=*/true) {
    const size_t n = (size_t)cfg.num_envs;
    state_ = DevAlloc<pgx::State>(n);
    EnableErrorWord();
    mt_tile_default_ = 16;  // envs reset at their own times
    InitCommon();
  }
  int StateDim() const override { return 2 + pgx::HiddenWords<G>(); }
  void GetState(const int* d_ids, int k, double* d_out) override {
    hipLaunchKernelGGL(PgxGetState<G>, dim3((k + 255) / 256), dim3(256), 0, stream_, common_, state_, d_ids, k,
                       d_out);
  }
  void SetState(const int* d_ids, int k, const double* d_in) override {
    hipLaunchKernelGGL(PgxSetState<G>, dim3((k + 255) / 256), dim3(256), 0, stream_, common_, state_, err_dev_,
                       d_ids, k, d_in);
  }
  void RenderSize(int width, int height, int* w, int* h) const override { pgx::RenderSize<G>(width, height, w, h); }
  void Render(const int* d_ids, int k, int w, int h, int /*camera_id*/, void* d_rgb) override {
    render::LaunchRender<PgxPainter<G>>(state_, d_ids, k, w, h, d_rgb, stream_);
  }
  bool HasPlayout() const override { return true; }
  void Playout(const int* d_ids, const PlayoutArgs& a) override {
    const long long lanes = (long long)a.k * a.repeats;
    hipLaunchKernelGGL(PgxPlayoutKernel<G>, dim3((unsigned)((lanes + kPlayoutBlock - 1) / kPlayoutBlock)),
                       dim3(kPlayoutBlock), 0, stream_, common_, state_, d_ids, a, cfg_.env_id_offset);
  }
  std::string ErrorText(unsigned code) const override {
    if (code == kErrState) return "PGX: set_state was given words that are no position of the game";
    return Pool::ErrorText(code);
  }

 protected:
  void Launch(const int* d_ids, int k, const void* d_action, bool force_reset, const OutPtrs& out) override {
    StepArgs a{d_ids, k, force_reset ? 1 : 0, cfg_.max_episode_steps, cfg_.env_id_offset};
    hipLaunchKernelGGL(PgxStepKernel<G>, dim3((k + kBlock - 1) / kBlock), dim3(kBlock), 0, stream_, common_, a,
                       state_, static_cast<const int*>(d_action), out);
  }

 private:
  pgx::State* state_{nullptr};
};

}  // namespace

FamilySpec DescribePgx(const std::string& name, const Config&) {
  switch (GameOf(name)) {
    case pgx::kTicTacToe: return Spec<pgx::kTicTacToe>();
    case pgx::kConnectFour: return Spec<pgx::kConnectFour>();
    case pgx::kHex: return Spec<pgx::kHex>();
    default: return Spec<pgx::kOthello>();
  }
}

Pool* MakePgx(const std::string& name, const Config& cfg) {
  switch (GameOf(name)) {
    case pgx::kTicTacToe: return new PgxPool<pgx::kTicTacToe>(cfg);
    case pgx::kConnectFour: return new PgxPool<pgx::kConnectFour>(cfg);
    case pgx::kHex: return new PgxPool<pgx::kHex>(cfg);
    default: return new PgxPool<pgx::kOthello>(cfg);
  }
}

}  // namespace epa
