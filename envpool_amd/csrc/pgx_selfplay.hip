// PGX self-play driver: the three launches a ply needs beside the search, the network, the step and the recorder
// (pgx_selfplay.hip.h is the contract; Pool::SelfplayRun in engine.hip enqueues them).  Row i is local env i of the pool.
//   PgxSelfplayNoise  one thread per (row, action) element of the [k, A] noise rows: consecutive threads store
//                     consecutive floats.  The element's key is recomputed per thread (two splitmix rounds): cheaper
//                     than passing it through memory.
//   PgxSelfplayMove   Gumbel: one thread per (row, action) element copies the result's weights into the target rows;
//                     the thread of action 0 writes the row's action.  PUCT: a row belongs to a GROUP of LG lanes, LG
//                     the power of two at or above A, at most 64 (TicTacToe 16, ConnectFour 8, Othello and Hex 64);
//                     lane j owns the E = ceil(A / LG) consecutive actions j E .. j E + E - 1 (1, 1, 2, 2), so the
//                     lanes' totals scanned by __shfl_up are the prefix sums in action order.  V is the last lane's
//                     scan, the sampled move the lowest action whose prefix exceeds r and the greedy move the
//                     (visits, lowest action) maximum, both by a __shfl_xor butterfly inside the group.  Every lane
//                     stays active through the shuffles; loads and stores are predicated.  Integers only.
//   PgxSelfplayTally  one thread per row, a wave butterfly over the five integers, then lane 0's atomics on the
//                     int64 counters (a wave that saw no finished game adds nothing).  <true>, an arena's: the seven
//                     counters of pgx_arena.hip.h, wins_a and wins_b by the parity of the row's global env id.
// PUCT exploration (pgx_dirichlet.hip.h is the contract):
//   PgxSelfplayDirichlet  a row belongs to the GROUP of PgxSelfplayMove<PUCT> (LG lanes, E consecutive actions per
//                     lane).  A lane runs the rejection loop of each of its legal actions -- divergent, but almost
//                     every action accepts its first attempt --, adds its run in ascending order, and the group's
//                     __shfl_xor butterfly gives every lane S.  It stores eta to the noise rows and mixes it into the
//                     policy row of the root's leaf row (slot 0 of a width session) where the root's status is 0.
//                     Every lane stays active through the shuffles; loads and stores are predicated.
//   PgxSelfplayMoveTemp   PgxSelfplayMove<PUCT> for a temperature T != 1: vmax by a butterfly, the lanes' q, and the
//                     sampled move from the scan of q.  The target rows and the greedy move are PgxSelfplayMove's.
#include <algorithm>
#include <climits>

#include "engine.h"
#include "pgx_arena.hip.h"
#include "pgx_dirichlet.hip.h"
#include "pgx_env.hip.h"
#include "pgx_selfplay.hip.h"

namespace epa {
namespace {

static_assert(pgx::kSelfplayGumbel == EPA_SELFPLAY_GUMBEL && pgx::kSelfplayPuct == EPA_SELFPLAY_PUCT,
              "the C ABI states the header's policies");
constexpr int kSelfplayBlock = 256;

template <int G>
__global__ __launch_bounds__(kSelfplayBlock) void PgxSelfplayNoise(SelfplayArgs a) {
  constexpr int A = pgx::Dims<G>::A;
  const long long i = (long long)blockIdx.x * kSelfplayBlock + threadIdx.x;
  if (i >= (long long)a.k * A) return;
  const int row = (int)(i / A), act = (int)(i - (long long)row * A);
  float g = 0.0f;
  if (a.noise != 0) g = pgx::SelfplayNoise(pgx::SelfplayKey(a.seed, row + a.id_offset, a.t), act);
  a.gumbel[i] = g;
}

// lanes of a PUCT row's group
template <int G>
constexpr int SelfplayGroup() {
  constexpr int A = pgx::Dims<G>::A;
  int lg = 1;
  while (lg < A && lg < 64) lg <<= 1;
  return lg;
}

template <int G, int POLICY>
__global__ __launch_bounds__(kSelfplayBlock) void PgxSelfplayMove(SelfplayArgs a) {
  constexpr int A = pgx::Dims<G>::A;
  if constexpr (POLICY == pgx::kSelfplayGumbel) {
    const long long i = (long long)blockIdx.x * kSelfplayBlock + threadIdx.x;
    if (i >= (long long)a.k * A) return;
    // (moved as bits: nothing is computed with the weights)
    reinterpret_cast<uint32_t*>(a.target)[i] = reinterpret_cast<const uint32_t*>(a.weights)[i];
    const int row = (int)(i / A);
    if (i == (long long)row * A) a.action[row] = pgx::SelfplayGumbelAction(a.result_action[row]);
  } else {
    constexpr int LG = SelfplayGroup<G>(), E = (A + LG - 1) / LG;
    const int g = (int)(((long long)blockIdx.x * kSelfplayBlock + threadIdx.x) / LG), j = threadIdx.x & (LG - 1);
    const bool live = g < a.k;
    const int row = live ? g : 0;
    int v[E];
    int mine = 0;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int act = j * E + i;
      v[i] = (live && act < A) ? a.visits[(size_t)row * A + act] : 0;
      mine += v[i];
    }
    int x = mine;  // the group's inclusive scan of the lanes' totals
#pragma unroll
    for (int d = 1; d < LG; d <<= 1) {
      const int y = __shfl_up(x, d, LG);
      if (j >= d) x += y;
    }
    const int V = __shfl(x, LG - 1, LG);
    const bool zero = V == 0 || (live && a.result_action[row] < 0);
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int act = j * E + i;
      if (live && act < A) a.target[(size_t)row * A + act] = zero ? 0.0f : pgx::SelfplayTarget(v[i], V);
    }
    // both rules without a branch around the shuffles: the sampled move (the lowest action whose prefix exceeds r) ...
    const bool sample = live && !zero && a.cur_step[row] < a.sample_plies;
    const uint32_t r = pgx::SelfplaySampleAt(pgx::SelfplayKey(a.seed, row + a.id_offset, a.t), (uint32_t)V);
    uint32_t run = (uint32_t)(x - mine);
    int sampled = INT_MAX;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      run += (uint32_t)v[i];
      if (sampled == INT_MAX && run > r) sampled = j * E + i;
    }
    // ... and the greedy one (the most visited action, the lowest on ties)
    int best = v[0], greedy = j * E;
#pragma unroll
    for (int i = 1; i < E; ++i) {
      if (v[i] > best) {
        best = v[i];
        greedy = j * E + i;
      }
    }
#pragma unroll
    for (int w = LG / 2; w >= 1; w >>= 1) {
      sampled = std::min(sampled, __shfl_xor(sampled, w, LG));
      const int ob = __shfl_xor(best, w, LG), op = __shfl_xor(greedy, w, LG);
      if (ob > best || (ob == best && op < greedy)) {
        best = ob;
        greedy = op;
      }
    }
    if (live && j == 0) a.action[row] = zero ? 0 : (sample ? sampled : greedy);
  }
}

// Dirichlet root noise of a PUCT driver: eta to the noise rows, mixed into the roots' policy rows in place
template <int G>
__global__ __launch_bounds__(kSelfplayBlock) void PgxSelfplayDirichlet(SelfplayArgs a) {
  constexpr int A = pgx::Dims<G>::A;
  constexpr int LG = SelfplayGroup<G>(), E = (A + LG - 1) / LG;
  static_assert(LG == pgx::DirichletGroup(A) && E == pgx::DirichletRun(A), "the contract's summation order");
  const int g = (int)(((long long)blockIdx.x * kSelfplayBlock + threadIdx.x) / LG), j = threadIdx.x & (LG - 1);
  const bool live = g < a.k;
  const int row = live ? g : 0;
  const size_t leaf = (size_t)row * a.slots;  // the root's own leaf row: slot 0
  const uint64_t key = pgx::SelfplayKey(a.seed, row + a.id_offset, a.t);
  const pgx::DirichletParams prm{a.alpha, a.gamma_d, a.gamma_c};
  float gm[E];
  bool legal[E];
  float S = 0.0f;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const int act = j * E + i;
    legal[i] = live && act < A && a.mask[leaf * A + act] != 0;
    gm[i] = legal[i] ? pgx::DirichletGamma(key, act, prm, nullptr) : 0.0f;
    S = S + gm[i];
  }
#pragma unroll
  for (int w = LG / 2; w >= 1; w >>= 1) S = S + __shfl_xor(S, w, LG);
  const bool mix = live && a.status[leaf] == 0;
  const float om = 1.0f - a.eps;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const int act = j * E + i;
    if (live && act < A) {
      const float eta = legal[i] ? pgx::DirichletEta(gm[i], S) : 0.0f;
      a.gumbel[(size_t)row * A + act] = eta;
      if (mix && legal[i]) a.prior[leaf * A + act] = pgx::DirichletMix(a.prior[leaf * A + act], eta, om, a.eps);
    }
  }
}

// PgxSelfplayMove<G, PUCT> with a temperature T != 1 (pgx_dirichlet.hip.h: SelfplayPuctMoveTemp)
template <int G>
__global__ __launch_bounds__(kSelfplayBlock) void PgxSelfplayMoveTemp(SelfplayArgs a) {
  constexpr int A = pgx::Dims<G>::A;
  constexpr int LG = SelfplayGroup<G>(), E = (A + LG - 1) / LG;
  const int g = (int)(((long long)blockIdx.x * kSelfplayBlock + threadIdx.x) / LG), j = threadIdx.x & (LG - 1);
  const bool live = g < a.k;
  const int row = live ? g : 0;
  int v[E];
  int V = 0, vmax = 0;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const int act = j * E + i;
    v[i] = (live && act < A) ? a.visits[(size_t)row * A + act] : 0;
    V += v[i];
    vmax = std::max(vmax, v[i]);
  }
#pragma unroll
  for (int w = LG / 2; w >= 1; w >>= 1) {
    V += __shfl_xor(V, w, LG);
    vmax = std::max(vmax, __shfl_xor(vmax, w, LG));
  }
  const bool zero = V == 0 || (live && a.result_action[row] < 0);
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const int act = j * E + i;
    if (live && act < A) a.target[(size_t)row * A + act] = zero ? 0.0f : pgx::SelfplayTarget(v[i], V);
  }
  // the sampled move: the lowest action whose prefix sum of q exceeds r ...
  uint32_t q[E];
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    q[i] = pgx::TemperatureWeight(v[i], vmax, a.temperature);
    mine += q[i];
  }
  uint32_t x = mine;  // the group's inclusive scan of the lanes' totals
#pragma unroll
  for (int d = 1; d < LG; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, LG);
    if (j >= d) x += y;
  }
  const uint32_t Q = __shfl(x, LG - 1, LG);
  const bool sample = live && !zero && a.cur_step[row] < a.sample_plies;
  const uint32_t r = pgx::SelfplaySampleAt(pgx::SelfplayKey(a.seed, row + a.id_offset, a.t), Q);
  uint32_t run = x - mine;
  int sampled = INT_MAX;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    run += q[i];
    if (sampled == INT_MAX && run > r) sampled = j * E + i;
  }
  // ... and the greedy one (the most visited action, the lowest on ties)
  int best = v[0], greedy = j * E;
#pragma unroll
  for (int i = 1; i < E; ++i) {
    if (v[i] > best) {
      best = v[i];
      greedy = j * E + i;
    }
  }
#pragma unroll
  for (int w = LG / 2; w >= 1; w >>= 1) {
    sampled = std::min(sampled, __shfl_xor(sampled, w, LG));
    const int ob = __shfl_xor(best, w, LG), op = __shfl_xor(greedy, w, LG);
    if (ob > best || (ob == best && op < greedy)) {
      best = ob;
      greedy = op;
    }
  }
  if (live && j == 0) a.action[row] = zero ? 0 : (sample ? sampled : greedy);
}

// ARENA: the seven counters of pgx_arena.hip.h (PgxArenaTally in the documents)
template <bool ARENA>
__global__ __launch_bounds__(kSelfplayBlock) void PgxSelfplayTally(SelfplayArgs a) {
  constexpr int N = ARENA ? pgx::kArenaCounters : pgx::kSelfplayCounters;
  const int i = blockIdx.x * kSelfplayBlock + threadIdx.x;
  int c[N] = {};
  if (i < a.k) {
    const bool done = a.done[i] != 0;
    const float r0 = a.reward[2 * (size_t)i], r1 = a.reward[2 * (size_t)i + 1];
    if constexpr (ARENA) {
      pgx::ArenaTallyRow(done, r0, r1, a.elapsed[i], i + a.id_offset, c);
    } else {
      pgx::SelfplayTallyRow(done, r0, r1, a.elapsed[i], c);
    }
  }
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
#pragma unroll
    for (int q = 0; q < N; ++q) c[q] += __shfl_xor(c[q], w, 64);
  }
  if ((threadIdx.x & 63) == 0 && c[0] != 0) {
    unsigned long long* ctr = reinterpret_cast<unsigned long long*>(a.counters);
#pragma unroll
    for (int q = 0; q < N; ++q) {
      if (c[q] != 0) atomicAdd(&ctr[q], (unsigned long long)c[q]);
    }
  }
}

unsigned Blocks(long long threads) { return (unsigned)((threads + kSelfplayBlock - 1) / kSelfplayBlock); }

template <int G>
void LaunchNoise(const SelfplayArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(PgxSelfplayNoise<G>, dim3(Blocks((long long)a.k * pgx::Dims<G>::A)), dim3(kSelfplayBlock), 0, s, a);
}

template <int G>
void LaunchMove(const SelfplayArgs& a, hipStream_t s) {
  if (a.policy == pgx::kSelfplayGumbel) {
    hipLaunchKernelGGL((PgxSelfplayMove<G, pgx::kSelfplayGumbel>), dim3(Blocks((long long)a.k * pgx::Dims<G>::A)),
                       dim3(kSelfplayBlock), 0, s, a);
  } else if (a.temperature != 1.0f) {
    hipLaunchKernelGGL(PgxSelfplayMoveTemp<G>, dim3(Blocks((long long)a.k * SelfplayGroup<G>())), dim3(kSelfplayBlock),
                       0, s, a);
  } else {
    hipLaunchKernelGGL((PgxSelfplayMove<G, pgx::kSelfplayPuct>), dim3(Blocks((long long)a.k * SelfplayGroup<G>())),
                       dim3(kSelfplayBlock), 0, s, a);
  }
}

template <int G>
void LaunchDirichlet(const SelfplayArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(PgxSelfplayDirichlet<G>, dim3(Blocks((long long)a.k * SelfplayGroup<G>())), dim3(kSelfplayBlock), 0,
                     s, a);
}

}  // namespace

void PgxSelfplayLaunchNoise(int game, const SelfplayArgs& a, hipStream_t stream) {
  switch (game) {
    case pgx::kTicTacToe: return LaunchNoise<pgx::kTicTacToe>(a, stream);
    case pgx::kConnectFour: return LaunchNoise<pgx::kConnectFour>(a, stream);
    case pgx::kHex: return LaunchNoise<pgx::kHex>(a, stream);
    default: return LaunchNoise<pgx::kOthello>(a, stream);
  }
}

void PgxSelfplayLaunchMove(int game, const SelfplayArgs& a, hipStream_t stream) {
  switch (game) {
    case pgx::kTicTacToe: return LaunchMove<pgx::kTicTacToe>(a, stream);
    case pgx::kConnectFour: return LaunchMove<pgx::kConnectFour>(a, stream);
    case pgx::kHex: return LaunchMove<pgx::kHex>(a, stream);
    default: return LaunchMove<pgx::kOthello>(a, stream);
  }
}

void PgxSelfplayLaunchDirichlet(int game, const SelfplayArgs& a, hipStream_t stream) {
  switch (game) {
    case pgx::kTicTacToe: return LaunchDirichlet<pgx::kTicTacToe>(a, stream);
    case pgx::kConnectFour: return LaunchDirichlet<pgx::kConnectFour>(a, stream);
    case pgx::kHex: return LaunchDirichlet<pgx::kHex>(a, stream);
    default: return LaunchDirichlet<pgx::kOthello>(a, stream);
  }
}

void PgxSelfplayLaunchTally(const SelfplayArgs& a, hipStream_t stream) {
  if (a.arena != 0) {
    hipLaunchKernelGGL(PgxSelfplayTally<true>, dim3(Blocks(a.k)), dim3(kSelfplayBlock), 0, stream, a);
  } else {
    hipLaunchKernelGGL(PgxSelfplayTally<false>, dim3(Blocks(a.k)), dim3(kSelfplayBlock), 0, stream, a);
  }
}

}  // namespace epa
