// PGX self-play driver: the glue between two search rounds of a pool that plays against itself -- root noise, the
// choice of the move, the policy target and the game statistics -- as __host__ __device__ pieces shared by the kernels
// (PgxSelfplayNoise / PgxSelfplayMove / PgxSelfplayTally in pgx_selfplay.hip) and the g++ host harness of the tests
// (tests/cpu_harness/pgx_selfplay_host.cpp, which walks the lanes as loops).  This header is the authority; DESIGN.md
// "PGX self-play driver" restates it.
//
// The contract.  All integer arithmetic is mod 2^64, SM = PlayoutMix (pgx_playout.hip.h).  The build keeps
// -ffp-contract=off and no fast-math, as pgx_gumbel.hip.h requires.
//   counter   a driver has a ply counter t: 0 at open, + 1 per ply played, across run calls
//   key       key(e, t) = SM(seed ^ SM((uint64(global env id e) << 32) | uint32(t)))               (SelfplayKey)
//   uniform   n = uint32(SM(key + a) >> 41) for action a: 23 bits;  u = ((float)n + 0.5f) * 2^-23.  Both operations
//             are exact and 0 < u < 1 strictly (24 bits would round the top value to 1.0)           (SelfplayUniform)
//   GumbelLog(x), finite x > 0, only correctly rounded float32 + - * / and frexpf:
//             m, e = frexpf(x);  m < 0.70710678f: m *= 2, e -= 1
//             f = m - 1;  s = f / (2 + f);  z = s * s
//             p = 1/9;  p = p z + 1/7;  p = p z + 1/5;  p = p z + 1/3;  p = p z
//             r = (2 s) p + 2 s
//             (float)e * 0.693359375f + (r + (float)e * -2.12194440e-4f)            (the two-word ln 2 of GumbelExp)
//   noise     g = -GumbelLog(-GumbelLog(u)): finite for all 2^23 values of n, within 2e-6 of the float64
//             -log(-log(u)) (tests/test_pgx_selfplay_host.py runs them all).  noise off: the row is all zeros
//   move, Gumbel session:  action' = result.action < 0 ? 0 : result.action;  the target row is result.weights unchanged
//             (a root that was over at begin has a zero row, and the recorder's add skips it)
//   move, PUCT session:  V = the sum of visits[a].  V == 0, or the root was over (result.action < 0): action 0, a zero
//             row.  Otherwise target[a] = (float)visits[a] / (float)V, one division each, and
//               the env's elapsed step < sample_plies:  r = ((SM(key + 0x100) >> 32) * V) >> 32;  the action is the
//                   lowest a whose inclusive prefix sum of visits exceeds r                          (SelfplaySampleAt)
//               otherwise: the argmax of visits, ties to the lowest a
//             Integers only: the result does not depend on the launch geometry.
//   tally, after the step, from the result block's done [k], reward [k][2] and elapsed_step [k]: five int64 counters
//             gain, over the rows with done != 0: games 1, wins0 (reward[i][0] > 0), wins1 (reward[i][1] > 0), draws
//             (both rewards 0), plies (the row's elapsed step).  Integer atomics: a sum has no order.
#ifndef ENVPOOL_AMD_CSRC_PGX_SELFPLAY_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_SELFPLAY_HIP_H_

#include <cmath>

#include "pgx_playout.hip.h"

namespace epa {
namespace pgx {

constexpr int kSelfplayGumbel = 0;  // the driver's policies (EPA_SELFPLAY_GUMBEL / _PUCT)
constexpr int kSelfplayPuct = 1;
constexpr int kSelfplayCounters = 5;  // games, wins0, wins1, draws, plies
constexpr uint64_t kSelfplaySampleSalt = 0x100;  // above every action index

PGX_HD inline uint64_t SelfplayKey(uint64_t seed, int env_id, uint32_t t) {
  return PlayoutMix(seed ^ PlayoutMix(((uint64_t)(uint32_t)env_id << 32) | (uint64_t)t));
}

PGX_HD inline float SelfplayUniform(uint64_t key, int a) {
  const uint32_t n = (uint32_t)(PlayoutMix(key + (uint64_t)a) >> 41);
  return ((float)n + 0.5f) * 1.1920928955078125e-7f;  // 2^-23
}

PGX_HD inline float GumbelLog(float x) {
  int e;
  float m = frexpf(x, &e);
  if (m < 0.70710678f) {
    m *= 2.0f;
    e -= 1;
  }
  const float f = m - 1.0f;
  const float s = f / (2.0f + f);
  const float z = s * s;
  float p = 1.0f / 9.0f;
  p = p * z + 1.0f / 7.0f;
  p = p * z + 1.0f / 5.0f;
  p = p * z + 1.0f / 3.0f;
  p = p * z;
  const float s2 = 2.0f * s;
  const float r = s2 * p + s2;
  const float fe = (float)e;
  return fe * 0.693359375f + (r + fe * -2.12194440e-4f);
}

PGX_HD inline float SelfplayNoise(uint64_t key, int a) { return -GumbelLog(-GumbelLog(SelfplayUniform(key, a))); }

PGX_HD inline int SelfplayGumbelAction(int action) { return action < 0 ? 0 : action; }

// PUCT: where the sampled move's prefix sum has to pass, for a root of V > 0 visits
PGX_HD inline uint32_t SelfplaySampleAt(uint64_t key, uint32_t V) {
  return (uint32_t)(((PlayoutMix(key + kSelfplaySampleSalt) >> 32) * (uint64_t)V) >> 32);
}
PGX_HD inline float SelfplayTarget(int visits, int V) { return (float)visits / (float)V; }

// The PUCT move of one row, as a walk over its A actions (the harness; the kernel gives the row to a lane group).
// the lowest action whose inclusive prefix sum of visits exceeds r (r < V)
PGX_HD inline int SelfplayPickSampled(const int32_t* visits, int A, uint32_t r) {
  uint32_t run = 0;
  for (int a = 0; a < A; ++a) {
    run += (uint32_t)visits[a];
    if (run > r) return a;
  }
  return A - 1;  // (never: r < V)
}
// the most visited action, the lowest on ties
PGX_HD inline int SelfplayPickGreedy(const int32_t* visits, int A) {
  int best = 0;
  for (int a = 1; a < A; ++a) {
    if (visits[a] > visits[best]) best = a;
  }
  return best;
}
// target: A floats out.  Returns the action.
PGX_HD inline int SelfplayPuctMove(const int32_t* visits, int A, int result_action, int elapsed, int sample_plies,
                                   uint64_t key, float* target) {
  long long V = 0;
  for (int a = 0; a < A; ++a) V += visits[a];
  if (V == 0 || result_action < 0) {
    for (int a = 0; a < A; ++a) target[a] = 0.0f;
    return 0;
  }
  for (int a = 0; a < A; ++a) target[a] = SelfplayTarget(visits[a], (int)V);
  if (elapsed < sample_plies) return SelfplayPickSampled(visits, A, SelfplaySampleAt(key, (uint32_t)V));
  return SelfplayPickGreedy(visits, A);
}

// what one row of the step's results adds to the counters (games, wins0, wins1, draws, plies)
PGX_HD inline void SelfplayTallyRow(bool done, float r0, float r1, int elapsed, int out[kSelfplayCounters]) {
  out[0] = done ? 1 : 0;
  out[1] = (done && r0 > 0.0f) ? 1 : 0;
  out[2] = (done && r1 > 0.0f) ? 1 : 0;
  out[3] = (done && r0 == 0.0f && r1 == 0.0f) ? 1 : 0;
  out[4] = done ? elapsed : 0;
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_SELFPLAY_HIP_H_
