// PGX self-play driver, PUCT exploration: Dirichlet root noise and the move temperature, as __host__ __device__ pieces
// shared by the kernels (PgxSelfplayDirichlet / PgxSelfplayMoveTemp in pgx_selfplay.hip) and the g++ host harness of the
// tests (tests/cpu_harness/pgx_dirichlet_host.cpp, which walks the lanes as loops).  This header is the authority;
// DESIGN.md "PGX self-play driver: Dirichlet noise and temperature" restates it.
//
// The contract.  Everything is built from what the tree already proves bit-equal between g++, the device and numpy:
// SM = PlayoutMix, SelfplayKey / SelfplayUniform (pgx_selfplay.hip.h), GumbelLog, GumbelExp (pgx_gumbel.hip.h),
// ActorNormal (actor.hip.h) and correctly rounded float32 + - * /.  No other transcendental.  The build keeps
// -ffp-contract=off and no fast-math.  U(i) = SelfplayUniform(key(e, t), i) for env e at driver ply t.
//   draws     The driver's indices so far are the actions a < 127 (Gumbel noise) and 0x100 (the PUCT sample).  The new
//             ones live at I(a, j, c) = 0x200 + ((a * J + j) * 4 + c), J = 16, a the action:
//               attempt j < J of action a:  u0 = U(I(a, j, 0)),  u1 = U(I(a, j, 1))
//               the boost of action a:      u2 = U(I(a, J, 2))
//             (I(a, J, 2) = I(a + 1, 0, 2), and no attempt has a role 2: the indices are pairwise different)
//   gamma     One Gamma(alpha) variate per (row, action), 0 < alpha <= 100, always as a boosted Gamma(alpha + 1): one
//             code path.  d = (alpha + 1) - 1/3 and c = 1 / sqrt(9 d) are computed ON THE HOST in double from the
//             float32 alpha -- d = ((double)alpha + 1.0) - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d) -- rounded to float32
//             once and passed in (DirichletParams).  Attempt j (Marsaglia-Tsang), all float32:
//               x = ActorNormal(u0);  t = 1 + c * x;  v = (t * t) * t
//               v <= 0: rejected
//               otherwise accepted iff  GumbelLog(u1) < (((0.5f * x) * x + d) - d * v) + d * GumbelLog(v)
//             y = d * v of the first accepted attempt; none of the J accepted: y = d (the fallback).
//               g = y * GumbelExp(GumbelLog(u2) / alpha);   g = g < 1e-30f ? 1e-30f : g
//             (the floor: a subnormal product must not depend on a flush mode.  GumbelExp clamps its argument to
//             [-87, 0], so every g is positive and finite)                                          (DirichletGamma)
//   row       eta[a] = g[a] / S on the legal actions (mask[a] != 0), 0 elsewhere.  S is the sum of the legal g[a] in ONE
//             order, a function of A only: LG = the power of two at or above A, at most 64, E = ceil(A / LG) -- the
//             lane group of PgxSelfplayMove<PUCT> -- lane j's partial is ((0 + w(j E)) + w(j E + 1)) + ..., its E
//             consecutive actions in ascending order starting from +0.0f, w(a) = g[a] for a legal a < A and +0.0f
//             otherwise; then the butterfly x[j] += x[j ^ w] for w = LG / 2, .., 2, 1.  Every lane ends with the same
//             bits.  A row without a legal action is all zeros (S is not divided by)               (DirichletRow)
//   mix       om = 1.0f - eps, once.  p'[a] = om * p[a] + eps * eta[a] on the legal actions of a row whose root has
//             status 0 (evaluate); illegal entries are not touched (the net leaves them 0), nor is a row of another
//             status.  The noise row itself is written for every row (a root that is over has an empty mask and
//             gets zeros)                                                                            (DirichletMix)
//   temperature T (float32, T != 1), a PUCT row with V = SUM visits > 0 whose env's elapsed step < sample_plies:
//               vmax = the largest visit count
//               q[a] = (uint32)(GumbelExp(GumbelLog((float)visits[a] / (float)vmax) / T) * 1048576.0f), visits[a] > 0
//               q[a] = 0,  visits[a] == 0
//             The most visited action has q = 2^20 exactly (GumbelLog(1) = 0, GumbelExp(0) = 1), so Q = SUM q >= 2^20,
//             and Q <= 127 * 2^20 < 2^32.  The move is the existing integer pick over q: r = SelfplaySampleAt(key, Q),
//             the lowest a whose inclusive prefix sum of q exceeds r.  Integers from there on: no launch geometry
//             enters.  The target row stays visits / V; the greedy rule (elapsed >= sample_plies) and the zero rows are
//             SelfplayPuctMove's.  T == 1 IS SelfplayPuctMove: the driver takes this path only for T != 1
//                                                                                              (SelfplayPuctMoveTemp)
#ifndef ENVPOOL_AMD_CSRC_PGX_DIRICHLET_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_DIRICHLET_HIP_H_

#include <cmath>

#include "actor.hip.h"
#include "pgx_gumbel.hip.h"
#include "pgx_selfplay.hip.h"

namespace epa {
namespace pgx {

constexpr int kDirichletAttempts = 16;         // J
constexpr int kDirichletBase = 0x200;          // above the sample's 0x100
constexpr float kDirichletFloor = 1e-30f;
constexpr float kTemperatureScale = 1048576.0f;  // 2^20
constexpr float kDirichletMaxAlpha = 100.0f;
constexpr float kTemperatureMin = 0.05f, kTemperatureMax = 20.0f;

PGX_HD inline int DirichletIndex(int a, int j, int c) { return kDirichletBase + ((a * kDirichletAttempts + j) * 4 + c); }

// alpha with the two constants of its boosted sampler, as the host rounds them
struct DirichletParams {
  float alpha, d, c;
};
inline DirichletParams DirichletParamsOf(float alpha) {
  const double d = ((double)alpha + 1.0) - 1.0 / 3.0;
  return {alpha, (float)d, (float)(1.0 / std::sqrt(9.0 * d))};
}

// The lane group of a row of A actions: LG lanes, E consecutive actions each
PGX_HD constexpr int DirichletGroup(int A) {
  int lg = 1;
  while (lg < A && lg < 64) lg <<= 1;
  return lg;
}
PGX_HD constexpr int DirichletRun(int A) { return (A + DirichletGroup(A) - 1) / DirichletGroup(A); }

// g of (key, action a); *fallback (may be null) is set to 1 when none of the J attempts accepted
PGX_HD inline float DirichletGamma(uint64_t key, int a, const DirichletParams& p, int* fallback) {
  float y = p.d;
  bool accepted = false;
  for (int j = 0; j < kDirichletAttempts && !accepted; ++j) {
    const float x = actor::ActorNormal(SelfplayUniform(key, DirichletIndex(a, j, 0)));
    const float t = 1.0f + p.c * x;
    const float v = (t * t) * t;
    if (v <= 0.0f) continue;
    const float lhs = GumbelLog(SelfplayUniform(key, DirichletIndex(a, j, 1)));
    const float rhs = (((0.5f * x) * x + p.d) - p.d * v) + p.d * GumbelLog(v);
    if (lhs < rhs) {
      y = p.d * v;
      accepted = true;
    }
  }
  if (fallback != nullptr) *fallback = accepted ? 0 : 1;
  const float u2 = SelfplayUniform(key, DirichletIndex(a, kDirichletAttempts, 2));
  const float g = y * GumbelExp(GumbelLog(u2) / p.alpha);
  return g < kDirichletFloor ? kDirichletFloor : g;
}

// S of a row, in the contract's order (the harness; the kernel gives lane j of the row's group its run)
inline float DirichletSum(const float* g, const unsigned char* mask, int A) {
  const int LG = DirichletGroup(A), E = DirichletRun(A);
  float x[64], y[64];
  for (int j = 0; j < LG; ++j) {
    float part = 0.0f;
    for (int i = 0; i < E; ++i) {
      const int a = j * E + i;
      part = part + ((a < A && mask[a] != 0) ? g[a] : 0.0f);
    }
    x[j] = part;
  }
  for (int w = LG / 2; w >= 1; w >>= 1) {
    for (int j = 0; j < LG; ++j) y[j] = x[j] + x[j ^ w];
    for (int j = 0; j < LG; ++j) x[j] = y[j];
  }
  return x[0];
}

PGX_HD inline float DirichletEta(float g, float S) { return g / S; }
PGX_HD inline float DirichletMix(float p, float eta, float om, float eps) { return om * p + eps * eta; }

// One row as a walk (the harness): eta [A] out; prior [A] is mixed in place when status == 0 (null: no mix).
// Returns the number of actions that took the fallback.
inline int DirichletRow(uint64_t key, const unsigned char* mask, int A, const DirichletParams& p, float eps,
                        int status, float* eta, float* prior) {
  float g[128];
  int fallbacks = 0, legal = 0;
  for (int a = 0; a < A; ++a) {
    int fb = 0;
    g[a] = DirichletGamma(key, a, p, &fb);
    if (mask[a] != 0) {
      fallbacks += fb;
      ++legal;
    }
  }
  const float S = DirichletSum(g, mask, A);
  const float om = 1.0f - eps;
  for (int a = 0; a < A; ++a) {
    eta[a] = (legal != 0 && mask[a] != 0) ? DirichletEta(g[a], S) : 0.0f;
    if (prior != nullptr && status == 0 && mask[a] != 0) prior[a] = DirichletMix(prior[a], eta[a], om, eps);
  }
  return fallbacks;
}

// q of one action
PGX_HD inline uint32_t TemperatureWeight(int visits, int vmax, float T) {
  if (visits <= 0) return 0u;
  return (uint32_t)(GumbelExp(GumbelLog((float)visits / (float)vmax) / T) * kTemperatureScale);
}

// SelfplayPuctMove with a temperature: q [A] out (the weights the sampled move was drawn from; zeros where no move was
// sampled).  T == 1 calls SelfplayPuctMove.
inline int SelfplayPuctMoveTemp(const int32_t* visits, int A, int result_action, int elapsed, int sample_plies,
                                uint64_t key, float T, float* target, uint32_t* q) {
  for (int a = 0; a < A; ++a) q[a] = 0u;
  if (T == 1.0f) return SelfplayPuctMove(visits, A, result_action, elapsed, sample_plies, key, target);
  long long V = 0;
  int vmax = 0;
  for (int a = 0; a < A; ++a) {
    V += visits[a];
    vmax = visits[a] > vmax ? visits[a] : vmax;
  }
  if (V == 0 || result_action < 0) {
    for (int a = 0; a < A; ++a) target[a] = 0.0f;
    return 0;
  }
  for (int a = 0; a < A; ++a) target[a] = SelfplayTarget(visits[a], (int)V);
  if (elapsed >= sample_plies) return SelfplayPickGreedy(visits, A);
  uint32_t Q = 0;
  for (int a = 0; a < A; ++a) {
    q[a] = TemperatureWeight(visits[a], vmax, T);
    Q += q[a];
  }
  return SelfplayPickSampled(reinterpret_cast<const int32_t*>(q), A, SelfplaySampleAt(key, Q));
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_DIRICHLET_HIP_H_
