// PGX trainer: the contract of the rest of a training step of the built-in nets -- loss, gradient norm, optimizer,
// re-quantising and the minibatch gather -- behind `net.trainer(...)` (DESIGN.md "PGX trainer").  Host + device: the
// kernels (pgx_trainer.hip) and the g++ harness of the tests (tests/cpu_harness/pgx_trainer_host.cpp) run this code;
// tests/pgx_trainer_util.py restates it in numpy float64.  Built with -ffp-contract=off: every operation below is one
// rounding, in the order written.
//
// LOSS of a row, all float32.  Inputs: the forward's p int32 [A + 1], mask u8 [A], the targets pi float32 [A] (not
// negative; the recorder does not normalise them) and z, the net's scale_p and scale_v, value_weight, nf = (float)n
// for a minibatch of n rows.  Action a is legal when mask[a] != 0.
//   logit_a = NetLogit(p_a, scale_p);  m = the largest legal logit;  e_a = GumbelExp(logit_a - m)
//   S = SUM e_a,  T = SUM pi_a,  U = SUM pi_a * logit_a, each over the legal actions in ascending a from 0.0f
//   policy loss  T * (m + GumbelLog(S)) - U
//   dp_a = (scale_p * (T * (e_a / S) - pi_a)) / nf for a legal action, 0 for an illegal one
//   v = (float)p_A * scale_v (not clamped);  value loss  value_weight * ((v - z) * (v - z))
//   dp_A = ((2.0f * value_weight) * scale_v) * (v - z) / nf
// A row with no legal action has policy loss 0 and a zero policy gradient; its value part is as above.
//
// kLossErr.  Against the same formulas in exact arithmetic on the float32 logits and v (one conversion and one multiply
// each, which the float64 restatement repeats in float32), with u = 2^-24 and the argument of the exponential in
// [-87, 0] (GumbelExp clamps it; so does the restatement):
//   d = logit - m: one rounding, u |d| <= 87 u absolute, that is 87 u = 5.2e-6 relative in e; GumbelExp itself is
//   within 2^-20 = 9.5e-7 (its degree-6 polynomial leaves 0.35^7 / 5040 = 1.3e-7, its reduction and seven Horner steps a
//   few u each): e_a within 6.2e-6.  S: the same, plus at most 126 additions, 126 u = 7.5e-6.  e / S: u.  T: 126 u of
//   SUM |pi|.  T * q, the subtraction, the scaling and the division by nf: 4 u of the magnitudes.
//   |dp_a - exact| <= (2 * 6.2e-6 + 7.5e-6 + 7.5e-6 + 5 u) * scale_p (T q_a + |pi_a|) / n = 2.8e-5 of it.
// kLossErr = 2^-15 = 3.05e-5 covers that.  The value gradient takes five roundings: 5 u |dp_A|, far inside.  The
// policy loss is held to kLossErr * (T (|m| + |log S| + 1) + SUM |pi_a logit_a|): the 1 is the relative error of S as
// an absolute error of its logarithm, GumbelLog's own 2e-6 included.
//
// STATISTICS.  A step writes four doubles: SUM policy loss / n, SUM value loss / n, the gradient norm, n.  The row
// losses are widened to double and added per block of kTrainerLossRows rows in ascending row order, the blocks'
// partials in ascending block order.
//
// NORM.  All gradients form one flat table of SEGMENTS: the weight arrays of the layers in the blob's order, then the
// bias arrays, each padded with zeros to a multiple of kTrainerChunk = 1024 elements.  Thread t of a chunk's block adds
// the squares (exact in double) of elements 4 t .. 4 t + 3 in that order from 0.0; the 256 sums fold as a tree,
// s[t] += s[t + w] for w = 128, 64, .., 1; the chunks' partials are added in ascending chunk order and
// norm = sqrt(sum), IEEE.  clip_scale = clip == 0 ? 1 : min(1, clip / (norm + 1e-6)).
//
// UPDATE of one element, float64 (TrainerUpdateOne):  g = (double)grad * clip_scale + weight_decay * master;
//   sgd   buf = momentum * buf + g;  master = master - lr * buf
//   adam  m = beta1 * m + (1 - beta1) * g;  v = beta2 * v + ((1 - beta2) * g) * g;
//         master = master - (lr_t * m) / (sqrt(v) + eps),  lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) for step
//         t = 1, 2, .., the powers kept as running products; 1 - beta and lr_t are the host's doubles
// and then the quantised value of the new master, `Net.from_module`'s rule: rint (half to even), a weight clamped to
// -127 .. 127 as int8, a bias to +-2^30 as int32.
//
// GATHER.  Row j of step t (t counts the handle's steps from 0, across calls) is sample TrainerIndex(seed, t, j, count)
// of the sample arrays: sampling with replacement, count >= 1.
#ifndef ENVPOOL_AMD_CSRC_PGX_TRAINER_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_TRAINER_HIP_H_

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "pgx_net.hip.h"
#include "pgx_selfplay.hip.h"

namespace epa {
namespace pgx {

constexpr double kLossErr = 1.0 / 32768.0;
constexpr int kTrainerLossRows = 32;   // rows of a loss block: one partial of the statistics
constexpr int kTrainerChunk = 1024;    // elements of a norm / update block: 256 threads of 4
constexpr int kTrainerStatRows = 4096; // the ring of statistics rows
constexpr int kTrainerSgd = 0, kTrainerAdam = 1;

PGX_HD inline uint32_t TrainerIndex(uint64_t seed, uint32_t t, uint32_t j, uint32_t count) {
  const uint64_t h = PlayoutMix(seed ^ PlayoutMix(((uint64_t)t << 32) | (uint64_t)j));
  return (uint32_t)(((h >> 32) * (uint64_t)count) >> 32);
}

// the pieces of the loss the kernel's lanes and the row loop below share
PGX_HD inline float TrainerPolicyGrad(float scale_p, float T, float e, float S, float pi, float nf) {
  return (scale_p * (T * (e / S) - pi)) / nf;
}
PGX_HD inline float TrainerPolicyLoss(float T, float m, float S, float U) { return T * (m + GumbelLog(S)) - U; }
PGX_HD inline float TrainerValueGrad(float value_weight, float scale_v, float v, float z, float nf) {
  return ((2.0f * value_weight) * scale_v) * (v - z) / nf;
}
PGX_HD inline float TrainerValueLoss(float value_weight, float v, float z) { return value_weight * ((v - z) * (v - z)); }

// One row by the book: dp [A + 1] and loss[0] (policy), loss[1] (value).
inline void TrainerLossRow(const int32_t* p, const unsigned char* mask, const float* pi, float z, int A, float scale_p,
                           float scale_v, float value_weight, float nf, float* dp, float* loss) {
  float m = -FLT_MAX;
  bool any = false;
  for (int a = 0; a < A; ++a) {
    if (mask[a] == 0) continue;
    const float l = NetLogit(p[a], scale_p);
    any = true;
    m = l > m ? l : m;
  }
  float S = 0.0f, T = 0.0f, U = 0.0f;
  for (int a = 0; a < A; ++a) {
    if (mask[a] == 0) continue;
    const float l = NetLogit(p[a], scale_p);
    S = S + GumbelExp(l - m);
    T = T + pi[a];
    U = U + pi[a] * l;
  }
  for (int a = 0; a < A; ++a) {
    const float l = NetLogit(p[a], scale_p);
    dp[a] = mask[a] != 0 ? TrainerPolicyGrad(scale_p, T, GumbelExp(l - m), S, pi[a], nf) : 0.0f;
  }
  loss[0] = any ? TrainerPolicyLoss(T, m, S, U) : 0.0f;
  const float v = (float)p[A] * scale_v;
  dp[A] = TrainerValueGrad(value_weight, scale_v, v, z, nf);
  loss[1] = TrainerValueLoss(value_weight, v, z);
}

// What an update needs beside the element: the host's doubles.
struct TrainerRule {
  int optimizer;
  double lr, momentum, beta1, beta2, one_minus_beta1, one_minus_beta2, lr_t, eps, weight_decay;
};

// One element; s1 is sgd's buf or adam's m, s2 adam's v.
PGX_HD inline void TrainerUpdateOne(const TrainerRule& r, float grad, double clip_scale, double* master, double* s1,
                                    double* s2) {
  const double g = (double)grad * clip_scale + r.weight_decay * *master;
  if (r.optimizer == kTrainerSgd) {
    *s1 = r.momentum * *s1 + g;
    *master = *master - r.lr * *s1;
  } else {
    *s1 = r.beta1 * *s1 + r.one_minus_beta1 * g;
    *s2 = r.beta2 * *s2 + (r.one_minus_beta2 * g) * g;
    *master = *master - (r.lr_t * *s1) / (sqrt(*s2) + r.eps);
  }
}
PGX_HD inline int32_t TrainerQuantWeight(double master) {
  const double q = rint(master);
  return (int32_t)(q < -127.0 ? -127.0 : (q > 127.0 ? 127.0 : q));
}
PGX_HD inline int32_t TrainerQuantBias(double master) {
  const double q = rint(master), top = (double)kNetMaxBias;
  return (int32_t)(q < -top ? -top : (q > top ? top : q));
}
PGX_HD inline double TrainerClipScale(double clip, double norm) {
  if (clip == 0.0) return 1.0;
  const double s = clip / (norm + 1e-6);
  return s < 1.0 ? s : 1.0;
}

// The norm's sum over one chunk of kTrainerChunk gradients, in the kernel's order.
inline double TrainerChunkSquares(const float* grad) {
  double s[256];
  for (int t = 0; t < 256; ++t) {
    double a = 0.0;
    for (int q = 0; q < 4; ++q) a = a + (double)grad[4 * t + q] * (double)grad[4 * t + q];
    s[t] = a;
  }
  for (int w = 128; w >= 1; w >>= 1) {
    for (int t = 0; t < w; ++t) s[t] = s[t] + s[t + w];
  }
  return s[0];
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_TRAINER_HIP_H_
