// PPO trainer of the rollout actor: the contract of a PPO step on the built-in actor-critic -- the clipped-surrogate
// loss of both heads, the trained sigma of a Box head, the advantage statistics, the epoch permutation and the
// minibatch gather -- behind `actor.trainer(...)` (DESIGN.md section 2 "Rollout actor: PPO trainer").  Host + device:
// the kernels (ppo_trainer.hip) and the g++ harness of the tests (tests/cpu_harness/ppo_trainer_host.cpp) run this
// code; tests/ppo_trainer_util.py restates it in numpy float64.  Built with -ffp-contract=off: every operation below
// is one rounding, in the order written.  Norm, clip scale, update and re-quantising are pgx_trainer.hip.h's.
//
// A ROW has p int32 [H + 1] from the trunk's forward, the action a (int32, or float32 [H]), the old logp, adv, ret,
// the mask and nf = (float)rows of the minibatch; the options clip_ratio, value_weight, entropy_weight are float32,
// lo = 1.0f - clip_ratio, hi = 1.0f + clip_ratio and ew = entropy_weight / nf are formed once in float32.
// l_j = NetLogit(p_j, scale_p).  A row with mask 0 (the auto-reset step after a done) has dp = 0 in all H + 1 places,
// adds nothing to any sum and is counted in `rows` only.
//   discrete  top = max l_j;  e_j = GumbelExp(l_j - top);  S = SUM e_j in ascending j from 0.0f (SampleDiscrete's
//             order);  q_j = e_j / S;  lq_j = (l_j - top) - GumbelLog(S);  logp' = lq_a;
//             Hn = -(SUM q_j * lq_j), ascending j from 0.0f
//   box       mu_j = l_j;  z_j = (a_j - mu_j) / sigma_j;
//             logp' = SUM ((-0.5f * z_j) * z_j - GumbelLog(sigma_j)) - 0.9189385f, ascending j from 0.0f
//             (SampleBoxTerm's term with the given action);  Hn = SUM (0.5f + 0.9189385f) + GumbelLog(sigma_j)
//   masked    (actor.hip.h kind 2) discrete's formulas with j running over the row's legal set (LegalBit of its 128-bit
//             word) only: top, e_j, S, q_j, lq_j, Hn and dp_j exist for legal j, the ordered sums skip illegal j, and
//             dp_j = 0.0f exactly for illegal j.  The action is the flat index (a gather rebuilds it from the stored
//             components by ActorFlat) and must be legal.  A row whose set is everything is a discrete row, bit for bit.
//   ratio     d = clamp(logp' - logp, -kPpoLogRatio, kPpoLogRatio);  r = d <= 0 ? GumbelExp(d) : 1.0f / GumbelExp(-d)
//             (GumbelExp clamps its argument to [-87, 0]);  rc = clamp(r, lo, hi);  policy loss = -min(r adv, rc adv);
//             active = r adv <= rc adv;  g = active ? -(adv * r) / nf : 0
//   discrete  dp_j = scale_p * (g * ([j = a] - q_j) + ew * q_j * (lq_j + Hn))          (left to right)
//   box       dp_j = ((scale_p * g) * z_j) / sigma_j;  dsigma_j = (g * (z_j * z_j - 1.0f)) / sigma_j - ew / sigma_j
//   value     v = (float)p_H * scale_v; TrainerValueLoss / TrainerValueGrad with value_weight against ret
//
// STATISTICS.  A step writes kPpoStats = 8 doubles: the sums of policy loss, value loss and Hn over the unmasked rows
// each divided by their count (0 without any), the mean of (r - 1.0f) - d, the share of unmasked rows with r != rc, the
// gradient norm, the unmasked rows, the rows.  Row values are widened to double and added per block of kPpoLossRows rows
// in ascending row order, the blocks' partials in ascending block order (pgx_trainer.hip.h's order).
//
// SIGMA.  With train_sigma a Box actor's H sigmas are one more segment of the flat gradient table, padded to one chunk
// behind the biases: NORM covers it unchanged.  A block's rows' dsigma_j are added in double in ascending row order, the
// blocks' partials in ascending block order, and the gradient is (float) of that.  TrainerUpdateOne moves a float64
// master (it starts as the blob's sigma); the sigma a loss reads is (float)max(master, kPpoSigmaMin).
//
// ADVANTAGE STATISTICS of a horizon adv [T N] with mask [T N], in double by a fixed tree: a block takes kPpoAdvChunk =
// 1024 consecutive elements, thread t of 256 adds cnt += 1, s1 += x, s2 += x * x over its unmasked elements 4 t .. 4 t +
// 3 in that order from 0; the 256 triples fold as a tree, s[t] += s[t + w] for w = 128, 64, .., 1; the blocks' partials
// are added in ascending block order.  mean = s1 / cnt, std = sqrt(max(s2 / cnt - mean * mean, 0)) (both 0 for cnt = 0);
// adv_n = (float)(((double)adv - mean) / (std + 1e-8)).
//
// SAMPLING.  Flat row i = t N + e.  Position j of epoch E (counted over the handle's life) is PpoPermute(seed, E, j,
// T N): a balanced Feistel network of 4 rounds over 2 b bits, b >= 1 the smallest with 2^(2 b) >= T N, round function
// PlayoutMix(seed ^ PlayoutMix(E << 32 | round << 16 | half)) & (2^b - 1), applied again while the image is >= T N
// (cycle walking): a bijection of 0 .. T N - 1.  Step s of an epoch takes positions s batch .. s batch + batch - 1;
// an epoch makes T N / batch steps and leaves the tail of the permutation unused.
//
// GATHER.  Row i gives the feature bytes ActorFeature(ActorLoad(obs_k slot t row e), lo, scale) over the obs keys in key
// order, the action row converted to int32 (discrete) or float32 (box), logp[t][e], adv_n (adv as it is without
// normalize_adv), ret[t][e] and mask[t][e].
//
// kPpoErr.  Against the same formulas in exact arithmetic on the float32 inputs (l_j, v, sigma, lo, hi, ew as formed
// above, which the float64 restatement repeats in float32), u = 2^-24.  From pgx_trainer.hip.h: e_j within 6.2e-6, S
// within 1.37e-5, q_j within 2.0e-5 (relative).  GumbelLog(x) is within 4 u (|log x| + 0.35) absolute (its series leaves
// 7e-10, the rest are roundings of r and of e ln 2).
//   discrete  lq_j: u |l_j - top| + 1.37e-5 + 4 u (|log S| + 0.35) + u |lq_j| <= 1.6e-5 + 5 u M_j absolute,
//             M_j = |l_j - top| + |log S|;  W = 1 + max_j M_j / 128.
//   box       z_j 2 u relative; a term: 5 u (z_j^2 / 2) + 4 u (|log sigma_j| + 0.35) + 3 u |term|; H <= 127 additions:
//             logp' within 135 u M absolute, M = SUM z_j^2 / 2 + |log sigma_j| + 0.92;  W = 1 + M / 2.
//   d: one more rounding, 20 u.  r: d's absolute error as a relative one, GumbelExp's 2^-20 and the reciprocal's u:
//   relative error of r <= 1.9e-5 W (discrete: 1.6e-5 + 1.2e-6 + 1.1e-6 + 5 u M_a; box: 2.3e-6 + 8.1e-6 M).  g: 2 u more.
//   discrete dp_j: g ([j = a] - q_j) within |g| ([j = a] + q_j) (1.9e-5 W + 2.0e-5 + 4 u); Hn within 4.8e-5 Hn + 1.6e-5 W
//   (q_j, lq_j, 127 additions); ew q_j (lq_j + Hn) within ew q_j (|lq_j| + Hn + 1) 4.8e-5 W; scale and sum 2 u:
//     |dp_j - exact| <= kPpoErr * scale_p W (|g| ([j = a] + q_j) + ew q_j (|lq_j| + Hn + 1)),   kPpoErr = 2^-14 = 6.1e-5
//   box dp_j: relative 1.9e-5 W + 6 u: kPpoErr * W scale_p |g z_j| / sigma_j.
//   dsigma_j of a row: kPpoErr * W (|g| (z_j^2 + 1) + ew) / sigma_j; the sums in double and the final (float) add u.
//   The value gradient takes five roundings.  Loss terms: policy kPpoErr * W |adv| max(r, rc); value 4 u; Hn kPpoErr *
//   W (Hn + 1) (box: kPpoErr * SUM 1.42 + |log sigma_j|); (r - 1) - d: kPpoErr * W (r + 1).
//   masked: every bound above holds with its sums, maxima and M_j taken over the legal set -- the same operations on
//   fewer terms -- so kPpoErr and the discrete formula carry over unchanged; an illegal j has error 0.
// `active` and r != rc are not continuous: a row whose exact r lies within 1.9e-5 W of lo or hi may fall either way, and
// the tests keep their rows away from there.
#ifndef ENVPOOL_AMD_CSRC_PPO_TRAINER_HIP_H_
#define ENVPOOL_AMD_CSRC_PPO_TRAINER_HIP_H_

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "actor.hip.h"
#include "pgx_trainer.hip.h"

namespace epa {
namespace ppo {

constexpr double kPpoErr = 1.0 / 16384.0;
constexpr float kPpoLogRatio = 20.0f;
constexpr double kPpoSigmaMin = 1.0 / 1024.0;
constexpr int kPpoLossRows = pgx::kTrainerLossRows;  // rows of a loss block: one partial of the statistics
constexpr int kPpoPartials = 6;                       // a block's sums: the five of the statistics and the unmasked rows
constexpr int kPpoStats = 8;                          // doubles of a statistics row
constexpr int kPpoAdvChunk = 1024;                    // elements of an advantage-statistics block: 256 threads of 4
constexpr float kPpoHalfLog2Pi = 0.9189385f;

// ---- sampling --------------------------------------------------------------------------------------------------------
PGX_HD inline int PpoPermuteBits(uint32_t n) {
  int b = 1;
  while (b < 16 && ((uint64_t)1 << (2 * b)) < (uint64_t)n) ++b;
  return b;
}
PGX_HD inline uint32_t PpoPermute(uint64_t seed, uint32_t epoch, uint32_t j, uint32_t n) {
  const int b = PpoPermuteBits(n);
  const uint32_t half = ((uint32_t)1 << b) - 1u;
  uint32_t x = j;
  do {
    uint32_t left = x >> b, right = x & half;
    for (uint32_t round = 0; round < 4; ++round) {
      const uint64_t f = pgx::PlayoutMix(seed ^ pgx::PlayoutMix(((uint64_t)epoch << 32) | (uint64_t)(round << 16) | right));
      const uint32_t next = left ^ ((uint32_t)f & half);
      left = right;
      right = next;
    }
    x = (left << b) | right;
  } while (x >= n);
  return x;
}

// ---- advantage statistics ----------------------------------------------------------------------------------------------
struct AdvSums {
  double cnt, s1, s2;
};
PGX_HD inline void AdvAdd(AdvSums* s, float x, unsigned char mask) {
  if (mask == 0) return;
  const double v = (double)x;
  s->cnt = s->cnt + 1.0;
  s->s1 = s->s1 + v;
  s->s2 = s->s2 + v * v;
}
// mean and std from the horizon's sums
PGX_HD inline void AdvMoments(const AdvSums& s, double* mean, double* std) {
  *mean = 0.0, *std = 0.0;
  if (s.cnt == 0.0) return;
  *mean = s.s1 / s.cnt;
  const double var = s.s2 / s.cnt - *mean * *mean;
  *std = sqrt(var > 0.0 ? var : 0.0);
}
PGX_HD inline float AdvNormalize(float adv, double mean, double std) { return (float)(((double)adv - mean) / (std + 1e-8)); }
// one block of the tree, by the book: n <= kPpoAdvChunk elements
inline AdvSums AdvChunkSums(const float* adv, const unsigned char* mask, int n) {
  AdvSums s[256];
  for (int t = 0; t < 256; ++t) {
    s[t] = AdvSums{0.0, 0.0, 0.0};
    for (int q = 0; q < 4; ++q) {
      if (4 * t + q < n) AdvAdd(&s[t], adv[4 * t + q], mask[4 * t + q]);
    }
  }
  for (int w = 128; w >= 1; w >>= 1) {
    for (int t = 0; t < w; ++t) {
      s[t].cnt = s[t].cnt + s[t + w].cnt, s[t].s1 = s[t].s1 + s[t + w].s1, s[t].s2 = s[t].s2 + s[t + w].s2;
    }
  }
  return s[0];
}

// ---- the loss: the pieces the kernel's lanes and the row loops below share ---------------------------------------------
struct PpoOptions {
  float scale_p, scale_v, lo, hi, value_weight, ew, nf;  // lo, hi: 1 -+ clip_ratio; ew: entropy_weight / nf
};
PGX_HD inline PpoOptions PpoOptionsOf(float scale_p, float scale_v, float clip_ratio, float value_weight,
                                      float entropy_weight, int rows) {
  PpoOptions o;
  o.scale_p = scale_p, o.scale_v = scale_v, o.value_weight = value_weight, o.nf = (float)rows;
  o.lo = 1.0f - clip_ratio, o.hi = 1.0f + clip_ratio, o.ew = entropy_weight / o.nf;
  return o;
}
struct PpoRatioOut {
  float g, loss, kl;
  int clipped;
};
PGX_HD inline PpoRatioOut PpoRatio(float logp_new, float logp_old, float adv, const PpoOptions& o) {
  float d = logp_new - logp_old;
  d = d < -kPpoLogRatio ? -kPpoLogRatio : (d > kPpoLogRatio ? kPpoLogRatio : d);
  const float r = d <= 0.0f ? pgx::GumbelExp(d) : 1.0f / pgx::GumbelExp(-d);
  const float rc = r < o.lo ? o.lo : (r > o.hi ? o.hi : r);
  const float full = r * adv, cut = rc * adv;
  PpoRatioOut out;
  out.loss = -(full < cut ? full : cut);
  out.g = full <= cut ? -(adv * r) / o.nf : 0.0f;
  out.kl = (r - 1.0f) - d;
  out.clipped = r != rc ? 1 : 0;
  return out;
}
PGX_HD inline float PpoDiscreteGrad(const PpoOptions& o, float g, bool taken, float q, float lq, float Hn) {
  return o.scale_p * (g * ((taken ? 1.0f : 0.0f) - q) + o.ew * q * (lq + Hn));
}
PGX_HD inline float PpoBoxZ(float action, float mu, float sigma) { return (action - mu) / sigma; }
PGX_HD inline float PpoBoxTerm(float z, float log_sigma) { return ((-0.5f * z) * z - log_sigma) - kPpoHalfLog2Pi; }
PGX_HD inline float PpoBoxEntropyTerm(float log_sigma) { return (0.5f + kPpoHalfLog2Pi) + log_sigma; }
PGX_HD inline float PpoBoxGrad(const PpoOptions& o, float g, float z, float sigma) { return ((o.scale_p * g) * z) / sigma; }
PGX_HD inline float PpoSigmaGrad(const PpoOptions& o, float g, float z, float sigma) {
  return (g * (z * z - 1.0f)) / sigma - o.ew / sigma;
}
PGX_HD inline float PpoSigmaOf(double master) { return (float)(master > kPpoSigmaMin ? master : kPpoSigmaMin); }

// One row by the book.  dp [H + 1]; stat[5]: policy loss, value loss, Hn, (r - 1) - d, r != rc; dsigma [H] (box).  A
// masked row: zeros everywhere.
inline void PpoValuePart(const int32_t* p, int H, float ret, const PpoOptions& o, float* dp, float* stat) {
  const float v = (float)p[H] * o.scale_v;
  dp[H] = pgx::TrainerValueGrad(o.value_weight, o.scale_v, v, ret, o.nf);
  stat[1] = pgx::TrainerValueLoss(o.value_weight, v, ret);
}
// `legal`: the row's words of a masked head (actor::LegalBit); null: a discrete head, every j.
inline void PpoDiscreteRow(const int32_t* p, int H, int action, float logp, float adv, float ret, unsigned char mask,
                           const PpoOptions& o, float* dp, float* stat, const uint32_t* legal = nullptr) {
  for (int j = 0; j <= H; ++j) dp[j] = 0.0f;
  for (int j = 0; j < 5; ++j) stat[j] = 0.0f;
  if (mask == 0) return;
  auto in = [legal](int j) { return legal == nullptr || actor::LegalBit(legal, j); };
  float top = -FLT_MAX;
  for (int j = 0; j < H; ++j) {
    const float l = pgx::NetLogit(p[j], o.scale_p);
    if (in(j)) top = l > top ? l : top;
  }
  float S = 0.0f;
  for (int j = 0; j < H; ++j) {
    if (in(j)) S = S + pgx::GumbelExp(pgx::NetLogit(p[j], o.scale_p) - top);
  }
  const float log_s = pgx::GumbelLog(S);
  float sum = 0.0f;
  for (int j = 0; j < H; ++j) {
    const float x = pgx::NetLogit(p[j], o.scale_p) - top;
    if (in(j)) sum = sum + (pgx::GumbelExp(x) / S) * (x - log_s);
  }
  const float Hn = -sum;
  const PpoRatioOut r = PpoRatio((pgx::NetLogit(p[action], o.scale_p) - top) - log_s, logp, adv, o);
  for (int j = 0; j < H; ++j) {
    const float x = pgx::NetLogit(p[j], o.scale_p) - top;
    if (in(j)) dp[j] = PpoDiscreteGrad(o, r.g, j == action, pgx::GumbelExp(x) / S, x - log_s, Hn);
  }
  stat[0] = r.loss, stat[2] = Hn, stat[3] = r.kl, stat[4] = (float)r.clipped;
  PpoValuePart(p, H, ret, o, dp, stat);
}
inline void PpoBoxRow(const int32_t* p, int H, const float* action, const float* sigma, float logp, float adv, float ret,
                      unsigned char mask, const PpoOptions& o, float* dp, float* stat, float* dsigma) {
  for (int j = 0; j <= H; ++j) dp[j] = 0.0f;
  for (int j = 0; j < H; ++j) dsigma[j] = 0.0f;
  for (int j = 0; j < 5; ++j) stat[j] = 0.0f;
  if (mask == 0) return;
  float lp = 0.0f, Hn = 0.0f;
  for (int j = 0; j < H; ++j) {
    const float log_sigma = pgx::GumbelLog(sigma[j]);
    lp = lp + PpoBoxTerm(PpoBoxZ(action[j], pgx::NetLogit(p[j], o.scale_p), sigma[j]), log_sigma);
    Hn = Hn + PpoBoxEntropyTerm(log_sigma);
  }
  const PpoRatioOut r = PpoRatio(lp, logp, adv, o);
  for (int j = 0; j < H; ++j) {
    const float z = PpoBoxZ(action[j], pgx::NetLogit(p[j], o.scale_p), sigma[j]);
    dp[j] = PpoBoxGrad(o, r.g, z, sigma[j]);
    dsigma[j] = PpoSigmaGrad(o, r.g, z, sigma[j]);
  }
  stat[0] = r.loss, stat[2] = Hn, stat[3] = r.kl, stat[4] = (float)r.clipped;
  PpoValuePart(p, H, ret, o, dp, stat);
}

}  // namespace ppo
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PPO_TRAINER_HIP_H_
