// PPO trainer of the rollout actor: what a PPO step does around the trunk's forward and backward, and what a `fit` of
// a collected horizon does around its steps (ppo_trainer.hip.h is the contract; DESIGN.md section 2 "Rollout actor: PPO
// trainer").  Seven kernels and the handle that owns their memory; forward, backward, norm and update are the trunk's
// and the PGX trainer's kernels as they are (NetTrain, TrainerNormLaunch, TrainerUpdateLaunch).
//
// How the work is split.
// PpoAdvStats: a block per 1024 advantages, one 16-byte load of adv and one 4-byte load of the mask per thread, the
//   contract's tree in LDS, one (count, sum, sum of squares) partial per block; PpoAdvTail, one block, adds the partials
//   in block order (three waves, a column each) and writes count, mean and std.  Once per fit.
// PpoGather: a wave per minibatch row.  Lane 0 walks the Feistel cycle for the row's position and hands the horizon
//   index round by a shuffle; the wave then featurises the row's obs keys straight out of slot t of the collector's
//   buffers into the F contiguous bytes the forward reads, consecutive lanes taking consecutive components, converts
//   the action row, and lanes 0 .. 3 move logp, the (normalised) advantage, ret and the mask.  No copy of the
//   observations exists in between.  For a masked head the wave also ballots the row's legal word out of slot t of the
//   mask's obs key (actor.hip.h: LegalBallot; no copy of the mask exists either) and lane 4 folds the stored C
//   components into the flat index.
// PpoLoss<masked> is PpoLoss<discrete> with the rows' legal words in LDS beside p: lanes skip illegal j, and the
//   single-lane walks of S and of the entropy skip them by testing the bit; dp of an illegal j leaves as 0.0f.  Three
//   instantiations in all.
// PpoLoss<box>: a block of 256 threads takes kPpoLossRows = 32 rows, eight lanes a row; p, the Box action rows and
//   the per-row inputs enter LDS as flat 16-byte copies.  The order-free work is spread over a row's eight lanes
//   (j = lane, lane + 8, ..): logits, their maximum by three xor shuffles, exponentials, q, z, the terms and the
//   gradients.  Every ordered sum is walked in ascending j by ONE lane over the values in LDS.  Box: lane 0 walks logp'
//   and lane 1 the entropy at the same time.  Discrete: S, then the entropy, one after the other by lane 0 -- the
//   entropy's terms need q = e / S, so the two walks cannot overlap as the Box head's do (changed from the starting
//   design).  Lane 0 forms the ratio and g, shuffles hand them round; dp leaves LDS as one flat 16-byte copy.  Box:
//   GumbelLog(sigma_j) is taken once per block, the rows' dsigma go through LDS and thread j < H adds the block's rows
//   in row order in double.  Thread 0 adds the block's five statistic sums and the unmasked rows in double.  Two
//   instantiations, no run-time branch on the head.
// PpoSigmaSum: one block; thread j < H adds the loss blocks' dsigma partials in block order into the sigma segment of
//   the gradient table, before the norm reads it (split off the tail, as the starting design allows).
// PpoTail: one block of eight waves; waves 0 .. 5 add a column of the loss partials each, wave 6 the norm partials,
//   thread 0 writes the statistics row and the clip scale.
// PpoSigmaUpdate: one block; thread j < H applies TrainerUpdateOne to the sigma master and writes the floored float32
//   sigma the next loss reads.
// Stream order of a step: (gather,) forward, loss, backward, sigma sum, norm, tail, update, sigma update.  All launches
// of a call are enqueued from one C++ function on the caller's stream; nothing waits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine.h"
#include "ppo_trainer.hip.h"

namespace epa {
namespace {

constexpr int kRows = ppo::kPpoLossRows, kGroup = 8;
constexpr int kChunk = pgx::kTrainerChunk;
constexpr int kWide = 128;  // an LDS row: H + 1 <= 128
static_assert(kRows * kGroup == 256 && pgx::kNetMaxActions + 1 <= kWide, "the block shapes of the contract");

// A flat copy of `bytes` bytes by `n` threads from `t` on: 16 bytes a turn where both addresses allow, the rest in
// 4-byte or single-byte turns.
__device__ inline void FlatCopy(void* dst, const void* src, size_t bytes, int t, int n) {
  const uintptr_t both = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src);
  size_t done = 0;
  if ((both & 15) == 0) {
    const size_t q = bytes / 16;
    for (size_t i = t; i < q; i += n) static_cast<uint4*>(dst)[i] = static_cast<const uint4*>(src)[i];
    done = q * 16;
  }
  if ((both & 3) == 0) {
    const size_t q = (bytes - done) / 4;
    uint32_t* d = reinterpret_cast<uint32_t*>(static_cast<char*>(dst) + done);
    const uint32_t* s = reinterpret_cast<const uint32_t*>(static_cast<const char*>(src) + done);
    for (size_t i = t; i < q; i += n) d[i] = s[i];
    done += q * 4;
  }
  for (size_t i = done + t; i < bytes; i += n) static_cast<char*>(dst)[i] = static_cast<const char*>(src)[i];
}

// ---------------------------------------------------------------------------
// PpoAdvStats, PpoAdvTail
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void PpoAdvStats(const float* __restrict__ adv, const unsigned char* __restrict__ mask,
                                                   uint32_t n, double* __restrict__ partial) {
  __shared__ double s[3][256];
  const int t = threadIdx.x;
  const uint32_t at = blockIdx.x * (uint32_t)ppo::kPpoAdvChunk + 4u * (uint32_t)t;
  ppo::AdvSums a{0.0, 0.0, 0.0};
  if (at + 3 < n && (reinterpret_cast<uintptr_t>(mask) & 3) == 0) {
    const float4 x = *reinterpret_cast<const float4*>(adv + at);
    const uchar4 m = *reinterpret_cast<const uchar4*>(mask + at);
    ppo::AdvAdd(&a, x.x, m.x), ppo::AdvAdd(&a, x.y, m.y), ppo::AdvAdd(&a, x.z, m.z), ppo::AdvAdd(&a, x.w, m.w);
  } else {
    for (uint32_t q = 0; q < 4; ++q) {
      if (at + q < n) ppo::AdvAdd(&a, adv[at + q], mask[at + q]);
    }
  }
  s[0][t] = a.cnt, s[1][t] = a.s1, s[2][t] = a.s2;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) s[0][t] = s[0][t] + s[0][t + w], s[1][t] = s[1][t] + s[1][t + w], s[2][t] = s[2][t] + s[2][t + w];
    __syncthreads();
  }
  if (t < 3) partial[3 * (size_t)blockIdx.x + t] = s[t][0];
}

__global__ __launch_bounds__(192) void PpoAdvTail(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
  __shared__ double s[3];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    double x = 0.0;
    for (int i = 0; i < blocks; ++i) x = x + partial[3 * (size_t)i + wave];
    s[wave] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double mean, std;
    ppo::AdvMoments(ppo::AdvSums{s[0], s[1], s[2]}, &mean, &std);
    out[0] = s[0], out[1] = mean, out[2] = std;
  }
}

// ---------------------------------------------------------------------------
// PpoGather
// ---------------------------------------------------------------------------
struct GatherArgs {
  int rows, F, H, box, normalize, action_dtype;
  uint32_t epoch, first, n;  // the epoch, the step's first position, T N
  uint64_t seed;
  actor::FeatureKeys keys;  // src: slot 0 of a key's buffer
  const double* lo;
  const double* scale;
  const char* action;
  const float* logp;
  const float* adv;
  const float* ret;
  const unsigned char* mask;
  const double* adv_stats;  // count, mean, std
  unsigned char* out_features;
  void* out_action;
  float* out_logp;
  float* out_adv;
  float* out_ret;
  unsigned char* out_mask;
  // a masked head: the stored action row is C int32 components of the flat index; the mask is slot 0 of its obs key
  // (null: none), rows of mask_elems elements, from element mask_first on
  int masked, C, nvec[actor::kMaxComponents], mask_elems, mask_first, mask_dtype;
  const char* mask_src;
  uint4* out_legal;
};

__global__ __launch_bounds__(256) void PpoGather(GatherArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  uint32_t walked = 0;
  if (lane == 0) walked = ppo::PpoPermute(a.seed, a.epoch, a.first + (uint32_t)row, a.n);
  const size_t idx = (size_t)__shfl(walked, 0);  // t N + e: row e of slot t of every buffer
  unsigned char* out = a.out_features + (size_t)row * a.F;
#pragma unroll
  for (int j = 0; j < rollout::kMaxKeys; ++j) {
    if (j >= a.keys.n) break;
    const int elems = a.keys.elems[j], comp0 = a.keys.comp0[j], dtype = a.keys.dtype[j];
    const char* src = a.keys.src[j];
    const size_t first = idx * (size_t)elems;
    for (int c = lane; c < elems; c += 64) {
      out[comp0 + c] = actor::ActorFeature(actor::ActorLoad(src, dtype, first + (size_t)c), a.lo[comp0 + c],
                                           a.scale[comp0 + c]);
    }
  }
  if (a.box) {
    float* act = static_cast<float*>(a.out_action) + (size_t)row * a.H;
    for (int c = lane; c < a.H; c += 64) {
      const size_t at = idx * (size_t)a.H + (size_t)c;
      act[c] = a.action_dtype == actor::kF32 ? reinterpret_cast<const float*>(a.action)[at]
                                             : (float)reinterpret_cast<const double*>(a.action)[at];
    }
  } else if (a.masked) {  // (uniform in the launch: every lane of the wave takes the ballots)
    const uint4 w = actor::LegalBallot(a.mask_src, a.mask_dtype, idx * (size_t)a.mask_elems + (size_t)a.mask_first,
                                       a.H, lane);
    if (lane == 5) a.out_legal[row] = w;
    if (lane == 4) {
      static_cast<int32_t*>(a.out_action)[row] =
          actor::ActorFlat(reinterpret_cast<const int32_t*>(a.action) + idx * (size_t)a.C, a.nvec, a.C);
    }
  } else if (lane == 4) {
    static_cast<int32_t*>(a.out_action)[row] = reinterpret_cast<const int32_t*>(a.action)[idx];
  }
  if (lane == 0) a.out_logp[row] = a.logp[idx];
  if (lane == 1) a.out_adv[row] = a.normalize ? ppo::AdvNormalize(a.adv[idx], a.adv_stats[1], a.adv_stats[2]) : a.adv[idx];
  if (lane == 2) a.out_ret[row] = a.ret[idx];
  if (lane == 3) a.out_mask[row] = a.mask[idx];
}

// ---------------------------------------------------------------------------
// PpoLoss
// ---------------------------------------------------------------------------
struct LossArgs {
  int rows, H;
  ppo::PpoOptions o;
  const int32_t* p;
  const void* action;  // int32 [rows], or float32 [rows][H]
  const float* logp;
  const float* adv;
  const float* ret;
  const unsigned char* mask;  // null: every row counts
  const float* sigma;         // box: [H]
  float* dp;
  double* partial;        // [blocks][kPpoPartials]
  double* sigma_partial;  // box with a trained sigma: [blocks][H]; else null
  const uint4* legal;     // masked: the rows' legal words
};

template <int kHead>  // actor::kDiscrete, kBox, kMasked
__global__ __launch_bounds__(256) void PpoLoss(LossArgs a) {
  constexpr bool kBox = kHead == actor::kBox, kMask = kHead == actor::kMasked;
  __shared__ __attribute__((aligned(16))) uint32_t s_legal[kMask ? kRows : 1][4];  // masked: beside p
  __shared__ __attribute__((aligned(16))) int32_t s_p[kRows * kWide];  // p, then the bits of the logits, then of dp
  __shared__ __attribute__((aligned(16))) float s_x[kRows * kWide];    // discrete: e, then q; box: the action, then z
  __shared__ __attribute__((aligned(16))) float s_t[kRows * kWide];    // the terms of the ordered sum; box: then dsigma
  __shared__ __attribute__((aligned(16))) int32_t s_in[4][kRows];      // action (discrete), logp, adv, ret
  __shared__ __attribute__((aligned(16))) unsigned char s_mask[kRows];
  __shared__ float s_sigma[kWide], s_ls[kWide];
  __shared__ float s_stat[kRows * 5];
  const int H = a.H, t = threadIdx.x;
  const int r0 = blockIdx.x * kRows;
  const int nr = a.rows - r0 < kRows ? a.rows - r0 : kRows;
  FlatCopy(s_p, a.p + (size_t)r0 * (H + 1), (size_t)nr * (H + 1) * 4, t, 256);
  if (kBox) {
    FlatCopy(s_x, static_cast<const float*>(a.action) + (size_t)r0 * H, (size_t)nr * H * 4, t, 256);
    if (t < H) {
      const float sigma = a.sigma[t];
      s_sigma[t] = sigma;
      s_ls[t] = pgx::GumbelLog(sigma);
    }
  } else {
    FlatCopy(s_in[0], static_cast<const int32_t*>(a.action) + r0, (size_t)nr * 4, t, 256);
    if (kMask) FlatCopy(s_legal, a.legal + r0, (size_t)nr * 16, t, 256);
  }
  FlatCopy(s_in[1], a.logp + r0, (size_t)nr * 4, t, 256);
  FlatCopy(s_in[2], a.adv + r0, (size_t)nr * 4, t, 256);
  FlatCopy(s_in[3], a.ret + r0, (size_t)nr * 4, t, 256);
  if (a.mask != nullptr) {
    FlatCopy(s_mask, a.mask + r0, (size_t)nr, t, 256);
  } else if (t < kRows) {
    s_mask[t] = 1;
  }
  __syncthreads();

  const int row = t >> 3, l = t & (kGroup - 1), base = (t & 63) & ~(kGroup - 1);
  const bool live = row < nr && s_mask[row < nr ? row : 0] != 0;  // a masked row computes nothing
  int32_t* p = s_p + row * (H + 1);
  float* x = s_x + row * H;
  float* term = s_t + row * H;
  float top = 0.0f, log_s = 0.0f, Hn = 0.0f, lp = 0.0f;
  int action = 0;
  const uint32_t* legal = s_legal[kMask && row < nr ? row : 0];
  auto in = [legal](int k) { return !kMask || actor::LegalBit(legal, k); };  // (a masked head: lanes skip illegal k)

  if (kBox) {
    if (live) {
      for (int k = l; k < H; k += kGroup) {
        const float z = ppo::PpoBoxZ(x[k], pgx::NetLogit(p[k], a.o.scale_p), s_sigma[k]);
        x[k] = z;
        term[k] = ppo::PpoBoxTerm(z, s_ls[k]);
      }
    }
    __syncthreads();
    // the ordered sums: lane 0 walks logp', lane 1 the entropy
    float sum = 0.0f;
    if (live && l < 2) {
      for (int k = 0; k < H; ++k) sum = sum + (l == 0 ? term[k] : ppo::PpoBoxEntropyTerm(s_ls[k]));
    }
    lp = __shfl(sum, base);
    Hn = __shfl(sum, base + 1);
  } else {
    top = -FLT_MAX;
    if (live) {
      for (int k = l; k < H; k += kGroup) {
        const float logit = pgx::NetLogit(p[k], a.o.scale_p);
        p[k] = pgx::NetFloatBits(logit);
        if (in(k)) top = logit > top ? logit : top;
      }
    }
    for (int w = kGroup / 2; w >= 1; w >>= 1) {
      const float other = __shfl_xor(top, w);
      top = other > top ? other : top;
    }
    if (live) {
      for (int k = l; k < H; k += kGroup) {
        if (in(k)) x[k] = pgx::GumbelExp(pgx::NetBitsFloat(p[k]) - top);
      }
    }
    __syncthreads();
    // the ordered sums, both by lane 0: S, and behind it the entropy over q = e / S
    float sum = 0.0f;
    if (live && l == 0) {
      for (int k = 0; k < H; ++k) {
        if (in(k)) sum = sum + x[k];
      }
    }
    const float S = __shfl(sum, base);
    __syncthreads();
    if (live) {
      log_s = pgx::GumbelLog(S);
      for (int k = l; k < H; k += kGroup) {
        if (!in(k)) continue;
        const float q = x[k] / S;
        x[k] = q;
        term[k] = q * ((pgx::NetBitsFloat(p[k]) - top) - log_s);
      }
    }
    __syncthreads();
    sum = 0.0f;
    if (live && l == 0) {
      for (int k = 0; k < H; ++k) {
        if (in(k)) sum = sum + term[k];
      }
      action = s_in[0][row];
      action = action < 0 ? 0 : (action >= H ? H - 1 : action);  // (LDS stays in bounds whatever the caller sent)
      lp = (pgx::NetBitsFloat(p[action]) - top) - log_s;
    }
    Hn = -__shfl(sum, base);
    action = __shfl(action, base);
  }

  ppo::PpoRatioOut r{0.0f, 0.0f, 0.0f, 0};
  if (live && l == 0) r = ppo::PpoRatio(lp, pgx::NetBitsFloat(s_in[1][row]), pgx::NetBitsFloat(s_in[2][row]), a.o);
  const float g = __shfl(r.g, base);
  __syncthreads();
  if (row < nr) {
    for (int k = l; k < H; k += kGroup) {
      float d = 0.0f;
      if (kBox) {
        if (live) d = ppo::PpoBoxGrad(a.o, g, x[k], s_sigma[k]);
        term[k] = live ? ppo::PpoSigmaGrad(a.o, g, x[k], s_sigma[k]) : 0.0f;
      } else if (live && in(k)) {
        d = ppo::PpoDiscreteGrad(a.o, g, k == action, x[k], (pgx::NetBitsFloat(p[k]) - top) - log_s, Hn);
      }
      p[k] = pgx::NetFloatBits(d);
    }
    if (l == 0) {
      float* stat = s_stat + 5 * row;
      float dv = 0.0f;
      stat[0] = stat[1] = stat[2] = stat[3] = stat[4] = 0.0f;
      if (live) {
        const float v = (float)p[H] * a.o.scale_v, ret = pgx::NetBitsFloat(s_in[3][row]);
        dv = pgx::TrainerValueGrad(a.o.value_weight, a.o.scale_v, v, ret, a.o.nf);
        stat[0] = r.loss, stat[1] = pgx::TrainerValueLoss(a.o.value_weight, v, ret), stat[2] = Hn, stat[3] = r.kl;
        stat[4] = (float)r.clipped;
      }
      p[H] = pgx::NetFloatBits(dv);
    }
  }
  __syncthreads();
  FlatCopy(a.dp + (size_t)r0 * (H + 1), s_p, (size_t)nr * (H + 1) * 4, t, 256);
  if (kBox && a.sigma_partial != nullptr && t < H) {
    double s = 0.0;
    for (int r2 = 0; r2 < nr; ++r2) {
      if (s_mask[r2] != 0) s = s + (double)s_t[r2 * H + t];
    }
    a.sigma_partial[(size_t)blockIdx.x * H + t] = s;
  }
  if (t == 0) {
    double s[ppo::kPpoPartials] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r2 = 0; r2 < nr; ++r2) {
      if (s_mask[r2] == 0) continue;
#pragma unroll
      for (int q = 0; q < 5; ++q) s[q] = s[q] + (double)s_stat[5 * r2 + q];
      s[5] = s[5] + 1.0;
    }
#pragma unroll
    for (int q = 0; q < ppo::kPpoPartials; ++q) a.partial[(size_t)ppo::kPpoPartials * blockIdx.x + q] = s[q];
  }
}

// ---------------------------------------------------------------------------
// PpoSigmaSum, PpoTail, PpoSigmaUpdate
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWide) void PpoSigmaSum(const double* __restrict__ partial, int blocks, int H,
                                                     float* __restrict__ grad) {
  const int t = threadIdx.x;
  if (t >= H) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s = s + partial[(size_t)b * H + t];
  grad[t] = (float)s;
}

struct TailArgs {
  int rows, loss_blocks, chunks;
  double clip;
  const double* loss_partial;
  const double* norm_partial;
  double* stats;       // this step's row
  double* clip_scale;  // [1]
};

__global__ __launch_bounds__(512) void PpoTail(TailArgs a) {
  __shared__ double s[ppo::kPpoPartials + 1];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0 && wave <= ppo::kPpoPartials) {
    double x = 0.0;
    if (wave < ppo::kPpoPartials) {
      for (int i = 0; i < a.loss_blocks; ++i) x = x + a.loss_partial[(size_t)ppo::kPpoPartials * i + wave];
    } else {
      for (int i = 0; i < a.chunks; ++i) x = x + a.norm_partial[i];
    }
    s[wave] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = s[5], norm = sqrt(s[ppo::kPpoPartials]);
    for (int q = 0; q < 5; ++q) a.stats[q] = n > 0.0 ? s[q] / n : 0.0;
    a.stats[5] = norm;
    a.stats[6] = n;
    a.stats[7] = (double)a.rows;
    *a.clip_scale = pgx::TrainerClipScale(a.clip, norm);
  }
}

__global__ __launch_bounds__(kWide) void PpoSigmaUpdate(pgx::TrainerRule rule, int H, const float* __restrict__ grad,
                                                        const double* __restrict__ clip_scale, double* master, double* s1,
                                                        double* s2, float* __restrict__ sigma) {
  const int t = threadIdx.x;
  if (t >= H) return;
  double m = master[t], a = s1[t], b = s2[t];
  pgx::TrainerUpdateOne(rule, grad[t], *clip_scale, &m, &a, &b);
  master[t] = m, s1[t] = a, s2[t] = b;
  sigma[t] = ppo::PpoSigmaOf(m);
}

size_t Align256(size_t n) { return (n + 255) & ~(size_t)255; }

void CheckOption(const char* name, double v) {
  if (!(v >= 0.0) || !std::isfinite(v)) {
    throw std::invalid_argument(std::string("ppo_create: ") + name + " = " + std::to_string(v) +
                                " must be finite and not negative");
  }
}

// the launches of a block of code on the handle's device, the caller's device current again behind them
template <class F>
void OnDevice(int device, F launch) {
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device));
  launch();
  const hipError_t launched = hipGetLastError();
  (void)hipSetDevice(before);
  EPA_HIP(launched);
}

}  // namespace

// ---------------------------------------------------------------------------
// the handle (engine.h: PpoTrainer)
// ---------------------------------------------------------------------------
struct PpoTrainer::Layout {
  int arrays{0};  // the net's parameter arrays, plus one for a trained sigma
  size_t count[2 * kNetImageLayers + 1]{}, eoff[2 * kNetImageLayers + 1]{};  // elements and the flat offset of an array
  size_t net_elems{0}, elems{0}, weight_elems{0};                            // of the flat space, all whole chunks
  // byte offsets into the block
  size_t grad, master, s1, s2, q_weight, q_bias, sigma, lo, scale, dp, p, features, action, logp, adv, ret, mask, legal,
      loss_partial, sigma_partial, norm_partial, clip, adv_stats, stats, total;
  // and into the horizon's
  size_t h_adv, h_ret, h_partial;
};

PpoTrainer::PpoTrainer(int device, const void* blob, size_t bytes, const PpoTrainerOptions& o, long long max_rows)
    : device_(device), max_rows_((int)max_rows), opt_(o), at_(new Layout()) {
  const TrainerOptions& b = o.base;
  if (b.optimizer != pgx::kTrainerSgd && b.optimizer != pgx::kTrainerAdam) {
    throw std::invalid_argument("ppo_create: optimizer = " + std::to_string(b.optimizer) + " must be 0 (sgd) or 1 (adam)");
  }
  CheckOption("lr", b.lr), CheckOption("momentum", b.momentum), CheckOption("beta1", b.beta1);
  CheckOption("beta2", b.beta2), CheckOption("eps", b.eps), CheckOption("weight_decay", b.weight_decay);
  CheckOption("value_weight", b.value_weight), CheckOption("clip", b.clip);
  CheckOption("clip_ratio", o.clip_ratio), CheckOption("entropy_weight", o.entropy_weight);
  if (max_rows < 1 || max_rows > (1 << 22)) {
    throw std::invalid_argument("ppo_create: max_rows = " + std::to_string(max_rows) + " must be 1 .. 2^22");
  }
  char err[240];
  actor::ActorView v;
  if (!actor::ActorParse(blob, bytes, &v, err, sizeof(err))) throw std::invalid_argument(err);
  Layout& at = *at_;
  layers_ = v.net.layers(), F_ = v.F, H_ = v.H, kind_ = v.kind, scale_p_ = v.scale_p, scale_v_ = v.scale_v;
  sigma_ = kind_ == actor::kBox && o.train_sigma != 0;
  mask0_ = v.mask0, C_ = v.C;
  std::memcpy(nvec_, v.nvec, sizeof(nvec_));
  for (int i = 0; i < layers_; ++i) {
    const pgx::NetLayer& l = v.net.layer[i];
    at.count[i] = (size_t)l.n_out * l.k_in, at.count[layers_ + i] = (size_t)l.n_out;
    shift_[i] = l.shift;
  }
  net_.reset(new NetTrain(device, v.F, v.H, v.D, v.L, max_rows));
  at.arrays = 2 * layers_;
  for (int s = 0; s < at.arrays; ++s) {
    at.eoff[s] = at.elems;
    at.elems += (at.count[s] + kChunk - 1) / kChunk * kChunk;
    if (s == layers_ - 1) at.weight_elems = at.elems;
  }
  at.net_elems = at.elems;
  if (sigma_) {  // one more segment behind the biases
    at.eoff[at.arrays] = at.elems, at.count[at.arrays] = (size_t)H_;
    at.elems += kChunk, at.arrays += 1;
  }
  const size_t rows = (size_t)max_rows_, E = at.elems, H1 = (size_t)H_ + 1, blocks = (rows + kRows - 1) / kRows;
  size_t end = 0;
  auto take = [&](size_t n) {
    const size_t here = end;
    end += Align256(n);
    return here;
  };
  at.grad = take(4 * E), at.master = take(8 * E), at.s1 = take(8 * E), at.s2 = take(8 * E);
  at.q_weight = take(at.weight_elems), at.q_bias = take(4 * (at.net_elems - at.weight_elems));
  at.sigma = take(4 * kWide), at.lo = take(8 * (size_t)F_), at.scale = take(8 * (size_t)F_);
  at.dp = take(rows * H1 * 4), at.p = take(rows * H1 * 4);
  at.features = take(rows * F_), at.action = take(rows * (size_t)H_ * 4);
  at.logp = take(rows * 4), at.adv = take(rows * 4), at.ret = take(rows * 4), at.mask = take(rows);
  at.legal = take(kind_ == actor::kMasked ? rows * 16 : 0);
  at.loss_partial = take(blocks * ppo::kPpoPartials * 8), at.sigma_partial = take(blocks * (size_t)H_ * 8);
  at.norm_partial = take(E / kChunk * 8), at.clip = take(8), at.adv_stats = take(24);
  at.stats = take((size_t)pgx::kTrainerStatRows * ppo::kPpoStats * 8);
  at.total = end;

  // the start: masters = the blob's integers and sigma, their quantised arrays, everything else zero
  std::vector<double> master(E, 0.0);
  std::vector<signed char> qw(at.weight_elems, 0);
  std::vector<int32_t> qb(at.net_elems - at.weight_elems, 0);
  std::vector<float> sigma(kWide, 1.0f);
  for (int i = 0; i < layers_; ++i) {
    const pgx::NetLayer& l = v.net.layer[i];
    for (size_t k = 0; k < at.count[i]; ++k) master[at.eoff[i] + k] = (double)(qw[at.eoff[i] + k] = l.w[k]);
    const size_t bo = at.eoff[layers_ + i];
    for (size_t k = 0; k < at.count[layers_ + i]; ++k) master[bo + k] = (double)(qb[bo - at.weight_elems + k] = l.b[k]);
  }
  for (size_t j = 0; j < v.sigma.size(); ++j) {
    sigma[j] = v.sigma[j];
    if (sigma_) sigma[j] = ppo::PpoSigmaOf(master[at.net_elems + j] = (double)v.sigma[j]);
  }
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  try {
    mem_.Alloc(at.total);
    EPA_HIP(hipMemset(mem_.p, 0, at.total));
    EPA_HIP(hipMemcpy(mem_.p + at.master, master.data(), 8 * E, hipMemcpyHostToDevice));
    EPA_HIP(hipMemcpy(mem_.p + at.q_weight, qw.data(), qw.size(), hipMemcpyHostToDevice));
    EPA_HIP(hipMemcpy(mem_.p + at.q_bias, qb.data(), 4 * qb.size(), hipMemcpyHostToDevice));
    EPA_HIP(hipMemcpy(mem_.p + at.sigma, sigma.data(), 4 * sigma.size(), hipMemcpyHostToDevice));
    EPA_HIP(hipMemcpy(mem_.p + at.lo, v.lo.data(), 8 * (size_t)F_, hipMemcpyHostToDevice));
    EPA_HIP(hipMemcpy(mem_.p + at.scale, v.scale.data(), 8 * (size_t)F_, hipMemcpyHostToDevice));
    EPA_HIP(hipDeviceSynchronize());
  } catch (...) {
    (void)hipSetDevice(before);
    throw;
  }
  EPA_HIP(hipSetDevice(before));
}

PpoTrainer::~PpoTrainer() {
  int before = 0;
  if (hipGetDevice(&before) != hipSuccess) return;
  (void)hipSetDevice(device_);
  mem_.Free(), horizon_.Free();
  net_.reset();
  (void)hipSetDevice(before);
}

void PpoTrainer::Enqueue(hipStream_t stream, int rows, const unsigned char* features, const void* action,
                         const float* logp, const float* adv, const float* ret, const unsigned char* mask,
                         const void* legal) {
  const Layout& at = *at_;
  char* m = mem_.p;
  const void* qw[kNetImageLayers];
  const void* qb[kNetImageLayers];
  void* dw[kNetImageLayers];
  void* db[kNetImageLayers];
  float* grad = reinterpret_cast<float*>(m + at.grad);
  for (int i = 0; i < layers_; ++i) {
    qw[i] = m + at.q_weight + at.eoff[i];
    qb[i] = m + at.q_bias + 4 * (at.eoff[layers_ + i] - at.weight_elems);
    dw[i] = grad + at.eoff[i];
    db[i] = grad + at.eoff[layers_ + i];
  }
  int32_t* p = reinterpret_cast<int32_t*>(m + at.p);
  float* dp = reinterpret_cast<float*>(m + at.dp);
  net_->Forward(stream, rows, qw, qb, shift_, features, p);
  const int loss_blocks = (rows + kRows - 1) / kRows, chunks = (int)(at.elems / kChunk);
  const int net_chunks = (int)(at.net_elems / kChunk);
  double* loss_partial = reinterpret_cast<double*>(m + at.loss_partial);
  double* sigma_partial = reinterpret_cast<double*>(m + at.sigma_partial);
  double* norm_partial = reinterpret_cast<double*>(m + at.norm_partial);
  double* clip_scale = reinterpret_cast<double*>(m + at.clip);
  float* sigma = reinterpret_cast<float*>(m + at.sigma);
  const bool box = kind_ == actor::kBox;
  const LossArgs loss{rows, H_,
                      ppo::PpoOptionsOf(scale_p_, scale_v_, (float)opt_.clip_ratio, (float)opt_.base.value_weight,
                                        (float)opt_.entropy_weight, rows),
                      p, action, logp, adv, ret, mask, sigma, dp, loss_partial, sigma_ ? sigma_partial : nullptr,
                      static_cast<const uint4*>(legal)};
  OnDevice(device_, [&] {
    if (box) {
      hipLaunchKernelGGL(PpoLoss<actor::kBox>, dim3(loss_blocks), dim3(256), 0, stream, loss);
    } else if (kind_ == actor::kMasked) {
      hipLaunchKernelGGL(PpoLoss<actor::kMasked>, dim3(loss_blocks), dim3(256), 0, stream, loss);
    } else {
      hipLaunchKernelGGL(PpoLoss<actor::kDiscrete>, dim3(loss_blocks), dim3(256), 0, stream, loss);
    }
  });
  net_->Backward(stream, rows, dp, dw, db);
  // the step's constants, in the host's doubles
  const TrainerOptions& o = opt_.base;
  beta1_pow_ *= o.beta1, beta2_pow_ *= o.beta2;
  pgx::TrainerRule rule{};
  rule.optimizer = o.optimizer, rule.lr = o.lr, rule.momentum = o.momentum;
  rule.beta1 = o.beta1, rule.beta2 = o.beta2, rule.eps = o.eps, rule.weight_decay = o.weight_decay;
  rule.one_minus_beta1 = 1.0 - o.beta1, rule.one_minus_beta2 = 1.0 - o.beta2;
  rule.lr_t = o.optimizer == pgx::kTrainerAdam ? o.lr * std::sqrt(1.0 - beta2_pow_) / (1.0 - beta1_pow_) : 0.0;
  double* stats = reinterpret_cast<double*>(m + at.stats) + ppo::kPpoStats * (size_t)(steps_ % pgx::kTrainerStatRows);
  const TailArgs tail{rows, loss_blocks, chunks, o.clip, loss_partial, norm_partial, stats, clip_scale};
  double* master = reinterpret_cast<double*>(m + at.master);
  double* s1 = reinterpret_cast<double*>(m + at.s1);
  double* s2 = reinterpret_cast<double*>(m + at.s2);
  const size_t so = at.net_elems;  // the sigma segment
  OnDevice(device_, [&] {
    if (sigma_) hipLaunchKernelGGL(PpoSigmaSum, dim3(1), dim3(kWide), 0, stream, sigma_partial, loss_blocks, H_, grad + so);
    TrainerNormLaunch(grad, chunks, norm_partial, stream);
    hipLaunchKernelGGL(PpoTail, dim3(1), dim3(512), 0, stream, tail);
    TrainerUpdateLaunch(rule, net_chunks, (int)(at.weight_elems / kChunk), grad, master, s1, s2, clip_scale,
                        reinterpret_cast<signed char*>(m + at.q_weight), reinterpret_cast<int32_t*>(m + at.q_bias),
                        stream);
    if (sigma_) {
      hipLaunchKernelGGL(PpoSigmaUpdate, dim3(1), dim3(kWide), 0, stream, rule, H_, grad + so, clip_scale, master + so,
                         s1 + so, s2 + so, sigma);
    }
  });
  ++steps_, rows_ = rows, last_ = stream;
}

void PpoTrainer::Step(hipStream_t stream, int rows, const void* d_features, const void* d_action, const void* d_logp,
                      const void* d_adv, const void* d_ret, const void* d_mask, const void* d_legal) {
  if (d_features == nullptr || d_action == nullptr || d_logp == nullptr || d_adv == nullptr || d_ret == nullptr) {
    throw std::invalid_argument("ppo_step: null argument");
  }
  if ((kind_ == actor::kMasked) != (d_legal != nullptr)) {
    throw std::invalid_argument("ppo_step: a masked actor (kind 2), and no other, takes the rows' legal words "
                                "(epa_ppo_step_legal_device)");
  }
  if (d_legal != nullptr && reinterpret_cast<uintptr_t>(d_legal) % 16 != 0) {
    throw std::invalid_argument("ppo_step: the legal words must be 16-byte aligned");
  }
  if (rows < 1 || rows > max_rows_) {
    throw std::invalid_argument("ppo_step: rows = " + std::to_string(rows) + " must be 1 .. " +
                                std::to_string(max_rows_) + " (the handle's max_rows)");
  }
  Enqueue(stream, rows, static_cast<const unsigned char*>(d_features), d_action, static_cast<const float*>(d_logp),
          static_cast<const float*>(d_adv), static_cast<const float*>(d_ret), static_cast<const unsigned char*>(d_mask),
          d_legal);
}

void PpoTrainer::Horizon(const PpoSource& src, int batch, int epochs, float** adv, float** ret) {
  if (adv == nullptr || ret == nullptr || src.action == nullptr || src.mask == nullptr || src.logp == nullptr) {
    throw std::invalid_argument("ppo_fit: null argument");
  }
  if (src.horizon < 1 || src.envs < 1 || (long long)src.horizon * src.envs >= (1ll << 31)) {
    throw std::invalid_argument("ppo_fit: a horizon of " + std::to_string(src.horizon) + " steps of " +
                                std::to_string(src.envs) + " envs; T N must be 1 .. 2^31 - 1");
  }
  const long long TN = (long long)src.horizon * src.envs;
  if (batch < 1 || batch > max_rows_ || batch > TN) {
    throw std::invalid_argument("ppo_fit: batch = " + std::to_string(batch) + " must be 1 .. min(T N = " +
                                std::to_string(TN) + ", max_rows = " + std::to_string(max_rows_) + ")");
  }
  if (epochs < 1) throw std::invalid_argument("ppo_fit: epochs = " + std::to_string(epochs) + " must be at least 1");
  long long F = 0;
  if (src.n_obs < 1 || src.n_obs >= rollout::kMaxKeys) throw std::invalid_argument("ppo_fit: n_obs must be 1 .. 7");
  for (int j = 0; j < src.n_obs; ++j) {
    if (src.obs[j] == nullptr || src.obs_elems[j] < 1 || src.obs_dtype[j] < actor::kI32 || src.obs_dtype[j] > actor::kU8) {
      throw std::invalid_argument("ppo_fit: obs key " + std::to_string(j) + " is null, empty or of an unknown dtype");
    }
    F += src.obs_elems[j];
  }
  const bool box = kind_ == actor::kBox;
  bool fits = box ? (src.action_dtype == actor::kF32 || src.action_dtype == actor::kF64) && src.action_elems == H_
                  : src.action_dtype == actor::kI32 && src.action_elems == (kind_ == actor::kMasked ? C_ : 1);
  if (kind_ == actor::kMasked && mask0_ >= 0 && F == F_) {  // the mask lies inside one obs key
    bool inside = false;
    int comp = 0;
    for (int j = 0; j < src.n_obs; ++j) {
      inside = inside || (mask0_ >= comp && mask0_ + H_ <= comp + src.obs_elems[j]);
      comp += src.obs_elems[j];
    }
    fits = fits && inside;
  }
  if (F != F_ || !fits) {
    throw std::invalid_argument("ppo_fit: the collector has F = " + std::to_string(F) + " and action rows of " +
                                std::to_string(src.action_elems) + " of dtype " + std::to_string(src.action_dtype) +
                                "; the trainer's actor has F = " + std::to_string(F_) + ", H = " + std::to_string(H_) +
                                ", kind = " + std::to_string(kind_));
  }
  Layout& at = *at_;
  if ((size_t)TN != horizon_rows_) {
    at.h_adv = 0, at.h_ret = Align256(4 * (size_t)TN);
    at.h_partial = at.h_ret + Align256(4 * (size_t)TN);
    const size_t blocks = ((size_t)TN + ppo::kPpoAdvChunk - 1) / ppo::kPpoAdvChunk;
    int before = 0;
    EPA_HIP(hipGetDevice(&before));
    EPA_HIP(hipSetDevice(device_));
    try {
      horizon_.Alloc(at.h_partial + Align256(24 * blocks));
    } catch (...) {
      (void)hipSetDevice(before);
      horizon_rows_ = 0;
      throw;
    }
    (void)hipSetDevice(before);
    horizon_rows_ = (size_t)TN;
  }
  *adv = reinterpret_cast<float*>(horizon_.p + at.h_adv);
  *ret = reinterpret_cast<float*>(horizon_.p + at.h_ret);
}

void PpoTrainer::Fit(hipStream_t stream, const PpoSource& src, int batch, int epochs) {
  const Layout& at = *at_;
  char* m = mem_.p;
  const uint32_t TN = (uint32_t)horizon_rows_;
  if (horizon_rows_ == 0 || (long long)src.horizon * src.envs != (long long)horizon_rows_) {
    throw std::invalid_argument("ppo_fit: the horizon's buffers are not of this collector's shape");
  }
  const float* adv = reinterpret_cast<const float*>(horizon_.p + at.h_adv);
  double* adv_partial = reinterpret_cast<double*>(horizon_.p + at.h_partial);
  double* adv_stats = reinterpret_cast<double*>(m + at.adv_stats);
  const int adv_blocks = (int)((TN + ppo::kPpoAdvChunk - 1) / ppo::kPpoAdvChunk);
  if (opt_.normalize_adv != 0) {
    OnDevice(device_, [&] {
      hipLaunchKernelGGL(PpoAdvStats, dim3(adv_blocks), dim3(256), 0, stream, adv, src.mask, TN, adv_partial);
      hipLaunchKernelGGL(PpoAdvTail, dim3(1), dim3(192), 0, stream, adv_partial, adv_blocks, adv_stats);
    });
  }
  GatherArgs g{};
  g.rows = batch, g.F = F_, g.H = H_, g.box = kind_ == actor::kBox ? 1 : 0, g.normalize = opt_.normalize_adv != 0 ? 1 : 0;
  g.action_dtype = src.action_dtype, g.n = TN, g.seed = opt_.base.seed;
  g.keys.n = src.n_obs, g.keys.F = F_;
  int comp = 0;
  for (int j = 0; j < src.n_obs; ++j) {
    g.keys.src[j] = static_cast<const char*>(src.obs[j]);
    g.keys.elems[j] = src.obs_elems[j], g.keys.dtype[j] = src.obs_dtype[j], g.keys.comp0[j] = comp;
    if (kind_ == actor::kMasked && mask0_ >= comp && mask0_ + H_ <= comp + src.obs_elems[j]) {
      g.mask_src = g.keys.src[j], g.mask_elems = src.obs_elems[j], g.mask_dtype = src.obs_dtype[j];
      g.mask_first = mask0_ - comp;
    }
    comp += src.obs_elems[j];
  }
  if (kind_ == actor::kMasked) {
    if (mask0_ >= 0 && g.mask_src == nullptr) throw std::invalid_argument("ppo_fit: the mask does not lie inside one obs key");
    if (src.action_elems != C_) throw std::invalid_argument("ppo_fit: the action rows are not the actor's components");
    g.masked = 1, g.C = C_;
    std::memcpy(g.nvec, nvec_, sizeof(g.nvec));
    g.out_legal = reinterpret_cast<uint4*>(m + at.legal);
  }
  g.lo = reinterpret_cast<const double*>(m + at.lo), g.scale = reinterpret_cast<const double*>(m + at.scale);
  g.action = static_cast<const char*>(src.action), g.logp = src.logp, g.adv = adv;
  g.ret = reinterpret_cast<const float*>(horizon_.p + at.h_ret), g.mask = src.mask, g.adv_stats = adv_stats;
  g.out_features = reinterpret_cast<unsigned char*>(m + at.features), g.out_action = m + at.action;
  g.out_logp = reinterpret_cast<float*>(m + at.logp), g.out_adv = reinterpret_cast<float*>(m + at.adv);
  g.out_ret = reinterpret_cast<float*>(m + at.ret), g.out_mask = reinterpret_cast<unsigned char*>(m + at.mask);
  const int steps = (int)(TN / (uint32_t)batch);
  for (int e = 0; e < epochs; ++e) {
    g.epoch = (uint32_t)epochs_;
    for (int s = 0; s < steps; ++s) {
      g.first = (uint32_t)s * (uint32_t)batch;
      OnDevice(device_, [&] { hipLaunchKernelGGL(PpoGather, dim3((batch + 3) / 4), dim3(256), 0, stream, g); });
      Enqueue(stream, batch, g.out_features, g.out_action, g.out_logp, g.out_adv, g.out_ret, g.out_mask, g.out_legal);
    }
    ++epochs_;
  }
}

void PpoTrainer::Read(int what, int layer, void* out) {
  const Layout& at = *at_;
  size_t from = 0, bytes = 0;
  const bool array = what >= 0 && what <= 4;
  if ((array || what == 8) && (layer < 0 || layer >= at.arrays)) {
    throw std::invalid_argument("ppo_read: layer = " + std::to_string(layer) + " must be 0 .. " +
                                std::to_string(at.arrays - 1));
  }
  if (what == 8) {
    const int64_t info[4] = {at.arrays, steps_, rows_, (int64_t)at.count[layer]};
    std::memcpy(out, info, sizeof(info));
    return;
  }
  const size_t n = (size_t)rows_;
  if (array) {
    const size_t e = at.eoff[layer], c = at.count[layer];
    const bool weight = layer < layers_, sigma = layer == 2 * layers_;
    if (what <= 2) {
      from = (what == 0 ? at.master : (what == 1 ? at.s1 : at.s2)) + 8 * e, bytes = 8 * c;
    } else if (what == 3) {
      from = sigma ? at.sigma : (weight ? at.q_weight + e : at.q_bias + 4 * (e - at.weight_elems));
      bytes = weight ? c : 4 * c;
    } else {
      from = at.grad + 4 * e, bytes = 4 * c;
    }
  } else if (what == 5 || what == 6) {
    from = what == 5 ? at.dp : at.p, bytes = n * (H_ + 1) * 4;
  } else if (what == 7) {
    if (layer < 0 || layer > pgx::kTrainerStatRows || layer > steps_) {
      throw std::invalid_argument("ppo_read: " + std::to_string(layer) + " statistics rows; there are " +
                                  std::to_string(steps_ < pgx::kTrainerStatRows ? steps_ : pgx::kTrainerStatRows));
    }
  } else if (what == 9) {
    const size_t action_bytes = kind_ == actor::kBox ? n * (size_t)H_ * 4 : n * 4;
    const size_t offs[8] = {at.features, at.action, at.logp, at.adv, at.ret, at.mask, at.adv_stats, at.legal};
    const size_t sizes[8] = {n * (size_t)F_, action_bytes, 4 * n, 4 * n, 4 * n, n, 24, 16 * n};
    if (layer < 0 || layer > (kind_ == actor::kMasked ? 7 : 6)) {
      throw std::invalid_argument("ppo_read: a minibatch has parts 0 .. 6, and 7 (the legal words) for a masked actor");
    }
    from = offs[layer], bytes = sizes[layer];
  } else {
    throw std::invalid_argument("ppo_read: what = " + std::to_string(what) + " must be 0 .. 9");
  }
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  hipError_t e = hipStreamSynchronize(last_);
  const size_t row_bytes = ppo::kPpoStats * 8;
  if (e == hipSuccess && what == 7) {
    for (int i = 0; i < layer && e == hipSuccess; ++i) {  // (the ring: row by row)
      const size_t slot = (size_t)((steps_ - layer + i) % pgx::kTrainerStatRows);
      e = hipMemcpy(static_cast<char*>(out) + row_bytes * (size_t)i, mem_.p + at.stats + row_bytes * slot, row_bytes,
                    hipMemcpyDeviceToHost);
    }
  } else if (e == hipSuccess && bytes != 0) {
    e = hipMemcpy(out, mem_.p + from, bytes, hipMemcpyDeviceToHost);
  }
  (void)hipSetDevice(before);
  EPA_HIP(e);
}

}  // namespace epa
