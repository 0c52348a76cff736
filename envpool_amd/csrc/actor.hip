// Rollout actor kernels (actor.hip.h is the contract; DESIGN.md section 2 "Rollout actor and collect").  Family
// independent: they read observation rows where the collector (or a caller) keeps them, never an env's state.  The
// trunk between the two is PgxNetEval<false, true> (pgx_net.hip).
//   ActorFeatures   a block per kFeatureRows rows, which are in env id order: nothing is scattered.  Key by key the
//                   block reads the key's rows as ONE span, consecutive threads consecutive elements, converts per
//                   dtype (ActorFeature) and puts the byte at its place of the rows' image in LDS; the image, nr * F
//                   contiguous bytes of the output, then leaves in 16-byte words with a byte head and tail (CopySpan:
//                   the image starts at the output's offset inside a 16-byte word).
//   ActorSample     a lane per row.  Reads the head's int32 row twice with running values (no per-thread array), draws
//                   its noise from (seed, global env id, step, j), writes the action row into the staging the step
//                   reads, logp and value.  value_only: just the value (slot T).
//   ActorLegal      the masked head's legal words.  A wave takes a row at a time, four waves a block, rows grid-strided:
//                   lanes j and j + 64 load the row's raw mask components (consecutive lanes, consecutive elements, any
//                   dtype), two ballots give the four words, an empty set -- and an actor without a mask -- becomes all
//                   ones, lane 0 writes the row's uint4 in one store.  Collect and eval share it.
//   ActorSampleMasked  kind 2's own kernel; ActorSample stays as it is for kinds 0 and 1 (and for value_only of every
//                   kind: that path reads p[H] alone).  A block of 256 threads takes kSampleRows = 32 rows, eight lanes a
//                   row; the rows' p enter LDS as one flat copy, in 16-byte words where the head's address allows.  A
//                   row's eight lanes share the order-free work over j = lane, lane + 8, .. of the legal set: logits, the
//                   two GumbelLogs of the noise, the running (score, j) with the lowest j winning ties, folded with the
//                   rows' top by three xor shuffles -- and, once top is known, the exponentials, which go back into LDS
//                   over the integers they came from (added to the starting design: the walk then only adds).  Lane 0
//                   walks S in ascending legal j over LDS, writes logp and value and the C int32 components of the flat
//                   index into the staging the step reads.
// Plain vector loads and stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.h"
#include "actor.hip.h"

namespace epa {
namespace {

using actor::kFeatureBlock;
using actor::kFeatureRows;

__global__ __launch_bounds__(kFeatureBlock) void ActorFeatures(actor::FeatureKeys keys, const double* __restrict__ lo,
                                                               const double* __restrict__ scale, int rows,
                                                               unsigned char* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char image[];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * kFeatureRows;
  const int nr = min(kFeatureRows, rows - r0);
  unsigned char* dst = out + (size_t)r0 * keys.F;
  unsigned char* stage = image + (reinterpret_cast<uintptr_t>(dst) & 15);
  for (int j = 0; j < keys.n; ++j) actor::FeatureKeySpan(keys, j, lo, scale, r0, nr, stage, tid, kFeatureBlock);
  __syncthreads();
  rollout::CopySpan(reinterpret_cast<const char*>(stage), reinterpret_cast<char*>(dst), (size_t)nr * keys.F, tid,
                    kFeatureBlock);
}

__global__ __launch_bounds__(256) void ActorSample(ActorSampleArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.rows) return;
  const int32_t* p = a.head + (size_t)i * (a.H + 1);
  if (a.value_only != 0) {
    a.value[i] = (float)p[a.H] * a.scale_v;
    return;
  }
  const int env = a.env_id != nullptr ? a.env_id[i] : a.id_offset + i;
  const uint64_t key = actor::ActorKey(a.seed, env, a.step);
  const bool det = a.deterministic != 0;
  actor::SampleOut o;
  if (a.kind == actor::kDiscrete) {
    o = actor::SampleDiscrete(p, a.H, a.scale_p, a.scale_v, key, det);
    static_cast<int32_t*>(a.action)[i] = o.action;
  } else if (a.action_dtype == EPA_F64) {
    o = actor::SampleBox<double>(p, a.H, a.scale_p, a.scale_v, a.sigma, a.low, a.high, key, det,
                                 static_cast<double*>(a.action) + (size_t)i * a.H);
  } else {
    o = actor::SampleBox<float>(p, a.H, a.scale_p, a.scale_v, a.sigma, a.low, a.high, key, det,
                                static_cast<float*>(a.action) + (size_t)i * a.H);
  }
  a.logp[i] = o.logp;
  a.value[i] = o.value;
}

__global__ __launch_bounds__(256) void ActorLegal(ActorLegalArgs a) {
  const int lane = threadIdx.x & 63;
  for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < a.rows; row += gridDim.x * 4) {  // (uniform in a wave)
    const uint4 w = actor::LegalBallot(a.src, a.dtype, (size_t)row * (size_t)a.elems + (size_t)a.first, a.H, lane);
    if (lane == 0) a.legal[row] = w;
  }
}

constexpr int kSampleRows = actor::kSampleRows, kSampleGroup = 8;
static_assert(kSampleRows * kSampleGroup == 256, "eight lanes a row");

__global__ __launch_bounds__(256) void ActorSampleMasked(ActorSampleArgs a) {
  // the block's rows of p behind the head's offset inside a 16-byte word
  __shared__ __attribute__((aligned(16))) int32_t s_p[kSampleRows * (pgx::kNetMaxActions + 1) + 4];
  const int t = threadIdx.x, H = a.H;
  const int r0 = blockIdx.x * kSampleRows;
  const int nr = min(kSampleRows, a.rows - r0);
  const int32_t* src = a.head + (size_t)r0 * (H + 1);
  int32_t* stage = s_p + ((reinterpret_cast<uintptr_t>(src) & 15) >> 2);
  rollout::CopySpan(reinterpret_cast<const char*>(src), reinterpret_cast<char*>(stage), (size_t)nr * (H + 1) * 4, t, 256);
  __syncthreads();

  const int row = t >> 3, l = t & (kSampleGroup - 1);
  const bool live = row < nr;
  const int i = r0 + (live ? row : 0);
  int32_t* p = stage + (live ? row : 0) * (H + 1);
  const uint4 lw = a.legal[i];
  const uint32_t legal[4] = {lw.x, lw.y, lw.z, lw.w};
  const int env = a.env_id != nullptr ? a.env_id[i] : a.id_offset + i;
  const uint64_t key = actor::ActorKey(a.seed, env, a.step);
  const bool det = a.deterministic != 0;

  float top = -FLT_MAX;
  actor::MaskedBest best{-FLT_MAX, 0.0f, actor::kNoAction};
  if (live) {
    for (int j = l; j < H; j += kSampleGroup) {
      if (!actor::LegalBit(legal, j)) continue;
      const float logit = pgx::NetLogit(p[j], a.scale_p);
      const actor::MaskedBest c{det ? logit : logit + pgx::SelfplayNoise(key, j), logit, j};
      top = logit > top ? logit : top;
      if (actor::MaskedBetter(c, best)) best = c;
    }
  }
  for (int w = kSampleGroup / 2; w >= 1; w >>= 1) {
    const actor::MaskedBest other{__shfl_xor(best.score, w), __shfl_xor(best.logit, w), __shfl_xor(best.j, w)};
    const float other_top = __shfl_xor(top, w);
    top = other_top > top ? other_top : top;
    if (actor::MaskedBetter(other, best)) best = other;
  }
  const float value = live ? (float)p[H] * a.scale_v : 0.0f;
  if (live) {
    for (int j = l; j < H; j += kSampleGroup) {
      if (actor::LegalBit(legal, j)) p[j] = pgx::NetFloatBits(pgx::GumbelExp(pgx::NetLogit(p[j], a.scale_p) - top));
    }
  }
  __syncthreads();
  if (!live || l != 0) return;
  float sum = 0.0f;
  for (int j = 0; j < H; ++j) {
    if (actor::LegalBit(legal, j)) sum = sum + pgx::NetBitsFloat(p[j]);
  }
  const int action = best.j == actor::kNoAction ? 0 : best.j;
  a.logp[i] = (best.logit - top) - pgx::GumbelLog(sum);
  a.value[i] = value;
  actor::ActorComponents(action, a.nvec, a.C, static_cast<int32_t*>(a.action) + (size_t)i * a.C);
}

}  // namespace

void ActorLaunchLegal(const ActorLegalArgs& a, hipStream_t s) {
  const unsigned blocks = (unsigned)std::min((a.rows + 3) / 4, 4096);
  hipLaunchKernelGGL(ActorLegal, dim3(blocks), dim3(256), 0, s, a);
}

void ActorLaunchFeatures(const actor::FeatureKeys& keys, const double* lo, const double* scale, int rows,
                         unsigned char* out, hipStream_t s) {
  const unsigned blocks = (unsigned)((rows + kFeatureRows - 1) / kFeatureRows);
  // (F <= 512: at most 32 KiB + the offset inside a word)
  const size_t lds = ((size_t)kFeatureRows * (size_t)keys.F + 16 + 15) & ~(size_t)15;
  hipLaunchKernelGGL(ActorFeatures, dim3(blocks), dim3(kFeatureBlock), lds, s, keys, lo, scale, rows, out);
}

void ActorLaunchSample(const ActorSampleArgs& a, hipStream_t s) {
  if (a.kind == actor::kMasked && a.value_only == 0) {
    hipLaunchKernelGGL(ActorSampleMasked, dim3((unsigned)((a.rows + kSampleRows - 1) / kSampleRows)), dim3(256), 0, s, a);
    return;
  }
  hipLaunchKernelGGL(ActorSample, dim3((unsigned)((a.rows + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace epa
