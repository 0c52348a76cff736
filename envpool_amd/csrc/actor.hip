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

}  // namespace

void ActorLaunchFeatures(const actor::FeatureKeys& keys, const double* lo, const double* scale, int rows,
                         unsigned char* out, hipStream_t s) {
  const unsigned blocks = (unsigned)((rows + kFeatureRows - 1) / kFeatureRows);
  // (F <= 512: at most 32 KiB + the offset inside a word)
  const size_t lds = ((size_t)kFeatureRows * (size_t)keys.F + 16 + 15) & ~(size_t)15;
  hipLaunchKernelGGL(ActorFeatures, dim3(blocks), dim3(kFeatureBlock), lds, s, keys, lo, scale, rows, out);
}

void ActorLaunchSample(const ActorSampleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ActorSample, dim3((unsigned)((a.rows + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace epa
