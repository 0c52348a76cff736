// Rollout collector kernels (rollout.hip.h is the contract; DESIGN.md section 2 "Rollout collector").  Family
// independent: they read a step's result block and the collector's own memory, never an env's state.
//   RolloutStore    a block per kStoreRows batch rows.  The rows' local env ids go to LDS; if they are consecutive
//                   (always, for a step of the whole pool in id order) each key's rows are ONE span that the block
//                   copies in 16-byte words with byte head and tail (CopySpan); otherwise a wave copies a row.  The
//                   first nr threads then do the rows' scalars: reward, term, trunc, mask, the carried done flag, the
//                   episode accumulators and the emission flag (StepRow).
//   RolloutScan     a block per kScanEnvs envs, in env order.  Its offset is the number of emission flags of all envs
//                   before it, counted from the flag bytes themselves (16 at a time, a population count per word; the
//                   redundant reads are N^2 / 2048 bytes in all); inside the block a ballot per wave and the waves'
//                   totals through LDS.  No atomics.  The last block commits the count (Control: parity words).
//   RolloutGae      a lane per env, t = T-1 .. 0; every load and store is a coalesced row of the time-major arrays
//   RolloutMoments  a block per group of kMomentRows rows: thread (leaf, component) sums its leaf in row order, the
//                   leaves of a component are summed in leaf order through LDS, tiles of 16 components at a time;
//   RolloutMomentsFold  one block: a thread per component sums the groups in group order (loads 32 groups ahead of
//                   the adds) and adds to the accumulators.
#include <algorithm>

#include "engine.h"
#include "rollout.hip.h"

namespace epa {
namespace {

using rollout::kMomentLeaf;
using rollout::kMomentLeaves;
using rollout::kMomentRows;
using rollout::kScanEnvs;
using rollout::kStoreBlock;
using rollout::kStoreRows;

__global__ __launch_bounds__(kStoreBlock) void RolloutStore(RolloutStepArgs a, int scalars) {
  __shared__ int env[kStoreRows];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * kStoreRows;
  const int nr = min(kStoreRows, a.k - r0);
  if (tid < nr) env[tid] = a.env_id != nullptr ? a.env_id[r0 + tid] - a.id_offset : r0 + tid;
  __syncthreads();
  // (an id outside the pool cannot come out of a step kernel; such a row is skipped all the same, never written)
  const bool in_range = tid < nr && env[tid] >= 0 && env[tid] < a.n;
  const int is_run = __syncthreads_and(tid >= nr || (in_range && env[tid] == env[0] + tid));
  for (int j = 0; j < a.keys.n; ++j) {
    const size_t rb = (size_t)a.keys.row_bytes[j];
    if (is_run) {
      rollout::CopySpan(a.keys.src[j] + (size_t)r0 * rb, a.keys.dst[j] + (size_t)env[0] * rb, (size_t)nr * rb, tid,
                        kStoreBlock);
    } else {
      for (int r = tid >> 6; r < nr; r += kStoreBlock / 64) {
        const int e = env[r];
        if (e < 0 || e >= a.n) continue;
        rollout::CopySpan(a.keys.src[j] + (size_t)(r0 + r) * rb, a.keys.dst[j] + (size_t)e * rb, rb, tid & 63, 64);
      }
    }
  }
  if (scalars == 0 || !in_range) return;
  const int i = r0 + tid, e = env[tid];
  const float rw = a.reward[i];
  double ret = a.acc_ret[e];
  int32_t len = a.acc_len[e];
  const rollout::StepRowOut o = rollout::StepRow(a.done[i] != 0, a.trunc[i] != 0, rw, a.carry[e], &ret, &len);
  a.rew[e] = rw;
  a.term[e] = o.term;
  a.trc[e] = o.trunc;
  a.mask[e] = o.mask;
  a.carry[e] = o.carry;
  a.emit[e] = o.emit;
  if (o.emit) {
    a.emit_ret[e] = ret;
    a.emit_len[e] = len;
    ret = 0.0;
    len = 0;
  }
  a.acc_ret[e] = ret;
  a.acc_len[e] = len;
}

__global__ __launch_bounds__(kScanEnvs) void RolloutScan(RolloutStepArgs a) {
  constexpr int kWaves = kScanEnvs / 64;
  __shared__ int before_blocks[kWaves], wave_total[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int e = blockIdx.x * kScanEnvs + tid;
  // emissions of the envs in front of this block: the flags are 0 / 1 bytes, so a word's population count is its sum
  int s = 0;
  const uint4* flags = reinterpret_cast<const uint4*>(a.emit);
  const int words = blockIdx.x * (kScanEnvs / 16);
  for (int i = tid; i < words; i += kScanEnvs) {
    const uint4 v = flags[i];
    s += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const bool f = e < a.n && a.emit[e] != 0;
  const unsigned long long bal = __ballot(f);
  if (lane == 0) {
    before_blocks[w] = s;
    wave_total[w] = __popcll(bal);
  }
  __syncthreads();
  long long prefix = 0, before = 0, block_total = 0;
  for (int i = 0; i < kWaves; ++i) {
    prefix += before_blocks[i];
    if (i < w) before += wave_total[i];
    block_total += wave_total[i];
  }
  const long long base = a.ctl->base[a.step & 1];
  const long long rank = prefix + before + __popcll(bal & ((1ull << lane) - 1ull));
  if (f && rollout::ScanFits(base, rank, a.capacity)) {
    const size_t row = (size_t)(base + rank);
    a.ep_env[row] = e + a.id_offset;
    a.ep_step[row] = a.step;
    a.ep_ret[row] = a.emit_ret[e];
    a.ep_len[row] = a.emit_len[e];
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {
    const long long total = prefix + block_total;
    const rollout::ScanCommitOut c = rollout::ScanCommit(base, total, a.capacity);
    a.ctl->count = c.count;
    a.ctl->base[(a.step + 1) & 1] = c.count;
    a.ctl->finished += total;
    a.ctl->dropped += c.dropped;
  }
}

__global__ __launch_bounds__(256) void RolloutGae(int horizon, int n, const float* __restrict__ reward,
                                                  const unsigned char* __restrict__ term,
                                                  const unsigned char* __restrict__ trunc,
                                                  const unsigned char* __restrict__ mask,
                                                  const float* __restrict__ values, float gamma, float lam,
                                                  float* __restrict__ adv, float* __restrict__ ret) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) rollout::GaeEnv(horizon, n, e, reward, term, trunc, mask, values, gamma, lam, adv, ret);
}

template <class T>
__global__ __launch_bounds__(256) void RolloutMoments(const T* __restrict__ x, int n, int comps, int comp0,
                                                      int comps_total, double* __restrict__ partial) {
  __shared__ double leaf[kMomentLeaves][16][2];
  const int g = blockIdx.x, l = threadIdx.x >> 4, cc = threadIdx.x & 15;
  const int r0 = min(n, g * kMomentRows + l * kMomentLeaf), r1 = min(n, r0 + kMomentLeaf);
  for (int c0 = 0; c0 < comps; c0 += 16) {
    const int c = c0 + cc;
    double s1 = 0.0, s2 = 0.0;
    if (c < comps) rollout::MomentLeafSum(x, comps, c, r0, r1, &s1, &s2);
    leaf[l][cc][0] = s1;
    leaf[l][cc][1] = s2;
    __syncthreads();
    if (l == 0 && c < comps) {
      double t1 = 0.0, t2 = 0.0;
      for (int i = 0; i < kMomentLeaves; ++i) {
        t1 = t1 + leaf[i][cc][0];
        t2 = t2 + leaf[i][cc][1];
      }
      double* p = partial + ((size_t)g * comps_total + comp0 + c) * 2;
      p[0] = t1;
      p[1] = t2;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void RolloutMomentsFold(const double* __restrict__ partial, int groups, int n,
                                                          int comps_total, double* __restrict__ acc) {
  // The groups are added in group order, one thread per component.  kAhead groups' pairs are loaded before they are
  // added: the adds are the contract's and stay in order, the loads are independent, so a trip waits for memory once
  // and not kAhead times (one load per add made this kernel 49 us at 256 groups, all of it latency; 8 ahead 17 us).
  constexpr int kAhead = 32;
  const double2* pairs = reinterpret_cast<const double2*>(partial);
  for (int c = threadIdx.x; c < comps_total; c += 256) {
    double s1 = 0.0, s2 = 0.0;
    for (int g0 = 0; g0 < groups; g0 += kAhead) {
      double2 v[kAhead];
#pragma unroll
      for (int j = 0; j < kAhead; ++j) {
        v[j] = g0 + j < groups ? pairs[(size_t)(g0 + j) * comps_total + c] : make_double2(0.0, 0.0);
      }
#pragma unroll
      for (int j = 0; j < kAhead; ++j) {
        if (g0 + j < groups) {
          s1 = s1 + v[j].x;
          s2 = s2 + v[j].y;
        }
      }
    }
    acc[c] = acc[c] + (double)n;
    acc[comps_total + c] = acc[comps_total + c] + s1;
    acc[2 * comps_total + c] = acc[2 * comps_total + c] + s2;
  }
}

}  // namespace

void RolloutLaunchStore(const RolloutStepArgs& a, bool scalars, hipStream_t s) {
  const unsigned blocks = (unsigned)((a.k + kStoreRows - 1) / kStoreRows);
  hipLaunchKernelGGL(RolloutStore, dim3(blocks), dim3(kStoreBlock), 0, s, a, scalars ? 1 : 0);
}

void RolloutLaunchScan(const RolloutStepArgs& a, hipStream_t s) {
  const unsigned blocks = (unsigned)((a.n + kScanEnvs - 1) / kScanEnvs);
  hipLaunchKernelGGL(RolloutScan, dim3(blocks), dim3(kScanEnvs), 0, s, a);
}

void RolloutLaunchGae(int horizon, int n, const float* reward, const unsigned char* term, const unsigned char* trunc,
                      const unsigned char* mask, const float* values, float gamma, float lam, float* adv, float* ret,
                      hipStream_t s) {
  hipLaunchKernelGGL(RolloutGae, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, horizon, n, reward, term, trunc,
                     mask, values, gamma, lam, adv, ret);
}

void RolloutLaunchMoments(const void* x, int dtype, int n, int comps, int comp0, int comps_total, double* partial,
                          hipStream_t s) {
  const unsigned groups = (unsigned)rollout::MomentGroups(n);
  if (dtype == EPA_F64) {
    hipLaunchKernelGGL(RolloutMoments<double>, dim3(groups), dim3(256), 0, s, static_cast<const double*>(x), n, comps,
                       comp0, comps_total, partial);
  } else {
    hipLaunchKernelGGL(RolloutMoments<float>, dim3(groups), dim3(256), 0, s, static_cast<const float*>(x), n, comps,
                       comp0, comps_total, partial);
  }
}

void RolloutLaunchMomentsFold(const double* partial, int n, int comps_total, double* acc, hipStream_t s) {
  hipLaunchKernelGGL(RolloutMomentsFold, dim3(1), dim3(256), 0, s, partial, rollout::MomentGroups(n), n, comps_total,
                     acc);
}

}  // namespace epa
