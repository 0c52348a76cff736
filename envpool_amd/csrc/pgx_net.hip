// PGX built-in network on the int8 matrix cores (pgx_net.hip.h is the contract; DESIGN.md "PGX built-in network").
//
// PgxNetEval: one launch per evaluation, one wave per block, 64 rows per wave as two 32-row tiles.  Every layer is
// OUT[n][row] = SUM_k W[n][k] X[row][k] on v_mfma_i32_32x32x32_i8 with the WEIGHTS as the A operand (M = 32 output
// neurons) and the ACTIVATIONS as the B operand (N = 32 rows), so that a result tile -- column = lane & 31 = the row,
// neuron (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) in register reg -- becomes, after shift, clamp and packing to bytes,
// the B fragment of the next layer's k-step with no lane movement: dword g of lane (r, hh) holds neurons
// 8 g + 4 hh .. + 3 of the tile.  The k order inside a step is therefore (g, hh, byte) and not natural; the weights are
// laid out to match at upload (NetBuildImage): for output tile `ot` and k-step `kt` the wave reads 1 KiB, lane (r, hh)
// its 16 bytes, dword g = W[32 ot + r][32 kt + 8 g + 4 hh .. + 3].  The first layer's B fragments are read from `obs`
// in that same order.  Whatever order the matrix core gives the 16 bytes of a lane's fragment inside its k-step, A
// and B use the same one, so only the documented C/D map is relied on (the single-layer test of
// tests/test_gpu_pgx_net.py pins it with an identity-like W_in and an asymmetric head).
//
// Activations never leave the CU: a lane keeps its packed fragments of h and t in LDS slots only it reads and writes
// (LDS as an indexed register file: no barrier), 2 KiB per 32 neurons and wave.  The head's int32 results go through
// LDS once to turn them from (neuron in register, row on lane) to one row per lane for NetOutputs -- the one
// barrier pair --, and the float rows leave in coalesced stores.  Weights are read from global memory (L2).
//
// The pair form (pgx_arena.hip.h is the contract; DESIGN.md "PGX arena"): PgxNetEval<true> takes two networks, the plan
// `order` / `n0` of PgxNetPlan and one wave more than the single form.  A wave finds its net and its entries of the plan
// with ArenaWaveOf, gathers its two row tiles through `order`, runs that net's layers and stores each row's value and
// policy back to the row's own place, A floats in a run.  The weights being the A operand, a wave serves one net: the
// plan is what puts rows of one net side by side.  Lanes past the wave's entries load nothing and store nothing but
// stay in every MFMA and barrier.
//
// PgxNetPlan: the stable partition of the rows by side in two launches of single-wave blocks, 256 rows per wave as four
// ballots.  PgxNetPlanCount leaves each block's number of side-0 rows; PgxNetPlanPlace adds up the counts of the blocks
// in front of its own (lane l the counts l, l + 64, .., then a butterfly: the scan across blocks), takes a row's place
// inside the wave from the popcount of the ballot below its lane, and scatters the row index.  No atomics, no LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "engine.h"
#include "pgx_arena.hip.h"
#include "pgx_net.hip.h"

namespace epa {
namespace {

using pgx::kGuidedIdle;

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kWave = 64, kRowsPerWave = 64;
static_assert(pgx::kNetMaxLayers == kNetImageLayers, "engine.h: NetImage");

struct NetDev {
  int F, A, D, L;
  float scale_p, scale_v;
  const char* base;
  uint32_t w_off[pgx::kNetMaxLayers], b_off[pgx::kNetMaxLayers];
  int32_t shift[pgx::kNetMaxLayers];
};

// the neuron (within its 32-neuron tile) of accumulator register `reg` of a lane of half `hh`
__device__ inline int TileNeuron(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }

// One layer for the wave's two row tiles: in / out / res are the lane's LDS slots, [tile][row tile][lane] of 16 bytes.
// res == nullptr: out = act(rs(.)); otherwise out = clamp(rs(.) + res, 0, 127) (res may be out).
__device__ inline void NetLayerTiles(const v4i* __restrict__ w, const int32_t* __restrict__ bias, int shift, int n_tiles,
                                     int k_tiles, const v4i* in, v4i* out, const v4i* res, int lane) {
  const int hh = lane >> 5;
  for (int ot = 0; ot < n_tiles; ++ot) {
    v16i acc0, acc1;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc0[reg] = acc1[reg] = bias[32 * ot + TileNeuron(reg, hh)];
    const v4i* wt = w + (size_t)ot * k_tiles * kWave + lane;
    for (int kt = 0; kt < k_tiles; ++kt) {
      const v4i a = wt[(size_t)kt * kWave];
      const v4i b0 = in[(kt * 2 + 0) * kWave + lane];
      const v4i b1 = in[(kt * 2 + 1) * kWave + lane];
      acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b1, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const v16i& acc = rt == 0 ? acc0 : acc1;
      v4i old = {0, 0, 0, 0};
      if (res != nullptr) old = res[(ot * 2 + rt) * kWave + lane];
      v4i packed;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          int32_t v = pgx::NetRs(acc[4 * g + b], shift);
          if (res != nullptr) v += (int32_t)(((uint32_t)old[g] >> (8 * b)) & 255u);
          word |= (uint32_t)pgx::NetAct(v) << (8 * b);
        }
        packed[g] = (int)word;
      }
      out[(ot * 2 + rt) * kWave + lane] = packed;
    }
  }
}

// The kernel's networks: indexed by the wave's net, which is uniform, so the fields stay scalar loads from the kernel
// arguments (two separate arguments chosen by a select would be copied to scratch)
struct NetPair {
  NetDev n[2];
};

// The plan of a pair evaluation (null and unused in the single form)
struct NetPlan {
  const int32_t* order;  // [rows]
  const int32_t* n0;
};

// PAIR: nets.n[1] and plan are read, and the wave's rows are its entries of the plan; otherwise rows row0 .. row0 + 63.
// A row past the wave's share is `rows`, which every `< rows` test below turns away.
// RAW (the rollout actor, actor.hip.h): the input bytes are features 0 .. 127 and not 0 / 1, every row below `rows` is
// evaluated (mask and status are not read), and what leaves is the head's int32 p, A + 1 words per row, through
// `policy`; `value` is not written.  The single form only.
template <bool PAIR, bool RAW = false>
__global__ __launch_bounds__(kWave) void PgxNetEval(NetPair nets, NetPlan plan, int rows, int mode,
                                                     const unsigned char* __restrict__ obs,
                                                     const unsigned char* __restrict__ mask,
                                                     const unsigned char* __restrict__ status,
                                                     float* __restrict__ policy, float* __restrict__ value,
                                                     unsigned int* pending) {
  extern __shared__ v4i lds[];
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  pgx::ArenaWave wave{0, (int)blockIdx.x * kRowsPerWave, 0};
  if constexpr (PAIR) {
    wave = pgx::ArenaWaveOf((int)blockIdx.x, rows, *plan.n0);
    if (wave.count == 0) return;  // (the whole wave, before any barrier)
  }
  const NetDev& net = nets.n[PAIR ? wave.net : 0];
  const int row0 = wave.first;
  const int F = net.F, A = net.A, d_tiles = net.D / 32, f_tiles = (F + 31) / 32, a_tiles = (A + 1 + 31) / 32;
  int my_row = row0 + lane;
  if constexpr (PAIR) my_row = lane < wave.count ? plan.order[row0 + lane] : rows;
  int my_status = kGuidedIdle;
  if constexpr (RAW) {
    my_status = my_row < rows ? pgx::kGuidedEvaluate : kGuidedIdle;
  } else {
    my_status = my_row < rows ? (int)status[my_row] : kGuidedIdle;
  }
  // the run loop's word: some row of the call is not idle (an ordinary atomic of one lane per wave)
  const bool wave_pending = __any(my_status != kGuidedIdle) != 0;
  if (wave_pending && lane == 0 && pending != nullptr) atomicOr(pending, 1u);

  v4i* hbuf = lds;                                // [d_tiles][2][64]
  v4i* tbuf = lds + (size_t)d_tiles * 2 * kWave;  // [max(d_tiles, f_tiles)][2][64], then the head's rows
  const int stride = 32 * a_tiles + 1;            // words per row of the head's image (odd: no bank conflicts)
  int32_t* rows_io = reinterpret_cast<int32_t*>(tbuf);

  if (__any(my_status == pgx::kGuidedEvaluate) != 0) {
    // the input fragments, in the k order of the header comment
    const bool words = (F & 3) == 0 && (reinterpret_cast<uintptr_t>(obs) & 3) == 0;
    for (int kt = 0; kt < f_tiles; ++kt) {
      for (int rt = 0; rt < 2; ++rt) {
        int row = row0 + 32 * rt + r;
        if constexpr (PAIR) row = __shfl(my_row, 32 * rt + r, kWave);
        v4i frag = {0, 0, 0, 0};
        if (row < rows) {
          const unsigned char* x = obs + (size_t)row * F;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int k = 32 * kt + 8 * g + 4 * hh;
            uint32_t word = 0;
            if (words) {
              if (k < F) word = *reinterpret_cast<const uint32_t*>(x + k);
            } else {
              for (int b = 0; b < 4; ++b) {
                if (k + b < F) word |= (uint32_t)x[k + b] << (8 * b);
              }
            }
            // (a bool's byte is 0 or 1; anything else counts as its low bit.  RAW: a feature is 0 .. 127)
            frag[g] = (int)(word & (RAW ? 0x7f7f7f7fu : 0x01010101u));
          }
        }
        tbuf[(kt * 2 + rt) * kWave + lane] = frag;
      }
    }
    auto weights = [&](int i) { return reinterpret_cast<const v4i*>(net.base + net.w_off[i]); };
    auto biases = [&](int i) { return reinterpret_cast<const int32_t*>(net.base + net.b_off[i]); };
    NetLayerTiles(weights(0), biases(0), net.shift[0], d_tiles, f_tiles, tbuf, hbuf, nullptr, lane);
    for (int l = 0; l < net.L; ++l) {
      NetLayerTiles(weights(1 + 2 * l), biases(1 + 2 * l), net.shift[1 + 2 * l], d_tiles, d_tiles, hbuf, tbuf, nullptr,
                    lane);
      NetLayerTiles(weights(2 + 2 * l), biases(2 + 2 * l), net.shift[2 + 2 * l], d_tiles, d_tiles, tbuf, hbuf, hbuf,
                    lane);
    }
    // the head: p into the rows' image, row 32 rt + r, neuron in register
    const int head = 2 * net.L + 1;
    const v4i* w = weights(head);
    const int32_t* bias = biases(head);
    __syncthreads();  // (every lane is done with tbuf as fragments: the rows' image takes its place)
    for (int ot = 0; ot < a_tiles; ++ot) {
      v16i acc0, acc1;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) acc0[reg] = acc1[reg] = bias[32 * ot + TileNeuron(reg, hh)];
      for (int kt = 0; kt < d_tiles; ++kt) {
        const v4i a = w[((size_t)ot * d_tiles + kt) * kWave + lane];
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, hbuf[(kt * 2 + 0) * kWave + lane], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, hbuf[(kt * 2 + 1) * kWave + lane], acc1, 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int n = 32 * ot + TileNeuron(reg, hh);  // (n < 32 a_tiles < stride)
        rows_io[r * stride + n] = acc0[reg];
        rows_io[(32 + r) * stride + n] = acc1[reg];
      }
    }
    __syncthreads();
    if constexpr (!RAW) {
      if (my_row < rows) {
        pgx::NetOutputs(rows_io + lane * stride, mask + (size_t)my_row * A, A, net.scale_p, net.scale_v, mode,
                        my_status);
      }
    }
  } else {
    for (int a = 0; a <= A; ++a) rows_io[lane * stride + a] = 0;  // no row of the wave is to be evaluated
  }
  __syncthreads();
  if constexpr (RAW) {
    const int n_rows = rows - row0 < kRowsPerWave ? rows - row0 : kRowsPerWave;
    int32_t* head = reinterpret_cast<int32_t*>(policy);
    for (int i = lane; i < n_rows * (A + 1); i += kWave) {
      head[(size_t)row0 * (A + 1) + i] = rows_io[(i / (A + 1)) * stride + i % (A + 1)];
    }
    return;
  }
  if (my_row < rows) value[my_row] = pgx::NetBitsFloat(rows_io[lane * stride + A]);
  if constexpr (PAIR) {
    // entry e's A floats go to its row's own place: consecutive lanes, consecutive floats of a run
    for (int i = lane; i < wave.count * A; i += kWave) {
      const int e = i / A, a = i - e * A;
      policy[(size_t)plan.order[row0 + e] * A + a] = pgx::NetBitsFloat(rows_io[e * stride + a]);
    }
  } else {
    const int n_rows = rows - row0 < kRowsPerWave ? rows - row0 : kRowsPerWave;
    for (int i = lane; i < n_rows * A; i += kWave) {
      policy[(size_t)row0 * A + i] = pgx::NetBitsFloat(rows_io[(i / A) * stride + i % A]);
    }
  }
}

constexpr int kPlanChunk = 4;                     // ballots of a wave
constexpr int kPlanRows = kPlanChunk * kWave;     // rows of a wave of the plan
static_assert(pgx::kArenaMaxRows == kNetPlanMaxRows && pgx::kArenaMaxRows % kPlanRows == 0, "engine.h: a plan's rows");

// side-0 rows of block b's rows (every lane gets the sum), and the ballot of each of its chunks
__device__ inline int PlanBallots(const unsigned char* __restrict__ side, int rows, int lane,
                                  unsigned long long zero[kPlanChunk]) {
  int count = 0;
#pragma unroll
  for (int c = 0; c < kPlanChunk; ++c) {
    const int row = (int)blockIdx.x * kPlanRows + c * kWave + lane;
    zero[c] = __ballot(row < rows && side[row] == 0);
    count += __popcll(zero[c]);
  }
  return count;
}

__global__ __launch_bounds__(kWave) void PgxNetPlanCount(const unsigned char* __restrict__ side, int rows,
                                                          int32_t* __restrict__ counts) {
  unsigned long long zero[kPlanChunk];
  const int count = PlanBallots(side, rows, threadIdx.x, zero);
  if (threadIdx.x == 0) counts[blockIdx.x] = count;
}

__global__ __launch_bounds__(kWave) void PgxNetPlanPlace(const unsigned char* __restrict__ side, int rows,
                                                          const int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ order, int32_t* __restrict__ n0_out) {
  const int lane = threadIdx.x, b = blockIdx.x, blocks = gridDim.x;
  int before = 0, all = 0;  // the side-0 rows of the blocks in front of this one, and of all blocks
  for (int j = lane; j < blocks; j += kWave) {
    const int c = counts[j];
    before += j < b ? c : 0;
    all += c;
  }
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    before += __shfl_xor(before, w, kWave);
    all += __shfl_xor(all, w, kWave);
  }
  if (b == 0 && lane == 0) *n0_out = all;
  unsigned long long zero[kPlanChunk];
  PlanBallots(side, rows, lane, zero);
  int below0 = before;  // the side-0 rows below the chunk
#pragma unroll
  for (int c = 0; c < kPlanChunk; ++c) {
    const int row = b * kPlanRows + c * kWave + lane;
    const unsigned long long mine = 1ull << lane;
    if (row < rows) {
      const int s = (zero[c] & mine) != 0 ? 0 : 1;
      order[pgx::ArenaPlace(s, row, below0 + __popcll(zero[c] & (mine - 1)), all)] = row;
    }
    below0 += __popcll(zero[c]);
  }
}

size_t LdsBytes(int F, int A, int D) {
  const size_t d_tiles = (size_t)D / 32, f_tiles = ((size_t)F + 31) / 32, a_tiles = ((size_t)A + 1 + 31) / 32;
  const size_t frag = 2 * kWave * sizeof(v4i);  // a tile of both row tiles
  const size_t second = std::max(std::max(d_tiles, f_tiles) * frag, (size_t)kRowsPerWave * (32 * a_tiles + 1) * 4);
  return d_tiles * frag + second;
}

}  // namespace

void NetBuildImage(const void* blob, size_t bytes, NetImage* out) {
  pgx::NetView v{};
  char err[200];
  if (!pgx::NetParse(blob, bytes, &v, err, sizeof(err))) throw std::invalid_argument(err);
  out->F = v.F, out->A = v.A, out->D = v.D, out->L = v.L;
  out->scale_p = v.scale_p, out->scale_v = v.scale_v;
  out->layers = v.layers();
  out->bytes.clear();
  for (int i = 0; i < v.layers(); ++i) {
    const pgx::NetLayer& l = v.layer[i];
    const size_t n_tiles = ((size_t)l.n_out + 31) / 32, k_tiles = ((size_t)l.k_in + 31) / 32;
    out->shift[i] = l.shift;
    out->w_off[i] = (uint32_t)out->bytes.size();
    out->bytes.resize(out->bytes.size() + n_tiles * k_tiles * 1024, 0);
    char* w = out->bytes.data() + out->w_off[i];
    for (size_t ot = 0; ot < n_tiles; ++ot) {
      for (size_t kt = 0; kt < k_tiles; ++kt) {
        for (int lane = 0; lane < kWave; ++lane) {
          const size_t n = 32 * ot + (size_t)(lane & 31);
          for (int e = 0; e < 16; ++e) {  // byte e of the lane's 16: dword g = e / 4
            const size_t k = 32 * kt + 8 * (size_t)(e >> 2) + 4 * (size_t)(lane >> 5) + (size_t)(e & 3);
            if (n < (size_t)l.n_out && k < (size_t)l.k_in) {
              w[((ot * k_tiles + kt) * kWave + lane) * 16 + e] = (char)l.w[n * l.k_in + k];
            }
          }
        }
      }
    }
    out->b_off[i] = (uint32_t)out->bytes.size();
    out->bytes.resize(out->bytes.size() + n_tiles * 32 * 4, 0);
    std::memcpy(out->bytes.data() + out->b_off[i], l.b, 4 * (size_t)l.n_out);
  }
  out->bytes.resize((out->bytes.size() + 255) & ~(size_t)255, 0);
}

namespace {
NetDev DevOf(const NetImage& im, const char* d_image) {
  NetDev net{};
  net.F = im.F, net.A = im.A, net.D = im.D, net.L = im.L;
  net.scale_p = im.scale_p, net.scale_v = im.scale_v;
  net.base = d_image;
  for (int i = 0; i < im.layers; ++i) {
    net.w_off[i] = im.w_off[i], net.b_off[i] = im.b_off[i], net.shift[i] = im.shift[i];
  }
  return net;
}
}  // namespace

void NetLaunch(const NetImage& im, const char* d_image, int rows, int mode, const unsigned char* obs,
               const unsigned char* mask, const unsigned char* status, float* policy, float* value,
               unsigned int* pending, hipStream_t stream) {
  NetPair nets{};
  nets.n[0] = DevOf(im, d_image);
  const size_t lds = LdsBytes(im.F, im.A, im.D);
  if (lds > 48 * 1024) {
    EPA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&PgxNetEval<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  const int blocks = (rows + kRowsPerWave - 1) / kRowsPerWave;
  hipLaunchKernelGGL(PgxNetEval<false>, dim3(blocks), dim3(kWave), lds, stream, nets, NetPlan{nullptr, nullptr},
                     rows, mode, obs, mask, status, policy, value, pending);
}

void NetLaunchRaw(const NetImage& im, const char* d_image, int rows, const unsigned char* features, int32_t* head,
                  hipStream_t stream) {
  NetPair nets{};
  nets.n[0] = DevOf(im, d_image);
  const size_t lds = LdsBytes(im.F, im.A, im.D);
  if (lds > 48 * 1024) {
    EPA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&PgxNetEval<false, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  const int blocks = (rows + kRowsPerWave - 1) / kRowsPerWave;
  hipLaunchKernelGGL((PgxNetEval<false, true>), dim3(blocks), dim3(kWave), lds, stream, nets, NetPlan{nullptr, nullptr},
                     rows, 0, features, nullptr, nullptr, reinterpret_cast<float*>(head), nullptr, nullptr);
}

size_t NetPlanCountBytes(size_t rows) { return 4 * ((rows + kPlanRows - 1) / kPlanRows); }

void NetPlanLaunch(int rows, const unsigned char* side, int32_t* counts, int32_t* order, int32_t* n0,
                   hipStream_t stream) {
  const int blocks = (rows + kPlanRows - 1) / kPlanRows;
  hipLaunchKernelGGL(PgxNetPlanCount, dim3(blocks), dim3(kWave), 0, stream, side, rows, counts);
  hipLaunchKernelGGL(PgxNetPlanPlace, dim3(blocks), dim3(kWave), 0, stream, side, rows, counts, order, n0);
}

void NetLaunchPair(const NetImage& im_a, const char* d_image_a, const NetImage& im_b, const char* d_image_b, int rows,
                   int mode, const int32_t* order, const int32_t* n0, const unsigned char* obs,
                   const unsigned char* mask, const unsigned char* status, float* policy, float* value,
                   unsigned int* pending, hipStream_t stream) {
  // (the larger of the two nets: a wave of either fits)
  const size_t lds = std::max(LdsBytes(im_a.F, im_a.A, im_a.D), LdsBytes(im_b.F, im_b.A, im_b.D));
  if (lds > 48 * 1024) {
    EPA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&PgxNetEval<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  NetPair nets{};
  nets.n[0] = DevOf(im_a, d_image_a), nets.n[1] = DevOf(im_b, d_image_b);
  hipLaunchKernelGGL(PgxNetEval<true>, dim3(pgx::ArenaWaves(rows)), dim3(kWave), lds, stream, nets, NetPlan{order, n0},
                     rows, mode, obs, mask, status, policy, value, pending);
}

}  // namespace epa
