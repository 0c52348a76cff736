// PGX built-in network, training, on the matrix cores (pgx_train.hip.h is the contract; DESIGN.md "PGX built-in
// network: training").  Five kernels and the handle that owns their memory.
//
// TrainPack, once per forward: the caller's quantised weights, int8 [N][K] row-major on the device, into the two forms
//   the other kernels read -- the 1 KiB (output tile, k-step) fragments of PgxNetEval with the bias padded to whole
//   tiles, and the transpose as bf16 [K32][N16] (N16 = N up to a multiple of 16, K32 = K up to a multiple of 32, which
//   only the trunk's F can be short of; zeros behind N and K; an int8 is exact in bf16), in which a B fragment of
//   dx = dz W is one 128-bit load.
// TrainForward: PgxNetEval's tiling -- one wave per block and 64 rows as two 32-column tiles, the weights as the A
//   operand of v_mfma_i32_32x32x32_i8, a lane's packed result the next layer's B fragment, activations in LDS slots only
//   their lane touches.  After every layer the lane stores its four result words, with bit 7 of a byte set where the
//   clamp changed the value, to the saved bytes (32 bytes of a row per tile from a lane pair); the copy in LDS keeps bit
//   7 clear.  The head's int32 p leaves through the rows' image in LDS, A + 1 words per row.
// TrainSplitDp: dp float32 [rows][A + 1] -> the split form [rows][N16].
// TrainBackRow<T>, per layer from the head down to layer 1: dx = dz W on v_mfma_f32_32x32x16_bf16.  A block of four
//   waves takes 64 rows.  dz is the A operand (M = 32 rows): lane (r, hh) loads the 8 split words
//   dz[row r][16 ns + 8 hh ..] and tears them into a hi and a lo fragment with four byte permutes each.  W^T is the B
//   operand (N = 32 input neurons): lane (c, hh) loads Wt[32 kt + c][16 ns + 8 hh ..].  Wave w owns the column tiles
//   kt = w, w + 4, .. (T of them, D <= 128 T), all of whose accumulators stay in registers over one pass through N, so
//   a dz fragment is loaded and torn once per wave.  The result tile has column c on the lane and row
//   (reg & 3) + 8 (reg >> 2) + 4 hh in register reg: the epilogue adds the residual branch (the split dz of the
//   block's second layer times 2^s, read before the same lane overwrites it: the kernel may run in place), applies the
//   saved mask bit and the 2^-s of the layer below, and stores the split result, 128 bytes of a row per register.
//   TrainBackRow<T, true> is the same product for layer 0 (NetTrain::InputGrad): the column tiles cover F, and the
//   epilogue stores the float32 sums of the columns below F as they are.
// TrainReduce: dW = dz^T x and db.  Grid (K tile of 64, N tile of 64, row slice), four waves, one 32 x 32 tile each.
//   Both operands need the row as the k index, so 64 rows at a time go through LDS transposed: dz as two bf16 planes
//   [n][row], x as bf16 [k][row] (a saved byte less its bit 7), rows of 72 elements so that a fragment is one aligned
//   128-bit read and the transposing 16-bit writes of a wave spread over the banks.  Two MFMAs per 16 rows (hi, lo);
//   the waves of K tile 0 add two more against a fragment of ones, which is db.  Every 128 rows the accumulator is
//   folded into a second one (the contract's error bound).  The slice's partial sums go to the workspace
//   [slice][N][K + 1], db in column K.
// TrainSum: a thread per element adds the slices in ascending order and writes dW and db.
//
// All launches of a call are enqueued from one C++ function on the caller's stream; nothing waits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "engine.h"
#include "pgx_train.hip.h"

namespace epa {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

constexpr int kWave = 64, kRowsPerWave = 64;
constexpr int kL = pgx::kNetMaxLayers;

// the row (within its 32-row tile) of accumulator register `reg` of a lane of half `hh`: the C/D map of both MFMAs
__device__ inline int TileRow(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }

// ---------------------------------------------------------------------------
// TrainPack
// ---------------------------------------------------------------------------
struct PackArgs {
  int layers;
  const signed char* w[kL];
  const int32_t* b[kL];
  int n_out[kL], k_in[kL];
  char* image;       // the forward's fragments and biases
  uint16_t* wt;      // the bf16 transposes
  uint32_t w_off[kL], b_off[kL], wt_off[kL];  // bytes into image; elements into wt
};

__global__ __launch_bounds__(256) void TrainPack(PackArgs a) {
  const int i = blockIdx.y;
  const int N = a.n_out[i], K = a.k_in[i];
  const int n_tiles = (N + 31) / 32, k_tiles = (K + 31) / 32, n16 = (N + 15) / 16 * 16;
  const int frag_bytes = n_tiles * k_tiles * 1024, bias_words = n_tiles * 32, wt_elems = 32 * k_tiles * n16;
  const signed char* __restrict__ w = a.w[i];
  for (int q = blockIdx.x * 256 + threadIdx.x; q < frag_bytes + bias_words + wt_elems; q += gridDim.x * 256) {
    if (q < frag_bytes) {
      const int e = q & 15, lane = (q >> 4) & 63, tile = q >> 10;
      const int n = 32 * (tile / k_tiles) + (lane & 31);
      const int k = 32 * (tile % k_tiles) + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
      a.image[a.w_off[i] + q] = n < N && k < K ? (char)w[(size_t)n * K + k] : (char)0;
    } else if (q < frag_bytes + bias_words) {
      const int n = q - frag_bytes;
      reinterpret_cast<int32_t*>(a.image + a.b_off[i])[n] = n < N ? a.b[i][n] : 0;
    } else {
      const int t = q - frag_bytes - bias_words, k = t / n16, n = t - k * n16;
      const float v = n < N && k < K ? (float)w[(size_t)n * K + k] : 0.0f;
      a.wt[a.wt_off[i] + t] = (uint16_t)((uint32_t)pgx::NetFloatBits(v) >> 16);  // (7 bits: exact)
    }
  }
}

// ---------------------------------------------------------------------------
// TrainForward
// ---------------------------------------------------------------------------
struct FwdNet {
  int F, A, D, L;
  const char* image;
  uint32_t w_off[kL], b_off[kL];
  int32_t shift[kL];
};

// One layer for the wave's two row tiles (pgx_net.hip: NetLayerTiles) that also stores the saved bytes of its output:
// `keep` points at the row tile's first row of activation j, `rows_left` rows of it exist.
__device__ inline void TrainLayerTiles(const v4i* __restrict__ w, const int32_t* __restrict__ bias, int shift,
                                       int n_tiles, int k_tiles, const v4i* in, v4i* out, const v4i* res,
                                       unsigned char* __restrict__ keep, int D, int rows_left, int lane) {
  const int r = lane & 31, hh = lane >> 5;
  for (int ot = 0; ot < n_tiles; ++ot) {
    v16i acc0, acc1;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc0[reg] = acc1[reg] = bias[32 * ot + TileRow(reg, hh)];
    const v4i* wt = w + (size_t)ot * k_tiles * kWave + lane;
    for (int kt = 0; kt < k_tiles; ++kt) {
      const v4i a = wt[(size_t)kt * kWave];
      acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, in[(kt * 2 + 0) * kWave + lane], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, in[(kt * 2 + 1) * kWave + lane], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const v16i& acc = rt == 0 ? acc0 : acc1;
      v4i old = {0, 0, 0, 0};
      if (res != nullptr) old = res[(ot * 2 + rt) * kWave + lane];
      v4i packed, flagged;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint32_t word = 0, flags = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          int32_t v = pgx::NetRs(acc[4 * g + b], shift);
          if (res != nullptr) v += (int32_t)(((uint32_t)old[g] >> (8 * b)) & 255u);
          const int32_t act = pgx::NetAct(v);
          word |= (uint32_t)act << (8 * b);
          flags |= (act != v ? 128u : 0u) << (8 * b);
        }
        packed[g] = (int)word;
        flagged[g] = (int)(word | flags);
      }
      out[(ot * 2 + rt) * kWave + lane] = packed;
      const int row = 32 * rt + r;
      if (row < rows_left) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(keep + (size_t)row * D + 32 * ot + 4 * hh);
#pragma unroll
        for (int g = 0; g < 4; ++g) dst[2 * g] = (uint32_t)flagged[g];  // neurons 32 ot + 8 g + 4 hh .. + 3
      }
    }
  }
}

__global__ __launch_bounds__(kWave) void TrainForward(FwdNet net, int rows, const unsigned char* __restrict__ x,
                                                       unsigned char* __restrict__ saved, int32_t* __restrict__ p) {
  extern __shared__ v4i lds[];
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const int row0 = (int)blockIdx.x * kRowsPerWave;
  const int F = net.F, A = net.A, D = net.D;
  const int d_tiles = D / 32, f_tiles = (F + 31) / 32, a_tiles = (A + 1 + 31) / 32;
  v4i* hbuf = lds;                                // [d_tiles][2][64]
  v4i* tbuf = lds + (size_t)d_tiles * 2 * kWave;  // [max(d_tiles, f_tiles)][2][64], then the head's rows
  const int stride = 32 * a_tiles + 1;
  int32_t* rows_io = reinterpret_cast<int32_t*>(tbuf);

  const bool words = (F & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 3) == 0;
  for (int kt = 0; kt < f_tiles; ++kt) {
    for (int rt = 0; rt < 2; ++rt) {
      const int row = row0 + 32 * rt + r;
      v4i frag = {0, 0, 0, 0};
      if (row < rows) {
        const unsigned char* xr = x + (size_t)row * F;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int k = 32 * kt + 8 * g + 4 * hh;
          uint32_t word = 0;
          if (words) {
            if (k < F) word = *reinterpret_cast<const uint32_t*>(xr + k);
          } else {
            for (int b = 0; b < 4; ++b) {
              if (k + b < F) word |= (uint32_t)xr[k + b] << (8 * b);
            }
          }
          frag[g] = (int)(word & 0x7f7f7f7fu);
        }
      }
      tbuf[(kt * 2 + rt) * kWave + lane] = frag;
    }
  }
  auto weights = [&](int i) { return reinterpret_cast<const v4i*>(net.image + net.w_off[i]); };
  auto biases = [&](int i) { return reinterpret_cast<const int32_t*>(net.image + net.b_off[i]); };
  auto keep = [&](int j) { return saved + ((size_t)j * rows + row0) * D; };
  const int left = rows - row0;
  TrainLayerTiles(weights(0), biases(0), net.shift[0], d_tiles, f_tiles, tbuf, hbuf, nullptr, keep(0), D, left, lane);
  for (int l = 0; l < net.L; ++l) {
    TrainLayerTiles(weights(1 + 2 * l), biases(1 + 2 * l), net.shift[1 + 2 * l], d_tiles, d_tiles, hbuf, tbuf, nullptr,
                    keep(1 + 2 * l), D, left, lane);
    TrainLayerTiles(weights(2 + 2 * l), biases(2 + 2 * l), net.shift[2 + 2 * l], d_tiles, d_tiles, tbuf, hbuf, hbuf,
                    keep(2 + 2 * l), D, left, lane);
  }
  const int head = 2 * net.L + 1;
  const v4i* w = weights(head);
  const int32_t* bias = biases(head);
  __syncthreads();  // (every lane is done with tbuf as fragments: the rows' image takes its place)
  for (int ot = 0; ot < a_tiles; ++ot) {
    v16i acc0, acc1;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc0[reg] = acc1[reg] = bias[32 * ot + TileRow(reg, hh)];
    for (int kt = 0; kt < d_tiles; ++kt) {
      const v4i a = w[((size_t)ot * d_tiles + kt) * kWave + lane];
      acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, hbuf[(kt * 2 + 0) * kWave + lane], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, hbuf[(kt * 2 + 1) * kWave + lane], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int n = 32 * ot + TileRow(reg, hh);  // (n < 32 a_tiles < stride)
      rows_io[r * stride + n] = acc0[reg];
      rows_io[(32 + r) * stride + n] = acc1[reg];
    }
  }
  __syncthreads();
  const int n_rows = left < kRowsPerWave ? left : kRowsPerWave;
  for (int i = lane; i < n_rows * (A + 1); i += kWave) {
    p[(size_t)row0 * (A + 1) + i] = rows_io[(i / (A + 1)) * stride + i % (A + 1)];
  }
}

size_t ForwardLds(int F, int A, int D) {
  const size_t d_tiles = (size_t)D / 32, f_tiles = ((size_t)F + 31) / 32, a_tiles = ((size_t)A + 1 + 31) / 32;
  const size_t frag = 2 * kWave * sizeof(v4i);
  return d_tiles * frag + std::max(std::max(d_tiles, f_tiles) * frag, (size_t)kRowsPerWave * (32 * a_tiles + 1) * 4);
}

// ---------------------------------------------------------------------------
// TrainSplitDp
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void TrainSplitDp(const float* __restrict__ dp, int rows, int N, int n16,
                                                     uint32_t* __restrict__ out) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (size_t)rows * n16) return;
  const size_t row = q / n16;
  const int n = (int)(q - row * n16);
  out[q] = n < N ? pgx::TrainSplit(dp[row * N + n]) : 0u;
}

// ---------------------------------------------------------------------------
// TrainBackRow
// ---------------------------------------------------------------------------
// eight split words -> the fragment of their hi halves and the fragment of their lo halves
__device__ inline void TearSplit(const v4i& a, const v4i& b, v8bf* hi, v8bf* lo) {
  v4i h, l;
  h[0] = (int)__builtin_amdgcn_perm((uint32_t)a[1], (uint32_t)a[0], 0x07060302u);
  h[1] = (int)__builtin_amdgcn_perm((uint32_t)a[3], (uint32_t)a[2], 0x07060302u);
  h[2] = (int)__builtin_amdgcn_perm((uint32_t)b[1], (uint32_t)b[0], 0x07060302u);
  h[3] = (int)__builtin_amdgcn_perm((uint32_t)b[3], (uint32_t)b[2], 0x07060302u);
  l[0] = (int)__builtin_amdgcn_perm((uint32_t)a[1], (uint32_t)a[0], 0x05040100u);
  l[1] = (int)__builtin_amdgcn_perm((uint32_t)a[3], (uint32_t)a[2], 0x05040100u);
  l[2] = (int)__builtin_amdgcn_perm((uint32_t)b[1], (uint32_t)b[0], 0x05040100u);
  l[3] = (int)__builtin_amdgcn_perm((uint32_t)b[3], (uint32_t)b[2], 0x05040100u);
  *hi = __builtin_bit_cast(v8bf, h);
  *lo = __builtin_bit_cast(v8bf, l);
}

struct RowArgs {
  int rows, D;
  const uint32_t* dz;      // [rows][ldn] split, the layer's dz
  int ldn, n16;            // its row length, and the layer's N up to a multiple of 16 (<= ldn)
  const uint16_t* wt;      // bf16 [D][n16]
  const uint32_t* res;     // null, or [rows][D] split: the dz of the block's second layer (may be `out`)
  float res_scale;         // 2^s of that layer
  const unsigned char* flags;  // [rows][D]: the saved bytes of the activation below
  float out_scale;         // 2^-s of the layer that made it
  uint32_t* out;           // [rows][D] split
  float* dx;               // kIn: [rows][D] float32 in place of res, flags and out; D is then any width, wt [D32][n16]
};

template <int T, bool kIn>
__global__ __launch_bounds__(256) void TrainBackRow(RowArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, hh = lane >> 5;
  const int row0 = (int)blockIdx.x * 64, tiles = (a.D + 31) / 32;
  v16f acc[T][2];
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[t][0][reg] = acc[t][1][reg] = 0.0f;
  }
  for (int ns = 0; ns < a.n16 / 16; ++ns) {
    v8bf hi[2], lo[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int row = row0 + 32 * rt + c;
      v4i w0 = {0, 0, 0, 0}, w1 = {0, 0, 0, 0};
      if (row < a.rows) {
        const v4i* src = reinterpret_cast<const v4i*>(a.dz + (size_t)row * a.ldn + 16 * ns + 8 * hh);
        w0 = src[0], w1 = src[1];
      }
      TearSplit(w0, w1, &hi[rt], &lo[rt]);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int kt = wave + 4 * t;
      if (kt < tiles) {  // (uniform in the wave)
        const v4i raw = *reinterpret_cast<const v4i*>(a.wt + (size_t)(32 * kt + c) * a.n16 + 16 * ns + 8 * hh);
        const v8bf b = __builtin_bit_cast(v8bf, raw);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          acc[t][rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hi[rt], b, acc[t][rt], 0, 0, 0);
          acc[t][rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lo[rt], b, acc[t][rt], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int kt = wave + 4 * t;
    if (kt >= tiles) continue;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = row0 + 32 * rt + TileRow(reg, hh);
        if (row >= a.rows) continue;
        const size_t at = (size_t)row * a.D + 32 * kt + c;
        float g = acc[t][rt][reg];
        if constexpr (kIn) {
          if (32 * kt + c < a.D) a.dx[at] = g;
          continue;
        }
        if (a.res != nullptr) g = g + pgx::TrainJoin(a.res[at]) * a.res_scale;
        a.out[at] = pgx::TrainSplit((a.flags[at] & 128) != 0 ? 0.0f : g * a.out_scale);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// TrainReduce, TrainSum
// ---------------------------------------------------------------------------
constexpr int kRedRows = 64, kRedPitch = 72;  // rows of a pass through LDS; elements of an LDS row (144 bytes)
static_assert(pgx::kTrainRunRows == 2 * kRedRows, "a run is two passes");

struct RedArgs {
  int rows, N, K;
  const uint32_t* dz;       // [rows][ldn] split
  int ldn;                  // a multiple of 4, >= N; words behind N are zero
  const unsigned char* x;   // [rows][K]: saved bytes, or the input
  int slice_rows;
  float* ws;                // [slices][N][K + 1]
};

__global__ __launch_bounds__(256) void TrainReduce(RedArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t zh[64 * kRedPitch], zl[64 * kRedPitch], xt[64 * kRedPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, hh = lane >> 5;
  const int nt = wave >> 1, kt = wave & 1;
  const int k0 = (int)blockIdx.x * 64, n0 = (int)blockIdx.y * 64, slice = blockIdx.z;
  const int begin = slice * a.slice_rows, end = min(a.rows, begin + a.slice_rows);
  const bool with_db = blockIdx.x == 0 && kt == 0;
  const bool x_words = (a.K & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 3) == 0;
  v4i ones_raw = {0x3f803f80, 0x3f803f80, 0x3f803f80, 0x3f803f80};
  const v8bf ones = __builtin_bit_cast(v8bf, ones_raw);
  v16f acc, total, acc_b, total_b;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) acc[reg] = total[reg] = acc_b[reg] = total_b[reg] = 0.0f;
  int pass = 0;
  for (int base = begin; base < end; base += kRedRows, ++pass) {
    __syncthreads();  // (the last pass's fragments are read)
    // dz: 64 rows x 64 n, four words at a time, transposed into the hi and lo planes
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int e = tid + 256 * it, rl = e >> 4, n4 = (e & 15) * 4;
      const int row = base + rl;
      v4i wds = {0, 0, 0, 0};
      if (row < end && n0 + n4 < a.ldn) wds = *reinterpret_cast<const v4i*>(a.dz + (size_t)row * a.ldn + n0 + n4);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        zh[(n4 + q) * kRedPitch + rl] = (uint16_t)((uint32_t)wds[q] >> 16);
        zl[(n4 + q) * kRedPitch + rl] = (uint16_t)((uint32_t)wds[q] & 0xffffu);
      }
    }
    // x: 64 rows x 64 k bytes, sixteen a thread
    {
      const int rl = tid >> 2, k16 = (tid & 3) * 16;
      const int row = base + rl;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int k = k0 + k16 + 4 * q4;
        uint32_t word = 0;
        if (row < end) {
          const unsigned char* xr = a.x + (size_t)row * a.K;
          if (x_words) {
            if (k < a.K) word = *reinterpret_cast<const uint32_t*>(xr + k);
          } else {
            for (int b = 0; b < 4; ++b) {
              if (k + b < a.K) word |= (uint32_t)xr[k + b] << (8 * b);
            }
          }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float v = (float)((word >> (8 * b)) & 127u);
          xt[(k16 + 4 * q4 + b) * kRedPitch + rl] = (uint16_t)((uint32_t)pgx::NetFloatBits(v) >> 16);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int step = 0; step < kRedRows / 16; ++step) {
      const int at = 16 * step + 8 * hh;
      const v8bf a_hi = __builtin_bit_cast(v8bf, *reinterpret_cast<const v4i*>(&zh[(32 * nt + c) * kRedPitch + at]));
      const v8bf a_lo = __builtin_bit_cast(v8bf, *reinterpret_cast<const v4i*>(&zl[(32 * nt + c) * kRedPitch + at]));
      const v8bf b = __builtin_bit_cast(v8bf, *reinterpret_cast<const v4i*>(&xt[(32 * kt + c) * kRedPitch + at]));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b, acc, 0, 0, 0);
      if (with_db) {
        acc_b = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, ones, acc_b, 0, 0, 0);
        acc_b = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, ones, acc_b, 0, 0, 0);
      }
    }
    if ((pass & 1) != 0 || base + kRedRows >= end) {  // a run of 128 rows, or the slice's last
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        total[reg] = total[reg] + acc[reg], acc[reg] = 0.0f;
        total_b[reg] = total_b[reg] + acc_b[reg], acc_b[reg] = 0.0f;
      }
    }
  }
  float* ws = a.ws + (size_t)slice * a.N * (a.K + 1);
  const int k = k0 + 32 * kt + c;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int n = n0 + 32 * nt + TileRow(reg, hh);
    if (n >= a.N) continue;
    if (k < a.K) ws[(size_t)n * (a.K + 1) + k] = total[reg];
    if (with_db && c == 0) ws[(size_t)n * (a.K + 1) + a.K] = total_b[reg];
  }
}

__global__ __launch_bounds__(256) void TrainSum(const float* __restrict__ ws, int slices, int N, int K,
                                                 float* __restrict__ dw, int ldw, float* __restrict__ db) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= N * (K + 1)) return;
  float s = 0.0f;
  for (int i = 0; i < slices; ++i) s = s + ws[(size_t)i * N * (K + 1) + q];
  const int n = q / (K + 1), k = q - n * (K + 1);
  if (k < K) {
    dw[(size_t)n * ldw + k] = s;
  } else {
    db[n] = s;
  }
}

size_t Align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

// ---------------------------------------------------------------------------
// the launches the convolutional training handle shares (engine.h)
// ---------------------------------------------------------------------------
void TrainSplitLaunch(const float* dp, int rows, int N, int n16, uint32_t* out, hipStream_t stream) {
  const size_t cells = (size_t)rows * n16;
  hipLaunchKernelGGL(TrainSplitDp, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, dp, rows, N, n16, out);
}

void TrainReduceLaunch(int rows, int N, int K, const uint32_t* dz, int ldn, const unsigned char* x, float* ws,
                       float* dw, float* db, hipStream_t stream) {
  TrainReduceLaunchLd(rows, N, K, dz, ldn, x, ws, dw, K, db, stream);
}

void TrainReduceLaunchLd(int rows, int N, int K, const uint32_t* dz, int ldn, const unsigned char* x, float* ws,
                         float* dw, int ldw, float* db, hipStream_t stream) {
  const pgx::TrainSlicing s = pgx::TrainSlices(rows, N, K);
  RedArgs r{rows, N, K, dz, ldn, x, s.slice_rows, ws};
  hipLaunchKernelGGL(TrainReduce, dim3((K + 63) / 64, (N + 63) / 64, s.slices), dim3(256), 0, stream, r);
  hipLaunchKernelGGL(TrainSum, dim3((N * (K + 1) + 255) / 256), dim3(256), 0, stream, ws, s.slices, N, K, dw, ldw, db);
}

void TrainSumLaunch(const float* ws, int slices, int N, int K, float* dw, float* db, hipStream_t stream) {
  hipLaunchKernelGGL(TrainSum, dim3((N * (K + 1) + 255) / 256), dim3(256), 0, stream, ws, slices, N, K, dw, K, db);
}

// ---------------------------------------------------------------------------
// the handle (engine.h: NetTrain)
// ---------------------------------------------------------------------------
struct NetTrain::Layout {
  uint32_t w_off[kL], b_off[kL], wt_off[kL];
  size_t image, wt, x, saved, dz_a, dz_b, dp, ws;  // byte offsets into the block
};

NetTrain::NetTrain(int device, int F, int A, int D, int L, long long max_rows)
    : device_(device), F_(F), A_(A), D_(D), L_(L), max_rows_((int)max_rows), at_(new Layout()) {
  char err[200];
  if (!pgx::TrainCheck(F, A, D, L, max_rows, err, sizeof(err))) throw std::invalid_argument(err);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
  if (device < 0 || device >= count) {
    throw std::invalid_argument("net_train_create: device = " + std::to_string(device) + " must be 0 .. " +
                                std::to_string(count - 1));
  }
  const int layers = 2 * L + 2;
  size_t image = 0, wt = 0, ws = 0;
  for (int i = 0; i < layers; ++i) {
    const size_t N = i == layers - 1 ? A + 1 : D, K = i == 0 ? F : D;
    const size_t n_tiles = (N + 31) / 32, k_tiles = (K + 31) / 32;
    at_->w_off[i] = (uint32_t)image, image += n_tiles * k_tiles * 1024;
    at_->b_off[i] = (uint32_t)image, image += n_tiles * 32 * 4;
    at_->wt_off[i] = (uint32_t)wt, wt += 32 * k_tiles * ((N + 15) / 16 * 16);
    ws = std::max(ws, (size_t)pgx::TrainMostSlices(max_rows_, (int)N, (int)K) * N * (K + 1) * 4);
  }
  const size_t rows = (size_t)max_rows_, n16 = ((size_t)A + 1 + 15) / 16 * 16;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += Align256(bytes);
    return here;
  };
  at_->image = take(image), at_->wt = take(2 * wt), at_->x = take(rows * F);
  at_->saved = take((size_t)(2 * L + 1) * rows * D);
  at_->dz_a = take(rows * D * 4), at_->dz_b = take(rows * D * 4), at_->dp = take(rows * n16 * 4), at_->ws = take(ws);
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  try {
    mem_.Alloc(at);
  } catch (...) {
    (void)hipSetDevice(before);
    throw;
  }
  const size_t lds = ForwardLds(F, A, D);
  if (lds > 48 * 1024) {
    EPA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&TrainForward),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  EPA_HIP(hipSetDevice(before));
}

NetTrain::~NetTrain() {
  int before = 0;
  if (hipGetDevice(&before) != hipSuccess) return;
  (void)hipSetDevice(device_);
  mem_.Free();
  (void)hipSetDevice(before);
}

void NetTrain::Forward(hipStream_t stream, int rows, const void* const* d_w, const void* const* d_b,
                       const int32_t* shifts, const void* d_x, void* d_p) {
  char err[200];
  if (d_w == nullptr || d_b == nullptr || shifts == nullptr || d_x == nullptr || d_p == nullptr) {
    throw std::invalid_argument("net_train_forward: null argument");
  }
  if (rows < 1 || rows > max_rows_) {
    throw std::invalid_argument("net_train_forward: rows = " + std::to_string(rows) + " must be 1 .. " +
                                std::to_string(max_rows_) + " (the handle's max_rows)");
  }
  if (!pgx::TrainCheckShifts(L_, shifts, err, sizeof(err))) throw std::invalid_argument(err);
  const int layers = 2 * L_ + 2;
  PackArgs pack{};
  FwdNet net{};
  pack.layers = layers;
  pack.image = mem_.p + at_->image;
  pack.wt = reinterpret_cast<uint16_t*>(mem_.p + at_->wt);
  net.F = F_, net.A = A_, net.D = D_, net.L = L_, net.image = pack.image;
  for (int i = 0; i < layers; ++i) {
    if (d_w[i] == nullptr || d_b[i] == nullptr) throw std::invalid_argument("net_train_forward: null argument");
    pack.w[i] = static_cast<const signed char*>(d_w[i]);
    pack.b[i] = static_cast<const int32_t*>(d_b[i]);
    pack.n_out[i] = i == layers - 1 ? A_ + 1 : D_;
    pack.k_in[i] = i == 0 ? F_ : D_;
    pack.w_off[i] = net.w_off[i] = at_->w_off[i];
    pack.b_off[i] = net.b_off[i] = at_->b_off[i];
    pack.wt_off[i] = at_->wt_off[i];
    net.shift[i] = shift_[i] = shifts[i];
  }
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  rows_ = back_rows_ = 0;  // (a forward that fails leaves nothing to go back through)
  hipLaunchKernelGGL(TrainPack, dim3(64, layers), dim3(256), 0, stream, pack);
  unsigned char* x = reinterpret_cast<unsigned char*>(mem_.p + at_->x);
  const hipError_t copied = hipMemcpyAsync(x, d_x, (size_t)rows * F_, hipMemcpyDeviceToDevice, stream);
  if (copied == hipSuccess) {
    hipLaunchKernelGGL(TrainForward, dim3((rows + kRowsPerWave - 1) / kRowsPerWave), dim3(kWave),
                       ForwardLds(F_, A_, D_), stream, net, rows, x,
                       reinterpret_cast<unsigned char*>(mem_.p + at_->saved), static_cast<int32_t*>(d_p));
  }
  const hipError_t launched = hipGetLastError();
  (void)hipSetDevice(before);
  EPA_HIP(copied);
  EPA_HIP(launched);
  rows_ = rows;
}

void NetTrain::Backward(hipStream_t stream, int rows, const void* d_dp, void* const* d_dw, void* const* d_db) {
  if (d_dp == nullptr || d_dw == nullptr || d_db == nullptr) {
    throw std::invalid_argument("net_train_backward: null argument");
  }
  const int layers = 2 * L_ + 2;
  for (int i = 0; i < layers; ++i) {
    if (d_dw[i] == nullptr || d_db[i] == nullptr) throw std::invalid_argument("net_train_backward: null argument");
  }
  if (rows_ == 0) throw std::invalid_argument("net_train_backward: no forward has been made with this handle");
  if (rows != rows_) {
    throw std::invalid_argument("net_train_backward: rows = " + std::to_string(rows) + ", but the last forward had " +
                                std::to_string(rows_));
  }
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  const unsigned char* x = reinterpret_cast<const unsigned char*>(mem_.p + at_->x);
  const unsigned char* saved = reinterpret_cast<const unsigned char*>(mem_.p + at_->saved);
  auto activation = [&](int j) { return saved + (size_t)j * rows * D_; };
  uint32_t* buf_a = reinterpret_cast<uint32_t*>(mem_.p + at_->dz_a);
  uint32_t* buf_b = reinterpret_cast<uint32_t*>(mem_.p + at_->dz_b);
  uint32_t* dp = reinterpret_cast<uint32_t*>(mem_.p + at_->dp);
  float* ws = reinterpret_cast<float*>(mem_.p + at_->ws);
  const uint16_t* wt = reinterpret_cast<const uint16_t*>(mem_.p + at_->wt);
  const int n16 = (A_ + 1 + 15) / 16 * 16;

  // dW and db of layer i from its dz
  auto reduce = [&](int i, const uint32_t* dz, int ldn) {
    const int N = i == layers - 1 ? A_ + 1 : D_, K = i == 0 ? F_ : D_;
    TrainReduceLaunch(rows, N, K, dz, ldn, i == 0 ? x : activation(i - 1), ws, static_cast<float*>(d_dw[i]),
                      static_cast<float*>(d_db[i]), stream);
  };
  // the dz of layer i - 1 from the dz of layer i >= 1
  auto below = [&](int i, const uint32_t* dz, int ldn, int width, const uint32_t* res, int res_layer, uint32_t* out) {
    RowArgs r{rows, D_, dz, ldn, width, wt + at_->wt_off[i], res,
              res != nullptr ? (float)(1 << shift_[res_layer]) : 0.0f, activation(i - 1),
              1.0f / (float)(1 << shift_[i - 1]), out, nullptr};
    const dim3 grid((rows + 63) / 64), block(256);
    if (D_ <= 128) {
      hipLaunchKernelGGL((TrainBackRow<1, false>), grid, block, 0, stream, r);
    } else if (D_ <= 256) {
      hipLaunchKernelGGL((TrainBackRow<2, false>), grid, block, 0, stream, r);
    } else if (D_ <= 384) {
      hipLaunchKernelGGL((TrainBackRow<3, false>), grid, block, 0, stream, r);
    } else {
      hipLaunchKernelGGL((TrainBackRow<4, false>), grid, block, 0, stream, r);
    }
  };
  TrainSplitLaunch(static_cast<const float*>(d_dp), rows, A_ + 1, n16, dp, stream);
  reduce(layers - 1, dp, n16);
  below(layers - 1, dp, n16, n16, nullptr, 0, buf_a);
  for (int l = L_ - 1; l >= 0; --l) {
    reduce(2 + 2 * l, buf_a, D_);
    below(2 + 2 * l, buf_a, D_, D_, nullptr, 0, buf_b);
    reduce(1 + 2 * l, buf_b, D_);
    below(1 + 2 * l, buf_b, D_, D_, buf_a, 2 + 2 * l, buf_a);  // (in place: a lane reads its word, then writes it)
  }
  reduce(0, buf_a, D_);
  const hipError_t launched = hipGetLastError();
  (void)hipSetDevice(before);
  EPA_HIP(launched);
  back_rows_ = rows;
}

void NetTrain::InputGrad(hipStream_t stream, int rows, void* d_dx) {
  if (d_dx == nullptr) throw std::invalid_argument("net_train_input_grad: null argument");
  if (back_rows_ == 0) {
    throw std::invalid_argument("net_train_input_grad: no backward has been made since the last forward");
  }
  if (rows != back_rows_) {
    throw std::invalid_argument("net_train_input_grad: rows = " + std::to_string(rows) + ", but the last backward had " +
                                std::to_string(back_rows_));
  }
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  // (the last Backward left the split dz of layer 0 in the first buffer)
  RowArgs r{rows, F_, reinterpret_cast<const uint32_t*>(mem_.p + at_->dz_a), D_, D_,
            reinterpret_cast<const uint16_t*>(mem_.p + at_->wt) + at_->wt_off[0], nullptr, 0.0f, nullptr, 0.0f, nullptr,
            static_cast<float*>(d_dx)};
  const dim3 grid((rows + 63) / 64), block(256);
  if (F_ <= 128) {
    hipLaunchKernelGGL((TrainBackRow<1, true>), grid, block, 0, stream, r);
  } else if (F_ <= 256) {
    hipLaunchKernelGGL((TrainBackRow<2, true>), grid, block, 0, stream, r);
  } else if (F_ <= 384) {
    hipLaunchKernelGGL((TrainBackRow<3, true>), grid, block, 0, stream, r);
  } else {
    hipLaunchKernelGGL((TrainBackRow<4, true>), grid, block, 0, stream, r);
  }
  const hipError_t launched = hipGetLastError();
  (void)hipSetDevice(before);
  EPA_HIP(launched);
}

}  // namespace epa
