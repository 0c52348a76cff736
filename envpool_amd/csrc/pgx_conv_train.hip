// PGX convolutional network, training, on the matrix cores (pgx_conv_train.hip.h is the contract; DESIGN.md "PGX
// convolutional network: training").  Five kernels of its own, the dense TrainSplitDp / TrainReduce / TrainSum of
// pgx_train.hip for the reduce layer and the head, and the handle that owns their memory.
//
// ConvTrainPack, once per forward: the caller's quantised weights, int8 in the blob's order on the device, into
//   ConvBuildImage's 1 KiB (output tile, tap, k-step) fragments with the bias padded to whole tiles, and for every
//   layer but the stem the bf16 operand its dx reads (an int8 is exact in bf16): a 3x3 layer's is per tap the
//   transpose [c][n] with the tap mirrored, wt[tap][c][n] = W[n][8 - tap][c]; the reduce layer's [D][P16] (P16 = P up
//   to a multiple of 16, zeros behind P); the head's [H W P16][n16] with zero rows behind P, so that its dx leaves as
//   the reduce layer's dz [rows H W][P16].
// ConvTrainForward: PgxConvEval's tiling (pgx_conv.hip has the details) -- four waves and a group of G boards per
//   block, h and t in LDS as [board][(H + 2)(W + 2)][D + 16 bytes] with a zero halo, records in the (half, dword, byte)
//   tile order so that a lane's result is one 128-bit LDS store and a B fragment one 128-bit load, the weights as the A
//   operand of v_mfma_i32_32x32x32_i8, an item = one output tile against up to four column tiles, G from the LDS
//   budget.  The epilogue also stores the lane's four words, bit 7 of a byte set where the clamp changed the value, to
//   the saved bytes in their natural order (channels 32 ot + 8 g + 4 hh .. + 3 are word 2 g of the lane's 32 bytes);
//   the copy in LDS keeps bit 7 clear.  The reduce layer scatters its bytes to g in LDS (the head's B fragment, board
//   = column) and to the saved g.  The head's int32 p leaves through LDS as [rows][A + 1].  Barriers: after zeroing,
//   after the input, after every layer, after the head's integers.
// ConvTrainRow: dx = dz W of a dense layer whose output width need not be a multiple of 32 (the head: H W P16 columns;
//   the reduce layer: D).  64 rows a block, dz the A operand torn into hi and lo as in TrainBackRow, wave w the column
//   tiles w, w + 4, .. one after another; the epilogue applies the saved mask bit and the 2^-s and stores the split.
// ConvTrainDx: dx of a 3x3 layer.  A block keeps G boards of split dz in LDS as [board][(H + 2)(W + 2)][D + 4 words]
//   with a zero halo (zeroed, barrier, live records copied in 128-bit pieces, barrier; nothing is written afterwards),
//   so a tap is an address offset and off-board gradient is 0 without a branch.  An item is one 32-channel tile of the
//   INPUT channels c against up to four 32-square column tiles; items go round the four waves.  dz is the A operand
//   (M = 32 squares): lane (r, hh) reads the 8 split words of its square's record at tap offset + 16 ns + 8 hh as two
//   128-bit LDS reads and tears them into a hi and a lo fragment; the mirrored W^T is the B operand (N = 32 channels
//   c), one 128-bit global load per (tap, n-step) shared by the item's column tiles.  One accumulator per output tile
//   over all 9 taps and D / 16 n-steps (the contract's d = 4608).  The epilogue is the dense one: the residual term
//   times 2^s (read before the same lane overwrites it: the kernel may run in place on the residual), the saved mask
//   bit, the 2^-s of the layer below, split, store -- 128 bytes of a record per register.
// ConvTrainDw: dW and db of a 3x3 layer.  Grid (tile of 64 input channels, tile of 64 output channels, slice of
//   boards), four waves with one 32 x 32 tile each.  The contraction index is the position, so a PASS of boards goes
//   through LDS transposed, as in TrainReduce: dz as two bf16 planes [n][u] and the input as bf16 [c][margin + u],
//   where u runs over the pass's haloed positions (ConvTrainPassOf: rows of W + 1, boards of (H + 1)(W + 1), every
//   halo cell shared and zero).  Then the nine taps are nine shifted reads of the same input rows against ONE dz
//   fragment: the lane reads five dwords at the even element below its shifted start and funnels them by 16 bits if
//   the start is odd (v_alignbit), since an LDS read wider than a dword must be aligned.  The taps are taken a row of
//   three at a time (three accumulators of 16 registers), each folded after the pass into one of nine second
//   accumulators (the contract's error count); the waves of channel tile 0 add two MFMAs against a fragment of ones
//   for db, once per step, not per tap.  The slice's partial sums go to the workspace [slice][N][9 K + 1], db in the
//   last column; TrainSum adds the slices in ascending order into dW [N][3][3][K] and db.
// Registers and LDS of each kernel as built are in DESIGN.md; no kernel uses scratch.
//
// All launches of a call are enqueued from one C++ function on the caller's stream; nothing waits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "engine.h"
#include "pgx_conv_train.hip.h"

namespace epa {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

constexpr int kWave = 64, kWaves = 4, kThreads = kWave * kWaves;
constexpr int kFwdMaxBoards = 32;   // the head's columns are one tile
constexpr int kDxMaxBoards = 128;
constexpr int kChunk = 4;           // column tiles of an item
constexpr size_t kStaticLds = 1024;  // an upper bound of a kernel's static LDS
constexpr int kL = pgx::kConvMaxLayers;
static_assert(kL == kConvImageLayers, "engine.h: ConvTrain");

// the row (within its 32-row tile) of accumulator register `reg` of a lane of half `hh`: the C/D map of both MFMAs
__device__ inline int TileRow(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }
// where element k of a row lies in the (half, dword, byte) order of its 32-element tile
__host__ __device__ inline int TilePlace(int k) { return (k & ~31) + 16 * ((k >> 2) & 1) + 4 * ((k >> 3) & 3) + (k & 3); }

__device__ inline uint16_t Bf16OfSmall(float v) { return (uint16_t)((uint32_t)pgx::NetFloatBits(v) >> 16); }  // (7 bits)

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

// ---------------------------------------------------------------------------
// ConvTrainPack
// ---------------------------------------------------------------------------
struct PackArgs {
  int layers, S, P, P16, n16;  // n16: A + 1 up to a multiple of 16
  const signed char* w[kL];
  const int32_t* b[kL];
  int n_out[kL], taps[kL], k_in[kL];
  char* image;   // the forward's fragments and biases
  uint16_t* wt;  // the bf16 operands of dx
  uint32_t w_off[kL], b_off[kL], wt_off[kL];  // bytes into image; elements into wt
};

__global__ __launch_bounds__(256) void ConvTrainPack(PackArgs a) {
  const int i = blockIdx.y;
  const int N = a.n_out[i], T = a.taps[i], K = a.k_in[i];
  const int n_tiles = (N + 31) / 32, k_tiles = (K + 31) / 32;
  const int frag_bytes = n_tiles * T * k_tiles * 1024, bias_words = n_tiles * 32;
  const bool head = i == a.layers - 1, reduce = i == a.layers - 2;
  const int wt_elems = i == 0 ? 0 : (head ? a.S * a.P16 * a.n16 : (reduce ? K * a.P16 : 9 * K * N));
  const signed char* __restrict__ w = a.w[i];
  for (int q = blockIdx.x * 256 + threadIdx.x; q < frag_bytes + bias_words + wt_elems; q += gridDim.x * 256) {
    if (q < frag_bytes) {
      const int e = q & 15, lane = (q >> 4) & 63, frag = q >> 10;
      const int kt = frag % k_tiles, tap = (frag / k_tiles) % T, ot = frag / (k_tiles * T);
      const int n = 32 * ot + (lane & 31), k = 32 * kt + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
      a.image[a.w_off[i] + q] = n < N && k < K ? (char)w[((size_t)n * T + tap) * K + k] : (char)0;
    } else if (q < frag_bytes + bias_words) {
      const int n = q - frag_bytes;
      reinterpret_cast<int32_t*>(a.image + a.b_off[i])[n] = n < N ? a.b[i][n] : 0;
    } else {
      const int t = q - frag_bytes - bias_words;
      float v = 0.0f;
      if (head) {
        const int kk = t / a.n16, n = t - kk * a.n16, sq = kk / a.P16, pl = kk - sq * a.P16;
        if (n < N && pl < a.P) v = (float)w[(size_t)n * K + sq * a.P + pl];
      } else if (reduce) {
        const int c = t / a.P16, pl = t - c * a.P16;
        if (pl < N) v = (float)w[(size_t)pl * K + c];
      } else {  // (K = N = D)
        const int n = t % N, c = (t / N) % K, tap = t / (N * K);
        v = (float)w[((size_t)n * 9 + (8 - tap)) * K + c];
      }
      a.wt[a.wt_off[i] + t] = Bf16OfSmall(v);
    }
  }
}

// ---------------------------------------------------------------------------
// ConvTrainForward
// ---------------------------------------------------------------------------
struct FwdDev {
  int H, W, C, A, D, L, P, G;
  const char* base;
  uint32_t w_off[kL], b_off[kL];
  int32_t shift[kL];
};

// The block's LDS, in bytes (pgx_conv.hip: ConvLayout): h at 0 and t at `second`, `buf` bytes each; the head's rows
// overlay h, the reduce layer's image g overlays t.
struct FwdLds {
  int stride, records, buf, kp, g_stride, io_stride, second, total;
};
__host__ __device__ inline FwdLds FwdLayout(int H, int W, int D, int P, int A, int G) {
  FwdLds l;
  l.stride = D + 16;
  l.records = (H + 2) * (W + 2);
  l.buf = G * l.records * l.stride;
  l.kp = (H * W * P + 31) & ~31;
  l.g_stride = l.kp + 16;
  l.io_stride = 32 * ((A + 1 + 31) / 32) + 1;
  const int io = (G * l.io_stride * 4 + 15) & ~15, g = (G * l.g_stride + 15) & ~15;
  l.second = l.buf > io ? l.buf : io;
  l.total = l.second + (l.buf > g ? l.buf : g);
  return l;
}

struct FwdGroup {
  int first, boards, cols;  // the group's first row, its live boards, their squares: the live columns
  int S, W, P, D;
  FwdLds lds;
};

enum { kEpiAct = 0, kEpiResidual = 1, kEpiReduce = 2 };

// One item: output tile `ot` of a layer against the CT column tiles from `tile0` on (pgx_conv.hip: ConvItem), which
// also stores the saved bytes: `keep` is the activation's (or g's) first byte.
template <int CT>
__device__ inline void FwdItem(const FwdGroup& grp, const v4i* __restrict__ w, const int32_t* __restrict__ bias,
                               int shift, int taps, int k_tiles, int ot, int tile0, const char* in, char* out, int epi,
                               unsigned char* __restrict__ keep, int lane) {
  const int r = lane & 31, hh = lane >> 5;
  const int stride = grp.lds.stride, row_bytes = (grp.W + 2) * stride;
  int addr[CT], board[CT], square[CT];
  bool live[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int col = 32 * (tile0 + c) + r;
    live[c] = col < grp.cols;
    const int cc = live[c] ? col : 0;
    board[c] = cc / grp.S;
    square[c] = cc - board[c] * grp.S;
    const int y = square[c] / grp.W, x = square[c] - y * grp.W;
    addr[c] = (board[c] * grp.lds.records + (y + 1) * (grp.W + 2) + (x + 1)) * stride + 16 * hh;
  }
  v16i acc[CT];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int32_t b = bias[32 * ot + TileRow(reg, hh)];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c][reg] = b;
  }
  const v4i* wt = w + (size_t)ot * taps * k_tiles * kWave + lane;
  for (int tap = 0; tap < taps; ++tap) {
    const int off = taps == 1 ? 0 : (tap / 3 - 1) * row_bytes + (tap % 3 - 1) * stride;
    for (int kt = 0; kt < k_tiles; ++kt) {
      const v4i a = wt[(size_t)(tap * k_tiles + kt) * kWave];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const v4i b = *reinterpret_cast<const v4i*>(in + addr[c] + off + 32 * kt);
        acc[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[c], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    if (!live[c]) continue;  // a column past the group's squares stores nothing
    const size_t pos = (size_t)(grp.first + board[c]) * grp.S + square[c];
    if (epi == kEpiReduce) {
      char* g = out + board[c] * grp.lds.g_stride;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int q = TileRow(reg, hh);
        if (q < grp.P) {
          const int32_t v = pgx::NetRs(acc[c][reg], shift), act = pgx::NetAct(v);
          g[TilePlace(square[c] * grp.P + q)] = (char)act;
          keep[pos * grp.P + q] = (unsigned char)(act | (act != v ? 128 : 0));
        }
      }
      continue;
    }
    v4i* dst = reinterpret_cast<v4i*>(out + addr[c] + 32 * ot);
    v4i old = {0, 0, 0, 0};
    if (epi == kEpiResidual) old = *dst;
    v4i packed;
    uint32_t* kept = reinterpret_cast<uint32_t*>(keep + pos * grp.D + 32 * ot + 4 * hh);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint32_t word = 0, flags = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        int32_t v = pgx::NetRs(acc[c][4 * g + b], shift);
        if (epi == kEpiResidual) v += (int32_t)(((uint32_t)old[g] >> (8 * b)) & 255u);
        const int32_t act = pgx::NetAct(v);
        word |= (uint32_t)act << (8 * b);
        flags |= (act != v ? 128u : 0u) << (8 * b);
      }
      packed[g] = (int)word;
      kept[2 * g] = word | flags;  // channels 32 ot + 8 g + 4 hh .. + 3
    }
    *dst = packed;
  }
}

__device__ inline void FwdLayerPass(const FwdGroup& grp, const FwdDev& net, int layer, int n_tiles, int taps,
                                    int k_tiles, const char* in, char* out, int epi, unsigned char* keep, int wave,
                                    int lane) {
  const v4i* w = reinterpret_cast<const v4i*>(net.base + net.w_off[layer]);
  const int32_t* bias = reinterpret_cast<const int32_t*>(net.base + net.b_off[layer]);
  const int shift = net.shift[layer];
  const int col_tiles = (grp.cols + 31) / 32, chunks = (col_tiles + kChunk - 1) / kChunk;
  for (int item = wave; item < n_tiles * chunks; item += kWaves) {
    const int ot = item / chunks, tile0 = kChunk * (item - ot * chunks);
    const int left = col_tiles - tile0;
    if (left >= 4) {
      FwdItem<4>(grp, w, bias, shift, taps, k_tiles, ot, tile0, in, out, epi, keep, lane);
    } else if (left == 3) {
      FwdItem<3>(grp, w, bias, shift, taps, k_tiles, ot, tile0, in, out, epi, keep, lane);
    } else if (left == 2) {
      FwdItem<2>(grp, w, bias, shift, taps, k_tiles, ot, tile0, in, out, epi, keep, lane);
    } else {
      FwdItem<1>(grp, w, bias, shift, taps, k_tiles, ot, tile0, in, out, epi, keep, lane);
    }
  }
}

__global__ __launch_bounds__(kThreads, 2) void ConvTrainForward(FwdDev net, int rows,
                                                                 const unsigned char* __restrict__ x,
                                                                 unsigned char* __restrict__ saved,
                                                                 unsigned char* __restrict__ gsaved,
                                                                 int32_t* __restrict__ p) {
  extern __shared__ v4i lds4[];
  char* lds = reinterpret_cast<char*>(lds4);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  FwdGroup grp;
  grp.first = (int)blockIdx.x * net.G;
  if (grp.first >= rows) return;  // (the whole block, before any barrier)
  grp.boards = rows - grp.first < net.G ? rows - grp.first : net.G;
  grp.S = net.H * net.W, grp.W = net.W, grp.P = net.P, grp.D = net.D;
  grp.cols = grp.boards * grp.S;
  grp.lds = FwdLayout(net.H, net.W, net.D, net.P, net.A, net.G);
  const int A = net.A, io_stride = grp.lds.io_stride;
  char* hbuf = lds;
  char* tbuf = lds + grp.lds.second;
  int32_t* rows_io = reinterpret_cast<int32_t*>(lds);

  for (int i = tid; i < grp.lds.total / 16; i += kThreads) lds4[i] = v4i{0, 0, 0, 0};
  __syncthreads();  // the zeros lie before the input is written over them
  const int C = net.C;
  for (int i = tid; i < grp.cols; i += kThreads) {
    const int b = i / grp.S, sq = i - b * grp.S, y = sq / grp.W, xx = sq - y * grp.W;
    const unsigned char* src = x + ((size_t)(grp.first + b) * grp.S + sq) * C;
    uint32_t word[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < pgx::kConvMaxChannels; ++c) {
      if (c < C) word[TilePlace(c) >> 2] |= (uint32_t)(src[c] & 127u) << (8 * (TilePlace(c) & 3));
    }
    v4i* dst = reinterpret_cast<v4i*>(tbuf + (b * grp.lds.records + (y + 1) * (grp.W + 2) + (xx + 1)) * grp.lds.stride);
    dst[0] = v4i{(int)word[0], (int)word[1], (int)word[2], (int)word[3]};
    dst[1] = v4i{(int)word[4], (int)word[5], (int)word[6], (int)word[7]};
  }
  __syncthreads();  // the input is complete
  const int d_tiles = net.D / 32;
  auto keep = [&](int j) { return saved + (size_t)j * rows * grp.S * net.D; };
  FwdLayerPass(grp, net, 0, d_tiles, 9, 1, tbuf, hbuf, kEpiAct, keep(0), wave, lane);
  __syncthreads();  // a layer's output is complete before it is read
  for (int l = 0; l < net.L; ++l) {
    FwdLayerPass(grp, net, 1 + 2 * l, d_tiles, 9, d_tiles, hbuf, tbuf, kEpiAct, keep(1 + 2 * l), wave, lane);
    __syncthreads();
    FwdLayerPass(grp, net, 2 + 2 * l, d_tiles, 9, d_tiles, tbuf, hbuf, kEpiResidual, keep(2 + 2 * l), wave, lane);
    __syncthreads();
  }
  // (g takes t's place; what t leaves in g's padding meets zero weights in the head)
  FwdLayerPass(grp, net, 2 * net.L + 1, 1, 1, d_tiles, hbuf, tbuf, kEpiReduce, gsaved, wave, lane);
  __syncthreads();  // g is complete, and every wave is done with h: the head's rows take its place
  {
    const int head = 2 * net.L + 2, a_tiles = (A + 1 + 31) / 32, k_tiles = grp.lds.kp / 32;
    const int r = lane & 31, hh = lane >> 5;
    const v4i* w = reinterpret_cast<const v4i*>(net.base + net.w_off[head]);
    const int32_t* bias = reinterpret_cast<const int32_t*>(net.base + net.b_off[head]);
    const char* g = tbuf + (r < grp.boards ? r : 0) * grp.lds.g_stride + 16 * hh;
    for (int ot = wave; ot < a_tiles; ot += kWaves) {
      v16i acc;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) acc[reg] = bias[32 * ot + TileRow(reg, hh)];
      for (int kt = 0; kt < k_tiles; ++kt) {
        const v4i a = w[((size_t)ot * k_tiles + kt) * kWave + lane];
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, *reinterpret_cast<const v4i*>(g + 32 * kt), acc, 0, 0, 0);
      }
      if (r < grp.boards) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) rows_io[r * io_stride + 32 * ot + TileRow(reg, hh)] = acc[reg];
      }
    }
  }
  __syncthreads();  // the head's integers: written a column per lane, stored a row after the other
  for (int i = tid; i < grp.boards * (A + 1); i += kThreads) {
    p[(size_t)grp.first * (A + 1) + i] = rows_io[(i / (A + 1)) * io_stride + i % (A + 1)];
  }
}

// ---------------------------------------------------------------------------
// ConvTrainRow
// ---------------------------------------------------------------------------
struct RowArgs {
  int rows, width;         // the layer's rows; the columns of its dx
  const uint32_t* dz;      // [rows][ldn] split
  int ldn, n16;            // the layer's N up to a multiple of 16 (<= ldn)
  const uint16_t* wt;      // bf16 [width][n16]
  int P, P16, flag_ld;     // P16 > 0 (the head): column k = square * P16 + plane, its flag at row * flag_ld + square * P
                           // + plane, zero for plane >= P; P16 = 0: the flag at row * flag_ld + k
  const unsigned char* flags;
  float out_scale;
  uint32_t* out;           // [rows][width] split
};

__global__ __launch_bounds__(256) void ConvTrainRow(RowArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, hh = lane >> 5;
  const int row0 = (int)blockIdx.x * 64, tiles = (a.width + 31) / 32;
  for (int kt = wave; kt < tiles; kt += 4) {  // (uniform in the wave)
    const int col = 32 * kt + c;
    const bool col_ok = col < a.width;
    v16f acc[2];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[0][reg] = acc[1][reg] = 0.0f;
    for (int ns = 0; ns < a.n16 / 16; ++ns) {
      v4i raw = {0, 0, 0, 0};
      if (col_ok) raw = *reinterpret_cast<const v4i*>(a.wt + (size_t)col * a.n16 + 16 * ns + 8 * hh);
      const v8bf b = __builtin_bit_cast(v8bf, raw);
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const int row = row0 + 32 * rt + c;
        v4i w0 = {0, 0, 0, 0}, w1 = {0, 0, 0, 0};
        if (row < a.rows) {
          const v4i* src = reinterpret_cast<const v4i*>(a.dz + (size_t)row * a.ldn + 16 * ns + 8 * hh);
          w0 = src[0], w1 = src[1];
        }
        v8bf hi, lo;
        TearSplit(w0, w1, &hi, &lo);
        acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hi, b, acc[rt], 0, 0, 0);
        acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lo, b, acc[rt], 0, 0, 0);
      }
    }
    if (!col_ok) continue;
    bool real = true;
    int flag_at = col;
    if (a.P16 > 0) {
      const int sq = col / a.P16, pl = col - sq * a.P16;
      real = pl < a.P;
      flag_at = sq * a.P + pl;
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = row0 + 32 * rt + TileRow(reg, hh);
        if (row >= a.rows) continue;
        float g = 0.0f;
        if (real && (a.flags[(size_t)row * a.flag_ld + flag_at] & 128) == 0) g = acc[rt][reg] * a.out_scale;
        a.out[(size_t)row * a.width + col] = pgx::TrainSplit(g);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// ConvTrainDx
// ---------------------------------------------------------------------------
struct DxArgs {
  int rows, H, W, D, G;
  const uint32_t* dz;      // [rows][H W][D] split
  const uint16_t* wt;      // bf16 [9][D][D]: the mirrored transposes
  const uint32_t* res;     // null, or [rows][H W][D] split: the dz of the block's second layer (may be `out`)
  float res_scale;         // 2^s of that layer
  const unsigned char* flags;  // the saved bytes of the activation below
  float out_scale;         // 2^-s of the layer that made it
  uint32_t* out;           // [rows][H W][D] split
};

__host__ __device__ inline size_t DxLds(int H, int W, int D, int G) {
  return (size_t)G * (H + 2) * (W + 2) * (D + 4) * 4;
}

template <int CT>
__device__ inline void DxItem(const DxArgs& a, const uint32_t* lds, int first, int cols, int kt, int tile0, int lane) {
  const int r = lane & 31, hh = lane >> 5, S = a.H * a.W, stride = a.D + 4, records = (a.H + 2) * (a.W + 2);
  int addr[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int col = 32 * (tile0 + c) + r;
    const int cc = col < cols ? col : 0;  // (a column past the group's squares reads board 0's first: dropped below)
    const int b = cc / S, sq = cc - b * S, y = sq / a.W, x = sq - y * a.W;
    addr[c] = (b * records + (y + 1) * (a.W + 2) + (x + 1)) * stride + 8 * hh;
  }
  v16f acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[c][reg] = 0.0f;
  }
  for (int tap = 0; tap < 9; ++tap) {
    const int off = ((tap / 3 - 1) * (a.W + 2) + (tap % 3 - 1)) * stride;
    const uint16_t* wrow = a.wt + ((size_t)tap * a.D + 32 * kt + r) * a.D + 8 * hh;
    for (int ns = 0; ns < a.D / 16; ++ns) {
      const v8bf b = __builtin_bit_cast(v8bf, *reinterpret_cast<const v4i*>(wrow + 16 * ns));
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const v4i* src = reinterpret_cast<const v4i*>(lds + addr[c] + off + 16 * ns);
        v8bf hi, lo;
        TearSplit(src[0], src[1], &hi, &lo);
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hi, b, acc[c], 0, 0, 0);
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lo, b, acc[c], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int col = 32 * (tile0 + c) + TileRow(reg, hh);
      if (col >= cols) continue;
      const size_t at = ((size_t)first * S + col) * a.D + 32 * kt + r;
      float g = acc[c][reg];
      if (a.res != nullptr) g = g + pgx::TrainJoin(a.res[at]) * a.res_scale;
      a.out[at] = pgx::TrainSplit((a.flags[at] & 128) != 0 ? 0.0f : g * a.out_scale);
    }
  }
}

__global__ __launch_bounds__(kThreads) void ConvTrainDx(DxArgs a) {
  extern __shared__ v4i lds4[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int S = a.H * a.W, stride = a.D + 4, records = (a.H + 2) * (a.W + 2), quads = a.D / 4;
  const int first = (int)blockIdx.x * a.G;
  if (first >= a.rows) return;
  const int boards = a.rows - first < a.G ? a.rows - first : a.G, cols = boards * S;
  for (int i = tid; i < a.G * records * stride / 4; i += kThreads) lds4[i] = v4i{0, 0, 0, 0};
  __syncthreads();  // the zeros lie before the records are written over them
  const v4i* src = reinterpret_cast<const v4i*>(a.dz + (size_t)first * S * a.D);
  for (int i = tid; i < cols * quads; i += kThreads) {
    const int pos = i / quads, q4 = i - pos * quads;
    const int b = pos / S, sq = pos - b * S, y = sq / a.W, x = sq - y * a.W;
    lds4[(b * records + (y + 1) * (a.W + 2) + (x + 1)) * (stride / 4) + q4] = src[i];
  }
  __syncthreads();  // the group's dz is complete; LDS is only read from here on
  const uint32_t* lds = reinterpret_cast<const uint32_t*>(lds4);
  const int c_tiles = a.D / 32, col_tiles = (cols + 31) / 32, chunks = (col_tiles + kChunk - 1) / kChunk;
  for (int item = wave; item < c_tiles * chunks; item += kWaves) {
    const int kt = item / chunks, tile0 = kChunk * (item - kt * chunks);
    const int left = col_tiles - tile0;
    if (left >= 4) {
      DxItem<4>(a, lds, first, cols, kt, tile0, lane);
    } else if (left == 3) {
      DxItem<3>(a, lds, first, cols, kt, tile0, lane);
    } else if (left == 2) {
      DxItem<2>(a, lds, first, cols, kt, tile0, lane);
    } else {
      DxItem<1>(a, lds, first, cols, kt, tile0, lane);
    }
  }
}

// ---------------------------------------------------------------------------
// ConvTrainDw
// ---------------------------------------------------------------------------
struct DwArgs {
  int rows, H, W, N, K;
  const uint32_t* dz;      // [rows][H W][N] split
  const unsigned char* x;  // [rows][H W][K]: saved bytes, or the input
  int slice_boards;
  float* ws;               // [slices][N][9 K + 1]
};

// the LDS rows of a pass, in bf16 elements: a dz plane's and the input's (margin W + 2 on both sides of the run, and
// the dwords a funnelled read takes past its last element); both are 8 (mod 16), which spreads the rows over the banks
struct DwLds {
  int uz, ux;
};
__host__ __device__ inline DwLds DwLayout(int W, int run) {
  DwLds l;
  l.uz = run + 8;
  l.ux = (run + 2 * (W + 2) + 10 + 15) / 16 * 16 + 8;
  return l;
}
__host__ __device__ inline size_t DwLdsBytes(int W, int run) {
  const DwLds l = DwLayout(W, run);
  return (size_t)64 * (2 * l.uz + l.ux) * 2;
}
constexpr int kDwMaxSquares = 176;  // of a pass: ConvTrainPassOf's target, or one board of at most 128
static_assert(pgx::kConvTrainPassTarget <= kDwMaxSquares && pgx::kConvMaxSquares <= kDwMaxSquares, "s_at");

__global__ __launch_bounds__(kThreads) void ConvTrainDw(DwArgs a) {
  extern __shared__ v4i lds4[];
  __shared__ uint16_t s_at[kDwMaxSquares];  // square p of the pass -> its haloed position
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, hh = lane >> 5;
  const int nt = wave >> 1, kt = wave & 1;
  const int k0 = (int)blockIdx.x * 64, n0 = (int)blockIdx.y * 64, slice = blockIdx.z;
  const int S = a.H * a.W;
  const pgx::ConvTrainPass pass = pgx::ConvTrainPassOf(a.H, a.W);
  const DwLds l = DwLayout(a.W, pass.run);
  uint16_t* zh = reinterpret_cast<uint16_t*>(lds4);
  uint16_t* zl = zh + 64 * l.uz;
  uint16_t* xt = zl + 64 * l.uz;
  const int margin = a.W + 2, squares = pass.boards * S;
  const int begin = slice * a.slice_boards, end = min(a.rows, begin + a.slice_boards);
  const bool with_db = blockIdx.x == 0 && kt == 0;
  const bool x_words = (a.K & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 3) == 0;
  const v4i ones_raw = {0x3f803f80, 0x3f803f80, 0x3f803f80, 0x3f803f80};
  const v8bf ones = __builtin_bit_cast(v8bf, ones_raw);

  for (int i = tid; i < (int)(DwLdsBytes(a.W, pass.run) / 16); i += kThreads) lds4[i] = v4i{0, 0, 0, 0};
  for (int p = tid; p < squares; p += kThreads) {
    const int b = p / S, sq = p - b * S, y = sq / a.W, x = sq - y * a.W;
    s_at[p] = (uint16_t)(b * pass.stride + (y + 1) * (a.W + 1) + (x + 1));
  }
  v16f total[9], total_b;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) total[t][reg] = 0.0f;
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) total_b[reg] = 0.0f;

  for (int base = begin; base < end; base += pass.boards) {
    __syncthreads();  // the zeros and s_at (first pass); the last pass's fragments are read
    const int live = (end - base < pass.boards ? end - base : pass.boards) * S;
    // dz: the pass's squares x 64 n, four words at a time, transposed into the hi and lo planes (a board past the
    // slice's end: zeros)
    for (int e = tid; e < squares * 16; e += kThreads) {
      const int p = e >> 4, n4 = (e & 15) * 4;
      v4i wds = {0, 0, 0, 0};
      if (p < live && n0 + n4 < a.N) {
        wds = *reinterpret_cast<const v4i*>(a.dz + ((size_t)base * S + p) * a.N + n0 + n4);
      }
      const int u = s_at[p];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        zh[(n4 + q) * l.uz + u] = (uint16_t)((uint32_t)wds[q] >> 16);
        zl[(n4 + q) * l.uz + u] = (uint16_t)((uint32_t)wds[q] & 0xffffu);
      }
    }
    // the input: the pass's squares x 64 k bytes, sixteen at a time
    for (int e = tid; e < squares * 4; e += kThreads) {
      const int p = e >> 2, k16 = (e & 3) * 16;
      const int u = margin + s_at[p];
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int k = k0 + k16 + 4 * q4;
        uint32_t word = 0;
        if (p < live) {
          const unsigned char* xr = a.x + ((size_t)base * S + p) * a.K;
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
          xt[(k16 + 4 * q4 + b) * l.ux + u] = Bf16OfSmall((float)((word >> (8 * b)) & 127u));
        }
      }
    }
    __syncthreads();
    const uint32_t* xrow = reinterpret_cast<const uint32_t*>(xt + (32 * kt + c) * l.ux);  // (ux is even)
    v16f acc_b;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc_b[reg] = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      v16f acc[3];
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc[dx][reg] = 0.0f;
      }
      for (int step = 0; step < pass.run / 16; ++step) {
        const int at = 16 * step + 8 * hh;
        const v8bf a_hi = __builtin_bit_cast(v8bf, *reinterpret_cast<const v4i*>(&zh[(32 * nt + c) * l.uz + at]));
        const v8bf a_lo = __builtin_bit_cast(v8bf, *reinterpret_cast<const v4i*>(&zl[(32 * nt + c) * l.uz + at]));
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int e0 = margin + at + (dy - 1) * (a.W + 1) + (dx - 1);  // (>= 0: the margin is W + 2)
          const uint32_t* src = xrow + (e0 >> 1);
          const uint32_t shift = 16u * (uint32_t)(e0 & 1);
          v4i raw;
#pragma unroll
          for (int q = 0; q < 4; ++q) raw[q] = (int)__builtin_amdgcn_alignbit(src[q + 1], src[q], shift);
          const v8bf b = __builtin_bit_cast(v8bf, raw);
          acc[dx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b, acc[dx], 0, 0, 0);
          acc[dx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b, acc[dx], 0, 0, 0);
        }
        if (dy == 0 && with_db) {
          acc_b = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, ones, acc_b, 0, 0, 0);
          acc_b = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, ones, acc_b, 0, 0, 0);
        }
      }
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) total[3 * dy + dx][reg] = total[3 * dy + dx][reg] + acc[dx][reg];
      }
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) total_b[reg] = total_b[reg] + acc_b[reg];
  }
  const int ld = 9 * a.K + 1;
  float* ws = a.ws + (size_t)slice * a.N * ld;
  const int k = k0 + 32 * kt + c;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int n = n0 + 32 * nt + TileRow(reg, hh);
    if (n >= a.N) continue;
    if (k < a.K) {
#pragma unroll
      for (int t = 0; t < 9; ++t) ws[(size_t)n * ld + t * a.K + k] = total[t][reg];
    }
    if (with_db && c == 0) ws[(size_t)n * ld + 9 * a.K] = total_b[reg];
  }
}

size_t Align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

// ---------------------------------------------------------------------------
// the handle (engine.h: ConvTrain)
// ---------------------------------------------------------------------------
struct ConvTrain::Layout {
  uint32_t w_off[kL], b_off[kL], wt_off[kL];
  size_t image, wt, x, saved, g, dz_a, dz_b, dz_r, dp, ws;  // byte offsets into the block
  int g_fwd, g_dx;                                          // the boards of a block of ConvTrainForward / ConvTrainDx
  size_t lds_fwd, lds_dx, lds_dw;
};

ConvTrain::ConvTrain(int device, int H, int W, int C, int A, int D, int L, int P, long long max_rows)
    : device_(device), H_(H), W_(W), C_(C), A_(A), D_(D), L_(L), P_(P), max_rows_((int)max_rows), at_(new Layout()) {
  char err[240];
  if (!pgx::ConvTrainCheck(H, W, C, A, D, L, P, max_rows, err, sizeof(err))) throw std::invalid_argument(err);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
  if (device < 0 || device >= count) {
    throw std::invalid_argument("conv_train_create: device = " + std::to_string(device) + " must be 0 .. " +
                                std::to_string(count - 1));
  }
  int lds_limit = 0;
  EPA_HIP(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  const size_t limit = (size_t)lds_limit;
  // G of either kernel: the largest group whose LDS is at most half the limit (two blocks a CU); one board may take
  // all of it
  auto group = [&](int most, auto bytes, const char* what) {
    if (bytes(1) + kStaticLds > limit) {
      throw std::invalid_argument(std::string("conv_train: one board of H = ") + std::to_string(H) + ", W = " +
                                  std::to_string(W) + ", D = " + std::to_string(D) + " needs " +
                                  std::to_string(bytes(1) + kStaticLds) + " bytes of LDS in the " + what +
                                  ", the device gives a block " + std::to_string(limit));
    }
    for (int g = most; g > 1; --g) {
      if (bytes(g) + kStaticLds <= limit / 2) return g;
    }
    return 1;
  };
  at_->g_fwd = group(kFwdMaxBoards, [&](int g) { return (size_t)FwdLayout(H, W, D, P, A, g).total; }, "forward");
  at_->g_dx = group(kDxMaxBoards, [&](int g) { return DxLds(H, W, D, g); }, "backward");
  at_->lds_fwd = (size_t)FwdLayout(H, W, D, P, A, at_->g_fwd).total;
  at_->lds_dx = DxLds(H, W, D, at_->g_dx);
  at_->lds_dw = DwLdsBytes(W, pgx::ConvTrainPassOf(H, W).run);

  const int layers = 2 * L + 3, S = H * W;
  const size_t p16 = ((size_t)P + 15) / 16 * 16, n16 = ((size_t)A + 1 + 15) / 16 * 16;
  const size_t rows = (size_t)max_rows_, positions = rows * S;
  size_t image = 0, wt = 0, ws = 0;
  for (int i = 0; i < layers; ++i) {
    const bool head = i == layers - 1, reduce = i == layers - 2;
    const size_t N = head ? A + 1 : (reduce ? P : D), T = i < layers - 2 ? 9 : 1;
    const size_t K = i == 0 ? C : (head ? (size_t)S * P : D);
    const size_t n_tiles = (N + 31) / 32, k_tiles = (K + 31) / 32;
    at_->w_off[i] = (uint32_t)image, image += n_tiles * T * k_tiles * 1024;
    at_->b_off[i] = (uint32_t)image, image += n_tiles * 32 * 4;
    at_->wt_off[i] = (uint32_t)wt;
    wt += i == 0 ? 0 : (head ? (size_t)S * p16 * n16 : (reduce ? K * p16 : 9 * K * N));
    size_t slices;
    if (head) {
      slices = (size_t)pgx::TrainMostSlices(max_rows_, (int)N, (int)K);
    } else if (reduce) {
      slices = (size_t)pgx::TrainMostSlices((int)positions, (int)N, (int)K);
    } else {
      slices = (size_t)pgx::ConvTrainMostSlices(max_rows_, H, W, (int)N, (int)K);
    }
    ws = std::max(ws, slices * N * (T * K + 1) * 4);
  }
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += Align256(bytes);
    return here;
  };
  at_->image = take(image), at_->wt = take(2 * wt), at_->x = take(positions * C);
  at_->saved = take((size_t)(2 * L + 1) * positions * D), at_->g = take(positions * P);
  at_->dz_a = take(positions * D * 4), at_->dz_b = take(L > 0 ? positions * D * 4 : 0);
  at_->dz_r = take(positions * p16 * 4), at_->dp = take(rows * n16 * 4), at_->ws = take(ws);
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  try {
    mem_.Alloc(at);
  } catch (...) {
    (void)hipSetDevice(before);
    throw;
  }
  hipError_t set = hipSuccess;
  auto allow = [&](const void* kernel, size_t lds) {
    if (lds > 48 * 1024 && set == hipSuccess) {
      set = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
  };
  allow(reinterpret_cast<const void*>(&ConvTrainForward), at_->lds_fwd);
  allow(reinterpret_cast<const void*>(&ConvTrainDx), at_->lds_dx);
  allow(reinterpret_cast<const void*>(&ConvTrainDw), at_->lds_dw);
  (void)hipSetDevice(before);
  EPA_HIP(set);
}

ConvTrain::~ConvTrain() {
  int before = 0;
  if (hipGetDevice(&before) != hipSuccess) return;
  (void)hipSetDevice(device_);
  mem_.Free();
  (void)hipSetDevice(before);
}

void ConvTrain::Forward(hipStream_t stream, int rows, const void* const* d_w, const void* const* d_b,
                        const int32_t* shifts, const void* d_x, void* d_p) {
  char err[200];
  if (d_w == nullptr || d_b == nullptr || shifts == nullptr || d_x == nullptr || d_p == nullptr) {
    throw std::invalid_argument("conv_train_forward: null argument");
  }
  if (rows < 1 || rows > max_rows_) {
    throw std::invalid_argument("conv_train_forward: rows = " + std::to_string(rows) + " must be 1 .. " +
                                std::to_string(max_rows_) + " (the handle's max_rows)");
  }
  if (!pgx::ConvTrainCheckShifts(L_, shifts, err, sizeof(err))) throw std::invalid_argument(err);
  const int layers = 2 * L_ + 3, S = H_ * W_;
  PackArgs pack{};
  FwdDev net{};
  pack.layers = layers, pack.S = S, pack.P = P_, pack.P16 = (P_ + 15) / 16 * 16, pack.n16 = (A_ + 1 + 15) / 16 * 16;
  pack.image = mem_.p + at_->image;
  pack.wt = reinterpret_cast<uint16_t*>(mem_.p + at_->wt);
  net.H = H_, net.W = W_, net.C = C_, net.A = A_, net.D = D_, net.L = L_, net.P = P_, net.G = at_->g_fwd;
  net.base = pack.image;
  for (int i = 0; i < layers; ++i) {
    if (d_w[i] == nullptr || d_b[i] == nullptr) throw std::invalid_argument("conv_train_forward: null argument");
    const bool head = i == layers - 1, reduce = i == layers - 2;
    pack.w[i] = static_cast<const signed char*>(d_w[i]);
    pack.b[i] = static_cast<const int32_t*>(d_b[i]);
    pack.n_out[i] = head ? A_ + 1 : (reduce ? P_ : D_);
    pack.taps[i] = i < layers - 2 ? 9 : 1;
    pack.k_in[i] = i == 0 ? C_ : (head ? S * P_ : D_);
    pack.w_off[i] = net.w_off[i] = at_->w_off[i];
    pack.b_off[i] = net.b_off[i] = at_->b_off[i];
    pack.wt_off[i] = at_->wt_off[i];
    net.shift[i] = shift_[i] = shifts[i];
  }
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  rows_ = 0;  // (a forward that fails leaves nothing to go back through)
  hipLaunchKernelGGL(ConvTrainPack, dim3(64, layers), dim3(256), 0, stream, pack);
  unsigned char* x = reinterpret_cast<unsigned char*>(mem_.p + at_->x);
  const hipError_t copied = hipMemcpyAsync(x, d_x, (size_t)rows * S * C_, hipMemcpyDeviceToDevice, stream);
  if (copied == hipSuccess) {
    hipLaunchKernelGGL(ConvTrainForward, dim3((rows + net.G - 1) / net.G), dim3(kThreads), at_->lds_fwd, stream, net,
                       rows, x, reinterpret_cast<unsigned char*>(mem_.p + at_->saved),
                       reinterpret_cast<unsigned char*>(mem_.p + at_->g), static_cast<int32_t*>(d_p));
  }
  const hipError_t launched = hipGetLastError();
  (void)hipSetDevice(before);
  EPA_HIP(copied);
  EPA_HIP(launched);
  rows_ = rows;
}

void ConvTrain::Backward(hipStream_t stream, int rows, const void* d_dp, void* const* d_dw, void* const* d_db) {
  if (d_dp == nullptr || d_dw == nullptr || d_db == nullptr) {
    throw std::invalid_argument("conv_train_backward: null argument");
  }
  const int layers = 2 * L_ + 3, head = layers - 1, red = layers - 2;
  for (int i = 0; i < layers; ++i) {
    if (d_dw[i] == nullptr || d_db[i] == nullptr) throw std::invalid_argument("conv_train_backward: null argument");
  }
  if (rows_ == 0) throw std::invalid_argument("conv_train_backward: no forward has been made with this handle");
  if (rows != rows_) {
    throw std::invalid_argument("conv_train_backward: rows = " + std::to_string(rows) +
                                ", but the last forward had " + std::to_string(rows_));
  }
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  const int S = H_ * W_, positions = rows * S;
  const int p16 = (P_ + 15) / 16 * 16, n16 = (A_ + 1 + 15) / 16 * 16;
  const unsigned char* x = reinterpret_cast<const unsigned char*>(mem_.p + at_->x);
  const unsigned char* saved = reinterpret_cast<const unsigned char*>(mem_.p + at_->saved);
  const unsigned char* g = reinterpret_cast<const unsigned char*>(mem_.p + at_->g);
  auto activation = [&](int j) { return saved + (size_t)j * positions * D_; };
  uint32_t* buf_a = reinterpret_cast<uint32_t*>(mem_.p + at_->dz_a);
  uint32_t* buf_b = reinterpret_cast<uint32_t*>(mem_.p + at_->dz_b);
  uint32_t* dz_r = reinterpret_cast<uint32_t*>(mem_.p + at_->dz_r);
  uint32_t* dp = reinterpret_cast<uint32_t*>(mem_.p + at_->dp);
  float* ws = reinterpret_cast<float*>(mem_.p + at_->ws);
  const uint16_t* wt = reinterpret_cast<const uint16_t*>(mem_.p + at_->wt);
  auto dw = [&](int i) { return static_cast<float*>(d_dw[i]); };
  auto db = [&](int i) { return static_cast<float*>(d_db[i]); };
  auto down = [&](int i) { return 1.0f / (float)(1 << shift_[i]); };

  // dW and db of 3x3 layer i from its dz
  auto reduce_conv = [&](int i, const uint32_t* dz) {
    const int K = i == 0 ? C_ : D_;
    const pgx::ConvTrainSlicing s = pgx::ConvTrainSlices(rows, H_, W_, D_, K);
    DwArgs r{rows, H_, W_, D_, K, dz, i == 0 ? x : activation(i - 1), s.slice_boards, ws};
    hipLaunchKernelGGL(ConvTrainDw, dim3((K + 63) / 64, (D_ + 63) / 64, s.slices), dim3(kThreads), at_->lds_dw, stream,
                       r);
    TrainSumLaunch(ws, s.slices, D_, 9 * K, dw(i), db(i), stream);
  };
  // the dz of layer i - 1 from the dz of 3x3 layer i >= 1
  auto below_conv = [&](int i, const uint32_t* dz, const uint32_t* res, int res_layer, uint32_t* out) {
    DxArgs r{rows, H_, W_, D_, at_->g_dx, dz, wt + at_->wt_off[i], res,
             res != nullptr ? (float)(1 << shift_[res_layer]) : 0.0f, activation(i - 1), down(i - 1), out};
    hipLaunchKernelGGL(ConvTrainDx, dim3((rows + at_->g_dx - 1) / at_->g_dx), dim3(kThreads), at_->lds_dx, stream, r);
  };
  TrainSplitLaunch(static_cast<const float*>(d_dp), rows, A_ + 1, n16, dp, stream);
  // the head: `rows` rows of K = H W P; its dx is the reduce layer's dz, [rows H W][P16]
  TrainReduceLaunch(rows, A_ + 1, S * P_, dp, n16, g, ws, dw(head), db(head), stream);
  {
    RowArgs r{rows, S * p16, dp, n16, n16, wt + at_->wt_off[head], P_, p16, S * P_, g, down(red), dz_r};
    hipLaunchKernelGGL(ConvTrainRow, dim3((rows + 63) / 64), dim3(256), 0, stream, r);
  }
  // the reduce layer: rows H W rows of K = D, N = P
  TrainReduceLaunch(positions, P_, D_, dz_r, p16, activation(2 * L_), ws, dw(red), db(red), stream);
  {
    RowArgs r{positions, D_, dz_r, p16, p16, wt + at_->wt_off[red], 0, 0, D_, activation(2 * L_), down(2 * L_), buf_a};
    hipLaunchKernelGGL(ConvTrainRow, dim3((positions + 63) / 64), dim3(256), 0, stream, r);
  }
  for (int l = L_ - 1; l >= 0; --l) {
    reduce_conv(2 + 2 * l, buf_a);
    below_conv(2 + 2 * l, buf_a, nullptr, 0, buf_b);
    reduce_conv(1 + 2 * l, buf_b);
    below_conv(1 + 2 * l, buf_b, buf_a, 2 + 2 * l, buf_a);  // (in place: a lane reads its word, then writes it)
  }
  reduce_conv(0, buf_a);
  const hipError_t launched = hipGetLastError();
  (void)hipSetDevice(before);
  EPA_HIP(launched);
}

}  // namespace epa
