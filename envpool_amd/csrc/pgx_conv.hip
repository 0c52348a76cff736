// PGX convolutional network on the int8 matrix cores (pgx_conv.hip.h is the contract; DESIGN.md "PGX convolutional
// network").
//
// PgxConvEval: one launch per evaluation, four waves per block, a GROUP of G boards per block.  Every layer is a GEMM
// OUT[n][square] = SUM_{tap, c} W[n][tap][c] X[square + tap][c] on v_mfma_i32_32x32x32_i8 with the WEIGHTS as the A
// operand (M = 32 output channels) and the ACTIVATIONS as the B operand (N = 32 squares): the columns of a block are the
// squares of its boards, board after board, padded to a multiple of 32.  K runs over the 9 taps and the input channels
// in 32-channel k-steps.
//
// LDS.  h and t of the whole group lie in LDS as [board][(H + 2) (W + 2) squares][D + 16 bytes]: a board with a halo
// of zero records around it, so that a tap is an address offset -- (dy - 1) (W + 2) + (dx - 1) records -- and never a
// branch, and off-board reads are the contract's zero padding.  The halo is zeroed once and never written: a store
// goes to the record of a live column only.  A column past the group's squares reads the records of board 0's first
// square (any valid address: its results are dropped) and stores nothing.  The 16 bytes of padding per record spread
// the 128-bit accesses of neighbouring squares over the banks.
//
// Lane map.  As in pgx_net.hip a result tile has column = lane & 31 and channel (reg & 3) + 8 (reg >> 2) +
// 4 (lane >> 5) in register reg; after shift, clamp and packing, dword g of lane (r, hh) holds channels 8 g + 4 hh .. + 3
// of the tile.  A record therefore keeps each 32-channel tile in the order (half, dword, byte): channel
// 32 kt + 8 g + 4 hh + b lies at byte 32 kt + 16 hh + 4 g + b.  Then a lane's result is ONE 128-bit store at
// record + 32 ot + 16 hh, and its B fragment of k-step kt of any tap ONE 128-bit load at record + tap + 32 kt + 16 hh:
// no lane movement between layers.  The weights are laid out to match at upload (ConvBuildImage): for (layer, output
// tile ot, tap, k-step kt) the wave reads 1 KiB, lane (r, hh) its 16 bytes, dword g = W[32 ot + r][tap][32 kt + 8 g +
// 4 hh .. + 3].  Only the documented C/D map of the instruction is relied on: A and B use the same k order.
//
// Work split.  A layer's tiles are (output tile ot) x (column tile); an ITEM is one ot against a chunk of up to four
// column tiles, whose four accumulators a wave holds at once, so that a 1 KiB weight fragment read from L2 feeds up to
// four MFMAs and the whole group shares one pass over the layer's weights.  Items go round the four waves.  G is
// chosen on the host (ConvBuildImage) as the largest group of at most 32 boards whose LDS is at most half the device's
// per-block limit, so that two blocks fit a CU; a net whose single board needs more takes up to the whole limit.
//
// Barriers.  Waves read records other waves wrote (the neighbours of a square, the other output tiles of a record), so
// every layer ends in a __syncthreads: (1) after zeroing, before the input lands in zeroed records; (2) after the input;
// (3) after each layer, before its output is read as input -- the residual layer reads its old h only at the (record,
// tile) it overwrites itself, so in place is safe --; (4) after the reduce layer, whose byte image g overlays t; (5)
// after the head's integers, which overlay h, are stored one column per lane and before NetOutputs reads them one row
// per lane; (6) before the float rows leave in coalesced stores.  A block past its segment returns before all of them.
//
// The head needs boards as columns: the reduce layer scatters its bytes into g [board][H W P in the (half, dword,
// byte) order], which IS the head's B fragment with board = column; the head's p goes through LDS once more to turn
// (row in register, board on lane) into one row per lane for NetOutputs, as in PgxNetEval.
//
// The pair form: one launch per net over that net's segment of the plan (PgxNetPlan: `order`, `n0` read on the device).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "engine.h"
#include "pgx_conv.hip.h"

namespace epa {
namespace {

using pgx::kGuidedIdle;

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kWave = 64, kWaves = 4, kThreads = kWave * kWaves;
constexpr int kMaxBoards = 32;  // G: the head's columns are one tile
constexpr int kChunk = 4;       // column tiles of an item
constexpr size_t kStaticLds = 1024;  // an upper bound of the kernel's static LDS (s_row, the block-wide OR)
static_assert(pgx::kConvMaxLayers == kConvImageLayers, "engine.h: ConvImage");

struct ConvDev {
  int H, W, C, A, D, L, P, G;
  float scale_p, scale_v;
  const char* base;
  uint32_t w_off[pgx::kConvMaxLayers], b_off[pgx::kConvMaxLayers];
  int32_t shift[pgx::kConvMaxLayers];
};

// The block's LDS, in bytes: h at 0 and t at `second`, `buf` bytes each; the head's rows (int32, `io_stride` words a
// board) overlay h, the reduce layer's image g (`g_stride` bytes a board) overlays t.
struct ConvLds {
  int stride, records, buf, kp, g_stride, io_stride, second, total;
};
__host__ __device__ inline ConvLds ConvLayout(int H, int W, int D, int P, int A, int G) {
  ConvLds l;
  l.stride = D + 16;
  l.records = (H + 2) * (W + 2);
  l.buf = G * l.records * l.stride;
  l.kp = (H * W * P + 31) & ~31;
  l.g_stride = l.kp + 16;
  l.io_stride = 32 * ((A + 1 + 31) / 32) + 1;  // odd: no bank conflicts
  const int io = (G * l.io_stride * 4 + 15) & ~15, g = G * l.g_stride;
  l.second = l.buf > io ? l.buf : io;
  l.total = l.second + (l.buf > g ? l.buf : g);
  return l;
}

// the channel (within its 32-channel tile) of accumulator register `reg` of a lane of half `hh`
__device__ inline int TileChannel(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }
// where element k of a row lies in the (half, dword, byte) order of its 32-element tile
__host__ __device__ inline int TilePlace(int k) { return (k & ~31) + 16 * ((k >> 2) & 1) + 4 * ((k >> 3) & 3) + (k & 3); }

// What the kernel knows of its group
struct ConvGroup {
  int boards, cols;   // live boards, their squares: the live columns
  int S, W, P;        // squares of a board, its width, the planes
  ConvLds lds;
};

enum { kEpiAct = 0, kEpiResidual = 1, kEpiReduce = 2 };

// One item: output tile `ot` of a layer against the CT column tiles from `tile0` on.  w: the layer's fragments, bias:
// its padded bias; `in`: the records read (h or t), `out`: where the result goes -- records (kEpiAct, kEpiResidual:
// out = clamp(rs(.) + out, 0, 127) in place) or the image g (kEpiReduce, ot = 0).
template <int CT>
__device__ inline void ConvItem(const ConvGroup& grp, const v4i* __restrict__ w, const int32_t* __restrict__ bias,
                                int shift, int taps, int k_tiles, int ot, int tile0, const char* in, char* out, int epi,
                                int lane) {
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
    const int32_t b = bias[32 * ot + TileChannel(reg, hh)];
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
    if (epi == kEpiReduce) {
      char* g = out + board[c] * grp.lds.g_stride;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int q = TileChannel(reg, hh);
        if (q < grp.P) g[TilePlace(square[c] * grp.P + q)] = (char)pgx::NetAct(pgx::NetRs(acc[c][reg], shift));
      }
      continue;
    }
    v4i* dst = reinterpret_cast<v4i*>(out + addr[c] + 32 * ot);
    v4i old = {0, 0, 0, 0};
    if (epi == kEpiResidual) old = *dst;
    v4i packed;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        int32_t v = pgx::NetRs(acc[c][4 * g + b], shift);
        if (epi == kEpiResidual) v += (int32_t)(((uint32_t)old[g] >> (8 * b)) & 255u);
        word |= (uint32_t)pgx::NetAct(v) << (8 * b);
      }
      packed[g] = (int)word;
    }
    *dst = packed;
  }
}

// One layer: its items go round the block's waves.  n_tiles: the layer's output tiles.
__device__ inline void ConvLayerPass(const ConvGroup& grp, const ConvDev& net, int layer, int n_tiles, int taps,
                                     int k_tiles, const char* in, char* out, int epi, int wave, int lane) {
  const v4i* w = reinterpret_cast<const v4i*>(net.base + net.w_off[layer]);
  const int32_t* bias = reinterpret_cast<const int32_t*>(net.base + net.b_off[layer]);
  const int shift = net.shift[layer];
  const int col_tiles = (grp.cols + 31) / 32, chunks = (col_tiles + kChunk - 1) / kChunk;
  for (int item = wave; item < n_tiles * chunks; item += kWaves) {
    const int ot = item / chunks, tile0 = kChunk * (item - ot * chunks);
    const int left = col_tiles - tile0;
    if (left >= 4) {
      ConvItem<4>(grp, w, bias, shift, taps, k_tiles, ot, tile0, in, out, epi, lane);
    } else if (left == 3) {
      ConvItem<3>(grp, w, bias, shift, taps, k_tiles, ot, tile0, in, out, epi, lane);
    } else if (left == 2) {
      ConvItem<2>(grp, w, bias, shift, taps, k_tiles, ot, tile0, in, out, epi, lane);
    } else {
      ConvItem<1>(grp, w, bias, shift, taps, k_tiles, ot, tile0, in, out, epi, lane);
    }
  }
}

// order == null: rows 0 .. rows - 1, board j of block b is row b G + j.  Otherwise the entries [0, *n0) (seg 0) or
// [*n0, rows) (seg 1) of the plan `order`: board j of block b is the row order[first of the segment + b G + j].
// (two waves a SIMD: two blocks fit a CU's registers as they fit its LDS)
__global__ __launch_bounds__(kThreads, 2) void PgxConvEval(ConvDev net, const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ n0, int seg, int rows, int mode,
                                                         const unsigned char* __restrict__ obs,
                                                         const unsigned char* __restrict__ mask,
                                                         const unsigned char* __restrict__ status,
                                                         float* __restrict__ policy, float* __restrict__ value,
                                                         unsigned int* pending) {
  extern __shared__ v4i lds4[];
  __shared__ int s_row[kMaxBoards];
  char* lds = reinterpret_cast<char*>(lds4);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int seg_first = 0, seg_end = rows;
  if (order != nullptr) {
    const int n = *n0;
    seg_first = seg == 0 ? 0 : n;
    seg_end = seg == 0 ? n : rows;
  }
  const int first = seg_first + (int)blockIdx.x * net.G;
  if (first >= seg_end) return;  // (the whole block, before any barrier)
  ConvGroup grp;
  grp.boards = seg_end - first < net.G ? seg_end - first : net.G;
  grp.S = net.H * net.W, grp.W = net.W, grp.P = net.P;
  grp.cols = grp.boards * grp.S;
  grp.lds = ConvLayout(net.H, net.W, net.D, net.P, net.A, net.G);
  const int A = net.A, io_stride = grp.lds.io_stride;

  int my_row = rows, my_status = kGuidedIdle;  // thread j < boards: board j's row
  if (tid < grp.boards) {
    my_row = order != nullptr ? order[first + tid] : first + tid;
    my_status = (int)status[my_row];
  }
  if (tid < kMaxBoards) s_row[tid] = my_row;
  if (wave == 0) {
    // the run loop's word: some row of the call is not idle (an ordinary atomic of one lane per wave with rows)
    const bool wave_pending = __any(my_status != kGuidedIdle) != 0;
    if (wave_pending && lane == 0 && pending != nullptr) atomicOr(pending, 1u);
  }
  const int any_evaluate = __syncthreads_or(my_status == pgx::kGuidedEvaluate ? 1 : 0);  // (s_row is visible too)

  char* hbuf = lds;
  char* tbuf = lds + grp.lds.second;
  int32_t* rows_io = reinterpret_cast<int32_t*>(lds);
  if (any_evaluate != 0) {
    for (int i = tid; i < grp.lds.total / 16; i += kThreads) lds4[i] = v4i{0, 0, 0, 0};
    __syncthreads();  // (1) the zeros lie before the input is written over them
    // the input: a square's C bytes into the first k-tile of its record of t, in the records' channel order
    const int C = net.C;
    for (int i = tid; i < grp.cols; i += kThreads) {
      const int b = i / grp.S, sq = i - b * grp.S, y = sq / grp.W, x = sq - y * grp.W;
      const unsigned char* src = obs + ((size_t)s_row[b] * grp.S + sq) * C;
      uint32_t word[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < pgx::kConvMaxChannels; ++c) {
        // (a bool's byte is 0 or 1; anything else counts as its low bit)
        if (c < C) word[TilePlace(c) >> 2] |= (uint32_t)(src[c] & 1u) << (8 * (TilePlace(c) & 3));
      }
      v4i* dst = reinterpret_cast<v4i*>(tbuf + (b * grp.lds.records + (y + 1) * (grp.W + 2) + (x + 1)) * grp.lds.stride);
      dst[0] = v4i{(int)word[0], (int)word[1], (int)word[2], (int)word[3]};
      dst[1] = v4i{(int)word[4], (int)word[5], (int)word[6], (int)word[7]};
    }
    __syncthreads();  // (2) the input is complete
    const int d_tiles = net.D / 32;
    ConvLayerPass(grp, net, 0, d_tiles, 9, 1, tbuf, hbuf, kEpiAct, wave, lane);
    __syncthreads();  // (3) a layer's output is complete before it is read; t is free to be overwritten
    for (int l = 0; l < net.L; ++l) {
      ConvLayerPass(grp, net, 1 + 2 * l, d_tiles, 9, d_tiles, hbuf, tbuf, kEpiAct, wave, lane);
      __syncthreads();  // (3)
      ConvLayerPass(grp, net, 2 + 2 * l, d_tiles, 9, d_tiles, tbuf, hbuf, kEpiResidual, wave, lane);
      __syncthreads();  // (3)
    }
    // reduce: one padded 32-row tile per column tile; its bytes go to g, which takes t's place
    ConvLayerPass(grp, net, 2 * net.L + 1, 1, 1, d_tiles, hbuf, tbuf, kEpiReduce, wave, lane);
    __syncthreads();  // (4) g is complete, and every wave is done with h: the head's rows take its place
    {
      const int head = 2 * net.L + 2, a_tiles = (A + 1 + 31) / 32, k_tiles = grp.lds.kp / 32;
      const int r = lane & 31, hh = lane >> 5;
      const v4i* w = reinterpret_cast<const v4i*>(net.base + net.w_off[head]);
      const int32_t* bias = reinterpret_cast<const int32_t*>(net.base + net.b_off[head]);
      // the column is a board; a column past the group's boards reads board 0 and stores nothing
      const char* g = tbuf + (r < grp.boards ? r : 0) * grp.lds.g_stride + 16 * hh;
      for (int ot = wave; ot < a_tiles; ot += kWaves) {
        v16i acc;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc[reg] = bias[32 * ot + TileChannel(reg, hh)];
        for (int kt = 0; kt < k_tiles; ++kt) {
          const v4i a = w[((size_t)ot * k_tiles + kt) * kWave + lane];
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, *reinterpret_cast<const v4i*>(g + 32 * kt), acc, 0, 0, 0);
        }
        if (r < grp.boards) {
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) rows_io[r * io_stride + 32 * ot + TileChannel(reg, hh)] = acc[reg];
        }
      }
    }
    __syncthreads();  // (5) the head's integers: written a column per lane, read a row per lane
    if (tid < grp.boards) {
      pgx::NetOutputs(rows_io + tid * io_stride, mask + (size_t)my_row * A, A, net.scale_p, net.scale_v, mode,
                      my_status);
    }
  } else if (tid < grp.boards) {
    for (int a = 0; a <= A; ++a) rows_io[tid * io_stride + a] = 0;  // no row of the group is to be evaluated
  }
  __syncthreads();  // (6) the float rows are complete
  if (tid < grp.boards) value[my_row] = pgx::NetBitsFloat(rows_io[tid * io_stride + A]);
  for (int i = tid; i < grp.boards * A; i += kThreads) {
    const int e = i / A, a = i - e * A;
    // (without a plan the group's rows are first .. first + boards - 1: consecutive floats)
    policy[(size_t)s_row[e] * A + a] = pgx::NetBitsFloat(rows_io[e * io_stride + a]);
  }
}

}  // namespace

bool ConvIsBlob(const void* blob, size_t bytes) {
  uint32_t magic = 0;
  if (blob != nullptr && bytes >= 4) std::memcpy(&magic, blob, 4);
  return magic == pgx::kConvMagic;
}

void ConvBuildImage(const void* blob, size_t bytes, size_t lds_limit, ConvImage* out, std::vector<char>* image) {
  pgx::ConvView v{};
  char err[240];
  if (!pgx::ConvParse(blob, bytes, &v, err, sizeof(err))) throw std::invalid_argument(err);
  // G: the largest group whose LDS is at most half the limit (two blocks a CU); one board may take all of it
  const size_t one = (size_t)ConvLayout(v.H, v.W, v.D, v.P, v.A, 1).total + kStaticLds;
  if (one > lds_limit) {
    throw std::invalid_argument("conv: one board of H = " + std::to_string(v.H) + ", W = " + std::to_string(v.W) +
                                ", D = " + std::to_string(v.D) + " needs " + std::to_string(one) +
                                " bytes of LDS, the device gives a block " + std::to_string(lds_limit));
  }
  int G = 1;
  for (int g = kMaxBoards; g > 1; --g) {
    if ((size_t)ConvLayout(v.H, v.W, v.D, v.P, v.A, g).total + kStaticLds <= lds_limit / 2) {
      G = g;
      break;
    }
  }
  out->H = v.H, out->W = v.W, out->C = v.C, out->A = v.A, out->D = v.D, out->L = v.L, out->P = v.P;
  out->scale_p = v.scale_p, out->scale_v = v.scale_v;
  out->layers = v.layers();
  out->G = G;
  out->lds = (size_t)ConvLayout(v.H, v.W, v.D, v.P, v.A, G).total;
  image->clear();
  for (int i = 0; i < v.layers(); ++i) {
    const pgx::ConvLayer& l = v.layer[i];
    const size_t n_tiles = ((size_t)l.n_out + 31) / 32, k_tiles = ((size_t)l.k_in + 31) / 32, taps = (size_t)l.taps;
    out->shift[i] = l.shift;
    out->w_off[i] = (uint32_t)image->size();
    image->resize(image->size() + n_tiles * taps * k_tiles * 1024, 0);
    char* w = image->data() + out->w_off[i];
    for (size_t ot = 0; ot < n_tiles; ++ot) {
      for (size_t tap = 0; tap < taps; ++tap) {
        for (size_t kt = 0; kt < k_tiles; ++kt) {
          char* frag = w + ((ot * taps + tap) * k_tiles + kt) * 1024;
          for (int lane = 0; lane < kWave; ++lane) {
            const size_t n = 32 * ot + (size_t)(lane & 31);
            for (int e = 0; e < 16; ++e) {  // byte e of the lane's 16: dword g = e / 4
              const size_t k = 32 * kt + 8 * (size_t)(e >> 2) + 4 * (size_t)(lane >> 5) + (size_t)(e & 3);
              if (n < (size_t)l.n_out && k < (size_t)l.k_in) {
                frag[lane * 16 + e] = (char)l.w[(n * taps + tap) * (size_t)l.k_in + k];
              }
            }
          }
        }
      }
    }
    out->b_off[i] = (uint32_t)image->size();
    image->resize(image->size() + n_tiles * 32 * 4, 0);
    std::memcpy(image->data() + out->b_off[i], l.b, 4 * (size_t)l.n_out);
  }
  image->resize((image->size() + 255) & ~(size_t)255, 0);
}

void ConvLaunch(const ConvImage& im, const char* d_image, int rows, int mode, const int32_t* order, const int32_t* n0,
                int seg, const unsigned char* obs, const unsigned char* mask, const unsigned char* status,
                float* policy, float* value, unsigned int* pending, hipStream_t stream) {
  ConvDev net{};
  net.H = im.H, net.W = im.W, net.C = im.C, net.A = im.A, net.D = im.D, net.L = im.L, net.P = im.P, net.G = im.G;
  net.scale_p = im.scale_p, net.scale_v = im.scale_v;
  net.base = d_image;
  for (int i = 0; i < im.layers; ++i) {
    net.w_off[i] = im.w_off[i], net.b_off[i] = im.b_off[i], net.shift[i] = im.shift[i];
  }
  if (im.lds > 48 * 1024) {
    EPA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&PgxConvEval),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)im.lds));
  }
  // (a segment has at most `rows` entries: blocks past it return at once)
  const int blocks = (rows + im.G - 1) / im.G;
  hipLaunchKernelGGL(PgxConvEval, dim3(blocks), dim3(kThreads), im.lds, stream, net, order, n0, seg, rows, mode, obs,
                     mask, status, policy, value, pending);
}

}  // namespace epa
