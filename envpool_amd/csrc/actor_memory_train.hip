// The memory cell of the rollout actor, training, on the matrix cores (actor_memory_train.hip.h is the contract;
// DESIGN.md section 2 "Rollout actor, memory cell: training").  Three kernels and the handle that owns their memory;
// the weight gradients are TrainReduce's (pgx_train.hip).  Rows never interact across n, so in both big kernels a block
// of four waves owns a tile of R rows (CellTrainRows) and runs the time loop itself: one launch per horizon.
//
// CellTrainPack, once per forward: the caller's quantised layers Wz, Wn, int8 [M][F + M] on the device, into
//   CellImage's fragments (actor_memory.hip.h: the forward's A operand) and the transposes of their h-columns as ONE
//   bf16 matrix Wt [M][2 M], Wt[k][n] = Wz[n][F + k] for n < M and Wn[n - M][F + k] behind: the backward's B operand.
// CellTrainForward: ActorMemoryCell's tiling inside a time loop.  LDS holds two tiles of h, [R][M + 16] bytes, and the
//   staged x_t, [R][32 ceil(F / 32) + 16]; step t reads one h tile and writes the other.  Per step: the block copies
//   its input states to the handle (16-byte words: the reduction's operand) and stages x_t as ActorMemoryCell does;
//   after a barrier wave w takes the units (column tile ct, row tile rt) w, w + 4, .. -- the weights of (ct, k-step) are
//   the A operand of v_mfma_i32_32x32x32_i8 for the gate and the candidate, 16 bytes of tile row 32 rt + r the B
//   operand, from the h tile for the first M / 32 k-steps and from x behind --, so that accumulator register reg of
//   lane (r, hh) is column 32 ct + CellNeuron(reg, hh) of row 32 rt + r for z and n alike.  The epilogue blends in
//   registers and stores, per four consecutive columns, one dword each of h'_t, of the gate's saved bytes and of the
//   candidate's to global memory, and h_t -- zeros where mask[t] is 0 -- to the other h tile.  A second barrier ends
//   the step.  After the last step the h tile leaves as the unroll's state.
// CellTrainBackward<TT, RT>: the same ownership for t = T - 1 .. 0, R = 32 RT.  Wave w owns the column tiles
//   kt = w, w + 4, .. (TT of them, M <= 128 TT) of its rows; their accumulators, v16f [TT][RT], ARE the carry and stay in
//   registers over the whole horizon: register reg of lane (c, hh) is column 32 kt + c of row 32 rt + CellNeuron(reg,
//   hh), the C/D map of v_mfma_f32_32x32x16_bf16, as in TrainBackRow.  Per step the lane does the elementwise part for
//   exactly those elements: dy from dhp and the masked carry, the saved bytes and the input state (bytes, 32
//   consecutive ones per half wave), the split da_z and da_n to global memory (128 bytes of a row per register) and to
//   the LDS tile [R][2 M + 4] words, and `direct` into the accumulator.  After a barrier the carry GEMM
//   [R][2 M] x [2 M][M]: per 16 n the lane (r, hh) reads the 8 split words tile[32 rt + r][16 ns + 8 hh ..] and tears
//   them into a hi and a lo fragment (A), reads Wt[32 kt + c][16 ns + 8 hh ..] (B, one 128-bit load) and issues the
//   MFMA twice.  A second barrier ends the step; after t = 0 the accumulators are dh0.
//   LDS: R (2 M + 4) 4 bytes, up to 131 584 (M = 512, R = 32): above 48 KiB the kernels opt in with
//   hipFuncSetAttribute, as NetTrain does.
// Plain vector loads and stores, no atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "engine.h"
#include "actor_memory_train.hip.h"

namespace epa {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

using actor::kCellBlock;
using actor::kCellPad;
using actor::kCellTrainPad;

// ---------------------------------------------------------------------------
// CellTrainPack
// ---------------------------------------------------------------------------
struct CellPackArgs {
  int F, M;
  const signed char* w[2];  // [M][F + M]
  char* image;              // CellImage's layout
  uint16_t* wt;             // bf16 [M][2 M]
};

__global__ __launch_bounds__(256) void CellTrainPack(CellPackArgs a) {
  const int F = a.F, M = a.M, K = F + M, steps = actor::CellKSteps(F, M);
  const int image_bytes = (M / 32) * steps * 2048, wt_elems = 2 * M * M;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < image_bytes + wt_elems; q += gridDim.x * 256) {
    if (q < image_bytes) {
      const int b = q & 15, lane = (q >> 4) & 63, g = (q >> 10) & 1, tile = q >> 11;
      const int ct = tile / steps, kt = tile - ct * steps;
      const int kk = 32 * kt + 16 * (lane >> 5) + b;
      const signed char* row = a.w[g] + (size_t)(32 * ct + (lane & 31)) * K;
      a.image[q] = kk < M ? (char)row[F + kk] : (kk < K ? (char)row[kk - M] : (char)0);
    } else {
      const int e = q - image_bytes, k = e / (2 * M), n2 = e - k * 2 * M;
      const int g = n2 >= M ? 1 : 0, n = n2 - g * M;
      const float v = (float)a.w[g][(size_t)n * K + F + k];
      a.wt[e] = (uint16_t)((uint32_t)pgx::NetFloatBits(v) >> 16);  // (7 bits: exact)
    }
  }
}

// ---------------------------------------------------------------------------
// CellTrainForward
// ---------------------------------------------------------------------------
struct CellFwdArgs {
  int T, N, F, M, R;
  int shift_z, shift_n;
  const char* image;
  const int32_t* bias_z;      // [M] each
  const int32_t* bias_n;
  const unsigned char* x;     // [T][N][F]
  const unsigned char* h0;    // [N][M], 16-byte aligned
  const unsigned char* mask;  // [T][N]
  unsigned char* hp;          // [T][N][M]: h'
  unsigned char* h;           // [N][M]: the state after the last step
  unsigned char* hin;         // [T][N][M]: the state every step read
  unsigned char* sz;          // [T][N][M] each: the saved bytes
  unsigned char* sn;
};

__global__ __launch_bounds__(kCellBlock) void CellTrainForward(CellFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int F = a.F, M = a.M, N = a.N, R = a.R;
  const int hs = M + kCellPad, xs = actor::CellTrainXStride(F), steps = actor::CellKSteps(F, M), h_steps = M / 32;
  const int r0 = blockIdx.x * R;
  const int nr = min(R, N - r0);
  unsigned char* xbuf = lds + 2 * R * hs;
  const int hw = M / 16;  // 16-byte words of a row of h

  // zeros everywhere: the columns of x behind F and the rows behind nr are never written again
  for (int i = tid; i < R * (2 * hs + xs) / 16; i += kCellBlock) {
    reinterpret_cast<uint4*>(lds)[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  const uint4* h_src = reinterpret_cast<const uint4*>(a.h0 + (size_t)r0 * M);
  for (int i = tid; i < nr * hw; i += kCellBlock) {
    const int row = i / hw, c = i - row * hw;
    *reinterpret_cast<uint4*>(lds + row * hs + 16 * c) = h_src[i];
  }
  __syncthreads();

  const int row_tiles = R / 32, units = (M / 32) * row_tiles;
  const v4i* image = reinterpret_cast<const v4i*>(a.image);
  for (int t = 0; t < a.T; ++t) {
    const unsigned char* cur = lds + (t & 1) * R * hs;
    unsigned char* nxt = lds + ((t & 1) ^ 1) * R * hs;
    const size_t at = (size_t)t * N + r0;  // the tile's first row of slot t
    // ---- the input states leave; x_t enters ----
    uint4* hin = reinterpret_cast<uint4*>(a.hin + at * M);
    for (int i = tid; i < nr * hw; i += kCellBlock) {
      const int row = i / hw, c = i - row * hw;
      hin[i] = *reinterpret_cast<const uint4*>(cur + row * hs + 16 * c);
    }
    const unsigned char* x_src = a.x + at * F;
    const int head = (int)(reinterpret_cast<uintptr_t>(x_src) & 3), total = nr * F;
    const uint32_t* x_words = reinterpret_cast<const uint32_t*>(x_src - head);
    for (int w = tid; w < (head + total + 3) / 4; w += kCellBlock) {
      const uint32_t word = x_words[w];
      const int idx = 4 * w - head;  // the span index of the dword's byte 0
      const int b0 = idx < 0 ? -idx : 0;
      int row = (idx + b0) / F, c = (idx + b0) - row * F;
      for (int b = b0; b < 4 && idx + b < total; ++b) {
        xbuf[row * xs + c] = (unsigned char)(word >> (8 * b));
        if (++c == F) c = 0, ++row;
      }
    }
    __syncthreads();

    // ---- units ----
    for (int u = wave; u < units; u += kCellBlock / 64) {  // (uniform in a wave)
      const int ct = u / row_tiles, rt = u - ct * row_tiles;
      v16i az, an;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        az[reg] = a.bias_z[32 * ct + actor::CellNeuron(reg, hh)];
        an[reg] = a.bias_n[32 * ct + actor::CellNeuron(reg, hh)];
      }
      const v4i* w = image + (size_t)ct * steps * 128 + lane;
      const int rl = 32 * rt + r;
      const unsigned char* h_row = cur + rl * hs;
      const unsigned char* x_row = xbuf + rl * xs;
      for (int kt = 0; kt < steps; ++kt) {
        const v4i wz = w[kt * 128], wn = w[kt * 128 + 64];
        const unsigned char* src = kt < h_steps ? h_row + 32 * kt : x_row + 32 * (kt - h_steps);
        const v4i b = *reinterpret_cast<const v4i*>(src + 16 * hh);
        az = __builtin_amdgcn_mfma_i32_32x32x32_i8(wz, b, az, 0, 0, 0);
        an = __builtin_amdgcn_mfma_i32_32x32x32_i8(wn, b, an, 0, 0, 0);
      }
      // ---- blend ----
      const bool valid = rl < nr;
      const bool keep = valid && a.mask[at + rl] != 0;
      const size_t out = (at + rl) * M;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int m = 32 * ct + 8 * g + 4 * hh;
        const uint32_t old = *reinterpret_cast<const uint32_t*>(h_row + m);
        uint32_t word = 0, word_z = 0, word_n = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int32_t pre_z = 64 + pgx::NetRs(az[4 * g + b], a.shift_z);
          const int32_t pre_n = pgx::NetRs(an[4 * g + b], a.shift_n);
          const int32_t z = pre_z < 0 ? 0 : (pre_z > 128 ? 128 : pre_z);
          const int32_t n = pgx::NetAct(pre_n);
          word |= (uint32_t)actor::CellBlend(z, n, (int32_t)((old >> (8 * b)) & 255u)) << (8 * b);
          word_z |= actor::CellSavedGate(pre_z) << (8 * b);
          word_n |= actor::CellSavedCandidate(pre_n) << (8 * b);
        }
        *reinterpret_cast<uint32_t*>(nxt + rl * hs + m) = keep ? word : 0u;
        if (valid) {
          *reinterpret_cast<uint32_t*>(a.hp + out + m) = word;
          *reinterpret_cast<uint32_t*>(a.sz + out + m) = word_z;
          *reinterpret_cast<uint32_t*>(a.sn + out + m) = word_n;
        }
      }
    }
    __syncthreads();
  }

  // ---- leave ----
  const unsigned char* last = lds + (a.T & 1) * R * hs;
  uint4* h_out = reinterpret_cast<uint4*>(a.h + (size_t)r0 * M);
  for (int i = tid; i < nr * hw; i += kCellBlock) {
    const int row = i / hw, c = i - row * hw;
    h_out[i] = *reinterpret_cast<const uint4*>(last + row * hs + 16 * c);
  }
}

// ---------------------------------------------------------------------------
// CellTrainBackward
// ---------------------------------------------------------------------------
// eight split words -> the fragment of their hi halves and the fragment of their lo halves (pgx_train.hip: TearSplit)
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

struct CellBackArgs {
  int T, N, M;
  float scale_z, scale_n;     // 2^-sz, 2^-sn
  const float* dhp;           // [T][N][M]
  const float* dh;            // [N][M] or null
  const unsigned char* mask;  // [T][N]
  const unsigned char* hin;   // [T][N][M] each: what the forward kept
  const unsigned char* sz;
  const unsigned char* sn;
  const uint16_t* wt;         // bf16 [M][2 M]
  uint32_t* da;               // [T N][2 M] split: da_z, then da_n
  float* dh0;                 // [N][M]
};

template <int TT, int RT>
__global__ __launch_bounds__(256) void CellTrainBackward(CellBackArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t tile[];  // [32 RT][2 M + kCellTrainPad]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, hh = lane >> 5;
  const int M = a.M, N = a.N, tiles = M / 32, pitch = 2 * M + kCellTrainPad;
  const int r0 = (int)blockIdx.x * 32 * RT;
  v16f acc[TT][RT];  // the carry
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = r0 + 32 * rt + actor::CellNeuron(reg, hh), col = 32 * (wave + 4 * tt) + c;
        acc[tt][rt][reg] = a.dh != nullptr && row < N && col < M ? a.dh[(size_t)row * M + col] : 0.0f;
      }
    }
  }
  for (int t = a.T - 1; t >= 0; --t) {
    // ---- elementwise: the lane's own elements ----
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const int kt = wave + 4 * tt;
      if (kt >= tiles) continue;  // (uniform in the wave)
      const int col = 32 * kt + c;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int rl = 32 * rt + actor::CellNeuron(reg, hh), row = r0 + rl;
          float direct = 0.0f;
          uint32_t split_z = 0u, split_n = 0u;
          if (row < N) {
            const size_t slot = (size_t)t * N + row, e = slot * M + col;
            const float dy = a.dhp[e] + (a.mask[slot] != 0 ? acc[tt][rt][reg] : 0.0f);
            const uint32_t bz = a.sz[e], bn = a.sn[e];
            const int32_t z = actor::CellGateOf(bz), n = (int32_t)(bn & 127u), h = (int32_t)a.hin[e];
            const float dz = dy * (float)(h - n) * 0.0078125f;
            const float dn = dy * (float)(128 - z) * 0.0078125f;
            direct = dy * (float)z * 0.0078125f;
            split_z = pgx::TrainSplit(actor::CellGateClamped(bz) ? 0.0f : dz * a.scale_z);
            split_n = pgx::TrainSplit((bn & 128u) != 0u ? 0.0f : dn * a.scale_n);
            a.da[slot * 2 * M + col] = split_z;
            a.da[slot * 2 * M + M + col] = split_n;
          }
          tile[rl * pitch + col] = split_z;
          tile[rl * pitch + M + col] = split_n;
          acc[tt][rt][reg] = direct;
        }
      }
    }
    __syncthreads();
    // ---- the carry: acc += da [R][2 M] x Wt^T ----
    for (int ns = 0; ns < 2 * M / 16; ++ns) {
      v8bf hi[RT], lo[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const v4i* src = reinterpret_cast<const v4i*>(tile + (32 * rt + c) * pitch + 16 * ns + 8 * hh);
        TearSplit(src[0], src[1], &hi[rt], &lo[rt]);
      }
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const int kt = wave + 4 * tt;
        if (kt < tiles) {  // (uniform in the wave)
          const v4i raw = *reinterpret_cast<const v4i*>(a.wt + (size_t)(32 * kt + c) * 2 * M + 16 * ns + 8 * hh);
          const v8bf b = __builtin_bit_cast(v8bf, raw);
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            acc[tt][rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hi[rt], b, acc[tt][rt], 0, 0, 0);
            acc[tt][rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lo[rt], b, acc[tt][rt], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();  // (the tile is read: the next step writes it)
  }
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) {
    const int kt = wave + 4 * tt;
    if (kt >= tiles) continue;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = r0 + 32 * rt + actor::CellNeuron(reg, hh);
        if (row < N) a.dh0[(size_t)row * M + 32 * kt + c] = acc[tt][rt][reg];
      }
    }
  }
}

using BackKernel = void (*)(CellBackArgs);
BackKernel BackKernelOf(int M, int R) {
  const int tt = (M + 127) / 128;
  if (R == 64) return tt == 1 ? CellTrainBackward<1, 2> : (tt == 2 ? CellTrainBackward<2, 2> : CellTrainBackward<3, 2>);
  return tt == 1 ? CellTrainBackward<1, 1>
                 : (tt == 2 ? CellTrainBackward<2, 1> : (tt == 3 ? CellTrainBackward<3, 1> : CellTrainBackward<4, 1>));
}

size_t Align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

// ---------------------------------------------------------------------------
// the handle (engine.h: CellTrain)
// ---------------------------------------------------------------------------
struct CellTrain::Layout {
  size_t image, wt, x, mask, hin, sz, sn, da, ws, db;  // byte offsets into the block
};

CellTrain::CellTrain(int device, int F, int M, int kind, long long max_rows)
    : device_(device), F_(F), M_(M), max_rows_((int)max_rows), at_(new Layout()) {
  char err[200];
  if (!actor::CellTrainCheck(F, M, kind, 1, max_rows, err, sizeof(err))) throw std::invalid_argument(err);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
  if (device < 0 || device >= count) {
    throw std::invalid_argument("cell_train_create: device = " + std::to_string(device) + " must be 0 .. " +
                                std::to_string(count - 1));
  }
  const size_t rows = (size_t)max_rows_, m = (size_t)M;
  const size_t ws = std::max((size_t)pgx::TrainMostSlices(max_rows_, 2 * M, F) * 2 * m * ((size_t)F + 1),
                             (size_t)pgx::TrainMostSlices(max_rows_, 2 * M, M) * 2 * m * (m + 1)) * 4;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += Align256(bytes);
    return here;
  };
  at_->image = take(actor::CellImageBytes(F, M)), at_->wt = take(2 * m * m * 2);
  at_->x = take(rows * F + 4), at_->mask = take(rows);
  at_->hin = take(rows * m), at_->sz = take(rows * m), at_->sn = take(rows * m);
  at_->da = take(rows * 2 * m * 4), at_->ws = take(ws), at_->db = take(2 * m * 4);
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  try {
    mem_.Alloc(at);
    // (either tile of rows may be launched: both opt in where they need to)
    const size_t fwd = actor::CellTrainFwdLds(F, M, 64);
    if (fwd > 48 * 1024) {
      EPA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&CellTrainForward),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)fwd));
    }
    for (int R = 32; R <= 64; R += 32) {
      const size_t back = actor::CellTrainBackLds(M, R);
      if (back > 48 * 1024 && back <= (size_t)actor::kCellTrainLdsLimit) {
        EPA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(BackKernelOf(M, R)),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)back));
      }
    }
  } catch (...) {
    mem_.Free();
    (void)hipSetDevice(before);
    throw;
  }
  EPA_HIP(hipSetDevice(before));
}

CellTrain::~CellTrain() {
  int before = 0;
  if (hipGetDevice(&before) != hipSuccess) return;
  (void)hipSetDevice(device_);
  mem_.Free();
  (void)hipSetDevice(before);
}

void CellTrain::Forward(hipStream_t stream, int T, int N, const void* const* d_w, const void* const* d_b,
                        const int32_t* shifts, const void* d_x, const void* d_h0, const void* d_mask, void* d_hp,
                        void* d_h) {
  char err[200];
  if (d_w == nullptr || d_b == nullptr || shifts == nullptr || d_x == nullptr || d_h0 == nullptr || d_mask == nullptr ||
      d_hp == nullptr || d_h == nullptr || d_w[0] == nullptr || d_w[1] == nullptr || d_b[0] == nullptr ||
      d_b[1] == nullptr) {
    throw std::invalid_argument("cell_train_forward: null argument");
  }
  if (!actor::CellTrainCheck(F_, M_, actor::kDiscrete, T, N, err, sizeof(err))) throw std::invalid_argument(err);
  if ((long long)T * N > max_rows_) {
    throw std::invalid_argument("cell_train_forward: T N = " + std::to_string((long long)T * N) + " must be at most " +
                                std::to_string(max_rows_) + " (the handle's max_rows)");
  }
  for (int g = 0; g < 2; ++g) {
    if (shifts[g] < 0 || shifts[g] > pgx::kNetMaxShift) {
      throw std::invalid_argument("cell_train_forward: shift = " + std::to_string(shifts[g]) + " must be 0 .. " +
                                  std::to_string(pgx::kNetMaxShift));
    }
  }
  if (((reinterpret_cast<uintptr_t>(d_h0) | reinterpret_cast<uintptr_t>(d_hp) | reinterpret_cast<uintptr_t>(d_h)) &
       15) != 0) {
    throw std::invalid_argument("cell_train_forward: d_h0, d_hp and d_h must be 16-byte aligned");
  }
  const size_t rows = (size_t)T * N;
  unsigned char* base = reinterpret_cast<unsigned char*>(mem_.p);
  CellPackArgs pack{F_, M_, {static_cast<const signed char*>(d_w[0]), static_cast<const signed char*>(d_w[1])},
                    mem_.p + at_->image, reinterpret_cast<uint16_t*>(mem_.p + at_->wt)};
  CellFwdArgs f{};
  f.T = T, f.N = N, f.F = F_, f.M = M_, f.R = actor::CellTrainRows(N);
  f.shift_z = shift_[0] = shifts[0], f.shift_n = shift_[1] = shifts[1];
  f.image = pack.image;
  f.bias_z = static_cast<const int32_t*>(d_b[0]), f.bias_n = static_cast<const int32_t*>(d_b[1]);
  f.x = base + at_->x, f.h0 = static_cast<const unsigned char*>(d_h0), f.mask = base + at_->mask;
  f.hp = static_cast<unsigned char*>(d_hp), f.h = static_cast<unsigned char*>(d_h);
  f.hin = base + at_->hin, f.sz = base + at_->sz, f.sn = base + at_->sn;
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  T_ = N_ = 0;  // (a forward that fails leaves nothing to go back through)
  hipLaunchKernelGGL(CellTrainPack, dim3(64), dim3(256), 0, stream, pack);
  hipError_t copied = hipMemcpyAsync(base + at_->x, d_x, rows * F_, hipMemcpyDeviceToDevice, stream);
  if (copied == hipSuccess) {
    copied = hipMemcpyAsync(base + at_->mask, d_mask, rows, hipMemcpyDeviceToDevice, stream);
  }
  if (copied == hipSuccess) {
    hipLaunchKernelGGL(CellTrainForward, dim3((unsigned)((N + f.R - 1) / f.R)), dim3(kCellBlock),
                       actor::CellTrainFwdLds(F_, M_, f.R), stream, f);
  }
  const hipError_t launched = hipGetLastError();
  (void)hipSetDevice(before);
  EPA_HIP(copied);
  EPA_HIP(launched);
  T_ = T, N_ = N;
}

void CellTrain::Backward(hipStream_t stream, int T, int N, const void* d_dhp, const void* d_dh, void* d_dw, void* d_db,
                         void* d_dh0) {
  if (d_dhp == nullptr || d_dw == nullptr || d_db == nullptr || d_dh0 == nullptr) {
    throw std::invalid_argument("cell_train_backward: null argument");
  }
  if (T_ == 0) throw std::invalid_argument("cell_train_backward: no forward has been made with this handle");
  if (T != T_ || N != N_) {
    throw std::invalid_argument("cell_train_backward: T = " + std::to_string(T) + ", N = " + std::to_string(N) +
                                ", but the last forward had " + std::to_string(T_) + " and " + std::to_string(N_));
  }
  const unsigned char* base = reinterpret_cast<const unsigned char*>(mem_.p);
  const int M = M_, K = F_ + M_, rows = T * N, R = actor::CellTrainBackRows(N, M);
  uint32_t* da = reinterpret_cast<uint32_t*>(mem_.p + at_->da);
  float* ws = reinterpret_cast<float*>(mem_.p + at_->ws);
  CellBackArgs b{T, N, M, 1.0f / (float)(1 << shift_[0]), 1.0f / (float)(1 << shift_[1]),
                 static_cast<const float*>(d_dhp), static_cast<const float*>(d_dh), base + at_->mask, base + at_->hin,
                 base + at_->sz, base + at_->sn, reinterpret_cast<const uint16_t*>(mem_.p + at_->wt), da,
                 static_cast<float*>(d_dh0)};
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  hipLaunchKernelGGL(BackKernelOf(M, R), dim3((unsigned)((N + R - 1) / R)), dim3(256), actor::CellTrainBackLds(M, R),
                     stream, b);
  // both gates share the input: one reduction of N_out = 2 M over the x-columns and one over the h-columns, each into
  // its columns of dW [2 M][F + M]; db comes out of either (the same bits), the second goes to the block
  float* dw = static_cast<float*>(d_dw);
  TrainReduceLaunchLd(rows, 2 * M, F_, da, 2 * M, base + at_->x, ws, dw, K, static_cast<float*>(d_db), stream);
  TrainReduceLaunchLd(rows, 2 * M, M, da, 2 * M, base + at_->hin, ws, dw + F_, K,
                      reinterpret_cast<float*>(mem_.p + at_->db), stream);
  const hipError_t launched = hipGetLastError();
  (void)hipSetDevice(before);
  EPA_HIP(launched);
}

}  // namespace epa
