// The memory cell of the rollout actor on the int8 matrix cores (actor_memory.hip.h is the contract; DESIGN.md section 2
// "Rollout actor, memory cell").
//
// ActorMemoryCell: a block of four waves owns a tile of R = CellRows(F, M) rows, 64 or 32.
//   stage   The tile's rows [h ; x] enter LDS once, a row every CellStride bytes.  h comes from the state array in
//           16-byte words (M is a multiple of 32 and the array 16-byte aligned); x comes from the feature bytes
//           ActorFeatures wrote, whose nr * F bytes are one span of global memory: it is read as the aligned dwords that
//           cover it, and every byte of a dword finds its (row, column) by one division per dword and a running
//           column.  Columns between M + F and the next multiple of 32, and rows past the last one, are never written:
//           the weights there are zero, integers have no NaN, and what such rows give is never copied out.
//   units   A unit is (column tile ct of 32 columns m, row tile rt of 32 rows); the block has (M / 32) * (R / 32) of
//           them, wave w takes units w, w + 4, ..  Per k-step the wave reads the 2 KiB of (ct, kt) of the relaid weights
//           (CellImage) from global memory -- lane (r, hh) the 16 bytes of Wz and of Wn of row 32 ct + r -- and ONE
//           B fragment, 16 bytes of tile row 32 rt + r, from LDS, and issues v_mfma_i32_32x32x32_i8 twice: the
//           weights are the A operand, as in pgx_net.hip, so accumulator register reg of lane (r, hh) is column
//           32 ct + CellNeuron(reg, hh) of row 32 rt + r, for the gate and for the candidate alike.
//   blend   z and n of an element therefore meet in one lane's registers: no exchange.  The four columns of registers
//           4 g .. 4 g + 3 are consecutive bytes, so the old h is one dword of the staged tile and h' one dword of the
//           h' tile [R][M] behind it (a tile of its own: other waves still read the staged h as their B operand).
//   leave   After one barrier the h' tile, nr * M contiguous bytes, leaves in 16-byte words to the trunk's feature rows
//           and, unless nothing is to be committed, to the state array -- zeros for a row whose reset byte is set.  The
//           state may be the array h was read from: a block reads only its own rows, and all of them before the barrier.
// Plain vector loads and stores, no atomics, no scratch; integer sums: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "actor_memory.hip.h"

namespace epa {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

using actor::kCellBlock;

__global__ __launch_bounds__(kCellBlock) void ActorMemoryCell(ActorCellArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int F = a.F, M = a.M;
  const int steps = actor::CellKSteps(F, M), stride = actor::CellStride(F, M), R = actor::CellRows(F, M);
  const int r0 = blockIdx.x * R;
  const int nr = min(R, a.rows - r0);
  unsigned char* tile = lds;               // [R][stride]: h, x
  unsigned char* next = lds + R * stride;  // [R][M]: h'
  const int hw = M / 16;                   // 16-byte words of a row of h

  // ---- stage ----
  const uint4* h_src = reinterpret_cast<const uint4*>(a.h + (size_t)r0 * M);
  for (int i = tid; i < nr * hw; i += kCellBlock) {
    const int row = i / hw, c = i - row * hw;
    *reinterpret_cast<uint4*>(tile + row * stride + 16 * c) = h_src[i];
  }
  const unsigned char* x_src = a.x + (size_t)r0 * F;
  const int head = (int)(reinterpret_cast<uintptr_t>(x_src) & 3), total = nr * F;
  const uint32_t* x_words = reinterpret_cast<const uint32_t*>(x_src - head);
  for (int w = tid; w < (head + total + 3) / 4; w += kCellBlock) {
    const uint32_t word = x_words[w];
    const int idx = 4 * w - head;  // the span index of the dword's byte 0
    const int b0 = idx < 0 ? -idx : 0;
    int row = (idx + b0) / F, c = (idx + b0) - row * F;
    for (int b = b0; b < 4 && idx + b < total; ++b) {
      tile[row * stride + M + c] = (unsigned char)(word >> (8 * b));
      if (++c == F) c = 0, ++row;
    }
  }
  __syncthreads();

  // ---- units ----
  const int r = lane & 31, hh = lane >> 5;
  const int row_tiles = R / 32, units = (M / 32) * row_tiles;
  const v4i* image = reinterpret_cast<const v4i*>(a.image);
  for (int u = wave; u < units; u += kCellBlock / 64) {  // (uniform in a wave)
    const int ct = u / row_tiles, rt = u - ct * row_tiles;
    v16i az, an;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      az[reg] = a.bias_z[32 * ct + actor::CellNeuron(reg, hh)];
      an[reg] = a.bias_n[32 * ct + actor::CellNeuron(reg, hh)];
    }
    const v4i* w = image + (size_t)ct * steps * 128 + lane;
    const unsigned char* row = tile + (32 * rt + r) * stride;
    for (int kt = 0; kt < steps; ++kt) {
      const v4i wz = w[kt * 128], wn = w[kt * 128 + 64];
      const v4i b = *reinterpret_cast<const v4i*>(row + 32 * kt + 16 * hh);
      az = __builtin_amdgcn_mfma_i32_32x32x32_i8(wz, b, az, 0, 0, 0);
      an = __builtin_amdgcn_mfma_i32_32x32x32_i8(wn, b, an, 0, 0, 0);
    }
    // ---- blend ----
    unsigned char* out = next + (32 * rt + r) * M;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int m = 32 * ct + 8 * g + 4 * hh;
      const uint32_t old = *reinterpret_cast<const uint32_t*>(row + m);
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int32_t z = actor::CellGate(az[4 * g + b], a.shift_z);
        const int32_t n = actor::CellCandidate(an[4 * g + b], a.shift_n);
        word |= (uint32_t)actor::CellBlend(z, n, (int32_t)((old >> (8 * b)) & 255u)) << (8 * b);
      }
      *reinterpret_cast<uint32_t*>(out + m) = word;
    }
  }
  __syncthreads();

  // ---- leave ----
  const uint4* src = reinterpret_cast<const uint4*>(next);
  uint4* rows_out = reinterpret_cast<uint4*>(a.out + (size_t)r0 * M);
  uint4* h_out = a.h_out != nullptr ? reinterpret_cast<uint4*>(a.h_out + (size_t)r0 * M) : nullptr;
  for (int i = tid; i < nr * hw; i += kCellBlock) {
    uint4 v = src[i];
    rows_out[i] = v;
    if (h_out != nullptr) {
      if (a.reset != nullptr && a.reset[r0 + i / hw] != 0) v = make_uint4(0u, 0u, 0u, 0u);
      h_out[i] = v;
    }
  }
}

}  // namespace

void ActorLaunchCell(const ActorCellArgs& a, hipStream_t s) {
  const int R = actor::CellRows(a.F, a.M);
  hipLaunchKernelGGL(ActorMemoryCell, dim3((unsigned)((a.rows + R - 1) / R)), dim3(kCellBlock),
                     actor::CellLdsBytes(a.F, a.M), s, a);
}

}  // namespace epa
