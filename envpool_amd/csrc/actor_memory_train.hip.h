// Rollout actor with memory, training: the contract of the kernels behind `ActorModule.unroll(..., kernels=True)`
// (DESIGN.md section 2 "Rollout actor, memory cell: training").  Host + device, in the style of pgx_train.hip.h.  The
// authority is the torch twin of envpool_amd/actor.py (`cell`, `_cell_layer`, `unroll`); the trunk behind the cell is
// pgx_train.hip.h's.
//
// FORWARD, exact integers.  x bytes [T][N][F] (the features, 0 .. 127), h0 bytes [N][M] (0 .. 127), mask bytes [T][N],
// the cell's quantised layers Wz, Wn int8 [M][F + M] over [x ; h] with int32 biases and shifts sz, sn.  With
// h_{-1} = h0, for t = 0 .. T - 1:
//   h'_t = cell(x_t, h_{t-1})     actor_memory.hip.h: CellGate, CellCandidate, CellBlend
//   the trunk reads h'_t          (the forward writes hp bytes [T][N][M] for it)
//   h_t  = mask[t] ? h'_t : 0     the state rule; h_{T-1} is the unroll's third result
// Beside hp the handle keeps, per element (t, n, m), the input state h_{t-1} (one byte: the reduction's operand) and
// the two SAVED BYTES:
//   sz: the gate.  0 .. 128: z, whose clamp left the value as it was (64 + rs(.) in 0 .. 128 inclusive);
//       254: z = 0, the value was below 0;  255: z = 128, the value was above 128          (CellSavedGate, CellGateOf)
//   sn: the candidate.  Bits 0 .. 6: n; bit 7: the clamp changed the value, as in the trunk's saved bytes.
// Each is a plane [T][N][M], so that a lane's four consecutive columns are one dword of either.
//
// BACKWARD, the twin's straight-through rules.  Given dhp float32 [T][N][M] (the trunk's input gradient) and dh float32
// [N][M] (of the third result; may be absent).  carry_T = dh; for t = T - 1 .. 0, per element:
//   dy   = dhp_t + mask[t] carry_{t+1}
//   dz   = dy (h_{t-1} - n) / 128        dn = dy (128 - z) / 128        direct = dy z / 128
//   da_z = clamped gate ? 0 : dz 2^-sz   da_n = clamped candidate ? 0 : dn 2^-sn
//   carry_t = direct + da_z Wz[:, F:] + da_n Wn[:, F:]                    (a row times [2 M][M])
// dW = SUM over (t, n) of da^T [x_t ; h_{t-1}], db = SUM da, for both gates; dh0 = carry_0.  x gets no gradient.  A
// clamp passes the gradient where the integer before it lies in its range INCLUSIVE; rounding passes it through.
//
// LIMITS (CellTrainCheck, refused before any launch): F 1 .. 512, M a multiple of 32 in 32 .. 512, T >= 1,
// T N <= 2^20 (the trunk handle's row limit), the inner actor's kind 0 or 1, shifts 0 .. 24.
//
// ROWS PER BLOCK.  Rows never interact, so a block owns a tile of rows for the whole horizon, 64 or 32 of them
// (CellTrainRows): 64 where N gives every one of the device's 256 compute units a block of 64 (N >= 16384), else 32,
// which doubles the blocks of a small N; the backward also takes 32 where the tile of 64 does not fit its LDS
// (CellTrainBackLds > 160 KiB: M >= 320) -- halved rows, never spilled accumulators.
//
// THE DEVICE ARITHMETIC AND ITS ERROR CONSTANT (kCellTrainErr), per time step, derived as pgx_train.hip.h derives c:
// u = 2^-23 bounds one float32 addition or product in any rounding mode, an MFMA of 16 products counts as 16 additions
// in a row, and a sum whose terms pass through at most d additions is within d u SUM |terms| of the exact one.
//   elementwise: dy is one addition.  h - n, 128 - z and z are integers below 2^8, so dz, dn and direct are one rounded
//     product each (the divisions by 128 and the 2^-s are exact): 2 u on top of dy.  da_z and da_n are then SPLIT (bf16
//     hi + lo, pgx_train.hip.h: TrainSplit): 2^-16.
//   carry: the accumulator starts as `direct`; the GEMM adds 2 M <= 1024 exact products (an int8 weight times a bf16
//     term: 15 bits), twice over for hi and lo: d = 2048 additions in a row, 2048 u = 2^-12.  This alone is the 2^-12
//     of the trunk's constant, which is why that number is not taken over.
//   together: (2048 + 3) u + 2^-16 = 2.5976e-4  <=  kCellTrainErr = 2^-12 + 2^-16 + 2^-20 = 2.6035e-4.
//   dW, db: TrainReduce and TrainSum of pgx_train.hip.h over T N <= 2^20 rows, whose d <= 832 gives 9.9e-5, below the
//     constant; the da it reads are the split ones, already counted.
// The trunk's input gradient (NetTrain::InputGrad) is one more product dz W of pgx_train.hip.h: at most 1.38e-4.
// DEPTH.  The trunk has 2 L + 2 layers.  Its layer i has depth 2 L + 2 - i as before (TrainBackRow products and one
// reduction).  dhp has passed 2 L + 2 products.  A cell gradient sums terms that passed at most T time steps more and
// one reduction, dh0 T time steps: CellTrainDepth(L, T) = 2 L + 3 + T for all five.  With G_abs, the same backward
// over |W|, |dp|, |dh|, the local factors' magnitudes (|h - n|, 128 - z, z) and the same masks:
//   |g - g_exact| <= depth * kCellTrainErr * G_abs
// (the (1 + c)^m - 1 <= 1.01 m c of pgx_train.hip.h holds up to m c = 0.02, T about 70; beyond, the bound is first
// order only).  Underflow is not covered.
//
// DETERMINISM.  No atomics.  A block forms its rows' results in one fixed order; the reductions are TrainSlices',
// a function of the sizes only.
#ifndef ENVPOOL_AMD_CSRC_ACTOR_MEMORY_TRAIN_HIP_H_
#define ENVPOOL_AMD_CSRC_ACTOR_MEMORY_TRAIN_HIP_H_

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "actor_memory.hip.h"
#include "pgx_train.hip.h"

namespace epa {
namespace actor {

constexpr long long kCellTrainMaxRows = pgx::kTrainMaxRows;  // T N
constexpr double kCellTrainErr = 1.0 / 4096.0 + 1.0 / 65536.0 + 1.0 / 1048576.0;
constexpr int kCellTrainFillRows = 64 * 256;    // the least N whose tiles of 64 rows give every compute unit a block
constexpr int kCellTrainLdsLimit = 160 * 1024;  // gfx950: LDS of a compute unit, which one block may take
constexpr int kCellTrainPad = 4;                // words between two rows of the backward's da tile

PGX_HD inline int CellTrainDepth(int L, int T) { return 2 * L + 3 + T; }

inline bool CellTrainCheck(int F, int M, int kind, long long T, long long N, char* err, size_t err_bytes) {
  if (F < 1 || F > pgx::kNetMaxInputs) {
    std::snprintf(err, err_bytes, "cell_train: F = %d must be 1 .. %d", F, pgx::kNetMaxInputs);
  } else if (M < kMemoryMinWidth || M > kMemoryMaxWidth || M % 32 != 0) {
    std::snprintf(err, err_bytes, "cell_train: M = %d must be a multiple of 32 in %d .. %d", M, kMemoryMinWidth,
                  kMemoryMaxWidth);
  } else if (kind != kDiscrete && kind != kBox) {
    std::snprintf(err, err_bytes, "cell_train: kind = %d must be 0 (discrete) or 1 (box)", kind);
  } else if (T < 1 || N < 1 || T > kCellTrainMaxRows || N > kCellTrainMaxRows || T * N > kCellTrainMaxRows) {
    std::snprintf(err, err_bytes, "cell_train: T = %lld and N = %lld must be at least 1 with T N <= %lld", T, N,
                  kCellTrainMaxRows);
  } else {
    return true;
  }
  return false;
}

// ---- the saved bytes ---------------------------------------------------------------------------------------------------
// `pre` = 64 + rs(.), the gate before its clamp
PGX_HD inline uint32_t CellSavedGate(int32_t pre) { return pre < 0 ? 254u : (pre > 128 ? 255u : (uint32_t)pre); }
PGX_HD inline int32_t CellGateOf(uint32_t sz) { return sz <= 128u ? (int32_t)sz : (sz == 255u ? 128 : 0); }
PGX_HD inline bool CellGateClamped(uint32_t sz) { return sz > 128u; }
// `pre` = rs(.), the candidate before its clamp
PGX_HD inline uint32_t CellSavedCandidate(int32_t pre) {
  const int32_t n = pgx::NetAct(pre);
  return (uint32_t)n | (n != pre ? 128u : 0u);
}

// ---- the kernels' geometry (actor_memory_train.hip) --------------------------------------------------------------------
// Forward: two tiles of h, [R][M + kCellPad] bytes each (the step reads one and writes the other), and the staged x,
// [R][32 ceil(F / 32) + kCellPad].
PGX_HD inline int CellTrainXStride(int F) { return (F + 31) / 32 * 32 + kCellPad; }
PGX_HD inline size_t CellTrainFwdLds(int F, int M, int R) {
  return (size_t)R * (size_t)(2 * (M + kCellPad) + CellTrainXStride(F));
}
// Backward: the split da of the tile, [R][2 M + kCellTrainPad] words.
PGX_HD inline size_t CellTrainBackLds(int M, int R) { return (size_t)R * (size_t)(2 * M + kCellTrainPad) * 4; }
PGX_HD inline int CellTrainRows(int N) { return N >= kCellTrainFillRows ? 64 : 32; }
PGX_HD inline int CellTrainBackRows(int N, int M) {
  return CellTrainRows(N) == 64 && CellTrainBackLds(M, 64) <= (size_t)kCellTrainLdsLimit ? 64 : 32;
}

}  // namespace actor
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_ACTOR_MEMORY_TRAIN_HIP_H_
