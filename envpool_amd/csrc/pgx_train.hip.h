// PGX built-in network, training: the contract of the forward and backward kernels behind `Net.module(kernels=True)`
// (DESIGN.md "PGX built-in network: training").  Host + device: the kernels (pgx_train.hip) and the g++ harness of the
// tests (tests/cpu_harness/pgx_train_host.cpp) restate the torch twin of envpool_amd/pgx/net.py (`_make_module`), which
// is the authority.
//
// FORWARD.  p = the head's int32 sums of pgx_net.hip.h, from input bytes 0 .. 127 (PGX observations are 0 / 1, the
// actor's features fill 0 .. 127), int8 weights [N][K] row-major in -127 .. 127 and int32 biases: the master parameters
// quantised as the twin does, clamp(round(w), -127, 127) and round(b), half to even.  Beside p the forward keeps one
// byte per activation, the SAVED BYTES: activation j of a row, j = 0 the trunk's h, j = 1 + 2 l the t and j = 2 + 2 l the
// h of block l, lies at saved[(j * rows + row) * D + n]; bits 0 .. 6 are the activation 0 .. 127 and bit 7 is set where
// the clamp changed the value (the value before the clamp was below 0 or above 127).  The backward needs nothing else of
// the forward but the input bytes.
//
// BACKWARD, the twin's straight-through rules.  Given dp float32 [rows][A + 1]: a layer out = rs(W x + b, s) has
// dz = dout * 2^-s (exact), dW = dz^T x, db = SUM_rows dz, dx = dz W.  clamp(., 0, 127) passes the gradient where the
// value before the clamp lies in 0 .. 127 INCLUSIVE (bit 7 clear).  In a block the gradient of
// h_new = clamp(layer2(t) + h, 0, 127), after its clamp's mask, goes to layer2's output and to h alike.  Rounding and the
// weight clamp pass gradients through, so the gradient of a master weight is dW.  The input gets none: layer 0's dx is
// not computed.
//
// LIMITS: the net's own (F 1 .. 512, D a multiple of 32 in 32 .. 512, L 0 .. 8, A 1 .. 127, shifts 0 .. 24 and 0 for
// the head) and rows 1 .. 2^20 (TrainCheck).
//
// THE DEVICE ARITHMETIC AND ITS ERROR CONSTANT c (kTrainErr).  The kernels hold every dz as a SPLIT float: a pair of
// bf16 numbers hi + lo in one 32-bit word (TrainSplit), hi = bf16(v) and lo = bf16(v - hi), both round to nearest even.
// v - hi is exact in float32 and at most 2^-8 |v| (bf16 has 8 significant bits), so |v - (hi + lo)| <= 2^-16 |v|.  Every product
// of a GEMM has one factor that is an integer below 2^7 in magnitude (a weight or a saved byte, exact in bf16) and one
// bf16 term of a split dz (8 significant bits): 15 bits, exact in the float32 accumulator.  What is left is the
// rounding of the additions.  Take u = 2^-23 for one addition, which holds for any rounding mode of the matrix core's
// accumulator, and count an MFMA of 16 products as 16 additions in a row.  A sum whose terms pass through at most d
// additions is within d u SUM |terms| of the exact one (the (1 + u)^d - 1 of the textbook, d u < 2^-12 here).
//   dx = dz W (TrainBackRow): N <= 512 terms, twice for hi and lo, in one accumulator: d = 1024; one addition of the
//     residual branch, and the split of the result, 2^-16: at most (1025 * 2^-23 + 2^-16) = 1.38e-4 of the sum of the
//     magnitudes.  Masking and the scaling by 2^-s are exact.
//   dW = dz^T x, db (TrainReduce, TrainSum): the rows of a slice are summed 128 at a time (d = 256 with hi and lo), the
//     runs of 128 added one after another in a second accumulator (a slice has at most kTrainSliceRows = 8192 rows:
//     d = 64), the slices added in their order (at most kTrainMaxSlices = 512: d = 512): d <= 832, 9.9e-5.  The head's
//     dz is the split of dp, 2^-16 more: 1.15e-4.
// Both are below c = 2^-12 = 2.44e-4.  A gradient `m` layers below the output (the head's own: m = 1) has passed m - 1
// products dz W and one reduction, so with G_abs, the same backward pass over |W|, |dp| and the same masks, which
// bounds the sums of magnitudes at every stage:  |dW - dW_exact| <= ((1 + c)^m - 1) G_abs <= 1.01 m c G_abs for m <= 18,
// and the measured stage constants leave that 1 % many times over, so the tests assert  m c G_abs.  (Underflow is not
// covered: a |dz| below 2^-110 loses bits of its lo term.)
//
// DETERMINISM.  No atomics.  The slices of a reduction are TrainSlices(rows, N, K), a function of the sizes only; a
// slice's partial sums are formed in one fixed order by one block and added in ascending slice order by one thread.
#ifndef ENVPOOL_AMD_CSRC_PGX_TRAIN_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_TRAIN_HIP_H_

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pgx_net.hip.h"

namespace epa {
namespace pgx {

constexpr int kTrainMaxRows = 1 << 20;
constexpr double kTrainErr = 1.0 / 4096.0;  // c
constexpr int kTrainRunRows = 128;           // rows added in the first accumulator before it is folded
constexpr int kTrainSliceRows = 8192;        // the most rows of a slice
constexpr int kTrainMaxSlices = 512;
constexpr int kTrainTile = 64;               // a reduction block's tile of N and of K

// false with the reason in `err`: everything the contract bounds
inline bool TrainCheck(int F, int A, int D, int L, long long rows, char* err, size_t err_bytes) {
  if (F < 1 || F > kNetMaxInputs) {
    std::snprintf(err, err_bytes, "net_train: F = %d must be 1 .. %d", F, kNetMaxInputs);
  } else if (A < 1 || A > kNetMaxActions) {
    std::snprintf(err, err_bytes, "net_train: A = %d must be 1 .. %d", A, kNetMaxActions);
  } else if (D < kNetMinWidth || D > kNetMaxWidth || D % 32 != 0) {
    std::snprintf(err, err_bytes, "net_train: D = %d must be a multiple of 32 in %d .. %d", D, kNetMinWidth,
                  kNetMaxWidth);
  } else if (L < 0 || L > kNetMaxBlocks) {
    std::snprintf(err, err_bytes, "net_train: L = %d must be 0 .. %d", L, kNetMaxBlocks);
  } else if (rows < 1 || rows > kTrainMaxRows) {
    std::snprintf(err, err_bytes, "net_train: rows = %lld must be 1 .. %d", rows, kTrainMaxRows);
  } else {
    return true;
  }
  return false;
}

inline bool TrainCheckShifts(int L, const int32_t* shifts, char* err, size_t err_bytes) {
  for (int i = 0; i < 2 * L + 2; ++i) {
    const int top = i == 2 * L + 1 ? 0 : kNetMaxShift;
    if (shifts[i] < 0 || shifts[i] > top) {
      std::snprintf(err, err_bytes, "net_train: layer %d: shift = %d must be 0 .. %d", i, shifts[i], top);
      return false;
    }
  }
  return true;
}

// bf16(v), round to nearest even, as the upper 16 bits of a float (finite v)
PGX_HD inline uint32_t TrainBf16(float v) {
  const uint32_t b = (uint32_t)NetFloatBits(v);
  return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}
// the split of v: hi in the upper half, lo in the lower
PGX_HD inline uint32_t TrainSplit(float v) {
  const uint32_t hi = TrainBf16(v);
  const float rest = v - NetBitsFloat((int32_t)(hi << 16));
  return (hi << 16) | TrainBf16(rest);
}
PGX_HD inline float TrainJoin(uint32_t s) {
  return NetBitsFloat((int32_t)(s & 0xffff0000u)) + NetBitsFloat((int32_t)(s << 16));
}

// The slices of the reduction of a layer [N][K] over `rows`: enough blocks to fill the device at few rows, no slice
// past kTrainSliceRows, whole runs of kTrainRunRows.  The sizes decide, nothing else.
struct TrainSlicing {
  int slices, slice_rows;
};
PGX_HD inline TrainSlicing TrainSlices(int rows, int N, int K) {
  const int tiles = ((N + kTrainTile - 1) / kTrainTile) * ((K + kTrainTile - 1) / kTrainTile);
  int want = (1024 + tiles - 1) / tiles;
  const int runs = (rows + kTrainRunRows - 1) / kTrainRunRows;
  want = want < runs ? want : runs;
  const int least = (rows + kTrainSliceRows - 1) / kTrainSliceRows;
  want = want > least ? want : least;
  want = want < kTrainMaxSlices ? want : kTrainMaxSlices;
  TrainSlicing s;
  s.slice_rows = ((rows + want - 1) / want + kTrainRunRows - 1) / kTrainRunRows * kTrainRunRows;
  s.slices = (rows + s.slice_rows - 1) / s.slice_rows;
  return s;
}

// No call of at most `max_rows` rows has more slices than this: what a workspace is sized by.
inline int TrainMostSlices(int max_rows, int N, int K) {
  const int tiles = ((N + kTrainTile - 1) / kTrainTile) * ((K + kTrainTile - 1) / kTrainTile);
  const int want = (1024 + tiles - 1) / tiles, least = (max_rows + kTrainSliceRows - 1) / kTrainSliceRows;
  const int most = want > least ? want : least;
  return most < kTrainMaxSlices ? most : kTrainMaxSlices;
}

// A network as the training calls take it: per layer the quantised weights [N][K] and biases, and the shift.
struct TrainNet {
  int F, A, D, L;
  const signed char* w[kNetMaxLayers];
  const int32_t* b[kNetMaxLayers];
  int32_t shift[kNetMaxLayers];
  int layers() const { return 2 * L + 2; }
  int n_out(int i) const { return i == 2 * L + 1 ? A + 1 : D; }
  int k_in(int i) const { return i == 0 ? F : D; }
};

// The forward by the book: x [rows][F] -> saved [(2 L + 1)][rows][D] and p [rows][A + 1].
inline void TrainForwardHost(const TrainNet& v, int rows, const unsigned char* x, unsigned char* saved, int32_t* p) {
  const size_t D = (size_t)v.D;
  std::vector<int32_t> in(kNetMaxInputs), h(D), t(D);
  auto dot = [&](int i, int n, const int32_t* a) {
    int32_t s = v.b[i][n];
    for (int k = 0; k < v.k_in(i); ++k) s += (int32_t)v.w[i][(size_t)n * v.k_in(i) + k] * a[k];
    return NetRs(s, v.shift[i]);
  };
  auto keep = [&](int j, int row, int n, int32_t pre) {
    const int32_t a = NetAct(pre);
    saved[((size_t)j * rows + row) * D + n] = (unsigned char)(a | (a != pre ? 128 : 0));
    return a;
  };
  for (int row = 0; row < rows; ++row) {
    for (int k = 0; k < v.F; ++k) in[k] = x[(size_t)row * v.F + k] & 127;
    for (int n = 0; n < v.D; ++n) h[n] = keep(0, row, n, dot(0, n, in.data()));
    for (int l = 0; l < v.L; ++l) {
      for (int n = 0; n < v.D; ++n) t[n] = keep(1 + 2 * l, row, n, dot(1 + 2 * l, n, h.data()));
      std::vector<int32_t> next(D);
      for (int n = 0; n < v.D; ++n) next[n] = keep(2 + 2 * l, row, n, dot(2 + 2 * l, n, t.data()) + h[n]);
      h = next;
    }
    for (int n = 0; n <= v.A; ++n) p[(size_t)row * (v.A + 1) + n] = dot(2 * v.L + 1, n, h.data());
  }
}

// The backward by the book in double: dp [rows][A + 1], the forward's saved bytes and x -> dw[i] [N][K], db[i] [N].
// `absolute`: |W| for W, |dp| for dp and the same masks -- the G_abs of the error bound.
inline void TrainBackwardHost(const TrainNet& v, int rows, const unsigned char* x, const unsigned char* saved,
                              const double* dp, bool absolute, double* const* dw, double* const* db) {
  const size_t D = (size_t)v.D, R = (size_t)rows;
  auto weight = [&](int i, size_t n, size_t k) {
    const double w = (double)v.w[i][n * v.k_in(i) + k];
    return absolute && w < 0 ? -w : w;
  };
  auto byte = [&](int j, size_t row, size_t n) { return saved[((size_t)j * R + row) * D + n]; };
  // the gradients of layer i from its dz [rows][N] and its input (activation j_in, or x for layer 0)
  auto reduce = [&](int i, const std::vector<double>& dz) {
    const size_t N = v.n_out(i), K = v.k_in(i);
    for (size_t n = 0; n < N; ++n) {
      db[i][n] = 0.0;
      for (size_t k = 0; k < K; ++k) dw[i][n * K + k] = 0.0;
    }
    for (size_t row = 0; row < R; ++row) {
      for (size_t n = 0; n < N; ++n) {
        const double g = dz[row * N + n];
        db[i][n] += g;
        for (size_t k = 0; k < K; ++k) {
          const int in = i == 0 ? (x[row * K + k] & 127) : (byte(i - 1, row, k) & 127);
          dw[i][n * K + k] += g * in;
        }
      }
    }
  };
  // dx = dz W of layer i >= 1, plus `res` where there is one; then the mask of activation i - 1 and the 2^-s of the
  // layer that made it: the dz of layer i - 1
  auto below = [&](int i, const std::vector<double>& dz, const std::vector<double>* res, double res_scale) {
    const size_t N = v.n_out(i);
    const double scale = 1.0 / (double)(1 << v.shift[i - 1]);
    std::vector<double> out(R * D);
    for (size_t row = 0; row < R; ++row) {
      for (size_t k = 0; k < D; ++k) {
        double g = 0.0;
        for (size_t n = 0; n < N; ++n) g += dz[row * N + n] * weight(i, n, k);
        if (res != nullptr) g += (*res)[row * D + k] * res_scale;
        out[row * D + k] = (byte(i - 1, row, k) & 128) != 0 ? 0.0 : g * scale;
      }
    }
    return out;
  };
  const int head = 2 * v.L + 1;
  std::vector<double> dz(R * ((size_t)v.A + 1));
  for (size_t q = 0; q < dz.size(); ++q) dz[q] = absolute && dp[q] < 0 ? -dp[q] : dp[q];
  reduce(head, dz);
  std::vector<double> a = below(head, dz, nullptr, 0.0);  // the dz of layer 2 L
  for (int l = v.L - 1; l >= 0; --l) {
    reduce(2 + 2 * l, a);
    std::vector<double> b = below(2 + 2 * l, a, nullptr, 0.0);  // layer 1 + 2 l
    reduce(1 + 2 * l, b);
    // (a * 2^s is the masked gradient of the block's h_new: the residual branch)
    a = below(1 + 2 * l, b, &a, (double)(1 << v.shift[2 + 2 * l]));
  }
  reduce(0, a);
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_TRAIN_HIP_H_
