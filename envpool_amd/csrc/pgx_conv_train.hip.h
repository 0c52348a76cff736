// PGX convolutional network, training: the contract of the forward and backward kernels behind
// `ConvNet.module(kernels=True)` (DESIGN.md "PGX convolutional network: training").  Host + device: the kernels
// (pgx_conv_train.hip) and the g++ harness of the tests (tests/cpu_harness/pgx_conv_train_host.cpp) restate the torch
// twin of envpool_amd/pgx/net.py (`_make_conv_module`), which is the authority.  The split float, its helpers and the
// dense reduction are pgx_train.hip.h's.
//
// FORWARD.  p = the head's int32 sums of pgx_conv.hip.h (stem, L blocks, 1x1 reduce, dense head over (y, x, plane)),
// from input bytes 0 .. 127 as [rows][H W][C], int8 weights in -127 .. 127 in the blob's order ([N][3][3][K], [P][D],
// [A + 1][H W P]) and int32 biases: the master parameters quantised as the twin does, clamp(round(w), -127, 127) and
// round(b), half to even.  Beside p the forward keeps one byte per activation, the SAVED BYTES: activation j of a
// position-row, j = 0 the stem's h, j = 1 + 2 l the t and j = 2 + 2 l the h of block l, lies at
// saved[((j * rows + row) * H W + square) * D + n], and the reduce layer's g at g[(row * H W + square) * P + q]; bits
// 0 .. 6 are the activation and bit 7 is set where the clamp changed the value.
//   THE BYTE ORDER IN A RECORD IS THE NATURAL ONE, channel n at byte n.  The eval kernel's (half, dword, byte) tile
//   order would make a lane's store one 128-bit write instead of four 32-bit ones, but every reader of the bytes wants
//   the natural order: the reductions read a record as a row of a dense [positions][D] matrix, g as [rows][H W P] is
//   the head's input row as it stands, and the backward's mask lookup is saved[position * D + channel] with the
//   channel on the lane, a coalesced byte read.  The forward writes each byte once; the backward reads it three times.
//
// BACKWARD, the twin's straight-through rules as pgx_train.hip.h states them.  Given dp float32 [rows][A + 1]: a layer
// with shift s has dz = dout * 2^-s; a 3x3 layer contributes
//   db[n] = SUM_{row, square} dz,
//   dW[n][dy][dx][c] = SUM_{row, y, x} dz[row][y][x][n] * in[row][y + dy - 1][x + dx - 1][c]   (off board: 0),
//   dx[row][y][x][c] = SUM_{n, dy, dx} dz[row][y - dy + 1][x - dx + 1][n] * W[n][dy][dx][c]    (off board: 0);
// the reduce layer and the head are dense layers of rows * H W and of rows rows.  A clamp passes the gradient where the
// value before it lies in 0 .. 127 INCLUSIVE (bit 7 clear); the gradient of a block's h_new, after its mask, goes to
// layer 2's output and to h alike; the stem's dx is not computed.
//
// LIMITS: ConvParse's for the net (H W <= 128, C 1 .. 32, D a multiple of 32 in 32 .. 256, L 0 .. 8, P 1 .. 32 with
// H W P <= 512, A 1 .. 127, shifts 0 .. 24 and 0 for the head) and rows >= 1 with rows * H W <= 2^22 (ConvTrainCheck).
// The kernels keep whole boards in LDS and refuse, at creation, a net one board of which does not fit the device's
// block.
//
// THE ERROR CONSTANT c_conv (kConvTrainErr).  The device arithmetic is the dense backward's: every dz a split float
// (|v - (hi + lo)| <= 2^-16 |v|), every product exact in the float32 accumulator of v_mfma_f32_32x32x16_bf16, u = 2^-23
// per addition, an MFMA of 16 products counted as 16 additions in a row.
//   dx of a 3x3 layer (ConvTrainDx): 9 taps * D <= 2304 terms, twice for hi and lo, in ONE accumulator per output
//     tile: d = 4608; one addition of the residual branch and the split of the result:
//     4609 * 2^-23 + 2^-16 = 5.65e-4 of the sum of the magnitudes.
//   dx of the reduce layer and of the head (ConvTrainRow): at most 128 terms twice, d = 256: 4.6e-5.
//   dW, db of a 3x3 layer (ConvTrainDw): the positions of a pass (at most kConvTrainPassMax = 272 haloed positions,
//     hi and lo: d = 544) in a first accumulator, the passes of a slice folded one after another into a second one (a
//     slice has at most kConvTrainSlicePositions = 8192 positions and a pass at least 22: d < 373), the slices added
//     in their order (at most kConvTrainMaxSlices = 640): d <= 1557, 1.86e-4.
//   dW, db of the reduce layer and the head (TrainReduce, TrainSum): the dense 1.15e-4.
// All are below c_conv = 2^-10 = 9.77e-4.  As in the dense contract a gradient m layers below the output (m <= 19) is
// within ((1 + c)^m - 1) G_abs of the exact one, and (1 + c)^m - 1 <= m c (1 + (m - 1) c / 2 + ..) <= 1.01 m c since
// 18 * 2^-11 = 0.0088; the stage constants leave that 1 % several times over, so the tests assert m c_conv G_abs.
//
// DETERMINISM.  No atomics.  The slices of every reduction are a function of the sizes only (TrainSlices,
// ConvTrainSlices); a slice's partial sums are formed in one fixed order by one block and added in ascending slice
// order by one thread.
#ifndef ENVPOOL_AMD_CSRC_PGX_CONV_TRAIN_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_CONV_TRAIN_HIP_H_

#include <vector>

#include "pgx_conv.hip.h"
#include "pgx_train.hip.h"

namespace epa {
namespace pgx {

constexpr long long kConvTrainMaxPositions = 1ll << 22;  // rows * H W
constexpr double kConvTrainErr = 1.0 / 1024.0;           // c_conv
constexpr int kConvTrainPassTarget = 176;                // haloed positions of a pass of ConvTrainDw, if a board fits
constexpr int kConvTrainPassMax = 272;                   // (H + 1)(W + 1) <= 258, up to a multiple of 16
constexpr int kConvTrainSlicePositions = 8192;
constexpr int kConvTrainMaxSlices = 640;

// false with the reason in `err`: everything the contract bounds but the shifts
inline bool ConvTrainCheck(int H, int W, int C, int A, int D, int L, int P, long long rows, char* err,
                           size_t err_bytes) {
  if (H < 1 || W < 1 || H > kConvMaxSquares || W > kConvMaxSquares || H * W > kConvMaxSquares) {
    std::snprintf(err, err_bytes, "conv_train: H = %d, W = %d must be at least 1 with H W <= %d", H, W,
                  kConvMaxSquares);
  } else if (C < 1 || C > kConvMaxChannels) {
    std::snprintf(err, err_bytes, "conv_train: C = %d must be 1 .. %d", C, kConvMaxChannels);
  } else if (A < 1 || A > kNetMaxActions) {
    std::snprintf(err, err_bytes, "conv_train: A = %d must be 1 .. %d", A, kNetMaxActions);
  } else if (D < kConvMinWidth || D > kConvMaxWidth || D % 32 != 0) {
    std::snprintf(err, err_bytes, "conv_train: D = %d must be a multiple of 32 in %d .. %d", D, kConvMinWidth,
                  kConvMaxWidth);
  } else if (L < 0 || L > kConvMaxBlocks) {
    std::snprintf(err, err_bytes, "conv_train: L = %d must be 0 .. %d", L, kConvMaxBlocks);
  } else if (P < 1 || P > kConvMaxPlanes || H * W * P > kConvMaxFlat) {
    std::snprintf(err, err_bytes, "conv_train: P = %d must be 1 .. %d with H W P <= %d", P, kConvMaxPlanes,
                  kConvMaxFlat);
  } else if (rows < 1 || rows * H * W > kConvTrainMaxPositions) {
    std::snprintf(err, err_bytes, "conv_train: rows = %lld must be 1 .. %lld (rows H W <= 2^22)", rows,
                  kConvTrainMaxPositions / (H * W));
  } else {
    return true;
  }
  return false;
}

inline bool ConvTrainCheckShifts(int L, const int32_t* shifts, char* err, size_t err_bytes) {
  for (int i = 0; i < 2 * L + 3; ++i) {
    const int top = i == 2 * L + 2 ? 0 : kNetMaxShift;
    if (shifts[i] < 0 || shifts[i] > top) {
      std::snprintf(err, err_bytes, "conv_train: layer %d: shift = %d must be 0 .. %d", i, shifts[i], top);
      return false;
    }
  }
  return true;
}

// A pass of ConvTrainDw holds `boards` boards in LDS as one run of haloed positions: square (y, x) of board b at
// b * stride + (y + 1)(W + 1) + (x + 1), stride = (H + 1)(W + 1).  Every other position of the run is halo and stays
// zero: the column left of a row is the column right of the row above, the row under a board the row over the next.
struct ConvTrainPass {
  int boards, stride, run;  // run: boards * stride up to a multiple of 16, the contraction length of a pass
};
PGX_HD inline ConvTrainPass ConvTrainPassOf(int H, int W) {
  ConvTrainPass p;
  p.stride = (H + 1) * (W + 1);
  p.boards = kConvTrainPassTarget / p.stride > 1 ? kConvTrainPassTarget / p.stride : 1;
  p.run = (p.boards * p.stride + 15) / 16 * 16;
  return p;
}

// The slices of the reduction of a 3x3 layer [N][9 K] over `rows` boards, in whole passes: enough blocks to fill the
// device at few rows, no slice past kConvTrainSlicePositions positions.  The sizes decide, nothing else.
struct ConvTrainSlicing {
  int slices, slice_boards;
};
PGX_HD inline ConvTrainSlicing ConvTrainSlices(int rows, int H, int W, int N, int K) {
  const ConvTrainPass pass = ConvTrainPassOf(H, W);
  const int tiles = ((N + kTrainTile - 1) / kTrainTile) * ((K + kTrainTile - 1) / kTrainTile);
  const int passes = (rows + pass.boards - 1) / pass.boards;
  int want = (512 + tiles - 1) / tiles;
  want = want < kTrainMaxSlices ? want : kTrainMaxSlices;
  want = want < passes ? want : passes;
  int per = (passes + want - 1) / want;
  const int cap = kConvTrainSlicePositions / (pass.boards * H * W);  // (a pass has at most 176 squares: >= 46)
  per = per < cap ? per : cap;
  ConvTrainSlicing s;
  s.slice_boards = per * pass.boards;
  s.slices = (rows + s.slice_boards - 1) / s.slice_boards;
  return s;
}
// No call of at most `max_rows` boards has more slices than this: what a workspace is sized by.
inline int ConvTrainMostSlices(int max_rows, int H, int W, int N, int K) {
  const ConvTrainPass pass = ConvTrainPassOf(H, W);
  const int tiles = ((N + kTrainTile - 1) / kTrainTile) * ((K + kTrainTile - 1) / kTrainTile);
  const int most = (512 + tiles - 1) / tiles, want = most < kTrainMaxSlices ? most : kTrainMaxSlices;
  const int cap = kConvTrainSlicePositions / (pass.boards * H * W);
  const int least = (max_rows + cap * pass.boards - 1) / (cap * pass.boards);
  return want > least ? want : least;
}

// A network as the training calls take it: per layer the quantised weights in the blob's order, the biases, the shift.
struct ConvTrainNet {
  int H, W, C, A, D, L, P;
  const signed char* w[kConvMaxLayers];
  const int32_t* b[kConvMaxLayers];
  int32_t shift[kConvMaxLayers];
  int layers() const { return 2 * L + 3; }
  int S() const { return H * W; }
  int taps(int i) const { return i < 2 * L + 1 ? 9 : 1; }
  int n_out(int i) const { return i == 2 * L + 2 ? A + 1 : (i == 2 * L + 1 ? P : D); }
  int k_in(int i) const { return i == 0 ? C : (i == 2 * L + 2 ? H * W * P : D); }
};

// The forward by the book: x [rows][H W][C] -> saved [2 L + 1][rows][H W][D], g [rows][H W P], p [rows][A + 1].
inline void ConvTrainForwardHost(const ConvTrainNet& v, int rows, const unsigned char* x, unsigned char* saved,
                                 unsigned char* g, int32_t* p) {
  const int S = v.S(), D = v.D;
  ConvView view{};
  view.H = v.H, view.W = v.W;
  auto layer = [&](int i) {
    ConvLayer l;
    l.w = v.w[i], l.b = v.b[i], l.shift = v.shift[i], l.n_out = v.n_out(i), l.taps = v.taps(i), l.k_in = v.k_in(i);
    return l;
  };
  const size_t cells = (size_t)S * (D > v.C ? D : v.C);
  std::vector<int32_t> h(cells), t(cells), z(cells);
  auto keep = [&](unsigned char* at, int32_t pre) {
    const int32_t a = NetAct(pre);
    *at = (unsigned char)(a | (a != pre ? 128 : 0));
    return a;
  };
  for (int row = 0; row < rows; ++row) {
    auto act = [&](int j) { return saved + ((size_t)j * rows + row) * S * D; };
    for (int k = 0; k < S * v.C; ++k) t[k] = x[(size_t)row * S * v.C + k] & 127;
    ConvLayerSums(view, layer(0), t.data(), z.data());
    for (int k = 0; k < S * D; ++k) h[k] = keep(act(0) + k, NetRs(z[k], v.shift[0]));
    for (int l = 0; l < v.L; ++l) {
      ConvLayerSums(view, layer(1 + 2 * l), h.data(), z.data());
      for (int k = 0; k < S * D; ++k) t[k] = keep(act(1 + 2 * l) + k, NetRs(z[k], v.shift[1 + 2 * l]));
      ConvLayerSums(view, layer(2 + 2 * l), t.data(), z.data());
      for (int k = 0; k < S * D; ++k) h[k] = keep(act(2 + 2 * l) + k, NetRs(z[k], v.shift[2 + 2 * l]) + h[k]);
    }
    const int r = 2 * v.L + 1;
    for (int s = 0; s < S; ++s) {
      for (int q = 0; q < v.P; ++q) {
        int32_t sum = v.b[r][q];
        for (int c = 0; c < D; ++c) sum += (int32_t)v.w[r][(size_t)q * D + c] * h[(size_t)s * D + c];
        t[s * v.P + q] = keep(g + ((size_t)row * S + s) * v.P + q, NetRs(sum, v.shift[r]));
      }
    }
    for (int n = 0; n <= v.A; ++n) {
      int32_t sum = v.b[r + 1][n];
      for (int k = 0; k < S * v.P; ++k) sum += (int32_t)v.w[r + 1][(size_t)n * S * v.P + k] * t[k];
      p[(size_t)row * (v.A + 1) + n] = sum;
    }
  }
}

// The backward by the book in double: dp [rows][A + 1], the forward's saved bytes, g and x -> dw[i] in the blob's
// order, db[i] [N].  `absolute`: |W| for W, |dp| for dp and the same masks -- the G_abs of the error bound.
inline void ConvTrainBackwardHost(const ConvTrainNet& v, int rows, const unsigned char* x, const unsigned char* saved,
                                  const unsigned char* g, const double* dp, bool absolute, double* const* dw,
                                  double* const* db) {
  const int H = v.H, W = v.W;
  const size_t S = (size_t)v.S(), D = (size_t)v.D, R = (size_t)rows;
  auto weight = [&](int i, size_t at) {
    const double w = (double)v.w[i][at];
    return absolute && w < 0 ? -w : w;
  };
  auto act = [&](int j) { return saved + (size_t)j * R * S * D; };
  // a dense layer over `n_rows` rows: dz [n_rows][N], in [n_rows][K] bytes -> dw, db
  auto reduce_dense = [&](int i, size_t n_rows, const std::vector<double>& dz, const unsigned char* in) {
    const size_t N = v.n_out(i), K = v.k_in(i);
    for (size_t n = 0; n < N; ++n) db[i][n] = 0.0;
    for (size_t q = 0; q < N * K; ++q) dw[i][q] = 0.0;
    for (size_t row = 0; row < n_rows; ++row) {
      for (size_t n = 0; n < N; ++n) {
        const double gz = dz[row * N + n];
        db[i][n] += gz;
        for (size_t k = 0; k < K; ++k) dw[i][n * K + k] += gz * (in[row * K + k] & 127);
      }
    }
  };
  // dz W of a dense layer, then the mask `flags` and `scale`: the dz of the layer below, [n_rows][K]
  auto below_dense = [&](int i, size_t n_rows, const std::vector<double>& dz, const unsigned char* flags,
                         double scale) {
    const size_t N = v.n_out(i), K = v.k_in(i);
    std::vector<double> out(n_rows * K);
    for (size_t row = 0; row < n_rows; ++row) {
      for (size_t k = 0; k < K; ++k) {
        double s = 0.0;
        for (size_t n = 0; n < N; ++n) s += dz[row * N + n] * weight(i, n * K + k);
        out[row * K + k] = (flags[row * K + k] & 128) != 0 ? 0.0 : s * scale;
      }
    }
    return out;
  };
  // a 3x3 layer: dz [rows][S][D], in [rows][S][K] bytes -> dw [D][3][3][K], db
  auto reduce_conv = [&](int i, const std::vector<double>& dz, const unsigned char* in) {
    const size_t K = v.k_in(i);
    for (size_t n = 0; n < D; ++n) db[i][n] = 0.0;
    for (size_t q = 0; q < D * 9 * K; ++q) dw[i][q] = 0.0;
    for (size_t row = 0; row < R; ++row) {
      for (int y = 0; y < H; ++y) {
        for (int xx = 0; xx < W; ++xx) {
          const double* gz = &dz[((row * S) + (size_t)y * W + xx) * D];
          for (size_t n = 0; n < D; ++n) db[i][n] += gz[n];
          for (int dy = 0; dy < 3; ++dy) {
            for (int dx = 0; dx < 3; ++dx) {
              const int yy = y + dy - 1, xs = xx + dx - 1;
              if (yy < 0 || yy >= H || xs < 0 || xs >= W) continue;
              const unsigned char* src = in + ((row * S) + (size_t)yy * W + xs) * K;
              for (size_t n = 0; n < D; ++n) {
                double* to = dw[i] + ((n * 3 + dy) * 3 + dx) * K;
                for (size_t c = 0; c < K; ++c) to[c] += gz[n] * (src[c] & 127);
              }
            }
          }
        }
      }
    }
  };
  // dx of 3x3 layer i >= 1, plus `res` where there is one; then the mask of activation i - 1 and the 2^-s of the
  // layer that made it
  auto below_conv = [&](int i, const std::vector<double>& dz, const std::vector<double>* res, double res_scale) {
    const double scale = 1.0 / (double)(1 << v.shift[i - 1]);
    const unsigned char* flags = act(i - 1);
    std::vector<double> out(R * S * D);
    for (size_t row = 0; row < R; ++row) {
      for (int y = 0; y < H; ++y) {
        for (int xx = 0; xx < W; ++xx) {
          const size_t at = (row * S + (size_t)y * W + xx) * D;
          for (size_t c = 0; c < D; ++c) {
            double s = 0.0;
            for (int dy = 0; dy < 3; ++dy) {
              for (int dx = 0; dx < 3; ++dx) {
                const int yy = y - dy + 1, xs = xx - dx + 1;
                if (yy < 0 || yy >= H || xs < 0 || xs >= W) continue;
                const double* gz = &dz[(row * S + (size_t)yy * W + xs) * D];
                for (size_t n = 0; n < D; ++n) s += gz[n] * weight(i, ((n * 3 + dy) * 3 + dx) * D + c);
              }
            }
            if (res != nullptr) s += (*res)[at + c] * res_scale;
            out[at + c] = (flags[at + c] & 128) != 0 ? 0.0 : s * scale;
          }
        }
      }
    }
    return out;
  };
  const int head = 2 * v.L + 2, red = head - 1;
  std::vector<double> dz(R * ((size_t)v.A + 1));
  for (size_t q = 0; q < dz.size(); ++q) dz[q] = absolute && dp[q] < 0 ? -dp[q] : dp[q];
  reduce_dense(head, R, dz, g);
  // (g [rows][S P] read as [rows S][P]: the dz of the reduce layer)
  std::vector<double> dr = below_dense(head, R, dz, g, 1.0 / (double)(1 << v.shift[red]));
  reduce_dense(red, R * S, dr, act(2 * v.L));
  std::vector<double> a = below_dense(red, R * S, dr, act(2 * v.L), 1.0 / (double)(1 << v.shift[2 * v.L]));
  for (int l = v.L - 1; l >= 0; --l) {
    reduce_conv(2 + 2 * l, a, act(1 + 2 * l));
    std::vector<double> b = below_conv(2 + 2 * l, a, nullptr, 0.0);
    reduce_conv(1 + 2 * l, b, act(2 * l));
    a = below_conv(1 + 2 * l, b, &a, (double)(1 << v.shift[2 + 2 * l]));
  }
  reduce_conv(0, a, x);
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_CONV_TRAIN_HIP_H_
