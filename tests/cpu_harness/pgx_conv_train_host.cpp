// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_conv_train.hip.h, the contract of the training
// kernels of the PGX convolutional network, built with g++ by tests/test_pgx_conv_train_host.py: the forward by the book
// with its saved bytes, the backward by the book in double, and the size check.  Not linked by envpool_amd/.
#include <cstdint>
#include <cstring>

#include "../../envpool_amd/csrc/pgx_conv_train.hip.h"

using namespace epa::pgx;

extern "C" {

// 0, or -1 with the reason in err
int pgx_conv_train_check(int H, int W, int C, int A, int D, int L, int P, long long rows, char* err, int err_bytes) {
  return ConvTrainCheck(H, W, C, A, D, L, P, rows, err, (size_t)err_bytes) ? 0 : -1;
}

// x [rows][H W][C] -> saved [2 L + 1][rows][H W][D], g [rows][H W P], p [rows][A + 1]; then, with dp, dw[i] in the
// blob's order and db[i] [N] in double
int pgx_conv_train_run(int H, int W, int C, int A, int D, int L, int P, int rows, const int8_t* const* w,
                       const int32_t* const* b, const int32_t* shifts, const uint8_t* x, const double* dp, int absolute,
                       uint8_t* saved, uint8_t* g, int32_t* p, double* const* dw, double* const* db) {
  char err[240];
  if (!ConvTrainCheck(H, W, C, A, D, L, P, rows, err, sizeof(err)) || !ConvTrainCheckShifts(L, shifts, err, sizeof(err))) {
    return -1;
  }
  ConvTrainNet v{};
  v.H = H, v.W = W, v.C = C, v.A = A, v.D = D, v.L = L, v.P = P;
  for (int i = 0; i < v.layers(); ++i) {
    v.w[i] = reinterpret_cast<const signed char*>(w[i]), v.b[i] = b[i], v.shift[i] = shifts[i];
  }
  ConvTrainForwardHost(v, rows, x, saved, g, p);
  ConvTrainBackwardHost(v, rows, x, saved, g, dp, absolute != 0, dw, db);
  return 0;
}

// the slices of a 3x3 layer's reduction, and the most a workspace is sized for
void pgx_conv_train_slices(int rows, int H, int W, int N, int K, int* out) {
  const ConvTrainSlicing s = ConvTrainSlices(rows, H, W, N, K);
  out[0] = s.slices, out[1] = s.slice_boards, out[2] = ConvTrainMostSlices(rows, H, W, N, K);
}

}  // extern "C"
