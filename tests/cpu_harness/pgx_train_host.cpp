// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_train.hip.h, the contract of the training
// kernels of the PGX built-in network, built with g++ by tests/test_pgx_train_host.py: the forward by the book with its
// saved bytes, the backward by the book in double, the size check and the split of a float.  Not linked by envpool_amd/.
#include <cstdint>
#include <cstring>

#include "../../envpool_amd/csrc/pgx_train.hip.h"

using namespace epa::pgx;

extern "C" {

// 0, or -1 with the reason in err
int pgx_train_check(int F, int A, int D, int L, long long rows, char* err, int err_bytes) {
  return TrainCheck(F, A, D, L, rows, err, (size_t)err_bytes) ? 0 : -1;
}

// x [rows][F] -> saved [2 L + 1][rows][D], p [rows][A + 1]; then, with dp, dw[i] [N][K] and db[i] [N] in double
int pgx_train_run(int F, int A, int D, int L, int rows, const int8_t* const* w, const int32_t* const* b,
                  const int32_t* shifts, const uint8_t* x, const double* dp, int absolute, uint8_t* saved, int32_t* p,
                  double* const* dw, double* const* db) {
  char err[200];
  if (!TrainCheck(F, A, D, L, rows, err, sizeof(err)) || !TrainCheckShifts(L, shifts, err, sizeof(err))) return -1;
  TrainNet v{};
  v.F = F, v.A = A, v.D = D, v.L = L;
  for (int i = 0; i < v.layers(); ++i) {
    v.w[i] = reinterpret_cast<const signed char*>(w[i]), v.b[i] = b[i], v.shift[i] = shifts[i];
  }
  TrainForwardHost(v, rows, x, saved, p);
  TrainBackwardHost(v, rows, x, saved, dp, absolute != 0, dw, db);
  return 0;
}

// hi + lo of the split of v, and the slices of a reduction
float pgx_train_split_join(float v) { return TrainJoin(TrainSplit(v)); }
void pgx_train_slices(int rows, int N, int K, int* out) {
  const TrainSlicing s = TrainSlices(rows, N, K);
  out[0] = s.slices, out[1] = s.slice_rows, out[2] = TrainMostSlices(rows, N, K);
}

}  // extern "C"
