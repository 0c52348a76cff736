// TEST HARNESS (not product): envpool_amd/csrc/pgx_conv.hip.h built for the host by tests/test_pgx_conv_host.py:
// the blob check (ConvParse) and rows by the book (ConvEvalRow).  Not linked by envpool_amd/.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../envpool_amd/csrc/pgx_conv.hip.h"

using namespace epa::pgx;

extern "C" {

int pgx_conv_parse(const void* blob, size_t bytes, char* err, int err_bytes) {
  ConvView v{};
  return ConvParse(blob, bytes, &v, err, (size_t)err_bytes) ? 0 : -1;
}

int pgx_conv_dense_parse(const void* blob, size_t bytes, char* err, int err_bytes) {
  NetView v{};
  return NetParse(blob, bytes, &v, err, (size_t)err_bytes) ? 0 : -1;
}

size_t pgx_conv_blob_bytes(int H, int W, int C, int A, int D, int L, int P) {
  return ConvBlobBytes(H, W, C, A, D, L, P);
}

int pgx_conv_eval(const void* blob, size_t bytes, int rows, int mode, const uint8_t* obs, const uint8_t* mask,
                  const uint8_t* status, float* policy, float* value) {
  ConvView v{};
  char err[240];
  if (!ConvParse(blob, bytes, &v, err, sizeof(err))) return -1;
  const size_t S = (size_t)v.H * v.W, F = S * v.C, wide = S * (size_t)std::max(v.D, v.C);
  std::vector<int32_t> h(wide), t(wide), z(wide), io((size_t)v.A + 1);
  for (int r = 0; r < rows; ++r) {
    ConvEvalRow(v, obs + (size_t)r * F, mask + (size_t)r * v.A, status[r], mode, h.data(), t.data(), z.data(),
                io.data());
    std::memcpy(policy + (size_t)r * v.A, io.data(), 4 * (size_t)v.A);
    std::memcpy(value + r, io.data() + v.A, 4);
  }
  return 0;
}

}  // extern "C"
