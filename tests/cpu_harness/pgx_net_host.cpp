// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_net.hip.h, the contract of the PGX built-in
// network, built with g++ by tests/test_pgx_net_host.py: the blob check every user of a network goes through (NetParse)
// and the evaluation of rows by the book (NetEvalRow, NetOutputs).  Not linked by envpool_amd/.
//
// With -DPGX_NET_MAIN the file is a program of its own: a small random network on a few rows, for a run under the host
// sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../envpool_amd/csrc/pgx_net.hip.h"

using namespace epa::pgx;

extern "C" {

// 0 for a blob that is a network; -1 with the reason in err
int pgx_net_parse(const void* blob, size_t bytes, char* err, int err_bytes) {
  NetView v{};
  return NetParse(blob, bytes, &v, err, (size_t)err_bytes) ? 0 : -1;
}

// bytes of a blob of these sizes
size_t pgx_net_blob_bytes(int F, int A, int D, int L) { return NetBlobBytes(F, A, D, L); }

// rows [rows][F], mask [rows][A], status [rows] -> policy [rows][A], value [rows]; -1 for a blob that is no network
int pgx_net_eval(const void* blob, size_t bytes, int rows, int mode, const uint8_t* obs, const uint8_t* mask,
                 const uint8_t* status, float* policy, float* value) {
  NetView v{};
  char err[200];
  if (!NetParse(blob, bytes, &v, err, sizeof(err))) return -1;
  std::vector<int32_t> h(v.D), t(v.D), io((size_t)v.A + 1);
  for (int r = 0; r < rows; ++r) {
    NetEvalRow(v, obs + (size_t)r * v.F, mask + (size_t)r * v.A, status[r], mode, h.data(), t.data(), io.data());
    std::memcpy(policy + (size_t)r * v.A, io.data(), 4 * (size_t)v.A);
    std::memcpy(value + r, io.data() + v.A, 4);
  }
  return 0;
}

}  // extern "C"

#ifdef PGX_NET_MAIN
// F = 18, A = 9, D = 32, L = 1 with weights and inputs from an integer hash, five rows, both modes.
int main() {
  const int F = 18, A = 9, D = 32, L = 1, rows = 5;
  std::vector<int32_t> words((NetBlobBytes(F, A, D, L) + 3) / 4, 0);
  unsigned char* p = reinterpret_cast<unsigned char*>(words.data());
  const int32_t head[6] = {(int32_t)kNetMagic, kNetVersion, F, A, D, L};
  const float scale[2] = {1.0f / 256.0f, 1.0f / 4096.0f};
  std::memcpy(p, head, 24);
  std::memcpy(p + 24, scale, 8);
  size_t at = kNetHeaderBytes;
  uint32_t x = 2166136261u;
  for (int i = 0; i < 2 * L + 2; ++i) {
    const size_t n = i == 2 * L + 1 ? A + 1 : D, k = i == 0 ? F : D;
    for (size_t q = 0; q < n * k; ++q) {
      x = (x ^ (uint32_t)q) * 16777619u;
      p[at + q] = (unsigned char)(int8_t)((int)(x >> 24) % 128);
    }
    at += (n * k + 3) & ~(size_t)3;
    at += 4 * n;  // (zero biases)
    const int32_t shift = i == 2 * L + 1 ? 0 : 6;
    std::memcpy(p + at, &shift, 4);
    at += 4;
  }
  std::vector<uint8_t> obs((size_t)rows * F), mask((size_t)rows * A, 1), status(rows, 0);
  for (size_t q = 0; q < obs.size(); ++q) obs[q] = (uint8_t)((q * 2654435761u >> 13) & 1u);
  status[3] = 2;
  std::vector<float> policy((size_t)rows * A), value(rows);
  for (int mode = 0; mode < 2; ++mode) {
    if (pgx_net_eval(p, at, rows, mode, obs.data(), mask.data(), status.data(), policy.data(), value.data()) != 0) {
      return 1;
    }
    std::printf("mode %d: policy[0][0] %g value[0] %g value[3] %g\n", mode, policy[0], value[0], value[3]);
  }
  return 0;
}
#endif
