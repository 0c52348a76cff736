// envpool_amd/csrc/actor_memory.hip.h built for the host: the cell by the book (MemoryCellRow), the weights as the
// kernel reads them (CellImage) and MemoryParse.  Built by tests/test_actor_memory_host.py with g++.
#include <cstring>

#include "../../envpool_amd/csrc/actor_memory.hip.h"

using namespace epa::actor;

extern "C" {

// rows by the book: out = h', state = h' or zeros where reset[row] != 0 (reset may be null)
void mh_cell(int F, int M, const int8_t* wz, const int32_t* bz, int sz, const int8_t* wn, const int32_t* bn, int sn,
             int rows, const unsigned char* x, const unsigned char* h, const unsigned char* reset, unsigned char* out,
             unsigned char* state) {
  const CellLayer lz{wz, bz, sz}, ln{wn, bn, sn};
  for (int r = 0; r < rows; ++r) {
    MemoryCellRow(F, M, lz, ln, x + (size_t)r * F, h + (size_t)r * M, out + (size_t)r * M);
    for (int m = 0; m < M; ++m) state[(size_t)r * M + m] = reset != nullptr && reset[r] != 0 ? 0 : out[(size_t)r * M + m];
  }
}

// CellImage's bytes into `out` (null: nothing); returns CellImageBytes
size_t mh_image(int F, int M, const int8_t* wz, const int8_t* wn, int8_t* out) {
  if (out != nullptr) CellImage(F, M, CellLayer{wz, nullptr, 0}, CellLayer{wn, nullptr, 0}, out);
  return CellImageBytes(F, M);
}

// 1 and shape = F, M, sz, sn, the inner actor's F, H, kind -- or 0 and the reason
int mh_parse(const void* blob, size_t bytes, int* shape, char* err, int err_bytes) {
  MemoryView v;
  if (!MemoryParse(blob, bytes, &v, err, (size_t)err_bytes)) return 0;
  const int s[7] = {v.F, v.M, v.z.shift, v.n.shift, v.inner.F, v.inner.H, v.inner.kind};
  std::memcpy(shape, s, sizeof(s));
  return 1;
}

}  // extern "C"
