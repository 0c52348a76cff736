// Host build of envpool_amd/csrc/snapshot.hip.h for tests/test_snapshot_host.py: the index functions of the generator
// and stack kernels replayed thread by thread over a host image of the pool, the size arithmetic of a blob, and the
// header checks.  Every replay also verifies that no index leaves its section and that every blob element of the
// section is written exactly once.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../envpool_amd/csrc/snapshot.hip.h"

using namespace epa::snap;

namespace {
// one pass of the generator kernel's mapping; `tiled`: MtTileKernel, otherwise MtWordKernel with the two shifts.
// Returns 0, or a negative code: -1 pool index out of range, -2 blob index out of range, -3 a blob word touched
// twice, -4 a blob word never touched.  With the two position arrays (both or neither) the positions move as the
// kernels' thread of word 0 / quarter 0 of tile 0 moves them, and an unpack between different layouts ends like
// Pool::SnapUnpack: MtConvertKernel's one thread per row over the pool image.
int MtPass(bool tiled, bool unpack, uint32_t* pool, int n, int pool_sh, const int* ids, int k, uint32_t* blob,
           int blob_sh, int* pool_mti, int* blob_mti) {
  const size_t pool_words = (size_t)kMtWords * n, blob_words = (size_t)kMtWords * k;
  std::vector<unsigned char> hit(blob_words, 0);
  auto move = [&](size_t p, size_t b, int words) -> int {
    for (int w = 0; w < words; ++w) {
      if (p + w >= pool_words) return -1;
      if (b + w >= blob_words) return -2;
      if (hit[b + w]++) return -3;
      if (unpack) {
        pool[p + w] = blob[b + w];
      } else {
        blob[b + w] = pool[p + w];
      }
    }
    return 0;
  };
  if (tiled) {
    for (size_t t = 0; t < MtTileThreads(k); ++t) {
      int tile, row, q;
      MtTileThread(t, k, &tile, &row, &q);
      if (row < 0 || row >= k || tile < 0 || tile >= kMtTiles) return -2;
      if (int rc = move(MtQuarterIndex(tile, ids[row], n, q), MtQuarterIndex(tile, row, k, q), 4)) return rc;
    }
  } else {
    for (size_t t = 0; t < MtWordThreads(k); ++t) {
      int j, row;
      MtWordThread(t, k, &j, &row);
      if (row < 0 || row >= k || j < 0 || j >= kMtWords) return -2;
      if (int rc = move(MtWordIndex(j, ids[row], n, pool_sh), MtWordIndex(j, row, k, blob_sh), 1)) return rc;
    }
  }
  for (unsigned char h : hit) {
    if (h != 1) return -4;
  }
  if (pool_mti != nullptr && blob_mti != nullptr) {
    for (int row = 0; row < k; ++row) {
      if (unpack) {
        pool_mti[ids[row]] = blob_mti[row];
      } else {
        blob_mti[row] = pool_mti[ids[row]];
      }
    }
    if (unpack && !tiled && pool_sh != blob_sh) {
      for (int row = 0; row < k; ++row) MtConvertTile(pool, ids[row], n, pool_sh, blob_sh, pool_mti[ids[row]]);
    }
  }
  return 0;
}
}  // namespace

extern "C" {

// pack the listed columns of `pool` into `blob`, or unpack them; see MtPass for the result.  pool_mti [n] and
// blob_mti [k] may both be null: the words alone move then.
int snap_mt_pass(int tiled, int unpack, uint32_t* pool, int n, int pool_sh, const int* ids, int k, uint32_t* blob,
                 int blob_sh, int* pool_mti, int* blob_mti) {
  return MtPass(tiled != 0, unpack != 0, pool, n, pool_sh, ids, k, blob, blob_sh, pool_mti, blob_mti);
}

// where word j of env e lives in a pool image (the layout the step kernels use)
uint64_t snap_mt_word_index(int j, int e, int n, int sh) { return MtWordIndex(j, e, n, sh); }

// the stack kernel's mapping over rings of `len` doubles per env; same result codes
int snap_stack_pass(int unpack, double* ring, int n, const int* ids, int k, int len, double* blob) {
  const size_t ring_len = (size_t)n * len, blob_len = (size_t)k * len;
  std::vector<unsigned char> hit(blob_len, 0);
  for (size_t t = 0; t < StackThreads(k, len); ++t) {
    int row, pair;
    StackThread(t, len, &row, &pair);
    if (row < 0 || row >= k || pair < 0 || pair >= StackPairs(len)) return -2;
    const size_t p = StackIndex(ids[row], len, pair), b = StackIndex(row, len, pair);
    const int words = 2 * pair + 1 < len ? 2 : 1;
    for (int w = 0; w < words; ++w) {
      if (p + w >= ring_len) return -1;
      if (b + w >= blob_len) return -2;
      if (hit[b + w]++) return -3;
      if (unpack) {
        ring[p + w] = blob[b + w];
      } else {
        blob[b + w] = ring[p + w];
      }
    }
  }
  for (unsigned char h : hit) {
    if (h != 1) return -4;
  }
  return 0;
}

uint64_t snap_fnv1a(const char* s) { return Fnv1a(s); }

// desc: family_hash, num_envs, state_dim, has_rng, mt_shift, stack_s, stack_nobs, extra_bytes
static PoolDesc Desc(const uint64_t* d) {
  PoolDesc p{};
  p.family_hash = d[0];
  p.num_envs = (int32_t)d[1];
  p.state_dim = (int32_t)d[2];
  p.has_rng = (int32_t)d[3];
  p.mt_shift = (int32_t)d[4];
  p.stack_s = (int32_t)d[5];
  p.stack_nobs = (int32_t)d[6];
  p.extra_bytes = d[7];
  return p;
}

// the 64 header bytes of a snapshot of k envs of such a pool; returns the blob's byte count
uint64_t snap_make_header(const uint64_t* desc, int k, unsigned flags, void* header_out) {
  const Header h = MakeHeader(Desc(desc), k, flags);
  std::memcpy(header_out, &h, sizeof(h));
  return h.total_bytes;
}

// section offsets of a blob with this header: state, mt, mti, stack, heads, extra, total
void snap_layout(const void* header, uint64_t* out) {
  Header h;
  std::memcpy(&h, header, sizeof(h));
  const Layout l = LayoutOf(h);
  const size_t v[7] = {l.state, l.mt, l.mti, l.stack, l.heads, l.extra, l.total};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
}

// nullptr (accepted) or the reason the pool refuses the header for k target envs
const char* snap_check_header(const uint64_t* desc, const void* header, int k) {
  Header h;
  std::memcpy(&h, header, sizeof(h));
  return CheckHeader(Desc(desc), h, k);
}

}  // extern "C"
