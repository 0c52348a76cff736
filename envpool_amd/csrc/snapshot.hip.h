// Snapshots: the blob format, its header checks, the index arithmetic of the generator / stack sections and the
// gfx950 kernels that move them (Pool::SnapshotDevice / RestoreDevice / Fork, engine.hip).
//
// A snapshot of k envs is a byte blob: a 64-byte header, then sections, each starting on a 64-byte boundary:
//   state    [k][state_dim] doubles          what the family's GetState writes (cur_step and done are in it)
//   mt       624 k words                     only with EPA_SNAP_RNG and a pool that has generators; laid out like the
//                                            generator of a POOL OF k ENVS with the source pool's mt_shift:
//                                            shift 0 [624][k], shift 4 [39][k][16]
//   mti      [k] ints                        behind the words (same condition)
//   stack    [k][S][nobs] doubles            only when the pool has the generic observation ring (frame_stack > 1)
//   heads    [k] ints                        behind the ring rows
//   extra    [k][extra_bytes]                the family's PackExtra hook (0 bytes for every family today)
//
// Everything up to the kernels is plain C++ without a HIP dependency: tests/cpu_harness/snapshot_host.cpp builds it
// with g++ and checks the index functions, the size arithmetic and every header rejection rule.
//
// Thread mapping of the generator move (the hot path: 2.5 KB per env):
//   shift 4 on both sides  one thread = one 16-byte quarter of a 64-byte tile (uint4).  Thread t: quarter t & 3,
//                          row (t >> 2) % k, tile (t >> 2) / k.  Four consecutive lanes cover one env's tile (one
//                          64-byte sector on the pool side, whatever the id), sixteen rows per wave; on the blob side
//                          a wave's 1 KB is contiguous for ANY ids, and on the pool side too when ids are consecutive.
//   shift 0 on both sides  one thread = one word.  Thread t: row t % k, word t / k: lanes run along the rows, so a
//                          wave reads / writes 64 consecutive 4-byte columns of one word row in the blob, and of the
//                          pool's row too when the ids are consecutive.
//   mixed (a blob restored into a pool built with another "mt_tile")  the word mapping with each side's own index,
//                          then one thread per env converts the ONE partly consumed tile on the pool side
//                          (MtConvertTile below): the two layouts regenerate lazily at different grains -- [624][N]
//                          twists word i when it is consumed, the tiled layout twists a whole tile when its first
//                          word is reached -- so with mti % 16 != 0 the words mti .. mti | 15 are still the old
//                          block's in a shift-0 generator and already the new block's in a shift-4 one.  Every other
//                          word, and every word when mti % 16 == 0, means the same in both and is copied verbatim.
// The thread of word 0 / quarter 0 of tile 0 of a row also moves that row's mti.
// The stack ring moves as double2 (thread = one pair of a row) when S * nobs is even, so that every env's row starts on
// a 16-byte boundary on both sides; for an odd S * nobs the same thread moves its two doubles one by one.  The thread
// of pair 0 moves the row's head.  No LDS, no atomics, one launch per section; every kernel guards its tail.
#ifndef ENVPOOL_AMD_CSRC_SNAPSHOT_HIP_H_
#define ENVPOOL_AMD_CSRC_SNAPSHOT_HIP_H_

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EPA_SNAP_HD __host__ __device__
#else
#define EPA_SNAP_HD
#endif

namespace epa {
namespace snap {

constexpr uint32_t kMagic = 0x4e535045u;  // "EPSN"
constexpr uint32_t kVersion = 1;
constexpr unsigned kFlagRng = 1u;  // EPA_SNAP_RNG
constexpr int kMtWords = 624;
constexpr int kMtTiles = 39;  // of 16 words
constexpr size_t kHeaderBytes = 64;
constexpr size_t kSectionAlign = 64;

struct Header {
  uint32_t magic;
  uint32_t version;
  uint64_t family_hash;  // Fnv1a of the family name
  int32_t state_dim;
  int32_t k;
  uint32_t flags;     // kFlagRng: the generator section is present
  int32_t mt_shift;   // layout of the generator section (0 without one)
  int32_t stack_s;    // 1: no stack section
  int32_t stack_nobs;
  uint64_t extra_bytes;  // per env
  uint64_t total_bytes;
  uint64_t reserved;
};
static_assert(sizeof(Header) == kHeaderBytes, "the header is 64 bytes");

// what a header has to fit
struct PoolDesc {
  uint64_t family_hash;
  int32_t num_envs;
  int32_t state_dim;
  int32_t has_rng;
  int32_t mt_shift;
  int32_t stack_s;
  int32_t stack_nobs;
  uint64_t extra_bytes;  // per env
};

inline uint64_t Fnv1a(const char* s) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (; *s; ++s) {
    h ^= (unsigned char)*s;
    h *= 0x100000001b3ull;
  }
  return h;
}

// byte offsets of the sections of a blob; a section that is absent has the offset of the next one
struct Layout {
  size_t state, mt, mti, stack, heads, extra, total;
};

inline size_t AlignUp(size_t x) { return (x + kSectionAlign - 1) / kSectionAlign * kSectionAlign; }

inline Layout LayoutOf(int state_dim, int k, bool rng, int stack_s, int stack_nobs, size_t extra_bytes) {
  Layout l{};
  size_t off = kHeaderBytes;
  l.state = off;
  off = AlignUp(off + sizeof(double) * (size_t)k * (size_t)state_dim);
  l.mt = off;
  if (rng) off += sizeof(uint32_t) * (size_t)kMtWords * (size_t)k;
  l.mti = off;
  if (rng) off = AlignUp(off + sizeof(int32_t) * (size_t)k);
  l.stack = off;
  if (stack_s > 1) off += sizeof(double) * (size_t)k * (size_t)stack_s * (size_t)stack_nobs;
  l.heads = off;
  if (stack_s > 1) off = AlignUp(off + sizeof(int32_t) * (size_t)k);
  l.extra = off;
  off = AlignUp(off + extra_bytes * (size_t)k);
  l.total = off;
  return l;
}

inline Layout LayoutOf(const Header& h) {
  return LayoutOf(h.state_dim, h.k, (h.flags & kFlagRng) != 0, h.stack_s, h.stack_nobs, (size_t)h.extra_bytes);
}

// the header of a snapshot of k envs of such a pool (flags as the caller gave them)
inline Header MakeHeader(const PoolDesc& p, int k, unsigned flags) {
  Header h{};
  h.magic = kMagic;
  h.version = kVersion;
  h.family_hash = p.family_hash;
  h.state_dim = p.state_dim;
  h.k = k;
  const bool rng = (flags & kFlagRng) != 0 && p.has_rng != 0;
  h.flags = rng ? kFlagRng : 0u;
  h.mt_shift = rng ? p.mt_shift : 0;
  h.stack_s = p.stack_s;
  h.stack_nobs = p.stack_s > 1 ? p.stack_nobs : 0;
  h.extra_bytes = p.extra_bytes;
  h.total_bytes = LayoutOf(h).total;
  return h;
}

// nullptr when a blob with this header may be restored into k envs of the pool, the reason otherwise
inline const char* CheckHeader(const PoolDesc& p, const Header& h, int k) {
  if (h.magic != kMagic) return "snapshot: not a snapshot blob (bad magic)";
  if (h.version != kVersion) return "snapshot: unknown blob version";
  if (h.family_hash != p.family_hash) return "snapshot: blob of another env family";
  if (h.state_dim != p.state_dim) return "snapshot: state_dim of the blob does not fit this pool";
  if (h.stack_s != p.stack_s || h.stack_nobs != (p.stack_s > 1 ? p.stack_nobs : 0)) {
    return "snapshot: frame_stack of the blob does not fit this pool";
  }
  if ((h.flags & ~kFlagRng) != 0) return "snapshot: unknown flags in the blob";
  if ((h.flags & kFlagRng) != 0) {
    if (!p.has_rng) return "snapshot: blob carries generators, this pool has none";
    if (h.mt_shift != 0 && h.mt_shift != 4) return "snapshot: unknown generator layout in the blob";
  } else if (h.mt_shift != 0) {
    return "snapshot: generator layout without a generator section";
  }
  if (h.extra_bytes != p.extra_bytes) return "snapshot: family section of the blob does not fit this pool";
  if (h.k <= 0 || h.k > p.num_envs) return "snapshot: env count of the blob does not fit this pool";
  if (h.k != k) return "snapshot: blob holds another number of envs than ids were given";
  if (h.total_bytes != LayoutOf(h).total) return "snapshot: byte count of the blob does not fit its header";
  return nullptr;
}

// ---- index arithmetic (host and device) ------------------------------------------------------
// word j of column `col` of a generator of `cols` envs (Mt19937::At, device_common.hip.h)
EPA_SNAP_HD inline size_t MtWordIndex(int j, int col, int cols, int sh) {
  return ((((size_t)(j >> sh)) * (size_t)cols + (size_t)col) << sh) | (size_t)(j & ((1 << sh) - 1));
}
// first word of quarter q of tile `tile` of column `col` (shift 4)
EPA_SNAP_HD inline size_t MtQuarterIndex(int tile, int col, int cols, int q) {
  return (((size_t)tile * (size_t)cols + (size_t)col) << 4) + 4u * (size_t)q;
}
EPA_SNAP_HD inline size_t MtTileThreads(int k) { return (size_t)kMtTiles * (size_t)k * 4u; }
EPA_SNAP_HD inline void MtTileThread(size_t t, int k, int* tile, int* row, int* q) {
  *q = (int)(t & 3u);
  const size_t r = t >> 2;
  *row = (int)(r % (size_t)k);
  *tile = (int)(r / (size_t)k);
}
EPA_SNAP_HD inline size_t MtWordThreads(int k) { return (size_t)kMtWords * (size_t)k; }
EPA_SNAP_HD inline void MtWordThread(size_t t, int k, int* j, int* row) {
  *row = (int)(t % (size_t)k);
  *j = (int)(t / (size_t)k);
}
// the stack ring: thread = pair `pair` of row `row`; a row is `len` = S * nobs doubles
EPA_SNAP_HD inline int StackPairs(int len) { return (len + 1) / 2; }
EPA_SNAP_HD inline size_t StackThreads(int k, int len) { return (size_t)k * (size_t)StackPairs(len); }
EPA_SNAP_HD inline void StackThread(size_t t, int len, int* row, int* pair) {
  const size_t pairs = (size_t)StackPairs(len);
  *row = (int)(t / pairs);
  *pair = (int)(t % pairs);
}
EPA_SNAP_HD inline size_t StackIndex(int row, int len, int pair) { return (size_t)row * (size_t)len + 2u * (size_t)pair; }

// ---- the partly consumed tile of a generator that changes layout (host and device) ------------
// Mt19937::Twist1 (device_common.hip.h): word j of the next block out of words j, j + 1 and the partner j + 397
EPA_SNAP_HD inline uint32_t MtTwist1(uint32_t cur, uint32_t nxt, uint32_t partner) {
  const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
  return partner ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
EPA_SNAP_HD inline int MtPartner(int j) { return j >= 227 ? j - 227 : j + 397; }
// Column `col` of a generator of `cols` envs in layout `to_sh` holds the words of a generator of layout `from_sh`
// at position p = mti (a verbatim copy): make them the words a generator of layout `to_sh` holds at that position.
// Nothing to do when the layouts agree or p starts a tile.  Words p .. p | 15 change, nothing else is written; the
// partner words (227 away) and word 0 behind word 623 lie outside that range and mean the same in both layouts.
//   0 -> 4  the tile is expected regenerated: twist its remaining words in ascending order, exactly as Next() of the
//           [624][N] layout would when it consumes them (word j + 1 still old, word 0 behind 623 already new)
//   4 -> 0  the tile is expected old from p on: z = new[j] ^ partner = (y >> 1) ^ (y & 1 ? 0x9908b0df : 0) with
//           y = (old[j] & 0x80000000) | (old[j + 1] & 0x7fffffff); y >> 1 has a clear top bit and the constant a set
//           one, so the top bit of z is y & 1 and y is recovered whole.  old[j] is the top bit of y_j and the low
//           31 bits of y_{j - 1}; p - 1 is in the same tile (p % 16 != 0) and new in both layouts.
EPA_SNAP_HD inline void MtConvertTile(uint32_t* mt, int col, int cols, int to_sh, int from_sh, int p) {
  if (to_sh == from_sh || (p & 15) == 0 || p < 0 || p >= kMtWords) return;
  const int last = p | 15;
  if (from_sh == 0) {
    for (int j = p; j <= last; ++j) {
      uint32_t& w = mt[MtWordIndex(j, col, cols, to_sh)];
      w = MtTwist1(w, mt[MtWordIndex(j == kMtWords - 1 ? 0 : j + 1, col, cols, to_sh)],
                   mt[MtWordIndex(MtPartner(j), col, cols, to_sh)]);
    }
  } else {
    uint32_t prev = 0;  // y of word j - 1
    for (int j = p - 1; j <= last; ++j) {
      uint32_t& w = mt[MtWordIndex(j, col, cols, to_sh)];
      uint32_t z = w ^ mt[MtWordIndex(MtPartner(j), col, cols, to_sh)];
      const uint32_t bit = z >> 31;
      if (bit) z ^= 0x9908b0dfu;
      const uint32_t y = (z << 1) | bit;
      if (j >= p) w = (y & 0x80000000u) | (prev & 0x7fffffffu);
      prev = y;
    }
  }
}

#if defined(__HIPCC__)
// ---- kernels ----------------------------------------------------------------------------------
struct HeaderWords {
  uint32_t w[kHeaderBytes / 4];
};
__global__ __launch_bounds__(64) void WriteHeaderKernel(HeaderWords h, uint32_t* __restrict__ dst) {
  if (threadIdx.x < kHeaderBytes / 4) dst[threadIdx.x] = h.w[threadIdx.x];
}

// generator words, both sides tiled.  UNPACK: blob -> pool.
template <bool UNPACK>
__global__ __launch_bounds__(256) void MtTileKernel(uint32_t* __restrict__ pool_mt, int* __restrict__ pool_mti, int n,
                                                    const int* __restrict__ ids, int k,
                                                    uint32_t* __restrict__ blob_mt, int* __restrict__ blob_mti) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= MtTileThreads(k)) return;
  int tile, row, q;
  MtTileThread(t, k, &tile, &row, &q);
  const int e = ids[row];
  uint4* p = reinterpret_cast<uint4*>(pool_mt + MtQuarterIndex(tile, e, n, q));
  uint4* b = reinterpret_cast<uint4*>(blob_mt + MtQuarterIndex(tile, row, k, q));
  if (UNPACK) {
    *p = *b;
  } else {
    *b = *p;
  }
  if (tile == 0 && q == 0) {
    if (UNPACK) {
      pool_mti[e] = blob_mti[row];
    } else {
      blob_mti[row] = pool_mti[e];
    }
  }
}

// generator words one by one: both sides [624][cols] (lanes along the rows), or sides of different layouts
template <bool UNPACK>
__global__ __launch_bounds__(256) void MtWordKernel(uint32_t* __restrict__ pool_mt, int* __restrict__ pool_mti, int n,
                                                    int pool_sh, const int* __restrict__ ids, int k,
                                                    uint32_t* __restrict__ blob_mt, int* __restrict__ blob_mti,
                                                    int blob_sh) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= MtWordThreads(k)) return;
  int j, row;
  MtWordThread(t, k, &j, &row);
  const int e = ids[row];
  uint32_t* p = pool_mt + MtWordIndex(j, e, n, pool_sh);
  uint32_t* b = blob_mt + MtWordIndex(j, row, k, blob_sh);
  if (UNPACK) {
    *p = *b;
  } else {
    *b = *p;
  }
  if (j == 0) {
    if (UNPACK) {
      pool_mti[e] = blob_mti[row];
    } else {
      blob_mti[row] = pool_mti[e];
    }
  }
}

// behind MtWordKernel<true> with sides of different layouts: one thread per restored env converts its partly consumed
// tile in the pool (restore ids are unique: no two threads share a column)
__global__ __launch_bounds__(256) void MtConvertKernel(uint32_t* __restrict__ pool_mt, const int* __restrict__ pool_mti,
                                                       int n, int pool_sh, const int* __restrict__ ids, int k,
                                                       int blob_sh) {
  const int row = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (row >= k) return;
  const int e = ids[row];
  MtConvertTile(pool_mt, e, n, pool_sh, blob_sh, pool_mti[e]);
}

// the observation ring [N][len] <-> [k][len] and its heads.  WIDE: len is even, every row 16-byte aligned.
template <bool UNPACK, bool WIDE>
__global__ __launch_bounds__(256) void StackKernel(double* __restrict__ ring, int* __restrict__ head,
                                                   const int* __restrict__ ids, int k, int len,
                                                   double* __restrict__ blob_ring, int* __restrict__ blob_head) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= StackThreads(k, len)) return;
  int row, pair;
  StackThread(t, len, &row, &pair);
  const int e = ids[row];
  double* p = ring + StackIndex(e, len, pair);
  double* b = blob_ring + StackIndex(row, len, pair);
  if (WIDE) {
    if (UNPACK) {
      *reinterpret_cast<double2*>(p) = *reinterpret_cast<const double2*>(b);
    } else {
      *reinterpret_cast<double2*>(b) = *reinterpret_cast<const double2*>(p);
    }
  } else {
    const bool two = 2 * pair + 1 < len;
    if (UNPACK) {
      p[0] = b[0];
      if (two) p[1] = b[1];
    } else {
      b[0] = p[0];
      if (two) b[1] = p[1];
    }
  }
  if (pair == 0) {
    if (UNPACK) {
      head[e] = blob_head[row];
    } else {
      blob_head[row] = head[e];
    }
  }
}
#endif  // __HIPCC__

}  // namespace snap
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_SNAPSHOT_HIP_H_
