// Rollout actor with memory: the contract of the recurrent cell in front of the built-in actor-critic (DESIGN.md
// section 2 "Rollout actor, memory cell").  Host + device, in the style of actor.hip.h: the kernel (actor_memory.hip),
// the g++ harness of the tests (tests/cpu_harness/actor_memory_host.cpp) and the numpy restatement of
// tests/test_actor_memory_host.py compute the same bits.
//
// A memory actor is an ordinary actor (actor.hip.h) behind a cell.  The cell turns the feature row x (F bytes 0 .. 127,
// ActorFeature's) and the env's state h (M bytes 0 .. 127) into a new state h'; the inner actor's trunk reads h' as its
// features, so the inner actor's F is M.  The cell is a Light GRU (Ravanelli et al. 2018: no reset gate, a rectified
// candidate), stated in integers with NetRs and NetAct of pgx_net.hip.h:
//   v      = [x ; h]                                                   K = F + M bytes
//   z[m]   = clamp(64 + rs(Wz[m,:] . v + bz[m], sz), 0, 128)            the gate: 128 keeps h[m], 0 takes n[m]
//   n[m]   = act(rs(Wn[m,:] . v + bn[m], sn))                           the candidate, 0 .. 127
//   h'[m]  = (z[m] * h[m] + (128 - z[m]) * n[m] + 64) >> 7              0 .. 127
// M is a multiple of 32 in 32 .. 512, F is 1 .. 512, weights are int8 in -127 .. 127 (MemoryParse refuses -128),
// |b| <= 2^30, shifts 0 .. 24.
//
// THE ACCUMULATOR BOUND.  An inner product has K <= 1024 terms, each |w v| <= 127 * 127, so |sum| <= 1024 * 16129 =
// 16 516 096 < 2^24; with |b| <= 2^30 and rs's rounding term <= 2^23 every intermediate is below 2^30 + 2^24 + 2^23 <
// 2^31: int32 never wraps, and the order of the sum is free (the kernel sums [h ; x], k-step by k-step).  |rs(.)| is no
// larger than its argument, so the gate's 64 + rs(.) stays below 2^31 as well before it is clamped.  The blend: z and
// 128 - z are weights that add up to 128, so 0 <= z h + (128 - z) n <= 128 * 127 and h' <= (128 * 127 + 64) >> 7 = 127:
// h' is an activation in 0 .. 127, and the trunk's own proof (pgx_net.hip.h) covers its first layer unchanged.
//
// THE STATE RULE.  The state of env n is zero after reset(), after attach, and after the step of slot t if that step was
// the env's auto-reset row (mask[t][n] == 0, rollout.hip.h).  So the final observation of an episode, which lies in the
// slot of the auto-reset row, is evaluated with the episode's state (its value bootstraps a truncated episode), and the
// first observation of the next episode sees h = 0.  The evaluation of slot t commits h' -- zeros for a row whose
// `reset` byte is set: the collector passes its carry flags, which are what mask[t] is computed from --; value_only at
// the last slot evaluates the cell and commits nothing.
//
// THE BLOB (little endian, 4-byte aligned), a wrapper around an unchanged EPAA blob: a 24-byte header -- uint32 magic
// "EPAM", int32 version 1, int32 F, M, two reserved zero words -- then lo[F], scale[F] float64 (the OUTER features'),
// then the layer Wz -- int8 [M][K] row-major, zero bytes up to a multiple of 4, bz int32 [M], sz int32 --, the layer Wn
// the same with bn, sn, then a complete EPAA blob whose F equals M, whose lo and scale are 0 and 1 and whose kind is 0
// or 1: a masked head's mask0 indexes raw observation components, which do not survive the wrapper.
#ifndef ENVPOOL_AMD_CSRC_ACTOR_MEMORY_HIP_H_
#define ENVPOOL_AMD_CSRC_ACTOR_MEMORY_HIP_H_

#include <cstdint>
#include <cstring>
#include <vector>

#include "actor.hip.h"

namespace epa {
namespace actor {

constexpr uint32_t kMemoryMagic = 0x4d415045u;  // "EPAM"
constexpr int kMemoryVersion = 1;
constexpr int kMemoryHeaderBytes = 24;
constexpr int kMemoryMinWidth = 32, kMemoryMaxWidth = 512;  // M

// ---- the cell ----------------------------------------------------------------------------------------------------------
PGX_HD inline int32_t CellGate(int32_t acc, int shift) {
  const int32_t g = 64 + pgx::NetRs(acc, shift);
  return g < 0 ? 0 : (g > 128 ? 128 : g);
}
PGX_HD inline int32_t CellCandidate(int32_t acc, int shift) { return pgx::NetAct(pgx::NetRs(acc, shift)); }
PGX_HD inline int32_t CellBlend(int32_t z, int32_t n, int32_t h) { return (z * h + (128 - z) * n + 64) >> 7; }

struct CellLayer {
  const int8_t* w;   // [M][K] row-major
  const int32_t* b;  // [M]
  int shift;
};
// One row by the book: x [F], h [M] -> out [M] (out must not be h).
inline void MemoryCellRow(int F, int M, const CellLayer& lz, const CellLayer& ln, const unsigned char* x,
                          const unsigned char* h, unsigned char* out) {
  const int K = F + M;
  for (int m = 0; m < M; ++m) {
    int32_t az = lz.b[m], an = ln.b[m];
    const int8_t* wz = lz.w + (size_t)m * K;
    const int8_t* wn = ln.w + (size_t)m * K;
    for (int k = 0; k < K; ++k) {
      const int32_t v = k < F ? x[k] : h[k - F];
      az += (int32_t)wz[k] * v;
      an += (int32_t)wn[k] * v;
    }
    out[m] = (unsigned char)CellBlend(CellGate(az, lz.shift), CellCandidate(an, ln.shift), h[m]);
  }
}

// ---- the kernel's geometry (actor_memory.hip) -------------------------------------------------------------------------
// A row of the staged tile is [h (M) ; x (F) ; up to a multiple of 32 ; kCellPad]: h first, so that it lies on 16-byte
// words.  The matrix instruction takes 32 k at a time (a k-step): lane (r, hh) of a wave holds the 16 bytes
// 32 kt + 16 hh .. + 15 of tile row r as its B operand and of weight row 32 ct + r as its A operand.
constexpr int kCellBlock = 256;       // four waves
constexpr int kCellMaxRows = 64;      // rows per block ...
constexpr int kCellLdsBytes = 65536;  // ... or 32, where 64 staged rows and their h' would not fit in this
constexpr int kCellPad = 16;          // bytes between two staged rows: successive rows start 4 banks apart
PGX_HD inline int CellKSteps(int F, int M) { return (F + M + 31) / 32; }
PGX_HD inline int CellStride(int F, int M) { return 32 * CellKSteps(F, M) + kCellPad; }
PGX_HD inline int CellRows(int F, int M) {
  return kCellMaxRows * (CellStride(F, M) + M) <= kCellLdsBytes ? kCellMaxRows : kCellMaxRows / 2;
}
PGX_HD inline size_t CellLdsBytes(int F, int M) { return (size_t)CellRows(F, M) * (size_t)(CellStride(F, M) + M); }
// The weights as the kernel reads them: [column tile ct][k-step kt][gate: z, n][lane] of 16 bytes, so that a wave reads
// the 2 KiB of one (ct, kt) in a run.  Column kk of the tile is h[kk] below M, x[kk - M] below M + F, nothing above
// (zero weights: what the tile holds there does not count).
inline size_t CellImageBytes(int F, int M) { return (size_t)(M / 32) * (size_t)CellKSteps(F, M) * 2048; }
inline void CellImage(int F, int M, const CellLayer& lz, const CellLayer& ln, int8_t* out) {
  const int K = F + M, steps = CellKSteps(F, M);
  for (int ct = 0; ct < M / 32; ++ct) {
    for (int kt = 0; kt < steps; ++kt) {
      for (int g = 0; g < 2; ++g) {
        const int8_t* w = g == 0 ? lz.w : ln.w;
        for (int lane = 0; lane < 64; ++lane) {
          const int r = lane & 31, hh = lane >> 5;
          int8_t* dst = out + ((((size_t)ct * steps + kt) * 2 + g) * 64 + lane) * 16;
          for (int b = 0; b < 16; ++b) {
            const int kk = 32 * kt + 16 * hh + b;
            const int8_t* row = w + (size_t)(32 * ct + r) * K;
            dst[b] = kk < M ? row[F + kk] : (kk < K ? row[kk - M] : (int8_t)0);
          }
        }
      }
    }
  }
}
// the neuron (within its 32-column tile) of accumulator register `reg` of a lane of half hh (pgx_net.hip: TileNeuron)
PGX_HD inline int CellNeuron(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }

// ---- the blob ----------------------------------------------------------------------------------------------------------
struct MemoryView {
  int F, M;
  std::vector<double> lo, scale;  // the outer features'
  CellLayer z, n;                 // into the blob
  ActorView inner;
};
inline size_t MemoryLayerBytes(int F, int M) { return (((size_t)M * (size_t)(F + M) + 3) & ~(size_t)3) + 4 * (size_t)M + 4; }
inline size_t MemoryFrontBytes(int F, int M) { return (size_t)kMemoryHeaderBytes + 16 * (size_t)F + 2 * MemoryLayerBytes(F, M); }
inline bool IsMemoryBlob(const void* blob, size_t bytes) {
  uint32_t magic = 0;
  if (blob != nullptr && bytes >= 4) std::memcpy(&magic, blob, 4);
  return magic == kMemoryMagic;
}
inline bool MemoryParse(const void* blob, size_t bytes, MemoryView* v, char* err, size_t err_bytes) {
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  if (blob == nullptr || reinterpret_cast<uintptr_t>(blob) % 4 != 0) {
    std::snprintf(err, err_bytes, "actor memory: the blob must be 4-byte aligned");
    return false;
  }
  if (bytes < (size_t)kMemoryHeaderBytes) {
    std::snprintf(err, err_bytes, "actor memory: a blob of %zu bytes is shorter than a header", bytes);
    return false;
  }
  uint32_t magic;
  int32_t head[5];
  std::memcpy(&magic, p, 4);
  std::memcpy(head, p + 4, 20);
  if (magic != kMemoryMagic) {
    std::snprintf(err, err_bytes, "actor memory: the blob does not begin with the magic EPAM");
    return false;
  }
  if (head[0] != kMemoryVersion) {
    std::snprintf(err, err_bytes, "actor memory: version = %d must be %d", head[0], kMemoryVersion);
    return false;
  }
  v->F = head[1], v->M = head[2];
  if (v->F < 1 || v->F > pgx::kNetMaxInputs) {
    std::snprintf(err, err_bytes, "actor memory: F = %d must be 1 .. %d", v->F, pgx::kNetMaxInputs);
    return false;
  }
  if (v->M < kMemoryMinWidth || v->M > kMemoryMaxWidth || v->M % 32 != 0) {
    std::snprintf(err, err_bytes, "actor memory: M = %d must be a multiple of 32 in %d .. %d", v->M, kMemoryMinWidth,
                  kMemoryMaxWidth);
    return false;
  }
  if (head[3] != 0 || head[4] != 0) {
    std::snprintf(err, err_bytes, "actor memory: the reserved words must be 0");
    return false;
  }
  const size_t front = MemoryFrontBytes(v->F, v->M);
  if (bytes <= front) {
    std::snprintf(err, err_bytes, "actor memory: a blob of %zu bytes ends inside the cell (%zu bytes)", bytes, front);
    return false;
  }
  const size_t F = (size_t)v->F, M = (size_t)v->M, K = F + M;
  v->lo.resize(F);
  v->scale.resize(F);
  std::memcpy(v->lo.data(), p + kMemoryHeaderBytes, 8 * F);
  std::memcpy(v->scale.data(), p + kMemoryHeaderBytes + 8 * F, 8 * F);
  for (size_t i = 0; i < F; ++i) {
    if (!(std::fabs(v->lo[i]) <= DBL_MAX) || !(std::fabs(v->scale[i]) <= DBL_MAX)) {
      std::snprintf(err, err_bytes, "actor memory: lo and scale must be finite (component %zu)", i);
      return false;
    }
  }
  const unsigned char* at = p + kMemoryHeaderBytes + 16 * F;
  CellLayer* layers[2] = {&v->z, &v->n};
  for (int g = 0; g < 2; ++g) {
    CellLayer& l = *layers[g];
    l.w = reinterpret_cast<const int8_t*>(at);
    l.b = reinterpret_cast<const int32_t*>(at + ((M * K + 3) & ~(size_t)3));
    std::memcpy(&l.shift, reinterpret_cast<const unsigned char*>(l.b) + 4 * M, 4);
    at += MemoryLayerBytes(v->F, v->M);
    const char* name = g == 0 ? "Wz" : "Wn";
    for (size_t i = 0; i < M * K; ++i) {
      if (l.w[i] == -128) {
        std::snprintf(err, err_bytes, "actor memory: layer %s: a weight of -128 (row %zu)", name, i / K);
        return false;
      }
    }
    for (size_t m = 0; m < M; ++m) {
      if (l.b[m] > pgx::kNetMaxBias || l.b[m] < -pgx::kNetMaxBias) {
        std::snprintf(err, err_bytes, "actor memory: layer %s: |bias| above 2^30 (row %zu)", name, m);
        return false;
      }
    }
    if (l.shift < 0 || l.shift > pgx::kNetMaxShift) {
      std::snprintf(err, err_bytes, "actor memory: layer %s: shift = %d must be 0 .. %d", name, l.shift, pgx::kNetMaxShift);
      return false;
    }
  }
  if (!ActorParse(p + front, bytes - front, &v->inner, err, err_bytes)) return false;  // (also: a long or short rest)
  if (v->inner.kind == kMasked) {
    std::snprintf(err, err_bytes, "actor memory: a masked inner actor (kind 2) is not supported: its mask indexes raw "
                                  "observation components");
    return false;
  }
  if (v->inner.F != v->M) {
    std::snprintf(err, err_bytes, "actor memory: the inner actor's F = %d must be M = %d", v->inner.F, v->M);
    return false;
  }
  for (int i = 0; i < v->M; ++i) {
    if (v->inner.lo[(size_t)i] != 0.0 || v->inner.scale[(size_t)i] != 1.0) {
      std::snprintf(err, err_bytes, "actor memory: the inner actor's lo and scale must be 0 and 1 (component %d)", i);
      return false;
    }
  }
  return true;
}

// bytes the two state arrays add to a collector (rollout.hip.h: RolloutBytes)
PGX_HD inline long long MemoryRolloutBytes(long long n, long long m) { return 2 * n * m; }

}  // namespace actor
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_ACTOR_MEMORY_HIP_H_
