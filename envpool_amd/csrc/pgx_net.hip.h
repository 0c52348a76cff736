// PGX built-in network: the contract of the int8 policy-value evaluator of the PGX searches (DESIGN.md "PGX built-in
// network").  Host + device: the kernel (pgx_net.hip), the g++ harness of the tests
// (tests/cpu_harness/pgx_net_host.cpp) and the numpy restatement (tests/pgx_net_util.py) compute the same bits.
//
// The network knows two numbers of the game, F = H W C and A (Pool::GuidedShape).  A row's input x is the F bytes
// 0 / 1 of a leaf's `obs`.  All layers are integer:
//   rs(x, s)  = (x + (s ? 1 << (s - 1) : 0)) >> s          (arithmetic shift: round half up)
//   act(x)    = clamp(x, 0, 127)
//   trunk     h = act(rs(W_in x + b_in, s_in))                                  width D
//   block l   t = act(rs(W1 h + b1, s1));  h = clamp(rs(W2 t + b2, s2) + h, 0, 127)     l = 0 .. L-1
//   head      p = W_head h + b_head                                             A + 1 rows, int32, no shift
// Weights are int8 in -127 .. 127, biases int32 with |b| <= 2^30, shifts 0 .. 24, D a multiple of 32 in 32 .. 512,
// L 0 .. 8, F 1 .. 512, A 1 .. 127.
//
// THE ACCUMULATOR BOUND.  Every inner product has K <= 512 terms (K = F or D; NetParse enforces F <= 512 and
// D <= 512), each |w x| <= 127 * 127 (inputs are 0 / 1 or activations 0 .. 127; NetParse refuses a weight of -128), so
// |sum| <= 512 * 16129 = 8258048 < 2^23; with |b| <= 2^30 and rs's rounding term <= 2^23 every intermediate is below
// 2^30 + 2^24 < 2^31: int32 never wraps, and the order of the sum is free.
//
// Outputs, float32, of a row with status 0 (kGuidedEvaluate):
//   logit[a] = (float) p[a] * scale_p        one int -> float conversion (round to nearest even), one multiply
//   value    = clamp((float) p[A] * scale_v, -1, 1)
//   mode kNetLogits: policy[a] = logit[a] for every a (a session never reads the entries of illegal actions)
//   mode kNetPriors: policy[a] = e[a] / SUM for legal a (mask[a] != 0), 0 elsewhere, with top = the largest legal logit,
//     e[a] = GumbelExp(logit[a] - top), SUM = the e[a] of the legal actions added in ascending a, one division each;
//     nothing is fused (the file is built with -ffp-contract=off).  A row without a legal action: all zeros.
// A row with status != 0 has an all-zero policy row and value 0.
//
// THE BLOB (little endian, 4-byte aligned): a 32-byte header -- uint32 magic "PGXN", int32 version 1, int32 F, A, D, L,
// float32 scale_p, scale_v (finite, 0 < scale <= 1e20) -- and then the 2 L + 2 layers in the order in, (1, 2) of block
// 0, .., head; each layer is its matrix int8 [N][K] row-major, zero bytes up to a multiple of 4, its bias int32 [N] and
// its shift int32 (the head's is 0).  Nothing of the kernel's tiling is in the blob.
#ifndef ENVPOOL_AMD_CSRC_PGX_NET_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_NET_HIP_H_

#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "pgx_gumbel.hip.h"

namespace epa {
namespace pgx {

constexpr uint32_t kNetMagic = 0x4e584750u;  // "PGXN"
constexpr int kNetVersion = 1;
constexpr int kNetHeaderBytes = 32;
constexpr int kNetMinWidth = 32, kNetMaxWidth = 512;  // D
constexpr int kNetMaxBlocks = 8;                      // L
constexpr int kNetMaxShift = 24;
constexpr int kNetMaxInputs = 512;   // F: the K of the first layer
constexpr int kNetMaxActions = 127;  // A: the head's A + 1 rows fill at most four 32-row tiles
constexpr int32_t kNetMaxBias = 1 << 30;
constexpr int kNetMaxLayers = 2 * kNetMaxBlocks + 2;
constexpr int kNetLogits = 0, kNetPriors = 1;  // the modes of an evaluation

PGX_HD inline int32_t NetRs(int32_t x, int s) { return (x + (s != 0 ? (int32_t)1 << (s - 1) : 0)) >> s; }
PGX_HD inline int32_t NetAct(int32_t x) { return x < 0 ? 0 : (x > 127 ? 127 : x); }
PGX_HD inline float NetLogit(int32_t p, float scale_p) { return (float)p * scale_p; }
PGX_HD inline float NetValue(int32_t p, float scale_v) {
  const float v = (float)p * scale_v;
  return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
}
PGX_HD inline int32_t NetFloatBits(float x) {
  int32_t b;
  __builtin_memcpy(&b, &x, 4);
  return b;
}
PGX_HD inline float NetBitsFloat(int32_t b) {
  float x;
  __builtin_memcpy(&x, &b, 4);
  return x;
}

// The outputs of one row IN PLACE: io[0 .. A] holds the head's p on entry and the bits of the float32 policy row
// (io[0 .. A-1]) and of the value (io[A]) on return.  One lane of the kernel, one loop turn of the harness.
PGX_HD inline void NetOutputs(int32_t* io, const unsigned char* mask, int A, float scale_p, float scale_v, int mode,
                              int status) {
  if (status != kGuidedEvaluate) {
    for (int a = 0; a <= A; ++a) io[a] = 0;
    return;
  }
  io[A] = NetFloatBits(NetValue(io[A], scale_v));
  float top = -FLT_MAX;
  bool any = false;
  for (int a = 0; a < A; ++a) {
    const float l = NetLogit(io[a], scale_p);
    io[a] = NetFloatBits(l);
    if (mask[a] != 0) {
      any = true;
      top = l > top ? l : top;
    }
  }
  if (mode == kNetLogits) return;
  float sum = 0.0f;
  for (int a = 0; a < A; ++a) {
    const float e = mask[a] != 0 ? GumbelExp(NetBitsFloat(io[a]) - top) : 0.0f;
    io[a] = NetFloatBits(e);
    if (mask[a] != 0) sum = sum + e;
  }
  for (int a = 0; a < A; ++a) io[a] = NetFloatBits(any && mask[a] != 0 ? NetBitsFloat(io[a]) / sum : 0.0f);
}

// One layer as it lies in a blob: out[n] = SUM_k w[n * k_in + k] * in[k] + b[n], n < n_out.
struct NetLayer {
  const signed char* w;
  const int32_t* b;
  int shift;
  int n_out, k_in;
};

// A parsed blob: pointers into it.  layer[0] the trunk, layer[1 + 2 l], layer[2 + 2 l] block l, layer[2 L + 1] the head.
struct NetView {
  int F, A, D, L;
  float scale_p, scale_v;
  NetLayer layer[kNetMaxLayers];
  int layers() const { return 2 * L + 2; }
};

// Bytes of the blob of a network of these sizes.
inline size_t NetBlobBytes(int F, int A, int D, int L) {
  auto layer = [](size_t n, size_t k) { return ((n * k + 3) & ~(size_t)3) + 4 * n + 4; };
  return (size_t)kNetHeaderBytes + layer(D, F) + (size_t)(2 * L) * layer(D, D) + layer((size_t)A + 1, D);
}

// Checks a blob and points `v` into it: false with the reason in `err`.  What the accumulator bound rests on is
// enforced here, for every user of a blob.
inline bool NetParse(const void* blob, size_t bytes, NetView* v, char* err, size_t err_bytes) {
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  if (blob == nullptr || reinterpret_cast<uintptr_t>(blob) % 4 != 0) {
    std::snprintf(err, err_bytes, "net: the blob must be 4-byte aligned");
    return false;
  }
  if (bytes < (size_t)kNetHeaderBytes) {
    std::snprintf(err, err_bytes, "net: a blob of %zu bytes is shorter than a header", bytes);
    return false;
  }
  uint32_t magic;
  int32_t head[5];
  float scale[2];
  std::memcpy(&magic, p, 4);
  std::memcpy(head, p + 4, 20);
  std::memcpy(scale, p + 24, 8);
  if (magic != kNetMagic) {
    std::snprintf(err, err_bytes, "net: the blob does not begin with the magic PGXN");
    return false;
  }
  if (head[0] != kNetVersion) {
    std::snprintf(err, err_bytes, "net: version = %d must be %d", head[0], kNetVersion);
    return false;
  }
  v->F = head[1], v->A = head[2], v->D = head[3], v->L = head[4];
  v->scale_p = scale[0], v->scale_v = scale[1];
  if (v->F < 1 || v->F > kNetMaxInputs) {
    std::snprintf(err, err_bytes, "net: F = %d must be 1 .. %d", v->F, kNetMaxInputs);
    return false;
  }
  if (v->A < 1 || v->A > kNetMaxActions) {
    std::snprintf(err, err_bytes, "net: A = %d must be 1 .. %d", v->A, kNetMaxActions);
    return false;
  }
  if (v->D < kNetMinWidth || v->D > kNetMaxWidth || v->D % 32 != 0) {
    std::snprintf(err, err_bytes, "net: D = %d must be a multiple of 32 in %d .. %d", v->D, kNetMinWidth, kNetMaxWidth);
    return false;
  }
  if (v->L < 0 || v->L > kNetMaxBlocks) {
    std::snprintf(err, err_bytes, "net: L = %d must be 0 .. %d", v->L, kNetMaxBlocks);
    return false;
  }
  for (int i = 0; i < 2; ++i) {
    if (!(scale[i] > 0.0f && scale[i] <= 1e20f)) {
      std::snprintf(err, err_bytes, "net: %s must be finite, above 0 and at most 1e20", i == 0 ? "scale_p" : "scale_v");
      return false;
    }
  }
  const size_t want = NetBlobBytes(v->F, v->A, v->D, v->L);
  if (bytes != want) {
    std::snprintf(err, err_bytes, "net: a blob of %zu bytes for a network of %zu bytes (F = %d, A = %d, D = %d, L = %d)",
                  bytes, want, v->F, v->A, v->D, v->L);
    return false;
  }
  size_t at = (size_t)kNetHeaderBytes;
  for (int i = 0; i < v->layers(); ++i) {
    NetLayer& l = v->layer[i];
    l.n_out = i == v->layers() - 1 ? v->A + 1 : v->D;
    l.k_in = i == 0 ? v->F : v->D;
    const size_t wn = (size_t)l.n_out * (size_t)l.k_in;
    l.w = reinterpret_cast<const signed char*>(p + at);
    at += (wn + 3) & ~(size_t)3;
    l.b = reinterpret_cast<const int32_t*>(p + at);
    at += 4 * (size_t)l.n_out;
    std::memcpy(&l.shift, p + at, 4);
    at += 4;
    const bool is_head = i == v->layers() - 1;
    if (l.shift < 0 || l.shift > (is_head ? 0 : kNetMaxShift)) {
      std::snprintf(err, err_bytes, "net: layer %d: shift = %d must be 0 .. %d", i, l.shift, is_head ? 0 : kNetMaxShift);
      return false;
    }
    for (size_t q = 0; q < wn; ++q) {
      if (l.w[q] == -128) {
        std::snprintf(err, err_bytes, "net: layer %d: a weight of -128 (weights are -127 .. 127)", i);
        return false;
      }
    }
    for (int n = 0; n < l.n_out; ++n) {
      if (l.b[n] > kNetMaxBias || l.b[n] < -kNetMaxBias) {
        std::snprintf(err, err_bytes, "net: layer %d: a bias of %d is past 2^30 in magnitude", i, l.b[n]);
        return false;
      }
    }
  }
  return true;
}

// One row by the book: x [F] bytes 0 / 1 -> io [A + 1] (NetOutputs).  `h` and `t`: D int32 each.
inline void NetEvalRow(const NetView& v, const unsigned char* x, const unsigned char* mask, int status, int mode,
                       int32_t* h, int32_t* t, int32_t* io) {
  auto dot = [](const NetLayer& l, int n, const int32_t* in) {
    int32_t s = l.b[n];
    for (int k = 0; k < l.k_in; ++k) s += (int32_t)l.w[(size_t)n * l.k_in + k] * in[k];
    return s;
  };
  int32_t xin[kNetMaxInputs];
  for (int k = 0; k < v.F; ++k) xin[k] = x[k];
  for (int n = 0; n < v.D; ++n) h[n] = NetAct(NetRs(dot(v.layer[0], n, xin), v.layer[0].shift));
  for (int l = 0; l < v.L; ++l) {
    const NetLayer& l1 = v.layer[1 + 2 * l];
    const NetLayer& l2 = v.layer[2 + 2 * l];
    for (int n = 0; n < v.D; ++n) t[n] = NetAct(NetRs(dot(l1, n, h), l1.shift));
    // (h[n] is read only by turn n: in place)
    int32_t next[kNetMaxWidth];
    for (int n = 0; n < v.D; ++n) next[n] = NetAct(NetRs(dot(l2, n, t), l2.shift) + h[n]);
    for (int n = 0; n < v.D; ++n) h[n] = next[n];
  }
  for (int n = 0; n <= v.A; ++n) io[n] = dot(v.layer[v.layers() - 1], n, h);
  NetOutputs(io, mask, v.A, v.scale_p, v.scale_v, mode, status);
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_NET_HIP_H_
