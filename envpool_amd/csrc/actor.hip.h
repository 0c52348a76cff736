// Rollout actor: the contract of the built-in actor-critic of the rollout collector (DESIGN.md section 2 "Rollout actor
// and collect").  Host + device: the kernels (actor.hip), the g++ harness of the tests
// (tests/cpu_harness/actor_host.cpp) and the numpy restatement (tests/actor_util.py) compute the same bits.  The build
// keeps -ffp-contract=off and no fast-math.
//
//   features  A pool's observation is the concatenation, in key order, of every state key whose name starts with "obs"
//             (the keys the collector stores), flattened to F <= kNetMaxInputs components of dtype float64, float32,
//             int32, uint8 or bool.  An actor carries lo[F] and scale[F], float64.  The feature byte of component i:
//               f_i = clamp(rint(((double)x_i - lo_i) * scale_i), 0, 127)                                (ActorFeature)
//             in double arithmetic, rint to nearest even; a product that is not finite gives 0.  Every listed dtype
//             converts to double exactly.  FEATURES LIE IN 0 .. 127 ON PURPOSE: that is the activation range of the
//             accumulator bound of pgx_net.hip.h (|w x| <= 127 * 127 over K <= 512 terms), so that proof covers the
//             first layer of an actor as it stands.
//   trunk     pgx_net.hip.h's integer network, unchanged (NetParse, the layer section, NetRs, NetAct, D, L, shifts), on
//             the feature rows.  The head has H + 1 rows, H <= 127: H = the number of actions of a discrete space, the
//             action dimension of a Box space.  logit[j] = (float)p[j] * scale_p, value = (float)p[H] * scale_v (NOT
//             clamped: returns are not game results).
//   noise     counter based: key = SM(seed ^ SM(SM(step ^ kActorSalt) + uint32(global env id))), u_j =
//             SelfplayUniform(key, j) (23 bits, 0 < u < 1).  A draw depends on (seed, env id, the collector's step
//             counter, j) only; the salt keeps the streams apart from the self-play driver's.
//   discrete  g_j = -GumbelLog(-GumbelLog(u_j));  action = the lowest j that maximises logit[j] + g_j;  top = max logit;
//             S = SUM_j GumbelExp(logit[j] - top) in ascending j;  logp = (logit[action] - top) - GumbelLog(S).
//             deterministic: argmax logit (the lowest), no noise; logp is still that action's.
//   box       sigma[H] float32, finite and > 0.  mu_j = logit[j], z_j = ActorNormal(u_j) (deterministic: 0),
//             raw_j = mu_j + sigma_j * z_j; the env gets clamp(raw_j, low_j, high_j) (float32 bounds) converted to the
//             action dtype;  logp = SUM_j ((-0.5f * z_j) * z_j - GumbelLog(sigma_j)) - 0.9189385f, ascending j: the
//             density of the RAW action.
//   ActorNormal(u): the inverse normal CDF in float32 by Wichura's PPND7 (AS 241), from + - * /, sqrtf and GumbelLog
//             only.  With 23-bit uniforms u >= 2^-24, so sqrt(-log(min(u, 1 - u))) <= 4.08 < 5 and PPND7's far-tail
//             branch is never reached: it is left out.  u - 0.5 and 1 - u are exact, so ActorNormal(1 - u) =
//             -ActorNormal(u) for every u.  Measured over all 2^23 inputs against float64 (tests/test_actor_host.py):
//             max |error| 1.260977683159581e-06 (at the smallest u), max relative error 3.924487003430764e-07; finite and
//             strictly increasing everywhere.
//
// THE BLOB (little endian, 4-byte aligned): a 36-byte header -- uint32 magic "EPAA", int32 version 1, int32 F, H, D, L,
// kind (0 discrete, 1 box), float32 scale_p, scale_v -- then lo[F], scale[F] float64, sigma[H] float32 (box only), then
// the layer section exactly as a PGXN blob has it behind its header.  ActorParse refuses what NetParse refuses, and a
// lo, scale or sigma that is not finite, and sigma <= 0.
#ifndef ENVPOOL_AMD_CSRC_ACTOR_HIP_H_
#define ENVPOOL_AMD_CSRC_ACTOR_HIP_H_

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pgx_net.hip.h"
#include "pgx_selfplay.hip.h"
#include "rollout.hip.h"

namespace epa {
namespace actor {

constexpr uint32_t kActorMagic = 0x41415045u;  // "EPAA"
constexpr int kActorVersion = 1;
constexpr int kActorHeaderBytes = 36;
constexpr int kDiscrete = 0, kBox = 1;
constexpr uint64_t kActorSalt = 0x41435452ull;  // "ACTR": no stream of the self-play driver's
constexpr int kFeatureRows = 64;                // rows per block of ActorFeatures
constexpr int kFeatureBlock = 256;              // its threads
constexpr unsigned kFlagDeterministic = 1u;     // the flags word of begin
// dtype codes of a feature key (include/envpool_amd.h: EPA_I32 ..)
constexpr int kI32 = 0, kF32 = 1, kF64 = 2, kBool = 3, kU8 = 4;

// ---- features --------------------------------------------------------------------------------------------------------
PGX_HD inline unsigned char ActorFeature(double x, double lo, double scale) {
  const double p = (x - lo) * scale;
  if (!(fabs(p) <= DBL_MAX)) return 0;  // NaN and the infinities
  const double r = rint(p);
  return (unsigned char)(r < 0.0 ? 0.0 : (r > 127.0 ? 127.0 : r));
}
PGX_HD inline double ActorLoad(const char* src, int dtype, size_t i) {
  switch (dtype) {
    case kF64: return reinterpret_cast<const double*>(src)[i];
    case kF32: return (double)reinterpret_cast<const float*>(src)[i];
    case kI32: return (double)reinterpret_cast<const int32_t*>(src)[i];
    default: return (double)reinterpret_cast<const unsigned char*>(src)[i];  // uint8, bool
  }
}
// the obs keys of one features launch: key j's rows [N][elems], its components at comp0 of the F
struct FeatureKeys {
  int n, F;
  const char* src[rollout::kMaxKeys];
  int elems[rollout::kMaxKeys], dtype[rollout::kMaxKeys], comp0[rollout::kMaxKeys];
};
// The share of thread `tid` in the feature bytes of key j of the block's rows [r0, r0 + nr): element i of the key's span
// (consecutive threads, consecutive elements) goes to byte (i / elems) * F + comp0 + i % elems of `stage`.
PGX_HD inline void FeatureKeySpan(const FeatureKeys& k, int j, const double* lo, const double* scale, int r0, int nr,
                                  unsigned char* stage, int tid, int nthreads) {
  const int elems = k.elems[j], comp0 = k.comp0[j], dtype = k.dtype[j];
  const char* src = k.src[j];
  const size_t first = (size_t)r0 * (size_t)elems;
  for (int i = tid; i < nr * elems; i += nthreads) {
    const int row = i / elems, c = comp0 + (i - row * elems);
    stage[(size_t)row * k.F + c] = ActorFeature(ActorLoad(src, dtype, first + (size_t)i), lo[c], scale[c]);
  }
}

// ---- noise -----------------------------------------------------------------------------------------------------------
PGX_HD inline uint64_t ActorKey(uint64_t seed, int env_id, long long step) {
  return pgx::PlayoutMix(seed ^ pgx::PlayoutMix(pgx::PlayoutMix((uint64_t)step ^ kActorSalt) + (uint64_t)(uint32_t)env_id));
}

// ---- the inverse normal CDF ---------------------------------------------------------------------------------------------
PGX_HD inline float ActorNormal(float u) {
  const float q = u - 0.5f;
  if ((q < 0.0f ? -q : q) <= 0.425f) {
    const float r = 0.180625f - q * q;
    const float num = ((5.9109374720e+01f * r + 1.5929113202e+02f) * r + 5.0434271938e+01f) * r + 3.3871327179e+00f;
    const float den = ((6.7187563600e+01f * r + 7.8757757664e+01f) * r + 1.7895169469e+01f) * r + 1.0f;
    return (q * num) / den;
  }
  float r = q < 0.0f ? u : 1.0f - u;
  r = sqrtf(-pgx::GumbelLog(r)) - 1.6f;
  const float num = ((1.7023821103e-01f * r + 1.3067284816e+00f) * r + 2.7568153900e+00f) * r + 1.4234372777e+00f;
  const float den = (1.2021132975e-01f * r + 7.3700164250e-01f) * r + 1.0f;
  const float v = num / den;
  return q < 0.0f ? -v : v;
}

// ---- heads -----------------------------------------------------------------------------------------------------------
struct SampleOut {
  int action;  // discrete
  float logp, value;
};
// One row of a discrete head: p [H + 1], two passes with running values.
PGX_HD inline SampleOut SampleDiscrete(const int32_t* p, int H, float scale_p, float scale_v, uint64_t key,
                                       bool deterministic) {
  SampleOut o;
  float top = -FLT_MAX, best = -FLT_MAX, best_logit = 0.0f;
  o.action = 0;
  for (int j = 0; j < H; ++j) {
    const float l = pgx::NetLogit(p[j], scale_p);
    const float s = deterministic ? l : l + pgx::SelfplayNoise(key, j);
    top = l > top ? l : top;
    if (j == 0 || s > best) {
      best = s;
      best_logit = l;
      o.action = j;
    }
  }
  float sum = 0.0f;
  for (int j = 0; j < H; ++j) sum = sum + pgx::GumbelExp(pgx::NetLogit(p[j], scale_p) - top);
  o.logp = (best_logit - top) - pgx::GumbelLog(sum);
  o.value = (float)p[H] * scale_v;
  return o;
}
// Component j of a Box head: the raw action and what it adds to logp (before the constant).
struct BoxTerm {
  float raw, clamped, term;
};
PGX_HD inline BoxTerm SampleBoxTerm(int32_t pj, float scale_p, float sigma, float low, float high, uint64_t key, int j,
                                    bool deterministic) {
  BoxTerm t;
  const float mu = pgx::NetLogit(pj, scale_p);
  const float z = deterministic ? 0.0f : ActorNormal(pgx::SelfplayUniform(key, j));
  t.raw = mu + sigma * z;
  t.clamped = t.raw < low ? low : (t.raw > high ? high : t.raw);
  t.term = ((-0.5f * z) * z - pgx::GumbelLog(sigma)) - 0.9189385f;
  return t;
}

// One row of a Box head: action [H] of the env's dtype T out (null: nothing is written).
template <class T>
PGX_HD inline SampleOut SampleBox(const int32_t* p, int H, float scale_p, float scale_v, const float* sigma,
                                  const float* low, const float* high, uint64_t key, bool deterministic, T* action) {
  SampleOut o;
  o.action = 0;
  float logp = 0.0f;
  for (int j = 0; j < H; ++j) {
    const BoxTerm t = SampleBoxTerm(p[j], scale_p, sigma[j], low[j], high[j], key, j, deterministic);
    if (action != nullptr) action[j] = (T)t.clamped;
    logp = logp + t.term;
  }
  o.logp = logp;
  o.value = (float)p[H] * scale_v;
  return o;
}

// ---- the blob ----------------------------------------------------------------------------------------------------------
struct ActorView {
  int F, H, D, L, kind;
  float scale_p, scale_v;
  std::vector<double> lo, scale;
  std::vector<float> sigma;
  std::vector<uint32_t> net_blob;  // the PGXN blob of the trunk (header + the layer section), which `net` points into
  size_t net_bytes;                // its bytes
  pgx::NetView net;
};
inline size_t ActorBlobBytes(int F, int H, int D, int L, int kind) {
  return (size_t)kActorHeaderBytes + 16 * (size_t)F + (kind == kBox ? 4 * (size_t)H : 0) +
         (pgx::NetBlobBytes(F, H, D, L) - (size_t)pgx::kNetHeaderBytes);
}
inline bool ActorParse(const void* blob, size_t bytes, ActorView* v, char* err, size_t err_bytes) {
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  if (blob == nullptr || reinterpret_cast<uintptr_t>(blob) % 4 != 0) {
    std::snprintf(err, err_bytes, "actor: the blob must be 4-byte aligned");
    return false;
  }
  if (bytes < (size_t)kActorHeaderBytes) {
    std::snprintf(err, err_bytes, "actor: a blob of %zu bytes is shorter than a header", bytes);
    return false;
  }
  uint32_t magic;
  int32_t head[6];
  float sc[2];
  std::memcpy(&magic, p, 4);
  std::memcpy(head, p + 4, 24);
  std::memcpy(sc, p + 28, 8);
  if (magic != kActorMagic) {
    std::snprintf(err, err_bytes, "actor: the blob does not begin with the magic EPAA");
    return false;
  }
  if (head[0] != kActorVersion) {
    std::snprintf(err, err_bytes, "actor: version = %d must be %d", head[0], kActorVersion);
    return false;
  }
  v->F = head[1], v->H = head[2], v->D = head[3], v->L = head[4], v->kind = head[5];
  v->scale_p = sc[0], v->scale_v = sc[1];
  if (v->kind != kDiscrete && v->kind != kBox) {
    std::snprintf(err, err_bytes, "actor: kind = %d must be 0 (discrete) or 1 (box)", v->kind);
    return false;
  }
  // the trunk's header as NetParse takes it: it checks F, H (its A), D, L, the scales and the size of the layer section
  const size_t front = (size_t)kActorHeaderBytes +
                       ((v->F >= 1 && v->F <= pgx::kNetMaxInputs) ? 16 * (size_t)v->F : 0) +
                       ((v->kind == kBox && v->H >= 1 && v->H <= pgx::kNetMaxActions) ? 4 * (size_t)v->H : 0);
  const size_t rest = bytes >= front ? bytes - front : 0;
  v->net_blob.assign(((size_t)pgx::kNetHeaderBytes + rest + 3) / 4, 0u);
  unsigned char* nb = reinterpret_cast<unsigned char*>(v->net_blob.data());
  const uint32_t net_magic = pgx::kNetMagic;
  const int32_t net_head[5] = {pgx::kNetVersion, v->F, v->H, v->D, v->L};
  std::memcpy(nb, &net_magic, 4);
  std::memcpy(nb + 4, net_head, 20);
  std::memcpy(nb + 24, sc, 8);
  if (rest != 0) std::memcpy(nb + pgx::kNetHeaderBytes, p + front, rest);
  v->net_bytes = (size_t)pgx::kNetHeaderBytes + rest;
  if (!pgx::NetParse(nb, v->net_bytes, &v->net, err, err_bytes)) return false;
  v->lo.resize((size_t)v->F);
  v->scale.resize((size_t)v->F);
  std::memcpy(v->lo.data(), p + kActorHeaderBytes, 8 * (size_t)v->F);
  std::memcpy(v->scale.data(), p + kActorHeaderBytes + 8 * (size_t)v->F, 8 * (size_t)v->F);
  for (int i = 0; i < v->F; ++i) {
    if (!(std::fabs(v->lo[(size_t)i]) <= DBL_MAX) || !(std::fabs(v->scale[(size_t)i]) <= DBL_MAX)) {
      std::snprintf(err, err_bytes, "actor: lo and scale must be finite (component %d)", i);
      return false;
    }
  }
  v->sigma.clear();
  if (v->kind == kBox) {
    v->sigma.resize((size_t)v->H);
    std::memcpy(v->sigma.data(), p + kActorHeaderBytes + 16 * (size_t)v->F, 4 * (size_t)v->H);
    for (int j = 0; j < v->H; ++j) {
      if (!(v->sigma[(size_t)j] > 0.0f && v->sigma[(size_t)j] <= FLT_MAX)) {
        std::snprintf(err, err_bytes, "actor: sigma must be finite and above 0 (component %d)", j);
        return false;
      }
    }
  }
  return true;
}

// bytes the logp and value buffers add to a collector (rollout.hip.h: RolloutBytes)
PGX_HD inline long long ActorRolloutBytes(long long n, long long horizon) { return 4 * horizon * n + 4 * (horizon + 1) * n; }

}  // namespace actor
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_ACTOR_HIP_H_
