// envpool_amd/csrc/actor.hip.h built for the host: the actor's kernels (csrc/actor.hip) restated as loops over their
// blocks, threads and lanes, with the header's __host__ __device__ pieces doing the work.  Built by
// tests/test_actor_host.py with g++ -ffp-contract=off.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../envpool_amd/csrc/actor.hip.h"

using namespace epa::actor;
namespace pgx = epa::pgx;
namespace rollout = epa::rollout;

extern "C" {

void ah_feature(const double* x, const double* lo, const double* scale, int n, unsigned char* out) {
  for (int i = 0; i < n; ++i) out[i] = ActorFeature(x[i], lo[i], scale[i]);
}

// ActorFeatures: blocks of kFeatureRows rows, kFeatureBlock threads; the staging plays the kernel's LDS
void ah_features(int n, int F, int nkeys, const void* const* src, const int* elems, const int* dtype, const double* lo,
                 const double* scale, unsigned char* out) {
  FeatureKeys k{};
  k.n = nkeys;
  k.F = F;
  int comp = 0;
  for (int j = 0; j < nkeys; ++j) {
    k.src[j] = static_cast<const char*>(src[j]);
    k.elems[j] = elems[j];
    k.dtype[j] = dtype[j];
    k.comp0[j] = comp;
    comp += elems[j];
  }
  std::vector<unsigned char> lds((size_t)kFeatureRows * F + 32);
  // (the kernel's LDS base is 16-byte aligned)
  unsigned char* base = lds.data() + ((16 - (reinterpret_cast<uintptr_t>(lds.data()) & 15)) & 15);
  for (int r0 = 0; r0 < n; r0 += kFeatureRows) {
    const int nr = std::min(kFeatureRows, n - r0);
    unsigned char* dst = out + (size_t)r0 * F;
    unsigned char* stage = base + (reinterpret_cast<uintptr_t>(dst) & 15);
    for (int j = 0; j < nkeys; ++j) {
      for (int tid = 0; tid < kFeatureBlock; ++tid) FeatureKeySpan(k, j, lo, scale, r0, nr, stage, tid, kFeatureBlock);
    }
    for (int tid = 0; tid < kFeatureBlock; ++tid) {
      rollout::CopySpan(reinterpret_cast<const char*>(stage), reinterpret_cast<char*>(dst), (size_t)nr * F, tid,
                        kFeatureBlock);
    }
  }
}

void ah_normal(const float* u, int n, float* out) {
  for (int i = 0; i < n; ++i) out[i] = ActorNormal(u[i]);
}
// all 2^23 values of the uniform, in the order of n
void ah_normal_all(float* u, float* out) {
  for (uint32_t n = 0; n < (1u << 23); ++n) {
    u[n] = ((float)n + 0.5f) * 1.1920928955078125e-7f;
    out[n] = ActorNormal(u[n]);
  }
}

void ah_uniform(unsigned long long seed, int env_id, long long step, int H, float* out) {
  const uint64_t key = ActorKey(seed, env_id, step);
  for (int j = 0; j < H; ++j) out[j] = pgx::SelfplayUniform(key, j);
}

// ActorSample, one lane per row
void ah_discrete(const int32_t* p, int rows, int H, float scale_p, float scale_v, unsigned long long seed,
                 const int32_t* env_ids, long long step, int deterministic, int32_t* action, float* logp, float* value) {
  for (int r = 0; r < rows; ++r) {
    const SampleOut o = SampleDiscrete(p + (size_t)r * (H + 1), H, scale_p, scale_v, ActorKey(seed, env_ids[r], step),
                                       deterministic != 0);
    action[r] = o.action;
    logp[r] = o.logp;
    value[r] = o.value;
  }
}
void ah_box(const int32_t* p, int rows, int H, float scale_p, float scale_v, const float* sigma, const float* low,
            const float* high, unsigned long long seed, const int32_t* env_ids, long long step, int deterministic,
            float* action, float* logp, float* value) {
  for (int r = 0; r < rows; ++r) {
    const SampleOut o = SampleBox<float>(p + (size_t)r * (H + 1), H, scale_p, scale_v, sigma, low, high,
                                         ActorKey(seed, env_ids[r], step), deterministic != 0, action + (size_t)r * H);
    logp[r] = o.logp;
    value[r] = o.value;
  }
}

// 1 and shape = {F, H, D, L, kind}, or 0 and the reason
int ah_parse(const void* blob, size_t bytes, int* shape, char* err, int err_bytes) {
  ActorView v;
  err[0] = 0;
  if (!ActorParse(blob, bytes, &v, err, (size_t)err_bytes)) return 0;
  const int s[5] = {v.F, v.H, v.D, v.L, v.kind};
  std::memcpy(shape, s, sizeof(s));
  return 1;
}

// the head's integers p [rows][H + 1] of feature rows [rows][F], by the book
int ah_head(const void* blob, size_t bytes, const unsigned char* feat, int rows, int32_t* p) {
  ActorView v;
  char err[200];
  if (!ActorParse(blob, bytes, &v, err, sizeof(err))) return 0;
  const pgx::NetView& net = v.net;
  auto dot = [](const pgx::NetLayer& l, int n, const int32_t* in) {
    int32_t s = l.b[n];
    for (int k = 0; k < l.k_in; ++k) s += (int32_t)l.w[(size_t)n * l.k_in + k] * in[k];
    return s;
  };
  std::vector<int32_t> x((size_t)net.F), h((size_t)net.D), t((size_t)net.D), next((size_t)net.D);
  for (int r = 0; r < rows; ++r) {
    for (int k = 0; k < net.F; ++k) x[(size_t)k] = feat[(size_t)r * net.F + k];
    for (int n = 0; n < net.D; ++n) h[(size_t)n] = pgx::NetAct(pgx::NetRs(dot(net.layer[0], n, x.data()), net.layer[0].shift));
    for (int l = 0; l < net.L; ++l) {
      const pgx::NetLayer& l1 = net.layer[1 + 2 * l];
      const pgx::NetLayer& l2 = net.layer[2 + 2 * l];
      for (int n = 0; n < net.D; ++n) t[(size_t)n] = pgx::NetAct(pgx::NetRs(dot(l1, n, h.data()), l1.shift));
      for (int n = 0; n < net.D; ++n) {
        next[(size_t)n] = pgx::NetAct(pgx::NetRs(dot(l2, n, t.data()), l2.shift) + h[(size_t)n]);
      }
      h = next;
    }
    for (int n = 0; n <= net.A; ++n) p[(size_t)r * (net.A + 1) + n] = dot(net.layer[net.layers() - 1], n, h.data());
  }
  return 1;
}

}  // extern "C"
