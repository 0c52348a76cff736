// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_dirichlet.hip.h, the contract of the PUCT
// exploration of the PGX self-play driver, built with g++ by tests/test_pgx_dirichlet_host.py: the sampler's constants,
// the gamma variates, the Dirichlet rows with their mix (the lane group walked as loops), the temperature weights and
// the move.  Not linked by envpool_amd/.
//
// With -DPGX_DIRICHLET_MAIN the file is a program of its own: a few rows of everything, for a run under the host
// sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../envpool_amd/csrc/pgx_dirichlet.hip.h"

using namespace epa::pgx;

extern "C" {

void dr_params(float alpha, float* out) {
  const DirichletParams p = DirichletParamsOf(alpha);
  out[0] = p.alpha, out[1] = p.d, out[2] = p.c;
}

int dr_index(int a, int j, int c) { return DirichletIndex(a, j, c); }

// g and the fallback flag of every (row, action): global env ids id0 .. id0 + k - 1 at ply t
void dr_gamma(uint64_t seed, int id0, int k, uint32_t t, int A, float alpha, float* g, int32_t* fallback) {
  const DirichletParams p = DirichletParamsOf(alpha);
  for (int i = 0; i < k; ++i) {
    const uint64_t key = SelfplayKey(seed, id0 + i, t);
    for (int a = 0; a < A; ++a) {
      int fb = 0;
      g[(size_t)i * A + a] = DirichletGamma(key, a, p, &fb);
      fallback[(size_t)i * A + a] = fb;
    }
  }
}

float dr_sum(const float* g, const uint8_t* mask, int A) { return DirichletSum(g, mask, A); }

// eta [k][A] out, prior [k][A] mixed in place; returns the legal actions that took the fallback
int dr_rows(uint64_t seed, int id0, int k, uint32_t t, int A, float alpha, float eps, const uint8_t* mask,
            const uint8_t* status, float* prior, float* eta) {
  const DirichletParams p = DirichletParamsOf(alpha);
  int fallbacks = 0;
  for (int i = 0; i < k; ++i) {
    fallbacks += DirichletRow(SelfplayKey(seed, id0 + i, t), mask + (size_t)i * A, A, p, eps, status[i],
                              eta + (size_t)i * A, prior + (size_t)i * A);
  }
  return fallbacks;
}

void dr_weights(int k, int A, const int32_t* visits, float T, uint32_t* q) {
  for (int i = 0; i < k; ++i) {
    int vmax = 0;
    for (int a = 0; a < A; ++a) vmax = visits[(size_t)i * A + a] > vmax ? visits[(size_t)i * A + a] : vmax;
    for (int a = 0; a < A; ++a) q[(size_t)i * A + a] = TemperatureWeight(visits[(size_t)i * A + a], vmax, T);
  }
}

int dr_pick(const uint32_t* q, int A, uint32_t r) {
  return SelfplayPickSampled(reinterpret_cast<const int32_t*>(q), A, r);
}

void dr_move(int k, int A, const int32_t* visits, const int32_t* result_action, const int32_t* elapsed,
             int sample_plies, const uint64_t* keys, float T, int32_t* action, float* target, uint32_t* q) {
  for (int i = 0; i < k; ++i) {
    action[i] = SelfplayPuctMoveTemp(visits + (size_t)i * A, A, result_action[i], elapsed[i], sample_plies, keys[i], T,
                                     target + (size_t)i * A, q + (size_t)i * A);
  }
}

}  // extern "C"

#ifdef PGX_DIRICHLET_MAIN
int main() {
  const int k = 5, A = 65;
  std::vector<float> g((size_t)k * A), eta((size_t)k * A), prior((size_t)k * A, 1.0f / A), target((size_t)k * A);
  std::vector<int32_t> fb((size_t)k * A);
  dr_gamma(7, 3, k, 11, A, 0.3f, g.data(), fb.data());
  std::vector<uint8_t> mask((size_t)k * A, 1), status(k, 0);
  for (int a = 0; a < A; ++a) mask[(size_t)1 * A + a] = a == 40;  // one legal action
  for (int a = 0; a < A; ++a) mask[(size_t)2 * A + a] = 0;        // none
  status[3] = 2;
  const int fallbacks = dr_rows(7, 3, k, 11, A, 0.3f, 0.25f, mask.data(), status.data(), prior.data(), eta.data());
  std::vector<int32_t> visits((size_t)k * A, 0), ra(k, 0), el(k, 0), action(k, -1);
  std::vector<uint32_t> q((size_t)k * A);
  std::vector<uint64_t> keys(k);
  for (int i = 0; i < k; ++i) {
    keys[i] = SelfplayKey(7, 3 + i, 11);
    el[i] = i;
    for (int a = 0; a < A; ++a) visits[(size_t)i * A + a] = (a * 7 + i) % 5;
  }
  ra[4] = -1;
  dr_move(k, A, visits.data(), ra.data(), el.data(), 3, keys.data(), 0.5f, action.data(), target.data(), q.data());
  std::printf("gamma %.9g eta %.9g one %.9g none %.9g kept %.9g fallbacks %d action %d %d\n", g[0], eta[0],
              eta[(size_t)A + 40], eta[(size_t)2 * A], prior[(size_t)3 * A], fallbacks, action[0], action[4]);
  return (eta[(size_t)A + 40] == 1.0f && eta[(size_t)2 * A] == 0.0f && prior[(size_t)3 * A] == 1.0f / A &&
          action[4] == 0)
             ? 0
             : 1;
}
#endif
