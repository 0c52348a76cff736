// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_selfplay.hip.h, the contract of the PGX
// self-play driver, built with g++ by tests/test_pgx_selfplay_host.py: the key, the uniform, GumbelLog, the noise rows,
// the PUCT move of a row as a walk over its actions, and the tally.  Not linked by envpool_amd/.
//
// With -DPGX_SELFPLAY_MAIN the file is a program of its own: a few rows of everything, for a run under the host
// sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../envpool_amd/csrc/pgx_selfplay.hip.h"

using namespace epa::pgx;

extern "C" {

uint64_t sp_key(uint64_t seed, int env_id, uint32_t t) { return SelfplayKey(seed, env_id, t); }

void sp_gumbel_log(int n, const float* x, float* out) {
  for (int i = 0; i < n; ++i) out[i] = GumbelLog(x[i]);
}

// u and g of the 23-bit integers n0 .. n0 + count - 1
void sp_noise_of(uint32_t n0, int count, float* u, float* g) {
  for (int i = 0; i < count; ++i) {
    const float x = ((float)(n0 + (uint32_t)i) + 0.5f) * 1.1920928955078125e-7f;
    u[i] = x;
    g[i] = -GumbelLog(-GumbelLog(x));
  }
}

// the [k][A] noise rows of ply t for global env ids id0 .. id0 + k - 1
void sp_noise_rows(uint64_t seed, int id0, int k, uint32_t t, int A, int noise, float* u, float* g) {
  for (int i = 0; i < k; ++i) {
    const uint64_t key = SelfplayKey(seed, id0 + i, t);
    for (int a = 0; a < A; ++a) {
      u[(size_t)i * A + a] = SelfplayUniform(key, a);
      g[(size_t)i * A + a] = noise != 0 ? SelfplayNoise(key, a) : 0.0f;
    }
  }
}

uint32_t sp_sample_at(uint64_t key, uint32_t V) { return SelfplaySampleAt(key, V); }
int sp_pick_sampled(const int32_t* visits, int A, uint32_t r) { return SelfplayPickSampled(visits, A, r); }
int sp_pick_greedy(const int32_t* visits, int A) { return SelfplayPickGreedy(visits, A); }

void sp_puct(int k, int A, const int32_t* visits, const int32_t* result_action, const int32_t* elapsed,
             int sample_plies, const uint64_t* keys, int32_t* action, float* target) {
  for (int i = 0; i < k; ++i) {
    action[i] = SelfplayPuctMove(visits + (size_t)i * A, A, result_action[i], elapsed[i], sample_plies, keys[i],
                                 target + (size_t)i * A);
  }
}

void sp_gumbel_actions(int k, const int32_t* result_action, int32_t* action) {
  for (int i = 0; i < k; ++i) action[i] = SelfplayGumbelAction(result_action[i]);
}

void sp_tally(int k, const uint8_t* done, const float* reward, const int32_t* elapsed, int64_t* out) {
  for (int i = 0; i < k; ++i) {
    int c[kSelfplayCounters];
    SelfplayTallyRow(done[i] != 0, reward[2 * (size_t)i], reward[2 * (size_t)i + 1], elapsed[i], c);
    for (int q = 0; q < kSelfplayCounters; ++q) out[q] += c[q];
  }
}

}  // extern "C"

#ifdef PGX_SELFPLAY_MAIN
int main() {
  const int k = 5, A = 65;
  std::vector<float> u((size_t)k * A), g((size_t)k * A), target((size_t)k * A);
  sp_noise_rows(7, 3, k, 11, A, 1, u.data(), g.data());
  std::vector<int32_t> visits((size_t)k * A, 0), ra(k, 0), el(k, 0), action(k, -1);
  std::vector<uint64_t> keys(k);
  for (int i = 0; i < k; ++i) {
    keys[i] = sp_key(7, 3 + i, 11);
    el[i] = i;
    for (int a = 0; a < A; ++a) visits[(size_t)i * A + a] = (a * 7 + i) % 5;
  }
  ra[4] = -1;
  sp_puct(k, A, visits.data(), ra.data(), el.data(), 3, keys.data(), action.data(), target.data());
  const uint8_t done[k] = {1, 0, 1, 1, 0};
  const float reward[2 * k] = {1, -1, 0, 0, 0, 0, -1, 1, 0, 0};
  int64_t out[kSelfplayCounters] = {0, 0, 0, 0, 0};
  sp_tally(k, done, reward, el.data(), out);
  std::printf("noise %.9g %.9g action %d %d games %lld\n", g[0], g[(size_t)k * A - 1], action[0], action[4],
              (long long)out[0]);
  return (action[4] == 0 && out[0] == 3 && out[3] == 1) ? 0 : 1;
}
#endif
