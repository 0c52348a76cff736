// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/ppo_trainer.hip.h, the contract of the rollout
// actor's PPO trainer, built with g++ by tests/test_ppo_trainer_host.py: row loops for the loss of both heads, the
// permutation, the advantage tree and the sigma sum.  Not linked by envpool_amd/.
#include <cstdint>

#include "../../envpool_amd/csrc/ppo_trainer.hip.h"

using namespace epa::ppo;

extern "C" {

double ppo_err() { return kPpoErr; }

// p [n][H + 1], action [n], logp, adv, ret [n], mask [n] -> dp [n][H + 1], stat [n][5]
void ppo_loss_discrete(int n, int H, const int32_t* p, const int32_t* action, const float* logp, const float* adv,
                       const float* ret, const uint8_t* mask, float scale_p, float scale_v, float clip_ratio,
                       float value_weight, float entropy_weight, float* dp, float* stat) {
  const PpoOptions o = PpoOptionsOf(scale_p, scale_v, clip_ratio, value_weight, entropy_weight, n);
  for (int r = 0; r < n; ++r) {
    PpoDiscreteRow(p + (size_t)r * (H + 1), H, action[r], logp[r], adv[r], ret[r], mask[r], o, dp + (size_t)r * (H + 1),
                   stat + 5 * (size_t)r);
  }
}

// action [n][H], sigma [H] -> also dsigma [n][H]
void ppo_loss_box(int n, int H, const int32_t* p, const float* action, const float* sigma, const float* logp,
                  const float* adv, const float* ret, const uint8_t* mask, float scale_p, float scale_v, float clip_ratio,
                  float value_weight, float entropy_weight, float* dp, float* stat, float* dsigma) {
  const PpoOptions o = PpoOptionsOf(scale_p, scale_v, clip_ratio, value_weight, entropy_weight, n);
  for (int r = 0; r < n; ++r) {
    PpoBoxRow(p + (size_t)r * (H + 1), H, action + (size_t)r * H, sigma, logp[r], adv[r], ret[r], mask[r], o,
              dp + (size_t)r * (H + 1), stat + 5 * (size_t)r, dsigma + (size_t)r * H);
  }
}

uint32_t ppo_permute(uint64_t seed, uint32_t epoch, uint32_t j, uint32_t n) { return PpoPermute(seed, epoch, j, n); }

// out: count, mean, std
void ppo_adv_stats(const float* adv, const uint8_t* mask, int n, double* out) {
  AdvSums s{0.0, 0.0, 0.0};
  for (int c = 0; c < n; c += kPpoAdvChunk) {
    const AdvSums b = AdvChunkSums(adv + c, mask + c, n - c < kPpoAdvChunk ? n - c : kPpoAdvChunk);
    s.cnt = s.cnt + b.cnt, s.s1 = s.s1 + b.s1, s.s2 = s.s2 + b.s2;
  }
  out[0] = s.cnt;
  AdvMoments(s, &out[1], &out[2]);
}

float ppo_adv_normalize(float adv, double mean, double std) { return AdvNormalize(adv, mean, std); }

// the sigma gradient of dsigma [n][H]: blocks of kPpoLossRows rows in row order, the blocks in block order, in double
void ppo_sigma_sum(const float* dsigma, const uint8_t* mask, int n, int H, float* out) {
  for (int j = 0; j < H; ++j) {
    double total = 0.0;
    for (int r0 = 0; r0 < n; r0 += kPpoLossRows) {
      double s = 0.0;
      for (int r = r0; r < n && r < r0 + kPpoLossRows; ++r) {
        if (mask[r] != 0) s = s + (double)dsigma[(size_t)r * H + j];
      }
      total = total + s;
    }
    out[j] = (float)total;
  }
}

float ppo_sigma_of(double master) { return PpoSigmaOf(master); }

}  // extern "C"
