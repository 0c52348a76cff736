// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_trainer.hip.h, the contract of the PGX
// trainer, built with g++ by tests/test_pgx_trainer_host.py: the loss by the book, the update of an array with its
// quantised values, the norm's chunk sums and the index hash.  Not linked by envpool_amd/.
#include <cstdint>

#include "../../envpool_amd/csrc/pgx_trainer.hip.h"

using namespace epa::pgx;

extern "C" {

double pgx_trainer_loss_err() { return kLossErr; }

// p [n][A + 1], mask [n][A], pi [n][A], z [n] -> dp [n][A + 1], loss [n][2]
void pgx_trainer_loss(int n, int A, const int32_t* p, const uint8_t* mask, const float* pi, const float* z,
                      float scale_p, float scale_v, float value_weight, float* dp, float* loss) {
  for (int r = 0; r < n; ++r) {
    TrainerLossRow(p + (size_t)r * (A + 1), mask + (size_t)r * A, pi + (size_t)r * A, z[r], A, scale_p, scale_v,
                   value_weight, (float)n, dp + (size_t)r * (A + 1), loss + 2 * (size_t)r);
  }
}

// rule: optimizer, lr, momentum, beta1, beta2, 1 - beta1, 1 - beta2, lr_t, eps, weight_decay
void pgx_trainer_update(const double* rule, int count, const float* grad, double clip, double norm, int weight,
                        double* master, double* s1, double* s2, int32_t* q) {
  const TrainerRule r{(int)rule[0], rule[1], rule[2], rule[3], rule[4], rule[5], rule[6], rule[7], rule[8], rule[9]};
  const double scale = TrainerClipScale(clip, norm);
  for (int i = 0; i < count; ++i) {
    TrainerUpdateOne(r, grad[i], scale, &master[i], &s1[i], &s2[i]);
    q[i] = weight != 0 ? TrainerQuantWeight(master[i]) : TrainerQuantBias(master[i]);
  }
}

// the sum of the chunks' partials in ascending order; count is a multiple of kTrainerChunk
double pgx_trainer_squares(const float* grad, int count) {
  double s = 0.0;
  for (int c = 0; c < count; c += kTrainerChunk) s = s + TrainerChunkSquares(grad + c);
  return s;
}

uint32_t pgx_trainer_index(uint64_t seed, uint32_t t, uint32_t j, uint32_t count) {
  return TrainerIndex(seed, t, j, count);
}

}  // extern "C"
