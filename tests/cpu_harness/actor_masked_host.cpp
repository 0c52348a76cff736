// The masked head (kind 2) of envpool_amd/csrc/actor.hip.h built for the host: the __host__ __device__ pieces the
// kernels' lanes run, row by row.  Built by tests/test_actor_masked_host.py with g++ -ffp-contract=off.
#include <cstring>

#include "../../envpool_amd/csrc/actor.hip.h"

using namespace epa::actor;

extern "C" {

// 1 and shape = {F, H, D, L, kind, mask0, C, nvec[4]}, or 0 and the reason
int amh_parse(const void* blob, size_t bytes, int* shape, char* err, int err_bytes) {
  ActorView v;
  err[0] = 0;
  if (!ActorParse(blob, bytes, &v, err, (size_t)err_bytes)) return 0;
  const int s[11] = {v.F, v.H, v.D, v.L, v.kind, v.mask0, v.C, v.nvec[0], v.nvec[1], v.nvec[2], v.nvec[3]};
  std::memcpy(shape, s, sizeof(s));
  return 1;
}

// ActorLegal and ActorSampleMasked: row r's H raw mask bytes at mask + r * H; its C components, logp, value and words out
void amh_sample(const int32_t* p, const unsigned char* mask, int rows, int H, float scale_p, float scale_v,
                unsigned long long seed, const int32_t* env_ids, long long step, int deterministic, int C, const int* nvec,
                int32_t* action, float* logp, float* value, uint32_t* legal) {
  for (int r = 0; r < rows; ++r) {
    LegalOfRow(reinterpret_cast<const char*>(mask), kU8, (size_t)r * H, H, legal + 4 * (size_t)r);
    const SampleOut o = SampleMasked(p + (size_t)r * (H + 1), H, legal + 4 * (size_t)r, scale_p, scale_v,
                                     ActorKey(seed, env_ids[r], step), deterministic != 0);
    ActorComponents(o.action, nvec, C, action + (size_t)r * C);
    logp[r] = o.logp, value[r] = o.value;
  }
}

}  // extern "C"
