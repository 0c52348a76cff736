// Rollout collector: an on-policy trajectory buffer, episode statistics, GAE and observation moments for pools with one
// row per env, as __host__ __device__ pieces shared by the kernels (rollout.hip) and the g++ host harness of the tests
// (tests/cpu_harness/rollout_host.cpp, which walks the blocks and lanes as loops).
//
// The contract (DESIGN.md section 2 "Rollout collector").  N = the pool's envs, T = the horizon, e = a LOCAL env id (the
// global id minus the pool's id offset).  A step is what the pool's step kernel wrote into its result block: rows in
// any order, row i belonging to env env_id[i].
//   buffers   obs_k [T+1][N][row_k] per state key whose name starts with "obs"; action [T][N][row_a]; reward f32 [T][N];
//             term, trunc, mask u8 [T][N].  Row e of every slot is env e's, whatever row of the batch it came in.
//   reset()   obs -> slot 0; carry[e] = 0, the episode accumulators = 0 (an episode under way is abandoned); t = 0
//   step()    at slot t, per row i with e = env_id[i], d = done[i] != 0, tr = trunc[i] != 0:           (StepRow)
//               obs rows -> slot t+1, the action row -> slot t, reward[t][e] = reward[i]
//               mask[t][e] = carry[e] == 0;  term[t][e] = d && !tr;  trunc[t][e] = tr;  carry[e] = d
//               mask: ret_e += (double)reward[i] (float64), len_e += 1
//               d: the env EMITS (e + offset, the collector's step counter, ret_e, len_e); ret_e = 0, len_e = 0
//             mask[t][e] == 0 exactly when the step was the auto-reset step that follows a done: its action was
//             ignored, its reward is 0 and slot t holds the final observation of the episode before.
//   episodes  the emissions of one step are appended in env id order, successive steps in step order: emission number r
//             (0-based, in env id order) of a step that starts with `base` rows is written to row base + r iff
//             base + r < capacity (ScanFits), otherwise dropped; count = min(capacity, base + total), dropped +=
//             base + total - count (ScanCommit).  Integer only: ranks come from ballots and scanned counts.
//   gae()     per env, t = T-1 .. 0, float32, no contraction (GaeStep)
//   moments   per component c of a float obs key, float64: count += N, sum += S1, sumsq += S2 per stored slot, where
//             S1, S2 are the sums of x and x * x over the slot's N rows IN ENV ORDER by a fixed tree: leaves of
//             kMomentLeaf consecutive rows summed in row order, kMomentLeaves consecutive leaves summed in leaf order
//             (a group), the groups summed in group order.  No atomics: two runs give the same bits.
//   next()    obs slot t -> slot 0; t = 0; carry, accumulators, episodes and moments are kept (slot 0 is not counted
//             into the moments again)
#ifndef ENVPOOL_AMD_CSRC_ROLLOUT_HIP_H_
#define ENVPOOL_AMD_CSRC_ROLLOUT_HIP_H_

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ROLLOUT_HD __host__ __device__
#else
#define ROLLOUT_HD
#endif

namespace epa {
namespace rollout {

constexpr int kMaxKeys = 8;                       // obs keys plus the action key: the rows one store launch moves
constexpr int kStoreRows = 64;                    // batch rows per block of the store kernel
constexpr int kStoreBlock = 256;                  // its threads
constexpr int kScanEnvs = 1024;                   // envs per block of the episode scan (= its threads)
constexpr int kMomentLeaf = 16;                   // rows of a leaf
constexpr int kMomentLeaves = 16;                 // leaves of a group
constexpr int kMomentRows = kMomentLeaf * kMomentLeaves;  // rows of a group (one block)
constexpr long long kMaxBytes = 1ll << 31;        // the buffers of one collector (RolloutBytes)
constexpr unsigned kFlagMoments = 1u;             // the flags word of begin

// bytes of a collector's buffers, the figure the 2 GiB limit is about: obs_bytes and action_bytes per env and slot
ROLLOUT_HD inline long long RolloutBytes(long long n, long long horizon, long long episodes, long long obs_bytes,
                                         long long action_bytes) {
  return (horizon + 1) * n * obs_bytes + horizon * n * (action_bytes + 4 + 3) + episodes * 24;
}

// ---- store plan ------------------------------------------------------------------------------------------------------
// How a span of `bytes` bytes goes from src to dst: where both have the same offset inside a 16-byte word, `head`
// bytes up to dst's first boundary, `words` 16-byte words and `tail` bytes; otherwise in 4-byte units if everything is
// a multiple of 4, otherwise byte by byte (unit 1: all of it is `head`).
struct StorePlan {
  int unit;  // 16, 4 or 1
  size_t head, words, tail;
};
ROLLOUT_HD inline StorePlan StorePlanOf(uintptr_t src, uintptr_t dst, size_t bytes) {
  StorePlan p{1, bytes, 0, 0};
  if (((src ^ dst) & 15) == 0) {
    const size_t lead = (16 - (dst & 15)) & 15;
    p.unit = 16;
    p.head = lead < bytes ? lead : bytes;
    p.words = (bytes - p.head) / 16;
    p.tail = bytes - p.head - 16 * p.words;
  } else if (((src | dst | bytes) & 3) == 0) {
    p.unit = 4;
    p.head = 0;
    p.words = bytes / 4;
  }
  return p;
}
struct alignas(16) Word16 {
  uint32_t w[4];
};
// the share of thread `tid` of `nthreads` in the copy of one span
ROLLOUT_HD inline void CopySpan(const char* src, char* dst, size_t bytes, int tid, int nthreads) {
  const StorePlan p = StorePlanOf(reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(dst), bytes);
  for (size_t i = (size_t)tid; i < p.head; i += (size_t)nthreads) dst[i] = src[i];
  if (p.unit == 16) {
    const Word16* s = reinterpret_cast<const Word16*>(src + p.head);
    Word16* d = reinterpret_cast<Word16*>(dst + p.head);
    for (size_t i = (size_t)tid; i < p.words; i += (size_t)nthreads) d[i] = s[i];
    const size_t at = p.head + 16 * p.words;
    for (size_t i = (size_t)tid; i < p.tail; i += (size_t)nthreads) dst[at + i] = src[at + i];
  } else if (p.unit == 4) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (size_t i = (size_t)tid; i < p.words; i += (size_t)nthreads) d[i] = s[i];
  }
}

// the keys of one store launch: key j's rows of the batch go to its slot of the buffer, row e of N
struct StoreKeys {
  int n;                          // keys in use
  const char* src[kMaxKeys];      // the batch's section (the action: the caller's rows), row i at i * row_bytes
  char* dst[kMaxKeys];            // the slot, row e at e * row_bytes
  int row_bytes[kMaxKeys];
};

// ---- step: flags and episode accumulators ----------------------------------------------------------------------------
struct StepRowOut {
  unsigned char mask, term, trunc, carry, emit;
};
ROLLOUT_HD inline StepRowOut StepRow(bool done, bool trunc, float reward, unsigned char carry, double* ret, int32_t* len) {
  StepRowOut o;
  o.mask = carry == 0 ? 1 : 0;
  o.term = (done && !trunc) ? 1 : 0;
  o.trunc = trunc ? 1 : 0;
  o.carry = done ? 1 : 0;
  o.emit = o.carry;
  if (o.mask) {
    *ret = *ret + (double)reward;
    *len = *len + 1;
  }
  return o;
}

// ---- episode scan ------------------------------------------------------------------------------------------------------
ROLLOUT_HD inline bool ScanFits(long long base, long long rank, int capacity) { return base + rank < (long long)capacity; }
struct ScanCommitOut {
  int32_t count;
  long long dropped;
};
ROLLOUT_HD inline ScanCommitOut ScanCommit(long long base, long long total, int capacity) {
  const long long end = base + total;
  ScanCommitOut o;
  o.count = (int32_t)(end < (long long)capacity ? end : (long long)capacity);
  o.dropped = end - (long long)o.count;
  return o;
}
// the control words of a collector, 64 bytes: the row count as the readers see it; the count a step's scan starts
// from, by the parity of the step counter (a scan reads base[s & 1] and its last block writes base[(s + 1) & 1] and
// count, so no block reads a word another block of the launch writes); episodes finished and dropped since begin
struct Control {
  int32_t count;
  int32_t base[2];
  int32_t pad;
  long long finished;
  long long dropped;
  long long reserved[4];
};

// ---- GAE -------------------------------------------------------------------------------------------------------------
// gl = fl32(gamma * lam).  Flags select; nothing is multiplied by 0 or 1.
ROLLOUT_HD inline float GaeStep(float reward, float value, float value_next, bool term, bool trunc, bool mask, float gamma,
                                float gl, float next) {
  const float d = term ? reward : reward + gamma * value_next;
  const float delta = d - value;
  float a = (term || trunc) ? delta : delta + gl * next;
  a = mask ? a : 0.0f;
  return a;
}
// one env's recurrence over the horizon: arrays are time-major with stride n, this env at column e
ROLLOUT_HD inline void GaeEnv(int horizon, int n, int e, const float* reward, const unsigned char* term,
                              const unsigned char* trunc, const unsigned char* mask, const float* values, float gamma,
                              float lam, float* adv, float* ret) {
  const float gl = gamma * lam;
  float next = 0.0f;
  float v1 = values[(size_t)horizon * n + e];
  for (int t = horizon - 1; t >= 0; --t) {
    const size_t at = (size_t)t * n + e;
    const float v = values[at];
    const float a = GaeStep(reward[at], v, v1, term[at] != 0, trunc[at] != 0, mask[at] != 0, gamma, gl, next);
    adv[at] = a;
    ret[at] = a + v;
    next = a;
    v1 = v;
  }
}

// ---- moments ---------------------------------------------------------------------------------------------------------
// a leaf: rows [r0, r1) of component c of x [rows][comps], in row order
template <class T>
ROLLOUT_HD inline void MomentLeafSum(const T* x, int comps, int c, int r0, int r1, double* s1, double* s2) {
  double a = 0.0, b = 0.0;
  for (int r = r0; r < r1; ++r) {
    const double v = (double)x[(size_t)r * comps + c];
    a = a + v;
    b = b + v * v;
  }
  *s1 = a;
  *s2 = b;
}
ROLLOUT_HD inline int MomentGroups(int n) { return (n + kMomentRows - 1) / kMomentRows; }

}  // namespace rollout
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_ROLLOUT_HIP_H_
