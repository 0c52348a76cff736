// envpool_amd/csrc/rollout.hip.h built for the host: the collector's kernels (csrc/rollout.hip) restated as loops over
// their blocks and threads, with the header's __host__ __device__ pieces doing the work.  Built by
// tests/test_rollout_host.py with g++ -ffp-contract=off.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../envpool_amd/csrc/rollout.hip.h"

using namespace epa::rollout;

namespace {
struct Collector {
  int n, horizon, capacity, id_offset, nkeys;  // nkeys: the obs keys, then the action
  int t = 0;
  long long step = 0;
  std::vector<int> row_bytes, dtype;           // dtype: 0 none, 1 float32, 2 float64 (moments)
  std::vector<std::vector<char>> buf;          // per key: [T+1][N][row] (the action: [T][N][row])
  std::vector<float> reward;
  std::vector<unsigned char> term, trunc, mask, carry, emit;
  std::vector<double> acc_ret, emit_ret;
  std::vector<int32_t> acc_len, emit_len;
  std::vector<int32_t> ep_env, ep_len;
  std::vector<long long> ep_step;
  std::vector<double> ep_ret;
  Control ctl{};
  int comps = 0;
  std::vector<int> comp0;
  std::vector<double> mom;  // [3][comps]
};

// RolloutStore: blocks of kStoreRows rows, kStoreBlock threads
void Store(Collector& c, int k, const int32_t* env_id, const unsigned char* done, const unsigned char* trunc,
           const float* reward, const char* const* src, int nkeys, int obs_slot, bool scalars) {
  for (int r0 = 0; r0 < k; r0 += kStoreRows) {
    const int nr = std::min(kStoreRows, k - r0);
    int env[kStoreRows];
    bool run = true;
    for (int i = 0; i < nr; ++i) env[i] = env_id != nullptr ? env_id[r0 + i] - c.id_offset : r0 + i;
    for (int i = 0; i < nr; ++i) run = run && env[i] >= 0 && env[i] < c.n && env[i] == env[0] + i;
    for (int j = 0; j < nkeys; ++j) {
      const size_t rb = (size_t)c.row_bytes[j];
      const bool action = j == c.nkeys - 1;
      char* dst = c.buf[j].data() + (size_t)(action ? c.t : obs_slot) * (size_t)c.n * rb;
      if (run) {
        for (int tid = 0; tid < kStoreBlock; ++tid) {
          CopySpan(src[j] + (size_t)r0 * rb, dst + (size_t)env[0] * rb, (size_t)nr * rb, tid, kStoreBlock);
        }
      } else {
        for (int r = 0; r < nr; ++r) {
          if (env[r] < 0 || env[r] >= c.n) continue;
          for (int lane = 0; lane < 64; ++lane) {
            CopySpan(src[j] + (size_t)(r0 + r) * rb, dst + (size_t)env[r] * rb, rb, lane, 64);
          }
        }
      }
    }
    if (!scalars) continue;
    const size_t slot = (size_t)c.t * c.n;
    for (int i = 0; i < nr; ++i) {
      const int e = env[i];
      if (e < 0 || e >= c.n) continue;
      double ret = c.acc_ret[e];
      int32_t len = c.acc_len[e];
      const StepRowOut o = StepRow(done[r0 + i] != 0, trunc[r0 + i] != 0, reward[r0 + i], c.carry[e], &ret, &len);
      c.reward[slot + e] = reward[r0 + i];
      c.term[slot + e] = o.term;
      c.trunc[slot + e] = o.trunc;
      c.mask[slot + e] = o.mask;
      c.carry[e] = o.carry;
      c.emit[e] = o.emit;
      if (o.emit) {
        c.emit_ret[e] = ret;
        c.emit_len[e] = len;
        ret = 0.0;
        len = 0;
      }
      c.acc_ret[e] = ret;
      c.acc_len[e] = len;
    }
  }
}

// RolloutScan: blocks of kScanEnvs envs; a block's offset is the flag count of the envs in front of it
void Scan(Collector& c) {
  const int blocks = (c.n + kScanEnvs - 1) / kScanEnvs;
  const long long base = c.ctl.base[c.step & 1];
  for (int b = 0; b < blocks; ++b) {
    long long prefix = 0;
    for (int e = 0; e < b * kScanEnvs; ++e) prefix += c.emit[e];
    long long rank = prefix;
    for (int e = b * kScanEnvs; e < std::min(c.n, (b + 1) * kScanEnvs); ++e) {
      if (c.emit[e] == 0) continue;
      if (ScanFits(base, rank, c.capacity)) {
        const size_t row = (size_t)(base + rank);
        c.ep_env[row] = e + c.id_offset;
        c.ep_step[row] = c.step;
        c.ep_ret[row] = c.emit_ret[e];
        c.ep_len[row] = c.emit_len[e];
      }
      ++rank;
    }
    if (b == blocks - 1) {
      const ScanCommitOut o = ScanCommit(base, rank, c.capacity);
      c.ctl.count = o.count;
      c.ctl.base[(c.step + 1) & 1] = o.count;
      c.ctl.finished += rank;
      c.ctl.dropped += o.dropped;
    }
  }
}

// RolloutMoments + RolloutMomentsFold over one obs slot
template <class T>
void MomentsKey(Collector& c, const T* x, int comps, int comp0, std::vector<double>& partial) {
  const int groups = MomentGroups(c.n);
  for (int g = 0; g < groups; ++g) {
    for (int cc = 0; cc < comps; ++cc) {
      double t1 = 0.0, t2 = 0.0;
      for (int l = 0; l < kMomentLeaves; ++l) {
        const int r0 = std::min(c.n, g * kMomentRows + l * kMomentLeaf), r1 = std::min(c.n, r0 + kMomentLeaf);
        double s1, s2;
        MomentLeafSum(x, comps, cc, r0, r1, &s1, &s2);
        t1 = t1 + s1;
        t2 = t2 + s2;
      }
      partial[((size_t)g * c.comps + comp0 + cc) * 2] = t1;
      partial[((size_t)g * c.comps + comp0 + cc) * 2 + 1] = t2;
    }
  }
}
void Moments(Collector& c, int slot) {
  if (c.comps == 0) return;
  const int groups = MomentGroups(c.n);
  std::vector<double> partial((size_t)groups * c.comps * 2);
  for (int j = 0; j < c.nkeys - 1; ++j) {
    if (c.dtype[j] == 0) continue;
    const char* x = c.buf[j].data() + (size_t)slot * c.n * c.row_bytes[j];
    if (c.dtype[j] == 2) {
      MomentsKey(c, reinterpret_cast<const double*>(x), c.row_bytes[j] / 8, c.comp0[j], partial);
    } else {
      MomentsKey(c, reinterpret_cast<const float*>(x), c.row_bytes[j] / 4, c.comp0[j], partial);
    }
  }
  for (int cc = 0; cc < c.comps; ++cc) {
    double s1 = 0.0, s2 = 0.0;
    for (int g = 0; g < groups; ++g) {
      s1 = s1 + partial[((size_t)g * c.comps + cc) * 2];
      s2 = s2 + partial[((size_t)g * c.comps + cc) * 2 + 1];
    }
    c.mom[cc] = c.mom[cc] + (double)c.n;
    c.mom[c.comps + cc] = c.mom[c.comps + cc] + s1;
    c.mom[2 * c.comps + cc] = c.mom[2 * c.comps + cc] + s2;
  }
}
}  // namespace

extern "C" {

// row_bytes / dtype: nkeys entries, the action last (dtype 0: no moments for the key)
void* ro_begin(int n, int horizon, int capacity, int id_offset, int nkeys, const int* row_bytes, const int* dtype) {
  Collector* c = new Collector;
  c->n = n;
  c->horizon = horizon;
  c->capacity = capacity;
  c->id_offset = id_offset;
  c->nkeys = nkeys;
  c->row_bytes.assign(row_bytes, row_bytes + nkeys);
  c->dtype.assign(dtype, dtype + nkeys);
  c->comp0.assign((size_t)nkeys, 0);
  for (int j = 0; j < nkeys; ++j) {
    const size_t slots = (size_t)(j == nkeys - 1 ? horizon : horizon + 1);
    // (16 spare bytes in front would hide an alignment bug: the buffers start where the vector puts them)
    c->buf.emplace_back(slots * (size_t)n * (size_t)row_bytes[j], 0);
    if (j < nkeys - 1 && dtype[j] != 0) {
      c->comp0[(size_t)j] = c->comps;
      c->comps += row_bytes[j] / (dtype[j] == 2 ? 8 : 4);
    }
  }
  const size_t tn = (size_t)horizon * n;
  c->reward.assign(tn, 0.0f);
  c->term.assign(tn, 0);
  c->trunc.assign(tn, 0);
  c->mask.assign(tn, 0);
  c->carry.assign((size_t)n, 0);
  c->emit.assign((size_t)n, 0);
  c->acc_ret.assign((size_t)n, 0.0);
  c->emit_ret.assign((size_t)n, 0.0);
  c->acc_len.assign((size_t)n, 0);
  c->emit_len.assign((size_t)n, 0);
  c->ep_env.assign((size_t)capacity, 0);
  c->ep_len.assign((size_t)capacity, 0);
  c->ep_step.assign((size_t)capacity, 0);
  c->ep_ret.assign((size_t)capacity, 0.0);
  c->mom.assign(3 * (size_t)c->comps, 0.0);
  return c;
}
void ro_end(void* h) { delete static_cast<Collector*>(h); }

// src: the obs keys' rows of the batch
void ro_reset(void* h, int k, const int32_t* env_id, const char* const* src) {
  Collector& c = *static_cast<Collector*>(h);
  c.t = 0;
  Store(c, k, env_id, nullptr, nullptr, nullptr, src, c.nkeys - 1, 0, false);
  std::fill(c.carry.begin(), c.carry.end(), 0);
  std::fill(c.acc_ret.begin(), c.acc_ret.end(), 0.0);
  std::fill(c.acc_len.begin(), c.acc_len.end(), 0);
  Moments(c, 0);
}
// src: the obs keys' rows of the batch, then the action rows
int ro_step(void* h, int k, const int32_t* env_id, const unsigned char* done, const unsigned char* trunc,
            const float* reward, const char* const* src) {
  Collector& c = *static_cast<Collector*>(h);
  if (c.t >= c.horizon) return 1;
  Store(c, k, env_id, done, trunc, reward, src, c.nkeys, c.t + 1, true);
  Scan(c);
  Moments(c, c.t + 1);
  c.t += 1;
  c.step += 1;
  return 0;
}
void ro_next(void* h) {
  Collector& c = *static_cast<Collector*>(h);
  for (int j = 0; j < c.nkeys - 1; ++j) {
    const size_t slot = (size_t)c.n * c.row_bytes[j];
    std::memmove(c.buf[j].data(), c.buf[j].data() + (size_t)c.t * slot, slot);
  }
  c.t = 0;
}
// key < nkeys: that key's buffer; then reward, term, trunc, mask
const void* ro_buffer(void* h, int key) {
  Collector& c = *static_cast<Collector*>(h);
  if (key < c.nkeys) return c.buf[(size_t)key].data();
  switch (key - c.nkeys) {
    case 0: return c.reward.data();
    case 1: return c.term.data();
    case 2: return c.trunc.data();
    default: return c.mask.data();
  }
}
void ro_gae(void* h, const float* values, float gamma, float lam, float* adv, float* ret) {
  Collector& c = *static_cast<Collector*>(h);
  for (int e = 0; e < c.n; ++e) {
    GaeEnv(c.horizon, c.n, e, c.reward.data(), c.term.data(), c.trunc.data(), c.mask.data(), values, gamma, lam, adv,
           ret);
  }
}
// out: count, finished, dropped, step, t
void ro_counters(void* h, long long* out) {
  Collector& c = *static_cast<Collector*>(h);
  out[0] = c.ctl.count;
  out[1] = c.ctl.finished;
  out[2] = c.ctl.dropped;
  out[3] = c.step;
  out[4] = c.t;
}
void ro_episodes(void* h, int32_t* env_id, long long* step, double* ret, int32_t* length) {
  Collector& c = *static_cast<Collector*>(h);
  const size_t n = (size_t)c.ctl.count;
  std::memcpy(env_id, c.ep_env.data(), 4 * n);
  std::memcpy(step, c.ep_step.data(), 8 * n);
  std::memcpy(ret, c.ep_ret.data(), 8 * n);
  std::memcpy(length, c.ep_len.data(), 4 * n);
  c.ctl.count = 0;
  c.ctl.base[0] = c.ctl.base[1] = 0;
}
int ro_moments(void* h, double* out) {
  Collector& c = *static_cast<Collector*>(h);
  std::memcpy(out, c.mom.data(), 8 * c.mom.size());
  return c.comps;
}
// the store plan of one span, for the alignment cases: unit, head, words, tail
void ro_store_plan(unsigned long long src, unsigned long long dst, unsigned long long bytes, unsigned long long* out) {
  const StorePlan p = StorePlanOf((uintptr_t)src, (uintptr_t)dst, (size_t)bytes);
  out[0] = (unsigned long long)p.unit;
  out[1] = p.head;
  out[2] = p.words;
  out[3] = p.tail;
}
// CopySpan as `nthreads` threads, from src + src_off to dst + dst_off (any alignment)
void ro_copy_span(const char* src, char* dst, unsigned long long bytes, int nthreads) {
  for (int tid = 0; tid < nthreads; ++tid) CopySpan(src, dst, (size_t)bytes, tid, nthreads);
}

}  // extern "C"
