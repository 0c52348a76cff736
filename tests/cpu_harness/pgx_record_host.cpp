// Host build of the PGX self-play recorder (envpool_amd/csrc/pgx_record.hip.h) for the CPU tests: the pieces the
// kernels are made of, with the lanes walked as loops and the pool replaced by the caller's rows -- a position comes
// in as its hidden words (pgx::SetHidden), with the env's done flag and elapsed step beside it.
//   g++ -O2 -std=c++17 -shared -fPIC tests/cpu_harness/pgx_record_host.cpp -o libpgxrecordhost.so
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../envpool_amd/csrc/pgx_record.hip.h"

using namespace epa::pgx;

namespace {

struct Rec {
  int game, n_envs, capacity, plies, nsym, id_offset, A, OB, PS;
  std::vector<State> states;
  std::vector<int32_t> elapsed, staged, plan;
  std::vector<uint32_t> staged_policy;
  std::vector<uint8_t> obs, mask, sym;
  std::vector<uint32_t> policy, value;
  std::vector<int32_t> ply, env_id;
  int32_t count;
  long long counters[4];
};

template <int G>
Rec* Begin(int n_envs, int capacity, int max_plies, int symmetries, int id_offset) {
  Rec* r = new Rec{};
  r->game = G;
  r->n_envs = n_envs;
  r->capacity = capacity;
  r->plies = RecordPlies(max_plies);
  r->nsym = symmetries ? RecordSyms<G>() : 1;
  r->id_offset = id_offset;
  r->A = Dims<G>::A;
  r->OB = GuidedObsElems<G>();
  r->PS = RecordPolicyStride<G>();
  const size_t rows = (size_t)n_envs * r->plies, cap = (size_t)capacity;
  r->states.resize(rows);
  r->elapsed.resize(rows);
  r->staged_policy.assign(rows * r->PS, 0xdeadbeefu);
  r->staged.assign(n_envs, 0);
  r->plan.assign(n_envs, 0);
  r->obs.assign(cap * r->OB, 0xee);
  r->mask.assign(cap * r->A, 0xee);
  r->policy.assign(cap * r->A, 0xdeadbeefu);
  r->value.assign(cap, 0xdeadbeefu);
  r->ply.assign(cap, -7);
  r->env_id.assign(cap, -7);
  r->sym.assign(cap, 0xee);
  return r;
}

// PgxRecordAdd: the decision per row, then the row's words
template <int G>
int Add(Rec& r, int k, const int* ids, const int32_t* hidden, const uint8_t* over, const int32_t* elapsed,
        const uint32_t* policy) {
  constexpr int A = Dims<G>::A, PS = RecordPolicyStride<G>(), W = HiddenWords<G>();
  for (int i = 0; i < k; ++i) {
    const int e = ids[i];
    State s{};
    if (!over[i] && !SetHidden<G>(s, hidden + (size_t)i * W)) return -1;
    const RecordAddPlan p = RecordAddDecide(over[i] != 0, r.staged[e], elapsed[i], r.plies);
    r.counters[2] += p.drop_games;
    r.counters[3] += p.drop_plies;
    r.staged[e] = p.staged;
    if (p.slot < 0) continue;
    const size_t dst = (size_t)e * r.plies + p.slot;
    r.elapsed[dst] = elapsed[i];
    r.states[dst] = s;
    for (int q = 0; q < PS / 4; ++q) {  // a 16-byte word per lane
      for (int j = 0; j < 4; ++j) {
        const int a = q * 4 + j;
        r.staged_policy[dst * PS + a] = a < A ? RecordClean(policy[(size_t)i * A + a], Has(s.m, a)) : 0u;
      }
    }
  }
  return 0;
}

// PgxRecordPlan in trips of `block` rows (any block size gives the same plan), then PgxRecordEmit row by row
template <int G>
void Finish(Rec& r, int k, const int* ids, const uint32_t* reward, const uint8_t* done, int block) {
  constexpr int A = Dims<G>::A, OB = GuidedObsElems<G>(), PS = RecordPolicyStride<G>();
  const int NS = r.nsym;
  const long long base = r.count;
  long long carry = 0, acc[4] = {0, 0, 0, 0};
  for (int row0 = 0; row0 < k; row0 += block) {
    long long total = 0;
    for (int t = 0; t < block && row0 + t < k; ++t) {
      const int i = row0 + t, n = r.staged[ids[i]];
      const int c = RecordGameSamples(done[i] != 0, n, NS);
      const long long off = carry + total;
      int code = kRecordNoGame;
      if (c > 0) {
        if (RecordFits(base, off, c, r.capacity)) {
          code = (int)(base + off);
          acc[0] += c;
          acc[1] += 1;
        } else {
          code = kRecordDropped;
          acc[2] += 1;
          acc[3] += n;
        }
      }
      r.plan[i] = code;
      total += c;
    }
    carry += total;
  }
  r.count = (int32_t)(base + acc[0]);
  for (int j = 0; j < 4; ++j) r.counters[j] += acc[j];
  for (int row = 0; row < k; ++row) {
    const int code = r.plan[row];
    if (code == kRecordNoGame) continue;
    const int e = ids[row], n = r.staged[e];
    if (code >= 0) {
      for (int p = 0; p < n; ++p) {
        View view{};
        view.s = r.states[(size_t)e * r.plies + p];
        const int mover = SearchMover<G>(view.s);
        const uint32_t* pol = &r.staged_policy[((size_t)e * r.plies + p) * PS];
        const size_t s0 = (size_t)code + (size_t)p * NS;
        for (int i = 0; i < NS * OB; ++i) r.obs[s0 * OB + i] = (uint8_t)RecordObsElem<G>(view, mover, i / OB, i % OB);
        for (int i = 0; i < NS * A; ++i) r.mask[s0 * A + i] = (uint8_t)RecordMaskElem<G>(view, i / A, i % A);
        for (int i = 0; i < NS * A; ++i) r.policy[s0 * A + i] = pol[RecordPolicySource<G>(i / A, i % A)];
        for (int lane = 0; lane < NS; ++lane) {
          r.value[s0 + lane] = reward[(size_t)row * 2 + mover];
          r.ply[s0 + lane] = r.elapsed[(size_t)e * r.plies + p];
          r.env_id[s0 + lane] = e + r.id_offset;
          r.sym[s0 + lane] = (uint8_t)lane;
        }
      }
    }
    r.staged[e] = 0;
  }
}

// one step from a position given as hidden words: both seats' obs rows, the mask, done, the rewards, the hidden words
template <int G>
int StepFrom(const int32_t* hidden, int action, uint8_t* obs, uint8_t* mask, int32_t* done, float* reward,
             int32_t* hidden_out) {
  View v{};
  if (!SetHidden<G>(v.s, hidden)) return -1;
  const Rewards rw = Step<G>(v.s, action);
  for (int i = 0; i < ObsElems<G>(); ++i) obs[i] = (uint8_t)Elem<G>(v, kObs, i);
  for (int i = 0; i < Dims<G>::A; ++i) mask[i] = (uint8_t)Elem<G>(v, kMask, i);
  *done = v.s.done;
  reward[0] = rw.r[0];
  reward[1] = rw.r[1];
  Hidden<G>(v.s, hidden_out);
  return 0;
}

#define DISPATCH(game, call)                            \
  switch (game) {                                       \
    case kTicTacToe: return call(kTicTacToe);           \
    case kConnectFour: return call(kConnectFour);       \
    case kHex: return call(kHex);                       \
    default: return call(kOthello);                     \
  }

}  // namespace

extern "C" {

void* pgx_record_begin(int game, int n_envs, int capacity, int max_plies, int symmetries, int id_offset) {
#define CALL(G) Begin<G>(n_envs, capacity, max_plies, symmetries, id_offset)
  DISPATCH(game, CALL)
#undef CALL
}

int pgx_record_add(void* h, int k, const int* ids, const int32_t* hidden, const uint8_t* over, const int32_t* elapsed,
                   const uint32_t* policy) {
  Rec& r = *static_cast<Rec*>(h);
#define CALL(G) Add<G>(r, k, ids, hidden, over, elapsed, policy)
  DISPATCH(r.game, CALL)
#undef CALL
}

int pgx_record_finish(void* h, int k, const int* ids, const uint32_t* reward, const uint8_t* done, int block) {
  Rec& r = *static_cast<Rec*>(h);
#define CALL(G) (Finish<G>(r, k, ids, reward, done, block), 0)
  DISPATCH(r.game, CALL)
#undef CALL
}

int pgx_record_count(void* h) { return static_cast<Rec*>(h)->count; }

void pgx_record_counters(void* h, long long* out) { std::memcpy(out, static_cast<Rec*>(h)->counters, 32); }

void pgx_record_staged(void* h, int32_t* out) {
  Rec& r = *static_cast<Rec*>(h);
  std::memcpy(out, r.staged.data(), 4 * (size_t)r.n_envs);
}

// the first `count` rows of the seven arrays; the count goes back to 0
void pgx_record_drain(void* h, uint8_t* obs, uint8_t* mask, uint32_t* policy, uint32_t* value, int32_t* ply,
                      int32_t* env_id, uint8_t* sym) {
  Rec& r = *static_cast<Rec*>(h);
  const size_t n = (size_t)r.count;
  std::memcpy(obs, r.obs.data(), n * r.OB);
  std::memcpy(mask, r.mask.data(), n * r.A);
  std::memcpy(policy, r.policy.data(), 4 * n * r.A);
  std::memcpy(value, r.value.data(), 4 * n);
  std::memcpy(ply, r.ply.data(), 4 * n);
  std::memcpy(env_id, r.env_id.data(), 4 * n);
  std::memcpy(sym, r.sym.data(), n);
  r.count = 0;
}

void pgx_record_discard(void* h, int k, const int* ids) {
  Rec& r = *static_cast<Rec*>(h);
  for (int i = 0; i < k; ++i) r.staged[ids[i]] = 0;
}

void pgx_record_end(void* h) { delete static_cast<Rec*>(h); }

int pgx_record_syms(int game) {
#define CALL(G) RecordSyms<G>()
  DISPATCH(game, CALL)
#undef CALL
}

int pgx_record_sym_cell(int game, int j, int cell, int inverse) {
#define CALL(G) RecordSymCell<G>(j, cell, inverse != 0)
  DISPATCH(game, CALL)
#undef CALL
}

int pgx_record_sym_action(int game, int j, int a, int inverse) {
#define CALL(G) RecordSymAction<G>(j, a, inverse != 0)
  DISPATCH(game, CALL)
#undef CALL
}

int pgx_record_step(int game, const int32_t* hidden, int action, uint8_t* obs, uint8_t* mask, int32_t* done,
                    float* reward, int32_t* hidden_out) {
#define CALL(G) StepFrom<G>(hidden, action, obs, mask, done, reward, hidden_out)
  DISPATCH(game, CALL)
#undef CALL
}

}  // extern "C"
