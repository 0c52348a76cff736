// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_guided.hip.h with tree reuse, built with g++
// by tests/test_pgx_reroot_host.py.  It is the stepwise session of pgx_guided_host.cpp with a node capacity per root
// and reroot: begin / advance / result / reroot on host memory, run the way the kernels' wave does -- lane j owns
// actions j and j + 64, the mark / rank table is filled node by node and in trips of 64, the compaction is in place in
// the one node buffer -- with the wave's lanes walked as loops.  Positions come in as the hidden words of
// pgx_env.hip.h (SetHidden) plus the done flag.  Not linked by envpool_amd/.
//
// With -DPGX_REROOT_MAIN the file is a program of its own: three rounds of Hex with a reroot between them, for a run
// under the host sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../envpool_amd/csrc/pgx_guided.hip.h"

using namespace epa::pgx;

namespace {
struct Session {
  virtual ~Session() {}
  virtual int Advance(const float* priors, const float* values, uint8_t* obs, uint8_t* mask, uint8_t* status) = 0;
  virtual void Result(int32_t* visits, float* values, int32_t* action, int32_t* nodes_used) const = 0;
  virtual int Reroot(const int32_t* actions, int s2, uint8_t* obs, uint8_t* mask, uint8_t* status) = 0;
};

template <int G>
struct Run : Session {
  static constexpr int A = Dims<G>::A, L = kSearchWave, SL = SearchSlotsPerLane<G>(), OB = GuidedObsElems<G>();
  int n, simulations, capacity, calls{0};
  float c_puct;
  std::vector<GuidedRoot> roots;
  std::vector<GuidedNode<G>> nodes;  // [n][capacity]
  std::vector<int32_t> table;        // [capacity]: the wave's LDS table

  Run(int n_, int s, int cap, float c)
      : n(n_), simulations(s), capacity(cap), c_puct(c), roots((size_t)n_), nodes((size_t)n_ * cap),
        table((size_t)cap) {}
  GuidedNode<G>* Tree(int i) { return nodes.data() + (size_t)i * capacity; }
  const GuidedNode<G>* Tree(int i) const { return nodes.data() + (size_t)i * capacity; }

  static void ClearNode(GuidedNode<G>& nd) {
    for (int lane = 0; lane < L; ++lane) {
      for (int j = 0; j < SL; ++j) {
        if (lane + L * j < A) GuidedClearEdge<G>(nd, lane + L * j);
      }
    }
  }

  void Emit(int i, const State& s, uint8_t* obs, uint8_t* mask, uint8_t* status) const {
    View view{};
    view.s = s;
    const int st = roots[(size_t)i].status, mover = SearchMover<G>(s);
    for (int e = 0; e < OB; ++e) {
      obs[(size_t)i * OB + e] = st == kGuidedEvaluate ? (uint8_t)GuidedObsElem<G>(view, mover, e) : 0;
    }
    for (int e = 0; e < A; ++e) mask[(size_t)i * A + e] = st == kGuidedEvaluate ? (uint8_t)GuidedMaskElem<G>(view, e) : 0;
    status[i] = (uint8_t)st;
  }

  int Begin(const int32_t* hidden, const uint8_t* done, uint8_t* obs, uint8_t* mask, uint8_t* status) {
    constexpr int W = HiddenWords<G>();
    for (int i = 0; i < n; ++i) {
      State root{};
      if (!SetHidden<G>(root, hidden + (size_t)i * W)) return -2;
      root.done = done[i] ? 1 : 0;
      GuidedNode<G>& n0 = Tree(i)[0];
      n0.s = root;
      n0.term0 = 0;
      ClearNode(n0);
      GuidedClearRoot(roots[(size_t)i], done[i] != 0);
      Emit(i, root, obs, mask, status);
    }
    return 0;
  }

  int Advance(const float* priors, const float* values, uint8_t* obs, uint8_t* mask, uint8_t* status) override {
    if (calls > simulations) return -4;
    int rc = 0;
    for (int i = 0; i < n; ++i) {
      GuidedRoot& rec = roots[(size_t)i];
      GuidedNode<G>* tree = Tree(i);
      State s{};
      if (rec.status != kGuidedIdle) {
        GuidedNode<G>& leaf = tree[rec.pending];
        float val0;
        if (rec.status == kGuidedEvaluate) {
          for (int lane = 0; lane < L; ++lane) {
            for (int j = 0; j < SL; ++j) {
              const int a = lane + L * j;
              if (a < A) leaf.p[a] = GuidedClean(priors[(size_t)i * A + a]);
            }
          }
          val0 = (float)SearchSign<G>(leaf.s) * GuidedCleanV(values[i]);
        } else {
          val0 = (float)leaf.term0;
        }
        for (int d = 0; d < rec.depth; ++d) {
          GuidedNode<G>& nd = tree[rec.path[d] >> 8];
          nd.v[rec.path[d] & 255] += 1;
          nd.w0[rec.path[d] & 255] += val0;
        }
        if (calls >= simulations || rec.count >= capacity) {  // the last call, or the root's memory is used up
          rec.status = kGuidedIdle;
        } else {
          int node = 0, depth = 0;
          bool broken = false;
          s = tree[0].s;
          for (;;) {
            GuidedNode<G>& nd = tree[node];
            int total = 0;  // the wave sum of the lanes' own visits
            for (int lane = 0; lane < L; ++lane) {
              for (int j = 0; j < SL; ++j) {
                if (lane + L * j < A) total += nd.v[lane + L * j];
              }
            }
            const int sign = SearchSign<G>(s);
            SearchPick best = SearchNone();
            for (int lane = L - 1; lane >= 0; --lane) {  // (any order: SearchBetter is associative and commutative)
              SearchPick mine = SearchNone();
              for (int j = 0; j < SL; ++j) {
                const int a = lane + L * j;
                if (a < A && Has(s.m, a)) {
                  mine = SearchBetter(mine,
                                      SearchPick{GuidedScore(nd.v[a], nd.w0[a], nd.p[a], total, sign, c_puct), a, 1});
                }
              }
              best = SearchBetter(best, mine);
            }
            const int a = best.action;
            if (a < 0 || depth >= kSearchMaxPath) {
              broken = true;
              break;
            }
            rec.path[depth++] = node << 8 | a;
            if (nd.child[a] < 0) {
              const int c = rec.count++;
              GuidedNode<G>& nn = tree[c];
              nn.term0 = SearchExpand<G>(s, a, nn.s);
              ClearNode(nn);
              nd.child[a] = c;
              node = c;
              s = nn.s;
              break;
            }
            node = nd.child[a];
            s = tree[node].s;
            if (s.done) break;
          }
          rec.pending = node;
          rec.status = broken ? kGuidedIdle : s.done ? kGuidedTerminal : kGuidedEvaluate;
          rec.depth = broken ? 0 : depth;
          if (broken) {
            rec.broken = 1;
            rc = -3;
          }
        }
      }
      Emit(i, s, obs, mask, status);
    }
    ++calls;
    return rc;
  }

  void Result(int32_t* visits, float* values, int32_t* action, int32_t* nodes_used) const override {
    for (int i = 0; i < n; ++i) {
      const GuidedNode<G>& n0 = Tree(i)[0];
      const bool over = roots[(size_t)i].over != 0;
      const float sign = (float)SearchSign<G>(n0.s);
      SearchPick best = SearchNone();
      for (int a = 0; a < A; ++a) {
        const int v = over ? 0 : n0.v[a];
        visits[(size_t)i * A + a] = v;
        values[(size_t)i * A + a] = over ? 0.0f : sign * n0.w0[a];
        if (!over && Has(n0.s.m, a)) best = SearchBetter(best, SearchPick{(float)v, a, 1});
      }
      action[i] = best.action;
      nodes_used[i] = roots[(size_t)i].count;
    }
  }

  // PgxGuidedReroot, one root after the other.  -5: the round is not complete; -6: S2 outside 1 .. 4096 or above
  // capacity - 1.  (An action out of range ends its root, as the kernel does; the engine's host form refuses it.)
  int Reroot(const int32_t* actions, int s2, uint8_t* obs, uint8_t* mask, uint8_t* status) override {
    if (calls != simulations + 1) return -5;
    if (s2 < 1 || s2 > kSearchMaxSimulations || s2 + 1 > capacity) return -6;
    for (int i = 0; i < n; ++i) {
      GuidedRoot& rec = roots[(size_t)i];
      GuidedNode<G>* tree = Tree(i);
      const int act = actions[i];
      const int old_count = rec.count;
      bool over = rec.over != 0 || rec.broken != 0 || act < 0 || act >= A;
      int count = old_count;
      State s = tree[0].s;
      if (!over) {
        const int c = tree[0].child[act];
        if (c < 0) {
          State s2s;
          const int term0 = SearchExpand<G>(s, act, s2s);
          tree[0].s = s2s;
          tree[0].term0 = term0;
          ClearNode(tree[0]);
          s = s2s;
          count = 1;
        } else {
          s = tree[c].s;
          int32_t* t = table.data();
          for (int k = 0; k < old_count; ++k) t[k] = k == c ? 1 : 0;
          for (int k = c; k < old_count; ++k) {  // mark: the nodes in index order
            if (t[k] == 0) continue;
            for (int lane = 0; lane < L; ++lane) {
              for (int j = 0; j < SL; ++j) {
                if (lane + L * j < A) GuidedRerootReach(t, tree[k].child[lane + L * j]);
              }
            }
          }
          int kept = 0;
          for (int base = 0; base < old_count; base += L) {  // rank: a trip of 64 nodes, an inclusive scan, the carry
            int upto[L], m[L];
            for (int lane = 0; lane < L; ++lane) {
              m[lane] = base + lane < old_count && t[base + lane] != 0 ? 1 : 0;
              upto[lane] = m[lane] + (lane > 0 ? upto[lane - 1] : 0);
            }
            for (int lane = 0; lane < L; ++lane) {
              if (base + lane < old_count) {
                t[base + lane] = GuidedRerootRank(kept + upto[lane] - m[lane], m[lane] != 0);
              }
            }
            kept += upto[L - 1];
          }
          for (int k = c; k < old_count; ++k) {  // copy, in place
            const int dst = t[k];
            if (dst < 0 || dst == k) continue;
            const GuidedNode<G>& from = tree[k];
            GuidedNode<G>& to = tree[dst];
            to.s = from.s;  // lane 0
            to.term0 = from.term0;
            for (int lane = 0; lane < L; ++lane) {
              for (int j = 0; j < SL; ++j) {
                const int e = lane + L * j;
                if (e < A) {
                  to.child[e] = GuidedRerootEdge(t, from.child[e]);
                  to.v[e] = from.v[e];
                  to.w0[e] = from.w0[e];
                  to.p[e] = from.p[e];
                }
              }
            }
          }
          count = kept;
        }
        over = s.done != 0;
      }
      GuidedRerootRoot(rec, count, over);
      Emit(i, s, obs, mask, status);
    }
    simulations = s2;
    calls = 0;
    return 0;
  }
};

template <int G>
Session* Make(int n, const int32_t* hidden, const uint8_t* done, int simulations, int nodes, float c_puct,
              uint8_t* obs, uint8_t* mask, uint8_t* status, int* rc) {
  if (simulations < 1 || simulations > kSearchMaxSimulations || nodes < simulations + 1 || nodes > kGuidedMaxNodes) {
    *rc = -6;
    return nullptr;
  }
  Run<G>* r = new Run<G>(n, simulations, nodes, c_puct);
  *rc = r->Begin(hidden, done, obs, mask, status);
  if (*rc != 0) {
    delete r;
    return nullptr;
  }
  return r;
}
}  // namespace

extern "C" {

// A session of n roots (hidden[i]: HiddenWords words, done[i]) with `nodes` nodes per root; writes the emitted leaves
// and *rc (-1: no such game; -2: words that are no position; -6: simulations or nodes out of range) and returns the
// session, or null.
void* pgx_reroot_begin(int game, int n, const int32_t* hidden, const uint8_t* done, int simulations, int nodes,
                       float c_puct, uint8_t* obs, uint8_t* mask, uint8_t* status, int* rc) {
  switch (game) {
    case kTicTacToe: return Make<kTicTacToe>(n, hidden, done, simulations, nodes, c_puct, obs, mask, status, rc);
    case kConnectFour: return Make<kConnectFour>(n, hidden, done, simulations, nodes, c_puct, obs, mask, status, rc);
    case kHex: return Make<kHex>(n, hidden, done, simulations, nodes, c_puct, obs, mask, status, rc);
    case kOthello: return Make<kOthello>(n, hidden, done, simulations, nodes, c_puct, obs, mask, status, rc);
    default: *rc = -1; return nullptr;
  }
}

// One advance: 0, -3 (a broken invariant: that root ended with status 2) or -4 (a call number above S).
int pgx_reroot_advance(void* session, const float* priors, const float* values, uint8_t* obs, uint8_t* mask,
                       uint8_t* status) {
  return static_cast<Session*>(session)->Advance(priors, values, obs, mask, status);
}

void pgx_reroot_result(void* session, int32_t* visits, float* values, int32_t* action, int32_t* nodes_used) {
  static_cast<Session*>(session)->Result(visits, values, action, nodes_used);
}

// reroot by actions[n], the next round of s2 simulations: 0, -5 (the round is not complete) or -6 (s2 out of range)
int pgx_reroot_reroot(void* session, const int32_t* actions, int s2, uint8_t* obs, uint8_t* mask, uint8_t* status) {
  return static_cast<Session*>(session)->Reroot(actions, s2, obs, mask, status);
}

void pgx_reroot_end(void* session) { delete static_cast<Session*>(session); }

}  // extern "C"

#ifdef PGX_REROOT_MAIN
// Three moves of Hex from the empty board, S = 24 and nodes = 2 S + 1, rerooted by the most visited move after each
// round; the evaluator is an integer hash of the leaf's bytes.  Prints the moves and the nodes kept.
namespace {
struct Zero {
  uint32_t Next() { return 0u; }
};
}  // namespace

int main() {
  constexpr int G = kHex, A = Dims<G>::A, OB = GuidedObsElems<G>(), S = 24, C = 2 * S + 1, N = 2;
  Zero gen;
  State root{};
  Reset<G>(gen, root);
  std::vector<int32_t> hidden((size_t)N * HiddenWords<G>());
  for (int i = 0; i < N; ++i) Hidden<G>(root, hidden.data() + (size_t)i * HiddenWords<G>());
  std::vector<uint8_t> done(N, 0), obs((size_t)N * OB), mask((size_t)N * A), status(N);
  int rc = -9;
  void* h = pgx_reroot_begin(G, N, hidden.data(), done.data(), S, C, 1.25f, obs.data(), mask.data(), status.data(), &rc);
  if (h == nullptr || rc != 0) return 1;
  std::vector<float> priors((size_t)N * A), values(N);
  std::vector<int32_t> visits((size_t)N * A), action(N), used(N);
  std::vector<float> vals((size_t)N * A);
  for (int move = 0; move < 3; ++move) {
    for (int t = 0; t <= S; ++t) {
      for (int i = 0; i < N; ++i) {
        uint32_t x = 2166136261u;
        for (int e = 0; e < OB; ++e) x = (x ^ obs[(size_t)i * OB + e]) * 16777619u;
        int legal = 0;
        for (int a = 0; a < A; ++a) legal += mask[(size_t)i * A + a];
        for (int a = 0; a < A; ++a) {
          const uint32_t y = (x ^ (uint32_t)(a + 1) * 2654435761u) * 2246822519u;
          priors[(size_t)i * A + a] = mask[(size_t)i * A + a] ? (float)((y >> 12) + 1) / (1048576.0f * (float)legal) : 0.0f;
        }
        values[i] = (float)(x >> 8) / 8388608.0f - 1.0f;
      }
      if (pgx_reroot_advance(h, priors.data(), values.data(), obs.data(), mask.data(), status.data()) != 0) return 2;
    }
    pgx_reroot_result(h, visits.data(), vals.data(), action.data(), used.data());
    if (move == 1) action[1] = 121 - action[1] % 2;  // row 1: a second-slot action, most likely untried
    std::printf("move %d: actions %d %d, nodes %d %d\n", move, action[0], action[1], used[0], used[1]);
    if (pgx_reroot_reroot(h, action.data(), S, obs.data(), mask.data(), status.data()) != 0) return 3;
    pgx_reroot_result(h, visits.data(), vals.data(), action.data(), used.data());
    std::printf("        kept nodes %d %d\n", used[0], used[1]);
  }
  pgx_reroot_end(h);
  return 0;
}
#endif
