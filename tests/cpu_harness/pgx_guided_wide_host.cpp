// TEST HARNESS (not product): host instantiation of the wide sessions of envpool_amd/csrc/pgx_guided.hip.h ("Several
// leaves per launch"), built with g++ by tests/test_pgx_guided_wide_host.py.  It offers begin / advance / result /
// reroot of a session whose roots have W slots, on host memory, and runs them the way the kernels' wave does -- lane j
// owns actions j and j + 64, lane i holds depth and pending leaf of slot i of the launch, the virtual losses come from
// the earlier slots' paths, scores and reductions go lane by lane -- with the wave's lanes walked as loops.  Positions
// come in as the hidden words of pgx_env.hip.h (SetHidden) plus the done flag.  Not linked by envpool_amd/.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../envpool_amd/csrc/pgx_guided.hip.h"

using namespace epa::pgx;

namespace {
struct Session {
  virtual ~Session() {}
  virtual int Advance(const float* priors, const float* values, uint8_t* obs, uint8_t* mask, uint8_t* status) = 0;
  virtual void Result(int32_t* visits, float* values, int32_t* action, int32_t* nodes_used, int32_t* done) = 0;
  virtual int Reroot(const int32_t* actions, int s2, uint8_t* obs, uint8_t* mask, uint8_t* status) = 0;
};

template <int G>
struct Run : Session {
  static constexpr int A = Dims<G>::A, L = kSearchWave, SL = SearchSlotsPerLane<G>(), OB = GuidedObsElems<G>();
  int n, simulations, capacity, width, calls{0};
  float c_puct;
  std::vector<char> roots;           // [n] GuidedWideRoot and its W slots
  std::vector<GuidedNode<G>> nodes;  // [n][capacity]
  std::vector<int32_t> lpath;        // [kSearchMaxPath][W]: the launch's paths, as the kernel's LDS
  std::vector<int32_t> table;

  Run(int n_, int s, int cap, int w, float c)
      : n(n_), simulations(s), capacity(cap), width(w), c_puct(c), roots((size_t)n_ * GuidedWideRootBytes(w)),
        nodes((size_t)n_ * cap), lpath((size_t)kSearchMaxPath * w), table((size_t)cap) {}
  GuidedNode<G>* Tree(int i) { return nodes.data() + (size_t)i * capacity; }
  GuidedWideRoot& Rec(int i) { return GuidedWideRootAt(roots.data(), i, width); }

  static void ClearNode(GuidedNode<G>& nd) {
    for (int lane = 0; lane < L; ++lane) {
      for (int j = 0; j < SL; ++j) {
        if (lane + L * j < A) GuidedClearEdge<G>(nd, lane + L * j);
      }
    }
  }

  // row `row` of the leaf arrays
  void Emit(int row, int st, const State& s, uint8_t* obs, uint8_t* mask, uint8_t* status) const {
    View view{};
    view.s = s;
    const int mover = SearchMover<G>(s);
    for (int e = 0; e < OB; ++e) {
      obs[(size_t)row * OB + e] = st == kGuidedEvaluate ? (uint8_t)GuidedObsElem<G>(view, mover, e) : 0;
    }
    for (int e = 0; e < A; ++e) {
      mask[(size_t)row * A + e] = st == kGuidedEvaluate ? (uint8_t)GuidedMaskElem<G>(view, e) : 0;
    }
    status[row] = (uint8_t)st;
  }

  int Begin(const int32_t* hidden, const uint8_t* done, uint8_t* obs, uint8_t* mask, uint8_t* status) {
    constexpr int HW = HiddenWords<G>();
    for (int i = 0; i < n; ++i) {
      State root{};
      if (!SetHidden<G>(root, hidden + (size_t)i * HW)) return -2;
      root.done = done[i] ? 1 : 0;
      GuidedNode<G>& n0 = Tree(i)[0];
      n0.s = root;
      n0.term0 = 0;
      ClearNode(n0);
      GuidedWideClearRoot(Rec(i), width, 1, done[i] != 0);
      Emit(i * width, done[i] ? kGuidedIdle : kGuidedEvaluate, root, obs, mask, status);
      for (int j = 1; j < width; ++j) Emit(i * width + j, kGuidedIdle, root, obs, mask, status);
    }
    return 0;
  }

  int Advance(const float* priors, const float* values, uint8_t* obs, uint8_t* mask, uint8_t* status) override {
    if (calls > simulations) return -4;
    const int W = width;
    int rc = 0;
    for (int i = 0; i < n; ++i) {
      GuidedWideRoot& rec = Rec(i);
      GuidedWideSlot* slots = GuidedWideSlots(rec);
      GuidedNode<G>* tree = Tree(i);
      int done = rec.done;
      // A. the answers
      for (int j = 0; j < W; ++j) {
        if (slots[j].status == kGuidedIdle) continue;
        GuidedNode<G>& leaf = tree[slots[j].pending];
        const size_t lrow = (size_t)i * W + j;
        float val0;
        if (slots[j].status == kGuidedEvaluate) {
          for (int lane = 0; lane < L; ++lane) {
            for (int q = 0; q < SL; ++q) {
              const int a = lane + L * q;
              if (a < A) leaf.p[a] = GuidedClean(priors[lrow * A + a]);
            }
          }
          val0 = (float)SearchSign<G>(leaf.s) * GuidedCleanV(values[lrow]);
        } else {
          val0 = (float)leaf.term0;
        }
        for (int d = 0; d < slots[j].depth; ++d) {
          GuidedNode<G>& nd = tree[slots[j].path[d] >> 8];
          nd.v[slots[j].path[d] & 255] += 1;
          nd.w0[slots[j].path[d] & 255] += val0;
        }
        if (slots[j].depth > 0) ++done;
      }
      // B. the descents
      int count = rec.count;
      const bool idle = rec.over != 0 || rec.broken != 0;
      int my_depth[L], my_pend[L];  // lane i: slot i of this launch
      for (int lane = 0; lane < L; ++lane) {
        my_depth[lane] = 0;
        my_pend[lane] = -1;
      }
      int j = 0;
      bool broken = false;
      const State root = tree[0].s;
      for (; j < W && !idle; ++j) {
        if (!(done + j < simulations && count < capacity)) break;
        int node = 0, depth = 0;
        bool collided = false;
        State s = root;
        for (;;) {
          GuidedNode<G>& nd = tree[node];
          int o[L][SL], own = 0, osum = 0;
          for (int lane = 0; lane < L; ++lane) {
            for (int q = 0; q < SL; ++q) {
              o[lane][q] = 0;
              if (lane + L * q < A) own += nd.v[lane + L * q];
            }
          }
          for (int i2 = 0; i2 < j && i2 < L; ++i2) {  // the ballot of the lanes below j, then its set bits
            const int e = depth < my_depth[i2] ? lpath[(size_t)depth * W + i2] : -1;
            if (!GuidedWideOn(e, my_depth[i2], depth, node)) continue;
            ++osum;
            const int ai = e & 255;
            o[ai & (L - 1)][ai / L] += 1;  // the owner lane's
          }
          const int total = own + osum;
          const int sign = SearchSign<G>(s);
          SearchPick best = SearchNone();
          for (int lane = L - 1; lane >= 0; --lane) {  // (any order: SearchBetter is associative and commutative)
            SearchPick mine = SearchNone();
            for (int q = 0; q < SL; ++q) {
              const int a = lane + L * q;
              if (a < A && Has(s.m, a)) {
                mine = SearchBetter(mine, SearchPick{GuidedWideScore(nd.v[a], nd.w0[a], nd.p[a], o[lane][q], total,
                                                                     sign, c_puct),
                                                     a, 1});
              }
            }
            best = SearchBetter(best, mine);
          }
          const int a = best.action;
          if (a < 0 || depth >= kSearchMaxPath) {
            broken = true;
            break;
          }
          lpath[(size_t)depth * W + j] = node << 8 | a;
          slots[j].path[depth] = node << 8 | a;
          ++depth;
          if (nd.child[a] < 0) {
            const int c = count++;
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
          for (int i2 = 0; i2 < j; ++i2) collided = collided || my_pend[i2] == node;
          if (collided) break;
        }
        if (broken || collided) break;
        const int st = s.done ? kGuidedTerminal : kGuidedEvaluate;
        slots[j].pending = node;
        slots[j].status = st;
        slots[j].depth = depth;
        my_depth[j] = depth;
        my_pend[j] = st == kGuidedEvaluate ? node : -1;
        Emit(i * W + j, st, s, obs, mask, status);
      }
      if (broken) j = 0;
      for (int q = j; q < W; ++q) {
        slots[q].status = kGuidedIdle;
        slots[q].depth = 0;
        Emit(i * W + q, kGuidedIdle, root, obs, mask, status);
      }
      rec.count = count;
      rec.done = done;
      rec.live = j;
      if (broken) {
        rec.broken = 1;
        rc = -3;
      }
    }
    ++calls;
    return rc;
  }

  void Result(int32_t* visits, float* values, int32_t* action, int32_t* nodes_used, int32_t* done) override {
    for (int i = 0; i < n; ++i) {
      const GuidedNode<G>& n0 = Tree(i)[0];
      const bool over = Rec(i).over != 0;
      const float sign = (float)SearchSign<G>(n0.s);
      SearchPick best = SearchNone();
      for (int a = 0; a < A; ++a) {
        const int v = over ? 0 : n0.v[a];
        visits[(size_t)i * A + a] = v;
        values[(size_t)i * A + a] = over ? 0.0f : sign * n0.w0[a];
        if (!over && Has(n0.s.m, a)) best = SearchBetter(best, SearchPick{(float)v, a, 1});
      }
      action[i] = best.action;
      nodes_used[i] = Rec(i).count;
      done[i] = Rec(i).done;
    }
  }

  // PgxGuidedReroot<.., WIDE>, one root after the other.  -5: a slot is pending (what the engine's host form refuses;
  // `force` < 0 in s2 -- s2 = -S2 -- reroots all the same, as the device form does); -6: S2 out of range.
  int Reroot(const int32_t* actions, int s2, uint8_t* obs, uint8_t* mask, uint8_t* status) override {
    const bool force = s2 < 0;
    if (force) s2 = -s2;
    if (!force) {
      for (int i = 0; i < n; ++i) {
        if (Rec(i).live != 0) return -5;
      }
    }
    if (s2 < 1 || s2 > kSearchMaxSimulations || s2 + 1 > capacity) return -6;
    for (int i = 0; i < n; ++i) {
      GuidedWideRoot& rec = Rec(i);
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
          for (int k = c; k < old_count; ++k) {
            if (t[k] == 0) continue;
            for (int e = 0; e < A; ++e) GuidedRerootReach(t, tree[k].child[e]);
          }
          int kept = 0;
          for (int k = 0; k < old_count; ++k) {
            const bool m = t[k] != 0;
            t[k] = GuidedRerootRank(kept, m);
            kept += m ? 1 : 0;
          }
          for (int k = c; k < old_count; ++k) {
            const int dst = t[k];
            if (dst < 0 || dst == k) continue;
            const GuidedNode<G>& from = tree[k];
            GuidedNode<G>& to = tree[dst];
            to.s = from.s;
            to.term0 = from.term0;
            for (int e = 0; e < A; ++e) {
              to.child[e] = GuidedRerootEdge(t, from.child[e]);
              to.v[e] = from.v[e];
              to.w0[e] = from.w0[e];
              to.p[e] = from.p[e];
            }
          }
          count = kept;
        }
        over = s.done != 0;
      }
      GuidedWideClearRoot(rec, width, count, over);
      Emit(i * width, over ? kGuidedIdle : kGuidedEvaluate, s, obs, mask, status);
      for (int j = 1; j < width; ++j) Emit(i * width + j, kGuidedIdle, s, obs, mask, status);
    }
    simulations = s2;
    calls = 0;
    return 0;
  }
};

template <int G>
Session* Make(int n, const int32_t* hidden, const uint8_t* done, int simulations, int nodes, int width, float c_puct,
              uint8_t* obs, uint8_t* mask, uint8_t* status, int* rc) {
  if (simulations < 1 || simulations > kSearchMaxSimulations || nodes < simulations + 1 || nodes > kGuidedMaxNodes ||
      width < 1 || width > kGuidedMaxWidth) {
    *rc = -6;
    return nullptr;
  }
  Run<G>* r = new Run<G>(n, simulations, nodes, width, c_puct);
  *rc = r->Begin(hidden, done, obs, mask, status);
  if (*rc != 0) {
    delete r;
    return nullptr;
  }
  return r;
}
}  // namespace

extern "C" {

// A wide session of n roots (hidden[i]: HiddenWords words, done[i]) with `width` slots each; writes the n * width
// emitted leaf rows and *rc (-1: no such game; -2: words that are no position; -6: an argument out of range) and
// returns the session, or null.
void* pgx_wide_begin(int game, int n, const int32_t* hidden, const uint8_t* done, int simulations, int nodes, int width,
                     float c_puct, uint8_t* obs, uint8_t* mask, uint8_t* status, int* rc) {
  switch (game) {
    case kTicTacToe: return Make<kTicTacToe>(n, hidden, done, simulations, nodes, width, c_puct, obs, mask, status, rc);
    case kConnectFour:
      return Make<kConnectFour>(n, hidden, done, simulations, nodes, width, c_puct, obs, mask, status, rc);
    case kHex: return Make<kHex>(n, hidden, done, simulations, nodes, width, c_puct, obs, mask, status, rc);
    case kOthello: return Make<kOthello>(n, hidden, done, simulations, nodes, width, c_puct, obs, mask, status, rc);
    default: *rc = -1; return nullptr;
  }
}

// One advance over n * width rows: 0, -3 (a broken position: all slots of that root ended) or -4 (a call number above S).
int pgx_wide_advance(void* session, const float* priors, const float* values, uint8_t* obs, uint8_t* mask,
                     uint8_t* status) {
  return static_cast<Session*>(session)->Advance(priors, values, obs, mask, status);
}

void pgx_wide_result(void* session, int32_t* visits, float* values, int32_t* action, int32_t* nodes_used,
                     int32_t* done) {
  static_cast<Session*>(session)->Result(visits, values, action, nodes_used, done);
}

int pgx_wide_reroot(void* session, const int32_t* actions, int s2, uint8_t* obs, uint8_t* mask, uint8_t* status) {
  return static_cast<Session*>(session)->Reroot(actions, s2, obs, mask, status);
}

void pgx_wide_end(void* session) { delete static_cast<Session*>(session); }

int pgx_wide_root_bytes(int width) { return (int)GuidedWideRootBytes(width); }

}  // extern "C"
