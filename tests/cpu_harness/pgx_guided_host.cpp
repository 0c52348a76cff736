// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_guided.hip.h, built with g++ by
// tests/test_pgx_guided_host.py.  It offers the stepwise begin / advance / result interface of the guided search on
// host memory and runs it the way the kernels' wave does -- lane j owns actions j and j + 64, priors are stored,
// scores and reductions go lane by lane -- with the wave's lanes walked as loops.  Positions come in as the hidden
// words of pgx_env.hip.h (SetHidden) plus the done flag.  Not linked by envpool_amd/.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../envpool_amd/csrc/pgx_guided.hip.h"

using namespace epa::pgx;

namespace {
struct Session {
  virtual ~Session() {}
  virtual int Advance(const float* priors, const float* values, uint8_t* obs, uint8_t* mask, uint8_t* status) = 0;
  virtual void Result(int32_t* visits, float* values, int32_t* action, int32_t* nodes_used) const = 0;
};

template <int G>
struct Run : Session {
  static constexpr int A = Dims<G>::A, L = kSearchWave, SL = SearchSlotsPerLane<G>(), OB = GuidedObsElems<G>();
  int n, simulations, calls{0};
  float c_puct;
  std::vector<GuidedRoot> roots;
  std::vector<GuidedNode<G>> nodes;  // [n][simulations + 1]

  Run(int n_, int s, float c) : n(n_), simulations(s), c_puct(c), roots((size_t)n_), nodes((size_t)n_ * (s + 1)) {}
  GuidedNode<G>* Tree(int i) { return nodes.data() + (size_t)i * (simulations + 1); }
  const GuidedNode<G>* Tree(int i) const { return nodes.data() + (size_t)i * (simulations + 1); }

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
        if (calls >= simulations) {
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
              if (rec.count > simulations) {
                broken = true;
                break;
              }
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
          if (broken) rc = -3;
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
};

template <int G>
Session* Make(int n, const int32_t* hidden, const uint8_t* done, int simulations, float c_puct, uint8_t* obs,
              uint8_t* mask, uint8_t* status, int* rc) {
  Run<G>* r = new Run<G>(n, simulations, c_puct);
  *rc = r->Begin(hidden, done, obs, mask, status);
  if (*rc != 0) {
    delete r;
    return nullptr;
  }
  return r;
}
}  // namespace

extern "C" {

// A session of n roots (hidden[i]: HiddenWords words, done[i]); writes the emitted leaves and *rc (-1: no such game;
// -2: words that are no position) and returns the session, or null.
void* pgx_guided_begin(int game, int n, const int32_t* hidden, const uint8_t* done, int simulations, float c_puct,
                       uint8_t* obs, uint8_t* mask, uint8_t* status, int* rc) {
  switch (game) {
    case kTicTacToe: return Make<kTicTacToe>(n, hidden, done, simulations, c_puct, obs, mask, status, rc);
    case kConnectFour: return Make<kConnectFour>(n, hidden, done, simulations, c_puct, obs, mask, status, rc);
    case kHex: return Make<kHex>(n, hidden, done, simulations, c_puct, obs, mask, status, rc);
    case kOthello: return Make<kOthello>(n, hidden, done, simulations, c_puct, obs, mask, status, rc);
    default: *rc = -1; return nullptr;
  }
}

// One advance: 0, -3 (a broken invariant: that root ended with status 2) or -4 (a call number above S).
int pgx_guided_advance(void* session, const float* priors, const float* values, uint8_t* obs, uint8_t* mask,
                       uint8_t* status) {
  return static_cast<Session*>(session)->Advance(priors, values, obs, mask, status);
}

void pgx_guided_result(void* session, int32_t* visits, float* values, int32_t* action, int32_t* nodes_used) {
  static_cast<Session*>(session)->Result(visits, values, action, nodes_used);
}

void pgx_guided_end(void* session) { delete static_cast<Session*>(session); }

int pgx_guided_node_bytes(int game) {
  switch (game) {
    case kTicTacToe: return (int)sizeof(GuidedNode<kTicTacToe>);
    case kConnectFour: return (int)sizeof(GuidedNode<kConnectFour>);
    case kHex: return (int)sizeof(GuidedNode<kHex>);
    case kOthello: return (int)sizeof(GuidedNode<kOthello>);
    default: return -1;
  }
}

}  // extern "C"
