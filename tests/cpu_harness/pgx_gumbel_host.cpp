// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_gumbel.hip.h, built with g++ by
// tests/test_pgx_gumbel_host.py.  It offers the stepwise begin / advance / result interface of the Gumbel search on
// host memory and runs it the way the kernels' wave does -- lane j owns actions j and j + 64, a float sum over actions
// is the lanes' partials (slot j + slot j + 64) through the butterfly of GumbelWaveSum -- with the wave's lanes walked
// as loops.  Positions come in as the hidden words of pgx_env.hip.h (SetHidden) plus the done flag.  Not linked by
// envpool_amd/.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../envpool_amd/csrc/pgx_gumbel.hip.h"

using namespace epa::pgx;

namespace {
struct Session {
  virtual ~Session() {}
  virtual int Advance(const float* logits, const float* values, uint8_t* obs, uint8_t* mask, uint8_t* status) = 0;
  virtual void Result(int32_t* visits, float* values, int32_t* action, float* weights, int32_t* nodes_used) const = 0;
};

template <int G>
struct Run : Session {
  static constexpr int A = Dims<G>::A, L = kSearchWave, SL = SearchSlotsPerLane<G>(), OB = GuidedObsElems<G>();
  int n, simulations, considered, calls{0};
  float c_visit, c_scale;
  std::vector<GumbelRoot<G>> roots;
  std::vector<GumbelNode<G>> nodes;  // [n][simulations + 1]

  Run(int n_, int s, int m, float cv, float cs)
      : n(n_), simulations(s), considered(m), c_visit(cv), c_scale(cs), roots((size_t)n_),
        nodes((size_t)n_ * (s + 1)) {}
  GumbelNode<G>* Tree(int i) { return nodes.data() + (size_t)i * (simulations + 1); }
  const GumbelNode<G>* Tree(int i) const { return nodes.data() + (size_t)i * (simulations + 1); }

  static void ClearNode(GumbelNode<G>& nd) {
    for (int lane = 0; lane < L; ++lane) {
      for (int j = 0; j < SL; ++j) {
        if (lane + L * j < A) GumbelClearEdge<G>(nd, lane + L * j);
      }
    }
  }
  static bool Legal(const State& s, int a) { return a < A && Has(s.m, a); }

  // the wave's SUM of term(a) over the actions that take part: lane partials, then the butterfly
  template <class F>
  static float Sum(F term) {
    float part[L];
    for (int lane = 0; lane < L; ++lane) {
      float t[2] = {0.0f, 0.0f};
      for (int j = 0; j < SL; ++j) term(lane + L * j, t[j]);
      part[lane] = t[0] + t[1];
    }
    return GumbelWaveSum(part);
  }

  // what the picks need of a node: N, vmax, sigma per action, pi' per action
  struct Eval {
    int total, vmax;
    float sigma[A], pi[A];
  };
  Eval Evaluate(const GumbelNode<G>& nd) const {
    Eval e{};
    const State& s = nd.s;
    const int sign = SearchSign<G>(s);
    for (int a = 0; a < A; ++a) {
      if (!Legal(s, a)) continue;
      e.total += nd.v[a];
      e.vmax = std::max(e.vmax, nd.v[a]);
    }
    const float sum_pq = Sum([&](int a, float& t) {
      if (Legal(s, a) && nd.v[a] > 0) t = nd.p[a] * GumbelQ(nd.v[a], nd.w0[a], sign);
    });
    const float sum_p = Sum([&](int a, float& t) {
      if (Legal(s, a) && nd.v[a] > 0) t = nd.p[a];
    });
    const float mix = GumbelMix(nd.raw, sign, e.total, sum_pq, sum_p);
    float cq[A] = {}, lo = FLT_MAX, hi = -FLT_MAX;
    for (int a = 0; a < A; ++a) {
      if (!Legal(s, a)) continue;
      cq[a] = nd.v[a] > 0 ? GumbelQ(nd.v[a], nd.w0[a], sign) : mix;
      lo = std::min(lo, cq[a]);
      hi = std::max(hi, cq[a]);
    }
    const float scale = GumbelScale(c_visit, c_scale, e.vmax);
    float top = -FLT_MAX;
    for (int a = 0; a < A; ++a) {
      if (!Legal(s, a)) continue;
      e.sigma[a] = GumbelSigma(scale, cq[a], lo, hi);
      top = std::max(top, nd.logit[a] + e.sigma[a]);
    }
    float ex[A] = {};
    for (int a = 0; a < A; ++a) {
      if (Legal(s, a)) ex[a] = GumbelExp((nd.logit[a] + e.sigma[a]) - top);
    }
    const float sum = Sum([&](int a, float& t) {
      if (Legal(s, a)) t = ex[a];
    });
    for (int a = 0; a < A; ++a) e.pi[a] = Legal(s, a) ? ex[a] / sum : 0.0f;
    return e;
  }

  int RootPick(int i, const Eval& e, bool final) const {
    const GumbelNode<G>& nd = Tree(i)[0];
    int legal = 0;
    float top = -FLT_MAX;
    for (int a = 0; a < A; ++a) {
      if (!Legal(nd.s, a)) continue;
      ++legal;
      top = std::max(top, nd.logit[a]);
    }
    const int cv = final ? e.vmax : GumbelConsideredVisit(std::min(considered, legal), simulations, e.total);
    SearchPick best = SearchNone();
    for (int a = A - 1; a >= 0; --a) {  // (any order: SearchBetter is associative and commutative)
      if (Legal(nd.s, a) && nd.v[a] == cv) {
        best = SearchBetter(
            best, SearchPick{GumbelRootScore(roots[(size_t)i].gumbel[a], nd.logit[a], top, e.sigma[a]), a, 1});
      }
    }
    return best.action;
  }

  void Emit(int i, const State& s, uint8_t* obs, uint8_t* mask, uint8_t* status) const {
    View view{};
    view.s = s;
    const int st = roots[(size_t)i].r.status, mover = SearchMover<G>(s);
    for (int e = 0; e < OB; ++e) {
      obs[(size_t)i * OB + e] = st == kGuidedEvaluate ? (uint8_t)GuidedObsElem<G>(view, mover, e) : 0;
    }
    for (int e = 0; e < A; ++e) mask[(size_t)i * A + e] = st == kGuidedEvaluate ? (uint8_t)GuidedMaskElem<G>(view, e) : 0;
    status[i] = (uint8_t)st;
  }

  int Begin(const int32_t* hidden, const uint8_t* done, const float* gumbel, uint8_t* obs, uint8_t* mask,
            uint8_t* status) {
    constexpr int W = HiddenWords<G>();
    for (int i = 0; i < n; ++i) {
      State root{};
      if (!SetHidden<G>(root, hidden + (size_t)i * W)) return -2;
      root.done = done[i] ? 1 : 0;
      GumbelNode<G>& n0 = Tree(i)[0];
      n0.s = root;
      n0.term0 = 0;
      n0.raw = 0.0f;
      ClearNode(n0);
      GuidedClearRoot(roots[(size_t)i].r, done[i] != 0);
      for (int a = 0; a < A; ++a) roots[(size_t)i].gumbel[a] = GumbelCleanNoise(gumbel[(size_t)i * A + a]);
      Emit(i, root, obs, mask, status);
    }
    return 0;
  }

  int Advance(const float* logits, const float* values, uint8_t* obs, uint8_t* mask, uint8_t* status) override {
    if (calls > simulations) return -4;
    int rc = 0;
    for (int i = 0; i < n; ++i) {
      GuidedRoot& rec = roots[(size_t)i].r;
      GumbelNode<G>* tree = Tree(i);
      State s{};
      if (rec.status != kGuidedIdle) {
        GumbelNode<G>& leaf = tree[rec.pending];
        float val0;
        if (rec.status == kGuidedEvaluate) {
          const State& ls = leaf.s;
          float top = -FLT_MAX;
          for (int a = 0; a < A; ++a) {
            leaf.logit[a] = Legal(ls, a) ? GumbelCleanLogit(logits[(size_t)i * A + a]) : 0.0f;
            if (Legal(ls, a)) top = std::max(top, leaf.logit[a]);
          }
          float ex[A] = {};
          for (int a = 0; a < A; ++a) {
            if (Legal(ls, a)) ex[a] = GumbelExp(leaf.logit[a] - top);
          }
          const float sum = Sum([&](int a, float& t) {
            if (Legal(ls, a)) t = ex[a];
          });
          for (int a = 0; a < A; ++a) leaf.p[a] = Legal(ls, a) ? GumbelPrior(ex[a], sum) : 0.0f;
          val0 = (float)SearchSign<G>(ls) * GuidedCleanV(values[i]);
          leaf.raw = val0;
        } else {
          val0 = (float)leaf.term0;
        }
        for (int d = 0; d < rec.depth; ++d) {
          GumbelNode<G>& nd = tree[rec.path[d] >> 8];
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
            GumbelNode<G>& nd = tree[node];
            const Eval e = Evaluate(nd);
            int a;
            if (node == 0) {
              a = RootPick(i, e, false);
            } else {
              SearchPick best = SearchNone();
              for (int lane = L - 1; lane >= 0; --lane) {
                for (int j = 0; j < SL; ++j) {
                  const int b = lane + L * j;
                  if (Legal(s, b)) {
                    best = SearchBetter(best, SearchPick{GumbelInteriorScore(e.pi[b], nd.v[b], e.total), b, 1});
                  }
                }
              }
              a = best.action;
            }
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
              GumbelNode<G>& nn = tree[c];
              nn.term0 = SearchExpand<G>(s, a, nn.s);
              nn.raw = GumbelFreshRaw(nn.s, nn.term0);
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

  void Result(int32_t* visits, float* values, int32_t* action, float* weights, int32_t* nodes_used) const override {
    for (int i = 0; i < n; ++i) {
      const GumbelNode<G>& n0 = Tree(i)[0];
      const bool over = roots[(size_t)i].r.over != 0;
      const float sign = (float)SearchSign<G>(n0.s);
      const Eval e = Evaluate(n0);
      for (int a = 0; a < A; ++a) {
        visits[(size_t)i * A + a] = over ? 0 : n0.v[a];
        values[(size_t)i * A + a] = over ? 0.0f : sign * n0.w0[a];
        weights[(size_t)i * A + a] = over ? 0.0f : e.pi[a];
      }
      action[i] = over ? -1 : RootPick(i, e, true);
      nodes_used[i] = roots[(size_t)i].r.count;
    }
  }
};

template <int G>
Session* Make(int n, const int32_t* hidden, const uint8_t* done, int simulations, int considered, float c_visit,
              float c_scale, const float* gumbel, uint8_t* obs, uint8_t* mask, uint8_t* status, int* rc) {
  Run<G>* r = new Run<G>(n, simulations, considered, c_visit, c_scale);
  *rc = r->Begin(hidden, done, gumbel, obs, mask, status);
  if (*rc != 0) {
    delete r;
    return nullptr;
  }
  return r;
}
}  // namespace

extern "C" {

// A session of n roots (hidden[i]: HiddenWords words, done[i], gumbel[i]: A floats); writes the emitted leaves and *rc
// (-1: no such game; -2: words that are no position) and returns the session, or null.
void* pgx_gumbel_begin(int game, int n, const int32_t* hidden, const uint8_t* done, int simulations, int considered,
                       float c_visit, float c_scale, const float* gumbel, uint8_t* obs, uint8_t* mask, uint8_t* status,
                       int* rc) {
#define EPA_MAKE(G) Make<G>(n, hidden, done, simulations, considered, c_visit, c_scale, gumbel, obs, mask, status, rc)
  switch (game) {
    case kTicTacToe: return EPA_MAKE(kTicTacToe);
    case kConnectFour: return EPA_MAKE(kConnectFour);
    case kHex: return EPA_MAKE(kHex);
    case kOthello: return EPA_MAKE(kOthello);
    default: *rc = -1; return nullptr;
  }
#undef EPA_MAKE
}

// One advance: 0, -3 (a broken invariant: that root ended with status 2) or -4 (a call number above S).
int pgx_gumbel_advance(void* session, const float* logits, const float* values, uint8_t* obs, uint8_t* mask,
                       uint8_t* status) {
  return static_cast<Session*>(session)->Advance(logits, values, obs, mask, status);
}

void pgx_gumbel_result(void* session, int32_t* visits, float* values, int32_t* action, float* weights,
                       int32_t* nodes_used) {
  static_cast<Session*>(session)->Result(visits, values, action, weights, nodes_used);
}

void pgx_gumbel_end(void* session) { delete static_cast<Session*>(session); }

int pgx_gumbel_node_bytes(int game) {
  switch (game) {
    case kTicTacToe: return (int)sizeof(GumbelNode<kTicTacToe>);
    case kConnectFour: return (int)sizeof(GumbelNode<kConnectFour>);
    case kHex: return (int)sizeof(GumbelNode<kHex>);
    case kOthello: return (int)sizeof(GumbelNode<kOthello>);
    default: return -1;
  }
}

// the header's exponential and its walk of the table of considered visits
void pgx_gumbel_exp(const float* x, int n, float* out) {
  for (int i = 0; i < n; ++i) out[i] = GumbelExp(x[i]);
}
int pgx_gumbel_considered_visit(int m, int simulations, int t) { return GumbelConsideredVisit(m, simulations, t); }

}  // extern "C"
