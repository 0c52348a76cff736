// TEST HARNESS (not product): host instantiation of the batch sessions of envpool_amd/csrc/pgx_gumbel.hip.h ("A level
// per launch"), built with g++ by tests/test_pgx_gumbel_batch_host.py.  It offers the stepwise begin / advance / result
// interface on host memory with B slots per root -- row i * B + j of the leaf and answer arrays is slot j of root i --
// and runs it the way the kernels' wave does: lane j owns actions j and j + 64, a float sum over actions is the lanes'
// partials (slot j + slot j + 64) through the butterfly of GumbelWaveSum, with the wave's lanes walked as loops.
// Positions come in as the hidden words of pgx_env.hip.h (SetHidden) plus the done flag.  Not linked by envpool_amd/.
//
// With -DPGX_GUMBEL_BATCH_MAIN the file is a program of its own: a few rounds of Hex and Othello, for a run under the
// host sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
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
  int n, simulations, considered, batch, calls{0};
  float c_visit, c_scale;
  std::vector<char> roots;           // [n] GumbelBatchRoot<G> with its slots
  std::vector<GumbelNode<G>> nodes;  // [n][simulations + 1]

  Run(int n_, int s, int m, int b, float cv, float cs)
      : n(n_), simulations(s), considered(m), batch(b), c_visit(cv), c_scale(cs),
        roots((size_t)n_ * GumbelBatchRootBytes<G>(b) + 16), nodes((size_t)n_ * (s + 1)) {}
  void* RootMem() const {  // (the vector's memory, aligned as the record asks)
    return reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(roots.data()) + 15) & ~(uintptr_t)15);
  }
  GumbelBatchRoot<G>& Root(int i) const { return GumbelBatchRootAt<G>(RootMem(), i, batch); }
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

  // the root's scores: legal count, and score[a] of every legal action
  int RootScores(int i, const Eval& e, float* score) const {
    const GumbelNode<G>& nd = Tree(i)[0];
    int legal = 0;
    float top = -FLT_MAX;
    for (int a = 0; a < A; ++a) {
      if (!Legal(nd.s, a)) continue;
      ++legal;
      top = std::max(top, nd.logit[a]);
    }
    for (int a = 0; a < A; ++a) {
      score[a] = Legal(nd.s, a) ? GumbelRootScore(Root(i).gumbel[a], nd.logit[a], top, e.sigma[a]) : 0.0f;
    }
    return legal;
  }
  // the best action among those with cand[a] (ties: the lowest a); -1 without one
  static int Best(const float* score, const bool* cand) {
    SearchPick best = SearchNone();
    for (int a = A - 1; a >= 0; --a) {  // (any order: SearchBetter is associative and commutative)
      if (cand[a]) best = SearchBetter(best, SearchPick{score[a], a, 1});
    }
    return best.action;
  }

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
      GumbelBatchClearRoot(Root(i), batch, done[i] != 0);
      for (int a = 0; a < A; ++a) Root(i).gumbel[a] = GumbelCleanNoise(gumbel[(size_t)i * A + a]);
      Emit(i * batch, done[i] ? kGuidedIdle : kGuidedEvaluate, root, obs, mask, status);
      for (int j = 1; j < batch; ++j) Emit(i * batch + j, kGuidedIdle, State{}, obs, mask, status);
    }
    return 0;
  }

  // phase A for one slot: the leaf's logits, p and raw (status 0) and the backup along the slot's path
  void Answer(int i, int j, const float* logits, const float* values) {
    GumbelNode<G>* tree = Tree(i);
    GuidedWideSlot& sl = GumbelBatchSlots(Root(i))[j];
    GumbelNode<G>& leaf = tree[sl.pending];
    const size_t row = (size_t)i * batch + j;
    float val0;
    if (sl.status == kGuidedEvaluate) {
      const State& ls = leaf.s;
      float top = -FLT_MAX;
      for (int a = 0; a < A; ++a) {
        leaf.logit[a] = Legal(ls, a) ? GumbelCleanLogit(logits[row * A + a]) : 0.0f;
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
      val0 = (float)SearchSign<G>(ls) * GuidedCleanV(values[row]);
      leaf.raw = val0;
    } else {
      val0 = (float)leaf.term0;
    }
    for (int d = 0; d < sl.depth; ++d) {
      GumbelNode<G>& nd = tree[sl.path[d] >> 8];
      nd.v[sl.path[d] & 255] += 1;
      nd.w0[sl.path[d] & 255] += val0;
    }
    sl.status = kGuidedIdle;
    sl.depth = 0;
  }

  // one descent through root action `a` into slot `sl`: false for a broken position
  bool Descend(int i, int a, GuidedWideSlot& sl, State& s) {
    GumbelBatchRoot<G>& rec = Root(i);
    GumbelNode<G>* tree = Tree(i);
    int node = 0, depth = 0;
    s = tree[0].s;
    for (;;) {
      GumbelNode<G>& nd = tree[node];
      sl.path[depth++] = node << 8 | a;
      if (nd.child[a] < 0) {
        if (rec.count > simulations) return false;
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
      const GumbelNode<G>& in = tree[node];
      const Eval e = Evaluate(in);
      SearchPick best = SearchNone();
      for (int lane = L - 1; lane >= 0; --lane) {
        for (int q = 0; q < SL; ++q) {
          const int b = lane + L * q;
          if (Legal(s, b)) best = SearchBetter(best, SearchPick{GumbelInteriorScore(e.pi[b], in.v[b], e.total), b, 1});
        }
      }
      a = best.action;
      if (a < 0 || depth >= kSearchMaxPath) return false;
    }
    sl.pending = node;
    sl.status = s.done ? kGuidedTerminal : kGuidedEvaluate;
    sl.depth = depth;
    return true;
  }

  int Advance(const float* logits, const float* values, uint8_t* obs, uint8_t* mask, uint8_t* status) override {
    if (calls > simulations) return -4;
    int rc = 0;
    for (int i = 0; i < n; ++i) {
      GumbelBatchRoot<G>& rec = Root(i);
      GuidedWideSlot* slots = GumbelBatchSlots(rec);
      for (int j = 0; j < batch; ++j) {
        if (slots[j].status != kGuidedIdle) Answer(i, j, logits, values);
      }
      int j = 0;
      bool broken = false;
      if (rec.over == 0 && rec.broken == 0) {
        const GumbelNode<G>& n0 = Tree(i)[0];
        const Eval e = Evaluate(n0);
        if (e.total < simulations) {
          float score[A];
          bool cand[A];
          const int m_eff = std::min(considered, RootScores(i, e, score));
          const int cv = GumbelConsideredVisit(m_eff, simulations, e.total);
          const int b = std::min(batch, GumbelLevelLeft(m_eff, simulations, e.total));
          for (int a = 0; a < A; ++a) cand[a] = Legal(n0.s, a) && n0.v[a] == cv;
          for (; j < b; ++j) {
            const int a = Best(score, cand);
            if (a < 0) {
              broken = j == 0;
              break;
            }
            cand[a] = false;
            State s{};
            if (!Descend(i, a, slots[j], s)) {
              broken = true;
              break;
            }
            Emit(i * batch + j, slots[j].status, s, obs, mask, status);
          }
        }
      }
      if (broken) {
        j = 0;
        rec.broken = 1;
        rc = -3;
      }
      for (int q = j; q < batch; ++q) {
        slots[q].status = kGuidedIdle;
        slots[q].depth = 0;
        Emit(i * batch + q, kGuidedIdle, State{}, obs, mask, status);
      }
      rec.live = j;
    }
    ++calls;
    return rc;
  }

  void Result(int32_t* visits, float* values, int32_t* action, float* weights, int32_t* nodes_used) const override {
    for (int i = 0; i < n; ++i) {
      const GumbelNode<G>& n0 = Tree(i)[0];
      const bool over = Root(i).over != 0;
      const float sign = (float)SearchSign<G>(n0.s);
      const Eval e = Evaluate(n0);
      for (int a = 0; a < A; ++a) {
        visits[(size_t)i * A + a] = over ? 0 : n0.v[a];
        values[(size_t)i * A + a] = over ? 0.0f : sign * n0.w0[a];
        weights[(size_t)i * A + a] = over ? 0.0f : e.pi[a];
      }
      float score[A];
      bool cand[A];
      RootScores(i, e, score);
      for (int a = 0; a < A; ++a) cand[a] = Legal(n0.s, a) && n0.v[a] == e.vmax;
      action[i] = over ? -1 : Best(score, cand);
      nodes_used[i] = Root(i).count;
    }
  }
};

template <int G>
Session* Make(int n, const int32_t* hidden, const uint8_t* done, int simulations, int considered, int batch,
              float c_visit, float c_scale, const float* gumbel, uint8_t* obs, uint8_t* mask, uint8_t* status,
              int* rc) {
  Run<G>* r = new Run<G>(n, simulations, considered, batch, c_visit, c_scale);
  *rc = r->Begin(hidden, done, gumbel, obs, mask, status);
  if (*rc != 0) {
    delete r;
    return nullptr;
  }
  return r;
}
}  // namespace

extern "C" {

// A session of n roots with `batch` slots each (hidden[i]: HiddenWords words, done[i], gumbel[i]: A floats); writes the
// n * batch emitted rows and *rc (-1: no such game; -2: words that are no position; -5: a batch outside 1 ..
// kGumbelMaxBatch) and returns the session, or null.
void* pgx_gumbel_batch_begin(int game, int n, const int32_t* hidden, const uint8_t* done, int simulations,
                             int considered, int batch, float c_visit, float c_scale, const float* gumbel,
                             uint8_t* obs, uint8_t* mask, uint8_t* status, int* rc) {
  if (batch < 1 || batch > kGumbelMaxBatch) {
    *rc = -5;
    return nullptr;
  }
#define EPA_MAKE(G) \
  Make<G>(n, hidden, done, simulations, considered, batch, c_visit, c_scale, gumbel, obs, mask, status, rc)
  switch (game) {
    case kTicTacToe: return EPA_MAKE(kTicTacToe);
    case kConnectFour: return EPA_MAKE(kConnectFour);
    case kHex: return EPA_MAKE(kHex);
    case kOthello: return EPA_MAKE(kOthello);
    default: *rc = -1; return nullptr;
  }
#undef EPA_MAKE
}

// One advance over n * batch rows: 0, -3 (a broken invariant: that root ended with every status 2) or -4 (a call number
// above S).
int pgx_gumbel_batch_advance(void* session, const float* logits, const float* values, uint8_t* obs, uint8_t* mask,
                             uint8_t* status) {
  return static_cast<Session*>(session)->Advance(logits, values, obs, mask, status);
}

void pgx_gumbel_batch_result(void* session, int32_t* visits, float* values, int32_t* action, float* weights,
                             int32_t* nodes_used) {
  static_cast<Session*>(session)->Result(visits, values, action, weights, nodes_used);
}

void pgx_gumbel_batch_end(void* session) { delete static_cast<Session*>(session); }

// bytes of a root's record with its slots
int pgx_gumbel_batch_root_bytes(int game, int batch) {
  switch (game) {
    case kTicTacToe: return (int)GumbelBatchRootBytes<kTicTacToe>(batch);
    case kConnectFour: return (int)GumbelBatchRootBytes<kConnectFour>(batch);
    case kHex: return (int)GumbelBatchRootBytes<kHex>(batch);
    case kOthello: return (int)GumbelBatchRootBytes<kOthello>(batch);
    default: return -1;
  }
}

// the header's walks of the table of considered visits
int pgx_gumbel_batch_considered_visit(int m, int simulations, int t) { return GumbelConsideredVisit(m, simulations, t); }
int pgx_gumbel_batch_level_left(int m, int simulations, int t) { return GumbelLevelLeft(m, simulations, t); }

}  // extern "C"

#ifdef PGX_GUMBEL_BATCH_MAIN
// Three rounds each of Hex (B = 32, m = A, S = 64) and Othello (B = 4, m = 16, S = 32) from the start of the game, two
// roots, the evaluator an integer hash of the leaf's bytes.  Prints the advances a round took and the moves.
namespace {
struct Zero {
  uint32_t Next() { return 0u; }
};

template <int G>
int Rounds(int S, int m, int B) {
  constexpr int A = Dims<G>::A, OB = GuidedObsElems<G>(), N = 2;
  Zero gen;
  State root{};
  Reset<G>(gen, root);
  for (int round = 0; round < 3; ++round) {
    std::vector<int32_t> hidden((size_t)N * HiddenWords<G>());
    for (int i = 0; i < N; ++i) Hidden<G>(root, hidden.data() + (size_t)i * HiddenWords<G>());
    const int rows = N * B;
    std::vector<uint8_t> done(N, 0), obs((size_t)rows * OB), mask((size_t)rows * A), status(rows);
    std::vector<float> gumbel((size_t)N * A);
    for (size_t q = 0; q < gumbel.size(); ++q) gumbel[q] = (float)((q * 2654435761u >> 20) & 1023u) / 256.0f - 2.0f;
    int rc = -9;
    void* h = pgx_gumbel_batch_begin(G, N, hidden.data(), done.data(), S, m, B, 50.0f, 0.1f, gumbel.data(), obs.data(),
                                     mask.data(), status.data(), &rc);
    if (h == nullptr || rc != 0) return 1;
    std::vector<float> logits((size_t)rows * A), values(rows);
    int advances = 0;
    for (;;) {
      bool pending = false;
      for (int r = 0; r < rows; ++r) pending = pending || status[r] != kGuidedIdle;
      if (!pending) break;
      for (int r = 0; r < rows; ++r) {
        uint32_t x = 2166136261u;
        for (int e = 0; e < OB; ++e) x = (x ^ obs[(size_t)r * OB + e]) * 16777619u;
        for (int a = 0; a < A; ++a) {
          const uint32_t y = (x ^ (uint32_t)(a + 1) * 2654435761u) * 2246822519u;
          logits[(size_t)r * A + a] = mask[(size_t)r * A + a] ? (float)(y >> 12) / 174762.0f - 3.0f : 0.0f;
        }
        values[r] = (float)(x >> 8) / 8388608.0f - 1.0f;
      }
      if (pgx_gumbel_batch_advance(h, logits.data(), values.data(), obs.data(), mask.data(), status.data()) != 0) {
        return 2;
      }
      ++advances;
    }
    std::vector<int32_t> visits((size_t)N * A), action(N), used(N);
    std::vector<float> vals((size_t)N * A), weights((size_t)N * A);
    pgx_gumbel_batch_result(h, visits.data(), vals.data(), action.data(), weights.data(), used.data());
    pgx_gumbel_batch_end(h);
    std::printf("game %d round %d: %d advances, actions %d %d, nodes %d %d\n", G, round, advances, action[0],
                action[1], used[0], used[1]);
    if (action[0] < 0) return 3;
    Step<G>(root, action[0]);
    if (root.done) break;
  }
  return 0;
}
}  // namespace

int main() {
  const int rc = Rounds<kHex>(64, Dims<kHex>::A, 32);
  return rc != 0 ? rc : Rounds<kOthello>(32, 16, 4);
}
#endif
