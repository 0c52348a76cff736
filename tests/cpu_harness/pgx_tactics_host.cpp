// TEST HARNESS (not product): host instantiation of the exact leaf status of envpool_amd/csrc/pgx_guided.hip.h ("Exact
// leaf status"), built with g++ by tests/test_pgx_tactics_host.py.  The session is the wide harness's
// (pgx_guided_wide_host.cpp, included here: width 1 is the plain session, call for call) with the stage the kernels
// add: after an advance's descents every slot that rule 1 looks at has its leaf solved the way PgxSolveKernel's wave
// does -- the top tree level by level, the lanes in lockstep rounds, the combine between rounds, the lanes walked as
// loops -- and a decided leaf is marked as PgxGuidedTactics marks it; a reroot reopens a decided node that becomes the
// root.  It also offers one step of a position given by its hidden words (pgx_env.hip.h only), from which the tests'
// restatement takes its positions.  With -DPGX_TACTICS_MAIN it is a program: three rounds of one ConnectFour session.
// Not linked by envpool_amd/.
#include "pgx_guided_wide_host.cpp"

#include <memory>

#include "../../envpool_amd/csrc/pgx_solve.hip.h"

namespace {
struct Solved {
  int status, value;
  long long nodes;
};

// one root through the header's traversal (as tests/cpu_harness/pgx_solve_host.cpp walks it)
template <int G>
Solved SolveOne(const State& root, int depth, long long max_nodes, SolveTop& t, std::vector<SolveLane>& lanes,
                std::vector<SolveWord>& stack) {
  constexpr int L = kSolveWave;
  const int limit = SolveLimit(depth);
  const bool hard = depth == 0;
  SolveTopInit(t, root);
  SolveFlags flags{0, root.m == 0 ? 1 : 0};
  long long count = 1;
  bool gave_up = SolveGaveUp(count, max_nodes, flags);
  while (!gave_up) {  // the top tree
    SolveTopPlan(t);
    if (t.next_n == t.n) break;
    for (int lane = 0; lane < L; ++lane) {
      for (int c = t.hi + lane; c < t.next_n; c += L) SolveTopMake<G>(t, c, limit, hard, flags);
    }
    SolveTopAdvance(t);
    count = t.n;
    gave_up = SolveGaveUp(count, max_nodes, flags);
  }
  if (!gave_up) {
    SolveTopFrontier(t);
    for (int lane = 0; lane < L; ++lane) SolveLaneInit(lanes[(size_t)lane], lane);
    for (;;) {  // the rounds
      bool busy = false;
      for (int lane = 0; lane < L; ++lane) busy = busy || SolveLaneBusy(lanes[(size_t)lane], t);
      if (!busy) break;
      for (int lane = 0; lane < L; ++lane) {
        SolveLaneSlice<G>(lanes[(size_t)lane], t, stack.data(), lane, kSolveSlice, limit, hard);
      }
      count = t.n;
      for (int lane = 0; lane < L; ++lane) {
        count += lanes[(size_t)lane].visited;
        flags.overflow |= lanes[(size_t)lane].flags.overflow;
        flags.broken |= lanes[(size_t)lane].flags.broken;
      }
      gave_up = SolveGaveUp(count, max_nodes, flags);
      if (gave_up) break;
      SolveCombine(t);
    }
  }
  if (gave_up) return Solved{kSolveGivenUp, 0, count};
  SolveCombine(t);
  return Solved{kSolveSolved, t.val[0] == kSolveUnknown ? 0 : t.val[0], count};
}

struct TacticsSession {
  virtual ~TacticsSession() {}
  virtual void Decided(int32_t* decided, int64_t* nodes, uint8_t* given_up) const = 0;
};

template <int G>
struct TacticsRun : Run<G>, TacticsSession {
  using Base = Run<G>;
  int depth;
  long long max_nodes;
  std::vector<int32_t> decided;
  std::vector<int64_t> solved_nodes;
  std::vector<uint8_t> given_up;  // [n][W]: the slot's leaf of the last advance was given up (for the tests)
  std::unique_ptr<SolveTop> top;
  std::vector<SolveLane> lanes;
  std::vector<SolveWord> stack;

  TacticsRun(int n_, int s, int cap, int w, float c, int d, long long m)
      : Base(n_, s, cap, w, c), depth(d), max_nodes(m), decided((size_t)n_, 0), solved_nodes((size_t)n_, 0),
        given_up((size_t)n_ * w, 0), top(new SolveTop), lanes((size_t)kSolveWave),
        stack(SolveStackBytes(d > 0 ? d : 1) / sizeof(SolveWord)) {}

  // PgxGuidedTactics, one slot after the other
  int Advance(const float* priors, const float* values, uint8_t* obs, uint8_t* mask, uint8_t* status) override {
    const int rc = Base::Advance(priors, values, obs, mask, status);
    if (depth == 0 || rc == -4) return rc;
    const int W = this->width;
    for (int i = 0; i < this->n; ++i) {
      GuidedWideSlot* slots = GuidedWideSlots(this->Rec(i));
      for (int j = 0; j < W; ++j) {
        given_up[(size_t)i * W + j] = 0;
        if (!GuidedTacticsLooksAt(slots[j].status, slots[j].pending)) continue;
        GuidedNode<G>& leaf = this->Tree(i)[slots[j].pending];
        const State s = leaf.s;
        const Solved out = SolveOne<G>(s, depth, max_nodes, *top, lanes, stack);
        solved_nodes[(size_t)i] += out.nodes;
        given_up[(size_t)i * W + j] = out.status == kSolveGivenUp;
        if (!GuidedTacticsDecides(out.status, out.value)) continue;
        GuidedTacticsMark<G>(leaf, out.value);
        slots[j].status = kGuidedTerminal;
        ++decided[(size_t)i];
        this->Emit(i * W + j, kGuidedTerminal, s, obs, mask, status);
      }
    }
    return rc;
  }

  // PgxGuidedReroot with rule 5: the child that becomes the root is reopened (the kernel does it after the copy to
  // node 0; before the copy gives the same bytes, and a refused reroot changes nothing)
  int Reroot(const int32_t* actions, int s2, uint8_t* obs, uint8_t* mask, uint8_t* status) override {
    std::vector<int> reopened;
    for (int i = 0; i < this->n; ++i) {
      const GuidedWideRoot& rec = this->Rec(i);
      const int act = actions[i];
      if (rec.over != 0 || rec.broken != 0 || act < 0 || act >= Base::A) continue;
      const int c = this->Tree(i)[0].child[act];
      if (c >= 0 && GuidedTacticsReopen(this->Tree(i)[c].s)) reopened.push_back(i * this->capacity + c);
    }
    const int rc = Base::Reroot(actions, s2, obs, mask, status);
    if (rc != 0) {
      for (int at : reopened) this->nodes[(size_t)at].s.done = kGuidedDecided;
    }
    return rc;
  }

  void Decided(int32_t* d, int64_t* nodes, uint8_t* gu) const override {
    for (int i = 0; i < this->n; ++i) {
      d[i] = decided[(size_t)i];
      nodes[i] = solved_nodes[(size_t)i];
    }
    if (gu != nullptr) std::memcpy(gu, given_up.data(), given_up.size());
  }
};

template <int G>
Session* MakeTactics(int n, const int32_t* hidden, const uint8_t* done, int simulations, int nodes, int width,
                     float c_puct, int tactics, long long tactics_nodes, uint8_t* obs, uint8_t* mask, uint8_t* status,
                     int* rc) {
  if (simulations < 1 || simulations > kSearchMaxSimulations || nodes < simulations + 1 || nodes > kGuidedMaxNodes ||
      width < 1 || width > kGuidedMaxWidth || tactics < 0 || tactics > kGuidedMaxTactics || tactics_nodes < 1 ||
      tactics_nodes > kGuidedMaxTacticsNodes) {
    *rc = -6;
    return nullptr;
  }
  TacticsRun<G>* r = new TacticsRun<G>(n, simulations, nodes, width, c_puct, tactics, tactics_nodes);
  *rc = r->Begin(hidden, done, obs, mask, status);
  if (*rc != 0) {
    delete r;
    return nullptr;
  }
  return r;
}

// one step of a position given by its hidden words, through pgx_env.hip.h alone
template <int G>
int StepWords(const int32_t* hidden_in, int action, int32_t* hidden_out, uint8_t* obs, uint8_t* mask, int32_t* info) {
  constexpr int OB = Dims<G>::H * Dims<G>::W * Dims<G>::C;
  State s{};
  if (!SetHidden<G>(s, hidden_in)) return -2;
  Rewards rw{{0.0f, 0.0f}};
  if (action >= 0) rw = Step<G>(s, action);
  View v{};
  v.s = s;
  const int mover = (int)Elem<G>(v, kCurrentPlayer, 0);
  for (int e = 0; e < OB; ++e) obs[e] = (uint8_t)Elem<G>(v, kObs, mover * OB + e);
  for (int e = 0; e < Dims<G>::A; ++e) mask[e] = (uint8_t)Elem<G>(v, kMask, e);
  Hidden<G>(s, hidden_out);
  info[0] = s.done ? 1 : 0;
  info[1] = mover;
  info[2] = (int)rw.r[0];
  info[3] = (int)rw.r[1];
  return 0;
}
}  // namespace

extern "C" {

// A session as pgx_wide_begin's with the exact leaf status: tactics = D (0: off), tactics_nodes = M.  It is advanced,
// read, rerooted and ended through pgx_wide_advance / _result / _reroot / _end.  *rc as pgx_wide_begin; -6 also for D
// or M out of range.
void* pgx_tactics_begin(int game, int n, const int32_t* hidden, const uint8_t* done, int simulations, int nodes,
                        int width, float c_puct, int tactics, long long tactics_nodes, uint8_t* obs, uint8_t* mask,
                        uint8_t* status, int* rc) {
#define EPA_MAKE(G) \
  MakeTactics<G>(n, hidden, done, simulations, nodes, width, c_puct, tactics, tactics_nodes, obs, mask, status, rc)
  switch (game) {
    case kTicTacToe: return EPA_MAKE(kTicTacToe);
    case kConnectFour: return EPA_MAKE(kConnectFour);
    case kHex: return EPA_MAKE(kHex);
    case kOthello: return EPA_MAKE(kOthello);
    default: *rc = -1; return nullptr;
  }
#undef EPA_MAKE
}

// decided [n], the solver's visited positions [n], and (may be null) per slot whether its leaf of the last advance was
// given up [n * width]
void pgx_tactics_decided(void* session, int32_t* decided, int64_t* nodes, uint8_t* given_up) {
  dynamic_cast<TacticsSession*>(static_cast<Session*>(session))->Decided(decided, nodes, given_up);
}

// The position `hidden_in` after `action` (action < 0: the position itself): its hidden words, the mover's obs row,
// the legal mask, info = {done, the seat to move, seat 0's and seat 1's reward of the step}.  -2: no position.
int pgx_tactics_step(int game, const int32_t* hidden_in, int action, int32_t* hidden_out, uint8_t* obs, uint8_t* mask,
                     int32_t* info) {
  switch (game) {
    case kTicTacToe: return StepWords<kTicTacToe>(hidden_in, action, hidden_out, obs, mask, info);
    case kConnectFour: return StepWords<kConnectFour>(hidden_in, action, hidden_out, obs, mask, info);
    case kHex: return StepWords<kHex>(hidden_in, action, hidden_out, obs, mask, info);
    case kOthello: return StepWords<kOthello>(hidden_in, action, hidden_out, obs, mask, info);
    default: return -1;
  }
}

int pgx_tactics_limits(int which) {
  return which == 0 ? kGuidedMaxTactics : which == 1 ? (int)kGuidedMaxTacticsNodes : kGuidedDecided;
}

}  // extern "C"

#ifdef PGX_TACTICS_MAIN
#include <cstdio>

// Three rounds of one ConnectFour session (4 roots a few plies in, W = 4, D = 2, S = 24) with a constant evaluator and
// a reroot by the chosen move between the rounds: an ordinary process for the host sanitizers.
int main() {
  constexpr int G = kConnectFour, A = Dims<G>::A, OB = Dims<G>::H * Dims<G>::W * Dims<G>::C, HW = HiddenWords<G>();
  const int n = 4, S = 24, W = 4, C = 3 * S + 1;
  std::vector<int32_t> hidden((size_t)n * HW);
  std::vector<uint8_t> done((size_t)n, 0), o1(OB), m1(A);
  for (int i = 0; i < n; ++i) {
    State s{};
    s.done = 1;
    struct Gen {
      uint32_t x;
      uint32_t Next() { return x = x * 1664525u + 1013904223u; }
    } rng{(uint32_t)(7 + i)};
    Reset<G>(rng, s);
    std::vector<int32_t> w(HW), w2(HW);
    Hidden<G>(s, w.data());
    int32_t info[4];
    for (int ply = 0; ply < 6 + i; ++ply) {  // columns 3 4 3 4 .., then over the board: some threats
      const int a = (ply * (i + 2) + 3) % A;
      if (pgx_tactics_step(G, w.data(), a, w2.data(), o1.data(), m1.data(), info) != 0 || info[0]) break;
      w = w2;
    }
    std::memcpy(hidden.data() + (size_t)i * HW, w.data(), sizeof(int32_t) * HW);
  }
  std::vector<uint8_t> obs((size_t)n * W * OB), mask((size_t)n * W * A), status((size_t)n * W);
  int rc = -9;
  void* h = pgx_tactics_begin(G, n, hidden.data(), done.data(), S, C, W, 1.25f, 2, 4096, obs.data(), mask.data(),
                              status.data(), &rc);
  if (h == nullptr || rc != 0) return 1;
  std::vector<float> priors((size_t)n * W * A), values((size_t)n * W, 0.0f);
  std::vector<int32_t> visits((size_t)n * A), action(n), used(n), sims(n), decided(n);
  std::vector<float> vals((size_t)n * A);
  std::vector<int64_t> nodes(n);
  for (int round = 0; round < 3; ++round) {
    for (int t = 0; t <= S; ++t) {
      for (size_t r = 0; r < (size_t)n * W; ++r) {
        int legal = 0;
        for (int a = 0; a < A; ++a) legal += mask[r * A + a];
        for (int a = 0; a < A; ++a) priors[r * A + a] = mask[r * A + a] ? 1.0f / (float)legal : 0.0f;
      }
      if (pgx_wide_advance(h, priors.data(), values.data(), obs.data(), mask.data(), status.data()) != 0) return 2;
    }
    pgx_wide_result(h, visits.data(), vals.data(), action.data(), used.data(), sims.data());
    pgx_tactics_decided(h, decided.data(), nodes.data(), nullptr);
    for (int i = 0; i < n; ++i) {
      std::printf("round %d root %d: action %d, %d nodes, %d decided, %lld solved positions\n", round, i, action[i],
                  used[i], decided[i], (long long)nodes[i]);
      if (action[i] < 0) action[i] = 0;
    }
    if (round < 2 && pgx_wide_reroot(h, action.data(), S, obs.data(), mask.data(), status.data()) != 0) return 3;
  }
  pgx_wide_end(h);
  return 0;
}
#endif
