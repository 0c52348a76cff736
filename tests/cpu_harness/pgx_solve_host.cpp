// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_solve.hip.h, built with g++ by
// tests/test_pgx_solve_host.py.  It solves a root the way the kernel's wave does -- the top tree level by level, the
// lanes in lockstep rounds, the combine between rounds -- with the wave's lanes walked as loops.  Positions come in as
// the hidden words of pgx_env.hip.h (SetHidden) plus the done flag.  Not linked by envpool_amd/.
#include <cstdint>
#include <memory>
#include <vector>

#include "../../envpool_amd/csrc/pgx_solve.hip.h"

using namespace epa::pgx;

namespace {
template <int G>
int Run(int n, const int32_t* hidden, const uint8_t* done, int depth, long long max_nodes, int8_t* value, int8_t* q,
        int32_t* action, uint8_t* status, int64_t* nodes, uint8_t* broken, int64_t* rounds) {
  constexpr int W = HiddenWords<G>(), A = Dims<G>::A, L = kSolveWave;
  if (depth < 0 || depth > kSolveMaxDepth || max_nodes < 1) return -4;
  const int limit = SolveLimit(depth);
  const bool hard = depth == 0;
  std::vector<SolveWord> stack(SolveStackBytes(depth) / sizeof(SolveWord));
  std::unique_ptr<SolveTop> top(new SolveTop);
  std::vector<SolveLane> lanes((size_t)L);
  for (int i = 0; i < n; ++i) {
    int8_t* qi = q + (size_t)i * A;
    broken[i] = 0;
    nodes[i] = 0;
    if (rounds != nullptr) rounds[i] = 0;
    SolveNoResult<G>(qi, value + i, action + i);
    State root{};
    if (!SetHidden<G>(root, hidden + (size_t)i * W)) return -2;
    root.done = done[i] ? 1 : 0;
    if (done[i]) {
      status[i] = (uint8_t)kSolveOver;
      continue;
    }
    SolveTop& t = *top;
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
        if (rounds != nullptr) ++rounds[i];
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
    nodes[i] = count;
    broken[i] = (uint8_t)flags.broken;
    if (gave_up) {
      status[i] = (uint8_t)kSolveGivenUp;
      continue;
    }
    SolveCombine(t);
    if (t.val[0] == kSolveUnknown) return -3;  // every child of the root is known by now
    SolveRootResult<G>(t, qi, value + i, action + i);
    status[i] = (uint8_t)kSolveSolved;
  }
  return 0;
}
}  // namespace

extern "C" {

// n roots (hidden[i]: HiddenWords words, done[i]).  Row i of value [n], q [n, A], action [n], status [n], nodes [n]:
// the results of the contract; broken [n]: what the kernel reports through the pool's error word; rounds [n] (may be
// null): the lockstep rounds the root's wave ran, each of up to kSolveSlice positions per lane.  -1: no such game;
// -2: words that are no position; -3: a broken invariant; -4: an argument out of range.
int pgx_solve(int game, int n, const int32_t* hidden, const uint8_t* done, int depth, long long max_nodes,
              int8_t* value, int8_t* q, int32_t* action, uint8_t* status, int64_t* nodes, uint8_t* broken,
              int64_t* rounds) {
  switch (game) {
    case kTicTacToe:
      return Run<kTicTacToe>(n, hidden, done, depth, max_nodes, value, q, action, status, nodes, broken, rounds);
    case kConnectFour:
      return Run<kConnectFour>(n, hidden, done, depth, max_nodes, value, q, action, status, nodes, broken, rounds);
    case kHex: return Run<kHex>(n, hidden, done, depth, max_nodes, value, q, action, status, nodes, broken, rounds);
    case kOthello:
      return Run<kOthello>(n, hidden, done, depth, max_nodes, value, q, action, status, nodes, broken, rounds);
    default: return -1;
  }
}

int pgx_solve_max_depth() { return kSolveMaxDepth; }
int pgx_solve_slice() { return kSolveSlice; }
long long pgx_solve_stack_bytes(int depth) { return (long long)SolveStackBytes(depth); }

}  // extern "C"
