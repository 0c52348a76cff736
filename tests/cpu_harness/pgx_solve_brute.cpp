// TEST ORACLE (not product): the contract of the PGX solver as a plain recursive minimax over pgx::Step -- no pruning,
// no window, no stack of its own, no code of pgx_solve.hip.h (it includes pgx_env.hip.h only).  Values are kept as
// seat 0's and maximised or minimised by the seat that moves, so it does not rely on the seats alternating.  Built with
// g++ by tests/test_pgx_solve_host.py.  Not linked by envpool_amd/.
#include <cstdint>

#include "../../envpool_amd/csrc/pgx_env.hip.h"

using namespace epa::pgx;

namespace {
template <int G>
int Mover(const State& s) {
  if (G == kHex) return (s.turn & 1) == 0 ? s.cp : 1 - s.cp;
  return s.cp;
}

// seat 0's minimax value of `s` with `left` plies to the horizon (left < 0: none)
template <int G>
int Value0(const State& s, int left, int64_t& nodes) {
  if (left == 0) return 0;
  const bool maximise = Mover<G>(s) == 0;
  int best = maximise ? -2 : 2;
  for (int a = 0; a < Dims<G>::A; ++a) {
    if (!Has(s.m, a)) continue;
    State c = s;
    const Rewards rw = Step<G>(c, a);
    ++nodes;
    const int v = c.done ? (int)rw.r[0] : Value0<G>(c, left - 1, nodes);
    if (maximise ? v > best : v < best) best = v;
  }
  return best;
}

template <int G>
int Run(int n, const int32_t* hidden, const uint8_t* done, int depth, int8_t* value, int8_t* q, int32_t* action,
        uint8_t* status, int64_t* nodes) {
  constexpr int W = HiddenWords<G>(), A = Dims<G>::A;
  for (int i = 0; i < n; ++i) {
    int8_t* qi = q + (size_t)i * A;
    for (int a = 0; a < A; ++a) qi[a] = -128;
    value[i] = 0;
    action[i] = -1;
    nodes[i] = 0;
    State root{};
    if (!SetHidden<G>(root, hidden + (size_t)i * W)) return -2;
    if (done[i]) {
      status[i] = 2;
      continue;
    }
    const int sign = Mover<G>(root) == 0 ? 1 : -1;
    int64_t count = 1;
    int best = -2, arg = -1;
    for (int a = 0; a < A; ++a) {
      if (!Has(root.m, a)) continue;
      State c = root;
      const Rewards rw = Step<G>(c, a);
      ++count;
      const int v = sign * (c.done ? (int)rw.r[0] : Value0<G>(c, depth == 0 ? -1 : depth - 1, count));
      qi[a] = (int8_t)v;
      if (v > best) {
        best = v;
        arg = a;
      }
    }
    if (arg < 0) return -3;  // a running position has a legal action
    value[i] = (int8_t)best;
    action[i] = arg;
    status[i] = 0;
    nodes[i] = count;
  }
  return 0;
}
}  // namespace

extern "C" {

// n roots (hidden[i]: HiddenWords words, done[i]), depth D (0: to the end of the game).  Row i of value [n], q [n, A],
// action [n], status [n] (0 or 2) as the contract states them; nodes [n]: the positions of the full tree.
int pgx_solve_brute(int game, int n, const int32_t* hidden, const uint8_t* done, int depth, int8_t* value, int8_t* q,
                    int32_t* action, uint8_t* status, int64_t* nodes) {
  switch (game) {
    case kTicTacToe: return Run<kTicTacToe>(n, hidden, done, depth, value, q, action, status, nodes);
    case kConnectFour: return Run<kConnectFour>(n, hidden, done, depth, value, q, action, status, nodes);
    case kHex: return Run<kHex>(n, hidden, done, depth, value, q, action, status, nodes);
    case kOthello: return Run<kOthello>(n, hidden, done, depth, value, q, action, status, nodes);
    default: return -1;
  }
}

}  // extern "C"
