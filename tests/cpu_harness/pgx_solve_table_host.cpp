// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_solve.hip.h with its transposition tables,
// built with g++ by tests/pgx_solve_table_util.py.  It is pgx_solve_host.cpp's walk of a wave -- the top tree level by
// level, the lanes in lockstep rounds as loops, the combine between rounds -- with table_bits: every lane owns a table
// of 2^table_bits entries, zeroed per root; table_bits = 0 runs the TABLE = false instantiation.  Not linked by
// envpool_amd/.
#include <cstdint>
#include <memory>
#include <vector>

#include "../../envpool_amd/csrc/pgx_solve.hip.h"

using namespace epa::pgx;

namespace {
template <int G, bool TABLE>
int Run(int n, const int32_t* hidden, const uint8_t* done, int depth, long long max_nodes, int bits, int8_t* value,
        int8_t* q, int32_t* action, uint8_t* status, int64_t* nodes, uint8_t* broken, int64_t* rounds) {
  constexpr int W = HiddenWords<G>(), A = Dims<G>::A, L = kSolveWave;
  const int limit = SolveLimit(depth);
  const bool hard = depth == 0;
  std::vector<SolveWord> stack(SolveStackBytes(depth) / sizeof(SolveWord));
  std::vector<SolveWord> table(SolveTableBytes(bits) / sizeof(SolveWord));
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
    table.assign(table.size(), SolveWord{0, 0});  // empty at the start of every root
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
          SolveLaneSlice<G, TABLE>(lanes[(size_t)lane], t, stack.data(), lane, kSolveSlice, limit, hard,
                                   TABLE ? SolveLaneTable(table.data(), lane, bits) : nullptr, bits);
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

template <int G>
int RunBits(int n, const int32_t* hidden, const uint8_t* done, int depth, long long max_nodes, int bits, int8_t* value,
            int8_t* q, int32_t* action, uint8_t* status, int64_t* nodes, uint8_t* broken, int64_t* rounds) {
  if (depth < 0 || depth > kSolveMaxDepth || max_nodes < 1 || bits < 0 || bits > kSolveMaxTableBits) return -4;
  return bits == 0
             ? Run<G, false>(n, hidden, done, depth, max_nodes, 0, value, q, action, status, nodes, broken, rounds)
             : Run<G, true>(n, hidden, done, depth, max_nodes, bits, value, q, action, status, nodes, broken, rounds);
}

// stores `stored` with r = plies[0] plies left and the bounds, then looks `probed` up with r = plies[1], both in a
// table of one entry (table_bits = 0: every key has slot 0)
template <int G>
int KeyTest(const int32_t* stored, const int32_t* probed, const int* plies, int lo, int hi, int* got) {
  State s{}, p{};
  if (!SetHidden<G>(s, stored) || !SetHidden<G>(p, probed)) return -2;
  SolveWord table[2] = {SolveWord{0, 0}, SolveWord{0, 0}};
  if (SolveTableLookup(table, 0, SolveTableKey<G>(p, plies[1]), got, got + 1)) return -3;  // an empty table hits
  SolveTableStore(table, 0, SolveTableKey<G>(s, plies[0]), lo, hi);
  return SolveTableLookup(table, 0, SolveTableKey<G>(p, plies[1]), got, got + 1) ? 1 : 0;
}
}  // namespace

extern "C" {

// pgx_solve of pgx_solve_host.cpp with table_bits (0 .. kSolveMaxTableBits) behind max_nodes; the same rows and
// return codes.
int pgx_solve_table(int game, int n, const int32_t* hidden, const uint8_t* done, int depth, long long max_nodes,
                    int table_bits, int8_t* value, int8_t* q, int32_t* action, uint8_t* status, int64_t* nodes,
                    uint8_t* broken, int64_t* rounds) {
  switch (game) {
    case kTicTacToe:
      return RunBits<kTicTacToe>(n, hidden, done, depth, max_nodes, table_bits, value, q, action, status, nodes,
                                 broken, rounds);
    case kConnectFour:
      return RunBits<kConnectFour>(n, hidden, done, depth, max_nodes, table_bits, value, q, action, status, nodes,
                                   broken, rounds);
    case kHex:
      return RunBits<kHex>(n, hidden, done, depth, max_nodes, table_bits, value, q, action, status, nodes, broken,
                           rounds);
    case kOthello:
      return RunBits<kOthello>(n, hidden, done, depth, max_nodes, table_bits, value, q, action, status, nodes, broken,
                               rounds);
    default: return -1;
  }
}

// 1: the probe hit, got[0 .. 1] = the stored bounds; 0: it missed; -1: no such game; -2: words that are no position;
// -3: a hit in an empty table.
int pgx_solve_table_key_test(int game, const int32_t* stored, const int32_t* probed, const int* plies, int lo, int hi,
                             int* got) {
  switch (game) {
    case kTicTacToe: return KeyTest<kTicTacToe>(stored, probed, plies, lo, hi, got);
    case kConnectFour: return KeyTest<kConnectFour>(stored, probed, plies, lo, hi, got);
    case kHex: return KeyTest<kHex>(stored, probed, plies, lo, hi, got);
    case kOthello: return KeyTest<kOthello>(stored, probed, plies, lo, hi, got);
    default: return -1;
  }
}

int pgx_solve_slice() { return kSolveSlice; }
int pgx_solve_table_floor() { return kSolveTableFloor; }
int pgx_solve_table_max_bits() { return kSolveMaxTableBits; }
long long pgx_solve_table_bytes(int bits) { return (long long)SolveTableBytes(bits); }

}  // extern "C"
