// PGX exact solver: alpha-beta over pgx::Step for one root, as __host__ __device__ pieces shared by the solve kernel
// (PgxSolveKernel in pgx.hip, one wave per root) and the g++ host harness of the tests
// (tests/cpu_harness/pgx_solve_host.cpp, which walks a wave's lanes as loops).  No model, no random numbers, no
// floating point.
//
// The contract (DESIGN.md "PGX solve").  D = depth; D = 0: no horizon (up to kSolveMaxDepth plies).  T_D(root) is the
// game tree from the root's position, cut after D plies.
//   leaf values     a leaf that is a finished game: the reward of its last step for the mover at the root (+1, 0, -1;
//                   seat 1's is the negative of seat 0's, pgx_search.hip.h); a leaf cut by the horizon: 0
//   interior        plain minimax; an Othello pass and Hex's swap are plies like any other
//   q[A]     int8   per legal root action the exact minimax value of T_D through it, seen from the root's mover;
//                   -128 for an illegal action
//   value    int8   the maximum of q over the legal actions
//   action   int32  the lowest legal action whose q equals value
//   status   uint8  0 solved.  1 given up: more than max_nodes positions were visited for this root, or a line went
//                   past kSolveMaxDepth plies (D = 0 only), or the position is broken (below); value 0, action -1,
//                   q -128 throughout.  2 the env is over; the row is as for status 1.
//   nodes    int64  the positions visited (the root, every position a Step made)
// D > 0: value +1 is a forced win within D plies, -1 a forced loss within D plies, 0 neither; D = 0 is the
// game-theoretic value.  The values are exact, so they do not depend on the traversal; `nodes`, and which rows are
// given up at a tight max_nodes, do, and are fixed by the traversal below: the same call gives the same bytes, and a
// row does not depend on the other rows of the call (id order, repeated ids, sharding).
// A running position without a legal action is no position of the four games: the pool's error word is set, as in
// search(), and the row is given up.
//
// kSolveMaxDepth = 128 plies.  The longest Hex game is 122 plies (121 cells and the swap).  An Othello game has at
// most 60 placements and never two passes in a row before its last ply, so at most 60 + 61 plies.  Both fit, from the
// first position; TicTacToe (9) and ConnectFour (42) are far below.
//
// The traversal, for one root:
//   top tree    the first levels of T_D breadth-first, at most kSolveTopNodes nodes (SolveTop: in the kernel, LDS).
//               Level 1 is always opened (a root has at most 122 children): one node per root action, so q needs no
//               cut-off at the root.  The next level is opened while all the children of the last level's open nodes
//               still fit (SolveTopPlan: the frontier rule).  A node is open when its game runs on and it is above
//               the horizon; the open nodes of the last level, in node order, are the frontier.
//   lanes       lane j solves frontier entries j, j + 64, .. in that order, each by an iterative negamax alpha-beta
//               with the window [-1, 1] on an explicit stack (SolveLaneSlice): fail-hard, moves in action order, a
//               cut-off at alpha >= beta -- with three values, at the first +1.  The position after a ply is Step<G>
//               on a copy.  The node a lane is at lives in its registers; the stack holds the nodes below it.
//   rounds      the lanes run in lockstep rounds of kSolveSlice visited positions per lane.  Between two rounds the
//               wave adds up `nodes` (the status rule: SolveGaveUp), minimaxes what is known up the top tree
//               (SolveCombine; a node is known as soon as one child gives it +1, or all children are known) and marks
//               the nodes below a known node other than the root as dead.  A lane leaves a dead entry at the next
//               round boundary and skips dead entries when it takes its next one.  What a lane does in a round depends
//               on its own state and the marks of the round's start only, so `nodes` is deterministic.
//   result      q from the root's children, value and action from q (SolveRootResult).
//
// The stack (SolveStackBytes): per ply 5 words of 16 bytes per lane -- the State (4 words) and the moves not tried yet
// (122 bits) with alpha and beta in the 4 bits above them --, word w of ply p of lane j at 16-byte word
// (p * 5 + w) * 64 + j: the 64 lanes' words of one ply are contiguous, a wave's store or load of one word is 1 KiB in
// one piece.  It is touched on the way down (a push: 5 stores) and up (a pop: 5 loads) only; a position whose game is
// over or that the horizon cuts is valued from registers.
#ifndef ENVPOOL_AMD_CSRC_PGX_SOLVE_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_SOLVE_HIP_H_

#include "pgx_search.hip.h"

namespace epa {
namespace pgx {

constexpr int kSolveWave = kSearchWave;
constexpr int kSolveMaxDepth = 128;
constexpr int kSolveTopNodes = 256;
constexpr int kSolveSlice = 512;     // positions a lane may visit in one round
constexpr int kSolveUnknown = 2;     // a node's value before it is known
constexpr int kSolveIllegal = -128;  // q of an illegal action, and of every action of a row that is not solved
constexpr int kSolveWords = 5;       // 16-byte words per ply and lane of the stack
enum SolveStatus : int { kSolveSolved = 0, kSolveGivenUp = 1, kSolveOver = 2 };

// plies a line may have: the horizon, or the cap; `hard`: a line that reaches it undecided is given up, not cut
PGX_HD inline int SolveLimit(int depth) { return depth == 0 ? kSolveMaxDepth : depth; }
// bytes of one root's stack
PGX_HD inline size_t SolveStackBytes(int depth) {
  return (size_t)SolveLimit(depth) * kSolveWords * kSolveWave * 16;
}

struct alignas(16) SolveWord {
  uint64_t lo, hi;
};
PGX_HD inline SolveWord* SolveSlot(SolveWord* stack, int lane, int ply, int w) {
  return stack + ((size_t)ply * kSolveWords + w) * kSolveWave + lane;
}

// the value of the position `s` after a step with seat 0's reward `term0`, for the seat that moves at `s`
template <int G>
PGX_HD inline int SolveTerminal(const State& s, int term0) {
  return SearchSign<G>(s) * term0;
}

// The top of a root's tree, breadth-first: node 0 is the root, a node's children follow each other in action order,
// the levels follow each other.  val is the node's value for the seat that moves at it, or kSolveUnknown.
struct SolveTop {
  State s[kSolveTopNodes];
  int16_t parent[kSolveTopNodes];
  int16_t first[kSolveTopNodes];   // the first child; -1: none (not opened, or not open)
  int16_t list[kSolveTopNodes];    // the frontier: the open nodes of the last level
  uint8_t nchild[kSolveTopNodes];
  uint8_t act[kSolveTopNodes];     // the action that led here
  uint8_t depth[kSolveTopNodes];
  uint8_t dead[kSolveTopNodes];    // below a known node other than the root
  int8_t val[kSolveTopNodes];
  int32_t n;       // nodes
  int32_t lo, hi;  // the last level
  int32_t next_n;  // the nodes after the level that SolveTopPlan laid out
  int32_t count;   // frontier entries
};

PGX_HD inline int SolveLowest(u128 m) {
  const uint64_t lo = (uint64_t)m, hi = (uint64_t)(m >> 64);
#if defined(__HIP_DEVICE_COMPILE__)
  return lo ? __ffsll((unsigned long long)lo) - 1 : 64 + __ffsll((unsigned long long)hi) - 1;
#else
  return lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll(hi);
#endif
}

PGX_HD inline void SolveTopInit(SolveTop& t, const State& root) {
  t.s[0] = root;
  t.parent[0] = -1;
  t.first[0] = -1;
  t.nchild[0] = 0;
  t.act[0] = 0;
  t.depth[0] = 0;
  t.dead[0] = 0;
  t.val[0] = kSolveUnknown;
  t.n = 1;
  t.lo = 0;
  t.hi = 1;
  t.next_n = 1;
  t.count = 0;
}

// The frontier rule, by one lane: the children of the last level's open nodes are laid out behind it (parent, act,
// first, nchild; their positions come from SolveTopMake) if they all fit, and next_n counts them in; next_n = n
// otherwise, or when no node is open.
PGX_HD inline void SolveTopPlan(SolveTop& t) {
  int children = 0;
  for (int i = t.lo; i < t.hi; ++i) {
    if (t.val[i] == kSolveUnknown) children += Count(t.s[i].m);
  }
  t.next_n = t.n;
  if (children == 0 || t.n + children > kSolveTopNodes) return;
  int c = t.n;
  for (int i = t.lo; i < t.hi; ++i) {
    if (t.val[i] != kSolveUnknown) continue;
    u128 m = t.s[i].m;
    t.first[i] = (int16_t)c;
    t.nchild[i] = (uint8_t)Count(m);
    while (m != 0) {
      const int a = SolveLowest(m);
      m &= m - 1;
      t.parent[c] = (int16_t)i;
      t.act[c] = (uint8_t)a;
      ++c;
    }
  }
  t.next_n = c;
}

// what the making of positions met: a line at the cap (D = 0), a running position without a legal action
struct SolveFlags {
  int overflow, broken;
};

// node c of a level that SolveTopPlan laid out: its position and what is known of its value
template <int G>
PGX_HD inline void SolveTopMake(SolveTop& t, int c, int limit, bool hard, SolveFlags& f) {
  const int p = t.parent[c];
  State s;
  const int term0 = SearchExpand<G>(t.s[p], t.act[c], s);
  const int d = t.depth[p] + 1;
  int val = kSolveUnknown;
  if (s.done) {
    val = SolveTerminal<G>(s, term0);
  } else if (d >= limit) {
    val = 0;
    if (hard) f.overflow = 1;
  } else if (s.m == 0) {
    f.broken = 1;
  }
  t.s[c] = s;
  t.first[c] = -1;
  t.nchild[c] = 0;
  t.depth[c] = (uint8_t)d;
  t.dead[c] = 0;
  t.val[c] = (int8_t)val;
}

// the level is made: it is the last one now
PGX_HD inline void SolveTopAdvance(SolveTop& t) {
  t.lo = t.hi;
  t.hi = t.n = t.next_n;
}

// the frontier: the open nodes of the last level, in node order
PGX_HD inline void SolveTopFrontier(SolveTop& t) {
  int k = 0;
  for (int i = t.lo; i < t.hi; ++i) {
    if (t.val[i] == kSolveUnknown) t.list[k++] = (int16_t)i;
  }
  t.count = k;
}

// The combine, by one lane: what is known minimaxed up the tree (children have higher indices than their parent), then
// the dead marks down it.
PGX_HD inline void SolveCombine(SolveTop& t) {
  for (int i = t.n - 1; i >= 0; --i) {
    if (t.first[i] < 0) continue;
    int best = -1, unknown = 0;
    for (int c = t.first[i]; c < t.first[i] + t.nchild[i]; ++c) {
      const int v = t.val[c];
      if (v == kSolveUnknown) {
        unknown = 1;
      } else if (-v > best) {
        best = -v;
      }
    }
    t.val[i] = (int8_t)(best == 1 || !unknown ? best : kSolveUnknown);
  }
  for (int i = 1; i < t.n; ++i) {
    const int p = t.parent[i];
    t.dead[i] = (uint8_t)(p > 0 && (t.dead[p] || t.val[p] != kSolveUnknown));
  }
}

// the status rule, looked at after every level of the top tree and every round
PGX_HD inline bool SolveGaveUp(long long nodes, long long max_nodes, const SolveFlags& f) {
  return nodes > max_nodes || f.overflow != 0 || f.broken != 0;
}

// The row of a solved root (after SolveCombine with every child of the root known): q [A], the value, the action.
template <int G>
PGX_HD inline void SolveRootResult(const SolveTop& t, int8_t* q, int8_t* value, int32_t* action) {
  for (int a = 0; a < Dims<G>::A; ++a) q[a] = (int8_t)kSolveIllegal;
  int best = -2, arg = -1;
  for (int c = t.first[0]; c < t.first[0] + t.nchild[0]; ++c) {
    const int v = -t.val[c];
    q[t.act[c]] = (int8_t)v;
    if (v > best) {
      best = v;
      arg = t.act[c];
    }
  }
  *value = (int8_t)best;
  *action = arg;
}
// the row of a root that is given up or over
template <int G>
PGX_HD inline void SolveNoResult(int8_t* q, int8_t* value, int32_t* action) {
  for (int a = 0; a < Dims<G>::A; ++a) q[a] = (int8_t)kSolveIllegal;
  *value = 0;
  *action = -1;
}

// One lane's negamax: the node it is at (its position, the moves not tried yet, its window), the stack depth below
// it, the frontier entry it works on.
struct SolveLane {
  State cur;
  u128 rem;
  int32_t alpha, beta;
  int32_t sp;      // nodes on the stack below cur
  int32_t base;    // the depth of the entry's node in T_D
  int32_t entry;   // index into the frontier list; >= count: nothing left
  int32_t active;  // cur is a node of entry's subtree
  SolveFlags flags;
  long long visited;
};

PGX_HD inline void SolveLaneInit(SolveLane& l, int lane) {
  l.cur = State{};
  l.rem = 0;
  l.alpha = l.beta = 0;
  l.sp = l.base = 0;
  l.entry = lane;
  l.active = 0;
  l.flags = SolveFlags{0, 0};
  l.visited = 0;
}

PGX_HD inline bool SolveLaneBusy(const SolveLane& l, const SolveTop& t) { return l.active || l.entry < t.count; }

PGX_HD inline void SolvePush(SolveWord* stack, int lane, const SolveLane& l) {
  const u128 w[4] = {l.cur.a, l.cur.b, l.cur.m,
                     (u128)(uint32_t)l.cur.turn | (u128)(uint32_t)l.cur.cp << 32 | (u128)(uint32_t)l.cur.passed << 64 |
                         (u128)(uint32_t)l.cur.done << 96};
  for (int i = 0; i < 4; ++i) *SolveSlot(stack, lane, l.sp, i) = SolveWord{(uint64_t)w[i], (uint64_t)(w[i] >> 64)};
  const uint64_t ab = (uint64_t)(l.alpha + 1) | (uint64_t)(l.beta + 1) << 2;
  *SolveSlot(stack, lane, l.sp, 4) = SolveWord{(uint64_t)l.rem, (uint64_t)(l.rem >> 64) | ab << 60};
}
PGX_HD inline void SolvePop(const SolveWord* stack, int lane, SolveLane& l) {
  u128 w[4];
  for (int i = 0; i < 4; ++i) {
    const SolveWord x = *SolveSlot(const_cast<SolveWord*>(stack), lane, l.sp, i);
    w[i] = (u128)x.hi << 64 | x.lo;
  }
  l.cur.a = w[0];
  l.cur.b = w[1];
  l.cur.m = w[2];
  l.cur.turn = (int32_t)(uint32_t)w[3];
  l.cur.cp = (int32_t)(uint32_t)(w[3] >> 32);
  l.cur.passed = (int32_t)(uint32_t)(w[3] >> 64);
  l.cur.done = (int32_t)(uint32_t)(w[3] >> 96);
  const SolveWord x = *SolveSlot(const_cast<SolveWord*>(stack), lane, l.sp, 4);
  l.rem = (u128)(x.hi & ((1ull << 60) - 1)) << 64 | x.lo;
  l.alpha = (int)((x.hi >> 60) & 3) - 1;
  l.beta = (int)((x.hi >> 62) & 3) - 1;
}

// One round of one lane: up to `budget` positions visited.  Reads t.dead, t.list, the entries' nodes; writes the value
// of the entries it finishes (its own nodes only).
template <int G>
PGX_HD inline void SolveLaneSlice(SolveLane& l, SolveTop& t, SolveWord* stack, int lane, int budget, int limit,
                                  bool hard) {
  if (l.active && t.dead[t.list[l.entry]]) {  // decided above: left as it is
    l.active = 0;
    l.entry += kSolveWave;
  }
  while (budget > 0) {
    if (!l.active) {
      while (l.entry < t.count && t.dead[t.list[l.entry]]) l.entry += kSolveWave;
      if (l.entry >= t.count) break;
      const int node = t.list[l.entry];
      l.cur = t.s[node];
      l.rem = l.cur.m;
      l.alpha = -1;
      l.beta = 1;
      l.sp = 0;
      l.base = t.depth[node];
      l.active = 1;
    }
    if (l.alpha >= l.beta || l.rem == 0) {  // cur is done with: its value is alpha
      const int v = l.alpha;
      if (l.sp == 0) {
        t.val[t.list[l.entry]] = (int8_t)v;
        l.active = 0;
        l.entry += kSolveWave;
        continue;
      }
      --l.sp;
      SolvePop(stack, lane, l);
      if (-v > l.alpha) l.alpha = -v;
      continue;
    }
    const int a = SolveLowest(l.rem);
    l.rem &= l.rem - 1;
    State child;
    const int term0 = SearchExpand<G>(l.cur, a, child);
    ++l.visited;
    --budget;
    if (child.done) {
      const int v = -SolveTerminal<G>(child, term0);
      if (v > l.alpha) l.alpha = v;
    } else if (l.base + l.sp + 1 >= limit) {
      if (hard) l.flags.overflow = 1;
      if (0 > l.alpha) l.alpha = 0;
    } else {
      if (child.m == 0) l.flags.broken = 1;
      SolvePush(stack, lane, l);
      ++l.sp;
      const int na = -l.beta, nb = -l.alpha;
      l.cur = child;
      l.rem = child.m;
      l.alpha = na;
      l.beta = nb;
    }
  }
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_SOLVE_HIP_H_
