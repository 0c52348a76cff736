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
//
// Transposition tables (table_bits = b, 1 .. kSolveMaxTableBits; DESIGN.md "PGX solve: transposition tables").  b = 0
// is the traversal above, untouched (the TABLE = false instantiations).  With b > 0 every lane of the root's wave owns
// a private table of 2^b entries, empty (all bytes zero) at the start of the call and kept over the frontier entries
// the lane takes.  A lane reads and writes its own table only, so the determinism rule above still holds: a row
// depends on its position, D, max_nodes and b.
//   stored   when a node is finished (the "done with" branch of SolveLaneSlice), with r >= kSolveTableFloor plies left
//            (r = the limit minus the node's depth in T_D; with D = 0 the limit is the cap): a lower and an upper bound
//            of its value for its mover, from the fail-hard result v and the window [alpha0, beta] it started with --
//            v <= alpha0: [-1, v]; v >= beta: [v, 1]; otherwise [v, v].  alpha0 travels on the stack (bits 122 and 123
//            of word 4).  A node left unfinished (a dead entry, a give-up) stores nothing.  A store always replaces.
//   probed   a child that Step just made, that runs on and is above the horizon, with r >= kSolveTableFloor, before
//            it is pushed (the Step is counted in `nodes` as before).  A hit gives a value only where that is sound:
//            lo = hi, lo >= the child's beta, or hi <= the child's alpha; bounds cut, they never narrow a window.
//   key      a hit needs every field equal that the value for the mover depends on; the hash only picks the slot.
//            What Step reads, per game, and so what the key holds:
//              a, b     all games (TicTacToe / ConnectFour: the colours' cells; Hex / Othello: the mover's and the
//                       other's)
//              flags    TicTacToe / ConnectFour: turn (the colour that places; a, b are absolute).  Hex: turn as one of
//                       four classes -- 0 (the next ply opens the swap), 1 (the swap is open), even >= 2, odd >= 3 --:
//                       Step reads turn & 1 (the mover's edges) and turn == 1, and turn + 1 of class c is of a class
//                       that c fixes.  Othello: passed != 0.
//              r        always, also for D = 0: the value at r plies left is not the value at r' (the horizon cuts
//                       elsewhere; with D = 0 a line may pass the cap elsewhere), and an Othello pass lets a position
//                       occur at two depths.
//            Left out: cp -- the value is the mover's, whoever sits there: every reward is mapped to seats through
//            cp, and SolveTerminal maps it back through the same cp (Hex: HexCurrent) --; Othello's turn, which Step
//            only flips; m, a function of a, b and (Hex) turn == 1 by Step and SetHidden alike; done, 0 for every
//            position that is stored or probed.
//   entry    32 bytes, two 16-byte words: word 0 = a (bits 0 .. 120) and meta bits 0 .. 6 in bits 121 .. 127; word 1 =
//            b and meta bits 7 .. 13 likewise (no game has a cell above 120).  meta: bits 0 .. 3 the bounds, 1 + 3 (lo
//            + 1) + (hi + 1), 0: the entry is empty; bits 4 .. 5 the flags; bits 6 .. 12 r - 1; bit 13 zero.  Entry i
//            of lane j of a root at 32-byte entry j * 2^b + i of the root's k-th part of the table buffer
//            (SolveTableBytes per root).
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
constexpr int kSolveMaxTableBits = 16;
constexpr int kSolveTableFloor = 2;  // positions with fewer plies left are neither probed nor stored
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


// ---- transposition table (the header comment has the contract and the layout) ----
// bytes of one root's tables: 64 lanes x 2^bits entries of 32 bytes; 0 without a table
PGX_HD inline size_t SolveTableBytes(int bits) { return bits == 0 ? 0 : ((size_t)kSolveWave * 32) << bits; }
// lane j's table in a root's part of the buffer
PGX_HD inline SolveWord* SolveLaneTable(SolveWord* root_table, int lane, int bits) {
  return root_table + ((size_t)lane * 2 << bits);
}

// an entry's four 64-bit halves with the bounds zero
struct SolveKey {
  uint64_t w[4];
};
constexpr int kSolveMetaShift = 57;  // bit 121 of a 16-byte word, in its high half
constexpr uint64_t kSolveBoundsMask = 15ull << kSolveMetaShift;

template <int G>
PGX_HD inline int SolveTableFlags(const State& s) {
  if (G == kHex) return s.turn < 2 ? s.turn : 2 + (s.turn & 1);
  if (G == kOthello) return s.passed != 0 ? 1 : 0;
  return s.turn & 1;
}
template <int G>
PGX_HD inline SolveKey SolveTableKey(const State& s, int plies_left) {
  const uint64_t meta = (uint64_t)SolveTableFlags<G>(s) << 4 | (uint64_t)(plies_left - 1) << 6;
  return SolveKey{{(uint64_t)s.a, (uint64_t)(s.a >> 64) | (meta & 127) << kSolveMetaShift, (uint64_t)s.b,
                   (uint64_t)(s.b >> 64) | (meta >> 7) << kSolveMetaShift}};
}
// the slot of a key in a table of 2^bits entries
PGX_HD inline uint32_t SolveTableIndex(const SolveKey& k, int bits) {
  uint64_t h = k.w[0] * 0x9E3779B97F4A7C15ull ^ k.w[1] * 0xC2B2AE3D27D4EB4Full ^ k.w[2] * 0x165667B19E3779F9ull ^
               k.w[3] * 0xD6E8FEB86659FD93ull;
  h ^= h >> 32;
  h *= 0x9E3779B97F4A7C15ull;
  return (uint32_t)(h >> 32) & ((1u << bits) - 1u);
}
// the bounds stored under the key; false: none (the slot is empty or holds another position)
PGX_HD inline bool SolveTableLookup(const SolveWord* table, int bits, const SolveKey& k, int* lo, int* hi) {
  const SolveWord* e = table + (size_t)SolveTableIndex(k, bits) * 2;
  const SolveWord e0 = e[0], e1 = e[1];
  const int code = (int)((e0.hi & kSolveBoundsMask) >> kSolveMetaShift);
  if (code == 0 || e0.lo != k.w[0] || (e0.hi & ~kSolveBoundsMask) != k.w[1] || e1.lo != k.w[2] || e1.hi != k.w[3]) {
    return false;
  }
  *lo = (code - 1) / 3 - 1;
  *hi = (code - 1) % 3 - 1;
  return true;
}
// the value of the position for its mover in the window [alpha, beta], where the stored bounds give one; else
// kSolveUnknown
PGX_HD inline int SolveTableProbe(const SolveWord* table, int bits, const SolveKey& k, int alpha, int beta) {
  int lo, hi;
  if (!SolveTableLookup(table, bits, k, &lo, &hi)) return kSolveUnknown;
  if (lo == hi || lo >= beta) return lo;
  if (hi <= alpha) return hi;
  return kSolveUnknown;
}
PGX_HD inline void SolveTableStore(SolveWord* table, int bits, const SolveKey& k, int lo, int hi) {
  SolveWord* e = table + (size_t)SolveTableIndex(k, bits) * 2;
  const uint64_t code = (uint64_t)(1 + 3 * (lo + 1) + (hi + 1));
  e[0] = SolveWord{k.w[0], k.w[1] | code << kSolveMetaShift};
  e[1] = SolveWord{k.w[2], k.w[3]};
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
  int32_t alpha0;  // the alpha cur started with (used with a table only)
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
  l.alpha = l.beta = l.alpha0 = 0;
  l.sp = l.base = 0;
  l.entry = lane;
  l.active = 0;
  l.flags = SolveFlags{0, 0};
  l.visited = 0;
}

PGX_HD inline bool SolveLaneBusy(const SolveLane& l, const SolveTop& t) { return l.active || l.entry < t.count; }

template <bool TABLE = false>
PGX_HD inline void SolvePush(SolveWord* stack, int lane, const SolveLane& l) {
  const u128 w[4] = {l.cur.a, l.cur.b, l.cur.m,
                     (u128)(uint32_t)l.cur.turn | (u128)(uint32_t)l.cur.cp << 32 | (u128)(uint32_t)l.cur.passed << 64 |
                         (u128)(uint32_t)l.cur.done << 96};
  for (int i = 0; i < 4; ++i) *SolveSlot(stack, lane, l.sp, i) = SolveWord{(uint64_t)w[i], (uint64_t)(w[i] >> 64)};
  const uint64_t ab = (uint64_t)(l.alpha + 1) | (uint64_t)(l.beta + 1) << 2;
  const uint64_t a0 = TABLE ? (uint64_t)(l.alpha0 + 1) << 58 : 0;
  *SolveSlot(stack, lane, l.sp, 4) = SolveWord{(uint64_t)l.rem, (uint64_t)(l.rem >> 64) | a0 | ab << 60};
}
template <bool TABLE = false>
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
  l.rem = (u128)(x.hi & ((1ull << (TABLE ? 58 : 60)) - 1)) << 64 | x.lo;
  if (TABLE) l.alpha0 = (int)((x.hi >> 58) & 3) - 1;
  l.alpha = (int)((x.hi >> 60) & 3) - 1;
  l.beta = (int)((x.hi >> 62) & 3) - 1;
}

// One round of one lane: up to `budget` positions visited.  Reads t.dead, t.list, the entries' nodes; writes the value
// of the entries it finishes (its own nodes only).  TABLE: with the lane's own table of 2^bits entries.
template <int G, bool TABLE = false>
PGX_HD inline void SolveLaneSlice(SolveLane& l, SolveTop& t, SolveWord* stack, int lane, int budget, int limit,
                                  bool hard, SolveWord* table = nullptr, int bits = 0) {
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
      if (TABLE) l.alpha0 = -1;
      l.sp = 0;
      l.base = t.depth[node];
      l.active = 1;
    }
    if (l.alpha >= l.beta || l.rem == 0) {  // cur is done with: its value is alpha
      const int v = l.alpha;
      if (TABLE) {
        const int left = limit - (l.base + l.sp);
        if (left >= kSolveTableFloor) {
          SolveTableStore(table, bits, SolveTableKey<G>(l.cur, left), v >= l.beta ? v : v <= l.alpha0 ? -1 : v,
                          v >= l.beta ? 1 : v);
        }
      }
      if (l.sp == 0) {
        t.val[t.list[l.entry]] = (int8_t)v;
        l.active = 0;
        l.entry += kSolveWave;
        continue;
      }
      --l.sp;
      SolvePop<TABLE>(stack, lane, l);
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
      if (TABLE) {  // the child's window is [-beta, -alpha]
        const int left = limit - (l.base + l.sp + 1);
        if (left >= kSolveTableFloor) {
          const int v = SolveTableProbe(table, bits, SolveTableKey<G>(child, left), -l.beta, -l.alpha);
          if (v != kSolveUnknown) {
            if (-v > l.alpha) l.alpha = -v;
            continue;
          }
        }
      }
      SolvePush<TABLE>(stack, lane, l);
      ++l.sp;
      const int na = -l.beta, nb = -l.alpha;
      l.cur = child;
      l.rem = child.m;
      l.alpha = na;
      l.beta = nb;
      if (TABLE) l.alpha0 = na;
    }
  }
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_SOLVE_HIP_H_
