// PGX guided tree search: PUCT selection over a tree that lives on the device between launches, with the priors and
// the leaf values supplied by the caller (AlphaZero-style), as __host__ __device__ pieces shared by the stepwise
// kernels (PgxGuidedBegin / PgxGuidedAdvance / PgxGuidedResult in pgx.hip, one wave per root) and the g++ host harness
// of the tests (tests/cpu_harness/pgx_guided_host.cpp, which walks a wave's lanes as loops).
//
// The contract (DESIGN.md "PGX guided search").  S = simulations, A = Dims<G>::A.  A session covers k listed roots of
// one pool; each root has up to S + 1 nodes.  A node holds its State, `term0` (seat 0's reward of the step that made
// the node, int) and per action a: child[a] (int32, -1: none), v[a] (int32 visits), w0[a] (float32, seat 0's summed
// value through the edge) and p[a] (float32 prior).  Per root the session keeps the node count, the PENDING LEAF (a
// node index), its status and the current path of (node, action) pairs, at most kSearchMaxPath.
//   status 0: evaluate this leaf;  1: the leaf is a finished game, its value is known and the caller's row is ignored;
//          2: nothing is pending: the root was over at begin, or the session has used all its simulations.
//
//   begin(ids, S, c_puct):
//     per root: node 0 = the env's position; path = []; pending = 0; status = the env is over ? 2 : 0
//     emit leaves.
//   advance(priors[k, A], values[k]) -- call number t = 0 .. S:
//     per root with status != 2, L = pending:
//       status 0: for every a: L.p[a] = clean(priors[i, a]);  val0 = sign(L) * cleanv(values[i])
//       status 1: val0 = (float) L.term0
//       for (n, a) in path:  n.v[a] += 1;  n.w0[a] += val0            (float32 add)
//       if t == S:  status = 2
//       else:  node = 0; path = []
//         loop:
//           a = the legal action (bit of node.state.m) of the largest score(node, a); ties: the lowest a
//           path += (node, a)
//           if node.child[a] < 0:
//               c = new node {Step<G>(copy of node.state, a), term0};  node.child[a] = c;  node = c;  break
//           node = node.child[a]
//           if node.state.done: break
//         pending = node;  status = node.state.done ? 1 : 0
//     emit leaves.
//   score(node, a), float32, every operation correctly rounded, in this order, nothing fused:
//     V = sum over b of node.v[b] (int);  sign = +1 if seat 0 moves at the node else -1  (SearchSign<G>)
//     q = node.v[a] > 0 ? (sign * node.w0[a]) / (float) node.v[a] : 0.0f
//     score = q + ((c_puct * node.p[a]) * sqrtf((float)(V + 1))) / (float)(1 + node.v[a])
//   clean(x) = (x >= 0 && x <= FLT_MAX) ? x : 0.0f       cleanv(x) = (x >= -1 && x <= 1) ? x : 0.0f
// values[i] is the value of the leaf for the seat that moves there -- the seat whose observation was emitted.  Priors
// are used as given (the caller normalises them and mixes in root noise); entries of illegal actions are never read
// by a pick.  clean / cleanv make every input bit pattern give a defined result.
//
// Emitted leaves, for all k rows: obs bool [k, H, W, C], the observation row of the seat that moves at the pending
// leaf, element for element what a step into that position returns for that seat (pgx::Elem, kObs); mask bool [k, A],
// the position's legal-action mask; status uint8 [k].  Rows of status 1 or 2 are all zeros in obs and mask.
// Result: visits = the root's v, values = the root's w0 times the root mover's sign, action = the most visited legal
// action (ties: the lowest), -1 and zero rows for a root that was over at begin.
// A running position without a legal action, or a path past kSearchMaxPath, is no position of the game: that root
// ends with status 2 (the kernel also sets the pool's error word, the harness returns -3).
//
// Tree reuse (DESIGN.md "PGX guided search: tree reuse").  A session has a node CAPACITY per root, C: S + 1 unless
// begin is given `nodes = C` with S + 1 <= C <= kGuidedMaxNodes.  A root's node block has C nodes (its stride), and
// advance has one more rule: a root begins a descent only if count < C; otherwise it goes to status 2 for the rest of
// the round, a normal end ("memory used up") that sets no error.  With C = S + 1 and no reroot it never triggers
// (count <= t + 1 <= S at call t < S), so such a session is, byte for byte, the one described above.
//   reroot(actions[k], S2) -- only when the round is complete (simulations + 1 advances made); per root, a = actions[i]:
//     idle root (over != 0, or broken):  stays over (over = 1, status 2); a is ignored
//     a outside 0 .. A-1:                over = 1, status 2  (the host forms refuse such a row before any launch)
//     c = node0.child[a] >= 0:  the subtree of c is kept.  A node is kept if it is c or the child of a kept node
//         (GuidedRerootReach; a child's index is above its parent's, so one pass in index order finds them all).  The
//         new index of a kept node is its rank among the kept nodes in increasing old index (GuidedRerootRank), so
//         order is preserved and c becomes 0.  Each kept node is copied to its new slot with child[] remapped
//         (GuidedRerootEdge); State, term0, v, w0 and p stay bit for bit.  count = the number kept.  As new index <=
//         old index and the nodes are processed in increasing order, a copy only ever lands on a slot whose node was
//         dropped or has moved already, and no later copy reads it: the compaction is in place.
//     c < 0:  node 0 = Step<G>(root position, a), made as SearchExpand makes it; its edges are cleared; count = 1
//     then:   the new root's State.done set (also: an illegal played move, which Step turns into a finished game):
//             over = 1, status 2 -- result() gives -1 and zero rows as for a root that was over at begin;
//             otherwise pending = 0, depth = 0, status 0.
//     the session's simulations become S2 (1 .. 4096, S2 + 1 <= C) and the call number restarts at 0
//     emit leaves.
// The new root is ALWAYS handed out for evaluation, as begin hands out the root: advance 0 of the new round writes the
// caller's priors into it (replacing the stored ones: fresh root noise) and backs up nothing, the statistics below the
// root stay, and result() counts the kept visits.  So a round after reroot is again S2 + 1 advances in lockstep for
// all roots.  reroot has no floating-point arithmetic.
//
// Several leaves per launch (DESIGN.md "PGX guided search: several leaves per launch").  A WIDE session has a width W,
// 1 .. kGuidedMaxWidth: every root has W SLOTS, each what a plain session keeps once per root -- a pending leaf, a
// status and a path -- and an advance answers all pending slots and then descends up to W times, steering the descents
// apart with virtual losses: an edge on the path of an earlier descent of the same launch counts as one more visit
// that lost.  Nodes are GuidedNode<G>, unchanged; there is no per-edge virtual-loss array (the o[] below are
// recomputed from the launch's own paths).  The leaf arrays and the caller's rows have k * W rows, row i * W + j for
// slot j of root i.  The root record is GuidedWideRoot followed by W GuidedWideSlot.  `done` counts the root's
// completed simulations, C is the node capacity.
//   begin_wide(ids, S, C, W, c_puct):
//     as begin; slot 0 = {pending 0, path [], status: the env is over ? 2 : 0}; slots 1..W-1 status 2; done = 0
//   advance(priors[k, W, A], values[k, W]) -- call number t = 0 .. S:
//     A. answers, slots j = 0..W-1 in this order, status_j != 2, L = pending_j:
//          status 0: L.p[a] = clean(priors[i, j, a]) for every a;  val0 = sign(L) * cleanv(values[i, j])
//          status 1: val0 = (float) L.term0
//          for (n, a) in path_j in path order:  n.v[a] += 1;  n.w0[a] += val0        (float32 add)
//          if path_j is not empty: done += 1          (the root's own evaluation is no simulation)
//          status_j = 2; path_j = []
//     B. descents, slots j = 0, 1, ..: begin descent j only while  done + j < S  and  count < C  (and the root is
//        neither over nor broken);  node = 0, path = []:
//          loop:  d = len(path)
//            o[a] = number of slots i < j of THIS launch with len(path_i) > d and path_i[d] == (node, a)
//            pick the legal a of the largest wscore(node, a), ties: the lowest a;  path += (node, a)
//            if node.child[a] < 0:  expand as the plain advance does (SearchExpand); node = the new node; break
//            node = node.child[a]
//            if node.state.done: break
//            if node == pending_i for a slot i < j of this launch with status_i == 0:  COLLISION
//          COLLISION: the descent is dropped (it made no node, stores no path), and this root begins no further
//                     descent in this launch; slots j.. keep status 2
//          else: path_j = path; pending_j = node; status_j = node.state.done ? 1 : 0
//     emit leaves: every slot's row; rows of status 1 or 2 are zeros.
//   wscore(node, a), float32, each operation correctly rounded, nothing fused:
//     n = v[a] + o[a] (int);  V = sum_b v[b] + sum_b o[b] (int)
//     q = n > 0 ? (sign * w0[a] - (float) o[a]) / (float) n : 0.0f
//     wscore = q + ((c_puct * p[a]) * sqrtf((float)(V + 1))) / (float)(1 + n)
// Consequences:
//   - with every o zero, wscore is score (GuidedScore) bit for bit (x - 0.0f == x), and descent 0 of a launch has no
//     earlier slot: a wide session of W = 1 is the plain session, call for call
//   - slot 0 never collides; while done < S and count < C every advance completes at least one simulation, so a round
//     is complete -- all k * W statuses are 2 -- after at most S + 1 advances
//   - two slots of one launch may reach the same finished game: both have status 1 and both back up term0; this is no
//     collision.  No two status-0 slots of one launch share a node
//   - later advances on a complete round, up to call number S, change nothing; a call number above S is refused
//   - the root's visits sum to S after a round whose capacity sufficed; after a reroot the kept visits add to that
//   - a descent makes at most one node and begins only with count < C, so count <= C always
//   - a broken position (as above) ends ALL slots of that root: every status 2, the paths dropped, no later descent
//   - a tree is a tree: a node sits at one depth, so path_i[d] names `node` exactly when path i ran through it
// reroot of a wide session: the rule and the compaction above; afterwards slot 0 is the new root (status 0, or the root
// is over), the other slots are idle, done = 0 and the session's simulations become S2.  The host forms refuse a reroot
// while any status is not 2.  The device form cannot look: slots still pending there are dropped, their paths
// discarded and nothing backed up; their nodes stay unevaluated (priors 0) -- the caller finishes the round first.
//
// Exact leaf status (DESIGN.md "PGX guided search: exact leaf status").  A PUCT session, plain or wide, may be begun
// with tactics = D (1 .. kGuidedMaxTactics; 0: off, and nothing below applies) and tactics_nodes = M (1 .. 2^20).
// advance then has one more stage, AFTER all descents of the launch and before the leaves are final:
//   1. looked at: every slot whose status is 0 and whose pending leaf is not node 0 (GuidedTacticsLooksAt).  The root
//      is always handed out for evaluation; slots of status 1 or 2 are not looked at.
//   2. the leaf's position goes to the solver under the contract of pgx_solve.hip.h, unchanged: T_D of that position
//      with max_nodes = M.  Solve status "solved" and value v != 0: the leaf is DECIDED (GuidedTacticsDecides).  A
//      value of 0, or a leaf given up, leaves everything as it was: the caller evaluates that leaf.
//   3. a decided leaf is, for the rest of the session, a finished game whose last reward is v for the seat that moves
//      there (GuidedTacticsMark): State.done = kGuidedDecided (a second non-zero value, so every test of `done` treats
//      the node as finished), term0 = SearchSign(leaf) * v.  The slot's status becomes 1 and its obs and mask rows
//      zeros; the caller's row for it is ignored, the next advance backs up (float) term0 along the slot's path, and a
//      later descent that arrives at the node stops there with status 1, exactly as at a finished game.
//   4. wide sessions: the decision comes after the launch's descents.  Inside the launch a later descent that reaches
//      the new leaf still meets a status-0 pending leaf: a COLLISION by the rule above.  From the next launch on two
//      slots may reach the decided node together; both have status 1 and both back up term0, as for a finished game.
//   5. reroot: a decided node that becomes the new root (c >= 0) stops being decided (GuidedTacticsReopen): its game
//      runs on, it is handed out with status 0, its term0 is not used, and result() does not report -1 for it.
//      Decided nodes deeper in the kept subtree stay decided, bit for bit.  c < 0 makes a fresh root, undecided.  The
//      new root is node 0, which rule 1 never looks at: reroot has no solver stage.
//   6. result() is unchanged.  `decided` int32 [k] counts the leaves decided since begin and is not reduced by reroot.
//   7. the solver's values are exact and its given-up rows depend on the position, D and M only, so which leaves are
//      decided depends on the session's arguments, the positions and the caller's rows -- not on id order or sharding.
// In one sentence: the session is the plain guided search of the game in which a decided position counts as finished
// with result v.  The mark lives in State.done, the counters in a block of their own per session: GuidedNode and the
// root records are unchanged, and a session with tactics = 0 is, byte for byte, the one described above.
//
// Proven values (DESIGN.md "PGX guided search: proven values"; MCTS-Solver, Winands, Bjornsson, Saito 2008).  A PUCT
// session, plain or wide, with or without nodes=, tactics= and reroot, may be begun with the flag kGuidedProve; without
// it nothing below applies.  sign(n) = SearchSign<G>(n.state); kGuidedUnproven = -128 stands for "no proven value".
//   1. proven node.  A node is proven when state.done != 0, as before: 1 a finished game, kGuidedDecided a position
//      marked with an exact result.  Its value for seat 0 is term0 in {-1, 0, +1}; for the mover of a node n above it,
//      sign(n) * term0 (GuidedProofOf).  Interior nodes marked under rule 3 carry the same mark, GuidedTacticsMark with
//      the proven value, which may be 0.  Every test of `done` then treats the node as finished: descents stop there
//      with status 1 and (float) term0 is backed up from then on.  Node 0 is never marked: the root's proof lives in
//      pad[0] of GuidedRoot / GuidedWideRoot (GuidedProofEncode: 0 unproven, else value + 2).  No record grows.
//   2. the rule at a node n over its legal actions (bits of n.state.m; GuidedProofAdd / Merge / Value): if some legal a
//      has a child proven +1 for n's mover, n is proven +1; otherwise, if every legal a has a child and all of them
//      are proven, n is proven with the maximum of their values for n's mover (-1, 0 or +1); otherwise n is unproven.
//   3. climb, in the answer stage of an advance, right after the statistics of a slot whose status was 1 have been
//      backed up along its path (wide: slot by slot in slot order, after that slot's backup).  The path entries from
//      the last to the first, c = the node below the entry (the next entry's node; the pending leaf for the last):
//      c unproven: stop.  Rule 2 at the entry's node n; n unproven: stop.  n is node 0: store the root's proof and
//      stop.  Otherwise mark n and go on.  A mark never changes once set: proofs are exact, and deriving one again
//      (another slot's path through a marked node) gives the same value.  Slots of status 0 never climb.  Rule 2 is
//      the wave's job: every lane reads (done, term0) of the children of the actions it owns, one reduction decides.
//   4. selection.  score / wscore are unchanged.  A pick skips every legal action whose child is proven -1 for the
//      node's mover (GuidedProofClosed) -- finished games, decided leaves and marked interior nodes alike; ties stay
//      "the lowest action".  A node that a descent reaches has such an action left, or it would have been marked and
//      the descent would have stopped above it -- with one exception: a node whose last open actions were closed by
//      EARLIER DESCENTS OF THE SAME LAUNCH of a wide session (they reached finished games below it; the climb comes
//      with the next advance), or by slots a device-form reroot dropped.  There the pick is over all legal actions, as
//      without the flag: it reaches a proven child, status 1, and the next answer stage marks the node.  The root that
//      runs out of actions is proven (rule 5).  A pick learns a child's proof from the child's two words.
//   5. proven root.  A root whose proof is set begins no further descent in this round: status 2 (plain), stage B
//      begins nothing (wide).  A normal end like count == C, no error; later advances change nothing for that root.
//   6. result.  visits and values are unchanged.  action (GuidedProofPlays): for a proven root the most visited legal
//      action whose child is proven with the root's proven value for the root's mover; for an unproven root the most
//      visited legal action whose child is not proven -1 for the root's mover (all legal actions if none is left: the
//      case of rule 4); the lowest on ties; -1 for a root that is over.
//   7. proof.  value int8 [k]: the root's proven value for its mover, -128 if unproven or over.  q int8 [k, A]: per
//      legal root action the proven value of its child for the root's mover, -128 if unproven, without a child or
//      illegal (solve()'s convention), and for a root that is over.  It can be read at any time; a session without
//      the flag gives -128 everywhere.
//   8. reroot.  The compaction is unchanged and marks in the kept subtree stay bit for bit.  A marked node that
//      becomes node 0 is reopened (GuidedTacticsReopen, with or without tactics).  Then rule 2 is applied once to the
//      new node 0 over its kept children and the root's proof is set accordingly; a fresh root (c < 0) and a root that
//      is over are unproven.  The new root is handed out at advance 0 as always and, if proven, then begins no
//      descent.
//   9. tactics.  With tactics = D the decided leaves have status 1 and so feed the climb at the next advance; without
//      it only finished games do.  The tactics stage itself is unchanged.
//  10. without the flag the kernels launched, their arguments, the layouts and every byte stay as they are.
// In one sentence: the session is the guided search of the game in which every position whose value follows from
// proven positions below it counts as finished with that value, and in which no one walks into a proven loss.
//
// There are no random numbers.  Only seat 0's value is stored, as in pgx_search.hip.h: the games are zero-sum.  Build
// without fast-math and with -ffp-contract=off.
#ifndef ENVPOOL_AMD_CSRC_PGX_GUIDED_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_GUIDED_HIP_H_

#include <cfloat>
#include <cmath>

#include "pgx_search.hip.h"

namespace epa {
namespace pgx {

enum GuidedStatus : int { kGuidedEvaluate = 0, kGuidedTerminal = 1, kGuidedIdle = 2 };
// the largest node capacity of a root: reroot's mark / remap table, one int32 per node, is at most 32 KiB of LDS
constexpr int kGuidedMaxNodes = 8192;

// One node in the session's memory.  The per-action arrays are action-major, so the loads of a wave's lanes (lane j:
// entries j and j + 64) are contiguous.  The State is written by one lane when the node is made and read by every
// lane afterwards; an edge entry is only ever read and written by the lane that owns its action.
template <int G>
struct alignas(16) GuidedNode {
  State s;
  int32_t term0;
  int32_t pad[3];
  int32_t child[SearchEdges<G>()];
  int32_t v[SearchEdges<G>()];
  float w0[SearchEdges<G>()];
  float p[SearchEdges<G>()];
};

// What the session keeps per root beside its nodes.  A path entry is node << 8 | action.
struct alignas(16) GuidedRoot {
  int32_t count;    // nodes made
  int32_t pending;  // the pending leaf
  int32_t status;   // GuidedStatus
  int32_t depth;    // entries of `path`
  int32_t over;     // the env was over at begin, or the root became over at a reroot
  int32_t broken;   // advance met a position that is no position of the game
  int32_t pad[2];
  int32_t path[kSearchMaxPath];
};

PGX_HD inline float GuidedClean(float x) { return (x >= 0.0f && x <= FLT_MAX) ? x : 0.0f; }
PGX_HD inline float GuidedCleanV(float x) { return (x >= -1.0f && x <= 1.0f) ? x : 0.0f; }

// score(node, a): `v`, `w0`, `p` the edge's, `total` = V, `sign` the node's
PGX_HD inline float GuidedScore(int v, float w0, float p, int total, int sign, float c_puct) {
  const float q = v > 0 ? ((float)sign * w0) / (float)v : 0.0f;
  const float u = (c_puct * p) * sqrtf((float)(total + 1));
  return q + u / (float)(1 + v);
}

// a fresh node's edge entry
template <int G>
PGX_HD inline void GuidedClearEdge(GuidedNode<G>& n, int a) {
  n.child[a] = -1;
  n.v[a] = 0;
  n.w0[a] = 0.0f;
  n.p[a] = 0.0f;
}

// a fresh root record
PGX_HD inline void GuidedClearRoot(GuidedRoot& r, bool over) {
  r.count = 1;
  r.pending = 0;
  r.status = over ? kGuidedIdle : kGuidedEvaluate;
  r.depth = 0;
  r.over = over ? 1 : 0;
  r.broken = 0;
}

// reroot, the reachability rule: a kept node's edge keeps its child.  `mark` has one entry per node, nonzero: kept.
PGX_HD inline void GuidedRerootReach(int32_t* mark, int child) {
  if (child >= 0) mark[child] = 1;
}
// reroot, the rank: the new index of a node, given how many nodes of a lower index are kept; -1 for a dropped node
PGX_HD inline int GuidedRerootRank(int kept_below, bool kept) { return kept ? kept_below : -1; }
// reroot, one edge of a kept node: its child's new index out of the table of ranks
PGX_HD inline int GuidedRerootEdge(const int32_t* rank, int child) { return child >= 0 ? rank[child] : -1; }
// the root record after a reroot; `over`: the root is idle from now on
PGX_HD inline void GuidedRerootRoot(GuidedRoot& r, int count, bool over) {
  r.count = count;
  r.pending = 0;
  r.status = over ? kGuidedIdle : kGuidedEvaluate;
  r.depth = 0;
  r.over = over ? 1 : 0;
  r.broken = 0;
}

// ---- wide sessions: several leaves per root per launch ----
constexpr int kGuidedMaxWidth = 32;

// One slot of a wide root: what GuidedRoot keeps once.  A path entry is node << 8 | action.
struct alignas(16) GuidedWideSlot {
  int32_t pending;
  int32_t status;  // GuidedStatus
  int32_t depth;   // entries of `path`
  int32_t pad;
  int32_t path[kSearchMaxPath];
};
// What a wide session keeps per root beside its nodes: this header, then its W slots.
struct alignas(16) GuidedWideRoot {
  int32_t count;   // nodes made
  int32_t done;    // simulations completed in this round
  int32_t over;    // the env was over at begin, or the root became over at a reroot
  int32_t broken;  // advance met a position that is no position of the game
  int32_t live;    // slots whose status is not 2 (for the host forms' reroot check)
  int32_t pad[3];
};
PGX_HD inline size_t GuidedWideRootBytes(int width) {
  return sizeof(GuidedWideRoot) + (size_t)width * sizeof(GuidedWideSlot);
}
PGX_HD inline GuidedWideRoot& GuidedWideRootAt(void* roots, int row, int width) {
  return *reinterpret_cast<GuidedWideRoot*>(static_cast<char*>(roots) + (size_t)row * GuidedWideRootBytes(width));
}
PGX_HD inline GuidedWideSlot* GuidedWideSlots(GuidedWideRoot& r) { return reinterpret_cast<GuidedWideSlot*>(&r + 1); }

// wscore(node, a): `v`, `w0`, `p` the edge's, `o` its virtual losses, `total` = V (visits and virtual losses)
PGX_HD inline float GuidedWideScore(int v, float w0, float p, int o, int total, int sign, float c_puct) {
  const int n = v + o;
  const float q = n > 0 ? ((float)sign * w0 - (float)o) / (float)n : 0.0f;
  const float u = (c_puct * p) * sqrtf((float)(total + 1));
  return q + u / (float)(1 + n);
}
// whether path entry `e` of an earlier slot with `depth` entries, read at depth d, runs through `node`
PGX_HD inline bool GuidedWideOn(int e, int depth, int d, int node) { return d < depth && (e >> 8) == node; }

// a wide root record at begin and after a reroot: slot 0 holds the root, the others are idle
PGX_HD inline void GuidedWideClearRoot(GuidedWideRoot& r, int width, int count, bool over) {
  r.count = count;
  r.done = 0;
  r.over = over ? 1 : 0;
  r.broken = 0;
  r.live = over ? 0 : 1;
  GuidedWideSlot* sl = GuidedWideSlots(r);
  for (int j = 0; j < width; ++j) {
    sl[j].pending = 0;
    sl[j].status = (j == 0 && !over) ? kGuidedEvaluate : kGuidedIdle;
    sl[j].depth = 0;
  }
}

// ---- exact leaf status: tactics = D ----
constexpr int kGuidedMaxTactics = 16;              // the largest horizon D
constexpr long long kGuidedMaxTacticsNodes = 1 << 20;  // the largest M
constexpr int kGuidedDecided = 2;                  // State.done of a decided node (1: the game ended by a step)

// rule 1: a slot's leaf goes to the solver
PGX_HD inline bool GuidedTacticsLooksAt(int status, int pending) { return status == kGuidedEvaluate && pending != 0; }
// rule 2: what the solver said decides the leaf (solve_status: SolveStatus of pgx_solve.hip.h, 0 = solved)
PGX_HD inline bool GuidedTacticsDecides(int solve_status, int value) { return solve_status == 0 && value != 0; }
// rule 3: the node of a decided leaf; v is its value for the seat that moves there
template <int G>
PGX_HD inline void GuidedTacticsMark(GuidedNode<G>& leaf, int v) {
  leaf.term0 = SearchSign<G>(leaf.s) * v;
  leaf.s.done = kGuidedDecided;
}
// rule 5: the position of a node that becomes the root; true: it was decided and runs on now
PGX_HD inline bool GuidedTacticsReopen(State& s) {
  if (s.done != kGuidedDecided) return false;
  s.done = 0;
  return true;
}

// ---- proven values: the flag kGuidedProve ----
constexpr int kGuidedProve = 1;       // the flags word of begin
constexpr int kGuidedUnproven = -128;  // "no proven value" in proof's arrays and in the pieces below

// rule 1: the value of a node (its State.done and term0) for a mover of `sign`
PGX_HD inline int GuidedProofOf(int done, int term0, int sign) { return done != 0 ? sign * term0 : kGuidedUnproven; }
// rule 2 over a node's legal actions: the largest proven child value and the legal actions without a proven child
struct GuidedProofAcc {
  int best;
  int open;
};
PGX_HD inline GuidedProofAcc GuidedProofNone() { return GuidedProofAcc{kGuidedUnproven, 0}; }
// one legal action, cv: its child's value for the node's mover, kGuidedUnproven without a proven child
PGX_HD inline GuidedProofAcc GuidedProofAdd(GuidedProofAcc x, int cv) {
  return GuidedProofAcc{cv > x.best ? cv : x.best, x.open + (cv == kGuidedUnproven ? 1 : 0)};
}
PGX_HD inline GuidedProofAcc GuidedProofMerge(GuidedProofAcc x, GuidedProofAcc y) {
  return GuidedProofAcc{y.best > x.best ? y.best : x.best, x.open + y.open};
}
PGX_HD inline int GuidedProofValue(GuidedProofAcc x) {
  if (x.best == 1) return 1;
  return x.open == 0 ? x.best : kGuidedUnproven;  // (no legal action: best is kGuidedUnproven)
}
// rule 1: the root's proof in its record's pad word
PGX_HD inline int GuidedProofEncode(int v) { return v == kGuidedUnproven ? 0 : v + 2; }
PGX_HD inline int GuidedProofDecode(int word) { return word >= 1 && word <= 3 ? word - 2 : kGuidedUnproven; }
// rule 4: a pick skips the action of a child of this value
PGX_HD inline bool GuidedProofClosed(int cv) { return cv == -1; }
// rule 6: whether a legal root action whose child has value cv takes part in the result's pick
PGX_HD inline bool GuidedProofPlays(int root_proof, int cv) {
  return root_proof != kGuidedUnproven ? cv == root_proof : !GuidedProofClosed(cv);
}

// bytes of one emitted obs row: the mover's [H, W, C] block of the kObs key
template <int G>
PGX_HD constexpr int GuidedObsElems() {
  return Dims<G>::H * Dims<G>::W * Dims<G>::C;
}
// byte `e` of the emitted obs row of the position in `v` (only v.s is read), mover = SearchMover<G>(v.s)
template <int G>
PGX_HD inline uint32_t GuidedObsElem(const View& v, int mover, int e) {
  return Elem<G>(v, kObs, mover * GuidedObsElems<G>() + e);
}
template <int G>
PGX_HD inline uint32_t GuidedMaskElem(const View& v, int e) {
  return Elem<G>(v, kMask, e);
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_GUIDED_HIP_H_
