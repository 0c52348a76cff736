// PGX tree search: PUCT selection, expansion by pgx::Step and leaf evaluation by pgx::Playout for one root, as
// __host__ __device__ pieces shared by the search kernel (PgxSearchKernel in pgx.hip, one wave per root) and the g++
// host harness of the tests (tests/cpu_harness/pgx_search_host.cpp, which walks a wave's lanes as loops).
//
// The contract (DESIGN.md "PGX search").  S = simulations, R = leaf_playouts, e = the root's GLOBAL env id.
// A node holds its State, `term0` (seat 0's reward of the step that made the node) and per action a < A: child[a]
// (-1: none), v[a] (simulations through the edge), w0[a] (seat 0's summed playout returns through the edge); all
// int32.  Node 0 is the env's State; a root has at most S + 1 nodes.
//   simulation t = 0 .. S-1:
//     node = 0; path = []
//     loop:
//       if node.state.done:  val0 = R * node.term0; break
//       a = the legal action (bit of node.state.m) of the largest score(node, a); ties: the lowest a
//       path += (node, a)
//       if node.child[a] < 0:
//           s' = node.state; rw = Step<G>(s', a); c = new node {s', term0 = (int)rw.r[0]}; node.child[a] = c
//           if s'.done:  val0 = R * c.term0
//           else:        val0 = sum over r < R of (int)Playout<G>(s', false, PlayoutStream(seed, e, t * R + r),
//                                                                  PlayoutLimit(max_plies)).ret[0]
//           break
//       node = node.child[a]
//     for (n, a) in path:  n.v[a] += 1;  n.w0[a] += val0
//   score(node, a), float32, every operation correctly rounded, in this order, nothing fused:
//     V = sum over b of node.v[b];  sign = +1 if seat 0 moves at the node else -1  (the seat info:current_player reports)
//     q = node.v[a] > 0 ? (float)(sign * node.w0[a]) / (float)(node.v[a] * R) : 0.0f
//     score = q + (c_puct * sqrtf((float)V)) / (float)(1 + node.v[a])
// Results: visits = the root's v, returns = the root's w0 times the sign of the root's mover, action = the action with
// most visits (ties: the lowest).  The leaf playouts of a search are repeats 0 .. S*R-1 of playout(seed, env e), hence
// S * R <= kPlayoutMaxRepeats.
//
// Only seat 0's value is stored: legal play in the four games is zero-sum with step rewards 0 and +-1, so seat 1's
// return of every step and playout is the negative of seat 0's (the CPU test asserts it over every playout it uses),
// and the value sums are integers.  The only floating point is the score: one sqrtf, two divisions, one multiply, one
// add.  Build without fast-math and with -ffp-contract=off.
#ifndef ENVPOOL_AMD_CSRC_PGX_SEARCH_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_SEARCH_HIP_H_

#include <cmath>

#include "pgx_playout.hip.h"

namespace epa {
namespace pgx {

constexpr int kSearchMaxSimulations = 4096;
constexpr int kSearchMaxLeafPlayouts = 64;  // one leaf playout per lane of the root's wave
constexpr int kSearchWave = 64;
// (node, action) pairs of one simulation's path.  A path is a line of play from the root: at most 122 plies in Hex
// (121 cells and the swap), fewer in the other three games.
constexpr int kSearchMaxPath = 256;

// Lane j of the root's wave owns actions j and j + 64 of every node.
template <int G>
PGX_HD constexpr int SearchSlotsPerLane() {
  return Dims<G>::A > kSearchWave ? 2 : 1;
}
// entries of a node's per-action arrays: A rounded up to whole 16-byte words
template <int G>
PGX_HD constexpr int SearchEdges() {
  return (Dims<G>::A + 3) & ~3;
}

// One node in the tree scratch.  The three per-action arrays are action-major, so the loads of a wave's lanes (lane j:
// entries j and j + 64) are contiguous.  The State is written by one lane when the node is made and read by every
// lane afterwards; an edge entry is only ever read and written by the lane that owns its action.
template <int G>
struct alignas(16) SearchNode {
  State s;
  int32_t term0;
  int32_t pad[3];
  int32_t child[SearchEdges<G>()];
  int32_t v[SearchEdges<G>()];
  int32_t w0[SearchEdges<G>()];
};

// the seat that moves at `s`: what info:current_player reports
template <int G>
PGX_HD inline int SearchMover(const State& s) {
  return G == kHex ? HexCurrent(s) : s.cp;
}
template <int G>
PGX_HD inline int SearchSign(const State& s) {
  return SearchMover<G>(s) == 0 ? 1 : -1;
}

// score(node, a): `v`, `w0` the edge's, `total` = V, `sign` the node's
PGX_HD inline float SearchScore(int v, int w0, int total, int sign, int leaf_playouts, float c_puct) {
  const float q = v > 0 ? (float)(sign * w0) / (float)(v * leaf_playouts) : 0.0f;
  const float u = c_puct * sqrtf((float)total);
  return q + u / (float)(1 + v);
}

// A candidate of an arg-max with the lowest-index tie-break: `ok` (it takes part), its key, its action.
struct SearchPick {
  float key;
  int action;
  int ok;
};
PGX_HD inline SearchPick SearchNone() { return SearchPick{0.0f, -1, 0}; }
// the better of two candidates; commutative and associative, so a wave may reduce in any order
PGX_HD inline SearchPick SearchBetter(SearchPick x, SearchPick y) {
  if (!y.ok) return x;
  if (!x.ok) return y;
  if (x.key > y.key || (x.key == y.key && x.action < y.action)) return x;
  return y;
}

// expansion: the child position of `parent` after `action`, and its term0
template <int G>
PGX_HD inline int SearchExpand(const State& parent, int action, State& child) {
  child = parent;
  const Rewards rw = Step<G>(child, action);
  return (int)rw.r[0];
}

// leaf playout r < R of simulation t from the new node's position `s` (not over): seat 0's return
template <int G>
PGX_HD inline int SearchLeaf(const State& s, uint64_t seed, int env_id, int t, int leaf_playouts, int r, int limit) {
  State p = s;
  return (int)Playout<G>(p, false, PlayoutStream(seed, env_id, t * leaf_playouts + r), limit).ret[0];
}

// a fresh node's edge entry
template <int G>
PGX_HD inline void SearchClearEdge(SearchNode<G>& n, int a) {
  n.child[a] = -1;
  n.v[a] = 0;
  n.w0[a] = 0;
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_SEARCH_HIP_H_
