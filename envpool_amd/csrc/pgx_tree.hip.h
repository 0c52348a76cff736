// PGX tree search on the device: the wave-per-root building blocks that the kernels of pgx.hip share --
// PgxSearchKernel, the guided kernels (plain and wide), PgxGuidedReroot and the Gumbel kernels.  Device only: the arithmetic of the
// searches is in pgx_search.hip.h, pgx_guided.hip.h and pgx_gumbel.hip.h, which the host harnesses of the tests share;
// what is here is how a wave of 64 lanes walks, grows and updates a tree of their nodes.
//
// One wave per root, one block per wave.  Everything that steers the control flow -- the node, the picked action, the
// child, val0 -- is wave-uniform: it comes out of a butterfly reduction, a register broadcast or a load of one address,
// so every lane holds the same value and the loops need no divergence handling.
//   lane ownership  lane j owns actions j and j + 64 (Hex: two per lane; Othello's pass, action 64, is lane 0's second
//                   slot) of every node: it loads their edge entries (contiguous over the wave), scores them, and is
//                   the only lane that writes them -- at the node's making (MakeNode), at expansion (Expand: child),
//                   when priors arrive and in backup (Backup).  Edge statistics never pass between lanes through
//                   memory; the picked edge's child index reaches the other lanes by a register broadcast from its
//                   owner (OwnerChild).  ForOwned / ForSlots / ForLegal are the loop over a lane's slots.
//   hand-offs       a node's State and term0 are written by lane 0 and read by all lanes later: a hand-off between
//                   lanes through memory.  A wavefront-scope release fence (WaveRelease) follows such stores and an
//                   acquire fence (WaveAcquire) precedes the loads, so neither the compiler nor the memory pipeline
//                   reorders them.  The helpers here contain no fence: each kernel places its own pairs.
#ifndef ENVPOOL_AMD_CSRC_PGX_TREE_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_TREE_HIP_H_

#include <cfloat>
#include <cstdint>

#include "pgx_guided.hip.h"
#include "pgx_gumbel.hip.h"
#include "pgx_search.hip.h"

namespace epa {
namespace pgx {
namespace tree {

constexpr int kWave = kSearchWave;

__device__ __forceinline__ void WaveRelease() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); }
__device__ __forceinline__ void WaveAcquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

// f(j, act, owned) for every slot j of the lane: act = lane + 64 j, owned = act is an action of the game.  For the
// loops that also give the slot past the last action its neutral value.
template <int G, class F>
__device__ __forceinline__ void ForSlots(int lane, F f) {
#pragma unroll
  for (int j = 0; j < SearchSlotsPerLane<G>(); ++j) {
    const int act = lane + kWave * j;
    f(j, act, act < Dims<G>::A);
  }
}
// f(j, act) for the lane's own actions
template <int G, class F>
__device__ __forceinline__ void ForOwned(int lane, F f) {
#pragma unroll
  for (int j = 0; j < SearchSlotsPerLane<G>(); ++j) {
    const int act = lane + kWave * j;
    if (act < Dims<G>::A) f(j, act);
  }
}
// f(j, act) for the lane's own actions that are legal in a position with the legal-action set `m`
template <int G, class M, class F>
__device__ __forceinline__ void ForLegal(int lane, const M& m, F f) {
#pragma unroll
  for (int j = 0; j < SearchSlotsPerLane<G>(); ++j) {
    const int act = lane + kWave * j;
    if (act < Dims<G>::A && Has(m, act)) f(j, act);
  }
}

// The wave's butterfly (xor 32, 16, .. 1) of op(mine, theirs): every lane ends with the same value.  The order is part
// of the contract of the float sums (pgx_gumbel.hip.h), whose callers add a lane's two terms first.
template <class T, class Op>
__device__ __forceinline__ T WaveReduce(T x, Op op) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) x = op(x, __shfl_xor(x, m, kWave));
  return x;
}
template <class T>
__device__ __forceinline__ T WaveSum(T x) {
  return WaveReduce(x, [](T a, T o) { return a + o; });
}
template <class T>
__device__ __forceinline__ T WaveMax(T x) {
  return WaveReduce(x, [](T a, T o) { return o > a ? o : a; });
}
template <class T>
__device__ __forceinline__ T WaveMin(T x) {
  return WaveReduce(x, [](T a, T o) { return o < a ? o : a; });
}
// the wave's arg-max of SearchBetter (lowest action on ties)
__device__ __forceinline__ SearchPick WaveBest(SearchPick p) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    const SearchPick o{__shfl_xor(p.key, m, kWave), __shfl_xor(p.action, m, kWave), __shfl_xor(p.ok, m, kWave)};
    p = SearchBetter(p, o);
  }
  return p;
}
// the inclusive prefix sum over the wave's lanes
__device__ __forceinline__ int WaveScan(int x, int lane) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const int y = __shfl_up(x, m, kWave);
    if (lane >= m) x += y;
  }
  return x;
}

// The exponentials of a softmax over the wave's legal actions: ex[j] = GumbelExp(x[j] - max) on the lane's legal slots
// and 0 elsewhere (ex always has two entries); returns their sum (the lane's two terms first, then the butterfly).
// The caller divides, each in its own way.
template <int SL>
__device__ __forceinline__ float WaveSoftmax(const float* x, const bool* legal, float ex[2]) {
  float top = -FLT_MAX;
#pragma unroll
  for (int j = 0; j < SL; ++j) {
    if (legal[j]) top = x[j] > top ? x[j] : top;
  }
  top = WaveMax(top);
  ex[0] = ex[1] = 0.0f;
#pragma unroll
  for (int j = 0; j < SL; ++j) {
    if (legal[j]) ex[j] = GumbelExp(x[j] - top);
  }
  return WaveSum(ex[0] + ex[1]);
}

// the child of the picked edge `act` (wave-uniform), broadcast from the registers of its owner lane
template <int SL>
__device__ __forceinline__ int OwnerChild(const int* child, int act) {
  const int owner = act & (kWave - 1), slot = act / kWave;
  int c = __shfl(child[0], owner, kWave);
  if (SL > 1) {
    const int c1 = __shfl(child[SL - 1], owner, kWave);
    c = slot == 1 ? c1 : c;
  }
  return c;
}

// a fresh node's edge entry, by the node's type
template <int G>
__device__ __forceinline__ void ClearEdge(SearchNode<G>& n, int a) { SearchClearEdge<G>(n, a); }
template <int G>
__device__ __forceinline__ void ClearEdge(GuidedNode<G>& n, int a) { GuidedClearEdge<G>(n, a); }
template <int G>
__device__ __forceinline__ void ClearEdge(GumbelNode<G>& n, int a) { GumbelClearEdge<G>(n, a); }

struct NoExtra {
  template <class... T>
  __device__ __forceinline__ void operator()(T&&...) const {}
};

// A node's making: lane 0 stores its State and term0 -- and whatever else `lane0(node)` stores, a Gumbel node's raw or
// the root record at begin --, every lane clears its own edges.  The caller's release fence follows.
template <int G, class Node, class Lane0 = NoExtra>
__device__ __forceinline__ void MakeNode(Node& n, const State& s, int term0, int lane, Lane0 lane0 = {}) {
  if (lane == 0) {
    n.s = s;
    n.term0 = term0;
    lane0(n);
  }
  ForOwned<G>(lane, [&](int, int act) { ClearEdge<G>(n, act); });
}

// Expansion of edge `act` of nodes[node], whose position is `s`: the next node index is taken from `count`, the edge's
// owner lane stores it as the child, every lane runs the same pgx::Step on its copy of the State, and the node is made
// (MakeNode; lane0(node, its State, term0) for what else lane 0 stores).  Afterwards `node` and `s` are the new node's;
// returns its term0.  count < the root's capacity is the caller's to check.
template <int G, class Node, class Lane0 = NoExtra>
__device__ __forceinline__ int Expand(Node* nodes, int& node, State& s, int act, int& count, int lane,
                                      Lane0 lane0 = {}) {
  const int c = count++;
  if (lane == (act & (kWave - 1))) nodes[node].child[act] = c;
  State s2;
  const int term0 = SearchExpand<G>(s, act, s2);
  MakeNode<G>(nodes[c], s2, term0, lane, [&](Node& n) { lane0(n, s2, term0); });
  node = c;
  s = s2;
  return term0;
}

// Backup along `path` (entries node << 8 | action, read by every lane: wave-uniform): each pair's owner lane adds one
// visit and val0 (int or float, as the node's w0) to its edge.
template <class Node, class V>
__device__ __forceinline__ void Backup(Node* nodes, const int32_t* path, int depth, V val0, int lane) {
  for (int d = 0; d < depth; ++d) {
    const int p = path[d];
    const int act = p & 255;
    if ((act & (kWave - 1)) == lane) {
      Node& nd = nodes[p >> 8];
      nd.v[act] += 1;
      nd.w0[act] += val0;
    }
  }
}

// the lane's edges of a guided node for a PUCT pick (-1 / 0 past the last action); returns the lane's share of V
template <int G>
__device__ __forceinline__ int LoadPuctEdges(const GuidedNode<G>& nd, int lane, int* child, int* v, float* w0,
                                             float* pr) {
  int own = 0;
  ForSlots<G>(lane, [&](int j, int act, bool owned) {
    child[j] = -1;
    v[j] = 0;
    w0[j] = pr[j] = 0.0f;
    if (owned) {
      child[j] = nd.child[act];
      v[j] = nd.v[act];
      w0[j] = nd.w0[act];
      pr[j] = nd.p[act];
    }
    own += v[j];
  });
  return own;
}

// Proven values (pgx_guided.hip.h "Proven values") at the node whose legal-action set is `m`, whose mover has `sign`
// and whose child indices the lanes hold in child[] (LoadPuctEdges; -1 past the last action): cv[j] becomes the proven
// value of the child of the lane's slot j for that mover -- kGuidedUnproven for an illegal action, no child or an
// unproven one -- read from the child's two words.  Returns the lane's share of rule 2.  The children's State and term0
// were stored by lane 0: the caller's acquire fence precedes.
template <int G, class M>
__device__ __forceinline__ GuidedProofAcc ChildProofs(const GuidedNode<G>* nodes, int capacity, const int* child,
                                                      const M& m, int sign, int lane, int* cv) {
  GuidedProofAcc acc = GuidedProofNone();
  ForSlots<G>(lane, [&](int j, int act, bool owned) {
    cv[j] = kGuidedUnproven;
    if (owned && Has(m, act)) {
      if ((unsigned)child[j] < (unsigned)capacity) {
        const GuidedNode<G>& c = nodes[child[j]];
        cv[j] = GuidedProofOf(c.s.done, c.term0, sign);
      }
      acc = GuidedProofAdd(acc, cv[j]);
    }
  });
  return acc;
}
// rule 2 at that node: the wave's reduction of the lanes' shares gives its proven value (wave-uniform;
// kGuidedUnproven: none)
template <int G, class M>
__device__ __forceinline__ int WaveProof(const GuidedNode<G>* nodes, int capacity, const int* child, const M& m,
                                         int sign, int lane, int* cv) {
  GuidedProofAcc acc = ChildProofs<G>(nodes, capacity, child, m, sign, lane, cv);
  acc.best = WaveMax(acc.best);
  acc.open = WaveSum(acc.open);
  return GuidedProofValue(acc);
}
// the lane's child indices of a guided node (-1 past the last action), for WaveProof where no pick follows
template <int G>
__device__ __forceinline__ void LoadChildren(const GuidedNode<G>& nd, int lane, int* child) {
  ForSlots<G>(lane, [&](int j, int act, bool owned) { child[j] = owned ? nd.child[act] : -1; });
}

// The result rows of a root from its node n0 (position `root`): visits = v, vals = w0 times the root mover's sign (int
// or float, as the node's w0); zero rows when `zero` (a root that is over, or broken).  `column(j, act)` stores what
// else a policy gives per action.  Returns the most visited legal action (ties: the lowest), -1 without one or when
// `zero`.
template <int G, class Node, class W, class Column = NoExtra>
__device__ __forceinline__ int RootResult(const Node& n0, const State& root, bool zero, int lane, int32_t* visits,
                                          W* vals, Column column = {}) {
  const W sign = (W)SearchSign<G>(root);
  SearchPick mine = SearchNone();
  ForOwned<G>(lane, [&](int j, int act) {
    const int v = zero ? 0 : n0.v[act];
    visits[act] = v;
    vals[act] = zero ? (W)0 : sign * n0.w0[act];
    column(j, act);
    if (!zero && Has(root.m, act)) mine = SearchBetter(mine, SearchPick{(float)v, act, 1});
  });
  return WaveBest(mine).action;
}

// The root record of a guided session, plain (GuidedRoot, one leaf row per root) or wide (GuidedWideRoot with its
// slots, `width` leaf rows per root, the root's own in slot 0), for the kernels that serve both.
template <bool WIDE>
struct GuidedRec;
template <>
struct GuidedRec<false> {
  GuidedRoot& r;
  __device__ __forceinline__ GuidedRec(void* roots, int row, int /*width*/)
      : r(static_cast<GuidedRoot*>(roots)[row]) {}
  __device__ __forceinline__ int count() const { return r.count; }
  __device__ __forceinline__ bool over() const { return r.over != 0; }
  __device__ __forceinline__ bool idle() const { return r.over != 0 || r.broken != 0; }
  __device__ __forceinline__ int32_t& proof() const { return r.pad[0]; }  // proven values: GuidedProofEncode
  __device__ __forceinline__ void Clear(bool over) const { GuidedClearRoot(r, over); }                   // at begin
  __device__ __forceinline__ void Reset(int count, bool over) const { GuidedRerootRoot(r, count, over); }  // reroot
};
template <>
struct GuidedRec<true> {
  GuidedWideRoot& r;
  int width;
  __device__ __forceinline__ GuidedRec(void* roots, int row, int width_)
      : r(GuidedWideRootAt(roots, row, width_)), width(width_) {}
  __device__ __forceinline__ int count() const { return r.count; }
  __device__ __forceinline__ bool over() const { return r.over != 0; }
  __device__ __forceinline__ bool idle() const { return r.over != 0 || r.broken != 0; }
  __device__ __forceinline__ int32_t& proof() const { return r.pad[0]; }
  __device__ __forceinline__ void Clear(bool over) const { GuidedWideClearRoot(r, width, 1, over); }
  __device__ __forceinline__ void Reset(int count, bool over) const { GuidedWideClearRoot(r, width, count, over); }
};

// The root record of a Gumbel session, plain (GumbelRoot, one leaf row per root) or batch (GumbelBatchRoot with its
// slots, `batch` leaf rows per root, the root's own in slot 0), for the kernels that serve both.
template <int G, bool BATCH>
struct GumbelRec;
template <int G>
struct GumbelRec<G, false> {
  GumbelRoot<G>& r;
  __device__ __forceinline__ GumbelRec(void* roots, int row, int /*batch*/)
      : r(static_cast<GumbelRoot<G>*>(roots)[row]) {}
  __device__ __forceinline__ bool over() const { return r.r.over != 0; }
  __device__ __forceinline__ float* gumbel() const { return r.gumbel; }
  __device__ __forceinline__ void Clear(bool over) const { GuidedClearRoot(r.r, over); }  // at begin
};
template <int G>
struct GumbelRec<G, true> {
  GumbelBatchRoot<G>& r;
  int batch;
  __device__ __forceinline__ GumbelRec(void* roots, int row, int batch_)
      : r(GumbelBatchRootAt<G>(roots, row, batch_)), batch(batch_) {}
  __device__ __forceinline__ bool over() const { return r.over != 0; }
  __device__ __forceinline__ float* gumbel() const { return r.gumbel; }
  __device__ __forceinline__ void Clear(bool over) const { GumbelBatchClearRoot(r, batch, over); }
};

}  // namespace tree
}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_TREE_HIP_H_
