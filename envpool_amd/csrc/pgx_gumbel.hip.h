// PGX Gumbel search: the guided-search session of pgx_guided.hip.h with a second selection policy -- Gumbel top-m
// sampling with sequential halving at the root, a deterministic rule inside the tree and the improved policy
// softmax(logits + sigma(completed Q)) as the result's training target (Danihelka et al., "Policy improvement by
// planning with Gumbel", ICLR 2022) -- as __host__ __device__ pieces shared by the stepwise kernels (PgxGumbelBegin /
// PgxGumbelAdvance / PgxGumbelResult in pgx.hip, one wave per root) and the g++ host harness of the tests
// (tests/cpu_harness/pgx_gumbel_host.cpp, which walks a wave's lanes as loops).  This header is the authority: nothing
// here is pinned to another implementation's floating point.
//
// The contract (DESIGN.md "PGX Gumbel search").  S = simulations, m = max considered actions (1 .. A; the engine
// takes a larger one as A), A = Dims<G>::A.
// Inputs: gumbel[k, A] at begin (a non-finite entry counts as 0; all zeros is the noise-free evaluation mode); per
// advance logits[k, A] (cleanl: non-finite or |x| > 1e30 counts as 0) and values[k] (GuidedCleanV).  Entries of illegal
// actions are never read by a pick.  c_visit, c_scale: finite and >= 0.
// A node holds its State, term0, `raw` -- the caller's value of the node as seat 0's value, sign(node) * cleanv(value);
// (float)term0 for a finished node -- and per action a: child[a], v[a], w0[a] as in guided search, logit[a] and p[a].
// p is the softmax of the node's logits over its legal actions, floored at FLT_MIN, fixed when the logits arrive:
//     lmax = max over legal b of logit[b];  e[a] = exp_(logit[a] - lmax);  p[a] = max(e[a] / SUM(e), FLT_MIN)
// Per node, over its legal actions a, sign = SearchSign, all float32, in this order, nothing fused:
//     N = sum of v[a] (int);  vmax = max of v[a] (int);  sraw = (float)sign * raw
//     q(a)   = ((float)sign * w0[a]) / (float)v[a]                                   (where v[a] > 0)
//     v_mix  = N == 0 ? sraw : (sraw + (float)N * (SUM_{v>0}(p[a] * q(a)) / SUM_{v>0}(p[a]))) / (float)(1 + N)
//     cq(a)  = v[a] > 0 ? q(a) : v_mix                                               (completed Q)
//     scale  = min((c_visit + (float)vmax) * c_scale, 1e30f)
//     sg(a)  = (scale * (cq(a) - min cq)) / max(max cq - min cq, 1e-8f)              (sigma)
//     pi'(a) = e'(a) / SUM(e'),  e'(a) = exp_((logit[a] + sg(a)) - max over legal b of (logit[b] + sg(b)))
//   interior pick (every node but the root):  argmax of pi'(a) - (float)v[a] / (float)(1 + N);  ties: the lowest a
//   root pick at simulation index t = N(root):
//     m_eff = min(m, number of legal root actions);  cv = GumbelConsideredVisit(m_eff, S, t)
//     argmax over legal a with v[a] == cv of  (gumbel[a] + (logit[a] - lmax)) + sg(a);  ties: the lowest a
//   No such action: the position is no position of the game; that root ends with status 2 (the kernel also sets the
//   pool's error word, the harness returns -3), as a running position without a legal action does in guided search.
// Expansion, terminal leaves, kSearchMaxPath, the backup (v += 1, w0 += val0 in float32, val0 = the pending leaf's
// raw), the statuses and the emitted leaves are those of pgx_guided.hip.h.  Call number 0 stores the root's logits
// and value; call S completes the search.
// Result: visits = the root's v;  values = the root's w0 times the root mover's sign;  action = the root pick rule
// with cv = vmax, the recommended move;  weights[k, A] = pi' of the root, 0 on illegal actions: the training target.
// action = -1 and zero rows for a root that was over at begin.
//
// Determinism: the kernel and the harness agree bit for bit, because
//  (a) exp_ is GumbelExp below: only correctly rounded float32 + - *, rintf and ldexpf, the argument clamped to
//      [-87, 0] (neither the device's expf nor the host's is used);
//  (b) every float SUM over actions has one order: lane j's partial is term(j) + term(j + 64) (a term that does not
//      take part is +0.0f), then a butterfly x += x[lane ^ w] for w = 32, 16, 8, 4, 2, 1 (GumbelWaveSum restates it for
//      the host).  Maxima, minima and integer sums are order-free;
//  (c) every float operation is written out in order and the build uses -ffp-contract=off and no fast-math.
//
// A level per launch (batch sessions; DESIGN.md "PGX Gumbel search: a level per launch").  A LEVEL is the run of
// consecutive simulations with the same considered visit count cv.  All simulations of a level go through different
// root actions, so their descents live in disjoint subtrees: they cannot collide, need no virtual loss, and their
// interior picks do not see each other.  A batch session makes up to B = batch (1 .. kGumbelMaxBatch) of them in one
// launch.  Every root has B SLOTS, each what the plain session keeps once per root (pending node, status, path); row
// i * B + j of every leaf and answer array is slot j of root i.  The root rule differs from the plain session's, which
// re-scores the root before every simulation: a launch scores the root once and takes its actions together.
//   begin_batch(gumbel, ids, S, m, B, c_visit, c_scale):
//     as begin.  Slot 0 = {pending 0, path [], status: env over ? 2 : 0}.  Slots 1..B-1 status 2.
//   advance(logits, values), call number 0 .. S:
//     A. answers.  Slots j = 0..B-1 in this order, status_j != 2, L = pending_j:
//          status 0: L.logit / L.p / L.raw from row (i, j) exactly as the plain advance stores them; val0 = L.raw
//          status 1: val0 = (float) L.term0
//          backup along path_j in path order (v += 1, w0 += val0 in float32).  status_j = 2; path_j = []
//     B. t = N(root) after A (the sum of the root's v over legal actions).
//        If t >= S, or the root is over or broken: nothing more.
//        m_eff = min(m, legal root actions);  cv = GumbelConsideredVisit(m_eff, S, t)
//        r = GumbelLevelLeft(m_eff, S, t): the number of t' in t .. S-1 with GumbelConsideredVisit(m_eff, S, t') == cv
//        b = min(B, r)
//        Evaluate the root ONCE (the sigma of the tree as it stands after A).
//        score(a) = GumbelRootScore(gumbel[a], logit[a], lmax, sg(a)).
//        chosen = the b legal actions with v[a] == cv of the largest score, ties: the lowest a, in that order.
//        Fewer than b such actions: take those there are.  None: the root is broken (the error word, -3; every slot
//        ends with status 2 and the root begins no further descent).
//        Descents j = 0 .. len(chosen)-1 in that order:
//          path = [(0, chosen[j])], then the plain session's loop below the root (interior pick, expand or step down,
//          stop at a finished game or kSearchMaxPath).  Node indices are handed out in slot order.
//        Slot j = {pending, path, status 0 or 1}.  The other slots keep status 2.
//     emit: every slot's row.  Rows of status 1 or 2 are zeros.
//   result: the plain Gumbel result.  One row per root, not per slot.
// Consequences:
//   - B = 1 is the plain session, call for call, bit for bit: b = 1 and the one chosen action is the plain root pick
//   - the status-0 and status-1 slots of one launch belong to pairwise different root actions and their paths share no
//     node but the root: backup order changes no float (slot order is the stated order all the same)
//   - a descent makes at most one node, so count <= S + 1 and the node memory per root is that of the plain session
//   - while t < S every advance completes at least one simulation; a round is complete -- all k B statuses 2 -- after
//     exactly 1 + SUM over the levels of ceil(level size / B) advances, at most S + 1.  Later advances, up to call
//     number S, change nothing; a call number above S is refused
//   - after a complete round the root's visits sum to S and their sorted counts are the plain session's for the same
//     (m_eff, S), whatever the evaluator
//   - with an evaluator whose values are all 0 and no simulation reaching a finished game, sigma is 0 at every node
//     and the root order is fixed: the results equal the plain session's for every B, bit for bit, node for node
//   - with other values the result differs from the plain session's: sigma does not move inside a launch
#ifndef ENVPOOL_AMD_CSRC_PGX_GUMBEL_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_GUMBEL_HIP_H_

#include <cfloat>
#include <cmath>

#include "pgx_guided.hip.h"

namespace epa {
namespace pgx {

constexpr float kGumbelBig = 1e30f;  // the largest magnitude of a logit and of sigma's scale

// A node in the session's memory: GuidedNode's layout with `raw` in the header's padding and the logits behind w0.
template <int G>
struct alignas(16) GumbelNode {
  State s;
  int32_t term0;
  float raw;
  int32_t pad[2];
  int32_t child[SearchEdges<G>()];
  int32_t v[SearchEdges<G>()];
  float w0[SearchEdges<G>()];
  float logit[SearchEdges<G>()];
  float p[SearchEdges<G>()];
};

// What the session keeps per root beside its nodes: GuidedRoot and the root's cleaned Gumbel noise (action-major).
template <int G>
struct alignas(16) GumbelRoot {
  GuidedRoot r;
  float gumbel[SearchEdges<G>()];
};

PGX_HD inline float GumbelCleanLogit(float x) { return (x >= -kGumbelBig && x <= kGumbelBig) ? x : 0.0f; }
PGX_HD inline float GumbelCleanNoise(float x) { return (x >= -FLT_MAX && x <= FLT_MAX) ? x : 0.0f; }

// exp(x) for x clamped to [-87, 0]: Cody-Waite reduction with a two-word ln 2 whose high word has 9 significant bits
// (k * hi is exact for |k| <= 126), a degree-6 Taylor polynomial in Horner form on |r| <= 0.35, scaling by ldexpf.
// Every result is a normal number: exp(-87) = 1.6e-38 > FLT_MIN.
PGX_HD inline float GumbelExp(float x) {
  x = x < -87.0f ? -87.0f : x;
  x = x > 0.0f ? 0.0f : x;  // (a NaN cannot come in: every argument is a difference of finite numbers)
  const float k = rintf(x * 1.44269504f);
  const float r = (x - k * 0.693359375f) - k * -2.12194440e-4f;
  float p = 1.0f / 720.0f;
  p = p * r + 1.0f / 120.0f;
  p = p * r + 1.0f / 24.0f;
  p = p * r + 1.0f / 6.0f;
  p = p * r + 0.5f;
  p = p * r + 1.0f;
  p = p * r + 1.0f;
  return ldexpf(p, (int)k);
}

// mctx's table of considered visits, walked in integers: the visit count an action must have to be picked at
// simulation t of S when m actions are considered (sequential halving: every phase visits each of its c actions e
// times, then halves c).
PGX_HD inline int GumbelConsideredVisit(int m, int S, int t) {
  if (m <= 1) return t;
  int l = 0;
  while ((1 << l) < m) ++l;
  int c = m, vis = 0;
  for (;;) {
    int e = S / (l * c);
    e = e < 1 ? 1 : e;
    if (t < e * c) return vis + t / c;
    t -= e * c;
    vis += e;
    c = c / 2 < 2 ? 2 : c / 2;
  }
}

// What is left of the level of simulation t (t < S): the number of t' in t .. S-1 whose considered visit count is that
// of t.  The same walk of the table.
PGX_HD inline int GumbelLevelLeft(int m, int S, int t) {
  const int to_end = S - t;
  if (m <= 1) return to_end < 1 ? to_end : 1;  // (cv = t: every simulation is a level of its own)
  int l = 0;
  while ((1 << l) < m) ++l;
  int c = m;
  for (;;) {
    int e = S / (l * c);
    e = e < 1 ? 1 : e;
    if (t < e * c) {
      const int left = c - t % c;
      return left < to_end ? left : to_end;
    }
    t -= e * c;
    c = c / 2 < 2 ? 2 : c / 2;
  }
}

// ---- batch sessions: a level per launch ----
constexpr int kGumbelMaxBatch = kGuidedMaxWidth;

// What a batch session keeps per root beside its nodes: this record, then its B slots (GuidedWideSlot).
template <int G>
struct alignas(16) GumbelBatchRoot {
  int32_t count;   // nodes made
  int32_t over;    // the env was over at begin
  int32_t broken;  // advance met a position that is no position of the game
  int32_t live;    // slots whose status is not 2
  float gumbel[SearchEdges<G>()];
};
template <int G>
PGX_HD inline size_t GumbelBatchRootBytes(int batch) {
  return sizeof(GumbelBatchRoot<G>) + (size_t)batch * sizeof(GuidedWideSlot);
}
template <int G>
PGX_HD inline GumbelBatchRoot<G>& GumbelBatchRootAt(void* roots, int row, int batch) {
  char* at = static_cast<char*>(roots) + (size_t)row * GumbelBatchRootBytes<G>(batch);
  return *reinterpret_cast<GumbelBatchRoot<G>*>(at);
}
template <int G>
PGX_HD inline GuidedWideSlot* GumbelBatchSlots(GumbelBatchRoot<G>& r) {
  return reinterpret_cast<GuidedWideSlot*>(&r + 1);
}
// a batch root record at begin (the noise row apart): slot 0 holds the root, the others are idle
template <int G>
PGX_HD inline void GumbelBatchClearRoot(GumbelBatchRoot<G>& r, int batch, bool over) {
  r.count = 1;
  r.over = over ? 1 : 0;
  r.broken = 0;
  r.live = over ? 0 : 1;
  GuidedWideSlot* sl = GumbelBatchSlots(r);
  for (int j = 0; j < batch; ++j) {
    sl[j].pending = 0;
    sl[j].status = (j == 0 && !over) ? kGuidedEvaluate : kGuidedIdle;
    sl[j].depth = 0;
  }
}

PGX_HD inline float GumbelQ(int v, float w0, int sign) { return ((float)sign * w0) / (float)v; }
PGX_HD inline float GumbelMix(float raw, int sign, int total, float sum_pq, float sum_p) {
  const float sraw = (float)sign * raw;
  if (total == 0) return sraw;
  return (sraw + (float)total * (sum_pq / sum_p)) / (float)(1 + total);
}
PGX_HD inline float GumbelScale(float c_visit, float c_scale, int vmax) {
  const float s = (c_visit + (float)vmax) * c_scale;
  return s < kGumbelBig ? s : kGumbelBig;
}
PGX_HD inline float GumbelSigma(float scale, float cq, float cq_min, float cq_max) {
  const float range = cq_max - cq_min;
  return (scale * (cq - cq_min)) / (range > 1e-8f ? range : 1e-8f);
}
// p[a] of a node from e[a] = GumbelExp(logit[a] - lmax) and SUM(e)
PGX_HD inline float GumbelPrior(float e, float sum) {
  const float p = e / sum;
  return p > FLT_MIN ? p : FLT_MIN;
}
PGX_HD inline float GumbelInteriorScore(float pi, int v, int total) { return pi - (float)v / (float)(1 + total); }
PGX_HD inline float GumbelRootScore(float gumbel, float logit, float lmax, float sigma) {
  return (gumbel + (logit - lmax)) + sigma;
}

// (b) for the host: the wave's float SUM of the 64 lanes' partials, in the butterfly's order.  Every lane ends with
// the same bits (float addition is commutative), so lane 0's is returned.
inline float GumbelWaveSum(const float* part) {
  float x[kSearchWave], y[kSearchWave];
  for (int i = 0; i < kSearchWave; ++i) x[i] = part[i];
  for (int w = kSearchWave / 2; w >= 1; w >>= 1) {
    for (int i = 0; i < kSearchWave; ++i) y[i] = x[i] + x[i ^ w];
    for (int i = 0; i < kSearchWave; ++i) x[i] = y[i];
  }
  return x[0];
}

// a fresh node's edge entry, and its `raw`
template <int G>
PGX_HD inline void GumbelClearEdge(GumbelNode<G>& n, int a) {
  n.child[a] = -1;
  n.v[a] = 0;
  n.w0[a] = 0.0f;
  n.logit[a] = 0.0f;
  n.p[a] = 0.0f;
}
PGX_HD inline float GumbelFreshRaw(const State& s, int term0) { return s.done ? (float)term0 : 0.0f; }

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_GUMBEL_HIP_H_
