// PGX two-player board games (TicTacToe, ConnectFour, Hex, Othello): batched reset / step kernel, one env per
// lane, bit-exact with the reference.
//
// Replaces, for the whole batch in one launch, XxxEnv::{Reset,Step,WriteState} of envpool/pgx/board_games.h
// plus the runtime (async_envpool.h:118-132, env.h:184-256) of a pool with max_num_players = 2.  The env bodies
// are pgx_env.hip.h (shared with the host harness of the tests); one kernel instantiation per game.
//
// Data layout (HBM), see DESIGN.md "PGX":
//   state  pgx::State [N]   64 B per env, env-major: three 128-bit cell sets (stones, legal mask) + four words,
//                           read once and written once by the env's lane
//   mt     CommonDev, tiled (envs reset at their own times; one draw per reset)
// Outputs: every env writes 2 player rows, kept together as the [2, ...] block of its batch row (the reference's
// env-major player rows).  They are most of the traffic (Hex: 1.6 KB per env-step, obs 968 B of it), so a lane does
// not store its own row: it leaves its `View` (state + common keys, 96 B) in LDS, and then the block writes each
// key's section -- one contiguous range for the block's rows -- in 16-byte words, every thread computing the
// elements of its words from the views (pgx::Elem).  A wave's stores are then 1 KB contiguous instead of 64 rows
// apart.
// Render: pgx_render.hip.h painted by render_kernel.hip.h, one workgroup per band of a frame.
// Playout: pgx_playout.hip.h, one (env, repeat) per lane, the whole game in registers (PgxPlayoutKernel).
// Tree search, one wave per root: the kernels below are made of the building blocks of pgx_tree.hip.h (device only) --
// the loop over a lane's action slots (ForOwned / ForSlots / ForLegal), the wave butterflies (WaveReduce, WaveBest,
// WaveSoftmax), the child broadcast (OwnerChild), MakeNode / Expand / Backup, LoadPuctEdges, the result rows
// (RootResult) and the root record of a plain or a wide session (GuidedRec) -- over the arithmetic of the shared
// headers:
// Search: pgx_search.hip.h, the tree in the pool's side scratch (PgxSearchKernel).
// Guided search: pgx_guided.hip.h, one launch per simulation, the tree in the session's own memory between launches
// (PgxGuidedBegin / PgxGuidedAdvance / PgxGuidedResult), and PgxGuidedReroot, which keeps the played move's subtree for
// the next move by compacting it in place.  Wide sessions (PgxGuidedBegin / Result / Reroot with WIDE,
// PgxGuidedAdvanceWide) keep W slots per root and descend up to W times per launch, steered apart by virtual losses.
// Gumbel search: pgx_gumbel.hip.h, the same session with Gumbel root sampling, sequential halving and the improved
// policy as its result (PgxGumbelBegin / PgxGumbelAdvance / PgxGumbelResult).
// Exact solve: pgx_solve.hip.h, alpha-beta with the top of the tree in LDS and the lanes' stacks in the pool's side
// scratch (PgxSolveKernel).  Its traversal (SolveWave) also serves the exact leaf status of a guided session with
// tactics (PgxGuidedTactics, a launch behind every advance: a wave per slot solves the slot's new leaf).
// Self-play recorder: pgx_record.hip.h, finished games as training samples in the recorder's own memory (PgxRecordAdd /
// PgxRecordPlan / PgxRecordEmit).
// Self-play driver: pgx_selfplay.hip.h and pgx_dirichlet.hip.h; its kernels live in pgx_selfplay.hip, PgxPool only
// forwards the launches.
#include <algorithm>
#include <string>

#include "device_common.hip.h"
#include "engine.h"
#include "pgx_arena.hip.h"
#include "pgx_env.hip.h"
#include "pgx_guided.hip.h"
#include "pgx_gumbel.hip.h"
#include "pgx_playout.hip.h"
#include "pgx_record.hip.h"
#include "pgx_render.hip.h"
#include "pgx_search.hip.h"
#include "pgx_solve.hip.h"
#include "pgx_tree.hip.h"
#include "render_kernel.hip.h"

namespace epa {
namespace {

constexpr int kBlock = 256;
constexpr unsigned kErrState = 1;   // set_state words that are no position of the game
constexpr unsigned kErrSearch = 2;  // a search met a running position without a legal action, or a path past the cap
constexpr unsigned kErrGuided = 3;  // the same, met by a guided search
constexpr unsigned kErrGumbel = 4;  // the same, or a root without an action of the considered visit count (Gumbel)

// key K's section of rows [row0, row0 + nrows) of the launch, written by the whole block
template <int G, int K>
__device__ __forceinline__ void EmitKey(const OutPtrs& out, int row0, int nrows, const pgx::View* lv) {
  constexpr int re = pgx::RowElems<G>(K), eb = pgx::ElemBytes(K), per = 16 / eb;
  char* base = static_cast<char*>(out.p[K]) + (size_t)row0 * (re * eb);
  const int total = nrows * re;
  // head elements up to the first 16-byte boundary (a pipelined launch's second half may start anywhere)
  const int mis = (int)((uintptr_t)base & 15);
  const int head = std::min(total, mis == 0 ? 0 : (16 - mis) / eb);
  const int words = (total - head) / per;
  const int tail = head + words * per;
  auto one = [&](int i) {
    const int r = i / re;
    const uint32_t x = pgx::Elem<G>(lv[r], K, i - r * re);
    if (eb == 1) {
      base[i] = (char)x;
    } else {
      reinterpret_cast<uint32_t*>(base)[i] = x;
    }
  };
  for (int i = threadIdx.x; i < head; i += kBlock) one(i);
  for (int c = threadIdx.x; c < words; c += kBlock) {
    const int i0 = head + c * per;
    int r = i0 / re, e = i0 - r * re;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < per; ++j) {
      const uint32_t x = pgx::Elem<G>(lv[r], K, e);
      if (eb == 1) {
        w[j >> 2] |= (x & 0xffu) << (8 * (j & 3));
      } else {
        w[j] = x;
      }
      if (++e == re) {
        e = 0;
        ++r;
      }
    }
    *reinterpret_cast<uint4*>(base + (size_t)i0 * eb) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  for (int i = tail + threadIdx.x; i < total; i += kBlock) one(i);
}

template <int G, int... K>
__device__ __forceinline__ void EmitAll(const OutPtrs& out, int row0, int nrows, const pgx::View* lv,
                                        std::integer_sequence<int, K...>) {
  (EmitKey<G, K>(out, row0, nrows, lv), ...);
}

template <int G>
__global__ __launch_bounds__(kBlock) void PgxStepKernel(CommonDev cm, StepArgs a, pgx::State* st,
                                                        const int* __restrict__ action, OutPtrs out) {
  __shared__ pgx::View lv[kBlock];
  const int row0 = blockIdx.x * kBlock;
  const int row = row0 + threadIdx.x;
  if (row < a.k) {
    const int e = a.ids ? a.ids[row] - a.id_offset : row;
    pgx::State s = st[e];
    int cur = cm.cur_step[e];
    pgx::Rewards rw{{0.0f, 0.0f}};
    if (a.force_reset || cm.done[e] != 0) {  // async_envpool.h:127
      cur = 0;
      Mt19937 g(cm, e);
      pgx::Reset<G>(g, s);
      g.Commit();
    } else {
      ++cur;
      rw = pgx::Step<G>(s, action[row]);
    }
    st[e] = s;
    cm.done[e] = s.done ? 1 : 0;
    cm.cur_step[e] = cur;
    pgx::View v{};
    v.s = s;
    pgx::Finish(v, e + a.id_offset, cur, rw, a.max_episode_steps);
    lv[threadIdx.x] = v;
  }
  __syncthreads();
  if (row0 >= a.k) return;
  EmitAll<G>(out, row0, std::min(kBlock, a.k - row0), lv, std::make_integer_sequence<int, pgx::kNumKeys>());
}

// flat state per env: cur_step, done, then pgx::Hidden's words
template <int G>
__global__ void PgxGetState(CommonDev cm, const pgx::State* st, const int* ids, int k, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int e = ids[i];
  constexpr int W = pgx::HiddenWords<G>();
  double* o = out + (size_t)i * (2 + W);
  o[0] = cm.cur_step[e];
  o[1] = cm.done[e];
  int32_t w[W];
  pgx::Hidden<G>(st[e], w);
  for (int j = 0; j < W; ++j) o[2 + j] = w[j];
}

template <int G>
__global__ void PgxSetState(CommonDev cm, pgx::State* st, unsigned* err, const int* ids, int k, const double* in) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int e = ids[i];
  constexpr int W = pgx::HiddenWords<G>();
  const double* o = in + (size_t)i * (2 + W);
  int32_t w[W];
  for (int j = 0; j < W; ++j) w[j] = (int32_t)o[2 + j];
  pgx::State s{};
  bool done = o[1] != 0.0;
  if (!pgx::SetHidden<G>(s, w)) {
    *err = kErrState;
    done = true;  // such an env resets on its next step
  }
  s.done = done ? 1 : 0;
  st[e] = s;
  cm.cur_step[e] = (int)o[0];
  cm.done[e] = done ? 1 : 0;
}

// Random playouts (pgx_playout.hip.h): lane i plays repeat i % R of listed env i / R, so the repeats of one env sit
// in adjacent lanes -- they load the same 64-byte State (one sector for the group) and their games, from one position,
// are the likeliest to be of similar length -- and result i of each of the three arrays is lane i's, stored coalesced.
// No barrier, no memory traffic per ply and no LDS of its own (the compiler keeps Step's seat-indexed reward pairs in
// 16 bytes of LDS per lane): a block is one wave, which leaves its SIMD as soon as its own longest game is over.
// The loop is divergent per lane (a wave runs for its longest game, and Hex's flood fill for the lane with the
// largest group); lanes whose game is over idle until then.
// Commit (R == 1, ids that do not repeat: the engine checks both) also writes back what the plies' step launches
// would have: the State, done and cur_step.  An env that is over at the call -- cm.done, which an env before its first
// reset has set while its State is still all zeros -- plays nothing and is left as it is.
constexpr int kPlayoutBlock = 64;
static_assert(pgx::kPlayoutMaxPlies == EPA_PLAYOUT_MAX_PLIES && pgx::kPlayoutMaxRepeats == EPA_PLAYOUT_MAX_REPEATS,
              "the C ABI states the header's limits");

template <int G>
__global__ __launch_bounds__(kPlayoutBlock) void PgxPlayoutKernel(CommonDev cm, pgx::State* st,
                                                                  const int* __restrict__ ids, PlayoutArgs a,
                                                                  int id_offset) {
  const long long i = (long long)blockIdx.x * kPlayoutBlock + threadIdx.x;
  if (i >= (long long)a.k * a.repeats) return;
  const int row = (int)(i / a.repeats), r = (int)(i - (long long)row * a.repeats);
  const int e = ids[row];
  pgx::State s = st[e];
  const uint64_t h = pgx::PlayoutStream(a.seed, e + id_offset, r);
  const pgx::PlayoutResult res = pgx::Playout<G>(s, cm.done[e] != 0, h, pgx::PlayoutLimit(a.max_plies));
  reinterpret_cast<float2*>(a.returns)[i] = make_float2(res.ret[0], res.ret[1]);
  a.plies[i] = res.plies;
  a.status[i] = (unsigned char)res.status;
  if ((a.flags & EPA_PLAYOUT_COMMIT) != 0 && res.plies > 0) {
    st[e] = s;
    cm.done[e] = s.done ? 1 : 0;
    cm.cur_step[e] += res.plies;
  }
}

// Tree search (pgx_search.hip.h): one wave per root, one block per wave; block i searches listed env i in its own
// S + 1 nodes of the tree scratch.  The lane ownership, the wave-uniform control flow and the fences are those of
// pgx_tree.hip.h, whose helpers the kernel is made of:
//   selection       V is a wave integer sum (WaveSum), the pick a wave arg-max of pgx::SearchBetter (WaveBest), the
//                   child a register broadcast from the edge's owner (OwnerChild)
//   expansion       Expand: every lane runs the same pgx::Step on its copy of the node's State; lane 0 stores the new
//                   node's State and term0, every lane clears its own edges of it
//   leaf            lane r < R plays leaf playout r (the other 64 - R lanes idle); val0 is a wave integer sum
//   backup          the path's (node, action) pairs are kept in LDS by lane 0; Backup: each pair's owner lane adds to
//                   v, w0
// A wavefront-scope release fence follows the stores of an expansion and an acquire fence precedes the loads of a
// descent (the same pair brackets the path in LDS).
namespace tree = pgx::tree;
using tree::WaveAcquire;
using tree::WaveRelease;
constexpr int kSearchBlock = tree::kWave;
static_assert(pgx::kSearchMaxSimulations == EPA_SEARCH_MAX_SIMULATIONS &&
                  pgx::kSearchMaxLeafPlayouts == EPA_SEARCH_MAX_LEAF_PLAYOUTS &&
                  pgx::kGuidedMaxNodes == EPA_GUIDED_MAX_NODES,
              "the C ABI states the header's limits");

template <int G>
__global__ __launch_bounds__(kSearchBlock) void PgxSearchKernel(CommonDev cm, const pgx::State* st,
                                                                const int* __restrict__ ids, SearchArgs a,
                                                                int id_offset, unsigned* err) {
  constexpr int A = pgx::Dims<G>::A, SL = pgx::SearchSlotsPerLane<G>();
  using Node = pgx::SearchNode<G>;
  __shared__ int path[pgx::kSearchMaxPath];  // node << 8 | action
  const int row = blockIdx.x, lane = threadIdx.x;
  const int e = ids[row];
  const int S = a.simulations, R = a.leaf_playouts;
  const int limit = pgx::PlayoutLimit(a.max_plies);
  Node* nodes = static_cast<Node*>(a.nodes) + (size_t)row * (size_t)(S + 1);
  int32_t* visits = a.visits + (size_t)row * A;
  int32_t* returns = a.returns + (size_t)row * A;
  if (cm.done[e] != 0) {  // over at the call (an env before its first reset is)
    tree::ForOwned<G>(lane, [&](int, int act) { visits[act] = returns[act] = 0; });
    if (lane == 0) a.action[row] = -1;
    return;
  }
  const pgx::State root = st[e];
  tree::MakeNode<G>(nodes[0], root, 0, lane);
  WaveRelease();
  int count = 1;
  bool broken = false;
  for (int t = 0; t < S && !broken; ++t) {
    int node = 0, depth = 0, val0 = 0;
    for (;;) {
      WaveAcquire();
      Node& nd = nodes[node];
      pgx::State s = nd.s;
      if (s.done) {
        val0 = R * nd.term0;
        break;
      }
      int child[SL], v[SL], w0[SL];
      int own = 0;
      tree::ForSlots<G>(lane, [&](int j, int act, bool owned) {
        child[j] = -1;
        v[j] = w0[j] = 0;
        if (owned) {
          child[j] = nd.child[act];
          v[j] = nd.v[act];
          w0[j] = nd.w0[act];
        }
        own += v[j];
      });
      const int total = tree::WaveSum(own);
      const int sign = pgx::SearchSign<G>(s);
      pgx::SearchPick mine = pgx::SearchNone();
      // (tree::ForLegal written out: through the helper the backend lays this kernel's code out differently, and
      // Othello at one wave per SIMD, where nothing hides latency, measured 2.6 % slower)
#pragma unroll
      for (int j = 0; j < SL; ++j) {
        const int act = lane + kSearchBlock * j;
        if (act < A && pgx::Has(s.m, act)) {
          mine = pgx::SearchBetter(
              mine, pgx::SearchPick{pgx::SearchScore(v[j], w0[j], total, sign, R, a.c_puct), act, 1});
        }
      }
      const int act = tree::WaveBest(mine).action;
      // A running game has a legal action and a path is a line of play, far shorter than the LDS array: this is
      // unreachable from a position of the game.  A broken one is reported through the pool's error word, like
      // set_state's, and the root gives the rows of an env that is over (the host harness returns -3 here).
      if (act < 0 || depth >= pgx::kSearchMaxPath) {
        broken = true;
        break;
      }
      if (lane == 0) path[depth] = node << 8 | act;
      ++depth;
      const int c = tree::OwnerChild<SL>(child, act);
      if (c < 0) {
        const int term0 = tree::Expand<G>(nodes, node, s, act, count, lane);
        WaveRelease();
        if (s.done) {
          val0 = R * term0;
        } else {
          val0 = tree::WaveSum(lane < R ? pgx::SearchLeaf<G>(s, a.seed, e + id_offset, t, R, lane, limit) : 0);
        }
        break;
      }
      node = c;
    }
    WaveRelease();
    __syncthreads();
    WaveAcquire();
    tree::Backup(nodes, path, broken ? 0 : depth, val0, lane);
    __syncthreads();  // the path is read before the next simulation overwrites it
  }
  WaveAcquire();
  const int best = tree::RootResult<G>(nodes[0], root, broken, lane, visits, returns);
  if (lane == 0) {
    a.action[row] = best;
    if (broken) *err = kErrSearch;
  }
}

// Exact solve (pgx_solve.hip.h): one wave per root, one block per wave; block i solves listed env i.  The steps of the
// header's traversal, with every hand-off through LDS between two block barriers (a block is one wave, and the control
// flow around the barriers is wave-uniform: it depends on LDS words all lanes read, and on wave reductions):
//   top tree   SolveTop in LDS (19 KiB: 256 positions and 11 bytes of links and values per node).  Lane 0 lays a level
//              out (SolveTopPlan), the lanes make its positions, node hi + lane, + 64, .. (SolveTopMake)
//   lanes      SolveLaneSlice: the lane's node in registers, its stack in the side scratch -- word w of ply p of lane j
//              of root i at 16-byte word i * plies * 320 + (p * 5 + w) * 64 + j, plies = D or kSolveMaxDepth: a push
//              is five stores and a pop five loads of 1 KiB per wave, each in one piece
//   rounds     after a slice: `nodes` is a wave sum (WaveSum), the flags wave maxima; lane 0 runs SolveCombine
//   result     lane 0 writes the row (SolveRootResult)
// The loop of a slice is divergent per lane: a round lasts as long as its slowest lane's kSolveSlice positions, and
// lanes whose entries are done idle.  No floating point.
//   tables     TABLE (table_bits > 0): lane j's transposition table, 2^table_bits entries of 32 bytes at entry
//              (i * 64 + j) << table_bits of the table buffer, which the engine zeroed on the stream before the launch.
//              A lane loads and stores its own entries only (two 16-byte words each, a probe's two loads issued
//              together), in program order: no fence.  TABLE = false is the kernel without any of it.
constexpr unsigned kErrSolve = 5;  // a solve met a running position without a legal action
static_assert(pgx::kSolveMaxDepth == EPA_SOLVE_MAX_DEPTH, "the C ABI states the header's limits");
static_assert(pgx::kSolveMaxTableBits == EPA_SOLVE_MAX_TABLE_BITS, "the C ABI states the header's limits");

// what the traversal of one root came to: the positions visited, whether the root is given up, the broken flag
struct SolveOutcome {
  long long nodes;
  bool gave_up;
  int broken;
};

// The traversal for the block's root, shared by PgxSolveKernel and PgxGuidedTactics: the top tree, the rounds.  Every
// field of the outcome is wave-uniform.  A root that is not given up has every child of the root known after one more
// SolveCombine, which the caller's lane 0 runs (it has made every earlier LDS hand-off already).
template <int G, bool TABLE = false>
__device__ __forceinline__ SolveOutcome SolveWave(pgx::SolveTop& top, const pgx::State& root, pgx::SolveWord* stack,
                                                  int depth, long long max_nodes, int lane,
                                                  pgx::SolveWord* table = nullptr, int table_bits = 0) {
  const int limit = pgx::SolveLimit(depth);
  const bool hard = depth == 0;
  if (lane == 0) pgx::SolveTopInit(top, root);
  pgx::SolveFlags flags{0, root.m == 0 ? 1 : 0};
  long long count = 1;
  bool gave_up = pgx::SolveGaveUp(count, max_nodes, flags);
  __syncthreads();
  while (!gave_up) {  // the top tree
    if (lane == 0) pgx::SolveTopPlan(top);
    __syncthreads();
    const int hi = top.hi, next = top.next_n;
    if (next == top.n) break;
    for (int c = hi + lane; c < next; c += kSearchBlock) pgx::SolveTopMake<G>(top, c, limit, hard, flags);
    flags.overflow = tree::WaveMax(flags.overflow);
    flags.broken = tree::WaveMax(flags.broken);
    __syncthreads();
    if (lane == 0) pgx::SolveTopAdvance(top);
    __syncthreads();
    count = next;
    gave_up = pgx::SolveGaveUp(count, max_nodes, flags);
  }
  if (!gave_up) {
    if (lane == 0) pgx::SolveTopFrontier(top);
    __syncthreads();
    pgx::SolveLane l;
    pgx::SolveLaneInit(l, lane);
    for (;;) {  // the rounds
      if (tree::WaveMax(pgx::SolveLaneBusy(l, top) ? 1 : 0) == 0) break;
      pgx::SolveLaneSlice<G, TABLE>(l, top, stack, lane, pgx::kSolveSlice, limit, hard, table, table_bits);
      count = top.n + tree::WaveSum(l.visited);
      flags.overflow = tree::WaveMax(flags.overflow | l.flags.overflow);
      flags.broken = tree::WaveMax(flags.broken | l.flags.broken);
      gave_up = pgx::SolveGaveUp(count, max_nodes, flags);
      __syncthreads();
      if (gave_up) break;
      if (lane == 0) pgx::SolveCombine(top);
      __syncthreads();
    }
  }
  return SolveOutcome{count, gave_up, flags.broken};
}

template <int G, bool TABLE>
__global__ __launch_bounds__(kSearchBlock) void PgxSolveKernel(CommonDev cm, const pgx::State* st,
                                                               const int* __restrict__ ids, SolveArgs a,
                                                               unsigned* err) {
  constexpr int A = pgx::Dims<G>::A;
  __shared__ pgx::SolveTop top;
  const int row = blockIdx.x, lane = threadIdx.x;
  const int e = ids[row];
  int8_t* q = a.q + (size_t)row * A;
  if (cm.done[e] != 0) {  // over at the call (an env before its first reset is)
    if (lane == 0) {
      pgx::SolveNoResult<G>(q, a.value + row, a.action + row);
      a.status[row] = (uint8_t)pgx::kSolveOver;
      a.nodes[row] = 0;
    }
    return;
  }
  pgx::SolveWord* stack =
      reinterpret_cast<pgx::SolveWord*>(static_cast<char*>(a.stack) + (size_t)row * pgx::SolveStackBytes(a.depth));
  const pgx::State root = st[e];
  pgx::SolveWord* table = nullptr;  // the lane's own
  if (TABLE) {
    table = pgx::SolveLaneTable(reinterpret_cast<pgx::SolveWord*>(static_cast<char*>(a.table) +
                                                                  (size_t)row * pgx::SolveTableBytes(a.table_bits)),
                                lane, a.table_bits);
  }
  const SolveOutcome out = SolveWave<G, TABLE>(top, root, stack, a.depth, a.max_nodes, lane, table, a.table_bits);
  if (lane == 0) {
    a.nodes[row] = out.nodes;
    if (out.gave_up) {
      pgx::SolveNoResult<G>(q, a.value + row, a.action + row);
      a.status[row] = (uint8_t)pgx::kSolveGivenUp;
      if (out.broken) *err = kErrSolve;
    } else {
      pgx::SolveCombine(top);
      pgx::SolveRootResult<G>(top, q, a.value + row, a.action + row);
      a.status[row] = (uint8_t)pgx::kSolveSolved;
    }
  }
}

// Guided search (pgx_guided.hip.h): the search above cut into launches at every new leaf, so that the caller's model
// supplies the priors and the leaf value.  One wave per root, one block per wave; block i works on root i of the
// session: its GuidedRoot record and its nodes, which stay in the session's memory between launches.
//   lane ownership  as in pgx_tree.hip.h: lane j owns actions j and j + 64 of every node and is the only lane that
//                   writes their child / v / w0 / p -- at the node's making, when the priors arrive (GuidedAnswer), at
//                   expansion and in backup.  The priors row of the leaf is read coalesced by the owning lanes.
//   control flow    the status, the pending leaf, the picked action and the child are wave-uniform: they come out of a
//                   load of one address, a butterfly reduction or a register broadcast.
//   hand-offs       lane 0 stores a new node's State and term0 and the root record with its path; other lanes load
//                   them in a LATER launch.  Inside a launch the backup's owner lanes store v / w0 that the same lanes
//                   load in the descent.  Both sit between wavefront-scope release and acquire fences, so neither the
//                   compiler nor the memory pipeline reorders them.
//   leaves          the pending leaf's obs and mask rows are written by the whole wave from the leaf's State, which
//                   every lane holds in registers, in 16-byte words where the row's alignment allows (as EmitKey).
template <class F>
__device__ __forceinline__ void GuidedEmitRow(unsigned char* base, int total, int lane, F elem) {
  const int mis = (int)((uintptr_t)base & 15);
  const int head = std::min(total, mis == 0 ? 0 : 16 - mis);
  const int words = (total - head) / 16;
  const int tail = head + words * 16;
  for (int i = lane; i < head; i += kSearchBlock) base[i] = (unsigned char)elem(i);
  for (int c = lane; c < words; c += kSearchBlock) {
    const int i0 = head + c * 16;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j >> 2] |= (elem(i0 + j) & 0xffu) << (8 * (j & 3));
    *reinterpret_cast<uint4*>(base + i0) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  for (int i = tail + lane; i < total; i += kSearchBlock) base[i] = (unsigned char)elem(i);
}

// row `row` of the three leaf arrays: the position `s` for status 0, zeros otherwise
template <int G, class Args>
__device__ __forceinline__ void GuidedEmitLeaf(const Args& a, int row, int lane, int status, const pgx::State& s) {
  constexpr int A = pgx::Dims<G>::A, OB = pgx::GuidedObsElems<G>();
  pgx::View view{};
  view.s = s;
  const int mover = pgx::SearchMover<G>(s);
  const bool live = status == pgx::kGuidedEvaluate;
  GuidedEmitRow(a.obs + (size_t)row * OB, OB, lane,
                [&](int i) { return live ? pgx::GuidedObsElem<G>(view, mover, i) : 0u; });
  GuidedEmitRow(a.mask + (size_t)row * A, A, lane, [&](int i) { return live ? pgx::GuidedMaskElem<G>(view, i) : 0u; });
  if (lane == 0) a.status[row] = (unsigned char)status;
}

// rows `row` .. `row + n - 1` of the three leaf arrays, which are contiguous: idle slots of a wide session
template <int G, class Args>
__device__ __forceinline__ void GuidedEmitIdle(const Args& a, int row, int n, int lane) {
  constexpr int A = pgx::Dims<G>::A, OB = pgx::GuidedObsElems<G>();
  if (n <= 0) return;
  GuidedEmitRow(a.obs + (size_t)row * OB, n * OB, lane, [](int) { return 0u; });
  GuidedEmitRow(a.mask + (size_t)row * A, n * A, lane, [](int) { return 0u; });
  if (lane < n) a.status[row + lane] = (unsigned char)pgx::kGuidedIdle;
}

// the leaf rows of root `row` when its position `s` is handed out, at begin and after a reroot: the root's own row
// (idle when the root is over), and for a wide session (slot 0 holds the root) the idle rows of its other slots
template <int G, bool WIDE>
__device__ __forceinline__ void GuidedEmitRoot(const GuidedArgs& a, int row, int lane, bool over, const pgx::State& s) {
  const int W = WIDE ? a.width : 1;
  GuidedEmitLeaf<G>(a, row * W, lane, over ? pgx::kGuidedIdle : pgx::kGuidedEvaluate, s);
  if (WIDE) GuidedEmitIdle<G>(a, row * W + 1, W - 1, lane);
}

// The answer to a pending leaf (status 0 or 1): for status 0 its owner lanes store the caller's priors row `lrow` and
// the caller's value counts, for status 1 the finished game's term0.  Returns val0, seat 0's value of the leaf.
template <int G>
__device__ __forceinline__ float GuidedAnswer(const GuidedArgs& a, size_t lrow, pgx::GuidedNode<G>& leaf, int status,
                                              int lane) {
  if (status != pgx::kGuidedEvaluate) return (float)leaf.term0;
  tree::ForOwned<G>(lane, [&](int, int act) {
    leaf.p[act] = pgx::GuidedClean(a.priors[lrow * pgx::Dims<G>::A + act]);
  });
  return (float)pgx::SearchSign<G>(leaf.s) * pgx::GuidedCleanV(a.values[lrow]);
}

// Proven values (pgx_guided.hip.h "Proven values"), rule 3: the climb from a slot of status 1 whose statistics have
// just been backed up along `path`.  From the last entry up: the node below must be proven (one address: wave-uniform), rule
// 2 at the entry's node is the wave's (tree::WaveProof), and lane 0 marks a proven node other than node 0; the mark is
// a hand-off to the lanes that read it one entry higher, hence the fences.  Returns the root's proven value when the
// climb arrives there with one, pgx::kGuidedUnproven otherwise.
template <int G>
__device__ __forceinline__ int GuidedClimb(pgx::GuidedNode<G>* nodes, int capacity, const int32_t* path, int depth,
                                           int pending, int lane) {
  constexpr int SL = pgx::SearchSlotsPerLane<G>();
  int below = pending;
  for (int d = depth - 1; d >= 0; --d) {
    if ((unsigned)below >= (unsigned)capacity) break;  // (never)
    WaveAcquire();
    if (nodes[below].s.done == 0) break;
    const int n = path[d] >> 8;
    if ((unsigned)n >= (unsigned)capacity) break;  // (never)
    pgx::GuidedNode<G>& nd = nodes[n];
    const pgx::State s = nd.s;
    int child[SL], cv[SL];
    tree::LoadChildren<G>(nd, lane, child);
    const int v = tree::WaveProof<G>(nodes, capacity, child, s.m, pgx::SearchSign<G>(s), lane, cv);
    if (v == pgx::kGuidedUnproven) break;
    if (n == 0) return v;
    if (lane == 0) pgx::GuidedTacticsMark<G>(nd, v);
    WaveRelease();
    below = n;
  }
  return pgx::kGuidedUnproven;
}

// Rule 4: the pick among the lane's candidates `open` (the legal actions whose child is not proven -1 for the mover)
// and, only if the wave has none of those, among `all` legal actions.
__device__ __forceinline__ int GuidedProvePick(pgx::SearchPick open, pgx::SearchPick all) {
  const int act = tree::WaveBest(open).action;
  return act >= 0 ? act : tree::WaveBest(all).action;
}

// WIDE: a wide session (below): the record is pgx::GuidedWideRoot, the root goes to slot 0 (leaf row i * W), the other
// slots are idle and their rows zeros.
template <int G, bool WIDE>
__global__ __launch_bounds__(kSearchBlock) void PgxGuidedBegin(CommonDev cm, const pgx::State* st,
                                                               const int* __restrict__ ids, GuidedArgs a) {
  using Node = pgx::GuidedNode<G>;
  const int row = blockIdx.x, lane = threadIdx.x;
  const int e = ids[row];
  const bool over = cm.done[e] != 0;  // (an env before its first reset is)
  const pgx::State root = st[e];
  Node& n0 = static_cast<Node*>(a.nodes)[(size_t)row * (size_t)a.capacity];
  tree::MakeNode<G>(n0, root, 0, lane, [&](Node&) { tree::GuidedRec<WIDE>(a.roots, row, a.width).Clear(over); });
  WaveRelease();
  GuidedEmitRoot<G, WIDE>(a, row, lane, over, root);
}

// PROVE: a session with proven values (pgx_guided.hip.h "Proven values"): the climb after a status-1 answer, the pick
// that skips proven losses, no descent from a proven root.  The instantiations without it are the kernels as they were.
template <int G, bool PROVE = false>
__global__ __launch_bounds__(kSearchBlock) void PgxGuidedAdvance(GuidedArgs a, unsigned* err) {
  constexpr int SL = pgx::SearchSlotsPerLane<G>();
  using Node = pgx::GuidedNode<G>;
  const int row = blockIdx.x, lane = threadIdx.x;
  const int S = a.simulations;
  pgx::GuidedRoot& rec = static_cast<pgx::GuidedRoot*>(a.roots)[row];
  Node* nodes = static_cast<Node*>(a.nodes) + (size_t)row * (size_t)a.capacity;
  WaveAcquire();
  int status = rec.status;
  pgx::State s{};  // the pending leaf's position when the launch ends
  if (status != pgx::kGuidedIdle) {
    const float val0 = GuidedAnswer<G>(a, (size_t)row, nodes[rec.pending], status, lane);
    tree::Backup(nodes, rec.path, rec.depth, val0, lane);
    WaveRelease();
    int count = rec.count;
    bool proven = false;
    if constexpr (PROVE) {
      int proof = pgx::GuidedProofDecode(rec.pad[0]);
      if (status == pgx::kGuidedTerminal) {
        const int got =
            GuidedClimb<G>(nodes, a.capacity, rec.path, std::min(rec.depth, pgx::kSearchMaxPath), rec.pending, lane);
        if (got != pgx::kGuidedUnproven) {  // (a root proven before: the same value again)
          proof = got;
          if (lane == 0) rec.pad[0] = pgx::GuidedProofEncode(proof);
        }
      }
      proven = proof != pgx::kGuidedUnproven;
    }
    // the round's last call -- or the root's memory is used up (a rerooted tree may come to that): a normal end
    // (-- or, PROVE, the root is proven)
    if (a.call >= S || count >= a.capacity || proven) {
      status = pgx::kGuidedIdle;
      if (lane == 0) rec.status = status;
    } else {
      int node = 0, depth = 0;
      bool broken = false;
      WaveAcquire();
      s = nodes[0].s;
      for (;;) {
        int child[SL], v[SL];
        float w0[SL], pr[SL];
        const int total = tree::WaveSum(tree::LoadPuctEdges<G>(nodes[node], lane, child, v, w0, pr));
        const int sign = pgx::SearchSign<G>(s);
        pgx::SearchPick mine = pgx::SearchNone();
        int act;
        if constexpr (PROVE) {
          int cv[SL];
          tree::ChildProofs<G>(nodes, a.capacity, child, s.m, sign, lane, cv);
          pgx::SearchPick all = pgx::SearchNone();
          tree::ForLegal<G>(lane, s.m, [&](int j, int b) {
            const pgx::SearchPick p{pgx::GuidedScore(v[j], w0[j], pr[j], total, sign, a.c_puct), b, 1};
            all = pgx::SearchBetter(all, p);
            if (!pgx::GuidedProofClosed(cv[j])) mine = pgx::SearchBetter(mine, p);
          });
          act = GuidedProvePick(mine, all);
        } else {
          tree::ForLegal<G>(lane, s.m, [&](int j, int b) {
            mine = pgx::SearchBetter(
                mine, pgx::SearchPick{pgx::GuidedScore(v[j], w0[j], pr[j], total, sign, a.c_puct), b, 1});
          });
          act = tree::WaveBest(mine).action;
        }
        // unreachable from a position of the game (PgxSearchKernel): reported through the pool's error word
        if (act < 0 || depth >= pgx::kSearchMaxPath) {
          broken = true;
          break;
        }
        if (lane == 0) rec.path[depth] = node << 8 | act;
        ++depth;
        const int c = tree::OwnerChild<SL>(child, act);
        if (c < 0) {  // (count < capacity: checked before the descent, which makes one node at the most)
          tree::Expand<G>(nodes, node, s, act, count, lane);
          break;
        }
        node = c;
        WaveAcquire();
        s = nodes[node].s;
        if (s.done) break;
      }
      status = broken ? pgx::kGuidedIdle : s.done ? pgx::kGuidedTerminal : pgx::kGuidedEvaluate;
      if (lane == 0) {
        rec.count = count;
        rec.pending = node;
        rec.status = status;
        rec.depth = broken ? 0 : depth;
        if (broken) {
          rec.broken = 1;
          *err = kErrGuided;
        }
      }
    }
    WaveRelease();
  }
  GuidedEmitLeaf<G>(a, row, lane, status, s);
}

// (WIDE: the root record of a wide session; one row per root either way)
// (PROVE: proven values, rule 6: the action is picked among the actions that GuidedProofPlays admits)
template <int G, bool WIDE, bool PROVE = false>
__global__ __launch_bounds__(kSearchBlock) void PgxGuidedResult(GuidedArgs a) {
  constexpr int A = pgx::Dims<G>::A;
  using Node = pgx::GuidedNode<G>;
  const int row = blockIdx.x, lane = threadIdx.x;
  const Node& n0 = static_cast<const Node*>(a.nodes)[(size_t)row * (size_t)a.capacity];
  WaveAcquire();
  const bool over = tree::GuidedRec<WIDE>(a.roots, row, a.width).over();
  const pgx::State root = n0.s;
  int best = tree::RootResult<G>(n0, root, over, lane, a.visits + (size_t)row * A, a.vals + (size_t)row * A);
  if constexpr (PROVE) {
    if (!over) {
      constexpr int SL = pgx::SearchSlotsPerLane<G>();
      const int proof = pgx::GuidedProofDecode(tree::GuidedRec<WIDE>(a.roots, row, a.width).proof());
      int child[SL], cv[SL];
      tree::LoadChildren<G>(n0, lane, child);
      tree::ChildProofs<G>(&n0, a.capacity, child, root.m, pgx::SearchSign<G>(root), lane, cv);
      pgx::SearchPick mine = pgx::SearchNone();
      tree::ForLegal<G>(lane, root.m, [&](int j, int act) {
        if (!pgx::GuidedProofPlays(proof, cv[j])) return;
        mine = pgx::SearchBetter(mine, pgx::SearchPick{(float)n0.v[act], act, 1});
      });
      const int act = tree::WaveBest(mine).action;
      if (act >= 0) best = act;  // (none left: all legal actions, RootResult's pick)
    }
  }
  if (lane == 0) a.action[row] = best;  // (-1 without a legal action)
}

// Proven values, rule 7: the root's proven value and per legal root action its child's, for the root's mover.
template <int G, bool WIDE>
__global__ __launch_bounds__(kSearchBlock) void PgxGuidedProof(GuidedArgs a, signed char* value, signed char* q) {
  constexpr int A = pgx::Dims<G>::A, SL = pgx::SearchSlotsPerLane<G>();
  using Node = pgx::GuidedNode<G>;
  const int row = blockIdx.x, lane = threadIdx.x;
  const Node& n0 = static_cast<const Node*>(a.nodes)[(size_t)row * (size_t)a.capacity];
  WaveAcquire();
  const tree::GuidedRec<WIDE> rec(a.roots, row, a.width);
  const bool over = rec.over();
  const pgx::State root = n0.s;
  int child[SL], cv[SL];
  tree::LoadChildren<G>(n0, lane, child);
  tree::ChildProofs<G>(&n0, a.capacity, child, root.m, pgx::SearchSign<G>(root), lane, cv);
  tree::ForOwned<G>(lane, [&](int j, int act) {
    q[(size_t)row * A + act] = (signed char)(over ? pgx::kGuidedUnproven : cv[j]);
  });
  if (lane == 0) value[row] = (signed char)(over ? pgx::kGuidedUnproven : pgx::GuidedProofDecode(rec.proof()));
}

// reroot (pgx_guided.hip.h "Tree reuse"): the subtree under the played move becomes the tree, compacted in place.  One
// wave per root, one block per wave, the lane ownership of PgxGuidedAdvance: lane j is the only lane that reads or
// writes child / v / w0 / p of actions j and j + 64, in the source node and in the destination node; lane 0 moves
// State and term0 and writes the root record.
//   table          int32[capacity] in LDS, first the marks, then the ranks.  The array is static, in three sizes of
//                  512, 2048 and 8192 entries (2, 8 and 32 KiB; the launch takes the smallest that holds the session's
//                  capacity): with a dynamic array the backend keeps the per-lane homes of `Step`'s seat-indexed
//                  reward pairs in scratch instead of LDS
//   mark           the nodes in index order; whether node i is kept is one LDS word, so the branch is wave-uniform; the
//                  lanes of a kept node mark its children, whose indices are all above i
//   rank           64 nodes a trip: a lane's mark, an inclusive wave scan by register shifts (WaveScan), the carry of
//                  the trips before; the rank replaces the mark
//   copy           the nodes in index order again, kept ones only (wave-uniform); new index < old index, so a store
//                  lands on a slot that no later trip loads
// The table's hand-offs between lanes sit between wavefront-scope release and acquire fences with the block's barrier
// between them, as the path of PgxSearchKernel; so do the loads of what earlier launches stored and the stores that
// later launches load.
constexpr int kRerootTables[3] = {512, 2048, pgx::kGuidedMaxNodes};

// WIDE: a wide session (pgx_guided.hip.h "Several leaves per launch"): the record is pgx::GuidedWideRoot, the new root goes
// to slot 0 (leaf row i * W), the other slots become idle whatever they held, and their rows are zeros.
// PROVE: proven values, rule 8: rule 2 once at the new node 0 over its kept children; the root's proof is set anew.
template <int G, int CAP, bool WIDE, bool PROVE = false>
__global__ __launch_bounds__(kSearchBlock) void PgxGuidedReroot(GuidedArgs a) {
  constexpr int A = pgx::Dims<G>::A;
  using Node = pgx::GuidedNode<G>;
  __shared__ int32_t table[CAP];  // (a.capacity <= CAP)
  const int row = blockIdx.x, lane = threadIdx.x;
  const tree::GuidedRec<WIDE> rec(a.roots, row, a.width);
  Node* nodes = static_cast<Node*>(a.nodes) + (size_t)row * (size_t)a.capacity;
  WaveAcquire();
  const int act = a.actions[row];
  const int old_count = std::min(std::max(rec.count(), 1), std::min(a.capacity, CAP));  // (always 1 .. capacity)
  bool over = rec.idle() || act < 0 || act >= A;
  int count = old_count;
  int proof = pgx::kGuidedUnproven;
  pgx::State s = nodes[0].s;
  if (!over) {
    const int c = nodes[0].child[act];  // one address: wave-uniform
    if (c < 0 || c >= old_count) {      // (never >= count) a move the search did not try: a fresh tree on its position
      pgx::State s2;
      const int term0 = pgx::SearchExpand<G>(s, act, s2);
      tree::MakeNode<G>(nodes[0], s2, term0, lane);
      s = s2;
      count = 1;
    } else {
      s = nodes[c].s;  // (read before the copy below reuses the slot)
      for (int i = lane; i < old_count; i += kSearchBlock) table[i] = i == c ? 1 : 0;
      WaveRelease();
      __syncthreads();
      WaveAcquire();
      for (int i = c; i < old_count; ++i) {
        if (table[i] != 0) {
          tree::ForOwned<G>(lane, [&](int, int e) {
            const int ch = nodes[i].child[e];
            if (ch < old_count) pgx::GuidedRerootReach(table, ch);  // (never >= count)
          });
          WaveRelease();
          __syncthreads();
          WaveAcquire();
        }
      }
      int kept = 0;
      for (int base = 0; base < old_count; base += kSearchBlock) {
        const int i = base + lane;
        const int m = i < old_count && table[i] != 0 ? 1 : 0;
        const int upto = tree::WaveScan(m, lane);
        if (i < old_count) table[i] = pgx::GuidedRerootRank(kept + upto - m, m != 0);
        kept += __shfl(upto, kSearchBlock - 1, kSearchBlock);
      }
      WaveRelease();
      __syncthreads();
      WaveAcquire();
      for (int i = c; i < old_count; ++i) {
        const int dst = table[i];
        if (dst >= 0 && dst != i) {  // (dst < i: node 0 is never kept)
          const Node& from = nodes[i];
          Node& to = nodes[dst];
          if (lane == 0) {
            to.s = from.s;
            to.term0 = from.term0;
          }
          tree::ForOwned<G>(lane, [&](int, int e) {
            const int ch = from.child[e];
            to.child[e] = pgx::GuidedRerootEdge(table, ch < old_count ? ch : -1);
            to.v[e] = from.v[e];
            to.w0[e] = from.w0[e];
            to.p[e] = from.p[e];
          });
        }
      }
      count = kept;
      // exact leaf status, rule 5: a decided node that becomes the root runs on (lane 0 copied it to node 0 above)
      if (pgx::GuidedTacticsReopen(s) && lane == 0) nodes[0].s.done = 0;
      if constexpr (PROVE) {
        if (s.done == 0) {  // (the copies' State and term0 are lane 0's stores)
          constexpr int SL = pgx::SearchSlotsPerLane<G>();
          WaveRelease();
          __syncthreads();
          WaveAcquire();
          int child[SL], cv[SL];
          tree::LoadChildren<G>(nodes[0], lane, child);
          proof = tree::WaveProof<G>(nodes, std::min(count, a.capacity), child, s.m, pgx::SearchSign<G>(s), lane, cv);
        }
      }
    }
    over = s.done != 0;
  }
  if (lane == 0) {
    rec.Reset(count, over);
    if constexpr (PROVE) rec.proof() = pgx::GuidedProofEncode(proof);
  }
  WaveRelease();
  GuidedEmitRoot<G, WIDE>(a, row, lane, over, s);
}

// Several leaves per launch (pgx_guided.hip.h "Several leaves per launch"): PgxGuidedAdvance for a session whose roots
// have W slots (PgxGuidedBegin<G, true> begins it).  One wave per root, one block per wave, the lane ownership and the
// fences of PgxGuidedAdvance.
//   phase A    the slots in order: the owner lanes store the slot's priors row (row i * W + j) and add along its path,
//              read from the root record (one address a load: wave-uniform), in slot order, then path order
//   phase B    up to W descents.  Lane i holds depth and pending leaf of slot i of THIS launch in registers, and the
//              slot's path is column i of `lpath` in LDS ([depth][WB], so the lanes' loads of one depth are contiguous);
//              lane 0 writes a path entry to LDS and to the record, and a release / barrier / acquire separates two
//              descents, as around `path` in PgxSearchKernel.  At depth d lane i < j loads path_i[d] -- one LDS load
//              for the wave -- and compares it with the wave-uniform node; the matches are a ballot, whose population
//              is the sum of o, and the owner lane of each matched action bumps its o from a register broadcast.  The
//              collision test is a ballot over the lanes' pending leaves.
//   nodes      a node made by an earlier descent of the launch can be reached by a later one (a finished game: status
//              1; a running one is the collision): its State goes from lane 0 to the wave through memory inside the
//              launch, between the same release and acquire fences as in PgxSearchKernel.
//   leaves     slot j's State is in registers when its descent ends: its rows are emitted then; the idle slots' rows
//              are zeroed in one sweep at the end.
// `lpath` is static, in three width buckets (WB = 4, 16, 32: 4, 16 and 32 KiB), for the reason given at kRerootTables.
constexpr int kWideBuckets[3] = {4, 16, pgx::kGuidedMaxWidth};

// PROVE: proven values, as in PgxGuidedAdvance: the climb after each status-1 slot's backup in phase A, the pick that
// skips proven losses, and no descent from a proven root.
template <int G, int WB, bool PROVE = false>
__global__ __launch_bounds__(kSearchBlock) void PgxGuidedAdvanceWide(GuidedArgs a, unsigned* err) {
  constexpr int SL = pgx::SearchSlotsPerLane<G>();
  using Node = pgx::GuidedNode<G>;
  __shared__ int32_t lpath[pgx::kSearchMaxPath * WB];  // [depth][slot]: node << 8 | action  (a.width <= WB)
  const int row = blockIdx.x, lane = threadIdx.x;
  const int S = a.simulations, W = std::min(a.width, WB);
  pgx::GuidedWideRoot& rec = pgx::GuidedWideRootAt(a.roots, row, a.width);
  pgx::GuidedWideSlot* slots = pgx::GuidedWideSlots(rec);
  Node* nodes = static_cast<Node*>(a.nodes) + (size_t)row * (size_t)a.capacity;
  WaveAcquire();
  int done = rec.done;
  int proof = pgx::kGuidedUnproven;
  if constexpr (PROVE) proof = pgx::GuidedProofDecode(rec.pad[0]);
  // A. the answers
  for (int j = 0; j < W; ++j) {
    const int status = slots[j].status;
    if (status == pgx::kGuidedIdle) continue;
    const float val0 = GuidedAnswer<G>(a, (size_t)row * W + j, nodes[slots[j].pending], status, lane);
    const int backed = std::min(slots[j].depth, pgx::kSearchMaxPath);
    tree::Backup(nodes, slots[j].path, backed, val0, lane);
    if (backed > 0) ++done;
    if constexpr (PROVE) {
      if (status == pgx::kGuidedTerminal) {  // (every such slot climbs, also under a root proven before)
        WaveRelease();
        const int got = GuidedClimb<G>(nodes, a.capacity, slots[j].path, backed, slots[j].pending, lane);
        if (got != pgx::kGuidedUnproven) {
          proof = got;
          if (lane == 0) rec.pad[0] = pgx::GuidedProofEncode(proof);
        }
      }
    }
  }
  WaveRelease();
  // B. the descents (PROVE: none from a proven root)
  int count = rec.count;
  const bool idle = rec.over != 0 || rec.broken != 0 || (PROVE && proof != pgx::kGuidedUnproven);
  int my_depth = 0, my_pend = -1;  // lane i: slot i of this launch; the pending leaf only with status 0
  int j = 0;
  bool broken = false;
  WaveAcquire();
  const pgx::State root = nodes[0].s;
  for (; j < W && !idle; ++j) {
    if (!(done + j < S && count < a.capacity)) break;
    int node = 0, depth = 0;
    bool collided = false;
    pgx::State s = root;
    for (;;) {
      int child[SL], v[SL], o[SL] = {};
      float w0[SL], pr[SL];
      const int own = tree::LoadPuctEdges<G>(nodes[node], lane, child, v, w0, pr);
      // the virtual losses: the earlier slots of this launch whose path runs through `node`
      int mine_e = -1;
      if (lane < j && depth < my_depth) mine_e = lpath[depth * WB + lane];
      const bool on = lane < j && pgx::GuidedWideOn(mine_e, my_depth, depth, node);
      unsigned long long mb = __ballot(on);
      const int osum = __popcll(mb);
      while (mb != 0) {
        const int i = __ffsll((long long)mb) - 1;
        mb &= mb - 1;
        const int ai = __shfl(mine_e, i, kSearchBlock) & 255;
        tree::ForSlots<G>(lane, [&](int q, int act, bool) {
          if (ai == act) o[q] += 1;
        });
      }
      const int total = tree::WaveSum(own) + osum;
      const int sign = pgx::SearchSign<G>(s);
      pgx::SearchPick mine = pgx::SearchNone();
      int act;
      if constexpr (PROVE) {
        int cv[SL];
        tree::ChildProofs<G>(nodes, a.capacity, child, s.m, sign, lane, cv);
        pgx::SearchPick all = pgx::SearchNone();
        tree::ForLegal<G>(lane, s.m, [&](int q, int b) {
          const pgx::SearchPick p{pgx::GuidedWideScore(v[q], w0[q], pr[q], o[q], total, sign, a.c_puct), b, 1};
          all = pgx::SearchBetter(all, p);
          if (!pgx::GuidedProofClosed(cv[q])) mine = pgx::SearchBetter(mine, p);
        });
        act = GuidedProvePick(mine, all);
      } else {
        tree::ForLegal<G>(lane, s.m, [&](int q, int b) {
          mine = pgx::SearchBetter(
              mine, pgx::SearchPick{pgx::GuidedWideScore(v[q], w0[q], pr[q], o[q], total, sign, a.c_puct), b, 1});
        });
        act = tree::WaveBest(mine).action;
      }
      if (act < 0 || depth >= pgx::kSearchMaxPath) {  // unreachable from a position of the game (PgxGuidedAdvance)
        broken = true;
        break;
      }
      if (lane == 0) {
        lpath[depth * WB + j] = node << 8 | act;
        slots[j].path[depth] = node << 8 | act;
      }
      ++depth;
      const int c = tree::OwnerChild<SL>(child, act);
      if (c < 0) {  // (count < capacity: checked before the descent, which makes one node at the most)
        tree::Expand<G>(nodes, node, s, act, count, lane);
        break;
      }
      node = c;
      WaveAcquire();
      s = nodes[node].s;
      if (s.done) break;
      if (__ballot(lane < j && my_pend == node) != 0) {
        collided = true;
        break;
      }
    }
    if (broken || collided) break;
    const int status = s.done ? pgx::kGuidedTerminal : pgx::kGuidedEvaluate;
    if (lane == 0) {
      slots[j].pending = node;
      slots[j].status = status;
      slots[j].depth = depth;
    }
    if (lane == j) {
      my_depth = depth;
      my_pend = status == pgx::kGuidedEvaluate ? node : -1;
    }
    GuidedEmitLeaf<G>(a, row * W + j, lane, status, s);
    WaveRelease();
    __syncthreads();
    WaveAcquire();
  }
  if (broken) j = 0;  // a broken position ends all slots of the root
  // the record: the answered slots and the slots without a descent are idle
  if (lane >= j && lane < W) {
    slots[lane].status = pgx::kGuidedIdle;
    slots[lane].depth = 0;
  }
  if (lane == 0) {
    rec.count = count;
    rec.done = done;
    rec.live = j;
    if (broken) {
      rec.broken = 1;
      *err = kErrGuided;
    }
  }
  WaveRelease();
  GuidedEmitIdle<G>(a, row * W + j, W - j, lane);
}

// Exact leaf status (pgx_guided.hip.h "Exact leaf status"): the solver stage of an advance of a session with
// tactics = D > 0, enqueued on the same stream right after PgxGuidedAdvance or PgxGuidedAdvanceWide, whose record
// stores it loads (the header's release / acquire rule between launches).  One wave per slot, one block per wave:
// block i * W + j looks at slot j of root i (W = 1 for a plain session) and returns at once unless rule 1 hands the
// slot's leaf to the solver.  Otherwise it is PgxSolveKernel's traversal (SolveWave) on the leaf's position with the
// slot's own stack out of the session's memory, and for a decided leaf lane 0 marks the node, sets the slot's status
// and bumps the root's counter (an atomic add: a root's slots are different blocks), and the wave zeroes the slot's
// obs and mask rows (GuidedEmitLeaf: 16-byte words where aligned).  Two slots of status 0 never share a node, so no
// two blocks write the same node or slot.  Every branch around a barrier depends on loads of one address or on
// SolveWave's wave-uniform outcome.
static_assert(pgx::kGuidedProve == EPA_GUIDED_PROVE && pgx::kGuidedUnproven == EPA_GUIDED_UNPROVEN,
              "the C ABI states the header's values");
static_assert(pgx::kGuidedMaxTactics == EPA_GUIDED_MAX_TACTICS &&
                  pgx::kGuidedMaxTacticsNodes == EPA_GUIDED_MAX_TACTICS_NODES,
              "the C ABI states the header's limits");
template <int G, bool WIDE>
__global__ __launch_bounds__(kSearchBlock) void PgxGuidedTactics(GuidedArgs a, TacticsArgs t) {
  using Node = pgx::GuidedNode<G>;
  __shared__ pgx::SolveTop top;
  const int W = WIDE ? a.width : 1;
  const int slot = blockIdx.x, row = slot / W, lane = threadIdx.x;
  int32_t* status_at;
  int32_t* pending_at;
  if (WIDE) {
    pgx::GuidedWideSlot& sl = pgx::GuidedWideSlots(pgx::GuidedWideRootAt(a.roots, row, a.width))[slot - row * W];
    status_at = &sl.status;
    pending_at = &sl.pending;
  } else {
    pgx::GuidedRoot& rec = static_cast<pgx::GuidedRoot*>(a.roots)[row];
    status_at = &rec.status;
    pending_at = &rec.pending;
  }
  WaveAcquire();
  const int pending = *pending_at;
  if (!pgx::GuidedTacticsLooksAt(*status_at, pending) || pending < 0 || pending >= a.capacity) return;
  Node& leaf = (static_cast<Node*>(a.nodes) + (size_t)row * (size_t)a.capacity)[pending];
  const pgx::State s = leaf.s;
  if (s.done) return;  // (never with status 0)
  pgx::SolveWord* stack =
      reinterpret_cast<pgx::SolveWord*>(static_cast<char*>(t.stack) + (size_t)slot * pgx::SolveStackBytes(t.depth));
  const SolveOutcome out = SolveWave<G>(top, s, stack, t.depth, t.max_nodes, lane);
  if (lane == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(t.nodes + row), (unsigned long long)out.nodes);
    if (!out.gave_up) pgx::SolveCombine(top);
  }
  if (out.gave_up) return;  // rule 2: everything stays as it was
  __syncthreads();
  const int v = top.val[0];  // the root's minimax value: every child is known
  if (!pgx::GuidedTacticsDecides(pgx::kSolveSolved, v == pgx::kSolveUnknown ? 0 : v)) return;
  if (lane == 0) {
    pgx::GuidedTacticsMark<G>(leaf, v);
    *status_at = pgx::kGuidedTerminal;
    atomicAdd(t.decided + row, 1);
  }
  WaveRelease();
  GuidedEmitLeaf<G>(a, slot, lane, pgx::kGuidedTerminal, s);
}

// Gumbel search (pgx_gumbel.hip.h): the session, lane ownership, hand-offs and leaves of the guided kernels above with
// another pick.  Where PUCT needs one integer sum and one arg-max per node, a node here costs these wave reductions,
// all register butterflies (tree::WaveReduce, no LDS), every result wave-uniform:
//   GumbelEval      N (int sum) and vmax (int max); SUM p q and SUM p over the visited edges (float, in the header's
//                   order: the lane's two terms added first, then the butterfly); min and max of the completed Q
//   GumbelImproved  max of logit + sigma, SUM of the exponentials (tree::WaveSoftmax)
//   the pick        an arg-max (interior); at the root the legal count (int sum), the largest logit and an arg-max
// and the leaf whose logits arrive costs a max and a float SUM for its p (WaveSoftmax again).  The table of considered
// visits is walked per root by every lane on wave-uniform integers (scalar work), not read from memory.

// a lane's edges of one node (slot j: action lane + 64 j) with what the picks need of the whole node
template <int G>
struct GumbelEdges {
  static constexpr int SL = pgx::SearchSlotsPerLane<G>();
  bool legal[SL];
  int child[SL], v[SL];
  float w0[SL], logit[SL], sigma[SL];
  int total, vmax;  // N and the largest v of the node
};

template <int G>
__device__ __forceinline__ void GumbelEval(const pgx::GumbelNode<G>& nd, const pgx::State& s, int lane, float c_visit,
                                           float c_scale, GumbelEdges<G>& e) {
  constexpr int SL = pgx::SearchSlotsPerLane<G>();
  const int sign = pgx::SearchSign<G>(s);
  float p[SL], q[SL];
  int own = 0, top = 0;
  tree::ForSlots<G>(lane, [&](int j, int act, bool owned) {
    e.legal[j] = owned && pgx::Has(s.m, act);
    e.child[j] = -1;
    e.v[j] = 0;
    e.w0[j] = e.logit[j] = p[j] = 0.0f;
    if (owned) {
      e.child[j] = nd.child[act];
      e.v[j] = nd.v[act];
      e.w0[j] = nd.w0[act];
      e.logit[j] = nd.logit[act];
      p[j] = nd.p[act];
    }
    if (e.legal[j]) {
      own += e.v[j];
      top = std::max(top, e.v[j]);
    }
  });
  e.total = tree::WaveSum(own);
  e.vmax = tree::WaveMax(top);
  float pq[2] = {0.0f, 0.0f}, pp[2] = {0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < SL; ++j) {
    const bool on = e.legal[j] && e.v[j] > 0;
    q[j] = on ? pgx::GumbelQ(e.v[j], e.w0[j], sign) : 0.0f;
    if (on) {
      pq[j] = p[j] * q[j];
      pp[j] = p[j];
    }
  }
  const float sum_pq = tree::WaveSum(pq[0] + pq[1]);
  const float sum_p = tree::WaveSum(pp[0] + pp[1]);
  const float mix = pgx::GumbelMix(nd.raw, sign, e.total, sum_pq, sum_p);
  float cq[SL], lo = FLT_MAX, hi = -FLT_MAX;
#pragma unroll
  for (int j = 0; j < SL; ++j) {
    cq[j] = e.v[j] > 0 ? q[j] : mix;
    if (e.legal[j]) {
      lo = cq[j] < lo ? cq[j] : lo;
      hi = cq[j] > hi ? cq[j] : hi;
    }
  }
  lo = tree::WaveMin(lo);
  hi = tree::WaveMax(hi);
  const float scale = pgx::GumbelScale(c_visit, c_scale, e.vmax);
#pragma unroll
  for (int j = 0; j < SL; ++j) e.sigma[j] = e.legal[j] ? pgx::GumbelSigma(scale, cq[j], lo, hi) : 0.0f;
}

// pi'(a) of the lane's edges: 0 on illegal actions
template <int G>
__device__ __forceinline__ void GumbelImproved(const GumbelEdges<G>& e, float* pi) {
  constexpr int SL = pgx::SearchSlotsPerLane<G>();
  float x[SL], ex[2];
#pragma unroll
  for (int j = 0; j < SL; ++j) x[j] = e.logit[j] + e.sigma[j];
  const float sum = tree::WaveSoftmax<SL>(x, e.legal, ex);
#pragma unroll
  for (int j = 0; j < SL; ++j) pi[j] = e.legal[j] ? ex[j] / sum : 0.0f;
}

// the root pick: `final` picks among the most visited actions (the result), otherwise among those of the considered
// visit count of simulation N(root); -1 without such an action
template <int G>
__device__ __forceinline__ int GumbelRootPick(const GumbelEdges<G>& e, const float* gumbel, int lane, int considered,
                                              int simulations, bool final) {
  constexpr int SL = pgx::SearchSlotsPerLane<G>();
  int legal = 0;
  float top = -FLT_MAX;
#pragma unroll
  for (int j = 0; j < SL; ++j) {
    if (e.legal[j]) {
      ++legal;
      top = e.logit[j] > top ? e.logit[j] : top;
    }
  }
  legal = tree::WaveSum(legal);
  top = tree::WaveMax(top);
  const int cv =
      final ? e.vmax : pgx::GumbelConsideredVisit(std::min(considered, legal), simulations, e.total);
  pgx::SearchPick mine = pgx::SearchNone();
  tree::ForOwned<G>(lane, [&](int j, int act) {
    if (e.legal[j] && e.v[j] == cv) {
      mine = pgx::SearchBetter(
          mine, pgx::SearchPick{pgx::GumbelRootScore(gumbel[act], e.logit[j], top, e.sigma[j]), act, 1});
    }
  });
  return tree::WaveBest(mine).action;
}
template <int G>
__device__ __forceinline__ int GumbelRootPick(const GumbelEdges<G>& e, const pgx::GumbelRoot<G>& rec, int lane,
                                              int considered, int simulations, bool final) {
  return GumbelRootPick<G>(e, rec.gumbel, lane, considered, simulations, final);
}

// BATCH: a batch session (below): the record is pgx::GumbelBatchRoot with its slots, the root goes to slot 0 (leaf row
// i * B), the other slots are idle and their rows zeros.
template <int G, bool BATCH>
__global__ __launch_bounds__(kSearchBlock) void PgxGumbelBegin(CommonDev cm, const pgx::State* st,
                                                               const int* __restrict__ ids, GumbelArgs a) {
  constexpr int A = pgx::Dims<G>::A;
  using Node = pgx::GumbelNode<G>;
  const int row = blockIdx.x, lane = threadIdx.x;
  const int e = ids[row];
  const bool over = cm.done[e] != 0;  // (an env before its first reset is)
  const pgx::State root = st[e];
  Node& n0 = static_cast<Node*>(a.nodes)[(size_t)row * (size_t)(a.simulations + 1)];
  const tree::GumbelRec<G, BATCH> rec(a.roots, row, a.batch);
  tree::MakeNode<G>(n0, root, 0, lane, [&](Node& n) {
    n.raw = 0.0f;
    rec.Clear(over);
  });
  tree::ForOwned<G>(lane, [&](int, int act) {
    rec.gumbel()[act] = pgx::GumbelCleanNoise(a.gumbel[(size_t)row * A + act]);
  });
  WaveRelease();
  const int B = BATCH ? a.batch : 1;
  GuidedEmitLeaf<G>(a, row * B, lane, over ? pgx::kGuidedIdle : pgx::kGuidedEvaluate, root);
  if (BATCH) GuidedEmitIdle<G>(a, row * B + 1, B - 1, lane);
}

template <int G>
__global__ __launch_bounds__(kSearchBlock) void PgxGumbelAdvance(GumbelArgs a, unsigned* err) {
  constexpr int A = pgx::Dims<G>::A, SL = pgx::SearchSlotsPerLane<G>();
  using Node = pgx::GumbelNode<G>;
  const int row = blockIdx.x, lane = threadIdx.x;
  const int S = a.simulations;
  pgx::GumbelRoot<G>& rec = static_cast<pgx::GumbelRoot<G>*>(a.roots)[row];
  Node* nodes = static_cast<Node*>(a.nodes) + (size_t)row * (size_t)(S + 1);
  WaveAcquire();
  int status = rec.r.status;
  pgx::State s{};  // the pending leaf's position when the launch ends
  if (status != pgx::kGuidedIdle) {
    Node& leaf = nodes[rec.r.pending];
    float val0;
    if (status == pgx::kGuidedEvaluate) {
      // the leaf's logits arrive: logit and p of its legal actions (illegal entries are not read), and its raw
      const pgx::State ls = leaf.s;
      float lg[SL], ex[2];
      bool legal[SL];
      tree::ForSlots<G>(lane, [&](int j, int act, bool owned) {
        legal[j] = owned && pgx::Has(ls.m, act);
        lg[j] = legal[j] ? pgx::GumbelCleanLogit(a.logits[(size_t)row * A + act]) : 0.0f;
      });
      const float sum = tree::WaveSoftmax<SL>(lg, legal, ex);
      tree::ForOwned<G>(lane, [&](int j, int act) {
        leaf.logit[act] = lg[j];
        leaf.p[act] = legal[j] ? pgx::GumbelPrior(ex[j], sum) : 0.0f;
      });
      val0 = (float)pgx::SearchSign<G>(ls) * pgx::GuidedCleanV(a.values[row]);
      if (lane == 0) leaf.raw = val0;
    } else {
      val0 = (float)leaf.term0;
    }
    tree::Backup(nodes, rec.r.path, rec.r.depth, val0, lane);
    WaveRelease();
    if (a.call >= S) {
      status = pgx::kGuidedIdle;
      if (lane == 0) rec.r.status = status;
    } else {
      int node = 0, depth = 0, count = rec.r.count;
      bool broken = false;
      WaveAcquire();
      s = nodes[0].s;
      for (;;) {
        GumbelEdges<G> e;
        GumbelEval<G>(nodes[node], s, lane, a.c_visit, a.c_scale, e);
        int act;
        if (node == 0) {
          act = GumbelRootPick<G>(e, rec, lane, a.considered, S, false);
        } else {
          float pi[SL];
          GumbelImproved<G>(e, pi);
          pgx::SearchPick mine = pgx::SearchNone();
          tree::ForSlots<G>(lane, [&](int j, int b, bool) {
            if (e.legal[j]) {
              mine = pgx::SearchBetter(mine,
                                       pgx::SearchPick{pgx::GumbelInteriorScore(pi[j], e.v[j], e.total), b, 1});
            }
          });
          act = tree::WaveBest(mine).action;
        }
        // unreachable from a position of the game (PgxSearchKernel): reported through the pool's error word
        if (act < 0 || depth >= pgx::kSearchMaxPath) {
          broken = true;
          break;
        }
        if (lane == 0) rec.r.path[depth] = node << 8 | act;
        ++depth;
        const int c = tree::OwnerChild<SL>(e.child, act);
        if (c < 0) {
          if (count > S) {  // (one node per call: never; the session's memory ends here)
            broken = true;
            break;
          }
          tree::Expand<G>(nodes, node, s, act, count, lane,
                          [](Node& n, const pgx::State& s2, int term0) { n.raw = pgx::GumbelFreshRaw(s2, term0); });
          break;
        }
        node = c;
        WaveAcquire();
        s = nodes[node].s;
        if (s.done) break;
      }
      status = broken ? pgx::kGuidedIdle : s.done ? pgx::kGuidedTerminal : pgx::kGuidedEvaluate;
      if (lane == 0) {
        rec.r.count = count;
        rec.r.pending = node;
        rec.r.status = status;
        rec.r.depth = broken ? 0 : depth;
        if (broken) *err = kErrGumbel;
      }
    }
    WaveRelease();
  }
  GuidedEmitLeaf<G>(a, row, lane, status, s);
}

// A level per launch (pgx_gumbel.hip.h "A level per launch"): PgxGumbelAdvance for a session whose roots have B slots
// (PgxGumbelBegin<G, true> begins it).  One wave per root, one block per wave, the lane ownership and the fences of
// PgxGumbelAdvance.
//   phase A    the slots in order: the owner lanes store the slot's logits row (row i * B + j) with its p, lane 0 its
//              raw, and the owner lanes add along its path, read from the record (one address a load: wave-uniform)
//   phase B    the root is evaluated once and each lane keeps the root scores of its actions in registers.  The b picks
//              are b arg-max butterflies; each masks the winner out at its owner lane.  Nothing is sorted in memory.
//              The descents run one after the other.  They go through different root actions, so none loads what
//              another stored: there is no path table in LDS, no collision test, no barrier between two descents.
//   leaves     slot j's State is in registers when its descent ends: its rows are emitted then; the idle slots' rows
//              are zeroed in one sweep at the end.
// GumbelAnswer and GumbelInteriorPick are what PgxGumbelAdvance does in line; that kernel keeps its text, so that its
// code object stays what it was.

// The answer to a pending leaf (status 0 or 1): for status 0 its owner lanes store the caller's logits row `lrow` and
// the p they give, lane 0 the leaf's raw; for status 1 the finished game's term0 counts.  Returns val0.
template <int G>
__device__ __forceinline__ float GumbelAnswer(const GumbelArgs& a, size_t lrow, pgx::GumbelNode<G>& leaf, int status,
                                              int lane) {
  constexpr int A = pgx::Dims<G>::A, SL = pgx::SearchSlotsPerLane<G>();
  if (status != pgx::kGuidedEvaluate) return (float)leaf.term0;
  const pgx::State ls = leaf.s;
  float lg[SL], ex[2];
  bool legal[SL];
  tree::ForSlots<G>(lane, [&](int j, int act, bool owned) {
    legal[j] = owned && pgx::Has(ls.m, act);
    lg[j] = legal[j] ? pgx::GumbelCleanLogit(a.logits[lrow * A + act]) : 0.0f;
  });
  const float sum = tree::WaveSoftmax<SL>(lg, legal, ex);
  tree::ForOwned<G>(lane, [&](int j, int act) {
    leaf.logit[act] = lg[j];
    leaf.p[act] = legal[j] ? pgx::GumbelPrior(ex[j], sum) : 0.0f;
  });
  const float val0 = (float)pgx::SearchSign<G>(ls) * pgx::GuidedCleanV(a.values[lrow]);
  if (lane == 0) leaf.raw = val0;
  return val0;
}

// the interior pick of an evaluated node; -1 without a legal action
template <int G>
__device__ __forceinline__ int GumbelInteriorPick(const GumbelEdges<G>& e, int lane) {
  float pi[pgx::SearchSlotsPerLane<G>()];
  GumbelImproved<G>(e, pi);
  pgx::SearchPick mine = pgx::SearchNone();
  tree::ForSlots<G>(lane, [&](int j, int b, bool) {
    if (e.legal[j]) {
      mine = pgx::SearchBetter(mine, pgx::SearchPick{pgx::GumbelInteriorScore(pi[j], e.v[j], e.total), b, 1});
    }
  });
  return tree::WaveBest(mine).action;
}

static_assert(pgx::kGumbelMaxBatch == EPA_GUMBEL_MAX_BATCH, "the C ABI states the header's limit");

template <int G>
__global__ __launch_bounds__(kSearchBlock) void PgxGumbelAdvanceBatch(GumbelArgs a, unsigned* err) {
  constexpr int SL = pgx::SearchSlotsPerLane<G>();
  using Node = pgx::GumbelNode<G>;
  const int row = blockIdx.x, lane = threadIdx.x;
  const int S = a.simulations, B = std::min(a.batch, pgx::kGumbelMaxBatch);
  pgx::GumbelBatchRoot<G>& rec = pgx::GumbelBatchRootAt<G>(a.roots, row, a.batch);
  pgx::GuidedWideSlot* slots = pgx::GumbelBatchSlots(rec);
  Node* nodes = static_cast<Node*>(a.nodes) + (size_t)row * (size_t)(S + 1);
  WaveAcquire();
  // A. the answers
  for (int j = 0; j < B; ++j) {
    const int status = slots[j].status;
    if (status == pgx::kGuidedIdle) continue;
    const float val0 = GumbelAnswer<G>(a, (size_t)row * B + j, nodes[slots[j].pending], status, lane);
    tree::Backup(nodes, slots[j].path, std::min(slots[j].depth, pgx::kSearchMaxPath), val0, lane);
  }
  WaveRelease();
  // B. the descents of what is left of the level
  int count = rec.count, j = 0;
  bool broken = false;
  if (rec.over == 0 && rec.broken == 0) {
    WaveAcquire();
    const pgx::State root = nodes[0].s;
    GumbelEdges<G> e0;
    GumbelEval<G>(nodes[0], root, lane, a.c_visit, a.c_scale, e0);
    if (e0.total < S) {
      int legal = 0;
      float top = -FLT_MAX;
#pragma unroll
      for (int q = 0; q < SL; ++q) {
        if (e0.legal[q]) {
          ++legal;
          top = e0.logit[q] > top ? e0.logit[q] : top;
        }
      }
      legal = tree::WaveSum(legal);
      top = tree::WaveMax(top);
      const int m_eff = std::min(a.considered, legal);
      const int cv = pgx::GumbelConsideredVisit(m_eff, S, e0.total);
      const int b = std::min(B, pgx::GumbelLevelLeft(m_eff, S, e0.total));
      float score[SL];
      bool cand[SL];
      tree::ForSlots<G>(lane, [&](int q, int act, bool) {
        cand[q] = e0.legal[q] && e0.v[q] == cv;
        score[q] = cand[q] ? pgx::GumbelRootScore(rec.gumbel[act], e0.logit[q], top, e0.sigma[q]) : 0.0f;
      });
      for (; j < b; ++j) {
        pgx::SearchPick mine = pgx::SearchNone();
        tree::ForSlots<G>(lane, [&](int q, int act, bool) {
          if (cand[q]) mine = pgx::SearchBetter(mine, pgx::SearchPick{score[q], act, 1});
        });
        int act = tree::WaveBest(mine).action;
        if (act < 0) {  // fewer than b actions of this visit count; none at all is no position of the game
          broken = j == 0;
          break;
        }
        tree::ForSlots<G>(lane, [&](int q, int mine_act, bool) {
          if (mine_act == act) cand[q] = false;
        });
        int node = 0, depth = 0;
        int c = tree::OwnerChild<SL>(e0.child, act);
        pgx::State s = root;
        for (;;) {
          if (lane == 0) slots[j].path[depth] = node << 8 | act;
          ++depth;
          if (c < 0) {
            if (count > S) {  // (one node per simulation: never; the session's memory ends here)
              broken = true;
              break;
            }
            tree::Expand<G>(nodes, node, s, act, count, lane,
                            [](Node& n, const pgx::State& s2, int term0) { n.raw = pgx::GumbelFreshRaw(s2, term0); });
            break;
          }
          node = c;
          WaveAcquire();
          s = nodes[node].s;
          if (s.done) break;
          GumbelEdges<G> e;
          GumbelEval<G>(nodes[node], s, lane, a.c_visit, a.c_scale, e);
          act = GumbelInteriorPick<G>(e, lane);
          // unreachable from a position of the game (PgxSearchKernel): reported through the pool's error word
          if (act < 0 || depth >= pgx::kSearchMaxPath) {
            broken = true;
            break;
          }
          c = tree::OwnerChild<SL>(e.child, act);
        }
        if (broken) break;
        const int status = s.done ? pgx::kGuidedTerminal : pgx::kGuidedEvaluate;
        if (lane == 0) {
          slots[j].pending = node;
          slots[j].status = status;
          slots[j].depth = depth;
        }
        GuidedEmitLeaf<G>(a, row * B + j, lane, status, s);
      }
    }
  }
  if (broken) j = 0;  // a broken position ends all slots of the root
  // the record: the answered slots and the slots without a descent are idle
  if (lane >= j && lane < B) {
    slots[lane].status = pgx::kGuidedIdle;
    slots[lane].depth = 0;
  }
  if (lane == 0) {
    rec.count = count;
    rec.live = j;
    if (broken) {
      rec.broken = 1;
      *err = kErrGumbel;
    }
  }
  WaveRelease();
  GuidedEmitIdle<G>(a, row * B + j, B - j, lane);
}

// (BATCH: the root record of a batch session; one row per root either way)
template <int G, bool BATCH>
__global__ __launch_bounds__(kSearchBlock) void PgxGumbelResult(GumbelArgs a) {
  constexpr int A = pgx::Dims<G>::A, SL = pgx::SearchSlotsPerLane<G>();
  using Node = pgx::GumbelNode<G>;
  const int row = blockIdx.x, lane = threadIdx.x;
  const tree::GumbelRec<G, BATCH> rec(a.roots, row, a.batch);
  const Node& n0 = static_cast<const Node*>(a.nodes)[(size_t)row * (size_t)(a.simulations + 1)];
  WaveAcquire();
  const bool over = rec.over();
  const pgx::State root = n0.s;
  GumbelEdges<G> e;
  GumbelEval<G>(n0, root, lane, a.c_visit, a.c_scale, e);
  float pi[SL];
  GumbelImproved<G>(e, pi);
  const int best = GumbelRootPick<G>(e, rec.gumbel(), lane, a.considered, a.simulations, true);
  // the rows of the guided result with the improved policy as a third column; the action is the root pick's
  tree::RootResult<G>(n0, root, over, lane, a.visits + (size_t)row * A, a.vals + (size_t)row * A,
                      [&](int j, int act) { a.weights[(size_t)row * A + act] = over ? 0.0f : pi[j]; });
  if (lane == 0) a.action[row] = over ? -1 : best;
}

// Self-play recorder (pgx_record.hip.h): three kernels over the recorder's own memory.
//   PgxRecordAdd   a block takes kRecordAddRows rows.  Its first threads decide, one per row, what becomes of the
//                  env's staging (RecordAddDecide), store n_e and the elapsed step and leave (env, slot) in LDS.  Then
//                  the whole block copies the staged rows in 16-byte words, one word per thread and trip: the four
//                  words of the State, then the policy row's (a staged policy row is padded to whole words and starts
//                  on a 16-byte boundary; the caller's row is read float by float, cleaned against the position's mask).
//                  No lane walks a row of its own.  The drop counters are integer atomics: their values do not depend
//                  on the order.
//   PgxRecordPlan  one block: the exclusive scan of the rows' sample counts in row order, in trips of the block size
//                  (a wave scan by shuffles, the waves' totals through LDS, a running carry), the fit decision per row,
//                  the new count and the counters.  All integer: the order is fixed by definition.  The row's thread
//                  also clears n_e and, for a written game, lists its plies as (row, ply) items: the emission's work,
//                  dense from 0 because the written games are a prefix of the finished ones.
//   PgxRecordEmit  one wave per staged ply of a written game: a fixed grid of kRecordEmitWaves waves strides over the
//                  item list (a wave per finished ROW walked a game's plies one after the other, and with few rows
//                  ending the launch lasted as long as the longest game on one SIMD).  No items: every wave returns
//                  at once.  The ply's State is wave-uniform in registers, and the wave writes the ply's nsym samples
//                  -- contiguous in each sample array -- as ONE run per array in 16-byte words (GuidedEmitRow for the
//                  bytes, RecordEmitWords for the policy), every element read through the inverse symmetry.  Lanes
//                  j < nsym write the scalars of sample j.  No floating-point arithmetic: policy and reward are moved.
static_assert(pgx::kRecordMaxPlies == EPA_RECORD_MAX_PLIES && pgx::kRecordDefaultPlies == EPA_RECORD_DEFAULT_PLIES &&
                  (unsigned long long)pgx::kRecordMaxBytes == EPA_RECORD_MAX_BYTES &&
                  (unsigned)pgx::kRecordSymmetries == EPA_RECORD_SYMMETRIES,
              "the C ABI states the header's limits");
constexpr int kRecordAddRows = 32;
constexpr int kRecordPlanBlock = 1024;
constexpr int kRecordEmitWaves = 4096;

template <int G>
__global__ __launch_bounds__(kBlock) void PgxRecordAdd(CommonDev cm, const pgx::State* __restrict__ st,
                                                       const int* __restrict__ ids, RecordArgs a) {
  constexpr int A = pgx::Dims<G>::A, PS = pgx::RecordPolicyStride<G>(), RW = 4 + PS / 4;
  __shared__ int env[kRecordAddRows], slot[kRecordAddRows];
  const int row0 = blockIdx.x * kRecordAddRows;
  const int nrows = std::min(kRecordAddRows, a.k - row0);
  if ((int)threadIdx.x < nrows) {
    const int e = ids[row0 + threadIdx.x];
    const int el = cm.cur_step[e], n = a.staged[e];
    const pgx::RecordAddPlan p = pgx::RecordAddDecide(cm.done[e] != 0, n, el, a.plies);
    unsigned long long* ctr = reinterpret_cast<unsigned long long*>(a.counters);
    if (p.drop_games != 0) atomicAdd(&ctr[2], (unsigned long long)p.drop_games);
    if (p.drop_plies != 0) atomicAdd(&ctr[3], (unsigned long long)p.drop_plies);
    if (p.slot >= 0) a.elapsed[(size_t)e * a.plies + p.slot] = el;
    if (p.staged != n) a.staged[e] = p.staged;
    env[threadIdx.x] = e;
    slot[threadIdx.x] = p.slot;
  }
  __syncthreads();
  for (int w = threadIdx.x; w < nrows * RW; w += kBlock) {
    const int r = w / RW, q = w - r * RW;
    if (slot[r] < 0) continue;
    const int e = env[r];
    const size_t dst = (size_t)e * a.plies + slot[r];
    if (q < 4) {
      reinterpret_cast<uint4*>(a.states)[dst * 4 + q] = reinterpret_cast<const uint4*>(st + e)[q];
      continue;
    }
    const int a0 = (q - 4) * 4;
    const pgx::u128 m = st[e].m;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.in_policy) + (size_t)(row0 + r) * A;
    uint32_t x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = a0 + j < A ? pgx::RecordClean(src[a0 + j], pgx::Has(m, a0 + j)) : 0u;
    reinterpret_cast<uint4*>(a.staged_policy + dst * PS)[q - 4] = make_uint4(x[0], x[1], x[2], x[3]);
  }
}

__global__ __launch_bounds__(kRecordPlanBlock) void PgxRecordPlan(const int* __restrict__ ids, RecordArgs a) {
  constexpr int kWaves = kRecordPlanBlock / 64;
  __shared__ int wave_sum[kWaves];
  __shared__ unsigned long long acc[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t < 4) acc[t] = 0;
  const long long base = *a.count;
  long long carry = 0;  // the samples of the rows of earlier trips (the same in every thread)
  unsigned long long mine[4] = {0, 0, 0, 0};  // samples, games, dropped_games, dropped_plies of this thread's rows
  __syncthreads();
  for (int row0 = 0; row0 < a.k; row0 += kRecordPlanBlock) {
    const int i = row0 + t;
    int n = 0, c = 0;
    if (i < a.k) {
      const int e = ids[i];
      const bool done = a.done[i] != 0;
      n = a.staged[e];
      c = pgx::RecordGameSamples(done, n, a.nsym);
      if (done && n != 0) a.staged[e] = 0;  // written or dropped: the env's staging is empty afterwards
    }
    int x = c;  // the wave's inclusive scan
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[wv] = x;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kWaves; ++w) {
      const int s = wave_sum[w];
      before += w < wv ? s : 0;
      total += s;
    }
    const long long off = carry + before + (x - c);
    if (i < a.k) {
      int code = pgx::kRecordNoGame;
      if (c > 0) {
        if (pgx::RecordFits(base, off, c, a.capacity)) {
          code = (int)(base + off);
          mine[0] += (unsigned long long)c;
          mine[1] += 1;
          // the emission's work list: one item per staged ply.  Every game in front of a written one is written, so
          // the call's items are dense from 0: this game's begin at off / nsym
          int2* item = reinterpret_cast<int2*>(a.items) + off / a.nsym;
          for (int p = 0; p < n; ++p) item[p] = make_int2(i, p);
        } else {
          code = pgx::kRecordDropped;
          mine[2] += 1;
          mine[3] += (unsigned long long)n;
        }
      }
      a.plan[i] = code;
    }
    carry += total;
    __syncthreads();  // (wave_sum is written again in the next trip)
  }
  for (int j = 0; j < 4; ++j) {
    if (mine[j] != 0) atomicAdd(&acc[j], mine[j]);
  }
  __syncthreads();
  if (t == 0) {
    *a.count = (int)(base + (long long)acc[0]);
    *a.n_items = (int)(acc[0] / (unsigned long long)a.nsym);
    for (int j = 0; j < 4; ++j) a.counters[j] += (long long)acc[j];
  }
}

// `total` 4-byte elements at `base` (4-byte aligned) by the wave, in 16-byte words where the alignment allows
template <class F>
__device__ __forceinline__ void RecordEmitWords(uint32_t* base, int total, int lane, F elem) {
  const int mis = (int)(((uintptr_t)base & 15) / 4);
  const int head = std::min(total, mis == 0 ? 0 : 4 - mis);
  const int words = (total - head) / 4;
  const int tail = head + words * 4;
  for (int i = lane; i < head; i += kSearchBlock) base[i] = elem(i);
  for (int c = lane; c < words; c += kSearchBlock) {
    const int i0 = head + c * 4;
    *reinterpret_cast<uint4*>(base + i0) = make_uint4(elem(i0), elem(i0 + 1), elem(i0 + 2), elem(i0 + 3));
  }
  for (int i = tail + lane; i < total; i += kSearchBlock) base[i] = elem(i);
}

template <int G, bool SYM>
__global__ __launch_bounds__(kSearchBlock) void PgxRecordEmit(const int* __restrict__ ids, RecordArgs a) {
  constexpr int A = pgx::Dims<G>::A, OB = pgx::GuidedObsElems<G>(), PS = pgx::RecordPolicyStride<G>();
  constexpr int NS = SYM ? pgx::RecordSyms<G>() : 1;
  const int lane = threadIdx.x;
  const int n_items = *a.n_items;
  const int2* items = reinterpret_cast<const int2*>(a.items);
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
    const int row = items[it].x, p = items[it].y;
    const int e = ids[row];
    const size_t at = (size_t)e * a.plies + p;  // the staged row
    pgx::View view{};
    view.s = static_cast<const pgx::State*>(a.states)[at];
    const int mover = pgx::SearchMover<G>(view.s);
    const uint32_t* pol = reinterpret_cast<const uint32_t*>(a.staged_policy) + at * PS;
    const size_t s0 = (size_t)a.plan[row] + (size_t)p * NS;  // the ply's first sample; its NS samples are contiguous
    GuidedEmitRow(a.obs + s0 * OB, NS * OB, lane, [&](int i) {
      const int j = i / OB;
      return pgx::RecordObsElem<G>(view, mover, j, i - j * OB);
    });
    GuidedEmitRow(a.mask + s0 * A, NS * A, lane, [&](int i) {
      const int j = i / A;
      return pgx::RecordMaskElem<G>(view, j, i - j * A);
    });
    RecordEmitWords(reinterpret_cast<uint32_t*>(a.policy) + s0 * A, NS * A, lane, [&](int i) {
      const int j = i / A;
      return pol[pgx::RecordPolicySource<G>(j, i - j * A)];
    });
    if (lane < NS) {
      reinterpret_cast<uint32_t*>(a.value)[s0 + lane] = reinterpret_cast<const uint32_t*>(a.reward)[(size_t)row * 2 + mover];
      a.ply[s0 + lane] = a.elapsed[at];
      a.env_id[s0 + lane] = e + a.id_offset;
      a.sym[s0 + lane] = (unsigned char)lane;
    }
  }
}

// An arena's side bytes (pgx_arena.hip.h): one thread per env, row i is local env i; the env's `slots` leaf rows get the
// net of its root's mover.  (The state of an env that is over is whatever it was: its rows are idle and never read.)
template <int G>
__global__ __launch_bounds__(kBlock) void PgxArenaSides(const pgx::State* __restrict__ st, SelfplayArgs a) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.k) return;
  const unsigned char side = (unsigned char)pgx::ArenaNetOf(i + a.id_offset, pgx::SearchMover<G>(st[i]));
  for (int j = 0; j < a.slots; ++j) a.side[(size_t)i * a.slots + j] = side;
}

// the render kernel's painter of game G (render_kernel.hip.h)
template <int G>
struct PgxPainter {
  using State = pgx::State;
  static __device__ void Paint(render::Canvas& cv, const State& s) { pgx::Render<G>(cv, s); }
};

int GameOf(const std::string& family) {
  if (family == "TicTacToe") return pgx::kTicTacToe;
  if (family == "ConnectFour") return pgx::kConnectFour;
  if (family == "Hex") return pgx::kHex;
  return pgx::kOthello;
}

// the reference's StateSpec key order (after the common keys); "obs" and "info:players.id" are per player
template <int G>
FamilySpec Spec() {
  using D = pgx::Dims<G>;
  return {{{"obs", EPA_BOOL, {pgx::kPlayers, D::H, D::W, D::C}, pgx::kPlayers},
           {"info:board", EPA_I32, {D::H, D::W}},
           {"info:current_player", EPA_I32, {}},
           {"info:legal_action_mask", EPA_BOOL, {D::A}},
           {"info:players.id", EPA_I32, {pgx::kPlayers}, pgx::kPlayers}},
          {"action", EPA_I32, {}},
          pgx::kPlayers};
}

template <int G>
class PgxPool : public Pool {
 public:
  bool ConcurrentSafe() const override { return true; }  // per-env state + the launch's own rows only
  explicit PgxPool(const Config& cfg)
      : Pool(cfg, Spec<G>(), /*needs_rng=*/true) {
    const size_t n = (size_t)cfg.num_envs;
    state_ = DevAlloc<pgx::State>(n);
    EnableErrorWord();
    mt_tile_default_ = 16;  // envs reset at their own times
    InitCommon();
  }
  int StateDim() const override { return 2 + pgx::HiddenWords<G>(); }
  void GetState(const int* d_ids, int k, double* d_out) override {
    hipLaunchKernelGGL(PgxGetState<G>, dim3((k + 255) / 256), dim3(256), 0, stream_, common_, state_, d_ids, k,
                       d_out);
  }
  void SetState(const int* d_ids, int k, const double* d_in) override {
    hipLaunchKernelGGL(PgxSetState<G>, dim3((k + 255) / 256), dim3(256), 0, stream_, common_, state_, err_dev_,
                       d_ids, k, d_in);
  }
  void RenderSize(int width, int height, int* w, int* h) const override { pgx::RenderSize<G>(width, height, w, h); }
  void Render(const int* d_ids, int k, int w, int h, int /*camera_id*/, void* d_rgb) override {
    render::LaunchRender<PgxPainter<G>>(state_, d_ids, k, w, h, d_rgb, stream_);
  }
  bool HasPlayout() const override { return true; }
  void Playout(const int* d_ids, const PlayoutArgs& a) override {
    const long long lanes = (long long)a.k * a.repeats;
    hipLaunchKernelGGL(PgxPlayoutKernel<G>, dim3((unsigned)((lanes + kPlayoutBlock - 1) / kPlayoutBlock)),
                       dim3(kPlayoutBlock), 0, stream_, common_, state_, d_ids, a, cfg_.env_id_offset);
  }
  bool HasSearch() const override { return true; }
  int SearchActions() const override { return pgx::Dims<G>::A; }
  size_t SearchNodeBytes() const override { return sizeof(pgx::SearchNode<G>); }
  void Search(const int* d_ids, const SearchArgs& a) override {
    LaunchRoots(PgxSearchKernel<G>, a.k, common_, state_, d_ids, a, cfg_.env_id_offset, err_dev_);
  }
  bool HasSolve() const override { return true; }
  size_t SolveRootBytes(int depth) const override { return pgx::SolveStackBytes(depth); }
  size_t SolveTableBytes(int table_bits) const override { return pgx::SolveTableBytes(table_bits); }
  void Solve(const int* d_ids, const SolveArgs& a) override {
    if (a.table_bits != 0) {
      LaunchRoots(PgxSolveKernel<G, true>, a.k, common_, state_, d_ids, a, err_dev_);
      return;
    }
    LaunchRoots(PgxSolveKernel<G, false>, a.k, common_, state_, d_ids, a, err_dev_);
  }
  bool HasGuided() const override { return true; }
  void GuidedShape(int32_t shape[4]) const override {
    shape[0] = pgx::Dims<G>::H, shape[1] = pgx::Dims<G>::W, shape[2] = pgx::Dims<G>::C, shape[3] = pgx::Dims<G>::A;
  }
  size_t GuidedNodeBytes() const override { return sizeof(pgx::GuidedNode<G>); }
  size_t GuidedRootBytes() const override { return sizeof(pgx::GuidedRoot); }
  size_t GuidedWideRootBytes(int width) const override { return pgx::GuidedWideRootBytes(width); }
  size_t GuidedWideLiveOffset() const override { return offsetof(pgx::GuidedWideRoot, live); }
  // a.width != 0: a wide session; the plain kernels otherwise
  void GuidedBegin(const int* d_ids, const GuidedArgs& a) override {
    if (a.width != 0) {
      LaunchRoots(PgxGuidedBegin<G, true>, a.k, common_, state_, d_ids, a);
    } else {
      LaunchRoots(PgxGuidedBegin<G, false>, a.k, common_, state_, d_ids, a);
    }
  }
  // ... and a.flags has EPA_GUIDED_PROVE: the PROVE instantiations (pgx_guided.hip.h "Proven values")
  void GuidedAdvance(const GuidedArgs& a) override {
    Flags(a.width != 0, Proves(a), [&](auto wide, auto prove) {
      constexpr bool kProve = decltype(prove)::value;
      if constexpr (!decltype(wide)::value) {
        LaunchRoots(PgxGuidedAdvance<G, kProve>, a.k, a, err_dev_);
      } else {
        Bucket<kWideBuckets>(a.width, [&](auto wb) {
          LaunchRoots(PgxGuidedAdvanceWide<G, decltype(wb)::value, kProve>, a.k, a, err_dev_);
        });
      }
    });
  }
  void GuidedResult(const GuidedArgs& a) override {
    Flags(a.width != 0, Proves(a), [&](auto wide, auto prove) {
      LaunchRoots(PgxGuidedResult<G, decltype(wide)::value, decltype(prove)::value>, a.k, a);
    });
  }
  void GuidedReroot(const GuidedArgs& a) override {
    Flags(a.width != 0, Proves(a), [&](auto wide, auto prove) {
      Bucket<kRerootTables>(a.capacity, [&](auto cap) {
        LaunchRoots(PgxGuidedReroot<G, decltype(cap)::value, decltype(wide)::value, decltype(prove)::value>, a.k, a);
      });
    });
  }
  // the read-out of the proven values
  void GuidedProof(const GuidedArgs& a, signed char* value, signed char* q) override {
    if (a.width != 0) {
      LaunchRoots(PgxGuidedProof<G, true>, a.k, a, value, q);
    } else {
      LaunchRoots(PgxGuidedProof<G, false>, a.k, a, value, q);
    }
  }
  void GuidedTactics(const GuidedArgs& a, const TacticsArgs& t) override {
    if (a.width != 0) {
      LaunchRoots(PgxGuidedTactics<G, true>, a.k * a.width, a, t);
    } else {
      LaunchRoots(PgxGuidedTactics<G, false>, a.k, a, t);
    }
  }
  size_t GumbelNodeBytes() const override { return sizeof(pgx::GumbelNode<G>); }
  size_t GumbelRootBytes() const override { return sizeof(pgx::GumbelRoot<G>); }
  size_t GumbelBatchRootBytes(int batch) const override { return pgx::GumbelBatchRootBytes<G>(batch); }
  // a.batch != 0: a batch session; the plain kernels otherwise
  void GumbelBegin(const int* d_ids, const GumbelArgs& a) override {
    if (a.batch != 0) {
      LaunchRoots(PgxGumbelBegin<G, true>, a.k, common_, state_, d_ids, a);
    } else {
      LaunchRoots(PgxGumbelBegin<G, false>, a.k, common_, state_, d_ids, a);
    }
  }
  void GumbelAdvance(const GumbelArgs& a) override {
    if (a.batch != 0) return LaunchRoots(PgxGumbelAdvanceBatch<G>, a.k, a, err_dev_);
    LaunchRoots(PgxGumbelAdvance<G>, a.k, a, err_dev_);
  }
  void GumbelResult(const GumbelArgs& a) override {
    if (a.batch != 0) {
      LaunchRoots(PgxGumbelResult<G, true>, a.k, a);
    } else {
      LaunchRoots(PgxGumbelResult<G, false>, a.k, a);
    }
  }
  bool HasRecord() const override { return true; }
  int RecordSyms() const override { return pgx::RecordSyms<G>(); }
  size_t RecordStateBytes() const override { return sizeof(pgx::State); }
  int RecordPolicyStride() const override { return pgx::RecordPolicyStride<G>(); }
  void RecordAdd(const int* d_ids, const RecordArgs& a) override {
    hipLaunchKernelGGL(PgxRecordAdd<G>, dim3((unsigned)((a.k + kRecordAddRows - 1) / kRecordAddRows)), dim3(kBlock), 0,
                       stream_, common_, state_, d_ids, a);
  }
  void RecordPlan(const int* d_ids, const RecordArgs& a) override {
    hipLaunchKernelGGL(PgxRecordPlan, dim3(1), dim3(kRecordPlanBlock), 0, stream_, d_ids, a);
  }
  // a.nsym != 1: the recorder writes the game's symmetries
  void RecordEmit(const int* d_ids, const RecordArgs& a) override {
    if (a.nsym != 1) {
      LaunchRoots(PgxRecordEmit<G, true>, kRecordEmitWaves, d_ids, a);
    } else {
      LaunchRoots(PgxRecordEmit<G, false>, kRecordEmitWaves, d_ids, a);
    }
  }
  // the self-play driver's launches (pgx_selfplay.hip)
  bool HasSelfplay() const override { return true; }
  void SelfplayNoise(const SelfplayArgs& a) override { PgxSelfplayLaunchNoise(G, a, stream_); }
  void SelfplayMove(const SelfplayArgs& a) override {
    SelfplayArgs b = a;
    b.cur_step = common_.cur_step;
    PgxSelfplayLaunchMove(G, b, stream_);
  }
  void SelfplayTally(const SelfplayArgs& a) override { PgxSelfplayLaunchTally(a, stream_); }
  void SelfplayDirichlet(const SelfplayArgs& a) override { PgxSelfplayLaunchDirichlet(G, a, stream_); }
  void ArenaSides(const SelfplayArgs& a) override {
    hipLaunchKernelGGL(PgxArenaSides<G>, dim3((a.k + kBlock - 1) / kBlock), dim3(kBlock), 0, stream_, state_, a);
  }
  std::string ErrorText(unsigned code) const override {
    if (code == kErrGuided) return "PGX: guided search met a position that is no position of the game";
    if (code == kErrGumbel) return "PGX: gumbel search met a position that is no position of the game";
    if (code == kErrState) return "PGX: set_state was given words that are no position of the game";
    if (code == kErrSearch) return "PGX: search met a position that is no position of the game";
    if (code == kErrSolve) return "PGX: solve met a position that is no position of the game";
    return Pool::ErrorText(code);
  }

 protected:
  void Launch(const int* d_ids, int k, const void* d_action, bool force_reset, const OutPtrs& out) override {
    StepArgs a{d_ids, k, force_reset ? 1 : 0, cfg_.max_episode_steps, cfg_.env_id_offset};
    hipLaunchKernelGGL(PgxStepKernel<G>, dim3((k + kBlock - 1) / kBlock), dim3(kBlock), 0, stream_, common_, a,
                       state_, static_cast<const int*>(d_action), out);
  }

 private:
  // a tree-search kernel: one block of one wave per root
  template <class... P, class... Q>
  void LaunchRoots(void (*kernel)(P...), int k, const Q&... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)k), dim3(kSearchBlock), 0, stream_, args...);
  }
  // f(std::integral_constant<int, b>) for the first entry b >= value of an ascending table (the last one otherwise):
  // the static LDS arrays of PgxGuidedReroot and PgxGuidedAdvanceWide come in such sizes
  template <const int (&Table)[3], int I = 0, class F>
  static void Bucket(int value, F f) {
    if constexpr (I == 2) {
      f(std::integral_constant<int, Table[2]>{});
    } else if (value <= Table[I]) {
      f(std::integral_constant<int, Table[I]>{});
    } else {
      Bucket<Table, I + 1>(value, f);
    }
  }

  // f(std::bool_constant<a>, std::bool_constant<b>): two flags of the call as template arguments of its kernel
  template <class F>
  static void Flags(bool a, bool b, F f) {
    if (a) {
      b ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    } else {
      b ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
    }
  }
  static bool Proves(const GuidedArgs& a) { return (a.flags & EPA_GUIDED_PROVE) != 0; }

  pgx::State* state_{nullptr};
};

}  // namespace

FamilySpec DescribePgx(const std::string& name, const Config&) {
  switch (GameOf(name)) {
    case pgx::kTicTacToe: return Spec<pgx::kTicTacToe>();
    case pgx::kConnectFour: return Spec<pgx::kConnectFour>();
    case pgx::kHex: return Spec<pgx::kHex>();
    default: return Spec<pgx::kOthello>();
  }
}

Pool* MakePgx(const std::string& name, const Config& cfg) {
  switch (GameOf(name)) {
    case pgx::kTicTacToe: return new PgxPool<pgx::kTicTacToe>(cfg);
    case pgx::kConnectFour: return new PgxPool<pgx::kConnectFour>(cfg);
    case pgx::kHex: return new PgxPool<pgx::kHex>(cfg);
    default: return new PgxPool<pgx::kOthello>(cfg);
  }
}

}  // namespace epa
