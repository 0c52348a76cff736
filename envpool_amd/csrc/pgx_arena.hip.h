// PGX arena: two networks play each other in one pool -- which net moves, how an evaluation's rows are grouped by net,
// and the match statistics -- as __host__ __device__ pieces shared by the kernels (PgxNetPlan and the pair form of
// PgxNetEval in pgx_net.hip, PgxArenaSides in pgx.hip, PgxArenaTally in pgx_selfplay.hip) and the g++ host harness of
// the tests (tests/cpu_harness/pgx_arena_host.cpp, which walks the lanes as loops).  This header is the authority;
// DESIGN.md "PGX arena" restates it.  Everything the self-play driver's contract says (pgx_selfplay.hip.h: counter, key,
// noise, move) holds for an arena unchanged.
//
// The contract.
//   which net  ArenaNetOf(global env id e, seat m) = (m ^ e) & 1: net 0 (A) holds seat 0 of an env with an even global
//              id and seat 1 of an env with an odd one.  Seat 0 moves first or second by the env's reset coin, so over
//              a pool both nets get both seats and both colours.
//   sides      one uint8 per leaf row of the session: row i * slots + j (slots = batch or width, else 1) belongs to env
//              i and has the side ArenaNetOf(id of env i, SearchMover<G>(the env's state at the session's begin)).  The
//              sides are fixed for the ply: a tree is evaluated by its root mover's net throughout.
//   plan       the stable partition of the row indices 0 .. rows - 1 by side: order[0 .. n0) the side-0 rows ascending,
//              order[n0 .. rows) the side-1 rows ascending, n0 the number of side-0 rows.  No atomic decides a place:
//              the place of a side-0 row is the number of side-0 rows below it, that of a side-1 row n0 + the number of
//              side-1 rows below it (ArenaPlace).
//   waves      an evaluation of `rows` rows launches ArenaWaves(rows) = ceil(rows / 64) + 1 waves, an upper bound of
//              ceil(n0 / 64) + ceil((rows - n0) / 64).  Wave b (ArenaWaveOf): with w0 = ceil(n0 / 64),
//                b < w0:   net 0, entries 64 b .. of the plan, min(64, n0 - 64 b) of them
//                b >= w0:  net 1, entries n0 + 64 (b - w0) .., min(64, rows - n0 - 64 (b - w0)) of them, none when that
//                          is not positive: such a wave does nothing.
//              No wave holds rows of two nets, and every entry belongs to exactly one wave.
//   outputs    policy and value of row r are exactly NetOutputs (pgx_net.hip.h) of net side[r] on row r: the layers are
//              integer arithmetic, so the grouping changes no bit.  A row whose status is not "evaluate" is zeros, and
//              the pending word is ORed with 1 when some row is not idle, as for one net.
//   tally      seven int64 counters: the driver's five (SelfplayTallyRow) and, for a row with done of global env id e,
//              wins_a (reward[i][e & 1] > 0: the seat net A holds) and wins_b (reward[i][1 - (e & 1)] > 0).
//   two nets   agree in F and A (the pool's) and lie on the pool's device; D and L may differ.
#ifndef ENVPOOL_AMD_CSRC_PGX_ARENA_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_ARENA_HIP_H_

#include "pgx_selfplay.hip.h"

namespace epa {
namespace pgx {

constexpr int kArenaCounters = 7;        // games, wins0, wins1, draws, plies, wins_a, wins_b
constexpr int kArenaWaveRows = 64;       // rows of one wave of an evaluation
constexpr int kArenaMaxRows = 1 << 20;   // rows of one plan

PGX_HD inline int ArenaNetOf(int env_id, int seat) { return (seat ^ env_id) & 1; }

// where row r goes in the plan: `below0` side-0 rows lie below r
PGX_HD inline int ArenaPlace(int side, int r, int below0, int n0) { return side == 0 ? below0 : n0 + (r - below0); }

PGX_HD inline int ArenaWaves(int rows) { return (rows + kArenaWaveRows - 1) / kArenaWaveRows + 1; }

struct ArenaWave {
  int net;    // 0 / 1
  int first;  // the wave's first entry of the plan
  int count;  // 0 .. 64 entries; 0: the wave does nothing
};

PGX_HD inline ArenaWave ArenaWaveOf(int b, int rows, int n0) {
  const int w0 = (n0 + kArenaWaveRows - 1) / kArenaWaveRows;
  ArenaWave w;
  if (b < w0) {
    const int left = n0 - kArenaWaveRows * b;
    w.net = 0, w.first = kArenaWaveRows * b, w.count = left < kArenaWaveRows ? left : kArenaWaveRows;
    return w;
  }
  const int at = kArenaWaveRows * (b - w0), left = rows - n0 - at;
  w.net = 1, w.first = n0 + at, w.count = left <= 0 ? 0 : (left < kArenaWaveRows ? left : kArenaWaveRows);
  return w;
}

// what one row of the step's results adds to the seven counters
PGX_HD inline void ArenaTallyRow(bool done, float r0, float r1, int elapsed, int env_id, int out[kArenaCounters]) {
  SelfplayTallyRow(done, r0, r1, elapsed, out);
  const float ra = (env_id & 1) == 0 ? r0 : r1, rb = (env_id & 1) == 0 ? r1 : r0;
  out[5] = (done && ra > 0.0f) ? 1 : 0;
  out[6] = (done && rb > 0.0f) ? 1 : 0;
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_ARENA_HIP_H_
