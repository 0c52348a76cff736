// PGX self-play recorder: finished games of a pool as training samples, as __host__ __device__ pieces shared by the
// kernels (PgxRecordAdd / PgxRecordPlan / PgxRecordEmit in pgx.hip) and the g++ host harness of the tests
// (tests/cpu_harness/pgx_record_host.cpp, which walks the lanes as loops).
//
// The contract (DESIGN.md "PGX self-play recorder").  A = Dims<G>::A, N = the pool's envs, P = max_plies (0: 128; no
// game of the four lasts longer than 122 plies, pgx_playout.hip.h), nsym = RecordSyms<G>() with the symmetries flag,
// else 1.  The recorder keeps
//   staging   per env e: n_e (int32, the staged plies) and P rows of {the position's 64-byte State, its elapsed step
//             (int32), the cleaned policy row: RecordPolicyStride<G>() floats, A of them used, so a row starts on a
//             16-byte boundary}.  The POSITION is staged, not its observation: obs and mask are expanded at emission.
//   samples   seven arrays of `capacity` rows: obs uint8 [H, W, C] of the seat to move, mask uint8 [A], policy float32
//             [A], value float32, ply int32, env_id int32 (global), sym uint8; and the sample count (int32)
//   counters  int64: samples and games written, dropped_games, dropped_plies -- since begin, never reset
//
//   add(policy [k, A], ids [k]) -- ids do not repeat; per row i, e = ids[i]:
//     the env is over (the pool's done flag; also true before its first reset):  nothing
//     n_e > elapsed_step(e):  the staged plies belong to an abandoned game (a forced reset, a restore): they are
//         discarded, dropped_games += 1, dropped_plies += n_e, n_e = 0                              (RecordAddDecide)
//     n_e == P:  the ply is not staged, dropped_plies += 1
//     else:  row n_e of e = {State, elapsed_step(e), policy'[a] = (a legal && finite) ? policy[i][a] : 0};  n_e += 1
//         (RecordClean: the float's bits are moved or replaced by +0, never computed with; no normalisation)
//   finish(reward [k, 2], done [k], ids [k]) -- ids do not repeat; what the step returned:
//     c_i = (done[i] && n_e > 0) ? n_e * nsym : 0                                                  (RecordGameSamples)
//     off_i = the exclusive prefix sum of c_i over ALL rows in row order; base = the sample count at the call
//     game i is WRITTEN at base + off_i  iff  c_i > 0 and base + off_i + c_i <= capacity            (RecordFits)
//       otherwise, if c_i > 0, it is dropped whole: dropped_games += 1, dropped_plies += n_e
//       (off_i only grows and c_i > 0, so the written games are a prefix of the finished ones and the samples stay
//       dense: the new count is base + the sum of c_i over the written games)
//     n_e = 0 for every row with done[i]; rows with done[i] == 0 are untouched
//     sample base + off_i + p * nsym + j, for staged ply p and symmetry j, from the staged row {s, el, pol}:
//       mover = SearchMover<G>(s)
//       obs[sigma_j(cell), ch] = GuidedObsElem<G>(s, mover, cell, ch);  mask[sigma_j(a)] = GuidedMaskElem<G>(s, a)
//       policy[sigma_j(a)] = pol[a];  value = reward[i][mover];  ply = el;  env_id = e + the pool's id offset;  sym = j
//     the writer goes through the destination and reads through the INVERSE map (RecordSymCell / RecordSymAction with
//     inverse = true), so its stores are contiguous
//   Everything is integer or a move of 32 bits: the result depends on the arguments and the positions only, never on
//   the launch geometry, the order of the ids' shards or atomics.
//
// Symmetries.  sigma_0 is the identity.
//   TicTacToe (n = 3), Othello (n = 8): the dihedral group, nsym = 8.  j >= 4: first (r, c) -> (c, r); then j & 3
//     times (r, c) -> (c, n - 1 - r).  An action is its cell; Othello's pass (64) is fixed.
//   ConnectFour: nsym = 2, j = 1: (r, c) -> (r, 6 - c), action a -> 6 - a.
//   Hex: nsym = 2, j = 1: (x, y) -> (10 - x, 10 - y), i.e. cell -> 120 - cell; the swap action (121) is fixed.  The
//     transposition exchanges the colours' edges and is left out.
// Each sigma_j commutes with the game's Step for legal actions (tests/test_pgx_record_host.py checks it on fixture
// positions, so the tables are not taken on trust).
#ifndef ENVPOOL_AMD_CSRC_PGX_RECORD_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_RECORD_HIP_H_

#include "pgx_guided.hip.h"

namespace epa {
namespace pgx {

constexpr int kRecordMaxPlies = 256;      // the largest max_plies
constexpr int kRecordDefaultPlies = 128;  // max_plies = 0
constexpr int kRecordSymmetries = 1;      // the flags word of begin
constexpr long long kRecordMaxBytes = 1ll << 31;  // staging + samples of one recorder

// max_plies as the caller gives it (0: the default) -> staged rows per env
PGX_HD inline int RecordPlies(int max_plies) { return max_plies == 0 ? kRecordDefaultPlies : max_plies; }

template <int G>
PGX_HD constexpr int RecordSyms() {
  return (G == kTicTacToe || G == kOthello) ? 8 : 2;
}
// floats of a staged policy row: A rounded up to a 16-byte multiple
template <int G>
PGX_HD constexpr int RecordPolicyStride() {
  return (Dims<G>::A + 3) & ~3;
}

// sigma_j of a cell of a square board of side n under the dihedral group (inverse: sigma_j^-1)
PGX_HD inline int RecordDihedral(int n, int j, int cell, bool inverse) {
  int r = cell / n, c = cell - r * n;
  const int turns = inverse ? (4 - (j & 3)) & 3 : (j & 3);
  if (!inverse && j >= 4) {
    const int t = r;
    r = c;
    c = t;
  }
  for (int i = 0; i < turns; ++i) {  // (r, c) -> (c, n - 1 - r)
    const int t = r;
    r = c;
    c = n - 1 - t;
  }
  if (inverse && j >= 4) {
    const int t = r;
    r = c;
    c = t;
  }
  return r * n + c;
}

// sigma_j (or its inverse) of a board cell of game G
template <int G>
PGX_HD inline int RecordSymCell(int j, int cell, bool inverse) {
  if (j == 0) return cell;
  if (G == kTicTacToe || G == kOthello) return RecordDihedral(Dims<G>::W, j, cell, inverse);
  if (G == kConnectFour) {
    const int r = cell / 7;
    return r * 7 + 6 - (cell - r * 7);
  }
  return 120 - cell;  // Hex
}
// ... of an action
template <int G>
PGX_HD inline int RecordSymAction(int j, int a, bool inverse) {
  if (j == 0) return a;
  if (G == kConnectFour) return 6 - a;
  if (a >= Dims<G>::H * Dims<G>::W) return a;  // Othello's pass, Hex's swap
  return RecordSymCell<G>(j, a, inverse);
}

// the cleaned policy entry, as bits: the caller's for a legal action and a finite number, +0 otherwise
PGX_HD inline uint32_t RecordClean(uint32_t bits, bool legal) {
  return (legal && (bits & 0x7f800000u) != 0x7f800000u) ? bits : 0u;
}

// add, one row: what becomes of the env's staging.  slot >= 0: the ply is staged there.
struct RecordAddPlan {
  int slot;          // -1: nothing is staged
  int staged;        // n_e afterwards
  int drop_games;    // what the drop counters gain
  int drop_plies;
};
PGX_HD inline RecordAddPlan RecordAddDecide(bool over, int staged, int elapsed, int plies) {
  RecordAddPlan p{-1, staged, 0, 0};
  if (over) return p;
  if (p.staged > elapsed) {  // an abandoned game
    p.drop_games = 1;
    p.drop_plies = p.staged;
    p.staged = 0;
  }
  if (p.staged == plies) {
    p.drop_plies += 1;
    return p;
  }
  p.slot = p.staged;
  p.staged += 1;
  return p;
}

// finish: the samples of row i's game, and whether a game of c samples at offset off fits
PGX_HD inline int RecordGameSamples(bool done, int staged, int nsym) { return (done && staged > 0) ? staged * nsym : 0; }
PGX_HD inline bool RecordFits(long long base, long long off, int c, int capacity) {
  return base + off + (long long)c <= (long long)capacity;
}
// what finish leaves per row for the emission: the game's first sample, or one of these
constexpr int kRecordNoGame = -1;   // done == 0, or nothing staged (done: n_e is cleared all the same)
constexpr int kRecordDropped = -2;  // a finished game that did not fit

// byte e = cell' * C + ch of sample obs row j of the position in `v` (only v.s is read)
template <int G>
PGX_HD inline uint32_t RecordObsElem(const View& v, int mover, int j, int e) {
  constexpr int C = Dims<G>::C;
  const int cell = e / C, ch = e - cell * C;
  return GuidedObsElem<G>(v, mover, RecordSymCell<G>(j, cell, true) * C + ch);
}
template <int G>
PGX_HD inline uint32_t RecordMaskElem(const View& v, int j, int a) {
  return GuidedMaskElem<G>(v, RecordSymAction<G>(j, a, true));
}
// the staged policy entry that lands on action a of sample j
template <int G>
PGX_HD inline int RecordPolicySource(int j, int a) {
  return RecordSymAction<G>(j, a, true);
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_RECORD_HIP_H_
