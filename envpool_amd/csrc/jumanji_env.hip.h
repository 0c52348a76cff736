// Jumanji board puzzles: per-env reset / step / observation, written once as __host__ __device__ code.
//
// Restates, over a generator type G, the six board puzzles of the reference's envpool/jumanji/ (one env
// per call, no allocation), for jumanji.hip (one env per lane) and the g++ host harness of the tests:
//   Game2048           game2048_env.h: MoveLineLeft / Move / CanMove / HighestTile (:57-128), Reset / Step /
//                      AddRandomCell / WriteState (:205-294)
//   Minesweeper        minesweeper_env.h: CountAdjacentMines (:66-82), Reset / Step / IsSolved / Reveal /
//                      WriteState (:185-283)
//   SlidingTilePuzzle  sliding_tile_puzzle_env.h: SolvedPuzzle / FindEmpty / CountCorrect (:44-93), Reset /
//                      Step / RandomWalk / ApplyMove / DenseReward / WriteState (:181-267)
//   RubiksCube         rubiks_cube_env.h: RotateFaceClockwise / AdjacentIndices / Rotate (:86-173), Reset /
//                      Step / WriteState (:267-314); one code for both ids (time limit, scrambles from Cfg)
//   Snake              snake_env.h: Reset / Step / IsActionValid / IsComplete / UpdateTail / PlaceFruit /
//                      WriteState (:170-284)
//   Maze               maze_env.h: Reset / Step / AnyActionAvailable / WriteState (:174-241)
// The episode bookkeeping (elapsed step, done, trunc, auto-reset) is the caller's: the step count of every
// puzzle equals the engine's elapsed step, and `*done` is IsDone() after the call.
//
// Generator interface (draws of the env's std::mt19937, libstdc++ 11):
//   int    G::UniformInt(a, b)                            uniform_int_distribution<int>(a, b)
//   double G::Canonical()                                 generate_canonical<double, 53>: bernoulli_distribution(p)
//                                                         is Canonical() < p (bits/random.h, two words per draw)
//   void   G::UniformPair(uint32 b0, uint32 b1, int*, int*)  std::__gen_two_uniform_ints(b0, b1, g)
// std::shuffle of Minesweeper's 100 locations is restated in ShuffleLocations (bits/stl_algo.h:3713-3760).
//
// The per-env state structs live in HBM on the device (jumanji.hip) and are read and written in place.
#ifndef ENVPOOL_AMD_CSRC_JUMANJI_ENV_HIP_H_
#define ENVPOOL_AMD_CSRC_JUMANJI_ENV_HIP_H_

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define JM_HD __host__ __device__
#else
#define JM_HD
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define JM_ROLLED _Pragma("unroll 1")
#define JM_UNROLL _Pragma("unroll")
#else
#define JM_ROLLED
#define JM_UNROLL
#endif

namespace epa {
namespace jm {

enum Puzzle : int { kGame2048 = 0, kMinesweeper = 1, kSlidingTile = 2, kRubiksCube = 3, kSnake = 4, kMaze = 5 };

// Per-pool configuration (the parsed initial-state keys); `init` is uploaded once per pool.
struct Cfg {
  int puzzle;
  int time_limit;       // SlidingTilePuzzle 500, RubiksCube 200 / 20, Snake 4000, Maze 100 (0: none)
  int use_init;         // the initial-state string key was non-empty (board / puzzle / cube / walls / mines / head)
  int add_random_cell;  // Game2048
  int num_scrambles;    // RubiksCube
  int num_mines;        // Minesweeper: the configured count, else 10
  int pos[4];           // Snake head row, col, fruit row, col; Maze agent row, col, target row, col
  int max_tries;        // Snake: bound of the reset's fruit rejection loop (engine key snake_max_tries)
};
constexpr int kInitWords = 100;  // int32 words of `init`: board 16 / mine mask 100 / puzzle 25 / cube 54 / walls 100

struct Game2048State {
  int32_t board[16];  // exponents
};
struct MinesweeperState {
  int8_t board[100];  // -1 unexplored, else the adjacent-mine count
  uint8_t mine[100];
};
struct SlidingTileState {
  int32_t puzzle[25];
  int32_t empty_row, empty_col;
};
struct RubiksCubeState {
  int8_t cube[56];  // 54 stickers face-major, 2 bytes of padding
};
struct SnakeState {
  uint8_t body[144];  // 0 empty, else the segment's age (1 = tail, length = head)
  int16_t head_row, head_col, tail_row, tail_col, fruit_row, fruit_col, length, pad;
};
struct MazeState {
  uint8_t walls[100];
  int8_t agent_row, agent_col, target_row, target_col;
};

// Words of the hidden state after (elapsed step, done) in get_state / set_state, in the order the fixtures
// record them (tests/golden/make_jumanji_golden.py, HIDDEN)
JM_HD constexpr int HiddenWords(int puzzle) {
  return puzzle == kGame2048 ? 16 : puzzle == kMinesweeper ? 202 : puzzle == kSlidingTile ? 28
         : puzzle == kRubiksCube ? 55 : puzzle == kSnake ? 152 : 105;
}

constexpr int kMoves[4][2] = {{-1, 0}, {0, 1}, {1, 0}, {0, -1}};

// ---------------------------------------------------------------------------------------------- Game2048
// cell of line i, position j, for a move in direction a (Move's four index maps)
JM_HD constexpr int G2048Cell(int a, int i, int j) {
  return a == 0 ? j * 4 + i : a == 1 ? i * 4 + 3 - j : a == 2 ? (3 - j) * 4 + i : i * 4 + j;
}
JM_HD inline float G2048Pow2(int e) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ldexpf(1.0f, e);
#else
  return std::ldexp(1.0f, e);
#endif
}
// MoveLineLeft on one line in place; returns the line's reward
JM_HD inline float G2048Line(int (&l)[4]) {
  int c[4] = {0, 0, 0, 0};
  int n = 0;
JM_UNROLL
  for (int j = 0; j < 4; ++j) {
    const int v = l[j];
    // c[n] = v without a dynamically indexed store
JM_UNROLL
    for (int q = 0; q < 4; ++q) c[q] = (v != 0 && q == n) ? v : c[q];
    n += v != 0;
  }
  int m[4] = {0, 0, 0, 0};
  float reward = 0.0f;
  // the four outcomes of the compaction of <= 4 tiles, pairs merged left to right
  if (n >= 2 && c[0] == c[1]) {
    m[0] = c[0] + 1;
    reward += G2048Pow2(m[0]);
    if (n == 4 && c[2] == c[3]) {
      m[1] = c[2] + 1;
      reward += G2048Pow2(m[1]);
    } else {
      m[1] = c[2];
      m[2] = c[3];
    }
  } else {
    m[0] = c[0];
    if (n >= 3 && c[1] == c[2]) {
      m[1] = c[1] + 1;
      reward += G2048Pow2(m[1]);
      m[2] = c[3];
    } else {
      m[1] = c[1];
      if (n == 4 && c[2] == c[3]) {
        m[2] = c[2] + 1;
        reward += G2048Pow2(m[2]);
      } else {
        m[2] = c[2];
        m[3] = c[3];
      }
    }
  }
JM_UNROLL
  for (int j = 0; j < 4; ++j) l[j] = m[j];
  return reward;
}
template <int A>
JM_HD inline float G2048MoveA(int (&b)[16]) {
  float reward = 0.0f;
JM_UNROLL
  for (int i = 0; i < 4; ++i) {
    int l[4];
JM_UNROLL
    for (int j = 0; j < 4; ++j) l[j] = b[G2048Cell(A, i, j)];
    reward += G2048Line(l);
JM_UNROLL
    for (int j = 0; j < 4; ++j) b[G2048Cell(A, i, j)] = l[j];
  }
  return reward;
}
template <int A>
JM_HD inline bool G2048CanMoveA(const int (&b)[16]) {
  int m[16];
JM_UNROLL
  for (int i = 0; i < 16; ++i) m[i] = b[i];
  G2048MoveA<A>(m);
  bool diff = false;
JM_UNROLL
  for (int i = 0; i < 16; ++i) diff |= m[i] != b[i];
  return diff;
}
JM_HD inline unsigned G2048Mask(const int (&b)[16]) {
  return (G2048CanMoveA<0>(b) ? 1u : 0u) | (G2048CanMoveA<1>(b) ? 2u : 0u) | (G2048CanMoveA<2>(b) ? 4u : 0u) |
         (G2048CanMoveA<3>(b) ? 8u : 0u);
}
template <typename G>
JM_HD inline void G2048AddRandomCell(G& g, int (&b)[16]) {
  int empty = 0;
JM_UNROLL
  for (int i = 0; i < 16; ++i) empty += b[i] == 0;
  if (empty == 0) return;
  // `board_[empty[position_dist(gen_)]] = two_dist(gen_) ? 2 : 1;`: the right operand of an assignment is
  // sequenced first (C++17), so the bernoulli draw comes before the position draw
  const int v = g.Canonical() < 0.1 ? 2 : 1;
  int k = g.UniformInt(0, empty - 1);
JM_UNROLL
  for (int i = 0; i < 16; ++i) {
    if (b[i] == 0) {
      if (k == 0) b[i] = v;
      --k;
    }
  }
}
JM_HD inline void G2048Load(const Game2048State& s, int (&b)[16]) {
JM_UNROLL
  for (int i = 0; i < 16; ++i) b[i] = s.board[i];
}
JM_HD inline void G2048Store(Game2048State& s, const int (&b)[16]) {
JM_UNROLL
  for (int i = 0; i < 16; ++i) s.board[i] = b[i];
}
template <typename G>
JM_HD inline void G2048Reset(G& g, const Cfg& c, const int* init, Game2048State& s, bool* done) {
  int b[16];
JM_UNROLL
  for (int i = 0; i < 16; ++i) b[i] = c.use_init ? init[i] : 0;
  if (!c.use_init) G2048AddRandomCell(g, b);
  G2048Store(s, b);
  *done = G2048Mask(b) == 0;
}
template <typename G>
JM_HD inline float G2048Step(G& g, const Cfg& c, Game2048State& s, int action, bool* done) {
  const int a = action < 0 ? 0 : action > 3 ? 3 : action;
  int b[16];
  G2048Load(s, b);
  float reward = 0.0f;
  if ((G2048Mask(b) >> a) & 1u) {
    switch (a) {
      case 0: reward = G2048MoveA<0>(b); break;
      case 1: reward = G2048MoveA<1>(b); break;
      case 2: reward = G2048MoveA<2>(b); break;
      default: reward = G2048MoveA<3>(b); break;
    }
    if (c.add_random_cell) G2048AddRandomCell(g, b);
  }
  G2048Store(s, b);
  *done = G2048Mask(b) == 0;
  return reward;
}
// obs:board [4,4], obs:action_mask [4], info:highest_tile
JM_HD inline void G2048Obs(const Game2048State& s, int32_t* board, uint8_t* mask, int32_t* highest) {
  int b[16];
  G2048Load(s, b);
  int e = 0;
JM_UNROLL
  for (int i = 0; i < 16; ++i) {
    board[i] = b[i];
    e = b[i] > e ? b[i] : e;
  }
  const unsigned m = G2048Mask(b);
JM_UNROLL
  for (int a = 0; a < 4; ++a) mask[a] = (m >> a) & 1u;
  *highest = e == 0 ? 1 : (int)(1u << e);
}

// ---------------------------------------------------------------------------------------------- Minesweeper
JM_HD inline int MsAdjacent(const MinesweeperState& s, int row, int col) {
  int count = 0;
  for (int dr = -1; dr <= 1; ++dr) {
    for (int dc = -1; dc <= 1; ++dc) {
      const int r = row + dr, cc = col + dc;
      if ((dr != 0 || dc != 0) && 0 <= r && r < 10 && 0 <= cc && cc < 10 && s.mine[r * 10 + cc]) ++count;
    }
  }
  return count;
}
JM_HD inline void MsSwap(MinesweeperState& s, int i, int j) {
  const int8_t t = s.board[i];
  s.board[i] = s.board[j];
  s.board[j] = t;
}
// std::shuffle(locations, locations + 100, gen_) with libstdc++'s pair draws (the range 100 fits twice in the
// generator's 32 bits), in s.board as scratch: 100 is even, so one single draw first, then pairs
template <typename G>
JM_HD inline void ShuffleLocations(G& g, MinesweeperState& s) {
  JM_ROLLED
  for (int i = 0; i < 100; ++i) s.board[i] = (int8_t)i;
  MsSwap(s, 1, g.UniformInt(0, 1));
  JM_ROLLED
  for (int i = 2; i != 100; i += 2) {
    const uint32_t r = (uint32_t)i + 1u;
    int p0, p1;
    g.UniformPair(r, r + 1u, &p0, &p1);
    MsSwap(s, i, p0);
    MsSwap(s, i + 1, p1);
  }
}
template <typename G>
JM_HD inline void MsReset(G& g, const Cfg& c, const int* init, MinesweeperState& s, bool* done) {
  JM_ROLLED
  for (int i = 0; i < 100; ++i) s.mine[i] = c.use_init ? (uint8_t)(init[i] != 0) : 0;
  if (!c.use_init) {
    ShuffleLocations(g, s);
    JM_ROLLED
    for (int i = 0; i < c.num_mines; ++i) s.mine[(uint8_t)s.board[i]] = 1;
  }
  JM_ROLLED
  for (int i = 0; i < 100; ++i) s.board[i] = -1;
  *done = false;
}
// Reveal: the breadth-first fill of the reference reveals the same set of cells in any order -- every
// unexplored cell reachable from (row, col) through revealed cells with no adjacent mine that are not mines.
// `todo` holds the revealed cells still to expand, as a 100-bit set.
JM_HD inline void MsReveal(MinesweeperState& s, int row, int col) {
  uint64_t todo[2] = {0, 0};
  int off = row * 10 + col;
  int adj = MsAdjacent(s, row, col);
  s.board[off] = (int8_t)adj;
  if (adj == 0 && !s.mine[off]) todo[off >> 6] |= 1ull << (off & 63);
  JM_ROLLED
  while (todo[0] | todo[1]) {
    const int w = todo[0] ? 0 : 1;
#if defined(__HIP_DEVICE_COMPILE__)
    const int bit = __ffsll((unsigned long long)todo[w]) - 1;
#else
    const int bit = __builtin_ctzll(todo[w]);
#endif
    todo[w] &= todo[w] - 1;
    const int o = w * 64 + bit;
    const int r0 = o / 10, c0 = o % 10;
    JM_ROLLED
    for (int k = 0; k < 9; ++k) {
      const int r = r0 + k / 3 - 1, cc = c0 + k % 3 - 1;
      if (k == 4 || r < 0 || r >= 10 || cc < 0 || cc >= 10) continue;
      const int n = r * 10 + cc;
      if (s.board[n] != -1) continue;
      const int a = MsAdjacent(s, r, cc);
      s.board[n] = (int8_t)a;
      if (a == 0 && !s.mine[n]) todo[n >> 6] |= 1ull << (n & 63);
    }
  }
}
JM_HD inline float MsStep(const Cfg& c, MinesweeperState& s, const int* action, bool* done) {
  const int row = action[0] < 0 ? 0 : action[0] > 9 ? 9 : action[0];
  const int col = action[1] < 0 ? 0 : action[1] > 9 ? 9 : action[1];
  const int off = row * 10 + col;
  const bool valid = s.board[off] == -1;
  const bool hit = s.mine[off] != 0;
  float reward = 0.0f;
  if (valid) {
    MsReveal(s, row, col);
    reward = hit ? 0.0f : 1.0f;
  }
  int explored = 0;
  JM_ROLLED
  for (int i = 0; i < 100; ++i) explored += s.board[i] >= 0;
  *done = !valid || hit || explored == 100 - c.num_mines;
  return reward;
}
// obs:board [10,10], obs:action_mask [10,10], obs:num_mines, obs:step_count
JM_HD inline void MsObs(const Cfg& c, const MinesweeperState& s, int step, int32_t* board, uint8_t* mask,
                        int32_t* num_mines, int32_t* step_count) {
  JM_ROLLED
  for (int i = 0; i < 100; ++i) {
    board[i] = s.board[i];
    mask[i] = s.board[i] == -1;
  }
  *num_mines = c.num_mines;
  *step_count = step;
}

// ---------------------------------------------------------------------------------------------- SlidingTilePuzzle
JM_HD inline int StSolved(int i) { return i == 24 ? 0 : i + 1; }
JM_HD inline bool StInGrid(int r, int c) { return 0 <= r && r < 5 && 0 <= c && c < 5; }
JM_HD inline bool StIsSolved(const SlidingTileState& s) {
  bool ok = true;
  JM_ROLLED
  for (int i = 0; i < 25; ++i) ok &= s.puzzle[i] == StSolved(i);
  return ok;
}
// ApplyMove; returns DenseReward of the move (only the two swapped cells can change their correctness)
JM_HD inline float StApply(SlidingTileState& s, int a) {
  const int r = s.empty_row + kMoves[a][0], c = s.empty_col + kMoves[a][1];
  if (!StInGrid(r, c)) return 0.0f;
  const int p = s.empty_row * 5 + s.empty_col, q = r * 5 + c;
  const int vp = s.puzzle[p], vq = s.puzzle[q];
  const int before = (vp == StSolved(p)) + (vq == StSolved(q));
  s.puzzle[p] = vq;
  s.puzzle[q] = vp;
  const int after = (vq == StSolved(p)) + (vp == StSolved(q));
  s.empty_row = r;
  s.empty_col = c;
  return (float)(after - before);
}
template <typename G>
JM_HD inline void StReset(G& g, const Cfg& c, const int* init, SlidingTileState& s, bool* done) {
  int er = 4, ec = 4;
  bool found = false;
  JM_ROLLED
  for (int i = 0; i < 25; ++i) {
    const int v = c.use_init ? init[i] : StSolved(i);
    s.puzzle[i] = v;
    if (v == 0 && !found) {  // FindEmpty: the first 0 in row-major order, else (4, 4)
      found = true;
      er = i / 5;
      ec = i % 5;
    }
  }
  s.empty_row = er;
  s.empty_col = ec;
  if (!c.use_init) {
    JM_ROLLED
    for (int m = 0; m < 200; ++m) {  // RandomWalk(200): a uniform choice among the valid moves, in action order
      unsigned valid = 0;
      int nvalid = 0;
JM_UNROLL
      for (int a = 0; a < 4; ++a) {
        if (StInGrid(s.empty_row + kMoves[a][0], s.empty_col + kMoves[a][1])) {
          valid |= 1u << a;
          ++nvalid;
        }
      }
      int k = g.UniformInt(0, nvalid - 1);
      int pick = 0;
JM_UNROLL
      for (int a = 0; a < 4; ++a) {
        if ((valid >> a) & 1u) {
          if (k == 0) pick = a;
          --k;
        }
      }
      StApply(s, pick);
    }
  }
  *done = StIsSolved(s);
}
JM_HD inline float StStep(const Cfg& c, SlidingTileState& s, int action, int step, bool* done) {
  const int a = action < 0 ? 0 : action > 3 ? 3 : action;
  const float reward = StApply(s, a);
  *done = StIsSolved(s) || step >= c.time_limit;
  return reward;
}
// obs:puzzle [5,5], obs:empty_tile_position [2], obs:action_mask [4], obs:step_count, info:prop_correctly_placed
JM_HD inline void StObs(const SlidingTileState& s, int step, int32_t* puzzle, int32_t* empty, uint8_t* mask,
                        int32_t* step_count, float* prop) {
  int correct = 0;
  JM_ROLLED
  for (int i = 0; i < 25; ++i) {
    puzzle[i] = s.puzzle[i];
    correct += s.puzzle[i] == StSolved(i);
  }
  empty[0] = s.empty_row;
  empty[1] = s.empty_col;
JM_UNROLL
  for (int a = 0; a < 4; ++a) mask[a] = StInGrid(s.empty_row + kMoves[a][0], s.empty_col + kMoves[a][1]);
  *step_count = step;
  *prop = (float)correct / 25.0f;
}

// ---------------------------------------------------------------------------------------------- RubiksCube
// AdjacentIndices as sticker offsets (face * 9 + row * 3 + col): the 12 stickers around each face, in the
// order the turn cycles them
struct CubeRing {
  int8_t s[6][12];
};
constexpr CubeRing kCubeRing = {{{9, 10, 11, 36, 37, 38, 27, 28, 29, 18, 19, 20},
                                       {6, 7, 8, 18, 21, 24, 47, 46, 45, 44, 41, 38},
                                       {8, 5, 2, 27, 30, 33, 53, 50, 47, 17, 14, 11},
                                       {2, 1, 0, 36, 39, 42, 51, 52, 53, 26, 23, 20},
                                       {0, 3, 6, 9, 12, 15, 45, 48, 51, 35, 32, 29},
                                       {15, 16, 17, 24, 25, 26, 33, 34, 35, 42, 43, 44}}};
// Rotate(cube, F, amount_index) on a register copy of the cube (F a constant: every index folds)
template <int F>
JM_HD inline void CubeRotateF(int8_t (&c)[54], int amount_index) {
  const int turns = amount_index == 0 ? 1 : amount_index == 1 ? 3 : 2;  // (amount % 4 + 4) % 4
  JM_ROLLED
  for (int t = 0; t < turns; ++t) {  // RotateFaceClockwise: new (r, c) = old (2 - c, r)
    int8_t b[9];
JM_UNROLL
    for (int i = 0; i < 9; ++i) b[i] = c[F * 9 + i];
JM_UNROLL
    for (int r = 0; r < 3; ++r) {
JM_UNROLL
      for (int cc = 0; cc < 3; ++cc) c[F * 9 + r * 3 + cc] = b[(2 - cc) * 3 + r];
    }
  }
  int8_t v[12];
JM_UNROLL
  for (int i = 0; i < 12; ++i) v[i] = c[kCubeRing.s[F][i]];
  // shift = 3 * amount mod 12: 3 (amount 1), 9 (-1), 6 (2); new[i] = old[i - shift]
JM_UNROLL
  for (int i = 0; i < 12; ++i) {
    const int8_t s3 = v[(i + 9) % 12], s9 = v[(i + 3) % 12], s6 = v[(i + 6) % 12];
    c[kCubeRing.s[F][i]] = amount_index == 0 ? s3 : amount_index == 1 ? s9 : s6;
  }
}
JM_HD inline void CubeRotate(int8_t (&c)[54], int face, int amount_index) {
  switch (face) {
    case 0: CubeRotateF<0>(c, amount_index); break;
    case 1: CubeRotateF<1>(c, amount_index); break;
    case 2: CubeRotateF<2>(c, amount_index); break;
    case 3: CubeRotateF<3>(c, amount_index); break;
    case 4: CubeRotateF<4>(c, amount_index); break;
    default: CubeRotateF<5>(c, amount_index); break;
  }
}
JM_HD inline bool CubeIsSolved(const int8_t (&c)[54]) {
  bool ok = true;
JM_UNROLL
  for (int i = 0; i < 54; ++i) ok &= c[i] == c[(i / 9) * 9];
  return ok;
}
JM_HD inline void CubeLoad(const RubiksCubeState& s, int8_t (&c)[54]) {
JM_UNROLL
  for (int i = 0; i < 54; ++i) c[i] = s.cube[i];
}
JM_HD inline void CubeStore(RubiksCubeState& s, const int8_t (&c)[54]) {
JM_UNROLL
  for (int i = 0; i < 54; ++i) s.cube[i] = c[i];
}
template <typename G>
JM_HD inline void CubeReset(G& g, const Cfg& cfg, const int* init, RubiksCubeState& s, bool* done) {
  int8_t c[54];
JM_UNROLL
  for (int i = 0; i < 54; ++i) c[i] = cfg.use_init ? (int8_t)init[i] : (int8_t)(i / 9);
  if (!cfg.use_init) {
    JM_ROLLED
    for (int i = 0; i < cfg.num_scrambles; ++i) {
      // Rotate(&cube_, face_dist(gen_), amount_dist(gen_)): the reference's g++ build evaluates the two
      // arguments right to left, so the amount is drawn first
      const int amount = g.UniformInt(0, 2);
      const int face = g.UniformInt(0, 5);
      CubeRotate(c, face, amount);
    }
  }
  CubeStore(s, c);
  *done = false;
}
JM_HD inline float CubeStep(const Cfg& cfg, RubiksCubeState& s, const int* action, int step, bool* done) {
  const int face = action[0] < 0 ? 0 : action[0] > 5 ? 5 : action[0];
  const int amount = action[2] < 0 ? 0 : action[2] > 2 ? 2 : action[2];
  int8_t c[54];
  CubeLoad(s, c);
  CubeRotate(c, face, amount);
  CubeStore(s, c);
  const bool solved = CubeIsSolved(c);
  *done = solved || step >= cfg.time_limit;
  return solved ? 1.0f : 0.0f;
}

// ---------------------------------------------------------------------------------------------- Snake
JM_HD inline bool SnInGrid(int r, int c) { return 0 <= r && r < 12 && 0 <= c && c < 12; }
JM_HD inline bool SnValid(const SnakeState& s, int a) {
  const int r = s.head_row + kMoves[a][0], c = s.head_col + kMoves[a][1];
  return SnInGrid(r, c) && s.body[r * 12 + c] <= 1;
}
JM_HD inline unsigned SnMask(const SnakeState& s) {
  return (SnValid(s, 0) ? 1u : 0u) | (SnValid(s, 1) ? 2u : 0u) | (SnValid(s, 2) ? 4u : 0u) |
         (SnValid(s, 3) ? 8u : 0u);
}
JM_HD inline void SnUpdateTail(SnakeState& s) {
  JM_ROLLED
  for (int i = 0; i < 144; ++i) {
    if (s.body[i] == 1) {
      s.tail_row = (int16_t)(i / 12);
      s.tail_col = (int16_t)(i % 12);
      return;
    }
  }
}
// false: the fruit's rejection loop ran out of cfg.max_tries draws (the reference's do/while has no bound)
template <typename G>
JM_HD inline bool SnReset(G& g, const Cfg& c, SnakeState& s, bool* done) {
  JM_ROLLED
  for (int i = 0; i < 144; ++i) s.body[i] = 0;
  int hr = c.pos[0], hc = c.pos[1], fr = c.pos[2], fc = c.pos[3];
  bool ok = true;
  if (!c.use_init) {
    hr = g.UniformInt(0, 11);
    hc = g.UniformInt(0, 11);
    int tries = 0;
    JM_ROLLED
    do {
      if (tries++ >= c.max_tries) {
        ok = false;
        break;
      }
      fr = g.UniformInt(0, 11);
      fc = g.UniformInt(0, 11);
    } while (fr == hr && fc == hc);
  }
  s.head_row = (int16_t)hr;
  s.head_col = (int16_t)hc;
  s.fruit_row = (int16_t)fr;
  s.fruit_col = (int16_t)fc;
  s.length = 1;
  s.body[hr * 12 + hc] = 1;
  SnUpdateTail(s);
  *done = SnMask(s) == 0;
  return ok;
}
template <typename G>
JM_HD inline float SnStep(G& g, const Cfg& c, SnakeState& s, int action, int step, bool* done) {
  const int a = action < 0 ? 0 : action > 3 ? 3 : action;
  const bool valid = SnValid(s, a);
  float reward = 0.0f;
  if (valid) {
    const int nr = s.head_row + kMoves[a][0], nc = s.head_col + kMoves[a][1];
    const bool eaten = nr == s.fruit_row && nc == s.fruit_col;
    if (eaten) {
      ++s.length;
      reward = 1.0f;
    } else {
      JM_ROLLED
      for (int i = 0; i < 144; ++i) s.body[i] = s.body[i] ? s.body[i] - 1 : 0;
    }
    s.head_row = (int16_t)nr;
    s.head_col = (int16_t)nc;
    s.body[nr * 12 + nc] = (uint8_t)s.length;
    if (eaten) {  // PlaceFruit: a uniform choice among the empty cells, none if there is none
      int empty = 0;
      JM_ROLLED
      for (int i = 0; i < 144; ++i) empty += s.body[i] == 0;
      if (empty > 0) {
        int k = g.UniformInt(0, empty - 1);
        JM_ROLLED
        for (int i = 0; i < 144; ++i) {
          if (s.body[i] == 0) {
            if (k == 0) {
              s.fruit_row = (int16_t)(i / 12);
              s.fruit_col = (int16_t)(i % 12);
              break;
            }
            --k;
          }
        }
      }
    }
    SnUpdateTail(s);
  }
  bool complete = true;
  JM_ROLLED
  for (int i = 0; i < 144; ++i) complete &= s.body[i] > 0;
  *done = !valid || complete || step >= c.time_limit || SnMask(s) == 0;
  return reward;
}
// one cell's 5 channels of obs:grid [12,12,5]; channel 4 is an IEEE fp32 division, as in the reference
JM_HD inline void SnCell(const SnakeState& s, int i, float* o) {
  const int r = i / 12, c = i % 12;
  const int b = s.body[i];
  o[0] = b > 0 ? 1.0f : 0.0f;
  o[1] = r == s.head_row && c == s.head_col ? 1.0f : 0.0f;
  o[2] = r == s.tail_row && c == s.tail_col ? 1.0f : 0.0f;
  o[3] = r == s.fruit_row && c == s.fruit_col ? 1.0f : 0.0f;
  o[4] = s.length > 0 ? (float)b / (float)s.length : 0.0f;
}

// ---------------------------------------------------------------------------------------------- Maze
JM_HD inline bool MzOpen(const MazeState& s, int r, int c) {
  return 0 <= r && r < 10 && 0 <= c && c < 10 && !s.walls[r * 10 + c];
}
JM_HD inline unsigned MzMask(const MazeState& s) {
  unsigned m = 0;
JM_UNROLL
  for (int a = 0; a < 4; ++a) m |= MzOpen(s, s.agent_row + kMoves[a][0], s.agent_col + kMoves[a][1]) ? 1u << a : 0u;
  return m;
}
template <typename G>
JM_HD inline void MzReset(G& g, const Cfg& c, const int* init, MazeState& s, bool* done) {
  JM_ROLLED
  for (int i = 0; i < 100; ++i) s.walls[i] = c.use_init ? (uint8_t)(init[i] != 0) : (uint8_t)(g.Canonical() < 0.2);
  s.agent_row = (int8_t)c.pos[0];
  s.agent_col = (int8_t)c.pos[1];
  s.target_row = (int8_t)c.pos[2];
  s.target_col = (int8_t)c.pos[3];
  s.walls[c.pos[0] * 10 + c.pos[1]] = 0;
  s.walls[c.pos[2] * 10 + c.pos[3]] = 0;
  *done = c.pos[0] == c.pos[2] && c.pos[1] == c.pos[3];
}
JM_HD inline float MzStep(const Cfg& c, MazeState& s, int action, int step, bool* done) {
  const int a = action < 0 ? 0 : action > 3 ? 3 : action;
  const int nr = s.agent_row + kMoves[a][0], nc = s.agent_col + kMoves[a][1];
  if (MzOpen(s, nr, nc)) {
    s.agent_row = (int8_t)nr;
    s.agent_col = (int8_t)nc;
  }
  const bool reached = s.agent_row == s.target_row && s.agent_col == s.target_col;
  *done = reached || step >= c.time_limit || MzMask(s) == 0;
  return reached ? 1.0f : 0.0f;
}

// ---------------------------------------------------------------------------------------------- per puzzle
// The puzzle switch as templates: State<P>::T is the per-env state, and ResetP / StepP / ObsP / HiddenP /
// SetHiddenP the puzzle's reset, step, WriteState and get_state / set_state words.  o[j] is this row's slot
// of the puzzle's j-th state key (after the common keys), `action` the row's action elements.
template <int P> struct State;
template <> struct State<kGame2048> { using T = Game2048State; };
template <> struct State<kMinesweeper> { using T = MinesweeperState; };
template <> struct State<kSlidingTile> { using T = SlidingTileState; };
template <> struct State<kRubiksCube> { using T = RubiksCubeState; };
template <> struct State<kSnake> { using T = SnakeState; };
template <> struct State<kMaze> { using T = MazeState; };

// false: a bounded rejection loop ran out (Snake)
template <int P, typename G>
JM_HD inline bool ResetP(G& g, const Cfg& c, const int* init, typename State<P>::T& s, bool* done) {
  if constexpr (P == kGame2048) G2048Reset(g, c, init, s, done);
  if constexpr (P == kMinesweeper) MsReset(g, c, init, s, done);
  if constexpr (P == kSlidingTile) StReset(g, c, init, s, done);
  if constexpr (P == kRubiksCube) CubeReset(g, c, init, s, done);
  if constexpr (P == kSnake) return SnReset(g, c, s, done);
  if constexpr (P == kMaze) MzReset(g, c, init, s, done);
  return true;
}
template <int P, typename G>
JM_HD inline float StepP(G& g, const Cfg& c, typename State<P>::T& s, const int* action, int step, bool* done) {
  if constexpr (P == kGame2048) return G2048Step(g, c, s, action[0], done);
  if constexpr (P == kMinesweeper) return MsStep(c, s, action, done);
  if constexpr (P == kSlidingTile) return StStep(c, s, action[0], step, done);
  if constexpr (P == kRubiksCube) return CubeStep(c, s, action, step, done);
  if constexpr (P == kSnake) return SnStep(g, c, s, action[0], step, done);
  if constexpr (P == kMaze) return MzStep(c, s, action[0], step, done);
  return 0.0f;
}
template <int P>
JM_HD inline void ObsP(const Cfg& c, const typename State<P>::T& s, int step, void* const* o) {
  if constexpr (P == kGame2048) {
    G2048Obs(s, (int32_t*)o[0], (uint8_t*)o[1], (int32_t*)o[2]);
  }
  if constexpr (P == kMinesweeper) MsObs(c, s, step, (int32_t*)o[0], (uint8_t*)o[1], (int32_t*)o[2], (int32_t*)o[3]);
  if constexpr (P == kSlidingTile) {
    StObs(s, step, (int32_t*)o[0], (int32_t*)o[1], (uint8_t*)o[2], (int32_t*)o[3], (float*)o[4]);
  }
  if constexpr (P == kRubiksCube) {
    int8_t* cube = (int8_t*)o[0];
JM_UNROLL
    for (int i = 0; i < 54; ++i) cube[i] = s.cube[i];
    *(int32_t*)o[1] = step;
  }
  if constexpr (P == kSnake) {
    float* grid = (float*)o[0];
    JM_ROLLED
    for (int i = 0; i < 144; i += 4) {  // 4 cells = 20 floats = five 16-byte words
      float v[20];
JM_UNROLL
      for (int q = 0; q < 4; ++q) SnCell(s, i + q, v + 5 * q);
#if defined(__HIP_DEVICE_COMPILE__)
      if ((reinterpret_cast<uintptr_t>(grid) & 15u) == 0) {
        float4* w = reinterpret_cast<float4*>(grid + 5 * i);
JM_UNROLL
        for (int q = 0; q < 5; ++q) w[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        continue;
      }
#endif
      for (int q = 0; q < 20; ++q) grid[5 * i + q] = v[q];
    }
    *(int32_t*)o[1] = step;
    const unsigned m = SnMask(s);
    uint8_t* mask = (uint8_t*)o[2];
JM_UNROLL
    for (int a = 0; a < 4; ++a) mask[a] = (m >> a) & 1u;
  }
  if constexpr (P == kMaze) {
    *(int32_t*)o[0] = s.agent_row;
    *(int32_t*)o[1] = s.agent_col;
    *(int32_t*)o[2] = s.target_row;
    *(int32_t*)o[3] = s.target_col;
    uint8_t* walls = (uint8_t*)o[4];
    JM_ROLLED
    for (int i = 0; i < 100; ++i) walls[i] = s.walls[i];
    *(int32_t*)o[5] = step;
    const unsigned m = MzMask(s);
    uint8_t* mask = (uint8_t*)o[6];
JM_UNROLL
    for (int a = 0; a < 4; ++a) mask[a] = (m >> a) & 1u;
  }
}
// the hidden-state words (HiddenWords(P)) of get_state, after (elapsed step, done); `step` is the step count
template <int P, typename W>
JM_HD inline void HiddenP(const Cfg& c, const typename State<P>::T& s, int step, W* w) {
  if constexpr (P == kGame2048) {
    for (int i = 0; i < 16; ++i) w[i] = s.board[i];
  }
  if constexpr (P == kMinesweeper) {
    for (int i = 0; i < 100; ++i) w[i] = s.board[i];
    for (int i = 0; i < 100; ++i) w[100 + i] = s.mine[i];
    w[200] = c.num_mines;
    w[201] = step;
  }
  if constexpr (P == kSlidingTile) {
    for (int i = 0; i < 25; ++i) w[i] = s.puzzle[i];
    w[25] = s.empty_row;
    w[26] = s.empty_col;
    w[27] = step;
  }
  if constexpr (P == kRubiksCube) {
    for (int i = 0; i < 54; ++i) w[i] = s.cube[i];
    w[54] = step;
  }
  if constexpr (P == kSnake) {
    for (int i = 0; i < 144; ++i) w[i] = s.body[i];
    w[144] = s.head_row;
    w[145] = s.head_col;
    w[146] = s.tail_row;
    w[147] = s.tail_col;
    w[148] = s.fruit_row;
    w[149] = s.fruit_col;
    w[150] = s.length;
    w[151] = step;
  }
  if constexpr (P == kMaze) {
    for (int i = 0; i < 100; ++i) w[i] = s.walls[i];
    w[100] = s.agent_row;
    w[101] = s.agent_col;
    w[102] = s.target_row;
    w[103] = s.target_col;
    w[104] = step;
  }
}
// set_state: the inverse of HiddenP (the step count words are the caller's elapsed step, num_mines is the
// pool's).  false: a position off the board (the env then resets on its next step)
template <int P, typename W>
JM_HD inline bool SetHiddenP(typename State<P>::T& s, const W* w) {
  if constexpr (P == kGame2048) {
    for (int i = 0; i < 16; ++i) s.board[i] = (int32_t)w[i];
  }
  if constexpr (P == kMinesweeper) {
    for (int i = 0; i < 100; ++i) s.board[i] = (int8_t)w[i];
    for (int i = 0; i < 100; ++i) s.mine[i] = w[100 + i] != 0;
  }
  if constexpr (P == kSlidingTile) {
    for (int i = 0; i < 25; ++i) s.puzzle[i] = (int32_t)w[i];
    s.empty_row = (int32_t)w[25];
    s.empty_col = (int32_t)w[26];
    return StInGrid(s.empty_row, s.empty_col);
  }
  if constexpr (P == kRubiksCube) {
    for (int i = 0; i < 54; ++i) s.cube[i] = (int8_t)w[i];
  }
  if constexpr (P == kSnake) {
    for (int i = 0; i < 144; ++i) s.body[i] = (uint8_t)w[i];
    s.head_row = (int16_t)w[144];
    s.head_col = (int16_t)w[145];
    s.tail_row = (int16_t)w[146];
    s.tail_col = (int16_t)w[147];
    s.fruit_row = (int16_t)w[148];
    s.fruit_col = (int16_t)w[149];
    s.length = (int16_t)w[150];
    return SnInGrid(s.head_row, s.head_col);
  }
  if constexpr (P == kMaze) {
    for (int i = 0; i < 100; ++i) s.walls[i] = w[i] != 0;
    s.agent_row = (int8_t)w[100];
    s.agent_col = (int8_t)w[101];
    s.target_row = (int8_t)w[102];
    s.target_col = (int8_t)w[103];
    return 0 <= w[100] && w[100] < 10 && 0 <= w[101] && w[101] < 10;
  }
  return true;
}

}  // namespace jm
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_JUMANJI_ENV_HIP_H_
