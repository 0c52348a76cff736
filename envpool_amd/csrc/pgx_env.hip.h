// PGX two-player board games (TicTacToe, ConnectFour, Hex, Othello): the per-env logic of
// envpool/pgx/board_games.h (XxxEnv::{Reset,Step,StepGame,WriteState}) as __host__ __device__ code, shared by
// the batched kernel (pgx.hip) and the g++ host harness of the tests (tests/cpu_harness/pgx_host.cpp).
//
// Representation (free as long as every output matches, DESIGN.md "PGX"): each env is a 64-byte `State` of
// three 128-bit cell sets in the output's row-major cell order plus four words.
//   TicTacToe, ConnectFour  a = cells of color 0, b = cells of color 1 (the reference's board_ holds the color)
//   Hex, Othello            a = stones of the player to move (board_ > 0), b = the other's (board_ < 0): the
//                           reference negates its board after every move, here a and b trade places
//   m                       the legal action mask the next step checks (bit j = action j)
// The win tests are bit-parallel: ConnectFour's four directions as shifted ANDs, Hex's connection as a flood
// fill over the placer's 121-bit set (the reference's union-find relabelling keeps exactly these components in
// legal play, and after an illegal move the game is over whatever the labels say), Othello's legal moves as
// the eight-direction propagation of the reference's `Captures` scan.
//
// The output is written by `Elem`: one element of one state key from a `View` (the state plus the step's
// common keys), so the kernel can write a block's rows as contiguous 16-byte words (pgx.hip).
#ifndef ENVPOOL_AMD_CSRC_PGX_ENV_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_ENV_HIP_H_

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PGX_HD __host__ __device__
#else
#define PGX_HD
#endif

namespace epa {
namespace pgx {

typedef unsigned __int128 u128;

enum Game : int { kTicTacToe = 0, kConnectFour = 1, kHex = 2, kOthello = 3 };
constexpr int kPlayers = 2;

// board rows, columns, observation channels and actions of each game (the reference's StateSpec / ActionSpec)
template <int G> struct Dims;
template <> struct Dims<kTicTacToe> { static constexpr int H = 3, W = 3, C = 2, A = 9; };
template <> struct Dims<kConnectFour> { static constexpr int H = 6, W = 7, C = 2, A = 7; };
template <> struct Dims<kHex> { static constexpr int H = 11, W = 11, C = 4, A = 122; };
template <> struct Dims<kOthello> { static constexpr int H = 8, W = 8, C = 2, A = 65; };

struct alignas(16) State {
  u128 a, b, m;
  int32_t turn;    // TicTacToe / ConnectFour color_, Hex step_count_, Othello turn_
  int32_t cp;      // current_player_ (Hex: player_order_[0])
  int32_t passed;  // Othello passed_
  int32_t done;    // done_
};

PGX_HD inline u128 Bit(int i) { return (u128)1 << i; }
PGX_HD inline u128 Ones(int n) { return n >= 128 ? ~(u128)0 : Bit(n) - 1; }
PGX_HD inline bool Has(u128 s, int i) { return ((s >> i) & 1) != 0; }
PGX_HD inline int Count(u128 s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll((uint64_t)s) + __popcll((uint64_t)(s >> 64));
#else
  return __builtin_popcountll((uint64_t)s) + __builtin_popcountll((uint64_t)(s >> 64));
#endif
}
// cells whose column is `col` on a board `w` wide and `h` high
PGX_HD inline u128 ColumnMask(int col, int w, int h) {
  u128 m = 0;
  for (int r = 0; r < h; ++r) m |= Bit(r * w + col);
  return m;
}

struct Rewards {
  float r[2];
};
PGX_HD inline Rewards Illegal(int loser) {  // board_games::IllegalRewards
  Rewards x{{1.0f, 1.0f}};
  x.r[loser] = -1.0f;
  return x;
}
// TicTacToe / ConnectFour: ColorRewards then PlayerRewards
PGX_HD inline Rewards WinnerRewards(int winner, int cp, int color) {
  Rewards c{{0.0f, 0.0f}};
  if (winner >= 0) {
    c.r[0] = c.r[1] = -1.0f;
    c.r[winner] = 1.0f;
  }
  if (cp == color) return c;
  return Rewards{{c.r[1], c.r[0]}};
}

// ---------------------------------------------------------------------------------------------------------------
// reset: one draw of the env's generator (gen_() & 1) -- the first player, or Hex's seat swap
template <int G, class Gen>
PGX_HD void Reset(Gen& gen, State& s) {
  const int coin = (int)(gen.Next() & 1u);
  s.a = s.b = 0;
  s.turn = 0;
  s.passed = 0;
  s.done = 0;
  s.cp = coin;  // Hex: player_order_[0] = swap_players ? 1 : 0
  if (G == kOthello) {
    s.a = Bit(28) | Bit(35);
    s.b = Bit(27) | Bit(36);
    s.m = Bit(19) | Bit(26) | Bit(37) | Bit(44);
  } else if (G == kHex) {
    s.m = Ones(121);
  } else {
    s.m = Ones(Dims<G>::A);
  }
}

// ---------------------------------------------------------------------------------------------------------------
PGX_HD inline bool TicTacToeWon(u128 c) {
  const uint32_t x = (uint32_t)c;
  const uint32_t lines[8] = {0007, 0070, 0700, 0111, 0222, 0444, 0421, 0124};
  bool won = false;
  for (int i = 0; i < 8; ++i) won = won || (x & lines[i]) == lines[i];
  return won;
}

// four in a row of set `c` on the 6 x 7 row-major board, in any of the reference's four directions
PGX_HD inline bool ConnectFourWon(u128 c) {
  const uint64_t b = (uint64_t)c;
  uint64_t c0_3 = 0, c3_6 = 0;  // cells whose column is <= 3 / >= 3
  for (int r = 0; r < 6; ++r) {
    c0_3 |= (uint64_t)0x0f << (r * 7);
    c3_6 |= (uint64_t)0x78 << (r * 7);
  }
  const uint64_t h = b & (b >> 1) & (b >> 2) & (b >> 3) & c0_3;
  const uint64_t v = b & (b >> 7) & (b >> 14) & (b >> 21);
  const uint64_t d1 = b & (b >> 8) & (b >> 16) & (b >> 24) & c0_3;
  const uint64_t d2 = b & (b >> 6) & (b >> 12) & (b >> 18) & c3_6;
  return (h | v | d1 | d2) != 0;
}

// Hex (11 x 11, cell xy = x * 11 + y): the cells of `stones` connected to `seed`, over the reference's
// six neighbours (x, y-1) (x+1, y-1) (x-1, y) (x+1, y) (x-1, y+1) (x, y+1)
PGX_HD inline u128 HexComponent(u128 seed, u128 stones) {
  u128 col0 = 0, col10 = 0;
  for (int x = 0; x < 11; ++x) {
    col0 |= Bit(x * 11);
    col10 |= Bit(x * 11 + 10);
  }
  const u128 all = Ones(121);
  u128 f = seed & stones;
  for (;;) {
    const u128 ym = f & ~col0, yp = f & ~col10;
    const u128 g = f | (ym >> 1) | (yp << 1) | (f >> 11) | (f << 11) | (ym << 10) | (yp >> 10);
    const u128 nf = g & stones & all;
    if (nf == f) return f;
    f = nf;
  }
}

// Othello (8 x 8): one step of direction `dir` (the reference's kOthelloShifts order) on a set, cells leaving
// the board dropped -- EdgeOk of the reference
PGX_HD inline uint64_t OthelloShift(uint64_t x, int dir) {
  const uint64_t not_c0 = 0xfefefefefefefefeull, not_c7 = 0x7f7f7f7f7f7f7f7full;
  switch (dir) {
    case 0: return (x & not_c7) << 1;   // +1
    case 1: return (x & not_c0) >> 1;   // -1
    case 2: return x << 8;              // +8
    case 3: return x >> 8;              // -8
    case 4: return (x & not_c0) << 7;   // +7
    case 5: return (x & not_c7) >> 7;   // -7
    case 6: return (x & not_c7) << 9;   // +9
    default: return (x & not_c0) >> 9;  // -9
  }
}
// Captures(board, pos, shift) for every shift: the `opp` (board < 0) stones between `pos` and a `mine`
// (board > 0) stone
PGX_HD inline uint64_t OthelloFlips(int pos, uint64_t mine, uint64_t opp) {
  uint64_t flips = 0;
  for (int d = 0; d < 8; ++d) {
    uint64_t line = 0;
    uint64_t cur = OthelloShift((uint64_t)1 << pos, d);
    while (cur & opp) {
      line |= cur;
      cur = OthelloShift(cur, d);
    }
    if (cur & mine) flips |= line;
  }
  return flips;
}
// empty cells xy with a non-empty Captures(board, xy, shift) for some shift (board > 0: `mine`, < 0: `opp`)
PGX_HD inline uint64_t OthelloMoves(uint64_t mine, uint64_t opp, uint64_t empty) {
  uint64_t moves = 0;
  for (int d = 0; d < 8; ++d) {
    const int back = d ^ 1;  // the opposite direction
    uint64_t t = OthelloShift(mine, back) & opp;  // opp cells with a `mine` stone one step along d
    for (int i = 0; i < 5; ++i) t |= OthelloShift(t, back) & opp;
    moves |= OthelloShift(t, back) & empty;
  }
  return moves;
}

// ---------------------------------------------------------------------------------------------------------------
// One step of XxxEnv::Step(action): the game state after it, done_ in s.done, the two players' rewards.
template <int G>
PGX_HD Rewards Step(State& s, int act) {
  constexpr int A = Dims<G>::A;
  const bool in_range = act >= 0 && act < A;
  const bool illegal = !in_range || !Has(s.m, act);
  Rewards rw{{0.0f, 0.0f}};
  if (G == kTicTacToe || G == kConnectFour) {
    constexpr int cells = Dims<G>::H * Dims<G>::W;
    const int loser = s.cp;
    int winner = -1;
    if (in_range) {  // StepGame
      int cell = act;
      if (G == kConnectFour) {
        const int filled = Count((s.a | s.b) & ColumnMask(act, 7, 6));
        cell = filled < 6 ? (5 - filled) * 7 + act : -1;  // a full column places nothing
      }
      if (cell >= 0) {
        if (s.turn == 0) {
          s.a |= Bit(cell);
          s.b &= ~Bit(cell);
        } else {
          s.b |= Bit(cell);
          s.a &= ~Bit(cell);
        }
      }
      const u128 mine = s.turn == 0 ? s.a : s.b;
      const bool won = G == kTicTacToe ? TicTacToeWon(mine) : ConnectFourWon(mine);
      winner = won ? s.turn : -1;
      s.turn = 1 - s.turn;
      s.cp = 1 - s.cp;
    }
    if (illegal) {
      s.done = 1;
      s.m = Ones(A);
      return Illegal(loser);
    }
    const u128 occ = s.a | s.b;
    if (G == kTicTacToe) {
      s.m = ~occ & Ones(cells);
    } else {
      u128 m = 0;
      for (int c = 0; c < 7; ++c) m |= (u128)(Count(occ & ColumnMask(c, 7, 6)) < 6) << c;
      s.m = m;
    }
    s.done = winner >= 0 || (G == kTicTacToe ? occ == Ones(cells) : s.m == 0);
    if (s.done) {
      rw = WinnerRewards(winner, s.cp, s.turn);
      s.m = Ones(A);
    }
    return rw;
  } else if (G == kHex) {
    const int color = s.turn & 1;
    const int loser = color == 0 ? s.cp : 1 - s.cp;  // CurrentPlayer()
    if (in_range) {
      if (act != 121) {  // Place: a stone of the player to move, on any cell
        s.a |= Bit(act);
        s.b &= ~Bit(act);
        const u128 comp = HexComponent(Bit(act), s.a);
        ++s.turn;
        u128 t = s.a;  // negate the board
        s.a = s.b;
        s.b = t;
        // IsTerminal: the placer's group reaches both of its edges (Color() is now the next color)
        u128 lo = 0, hi = 0;
        for (int i = 0; i < 11; ++i) {
          if ((s.turn & 1) == 0) {
            lo |= Bit(i * 11);
            hi |= Bit(i * 11 + 10);
          } else {
            lo |= Bit(i);
            hi |= Bit(110 + i);
          }
        }
        s.done = (comp & lo) != 0 && (comp & hi) != 0;
      } else {  // Swap: the first stone moves to its transposed cell and changes hands
        const u128 occ = s.a | s.b;
        if (occ != 0) {
          const uint64_t lo = (uint64_t)occ;
          int ix;
#if defined(__HIP_DEVICE_COMPILE__)
          ix = lo ? __ffsll((unsigned long long)lo) - 1 : 64 + __ffsll((unsigned long long)(occ >> 64)) - 1;
#else
          ix = lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll((uint64_t)(occ >> 64));
#endif
          const int sw = (ix % 11) * 11 + ix / 11;
          s.a &= ~Bit(ix);
          s.b &= ~Bit(ix);
          s.a |= Bit(sw);
          s.b &= ~Bit(sw);
        }
        ++s.turn;
        u128 t = s.a;
        s.a = s.b;
        s.b = t;
      }
    }
    if (illegal) {
      s.done = 1;
      s.m = Ones(A);
      return Illegal(loser);
    }
    s.m = (~(s.a | s.b) & Ones(121)) | (s.turn == 1 ? Bit(121) : 0);
    if (s.done) {
      // ColorRewards: the next color (Color()) lost; PlayerRewards maps colors to seats by player_order_
      const int next = s.turn & 1;
      const int seat_of_next = next == 0 ? s.cp : 1 - s.cp;
      rw.r[seat_of_next] = -1.0f;
      rw.r[1 - seat_of_next] = 1.0f;
      s.m = Ones(A);
    }
    return rw;
  } else {  // Othello
    const int loser = s.cp;
    if (in_range) {  // StepGame
      uint64_t my = (uint64_t)s.a, opp = (uint64_t)s.b;
      if (act < 64) {
        const uint64_t flips = OthelloFlips(act, my, opp);
        my |= flips | ((uint64_t)1 << act);
        opp &= ~flips;  // (an occupied cell stays the opponent's too: my and opp both set)
      }
      const uint64_t emp = ~(my | opp);
      // legal moves of the next player on opponent_board: its stones = opp, the mover's = my & ~opp
      const uint64_t legal = OthelloMoves(opp, my & ~opp, emp);
      const bool full = emp == 0, wiped = opp == 0;
      s.done = full || wiped || (s.passed && act == 64);
      if (s.done) {  // GetReward, with the mover as current_player_
        const int mc = Count((u128)my), oc = Count((u128)opp);
        if (mc != oc) {
          const int w = mc > oc ? s.cp : 1 - s.cp;
          rw.r[0] = rw.r[1] = -1.0f;
          rw.r[w] = 1.0f;
        }
      }
      s.a = opp;
      s.b = my & ~opp;
      s.turn = 1 - s.turn;
      s.cp = 1 - s.cp;
      s.passed = act == 64;
      s.m = (u128)legal | (legal == 0 ? Bit(64) : 0);
    }
    if (illegal) {
      s.done = 1;
      s.m = Ones(A);
      return Illegal(loser);
    }
    if (s.done) s.m = Ones(A);
    return rw;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Output.  Key indices: the 8 common keys (device_common.hip.h kKey*), then the game's StateSpec order.
enum Key : int {
  kEnvId = 0, kPlayersEnvId, kElapsed, kDone, kReward, kDiscount, kStepType, kTrunc,
  kObs, kBoard, kCurrentPlayer, kMask, kPlayersId, kNumKeys
};

// What the rows of one env show after a reset or step.
struct View {
  State s;
  float reward[2];
  int32_t env_id, elapsed;
  int32_t step_type;
  uint8_t done, trunc, pad[2];
};

template <int G>
PGX_HD constexpr int ObsElems() {
  return kPlayers * Dims<G>::H * Dims<G>::W * Dims<G>::C;
}
// elements per env row of each key: the per-player keys carry the leading player dimension
template <int G>
PGX_HD constexpr int RowElems(int key) {
  return key == kObs ? ObsElems<G>() : key == kBoard ? Dims<G>::H * Dims<G>::W : key == kMask ? Dims<G>::A
         : (key == kPlayersEnvId || key == kReward || key == kDiscount || key == kPlayersId) ? kPlayers : 1;
}
PGX_HD constexpr int ElemBytes(int key) { return (key == kDone || key == kTrunc || key == kObs || key == kMask) ? 1 : 4; }

PGX_HD inline uint32_t FloatBits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

// Hex's current player: player_order_[Color()]
PGX_HD inline int HexCurrent(const State& s) { return (s.turn & 1) == 0 ? s.cp : 1 - s.cp; }

// element `e` of `key` in the rows of the env `v` (raw bits: a bool as 0 / 1, a float's bit pattern)
template <int G>
PGX_HD uint32_t Elem(const View& v, int key, int e) {
  const State& s = v.s;
  switch (key) {
    case kEnvId: case kPlayersEnvId: return (uint32_t)v.env_id;
    case kElapsed: return (uint32_t)v.elapsed;
    case kDone: return v.done;
    case kReward: return FloatBits(v.reward[e]);
    case kDiscount: return e == 0 && !v.done ? FloatBits(1.0f) : 0u;  // Allocate writes the first row only
    case kStepType: return (uint32_t)v.step_type;
    case kTrunc: return v.trunc;
    case kCurrentPlayer: return (uint32_t)(G == kHex ? HexCurrent(s) : s.cp);
    case kMask: return Has(s.m, e) ? 1u : 0u;
    case kPlayersId: return (uint32_t)e;
    case kBoard:
      if (G == kTicTacToe || G == kConnectFour) return Has(s.a, e) ? 0u : Has(s.b, e) ? 1u : (uint32_t)-1;
      return Has(s.a, e) ? 1u : Has(s.b, e) ? (uint32_t)-1 : 0u;
    default: {  // kObs [player][H][W][C]
      constexpr int C = Dims<G>::C, HW = Dims<G>::H * Dims<G>::W;
      const int p = e / (HW * C), cell = (e / C) % HW, ch = e % C;
      if (G == kTicTacToe || G == kConnectFour) {
        const int my_color = p == s.cp ? s.turn : 1 - s.turn;
        const int want = ch == 0 ? my_color : 1 - my_color;
        return Has(want == 0 ? s.a : s.b, cell) ? 1u : 0u;
      }
      const bool cur = p == (G == kHex ? HexCurrent(s) : s.cp);
      if (ch == 0) return Has(cur ? s.a : s.b, cell) ? 1u : 0u;
      if (ch == 1) return Has(cur ? s.b : s.a, cell) ? 1u : 0u;
      if (ch == 2) return (cur ? (s.turn & 1) : 1 - (s.turn & 1)) == 1 ? 1u : 0u;  // Hex: color == 1
      return s.turn == 1 ? 1u : 0u;                                               // Hex: can_swap
    }
  }
}

// The step's common keys (Env::Allocate): done, step type, trunc against max_episode_steps
PGX_HD inline void Finish(View& v, int env_id, int elapsed, Rewards rw, int max_episode_steps) {
  v.env_id = env_id;
  v.elapsed = elapsed;
  v.done = v.s.done ? 1 : 0;
  v.reward[0] = rw.r[0];
  v.reward[1] = rw.r[1];
  v.step_type = elapsed == 0 ? 0 : v.s.done ? 2 : 1;
  v.trunc = (v.s.done && elapsed >= max_episode_steps) ? 1 : 0;
}

// The hidden state the fixtures record per env (int32 words): the reference's board (TicTacToe / ConnectFour:
// the color or -1; Hex: the sign of its labels; Othello: +1 / -1 / 0 from the side to move), then
// TicTacToe / ConnectFour color_ current_player_; Hex step_count_ player_order_[0]; Othello turn_
// current_player_ passed_
template <int G>
PGX_HD constexpr int HiddenWords() {
  return Dims<G>::H * Dims<G>::W + (G == kOthello ? 3 : 2);
}
template <int G>
PGX_HD void Hidden(const State& s, int32_t* w) {
  constexpr int cells = Dims<G>::H * Dims<G>::W;
  View v{};
  v.s = s;
  for (int i = 0; i < cells; ++i) w[i] = (int32_t)Elem<G>(v, kBoard, i);
  w[cells] = s.turn;
  w[cells + 1] = s.cp;
  if (G == kOthello) w[cells + 2] = s.passed;
}
// the inverse (set_state); false if the words are no state of the game
template <int G>
PGX_HD bool SetHidden(State& s, const int32_t* w) {
  constexpr int cells = Dims<G>::H * Dims<G>::W;
  const bool color_board = G == kTicTacToe || G == kConnectFour;
  s.a = s.b = 0;
  for (int i = 0; i < cells; ++i) {
    const int32_t x = w[i];
    if (x == (color_board ? 0 : 1)) {
      s.a |= Bit(i);
    } else if (x == (color_board ? 1 : -1)) {
      s.b |= Bit(i);
    } else if (x != (color_board ? -1 : 0)) {
      return false;
    }
  }
  s.turn = w[cells];
  s.cp = w[cells + 1];
  s.passed = G == kOthello ? w[cells + 2] : 0;
  if (s.cp < 0 || s.cp > 1 || s.turn < 0 || (G != kHex && s.turn > 1)) return false;
  // the mask the next step checks, as the last legal step left it
  const u128 occ = s.a | s.b;
  if (G == kTicTacToe) {
    s.m = ~occ & Ones(cells);
  } else if (G == kConnectFour) {
    u128 m = 0;
    for (int c = 0; c < 7; ++c) m |= (u128)(Count(occ & ColumnMask(c, 7, 6)) < 6) << c;
    s.m = m;
  } else if (G == kHex) {
    s.m = (~occ & Ones(121)) | (s.turn == 1 ? Bit(121) : 0);
  } else {
    const uint64_t legal = OthelloMoves((uint64_t)s.a, (uint64_t)s.b, ~(uint64_t)occ);
    s.m = (u128)legal | (legal == 0 ? Bit(64) : 0);
  }
  return true;
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_ENV_HIP_H_
