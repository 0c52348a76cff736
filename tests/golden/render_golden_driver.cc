// Fixture driver for tests/golden/make_render_golden.py (not product code, not built by build()).
//
// Includes the reference's Jumanji board puzzles and PGX board games in place and drives each through its own
// AsyncEnvPool (sync mode, one thread) with a seeded policy: Reset(all) -> Recv(), then Send -> Recv() per step,
// auto-reset included.  A subclass of each env reads its hidden state after every Recv, in the word order of this
// engine's get_state (Hex: the sign of the union-find labels).  For the picked (step, env) pairs it also stores
// the frame pool.Render returns for that env at every listed size.
//
//   driver run <game> <out_dir> <n> <steps> <seed> <policy_seed> <picks> <sizes> <key=value>...
//       picks: "-" or "t:e,t:e,..."        sizes: "0x0,61x45,..." (width x height)
//       -> out_dir/hidden.bin  int32 [steps + 1, n, words]
//          out_dir/frame_<pick>_<size>.bin  uint8 [H, W, 3], out_dir/sizes.txt  the resolved "W H" per size
//   driver bench <game> <n> <threads> <reps>   -> JSON frames/s of pool.Render(all n envs) at the default size
//
// Jumanji: env 0 is steered with its hidden state (reveal a safe cell, walk to the fruit / the target); the other
// envs act at random.  PGX: a legal action drawn uniformly from the env's legal action mask.
//
// <game>: Game2048 Minesweeper SlidingTilePuzzle RubiksCube Snake Maze TicTacToe ConnectFour Hex Othello
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <numeric>
#include <queue>
#include <random>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "envpool/core/async_envpool.h"
#include "envpool/core/env.h"
#include "envpool/jumanji/game2048_env.h"
#include "envpool/jumanji/maze_env.h"
#include "envpool/jumanji/minesweeper_env.h"
#include "envpool/jumanji/rubiks_cube_env.h"
#include "envpool/jumanji/sliding_tile_puzzle_env.h"
#include "envpool/jumanji/snake_env.h"
// the board games keep their state private; the probes below read it
#define private protected
#include "envpool/pgx/board_games.h"
#undef private

namespace {

using Words = std::vector<int32_t>;
using Rng = std::mt19937;

// ---- probes: Hidden (get_state's word order), the action's width, a seeded action, env 0's steering --------------
struct G2048Probe : jumanji::Game2048Env {
  using jumanji::Game2048Env::Game2048Env;
  static constexpr int kActDim = 1, kPlayers = 1;
  void Hidden(Words* w) const { w->insert(w->end(), board_.begin(), board_.end()); }
  static void Act(Rng& g, int32_t* a) { a[0] = (int)(g() % 4); }
  void Steer(int32_t*) const {}
};
struct MinesProbe : jumanji::MinesweeperEnv {
  using jumanji::MinesweeperEnv::MinesweeperEnv;
  static constexpr int kActDim = 2, kPlayers = 1;
  void Hidden(Words* w) const {
    w->insert(w->end(), board_.begin(), board_.end());
    for (bool m : mines_) w->push_back(m);
    w->push_back(num_mines_);
    w->push_back(step_count_);
  }
  static void Act(Rng& g, int32_t* a) { a[0] = (int)(g() % 10), a[1] = (int)(g() % 10); }
  void Steer(int32_t* a) const {  // a safe unexplored cell, taken from a seeded start so the board opens unevenly
    const int start = (a[0] * 10 + a[1]) % 100;
    for (int j = 0; j < 100; ++j) {
      const int i = (start + j) % 100;
      if (board_[i] == -1 && !mines_[i]) {
        a[0] = i / 10, a[1] = i % 10;
        return;
      }
    }
  }
};
struct TileProbe : jumanji::SlidingTilePuzzleEnv {
  using jumanji::SlidingTilePuzzleEnv::SlidingTilePuzzleEnv;
  static constexpr int kActDim = 1, kPlayers = 1;
  void Hidden(Words* w) const {
    w->insert(w->end(), puzzle_.begin(), puzzle_.end());
    w->push_back(empty_row_);
    w->push_back(empty_col_);
    w->push_back(step_count_);
  }
  static void Act(Rng& g, int32_t* a) { a[0] = (int)(g() % 4); }
  void Steer(int32_t*) const {}
};
struct CubeProbe : jumanji::RubiksCubeEnv {
  using jumanji::RubiksCubeEnv::RubiksCubeEnv;
  static constexpr int kActDim = 3, kPlayers = 1;
  void Hidden(Words* w) const {
    w->insert(w->end(), cube_.begin(), cube_.end());
    w->push_back(step_count_);
  }
  static void Act(Rng& g, int32_t* a) { a[0] = (int)(g() % 6), a[1] = 0, a[2] = (int)(g() % 3); }
  void Steer(int32_t*) const {}
};
struct SnakeProbe : jumanji::SnakeEnv {
  using jumanji::SnakeEnv::SnakeEnv;
  static constexpr int kActDim = 1, kPlayers = 1;
  void Hidden(Words* w) const {
    w->insert(w->end(), body_state_.begin(), body_state_.end());
    for (int v : {head_row_, head_col_, tail_row_, tail_col_, fruit_row_, fruit_col_, length_, step_count_}) {
      w->push_back(v);
    }
  }
  static void Act(Rng& g, int32_t* a) { a[0] = (int)(g() % 4); }
  void Steer(int32_t* a) const {  // the valid move that ends nearest the fruit
    namespace s = jumanji::snake;
    int best_d = 1 << 20;
    for (int m = 0; m < 4; ++m) {
      const int r = head_row_ + s::kMoves[m][0], c = head_col_ + s::kMoves[m][1];
      if (!s::InGrid(r, c) || body_state_[s::Offset(r, c)] > 1) continue;
      const int d = std::abs(r - fruit_row_) + std::abs(c - fruit_col_);
      if (d < best_d) a[0] = m, best_d = d;
    }
  }
};
struct MazeProbe : jumanji::MazeEnv {
  using jumanji::MazeEnv::MazeEnv;
  static constexpr int kActDim = 1, kPlayers = 1;
  void Hidden(Words* w) const {
    for (bool b : walls_) w->push_back(b);
    for (int v : {agent_row_, agent_col_, target_row_, target_col_, step_count_}) w->push_back(v);
  }
  static void Act(Rng& g, int32_t* a) { a[0] = (int)(g() % 4); }
  void Steer(int32_t* a) const {  // the first move of a shortest path to the target, if there is one
    namespace m = jumanji::maze;
    std::array<int, 100> first{};
    first.fill(-2);
    std::queue<int> q;
    first[m::Offset(agent_row_, agent_col_)] = -1;
    q.push(m::Offset(agent_row_, agent_col_));
    while (!q.empty()) {
      const int o = q.front();
      q.pop();
      if (o == m::Offset(target_row_, target_col_)) {
        if (first[o] >= 0) a[0] = first[o];
        return;
      }
      for (int d = 0; d < 4; ++d) {
        const int r = o / 10 + m::kMoves[d][0], c = o % 10 + m::kMoves[d][1];
        if (!m::InGrid(r, c) || walls_[m::Offset(r, c)] || first[m::Offset(r, c)] != -2) continue;
        first[m::Offset(r, c)] = first[o] == -1 ? d : first[o];
        q.push(m::Offset(r, c));
      }
    }
  }
};

struct TicTacToeProbe : pgx::TicTacToeEnv {
  using pgx::TicTacToeEnv::TicTacToeEnv;
  static constexpr int kActDim = 1, kPlayers = 2, kActions = 9;
  void Hidden(Words* w) const {
    w->insert(w->end(), board_.begin(), board_.end());
    w->push_back(color_);
    w->push_back(current_player_);
  }
};
struct ConnectFourProbe : pgx::ConnectFourEnv {
  using pgx::ConnectFourEnv::ConnectFourEnv;
  static constexpr int kActDim = 1, kPlayers = 2, kActions = 7;
  void Hidden(Words* w) const {
    w->insert(w->end(), board_.begin(), board_.end());
    w->push_back(color_);
    w->push_back(current_player_);
  }
};
struct HexProbe : pgx::HexEnv {
  using pgx::HexEnv::HexEnv;
  static constexpr int kActDim = 1, kPlayers = 2, kActions = 122;
  void Hidden(Words* w) const {
    for (int v : board_) w->push_back(v > 0 ? 1 : v < 0 ? -1 : 0);
    w->push_back(step_count_);
    w->push_back(player_order_[0]);
  }
};
struct OthelloProbe : pgx::OthelloEnv {
  using pgx::OthelloEnv::OthelloEnv;
  static constexpr int kActDim = 1, kPlayers = 2, kActions = 65;
  void Hidden(Words* w) const {
    w->insert(w->end(), board_.begin(), board_.end());
    w->push_back(turn_);
    w->push_back(current_player_);
    w->push_back(passed_);
  }
};

template <typename Env>
struct ProbePool : AsyncEnvPool<Env> {
  using AsyncEnvPool<Env>::AsyncEnvPool;
  const Env& At(int i) const { return *this->envs_[i]; }
};

template <typename Env>
typename Env::Spec::Config MakeConfig(int argc, char** argv, int first, int n, int threads, int seed) {
  auto c = Env::Spec::kDefaultConfig;
  c["num_envs"_] = n;
  c["batch_size"_] = n;
  c["num_threads"_] = threads;
  c["seed"_] = seed;
  if constexpr (Env::kPlayers == 2) c["max_num_players"_] = 2;
  for (int i = first; i < argc; ++i) {
    const std::string a(argv[i]);
    const auto eq = a.find('=');
    const std::string k = a.substr(0, eq), v = a.substr(eq + 1);
    bool ok = false;
    if constexpr (std::is_base_of_v<jumanji::Game2048Env, Env>) {
      if (k == "game2048_initial_board") c["game2048_initial_board"_] = v, ok = true;
    }
    if (!ok) {
      std::cerr << "unknown key " << k << "\n";
      std::exit(2);
    }
  }
  return c;
}

std::vector<std::string> Split(const std::string& s, char sep) {
  std::vector<std::string> out;
  std::stringstream ss(s);
  std::string item;
  while (std::getline(ss, item, sep)) out.push_back(item);
  return out;
}

Array Ids(const std::vector<int32_t>& v) {
  Array a(::Spec<int>({(int)v.size()}));
  std::memcpy(a.Data(), v.data(), 4 * v.size());
  return a;
}

template <typename Env>
void Run(int argc, char** argv) {
  using S = typename Env::Spec;
  const std::string out = argv[3];
  const int n = std::stoi(argv[4]), steps = std::stoi(argv[5]);
  Rng policy((uint32_t)std::stoul(argv[7]));
  std::vector<std::pair<int, int>> picks;
  if (std::string(argv[8]) != "-") {
    for (const auto& p : Split(argv[8], ',')) {
      const auto te = Split(p, ':');
      picks.emplace_back(std::stoi(te[0]), std::stoi(te[1]));
    }
  }
  std::vector<std::pair<int, int>> sizes;
  for (const auto& s : Split(argv[9], ',')) {
    const auto wh = Split(s, 'x');
    sizes.emplace_back(std::stoi(wh[0]), std::stoi(wh[1]));
  }
  S spec(MakeConfig<Env>(argc, argv, 10, n, 1, std::stoi(argv[6])));
  ProbePool<Env> pool(spec);
  auto keys = S::StateSpec::AllKeys();
  int mask_key = -1;
  for (size_t i = 0; i < keys.size(); ++i) {
    if (keys[i] == "info:legal_action_mask") mask_key = (int)i;
  }
  std::ofstream hid(out + "/hidden.bin", std::ios::binary);
  std::ofstream resolved(out + "/sizes.txt");
  std::vector<int32_t> all(n);
  std::iota(all.begin(), all.end(), 0);
  std::vector<std::vector<char>> mask;
  auto after = [&](int t, const std::vector<Array>& ret) {
    for (int e = 0; e < n; ++e) {
      Words w;
      pool.At(e).Hidden(&w);
      hid.write(reinterpret_cast<const char*>(w.data()), w.size() * 4);
    }
    if constexpr (Env::kPlayers == 2) {  // rows come back in completion order: info:env_id is key 0
      const int* ids = static_cast<const int*>(ret[0].Data());
      const bool* m = static_cast<const bool*>(ret[mask_key].Data());
      mask.assign(n, std::vector<char>(Env::kActions, 0));
      for (int r = 0; r < n; ++r) {
        for (int a = 0; a < Env::kActions; ++a) mask[ids[r]][a] = m[(size_t)r * Env::kActions + a];
      }
    }
    for (size_t p = 0; p < picks.size(); ++p) {
      if (picks[p].first != t) continue;
      for (size_t s = 0; s < sizes.size(); ++s) {
        Array frame = pool.Render(Ids({picks[p].second}), sizes[s].first, sizes[s].second, -1);
        std::ofstream f(out + "/frame_" + std::to_string(p) + "_" + std::to_string(s) + ".bin", std::ios::binary);
        f.write(static_cast<const char*>(frame.Data()), frame.size * frame.element_size);
        if (p == 0) resolved << frame.Shape(2) << " " << frame.Shape(1) << "\n";
      }
    }
  };
  pool.Reset(Ids(all));
  after(0, pool.Recv());
  constexpr int D = Env::kActDim;
  for (int t = 0; t < steps; ++t) {
    std::vector<int32_t> a((size_t)n * D, 0);
    for (int e = 0; e < n; ++e) {
      if constexpr (Env::kPlayers == 2) {
        std::vector<int> legal;
        for (int j = 0; j < Env::kActions; ++j) {
          if (mask[e][j]) legal.push_back(j);
        }
        a[e] = legal.empty() ? 0 : legal[policy() % legal.size()];
      } else {
        Env::Act(policy, a.data() + (size_t)e * D);
        if (e == 0) pool.At(0).Steer(a.data());
      }
    }
    std::vector<Array> raw({Ids(all), Ids(all), D == 1 ? Array(::Spec<int>({n})) : Array(::Spec<int>({n, D}))});
    std::memcpy(raw[2].Data(), a.data(), 4 * a.size());
    pool.Send(raw);
    after(t + 1, pool.Recv());
  }
}

// frames/s of the reference's own pool.Render: all n envs per call at the default size, after one reset
template <typename Env>
void Bench(int argc, char** argv) {
  using S = typename Env::Spec;
  const int n = std::stoi(argv[3]), threads = std::stoi(argv[4]), reps = std::stoi(argv[5]);
  S spec(MakeConfig<Env>(argc, argv, 6, n, threads, 1));
  AsyncEnvPool<Env> pool(spec);
  std::vector<int32_t> all(n);
  std::iota(all.begin(), all.end(), 0);
  pool.Reset(Ids(all));
  (void)pool.Recv();
  const Array ids = Ids(all);
  (void)pool.Render(ids, 0, 0, -1);
  const auto t0 = std::chrono::steady_clock::now();
  size_t bytes = 0;
  for (int r = 0; r < reps; ++r) {
    Array f = pool.Render(ids, 0, 0, -1);
    bytes = f.size * f.element_size;
  }
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::cout << "{\"num_envs\": " << n << ", \"threads\": " << threads << ", \"bytes_per_call\": " << bytes
            << ", \"frames_per_s\": " << (double)n * reps / dt << "}\n";
}

template <typename Env>
int Main(int argc, char** argv) {
  const std::string cmd = argv[1];
  if (cmd == "run" && argc >= 10) {
    Run<Env>(argc, argv);
  } else if (cmd == "bench" && argc >= 6) {
    Bench<Env>(argc, argv);
  } else {
    return 2;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: driver run <game> out_dir n steps seed policy_seed picks sizes k=v... | driver bench "
                 "<game> n threads reps\n";
    return 2;
  }
  const std::string g = argv[2];
  if (g == "Game2048") return Main<G2048Probe>(argc, argv);
  if (g == "Minesweeper") return Main<MinesProbe>(argc, argv);
  if (g == "SlidingTilePuzzle") return Main<TileProbe>(argc, argv);
  if (g == "RubiksCube") return Main<CubeProbe>(argc, argv);
  if (g == "Snake") return Main<SnakeProbe>(argc, argv);
  if (g == "Maze") return Main<MazeProbe>(argc, argv);
  if (g == "TicTacToe") return Main<TicTacToeProbe>(argc, argv);
  if (g == "ConnectFour") return Main<ConnectFourProbe>(argc, argv);
  if (g == "Hex") return Main<HexProbe>(argc, argv);
  if (g == "Othello") return Main<OthelloProbe>(argc, argv);
  std::cerr << "unknown game " << g << "\n";
  return 2;
}
