// Fixture driver for tests/golden/make_jumanji_golden.py (not product code, not built by build()).
//
// Includes the reference's own Jumanji board-puzzle headers in place and drives each env through its own
// AsyncEnvPool (sync mode) exactly like the Python binding does: Reset(all) -> Recv(), then
// Send(env_id, players.env_id, action) -> Recv() per step, auto-reset included.  A subclass of each env
// reads its hidden state (board, mines, snake body, walls, positions, step count) after every Recv.
// Env 0 may be steered with that hidden state (reveal a safe cell, take the move that solves the puzzle,
// walk to the fruit or the target); the actions actually sent are written back.
//
//   driver spec <puzzle> <key=value>...                                  -> JSON config defaults + specs
//   driver run  <puzzle> <out_dir> <steps> <actions.bin> <steer> <key=value>...  -> raw arrays in out_dir
//
// <puzzle>: Game2048 Minesweeper SlidingTilePuzzle RubiksCube RubiksCubePartlyScrambled Snake Maze
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <queue>
#include <sstream>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "envpool/jumanji/game2048_env.h"
#include "envpool/jumanji/maze_env.h"
#include "envpool/jumanji/minesweeper_env.h"
#include "envpool/jumanji/rubiks_cube_env.h"
#include "envpool/jumanji/sliding_tile_puzzle_env.h"
#include "envpool/jumanji/snake_env.h"

namespace {

template <typename T>
std::string Json(const T& v) {
  std::ostringstream s;
  if constexpr (std::is_same_v<T, std::string>) {
    s << '"' << v << '"';
  } else if constexpr (std::is_same_v<T, bool>) {
    s << (v ? "true" : "false");
  } else if constexpr (std::is_same_v<T, std::vector<int>>) {
    s << '[';
    for (size_t i = 0; i < v.size(); ++i) s << (i ? ", " : "") << v[i];
    s << ']';
  } else if constexpr (std::is_floating_point_v<T>) {
    s.precision(9);
    s << v;
  } else {
    s << +v;
  }
  return s.str();
}

template <typename D>
const char* Dtype() {
  if (std::is_same_v<D, int>) return "int32";
  if (std::is_same_v<D, float>) return "float32";
  if (std::is_same_v<D, bool>) return "bool";
  if (std::is_same_v<D, uint8_t>) return "uint8";
  if (std::is_same_v<D, int8_t>) return "int8";
  if (std::is_same_v<D, double>) return "float64";
  return "?";
}

template <typename S>
std::string SpecJson(const S& sp) {
  using D = typename S::dtype;
  std::ostringstream s;
  s << "{\"dtype\": \"" << Dtype<D>() << "\", \"shape\": " << Json(sp.shape) << ", \"bounds\": ["
    << Json(std::get<0>(sp.bounds)) << ", " << Json(std::get<1>(sp.bounds)) << "], \"elementwise\": [[";
  const auto& lo = std::get<0>(sp.elementwise_bounds);
  const auto& hi = std::get<1>(sp.elementwise_bounds);
  for (size_t i = 0; i < lo.size(); ++i) s << (i ? ", " : "") << Json(lo[i]);
  s << "], [";
  for (size_t i = 0; i < hi.size(); ++i) s << (i ? ", " : "") << Json(hi[i]);
  s << "]]}";
  return s.str();
}

// the driver's view of an env's hidden state: int32 words, appended to `w`
struct G2048Probe : jumanji::Game2048Env {
  using jumanji::Game2048Env::Game2048Env;
  void Hidden(std::vector<int32_t>* w) const { w->insert(w->end(), board_.begin(), board_.end()); }
};
struct MinesProbe : jumanji::MinesweeperEnv {
  using jumanji::MinesweeperEnv::MinesweeperEnv;
  void Hidden(std::vector<int32_t>* w) const {
    w->insert(w->end(), board_.begin(), board_.end());
    for (bool m : mines_) w->push_back(m);
    w->push_back(num_mines_);
    w->push_back(step_count_);
  }
  // a safe unexplored cell, or -1
  int Safe() const {
    for (int i = 0; i < 100; ++i) {
      if (board_[i] == -1 && !mines_[i]) return i;
    }
    return -1;
  }
};
struct TileProbe : jumanji::SlidingTilePuzzleEnv {
  using jumanji::SlidingTilePuzzleEnv::SlidingTilePuzzleEnv;
  void Hidden(std::vector<int32_t>* w) const {
    w->insert(w->end(), puzzle_.begin(), puzzle_.end());
    w->push_back(empty_row_);
    w->push_back(empty_col_);
    w->push_back(step_count_);
  }
  int Solving() const {
    namespace s = jumanji::sliding_tile_puzzle;
    for (int a = 0; a < 4; ++a) {
      const int r = empty_row_ + s::kMoves[a][0], c = empty_col_ + s::kMoves[a][1];
      if (!s::InGrid(r, c)) continue;
      auto p = puzzle_;
      std::swap(p[s::Offset(empty_row_, empty_col_)], p[s::Offset(r, c)]);
      if (p == s::SolvedPuzzle()) return a;
    }
    return -1;
  }
};
template <typename Base>
struct CubeProbe : Base {
  using Base::Base;
  void Hidden(std::vector<int32_t>* w) const {
    w->insert(w->end(), this->cube_.begin(), this->cube_.end());
    w->push_back(this->step_count_);
  }
  int Solving() const {  // face * 3 + amount, or -1
    for (int m = 0; m < 18; ++m) {
      auto c = this->cube_;
      jumanji::rubiks_cube::Rotate(&c, m / 3, m % 3);
      if (jumanji::rubiks_cube::IsSolved(c)) return m;
    }
    return -1;
  }
};
using CubeProbeA = CubeProbe<jumanji::RubiksCubeEnv>;
using CubeProbeB = CubeProbe<jumanji::RubiksCubePartlyScrambledEnv>;
struct SnakeProbe : jumanji::SnakeEnv {
  using jumanji::SnakeEnv::SnakeEnv;
  void Hidden(std::vector<int32_t>* w) const {
    w->insert(w->end(), body_state_.begin(), body_state_.end());
    for (int v : {head_row_, head_col_, tail_row_, tail_col_, fruit_row_, fruit_col_, length_, step_count_}) {
      w->push_back(v);
    }
  }
  int Greedy() const {  // the valid move that ends nearest the fruit, or -1
    namespace s = jumanji::snake;
    int best = -1, best_d = 1 << 20;
    for (int a = 0; a < 4; ++a) {
      const int r = head_row_ + s::kMoves[a][0], c = head_col_ + s::kMoves[a][1];
      if (!s::InGrid(r, c) || body_state_[s::Offset(r, c)] > 1) continue;
      const int d = std::abs(r - fruit_row_) + std::abs(c - fruit_col_);
      if (d < best_d) best = a, best_d = d;
    }
    return best;
  }
};
struct MazeProbe : jumanji::MazeEnv {
  using jumanji::MazeEnv::MazeEnv;
  void Hidden(std::vector<int32_t>* w) const {
    for (bool b : walls_) w->push_back(b);
    for (int v : {agent_row_, agent_col_, target_row_, target_col_, step_count_}) w->push_back(v);
  }
  int Toward() const {  // first move of a shortest path to the target, or -1
    namespace m = jumanji::maze;
    std::array<int, 100> first{};
    first.fill(-2);
    std::queue<int> q;
    first[m::Offset(agent_row_, agent_col_)] = -1;
    q.push(m::Offset(agent_row_, agent_col_));
    while (!q.empty()) {
      const int o = q.front();
      q.pop();
      if (o == m::Offset(target_row_, target_col_)) return first[o];
      for (int a = 0; a < 4; ++a) {
        const int r = o / 10 + m::kMoves[a][0], c = o % 10 + m::kMoves[a][1];
        if (!m::InGrid(r, c) || walls_[m::Offset(r, c)] || first[m::Offset(r, c)] != -2) continue;
        first[m::Offset(r, c)] = first[o] == -1 ? a : first[o];
        q.push(m::Offset(r, c));
      }
    }
    return -1;
  }
};

template <typename Env>
struct ProbePool : AsyncEnvPool<Env> {
  using AsyncEnvPool<Env>::AsyncEnvPool;
  const Env& At(int i) const { return *this->envs_[i]; }
};

// env 0's action from its hidden state in place of the seeded one; the seeded one where no move qualifies
void Steer(const G2048Probe&, int32_t*) {}
void Steer(const MinesProbe& e, int32_t* a) {
  const int s = e.Safe();
  if (s >= 0) a[0] = s / 10, a[1] = s % 10;
}
void Steer(const TileProbe& e, int32_t* a) {
  const int m = e.Solving();
  if (m >= 0) a[0] = m;
}
template <typename B>
void Steer(const CubeProbe<B>& e, int32_t* a) {
  const int m = e.Solving();
  if (m >= 0) a[0] = m / 3, a[1] = 0, a[2] = m % 3;
}
void Steer(const SnakeProbe& e, int32_t* a) {
  const int m = e.Greedy();
  if (m >= 0) a[0] = m;
}
void Steer(const MazeProbe& e, int32_t* a) {
  const int m = e.Toward();
  if (m >= 0) a[0] = m;
}

template <typename Env, typename Conf>
void SetKey(Conf& c, const std::string& k, const std::string& v) {
  bool ok = true;
  if (k == "num_envs") c["num_envs"_] = std::stoi(v);
  else if (k == "batch_size") c["batch_size"_] = std::stoi(v);
  else if (k == "seed") c["seed"_] = std::stoi(v);
  else if (k == "max_episode_steps") c["max_episode_steps"_] = std::stoi(v);
  else if constexpr (std::is_base_of_v<jumanji::Game2048Env, Env>) {
    if (k == "game2048_initial_board") c["game2048_initial_board"_] = v;
    else if (k == "game2048_add_random_cell") c["game2048_add_random_cell"_] = v == "1" || v == "True";
    else ok = false;
  } else if constexpr (std::is_base_of_v<jumanji::MinesweeperEnv, Env>) {
    if (k == "minesweeper_mine_locations") c["minesweeper_mine_locations"_] = v;
    else ok = false;
  } else if constexpr (std::is_base_of_v<jumanji::SlidingTilePuzzleEnv, Env>) {
    if (k == "sliding_tile_initial_puzzle") c["sliding_tile_initial_puzzle"_] = v;
    else ok = false;
  } else if constexpr (std::is_base_of_v<jumanji::SnakeEnv, Env>) {
    if (k == "snake_head_position") c["snake_head_position"_] = v;
    else if (k == "snake_fruit_position") c["snake_fruit_position"_] = v;
    else ok = false;
  } else if constexpr (std::is_base_of_v<jumanji::MazeEnv, Env>) {
    if (k == "maze_walls") c["maze_walls"_] = v;
    else if (k == "maze_agent_position") c["maze_agent_position"_] = v;
    else if (k == "maze_target_position") c["maze_target_position"_] = v;
    else ok = false;
  } else {  // the two RubiksCube specs
    if (k == "rubiks_cube_initial_cube") c["rubiks_cube_initial_cube"_] = v;
    else if (k == "rubiks_cube_num_scrambles") c["rubiks_cube_num_scrambles"_] = std::stoi(v);
    else ok = false;
  }
  if (!ok) {
    std::cerr << "unknown key " << k << "\n";
    std::exit(2);
  }
}

template <typename Env>
typename Env::Spec::Config MakeConfig(int argc, char** argv, int first) {
  auto c = Env::Spec::kDefaultConfig;
  for (int i = first; i < argc; ++i) {
    std::string a(argv[i]);
    auto eq = a.find('=');
    SetKey<Env>(c, a.substr(0, eq), a.substr(eq + 1));
  }
  return c;
}

template <typename Env>
void DumpSpec(int argc, char** argv) {
  using S = typename Env::Spec;
  S spec(MakeConfig<Env>(argc, argv, 3));
  std::cout << "{\"default_config\": [";
  {
    auto keys = S::Config::AllKeys();
    auto vals = S::kDefaultConfig.AllValues();
    size_t i = 0;
    std::apply([&](auto&&... v) { ((std::cout << (i ? ", " : "") << "[\"" << keys[i] << "\", " << Json(v) << "]", ++i), ...); },
               vals);
  }
  std::cout << "], \"state_spec\": [";
  {
    auto keys = S::StateSpec::AllKeys();
    size_t i = 0;
    std::apply([&](auto&&... s) { ((std::cout << (i ? ", " : "") << "[\"" << keys[i] << "\", " << SpecJson(s) << "]", ++i), ...); },
               spec.state_spec.AllValues());
  }
  std::cout << "], \"action_spec\": [";
  {
    auto keys = S::ActionSpec::AllKeys();
    size_t i = 0;
    std::apply([&](auto&&... s) { ((std::cout << (i ? ", " : "") << "[\"" << keys[i] << "\", " << SpecJson(s) << "]", ++i), ...); },
               spec.action_spec.AllValues());
  }
  std::cout << "]}\n";
}

template <typename Env>
void Run(int argc, char** argv, int act_dim) {
  using S = typename Env::Spec;
  std::string out = argv[3];
  const int steps = std::stoi(argv[4]);
  const bool steer = std::stoi(argv[6]) != 0;
  auto conf = MakeConfig<Env>(argc, argv, 7);
  conf["num_threads"_] = 1;
  const int n = conf["num_envs"_];
  conf["batch_size"_] = n;
  std::vector<int32_t> acts((size_t)steps * n * act_dim);
  {
    std::ifstream f(argv[5], std::ios::binary);
    f.read(reinterpret_cast<char*>(acts.data()), acts.size() * 4);
    if (!f) {
      std::cerr << "short actions file\n";
      std::exit(2);
    }
  }
  S spec(conf);
  ProbePool<Env> pool(spec);
  auto keys = S::StateSpec::AllKeys();
  std::vector<std::ofstream> files;
  for (auto& k : keys) files.emplace_back(out + "/" + k + ".bin", std::ios::binary);
  std::ofstream names(out + "/keys.txt");
  for (auto& k : keys) names << k << "\n";
  std::ofstream hid(out + "/hidden.bin", std::ios::binary);
  std::vector<int> all(n);
  for (int i = 0; i < n; ++i) all[i] = i;
  auto dump = [&](const std::vector<Array>& ret) {
    for (size_t i = 0; i < ret.size(); ++i) {
      files[i].write(static_cast<const char*>(ret[i].Data()), ret[i].size * ret[i].element_size);
    }
    for (int e = 0; e < n; ++e) {
      std::vector<int32_t> w;
      pool.At(e).Hidden(&w);
      hid.write(reinterpret_cast<const char*>(w.data()), w.size() * 4);
    }
  };
  Array ids(::Spec<int>({n}));
  std::memcpy(ids.Data(), all.data(), 4 * n);
  pool.Reset(ids);
  dump(pool.Recv());
  for (int t = 0; t < steps; ++t) {
    int32_t* a = acts.data() + (size_t)t * n * act_dim;
    if (steer) Steer(pool.At(0), a);
    std::vector<Array> raw({Array(::Spec<int>({n})), Array(::Spec<int>({n})),
                            act_dim == 1 ? Array(::Spec<int>({n})) : Array(::Spec<int>({n, act_dim}))});
    std::memcpy(raw[0].Data(), all.data(), 4 * n);
    std::memcpy(raw[1].Data(), all.data(), 4 * n);
    std::memcpy(raw[2].Data(), a, 4 * n * act_dim);
    pool.Send(raw);
    dump(pool.Recv());
  }
  std::ofstream used(out + "/actions_used.bin", std::ios::binary);
  used.write(reinterpret_cast<const char*>(acts.data()), acts.size() * 4);
}

template <typename Env>
int Main(int argc, char** argv, int act_dim) {
  const std::string cmd = argv[1];
  if (cmd == "spec") {
    DumpSpec<Env>(argc, argv);
  } else if (cmd == "run" && argc >= 7) {
    Run<Env>(argc, argv, act_dim);
  } else {
    return 2;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: driver spec <puzzle> k=v... | driver run <puzzle> out_dir steps actions.bin steer k=v...\n";
    return 2;
  }
  const std::string p = argv[2];
  if (p == "Game2048") return Main<G2048Probe>(argc, argv, 1);
  if (p == "Minesweeper") return Main<MinesProbe>(argc, argv, 2);
  if (p == "SlidingTilePuzzle") return Main<TileProbe>(argc, argv, 1);
  if (p == "RubiksCube") return Main<CubeProbeA>(argc, argv, 3);
  if (p == "RubiksCubePartlyScrambled") return Main<CubeProbeB>(argc, argv, 3);
  if (p == "Snake") return Main<SnakeProbe>(argc, argv, 1);
  if (p == "Maze") return Main<MazeProbe>(argc, argv, 1);
  std::cerr << "unknown puzzle " << p << "\n";
  return 2;
}
