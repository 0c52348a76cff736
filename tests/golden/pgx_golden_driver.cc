// Fixture driver for tests/golden/make_pgx_golden.py (not product code, not built by build()).
//
// Includes the reference's PGX board games (envpool/pgx/board_games.h) in place and drives each game through its
// own AsyncEnvPool with max_num_players = 2, like the Python binding does: Reset(all) -> Recv(), then
// Send(env_id, players.env_id, action) -> Recv() per step, auto-reset included.  Rows come back in completion
// order; they are put in env id order here (a per-player key's two rows of one env stay together).  A subclass
// of each env reads its hidden state after every Recv: the board and turn, Othello's passed_, Hex's
// player_order_[0].
//
// The actions are picked online from each env's legal action mask by a seeded policy: a legal action drawn
// uniformly, or -- with a per-env probability -- an illegal one of a drawn kind (an occupied cell or a full
// column, -1, one past the action range, Hex's swap off turn 1, Othello's pass while a move exists).
//
//   driver spec <game>                                                  -> JSON config defaults + specs
//   driver run <game> <out_dir> <n> <steps> <seed> <policy_seed> <illegal_permille_of_env>... max_episode_steps=<m>
//   driver replay <game> <out_dir> <n> <steps> <seed> <actions_file> max_episode_steps=<m>
//                 the same outputs for the int32 actions[steps][n] of the file instead of the online policy
//   driver bench <game> <n> <threads> <steps>                           -> JSON env-steps/s of the reference's pool
//
// <game>: TicTacToe ConnectFour Hex Othello
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <numeric>
#include <random>
#include <sstream>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "envpool/core/async_envpool.h"
#include "envpool/core/env.h"
// the games keep their state private; the probes below read it
#define private protected
#include "envpool/pgx/board_games.h"
#undef private

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

// hidden state: int32 words appended to `w`
struct TicTacToeProbe : pgx::TicTacToeEnv {
  using pgx::TicTacToeEnv::TicTacToeEnv;
  static constexpr int kActions = 9, kCells = 9;
  void Hidden(std::vector<int32_t>* w) const {
    w->insert(w->end(), board_.begin(), board_.end());
    w->push_back(color_);
    w->push_back(current_player_);
  }
};
struct ConnectFourProbe : pgx::ConnectFourEnv {
  using pgx::ConnectFourEnv::ConnectFourEnv;
  static constexpr int kActions = 7, kCells = 7;  // "occupied": a full column
  void Hidden(std::vector<int32_t>* w) const {
    w->insert(w->end(), board_.begin(), board_.end());
    w->push_back(color_);
    w->push_back(current_player_);
  }
};
struct HexProbe : pgx::HexEnv {
  using pgx::HexEnv::HexEnv;
  static constexpr int kActions = 122, kCells = 121;
  void Hidden(std::vector<int32_t>* w) const {  // the raw union-find labels
    w->insert(w->end(), board_.begin(), board_.end());
    w->push_back(step_count_);
    w->push_back(player_order_[0]);
  }
};
struct OthelloProbe : pgx::OthelloEnv {
  using pgx::OthelloEnv::OthelloEnv;
  static constexpr int kActions = 65, kCells = 64;
  void Hidden(std::vector<int32_t>* w) const {
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
void DumpSpec() {
  using S = typename Env::Spec;
  auto conf = S::kDefaultConfig;
  S spec(conf);
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

// an action for a mask (all true after a terminal step: the action is then ignored by the reset)
template <typename Env>
int Pick(std::mt19937& g, const bool* mask, int permille) {
  constexpr int A = Env::kActions;
  std::vector<int> legal, occupied;
  for (int a = 0; a < Env::kCells; ++a) (mask[a] ? legal : occupied).push_back(a);
  for (int a = Env::kCells; a < A; ++a) {
    if (mask[a]) legal.push_back(a);
  }
  if ((int)(g() % 1000) < permille) {
    std::vector<int> kinds = {-1, A};
    if (!occupied.empty()) kinds.push_back(occupied[g() % occupied.size()]);
    if (A > Env::kCells && !mask[A - 1]) kinds.push_back(A - 1);  // Hex swap off turn 1, Othello pass
    return kinds[g() % kinds.size()];
  }
  if (legal.empty()) return 0;
  return legal[g() % legal.size()];
}

template <typename Env>
void Run(int argc, char** argv) {
  using S = typename Env::Spec;
  const std::string out = argv[3];
  const int n = std::stoi(argv[4]);
  const int steps = std::stoi(argv[5]);
  auto conf = S::kDefaultConfig;
  conf["num_envs"_] = n;
  conf["batch_size"_] = n;
  conf["num_threads"_] = 1;
  conf["max_num_players"_] = 2;
  conf["seed"_] = std::stoi(argv[6]);
  const bool replay = std::string(argv[1]) == "replay";
  std::mt19937 policy(replay ? 0u : (uint32_t)std::stoul(argv[7]));
  std::vector<int32_t> script;  // replay: actions[steps][n]
  if (replay) {
    script.resize((size_t)steps * n);
    std::ifstream in(argv[7], std::ios::binary);
    in.read(reinterpret_cast<char*>(script.data()), (std::streamsize)script.size() * 4);
    if (in.gcount() != (std::streamsize)script.size() * 4) {
      std::cerr << "short actions file " << argv[7] << "\n";
      std::exit(2);
    }
  }
  std::vector<int> permille(n, 0);
  for (int i = 8; i < argc; ++i) {
    std::string a(argv[i]);
    if (a.rfind("max_episode_steps=", 0) == 0) {
      conf["max_episode_steps"_] = std::stoi(a.substr(18));
    } else if (!replay) {
      permille[i - 8] = std::stoi(a);
    }
  }
  S spec(conf);
  ProbePool<Env> pool(spec);
  auto keys = S::StateSpec::AllKeys();
  std::vector<std::ofstream> files;
  for (auto& k : keys) files.emplace_back(out + "/" + k + ".bin", std::ios::binary);
  std::ofstream names(out + "/keys.txt");
  std::ofstream hid(out + "/hidden.bin", std::ios::binary);
  std::vector<int32_t> all(n);
  std::iota(all.begin(), all.end(), 0);
  std::vector<std::vector<char>> mask(n, std::vector<char>(Env::kActions, 1));
  int mask_key = -1;
  for (size_t i = 0; i < keys.size(); ++i) {
    if (keys[i] == "info:legal_action_mask") mask_key = (int)i;
  }
  auto dump = [&](const std::vector<Array>& ret) {
    // env id order: info:env_id is key 0; a per-player key has 2 rows per env
    const int* ids = static_cast<const int*>(ret[0].Data());
    std::vector<int> pos(n);
    for (int r = 0; r < n; ++r) pos[ids[r]] = r;
    for (size_t i = 0; i < ret.size(); ++i) {
      const size_t rows = ret[i].Shape(0);
      const size_t per = rows / n;  // 1, or 2 for a per-player key
      const size_t rb = ret[i].size / rows * ret[i].element_size;
      const char* base = static_cast<const char*>(ret[i].Data());
      for (int e = 0; e < n; ++e) files[i].write(base + (size_t)pos[e] * per * rb, per * rb);
      if (names.is_open()) names << keys[i] << " " << per << "\n";
    }
    names.close();
    const bool* m = static_cast<const bool*>(ret[mask_key].Data());
    for (int e = 0; e < n; ++e) {
      for (int a = 0; a < Env::kActions; ++a) mask[e][a] = m[(size_t)pos[e] * Env::kActions + a];
      std::vector<int32_t> w;
      pool.At(e).Hidden(&w);
      hid.write(reinterpret_cast<const char*>(w.data()), w.size() * 4);
    }
  };
  Array ids(::Spec<int>({n}));
  std::memcpy(ids.Data(), all.data(), 4 * n);
  pool.Reset(ids);
  dump(pool.Recv());
  std::ofstream used(out + "/actions.bin", std::ios::binary);
  for (int t = 0; t < steps; ++t) {
    std::vector<int32_t> a(n);
    for (int e = 0; e < n; ++e) {
      bool m[Env::kActions];
      for (int j = 0; j < Env::kActions; ++j) m[j] = mask[e][j] != 0;
      a[e] = replay ? script[(size_t)t * n + e] : Pick<Env>(policy, m, permille[e]);
    }
    std::vector<Array> raw({Array(::Spec<int>({n})), Array(::Spec<int>({n})), Array(::Spec<int>({n}))});
    std::memcpy(raw[0].Data(), all.data(), 4 * n);
    std::memcpy(raw[1].Data(), all.data(), 4 * n);
    std::memcpy(raw[2].Data(), a.data(), 4 * n);
    pool.Send(raw);
    dump(pool.Recv());
    used.write(reinterpret_cast<const char*>(a.data()), 4 * n);
  }
}

// env-steps/s of the reference's own pool: n envs, `threads` worker threads, sync batches of all envs; each action
// is the first legal one from a random start (picked on the calling thread, outside the timed Send / Recv)
template <typename Env>
void Bench(int n, int threads, int steps) {
  using S = typename Env::Spec;
  auto conf = S::kDefaultConfig;
  conf["num_envs"_] = n;
  conf["batch_size"_] = n;
  conf["num_threads"_] = threads;
  conf["max_num_players"_] = 2;
  S spec(conf);
  AsyncEnvPool<Env> pool(spec);
  std::vector<int32_t> all(n);
  std::iota(all.begin(), all.end(), 0);
  Array ids(::Spec<int>({n}));
  std::memcpy(ids.Data(), all.data(), 4 * n);
  pool.Reset(ids);
  auto ret = pool.Recv();
  std::mt19937 g(1);
  int mask_key = 11;
  double timed = 0;
  for (int t = 0; t < steps; ++t) {
    const int* rid = static_cast<const int*>(ret[0].Data());
    const bool* m = static_cast<const bool*>(ret[mask_key].Data());
    std::vector<int32_t> a(n, 0);
    for (int r = 0; r < n; ++r) {
      const int s0 = (int)(g() % Env::kActions);
      for (int j = 0; j < Env::kActions; ++j) {
        const int c = (s0 + j) % Env::kActions;
        if (m[(size_t)r * Env::kActions + c]) {
          a[rid[r]] = c;
          break;
        }
      }
    }
    std::vector<Array> raw({Array(::Spec<int>({n})), Array(::Spec<int>({n})), Array(::Spec<int>({n}))});
    std::memcpy(raw[0].Data(), all.data(), 4 * n);
    std::memcpy(raw[1].Data(), all.data(), 4 * n);
    std::memcpy(raw[2].Data(), a.data(), 4 * n);
    const auto t0 = std::chrono::steady_clock::now();
    pool.Send(raw);
    ret = pool.Recv();
    timed += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  std::cout << "{\"num_envs\": " << n << ", \"threads\": " << threads << ", \"env_steps_per_s\": "
            << (double)n * steps / timed << "}\n";
}

template <typename Env>
int Main(int argc, char** argv) {
  const std::string cmd = argv[1];
  if (cmd == "spec") {
    DumpSpec<Env>();
  } else if (cmd == "bench" && argc >= 6) {
    Bench<Env>(std::stoi(argv[3]), std::stoi(argv[4]), std::stoi(argv[5]));
  } else if ((cmd == "run" || cmd == "replay") && argc >= 8) {
    Run<Env>(argc, argv);
  } else {
    return 2;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: driver spec <game> | driver run <game> out_dir n steps seed policy_seed permille...\n";
    return 2;
  }
  const std::string g = argv[2];
  if (g == "TicTacToe") return Main<TicTacToeProbe>(argc, argv);
  if (g == "ConnectFour") return Main<ConnectFourProbe>(argc, argv);
  if (g == "Hex") return Main<HexProbe>(argc, argv);
  if (g == "Othello") return Main<OthelloProbe>(argc, argv);
  std::cerr << "unknown game " << g << "\n";
  return 2;
}
