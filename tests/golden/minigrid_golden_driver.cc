// Fixture driver for tests/golden/make_minigrid_golden.py (not product code, not built by build()).
//
// Links against the reference's own MiniGrid translation units compiled in place and drives its
// MiniGridEnvPool (AsyncEnvPool, sync mode) exactly like the Python binding does: Reset(all) -> Recv(),
// then Send(env_id, players.env_id, action) -> Recv() per step, auto-reset included.  After every step
// it also records MiniGridEnvPool::DebugStates (grid encoding, agent, carried object, obstacles).
//
//   driver spec  <key=value>...                          -> JSON config defaults + specs on stdout
//   driver run   <out_dir> <steps> <actions.bin> <key=value>...  -> raw arrays in out_dir
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "envpool/minigrid/minigrid.h"

using minigrid::MiniGridEnvPool;
using minigrid::MiniGridEnvSpec;

namespace {

template <typename T>
std::string Json(const T& v) {
  std::ostringstream s;
  if constexpr (std::is_same_v<T, std::string>) {
    s << '"' << v << '"';
  } else if constexpr (std::is_same_v<T, bool>) {
    s << (v ? "true" : "false");
  } else if constexpr (std::is_same_v<T, std::pair<int, int>>) {
    s << '[' << v.first << ", " << v.second << ']';
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
    << Json(std::get<0>(sp.bounds)) << ", " << Json(std::get<1>(sp.bounds)) << "]}";
  return s.str();
}

MiniGridEnvSpec::Config MakeConfig(int argc, char** argv, int first) {
  auto c = MiniGridEnvSpec::kDefaultConfig;
  for (int i = first; i < argc; ++i) {
    std::string a(argv[i]);
    auto eq = a.find('=');
    std::string k = a.substr(0, eq), v = a.substr(eq + 1);
    auto pair = [&]() {
      auto comma = v.find(',');
      return std::pair<int, int>(std::stoi(v.substr(0, comma)), std::stoi(v.substr(comma + 1)));
    };
    if (k == "num_envs") c["num_envs"_] = std::stoi(v);
    else if (k == "batch_size") c["batch_size"_] = std::stoi(v);
    else if (k == "seed") c["seed"_] = std::stoi(v);
    else if (k == "max_episode_steps") c["max_episode_steps"_] = std::stoi(v);
    else if (k == "env_name") c["env_name"_] = v;
    else if (k == "size") c["size"_] = std::stoi(v);
    else if (k == "width") c["width"_] = std::stoi(v);
    else if (k == "height") c["height"_] = std::stoi(v);
    else if (k == "agent_start_pos") c["agent_start_pos"_] = pair();
    else if (k == "agent_start_dir") c["agent_start_dir"_] = std::stoi(v);
    else if (k == "strip2_row") c["strip2_row"_] = std::stoi(v);
    else if (k == "num_crossings") c["num_crossings"_] = std::stoi(v);
    else if (k == "obstacle_type") c["obstacle_type"_] = v;
    else if (k == "n_obstacles") c["n_obstacles"_] = std::stoi(v);
    else if (k == "action_max") c["action_max"_] = std::stoi(v);
    else {
      std::cerr << "unknown key " << k << "\n";
      std::exit(2);
    }
  }
  return c;
}

void DumpSpec(int argc, char** argv) {
  auto conf = MakeConfig(argc, argv, 2);
  MiniGridEnvSpec spec(conf);
  std::cout << "{\"default_config\": [";
  {
    auto keys = MiniGridEnvSpec::Config::AllKeys();
    auto vals = MiniGridEnvSpec::kDefaultConfig.AllValues();
    size_t i = 0;
    std::apply([&](auto&&... v) { ((std::cout << (i ? ", " : "") << "[\"" << keys[i] << "\", " << Json(v) << "]", ++i), ...); },
               vals);
  }
  std::cout << "], \"state_spec\": [";
  {
    auto keys = MiniGridEnvSpec::StateSpec::AllKeys();
    size_t i = 0;
    std::apply([&](auto&&... s) { ((std::cout << (i ? ", " : "") << "[\"" << keys[i] << "\", " << SpecJson(s) << "]", ++i), ...); },
               spec.state_spec.AllValues());
  }
  std::cout << "], \"action_spec\": [";
  {
    auto keys = MiniGridEnvSpec::ActionSpec::AllKeys();
    size_t i = 0;
    std::apply([&](auto&&... s) { ((std::cout << (i ? ", " : "") << "[\"" << keys[i] << "\", " << SpecJson(s) << "]", ++i), ...); },
               spec.action_spec.AllValues());
  }
  std::cout << "]}\n";
}

void Run(int argc, char** argv) {
  std::string out = argv[2];
  int steps = std::stoi(argv[3]);
  auto conf = MakeConfig(argc, argv, 5);
  conf["num_threads"_] = 1;
  const int n = conf["num_envs"_];
  conf["batch_size"_] = n;
  std::vector<int32_t> acts((size_t)steps * n);
  {
    std::ifstream f(argv[4], std::ios::binary);
    f.read(reinterpret_cast<char*>(acts.data()), acts.size() * 4);
    if (!f) {
      std::cerr << "short actions file\n";
      std::exit(2);
    }
  }
  MiniGridEnvSpec spec(conf);
  MiniGridEnvPool pool(spec);
  auto keys = MiniGridEnvSpec::StateSpec::AllKeys();
  std::vector<std::ofstream> files;
  for (auto& k : keys) files.emplace_back(out + "/" + k + ".bin", std::ios::binary);
  std::ofstream names(out + "/keys.txt");
  for (auto& k : keys) names << k << "\n";
  std::ofstream dbg(out + "/debug.bin", std::ios::binary);
  std::vector<int> all(n);
  for (int i = 0; i < n; ++i) all[i] = i;
  auto dump = [&](const std::vector<Array>& ret) {
    for (size_t i = 0; i < ret.size(); ++i) {
      files[i].write(static_cast<const char*>(ret[i].Data()), ret[i].size * ret[i].element_size);
    }
    // per env (in env id order): width height ax ay dir carry(type color state) n_obst obst[16] grid[w*h*3]
    for (const auto& s : pool.DebugStates(all)) {
      int32_t head[26] = {s.width, s.height, s.agent_pos.first, s.agent_pos.second, s.agent_dir,
                          s.carrying_type, s.carrying_color, s.carrying_state,
                          (int32_t)s.obstacle_positions.size() / 2};
      for (int j = 0; j < 16; ++j) {
        head[9 + j] = j < (int)s.obstacle_positions.size() ? s.obstacle_positions[j] : -1;
      }
      head[25] = s.has_carrying;
      dbg.write(reinterpret_cast<const char*>(head), sizeof(head));
      dbg.write(reinterpret_cast<const char*>(s.grid.data()), s.grid.size());
    }
  };
  Array ids(::Spec<int>({n}));
  std::memcpy(ids.Data(), all.data(), 4 * n);
  pool.Reset(ids);
  dump(pool.Recv());
  for (int t = 0; t < steps; ++t) {
    std::vector<Array> raw({Array(::Spec<int>({n})), Array(::Spec<int>({n})), Array(::Spec<int>({n}))});
    std::memcpy(raw[0].Data(), all.data(), 4 * n);
    std::memcpy(raw[1].Data(), all.data(), 4 * n);
    std::memcpy(raw[2].Data(), acts.data() + (size_t)t * n, 4 * n);
    pool.Send(raw);
    dump(pool.Recv());
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "spec") {
    DumpSpec(argc, argv);
  } else if (argc >= 5 && std::string(argv[1]) == "run") {
    Run(argc, argv);
  } else {
    std::cerr << "usage: driver spec k=v... | driver run out_dir steps actions.bin k=v...\n";
    return 2;
  }
  return 0;
}
