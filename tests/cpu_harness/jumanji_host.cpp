// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/jumanji_env.hip.h, built with g++ by
// tests/test_jumanji_host.py and replayed against the reference fixtures (tests/golden/jumanji_*.npz).
// The generator is libstdc++'s own: std::mt19937 with uniform_int_distribution, generate_canonical and
// the pair draw of std::shuffle, the draws the kernel's device helpers restate.  Not linked by envpool_amd/.
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "../../envpool_amd/csrc/jumanji_env.hip.h"

using namespace epa::jm;

namespace {
struct HostGen {
  std::mt19937 g;
  int UniformInt(int a, int b) { return std::uniform_int_distribution<int>(a, b)(g); }
  double Canonical() { return std::generate_canonical<double, 53>(g); }
  void UniformPair(uint32_t b0, uint32_t b1, int* p0, int* p1) {
    const unsigned long x = std::uniform_int_distribution<unsigned long>{0, (unsigned long)b0 * b1 - 1}(g);
    *p0 = (int)(x / b1);
    *p1 = (int)(x % b1);
  }
};

struct Out {
  void* const* keys;
  const int* key_bytes;
  int n_keys;
  float* reward;
  uint8_t* done;
  uint8_t* trunc;
  int* elapsed;
  int* hidden;
};

template <int P>
int Replay(const Cfg& c, const int* init, int n, int steps, const int* seeds, const int* actions, int act_dim,
           int limit, const Out& out) {
  for (int e = 0; e < n; ++e) {
    HostGen rng{std::mt19937((uint32_t)seeds[e])};
    typename State<P>::T s{};
    bool is_done = true;
    int cur = 0;
    for (int t = 0; t <= steps; ++t) {
      const size_t row = (size_t)t * n + e;
      float r = 0.0f;
      if (t == 0 || is_done) {
        cur = 0;
        if (!ResetP<P>(rng, c, init, s, &is_done)) return 1 + (int)row;
      } else {
        ++cur;
        r = StepP<P>(rng, c, s, actions + ((size_t)(t - 1) * n + e) * act_dim, cur, &is_done);
      }
      void* o[8];
      for (int j = 0; j < out.n_keys; ++j) o[j] = static_cast<char*>(out.keys[j]) + row * out.key_bytes[j];
      ObsP<P>(c, s, cur, o);
      out.reward[row] = r;
      out.done[row] = is_done;
      out.trunc[row] = is_done && cur >= limit;
      out.elapsed[row] = cur;
      HiddenP<P>(c, s, cur, out.hidden + row * HiddenWords(P));
    }
  }
  return 0;
}
}  // namespace

extern "C" {

// Rolls n envs (seeds[e]) through `steps` steps of actions[t][e][act_dim] with the engine's auto-reset (a done
// env resets on its next step and ignores that action).  Per row (t = 0 is the initial reset): every env state
// key into keys[j] (key_bytes[j] per row), reward, done, trunc (done && elapsed >= limit), elapsed, and the
// hidden-state words of get_state.  cfg: the ints of epa::jm::Cfg; init: kInitWords ints.
// Returns 0, or 1 + the first row whose reset ran out of tries.
int jm_replay(const int* cfg, const int* init, int n, int steps, const int* seeds, const int* actions, int act_dim,
              int limit, void* const* keys, const int* key_bytes, int n_keys, float* reward, uint8_t* done,
              uint8_t* trunc, int* elapsed, int* hidden) {
  Cfg c{};
  std::memcpy(&c, cfg, sizeof(Cfg));
  const Out out{keys, key_bytes, n_keys, reward, done, trunc, elapsed, hidden};
  switch (c.puzzle) {
    case kGame2048: return Replay<kGame2048>(c, init, n, steps, seeds, actions, act_dim, limit, out);
    case kMinesweeper: return Replay<kMinesweeper>(c, init, n, steps, seeds, actions, act_dim, limit, out);
    case kSlidingTile: return Replay<kSlidingTile>(c, init, n, steps, seeds, actions, act_dim, limit, out);
    case kRubiksCube: return Replay<kRubiksCube>(c, init, n, steps, seeds, actions, act_dim, limit, out);
    case kSnake: return Replay<kSnake>(c, init, n, steps, seeds, actions, act_dim, limit, out);
    case kMaze: return Replay<kMaze>(c, init, n, steps, seeds, actions, act_dim, limit, out);
    default: return -1;
  }
}

int jm_cfg_words() { return (int)(sizeof(Cfg) / sizeof(int)); }

}  // extern "C"
