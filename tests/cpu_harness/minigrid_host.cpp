// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/minigrid_env.hip.h, built with g++ by
// tests/test_minigrid_host.py and replayed against the reference fixtures (tests/golden/minigrid_*.npz).
// The generator is libstdc++'s own: std::mt19937 with uniform_int_distribution, the draws the kernel's
// device helpers restate.  Not linked by envpool_amd/.
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "../../envpool_amd/csrc/minigrid_env.hip.h"

using namespace epa::mg;

namespace {
struct HostGen {
  std::mt19937 g;
  int UniformInt(int a, int b) { return std::uniform_int_distribution<int>(a, b)(g); }
  void UniformPair(uint32_t b0, uint32_t b1, int* p0, int* p1) {
    const unsigned long x = std::uniform_int_distribution<unsigned long>{0, (unsigned long)b0 * b1 - 1}(g);
    *p0 = (int)(x / b1);
    *p1 = (int)(x % b1);
  }
};
}  // namespace

extern "C" {

// Rolls n envs (seeds[e]) through `steps` steps of actions[t][e] with the engine's auto-reset (a done env
// resets on its next step and ignores that action).  Per row (t = 0 is the initial reset):
//   dir[t][e], image[t][e][147], pos[t][e][2], reward, done, trunc, elapsed (int8/float/int32)
//   grid[t][e][w*h*3] in DebugState order ((x * h + y) * 3)
// cfg: task width height size sx sy sdir num_crossings obstacle strip2_row n_obstacles max_steps max_tries see_through
// returns 0, or 1 + the first row whose reset ran out of tries
int mg_replay(const int* cfg, int n, int steps, const int* seeds, const int* actions, int* dir, uint8_t* image,
              int* pos, float* reward, uint8_t* done, uint8_t* trunc, int* elapsed, uint8_t* grid) {
  TaskCfg c{};
  std::memcpy(&c, cfg, sizeof(TaskCfg));
  const int cells = c.width * c.height;
  for (int e = 0; e < n; ++e) {
    HostGen rng{std::mt19937((uint32_t)seeds[e])};
    std::vector<uint16_t> cell(cells);
    GridRef g{cell.data(), c.width};
    EnvState s{};
    bool is_done = true;
    int cur = -1;
    for (int t = 0; t <= steps; ++t) {
      const size_t row = (size_t)t * n + e;
      float r = 0.0f;
      if (t == 0 || is_done) {
        if (!ResetEnv(rng, g, c, s)) return 1 + (int)row;
        cur = 0;
        is_done = false;
      } else {
        ++cur;
        bool term = false;
        r = StepEnv(rng, g, c, s, actions[(size_t)(t - 1) * n + e], cur, &term);
        is_done = term;
      }
      dir[row] = s.dir;
      GenImage(g, c, s, image + row * kImageBytes);
      pos[2 * row] = s.ax;
      pos[2 * row + 1] = s.ay;
      reward[row] = r;
      done[row] = is_done;
      trunc[row] = is_done && cur >= c.max_steps;
      elapsed[row] = cur;
      uint8_t* gr = grid + row * cells * 3;
      for (int x = 0; x < c.width; ++x) {
        for (int y = 0; y < c.height; ++y) {
          const uint16_t v = g.Get(x, y);
          uint8_t* o = gr + (x * c.height + y) * 3;
          o[0] = (uint8_t)TypeOf(v);
          o[1] = (uint8_t)ColorOf(v);
          o[2] = (uint8_t)StateOf(v);
        }
      }
    }
  }
  return 0;
}

}  // extern "C"
