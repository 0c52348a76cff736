// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_env.hip.h, built with g++ by
// tests/test_pgx_host.py and replayed against the reference fixtures (tests/golden/pgx_*.npz), and stepped once
// from given positions against the scalar restatement of the rules by tests/test_pgx_rules_host.py.  The generator
// is libstdc++'s std::mt19937, the one the reference's Env::gen_ is.  Not linked by envpool_amd/.
#include <cstdint>
#include <cstring>
#include <random>

#include "../../envpool_amd/csrc/pgx_env.hip.h"

using namespace epa::pgx;

namespace {
struct HostGen {
  std::mt19937 g;
  uint32_t Next() { return (uint32_t)g(); }
};

template <int G>
void Replay(int n, int steps, const int* seeds, const int* actions, int limit, void* const* keys, int32_t* hidden) {
  for (int e = 0; e < n; ++e) {
    HostGen rng{std::mt19937((uint32_t)seeds[e])};
    State s{};
    s.done = 1;
    int cur = 0;
    for (int t = 0; t <= steps; ++t) {
      const size_t row = (size_t)t * n + e;
      Rewards rw{{0.0f, 0.0f}};
      if (t == 0 || s.done) {  // the engine's auto-reset: a done env resets on its next step
        cur = 0;
        Reset<G>(rng, s);
      } else {
        ++cur;
        rw = Step<G>(s, actions[(size_t)(t - 1) * n + e]);
      }
      View v{};
      v.s = s;
      Finish(v, e, cur, rw, limit);
      for (int k = 0; k < kNumKeys; ++k) {
        const int re = RowElems<G>(k), eb = ElemBytes(k);
        char* dst = static_cast<char*>(keys[k]) + row * (size_t)(re * eb);
        for (int j = 0; j < re; ++j) {
          const uint32_t x = Elem<G>(v, k, j);
          if (eb == 1) {
            dst[j] = (char)x;
          } else {
            std::memcpy(dst + 4 * j, &x, 4);
          }
        }
      }
      Hidden<G>(s, hidden + row * HiddenWords<G>());
    }
  }
}
// set_state, one step, recv and get_state of n envs: SetHidden on a row's words, the kernel's step, every key through
// Elem and the new words through Hidden
template <int G>
int StepRows(int n, const int32_t* hidden, const int* elapsed, const int* done, const int* actions, int limit,
             void* const* keys, int32_t* hidden_out) {
  constexpr int W = HiddenWords<G>();
  for (int e = 0; e < n; ++e) {
    if (done[e]) return -3;
    State s{};
    if (!SetHidden<G>(s, hidden + (size_t)e * W)) return -2;
    const int cur = elapsed[e] + 1;
    const Rewards rw = Step<G>(s, actions[e]);
    View v{};
    v.s = s;
    Finish(v, e, cur, rw, limit);
    for (int k = 0; k < kNumKeys; ++k) {
      const int re = RowElems<G>(k), eb = ElemBytes(k);
      char* dst = static_cast<char*>(keys[k]) + (size_t)e * (size_t)(re * eb);
      for (int j = 0; j < re; ++j) {
        const uint32_t x = Elem<G>(v, k, j);
        if (eb == 1) {
          dst[j] = (char)x;
        } else {
          std::memcpy(dst + 4 * j, &x, 4);
        }
      }
    }
    Hidden<G>(s, hidden_out + (size_t)e * W);
  }
  return 0;
}
}  // namespace

extern "C" {

// One step from n rows of hidden words (hidden[e][HiddenWords], with elapsed[e] and done[e] as set_state takes
// them) with actions[e]: every state key of the step into keys[j] (n rows, info:env_id = e) and the hidden words
// after it.  The path of set_state, send, recv and get_state on the device.  -2: words that are no state; -3: a
// row that is over (its step would be a reset, which pgx_replay covers).
int pgx_step_rows(int game, int n, const int32_t* hidden, const int* elapsed, const int* done, const int* actions,
                  int limit, void* const* keys, int32_t* hidden_out) {
  switch (game) {
    case kTicTacToe: return StepRows<kTicTacToe>(n, hidden, elapsed, done, actions, limit, keys, hidden_out);
    case kConnectFour: return StepRows<kConnectFour>(n, hidden, elapsed, done, actions, limit, keys, hidden_out);
    case kHex: return StepRows<kHex>(n, hidden, elapsed, done, actions, limit, keys, hidden_out);
    case kOthello: return StepRows<kOthello>(n, hidden, elapsed, done, actions, limit, keys, hidden_out);
    default: return -1;
  }
}

// Rolls n envs (seeds[e]) through `steps` steps of actions[t][e] with the engine's auto-reset (a done env
// resets on its next step and ignores that action).  Per row (t = 0 is the initial reset, rows t * n + e):
// every state key into keys[j] in the order of epa::pgx::Key (per-player keys as [2, ...] per row), with
// info:env_id = e, and the hidden-state words of HiddenWords.  limit: max_episode_steps.
int pgx_replay(int game, int n, int steps, const int* seeds, const int* actions, int limit, void* const* keys,
               int32_t* hidden) {
  switch (game) {
    case kTicTacToe: Replay<kTicTacToe>(n, steps, seeds, actions, limit, keys, hidden); return 0;
    case kConnectFour: Replay<kConnectFour>(n, steps, seeds, actions, limit, keys, hidden); return 0;
    case kHex: Replay<kHex>(n, steps, seeds, actions, limit, keys, hidden); return 0;
    case kOthello: Replay<kOthello>(n, steps, seeds, actions, limit, keys, hidden); return 0;
    default: return -1;
  }
}

int pgx_hidden_words(int game) {
  switch (game) {
    case kTicTacToe: return HiddenWords<kTicTacToe>();
    case kConnectFour: return HiddenWords<kConnectFour>();
    case kHex: return HiddenWords<kHex>();
    case kOthello: return HiddenWords<kOthello>();
    default: return -1;
  }
}

}  // extern "C"
