// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_playout.hip.h, built with g++ by
// tests/test_pgx_playout_host.py.  Positions come in as the hidden words of pgx_env.hip.h (SetHidden) plus the done
// flag, and leave the same way.  Not linked by envpool_amd/.
#include <cstdint>

#include "../../envpool_amd/csrc/pgx_playout.hip.h"

using namespace epa::pgx;

namespace {
template <int G>
int Run(int n, const int32_t* hidden, const uint8_t* done, const int32_t* env_ids, int repeats, int max_plies,
        uint64_t seed, float* returns, int32_t* plies, uint8_t* status, int32_t* hidden_out, uint8_t* done_out) {
  constexpr int W = HiddenWords<G>();
  for (int i = 0; i < n; ++i) {
    for (int r = 0; r < repeats; ++r) {
      State s{};
      if (!SetHidden<G>(s, hidden + (size_t)i * W)) return -2;
      s.done = done[i] ? 1 : 0;
      const PlayoutResult res =
          Playout<G>(s, done[i] != 0, PlayoutStream(seed, env_ids[i], r), PlayoutLimit(max_plies));
      const size_t o = (size_t)i * repeats + r;
      returns[2 * o] = res.ret[0];
      returns[2 * o + 1] = res.ret[1];
      plies[o] = res.plies;
      status[o] = (uint8_t)res.status;
      Hidden<G>(s, hidden_out + o * W);
      done_out[o] = s.done ? 1 : 0;
    }
  }
  return 0;
}
}  // namespace

extern "C" {

// n positions (hidden[i]: HiddenWords words, done[i]) with global ids env_ids[i], `repeats` playouts each.  Entry
// i * repeats + r of every output: the returns [2], plies and status of the contract, and the position the playout
// ends in (what a commit writes back).  -1: no such game; -2: words that are no position.
int pgx_playout(int game, int n, const int32_t* hidden, const uint8_t* done, const int32_t* env_ids, int repeats,
                int max_plies, uint64_t seed, float* returns, int32_t* plies, uint8_t* status, int32_t* hidden_out,
                uint8_t* done_out) {
  switch (game) {
    case kTicTacToe:
      return Run<kTicTacToe>(n, hidden, done, env_ids, repeats, max_plies, seed, returns, plies, status, hidden_out,
                             done_out);
    case kConnectFour:
      return Run<kConnectFour>(n, hidden, done, env_ids, repeats, max_plies, seed, returns, plies, status, hidden_out,
                               done_out);
    case kHex:
      return Run<kHex>(n, hidden, done, env_ids, repeats, max_plies, seed, returns, plies, status, hidden_out,
                       done_out);
    case kOthello:
      return Run<kOthello>(n, hidden, done, env_ids, repeats, max_plies, seed, returns, plies, status, hidden_out,
                           done_out);
    default: return -1;
  }
}

// index of the (j+1)-th lowest set bit of the 128-bit set hi:lo
int pgx_select_bit(uint64_t lo, uint64_t hi, int j) { return SelectBit(((u128)hi << 64) | lo, j); }

uint64_t pgx_playout_mix(uint64_t x) { return PlayoutMix(x); }

}  // extern "C"
