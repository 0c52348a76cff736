// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/pgx_arena.hip.h, the contract of the PGX arena,
// built with g++ by tests/test_pgx_arena_host.py: which net moves, the plan (the two kernels of PgxNetPlan walked as
// loops over blocks, ballots and lanes, with the header's ArenaPlace), the wave mapping and the tally of seven.  Not
// linked by envpool_amd/.
//
// With -DPGX_ARENA_MAIN the file is a program of its own: a few rows of everything, for a run under the host
// sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../envpool_amd/csrc/pgx_arena.hip.h"

using namespace epa::pgx;

extern "C" {

int ar_net_of(int env_id, int seat) { return ArenaNetOf(env_id, seat); }
int ar_waves(int rows) { return ArenaWaves(rows); }

// the kernels' plan: blocks of 4 ballots of 64 lanes; counts per block, then places from the counts in front, the
// ballots below and the lanes below.  Returns n0.
int ar_plan(int rows, const uint8_t* side, int32_t* order) {
  const int kChunk = 4, kLanes = 64, kBlock = kChunk * kLanes;
  const int blocks = (rows + kBlock - 1) / kBlock;
  std::vector<int> counts((size_t)blocks, 0);
  for (int b = 0; b < blocks; ++b) {
    for (int i = 0; i < kBlock; ++i) {
      const int row = b * kBlock + i;
      if (row < rows && side[row] == 0) ++counts[(size_t)b];
    }
  }
  int n0 = 0;
  for (int b = 0; b < blocks; ++b) n0 += counts[(size_t)b];
  int before = 0;
  for (int b = 0; b < blocks; ++b) {
    int below0 = before;
    for (int c = 0; c < kChunk; ++c) {
      uint64_t zero = 0;  // the ballot
      for (int lane = 0; lane < kLanes; ++lane) {
        const int row = b * kBlock + c * kLanes + lane;
        if (row < rows && side[row] == 0) zero |= (uint64_t)1 << lane;
      }
      for (int lane = 0; lane < kLanes; ++lane) {
        const int row = b * kBlock + c * kLanes + lane;
        if (row >= rows) continue;
        const uint64_t mine = (uint64_t)1 << lane;
        const int s = (zero & mine) != 0 ? 0 : 1;
        order[ArenaPlace(s, row, below0 + __builtin_popcountll(zero & (mine - 1)), n0)] = row;
      }
      below0 += __builtin_popcountll(zero);
    }
    before += counts[(size_t)b];
  }
  return n0;
}

// wave b of every b < ArenaWaves(rows): out[b] = {net, first, count}
void ar_wave_map(int rows, int n0, int32_t* out) {
  for (int b = 0; b < ArenaWaves(rows); ++b) {
    const ArenaWave w = ArenaWaveOf(b, rows, n0);
    out[3 * b] = w.net, out[3 * b + 1] = w.first, out[3 * b + 2] = w.count;
  }
}

void ar_tally(int k, int id0, const uint8_t* done, const float* reward, const int32_t* elapsed, int64_t* out) {
  for (int i = 0; i < k; ++i) {
    int c[kArenaCounters];
    ArenaTallyRow(done[i] != 0, reward[2 * (size_t)i], reward[2 * (size_t)i + 1], elapsed[i], id0 + i, c);
    for (int q = 0; q < kArenaCounters; ++q) out[q] += c[q];
  }
}

}  // extern "C"

#ifdef PGX_ARENA_MAIN
int main() {
  int bad = 0;
  for (int rows : {1, 63, 64, 65, 257, 1000}) {
    std::vector<uint8_t> side((size_t)rows);
    for (int i = 0; i < rows; ++i) side[(size_t)i] = (uint8_t)((i * 7 + i / 5) & 1);
    std::vector<int32_t> order((size_t)rows, -1), map((size_t)3 * ArenaWaves(rows));
    const int n0 = ar_plan(rows, side.data(), order.data());
    ar_wave_map(rows, n0, map.data());
    std::vector<int> seen((size_t)rows, 0);
    for (int b = 0; b < ArenaWaves(rows); ++b) {
      for (int j = 0; j < map[(size_t)3 * b + 2]; ++j) {
        const int row = order[(size_t)(map[(size_t)3 * b + 1] + j)];
        bad += side[(size_t)row] != map[(size_t)3 * b];
        ++seen[(size_t)row];
      }
    }
    for (int i = 0; i < rows; ++i) bad += seen[(size_t)i] != 1;
  }
  const int k = 4;
  const uint8_t done[k] = {1, 1, 1, 0};
  const float reward[2 * k] = {1, -1, 1, -1, 0, 0, 1, -1};
  const int32_t el[k] = {5, 6, 9, 3};
  int64_t out[kArenaCounters] = {0, 0, 0, 0, 0, 0, 0};
  ar_tally(k, 2, done, reward, el, out);  // ids 2, 3, 4, 5: seat 0 is net A's in env 2 and net B's in env 3
  std::printf("bad %d games %lld wins_a %lld wins_b %lld\n", bad, (long long)out[0], (long long)out[5],
              (long long)out[6]);
  return (bad == 0 && out[0] == 3 && out[5] == 1 && out[6] == 1 && out[3] == 1 && out[4] == 20) ? 0 : 1;
}
#endif
