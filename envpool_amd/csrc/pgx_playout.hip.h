// PGX playouts: uniform-random play of one env to the end of its game, as __host__ __device__ code shared by the
// playout kernel (pgx.hip) and the g++ host harness of the tests (tests/cpu_harness/pgx_playout_host.cpp).
//
// The contract (DESIGN.md "PGX playouts"; all arithmetic mod 2^64):
//   SM(x)    x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
//            x = (x ^ (x >> 27)) * 0x94D049BB133111EB; return x ^ (x >> 31)                       (splitmix64)
//   stream   h = SM(seed ^ SM((uint64(env_id) << 32) | uint32(r)))      env_id: the GLOBAL id, r: the repeat
//   ply t    u = SM(h + t); n = popcount(s.m); j = ((u >> 32) * n) >> 32
//            action = index of the (j+1)-th lowest set bit of s.m; rewards += Step<G>(s, action)
// A pick depends on (seed, env_id, r, t) and the position only.  pgx::Step draws nothing from the env's generator, so
// a playout lives in the lane's registers: one State in, three results (and with commit the State) out.
#ifndef ENVPOOL_AMD_CSRC_PGX_PLAYOUT_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_PLAYOUT_HIP_H_

#include "pgx_env.hip.h"

namespace epa {
namespace pgx {

constexpr int kPlayoutMaxPlies = 256;     // the hard cap: no game of the four lasts longer than 122 plies
constexpr int kPlayoutMaxRepeats = 4096;

PGX_HD inline uint64_t PlayoutMix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

PGX_HD inline uint64_t PlayoutStream(uint64_t seed, int env_id, int r) {
  return PlayoutMix(seed ^ PlayoutMix(((uint64_t)(uint32_t)env_id << 32) | (uint32_t)r));
}

PGX_HD inline int Count32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return __builtin_popcount(x);
#endif
}

// index of the (j+1)-th lowest set bit of m, 0 <= j < Count(m): the 64-bit word by its popcount, then six halvings
// inside the word, every one a popcount of the lower half and two selects (no branch, no scan over the bits)
PGX_HD inline int SelectBit(u128 m, int j) {
  const uint64_t lo = (uint64_t)m, hi = (uint64_t)(m >> 64);
  const int clo = Count((u128)lo);
  const bool up = j >= clo;
  uint64_t w = up ? hi : lo;
  j -= up ? clo : 0;
  int base = up ? 64 : 0;
  uint32_t x = (uint32_t)w;
  {
    const int c = Count32(x);
    const bool u = j >= c;
    x = u ? (uint32_t)(w >> 32) : x;
    j -= u ? c : 0;
    base += u ? 32 : 0;
  }
  for (int half = 16; half >= 1; half >>= 1) {
    const int c = Count32(x & ((1u << half) - 1u));
    const bool u = j >= c;
    x = u ? x >> half : x;
    j -= u ? c : 0;
    base += u ? half : 0;
  }
  return base;
}

// max_plies as the caller gives it (0: the cap) -> plies a playout may play
PGX_HD inline int PlayoutLimit(int max_plies) { return max_plies == 0 ? kPlayoutMaxPlies : max_plies; }

struct PlayoutResult {
  float ret[2];    // per-player sum of the step rewards, in ply order (0 and +-1: exact)
  int32_t plies;
  int32_t status;  // 0 the game is over, 1 stopped at the limit
};

// Plays `s` on from its position with stream `h` until the game is over or `limit` plies are played.  `done`: the env
// is over already (an env before its first reset is): nothing is played.  `s` ends as the steps leave it.
template <int G>
PGX_HD PlayoutResult Playout(State& s, bool done, uint64_t h, int limit) {
  PlayoutResult out{{0.0f, 0.0f}, 0, 0};
  if (done) return out;
  int t = 0;
  while (t < limit) {
    const uint64_t u = PlayoutMix(h + (uint64_t)t);
    const uint64_t n = (uint64_t)Count(s.m);
    const int j = (int)(((u >> 32) * n) >> 32);
    const Rewards rw = Step<G>(s, SelectBit(s.m, j));
    out.ret[0] += rw.r[0];
    out.ret[1] += rw.r[1];
    ++t;
    if (s.done) break;
  }
  out.plies = t;
  out.status = s.done ? 0 : 1;
  return out;
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_PLAYOUT_HIP_H_
