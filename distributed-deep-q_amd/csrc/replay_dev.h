// Device helpers the replay kernels of kernels.hip and the prioritized-replay
// kernels of prio.hip share: the draw's hash, the n-step forbidden test, the
// index log.
#pragma once
#include "kernels.h"

namespace ddq {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// n-step returns (ddq_replay_set_nstep, include/ddq_hip.h): may a sample start
// at lane-local slot x of a lane with head h, v of L slots filled?  Not when
// one of its n window slots x+1..x+n is the write head's or a later, unwritten
// one: d = h - 1 - x in [0, n), d taken mod L on a full ring.  n = 1: x == h - 1.
// (slots fit 32 bits: capacity < 2^31)
__device__ __forceinline__ bool replay_forbidden(int x, int h, int v, int L, int n) {
  int d = h - 1 - x;
  if (d < 0 && n >= 2 && v == L) d += L;
  return (uint32_t)d < (uint32_t)n;
}

// Index log (ddq_index_log_enable): draw `ctr`'s sorted set, B entries.
__device__ __forceinline__ void log_draw(int32_t* log, int64_t cap, uint64_t ctr, int B, int t,
                                         int32_t v) {
  if (log && t < B) log[(int64_t)(ctr % (uint64_t)cap) * B + t] = v;
}

}  // namespace ddq
