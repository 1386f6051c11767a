// Proportional prioritized replay on the device (ddq_replay_set_priority,
// include/ddq_hip.h): the device helpers of the sum tree of kernels.h
// (PrioTree) -- the leaf update and the writer rule the ring's writers
// (ddq_replay_add, env.h's ring roles) apply.  The tree's own kernels (rebuild,
// draw, commit) are a translation unit of their own, prio.hip, so that the code
// object of kernels.hip keeps the layout it has without them.
//
// Everything is integer: leaves are uint32 fixed point, every sum is an exact
// uint64, an update is a leaf exchange plus a 64-bit integer atomic add of the
// (wrapping) delta on each ancestor and on the root.  The result therefore does
// not depend on the tree's shape or on the order of the atomics.  No float
// atomics.  Tree reads inside a launch that also updates the tree are
// agent-scope atomic loads (they bypass the CU's L1, which a same-launch atomic
// does not update).
#pragma once
#include "replay_dev.h"

namespace ddq {

__device__ __forceinline__ unsigned long long prio_ld64(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t prio_ld32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// leaf i <- v; the delta onto every ancestor and the root
__device__ __forceinline__ void prio_leaf_set(const PrioTree& t, int64_t i, uint32_t v) {
  const uint32_t old = atomicExch(t.leaf + i, v);
  if (old == v) return;
  const unsigned long long delta = (unsigned long long)v - (unsigned long long)old;   // wraps
  int64_t n = i;
#pragma unroll
  for (int k = 0; k < kPrioLevels; ++k) {
    if (k < t.nlev) {
      n >>= 6;
      atomicAdd(t.sum[k] + n, delta);
    }
  }
  atomicAdd(&t.st->total, delta);
}

// The writer rule.  One transition was added at lane-local slot h of the lane
// that starts at slot `base` (L slots, n-step length n); head2 / valid2 are the
// lane's head and valid AFTER the add.  The slot just written becomes forbidden
// (leaf 0) -- except at n = 1 when the head wrapped to 0, where
// replay_forbidden forbids nothing and the slot is drawable at once --, and
// slot h - n (mod L on a full ring), whose window no longer reaches the head,
// is released with the current pmax.
__device__ __forceinline__ void prio_on_add(const PrioTree& t, int64_t base, int h, int L,
                                            int head2, int valid2, int n) {
  const uint32_t pmax = prio_ld32(&t.st->pmax);
  prio_leaf_set(t, base + h, replay_forbidden(h, head2, valid2, L, n) ? 0u : pmax);
  int x = h - n;
  if (x < 0 && valid2 == L) x += L;
  if (x >= 0 && x != h && prio_ld32(t.leaf + base + x) == 0u) prio_leaf_set(t, base + x, pmax);
}

}  // namespace ddq
