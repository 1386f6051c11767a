// Proportional prioritized replay on the device (ddq_replay_set_priority,
// include/ddq_hip.h): the kernels of the sum tree of kernels.h (PrioTree) -- its
// rebuild, the one-workgroup stratified draw, the commit of |TD| after the head,
// the host add's writer launch -- and their launchers.  A translation unit of
// its own: none of these kernels is launched while prioritization is off, and
// kept out of kernels.hip they leave that file's code object as it is without
// them.  prio.h has the tree's arithmetic and the writer rule.
#include "prio.h"

namespace ddq {

#define CHECK_LAUNCH(x)                                             \
  do {                                                              \
    hipError_t e_ = (x);                                            \
    if (e_ != hipSuccess) {                                         \
      if (!*g_launch_where) g_launch_where = "prio.hip:" DDQ_PRIO_STR(__LINE__); \
      return e_;                                                    \
    }                                                               \
  } while (0)
#define DDQ_PRIO_STR2(x) #x
#define DDQ_PRIO_STR(x) DDQ_PRIO_STR2(x)

// ---- rebuild: every filled, allowed slot <- pmax, the rest 0; sums bottom-up ----
__global__ __launch_bounds__(256) void prio_rebuild_leaves_kernel(PrioTree t,
                                                                  const ReplayMeta* meta) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= t.padded[0]) return;
  uint32_t v = 0;
  if (i < t.capacity) {
    const int L = (int)meta->lane_len, valid = (int)meta->valid, head = (int)meta->head;
    const int x = (int)(i % L);
    if (x < valid && !replay_forbidden(x, head, valid, L, meta->nstep)) v = t.st->pmax;
  }
  t.leaf[i] = v;
}

// level k >= 1 (sum[k - 1]): node j = the sum of nodes 64 j .. 64 j + 63 below
__global__ __launch_bounds__(256) void prio_rebuild_level_kernel(PrioTree t, int k) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= t.padded[k]) return;
  unsigned long long s = 0;
  if (j < t.padded[k - 1] / 64) {
    if (k == 1) {
      const uint32_t* c = t.leaf + j * 64;
      for (int e = 0; e < 64; ++e) s += c[e];
    } else {
      const unsigned long long* c = t.sum[k - 2] + j * 64;
      for (int e = 0; e < 64; ++e) s += c[e];
    }
  }
  t.sum[k - 1][j] = s;
}

__global__ void prio_rebuild_root_kernel(PrioTree t) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long* top = t.sum[t.nlev - 1];
  unsigned long long s = 0;
  for (int e = 0; e < 64; ++e) s += top[e];
  t.st->total = s;
}

hipError_t launch_prio_rebuild(const PrioTree& t, const ReplayMeta* meta, hipStream_t s) {
  if (!t.leaf || t.nlev < 1 || t.nlev > kPrioLevels) return hipErrorInvalidValue;
  ddq_launch(prio_rebuild_leaves_kernel, dim3((uint32_t)((t.padded[0] + 255) / 256)), dim3(256), 0,
             s, t, meta);
  CHECK_LAUNCH(hipGetLastError());
  for (int k = 1; k <= t.nlev; ++k) {
    ddq_launch(prio_rebuild_level_kernel, dim3((uint32_t)((t.padded[k] + 255) / 256)), dim3(256), 0,
               s, t, k);
    CHECK_LAUNCH(hipGetLastError());
  }
  ddq_launch(prio_rebuild_root_kernel, dim3(1), dim3(64), 0, s, t);
  CHECK_LAUNCH(hipGetLastError());
  return hipSuccess;
}

// the rebuild's sum passes alone, over leaves written by ddq_state_write
hipError_t launch_prio_resum(const PrioTree& t, hipStream_t s) {
  if (!t.leaf || t.nlev < 1 || t.nlev > kPrioLevels) return hipErrorInvalidValue;
  for (int k = 1; k <= t.nlev; ++k) {
    ddq_launch(prio_rebuild_level_kernel, dim3((uint32_t)((t.padded[k] + 255) / 256)), dim3(256), 0,
               s, t, k);
    CHECK_LAUNCH(hipGetLastError());
  }
  ddq_launch(prio_rebuild_root_kernel, dim3(1), dim3(64), 0, s, t);
  CHECK_LAUNCH(hipGetLastError());
  return hipSuccess;
}

// ---- the stratified draw: thread j < B descends for sample j ----
// One node's 64 children: the first child whose inclusive prefix exceeds u.
// The loads of a chunk are independent and issued together, so a level costs a
// few memory latencies for the whole workgroup, not one per sample.  A zero
// child is never chosen; a sum that disagrees with its children (never, the
// updates are exact) would fall through to the node's last child, and the
// caller clamps to the level's real node count so no load leaves the arrays.
// FRESH: the launch also commits, so the loads bypass L1 (prio.h); a launch that
// only draws reads with plain loads (L1 starts every launch empty).
template <class T, bool FRESH>
__device__ __forceinline__ int prio_pick(const T* child, unsigned long long& u, T& val) {
  unsigned long long acc = 0;
  int sel = -1;
  T selv = 0;
  for (int c0 = 0; c0 < 64; c0 += 16) {
    T v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if constexpr (!FRESH) v[e] = child[c0 + e];
      else if constexpr (sizeof(T) == 8) v[e] = prio_ld64(child + c0 + e);
      else v[e] = prio_ld32(child + c0 + e);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const bool hit = sel < 0 && acc + (unsigned long long)v[e] > u;
      if (hit) { sel = c0 + e; selv = v[e]; }
      if (sel < 0) acc += (unsigned long long)v[e];
    }
    if (sel >= 0) break;
  }
  if (sel < 0) { sel = 63; acc = u; }
  u -= acc;
  val = selv;
  return sel;
}

template <bool FRESH>
__device__ __forceinline__ void prio_draw(const PrioTree& t, int B, uint64_t seed, uint64_t ctr,
                                          int32_t* __restrict__ idx_out, float* __restrict__ isw_out,
                                          int32_t* log, int64_t log_cap) {
  __shared__ uint32_t s_qmin;
  const int j = threadIdx.x;
  if (j == 0) s_qmin = 0xFFFFFFFFu;
  __syncthreads();
  int64_t node = 0;
  uint32_t qv = 1;
  if (j < B) {
    const unsigned long long T = prio_ld64(&t.st->total);
    const unsigned long long lo = T * (unsigned long long)j / (unsigned long long)B;
    const unsigned long long hi = T * (unsigned long long)(j + 1) / (unsigned long long)B;
    const uint64_t r = splitmix64(seed ^ splitmix64(ctr * 0x100000001B3ull + (uint64_t)j * 0x9E37ull));
    unsigned long long u = lo + __umul64hi(r, hi - lo);
    for (int k = t.nlev; k >= 1; --k) {
      unsigned long long cv;
      const int c = prio_pick<unsigned long long, FRESH>(t.sum[k - 1] + node * 64, u, cv);
      node = node * 64 + c;
      const int64_t real = t.padded[k - 1] / 64;           // level k's nodes without padding
      if (node >= real) node = real - 1;
    }
    uint32_t lv;
    const int c = prio_pick<uint32_t, FRESH>(t.leaf + node * 64, u, lv);
    node = node * 64 + c;
    if (node >= t.capacity) node = t.capacity - 1;
    qv = lv ? lv : 1u;
    atomicMin(&s_qmin, qv);
  }
  __syncthreads();
  if (j < B) {
    const float beta = t.st->beta;
    idx_out[j] = (int32_t)node;
    isw_out[j] = powf((float)s_qmin / (float)qv, beta);
    log_draw(log, log_cap, ctr, B, j, (int32_t)node);
  }
}

// p = (|d| + eps)^alpha as a leaf: rint(p 2^16) clamped to [1, 2^24]
__device__ __forceinline__ uint32_t prio_leaf_of(float d, float eps, float alpha) {
  const float p = powf(fabsf(d) + eps, alpha);
  if (!isfinite(p)) return kPrioMax;
  const float v = rintf(p * 65536.0f);
  if (!(v >= 1.0f)) return 1u;
  if (v >= (float)kPrioMax) return kPrioMax;
  return (uint32_t)v;
}

// One workgroup of 256 threads (B <= 256).  COMMIT: leaves of idx[0..B) <- the
// leaf of q_sa - target, only where the leaf is nonzero (a slot a writer has
// since made forbidden is not resurrected); a slot that appears more than once
// takes its highest b; pmax <- max(pmax, committed values).  Then the draw
// counter: bump = 1 advances it first, bump = 2 after the draw; draw != 0: that
// counter's sample into oidx / oisw.  The commit's atomics are complete (fence +
// barrier) before any thread descends, and the descent after a commit reads past
// L1 (prio_pick); the instantiation without a commit descends with plain loads.
template <bool COMMIT>
__global__ __launch_bounds__(256) void prio_commit_draw_kernel(
    PrioTree t, int B, const int32_t* __restrict__ idx, const float* __restrict__ q_sa,
    const float* __restrict__ target, ReplayMeta* meta, int bump, int draw, uint64_t seed,
    int32_t* __restrict__ oidx, float* __restrict__ oisw, int32_t* log, int64_t log_cap) {
  __shared__ int32_t s_idx[256];
  const int b = threadIdx.x;
  if (COMMIT) {
    s_idx[b] = b < B ? idx[b] : -1;
    __syncthreads();
    if (b < B) {
      const int32_t i = s_idx[b];
      bool win = i >= 0 && (int64_t)i < t.capacity;
      for (int o = b + 1; o < B; ++o) win = win && s_idx[o] != i;
      if (win && prio_ld32(t.leaf + i) != 0u) {
        const uint32_t v = prio_leaf_of(q_sa[b] - target[b], t.st->eps, t.st->alpha);
        prio_leaf_set(t, i, v);
        atomicMax(&t.st->pmax, v);
      }
    }
    __threadfence();
  }
  uint64_t ctr = meta->counter;
  __syncthreads();                       // every thread has read the counter; the commit is done
  if (bump == 1) ctr += 1;               // 1: advance, then draw; 2: draw, then advance
  if (bump && b == 0) meta->counter = bump == 2 ? ctr + 1 : ctr;
  if (draw) prio_draw<COMMIT>(t, B, seed, ctr, oidx, oisw, log, log_cap);
}

hipError_t launch_prio_sample(const NetBuffers& nb, ReplayMeta* meta, uint64_t seed, hipStream_t s,
                              bool advance) {
  if (!nb.prio.leaf || !nb.mb.isw || nb.B > 256) return hipErrorInvalidValue;
  ddq_launch(prio_commit_draw_kernel<false>, dim3(1), dim3(256), 0, s, nb.prio, nb.B,
             (const int32_t*)nullptr, (const float*)nullptr, (const float*)nullptr, meta,
             advance ? 2 : 0, 1, seed,
             nb.mb.idx, nb.mb.isw, nb.idx_log, nb.log_cap);
  return hipGetLastError();
}

hipError_t launch_prio_commit_draw(const NetBuffers& nb, ReplayMeta* bump, const NetBuffers* next,
                                   uint64_t seed, hipStream_t s) {
  if (!nb.prio.leaf || nb.B > 256 || !bump || (next && !next->mb.isw)) return hipErrorInvalidValue;
  ddq_launch(prio_commit_draw_kernel<true>, dim3(1), dim3(256), 0, s, nb.prio, nb.B,
             (const int32_t*)nb.mb.idx, (const float*)nb.q_sa, (const float*)nb.target, bump,
             1, next ? 1 : 0, seed, next ? next->mb.idx : (int32_t*)nullptr,
             next ? next->mb.isw : (float*)nullptr, nb.idx_log, nb.log_cap);
  return hipGetLastError();
}

// the explicit commit (ddq_replay_update_priorities_async): no counter, no draw
hipError_t launch_prio_commit(const NetBuffers& nb, ReplayMeta* meta, hipStream_t s) {
  if (!nb.prio.leaf || nb.B > 256) return hipErrorInvalidValue;
  ddq_launch(prio_commit_draw_kernel<true>, dim3(1), dim3(256), 0, s, nb.prio, nb.B,
             (const int32_t*)nb.mb.idx, (const float*)nb.q_sa, (const float*)nb.target, meta, 0, 0,
             (uint64_t)0, (int32_t*)nullptr, (float*)nullptr, (int32_t*)nullptr, (int64_t)0);
  return hipGetLastError();
}

__global__ void prio_add_kernel(PrioTree t, const ReplayMeta* meta, int64_t lane, int64_t h) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int L = (int)meta->lane_len;
  if (h < 0 || h >= L || (lane + 1) * (int64_t)L > t.capacity) return;
  prio_on_add(t, lane * L, (int)h, L, (int)meta->head, (int)meta->valid, meta->nstep);
}

// after the add's head / valid reached ReplayMeta (stream order)
hipError_t launch_prio_add(const PrioTree& t, const ReplayMeta* meta, int64_t lane, int64_t h,
                           hipStream_t s) {
  ddq_launch(prio_add_kernel, dim3(1), dim3(64), 0, s, t, meta, lane, h);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void prio_set_kernel(PrioTree t, const int32_t* __restrict__ idx,
                                                       const uint32_t* __restrict__ q, int n) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int32_t i = idx[k];
  if (i < 0 || (int64_t)i >= t.capacity) return;
  prio_leaf_set(t, i, q[k]);
  atomicMax(&t.st->pmax, q[k]);
}

hipError_t launch_prio_set(const PrioTree& t, const int32_t* idx, const uint32_t* q, int n,
                           hipStream_t s) {
  if (n <= 0) return hipSuccess;
  ddq_launch(prio_set_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t, idx, q, n);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void fill_ones_kernel(float* dst, int n) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n) dst[k] = 1.0f;
}

hipError_t launch_fill_ones(float* dst, int n, hipStream_t s) {
  ddq_launch(fill_ones_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dst, n);
  return hipGetLastError();
}

}  // namespace ddq
