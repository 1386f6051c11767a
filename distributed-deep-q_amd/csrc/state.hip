// Checkpoint and resume on the device (ddq_state_*, include/ddq_hip.h): the
// section digest and the leaf validation of ddq_state_commit.  A translation
// unit of its own, as prio.hip: none of these kernels is launched by a ctx that
// never calls the state entry points, and kept out of kernels.hip they leave
// that file's code object as it is without them.
#include <algorithm>

#include "replay_dev.h"

namespace ddq {

#define CHECK_LAUNCH(x)                                             \
  do {                                                              \
    hipError_t e_ = (x);                                            \
    if (e_ != hipSuccess) {                                         \
      if (!*g_launch_where) g_launch_where = "state.hip:" DDQ_STATE_STR(__LINE__); \
      return e_;                                                    \
    }                                                               \
  } while (0)
#define DDQ_STATE_STR2(x) #x
#define DDQ_STATE_STR(x) DDQ_STATE_STR2(x)

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

// word k of the section contributes splitmix64(w_k ^ ((k + 1) * golden))
__device__ __forceinline__ uint64_t digest_term(uint64_t w, uint64_t k) {
  return splitmix64(w ^ ((k + 1) * kGolden));
}

// The sum of a workgroup's 64-bit accumulators: per wave by shuffles, then the
// four waves through LDS.  Valid in thread 0.
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t acc) {
  __shared__ uint64_t s_wave[kStateThreads / kWave];
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    const uint32_t lo = __shfl_down((uint32_t)acc, d, kWave);
    const uint32_t hi = __shfl_down((uint32_t)(acc >> 32), d, kWave);
    acc += ((uint64_t)hi << 32) | lo;
  }
  const int t = threadIdx.x;
  if ((t & (kWave - 1)) == 0) s_wave[t / kWave] = acc;
  __syncthreads();
  uint64_t s = 0;
  if (t == 0)
    for (int w = 0; w < kStateThreads / kWave; ++w) s += s_wave[w];
  return s;
}

// Grid-stride stream over the section's whole 16-byte chunks (two words each,
// one 16-byte load; p is an allocation's base, so 16-byte aligned), 64-bit
// indices throughout: a ring past 4 GiB is one launch.  No load reaches past
// byte 16 * floor(n / 16); thread 0 of workgroup 0 reads the last n % 16 bytes
// one by one into up to two zero-padded words and adds splitmix64(n).
// part[blockIdx.x] <- the workgroup's sum (wrapping, so any split gives the
// same total).
__global__ __launch_bounds__(kStateThreads) void state_digest_kernel(
    const uint8_t* __restrict__ p, uint64_t n, uint64_t* __restrict__ part) {
  const uint64_t chunks = n >> 4;
  const uint64_t stride = (uint64_t)gridDim.x * kStateThreads;
  const ulonglong2* __restrict__ v = reinterpret_cast<const ulonglong2*>(p);
  uint64_t acc = 0;
  uint64_t c = (uint64_t)blockIdx.x * kStateThreads + threadIdx.x;
  // four independent loads in flight per thread
  for (; c + 3 * stride < chunks; c += 4 * stride) {
    const ulonglong2 a0 = v[c], a1 = v[c + stride], a2 = v[c + 2 * stride], a3 = v[c + 3 * stride];
    acc += digest_term(a0.x, 2 * c) + digest_term(a0.y, 2 * c + 1);
    acc += digest_term(a1.x, 2 * (c + stride)) + digest_term(a1.y, 2 * (c + stride) + 1);
    acc += digest_term(a2.x, 2 * (c + 2 * stride)) + digest_term(a2.y, 2 * (c + 2 * stride) + 1);
    acc += digest_term(a3.x, 2 * (c + 3 * stride)) + digest_term(a3.y, 2 * (c + 3 * stride) + 1);
  }
  for (; c < chunks; c += stride) {
    const ulonglong2 a = v[c];
    acc += digest_term(a.x, 2 * c) + digest_term(a.y, 2 * c + 1);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t done = chunks << 4, rest = n - done;   // rest < 16
    uint64_t w[2] = {0, 0};
    for (uint64_t b = 0; b < rest; ++b) w[b >> 3] |= (uint64_t)p[done + b] << (8 * (b & 7));
    if (rest > 0) acc += digest_term(w[0], 2 * chunks);
    if (rest > 8) acc += digest_term(w[1], 2 * chunks + 1);
    acc += splitmix64(n);
  }
  const uint64_t s = block_sum_u64(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one workgroup: *out <- the sum of part[0 .. nparts)
__global__ __launch_bounds__(kStateThreads) void state_digest_sum_kernel(
    const uint64_t* __restrict__ part, int nparts, uint64_t* __restrict__ out) {
  uint64_t acc = 0;
  for (int i = threadIdx.x; i < nparts; i += kStateThreads) acc += part[i];
  const uint64_t s = block_sum_u64(acc);
  if (threadIdx.x == 0) *out = s;
}

hipError_t launch_state_digest(const void* p, uint64_t n, uint64_t* part, uint64_t* out,
                               hipStream_t s) {
  if (!p || !part || !out) return hipErrorInvalidValue;
  // 64 bytes (four chunks) per thread and pass; never more than kStateParts partials
  const uint64_t want = ((n >> 4) + 4 * kStateThreads - 1) / (4 * kStateThreads);
  const int blocks = (int)std::min<uint64_t>(std::max<uint64_t>(want, 1), kStateParts);
  ddq_launch(state_digest_kernel, dim3(blocks), dim3(kStateThreads), 0, s,
             reinterpret_cast<const uint8_t*>(p), n, part);
  CHECK_LAUNCH(hipGetLastError());
  ddq_launch(state_digest_sum_kernel, dim3(1), dim3(kStateThreads), 0, s,
             (const uint64_t*)part, blocks, out);
  CHECK_LAUNCH(hipGetLastError());
  return hipSuccess;
}

// ddq_state_commit's leaf check under the ring's restored (head, valid) and n:
// a leaf above 2^24, or one whose zero-ness disagrees with "slot unfilled or
// forbidden", is counted; bad[0] += count, bad[1] = the lowest such slot
// (bad[] = {0, INT32_MAX} before the launch).  Integer atomics on two words.
__global__ __launch_bounds__(kStateThreads) void state_check_leaves_kernel(
    const uint32_t* __restrict__ leaf, int64_t capacity, int L, int head, int valid, int nstep,
    int32_t* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * kStateThreads;
  int cnt = 0;
  int64_t first = INT32_MAX;
  for (int64_t i = (int64_t)blockIdx.x * kStateThreads + threadIdx.x; i < capacity; i += stride) {
    const uint32_t q = leaf[i];
    const int x = (int)(i % L);
    const bool zero = !(x < valid) || replay_forbidden(x, head, valid, L, nstep);
    if (q > kPrioMax || (q == 0) != zero) {
      ++cnt;
      if (i < first) first = i;
    }
  }
  if (cnt) {
    atomicAdd(&bad[0], cnt);
    atomicMin(&bad[1], (int32_t)first);
  }
}

hipError_t launch_state_check_leaves(const PrioTree& t, int64_t lane_len, int64_t head,
                                     int64_t valid, int nstep, int32_t* bad, hipStream_t s) {
  if (!t.leaf || !bad || lane_len < 1) return hipErrorInvalidValue;
  const int64_t want = (t.capacity + kStateThreads - 1) / kStateThreads;
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>(want, 1), kStateParts);
  ddq_launch(state_check_leaves_kernel, dim3(blocks), dim3(kStateThreads), 0, s,
             (const uint32_t*)t.leaf, t.capacity, (int)lane_len, (int)head, (int)valid, nstep, bad);
  CHECK_LAUNCH(hipGetLastError());
  return hipSuccess;
}

}  // namespace ddq
