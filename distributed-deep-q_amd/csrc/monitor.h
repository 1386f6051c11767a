// Device-resident training monitor (ddq_monitor_*): the quantities the
// reference's NetLogger.write appends after every step (netutils.py:72-96) --
// the loss, the RMS of every blob's gradient and of every blob's parameters --
// taken by ONE launch and appended to a device ring of MonitorRecord.  Included
// by kernels.hip after env.h.
//
// One workgroup per chunk of the host-built chunk table (at most kMonChunk
// floats of one blob of theta_Q, theta_P or the gradient buffer): every element
// is squared and summed in double (the product of two fp32 values is exact
// there), non-finite elements are counted, the 64 lanes and then the 4 waves
// are reduced in a fixed order and one (sum, count) partial is published per
// chunk (write-through).  Every workgroup then takes a ticket (an agent-scope
// fetch-add on one integer); the one that takes the last
// ticket sums each blob's partials in chunk order, forms the 30 RMS values,
// copies the loss, averages max_a Q_out over the images in image order and
// writes the record.  No float atomics, no meeting (nobody waits for anybody:
// no co-residency is needed) and no model state is written.
#pragma once
#include "kernels.h"

namespace ddq {

constexpr int kMonThreads = 256;
constexpr int kMonVec = 8;          // float4 loads per thread
constexpr int kMonBatch = 2048;     // partials the finisher stages in LDS at a time
static_assert(kMonChunk == kMonThreads * kMonVec * 4, "a chunk is one pass of the workgroup");
static_assert(kMonBatch >= 1024, "the finisher stages the B <= 1024 image maxima there too");

__device__ __forceinline__ void mon_acc(float x, double& s, int& nf) {
  const double d = (double)x;
  s += d * d;
  nf += (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1 : 0;
}

__global__ __launch_bounds__(kMonThreads) void monitor_kernel(MonitorEnv e, int32_t period,
                                                              int64_t tag) {
  __shared__ double s_d[kMonBatch];
  __shared__ int32_t s_i[kMonBatch];
  __shared__ int s_last;
  const int t = threadIdx.x;
  const int ci = blockIdx.x;
  if (ci >= e.nchunks) return;
  // a step's own launch: the iteration after its update decides (uniform over
  // the launch: nothing here writes it), before anything is loaded
  const int64_t it = *e.iter;
  if (period > 0 && it % period != 0) return;

  const MonitorChunk ch = e.chunks[ci];
  const float* base = (ch.tensor == 0 ? e.t[0] : ch.tensor == 1 ? e.t[1] : e.t[2]) + ch.off;
  double s = 0.0;
  int nf = 0;
  if ((reinterpret_cast<uintptr_t>(base) & 15) == 0 && (ch.count & 3) == 0) {
    // thread t's fixed slice: float4 t, t + 256, ... of the chunk
    const float4* p = reinterpret_cast<const float4*>(base);
    const int n4 = ch.count >> 2;
    float4 v[kMonVec];
#pragma unroll
    for (int k = 0; k < kMonVec; ++k) {
      const int i = t + k * kMonThreads;
      v[k] = i < n4 ? p[i] : f4zero();
    }
#pragma unroll
    for (int k = 0; k < kMonVec; ++k) {
      mon_acc(v[k].x, s, nf);
      mon_acc(v[k].y, s, nf);
      mon_acc(v[k].z, s, nf);
      mon_acc(v[k].w, s, nf);
    }
  } else {   // a layout whose blobs are no multiple of 4 floats (none today)
    for (int i = t; i < ch.count; i += kMonThreads) mon_acc(base[i], s, nf);
  }
  // 64 lanes, then 4 waves, in a fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_down(s, o);
    nf += __shfl_down(nf, o);
  }
  if ((t & 63) == 0) {
    s_d[t >> 6] = s;
    s_i[t >> 6] = nf;
  }
  __syncthreads();
  if (t == 0) {
    const double tot = ((s_d[0] + s_d[1]) + s_d[2]) + s_d[3];
    const int tn = ((s_i[0] + s_i[1]) + s_i[2]) + s_i[3];
    // publish the partial, then take a ticket.  The finisher may run on another
    // XCD, whose L2 is its own: the 12 bytes are stored write-through (agent-
    // scope stores) and drained before the ticket, and the finisher reads every
    // partial with agent-scope loads, which L1 never serves.  So the ticket is a
    // relaxed add.  (Measured against an acq_rel ticket behind an agent release
    // fence, which writes the XCD's whole L2 back in each of the ~800
    // workgroups right after a step dirtied it: DESIGN.md, Device-resident
    // monitor.)
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(e.psum + ci),
                       (unsigned long long)__double_as_longlong(tot), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(e.pnf + ci, tn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int old = __hip_atomic_fetch_add(e.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == e.nchunks - 1;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (no instruction: keeps the
    s_last = last;                                           //  loads below the ticket)
  }
  __syncthreads();
  if (!s_last) return;

  // ---- the last ticket: thread j < 30 sums blob j's partials in chunk order ----
  MonitorBlob mb{0, 0, 1};
  if (t < kMonBlobs) mb = e.blobs[t];
  double bs = 0.0;
  int bn = 0;
  for (int b0 = 0; b0 < e.nchunks; b0 += kMonBatch) {
    const int nb = min(kMonBatch, e.nchunks - b0);
    __syncthreads();
    for (int i = t; i < nb; i += kMonThreads) {
      s_d[i] = __longlong_as_double((long long)__hip_atomic_load(
          reinterpret_cast<unsigned long long*>(e.psum + b0 + i), __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_AGENT));
      s_i[i] = __hip_atomic_load(e.pnf + b0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const int lo = max(mb.first, b0), hi = min(mb.first + mb.n, b0 + nb);
    int i = lo;
    for (; i + 8 <= hi; i += 8) {   // eight LDS reads in flight, the adds in chunk order
      double v[8];
      int n[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[k] = s_d[i - b0 + k];
        n[k] = s_i[i - b0 + k];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        bs += v[k];
        bn += n[k];
      }
    }
    for (; i < hi; ++i) {
      bs += s_d[i - b0];
      bn += s_i[i - b0];
    }
  }
  __syncthreads();
  // max_a Q_out per image (NaN wins, as numpy's max) and the blobs' counts
  for (int b = t; b < e.B; b += kMonThreads) {
    const float* q = e.q_out + 4 * b;
    float m = q[0];
    for (int a = 1; a < kActions; ++a) {
      const float x = q[a];
      if (x > m || x != x) m = x;
    }
    s_d[b] = (double)m;
  }
  if (t < kMonBlobs) s_i[t] = bn;
  __syncthreads();
  const int64_t cnt = *e.count;
  MonitorRecord* r = e.ring + cnt % e.capacity;
  if (t < kMonBlobs) {
    const float rms = (float)sqrt(bs / (double)mb.count);
    if (t < 20) r->param_rms[t / 10][t % 10] = rms;
    else r->grad_rms[t - 20] = rms;
  }
  if (t == 64) {   // image order, in double
    double qs = 0.0;
    for (int b = 0; b < e.B; ++b) qs += s_d[b];
    r->q_max_mean = (float)(qs / (double)e.B);
  }
  if (t == 128) {
    r->iteration = it;
    r->tag = tag;
    r->loss = *e.loss;
    for (int k = 0; k < 3; ++k) {
      int n = 0;
      for (int j = 0; j < 10; ++j) n += s_i[10 * k + j];
      r->nonfinite[k] = n;
    }
    r->reserved = 0;
  }
  __syncthreads();   // every thread has read the count
  if (t == 0) {
    *e.count = cnt + 1;
    __hip_atomic_store(e.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

hipError_t launch_monitor(const MonitorEnv& e, int32_t period, int64_t tag, hipStream_t s) {
  ddq_launch(monitor_kernel, dim3(e.nchunks), dim3(kMonThreads), 0, s, e, period, tag);
  CHECK_LAUNCH(hipGetLastError());
  return hipSuccess;
}

}  // namespace ddq
