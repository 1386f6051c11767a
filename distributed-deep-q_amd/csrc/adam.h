// Adam with global-norm gradient clipping (ddq_set_adam, DDQ_RULE_ADAM).
// Included at the end of kernels.hip, as monitor.h is; launch_apply dispatches
// here (launch_adam_apply).
//
// Adam keeps two state words per parameter (m in nb.opt, v in nb.opt2), so it
// is not a case of apply_rule: that function is inlined into the fused slab-
// reduce / K2 / K4 launches, whose code must not change.  An Adam step runs the
// gradient launches and then this apply launch, as an exchanged step does.
//
// grad_norm_kernel (clipping only): kGnBlocks workgroups, block k sums the
// squares of a fixed contiguous range of the gradient buffer in double (the
// product of two fp32 values is exact there), thread by thread in a fixed
// order, then the 64 lanes and the 4 waves as monitor.h does, and writes one
// partial.  No atomics; the gradient buffer is not modified.
//
// adam_apply_kernel<NS>: the launch shape of apply_kernel<NS>.  Blocks
// [0, pf.ng) draw / gather the next step's minibatch; then one float4 of
// parameters per thread.  All four streams (g, theta, m, v) are loaded first;
// under those loads thread 0 of the block forms the step's scalars -- the bias
// corrections from the device iteration counter (written by the bookkeeping
// before this launch, by nothing during it, so a captured graph replays t) and
// the clip scale from the partials summed in index order -- and hands them to
// the block through LDS.  theta, m, v (and P on a sync step) leave through
// 16-byte write-through stores; conv weights also refresh their split layouts
// (refresh_elems: exactly what apply_elems does).
#pragma once
#include "kernels.h"

namespace ddq {

constexpr int kGnVec = 4;           // float4 loads in flight per thread

struct AdamArgs {
  float beta1, beta2, omb1, omb2, eps, clip;
  float* v;                         // second moment
  const int64_t* iter;              // t: updates applied, this one included
  const double* gpart;              // [kGnBlocks] (clip > 0)
  float* gnorm;                     // the pre-clip norm (clip > 0)
};

// (a template, as adam_apply_kernel is: the compiler emits templates after the
// plain kernels, so both land behind every other kernel of the code object)
template <int kGnThreads>
__global__ __launch_bounds__(kGnThreads) void grad_norm_kernel(const float* __restrict__ g,
                                                               int64_t n,
                                                               double* __restrict__ part) {
  __shared__ double s_d[kGnThreads / 64];
  const int t = threadIdx.x;
  // block k: float4 [k per, (k + 1) per) of the buffer (padded to a float4 by
  // its allocation; elements >= n do not count)
  const int64_t n4 = (n + 3) >> 2, per = (n4 + kGnBlocks - 1) / kGnBlocks;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = min(lo + per, n4);
  const float4* p = reinterpret_cast<const float4*>(g);
  double s = 0.0;
  for (int64_t i0 = lo + t; i0 < hi; i0 += (int64_t)kGnVec * kGnThreads) {
    float4 v[kGnVec];
#pragma unroll
    for (int k = 0; k < kGnVec; ++k) {
      const int64_t i = i0 + (int64_t)k * kGnThreads;
      v[k] = i < hi ? p[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < kGnVec; ++k) {
      const int64_t e = (i0 + (int64_t)k * kGnThreads) * 4;
      const float x[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double d = e + j < n ? (double)x[j] : 0.0;
        s += d * d;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if ((t & 63) == 0) s_d[t >> 6] = s;
  __syncthreads();
  if (t == 0) part[blockIdx.x] = ((s_d[0] + s_d[1]) + s_d[2]) + s_d[3];
}

template <bool NS>
__global__ __launch_bounds__(256) void adam_apply_kernel(ApplyTail t, ApplyArgs a, AdamArgs ad,
                                                         Prefetch pf) {
  if ((int)blockIdx.x < pf.ng) {
    prefetch_body<NS>(pf, blockIdx.x);
    return;
  }
  __shared__ float s_k[3];          // c1, c2, clip scale
  const int blk = (int)blockIdx.x - pf.ng;
  const bool first = t.opt_init[2] != 0;
  const bool sync = t.opt_init[3] != 0;
  const int64_t i = ((int64_t)blk * 256 + threadIdx.x) * 4;
  const bool live = i < a.n;
  float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f), t4 = g4, m4 = g4, v4 = g4;
  if (live) {
    g4 = *reinterpret_cast<const float4*>(t.grad + i);
    t4 = *reinterpret_cast<const float4*>(t.theta + i);
    if (!first) {                   // first apply after a reset: m = v = 0, not loaded
      m4 = *reinterpret_cast<const float4*>(t.opt + i);
      v4 = *reinterpret_cast<const float4*>(ad.v + i);
    }
  }
  // (soft sync: the old P, with the four streams)
  const float4 p4 = refresh_old_p(a, live && sync, i, t.thetaP);
  if (threadIdx.x == 0) {
    const double tt = (double)*ad.iter;
    s_k[0] = (float)(1.0 - pow((double)ad.beta1, tt));
    s_k[1] = (float)(1.0 - pow((double)ad.beta2, tt));
    float sc = 1.0f;
    if (ad.clip > 0.f) {
      double tot = 0.0;
      for (int k = 0; k < kGnBlocks; ++k) tot += ad.gpart[k];
      const float nrm = (float)sqrt(tot);
      sc = nrm > ad.clip ? ad.clip / nrm : 1.0f;
      if (blk == 0) *ad.gnorm = nrm;
    }
    s_k[2] = sc;
  }
  __syncthreads();
  if (!live) return;
  const float c1 = s_k[0], c2 = s_k[1], sc = s_k[2];
  const bool clip = ad.clip > 0.f;
  float th[4] = {t4.x, t4.y, t4.z, t4.w};
  float m[4] = {m4.x, m4.y, m4.z, m4.w};
  float v[4] = {v4.x, v4.y, v4.z, v4.w};
  const float g[4] = {g4.x, g4.y, g4.z, g4.w};
  {
    // every operation rounded on its own, as apply_rule
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = clip ? sc * g[e] : g[e];
      m[e] = ad.beta1 * m[e] + ad.omb1 * ge;
      v[e] = ad.beta2 * v[e] + ad.omb2 * (ge * ge);
      th[e] = th[e] - (a.lr * (m[e] / c1)) / (sqrtf(v[e] / c2) + ad.eps);
    }
  }
  // write-through (split.h wt_store4): no dirty theta / state lines for the
  // launch's end to write back
  const uint32_t nb = (uint32_t)(((a.n + 3) & ~3ll) * 4), ib = (uint32_t)(i * 4);
  wt_store4(wt_rsrc(t.theta, nb), ib, make_float4(th[0], th[1], th[2], th[3]));
  wt_store4(wt_rsrc(t.opt, nb), ib, make_float4(m[0], m[1], m[2], m[3]));
  wt_store4(wt_rsrc(ad.v, nb), ib, make_float4(v[0], v[1], v[2], v[3]));
  // the P copy on a sync step, and the conv layouts of Q (and of P then)
  refresh_elems(a, sync, i, th, p4, t.thetaP, t.wks, t.wksP, t.wks_plane);
}

hipError_t launch_grad_norm(const NetBuffers& nb, hipStream_t s) {
  if (!nb.gn_part) return hipErrorInvalidValue;
  ddq_launch(grad_norm_kernel<256>, dim3(kGnBlocks), dim3(256), 0, s, (const float*)nb.grad,
             (int64_t)nb.L.total, nb.gn_part);
  return hipGetLastError();
}

// launch_apply's Adam branch (after its bookkeeping launch, if any)
hipError_t launch_adam_apply(const NetBuffers& nb, const StepPlan& plan, const ApplyArgs& a,
                             const Prefetch& pf, hipStream_t s) {
  if (!nb.opt2 || !nb.gn_part || !nb.gnorm || plan.fused()) return hipErrorInvalidValue;
  AdamArgs ad;
  ad.beta1 = nb.adam_beta1; ad.beta2 = nb.adam_beta2;
  ad.omb1 = (float)(1.0 - (double)nb.adam_beta1);
  ad.omb2 = (float)(1.0 - (double)nb.adam_beta2);
  ad.eps = nb.adam_eps; ad.clip = nb.adam_clip;
  ad.v = nb.opt2; ad.iter = nb.iter; ad.gpart = nb.gn_part; ad.gnorm = nb.gnorm;
  const int blocks = (int)(((a.n + 3) / 4 + 255) / 256);
  auto kern = nb.nstep > 1 ? adam_apply_kernel<true> : adam_apply_kernel<false>;
  ddq_launch(kern, dim3(blocks + pf.ng), dim3(256), 0, s, apply_tail(nb), a, ad, pf);
  return hipGetLastError();
}

}  // namespace ddq
