// Munchausen / soft-Q target (ddq_set_munchausen): the per-image math both
// heads run in their Munchausen instantiation -- the general head
// (kernels.hip head_body) and the small-map chain's head phase (small_bwd.h).
// One thread an image; nothing crosses lanes.  Every *, /, +, - is rounded on
// its own (no FMA contraction), so both heads produce the same bits from the
// same P_out / Pc_out and the CPU twin differs only by expf / logf.
#pragma once
#include <hip/hip_runtime.h>

namespace ddq {

// The constants of the launch (NetBuffers::m_*), uniform over it.
struct MunchArgs {
  float alpha, tau, clip_lo;
  const float* pc;                  // Pc_out (B,4) = P(s,.); nullptr while alpha == 0
  float* bonus;                     // m_bonus (B)
};

// m = max_a v[a] and lse = logf(sum_a expf((v[a] - m) / tau)), a = 0..3 in
// order.  The largest term is expf(0) = 1, so the sum is in [1, 4] and lse in
// [0, ln 4]: no overflow whatever tau is; gaps past ~104 tau underflow to 0.
__device__ __forceinline__ float munch_lse4(const float (&v)[4], float tau, float& m) {
#pragma clang fp contract(off)
  m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
  float s = expf((v[0] - m) / tau);
  s = s + expf((v[1] - m) / tau);
  s = s + expf((v[2] - m) / tau);
  s = s + expf((v[3] - m) / tau);
  return logf(s);
}

// V' = m' + tau lse' over P(s',.): the soft (entropy-regularised) value.
__device__ __forceinline__ float munch_soft_value(const float (&pn)[4], float tau) {
#pragma clang fp contract(off)
  float m;
  const float lse = munch_lse4(pn, tau, m);
  const float t = tau * lse;
  return m + t;
}

// bonus = alpha min(max(tau ln pi(a_t | s), l0), 0) over P(s,.); pa: P(s, a_t)
__device__ __forceinline__ float munch_bonus(const float (&pc)[4], float pa, float alpha, float tau,
                                             float clip_lo) {
#pragma clang fp contract(off)
  float m;
  const float lse = munch_lse4(pc, tau, m);
  const float lp = (pa - m) / tau - lse;
  const float sc = tau * lp;
  return alpha * fminf(fmaxf(sc, clip_lo), 0.f);
}

// The whole target side of one image: ps <- V' nt (blob P_sa), the bonus
// stored when `store`, and the return value target = gamma ps + (r + bonus).
// alpha == 0: the bonus is 0 exactly and Pc_out is not read.
__device__ __forceinline__ float munch_target(const MunchArgs& M, const float (&pn)[4],
                                              const float* ac, int b, float gamma, float r,
                                              float nt, bool store, float& ps) {
#pragma clang fp contract(off)
  ps = munch_soft_value(pn, M.tau) * nt;
  float bonus = 0.f;
  if (M.alpha != 0.f) {
    const float4 pv = *reinterpret_cast<const float4*>(M.pc + b * 4);
    const float pc[4] = {pv.x, pv.y, pv.z, pv.w};
    // the taken action: the first non-zero entry of the one-hot
    const float pa = ac[0] != 0.f ? pc[0] : (ac[1] != 0.f ? pc[1] : (ac[2] != 0.f ? pc[2] : pc[3]));
    bonus = munch_bonus(pc, pa, M.alpha, M.tau, M.clip_lo);
  }
  if (store) M.bonus[b] = bonus;
  const float gp = gamma * ps;
  const float rb = r + bonus;
  return gp + rb;
}

}  // namespace ddq
