// Parameter-space noise (ddq_set_param_noise, Plappert et al. 2017): the
// perturbed acting set -- theta~ = theta_Q + sigma eps as a flat fp32 vector in
// the ddq_param_layout order, and the three-plane split-bf16 forward copy wks~
// of its three convs in the layout of wks_local / put_conv_weight (kernels.hip)
// -- made by one launch, and the launch that measures the perturbed policy's
// distance and adapts sigma in device memory.  Implemented in param_noise.hip, a
// translation unit and so a code object of its own (as act_spread.hip).
//
// The noise (part of the ABI, include/ddq_hip.h has the same text).  Parameters
// 2j and 2j+1 of the flat order share the 64-bit word
//   w = splitmix64((seed ^ kPnSalt) ^ splitmix64(epoch * 0x100000001B3 + j * 0x9E37))
// and, every step in fp32 and rounded on its own (no FMA contraction):
//   u1 = ((w >> 40) + 1) * 2^-24          in (0, 1]
//   u2 = ((w >> 16) & 0xFFFFFF) * 2^-24   in [0, 1)
//   r  = sqrtf(-2 * logf(u1))             a = 6.2831855f * u2
//   eps_{2j} = r * cosf(a)                eps_{2j+1} = r * sinf(a)
//   theta~_i = theta_i + sigma * eps_i    (one multiply, one add)
// An odd last parameter takes the cosine branch of its own word.  The planes of
// wks~ are split3(theta~_i) exactly.  sigma is read from device memory (the
// adapt launch writes it there); epoch is the host's count of resamples.
#pragma once
#include "kernels.h"

namespace ddq {

constexpr uint64_t kPnSalt = 0x8EBC6AF09C88C6E3ull;

// One launch: theta~ and wks~ (plane stride nb.L.wks_total, as nb.wks[z]) from
// nb.theta[0].  The layout's total and every blob offset are multiples of 4
// for every frame side; hipErrorInvalidValue otherwise.
hipError_t launch_param_noise_draw(const NetBuffers& nb, float* theta_n, __bf16* wks_n,
                                   const float* sigma, uint64_t seed, uint64_t epoch,
                                   hipStream_t s);

// One workgroup: kl[b] = KL(softmax(q[b]) || softmax(qn[b])) over the 4 actions
// (munchausen.h's max-subtracted log-sum-exp at tau = 1, no contraction):
//   lp_a = (q_a - m) - lse     lq_a = (qn_a - mn) - lsen
//   kl   = sum_a expf(lp_a) * (lp_a - lq_a)          a = 0..3 in order
// then mean = (kl[0] + ... + kl[B-1]) / B summed in index order by one thread,
// and *sigma <- mean < delta ? *sigma * coef : *sigma / coef.
hipError_t launch_param_noise_adapt(const float* q, const float* qn, int B, float delta,
                                    float coef, float* kl, float* sigma, hipStream_t s);

}  // namespace ddq
