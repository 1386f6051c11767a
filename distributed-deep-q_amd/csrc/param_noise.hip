// Parameter-space noise kernels (param_noise.h), a translation unit and so a
// code object of their own: every other kernel's code object stays byte for
// byte what it was.
//
// param_noise_draw_kernel, one launch, 256 threads a workgroup.
//
// Work split.  The flat vector is cut at float4 granularity (every blob offset
// and the total are multiples of 4) into the three conv weight ranges and the
// rest -- the conv biases, fc4, Q_out -- which is 96 % of it at 64 x 64.
//  - Workgroups [0, kPnConvBlocks) own a block of output channels of one conv
//    layer: 4 of conv1's 32, 2 of conv2's 64, 2 of conv3's 64 (8 + 32 + 32).
//  - The rest are the stream: lane t of the grid owns quads t, t + T, ... (kPnQuads
//    of them for the sizing): a 16-byte load, two 64-bit words, four normals, a
//    16-byte store.  No LDS.
// The conv workgroups come first in the grid: they are the longer ones.
//
// A conv workgroup.  Phase 1 reads its channels' Caffe-order rows
// [co][ci][ky][kx] -- contiguous in theta -- as float4s, perturbs them in
// registers, stores theta~ in place order and the same float4 into LDS, rows
// at stride RS = the row length (ds_write_b128 of consecutive lanes).  Phase 2
// transposes out of LDS: a lane owns one 16-byte store per plane, 8 consecutive
// ci of one (co, tap) for conv2 / conv3, (2 kx) x (4 ci) of one (co, ky) for conv1
// (kx 7 zero), reads its 8 values with 8 ds_read_b32 at stride KK (the taps of
// a ci), splits them (split.h split_pack8) and stores the three planes.  One
// pass a wave: 4 passes a workgroup.
//
// LDS banks (64 banks of 4 bytes, a ds_read_b32 serves the 64 lanes at once;
// tools/lds_banks.py param_noise_reads checks these).  Per read the lanes'
// word addresses differ by
//   conv2  lane = (cq, tq, cg) = (l >> 5, (l >> 2) & 7, l & 3): RS cq + 200 cg + tq
//          with RS = 800 = 32 (mod 64), 200 = 8: 32 cq + 8 cg + tq, 64 distinct banks
//   conv3  lane = (tq, cg) = (l >> 3, l & 7): 72 cg + tq = 8 cg + tq (mod 64), 64
//          distinct banks, whatever RS is
//   conv1  lane = (ky, kxp) = (l >> 2, l & 3), l < 28: 7 ky + 2 kxp, distinct and < 49
// so no row padding is needed.  (Two conv1 channels a pass would need RS = s
// (mod 64) with {7 ky + 2 kxp} and its shift by s disjoint: no multiple of 4
// does it.)  The taps past the layer's last (25 = 3 x 8 + 1, 9 = 8 + 1) idle.
#include "param_noise.h"

#include "munchausen.h"
#include "replay_dev.h"
#include "split.h"

namespace ddq {

constexpr int kPnThreads = 256;
constexpr int kPnQuads = 2;                      // float4s a stream lane owns (grid sizing)
constexpr int kPnCB[3] = {4, 2, 2};              // output channels a conv workgroup owns
constexpr int kPnBlocks[3] = {32 / 4, 64 / 2, 64 / 2};
constexpr int kPnConvBlocks = kPnBlocks[0] + kPnBlocks[1] + kPnBlocks[2];
constexpr int kPnSmemFloats = 2 * 32 * 25;       // the largest block of rows (conv2)

struct PnArgs {
  const float* theta;
  float* out;
  __bf16* wks;
  const float* sigma;
  uint64_t key, ebase;               // seed ^ kPnSalt, epoch * 0x100000001B3
  int64_t wks_plane;
  uint32_t w_off[3], wks_off[3];     // conv weights: flat offset, offset in a wks plane
  uint32_t bq[3];                    // conv biases: first quad
  uint32_t q3;                       // first quad of fc4's weights (the tail runs to the end)
  uint32_t nstream;                  // quads of the stream
};

// the two normals of word j (param_noise.h)
__device__ __forceinline__ void pn_pair(uint64_t key, uint64_t ebase, uint32_t j, float& e0,
                                        float& e1) {
#pragma clang fp contract(off)
  const uint64_t w = splitmix64(key ^ splitmix64(ebase + (uint64_t)j * 0x9E37ull));
  const float u1 = (float)((uint32_t)(w >> 40) + 1u) * 0x1p-24f;
  const float u2 = (float)((uint32_t)(w >> 16) & 0xFFFFFFu) * 0x1p-24f;
  const float r = sqrtf(-2.f * logf(u1));
  const float a = 6.2831855f * u2;
  e0 = r * cosf(a);
  e1 = r * sinf(a);
}

// theta~ of quad q (flat parameters 4q .. 4q + 3: words 2q and 2q + 1)
__device__ __forceinline__ float4 pn_quad(const float4 x, float s, uint64_t key, uint64_t ebase,
                                          uint32_t q) {
#pragma clang fp contract(off)
  float e0, e1, e2, e3;
  pn_pair(key, ebase, 2 * q, e0, e1);
  pn_pair(key, ebase, 2 * q + 1, e2, e3);
  const float d0 = s * e0, d1 = s * e1, d2 = s * e2, d3 = s * e3;
  return f4(x.x + d0, x.y + d1, x.z + d2, x.w + d3);
}

__device__ __forceinline__ void pn_store_planes(const PnArgs& a, int64_t o, const float4& lo,
                                                const float4& hi) {
  u32x4 v[3];
  split_pack8(lo, hi, v);
#pragma unroll
  for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x4*>(a.wks + p * a.wks_plane + o) = v[p];
}

// Conv layer L's workgroup blk: channels [co0, co0 + CB)
template <int L, int CIN, int KS, int CB>
__device__ __forceinline__ void pn_conv_block(const PnArgs& a, int blk, float s, float* smem) {
  constexpr int KK = KS * KS, ROW = CIN * KK, RS = ROW, NQ = CB * ROW / 4;
  static_assert(ROW % 4 == 0 && CB * RS <= kPnSmemFloats, "rows are whole float4s and fit");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int co0 = blk * CB;
  const uint32_t qbase = (a.w_off[L] + (uint32_t)co0 * ROW) / 4;
  const float4* src4 = reinterpret_cast<const float4*>(a.theta);
  float4* dst4 = reinterpret_cast<float4*>(a.out);
  for (int i = t; i < NQ; i += kPnThreads) {
    const float4 y = pn_quad(src4[qbase + i], s, a.key, a.ebase, qbase + i);
    dst4[qbase + i] = y;
    *reinterpret_cast<float4*>(smem + 4 * i) = y;   // RS == ROW: the rows stay contiguous
  }
  __syncthreads();
  if constexpr (KS == 7) {
    // pass = channel: lane (ky, kxp) stores kx 2 kxp, 2 kxp + 1 of the 4 ci
    const int kxp = lane & 3, ky = lane >> 2;
    for (int col = wave; col < CB; col += kPnThreads / 64) {
      if (ky >= 7) continue;
      const float* p = smem + col * RS + ky * 7 + 2 * kxp;
      const float4 lo = f4(p[0], p[KK], p[2 * KK], p[3 * KK]);
      const float4 hi = kxp == 3 ? f4zero() : f4(p[1], p[KK + 1], p[2 * KK + 1], p[3 * KK + 1]);
      pn_store_planes(a, (int64_t)a.wks_off[L] + (((co0 + col) * 7 + ky) * 8 + 2 * kxp) * 4, lo, hi);
    }
  } else {
    constexpr int G = CIN / 8, CQ = 64 / (8 * G), TP = (KK + 7) / 8, NP = TP * (CB / CQ);
    static_assert(CQ >= 1 && CB % CQ == 0, "a pass covers whole channels");
    const int cg = lane % G, tq = (lane / G) % 8, cq = lane / (8 * G);
    for (int ps = wave; ps < NP; ps += kPnThreads / 64) {
      const int col = (ps / TP) * CQ + cq, tap = (ps % TP) * 8 + tq;
      if (tap >= KK) continue;
      const float* p = smem + col * RS + cg * 8 * KK + tap;
      const float4 lo = f4(p[0], p[KK], p[2 * KK], p[3 * KK]);
      const float4 hi = f4(p[4 * KK], p[5 * KK], p[6 * KK], p[7 * KK]);
      pn_store_planes(a, (int64_t)a.wks_off[L] + ((co0 + col) * KK + tap) * CIN + cg * 8, lo, hi);
    }
  }
}

__global__ __launch_bounds__(kPnThreads) void param_noise_draw_kernel(const PnArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[kPnSmemFloats];
  const float s = *a.sigma;
  int b = blockIdx.x;
  if (b < kPnBlocks[0]) return pn_conv_block<0, 4, 7, kPnCB[0]>(a, b, s, smem);
  b -= kPnBlocks[0];
  if (b < kPnBlocks[1]) return pn_conv_block<1, 32, 5, kPnCB[1]>(a, b, s, smem);
  b -= kPnBlocks[1];
  if (b < kPnBlocks[2]) return pn_conv_block<2, 64, 3, kPnCB[2]>(a, b, s, smem);
  b -= kPnBlocks[2];
  // the stream: quads [0, 8) / [8, 24) / [24, 40) are the conv biases, the rest
  // runs from fc4's weights to the end
  const float4* src4 = reinterpret_cast<const float4*>(a.theta);
  float4* dst4 = reinterpret_cast<float4*>(a.out);
  const uint32_t T = (gridDim.x - kPnConvBlocks) * kPnThreads;
  for (uint32_t k = b * kPnThreads + threadIdx.x; k < a.nstream; k += T) {
    const uint32_t q = k < 8 ? a.bq[0] + k : k < 24 ? a.bq[1] + (k - 8)
                     : k < 40 ? a.bq[2] + (k - 24) : a.q3 + (k - 40);
    dst4[q] = pn_quad(src4[q], s, a.key, a.ebase, q);
  }
}

hipError_t launch_param_noise_draw(const NetBuffers& nb, float* theta_n, __bf16* wks_n,
                                   const float* sigma, uint64_t seed, uint64_t epoch,
                                   hipStream_t s) {
  const ParamLayout& L = nb.L;
  PnArgs a{};
  a.theta = nb.theta[0]; a.out = theta_n; a.wks = wks_n; a.sigma = sigma;
  a.key = seed ^ kPnSalt;
  a.ebase = epoch * 0x100000001B3ull;
  a.wks_plane = L.wks_total;
  bool ok = L.total % 4 == 0 && L.w[3] % 4 == 0 && L.wks_total % 8 == 0 && L.total < (1ll << 31);
  for (int l = 0; l < 3; ++l) {
    ok = ok && L.w[l] % 4 == 0 && L.b[l] % 4 == 0 && L.wks_off[l] % 8 == 0;
    a.w_off[l] = (uint32_t)L.w[l];
    a.wks_off[l] = (uint32_t)L.wks_off[l];
    a.bq[l] = (uint32_t)(L.b[l] / 4);
  }
  ok = ok && L.bn[0] == 32 && L.bn[1] == 64 && L.bn[2] == 64;   // the stream's 8 + 16 + 16 quads
  // and its tail: conv3's bias is the last conv blob, everything after it streams
  ok = ok && L.b[2] + L.bn[2] == L.w[3] && L.w[3] <= L.total;
  if (!ok) return hipErrorInvalidValue;
  a.q3 = (uint32_t)(L.w[3] / 4);
  a.nstream = 40 + (uint32_t)((L.total - L.w[3]) / 4);
  const uint32_t per = kPnThreads * kPnQuads;
  const uint32_t nblk = (a.nstream + per - 1) / per;
  ddq_launch(param_noise_draw_kernel, dim3(kPnConvBlocks + nblk), dim3(kPnThreads), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// distance and adaptation (param_noise.h)
// ---------------------------------------------------------------------------
constexpr int kPnAdaptThreads = 256;
constexpr int kPnMaxB = 1024;        // ddq_create's largest batch

__device__ __forceinline__ float pn_kl4(const float (&q)[4], const float (&qn)[4]) {
#pragma clang fp contract(off)
  float m, mn;
  const float lse = munch_lse4(q, 1.f, m), lsen = munch_lse4(qn, 1.f, mn);
  float kl = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float lp = (q[a] - m) - lse, lq = (qn[a] - mn) - lsen;
    const float d = lp - lq;
    const float t = expf(lp) * d;
    kl = a == 0 ? t : kl + t;
  }
  return kl;
}

__global__ __launch_bounds__(kPnAdaptThreads) void param_noise_adapt_kernel(
    const float* __restrict__ q, const float* __restrict__ qn, int B, float delta, float coef,
    float* __restrict__ kl, float* sigma) {
#pragma clang fp contract(off)
  __shared__ float row[kPnMaxB];
  for (int b = threadIdx.x; b < B; b += kPnAdaptThreads) {
    const float4 x = reinterpret_cast<const float4*>(q)[b], y = reinterpret_cast<const float4*>(qn)[b];
    const float xv[4] = {x.x, x.y, x.z, x.w}, yv[4] = {y.x, y.y, y.z, y.w};
    const float v = pn_kl4(xv, yv);
    kl[b] = v;
    row[b] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = row[0];
    for (int b = 1; b < B; ++b) sum = sum + row[b];
    const float mean = sum / (float)B;
    const float sg = *sigma;
    *sigma = mean < delta ? sg * coef : sg / coef;
  }
}

hipError_t launch_param_noise_adapt(const float* q, const float* qn, int B, float delta,
                                    float coef, float* kl, float* sigma, hipStream_t s) {
  if (B < 1 || B > kPnMaxB) return hipErrorInvalidValue;
  ddq_launch(param_noise_adapt_kernel, dim3(1), dim3(kPnAdaptThreads), 0, s, q, qn, B, delta, coef,
             kl, sigma);
  return hipGetLastError();
}

}  // namespace ddq
