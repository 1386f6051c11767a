// Spread acting forward (ddq_set_acting_path, DDQ_ACT_SPREAD): the three
// convolutions of launch_act for a handful of images.
//
// The training kernels (split.h) give a workgroup one image x one pixel tile
// x ALL output channels: 4 workgroups an image at 64 x 64, one round of the
// chip at B = 32 x two towers, 4 of 256 CUs at n = 1.  Here a workgroup is
// (image, small pixel tile, slice of 16 output channels):
//
//            tile     slices  workgroups / image at S = 64   waves (m x k)
//   conv1    8 x 8    2       128                            4 x 1
//   conv2    8 x 8    4        64                            4 x 2
//   conv3    4 x 4    4        64                            1 x 3
//
// so n = 1 already covers 64 CUs and the grid grows linearly with n.  A tile
// the map does not divide is a ragged edge tile: its outside pixels stage
// zeros (bounds-checked buffer loads) and its outside windows are not stored.
//
// Data movement.  The halo patch is staged once: fp32 NHWC through one buffer
// descriptor per image (H W C 4 bytes <= 2 MiB whatever n), split into three
// bf16 planes on the way to LDS (split_pack8; conv1's frames are integers,
// exact in bf16: one plane).  The weights come out of the forward's split
// copy `wks` ([co][tap][ci], planes wk_elems apart) -- no derived copy of
// their own -- one kernel ROW (KS taps: a contiguous run of KS * CIN bf16 per
// output channel; conv1: 8 x 4 with the zero tap) of the slice's 16 output
// channels per step through a two-slot LDS ring: 7 / 5 / 3 ring steps and
// barriers instead of the 25 / 9 taps of the training kernels, the next row's
// global loads in flight under the current row's MFMAs.
//
// Arithmetic: split.h's fp32-exact scheme unchanged, on
// v_mfma_f32_16x16x32_bf16 -- A = 16 pixels (four 2x2 pooling windows, window
// major: a lane's four accumulator rows are one window) x 32 channels, B = the
// slice's 16 output channels; six products (conv1 three) into a main and a
// correction accumulator, added once.  The k-steps of a kernel row (conv2: 5
// taps x 1, conv3: 3 taps x 2) are dealt round-robin to WK wave groups whose
// sums meet in LDS in the fixed order 0, 1, .. WK-1; group 0 finishes bias,
// ReLU and the max-pool in registers and stores 64-byte runs (NHWC) or pool3
// in Caffe order.  No atomics, no meetings between workgroups; an image's
// output depends on nothing but its own frame.
//
// LDS strides (tools/lds_banks.py's bank model of the four 16-lane groups of a
// ds_read_b128): pixel stride CIN + 16 bf16 and patch rows == 64 (mod 128)
// bf16 as split.h's MF = 1 reads; weight rows of the row's bf16 + 16 (conv1 24,
// conv2 88, conv3 104 dwords): A and B reads of all three layers take the
// minimum of 4 cycles in the model, conv1's two ds_read_b64 of a patch row of
// 32 dwords 2 each.
#pragma once
#include "split.h"

namespace ddq {

struct ActConvArgs {
  int n, H, W;               // images, conv grid (stride 1, same padding)
  int tiles_x, tiles;
  const float* in;           // fp32 NHWC (n, H, W, CIN)
  const __bf16* wk;          // the layer's split forward weights
  int64_t wk_elems;          // plane stride
  const float* bias;
  float* out;                // pooled fp32: NHWC (n, H/2, W/2, N) or, nchw, Caffe order
  int nchw;
};

template <int CIN, int KS, int N, int TY, int TX, int WM, int WK>
struct ActCfg {
  static constexpr bool C1 = CIN == 4;              // conv1: frames, one exact plane
  static constexpr int NS = 16;                     // output channels of a slice
  static constexpr int NSL = N / NS;
  static constexpr int PAD = KS / 2;
  static constexpr int PH = TY + KS - 1;
  static constexpr int PW = TX + KS - 1 + (C1 ? 2 : 0);   // conv1: the zero tap's pixels
  static constexpr int CS = C1 ? 4 : CIN + 16;      // bf16 per patch pixel
  static constexpr int RS0 = PW * CS;
  static constexpr int RS = RS0 + ((64 - (RS0 % 128)) + 128) % 128;   // == 64 (mod 128) bf16
  static constexpr int NPL = C1 ? 1 : 3;            // patch planes
  static constexpr int kPlane = PH * RS;
  static constexpr int RW = C1 ? 32 : KS * CIN;     // bf16 of one (co, ky) weight row
  static constexpr int RWP = RW + 16;
  static constexpr int NU = RW / 32;                // k-steps of a kernel row
  static constexpr int KPT = C1 ? 1 : CIN / 32;     // k-steps per tap
  static constexpr int MB = TY * TX / 16;           // 16-row blocks (4 windows each)
  static constexpr int TMB = MB / WM;
  static constexpr int kThreads = 64 * WM * WK;
  static constexpr int kSlot = 3 * NS * RWP;        // bf16 per ring slot
  static constexpr int kPatchB = NPL * kPlane * 2;
  static constexpr int kWB = 2 * kSlot * 2;
  static constexpr int kRedB = (WK - 1) * WM * TMB * 4 * 64 * 4;
  static constexpr int kSmemB = kPatchB + kWB + kRedB;
  static constexpr int NVW = 3 * NS * (RW / 8);     // 16-byte vectors per ring step
  static constexpr int kPer = (NVW + kThreads - 1) / kThreads;
  static_assert(N % NS == 0 && TY % 2 == 0 && TX % 2 == 0 && (TY * TX) % 16 == 0, "tile");
  static_assert(MB % WM == 0 && TMB >= 1, "m blocks per wave");
  static_assert(C1 || CIN % 32 == 0, "whole 32-channel k-steps");
  static_assert(kPatchB % 16 == 0 && RWP % 8 == 0 && CS % 4 == 0, "16-byte LDS vectors");
  static_assert(kThreads <= 1024 && kSmemB <= 160 * 1024, "workgroup");
};

// One fp32 add the compiler cannot pair with its neighbour into a packed fp32
// instruction (these kernels do without them): an operand and the sum pass through
// empty asm statements, the add itself stays the compiler's.
__device__ __forceinline__ float act_add(float x, float y) {
  asm volatile("" : "+v"(y));
  float r = x + y;
  asm volatile("" : "+v"(r));
  return r;
}

template <int CIN, int KS, int N, int TY, int TX, int WM, int WK>
__global__ __launch_bounds__(64 * WM * WK) void act_conv_kernel(const ActConvArgs a) {
  using C = ActCfg<CIN, KS, N, TY, TX, WM, WK>;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) char sm_act[];
  char* smem = sm_act;
  __bf16* patch = reinterpret_cast<__bf16*>(smem);
  __bf16* wbuf = reinterpret_cast<__bf16*>(smem + C::kPatchB);
  float* red = reinterpret_cast<float*>(smem + C::kPatchB + C::kWB);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.y;
  const int tile = blockIdx.x / C::NSL, co0 = (blockIdx.x % C::NSL) * C::NS;
  const int y0 = (tile / a.tiles_x) * TY, x0 = (tile % a.tiles_x) * TX;
  const int wkg = wid / WM, wmi = wid % WM;
  const int r16 = lane & 15, q4 = lane >> 4;
  const float bias = a.bias[co0 + r16];

  // ---- the kernel row ky of the slice's weights: global -> registers ----
  u32x4 wr[C::kPer];
  auto wload = [&](int ky) {
#pragma unroll
    for (int s = 0; s < C::kPer; ++s) {   // clamped, unconditional: the store drops extra lanes
      const int f0 = tid + s * C::kThreads;
      const int f = C::NVW % C::kThreads == 0 || f0 < C::NVW ? f0 : C::NVW - 1;
      const int p = f / (C::NS * (C::RW / 8)), r = f % (C::NS * (C::RW / 8));
      const int n = r / (C::RW / 8), c8 = r % (C::RW / 8);
      wr[s] = *reinterpret_cast<const u32x4*>(a.wk + p * a.wk_elems +
                                              ((size_t)(co0 + n) * KS + ky) * C::RW + 8 * c8);
    }
  };
  auto wstore = [&](int slot) {
#pragma unroll
    for (int s = 0; s < C::kPer; ++s) {
      const int f = tid + s * C::kThreads;
      if (C::NVW % C::kThreads != 0 && f >= C::NVW) continue;
      const int p = f / (C::NS * (C::RW / 8)), r = f % (C::NS * (C::RW / 8));
      const int n = r / (C::RW / 8), c8 = r % (C::RW / 8);
      *reinterpret_cast<u32x4*>(wbuf + slot * C::kSlot + (p * C::NS + n) * C::RWP + 8 * c8) = wr[s];
    }
  };
  wload(0);

  // ---- the halo patch: one descriptor over the image, zeros outside it ----
  constexpr uint32_t kOOB = 0x80000000u;
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.in + (size_t)b * a.H * a.W * CIN), (short)0, (int)(a.H * a.W * CIN * 4), 0x00020000);
  if constexpr (C::C1) {
    constexpr int NP = C::PH * C::PW;                        // items: pixels of 4 channels
    constexpr int NIT = (NP + C::kThreads - 1) / C::kThreads;
    float4 v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int f = tid + it * C::kThreads;
      const int py = f / C::PW, px = f % C::PW;
      const int gy = y0 - C::PAD + py, gx = x0 - C::PAD + px;
      const bool ok = f < NP && px < TX + KS - 1 && (unsigned)gy < (unsigned)a.H &&
                      (unsigned)gx < (unsigned)a.W;
      v[it] = __builtin_bit_cast(
          float4, __builtin_amdgcn_raw_buffer_load_b128(rin, (int)(ok ? (uint32_t)((gy * a.W + gx) * 16) : kOOB), 0, 0));
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int f = tid + it * C::kThreads;
      if (f >= NP) continue;
      __bf16 q[4] = {(__bf16)v[it].x, (__bf16)v[it].y, (__bf16)v[it].z, (__bf16)v[it].w};
      *reinterpret_cast<uint2*>(patch + (f / C::PW) * C::RS + (f % C::PW) * 4) =
          *reinterpret_cast<uint2*>(q);
    }
  } else {
    constexpr int NV = C::PH * C::PW * (CIN / 8);            // items: 8 channels of a pixel
    constexpr int NIT = (NV + C::kThreads - 1) / C::kThreads;
    float4 v[NIT][2];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int f = tid + it * C::kThreads;
      const int pix = f / (CIN / 8), c8 = f % (CIN / 8);
      const int py = pix / C::PW, px = pix % C::PW;
      const int gy = y0 - C::PAD + py, gx = x0 - C::PAD + px;
      const bool ok = f < NV && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
      const uint32_t o = (uint32_t)(((gy * a.W + gx) * CIN + 8 * c8) * 4);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
        v[it][hh] = __builtin_bit_cast(
            float4, __builtin_amdgcn_raw_buffer_load_b128(rin, (int)(ok ? o + 16 * hh : kOOB), 0, 0));
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int f = tid + it * C::kThreads;
      if (f >= NV) continue;
      const int pix = f / (CIN / 8), c8 = f % (CIN / 8);
      u32x4 s3[3];
      split_pack8(v[it][0], v[it][1], s3);
#pragma unroll
      for (int p = 0; p < 3; ++p)
        *reinterpret_cast<u32x4*>(patch + p * C::kPlane + (pix / C::PW) * C::RS +
                                  (pix % C::PW) * C::CS + 8 * c8) = s3[p];
    }
  }
  wstore(0);
  if (KS > 1) wload(1);
  __syncthreads();

  // ---- per-lane operand offsets: row r16 of 16-row block i, channels [8 q4, +8)
  // of a 32-channel k-step (conv1: taps 2 q4, 2 q4 + 1 of the row's eight) ----
  int abase[C::TMB];
#pragma unroll
  for (int i = 0; i < C::TMB; ++i) {
    const int m = 16 * (wmi * C::TMB + i) + r16;
    const int win = m >> 2, dy = (m >> 1) & 1, dx = m & 1;
    const int wy = win / (TX / 2), wx = win % (TX / 2);
    abase[i] = (2 * wy + dy) * C::RS + (2 * wx + dx) * C::CS + 8 * q4;
  }
  const int bbase = r16 * C::RWP + 8 * q4;
  f32x4 acc[C::TMB], cor[C::TMB];
#pragma unroll
  for (int i = 0; i < C::TMB; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) { acc[i][r] = 0.f; cor[i][r] = 0.f; }

#pragma unroll
  for (int ky = 0; ky < KS; ++ky) {
    const __bf16* wb = wbuf + (ky & 1) * C::kSlot;
#pragma unroll
    for (int u = 0; u < C::NU; ++u) {
      if ((ky * C::NU + u) % WK != wkg) continue;            // (wave-uniform)
      const int kx = u / C::KPT, g = u % C::KPT;
      bf16x8 bv[3];
#pragma unroll
      for (int p = 0; p < 3; ++p)
        bv[p] = *reinterpret_cast<const bf16x8*>(wb + p * C::NS * C::RWP + bbase + 32 * u);
#pragma unroll
      for (int i = 0; i < C::TMB; ++i) {
        const __bf16* pa = patch + abase[i] + ky * C::RS + kx * C::CS + 32 * g;
        if constexpr (C::C1) {
          // (8-byte aligned: two adjacent pixels of 4 channels)
          const u32x2 lo = *reinterpret_cast<const u32x2*>(pa);
          const u32x2 hi = *reinterpret_cast<const u32x2*>(pa + 4);
          const u32x4 a4 = {lo[0], lo[1], hi[0], hi[1]};
          const bf16x8 av = __builtin_bit_cast(bf16x8, a4);
          cor[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv[2], cor[i], 0, 0, 0);
          cor[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv[1], cor[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv[0], acc[i], 0, 0, 0);
        } else {
          bf16x8 av[3];
#pragma unroll
          for (int p = 0; p < 3; ++p) av[p] = *reinterpret_cast<const bf16x8*>(pa + p * C::kPlane);
          cor[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[2], bv[0], cor[i], 0, 0, 0);
          cor[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bv[1], cor[i], 0, 0, 0);
          cor[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bv[2], cor[i], 0, 0, 0);
          cor[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bv[0], cor[i], 0, 0, 0);
          cor[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bv[1], cor[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bv[0], acc[i], 0, 0, 0);
        }
      }
    }
    if (ky + 1 < KS) {
      // the next row into the other slot (its readers passed the barrier of
      // step ky - 1), then the loads of the row after it
      wstore((ky + 1) & 1);
      if (ky + 2 < KS) wload(ky + 2);
      __syncthreads();
    }
  }
#pragma unroll
  for (int i = 0; i < C::TMB; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[i][r] = act_add(acc[i][r], cor[i][r]);

  // ---- the k groups' sums, in the order 0, 1, .. WK - 1, by group 0 ----
  if constexpr (WK > 1) {
    if (wkg > 0) {
#pragma unroll
      for (int i = 0; i < C::TMB; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          red[((((wkg - 1) * WM + wmi) * C::TMB + i) * 4 + r) * 64 + lane] = acc[i][r];
    }
    __syncthreads();
    if (wkg > 0) return;
#pragma unroll
    for (int k = 1; k < WK; ++k)
#pragma unroll
      for (int i = 0; i < C::TMB; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[i][r] = act_add(acc[i][r], red[((((k - 1) * WM + wmi) * C::TMB + i) * 4 + r) * 64 + lane]);
  }

  // ---- bias, ReLU, 2x2 max-pool: a lane's four rows are window 4 mb + q4 of
  // output channel co0 + r16 ----
  const int Hp = a.H >> 1, Wp = a.W >> 1;
#pragma unroll
  for (int i = 0; i < C::TMB; ++i) {
    const int win = 4 * (wmi * C::TMB + i) + q4;
    const int py = y0 / 2 + win / (TX / 2), px = x0 / 2 + win % (TX / 2);
    if (py >= Hp || px >= Wp) continue;                      // ragged edge tile
    const float v0 = act_add(bias, acc[i][0]), v1 = act_add(bias, acc[i][1]);
    const float v2 = act_add(bias, acc[i][2]), v3 = act_add(bias, acc[i][3]);
    float mx = v0;
    if (v1 > mx) mx = v1;
    if (v2 > mx) mx = v2;
    if (v3 > mx) mx = v3;
    const float o = mx > 0.f ? mx : 0.f;
    const int n = co0 + r16;
    a.out[a.nchw ? (((size_t)b * N + n) * Hp + py) * Wp + px
                 : (((size_t)b * Hp + py) * Wp + px) * N + n] = o;
  }
}

template <int CIN, int KS, int N, int TY, int TX, int WM, int WK>
inline hipError_t launch_act_conv(ActConvArgs a, hipStream_t st) {
  using C = ActCfg<CIN, KS, N, TY, TX, WM, WK>;
  a.tiles_x = (a.W + TX - 1) / TX;
  a.tiles = a.tiles_x * ((a.H + TY - 1) / TY);
  auto kern = act_conv_kernel<CIN, KS, N, TY, TX, WM, WK>;
  static std::atomic<uint64_t> attr{0};
  if (hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(kern), attr, C::kSmemB)) return e;
  ddq_launch(kern, dim3(a.tiles * C::NSL, a.n), dim3(C::kThreads), C::kSmemB, st, a);
  return hipGetLastError();
}

// conv1 -> pool1f, conv2 -> pool2f, conv3 -> pool3 of n images, as
// launch_forward's three conv launches at nz = 1 wire them (kernels.hip
// launch_act; fc4 and the head follow there)
hipError_t launch_act_spread_convs(const NetBuffers& nb, int n, hipStream_t s, Marks M) {
  const ParamLayout& L = nb.L;
  const int S = nb.S;
  ActConvArgs a{};
  a.n = n;
  a.wk_elems = L.wks_total;
  a.H = a.W = S;
  a.in = nb.mb.state;
  a.wk = nb.wks[0] + L.wks_off[0];
  a.bias = nb.theta[0] + L.b[0];
  a.out = nb.pool1f[0];
  M("conv1_fwd");
  if (hipError_t e = launch_act_conv<4, 7, 32, 8, 8, 4, 1>(a, s)) return e;
  a.H = a.W = S / 2;
  a.in = nb.pool1f[0];
  a.wk = nb.wks[0] + L.wks_off[1];
  a.bias = nb.theta[0] + L.b[1];
  a.out = nb.pool2f[0];
  M("conv2_fwd");
  if (hipError_t e = launch_act_conv<32, 5, 64, 8, 8, 4, 2>(a, s)) return e;
  a.H = a.W = S / 4;
  a.in = nb.pool2f[0];
  a.wk = nb.wks[0] + L.wks_off[2];
  a.bias = nb.theta[0] + L.b[2];
  a.out = nb.pool3[0];
  a.nchw = 1;
  M("conv3_fwd");
  return launch_act_conv<64, 3, 64, 4, 4, 1, 3>(a, s);
}

}  // namespace ddq
