// Random-shift augmentation (DrQ / RAD) in the device replay gather:
// gather_shift_kernel<NS>, the gather of gather_kernel<NS> (u8 CHW ring slot ->
// f32 NHWC state / next_state, action one-hot, reward, non_terminal, the n-step
// window through replay_window, laned rings through ReplayMeta) with every
// frame replicate-padded by `pad` pixels and cropped back at a random offset:
//   out(b, z)[y][x][c] = S[slot(b, z)][c][clamp(y + dy, 0, S-1)][clamp(x + dx, 0, S-1)]
// z = 0 the state, z = 1 next_state, the shift (dy, dx)[b][z] the same for the
// slot's four channels and independent between s and s'.  Included by
// kernels.hip after gather_body (replay_window, f4, ddq_launch, splitmix64).
//
// The shift stream.  Draw `ctr` (the draw counter the index set was drawn
// under), sample position j in [0, B), side z, pad p:
//   r  = splitmix64((seed ^ kAugSalt) ^ splitmix64(ctr * 0x100000001B3 + (2 j + z) * 0x9E37))
//   dy = (int)(r mod (2 p + 1)) - p            (r as the unsigned 64-bit value)
//   dx = (int)((r >> 32) mod (2 p + 1)) - p
// kAugSalt = 0xD1B54A32D192ED03.  The index stream hashes under `seed` itself
// and is not touched: an augmented run draws the indices of the plain run.
//
// Work split.  A thread owns a run of 16 output pixels of one row; a row is
// R = ceil(S / 16) runs, a frame S * R of them.  One wave a workgroup, grid
// (ceil(S R / 64), B, 2): 256 workgroups at 64 x 64, B = 32 (one per CU) and 64
// at 16 x 16, where the whole gather is 1024 runs.  A workgroup lies inside one
// (b, z), so the hash, the two modulos and the slot (the n-step window's loads)
// are wave-uniform: computed once per workgroup, on the scalar unit.
//
// Data movement, per channel plane: the source bytes of the run are columns
// [a, a + 16), a = x0 + dx, of source row clamp(y + dy).  x0 is a multiple of 16,
// so the 32-byte window that starts at a16 = a & ~15 covers them at the
// wave-uniform byte offset o = dx & 15.  The window is loaded as two aligned
// 16-byte vectors when rows are 16-byte aligned (S % 16 == 0), else as four
// 8-byte pieces (rows are always 8-byte aligned: S % 8 == 0); a vector or piece
// that would leave the row is clamped to the row's last / first one, so every
// load stays inside the slot.  All 4 x 2 (or 4 x 4) vector loads and the 8 edge
// bytes are issued before the first convert.  The 16 bytes come out of the
// window's eight dwords by a uniform branch on the dword offset (o >> 2) and v_alignbyte_b32
// (o & 3); the columns that fall off the row (at most pad of them, on one side)
// take the row's first / last byte instead.  The four planes interleave into 16
// float4 NHWC stores, f4(c0, c1, c2, c3) as gather_body's.  No LDS.
#pragma once

namespace ddq {

constexpr uint64_t kAugSalt = 0xD1B54A32D192ED03ull;

struct AugShift {
  int dy, dx;
};
__device__ __forceinline__ AugShift aug_shift(uint64_t seed, uint64_t ctr, int j, int z, int pad) {
  const uint64_t r = splitmix64((seed ^ kAugSalt) ^
                                splitmix64(ctr * 0x100000001B3ull + (uint64_t)(2 * j + z) * 0x9E37ull));
  const uint32_t w = 2u * (uint32_t)pad + 1u;
  return AugShift{(int)(r % w) - pad, (int)((uint32_t)(r >> 32) % w) - pad};
}

// the four planes' 16 bytes: the window's dwords from dword Q on, funnelled by r bytes
// (Q a template argument: constant register indices, nothing indexed in scratch)
template <int Q>
__device__ __forceinline__ void aug_funnel(const uint32_t (&w)[4][8], int r, uint32_t (&d)[4][4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      d[c][k] = __builtin_amdgcn_alignbyte(w[c][Q + k + 1], w[c][Q + k], (uint32_t)r);
}

// grid (ceil(S * ceil(S / 16) / 64), B, 2), 64 threads; indices from idx (sample_kernel or
// the prioritized draw).  back: how far the draw counter moved on since that draw (the
// two-launch draw advances it itself, the prioritized one leaves it to the commit).
template <bool NS>
__global__ __launch_bounds__(64) void gather_shift_kernel(
    const uint8_t* __restrict__ st, const uint8_t* __restrict__ act,
    const int16_t* __restrict__ rew, const uint8_t* __restrict__ nt, ReplayMeta* meta,
    const int32_t* __restrict__ idx, int S, uint64_t seed, int pad, int back,
    float* __restrict__ sQ, float* __restrict__ sP, float* __restrict__ action,
    float* __restrict__ reward, float* __restrict__ nonterm, float* __restrict__ shift) {
  const int b = blockIdx.y, z = blockIdx.z, bx = blockIdx.x;
  const int64_t i = idx[b];
  // the slot and the scalars: gather_body's
  ReplayWindow W{1, 0.f, 0.f, 0u, 0u};
  int64_t nxt, slot;
  if (NS) {
    W = replay_window(rew, nt, meta, i, z == 1, z == 1 && bx == 0 && threadIdx.x == 0);
    nxt = W.s1;
    slot = z ? (int64_t)W.sm : i;
  } else {
    const int64_t L = meta->lane_len;
    nxt = (i + 1 == L) ? 0 : i + 1;
    if (meta->lanes > 1 && (uint32_t)(i + 1) % (uint32_t)L == 0) nxt = i + 1 - L;
    slot = z ? nxt : i;
  }
  const AugShift sh = aug_shift(seed, meta->counter - (uint64_t)back, b, z, pad);
  const int dy = sh.dy, dx = sh.dx;

  const int SS = S * S, R = (S + 15) >> 4;
  const int item = bx * 64 + threadIdx.x;
  if (item < S * R) {
    const int y = item / R, x0 = (item - y * R) << 4;
    const int ys = min(max(y + dy, 0), S - 1);
    const int a = x0 + dx;              // >= -pad
    const int a16 = a & ~15, o = a & 15;   // o == dx & 15: wave-uniform
    const uint8_t* row = st + slot * 4 * SS + ys * S;
    uint32_t w[4][8];
    uint32_t e0[4], e1[4];
    if ((S & 15) == 0) {
      const int nv = S >> 4;
      const int v0 = min(max(a16 >> 4, 0), nv - 1), v1 = min(max((a16 >> 4) + 1, 0), nv - 1);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint4 lo = *reinterpret_cast<const uint4*>(row + c * SS + v0 * 16);
        const uint4 hi = *reinterpret_cast<const uint4*>(row + c * SS + v1 * 16);
        w[c][0] = lo.x; w[c][1] = lo.y; w[c][2] = lo.z; w[c][3] = lo.w;
        w[c][4] = hi.x; w[c][5] = hi.y; w[c][6] = hi.z; w[c][7] = hi.w;
      }
    } else {
      const int np = S >> 3;
      int p[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) p[k] = min(max((a16 >> 3) + k, 0), np - 1);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint2 v = *reinterpret_cast<const uint2*>(row + c * SS + p[k] * 8);
          w[c][2 * k] = v.x; w[c][2 * k + 1] = v.y;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      e0[c] = row[c * SS];
      e1[c] = row[c * SS + S - 1];
    }
    // columns j < nl of the run lie left of the row, columns j >= jr right of it
    const int nl = -a, jr = S - a;
    uint32_t d[4][4];
    switch (o >> 2) {   // wave-uniform
      case 0: aug_funnel<0>(w, o & 3, d); break;
      case 1: aug_funnel<1>(w, o & 3, d); break;
      case 2: aug_funnel<2>(w, o & 3, d); break;
      default: aug_funnel<3>(w, o & 3, d); break;
    }
    float4* dst = reinterpret_cast<float4*>((z ? sP : sQ) + ((size_t)b * SS + y * S + x0) * 4);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      uint32_t px[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t v = (d[c][j >> 2] >> (8 * (j & 3))) & 0xFFu;
        px[c] = j < nl ? e0[c] : j >= jr ? e1[c] : v;
      }
      if (x0 + j < S) dst[j] = f4(px[0], px[1], px[2], px[3]);
    }
  }
  if (bx == 0 && threadIdx.x == 0) {
    shift[b * 4 + 2 * z] = (float)dy;
    shift[b * 4 + 2 * z + 1] = (float)dx;
  }
  if (z == 1 && bx == 0 && threadIdx.x < 4) {
    const int an = act[nxt];
    if (an >= kActions) meta->err = 1;
    action[b * 4 + threadIdx.x] = (threadIdx.x == an) ? 1.f : 0.f;
    if (threadIdx.x == 0) {
      reward[b] = NS ? W.R : (float)rew[nxt];
      nonterm[b] = NS ? W.w : (nt[nxt] ? 1.f : 0.f);
    }
  }
}

hipError_t launch_gather_shift(const NetBuffers& nb, const ReplayRing& r, uint64_t seed, int pad,
                               int back, hipStream_t s) {
  const Minibatch& m = nb.mb;
  if (pad < 1 || pad > kAugPadMax || 4 * pad > nb.S || !m.shift) return hipErrorInvalidValue;
  const int runs = nb.S * ((nb.S + 15) / 16);
  dim3 grid((runs + 63) / 64, nb.B, 2);
  auto kern = nb.nstep > 1 ? gather_shift_kernel<true> : gather_shift_kernel<false>;
  ddq_launch(kern, grid, dim3(64), 0, s, r.state, r.action, r.reward, r.nonterm, r.meta, m.idx, nb.S,
             seed, pad, back, m.state, m.next_state, m.action, m.reward, m.nonterm, m.shift);
  return hipGetLastError();
}

}  // namespace ddq
