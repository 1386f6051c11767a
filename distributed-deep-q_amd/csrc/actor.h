// Device-resident Snake actor (ddq_actor_*): one generate_experience
// (expgain.py:82-111) per launch pair -- launch_act's Q forward of the actor's
// own NHWC input, then actor_env_kernel: epsilon-greedy choice, one game step
// by the rules of gamesim/SnakeGame.py (as ddq/snake.py restates them),
// add_experience into the ring (replay.py:70-92) and the render of the next
// state, which is the next forward's input.  Included by kernels.hip (uses its
// splitmix64 and CHECK_LAUNCH).
//
// The game is 100 cells and a handful of branches: one thread plays it on a
// board in LDS (a few hundred LDS reads, no global traffic but the ring's three
// scalars), then the whole workgroup renders.  The render is the only part
// with any bytes to move (4 S^2 u8 + 16 S^2 f32: 80 KB at S = 64), written as
// uchar4 / float4 per thread like gather_body reads them; one workgroup keeps
// the launch a single dispatch with no inter-workgroup hand-off.
#pragma once
#include "kernels.h"

namespace ddq {

constexpr int kCells = 100;            // 10 x 10 board, cell index x * 10 + y
constexpr int kSide = 10;
constexpr int kEmptyCell = -1, kAppleCell = -2;   // SnakeGame.encode_state codes
constexpr int kActorThreads = 256;

__device__ __forceinline__ uint64_t actor_draw(uint64_t seed, uint64_t& k) {
  return splitmix64(seed ^ splitmix64(k++));
}

// gray_scale (SnakeGame.py:268-292): empty 0, apple 255, snake 200
__device__ __forceinline__ uint8_t actor_level(int v) {
  return v == kEmptyCell ? 0 : (v == kAppleCell ? 255 : 200);
}

// first maximum of a state's four Q values, as argmax_kernel
__device__ __forceinline__ int actor_first_max(const float* __restrict__ q) {
  int act = 0;
  for (int a = 1; a < kActions; ++a)
    if (q[a] > q[act]) act = a;
  return act;
}

// One SnakeGame.cpu_play by one thread: action act on board cur, the board
// after the move into nbd (untouched when the game is over).  Returns the
// reward: 1 apple eaten, 0 plain move, -1 game over (wall or body).  The new
// apple is draw k of the stream, k advanced.  Shared by the actor's and the
// evaluator's environment kernels: the rules exist once.
__device__ __forceinline__ int snake_move(const int8_t* cur, int8_t* nbd, int act, uint64_t seed,
                                          uint64_t& k) {
  int head = 0, neck = 0, len = 0;
  for (int c = 0; c < kCells; ++c) {
    const int v = cur[c];
    if (v == 0) head = c;
    if (v == 1) neck = c;
    len += v >= 0;
  }
  const int hx = head / kSide, hy = head % kSide;
  const int dx = hx - neck / kSide, dy = hy - neck % kSide;   // heading (set_state)
  // ["w","a","s","d"] = y+1, x-1, y-1, x+1
  int mx = (act == 3) - (act == 1), my = (act == 0) - (act == 2);
  if (mx == -dx && my == -dy) { mx = dx; my = dy; }   // a reversal keeps the heading
  const int nx = hx + mx, ny = hy + my, nc = nx * kSide + ny;
  if (nx < 0 || nx >= kSide || ny < 0 || ny >= kSide || cur[nc] >= 0) return -1;
  const bool eat = cur[nc] == kAppleCell;
  for (int c = 0; c < kCells; ++c) {
    int v = cur[c];
    if (v >= 0) v = (!eat && v == len - 1) ? kEmptyCell : v + 1;   // the tail moves on
    nbd[c] = (int8_t)v;
  }
  nbd[nc] = 0;
  if (eat) {   // the new apple: entry randrange(n) of the empty cells, x-major then y
    int n = 0;
    for (int c = 0; c < kCells; ++c) n += nbd[c] == kEmptyCell;
    if (n > 0) {
      int j = (int)__umul64hi(actor_draw(seed, k), (uint64_t)n);
      for (int c = 0; c < kCells; ++c)
        if (nbd[c] == kEmptyCell && j-- == 0) { nbd[c] = kAppleCell; break; }
    }
  }
  return eat ? 1 : 0;
}

// Pixels p..p+3 (one row, p % 4 == 0) of the four frames through the zoom maps,
// from the gray levels lv[4][kCells]
__device__ __forceinline__ void actor_pixels(const uint8_t* lv, const uint8_t* __restrict__ maps,
                                             int S, int p, uchar4 px[4]) {
  const int i = p / S, j = p - i * S;
  const int row = maps[i] * kSide;
  const uchar4 cm = *reinterpret_cast<const uchar4*>(maps + S + j);
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const uint8_t* l = lv + f * kCells + row;
    px[f] = make_uchar4(l[cm.x], l[cm.y], l[cm.z], l[cm.w]);
  }
}

// the same four pixels as f32 NHWC: 16 floats at in + 4 p
__device__ __forceinline__ void actor_store_nhwc(float* __restrict__ in, int p,
                                                 const uchar4 px[4]) {
  float4* dst = reinterpret_cast<float4*>(in + (size_t)p * 4);
  dst[0] = f4(px[0].x, px[1].x, px[2].x, px[3].x);
  dst[1] = f4(px[0].y, px[1].y, px[2].y, px[3].y);
  dst[2] = f4(px[0].z, px[1].z, px[2].z, px[3].z);
  dst[3] = f4(px[0].w, px[1].w, px[2].w, px[3].w);
}

// play = 0: render the current boards into actor_in only (ddq_actor_create).
// thresh = ceil(epsilon * 2^53): explore iff (r >> 11) < thresh, which is
// random() < epsilon for random() = (r >> 11) * 2^-53.
__global__ __launch_bounds__(kActorThreads) void actor_env_kernel(
    ActorState* __restrict__ as, const uint8_t* __restrict__ maps, const float* __restrict__ q,
    uint64_t thresh, int play, int S, uint8_t* __restrict__ r_state,
    uint8_t* __restrict__ r_action, int16_t* __restrict__ r_reward,
    uint8_t* __restrict__ r_nonterm, ReplayMeta* __restrict__ meta,
    float* __restrict__ actor_in, const PrioTree* __restrict__ prio) {
  __shared__ int8_t bd[5 * kCells];     // 4-frame history (oldest first), then init_board
  __shared__ int8_t nbd[kCells];        // the board after this move
  __shared__ uint8_t lv[4 * kCells];    // gray levels of the next state's four boards
  __shared__ int64_t s_slot;            // ring slot that receives the frames, -1: none
  __shared__ int s_over;
  const int t = threadIdx.x;
  for (int i = t; i < 5 * kCells; i += kActorThreads) bd[i] = as->boards[i];
  if (t == 0) { s_slot = -1; s_over = 0; }
  __syncthreads();

  if (play && t == 0) {
    const int8_t* cur = bd + 3 * kCells;
    // 1. greedy action: first maximum, as argmax_kernel
    int act = actor_first_max(q);
    // 2. coin, then the action when exploring
    const uint64_t seed = as->seed;
    uint64_t k = as->draws;
    if ((actor_draw(seed, k) >> 11) < thresh) act = (int)__umul64hi(actor_draw(seed, k), kActions);
    // 3. one move
    const int reward = snake_move(cur, nbd, act, seed, k);
    const bool over = reward < 0;
    // 4./5. the transition's scalars into slot head; head / valid; the stats
    const int64_t cap = meta->capacity, h = meta->head;
    if (h >= 0 && h < cap) {
      r_action[h] = (uint8_t)act;
      r_reward[h] = (int16_t)reward;
      r_nonterm[h] = over ? 0 : 1;
      if (!over) s_slot = h;             // a terminal step leaves the slot's frames stale
      meta->head = h + 1 == cap ? 0 : h + 1;
      const int64_t v = meta->valid;
      meta->valid = v < cap ? v + 1 : cap;
      // prioritized replay: the writer rule (prio.h) on the slot just written
      if (prio)
        prio_on_add(*prio, 0, (int)h, (int)cap, (int)(h + 1 == cap ? 0 : h + 1),
                    (int)(v < cap ? v + 1 : cap), meta->nstep);
    }
    s_over = over;
    as->draws = k;
    as->steps += 1;
    as->games += over;
    as->reward_sum += reward;
  }
  __syncthreads();

  // the next state's boards: the history shifted by one, or four init boards
  // after a game over (reset_game)
  if (play) {
    const bool over = s_over;
    for (int i = t; i < 4 * kCells; i += kActorThreads) {
      const int f = i / kCells, c = i - f * kCells;
      const int8_t v = over ? bd[4 * kCells + c] : (f < 3 ? bd[i + kCells] : nbd[c]);
      as->boards[i] = v;
      lv[i] = actor_level(v);
    }
  } else {
    for (int i = t; i < 4 * kCells; i += kActorThreads) lv[i] = actor_level(bd[i]);
  }
  __syncthreads();

  // render through the zoom maps, 4 pixels of one row per thread (S % 8 == 0):
  // u8 (C,H,W) into the ring slot, f32 NHWC into actor_in
  const int SS = S * S;
  uint8_t* slot = s_slot >= 0 ? r_state + (size_t)s_slot * 4 * SS : nullptr;
  for (int p4 = t; p4 * 4 < SS; p4 += kActorThreads) {
    const int p = p4 * 4;
    uchar4 px[4];
    actor_pixels(lv, maps, S, p, px);
    if (slot) {
#pragma unroll
      for (int f = 0; f < 4; ++f) *reinterpret_cast<uchar4*>(slot + (size_t)f * SS + p) = px[f];
    }
    actor_store_nhwc(actor_in, p, px);
  }
}

hipError_t launch_actor_env(const ActorEnv& e, const float* q, uint64_t thresh, int play,
                            hipStream_t s) {
  ddq_launch(actor_env_kernel, dim3(1), dim3(kActorThreads), 0, s, e.state, e.maps, q, thresh,
             play, e.S, e.r_state, e.r_action, e.r_reward, e.r_nonterm, e.meta, e.actor_in,
             e.prio);
  CHECK_LAUNCH(hipGetLastError());
  return hipSuccess;
}

}  // namespace ddq
