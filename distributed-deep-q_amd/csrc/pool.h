// Device actor pool (ddq_actors_*): ngames Snake games in lock step feeding a
// laned replay ring (ReplayMeta), one lane per game.  One move is launch_act's Q
// forward of all the games' states at n = ngames, then pool_env_kernel, one
// workgroup per game: the actor's epsilon-greedy choice from the game's own row
// of Q (the coin is always drawn, as actor_env_kernel does), one move by
// snake_move (actor.h: the rules exist once), add_experience into the game's
// lane, and the render of the next state into the lane's slot and into the
// game's slice of the forward's input.  Included by kernels.hip after eval.h.
//
// A game's slot is lane base + (h0 + its own step counter) mod lane_len with
// the launch constants (h0, v0), the ring's per-lane head / valid when the pool
// was created; nothing in the launch reads meta->head / valid.  Workgroup 0
// alone publishes the new per-lane values (every game has made the same number
// of steps).  So no workgroup depends on another: no atomics, no meetings, and
// the arguments are the same for every move.
#pragma once
#include "eval.h"

namespace ddq {

// play = 0: render the current boards into pool_in only (ddq_actors_create).
// thresh = ceil(epsilon * 2^53): explore iff (r >> 11) < thresh.
__global__ __launch_bounds__(kActorThreads) void pool_env_kernel(
    ActorState* __restrict__ games, const uint8_t* __restrict__ maps, const float* __restrict__ q,
    uint64_t thresh, int play, int S, int64_t lane_len, int64_t h0, int64_t v0,
    uint8_t* __restrict__ r_state, uint8_t* __restrict__ r_action, int16_t* __restrict__ r_reward,
    uint8_t* __restrict__ r_nonterm, ReplayMeta* __restrict__ meta, float* __restrict__ pool_in,
    const PrioTree* __restrict__ prio) {
  __shared__ int8_t bd[5 * kCells];     // 4-frame history (oldest first), then init_board
  __shared__ int8_t nbd[kCells];        // the board after this move
  __shared__ uint8_t lv[4 * kCells];    // gray levels of the next state's four boards
  __shared__ int64_t s_slot;            // ring slot that receives the frames, -1: none
  __shared__ int s_over;
  const int t = threadIdx.x, gi = blockIdx.x;
  ActorState* as = games + gi;
  for (int i = t; i < 5 * kCells; i += kActorThreads) bd[i] = as->boards[i];
  if (t == 0) { s_slot = -1; s_over = 0; }
  __syncthreads();

  if (play && t == 0) {
    const int8_t* cur = bd + 3 * kCells;
    int act = actor_first_max(q + 4 * gi);
    const uint64_t seed = as->seed;
    uint64_t k = as->draws;
    if ((actor_draw(seed, k) >> 11) < thresh) act = (int)__umul64hi(actor_draw(seed, k), kActions);
    const int reward = snake_move(cur, nbd, act, seed, k);
    const bool over = reward < 0;
    // the transition's scalars into the lane's slot (h0 + steps) mod lane_len
    const int64_t steps = as->steps;
    const int64_t h = (h0 + steps) % lane_len;
    const int64_t slot = (int64_t)gi * lane_len + h;
    r_action[slot] = (uint8_t)act;
    r_reward[slot] = (int16_t)reward;
    r_nonterm[slot] = over ? 0 : 1;
    if (!over) s_slot = slot;            // a terminal step leaves the slot's frames stale
    if (gi == 0) {                       // the lanes' shared head / valid
      meta->head = h + 1 == lane_len ? 0 : h + 1;
      const int64_t v = v0 + steps + 1;
      meta->valid = v < lane_len ? v : lane_len;
    }
    // prioritized replay: the writer rule (prio.h) on this lane's slot; the
    // lanes' shared ancestors take integer atomic adds, which are exact
    if (prio) {
      const int64_t v2 = v0 + steps + 1;
      prio_on_add(*prio, (int64_t)gi * lane_len, (int)h, (int)lane_len,
                  (int)(h + 1 == lane_len ? 0 : h + 1), (int)(v2 < lane_len ? v2 : lane_len),
                  meta->nstep);
    }
    s_over = over;
    as->draws = k;
    as->steps = steps + 1;
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
  // u8 (C,H,W) into the lane's slot, f32 NHWC into the game's slice of pool_in
  const int SS = S * S;
  uint8_t* slot = s_slot >= 0 ? r_state + (size_t)s_slot * 4 * SS : nullptr;
  float* in = pool_in + (size_t)gi * SS * 4;
  for (int p4 = t; p4 * 4 < SS; p4 += kActorThreads) {
    const int p = p4 * 4;
    uchar4 px[4];
    actor_pixels(lv, maps, S, p, px);
    if (slot) {
#pragma unroll
      for (int f = 0; f < 4; ++f) *reinterpret_cast<uchar4*>(slot + (size_t)f * SS + p) = px[f];
    }
    actor_store_nhwc(in, p, px);
  }
}

hipError_t launch_pool_env(const PoolEnv& e, const float* q, uint64_t thresh, int play,
                           hipStream_t s) {
  ddq_launch(pool_env_kernel, dim3(e.ngames), dim3(kActorThreads), 0, s, e.games, e.maps, q,
             thresh, play, e.S, e.lane_len, e.h0, e.v0, e.r_state, e.r_action, e.r_reward,
             e.r_nonterm, e.meta, e.pool_in, e.prio);
  CHECK_LAUNCH(hipGetLastError());
  return hipSuccess;
}

}  // namespace ddq
