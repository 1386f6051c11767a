// Device-resident policy evaluation (ddq_eval_*): PolicyEvaluator.evaluate
// (evaluation.py:10-51) without the host between the moves.  ngames <= B Snake
// games play in lock step: launch_act's Q forward of all their states at
// n = ngames, then eval_env_kernel, one workgroup per game: the game's action
// from its own row of Q, one move by snake_move (actor.h: the actor's rules,
// not a copy), the episode record when the episode ends, and the render of the
// game's next state into its slice of the forward's input.  Included by
// kernels.hip after actor.h.
//
// Nothing is shared between the workgroups: every game has its own RNG stream,
// move counter and log, so the kernel needs no atomics and no ordering, and
// its arguments are the same for every move (one captured move replays).
#pragma once
#include "actor.h"

namespace ddq {

// play = 0: render the current boards into eval_in only (ddq_eval_create).
// thresh = ceil(epsilon * 2^53); 0: greedy evaluation, no coin is drawn.
__global__ __launch_bounds__(kActorThreads) void eval_env_kernel(
    EvalGame* __restrict__ games, int32_t* __restrict__ log, const uint8_t* __restrict__ maps,
    const float* __restrict__ q, uint64_t thresh, int play, int S, int max_moves,
    int max_episodes, float* __restrict__ eval_in) {
  __shared__ int8_t bd[5 * kCells];     // 4-frame history (oldest first), then the start board
  __shared__ int8_t nbd[kCells];        // the board after this move
  __shared__ uint8_t lv[4 * kCells];    // gray levels of the next state's four boards
  __shared__ int s_end;                 // the episode ended with this move
  const int t = threadIdx.x, gi = blockIdx.x;
  EvalGame* g = games + gi;
  // a full log: the game is idle (uniform over the workgroup; its row of the
  // forward's input keeps its last render)
  if (play && g->episodes >= max_episodes) return;
  for (int i = t; i < 5 * kCells; i += kActorThreads) bd[i] = g->boards[i];
  if (t == 0) s_end = 0;
  __syncthreads();

  if (play && t == 0) {
    const int8_t* cur = bd + 3 * kCells;
    int act = actor_first_max(q + 4 * gi);
    const uint64_t seed = g->seed;
    uint64_t k = g->draws;
    if (thresh && (actor_draw(seed, k) >> 11) < thresh)
      act = (int)__umul64hi(actor_draw(seed, k), kActions);
    const int reward = snake_move(cur, nbd, act, seed, k);
    int score = g->score + reward, moves = g->moves + 1;
    const int mv = g->move;
    // game over wins over max_moves on the same move
    const int end = reward < 0 ? 1 : (max_moves > 0 && moves >= max_moves ? 2 : 0);
    if (end) {
      const int ep = g->episodes;
      int32_t* rec = log + ((size_t)gi * max_episodes + ep) * 4;
      rec[0] = mv; rec[1] = score; rec[2] = moves; rec[3] = end - 1;
      g->episodes = ep + 1;
      score = 0;
      moves = 0;
    }
    g->score = score;
    g->moves = moves;
    g->move = mv + 1;
    g->draws = k;
    g->reward_sum += reward;
    s_end = end;
  }
  __syncthreads();

  // the next state's boards: the history shifted by one, or four start boards
  // after an episode's end (reset_game)
  if (play) {
    const bool end = s_end != 0;
    for (int i = t; i < 4 * kCells; i += kActorThreads) {
      const int f = i / kCells, c = i - f * kCells;
      const int8_t v = end ? bd[4 * kCells + c] : (f < 3 ? bd[i + kCells] : nbd[c]);
      g->boards[i] = v;
      lv[i] = actor_level(v);
    }
  } else {
    for (int i = t; i < 4 * kCells; i += kActorThreads) lv[i] = actor_level(bd[i]);
  }
  __syncthreads();

  // render through the zoom maps, 4 pixels of one row per thread (S % 8 == 0),
  // f32 NHWC into the game's slice of eval_in
  const int SS = S * S;
  float* in = eval_in + (size_t)gi * SS * 4;
  for (int p4 = t; p4 * 4 < SS; p4 += kActorThreads) {
    uchar4 px[4];
    actor_pixels(lv, maps, S, p4 * 4, px);
    actor_store_nhwc(in, p4 * 4, px);
  }
}

hipError_t launch_eval_env(const EvalEnv& e, const float* q, uint64_t thresh, int play,
                           hipStream_t s) {
  ddq_launch(eval_env_kernel, dim3(e.ngames), dim3(kActorThreads), 0, s, e.games, e.log, e.maps,
             q, thresh, play, e.S, e.max_moves, e.max_episodes, e.eval_in);
  CHECK_LAUNCH(hipGetLastError());
  return hipSuccess;
}

}  // namespace ddq
