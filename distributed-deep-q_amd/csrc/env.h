// Device-resident Snake environment: the move that follows launch_act's Q
// forward of the games' own NHWC input.  One kernel body, env_body, one
// workgroup per game: epsilon-greedy choice from the game's row of Q, one game
// step by the rules of gamesim/SnakeGame.py (as ddq/snake.py restates them), the
// role's commit, and the render of the next state, which is the next forward's
// input.  Three roles (kernels.h) instantiate it:
//   ActorRole  ddq_actor_*   one generate_experience (expgain.py:82-111): the
//                            transition into ring slot meta->head
//   PoolRole   ddq_actors_*  N actors in lock step, game g into lane g of a
//                            laned ring
//   EvalRole   ddq_eval_*    PolicyEvaluator.evaluate (evaluation.py:10-51): N
//                            games, an episode record instead of a transition
// What a role differs in is its state type, its two flags, env_idle and
// env_commit below; everything else is written once.  Included by kernels.hip
// (uses its splitmix64 and CHECK_LAUNCH) after prio.h.
//
// The game is 100 cells and a handful of branches: one thread plays it on a
// board in LDS (a few hundred LDS reads, no global traffic but the commit's
// scalars), then the whole workgroup renders.  The render is the only part
// with any bytes to move (4 S^2 u8 + 16 S^2 f32: 80 KB at S = 64), written as
// uchar4 / float4 per thread like gather_body reads them; one workgroup per
// game keeps the launch a single dispatch with no inter-workgroup hand-off.
// Nothing is shared between the workgroups: every game has its own RNG stream
// and counters, so the kernel needs no atomics and no ordering, and a role's
// arguments are the same for every move (one captured move replays).
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
// apple is draw k of the stream, k advanced.  The rules exist once.
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

// ---- the roles: env_idle (uniform over the workgroup, checked before anything
// is loaded) and env_commit, thread 0 after snake_move: every global scalar
// of the move.  env_commit returns whether the episode ended; a ring role also
// sets *slot to the ring slot that receives the next state's frames (left at
// -1 after a terminal step: the slot's frames stay stale).

// the transition's scalars into ring slot `slot`
__device__ __forceinline__ void ring_put(const ReplayRing& ring, int64_t slot, int act,
                                         int reward) {
  ring.action[slot] = (uint8_t)act;
  ring.reward[slot] = (int16_t)reward;
  ring.nonterm[slot] = reward < 0 ? 0 : 1;
}

// an acting game's counters (after the ring's words, as add_experience's caller)
__device__ __forceinline__ void actor_count(ActorState* as, int reward, uint64_t k) {
  as->draws = k;
  as->steps += 1;
  as->games += reward < 0;
  as->reward_sum += reward;
}

__device__ __forceinline__ bool env_idle(const ActorRole&, const ActorState*) { return false; }
__device__ __forceinline__ bool env_idle(const PoolRole&, const ActorState*) { return false; }
// a full log: the game is idle (its row of the forward's input keeps its last render)
__device__ __forceinline__ bool env_idle(const EvalRole& r, const EvalGame* g) {
  return g->episodes >= r.max_episodes;
}

// Single actor: slot meta->head, read here so that host ddq_replay_add calls
// may interleave; head / valid advanced here.
__device__ __forceinline__ bool env_commit(const ActorRole& r, ActorState* as, int, int act,
                                           int reward, uint64_t k, int64_t* slot) {
  const bool over = reward < 0;
  ReplayMeta* meta = r.ring.meta;
  const int64_t cap = meta->capacity, h = meta->head;
  if (h >= 0 && h < cap) {
    ring_put(r.ring, h, act, reward);
    if (!over) *slot = h;
    const int64_t nh = h + 1 == cap ? 0 : h + 1;
    meta->head = nh;
    const int64_t v = meta->valid, nv = v < cap ? v + 1 : cap;
    meta->valid = nv;
    // prioritized replay: the writer rule (prio.h) on the slot just written
    if (r.ring.prio) prio_on_add(*r.ring.prio, 0, (int)h, (int)cap, (int)nh, (int)nv, meta->nstep);
  }
  actor_count(as, reward, k);
  return over;
}

// Pool: game gi's slot is lane base + (h0 + its own step counter) mod lane_len
// with the launch constants (h0, v0); nothing here reads meta->head / valid.
// Workgroup 0 alone publishes the new per-lane values (every game has made the
// same number of steps), so no workgroup depends on another.
__device__ __forceinline__ bool env_commit(const PoolRole& r, ActorState* as, int gi, int act,
                                           int reward, uint64_t k, int64_t* slot) {
  const bool over = reward < 0;
  ReplayMeta* meta = r.ring.meta;
  const int64_t len = r.lane_len, steps = as->steps;
  const int64_t h = (r.h0 + steps) % len, base = (int64_t)gi * len;
  ring_put(r.ring, base + h, act, reward);
  if (!over) *slot = base + h;
  const int64_t nh = h + 1 == len ? 0 : h + 1;
  const int64_t v = r.v0 + steps + 1, nv = v < len ? v : len;
  if (gi == 0) {                       // the lanes' shared head / valid
    meta->head = nh;
    meta->valid = nv;
  }
  // prioritized replay: the writer rule (prio.h) on this lane's slot; the
  // lanes' shared ancestors take integer atomic adds, which are exact
  if (r.ring.prio) prio_on_add(*r.ring.prio, base, (int)h, (int)len, (int)nh, (int)nv, meta->nstep);
  actor_count(as, reward, k);
  return over;
}

// Evaluator: the running episode's score / moves, and its record when it ends
__device__ __forceinline__ bool env_commit(const EvalRole& r, EvalGame* g, int gi, int,
                                           int reward, uint64_t k, int64_t*) {
  int score = g->score + reward, moves = g->moves + 1;
  const int mv = g->move;
  // game over wins over max_moves on the same move
  const int end = reward < 0 ? 1 : (r.max_moves > 0 && moves >= r.max_moves ? 2 : 0);
  if (end) {
    const int ep = g->episodes;
    int32_t* rec = r.log + ((size_t)gi * r.max_episodes + ep) * 4;
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
  return end != 0;
}

// play = 0: render the current boards into io.in only (the create calls).
// thresh = ceil(epsilon * 2^53): explore iff (r >> 11) < thresh, which is
// random() < epsilon for random() = (r >> 11) * 2^-53.  A role without
// kCoinAlways draws no coin at thresh == 0 (greedy evaluation).
template <class Role>
__device__ __forceinline__ void env_body(const Role& r, const EnvIO& io,
                                         const float* __restrict__ q, uint64_t thresh, int play) {
  __shared__ int8_t bd[5 * kCells];     // 4-frame history (oldest first), then the start board
  __shared__ int8_t nbd[kCells];        // the board after this move
  __shared__ uint8_t lv[4 * kCells];    // gray levels of the next state's four boards
  __shared__ int64_t s_slot;            // ring slot that receives the frames, -1: none
  __shared__ int s_end;                 // the episode ended with this move
  const int t = threadIdx.x, gi = blockIdx.x;
  typename Role::Game* g = r.games + gi;
  if (play && env_idle(r, g)) return;
  for (int i = t; i < 5 * kCells; i += kActorThreads) bd[i] = g->boards[i];
  if (t == 0) { s_slot = -1; s_end = 0; }
  __syncthreads();

  if (play && t == 0) {
    // 1. greedy action: first maximum of the game's row of Q
    int act = actor_first_max(q + 4 * gi);
    // 2. coin, then the action when exploring
    const uint64_t seed = g->seed;
    uint64_t k = g->draws;
    if ((Role::kCoinAlways || thresh) && (actor_draw(seed, k) >> 11) < thresh)
      act = (int)__umul64hi(actor_draw(seed, k), kActions);
    // 3. one move on the newest board, 4. the role's scalars
    const int reward = snake_move(bd + 3 * kCells, nbd, act, seed, k);
    int64_t slot = -1;
    s_end = env_commit(r, g, gi, act, reward, k, &slot);
    if constexpr (Role::kRing) s_slot = slot;
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

  // render through the zoom maps, 4 pixels of one row per thread (S % 8 == 0):
  // u8 (C,H,W) into the ring slot, f32 NHWC into the game's slice of io.in
  const int S = io.S, SS = S * S;
  uint8_t* frames = nullptr;
  if constexpr (Role::kRing)
    if (s_slot >= 0) frames = r.ring.state + (size_t)s_slot * 4 * SS;
  float* in = io.in + (size_t)gi * SS * 4;
  for (int p4 = t; p4 * 4 < SS; p4 += kActorThreads) {
    const int p = p4 * 4;
    uchar4 px[4];
    actor_pixels(lv, io.maps, S, p, px);
    if constexpr (Role::kRing) {
      if (frames) {
#pragma unroll
        for (int f = 0; f < 4; ++f) *reinterpret_cast<uchar4*>(frames + (size_t)f * SS + p) = px[f];
      }
    }
    actor_store_nhwc(in, p, px);
  }
}

// The three instantiations.  Plain kernels around the one body, not a kernel
// template: a template's instantiations are emitted after every other kernel
// of the code object, and with these three moved there the training kernels
// that follow them shifted and the flagship step, which runs none of this,
// measured 0.5 - 1 % slower (profiles/env_refactor_ab.json).
__global__ __launch_bounds__(kActorThreads) void actor_env_kernel(
    const ActorRole r, const EnvIO io, const float* __restrict__ q, uint64_t thresh, int play) {
  env_body(r, io, q, thresh, play);
}
__global__ __launch_bounds__(kActorThreads) void eval_env_kernel(
    const EvalRole r, const EnvIO io, const float* __restrict__ q, uint64_t thresh, int play) {
  env_body(r, io, q, thresh, play);
}
__global__ __launch_bounds__(kActorThreads) void pool_env_kernel(
    const PoolRole r, const EnvIO io, const float* __restrict__ q, uint64_t thresh, int play) {
  env_body(r, io, q, thresh, play);
}

template <class Kernel, class Role>
static hipError_t launch_env_kernel(Kernel kern, const Role& r, const EnvIO& io, const float* q,
                                    uint64_t thresh, int play, hipStream_t s) {
  ddq_launch(kern, dim3(io.ngames), dim3(kActorThreads), 0, s, r, io, q, thresh, play);
  CHECK_LAUNCH(hipGetLastError());
  return hipSuccess;
}
hipError_t launch_env(const ActorRole& r, const EnvIO& io, const float* q, uint64_t thresh,
                      int play, hipStream_t s) {
  return launch_env_kernel(actor_env_kernel, r, io, q, thresh, play, s);
}
hipError_t launch_env(const EvalRole& r, const EnvIO& io, const float* q, uint64_t thresh, int play,
                      hipStream_t s) {
  return launch_env_kernel(eval_env_kernel, r, io, q, thresh, play, s);
}
hipError_t launch_env(const PoolRole& r, const EnvIO& io, const float* q, uint64_t thresh, int play,
                      hipStream_t s) {
  return launch_env_kernel(pool_env_kernel, r, io, q, thresh, play, s);
}

}  // namespace ddq
