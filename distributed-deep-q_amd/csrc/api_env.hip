// libddq_hip C-ABI: the device-resident Snake environments.
#include <cmath>

#include "ctx.h"

using namespace ddq;
// (the ddq_* definitions take their C linkage from include/ddq_hip.h)

// ---------------- device-resident Snake environments ----------------
// The single actor (ddq_actor_*), the policy evaluator (ddq_eval_*) and the
// actor pool (ddq_actors_*): one kernel body under three roles (env.h), one
// set-up path (env_create) and one lock-step move (env_move) here.

// expgain.epsilon (expgain.py:55-60) in double, same operation order
static double actor_epsilon(int64_t it) {
  const double lo = 0.1, hi = 1.0, limit = 50000.0;
  if (it > 50000) return lo;
  const int64_t left = std::max<int64_t>(50000 - it, 0);
  return lo + (hi - lo) * (double)left / limit;
}

// explore iff random() = (r >> 11) * 2^-53 < epsilon, i.e. (r >> 11) < ceil(epsilon * 2^53)
static uint64_t env_thresh(double epsilon) {
  return (uint64_t)std::ceil(epsilon * 9007199254740992.0);
}

static uint64_t env_mix64(uint64_t x) {   // splitmix64
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// seed of game g's stream: splitmix64(splitmix64(seed) ^ g) (ddq.actor.game_seed)
static uint64_t env_game_seed(uint64_t seed, int g) {
  return env_mix64(env_mix64(seed) ^ (uint64_t)g);
}

// init_board: snake cells are exactly the codes 0..k-1 (k >= 2), head and neck
// neighbours; every other cell empty (-1) or apple (-2)
const char* ddq::actor_board_error(const int8_t* b) {
  int at[100];
  int k = 0;
  for (int i = 0; i < 100; ++i) at[i] = -1;
  for (int c = 0; c < 100; ++c) {
    const int v = b[c];
    if (v < -2 || v >= 100) return "board code out of range";
    if (v >= 0) {
      if (at[v] >= 0) return "snake code used twice";
      at[v] = c;
      ++k;
    }
  }
  if (k < 2) return "snake shorter than 2 cells";
  for (int i = 0; i < k; ++i)
    if (at[i] < 0) return "snake codes are not 0..k-1";
  const int dx = at[0] / 10 - at[1] / 10, dy = at[0] % 10 - at[1] % 10;
  if (std::abs(dx) + std::abs(dy) != 1) return "head and neck are not neighbours";
  return nullptr;
}

// row_map / col_map checked and packed into the kernel's [2S] byte maps
static int env_pack_maps(ddq_ctx* c, const int32_t* row_map, const int32_t* col_map,
                         std::vector<uint8_t>* maps) {
  const int S = c->nb.S;
  maps->resize(2 * (size_t)S);
  for (int i = 0; i < S; ++i) {
    if (row_map[i] < 0 || row_map[i] >= 10 || col_map[i] < 0 || col_map[i] >= 10)
      return fail(c, DDQ_EINVAL, "zoom map entry %d outside [0,10)", i);
    (*maps)[i] = (uint8_t)row_map[i];
    (*maps)[S + i] = (uint8_t)col_map[i];
  }
  return DDQ_OK;
}

// n start boards; single: the one board of ddq_actor_create's init_board
static int env_check_boards(ddq_ctx* c, const int8_t* boards, int n, bool single) {
  for (int g = 0; g < n; ++g)
    if (const char* why = actor_board_error(boards + 100 * g))
      return single ? fail(c, DDQ_EINVAL, "init_board: %s", why)
                    : fail(c, DDQ_EINVAL, "init_boards[%d]: %s", g, why);
  return DDQ_OK;
}

// a game at create: zero counters, its stream's seed, five copies of its start board
template <class Game>
static Game env_new_game(uint64_t seed, const int8_t* board) {
  Game g{};
  g.seed = seed;
  for (int f = 0; f < 5; ++f) memcpy(g.boards + f * 100, board, 100);
  return g;
}

ActorRole ddq::actor_role(const ddq_ctx* c) { return ActorRole{c->envs.a_env.games, c->replay.ring}; }
static EvalRole eval_role(const ddq_ctx* c) {
  return EvalRole{c->envs.e_env.games, c->envs.e_log, c->envs.e_max_moves, c->envs.e_max_ep};
}
PoolRole ddq::pool_role(const ddq_ctx* c) {
  return PoolRole{c->envs.p_env.games, c->replay.ring, c->replay.lane_len, c->envs.p_h0, c->envs.p_v0};
}

// (Re)create an environment: its buffers allocated once with room for `room`
// games, the games and the maps filled, then the render-only launch (play = 0)
// of the start states into b->in.  b->n stays 0 when any of it fails.  The
// role's own ctx fields are set before the call.
template <class Game, class Role>
static int env_create(ddq_ctx* c, EnvBufs<Game>* b, int room, const std::vector<Game>& gs,
                      const std::vector<uint8_t>& maps, Role (*role)(const ddq_ctx*),
                      const char* what) {
  const int S = c->nb.S;
  b->n = 0;
  if (!b->games) TRY(dalloc(c, &b->games, (size_t)room));
  if (!b->maps) TRY(dalloc(c, &b->maps, maps.size()));
  if (!b->in) TRY(dalloc(c, &b->in, (size_t)room * S * S * 4));
  HIP_TRY(c, scopy(c, b->games, gs.data(), gs.size() * sizeof(Game), hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, b->maps, maps.data(), maps.size(), hipMemcpyHostToDevice));
  b->n = (int)gs.size();
  const hipError_t e = launch_env(role(c), env_io(c, *b), c->act.act_q, 0, 0, c->stream);
  if (e != hipSuccess) {
    b->n = 0;
    return fail(c, DDQ_EHIP, "%s render failed: %s", what, hipGetErrorString(e));
  }
  return DDQ_OK;
}

// One lock-step move: the Q forward of ddq_select_action at n = b.n on the
// environment's own input (the act_* scratch is shared with ddq_select_action
// and the other environments: calls on a ctx are serialised), then the
// environment kernel.
// (Eager enqueue on purpose: the move's launch arguments never change, so it
// replays from a captured graph, and that was built and measured for the
// evaluator -- 72.3 us per move against 73.1 eager at 64x64, N = 32, the device
// being the limit at 19 us of host enqueue per move;
// profiles/eval_rate_graph_ab.json.  Not faster beyond the noise, so it is
// not kept.)
// The ring roles (the actor, the pool) act on the perturbed set while
// parameter-space noise is on, and count the move; the evaluator never does.
template <class Role, class Game>
static int env_move(ddq_ctx* c, const Role& r, const EnvBufs<Game>& b, uint64_t thresh) {
  const ActWeights* over = nullptr;
  if (Role::kRing) TRY(param_noise_move(c, &over));
  HIP_TRY(c, launch_act(c->nb, b.in, b.n, c->act.act_p3, c->act.act_h4, c->act.act_part, c->act.act_q, nullptr,
                        c->act.act_p1s, c->act.act_p2s, c->stream, {}, c->act.act_path, 0, over));
  HIP_TRY(c, launch_env(r, env_io(c, b), c->act.act_q, thresh, 1, c->stream));
  return DDQ_OK;
}

int ddq_actor_create(ddq_ctx* c, const int8_t* init_board, const int32_t* row_map,
                     const int32_t* col_map, uint64_t seed) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!init_board || !row_map || !col_map) return fail(c, DDQ_EINVAL, "null argument");
  std::vector<uint8_t> maps;
  TRY(env_pack_maps(c, row_map, col_map, &maps));
  TRY(env_check_boards(c, init_board, 1, true));
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->replay.lanes > 1)
    return fail(c, DDQ_ESTATE, "ddq_actor_create on a laned ring (%d lanes): use ddq_actors_create",
                c->replay.lanes);
  TRY(set_dev(c));
  // the one game's stream takes the seed verbatim
  const std::vector<ActorState> gs{env_new_game<ActorState>(seed, init_board)};
  return env_create(c, &c->envs.a_env, 1, gs, maps, actor_role, "actor");
}

int ddq_actor_step_async(ddq_ctx* c, int32_t nsteps, int64_t iter_num) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->envs.a_env.n) return fail(c, DDQ_ESTATE, "no actor (call ddq_actor_create)");
  if (nsteps < 1) return fail(c, DDQ_EINVAL, "nsteps must be >= 1 (got %d)", nsteps);
  TRY(guard(c));
  const uint64_t thresh = env_thresh(actor_epsilon(iter_num));
  const ActorRole r = actor_role(c);
  for (int i = 0; i < nsteps; ++i) TRY(env_move(c, r, c->envs.a_env, thresh));
  // host mirror of the ring: one transition per step, as ddq_replay_add
  c->replay.head = (c->replay.head + nsteps) % c->replay.capacity;
  c->replay.valid = std::min(c->replay.capacity, c->replay.valid + nsteps);
  return DDQ_OK;
}

int ddq_actor_read(ddq_ctx* c, int8_t* boards, int64_t* stats) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->envs.a_env.n) return fail(c, DDQ_ESTATE, "no actor (call ddq_actor_create)");
  TRY(set_dev(c));
  ActorState st;
  HIP_TRY(c, scopy(c, &st, c->envs.a_env.games, sizeof(st), hipMemcpyDeviceToHost));
  if (boards) memcpy(boards, st.boards, 400);
  if (stats) {
    stats[0] = st.steps; stats[1] = st.games; stats[2] = st.reward_sum;
    stats[3] = (int64_t)st.draws;
  }
  return DDQ_OK;
}

int ddq_eval_create(ddq_ctx* c, int32_t ngames, const int8_t* init_boards, const int32_t* row_map,
                    const int32_t* col_map, uint64_t seed, double epsilon, int32_t max_moves,
                    int32_t max_episodes) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!init_boards || !row_map || !col_map) return fail(c, DDQ_EINVAL, "null argument");
  const int B = c->nb.B;
  if (ngames < 1 || ngames > B)
    return fail(c, DDQ_EINVAL, "ngames must be in [1,B] (got %d, B = %d)", ngames, B);
  if (!(epsilon >= 0.0 && epsilon <= 1.0))
    return fail(c, DDQ_EINVAL, "epsilon must be in [0,1] (got %g)", epsilon);
  if (max_moves < 0) return fail(c, DDQ_EINVAL, "max_moves must be >= 0 (got %d)", max_moves);
  if (max_episodes < 1)
    return fail(c, DDQ_EINVAL, "max_episodes must be >= 1 (got %d)", max_episodes);
  std::vector<uint8_t> maps;
  TRY(env_pack_maps(c, row_map, col_map, &maps));
  TRY(env_check_boards(c, init_boards, ngames, false));
  TRY(set_dev(c));
  c->envs.e_env.n = 0;                    // before the log it plays into is replaced
  const size_t nlog = (size_t)ngames * max_episodes * 4;
  if (nlog > c->envs.e_log_cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    dfree(c, c->envs.e_log);
    c->envs.e_log_cap = 0;
    TRY(dalloc(c, &c->envs.e_log, nlog));
    c->envs.e_log_cap = nlog;
  }
  HIP_TRY(c, hipMemsetAsync(c->envs.e_log, 0, nlog * sizeof(int32_t), c->stream));
  c->envs.e_max_moves = max_moves;
  c->envs.e_max_ep = max_episodes;
  c->envs.e_thresh = env_thresh(epsilon);   // epsilon = 0: no coin at all
  c->envs.e_moves = 0;
  std::vector<EvalGame> gs(ngames);
  for (int g = 0; g < ngames; ++g)
    gs[g] = env_new_game<EvalGame>(env_game_seed(seed, g), init_boards + 100 * g);
  return env_create(c, &c->envs.e_env, B, gs, maps, eval_role, "eval");
}

int ddq_eval_run_async(ddq_ctx* c, int32_t nmoves) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->envs.e_env.n) return fail(c, DDQ_ESTATE, "no evaluator (call ddq_eval_create)");
  if (nmoves < 1) return fail(c, DDQ_EINVAL, "nmoves must be >= 1 (got %d)", nmoves);
  TRY(guard(c));
  const EvalRole r = eval_role(c);
  for (int i = 0; i < nmoves; ++i) TRY(env_move(c, r, c->envs.e_env, c->envs.e_thresh));
  c->envs.e_moves += nmoves;
  return DDQ_OK;
}

int ddq_eval_read(ddq_ctx* c, int64_t* stats, int32_t* episodes, int32_t* log, int8_t* boards,
                  uint64_t* draws) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->envs.e_env.n) return fail(c, DDQ_ESTATE, "no evaluator (call ddq_eval_create)");
  TRY(set_dev(c));
  const int n = c->envs.e_env.n;
  std::vector<EvalGame> gs(n);
  HIP_TRY(c, scopy(c, gs.data(), c->envs.e_env.games, gs.size() * sizeof(EvalGame),
                   hipMemcpyDeviceToHost));
  if (log)
    HIP_TRY(c, scopy(c, log, c->envs.e_log, (size_t)n * c->envs.e_max_ep * 4 * sizeof(int32_t),
                     hipMemcpyDeviceToHost));
  int64_t eps = 0, rew = 0, dr = 0;
  for (int g = 0; g < n; ++g) {
    eps += gs[g].episodes;
    rew += gs[g].reward_sum;
    dr += (int64_t)gs[g].draws;
    if (episodes) episodes[g] = gs[g].episodes;
    if (boards) memcpy(boards + 400 * g, gs[g].boards, 400);
    if (draws) draws[g] = gs[g].draws;
  }
  if (stats) { stats[0] = c->envs.e_moves; stats[1] = eps; stats[2] = rew; stats[3] = dr; }
  return DDQ_OK;
}

int ddq_actors_create(ddq_ctx* c, int32_t ngames, const int8_t* init_boards,
                      const int32_t* row_map, const int32_t* col_map, uint64_t seed) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!init_boards || !row_map || !col_map) return fail(c, DDQ_EINVAL, "null argument");
  const int B = c->nb.B;
  if (ngames < 1 || ngames > B)
    return fail(c, DDQ_EINVAL, "ngames must be in [1,B] (got %d, B = %d)", ngames, B);
  std::vector<uint8_t> maps;
  TRY(env_pack_maps(c, row_map, col_map, &maps));
  TRY(env_check_boards(c, init_boards, ngames, false));
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (ngames != c->replay.lanes)
    return fail(c, DDQ_EINVAL, "ngames %d != the ring's %d lanes (ddq_replay_set_lanes)", ngames,
                c->replay.lanes);
  TRY(set_dev(c));
  // the games' slots come from the ring's per-lane head / valid now
  c->envs.p_h0 = c->replay.head;
  c->envs.p_v0 = c->replay.valid;
  c->envs.p_moves = 0;
  std::vector<ActorState> gs(ngames);
  for (int g = 0; g < ngames; ++g)
    gs[g] = env_new_game<ActorState>(env_game_seed(seed, g), init_boards + 100 * g);
  return env_create(c, &c->envs.p_env, B, gs, maps, pool_role, "pool");
}

int ddq_actors_step_async(ddq_ctx* c, int32_t nmoves, int64_t iter_num) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->envs.p_env.n) return fail(c, DDQ_ESTATE, "no actor pool (call ddq_actors_create)");
  if (nmoves < 1) return fail(c, DDQ_EINVAL, "nmoves must be >= 1 (got %d)", nmoves);
  // the games' slots come from (h0, v0) and their own step counters
  if (c->replay.head != (c->envs.p_h0 + c->envs.p_moves) % c->replay.lane_len)
    return fail(c, DDQ_ESTATE, "the ring's head moved since ddq_actors_create: create the pool again");
  TRY(guard(c));
  const uint64_t thresh = env_thresh(actor_epsilon(iter_num));
  const PoolRole r = pool_role(c);
  for (int i = 0; i < nmoves; ++i) TRY(env_move(c, r, c->envs.p_env, thresh));
  // host mirror of the ring: one transition per lane and move
  c->envs.p_moves += nmoves;
  c->replay.head = (c->replay.head + nmoves) % c->replay.lane_len;
  c->replay.valid = std::min(c->replay.lane_len, c->replay.valid + nmoves);
  return DDQ_OK;
}

int ddq_actors_read(ddq_ctx* c, int8_t* boards, int64_t* stats, int64_t* totals) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->envs.p_env.n) return fail(c, DDQ_ESTATE, "no actor pool (call ddq_actors_create)");
  TRY(set_dev(c));
  const int n = c->envs.p_env.n;
  std::vector<ActorState> gs(n);
  HIP_TRY(c, scopy(c, gs.data(), c->envs.p_env.games, gs.size() * sizeof(ActorState),
                   hipMemcpyDeviceToHost));
  int64_t tot[4] = {0, 0, 0, 0};
  for (int g = 0; g < n; ++g) {
    const int64_t st[4] = {gs[g].steps, gs[g].games, gs[g].reward_sum, (int64_t)gs[g].draws};
    for (int k = 0; k < 4; ++k) {
      tot[k] += st[k];
      if (stats) stats[4 * g + k] = st[k];
    }
    if (boards) memcpy(boards + 400 * g, gs[g].boards, 400);
  }
  if (totals) memcpy(totals, tot, sizeof(tot));
  return DDQ_OK;
}
