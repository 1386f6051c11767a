// libddq_hip C-ABI: checkpoint and resume, host side.
#include "ctx.h"

using namespace ddq;
// (the ddq_* definitions take their C linkage from include/ddq_hip.h)

// ---------------- checkpoint and resume ----------------
// The training state as named sections (include/ddq_hip.h): device buffers
// read and written in place, and two small structs assembled on the host --
// "config", a fingerprint that is only ever compared, and "counters", which a
// restore holds in c->state.st_ctr until ddq_state_commit pushes it.
static_assert(sizeof(ddq_state_section) == 32 && sizeof(ddq_state_config) == 64 &&
                  sizeof(ddq_state_counters) == 96 && sizeof(ActorState) == 544,
              "the state sections' fixed sizes (include/ddq_hip.h)");

static constexpr int kStateMax = 16;   // sections at most (13 today)
struct StateSec {
  const char* name;
  int64_t bytes;
  void* dev;        // nullptr: "config" / "counters", assembled on the host
};

static int state_table(const ddq_ctx* c, StateSec* t) {
  const NetBuffers& nb = c->nb;
  const int64_t P4 = nb.L.total * 4, cap = c->replay.capacity;
  int n = 0;
  t[n++] = {"config", (int64_t)sizeof(ddq_state_config), nullptr};
  t[n++] = {"theta_q", P4, nb.theta[0]};
  t[n++] = {"theta_p", P4, nb.theta[1]};
  t[n++] = {"opt", P4, nb.opt};
  if (c->adam_on) t[n++] = {"opt2", P4, nb.opt2};
  t[n++] = {"counters", (int64_t)sizeof(ddq_state_counters), nullptr};
  if (c->replay.ring.state) {
    t[n++] = {"ring_state", cap * 4 * nb.S * nb.S, c->replay.ring.state};
    t[n++] = {"ring_action", cap, c->replay.ring.action};
    t[n++] = {"ring_reward", 2 * cap, c->replay.ring.reward};
    t[n++] = {"ring_nonterm", cap, c->replay.ring.nonterm};
  }
  if (c->prio.prio_on) t[n++] = {"prio_leaf", 4 * cap, nb.prio.leaf};
  if (c->envs.a_env.n) t[n++] = {"actor", (int64_t)sizeof(ActorState), c->envs.a_env.games};
  if (c->envs.p_env.n) t[n++] = {"pool", (int64_t)c->envs.p_env.n * (int64_t)sizeof(ActorState), c->envs.p_env.games};
  return n;
}

static ddq_state_config state_config(const ddq_ctx* c) {
  const NetBuffers& nb = c->nb;
  ddq_state_config k;
  memset(&k, 0, sizeof(k));
  k.batch = (int16_t)nb.B;
  k.frame = (int16_t)nb.S;
  memcpy(&k.gamma_bits, &nb.gamma, 4);
  const bool ring = c->replay.ring.state != nullptr;
  k.capacity = ring ? c->replay.capacity : 0;
  k.lanes = ring ? c->replay.lanes : 1;
  k.nstep = (uint8_t)(ring ? c->replay.nstep : 1);
  if (c->prio.prio_on) {
    k.prio_enabled = 1;
    k.prio_alpha = c->prio.prio_cfg.alpha; k.prio_beta = c->prio.prio_cfg.beta; k.prio_eps = c->prio.prio_cfg.eps;
  }
  k.obj_target = (uint8_t)nb.obj_target;
  k.obj_loss = (uint8_t)nb.obj_loss;
  k.huber_delta = nb.huber_delta;
  if (c->adam_on) {
    k.adam_on = 1;
    k.adam_beta1 = nb.adam_beta1; k.adam_beta2 = nb.adam_beta2;
    k.adam_eps = nb.adam_eps; k.adam_max_grad_norm = nb.adam_clip;
  }
  k.actor = c->envs.a_env.n ? 1 : 0;
  k.pool_games = (int16_t)c->envs.p_env.n;
  k.target_tau = nb.target_tau;
  return k;
}

// the first field in which two configs differ, nullptr: equal
static const char* state_config_diff(const ddq_state_config& a, const ddq_state_config& b) {
#define DDQ_CFG_FIELD(f) \
  if (memcmp(&a.f, &b.f, sizeof(a.f)) != 0) return #f;
  DDQ_CFG_FIELD(batch) DDQ_CFG_FIELD(frame) DDQ_CFG_FIELD(gamma_bits) DDQ_CFG_FIELD(capacity)
  DDQ_CFG_FIELD(lanes) DDQ_CFG_FIELD(nstep) DDQ_CFG_FIELD(prio_enabled) DDQ_CFG_FIELD(obj_target)
  DDQ_CFG_FIELD(obj_loss) DDQ_CFG_FIELD(prio_alpha) DDQ_CFG_FIELD(prio_beta) DDQ_CFG_FIELD(prio_eps)
  DDQ_CFG_FIELD(huber_delta) DDQ_CFG_FIELD(adam_on) DDQ_CFG_FIELD(actor) DDQ_CFG_FIELD(pool_games)
  DDQ_CFG_FIELD(adam_beta1) DDQ_CFG_FIELD(adam_beta2) DDQ_CFG_FIELD(adam_eps)
  DDQ_CFG_FIELD(adam_max_grad_norm) DDQ_CFG_FIELD(target_tau)
#undef DDQ_CFG_FIELD
  return nullptr;
}

// the counters as the device has them (the stream is idle)
static int state_counters_now(ddq_ctx* c, ddq_state_counters* k) {
  memset(k, 0, sizeof(*k));
  HIP_TRY(c, scopy(c, &k->iteration, c->nb.iter, 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, scopy(c, &k->opt_init, c->nb.opt_init, 4, hipMemcpyDeviceToHost));
  k->steps = c->steps;
  if (c->replay.ring.state) {
    ReplayMeta m;
    HIP_TRY(c, scopy(c, &m, c->replay.ring.meta, sizeof(m), hipMemcpyDeviceToHost));
    k->head = m.head;
    k->valid = m.valid;
    k->draws = m.counter;
    k->ring_err = m.err;
    k->batch_ctr = c->replay.batch_ctr;
  }
  if (c->envs.p_env.n) {
    k->pool_h0 = c->envs.p_h0;
    k->pool_v0 = c->envs.p_v0;
    k->pool_moves = c->envs.p_moves;
  }
  if (c->prio.prio_on) {
    PrioState st;
    HIP_TRY(c, scopy(c, &st, c->nb.prio.st, sizeof(st), hipMemcpyDeviceToHost));
    k->pmax = st.pmax;
  }
  return DDQ_OK;
}

// Every state call begins here: not during the async exchange (the central
// model lives in the owners' shards), the ctx's streams idle, the scratch there.
static int state_begin(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->async.async_on)
    return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx: its state is spread "
                               "over the owners' shards");
  TRY(set_dev(c));
  if (c->comm.cs) HIP_TRY(c, hipStreamSynchronize(c->comm.cs));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (!c->state.st_dev) TRY(dalloc(c, &c->state.st_dev, (size_t)kStateParts + kStateMax + 16 + 2));
  return DDQ_OK;
}

static int state_find(ddq_ctx* c, const char* name, StateSec* out) {
  if (!name) return fail(c, DDQ_EINVAL, "null section name");
  StateSec t[kStateMax];
  const int n = state_table(c, t);
  for (int i = 0; i < n; ++i)
    if (!strcmp(t[i].name, name)) {
      *out = t[i];
      return DDQ_OK;
    }
  return fail(c, DDQ_EINVAL, "no section '%s' on this ctx", name);
}

// a host-assembled section's bytes: the config; the counters as written while
// restoring, as the device has them otherwise
static int state_host_bytes(ddq_ctx* c, const StateSec& s, uint8_t* buf) {
  if (!strcmp(s.name, "config")) {
    const ddq_state_config k = state_config(c);
    memcpy(buf, &k, sizeof(k));
    return DDQ_OK;
  }
  ddq_state_counters k;
  if (c->state.restoring) k = c->state.st_ctr;
  else TRY(state_counters_now(c, &k));
  memcpy(buf, &k, sizeof(k));
  return DDQ_OK;
}

// enqueue section s's digest into digest word `slot` of the scratch; stage: its
// 64-byte-aligned slice of the scratch for a host-assembled section
static int state_enqueue_digest(ddq_ctx* c, const StateSec& s, int slot) {
  uint64_t* part = c->state.st_dev;
  uint64_t* dig = c->state.st_dev + kStateParts;
  const void* p = s.dev;
  if (!p) {
    uint8_t buf[128];
    TRY(state_host_bytes(c, s, buf));
    uint64_t* stage = dig + kStateMax;
    HIP_TRY(c, scopy(c, stage, buf, (size_t)s.bytes, hipMemcpyHostToDevice));
    p = stage;
  }
  HIP_TRY(c, launch_state_digest(p, (uint64_t)s.bytes, part, dig + slot, c->stream));
  return DDQ_OK;
}

int ddq_state_sections(ddq_ctx* c, ddq_state_section* out, int32_t cap, int32_t* n) {
  TRY(state_begin(c));
  if (!n) return fail(c, DDQ_EINVAL, "null argument");
  StateSec t[kStateMax];
  const int k = state_table(c, t);
  *n = k;
  if (!out) return DDQ_OK;
  if (cap < k) return fail(c, DDQ_EINVAL, "the ctx has %d sections (cap = %d)", k, cap);
  // (the launches of one section reuse the partials: stream order keeps them apart)
  for (int i = 0; i < k; ++i) TRY(state_enqueue_digest(c, t[i], i));
  uint64_t dig[kStateMax];
  HIP_TRY(c, scopy(c, dig, c->state.st_dev + kStateParts, sizeof(dig), hipMemcpyDeviceToHost));
  for (int i = 0; i < k; ++i) {
    memset(&out[i], 0, sizeof(out[i]));
    snprintf(out[i].name, sizeof(out[i].name), "%s", t[i].name);
    out[i].bytes = t[i].bytes;
    out[i].digest = dig[i];
  }
  return DDQ_OK;
}

int ddq_state_digest(ddq_ctx* c, const char* name, uint64_t* digest) {
  TRY(state_begin(c));
  if (!digest) return fail(c, DDQ_EINVAL, "null argument");
  StateSec s{};
  TRY(state_find(c, name, &s));
  TRY(state_enqueue_digest(c, s, 0));
  HIP_TRY(c, scopy(c, digest, c->state.st_dev + kStateParts, 8, hipMemcpyDeviceToHost));
  return DDQ_OK;
}

static int state_range(ddq_ctx* c, const StateSec& s, int64_t offset, int64_t bytes) {
  if (offset < 0 || bytes <= 0 || offset > s.bytes || bytes > s.bytes - offset)
    return fail(c, DDQ_EINVAL, "section '%s' has %lld bytes: [%lld, %lld + %lld) is not inside it",
                s.name, (long long)s.bytes, (long long)offset, (long long)offset, (long long)bytes);
  return DDQ_OK;
}

int ddq_state_read(ddq_ctx* c, const char* name, int64_t offset, void* dst, int64_t bytes) {
  TRY(state_begin(c));
  if (!dst) return fail(c, DDQ_EINVAL, "null argument");
  StateSec s{};
  TRY(state_find(c, name, &s));
  TRY(state_range(c, s, offset, bytes));
  if (s.dev) {
    HIP_TRY(c, scopy(c, dst, (const uint8_t*)s.dev + offset, (size_t)bytes, hipMemcpyDeviceToHost));
    return DDQ_OK;
  }
  uint8_t buf[128];
  TRY(state_host_bytes(c, s, buf));
  memcpy(dst, buf + offset, (size_t)bytes);
  return DDQ_OK;
}

int ddq_state_write(ddq_ctx* c, const char* name, int64_t offset, const void* src, int64_t bytes) {
  TRY(state_begin(c));
  if (!src) return fail(c, DDQ_EINVAL, "null argument");
  StateSec s{};
  TRY(state_find(c, name, &s));
  TRY(state_range(c, s, offset, bytes));
  if (!strcmp(s.name, "config")) {   // compared, never written
    if (offset != 0 || bytes != s.bytes)
      return fail(c, DDQ_EINVAL, "section 'config' is compared as a whole (%lld bytes)", (long long)s.bytes);
    ddq_state_config theirs;
    memcpy(&theirs, src, sizeof(theirs));
    if (const char* f = state_config_diff(state_config(c), theirs))
      return fail(c, DDQ_EINVAL, "config mismatch: field '%s' of the checkpoint differs from this ctx "
                                 "(configure the ctx as the writer was configured)", f);
    return DDQ_OK;
  }
  if (!c->state.restoring) {
    TRY(state_counters_now(c, &c->state.st_ctr));
    c->state.restoring = true;
  }
  if (!s.dev) {
    memcpy(reinterpret_cast<uint8_t*>(&c->state.st_ctr) + offset, src, (size_t)bytes);
    return DDQ_OK;
  }
  HIP_TRY(c, scopy(c, (uint8_t*)s.dev + offset, src, (size_t)bytes, hipMemcpyHostToDevice));
  return DDQ_OK;
}

int ddq_state_commit(ddq_ctx* c) {
  TRY(state_begin(c));
  if (!c->state.restoring) return DDQ_OK;
  const ddq_state_counters k = c->state.st_ctr;
  const bool ring = c->replay.ring.state != nullptr;
  const int64_t L = c->replay.lane_len;
  // ---- validation: nothing is pushed before all of it passed ----
  if (k.iteration < 0 || k.steps < 0 || (k.opt_init != 0 && k.opt_init != 1) || k.ring_err < 0 ||
      k.ring_err > 2 || k.reserved[0] || k.reserved[1] || k.reserved[2])
    return fail(c, DDQ_EINVAL, "counters: iteration %lld, steps %lld, opt_init %d, ring_err %d or a "
                               "reserved word out of range",
                (long long)k.iteration, (long long)k.steps, k.opt_init, k.ring_err);
  if (ring ? (k.head < 0 || k.head >= L || k.valid < 0 || k.valid > L)
           : (k.head != 0 || k.valid != 0 || k.draws != 0 || k.batch_ctr != 0))
    return fail(c, DDQ_EINVAL, "counters: head %lld / valid %lld outside the ring's lane length %lld",
                (long long)k.head, (long long)k.valid, (long long)(ring ? L : 0));
  if (c->envs.p_env.n ? (k.pool_h0 < 0 || k.pool_h0 >= L || k.pool_v0 < 0 || k.pool_v0 > L ||
                    k.pool_moves < 0 || k.head != (k.pool_h0 + k.pool_moves % L) % L ||
                    k.valid != std::min(L, k.pool_v0 + std::min(k.pool_moves, L)))
                 : (k.pool_h0 != 0 || k.pool_v0 != 0 || k.pool_moves != 0))
    return fail(c, DDQ_EINVAL, "counters: the pool's h0 %lld, v0 %lld, moves %lld do not give the "
                               "ring's head %lld / valid %lld",
                (long long)k.pool_h0, (long long)k.pool_v0, (long long)k.pool_moves,
                (long long)k.head, (long long)k.valid);
  // the games: boards the environment kernel can play, the pool in lock step
  for (int role = 0; role < 2; ++role) {
    const EnvBufs<ActorState>& b = role ? c->envs.p_env : c->envs.a_env;
    if (!b.n) continue;
    std::vector<ActorState> gs((size_t)b.n);
    HIP_TRY(c, scopy(c, gs.data(), b.games, gs.size() * sizeof(ActorState), hipMemcpyDeviceToHost));
    for (int g = 0; g < b.n; ++g) {
      for (int f = 0; f < 5; ++f)
        if (const char* why = actor_board_error(gs[g].boards + 100 * f))
          return fail(c, DDQ_EINVAL, "%s: game %d, board %d: %s", role ? "pool" : "actor", g, f, why);
      if (gs[g].steps < 0 || (role && gs[g].steps != k.pool_moves))
        return fail(c, DDQ_EINVAL, "%s: game %d made %lld steps (the pool's moves: %lld)",
                    role ? "pool" : "actor", g, (long long)gs[g].steps, (long long)k.pool_moves);
    }
  }
  if (c->prio.prio_on) {
    if (k.pmax < kPrioOne || k.pmax > kPrioMax)
      return fail(c, DDQ_EINVAL, "counters: pmax %u outside [65536, 2^24]", k.pmax);
    int32_t* bad = reinterpret_cast<int32_t*>(c->state.st_dev + kStateParts + kStateMax + 16);
    int32_t hb[2] = {0, INT32_MAX};
    HIP_TRY(c, scopy(c, bad, hb, sizeof(hb), hipMemcpyHostToDevice));
    HIP_TRY(c, launch_state_check_leaves(c->nb.prio, L, k.head, k.valid, c->replay.nstep, bad, c->stream));
    HIP_TRY(c, scopy(c, hb, bad, sizeof(hb), hipMemcpyDeviceToHost));
    if (hb[0])
      return fail(c, DDQ_EINVAL, "prio_leaf: %d leaves are above 2^24 or break \"zero <=> slot unfilled "
                                 "or forbidden\" under head %lld, valid %lld, n %d (first: slot %d)",
                  hb[0], (long long)k.head, (long long)k.valid, c->replay.nstep, hb[1]);
  } else if (k.pmax != 0) {
    return fail(c, DDQ_EINVAL, "counters: pmax %u while prioritized replay is off", k.pmax);
  }
  // ---- push: device memory, then the host mirrors ----
  HIP_TRY(c, hipMemcpyAsync(c->nb.iter, &k.iteration, 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->nb.opt_init, &k.opt_init, 4, hipMemcpyHostToDevice, c->stream));
  if (ring) {
    char* m = reinterpret_cast<char*>(c->replay.ring.meta);
    const int64_t hv[2] = {k.head, k.valid};
    HIP_TRY(c, hipMemcpyAsync(m, hv, sizeof(hv), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(m + offsetof(ReplayMeta, counter), &k.draws, 8, hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, hipMemcpyAsync(m + offsetof(ReplayMeta, err), &k.ring_err, 4, hipMemcpyHostToDevice,
                              c->stream));
  }
  if (c->prio.prio_on) {
    HIP_TRY(c, hipMemcpyAsync(&c->nb.prio.st->pmax, &k.pmax, 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_prio_resum(c->nb.prio, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (k is this frame's: copied before it goes)
  c->applied = k.iteration;
  c->steps = k.steps;
  c->replay.head = k.head;
  c->replay.valid = k.valid;
  c->replay.batch_ctr = k.batch_ctr;
  c->envs.p_h0 = k.pool_h0;
  c->envs.p_v0 = k.pool_v0;
  c->envs.p_moves = k.pool_moves;
  c->pn.on = false;   // the noise state is not checkpointed: off until it is set again
  c->pn.cfg = ddq_param_noise_cfg{};
  // ---- derived: the conv weights' copies of both towers, the games' rendered states ----
  for (int z = 0; z < 2; ++z) HIP_TRY(c, launch_relayout(c->nb, z, c->stream));
  if (c->envs.a_env.n)
    HIP_TRY(c, launch_env(actor_role(c), env_io(c, c->envs.a_env), c->act.act_q, 0, 0, c->stream));
  if (c->envs.p_env.n)
    HIP_TRY(c, launch_env(pool_role(c), env_io(c, c->envs.p_env), c->act.act_q, 0, 0, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);
  c->replay.idx_bound = false;
  c->state.restoring = false;
  return DDQ_OK;
}
