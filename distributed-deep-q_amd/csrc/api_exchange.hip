// libddq_hip C-ABI: the RCCL communicator and all-reduce, the asynchronous
// parameter server with its tick and round graphs, in-process groups.
#include <thread>

#include "step.h"

using namespace ddq;
// (the ddq_* definitions take their C linkage from include/ddq_hip.h)

// ---------------- comm ----------------
int ddq_comm_get_unique_id(uint8_t id[128]) {
  static_assert(sizeof(ncclUniqueId) == 128, "unique id size");
  ncclUniqueId u;
  ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess) return fail(nullptr, DDQ_ERCCL, "ncclGetUniqueId: %s", ncclGetErrorString(r));
  memcpy(id, &u, 128);
  return DDQ_OK;
}

// Shard geometry and exchange buffers for W ranks (RCCL or in-process).
static int setup_shards(ddq_ctx* c, int W) {
  const int64_t P = c->nb.L.total;
  c->comm.shard_len = ((P + (int64_t)W * 64 - 1) / ((int64_t)W * 64)) * 64;
  if (!c->comm.cs) {
    HIP_TRY(c, hipStreamCreateWithFlags(&c->comm.cs, hipStreamNonBlocking));
    for (auto& e : c->comm.cev) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  // exchange buffers are allocated once for the largest W (kMaxRanks slices
  // of at most P/W + 64 floats fit in P + kShardPad ... per slice set)
  if (!c->comm.gsl) TRY(dalloc(c, &c->comm.gsl, (size_t)P + kShardPad));
  return DDQ_OK;
}

int ddq_comm_init(ddq_ctx* c, const uint8_t id[128], int32_t nranks, int32_t rank) {
  if (!c || !id) return fail(c, DDQ_EINVAL, "null argument");
  if (nranks < 1 || nranks > kMaxRanks || rank < 0 || rank >= nranks)
    return fail(c, DDQ_EINVAL, "bad rank/nranks (nranks <= %d)", kMaxRanks);
  if (c->comm.local) return fail(c, DDQ_ESTATE, "ctx belongs to an in-process group");
  TRY(prio_refuse(c, "ddq_comm_init"));
  TRY(set_dev(c));
  if (c->comm.comm) ncclCommDestroy(c->comm.comm);
  c->comm.comm = nullptr;
  ncclUniqueId u;
  memcpy(&u, id, 128);
  NCCL_TRY(c, ncclCommInitRank(&c->comm.comm, nranks, u, rank));
  c->comm.nranks = nranks;
  c->comm.rank = rank;
  TRY(setup_shards(c, nranks));
  invalidate_graph(c);
  return DDQ_OK;
}

int ddq_allreduce_grads_async(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->comm.comm) return fail(c, DDQ_ESTATE, "no communicator (call ddq_comm_init)");
  TRY(set_dev(c));
  NCCL_TRY(c, ncclAllReduce(c->nb.grad, c->nb.grad, (size_t)c->nb.L.total, ncclFloat, ncclSum,
                            c->comm.comm, c->stream));
  return DDQ_OK;
}

int ddq_allreduce_grads(ddq_ctx* c) {
  TRY(ddq_allreduce_grads_async(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

// ---------------- asynchronous param server (DDQ_EXCHANGE_ASYNC) ----------------
// The reference's workers free-run (main.py:61-112: fetch -> experience ->
// full_pass -> push) against one server that applies every pushed gradient on
// arrival (server.py:196-209) and copies Q -> P on a pull that sees
// iteration % period == 0 (server.py:181-193).  Here rank r owns shard r of
// the central model and its optimizer state; a TICK is one push: worker w's
// gradient slices go to the owners, each owner applies its slice (iteration
// += 1), the owners send worker w their shards (and the central P's when a
// special update happened since w's last pull), and w computes its next
// gradient on the model it pulled while the other ticks proceed.  Which
// worker pushes at each tick is the arrival order: round-robin (the
// deterministic test schedule, one step = W ticks) or ticket order (the
// worker whose gradient is ready first; ddq_async_tick / ddq_group_async_run).

// Worker side: the minibatch draw + gather and the forward/backward on the
// model this worker last pulled (no apply bookkeeping: the owners keep the
// iteration), into nb.grad, on the ctx stream; grad_ev marks it ready.
// drawn: the minibatch was drawn + gathered already (by the owner apply of
// this worker's own push, async_owner_apply)
static int async_compute(ddq_ctx* c, const ddq_step_cfg* cfg, bool drawn = false) {
  StepLaunch sl;
  TRY(plan_launches(c, cfg, step_facts(c, cfg), &sl));
  if (!drawn) TRY(enqueue_draw(c, c->nb, cfg->seed, c->stream));
  TRY(enqueue_fwd_bwd(c, c->nb, sl));
  HIP_TRY(c, hipEventRecord(c->async.grad_ev, c->stream));
  c->async.ready_seen = false;
  c->async.grad_ev_captured = c->async.acapture;
  return DDQ_OK;
}

// The special update (server.py:186-189) runs when a pull sees iteration %
// period == 0; with one pull per tick that is every multiple of the period, so
// a worker's P must be re-pulled iff a multiple lies in (its last pull, now].
static bool async_pull_p(const ddq_step_cfg* cfg, int64_t last, int64_t now) {
  return cfg->target_period > 0 && now / cfg->target_period > last / cfg->target_period;
}

// Start of the async exchange on this ctx (any earlier steps taken, the
// replicas equal): the central model's shards start from this replica (after
// the pull at the current iteration -- a special update when it is a
// multiple of the period, e.g. 0), every worker pulled there, and the
// worker's first gradient is computed on it.
static int async_begin(ddq_ctx* c, const ddq_step_cfg* cfg) {
  const int64_t P = c->nb.L.total;
  if (!c->async.own) TRY(dalloc(c, &c->async.own, (size_t)P + kShardPad));
  if (!c->async.pown) TRY(dalloc(c, &c->async.pown, (size_t)P + kShardPad));
  if (!c->async.grad_ev) {
    HIP_TRY(c, hipEventCreateWithFlags(&c->async.grad_ev, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->async.tick_ev, hipEventDisableTiming));
  }
  TRY(initial_target_sync(c, cfg));
  HIP_TRY(c, hipMemcpyAsync(c->async.own, c->nb.theta[0], P * 4, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->async.pown, c->nb.theta[1], P * 4, hipMemcpyDeviceToDevice, c->stream));
  c->async.last_pull.assign(c->comm.nranks, c->applied);
  c->async.async_on = true;
  // the owner duties run on the comm stream: it starts after the copies
  HIP_TRY(c, hipEventRecord(c->comm.cev[0], c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->comm.cs, c->comm.cev[0], 0));
  return async_compute(c, cfg);
}

// Owner side of a tick, on the comm stream: the received slice (in gsl)
// applied to the owned shard on arrival (iteration += 1, the launch's own
// bookkeeping), and the central P shard updated when this tick's pull (at
// iteration it) is a special update.
// own: the push is this rank's own gradient -- applied from the gradient
// buffer in place (no copy to gsl), and the worker's copy of the shard written
// beside the central one (no pull copy)
// -- and, from the same values, that shard's kernel layouts and (on a tick that
// updates the central P) the worker's P shard and its layouts: the worker's
// refreshes after the pull skip the shard (async_after_pull)
static bool async_p_now(const ddq_step_cfg* cfg, int64_t it) {
  return cfg->target_period > 0 && it % cfg->target_period == 0;
}

// draw: the launch also draws + gathers the worker's next minibatch (B <=
// 256; the caller ordered every ctx-stream op before it, and the worker's
// compute after it), as async_compute's draw launch would
static int async_owner_apply(ddq_ctx* c, const ddq_step_cfg* cfg, int64_t it, bool own,
                             bool draw = false) {
  const ddq_update_cfg& u = cfg->update;
  const int64_t L = c->comm.shard_len, off = (int64_t)c->comm.rank * L;
  // (the apply kernel indexes the gradient slice from the shard's start)
  const float* g = own ? c->nb.grad + off : c->comm.gsl;
  Prefetch pf{};
  if (draw) pf = make_prefetch(c->nb, c->replay.ring, cfg->seed);
  ShardOpts o;
  o.theta = c->async.own;
  o.first = c->applied == 0 ? 1 : 0;
  o.pre = draw ? &pf : nullptr;
  o.mirror = own ? c->nb.theta[0] : nullptr;
  o.refresh_own = own ? (async_p_now(cfg, it) ? 2 : 1) : 0;
  HIP_TRY(c, launch_apply_shard(c->nb, rule_of(u, 0), g, off, L, L, 1, c->comm.cs, o));
  if (async_p_now(cfg, it))
    HIP_TRY(c, hipMemcpyAsync(c->async.pown + off, c->async.own + off, L * 4, hipMemcpyDeviceToDevice, c->comm.cs));
  return DDQ_OK;
}

// Worker side after its pull (theta[0], and theta[1] when pull_p, hold the
// central model; the ctx stream waited for them): kernel layouts of Q (and
// P), then the next gradient.  own: the worker's own shard was refreshed by
// its owner apply (Q; P too when this tick updated the central P: p_own).
static int async_after_pull(ddq_ctx* c, const ddq_step_cfg* cfg, bool pull_p, bool own = false,
                            bool p_own = false, bool drawn = false) {
  const int64_t lo = own ? (int64_t)c->comm.rank * c->comm.shard_len : 0;
  const int64_t hi = own ? lo + c->comm.shard_len : 0;
  p_own = p_own && own;
  HIP_TRY(c, launch_refresh(c->nb, c->stream, 0, lo, hi));
  if (pull_p) {   // P's layouts from the pulled P weights
    NetBuffers pb = c->nb;
    pb.theta[0] = c->nb.theta[1]; pb.wks[0] = c->nb.wks[1];
    HIP_TRY(c, launch_refresh(pb, c->stream, 0, p_own ? lo : 0, p_own ? hi : 0));
  }
  return async_compute(c, cfg, drawn);
}

// Host bookkeeping of a tick (every rank / member: the same tick sequence).
static void async_advance(ddq_ctx* c, int w, int64_t it) {
  c->applied = it;
  c->async.last_pull[w] = it;
  c->async.async_ticks++;
}

// One tick over RCCL (worker w pushes): point-to-point pushes / pulls and the
// owner apply on the comm stream, the pulling worker's next gradient on its
// ctx stream -- it overlaps the later ticks' owner duties.
static int rccl_async_tick(ddq_ctx* c, const ddq_step_cfg* cfg, int w) {
  const int W = c->comm.nranks, r = c->comm.rank;
  const int64_t L = c->comm.shard_len;
  NetBuffers& nb = c->nb;
  const int64_t it = c->applied + 1;    // iteration after this tick's apply
  const bool pull_p = async_pull_p(cfg, c->async.last_pull[w], it);
  // the own push's owner apply draws + gathers this worker's next minibatch:
  // it follows everything on the ctx stream so far (the gradient, and any
  // replay insert enqueued since), not only grad_ev
  const bool draw = r == w && nb.B <= 256;
  if (draw) {
    HIP_TRY(c, hipEventRecord(c->comm.cev[0], c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->comm.cs, c->comm.cev[0], 0));
  } else if (r == w && (!c->async.acapture || c->async.grad_ev_captured)) {
    HIP_TRY(c, hipStreamWaitEvent(c->comm.cs, c->async.grad_ev, 0));
  }
  // push: worker w's gradient slices to their owners
  if (W > 1) {
    NCCL_TRY(c, ncclGroupStart());
    if (r == w) {
      for (int j = 0; j < W; ++j)
        if (j != r) NCCL_TRY(c, ncclSend(nb.grad + (size_t)j * L, L, ncclFloat, j, c->comm.comm, c->comm.cs));
    } else {
      NCCL_TRY(c, ncclRecv(c->comm.gsl, L, ncclFloat, w, c->comm.comm, c->comm.cs));
    }
    NCCL_TRY(c, ncclGroupEnd());
  }
  TRY(async_owner_apply(c, cfg, it, r == w, draw));
  // pull: the owners' shards to worker w
  if (W > 1) {
    NCCL_TRY(c, ncclGroupStart());
    if (r != w) {
      NCCL_TRY(c, ncclSend(c->async.own + (size_t)r * L, L, ncclFloat, w, c->comm.comm, c->comm.cs));
      if (pull_p) NCCL_TRY(c, ncclSend(c->async.pown + (size_t)r * L, L, ncclFloat, w, c->comm.comm, c->comm.cs));
    } else {
      for (int j = 0; j < W; ++j) {
        if (j == r) continue;
        NCCL_TRY(c, ncclRecv(nb.theta[0] + (size_t)j * L, L, ncclFloat, j, c->comm.comm, c->comm.cs));
        if (pull_p)
          NCCL_TRY(c, ncclRecv(nb.theta[1] + (size_t)j * L, L, ncclFloat, j, c->comm.comm, c->comm.cs));
      }
    }
    NCCL_TRY(c, ncclGroupEnd());
  }
  if (r == w) {   // (the own shard of theta[0]: written by the owner apply;
                  // of theta[1] too when this tick updated the central P)
    const bool p_own = async_p_now(cfg, it);
    if (pull_p && !p_own)
      HIP_TRY(c, hipMemcpyAsync(nb.theta[1] + (size_t)r * L, c->async.pown + (size_t)r * L, L * 4,
                                hipMemcpyDeviceToDevice, c->comm.cs));
    HIP_TRY(c, hipEventRecord(c->async.tick_ev, c->comm.cs));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->async.tick_ev, 0));
    TRY(async_after_pull(c, cfg, pull_p, true, p_own, draw));
  }
  async_advance(c, w, it);
  return DDQ_OK;
}

// the ctx stream waits for the comm stream's owner duties so far
static int async_join(ddq_ctx* c) {
  HIP_TRY(c, hipEventRecord(c->comm.cev[1], c->comm.cs));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->comm.cev[1], 0));
  return DDQ_OK;
}

int ddq::async_prepare(ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (c->comm.local) return fail(c, DDQ_ESTATE, "in-process group members step with ddq_group_step");
  if (!c->comm.cs) TRY(setup_shards(c, c->comm.nranks));
  if (!c->async.async_on) TRY(async_begin(c, cfg));
  return DDQ_OK;
}

// One round-robin round (W ticks, worker 0 .. W-1): a step of the async exchange.
static int rccl_async_round(ddq_ctx* c, const ddq_step_cfg* cfg) {
  for (int w = 0; w < c->comm.nranks; ++w) TRY(rccl_async_tick(c, cfg, w));
  return async_join(c);   // the step ends when this rank's owner duties are done
}

int ddq_async_begin(ddq_ctx* c, const ddq_step_cfg* cfg) {
  TRY(prio_refuse(c, "ddq_async_begin"));
  TRY(check_step(c, cfg));
  if (cfg->exchange != DDQ_EXCHANGE_ASYNC) return fail(c, DDQ_EINVAL, "cfg exchange is not async");
  if (cfg->update.rule == DDQ_RULE_ADAM)
    return fail(c, DDQ_EINVAL, "the async exchange does not take DDQ_RULE_ADAM");
  if (c->nb.target_tau < 1.f)
    return fail(c, DDQ_EINVAL, "soft target updates (tau %g < 1) with DDQ_EXCHANGE_ASYNC: its P "
                               "travels by pulls, not by the steps' syncs",
                (double)c->nb.target_tau);
  if (c->replay.aug_pad > 0)
    return fail(c, DDQ_EINVAL, "augmentation (pad %d) with DDQ_EXCHANGE_ASYNC: its workers' draws "
                               "ride on the owner applies", c->replay.aug_pad);
  if (c->mon.mon.ring && c->mon.mon_period > 0)
    return fail(c, DDQ_ESTATE, "the async exchange takes no monitor records: disable the monitor or "
                               "enable it with period 0");
  TRY(set_dev(c));
  return async_prepare(c, cfg);
}

// Is this worker's gradient pushable: computed (grad_ev), and -- for an
// emulated straggler -- straggle_us of host time since that was first seen.
static int grad_ready(ddq_ctx* c, bool* ready) {
  const hipError_t e = hipEventQuery(c->async.grad_ev);
  if (e != hipSuccess && e != hipErrorNotReady)
    return fail(c, DDQ_EHIP, "hipEventQuery: %s", hipGetErrorString(e));
  *ready = false;
  if (e != hipSuccess) return DDQ_OK;
  const auto now = std::chrono::steady_clock::now();
  if (!c->async.ready_seen) {
    c->async.ready_seen = true;
    c->async.ready_at = now;
  }
  *ready = now - c->async.ready_at >= std::chrono::microseconds(c->async.straggle_us);
  return DDQ_OK;
}

int ddq_async_ready(ddq_ctx* c, int32_t* ready) {
  if (!c || !ready) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->async.async_on) return fail(c, DDQ_ESTATE, "async exchange not begun (ddq_async_begin)");
  TRY(set_dev(c));
  bool r = false;
  TRY(grad_ready(c, &r));
  *ready = r ? 1 : 0;
  return DDQ_OK;
}

static int after_async_graph(ddq_ctx* c);

// This rank's own tick (worker == rank) as a graph.  Its launches depend on
// the host state only through whether this tick pulls P and whether its
// iteration is a special update (and the first apply of all: eager), so two
// bits pick the graph; the capture leaves the host bookkeeping as it was.
static int ensure_tick_graph(ddq_ctx* c, const ddq_step_cfg* cfg, int key) {
  auto& t = c->graphs.tick;
  if (!t.holds(cfg)) {
    t.reset();
    t.key(cfg);
  }
  if (t.exec[key]) return DDQ_OK;
  return capture_exec(c, &t.exec[key], [&] { return rccl_async_tick(c, cfg, c->comm.rank); },
                      "tick graph");
}

int ddq_async_tick(ddq_ctx* c, const ddq_step_cfg* cfg, int32_t worker) {
  TRY(check_step(c, cfg));
  if (cfg->exchange != DDQ_EXCHANGE_ASYNC) return fail(c, DDQ_EINVAL, "cfg exchange is not async");
  if (worker < 0 || worker >= c->comm.nranks)
    return fail(c, DDQ_EINVAL, "worker %d out of [0, %d)", worker, c->comm.nranks);
  TRY(set_dev(c));
  TRY(async_prepare(c, cfg));
  c->async.rr_rounds = 0;   // the round-robin graph's steady state no longer holds
  // this rank's own ticks (the heavy ones: its next gradient) replay a graph;
  // the other workers' ticks (a receive, the owner apply, a send) stay eager
  if (worker == c->comm.rank && c->applied > 0) {
    const int64_t it = c->applied + 1;
    const bool pull_p = async_pull_p(cfg, c->async.last_pull[worker], it);
    const bool special = cfg->target_period > 0 && it % cfg->target_period == 0;
    const int key = (pull_p ? 2 : 0) | (special ? 1 : 0);
    TRY(ensure_tick_graph(c, cfg, key));
    HIP_TRY(c, hipGraphLaunch(c->graphs.tick.exec[key], c->stream));
    TRY(after_async_graph(c));
    async_advance(c, worker, it);
    return DDQ_OK;
  }
  return rccl_async_tick(c, cfg, worker);
}

// ---- round-robin rounds as hipGraphs ----
// A round's launches depend on the host state only through the iteration's
// residue mod the special-update period (which ticks pull P, which owners
// copy Q -> P) and the workers' last pulls, which after one whole round-robin
// round are one round back for everyone.  So K = period / gcd(W, period)
// rounds (K W iterations, a multiple of the period) form a graph that is
// valid whenever a round starts at the residue it was captured at; the host
// bookkeeping of a replay is the captured ticks' (async_advance).  Rounds
// before that alignment (and the remainder of a call) run eagerly.
static constexpr int kAsyncGraphMaxRounds = 16;

static int async_graph_rounds(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (cfg->target_period <= 0) return 1;
  int a = c->comm.nranks, b = cfg->target_period;
  while (b) { const int t = a % b; a = b; b = t; }
  return cfg->target_period / a;
}

static int64_t async_phase(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  return cfg->target_period > 0 ? c->applied % cfg->target_period : 0;
}

int ddq::async_round_eager(ddq_ctx* c, const ddq_step_cfg* cfg) {
  TRY(rccl_async_round(c, cfg));
  c->steps++;
  c->async.rr_rounds++;
  return DDQ_OK;
}

static int ensure_async_graph(ddq_ctx* c, const ddq_step_cfg* cfg, int K) {
  auto& r = c->graphs.round;
  if (r.holds(cfg)) return DDQ_OK;
  r.reset();
  TRY(capture_exec(c, &r.exec[0], [&]() -> int {
    for (int k = 0; k < K; ++k) TRY(rccl_async_round(c, cfg));
    return DDQ_OK;
  }, "async graph"));
  r.key(cfg);
  r.phase = async_phase(c, cfg);
  return DDQ_OK;
}

// After a replay of the round-robin graph: the graph's comm-stream work is a
// branch of the launch, so the comm stream itself is not ordered behind it --
// make it wait for the launch (the eager ticks / rounds that follow queue
// RCCL calls, owner applies and gsl copies on it).  A graph replay re-records
// no event either: grad_ev still marks the gradient from before the capture,
// so record it again behind the launch (whose last round computed nb.grad),
// and forget an earlier readiness observation.
static int after_async_graph(ddq_ctx* c) {
  HIP_TRY(c, hipEventRecord(c->comm.cev[0], c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->comm.cs, c->comm.cev[0], 0));
  HIP_TRY(c, hipEventRecord(c->async.grad_ev, c->stream));
  c->async.ready_seen = false;
  c->async.grad_ev_captured = false;
  return DDQ_OK;
}

int ddq::async_graph_steps(ddq_ctx* c, const ddq_step_cfg* cfg, int nsteps) {
  TRY(async_prepare(c, cfg));
  const int K = async_graph_rounds(c, cfg);
  int i = 0;
  if (K > kAsyncGraphMaxRounds) {
    for (; i < nsteps; ++i) TRY(async_round_eager(c, cfg));
    return DDQ_OK;
  }
  while (i < nsteps) {
    const bool steady = c->async.rr_rounds >= 1;
    if (steady && nsteps - i >= K &&
        (!c->graphs.round.holds(cfg) || async_phase(c, cfg) == c->graphs.round.phase)) {
      TRY(ensure_async_graph(c, cfg, K));
      HIP_TRY(c, hipGraphLaunch(c->graphs.round.exec[0], c->stream));
      TRY(after_async_graph(c));
      for (int k = 0; k < K; ++k)
        for (int w = 0; w < c->comm.nranks; ++w) async_advance(c, w, c->applied + 1);
      c->steps += K;
      c->async.rr_rounds += K;
      i += K;
      continue;
    }
    TRY(async_round_eager(c, cfg));
    ++i;
  }
  return DDQ_OK;
}

int ddq_set_straggle(ddq_ctx* c, int64_t usec) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (usec < 0 || usec > 1000000) return fail(c, DDQ_EINVAL, "usec must be in [0, 1e6]");
  c->async.straggle_us = usec;
  return DDQ_OK;
}

// ---------------- in-process groups ----------------
int ddq_group_init(ddq_ctx** ctxs, int32_t W) {
  if (!ctxs || W < 1 || W > kMaxRanks) return fail(nullptr, DDQ_EINVAL, "bad group");
  for (int r = 0; r < W; ++r) {
    ddq_ctx* c = ctxs[r];
    if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx in group");
    if (c->comm.comm) return fail(c, DDQ_ESTATE, "ctx already has an RCCL communicator");
    TRY(prio_refuse(c, "ddq_group_init"));
    if (c->nb.S != ctxs[0]->nb.S || c->nb.B != ctxs[0]->nb.B)
      return fail(c, DDQ_EINVAL, "group members must share batch and frame");
  }
  for (int r = 0; r < W; ++r) {
    ddq_ctx* c = ctxs[r];
    TRY(set_dev(c));
    c->comm.local = true;
    c->comm.nranks = W;
    c->comm.rank = r;
    TRY(setup_shards(c, W));
    if (!c->comm.gstage) TRY(dalloc(c, &c->comm.gstage, (size_t)W * (c->nb.L.total + kShardPad)));
    invalidate_graph(c);
  }
  return DDQ_OK;
}

// In-process group ticks: rccl_async_tick with the point-to-point transfers
// as device copies, ordered by events only (no host synchronisation): owner r
// copies worker w's slice into its gsl on its comm stream once w's gradient is
// ready, applies it, and copies its shard (and P's) into w's replica -- the
// sender side of the pull, so its next apply cannot overtake the copy -- then
// marks the tick; worker w's ctx stream waits for every owner's mark, and
// recomputes.
static int group_async_tick(ddq_ctx** ctxs, int W, const ddq_step_cfg* cfg, int w) {
  ddq_ctx* cw = ctxs[w];
  const int64_t L = ctxs[0]->comm.shard_len;
  const int64_t it = ctxs[0]->applied + 1;
  const bool pull_p = async_pull_p(cfg, ctxs[0]->async.last_pull[w], it);
  for (int r = 0; r < W; ++r) {
    ddq_ctx* c = ctxs[r];
    TRY(set_dev(c));
    HIP_TRY(c, hipStreamWaitEvent(c->comm.cs, cw->async.grad_ev, 0));
    HIP_TRY(c, hipMemcpyAsync(c->comm.gsl, cw->nb.grad + (size_t)r * L, L * 4,
                              hipMemcpyDeviceToDevice, c->comm.cs));
    TRY(async_owner_apply(c, cfg, it, false));
    HIP_TRY(c, hipMemcpyAsync(cw->nb.theta[0] + (size_t)r * L, c->async.own + (size_t)r * L, L * 4,
                              hipMemcpyDeviceToDevice, c->comm.cs));
    if (pull_p)
      HIP_TRY(c, hipMemcpyAsync(cw->nb.theta[1] + (size_t)r * L, c->async.pown + (size_t)r * L, L * 4,
                                hipMemcpyDeviceToDevice, c->comm.cs));
    HIP_TRY(c, hipEventRecord(c->async.tick_ev, c->comm.cs));
  }
  TRY(set_dev(cw));
  for (int r = 0; r < W; ++r) HIP_TRY(cw, hipStreamWaitEvent(cw->stream, ctxs[r]->async.tick_ev, 0));
  TRY(async_after_pull(cw, cfg, pull_p));
  for (int r = 0; r < W; ++r) async_advance(ctxs[r], w, it);
  return DDQ_OK;
}

static int group_async_prepare(ddq_ctx** ctxs, int W, const ddq_step_cfg* cfg) {
  for (int r = 0; r < W; ++r) {
    if (ctxs[r]->async.async_on) continue;
    TRY(set_dev(ctxs[r]));
    TRY(async_begin(ctxs[r], cfg));
  }
  return DDQ_OK;
}

static int group_sync_all(ddq_ctx** ctxs, int W) {
  for (int r = 0; r < W; ++r) {
    ddq_ctx* c = ctxs[r];
    TRY(set_dev(c));
    HIP_TRY(c, hipStreamSynchronize(c->comm.cs));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return DDQ_OK;
}

// One round-robin round of an in-process group (synchronised at its end).
static int group_async_round(ddq_ctx** ctxs, int W, const ddq_step_cfg* cfg) {
  TRY(group_async_prepare(ctxs, W, cfg));
  for (int w = 0; w < W; ++w) TRY(group_async_tick(ctxs, W, cfg, w));
  TRY(group_sync_all(ctxs, W));
  for (int r = 0; r < W; ++r) ctxs[r]->steps++;
  return DDQ_OK;
}

static int check_group(ddq_ctx** ctxs, int W, const ddq_step_cfg* cfg) {
  if (!ctxs || !cfg || W < 1) return fail(nullptr, DDQ_EINVAL, "bad argument");
  for (int r = 0; r < W; ++r) {
    ddq_ctx* c = ctxs[r];
    TRY(prio_refuse(c, "a group step or tick"));
    if (!c || !c->comm.local || c->comm.nranks != W || c->comm.rank != r)
      return fail(c, DDQ_ESTATE, "ctx %d is not rank %d of a %d-member group", r, r, W);
    TRY(check_step(c, cfg));
  }
  return DDQ_OK;
}

// Ticks in a given worker order (deterministic: the order of a ticket run, or
// any test schedule), synchronised at the end.
int ddq_group_async_ticks(ddq_ctx** ctxs, int32_t W, const ddq_step_cfg* cfg, int32_t n,
                          const int32_t* order) {
  TRY(check_group(ctxs, W, cfg));
  if (cfg->exchange != DDQ_EXCHANGE_ASYNC) return fail(ctxs[0], DDQ_EINVAL, "cfg exchange is not async");
  if (n < 0 || (n > 0 && !order)) return fail(ctxs[0], DDQ_EINVAL, "bad tick order");
  for (int t = 0; t < n; ++t)
    if (order[t] < 0 || order[t] >= W)
      return fail(ctxs[0], DDQ_EINVAL, "tick %d: worker %d out of [0, %d)", t, order[t], W);
  TRY(group_async_prepare(ctxs, W, cfg));
  for (int t = 0; t < n; ++t) TRY(group_async_tick(ctxs, W, cfg, order[t]));
  return group_sync_all(ctxs, W);
}

// Ticket order (arrival order) for an in-process group: the host polls the
// members' gradient-ready events and gives the next ticket to the first
// member found ready (the scan starts after the last ticket's holder), then
// enqueues that tick.  Nothing waits on the device for a ticket: the order is
// decided on the host, as the reference's single server decides it by the
// order its HTTP handler takes modelLock (server.py:196-209).
int ddq_group_async_run(ddq_ctx** ctxs, int32_t W, const ddq_step_cfg* cfg, int32_t npush,
                        int32_t* order) {
  TRY(check_group(ctxs, W, cfg));
  if (cfg->exchange != DDQ_EXCHANGE_ASYNC) return fail(ctxs[0], DDQ_EINVAL, "cfg exchange is not async");
  if (npush < 0) return fail(ctxs[0], DDQ_EINVAL, "npush must be >= 0");
  TRY(group_async_prepare(ctxs, W, cfg));
  int start = 0;
  for (int t = 0; t < npush; ++t) {
    int pick = -1;
    for (int64_t spin = 0; pick < 0; ++spin) {
      for (int k = 0; k < W && pick < 0; ++k) {
        const int w = (start + k) % W;
        TRY(set_dev(ctxs[w]));
        bool r = false;
        TRY(grad_ready(ctxs[w], &r));
        if (r) pick = w;
      }
      if (pick < 0) {
        if (spin > 2000000)   // ~minutes without any gradient finishing: a stall
          return fail(ctxs[0], DDQ_EHIP, "async run: no gradient became ready");
        std::this_thread::sleep_for(std::chrono::microseconds(20));
      }
    }
    if (order) order[t] = pick;
    TRY(group_async_tick(ctxs, W, cfg, pick));
    start = (pick + 1) % W;
  }
  return group_sync_all(ctxs, W);
}

// One synchronous data-parallel step of an in-process group: the same
// kernels and exchange semantics as RCCL ranks, with the collectives done as
// device copies between the members' buffers, phase by phase.
int ddq_group_step(ddq_ctx** ctxs, int32_t W, const ddq_step_cfg* cfg) {
  TRY(check_group(ctxs, W, cfg));
  const int ex = cfg->exchange;
  if (ex == DDQ_EXCHANGE_ASYNC) return group_async_round(ctxs, W, cfg);
  for (int r = 0; r < W; ++r) TRY(check_not_async(ctxs[r]));
  const int64_t P = ctxs[0]->nb.L.total;
  std::vector<hipEvent_t> ev(W);
  std::vector<StepLaunch> sl(W);
  auto record_all = [&](void) -> int {
    for (int r = 0; r < W; ++r) {
      ddq_ctx* c = ctxs[r];
      TRY(set_dev(c));
      if (ev[r] == nullptr) HIP_TRY(c, hipEventCreateWithFlags(&ev[r], hipEventDisableTiming));
      HIP_TRY(c, hipEventRecord(ev[r], c->stream));
    }
    return DDQ_OK;
  };
  auto wait_all = [&](ddq_ctx* c) -> int {
    for (int j = 0; j < W; ++j) HIP_TRY(c, hipStreamWaitEvent(c->stream, ev[j], 0));
    return DDQ_OK;
  };
  int rc = [&]() -> int {
    // phase 1: sample + gather + forward/backward (+ bookkeeping) per member
    for (int r = 0; r < W; ++r) {
      ddq_ctx* c = ctxs[r];
      TRY(set_dev(c));
      if (c->steps == 0) TRY(initial_target_sync(c, cfg));
      StepFacts f = step_facts(c, cfg);
      f.fused_apply_ok = false;   // (the apply is phase 2, after the members' exchange)
      TRY(plan_launches(c, cfg, f, &sl[r]));
      TRY(enqueue_draw(c, c->nb, cfg->seed, c->stream));
      TRY(enqueue_fwd_bwd(c, c->nb, sl[r]));
    }
    TRY(record_all());
    // phase 2: exchange + (owner) apply
    for (int r = 0; r < W; ++r) {
      ddq_ctx* c = ctxs[r];
      TRY(set_dev(c));
      TRY(wait_all(c));
      const NetBuffers& nb = c->nb;
      const int64_t len = c->comm.shard_len;
      if (ex == DDQ_EXCHANGE_NONE) {
        TRY(enqueue_apply(c, nb, sl[r]));
        continue;
      }
      if (ex == DDQ_EXCHANGE_ALLREDUCE) {   // gather every gradient first (summed below)
        for (int j = 0; j < W; ++j)
          HIP_TRY(c, hipMemcpyAsync(c->comm.gstage + (size_t)j * P, ctxs[j]->nb.grad, P * 4,
                                    hipMemcpyDeviceToDevice, c->stream));
        continue;
      }
      for (int j = 0; j < W; ++j)
        HIP_TRY(c, hipMemcpyAsync(c->comm.gsl + (size_t)j * len, ctxs[j]->nb.grad + (size_t)r * len,
                                  len * 4, hipMemcpyDeviceToDevice, c->stream));
      int nsl = W;
      if (ex == DDQ_EXCHANGE_SHARDED) {
        HIP_TRY(c, launch_sum_slices(c->comm.gsl, c->comm.gsl, W, len, len, c->stream));
        nsl = 1;
      }
      HIP_TRY(c, launch_apply_shard(nb, sl[r].u, c->comm.gsl, (int64_t)r * len, len, len, nsl, c->stream));
    }
    if (ex == DDQ_EXCHANGE_ALLREDUCE) {
      TRY(record_all());       // every member holds all W gradients: sum in rank order, apply
      for (int r = 0; r < W; ++r) {
        ddq_ctx* c = ctxs[r];
        TRY(set_dev(c));
        TRY(wait_all(c));
        HIP_TRY(c, launch_sum_slices(c->nb.grad, c->comm.gstage, W, P, P, c->stream));
        TRY(enqueue_apply(c, c->nb, sl[r]));
      }
    }
    if (ex == DDQ_EXCHANGE_SHARDED || ex == DDQ_EXCHANGE_SERVER) {
      TRY(record_all());
      // phase 3: all-gather of the owners' shards + refresh
      for (int r = 0; r < W; ++r) {
        ddq_ctx* c = ctxs[r];
        TRY(set_dev(c));
        TRY(wait_all(c));
        const int64_t len = c->comm.shard_len;
        for (int j = 0; j < W; ++j)
          if (j != r)
            HIP_TRY(c, hipMemcpyAsync(c->nb.theta[0] + (size_t)j * len,
                                      ctxs[j]->nb.theta[0] + (size_t)j * len, len * 4,
                                      hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, launch_refresh(c->nb, c->stream));
      }
    }
    for (int r = 0; r < W; ++r) {
      ddq_ctx* c = ctxs[r];
      TRY(set_dev(c));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      count_steps(c, cfg, 1);
    }
    return DDQ_OK;
  }();
  for (auto& e : ev)
    if (e) hipEventDestroy(e);
  return rc;
}
