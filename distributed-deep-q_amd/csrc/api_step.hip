// libddq_hip C-ABI: what a step is and its plan, exchange plus apply, the
// draw, the train body; the eager, graph and pipelined step modes; graph
// capture.
#include "step.h"

using namespace ddq;
// (the ddq_* definitions take their C linkage from include/ddq_hip.h)

// ---------------- step ----------------
static bool has_exchange(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  return cfg->exchange != DDQ_EXCHANGE_NONE && (c->comm.comm != nullptr || c->comm.local);
}
// param-server iterations one step consumes (server.py:200 INCR per gradient)
static int step_inc(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  return (has_exchange(c, cfg) &&
          (cfg->exchange == DDQ_EXCHANGE_SERVER || cfg->exchange == DDQ_EXCHANGE_ASYNC))
             ? c->comm.nranks
             : 1;
}
// host mirrors of the device counters after n more steps
void ddq::count_steps(ddq_ctx* c, const ddq_step_cfg* cfg, int n) {
  c->steps += n;
  c->applied += (int64_t)n * step_inc(c, cfg);
}
// the target period as the apply bookkeeping takes it (0: no P <- Q sync)
static int book_period(const ddq_step_cfg* cfg) {
  return cfg->target_period > 0 ? cfg->target_period : 0;
}
bool ddq::is_async(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  return has_exchange(c, cfg) && cfg->exchange == DDQ_EXCHANGE_ASYNC;
}
// Once the async exchange began, the central model lives in the owners'
// shards: other step kinds would train a replica the owners never see.
int ddq::check_not_async(ddq_ctx* c) {
  if (c->async.async_on)
    return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx (its central "
                               "model lives in the owners' shards): async steps only");
  return DDQ_OK;
}

// Overlapped all-reduce, part 1 (called by launch_backward right after the
// fc4 weight-gradient kernel): the comm stream sums the fc4 weight bucket
// (2.1 M of the 2.2 M parameters at 64x64) while the conv backward runs;
// cev[2] marks it done (the fused apply's slab-reduce launch waits for it).
static hipError_t fc4_bucket_start(void* arg) {
  ddq_ctx* c = reinterpret_cast<ddq_ctx*>(arg);
  const ParamLayout& L = c->nb.L;
  hipError_t e = hipEventRecord(c->comm.cev[0], c->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(c->comm.cs, c->comm.cev[0], 0);
  if (e != hipSuccess) return e;
  ncclResult_t r = ncclAllReduce(c->nb.grad + L.w[3], c->nb.grad + L.w[3], (size_t)L.wn[3],
                                 ncclFloat, ncclSum, c->comm.comm, c->comm.cs);
  if (r != ncclSuccess) {
    c->comm.comm_err = ncclGetErrorString(r);
    return hipErrorUnknown;
  }
  return hipEventRecord(c->comm.cev[2], c->comm.cs);
}

// What a step of (ctx, cfg) is, for plan_step.
StepFacts ddq::step_facts(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  StepFacts f;
  const int ex = has_exchange(c, cfg) ? cfg->exchange : DDQ_EXCHANGE_NONE;
  f.small = c->nb.small;
  f.b_le_256 = c->nb.B <= 256;
  f.prio = c->nb.prio.leaf != nullptr;
  f.adam = cfg->update.rule == DDQ_RULE_ADAM;
  // (an Adam step's all-reduce is one call on the ctx stream: cfg->overlap is
  // for the fused fc4 apply, which Adam does not take)
  f.ex = ex == DDQ_EXCHANGE_ALLREDUCE
             ? (cfg->overlap && c->comm.comm && !f.adam ? Exchange::AllReduceOverlap : Exchange::AllReduce)
         : ex == DDQ_EXCHANGE_SHARDED ? Exchange::Sharded
         : ex == DDQ_EXCHANGE_SERVER  ? Exchange::Server
         : ex == DDQ_EXCHANGE_ASYNC   ? Exchange::AsyncWorker
                                      : Exchange::None;
  f.fused_apply_ok = fused_apply_ok(c->nb.L);
  f.no_grad_store = (cfg->flags & DDQ_STEP_NO_GRAD_STORE) != 0;
  // (only the two-launch draw moved the counter on itself: enqueue_draw)
  f.augment = c->replay.aug_pad > 0;
  f.holds_counter = c->prio.prio_on || (c->nb.B <= 256 && !f.augment);
  // (the owners keep the async exchange's iteration)
  const bool worker = f.ex == Exchange::AsyncWorker;
  f.book_period = worker ? -1 : book_period(cfg);
  f.book_step = worker ? 1 : step_inc(c, cfg);
  return f;
}

// The plan of a step with these facts and what its launches need of the ctx.
int ddq::plan_launches(ddq_ctx* c, const ddq_step_cfg* cfg, const StepFacts& f, StepLaunch* sl) {
  const char* why = "";
  if (!plan_step(f, &sl->plan, &why)) return fail(c, DDQ_ESTATE, "internal: %s", why);
  sl->u = rule_of(cfg->update, cfg->target_period);
  sl->meta = c->replay.ring.meta;
  sl->fc4_wait = sl->plan.ext() ? c->comm.cev[2] : nullptr;
  return DDQ_OK;
}

// Gradient exchange + apply of one step over RCCL (graph-capturable):
//  ALLREDUCE  sum all-reduce, replicated apply (overlap: fc4 bucket on the
//             comm stream under the conv backward, applied by the slab-reduce
//             launch (StepPlan::ext); the rest -- conv layers, fc4 bias, Q_out --
//             as one grouped call after the slab reduce, then their apply);
//  SHARDED    reduce-scatter(sum) -> owner apply of its 1/W shard ->
//             in-place all-gather of theta -> conv layouts / P <- Q refresh;
//  SERVER     all-to-all of gradient slices -> owner applies the W gradients
//             one by one in rank order (server.py:196-209 on arrival) ->
//             all-gather -> refresh.
static int enqueue_exchange_apply(ddq_ctx* c, const ddq_step_cfg* cfg, const NetBuffers& nb,
                                  const StepLaunch& sl, Marks m, bool overlap) {
  const ParamLayout& L = nb.L;
  const int ex = has_exchange(c, cfg) ? cfg->exchange : DDQ_EXCHANGE_NONE;
  if (ex == DDQ_EXCHANGE_NONE || ex == DDQ_EXCHANGE_ALLREDUCE) {
    if (ex == DDQ_EXCHANGE_ALLREDUCE) {
      m("allreduce");
      if (sl.plan.ext()) {
        // fc4's weights were summed under the conv backward and applied by
        // the slab-reduce launch, whose stream waited for that
        // all-reduce: the rest (4 % of the parameters) right here on the ctx
        // stream -- nothing is left to overlap it with, and a comm-stream
        // round trip costs a graph fork / join (measured 0.968 against 0.995
        // of the exchange-free step at world 1 with it)
        NCCL_TRY(c, ncclGroupStart());
        NCCL_TRY(c, ncclAllReduce(nb.grad, nb.grad, (size_t)L.w[3], ncclFloat, ncclSum, c->comm.comm,
                                  c->stream));
        NCCL_TRY(c, ncclAllReduce(nb.grad + L.b[3], nb.grad + L.b[3], (size_t)(L.total - L.b[3]),
                                  ncclFloat, ncclSum, c->comm.comm, c->stream));
        NCCL_TRY(c, ncclGroupEnd());
      } else if (overlap) {
        HIP_TRY(c, hipEventRecord(c->comm.cev[0], c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->comm.cs, c->comm.cev[0], 0));
        NCCL_TRY(c, ncclGroupStart());
        NCCL_TRY(c, ncclAllReduce(nb.grad, nb.grad, (size_t)L.w[3], ncclFloat, ncclSum, c->comm.comm,
                                  c->comm.cs));
        NCCL_TRY(c, ncclAllReduce(nb.grad + L.b[3], nb.grad + L.b[3], (size_t)(L.total - L.b[3]),
                                  ncclFloat, ncclSum, c->comm.comm, c->comm.cs));
        NCCL_TRY(c, ncclGroupEnd());
        HIP_TRY(c, hipEventRecord(c->comm.cev[1], c->comm.cs));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->comm.cev[1], 0));
      } else {
        NCCL_TRY(c, ncclAllReduce(nb.grad, nb.grad, (size_t)L.total, ncclFloat, ncclSum, c->comm.comm,
                                  c->stream));
      }
    }
    return enqueue_apply(c, nb, sl, m);
  }
  const int W = c->comm.nranks;
  const size_t len = (size_t)c->comm.shard_len;
  m(ex == DDQ_EXCHANGE_SHARDED ? "reduce_scatter" : "all_to_all");
  if (ex == DDQ_EXCHANGE_SHARDED)
    NCCL_TRY(c, ncclReduceScatter(nb.grad, c->comm.gsl, len, ncclFloat, ncclSum, c->comm.comm, c->stream));
  else if (W > 1) {
    // all-to-all without the rank's own slice: the owner apply reads that one
    // in place from nb.grad (no self copy of len floats through RCCL)
    NCCL_TRY(c, ncclGroupStart());
    for (int p = 0; p < W; ++p) {
      if (p == c->comm.rank) continue;
      NCCL_TRY(c, ncclSend(nb.grad + (size_t)p * len, len, ncclFloat, p, c->comm.comm, c->stream));
      NCCL_TRY(c, ncclRecv(c->comm.gsl + (size_t)p * len, len, ncclFloat, p, c->comm.comm, c->stream));
    }
    NCCL_TRY(c, ncclGroupEnd());
  }
  m("apply_shard");
  ShardOpts o;
  if (sl.plan.gather == Site::OwnerApply) o.pre = sl.next;
  o.refresh_own = -1;
  o.own_w = c->comm.rank;
  o.own_g = ex == DDQ_EXCHANGE_SHARDED ? nullptr : nb.grad + (size_t)c->comm.rank * len;
  HIP_TRY(c, launch_apply_shard(nb, sl.u, c->comm.gsl, (int64_t)c->comm.rank * len, (int64_t)len,
                                (int64_t)len, ex == DDQ_EXCHANGE_SHARDED ? 1 : W, c->stream, o));
  m("all_gather");
  NCCL_TRY(c, ncclAllGather(nb.theta[0] + (size_t)c->comm.rank * len, nb.theta[0], len, ncclFloat,
                            c->comm.comm, c->stream));
  // the owner's shard was refreshed by its apply: the other ranks' shards
  // only (no launch when one rank owns every parameter)
  m("refresh");
  HIP_TRY(c, launch_refresh(nb, c->stream, -1, (int64_t)c->comm.rank * len,
                            (int64_t)(c->comm.rank + 1) * len));
  return DDQ_OK;
}

// The draw of a minibatch and its gather into nb's set, on `stream`.
int ddq::enqueue_draw(ddq_ctx* c, const NetBuffers& nb, uint64_t seed, hipStream_t stream,
                      Marks m) {
  if (c->replay.aug_pad > 0) {   // the draw, then the shifting gather: never fused (gather_shift.h)
    m(c->prio.prio_on ? "prio_sample" : "sample");
    if (c->prio.prio_on)       // (leaves the counter to the step's commit: back = 0)
      HIP_TRY(c, launch_prio_sample(nb, c->replay.ring.meta, seed, stream));
    else
      HIP_TRY(c, launch_sample(nb, c->replay.ring.meta, seed, stream));
    m("gather_shift");
    HIP_TRY(c, launch_gather_shift(nb, c->replay.ring, seed, c->replay.aug_pad, c->prio.prio_on ? 0 : 1, stream));
  } else if (c->prio.prio_on) {   // one workgroup descends the sum tree, then the plain gather
    m("prio_sample");
    HIP_TRY(c, launch_prio_sample(nb, c->replay.ring.meta, seed, stream));
    m("gather");
    HIP_TRY(c, launch_gather(nb, c->replay.ring, stream));
  } else if (nb.B <= 256) {   // one kernel: every gather workgroup draws the same index set
    m("sample_gather");
    HIP_TRY(c, launch_sample_gather(nb, c->replay.ring, seed, stream));
  } else {
    m("sample");
    HIP_TRY(c, launch_sample(nb, c->replay.ring.meta, seed, stream));
    m("gather");
    HIP_TRY(c, launch_gather(nb, c->replay.ring, stream));
  }
  return DDQ_OK;
}

// Pipelined steps whose next draw + gather ride on launches of the step (no
// side stream): every exchange but the async one, B <= 256 (StepPlan::gather).
static bool fused_prefetch(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  return !is_async(c, cfg) && c->nb.B <= 256;
}

// fwd/bwd -> exchange -> apply on the minibatch held by `nb`, as the step's
// plan has it; when `pre` is given, the NEXT step's sample + gather into
// `pre`'s minibatch set run beside this step (the replay ring is not written
// inside a step, and the device RNG counter moves on in the same order, so
// the index stream equals the sequential one).
// fault: ddq_inject_fault's meeting timeout, for this step's launches only
static int enqueue_train_body(ddq_ctx* c, const ddq_step_cfg* cfg, const NetBuffers& nb,
                              const NetBuffers* pre, Marks m, bool fault) {
  StepFacts f = step_facts(c, cfg);
  f.prefetch = pre != nullptr;
  f.fault_k2_short = fault;
  StepLaunch sl;
  TRY(plan_launches(c, cfg, f, &sl));
  const bool side = sl.plan.draw == Site::Side, overlap = f.ex == Exchange::AllReduceOverlap;
  Prefetch pf;
  if (on_ctx_stream(sl.plan.gather)) {
    pf = make_prefetch(*pre, c->replay.ring, cfg->seed);
    pf.predrawn = sl.plan.predrawn();
    sl.next = &pf;
  }
  if (side) {
    HIP_TRY(c, hipEventRecord(nb.ev[6], c->stream));
    HIP_TRY(c, hipStreamWaitEvent(nb.side, nb.ev[6], 0));
    TRY(enqueue_draw(c, *pre, cfg->seed, nb.side));
    HIP_TRY(c, hipEventRecord(nb.ev[7], nb.side));
  }
  const Fc4Done fc4_done = overlap ? Fc4Done{fc4_bucket_start, c} : Fc4Done{};
  TRY(enqueue_fwd_bwd(c, nb, sl, m, fc4_done, pre, cfg->seed));
  TRY(enqueue_exchange_apply(c, cfg, nb, sl, m, overlap));
  if (side) HIP_TRY(c, hipStreamWaitEvent(c->stream, nb.ev[7], 0));
  return DDQ_OK;
}

// The step, then (ddq_monitor_enable with period > 0) the monitor as its last
// launch: loss_t, g_t and the parameters after update t; the kernel itself
// tests the device iteration against the period, so the launch is the same
// every step and replays from a captured graph.
static int enqueue_train(ddq_ctx* c, const ddq_step_cfg* cfg, const NetBuffers& nb,
                         const NetBuffers* pre, Marks m, bool fault = false) {
  TRY(enqueue_train_body(c, cfg, nb, pre, m, fault));
  if (c->mon.mon.ring && c->mon.mon_period > 0) {
    m("monitor");
    HIP_TRY(c, launch_monitor(c->mon.mon, c->mon.mon_period, -1, c->stream));
  }
  return DDQ_OK;
}

int ddq::enqueue_step(ddq_ctx* c, const ddq_step_cfg* cfg, Marks m, bool fault) {
  TRY(enqueue_draw(c, c->nb, cfg->seed, c->stream, m));
  return enqueue_train(c, cfg, c->nb, nullptr, m, fault);
}

// the ctx's buffers with minibatch set p (0 = its own, 1 = the pipelining twin)
static NetBuffers mb_view(const ddq_ctx* c, int p) {
  NetBuffers v = c->nb;
  v.mb = c->mb[p];
  return v;
}

// The pull at iteration 0 copies Q -> P (server.py:188-189, 0 % period == 0);
// later syncs are fused into the apply kernel of the preceding update.
int ddq::initial_target_sync(ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (cfg->target_period > 0 && c->applied % cfg->target_period == 0) {
    HIP_TRY(c, hipMemcpyAsync(c->nb.theta[1], c->nb.theta[0], c->nb.L.total * 4,
                              hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->nb.wks[1], c->nb.wks[0], c->nb.L.wks_total * 3 * 2,
                              hipMemcpyDeviceToDevice, c->stream));
  }
  return DDQ_OK;
}

int ddq::check_step(ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!cfg) return fail(c, DDQ_EINVAL, "null step cfg");
  TRY(not_restoring(c));   // (every step kind, the group's and the async ones)
  TRY(check_cfg(c, &cfg->update));
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (too_few_slots(c, c->nb.B))
    return fail(c, DDQ_EINVAL, "Can't draw sample of size %d from replay dataset of size %lld",
                c->nb.B, (long long)(c->replay.lanes * c->replay.valid));
  if (cfg->exchange < DDQ_EXCHANGE_NONE || cfg->exchange > DDQ_EXCHANGE_ASYNC)
    return fail(c, DDQ_EINVAL, "unknown exchange %d", cfg->exchange);
  if (cfg->flags & ~DDQ_STEP_NO_GRAD_STORE)
    return fail(c, DDQ_EINVAL, "unknown step flags 0x%x", (unsigned)cfg->flags);
  if (cfg->exchange != DDQ_EXCHANGE_NONE && c->comm.nranks > 1 && !c->comm.comm && !c->comm.local)
    return fail(c, DDQ_ESTATE, "no communicator");
  if (has_exchange(c, cfg)) TRY(prio_refuse(c, "an exchanged step"));
  if (cfg->update.rule == DDQ_RULE_ADAM && has_exchange(c, cfg) &&
      cfg->exchange != DDQ_EXCHANGE_ALLREDUCE)
    return fail(c, DDQ_EINVAL, "DDQ_RULE_ADAM runs without an exchange or under "
                               "DDQ_EXCHANGE_ALLREDUCE only (exchange %d shards one state buffer)",
                cfg->exchange);
  if (c->replay.aug_pad > 0 && is_async(c, cfg))
    return fail(c, DDQ_EINVAL, "augmentation (pad %d) with DDQ_EXCHANGE_ASYNC: its workers' draws "
                               "ride on the owner applies", c->replay.aug_pad);
  if (c->nb.target_tau < 1.f && is_async(c, cfg))
    return fail(c, DDQ_EINVAL, "soft target updates (tau %g < 1) with DDQ_EXCHANGE_ASYNC: its P "
                               "travels by pulls, not by the steps' syncs",
                (double)c->nb.target_tau);
  return DDQ_OK;
}

// Single-ctx steps while the monitor records every period-th step: the record
// needs the step's whole gradient in the buffer and the ctx's own iteration.
int ddq::check_monitor_step(ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (!c->mon.mon.ring || c->mon.mon_period <= 0) return DDQ_OK;
  if (cfg->flags & DDQ_STEP_NO_GRAD_STORE)
    return fail(c, DDQ_EINVAL, "DDQ_STEP_NO_GRAD_STORE while the monitor records steps (period %d): "
                               "fc4's gradient block in the buffer would be an earlier step's",
                c->mon.mon_period);
  if (is_async(c, cfg))
    return fail(c, DDQ_ESTATE, "the async exchange takes no monitor records: disable the monitor or "
                               "enable it with period 0");
  return DDQ_OK;
}

// ---- graph capture ----
// The scope of a capture of async ticks (what: the graph's name in errors;
// null: a capture of other steps, nothing to guard).  fork() has the comm
// stream join the capture (its owner duties follow the graph's start); a
// grad_ev recorded before the capture began is not waited on inside it
// (acapture / grad_ev_captured); and the captured ticks' host bookkeeping is
// undone when the scope ends, whether or not the body succeeded.
struct AsyncCapture {
  ddq_ctx* c;
  const char* what;
  int64_t applied = 0, ticks = 0;
  std::vector<int64_t> last;
  AsyncCapture(ddq_ctx* c_, const char* what_) : c(c_), what(what_) {
    if (!what) return;
    applied = c->applied;
    ticks = c->async.async_ticks;
    last = c->async.last_pull;
    c->async.acapture = true;
    c->async.grad_ev_captured = false;
  }
  ~AsyncCapture() {
    if (!what) return;
    c->async.acapture = false;
    c->applied = applied;
    c->async.async_ticks = ticks;
    c->async.last_pull = last;
  }
  int fork() const {
    if (!what) return DDQ_OK;
    hipError_t e = hipEventRecord(c->comm.cev[0], c->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->comm.cs, c->comm.cev[0], 0);
    if (e != hipSuccess) return fail(c, DDQ_EHIP, "%s fork: %s", what, hipGetErrorString(e));
    return DDQ_OK;
  }
};

// `body`'s launches on the ctx stream as one instantiated, uploaded exec.
int ddq::capture_exec(ddq_ctx* c, hipGraphExec_t* out, const std::function<int()>& body,
                      const char* async_what) {
  HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  hipGraph_t g = nullptr;
  int rc;
  hipError_t e;
  {
    const AsyncCapture scope(c, async_what);
    rc = scope.fork();
    if (rc == DDQ_OK) rc = body();
    e = hipStreamEndCapture(c->stream, &g);
  }
  if (rc != DDQ_OK) {
    if (g) hipGraphDestroy(g);
    return rc;
  }
  if (e != hipSuccess) return fail(c, DDQ_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
  e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (e != hipSuccess) return fail(c, DDQ_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  // upload now: the first launch of a never-uploaded exec pays the upload on
  // the stream (measured ~0.3 ms in the first timed chunk otherwise)
  HIP_TRY(c, hipGraphUpload(*out, c->stream));
  return DDQ_OK;
}

int ddq_step_async(ddq_ctx* c, const ddq_step_cfg* cfg) {
  TRY(check_step(c, cfg));
  TRY(check_monitor_step(c, cfg));
  TRY(set_dev(c));
  if (is_async(c, cfg)) {
    TRY(async_prepare(c, cfg));
    return async_round_eager(c, cfg);
  }
  TRY(check_not_async(c));
  if (c->steps == 0) TRY(initial_target_sync(c, cfg));
  const bool fault = c->fault == DDQ_FAULT_MEET_TIMEOUT;
  c->fault = 0;
  TRY(enqueue_step(c, cfg, {}, fault));
  count_steps(c, cfg, 1);
  c->replay.idx_bound = true;
  return DDQ_OK;
}

static int ensure_graph(ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (is_async(c, cfg)) return DDQ_OK;   // captured when a round starts at its phase
  TRY(check_not_async(c));
  auto& g = c->graphs.plain;
  if (g.holds(cfg)) return DDQ_OK;
  invalidate_graph(c);
  auto capture = [&](hipGraphExec_t* out, int k) {
    return capture_exec(c, out, [&]() -> int {
      for (int i = 0; i < k; ++i) TRY(enqueue_step(c, cfg));
      return DDQ_OK;
    });
  };
  TRY(capture(&g.exec[0], 1));
  TRY(capture(&g.exec[1], kGraphSteps));
  g.key(cfg);
  return DDQ_OK;
}

int ddq_step_graph_async(ddq_ctx* c, const ddq_step_cfg* cfg, int32_t nsteps) {
  TRY(check_step(c, cfg));
  TRY(check_monitor_step(c, cfg));
  TRY(set_dev(c));
  if (is_async(c, cfg)) return async_graph_steps(c, cfg, nsteps);
  TRY(ensure_graph(c, cfg));
  if (c->steps == 0 && nsteps > 0) TRY(initial_target_sync(c, cfg));
  const auto& g = c->graphs.plain;
  int i = 0;
  for (; i + kGraphSteps <= nsteps; i += kGraphSteps)
    HIP_TRY(c, hipGraphLaunch(g.exec[1], c->stream));
  for (; i < nsteps; ++i) HIP_TRY(c, hipGraphLaunch(g.exec[0], c->stream));
  if (nsteps > 0) c->replay.idx_bound = true;
  count_steps(c, cfg, nsteps);
  return DDQ_OK;
}

// nsteps training steps as a chain of graph replays in which step t+1's
// sample + gather overlap step t.  Graph step(p, f) trains on minibatch set p
// and (f = 1) prefetches into set 1-p; the chain starts on the parity that
// makes the LAST step train on set 0, so afterwards the ctx's minibatch,
// indices and counters are exactly those of nsteps sequential steps.
// With fused_prefetch the prefetch is extra blocks of the apply launch (no
// side stream), the first draw is the fused sample_gather kernel (which does
// not advance the counter) and every step's bookkeeping advances it, as in
// the plain graph step; chains longer than kGraphSteps + 1 replay
// kGraphSteps-step graphs (an even count: they start and end on set p).
static int ensure_pipe(ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (is_async(c, cfg))
    return fail(c, DDQ_EINVAL, "the async exchange runs round-robin rounds (ddq_step_async, "
                               "ddq_step_graph_async) or ticks (ddq_async_tick)");
  TRY(check_not_async(c));
  if (!c->mb[1].state) {
    TRY(mb_alloc(c, &c->mb[1]));
    mb_bind_weights(c, c->prio.prio_on);
  }
  auto& g = c->graphs.pipe;
  if (g.holds(cfg)) return DDQ_OK;
  invalidate_graph(c);
  const bool fpf = fused_prefetch(c, cfg);
  // r steps on alternating sets from set p; pf_last: the last one prefetches too
  auto capture = [&](hipGraphExec_t* out, int p, int r, bool pf_last) {
    return capture_exec(c, out, [&]() -> int {
      for (int k = 0; k < r; ++k) {
        const int q = p ^ (k & 1);
        const NetBuffers cur = mb_view(c, q), nxt = mb_view(c, 1 - q);
        TRY(enqueue_train(c, cfg, cur, (k + 1 < r || pf_last) ? &nxt : nullptr, {}));
      }
      return DDQ_OK;
    });
  };
  for (int p = 0; p < 2; ++p) {
    for (int f = 0; f < 2; ++f) TRY(capture(&g.step(p, f), p, 1, f));
    if (!fpf) continue;
    TRY(capture(&g.chain(p), p, kGraphSteps, true));
    for (int r = 2; r <= kGraphSteps; ++r) TRY(capture(&g.tail(p, r), p, r, false));
  }
  g.key(cfg);
  return DDQ_OK;
}

int ddq_step_prepare(ddq_ctx* c, const ddq_step_cfg* cfg, int32_t mode) {
  TRY(check_step(c, cfg));
  TRY(check_monitor_step(c, cfg));
  TRY(set_dev(c));
  if (mode == 1) return ensure_graph(c, cfg);
  if (mode == 2) return ensure_pipe(c, cfg);
  if (mode != 0) return fail(c, DDQ_EINVAL, "mode must be 0 (eager), 1 (graph) or 2 (pipelined)");
  return DDQ_OK;
}

int ddq_step_pipelined_async(ddq_ctx* c, const ddq_step_cfg* cfg, int32_t nsteps) {
  TRY(check_step(c, cfg));
  TRY(check_monitor_step(c, cfg));
  TRY(set_dev(c));
  if (nsteps <= 0) return DDQ_OK;
  TRY(ensure_pipe(c, cfg));
  const bool fpf = fused_prefetch(c, cfg);
  if (c->steps == 0) TRY(initial_target_sync(c, cfg));
  c->replay.idx_bound = true;
  auto& g = c->graphs.pipe;
  int p = (nsteps - 1) & 1;
  TRY(enqueue_draw(c, mb_view(c, p), cfg->seed, c->stream));
  for (int i = 0; i < nsteps;) {
    int r = 1;   // steps this launch takes
    if (fpf && nsteps - i > kGraphSteps) {
      r = kGraphSteps;
      HIP_TRY(c, hipGraphLaunch(g.chain(p), c->stream));   // ends on set p again
    } else if (fpf && nsteps - i > 1) {   // the chain's last r steps: one graph
      r = nsteps - i;
      HIP_TRY(c, hipGraphLaunch(g.tail(p, r), c->stream));
      p ^= (r - 1) & 1;   // == 0: every chain ends on set 0
    } else {
      HIP_TRY(c, hipGraphLaunch(g.step(p, i + 1 < nsteps), c->stream));
      p ^= 1;
    }
    count_steps(c, cfg, r);
    i += r;
  }
  return DDQ_OK;
}

int64_t ddq_step_count(const ddq_ctx* c) { return c ? c->steps : -1; }
