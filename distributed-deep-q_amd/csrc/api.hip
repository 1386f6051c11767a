// libddq_hip C-ABI (include/ddq_hip.h): context, device memory, replay ring,
// step orchestration, hipGraph capture, RCCL gradient exchange.
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ddq_hip.h"
#include "kernels.h"

namespace ddq {
int fc4_splits_for(int S);
int wgrad_splits_for(int layer, int B, int S, int* np);
}  // namespace ddq

using namespace ddq;

static_assert(sizeof(MonitorRecord) == sizeof(ddq_monitor_record) && sizeof(MonitorRecord) == 160 &&
                  offsetof(MonitorRecord, grad_rms) == offsetof(ddq_monitor_record, grad_rms),
              "MonitorRecord is ddq_monitor_record");

static thread_local std::string g_last_error;

// the largest frame side: launch_wgrads_conv23 (wgrads.h) has forms for conv2
// maps up to 64 x 64
static constexpr int kMaxFrame = 128;
static constexpr int kMaxRanks = 64;
static constexpr int64_t kShardPad = 64 * kMaxRanks;

// The device buffers of one Snake environment: its games' state, the zoom maps
// and the games' states as NHWC input of the forward.
template <class Game>
struct EnvBufs {
  Game* games = nullptr;
  uint8_t* maps = nullptr;
  float* in = nullptr;
  int n = 0;                       // games playing; 0: not created
};

// One graph holds kGraphSteps steps back to back (the launch of a graph
// costs ~9 us of device idle, measured, so it is paid once per kGraphSteps
// steps), plus a one-step graph for the remainder.  The device-side counters
// make every captured step read its own iteration / RNG state.
static constexpr int kGraphSteps = 8;

// The execs of one family of captured step graphs and the cfg they hold.
template <int N>
struct GraphFamily {
  hipGraphExec_t exec[N] = {};
  ddq_step_cfg cfg{};
  bool keyed = false;
  bool holds(const ddq_step_cfg* c) const { return keyed && memcmp(&cfg, c, sizeof(cfg)) == 0; }
  void key(const ddq_step_cfg* c) { cfg = *c; keyed = true; }
  void reset() {
    for (auto& g : exec) {
      if (g) hipGraphExecDestroy(g);
      g = nullptr;
    }
    keyed = false;
  }
};

// Every captured graph of a ctx.  An exec bakes in the pointers and launch
// arguments of its capture, so:
//  - whatever replaces one of those (the stream, the index log, the objective,
//    the ring's layout, the communicator, ...) calls invalidate_graph, which
//    drops every exec of every family;
//  - an exec is replayed only while its family holds() the caller's cfg, byte
//    for byte;
//  - ensure_graph / ensure_pipe, when they have to capture, drop every family
//    first; a cfg change seen by the tick or the round graphs drops that family;
//  - the round graph's phase is reset together with its exec.
struct StepGraphs {
  GraphFamily<2> plain;   // ddq_step_graph_async: [0] one step, [1] kGraphSteps steps
  // ddq_step_pipelined_async, on minibatch set p:
  struct Pipe : GraphFamily<2 * 2 + 2 + 2 * (kGraphSteps + 1)> {
    hipGraphExec_t& step(int p, int f) { return exec[2 * p + f]; }   // one step, f: prefetching
    hipGraphExec_t& chain(int p) { return exec[4 + p]; }   // kGraphSteps prefetching steps
    // r = 2..kGraphSteps steps, the last one not prefetching (the end of a fused chain)
    hipGraphExec_t& tail(int p, int r) { return exec[6 + p * (kGraphSteps + 1) + r]; }
  } pipe;
  // async round-robin rounds as one graph
  struct Round : GraphFamily<1> {
    int64_t phase = -1;   // iteration % period the graph was captured at
    void reset() { GraphFamily::reset(); phase = -1; }
  } round;
  // ticket-order ticks of this rank's own gradient, one per (P pull due,
  // special update due): ddq_async_tick replays instead of re-enqueueing
  GraphFamily<4> tick;
  void reset() {
    plain.reset();
    pipe.reset();
    round.reset();
    tick.reset();
  }
};

struct ddq_ctx {
  int device = 0;
  ddq_net_desc desc{};
  hipStream_t stream = nullptr;
  bool own_stream = true;
  NetBuffers nb{};
  std::vector<void*> allocs;
  std::string err;
  // replay ring: the view every launch takes (state == nullptr: not created;
  // meta: device; prio follows d_prio, nullptr while prioritization is off)
  ReplayRing ring{};
  uint32_t* r_bitmap = nullptr;    // large-batch sampler scratch (lazy)
  int32_t* r_blk = nullptr;
  uint64_t batch_ctr = 0;          // large-batch draws so far (RNG stream position)
  int64_t head = 0, valid = 0, capacity = 0;
  int32_t lanes = 1;               // laned ring (ddq_replay_set_lanes): head / valid per lane
  int64_t lane_len = 0;            // capacity / lanes
  int32_t nstep = 1;               // n-step returns (ddq_replay_set_nstep)
  // prioritized replay (ddq_replay_set_priority): nb.prio and the sets' isw are bound while on
  bool prio_on = false;
  ddq_priority_cfg prio_cfg{0, 0.f, 0.f, 0.f};
  PrioTree* d_prio = nullptr;      // device copy of nb.prio: the ring writers' argument
  int32_t* pset_idx = nullptr;     // ddq_replay_set_priorities staging (grown on demand)
  uint32_t* pset_q = nullptr;
  int32_t pset_cap = 0;
  bool idx_bound = false;          // nb.mb.idx holds the bound minibatch's slots
  bool adam_on = false;            // ddq_set_adam was called: nb.opt2 / gn_part / gnorm exist
  // acting scratch
  uint8_t* act_u8 = nullptr;
  float *act_in = nullptr, *act_p3 = nullptr;
  float *act_h4 = nullptr, *act_part = nullptr, *act_q = nullptr;
  __bf16 *act_p1s = nullptr, *act_p2s = nullptr;
  int32_t* act_out = nullptr;
  // device-resident Snake environments (env_create): the single actor
  // (ddq_actor_create, one game), the evaluator (ddq_eval_create) and the actor
  // pool (ddq_actors_create), each with room for B games
  EnvBufs<ActorState> a_env, p_env;
  EnvBufs<EvalGame> e_env;
  // evaluator: the per-game episode logs (grown on demand)
  int32_t* e_log = nullptr;
  size_t e_log_cap = 0;            // int32 elements allocated
  int e_max_moves = 0, e_max_ep = 0;
  uint64_t e_thresh = 0;
  int64_t e_moves = 0;             // lock-step moves enqueued since create
  // pool: the ring's per-lane head / valid at create, moves enqueued since
  int64_t p_h0 = 0, p_v0 = 0, p_moves = 0;
  // index log (ddq_index_log_enable)
  int32_t* log_buf = nullptr;
  int64_t log_buf_cap = 0;
  int64_t log_first = 0;           // first draw the log holds (the counter at enable)
  // training monitor (ddq_monitor_enable): mon.ring == nullptr while off
  MonitorEnv mon{};
  int32_t mon_period = 0;          // > 0: every single-ctx step ends with the monitor launch
  // comm (RCCL ranks, or an in-process group of ctxs exchanging by device copies)
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  bool local = false;              // member of an in-process group (ddq_group_init)
  hipStream_t cs = nullptr;        // comm stream of the overlapped all-reduce
  hipEvent_t cev[3] = {};
  int64_t shard_len = 0;           // parameters owned per rank (multiple of 64)
  float* gsl = nullptr;            // [W][shard_len] received gradient slices
  float* gstage = nullptr;         // [W][P] in-process all-reduce staging
  // async exchange: the central model's shard this rank owns (Q, and P as of
  // the last special-update pull), both at full-vector offsets
  float* own = nullptr;
  float* pown = nullptr;
  bool async_on = false;           // the async exchange began (async_begin)
  std::vector<int64_t> last_pull;  // iteration of every worker's last pull
  int64_t async_ticks = 0;         // pushes applied since async_begin
  hipEvent_t grad_ev = nullptr;    // this worker's gradient is ready (pushable)
  hipEvent_t tick_ev = nullptr;    // owner duties of the last tick done (comm stream)
  int64_t straggle_us = 0;         // ddq_set_straggle: host-side delay per gradient
  bool ready_seen = false;         // grad_ev observed complete at ready_at
  std::chrono::steady_clock::time_point ready_at{};
  int64_t rr_rounds = 0;           // round-robin rounds since the last ticket-order tick
  bool acapture = false;           // capturing async rounds: grad_ev recorded before the
  bool grad_ev_captured = false;   // capture began is not waited on (the graph launch
                                   // follows that work on the stream anyway)
  std::string comm_err;
  // ddq_inject_fault: armed failpoint, consumed by the next eager step
  int fault = 0;
  std::string small_off;           // why the small-map step is off at S = 16 (empty: on)
  StepGraphs graphs;
  // minibatch sets: [0] the ctx's own (nb.mb is its copy), [1] the twin of
  // pipelined stepping (ensure_pipe allocates it)
  Minibatch mb[2] = {};
  int64_t steps = 0;
  int64_t applied = 0;               // host mirror of the device iteration counter
  // checkpoint and resume (ddq_state_*): restoring from the first ddq_state_write
  // of a section other than "config" until ddq_state_commit; st_ctr: the
  // "counters" section as written, pushed by the commit; st_dev: device scratch
  // (kStateParts digest partials, kStateMax digests, a 128-byte stage, bad[2])
  bool restoring = false;
  ddq_state_counters st_ctr{};
  uint64_t* st_dev = nullptr;
  // profiling marks: a kernel's own dispatch start / stop events
  struct Mark {
    std::string name;
    hipEvent_t start, stop;
  };
  std::vector<Mark> marks;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
};

static int fail(ddq_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  g_last_error = buf;
  return code;
}

#define HIP_TRY(c, x)                                                                         \
  do {                                                                                        \
    g_launch_where = "";                                                                      \
    (void)hipGetLastError();  /* launches report via hipGetLastError: drop stale errors */    \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess)                                                                     \
      return fail((c), DDQ_EHIP, "%s failed: %s (%s:%d%s%s)", #x, hipGetErrorString(e_),      \
                  __FILE__, __LINE__, *g_launch_where ? ", at " : "", g_launch_where);        \
  } while (0)

#define NCCL_TRY(c, x)                                                                           \
  do {                                                                                           \
    ncclResult_t r_ = (x);                                                                       \
    if (r_ != ncclSuccess) return fail((c), DDQ_ERCCL, "%s failed: %s", #x, ncclGetErrorString(r_)); \
  } while (0)

template <class T>
static int dalloc(ddq_ctx* c, T** p, size_t count) {
  void* q = nullptr;
  const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return fail(c, DDQ_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  // stream-ordered zero fill: every device access of the ctx goes through
  // c->stream (a non-blocking stream does not order against the null stream)
  e = hipMemsetAsync(q, 0, bytes, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, DDQ_EHIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
  c->allocs.push_back(q);
  *p = reinterpret_cast<T*>(q);
  return DDQ_OK;
}

// Free one dalloc'd buffer before the ctx goes (the stream is idle).
template <class T>
static void dfree(ddq_ctx* c, T*& p) {
  if (!p) return;
  auto it = std::find(c->allocs.begin(), c->allocs.end(), (void*)p);
  if (it != c->allocs.end()) c->allocs.erase(it);
  hipFree((void*)p);
  p = nullptr;
}

#define TRY(x)                \
  do {                        \
    int r_ = (x);             \
    if (r_ != DDQ_OK) return r_; \
  } while (0)

// One minibatch set's buffers, all or none.  The reward buffer holds 2 * B
// floats: the B rewards, then the B importance-sampling weights of prioritized
// replay (mb_bind_weights).
static int mb_alloc(ddq_ctx* c, Minibatch* out) {
  const size_t B = c->nb.B, frames = B * c->nb.S * c->nb.S * 4;
  Minibatch m{};
  TRY(dalloc(c, &m.state, frames));
  TRY(dalloc(c, &m.next_state, frames));
  TRY(dalloc(c, &m.action, B * 4));
  TRY(dalloc(c, &m.reward, 2 * B));
  TRY(dalloc(c, &m.nonterm, B));
  TRY(dalloc(c, &m.idx, B));
  *out = m;
  return DDQ_OK;
}

// The weights of every allocated set: the second half of its reward buffer
// while prioritization is on, none otherwise.  nb.mb follows set 0.
static void mb_bind_weights(ddq_ctx* c, bool on) {
  for (Minibatch& m : c->mb) m.isw = on && m.reward ? m.reward + c->nb.B : nullptr;
  c->nb.mb = c->mb[0];
}

// Blocking copy ordered on the ctx stream.
static hipError_t scopy(ddq_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(c->stream);
}

static int set_dev(ddq_ctx* c) {
  HIP_TRY(c, hipSetDevice(c->device));
  return DDQ_OK;
}

// The guard of every call that launches work reading the training state:
// between the first ddq_state_write and ddq_state_commit the state is partly
// the checkpoint's and its derived copies are stale.
static int not_restoring(ddq_ctx* c) {
  if (c->restoring)
    return fail(c, DDQ_ESTATE, "restore not committed: sections were written with ddq_state_write, "
                               "call ddq_state_commit first");
  return DDQ_OK;
}
static int guard(ddq_ctx* c) {
  TRY(not_restoring(c));
  return set_dev(c);
}

static void invalidate_graph(ddq_ctx* c) { c->graphs.reset(); }

extern "C" {

int ddq_abi_version(void) { return DDQ_ABI_VERSION; }

const char* ddq_last_error(const ddq_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_last_error.c_str();
}

int ddq_create(ddq_ctx** out, int device, const ddq_net_desc* desc) {
  if (!out || !desc) return fail(nullptr, DDQ_EINVAL, "null argument");
  *out = nullptr;
  if (desc->channels != 4 || desc->actions != 4)
    return fail(nullptr, DDQ_EINVAL, "channels and actions must be 4 (got %d, %d)",
                desc->channels, desc->actions);
  if (desc->frame < 16 || desc->frame % 8 != 0 || desc->frame > 1024)
    return fail(nullptr, DDQ_EINVAL, "frame side must be a multiple of 8 in [16,1024] (got %d)",
                desc->frame);
  if (desc->batch < 1 || desc->batch > 1024)
    return fail(nullptr, DDQ_EINVAL, "batch must be in [1,1024] (got %d)", desc->batch);
  // The kernels address every tensor through 32-bit buffer descriptors and
  // offsets, and give an out-of-image vector the offset kOOB = 2^31, which
  // reads 0 only while it is >= the descriptor's num_records.  The largest
  // extents, in bytes (tests/_limit_shapes.py has the whole table):
  //   fp32 pool1 (conv2 forward's source, one descriptor)        32 B S^2
  //   the three split planes of pool1 (conv2 forward's side
  //     output for the weight gradient, one descriptor)          48 B S^2
  //   the three split planes of dpool2 (conv2 data gradient)     24 B S^2
  //   conv1's weight-gradient slabs (stores only, one
  //     descriptor, 32 KB a tile of conv2's data gradient)       64 B S^2 (8 x 16 tiles)
  //   fc4's weights                                              2^11 S^2
  // This guard bounds a split plane (16 B S^2) and W4 only: alone it would let
  // pool1 pass 2^31 from B S^2 = 2^26 on (kOOB then lies inside it and a halo
  // vector reads another image) and the slab and 48 B S^2 descriptors wrap
  // 2^32.  The frame limit below is what keeps them in range: with S <= 128
  // and B <= 1024, B S^2 <= 2^24, so pool1 is at most 2^29 bytes, the three
  // pool1 planes 3 * 2^28, the slabs 2^30 (2^31 if every map took 8 x 8
  // tiles), W4 2^25: every descriptor that is read through stays below kOOB.
  if ((int64_t)16 * desc->batch * desc->frame * desc->frame >= (1ll << 31) ||
      (int64_t)2048 * desc->frame * desc->frame >= (1ll << 31))
    return fail(nullptr, DDQ_EINVAL,
                "batch * frame^2 too large for 32-bit tensor offsets (need 16*B*S^2 < 2^31 "
                "and S < 1024; got B=%d, S=%d)", desc->batch, desc->frame);
  // conv2's and conv3's weight gradients (wgrads.h) stage whole map rows in
  // LDS, one region per wave: maps wider than 64 do not fit, and the backward
  // pass of a frame past 128 used to end in hipErrorInvalidValue after its
  // first launches.  Such a context could act but never train: refused here.
  if (desc->frame > kMaxFrame)
    return fail(nullptr, DDQ_EINVAL,
                "frame side %d not supported: the backward pass handles frames up to %d (the "
                "conv weight gradients stage whole map rows in LDS)", desc->frame, kMaxFrame);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(nullptr, DDQ_EHIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= ndev)
    return fail(nullptr, DDQ_EINVAL, "device %d out of range (%d devices)", device, ndev);
  ddq_ctx* c = new ddq_ctx();
  c->device = device;
  c->desc = *desc;
  int rc = [&]() -> int {
    TRY(set_dev(c));
    HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    NetBuffers& nb = c->nb;
    HIP_TRY(c, hipStreamCreateWithFlags(&nb.side, hipStreamNonBlocking));
    for (auto& e : nb.ev) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int B = desc->batch, S = desc->frame;
    nb.B = B; nb.S = S; nb.gamma = desc->gamma;
    nb.L = make_layout(S);
    const int64_t P = nb.L.total;
    const int S2 = S / 2, S3 = S / 4, S4 = S / 8;
    TRY(mb_alloc(c, &c->mb[0]));
    nb.mb = c->mb[0];
    for (int z = 0; z < 2; ++z) {
      TRY(dalloc(c, &nb.pool3[z], (size_t)B * S4 * S4 * 64));
      TRY(dalloc(c, &nb.h4[z], (size_t)B * 512));
      TRY(dalloc(c, &nb.theta[z], (size_t)P + kShardPad));
      TRY(dalloc(c, &nb.wks[z], (size_t)3 * nb.L.wks_total));   // zero: conv1's kx 7 stays 0
      TRY(dalloc(c, &nb.pool1f[z], (size_t)B * S2 * S2 * 32));
      TRY(dalloc(c, &nb.pool2f[z], (size_t)B * S3 * S3 * 64));
    }
    TRY(dalloc(c, &nb.pool1s[0], (size_t)3 * B * S2 * S2 * 32));   // Q tower only
    TRY(dalloc(c, &nb.pool2s[0], (size_t)3 * B * S3 * S3 * 64));
    TRY(dalloc(c, &nb.mask1, (size_t)B * S2 * S2 * 32));
    TRY(dalloc(c, &nb.mask2, (size_t)B * S3 * S3 * 64));
    TRY(dalloc(c, &nb.mask3, (size_t)B * S4 * S4 * 64));
    nb.fc4_splits = fc4_splits_for(S);
    TRY(dalloc(c, &nb.fc4_part, (size_t)nb.fc4_splits * 2 * B * 512));
    TRY(dalloc(c, &nb.q_out, (size_t)B * 4));
    TRY(dalloc(c, &nb.p_out, (size_t)B * 4));
    TRY(dalloc(c, &nb.q_sa, (size_t)B));
    TRY(dalloc(c, &nb.p_sa, (size_t)B));
    TRY(dalloc(c, &nb.target, (size_t)B));
    TRY(dalloc(c, &nb.loss, 1));
    TRY(dalloc(c, &nb.dh4, (size_t)B * 512));
    TRY(dalloc(c, &nb.dqbuf, (size_t)B * 4));
    TRY(dalloc(c, &nb.lpart, (size_t)B));
    TRY(dalloc(c, &nb.dconv3, (size_t)B * S3 * S3 * 64));
    TRY(dalloc(c, &nb.dconv2s, (size_t)3 * B * S3 * S3 * 64));
    TRY(dalloc(c, &nb.dconv3s, (size_t)3 * B * S3 * S3 * 64));
    if (S == 16) {   // K1 (tower_fwd16s): the pool2 halves' exchange; meeting words
      TRY(dalloc(c, &nb.xchg, (size_t)B * 2 * 2 * 1536));
      TRY(dalloc(c, &nb.pairc, (size_t)B * 2));
      TRY(dalloc(c, &nb.csync, 64));
    }
    // the four-launch small-map step needs every meeting launch's workgroups
    // co-resident (small_coresident); otherwise the general kernels run
    nb.small = 0;
    if (S == 16 && B <= 256) {
      int ok = 0;
      char why[256] = "";
      HIP_TRY(c, small_coresident(B, &ok, why, sizeof(why)));
      nb.small = ok;
      if (!ok) c->small_off = why;
    } else {
      c->small_off = S == 16 ? "batch > 256" : "frame != 16";
    }
    if (nb.small) {
      TRY(dalloc(c, &nb.qpart, (size_t)32 * 2 * B * 4));
      TRY(dalloc(c, &nb.dpart, (size_t)32 * B * 256));
      TRY(dalloc(c, &nb.dconv2x, (size_t)3 * B * 4096));
      int G2, G3;
      small_groups(B, &G2, &G3);
      TRY(dalloc(c, &nb.slab2, (size_t)10 * G2 * (32 * 5 * 32 + 32)));
      TRY(dalloc(c, &nb.slab3, (size_t)6 * G3 * (32 * 3 * 64 + 32)));
      nb.small_G = B > 32 ? (B + 31) / 32 : 1;   // <= 8: 32 G fc4 workgroups, all resident
      if (nb.small_G > 1) {
        TRY(dalloc(c, &nb.upart, (size_t)nb.small_G * 32 * 96));
        TRY(dalloc(c, &nb.w4part, (size_t)nb.small_G * 512 * 256));
      }
    }
    int64_t off = 0;
    const int cout[3] = {32, 64, 64};
    for (int l = 0; l < 3; ++l) {
      nb.wsplits[l] = wgrad_splits_for(l, B, S, &nb.wnp[l]);
      nb.wpart_off[l] = off;
      off += (int64_t)nb.wsplits[l] * cout[l] * nb.wnp[l];
    }
    TRY(dalloc(c, &nb.wpart, (size_t)off));
    // zero tails of kShardPad floats: W equal shards of a multiple of 64
    // floats cover P for every W <= kMaxRanks
    TRY(dalloc(c, &nb.grad, (size_t)P + kShardPad));
    TRY(dalloc(c, &nb.opt, (size_t)P + kShardPad));
    TRY(dalloc(c, &nb.opt_init, 4));
    TRY(dalloc(c, &nb.iter, 1));
    // acting scratch (n <= B)
    TRY(dalloc(c, &c->act_u8, (size_t)B * 4 * S * S));
    TRY(dalloc(c, &c->act_in, (size_t)B * S * S * 4));
    TRY(dalloc(c, &c->act_p1s, (size_t)3 * B * S2 * S2 * 32));
    TRY(dalloc(c, &c->act_p2s, (size_t)3 * B * S3 * S3 * 64));
    TRY(dalloc(c, &c->act_p3, (size_t)B * S4 * S4 * 64));
    TRY(dalloc(c, &c->act_h4, (size_t)B * 512));
    TRY(dalloc(c, &c->act_part, (size_t)nb.fc4_splits * 2 * B * 512));
    TRY(dalloc(c, &c->act_q, (size_t)B * 4));
    TRY(dalloc(c, &c->act_out, (size_t)B));
    TRY(dalloc(c, &c->ring.meta, 1));
    return DDQ_OK;
  }();
  if (rc != DDQ_OK) {
    g_last_error = c->err;
    ddq_destroy(c);
    return rc;
  }
  *out = c;
  return DDQ_OK;
}

int ddq_destroy(ddq_ctx* c) {
  if (!c) return DDQ_OK;
  hipSetDevice(c->device);
  if (c->cs) hipStreamSynchronize(c->cs);
  if (c->stream) hipStreamSynchronize(c->stream);
  invalidate_graph(c);   // (every graph exec: the step, pipelined, async ones)
  for (auto& e : c->ev_pool) hipEventDestroy(e);
  if (c->comm) ncclCommDestroy(c->comm);
  for (void* p : c->allocs) hipFree(p);
  if (c->stream && c->own_stream) hipStreamDestroy(c->stream);
  for (auto& e : c->nb.ev)
    if (e) hipEventDestroy(e);
  if (c->nb.side) hipStreamDestroy(c->nb.side);
  if (c->cs) hipStreamDestroy(c->cs);
  if (c->grad_ev) hipEventDestroy(c->grad_ev);
  if (c->tick_ev) hipEventDestroy(c->tick_ev);
  for (auto& e : c->cev)
    if (e) hipEventDestroy(e);
  delete c;
  return DDQ_OK;
}

int ddq_set_stream(ddq_ctx* c, void* s) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->own_stream) hipStreamDestroy(c->stream);
  if (s) {
    c->stream = reinterpret_cast<hipStream_t>(s);
    c->own_stream = false;
  } else {
    HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  invalidate_graph(c);
  return DDQ_OK;
}

int ddq_get_stream(const ddq_ctx* c, void** s) {
  if (!c || !s) return fail(nullptr, DDQ_EINVAL, "null argument");
  *s = reinterpret_cast<void*>(c->stream);
  return DDQ_OK;
}

int ddq_synchronize(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(set_dev(c));
  if (c->cs) HIP_TRY(c, hipStreamSynchronize(c->cs));   // owner duties of async ticks
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->nb.csync) {                  // the small-map kernels' sticky spin-timeout words
    int32_t w[64];
    HIP_TRY(c, hipMemcpy(w, c->nb.csync, sizeof(w), hipMemcpyDeviceToHost));
    const int at[3] = {2, 40, 48};
    const char* who[3] = {"fc4 chain fan-in", "wgrad slab reduce", "tower pool2 exchange"};
    for (int k = 0; k < 3; ++k)
      if (w[at[k]]) {
        // the launches after the failure wrote no parameter, optimizer state
        // or iteration (they read the sticky words); start the meeting
        // counters afresh (a launch short of a party leaves them off by its
        // count) and take the device iteration back as the host's
        HIP_TRY(c, hipMemsetAsync(c->nb.csync, 0, 64 * sizeof(int32_t), c->stream));
        if (c->nb.pairc)
          HIP_TRY(c, hipMemsetAsync(c->nb.pairc, 0, (size_t)c->nb.B * 2 * sizeof(uint64_t), c->stream));
        int64_t it = 0;
        HIP_TRY(c, hipMemcpyAsync(&it, c->nb.iter, sizeof(it), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->applied = it;
        return fail(c, DDQ_ESTATE,
                    "small-map step: %s meeting timed out (that step and any after it up to "
                    "this call applied nothing)", who[k]);
      }
  }
  return DDQ_OK;
}

int ddq_inject_fault(ddq_ctx* c, int32_t fault) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (fault == DDQ_FAULT_NONE) {
    c->fault = 0;
    return DDQ_OK;
  }
  if (fault != DDQ_FAULT_MEET_TIMEOUT) return fail(c, DDQ_EINVAL, "unknown fault %d", fault);
  if (!c->nb.small) return fail(c, DDQ_ESTATE, "no small-map step on this ctx (S = 16, B <= 256)");
  c->fault = fault;
  return DDQ_OK;
}

int ddq_small_path(const ddq_ctx* c, char* why, int32_t cap) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (why && cap > 0) snprintf(why, (size_t)cap, "%s", c->small_off.c_str());
  return c->nb.small ? 1 : 0;
}

// ---------------- parameters ----------------
int64_t ddq_num_params(const ddq_ctx* c) { return c ? c->nb.L.total : -1; }

int ddq_param_layout(const ddq_ctx* c, ddq_blob_desc* out, int32_t cap, int32_t* n) {
  if (!c || !n) return fail(nullptr, DDQ_EINVAL, "null argument");
  const ParamLayout& L = c->nb.L;
  const char* names[5] = {"Qconv1", "Qconv2", "Qconv3", "Qfc4", "Q_out"};
  const int cout[3] = {32, 64, 64}, cin[3] = {4, 32, 64}, ks[3] = {7, 5, 3};
  *n = 10;
  if (!out) return DDQ_OK;
  if (cap < 10) return fail(const_cast<ddq_ctx*>(c), DDQ_EINVAL, "layout needs 10 entries");
  for (int l = 0; l < 5; ++l) {
    for (int i = 0; i < 2; ++i) {
      ddq_blob_desc& d = out[2 * l + i];
      memset(&d, 0, sizeof(d));
      snprintf(d.name, sizeof(d.name), "%s", names[l]);
      d.index = i;
      if (i == 0) {
        if (l < 3) { d.shape[0] = cout[l]; d.shape[1] = cin[l]; d.shape[2] = ks[l]; d.shape[3] = ks[l]; }
        else { d.shape[0] = 1; d.shape[1] = 1; d.shape[2] = l == 3 ? 512 : 4;
               d.shape[3] = l == 3 ? (int)(64 * L.S4 * L.S4) : 512; }
        d.offset = L.w[l]; d.count = L.wn[l];
      } else {
        d.shape[0] = 1; d.shape[1] = 1; d.shape[2] = 1; d.shape[3] = (int)L.bn[l];
        d.offset = L.b[l]; d.count = L.bn[l];
      }
    }
  }
  return DDQ_OK;
}

static int copy_in(ddq_ctx* c, float* dst, const float* src, int64_t n, int on_dev) {
  HIP_TRY(c, hipMemcpyAsync(dst, src, n * sizeof(float),
                            on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  return DDQ_OK;
}
static int copy_out(ddq_ctx* c, float* dst, const float* src, int64_t n, int on_dev) {
  HIP_TRY(c, hipMemcpyAsync(dst, src, n * sizeof(float),
                            on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_set_params(ddq_ctx* c, int32_t which, const float* src, int64_t n, int32_t on_dev) {
  if (!c || !src) return fail(c, DDQ_EINVAL, "null argument");
  if (which != 0 && which != 1) return fail(c, DDQ_EINVAL, "which must be 0 (Q) or 1 (P)");
  if (n != c->nb.L.total)
    return fail(c, DDQ_EINVAL, "expected %lld params, got %lld", (long long)c->nb.L.total, (long long)n);
  TRY(set_dev(c));
  TRY(copy_in(c, c->nb.theta[which], src, n, on_dev));
  HIP_TRY(c, launch_relayout(c->nb, which, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_get_params(ddq_ctx* c, int32_t which, float* dst, int64_t n, int32_t on_dev) {
  if (!c || !dst) return fail(c, DDQ_EINVAL, "null argument");
  if (which != 0 && which != 1) return fail(c, DDQ_EINVAL, "which must be 0 (Q) or 1 (P)");
  if (n != c->nb.L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  TRY(set_dev(c));
  return copy_out(c, dst, c->nb.theta[which], n, on_dev);
}

int ddq_get_grads(ddq_ctx* c, float* dst, int64_t n, int32_t on_dev) {
  if (!c || !dst) return fail(c, DDQ_EINVAL, "null argument");
  if (n != c->nb.L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  TRY(set_dev(c));
  return copy_out(c, dst, c->nb.grad, n, on_dev);
}

int ddq_set_grads(ddq_ctx* c, const float* src, int64_t n, int32_t on_dev) {
  if (!c || !src) return fail(c, DDQ_EINVAL, "null argument");
  if (n != c->nb.L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  TRY(set_dev(c));
  TRY(copy_in(c, c->nb.grad, src, n, on_dev));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_sync_target(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(set_dev(c));
  HIP_TRY(c, hipMemcpyAsync(c->nb.theta[1], c->nb.theta[0], c->nb.L.total * 4,
                            hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->nb.wks[1], c->nb.wks[0], c->nb.L.wks_total * 3 * 2,
                            hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

// ---------------- soft target updates ----------------
int ddq_set_target_tau(ddq_ctx* c, float tau) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!(tau > 0.f && tau <= 1.f))
    return fail(c, DDQ_EINVAL, "target tau must be in (0, 1] (got %g)", (double)tau);
  if (c->async_on && tau < 1.f)
    return fail(c, DDQ_EINVAL, "soft target updates (tau %g < 1) with the async exchange: its P "
                               "travels by pulls, not by the steps' syncs", (double)tau);
  invalidate_graph(c);   // captured steps hold tau as a launch argument
  c->nb.target_tau = tau;
  return DDQ_OK;
}

int ddq_get_target_tau(const ddq_ctx* c, float* tau) {
  if (!c || !tau) return fail(nullptr, DDQ_EINVAL, "null argument");
  *tau = c->nb.target_tau;
  return DDQ_OK;
}

// One launch: the refresh with its sync forced blends every parameter of P
// towards Q (target_blend) and rewrites the conv weights' split copies from
// the blended values.
int ddq_soft_sync_target(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->nb.target_tau >= 1.f) return ddq_sync_target(c);
  TRY(set_dev(c));
  HIP_TRY(c, launch_refresh(c->nb, c->stream, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

// ---------------- prioritized replay: tree set-up ----------------
static void prio_release(ddq_ctx* c) {
  PrioTree& t = c->nb.prio;
  dfree(c, t.leaf);
  for (auto& p : t.sum) dfree(c, p);
  dfree(c, t.st);
  t = PrioTree{};
  mb_bind_weights(c, false);
  c->ring.prio = nullptr;
  c->prio_on = false;
  c->prio_cfg.enabled = 0;
}

// every filled, allowed slot <- pmax = 1.0, the rest 0, sums bottom-up
// (enable, import, fill_tiled, set_nstep, set_lanes); synchronises
static int prio_rebuild(ddq_ctx* c) {
  if (!c->prio_on) return DDQ_OK;
  const uint32_t one = kPrioOne;
  HIP_TRY(c, hipMemcpyAsync(&c->nb.prio.st->pmax, &one, 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_prio_rebuild(c->nb.prio, c->ring.meta, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->idx_bound = false;
  return DDQ_OK;
}

// the enable path's device work: the scalars, the writers' copy of the tree,
// weights of 1 for a minibatch bound before any draw, the first rebuild
static int prio_enable_fill(ddq_ctx* c, const float abe[3]) {
  const PrioTree& t = c->nb.prio;
  HIP_TRY(c, hipMemcpyAsync(t.st, abe, 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->d_prio, &t, sizeof(t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_fill_ones(c->nb.mb.isw, c->nb.B, c->stream));
  return prio_rebuild(c);
}

static int prio_refuse(ddq_ctx* c, const char* what) {
  if (c && c->prio_on)
    return fail(c, DDQ_ESTATE, "%s while prioritized replay is on: priorities are kept per ring, "
                               "not across ranks (ddq_replay_set_priority with enabled = 0 first)",
                what);
  return DDQ_OK;
}

// ---------------- replay ----------------
static int push_meta(ddq_ctx* c, bool prio_add = false, int64_t h = 0) {
  int64_t hv[2] = {c->head, c->valid};
  HIP_TRY(c, hipMemcpyAsync(c->ring.meta, hv, sizeof(hv), hipMemcpyHostToDevice, c->stream));
  // prioritized replay: the writer rule on the slot just added, after the new
  // head / valid (stream order)
  if (prio_add) HIP_TRY(c, launch_prio_add(c->nb.prio, c->ring.meta, 0, h, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_replay_create(ddq_ctx* c, int64_t capacity) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (capacity < 2 || capacity > (int64_t)INT32_MAX)
    return fail(c, DDQ_EINVAL, "capacity must be in [2, 2^31) (got %lld)", (long long)capacity);
  if (c->ring.state) return fail(c, DDQ_ESTATE, "replay already created");
  TRY(set_dev(c));
  const size_t slot = (size_t)4 * c->nb.S * c->nb.S;
  TRY(dalloc(c, &c->ring.state, slot * capacity));
  TRY(dalloc(c, &c->ring.action, (size_t)capacity));
  TRY(dalloc(c, &c->ring.reward, (size_t)capacity));
  TRY(dalloc(c, &c->ring.nonterm, (size_t)capacity));
  c->capacity = capacity;
  c->head = c->valid = 0;
  c->lanes = 1;
  c->lane_len = capacity;
  c->nstep = 1;
  c->nb.nstep = 1;
  prio_release(c);
  ReplayMeta m{};
  m.capacity = capacity;
  m.lanes = 1;
  m.lane_len = capacity;
  m.nstep = 1;
  m.gamma = c->nb.gamma;
  HIP_TRY(c, scopy(c, c->ring.meta, &m, sizeof(m), hipMemcpyHostToDevice));
  invalidate_graph(c);
  return DDQ_OK;
}

int ddq_replay_add(ddq_ctx* c, int32_t action, int32_t reward, const uint8_t* state) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->lanes > 1) return fail(c, DDQ_ESTATE, "ddq_replay_add on a laned ring (%d lanes)", c->lanes);
  if (action < 0 || action > 255) return fail(c, DDQ_EINVAL, "action must fit uint8");
  if (reward < -32768 || reward > 32767) return fail(c, DDQ_EINVAL, "reward must fit int16");
  TRY(guard(c));
  const size_t slot = (size_t)4 * c->nb.S * c->nb.S;
  const int64_t h = c->head;
  uint8_t a = (uint8_t)action, nt = state ? 1 : 0;
  int16_t r = (int16_t)reward;
  HIP_TRY(c, hipMemcpyAsync(c->ring.action + h, &a, 1, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->ring.reward + h, &r, 2, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->ring.nonterm + h, &nt, 1, hipMemcpyHostToDevice, c->stream));
  if (state)
    HIP_TRY(c, hipMemcpyAsync(c->ring.state + h * slot, state, slot, hipMemcpyHostToDevice, c->stream));
  c->head = (c->head + 1) % c->capacity;
  c->valid = std::min(c->capacity, c->valid + 1);
  return push_meta(c, c->prio_on, h);
}

int ddq_replay_info(const ddq_ctx* c, int64_t* head, int64_t* valid, int64_t* capacity) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (head) *head = c->head;
  if (valid) *valid = c->valid;
  if (capacity) *capacity = c->capacity;
  return DDQ_OK;
}

// n-step returns (include/ddq_hip.h): forbidden start slots and the allowed
// count A per lane, on the host mirror of head / valid
static bool slot_forbidden(const ddq_ctx* c, int64_t x) {
  int64_t d = c->head - 1 - x;
  if (d < 0 && c->nstep >= 2 && c->valid == c->lane_len) d += c->lane_len;
  return d >= 0 && d < c->nstep;
}

static int64_t allowed_slots(const ddq_ctx* c) {
  if (c->nstep < 2) return c->valid - 1;
  if (c->valid == c->lane_len) return c->lane_len - c->nstep;
  const int64_t lo = std::max<int64_t>(0, c->head - c->nstep);
  const int64_t hi = std::min(c->head - 1, c->valid - 1);
  return c->valid - std::max<int64_t>(0, hi - lo + 1);
}

// fewest filled, allowed slots a draw of B needs: B <= lanes * A, which is
// B <= lanes * (valid - 1) at n = 1 (B < valid on a plain ring)
static bool too_few_slots(const ddq_ctx* c, int64_t batch) {
  return batch > c->lanes * allowed_slots(c);
}

int ddq_replay_set_lanes(ddq_ctx* c, int32_t lanes) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->valid != 0) return fail(c, DDQ_ESTATE, "set_lanes needs an empty ring (valid = %lld)",
                                 (long long)c->valid);
  if (lanes < 1 || c->capacity % lanes != 0 || c->capacity / lanes < 2)
    return fail(c, DDQ_EINVAL, "lanes must divide capacity %lld into lanes of >= 2 slots (got %d)",
                (long long)c->capacity, lanes);
  if (c->capacity / lanes <= c->nstep)
    return fail(c, DDQ_EINVAL, "%d lanes of %lld slots cannot hold the ring's %d-step windows",
                lanes, (long long)(c->capacity / lanes), c->nstep);
  if (lanes == c->lanes) return DDQ_OK;
  TRY(set_dev(c));
  c->lanes = lanes;
  c->lane_len = c->capacity / lanes;
  c->head = 0;
  c->p_env.n = 0;                    // a pool or an actor belongs to the lanes it was
  c->a_env.n = 0;                    // created on
  char* m = reinterpret_cast<char*>(c->ring.meta);
  HIP_TRY(c, scopy(c, m + offsetof(ReplayMeta, lanes), &c->lanes, 4, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, m + offsetof(ReplayMeta, lane_len), &c->lane_len, 8, hipMemcpyHostToDevice));
  TRY(push_meta(c));
  return prio_rebuild(c);
}

int ddq_replay_lanes(const ddq_ctx* c, int32_t* lanes, int64_t* lane_len) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->ring.state) return fail(const_cast<ddq_ctx*>(c), DDQ_ESTATE, "no replay buffer");
  if (lanes) *lanes = c->lanes;
  if (lane_len) *lane_len = c->lane_len;
  return DDQ_OK;
}

static_assert(kNstepMax == DDQ_NSTEP_MAX, "the window loops unroll to DDQ_NSTEP_MAX");

int ddq_replay_set_nstep(ddq_ctx* c, int32_t n) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->async_on)
    return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx: set the n-step "
                               "length before ddq_async_begin");
  if (n < 1 || n > DDQ_NSTEP_MAX || n >= c->lane_len)
    return fail(c, DDQ_EINVAL, "n-step length must be in [1, %d] and below lane_len %lld (got %d)",
                DDQ_NSTEP_MAX, (long long)c->lane_len, n);
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);   // a pipelined chain holds a minibatch gathered under the old n
  c->nstep = n;
  c->nb.nstep = n;   // n >= 2: the n-step instantiations of the drawing / gathering kernels
  HIP_TRY(c, scopy(c, reinterpret_cast<char*>(c->ring.meta) + offsetof(ReplayMeta, nstep), &c->nstep,
                   4, hipMemcpyHostToDevice));
  return prio_rebuild(c);
}

int ddq_replay_nstep(const ddq_ctx* c, int32_t* n) {
  if (!c || !n) return fail(nullptr, DDQ_EINVAL, "null argument");
  if (!c->ring.state) return fail(const_cast<ddq_ctx*>(c), DDQ_ESTATE, "no replay buffer");
  *n = c->nstep;
  return DDQ_OK;
}

// ---------------- prioritized replay: entry points ----------------
static bool unit_interval(float x) { return std::isfinite(x) && x >= 0.f && x <= 1.f; }

int ddq_replay_set_priority(ddq_ctx* c, const ddq_priority_cfg* p) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!p) return fail(c, DDQ_EINVAL, "null priority cfg");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  TRY(set_dev(c));
  if (!p->enabled) {
    if (!c->prio_on) return DDQ_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    invalidate_graph(c);   // captured steps hold the tree, the weights and the extra launches
    prio_release(c);
    return DDQ_OK;
  }
  if (!unit_interval(p->alpha)) return fail(c, DDQ_EINVAL, "alpha must be in [0, 1] (got %g)", (double)p->alpha);
  if (!unit_interval(p->beta)) return fail(c, DDQ_EINVAL, "beta must be in [0, 1] (got %g)", (double)p->beta);
  if (!(std::isfinite(p->eps) && p->eps > 0.f))
    return fail(c, DDQ_EINVAL, "eps must be finite and > 0 (got %g)", (double)p->eps);
  if (c->nb.B > 256)
    return fail(c, DDQ_EINVAL, "prioritized replay draws B <= 256 in one workgroup (B = %d)", c->nb.B);
  // (the async exchange needs a communicator or a group, so it is named first)
  if (c->async_on) return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx");
  if (c->comm || c->local)
    return fail(c, DDQ_ESTATE, "prioritized replay on a ctx with a communicator or in a group: "
                               "priorities are kept per ring, not across ranks");
  const float abe[3] = {p->alpha, p->beta, p->eps};
  if (c->prio_on) {
    // the annealing path: three scalars in device memory, stream-ordered; captured
    // graphs read them live.  No synchronisation, no rebuild, no graph drop.
    HIP_TRY(c, hipMemcpyAsync(c->nb.prio.st, abe, sizeof(abe), hipMemcpyHostToDevice, c->stream));
    c->prio_cfg = ddq_priority_cfg{1, p->alpha, p->beta, p->eps};
    return DDQ_OK;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);
  PrioTree t{};
  t.capacity = c->capacity;
  t.padded[0] = (c->capacity + 63) / 64 * 64;
  int K = 0;
  do {
    ++K;
    t.padded[K] = (t.padded[K - 1] / 64 + 63) / 64 * 64;
  } while (t.padded[K - 1] / 64 > 64 && K < kPrioLevels);
  if (t.padded[K - 1] / 64 > 64) return fail(c, DDQ_EINVAL, "ring too large for the priority tree");
  t.nlev = K;
  int rc = dalloc(c, &t.leaf, (size_t)t.padded[0]);
  for (int k = 1; k <= K && rc == DDQ_OK; ++k) rc = dalloc(c, &t.sum[k - 1], (size_t)t.padded[k]);
  if (rc == DDQ_OK) rc = dalloc(c, &t.st, 1);
  // (d_prio and the ddq_replay_set_priorities staging outlive a disable: the next
  // enable reuses them, ddq_destroy frees them with every other allocation)
  if (rc == DDQ_OK && !c->d_prio) rc = dalloc(c, &c->d_prio, 1);
  c->nb.prio = t;
  mb_bind_weights(c, true);
  c->ring.prio = c->d_prio;
  c->prio_on = true;
  if (rc == DDQ_OK) rc = prio_enable_fill(c, abe);
  if (rc != DDQ_OK) { prio_release(c); return rc; }   // all or nothing: no half-bound tree
  c->prio_cfg = ddq_priority_cfg{1, p->alpha, p->beta, p->eps};
  return DDQ_OK;
}

int ddq_replay_get_priority(const ddq_ctx* c, ddq_priority_cfg* p) {
  if (!c || !p) return fail(nullptr, DDQ_EINVAL, "null argument");
  *p = c->prio_cfg;
  return DDQ_OK;
}

int ddq_replay_priorities(ddq_ctx* c, uint32_t* leaves, int64_t n, uint64_t* total, uint32_t* pmax) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->prio_on) return fail(c, DDQ_ESTATE, "prioritized replay is off");
  if (leaves && n != c->capacity)
    return fail(c, DDQ_EINVAL, "the ring has %lld leaves (got n = %lld)", (long long)c->capacity,
                (long long)n);
  TRY(set_dev(c));
  if (leaves) HIP_TRY(c, scopy(c, leaves, c->nb.prio.leaf, (size_t)n * 4, hipMemcpyDeviceToHost));
  PrioState st;
  HIP_TRY(c, scopy(c, &st, c->nb.prio.st, sizeof(st), hipMemcpyDeviceToHost));
  if (total) *total = st.total;
  if (pmax) *pmax = st.pmax;
  return DDQ_OK;
}

int ddq_replay_set_priorities(ddq_ctx* c, const int32_t* idx, const uint32_t* q, int32_t n) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->prio_on) return fail(c, DDQ_ESTATE, "prioritized replay is off");
  if (n < 0 || (n > 0 && (!idx || !q))) return fail(c, DDQ_EINVAL, "bad argument");
  if (n == 0) return DDQ_OK;
  TRY(set_dev(c));
  std::vector<uint32_t> leaf((size_t)c->capacity);
  HIP_TRY(c, scopy(c, leaf.data(), c->nb.prio.leaf, leaf.size() * 4, hipMemcpyDeviceToHost));
  for (int k = 0; k < n; ++k) {
    if (idx[k] < 0 || idx[k] >= c->capacity) return fail(c, DDQ_EINVAL, "index %d out of range", idx[k]);
    if (q[k] > kPrioMax) return fail(c, DDQ_EINVAL, "priority %u above 2^24", q[k]);
    if ((q[k] == 0) != (leaf[idx[k]] == 0))
      return fail(c, DDQ_EINVAL, "slot %d: a zero leaf (unfilled or forbidden slot) stays zero and "
                                 "a nonzero leaf stays nonzero", idx[k]);
  }
  // a slot given twice takes its last value
  std::vector<int32_t> hi;
  std::vector<uint32_t> hq;
  for (int k = 0; k < n; ++k) {
    bool later = false;
    for (int o = k + 1; o < n && !later; ++o) later = idx[o] == idx[k];
    if (!later) { hi.push_back(idx[k]); hq.push_back(q[k]); }
  }
  const int m = (int)hi.size();
  if (m > c->pset_cap) {
    dfree(c, c->pset_idx);
    dfree(c, c->pset_q);
    c->pset_cap = 0;
    TRY(dalloc(c, &c->pset_idx, (size_t)m));
    TRY(dalloc(c, &c->pset_q, (size_t)m));
    c->pset_cap = m;
  }
  HIP_TRY(c, hipMemcpyAsync(c->pset_idx, hi.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->pset_q, hq.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_prio_set(c->nb.prio, c->pset_idx, c->pset_q, m, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_replay_update_priorities_async(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->prio_on) return fail(c, DDQ_ESTATE, "prioritized replay is off");
  if (!c->idx_bound)
    return fail(c, DDQ_ESTATE, "no device-side index set is bound (the minibatch was not drawn from "
                               "the ring)");
  TRY(set_dev(c));
  HIP_TRY(c, launch_prio_commit(c->nb, c->ring.meta, c->stream));
  return DDQ_OK;
}

int ddq_replay_import(ddq_ctx* c, const uint8_t* state, const uint8_t* action,
                      const int16_t* reward, const uint8_t* nonterm, int64_t n, int64_t head,
                      int64_t valid) {
  if (!c || !state || !action || !reward || !nonterm) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (n != c->capacity) return fail(c, DDQ_EINVAL, "import size %lld != capacity %lld",
                                    (long long)n, (long long)c->capacity);
  if (head < 0 || head >= c->lane_len || valid < 0 || valid > c->lane_len)
    return fail(c, DDQ_EINVAL, "head/valid out of range");
  TRY(set_dev(c));
  const size_t slot = (size_t)4 * c->nb.S * c->nb.S;
  HIP_TRY(c, scopy(c, c->ring.state, state, slot * n, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, c->ring.action, action, n, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, c->ring.reward, reward, 2 * n, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, c->ring.nonterm, nonterm, n, hipMemcpyHostToDevice));
  c->head = head;
  c->valid = valid;
  TRY(push_meta(c));
  return prio_rebuild(c);
}

int ddq_replay_export(ddq_ctx* c, uint8_t* state, uint8_t* action, int16_t* reward,
                      uint8_t* nonterm, int64_t n) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (n != c->capacity) return fail(c, DDQ_EINVAL, "export size mismatch");
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t slot = (size_t)4 * c->nb.S * c->nb.S;
  if (state) HIP_TRY(c, scopy(c, state, c->ring.state, slot * n, hipMemcpyDeviceToHost));
  if (action) HIP_TRY(c, scopy(c, action, c->ring.action, n, hipMemcpyDeviceToHost));
  if (reward) HIP_TRY(c, scopy(c, reward, c->ring.reward, 2 * n, hipMemcpyDeviceToHost));
  if (nonterm) HIP_TRY(c, scopy(c, nonterm, c->ring.nonterm, n, hipMemcpyDeviceToHost));
  return DDQ_OK;
}

static int check_err_flag(ddq_ctx* c) {
  ReplayMeta m;
  HIP_TRY(c, hipMemcpyAsync(&m, c->ring.meta, sizeof(m), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (m.err) {
    int32_t z = 0;
    HIP_TRY(c, scopy(c, reinterpret_cast<char*>(c->ring.meta) + offsetof(ReplayMeta, err), &z, 4,
                         hipMemcpyHostToDevice));
    if (m.err == 2) return fail(c, DDQ_ERANGE, "batch sampler could not find distinct indices");
    return fail(c, DDQ_ERANGE, "stored action index out of range for %d actions", 4);
  }
  return DDQ_OK;
}

int ddq_replay_sample(ddq_ctx* c, const int32_t* idx, int32_t batch) {
  if (!c || !idx) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (too_few_slots(c, batch))
    return fail(c, DDQ_EINVAL, "Can't draw sample of size %d from replay dataset of size %lld",
                batch, (long long)(c->lanes * c->valid));
  if (batch != c->nb.B)
    return fail(c, DDQ_EINVAL, "sample size %d != net batch %d", batch, c->nb.B);
  for (int i = 0; i < batch; ++i) {
    if (idx[i] < 0 || idx[i] >= c->capacity || idx[i] % c->lane_len >= c->valid)
      return fail(c, DDQ_EINVAL, "index %d out of [0,valid)", idx[i]);
    if (c->nstep >= 2 && slot_forbidden(c, idx[i] % c->lane_len))
      return fail(c, DDQ_EINVAL, "index %d: its %d-step window reaches the write head", idx[i],
                  c->nstep);
    if (i && idx[i] <= idx[i - 1]) return fail(c, DDQ_EINVAL, "indices must be sorted and distinct");
  }
  TRY(guard(c));
  HIP_TRY(c, hipMemcpyAsync(c->nb.mb.idx, idx, batch * 4, hipMemcpyHostToDevice, c->stream));
  if (c->nb.mb.isw) HIP_TRY(c, launch_fill_ones(c->nb.mb.isw, batch, c->stream));   // host-given set
  HIP_TRY(c, launch_gather(c->nb, c->ring, c->stream));
  c->idx_bound = true;
  return check_err_flag(c);
}

int ddq_replay_sample_device_async(ddq_ctx* c, uint64_t seed) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (too_few_slots(c, c->nb.B))
    return fail(c, DDQ_EINVAL, "Can't draw sample of size %d from replay dataset of size %lld",
                c->nb.B, (long long)(c->lanes * c->valid));
  TRY(guard(c));
  if (c->prio_on) {   // the prioritized draw (one workgroup), then its counter's advance
    HIP_TRY(c, launch_prio_sample(c->nb, c->ring.meta, seed, c->stream, true));
  } else {
    HIP_TRY(c, launch_sample(c->nb, c->ring.meta, seed, c->stream));
  }
  HIP_TRY(c, launch_gather(c->nb, c->ring, c->stream));
  c->idx_bound = true;
  return DDQ_OK;
}

int ddq_replay_fill_tiled(ddq_ctx* c, const uint8_t* state, const uint8_t* action,
                          const int16_t* reward, const uint8_t* nonterm, int64_t pool,
                          int64_t head, int64_t valid) {
  if (!c || !state || !action || !reward || !nonterm) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (c->lanes > 1)
    return fail(c, DDQ_ESTATE, "ddq_replay_fill_tiled on a laned ring (%d lanes)", c->lanes);
  const int64_t n = c->capacity;
  if (pool < 1 || pool > n) return fail(c, DDQ_EINVAL, "pool must be in [1, capacity]");
  if (head < 0 || head >= n || valid < 0 || valid > n)
    return fail(c, DDQ_EINVAL, "head/valid out of range");
  TRY(set_dev(c));
  const size_t slot = (size_t)4 * c->nb.S * c->nb.S;
  HIP_TRY(c, scopy(c, c->ring.state, state, slot * pool, hipMemcpyHostToDevice));
  if (pool < n)
    HIP_TRY(c, launch_tile(c->ring.state + slot * pool, c->ring.state, slot * pool,
                           slot * (n - pool), c->stream));
  std::vector<uint8_t> a(n), t(n);
  std::vector<int16_t> r(n);
  for (int64_t i = 0; i < n; ++i) {
    a[i] = action[i % pool]; r[i] = reward[i % pool]; t[i] = nonterm[i % pool];
  }
  HIP_TRY(c, scopy(c, c->ring.action, a.data(), n, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, c->ring.reward, r.data(), 2 * n, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, c->ring.nonterm, t.data(), n, hipMemcpyHostToDevice));
  c->head = head;
  c->valid = valid;
  TRY(push_meta(c));
  return prio_rebuild(c);
}

static int check_batch_out(ddq_ctx* c, int32_t n, const Minibatch& out) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!out.state || !out.action || !out.reward || !out.next_state || !out.nonterm)
    return fail(c, DDQ_EINVAL, "null output buffer");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (c->lanes > 1)
    return fail(c, DDQ_ESTATE, "the large-batch sampler does not read a laned ring (%d lanes)",
                c->lanes);
  if (n < 1) return fail(c, DDQ_EINVAL, "n must be >= 1");
  if ((int64_t)n * c->nb.S * c->nb.S >= (int64_t)1 << 31)
    return fail(c, DDQ_EINVAL, "n * S^2 must be < 2^31 (n=%d)", n);
  if (too_few_slots(c, n))   // n > A; n >= valid at nstep == 1
    return fail(c, DDQ_EINVAL, "Can't draw sample of size %d from replay dataset of size %lld",
                n, (long long)c->valid);
  return DDQ_OK;
}

int ddq_replay_sample_batch_async(ddq_ctx* c, int32_t n, uint64_t seed, int32_t* idx,
                                  float* state, float* action, float* reward, float* next_state,
                                  float* nonterm) {
  const Minibatch out{state, next_state, action, reward, nonterm};
  TRY(check_batch_out(c, n, out));
  if (!idx) return fail(c, DDQ_EINVAL, "null idx");
  if (2 * (int64_t)n > c->valid)
    return fail(c, DDQ_EINVAL, "batch sampler needs n <= valid/2 (n=%d, valid=%lld)", n,
                (long long)c->valid);
  TRY(guard(c));
  if (!c->r_bitmap) {   // sized for the full ring: valid never exceeds capacity
    const int64_t nblk = ((c->capacity + 31) / 32 + 1023) / 1024;
    TRY(dalloc(c, &c->r_bitmap, (size_t)nblk * 1024));
    TRY(dalloc(c, &c->r_blk, (size_t)nblk));
  }
  HIP_TRY(c, launch_sample_batch(c->ring.meta, c->valid, n, seed, c->batch_ctr++, c->r_bitmap,
                                 c->r_blk, idx, c->stream, c->nstep));
  HIP_TRY(c, launch_gather_nchw(c->ring, idx, n, c->nb.S, out, c->stream, c->nstep));
  return DDQ_OK;
}

int ddq_replay_gather_batch_async(ddq_ctx* c, const int32_t* idx, int32_t n, float* state,
                                  float* action, float* reward, float* next_state,
                                  float* nonterm) {
  const Minibatch out{state, next_state, action, reward, nonterm};
  TRY(check_batch_out(c, n, out));
  if (!idx) return fail(c, DDQ_EINVAL, "null idx");
  TRY(guard(c));
  HIP_TRY(c, launch_gather_nchw(c->ring, idx, n, c->nb.S, out, c->stream, c->nstep));
  return DDQ_OK;
}

int ddq_index_log_enable(ddq_ctx* c, int64_t draws) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (draws < 0 || draws > (1ll << 24)) return fail(c, DDQ_EINVAL, "draws must be in [0, 2^24]");
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // the ring restarts at the current draw: earlier draws (or entries of a
  // ring of another capacity) are never reported as logged
  ReplayMeta m;
  HIP_TRY(c, scopy(c, &m, c->ring.meta, sizeof(m), hipMemcpyDeviceToHost));
  c->log_first = (int64_t)m.counter;
  if (draws == 0) {
    c->nb.idx_log = nullptr;
    c->nb.log_cap = 0;
  } else if (draws > c->log_buf_cap) {
    TRY(dalloc(c, &c->log_buf, (size_t)draws * c->nb.B));
    c->log_buf_cap = draws;
    c->nb.idx_log = c->log_buf;
    c->nb.log_cap = draws;
  } else {
    c->nb.idx_log = c->log_buf;
    c->nb.log_cap = draws;
  }
  invalidate_graph(c);   // captured kernels hold the log pointer
  return DDQ_OK;
}

int ddq_replay_draws(ddq_ctx* c, int64_t* draws) {
  if (!c || !draws) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  TRY(set_dev(c));
  ReplayMeta m;
  HIP_TRY(c, hipMemcpyAsync(&m, c->ring.meta, sizeof(m), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *draws = (int64_t)m.counter;
  return DDQ_OK;
}

int ddq_index_log_read(ddq_ctx* c, int64_t first, int64_t n, int32_t* out) {
  if (!c || !out) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->nb.idx_log) return fail(c, DDQ_ESTATE, "index log not enabled");
  int64_t drawn = 0;
  TRY(ddq_replay_draws(c, &drawn));
  if (first < c->log_first || n < 0 || first + n > drawn || drawn - first > c->nb.log_cap)
    return fail(c, DDQ_EINVAL,
                "draws [%lld, %lld) not in the log (logged from draw %lld, drawn %lld, cap %lld)",
                (long long)first, (long long)(first + n), (long long)c->log_first,
                (long long)drawn, (long long)c->nb.log_cap);
  const int B = c->nb.B;
  for (int64_t d = first; d < first + n; ++d)
    HIP_TRY(c, hipMemcpyAsync(out + (d - first) * B, c->nb.idx_log + (d % c->nb.log_cap) * B,
                              (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_replay_status(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  TRY(set_dev(c));
  return check_err_flag(c);
}

int ddq_read_indices(ddq_ctx* c, int32_t* idx, int32_t batch) {
  if (!c || !idx || batch != c->nb.B) return fail(c, DDQ_EINVAL, "bad argument");
  TRY(set_dev(c));
  HIP_TRY(c, hipMemcpyAsync(idx, c->nb.mb.idx, batch * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_read_minibatch(ddq_ctx* c, float* state, float* action, float* reward, float* next_state,
                       float* nonterm) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(set_dev(c));
  const int B = c->nb.B, SS = c->nb.S * c->nb.S;
  std::vector<float> tmp((size_t)B * SS * 4);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int which = 0; which < 2; ++which) {
    float* dst = which ? next_state : state;
    if (!dst) continue;
    HIP_TRY(c, scopy(c, tmp.data(), which ? c->nb.mb.next_state : c->nb.mb.state, tmp.size() * 4,
                         hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
      for (int ch = 0; ch < 4; ++ch)
        for (int p = 0; p < SS; ++p)
          dst[((size_t)b * 4 + ch) * SS + p] = tmp[((size_t)b * SS + p) * 4 + ch];
  }
  if (action) HIP_TRY(c, scopy(c, action, c->nb.mb.action, B * 16, hipMemcpyDeviceToHost));
  if (reward) HIP_TRY(c, scopy(c, reward, c->nb.mb.reward, B * 4, hipMemcpyDeviceToHost));
  if (nonterm) HIP_TRY(c, scopy(c, nonterm, c->nb.mb.nonterm, B * 4, hipMemcpyDeviceToHost));
  return DDQ_OK;
}

int ddq_write_minibatch(ddq_ctx* c, const float* state, const float* action, const float* reward,
                        const float* next_state, const float* nonterm) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(set_dev(c));
  const int B = c->nb.B, SS = c->nb.S * c->nb.S;
  std::vector<float> tmp((size_t)B * SS * 4);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int which = 0; which < 2; ++which) {
    const float* src = which ? next_state : state;
    if (!src) continue;
    for (int b = 0; b < B; ++b)
      for (int ch = 0; ch < 4; ++ch)
        for (int p = 0; p < SS; ++p)
          tmp[((size_t)b * SS + p) * 4 + ch] = src[((size_t)b * 4 + ch) * SS + p];
    HIP_TRY(c, scopy(c, which ? c->nb.mb.next_state : c->nb.mb.state, tmp.data(), tmp.size() * 4,
                         hipMemcpyHostToDevice));
  }
  if (action) HIP_TRY(c, scopy(c, c->nb.mb.action, action, B * 16, hipMemcpyHostToDevice));
  if (reward) HIP_TRY(c, scopy(c, c->nb.mb.reward, reward, B * 4, hipMemcpyHostToDevice));
  if (nonterm) HIP_TRY(c, scopy(c, c->nb.mb.nonterm, nonterm, B * 4, hipMemcpyHostToDevice));
  if (c->nb.mb.isw) {   // a minibatch set directly has no draw: weights 1
    HIP_TRY(c, launch_fill_ones(c->nb.mb.isw, B, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->idx_bound = false;
  return DDQ_OK;
}

// ---------------- compute ----------------
// Double target (ddq_set_objective): Q(s',.) under theta_Q for the minibatch view
// the pass trains on, the pass's first launch group -- ddq_forward_q's kernels
// at n = B over nb.mb.next_state in the acting scratch (the actor, pool and
// evaluator are serial on the same stream), into the ctx's Qn_out buffer.  It
// depends on theta_Q and the bound view only: stream order after the previous
// step's apply is enough.  Profile names: "qn_<kernel>".
static void qn_mark(void* a, const char* name) {
  const std::string s = std::string("qn_") + name;
  (*reinterpret_cast<const Marks*>(a))(s.c_str());
}
static int enqueue_qn_forward(ddq_ctx* c, const NetBuffers& nb, Marks m) {
  if (nb.obj_target != DDQ_TARGET_DOUBLE) return DDQ_OK;
  const Marks qn = m.fn ? Marks{qn_mark, &m} : Marks{};
  HIP_TRY(c, launch_act(nb, nb.mb.next_state, nb.B, c->act_p3, c->act_h4, c->act_part, nb.qn_out,
                        nullptr, c->act_p1s, c->act_p2s, c->stream, qn));
  return DDQ_OK;
}

// The gradient launches of a step as sl.plan has them; fc4_done: the
// overlapped all-reduce's start, its argument the ctx (launch_backward).
// (one stream: forking the weight-gradient kernels onto a side stream cost
// more in cross-stream graph edges (6-14 us idle each, measured) than the
// overlap returned, as every kernel here fills the GPU on its own)
static int enqueue_fwd_bwd(ddq_ctx* c, const NetBuffers& nb, const StepLaunch& sl, Marks m = {},
                           Fc4Done fc4_done = {}, const NetBuffers* prio_next = nullptr,
                           uint64_t prio_seed = 0) {
  TRY(enqueue_qn_forward(c, nb, m));
  if (nb.small) {
    HIP_TRY(c, launch_small_fwd_head(nb, sl, c->stream, m));
  } else {
    HIP_TRY(c, launch_forward(nb, 2, c->stream, m, false));
    m("head");
    HIP_TRY(c, launch_head(nb, sl, c->stream));
  }
  // prioritized replay: right after the launch that wrote Q_sa and target_Q_sa,
  // one workgroup commits this step's |TD|, moves the counter on and, when a
  // next step is being prefetched, draws its index set and weights
  if (sl.plan.prio_commit) {
    m("prio_commit");
    HIP_TRY(c, launch_prio_commit_draw(nb, sl.meta, sl.plan.draw == Site::PrioCommit ? prio_next : nullptr,
                                       prio_seed, c->stream));
  }
  hipError_t e = nb.small ? launch_small_bwd(nb, sl, c->stream, m, fc4_done)
                          : launch_backward(nb, sl, c->stream, m, fc4_done);
  if (e != hipSuccess && !c->comm_err.empty()) {
    std::string m = c->comm_err;
    c->comm_err.clear();
    return fail(c, DDQ_ERCCL, "overlapped all-reduce: %s", m.c_str());
  }
  HIP_TRY(c, e);
  return DDQ_OK;
}

int ddq_forward_backward_async(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(guard(c));
  StepLaunch sl;
  sl.plan = plan_grad_only();
  return enqueue_fwd_bwd(c, c->nb, sl);
}

int ddq_forward_backward(ddq_ctx* c, float* loss) {
  TRY(ddq_forward_backward_async(c));
  if (loss) return copy_out(c, loss, c->nb.loss, 1, 0);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

// ---------------- selectable objective ----------------
int ddq_set_objective(ddq_ctx* c, const ddq_objective* o) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!o) return fail(c, DDQ_EINVAL, "null objective");
  if (o->target != DDQ_TARGET_MAX && o->target != DDQ_TARGET_DOUBLE)
    return fail(c, DDQ_EINVAL, "unknown target %d", o->target);
  if (o->loss != DDQ_LOSS_EUCLIDEAN && o->loss != DDQ_LOSS_HUBER)
    return fail(c, DDQ_EINVAL, "unknown loss %d", o->loss);
  if (o->loss == DDQ_LOSS_HUBER && !(std::isfinite(o->huber_delta) && o->huber_delta > 0.f))
    return fail(c, DDQ_EINVAL, "huber_delta must be finite and > 0 (got %g)", (double)o->huber_delta);
  if (o->reserved != 0) return fail(c, DDQ_EINVAL, "reserved must be 0");
  if (c->async_on)
    return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx: set the objective "
                               "before ddq_async_begin");
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);   // captured steps hold (or lack) the extra forward and the head's objective
  NetBuffers& nb = c->nb;
  if (o->target == DDQ_TARGET_DOUBLE) {
    if (!nb.qn_out) TRY(dalloc(c, &nb.qn_out, (size_t)nb.B * 4));
    // one run of the extra forward now: its kernels' function attributes are set
    // outside any capture (the result is overwritten by the first pass)
    HIP_TRY(c, launch_act(nb, nb.mb.next_state, nb.B, c->act_p3, c->act_h4, c->act_part, nb.qn_out,
                          nullptr, c->act_p1s, c->act_p2s, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  nb.obj_target = o->target;
  nb.obj_loss = o->loss;
  nb.huber_delta = o->loss == DDQ_LOSS_HUBER ? o->huber_delta : 0.f;
  return DDQ_OK;
}

int ddq_get_objective(const ddq_ctx* c, ddq_objective* o) {
  if (!c || !o) return fail(nullptr, DDQ_EINVAL, "null argument");
  *o = ddq_objective{c->nb.obj_target, c->nb.obj_loss, c->nb.huber_delta, 0};
  return DDQ_OK;
}

int ddq_forward_q(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(guard(c));
  HIP_TRY(c, launch_act(c->nb, c->nb.mb.state, c->nb.B, c->act_p3, c->act_h4, c->act_part,
                        c->nb.q_out, nullptr, c->act_p1s, c->act_p2s, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_read_blob(ddq_ctx* c, const char* name, float* dst, int64_t n) {
  if (!c || !name || !dst) return fail(c, DDQ_EINVAL, "null argument");
  const int B = c->nb.B;
  struct { const char* nm; float* p; int64_t cnt; } t[] = {
      {"Q_out", c->nb.q_out, 4ll * B}, {"P_out", c->nb.p_out, 4ll * B},
      {"Q_sa", c->nb.q_sa, B},         {"P_sa", c->nb.p_sa, B},
      {"target_Q_sa", c->nb.target, B}, {"loss", c->nb.loss, 1},
      {"Qn_out", c->nb.qn_out, 4ll * B}, {"Q_out.diff", c->nb.dqbuf, 4ll * B},
      {"is_weight", c->nb.mb.isw, B},       {"grad_norm", c->nb.gnorm, 1}};
  for (auto& e : t) {
    if (strcmp(e.nm, name) == 0) {
      if (n != e.cnt) return fail(c, DDQ_EINVAL, "blob %s has %lld elements", name, (long long)e.cnt);
      if (!strcmp(name, "grad_norm") && !(c->adam_on && c->nb.adam_clip > 0.f))
        return fail(c, DDQ_ESTATE, "blob grad_norm exists while Adam's gradient clipping is on");
      if (!strcmp(name, "Qn_out") && c->nb.obj_target != DDQ_TARGET_DOUBLE)
        return fail(c, DDQ_ESTATE, "blob Qn_out exists under the double target only");
      if (!strcmp(name, "is_weight") && !c->nb.mb.isw)
        return fail(c, DDQ_ESTATE, "blob is_weight exists while prioritized replay is on");
      TRY(set_dev(c));
      return copy_out(c, dst, e.p, n, 0);
    }
  }
  return fail(c, DDQ_EINVAL, "unknown blob '%s'", name);
}

int ddq_read_pool_mask(ddq_ctx* c, int32_t layer, uint8_t* dst, int64_t n) {
  if (!c || !dst) return fail(c, DDQ_EINVAL, "null argument");
  if (layer < 1 || layer > 3) return fail(c, DDQ_EINVAL, "layer must be 1..3");
  const int B = c->nb.B, C = layer == 1 ? 32 : 64, Hp = c->nb.S >> layer;
  const int64_t cnt = (int64_t)B * C * Hp * Hp;
  if (n != cnt) return fail(c, DDQ_EINVAL, "mask %d has %lld elements", layer, (long long)cnt);
  TRY(set_dev(c));
  std::vector<uint8_t> tmp(cnt);
  const uint8_t* src = layer == 1 ? c->nb.mask1 : (layer == 2 ? c->nb.mask2 : c->nb.mask3);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, scopy(c, tmp.data(), src, cnt, hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b)
    for (int ch = 0; ch < C; ++ch)
      for (int p = 0; p < Hp * Hp; ++p)
        dst[((size_t)b * C + ch) * Hp * Hp + p] = tmp[((size_t)b * Hp * Hp + p) * C + ch];
  return DDQ_OK;
}

int ddq_select_action(ddq_ctx* c, const uint8_t* states, int32_t n, int32_t* actions) {
  if (!c || !states || !actions) return fail(c, DDQ_EINVAL, "null argument");
  if (n < 1 || n > c->nb.B) return fail(c, DDQ_EINVAL, "n must be in [1,B]");
  TRY(guard(c));
  const size_t bytes = (size_t)n * 4 * c->nb.S * c->nb.S;
  HIP_TRY(c, hipMemcpyAsync(c->act_u8, states, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_u8_to_nhwc(c->act_u8, n, c->nb.S, c->act_in, c->stream));
  HIP_TRY(c, launch_act(c->nb, c->act_in, n, c->act_p3, c->act_h4, c->act_part, c->act_q,
                        c->act_out, c->act_p1s, c->act_p2s, c->stream));
  HIP_TRY(c, hipMemcpyAsync(actions, c->act_out, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

}  // extern "C"

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
static const char* actor_board_error(const int8_t* b) {
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

template <class Game>
static EnvIO env_io(const ddq_ctx* c, const EnvBufs<Game>& b) {
  return EnvIO{b.maps, b.in, c->nb.S, b.n};
}

static ActorRole actor_role(const ddq_ctx* c) { return ActorRole{c->a_env.games, c->ring}; }
static EvalRole eval_role(const ddq_ctx* c) {
  return EvalRole{c->e_env.games, c->e_log, c->e_max_moves, c->e_max_ep};
}
static PoolRole pool_role(const ddq_ctx* c) {
  return PoolRole{c->p_env.games, c->ring, c->lane_len, c->p_h0, c->p_v0};
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
  const hipError_t e = launch_env(role(c), env_io(c, *b), c->act_q, 0, 0, c->stream);
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
template <class Role, class Game>
static int env_move(ddq_ctx* c, const Role& r, const EnvBufs<Game>& b, uint64_t thresh) {
  HIP_TRY(c, launch_act(c->nb, b.in, b.n, c->act_p3, c->act_h4, c->act_part, c->act_q, nullptr,
                        c->act_p1s, c->act_p2s, c->stream));
  HIP_TRY(c, launch_env(r, env_io(c, b), c->act_q, thresh, 1, c->stream));
  return DDQ_OK;
}

extern "C" {

int ddq_actor_create(ddq_ctx* c, const int8_t* init_board, const int32_t* row_map,
                     const int32_t* col_map, uint64_t seed) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!init_board || !row_map || !col_map) return fail(c, DDQ_EINVAL, "null argument");
  std::vector<uint8_t> maps;
  TRY(env_pack_maps(c, row_map, col_map, &maps));
  TRY(env_check_boards(c, init_board, 1, true));
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->lanes > 1)
    return fail(c, DDQ_ESTATE, "ddq_actor_create on a laned ring (%d lanes): use ddq_actors_create",
                c->lanes);
  TRY(set_dev(c));
  // the one game's stream takes the seed verbatim
  const std::vector<ActorState> gs{env_new_game<ActorState>(seed, init_board)};
  return env_create(c, &c->a_env, 1, gs, maps, actor_role, "actor");
}

int ddq_actor_step_async(ddq_ctx* c, int32_t nsteps, int64_t iter_num) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->a_env.n) return fail(c, DDQ_ESTATE, "no actor (call ddq_actor_create)");
  if (nsteps < 1) return fail(c, DDQ_EINVAL, "nsteps must be >= 1 (got %d)", nsteps);
  TRY(guard(c));
  const uint64_t thresh = env_thresh(actor_epsilon(iter_num));
  const ActorRole r = actor_role(c);
  for (int i = 0; i < nsteps; ++i) TRY(env_move(c, r, c->a_env, thresh));
  // host mirror of the ring: one transition per step, as ddq_replay_add
  c->head = (c->head + nsteps) % c->capacity;
  c->valid = std::min(c->capacity, c->valid + nsteps);
  return DDQ_OK;
}

int ddq_actor_read(ddq_ctx* c, int8_t* boards, int64_t* stats) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->a_env.n) return fail(c, DDQ_ESTATE, "no actor (call ddq_actor_create)");
  TRY(set_dev(c));
  ActorState st;
  HIP_TRY(c, scopy(c, &st, c->a_env.games, sizeof(st), hipMemcpyDeviceToHost));
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
  c->e_env.n = 0;                    // before the log it plays into is replaced
  const size_t nlog = (size_t)ngames * max_episodes * 4;
  if (nlog > c->e_log_cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    dfree(c, c->e_log);
    c->e_log_cap = 0;
    TRY(dalloc(c, &c->e_log, nlog));
    c->e_log_cap = nlog;
  }
  HIP_TRY(c, hipMemsetAsync(c->e_log, 0, nlog * sizeof(int32_t), c->stream));
  c->e_max_moves = max_moves;
  c->e_max_ep = max_episodes;
  c->e_thresh = env_thresh(epsilon);   // epsilon = 0: no coin at all
  c->e_moves = 0;
  std::vector<EvalGame> gs(ngames);
  for (int g = 0; g < ngames; ++g)
    gs[g] = env_new_game<EvalGame>(env_game_seed(seed, g), init_boards + 100 * g);
  return env_create(c, &c->e_env, B, gs, maps, eval_role, "eval");
}

int ddq_eval_run_async(ddq_ctx* c, int32_t nmoves) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->e_env.n) return fail(c, DDQ_ESTATE, "no evaluator (call ddq_eval_create)");
  if (nmoves < 1) return fail(c, DDQ_EINVAL, "nmoves must be >= 1 (got %d)", nmoves);
  TRY(guard(c));
  const EvalRole r = eval_role(c);
  for (int i = 0; i < nmoves; ++i) TRY(env_move(c, r, c->e_env, c->e_thresh));
  c->e_moves += nmoves;
  return DDQ_OK;
}

int ddq_eval_read(ddq_ctx* c, int64_t* stats, int32_t* episodes, int32_t* log, int8_t* boards,
                  uint64_t* draws) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->e_env.n) return fail(c, DDQ_ESTATE, "no evaluator (call ddq_eval_create)");
  TRY(set_dev(c));
  const int n = c->e_env.n;
  std::vector<EvalGame> gs(n);
  HIP_TRY(c, scopy(c, gs.data(), c->e_env.games, gs.size() * sizeof(EvalGame),
                   hipMemcpyDeviceToHost));
  if (log)
    HIP_TRY(c, scopy(c, log, c->e_log, (size_t)n * c->e_max_ep * 4 * sizeof(int32_t),
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
  if (stats) { stats[0] = c->e_moves; stats[1] = eps; stats[2] = rew; stats[3] = dr; }
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
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (ngames != c->lanes)
    return fail(c, DDQ_EINVAL, "ngames %d != the ring's %d lanes (ddq_replay_set_lanes)", ngames,
                c->lanes);
  TRY(set_dev(c));
  // the games' slots come from the ring's per-lane head / valid now
  c->p_h0 = c->head;
  c->p_v0 = c->valid;
  c->p_moves = 0;
  std::vector<ActorState> gs(ngames);
  for (int g = 0; g < ngames; ++g)
    gs[g] = env_new_game<ActorState>(env_game_seed(seed, g), init_boards + 100 * g);
  return env_create(c, &c->p_env, B, gs, maps, pool_role, "pool");
}

int ddq_actors_step_async(ddq_ctx* c, int32_t nmoves, int64_t iter_num) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->p_env.n) return fail(c, DDQ_ESTATE, "no actor pool (call ddq_actors_create)");
  if (nmoves < 1) return fail(c, DDQ_EINVAL, "nmoves must be >= 1 (got %d)", nmoves);
  // the games' slots come from (h0, v0) and their own step counters
  if (c->head != (c->p_h0 + c->p_moves) % c->lane_len)
    return fail(c, DDQ_ESTATE, "the ring's head moved since ddq_actors_create: create the pool again");
  TRY(guard(c));
  const uint64_t thresh = env_thresh(actor_epsilon(iter_num));
  const PoolRole r = pool_role(c);
  for (int i = 0; i < nmoves; ++i) TRY(env_move(c, r, c->p_env, thresh));
  // host mirror of the ring: one transition per lane and move
  c->p_moves += nmoves;
  c->head = (c->head + nmoves) % c->lane_len;
  c->valid = std::min(c->lane_len, c->valid + nmoves);
  return DDQ_OK;
}

int ddq_actors_read(ddq_ctx* c, int8_t* boards, int64_t* stats, int64_t* totals) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->p_env.n) return fail(c, DDQ_ESTATE, "no actor pool (call ddq_actors_create)");
  TRY(set_dev(c));
  const int n = c->p_env.n;
  std::vector<ActorState> gs(n);
  HIP_TRY(c, scopy(c, gs.data(), c->p_env.games, gs.size() * sizeof(ActorState),
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

// ---------------- apply ----------------
static int check_cfg(ddq_ctx* c, const ddq_update_cfg* u) {
  if (!u) return fail(c, DDQ_EINVAL, "null update cfg");
  if (u->rule < 0 || u->rule > DDQ_RULE_ADAM)
    return fail(c, DDQ_EINVAL, "unknown update rule %d", u->rule);
  if (u->rule == DDQ_RULE_ADAM && !c->adam_on)
    return fail(c, DDQ_ESTATE, "DDQ_RULE_ADAM before ddq_set_adam");
  return DDQ_OK;
}

// The apply launch of one update (every caller of launch_apply).  Adam with
// clipping on: the gradient-norm launch first, over the buffer the apply reads
// (under all-reduce: the summed gradient).
static UpdateRule rule_of(const ddq_update_cfg& u, int period) {
  return UpdateRule{u.rule, period, u.lr, u.decay, u.eps, u.momentum, u.weight_decay};
}
static int enqueue_apply(ddq_ctx* c, const NetBuffers& nb, const StepLaunch& sl, Marks m = {}) {
  const bool adam = sl.u.rule == DDQ_RULE_ADAM;
  if (adam && nb.adam_clip > 0.f) {
    m("grad_norm");
    HIP_TRY(c, launch_grad_norm(nb, c->stream));
  }
  m(adam ? "adam_apply" : "apply");
  HIP_TRY(c, launch_apply(nb, sl, c->stream));
  return DDQ_OK;
}

int ddq_apply_async(ddq_ctx* c, const ddq_update_cfg* u) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(check_cfg(c, u));
  TRY(guard(c));
  StepLaunch sl;
  sl.plan = plan_apply_only();
  sl.u = rule_of(*u, 0);
  TRY(enqueue_apply(c, c->nb, sl));
  c->applied++;
  return DDQ_OK;
}

// ---------------- Adam ----------------
int ddq_set_adam(ddq_ctx* c, const ddq_adam_cfg* a) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!a) return fail(c, DDQ_EINVAL, "null adam cfg");
  if (!(a->beta1 >= 0.f && a->beta1 < 1.f) || !(a->beta2 >= 0.f && a->beta2 < 1.f))
    return fail(c, DDQ_EINVAL, "beta1 and beta2 must be in [0, 1) (got %g, %g)", (double)a->beta1,
                (double)a->beta2);
  if (!(std::isfinite(a->eps) && a->eps > 0.f))
    return fail(c, DDQ_EINVAL, "eps must be finite and > 0 (got %g)", (double)a->eps);
  if (!(std::isfinite(a->max_grad_norm) && a->max_grad_norm >= 0.f))
    return fail(c, DDQ_EINVAL, "max_grad_norm must be 0 (off) or finite and > 0 (got %g)",
                (double)a->max_grad_norm);
  if (c->async_on)
    return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx");
  TRY(set_dev(c));
  NetBuffers& nb = c->nb;
  if (!c->adam_on) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!nb.opt2) TRY(dalloc(c, &nb.opt2, (size_t)nb.L.total + kShardPad));
    if (!nb.gn_part) TRY(dalloc(c, &nb.gn_part, (size_t)kGnBlocks));
    if (!nb.gnorm) TRY(dalloc(c, &nb.gnorm, 1));
    c->adam_on = true;
  }
  invalidate_graph(c);   // captured steps hold the constants as launch arguments
  nb.adam_beta1 = a->beta1; nb.adam_beta2 = a->beta2;
  nb.adam_eps = a->eps; nb.adam_clip = a->max_grad_norm;
  return DDQ_OK;
}

int ddq_get_adam(const ddq_ctx* c, ddq_adam_cfg* a) {
  if (!c || !a) return fail(nullptr, DDQ_EINVAL, "null argument");
  if (!c->adam_on) return fail(nullptr, DDQ_ESTATE, "ddq_get_adam before ddq_set_adam");
  *a = ddq_adam_cfg{c->nb.adam_beta1, c->nb.adam_beta2, c->nb.adam_eps, c->nb.adam_clip};
  return DDQ_OK;
}

int ddq_adam_state(ddq_ctx* c, float* m, float* v, int64_t n, int64_t* t) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->adam_on) return fail(c, DDQ_ESTATE, "ddq_adam_state before ddq_set_adam");
  if ((m || v) && n != c->nb.L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (m) TRY(copy_out(c, m, c->nb.opt, n, 0));
  if (v) TRY(copy_out(c, v, c->nb.opt2, n, 0));
  if (t) HIP_TRY(c, scopy(c, t, c->nb.iter, 8, hipMemcpyDeviceToHost));
  return DDQ_OK;
}

int ddq_apply(ddq_ctx* c, const ddq_update_cfg* u) {
  TRY(ddq_apply_async(c, u));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_reset_optimizer(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(set_dev(c));
  HIP_TRY(c, hipMemsetAsync(c->nb.opt, 0, c->nb.L.total * 4, c->stream));
  if (c->nb.opt2) HIP_TRY(c, hipMemsetAsync(c->nb.opt2, 0, c->nb.L.total * 4, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->nb.opt_init, 0, 4, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->nb.iter, 0, 8, c->stream));
  c->applied = 0;
  c->steps = 0;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_get_optimizer_state(ddq_ctx* c, float* dst, int64_t n) {
  if (!c || !dst) return fail(c, DDQ_EINVAL, "null argument");
  if (n != c->nb.L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  TRY(set_dev(c));
  return copy_out(c, dst, c->nb.opt, n, 0);
}

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
  c->shard_len = ((P + (int64_t)W * 64 - 1) / ((int64_t)W * 64)) * 64;
  if (!c->cs) {
    HIP_TRY(c, hipStreamCreateWithFlags(&c->cs, hipStreamNonBlocking));
    for (auto& e : c->cev) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  // exchange buffers are allocated once for the largest W (kMaxRanks slices
  // of at most P/W + 64 floats fit in P + kShardPad ... per slice set)
  if (!c->gsl) TRY(dalloc(c, &c->gsl, (size_t)P + kShardPad));
  return DDQ_OK;
}

int ddq_comm_init(ddq_ctx* c, const uint8_t id[128], int32_t nranks, int32_t rank) {
  if (!c || !id) return fail(c, DDQ_EINVAL, "null argument");
  if (nranks < 1 || nranks > kMaxRanks || rank < 0 || rank >= nranks)
    return fail(c, DDQ_EINVAL, "bad rank/nranks (nranks <= %d)", kMaxRanks);
  if (c->local) return fail(c, DDQ_ESTATE, "ctx belongs to an in-process group");
  TRY(prio_refuse(c, "ddq_comm_init"));
  TRY(set_dev(c));
  if (c->comm) ncclCommDestroy(c->comm);
  c->comm = nullptr;
  ncclUniqueId u;
  memcpy(&u, id, 128);
  NCCL_TRY(c, ncclCommInitRank(&c->comm, nranks, u, rank));
  c->nranks = nranks;
  c->rank = rank;
  TRY(setup_shards(c, nranks));
  invalidate_graph(c);
  return DDQ_OK;
}

int ddq_allreduce_grads_async(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->comm) return fail(c, DDQ_ESTATE, "no communicator (call ddq_comm_init)");
  TRY(set_dev(c));
  NCCL_TRY(c, ncclAllReduce(c->nb.grad, c->nb.grad, (size_t)c->nb.L.total, ncclFloat, ncclSum,
                            c->comm, c->stream));
  return DDQ_OK;
}

int ddq_allreduce_grads(ddq_ctx* c) {
  TRY(ddq_allreduce_grads_async(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

// ---------------- step ----------------
static bool has_exchange(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  return cfg->exchange != DDQ_EXCHANGE_NONE && (c->comm != nullptr || c->local);
}
// param-server iterations one step consumes (server.py:200 INCR per gradient)
static int step_inc(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  return (has_exchange(c, cfg) &&
          (cfg->exchange == DDQ_EXCHANGE_SERVER || cfg->exchange == DDQ_EXCHANGE_ASYNC))
             ? c->nranks
             : 1;
}
// host mirrors of the device counters after n more steps
static void count_steps(ddq_ctx* c, const ddq_step_cfg* cfg, int n) {
  c->steps += n;
  c->applied += (int64_t)n * step_inc(c, cfg);
}
// the target period as the apply bookkeeping takes it (0: no P <- Q sync)
static int book_period(const ddq_step_cfg* cfg) {
  return cfg->target_period > 0 ? cfg->target_period : 0;
}
static bool is_async(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  return has_exchange(c, cfg) && cfg->exchange == DDQ_EXCHANGE_ASYNC;
}
// Once the async exchange began, the central model lives in the owners'
// shards: other step kinds would train a replica the owners never see.
static int check_not_async(ddq_ctx* c) {
  if (c->async_on)
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
  hipError_t e = hipEventRecord(c->cev[0], c->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(c->cs, c->cev[0], 0);
  if (e != hipSuccess) return e;
  ncclResult_t r = ncclAllReduce(c->nb.grad + L.w[3], c->nb.grad + L.w[3], (size_t)L.wn[3],
                                 ncclFloat, ncclSum, c->comm, c->cs);
  if (r != ncclSuccess) {
    c->comm_err = ncclGetErrorString(r);
    return hipErrorUnknown;
  }
  return hipEventRecord(c->cev[2], c->cs);
}

// What a step of (ctx, cfg) is, for plan_step.
static StepFacts step_facts(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  StepFacts f;
  const int ex = has_exchange(c, cfg) ? cfg->exchange : DDQ_EXCHANGE_NONE;
  f.small = c->nb.small;
  f.b_le_256 = c->nb.B <= 256;
  f.prio = c->nb.prio.leaf != nullptr;
  f.adam = cfg->update.rule == DDQ_RULE_ADAM;
  // (an Adam step's all-reduce is one call on the ctx stream: cfg->overlap is
  // for the fused fc4 apply, which Adam does not take)
  f.ex = ex == DDQ_EXCHANGE_ALLREDUCE
             ? (cfg->overlap && c->comm && !f.adam ? Exchange::AllReduceOverlap : Exchange::AllReduce)
         : ex == DDQ_EXCHANGE_SHARDED ? Exchange::Sharded
         : ex == DDQ_EXCHANGE_SERVER  ? Exchange::Server
         : ex == DDQ_EXCHANGE_ASYNC   ? Exchange::AsyncWorker
                                      : Exchange::None;
  f.fused_apply_ok = fused_apply_ok(c->nb.L);
  f.no_grad_store = (cfg->flags & DDQ_STEP_NO_GRAD_STORE) != 0;
  // (only the two-launch draw moved the counter on itself: enqueue_draw)
  f.holds_counter = c->prio_on || c->nb.B <= 256;
  // (the owners keep the async exchange's iteration)
  const bool worker = f.ex == Exchange::AsyncWorker;
  f.book_period = worker ? -1 : book_period(cfg);
  f.book_step = worker ? 1 : step_inc(c, cfg);
  return f;
}

// The plan of a step with these facts and what its launches need of the ctx.
static int plan_launches(ddq_ctx* c, const ddq_step_cfg* cfg, const StepFacts& f, StepLaunch* sl) {
  const char* why = "";
  if (!plan_step(f, &sl->plan, &why)) return fail(c, DDQ_ESTATE, "internal: %s", why);
  sl->u = rule_of(cfg->update, cfg->target_period);
  sl->meta = c->ring.meta;
  sl->fc4_wait = sl->plan.ext() ? c->cev[2] : nullptr;
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
        NCCL_TRY(c, ncclAllReduce(nb.grad, nb.grad, (size_t)L.w[3], ncclFloat, ncclSum, c->comm,
                                  c->stream));
        NCCL_TRY(c, ncclAllReduce(nb.grad + L.b[3], nb.grad + L.b[3], (size_t)(L.total - L.b[3]),
                                  ncclFloat, ncclSum, c->comm, c->stream));
        NCCL_TRY(c, ncclGroupEnd());
      } else if (overlap) {
        HIP_TRY(c, hipEventRecord(c->cev[0], c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->cs, c->cev[0], 0));
        NCCL_TRY(c, ncclGroupStart());
        NCCL_TRY(c, ncclAllReduce(nb.grad, nb.grad, (size_t)L.w[3], ncclFloat, ncclSum, c->comm,
                                  c->cs));
        NCCL_TRY(c, ncclAllReduce(nb.grad + L.b[3], nb.grad + L.b[3], (size_t)(L.total - L.b[3]),
                                  ncclFloat, ncclSum, c->comm, c->cs));
        NCCL_TRY(c, ncclGroupEnd());
        HIP_TRY(c, hipEventRecord(c->cev[1], c->cs));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->cev[1], 0));
      } else {
        NCCL_TRY(c, ncclAllReduce(nb.grad, nb.grad, (size_t)L.total, ncclFloat, ncclSum, c->comm,
                                  c->stream));
      }
    }
    return enqueue_apply(c, nb, sl, m);
  }
  const int W = c->nranks;
  const size_t len = (size_t)c->shard_len;
  m(ex == DDQ_EXCHANGE_SHARDED ? "reduce_scatter" : "all_to_all");
  if (ex == DDQ_EXCHANGE_SHARDED)
    NCCL_TRY(c, ncclReduceScatter(nb.grad, c->gsl, len, ncclFloat, ncclSum, c->comm, c->stream));
  else if (W > 1) {
    // all-to-all without the rank's own slice: the owner apply reads that one
    // in place from nb.grad (no self copy of len floats through RCCL)
    NCCL_TRY(c, ncclGroupStart());
    for (int p = 0; p < W; ++p) {
      if (p == c->rank) continue;
      NCCL_TRY(c, ncclSend(nb.grad + (size_t)p * len, len, ncclFloat, p, c->comm, c->stream));
      NCCL_TRY(c, ncclRecv(c->gsl + (size_t)p * len, len, ncclFloat, p, c->comm, c->stream));
    }
    NCCL_TRY(c, ncclGroupEnd());
  }
  m("apply_shard");
  ShardOpts o;
  if (sl.plan.gather == Site::OwnerApply) o.pre = sl.next;
  o.refresh_own = -1;
  o.own_w = c->rank;
  o.own_g = ex == DDQ_EXCHANGE_SHARDED ? nullptr : nb.grad + (size_t)c->rank * len;
  HIP_TRY(c, launch_apply_shard(nb, sl.u, c->gsl, (int64_t)c->rank * len, (int64_t)len,
                                (int64_t)len, ex == DDQ_EXCHANGE_SHARDED ? 1 : W, c->stream, o));
  m("all_gather");
  NCCL_TRY(c, ncclAllGather(nb.theta[0] + (size_t)c->rank * len, nb.theta[0], len, ncclFloat,
                            c->comm, c->stream));
  // the owner's shard was refreshed by its apply: the other ranks' shards
  // only (no launch when one rank owns every parameter)
  m("refresh");
  HIP_TRY(c, launch_refresh(nb, c->stream, -1, (int64_t)c->rank * len,
                            (int64_t)(c->rank + 1) * len));
  return DDQ_OK;
}

// The draw of a minibatch and its gather into nb's set, on `stream`.
static int enqueue_draw(ddq_ctx* c, const NetBuffers& nb, uint64_t seed, hipStream_t stream,
                        Marks m = {}) {
  if (c->prio_on) {   // one workgroup descends the sum tree, then the plain gather
    m("prio_sample");
    HIP_TRY(c, launch_prio_sample(nb, c->ring.meta, seed, stream));
    m("gather");
    HIP_TRY(c, launch_gather(nb, c->ring, stream));
  } else if (nb.B <= 256) {   // one kernel: every gather workgroup draws the same index set
    m("sample_gather");
    HIP_TRY(c, launch_sample_gather(nb, c->ring, seed, stream));
  } else {
    m("sample");
    HIP_TRY(c, launch_sample(nb, c->ring.meta, seed, stream));
    m("gather");
    HIP_TRY(c, launch_gather(nb, c->ring, stream));
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
    pf = make_prefetch(*pre, c->ring, cfg->seed);
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
  if (c->mon.ring && c->mon_period > 0) {
    m("monitor");
    HIP_TRY(c, launch_monitor(c->mon, c->mon_period, -1, c->stream));
  }
  return DDQ_OK;
}

static int enqueue_step(ddq_ctx* c, const ddq_step_cfg* cfg, Marks m = {}, bool fault = false) {
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
static int initial_target_sync(ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (cfg->target_period > 0 && c->applied % cfg->target_period == 0) {
    HIP_TRY(c, hipMemcpyAsync(c->nb.theta[1], c->nb.theta[0], c->nb.L.total * 4,
                              hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->nb.wks[1], c->nb.wks[0], c->nb.L.wks_total * 3 * 2,
                              hipMemcpyDeviceToDevice, c->stream));
  }
  return DDQ_OK;
}

static int check_step(ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!cfg) return fail(c, DDQ_EINVAL, "null step cfg");
  TRY(not_restoring(c));   // (every step kind, the group's and the async ones)
  TRY(check_cfg(c, &cfg->update));
  if (!c->ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (too_few_slots(c, c->nb.B))
    return fail(c, DDQ_EINVAL, "Can't draw sample of size %d from replay dataset of size %lld",
                c->nb.B, (long long)(c->lanes * c->valid));
  if (cfg->exchange < DDQ_EXCHANGE_NONE || cfg->exchange > DDQ_EXCHANGE_ASYNC)
    return fail(c, DDQ_EINVAL, "unknown exchange %d", cfg->exchange);
  if (cfg->flags & ~DDQ_STEP_NO_GRAD_STORE)
    return fail(c, DDQ_EINVAL, "unknown step flags 0x%x", (unsigned)cfg->flags);
  if (cfg->exchange != DDQ_EXCHANGE_NONE && c->nranks > 1 && !c->comm && !c->local)
    return fail(c, DDQ_ESTATE, "no communicator");
  if (has_exchange(c, cfg)) TRY(prio_refuse(c, "an exchanged step"));
  if (cfg->update.rule == DDQ_RULE_ADAM && has_exchange(c, cfg) &&
      cfg->exchange != DDQ_EXCHANGE_ALLREDUCE)
    return fail(c, DDQ_EINVAL, "DDQ_RULE_ADAM runs without an exchange or under "
                               "DDQ_EXCHANGE_ALLREDUCE only (exchange %d shards one state buffer)",
                cfg->exchange);
  if (c->nb.target_tau < 1.f && is_async(c, cfg))
    return fail(c, DDQ_EINVAL, "soft target updates (tau %g < 1) with DDQ_EXCHANGE_ASYNC: its P "
                               "travels by pulls, not by the steps' syncs",
                (double)c->nb.target_tau);
  return DDQ_OK;
}

// Single-ctx steps while the monitor records every period-th step: the record
// needs the step's whole gradient in the buffer and the ctx's own iteration.
static int check_monitor_step(ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (!c->mon.ring || c->mon_period <= 0) return DDQ_OK;
  if (cfg->flags & DDQ_STEP_NO_GRAD_STORE)
    return fail(c, DDQ_EINVAL, "DDQ_STEP_NO_GRAD_STORE while the monitor records steps (period %d): "
                               "fc4's gradient block in the buffer would be an earlier step's",
                c->mon_period);
  if (is_async(c, cfg))
    return fail(c, DDQ_ESTATE, "the async exchange takes no monitor records: disable the monitor or "
                               "enable it with period 0");
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
  HIP_TRY(c, hipEventRecord(c->grad_ev, c->stream));
  c->ready_seen = false;
  c->grad_ev_captured = c->acapture;
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
  if (!c->own) TRY(dalloc(c, &c->own, (size_t)P + kShardPad));
  if (!c->pown) TRY(dalloc(c, &c->pown, (size_t)P + kShardPad));
  if (!c->grad_ev) {
    HIP_TRY(c, hipEventCreateWithFlags(&c->grad_ev, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->tick_ev, hipEventDisableTiming));
  }
  TRY(initial_target_sync(c, cfg));
  HIP_TRY(c, hipMemcpyAsync(c->own, c->nb.theta[0], P * 4, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->pown, c->nb.theta[1], P * 4, hipMemcpyDeviceToDevice, c->stream));
  c->last_pull.assign(c->nranks, c->applied);
  c->async_on = true;
  // the owner duties run on the comm stream: it starts after the copies
  HIP_TRY(c, hipEventRecord(c->cev[0], c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->cs, c->cev[0], 0));
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
  const int64_t L = c->shard_len, off = (int64_t)c->rank * L;
  // (the apply kernel indexes the gradient slice from the shard's start)
  const float* g = own ? c->nb.grad + off : c->gsl;
  Prefetch pf{};
  if (draw) pf = make_prefetch(c->nb, c->ring, cfg->seed);
  ShardOpts o;
  o.theta = c->own;
  o.first = c->applied == 0 ? 1 : 0;
  o.pre = draw ? &pf : nullptr;
  o.mirror = own ? c->nb.theta[0] : nullptr;
  o.refresh_own = own ? (async_p_now(cfg, it) ? 2 : 1) : 0;
  HIP_TRY(c, launch_apply_shard(c->nb, rule_of(u, 0), g, off, L, L, 1, c->cs, o));
  if (async_p_now(cfg, it))
    HIP_TRY(c, hipMemcpyAsync(c->pown + off, c->own + off, L * 4, hipMemcpyDeviceToDevice, c->cs));
  return DDQ_OK;
}

// Worker side after its pull (theta[0], and theta[1] when pull_p, hold the
// central model; the ctx stream waited for them): kernel layouts of Q (and
// P), then the next gradient.  own: the worker's own shard was refreshed by
// its owner apply (Q; P too when this tick updated the central P: p_own).
static int async_after_pull(ddq_ctx* c, const ddq_step_cfg* cfg, bool pull_p, bool own = false,
                            bool p_own = false, bool drawn = false) {
  const int64_t lo = own ? (int64_t)c->rank * c->shard_len : 0;
  const int64_t hi = own ? lo + c->shard_len : 0;
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
  c->last_pull[w] = it;
  c->async_ticks++;
}

// One tick over RCCL (worker w pushes): point-to-point pushes / pulls and the
// owner apply on the comm stream, the pulling worker's next gradient on its
// ctx stream -- it overlaps the later ticks' owner duties.
static int rccl_async_tick(ddq_ctx* c, const ddq_step_cfg* cfg, int w) {
  const int W = c->nranks, r = c->rank;
  const int64_t L = c->shard_len;
  NetBuffers& nb = c->nb;
  const int64_t it = c->applied + 1;    // iteration after this tick's apply
  const bool pull_p = async_pull_p(cfg, c->last_pull[w], it);
  // the own push's owner apply draws + gathers this worker's next minibatch:
  // it follows everything on the ctx stream so far (the gradient, and any
  // replay insert enqueued since), not only grad_ev
  const bool draw = r == w && nb.B <= 256;
  if (draw) {
    HIP_TRY(c, hipEventRecord(c->cev[0], c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->cs, c->cev[0], 0));
  } else if (r == w && (!c->acapture || c->grad_ev_captured)) {
    HIP_TRY(c, hipStreamWaitEvent(c->cs, c->grad_ev, 0));
  }
  // push: worker w's gradient slices to their owners
  if (W > 1) {
    NCCL_TRY(c, ncclGroupStart());
    if (r == w) {
      for (int j = 0; j < W; ++j)
        if (j != r) NCCL_TRY(c, ncclSend(nb.grad + (size_t)j * L, L, ncclFloat, j, c->comm, c->cs));
    } else {
      NCCL_TRY(c, ncclRecv(c->gsl, L, ncclFloat, w, c->comm, c->cs));
    }
    NCCL_TRY(c, ncclGroupEnd());
  }
  TRY(async_owner_apply(c, cfg, it, r == w, draw));
  // pull: the owners' shards to worker w
  if (W > 1) {
    NCCL_TRY(c, ncclGroupStart());
    if (r != w) {
      NCCL_TRY(c, ncclSend(c->own + (size_t)r * L, L, ncclFloat, w, c->comm, c->cs));
      if (pull_p) NCCL_TRY(c, ncclSend(c->pown + (size_t)r * L, L, ncclFloat, w, c->comm, c->cs));
    } else {
      for (int j = 0; j < W; ++j) {
        if (j == r) continue;
        NCCL_TRY(c, ncclRecv(nb.theta[0] + (size_t)j * L, L, ncclFloat, j, c->comm, c->cs));
        if (pull_p)
          NCCL_TRY(c, ncclRecv(nb.theta[1] + (size_t)j * L, L, ncclFloat, j, c->comm, c->cs));
      }
    }
    NCCL_TRY(c, ncclGroupEnd());
  }
  if (r == w) {   // (the own shard of theta[0]: written by the owner apply;
                  // of theta[1] too when this tick updated the central P)
    const bool p_own = async_p_now(cfg, it);
    if (pull_p && !p_own)
      HIP_TRY(c, hipMemcpyAsync(nb.theta[1] + (size_t)r * L, c->pown + (size_t)r * L, L * 4,
                                hipMemcpyDeviceToDevice, c->cs));
    HIP_TRY(c, hipEventRecord(c->tick_ev, c->cs));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->tick_ev, 0));
    TRY(async_after_pull(c, cfg, pull_p, true, p_own, draw));
  }
  async_advance(c, w, it);
  return DDQ_OK;
}

// the ctx stream waits for the comm stream's owner duties so far
static int async_join(ddq_ctx* c) {
  HIP_TRY(c, hipEventRecord(c->cev[1], c->cs));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->cev[1], 0));
  return DDQ_OK;
}

static int async_prepare(ddq_ctx* c, const ddq_step_cfg* cfg) {
  if (c->local) return fail(c, DDQ_ESTATE, "in-process group members step with ddq_group_step");
  if (!c->cs) TRY(setup_shards(c, c->nranks));
  if (!c->async_on) TRY(async_begin(c, cfg));
  return DDQ_OK;
}

// One round-robin round (W ticks, worker 0 .. W-1): a step of the async exchange.
static int rccl_async_round(ddq_ctx* c, const ddq_step_cfg* cfg) {
  for (int w = 0; w < c->nranks; ++w) TRY(rccl_async_tick(c, cfg, w));
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
  if (c->mon.ring && c->mon_period > 0)
    return fail(c, DDQ_ESTATE, "the async exchange takes no monitor records: disable the monitor or "
                               "enable it with period 0");
  TRY(set_dev(c));
  return async_prepare(c, cfg);
}

// Is this worker's gradient pushable: computed (grad_ev), and -- for an
// emulated straggler -- straggle_us of host time since that was first seen.
static int grad_ready(ddq_ctx* c, bool* ready) {
  const hipError_t e = hipEventQuery(c->grad_ev);
  if (e != hipSuccess && e != hipErrorNotReady)
    return fail(c, DDQ_EHIP, "hipEventQuery: %s", hipGetErrorString(e));
  *ready = false;
  if (e != hipSuccess) return DDQ_OK;
  const auto now = std::chrono::steady_clock::now();
  if (!c->ready_seen) {
    c->ready_seen = true;
    c->ready_at = now;
  }
  *ready = now - c->ready_at >= std::chrono::microseconds(c->straggle_us);
  return DDQ_OK;
}

int ddq_async_ready(ddq_ctx* c, int32_t* ready) {
  if (!c || !ready) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->async_on) return fail(c, DDQ_ESTATE, "async exchange not begun (ddq_async_begin)");
  TRY(set_dev(c));
  bool r = false;
  TRY(grad_ready(c, &r));
  *ready = r ? 1 : 0;
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
    ticks = c->async_ticks;
    last = c->last_pull;
    c->acapture = true;
    c->grad_ev_captured = false;
  }
  ~AsyncCapture() {
    if (!what) return;
    c->acapture = false;
    c->applied = applied;
    c->async_ticks = ticks;
    c->last_pull = last;
  }
  int fork() const {
    if (!what) return DDQ_OK;
    hipError_t e = hipEventRecord(c->cev[0], c->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->cs, c->cev[0], 0);
    if (e != hipSuccess) return fail(c, DDQ_EHIP, "%s fork: %s", what, hipGetErrorString(e));
    return DDQ_OK;
  }
};

// `body`'s launches on the ctx stream as one instantiated, uploaded exec.
static int capture_exec(ddq_ctx* c, hipGraphExec_t* out, const std::function<int()>& body,
                        const char* async_what = nullptr) {
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
  return capture_exec(c, &t.exec[key], [&] { return rccl_async_tick(c, cfg, c->rank); },
                      "tick graph");
}

int ddq_async_tick(ddq_ctx* c, const ddq_step_cfg* cfg, int32_t worker) {
  TRY(check_step(c, cfg));
  if (cfg->exchange != DDQ_EXCHANGE_ASYNC) return fail(c, DDQ_EINVAL, "cfg exchange is not async");
  if (worker < 0 || worker >= c->nranks)
    return fail(c, DDQ_EINVAL, "worker %d out of [0, %d)", worker, c->nranks);
  TRY(set_dev(c));
  TRY(async_prepare(c, cfg));
  c->rr_rounds = 0;   // the round-robin graph's steady state no longer holds
  // this rank's own ticks (the heavy ones: its next gradient) replay a graph;
  // the other workers' ticks (a receive, the owner apply, a send) stay eager
  if (worker == c->rank && c->applied > 0) {
    const int64_t it = c->applied + 1;
    const bool pull_p = async_pull_p(cfg, c->last_pull[worker], it);
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
  int a = c->nranks, b = cfg->target_period;
  while (b) { const int t = a % b; a = b; b = t; }
  return cfg->target_period / a;
}

static int64_t async_phase(const ddq_ctx* c, const ddq_step_cfg* cfg) {
  return cfg->target_period > 0 ? c->applied % cfg->target_period : 0;
}

static int async_round_eager(ddq_ctx* c, const ddq_step_cfg* cfg) {
  TRY(rccl_async_round(c, cfg));
  c->steps++;
  c->rr_rounds++;
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
  HIP_TRY(c, hipEventRecord(c->cev[0], c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->cs, c->cev[0], 0));
  HIP_TRY(c, hipEventRecord(c->grad_ev, c->stream));
  c->ready_seen = false;
  c->grad_ev_captured = false;
  return DDQ_OK;
}

static int async_graph_steps(ddq_ctx* c, const ddq_step_cfg* cfg, int nsteps) {
  TRY(async_prepare(c, cfg));
  const int K = async_graph_rounds(c, cfg);
  int i = 0;
  if (K > kAsyncGraphMaxRounds) {
    for (; i < nsteps; ++i) TRY(async_round_eager(c, cfg));
    return DDQ_OK;
  }
  while (i < nsteps) {
    const bool steady = c->rr_rounds >= 1;
    if (steady && nsteps - i >= K &&
        (!c->graphs.round.holds(cfg) || async_phase(c, cfg) == c->graphs.round.phase)) {
      TRY(ensure_async_graph(c, cfg, K));
      HIP_TRY(c, hipGraphLaunch(c->graphs.round.exec[0], c->stream));
      TRY(after_async_graph(c));
      for (int k = 0; k < K; ++k)
        for (int w = 0; w < c->nranks; ++w) async_advance(c, w, c->applied + 1);
      c->steps += K;
      c->rr_rounds += K;
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
  c->straggle_us = usec;
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
  c->idx_bound = true;
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
  if (nsteps > 0) c->idx_bound = true;
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
    mb_bind_weights(c, c->prio_on);
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
  c->idx_bound = true;
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

// ---------------- in-process groups ----------------
int ddq_group_init(ddq_ctx** ctxs, int32_t W) {
  if (!ctxs || W < 1 || W > kMaxRanks) return fail(nullptr, DDQ_EINVAL, "bad group");
  for (int r = 0; r < W; ++r) {
    ddq_ctx* c = ctxs[r];
    if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx in group");
    if (c->comm) return fail(c, DDQ_ESTATE, "ctx already has an RCCL communicator");
    TRY(prio_refuse(c, "ddq_group_init"));
    if (c->nb.S != ctxs[0]->nb.S || c->nb.B != ctxs[0]->nb.B)
      return fail(c, DDQ_EINVAL, "group members must share batch and frame");
  }
  for (int r = 0; r < W; ++r) {
    ddq_ctx* c = ctxs[r];
    TRY(set_dev(c));
    c->local = true;
    c->nranks = W;
    c->rank = r;
    TRY(setup_shards(c, W));
    if (!c->gstage) TRY(dalloc(c, &c->gstage, (size_t)W * (c->nb.L.total + kShardPad)));
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
  const int64_t L = ctxs[0]->shard_len;
  const int64_t it = ctxs[0]->applied + 1;
  const bool pull_p = async_pull_p(cfg, ctxs[0]->last_pull[w], it);
  for (int r = 0; r < W; ++r) {
    ddq_ctx* c = ctxs[r];
    TRY(set_dev(c));
    HIP_TRY(c, hipStreamWaitEvent(c->cs, cw->grad_ev, 0));
    HIP_TRY(c, hipMemcpyAsync(c->gsl, cw->nb.grad + (size_t)r * L, L * 4,
                              hipMemcpyDeviceToDevice, c->cs));
    TRY(async_owner_apply(c, cfg, it, false));
    HIP_TRY(c, hipMemcpyAsync(cw->nb.theta[0] + (size_t)r * L, c->own + (size_t)r * L, L * 4,
                              hipMemcpyDeviceToDevice, c->cs));
    if (pull_p)
      HIP_TRY(c, hipMemcpyAsync(cw->nb.theta[1] + (size_t)r * L, c->pown + (size_t)r * L, L * 4,
                                hipMemcpyDeviceToDevice, c->cs));
    HIP_TRY(c, hipEventRecord(c->tick_ev, c->cs));
  }
  TRY(set_dev(cw));
  for (int r = 0; r < W; ++r) HIP_TRY(cw, hipStreamWaitEvent(cw->stream, ctxs[r]->tick_ev, 0));
  TRY(async_after_pull(cw, cfg, pull_p));
  for (int r = 0; r < W; ++r) async_advance(ctxs[r], w, it);
  return DDQ_OK;
}

static int group_async_prepare(ddq_ctx** ctxs, int W, const ddq_step_cfg* cfg) {
  for (int r = 0; r < W; ++r) {
    if (ctxs[r]->async_on) continue;
    TRY(set_dev(ctxs[r]));
    TRY(async_begin(ctxs[r], cfg));
  }
  return DDQ_OK;
}

static int group_sync_all(ddq_ctx** ctxs, int W) {
  for (int r = 0; r < W; ++r) {
    ddq_ctx* c = ctxs[r];
    TRY(set_dev(c));
    HIP_TRY(c, hipStreamSynchronize(c->cs));
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
    if (!c || !c->local || c->nranks != W || c->rank != r)
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
      const int64_t len = c->shard_len;
      if (ex == DDQ_EXCHANGE_NONE) {
        TRY(enqueue_apply(c, nb, sl[r]));
        continue;
      }
      if (ex == DDQ_EXCHANGE_ALLREDUCE) {   // gather every gradient first (summed below)
        for (int j = 0; j < W; ++j)
          HIP_TRY(c, hipMemcpyAsync(c->gstage + (size_t)j * P, ctxs[j]->nb.grad, P * 4,
                                    hipMemcpyDeviceToDevice, c->stream));
        continue;
      }
      for (int j = 0; j < W; ++j)
        HIP_TRY(c, hipMemcpyAsync(c->gsl + (size_t)j * len, ctxs[j]->nb.grad + (size_t)r * len,
                                  len * 4, hipMemcpyDeviceToDevice, c->stream));
      int nsl = W;
      if (ex == DDQ_EXCHANGE_SHARDED) {
        HIP_TRY(c, launch_sum_slices(c->gsl, c->gsl, W, len, len, c->stream));
        nsl = 1;
      }
      HIP_TRY(c, launch_apply_shard(nb, sl[r].u, c->gsl, (int64_t)r * len, len, len, nsl, c->stream));
    }
    if (ex == DDQ_EXCHANGE_ALLREDUCE) {
      TRY(record_all());       // every member holds all W gradients: sum in rank order, apply
      for (int r = 0; r < W; ++r) {
        ddq_ctx* c = ctxs[r];
        TRY(set_dev(c));
        TRY(wait_all(c));
        HIP_TRY(c, launch_sum_slices(c->nb.grad, c->gstage, W, P, P, c->stream));
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
        const int64_t len = c->shard_len;
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

int64_t ddq_step_count(const ddq_ctx* c) { return c ? c->steps : -1; }

// ---------------- training monitor ----------------
static void monitor_release(ddq_ctx* c) {
  MonitorEnv& m = c->mon;
  MonitorChunk* ch = const_cast<MonitorChunk*>(m.chunks);
  MonitorBlob* bl = const_cast<MonitorBlob*>(m.blobs);
  dfree(c, ch);
  dfree(c, bl);
  dfree(c, m.psum);
  dfree(c, m.pnf);
  dfree(c, m.ticket);
  dfree(c, m.count);
  dfree(c, m.ring);
  m = MonitorEnv{};
  c->mon_period = 0;
}

int ddq_monitor_enable(ddq_ctx* c, int64_t capacity, int32_t period) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (capacity < 0 || capacity > (1ll << 24))
    return fail(c, DDQ_EINVAL, "capacity must be in [0, 2^24] (got %lld)", (long long)capacity);
  if (period < 0) return fail(c, DDQ_EINVAL, "period must be >= 0 (got %d)", period);
  if (period > 0 && capacity > 0 && c->async_on)
    return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx: it takes no monitor "
                               "records of its own (period must be 0)");
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);   // captured steps hold (or lack) the monitor launch
  monitor_release(c);
  if (capacity == 0) return DDQ_OK;
  // chunk table: (tensor, blob) major, offset minor; no chunk straddles a blob
  const ParamLayout& L = c->nb.L;
  std::vector<MonitorChunk> chunks;
  std::vector<MonitorBlob> blobs(kMonBlobs);
  for (int t = 0; t < 3; ++t)
    for (int l = 0; l < 5; ++l)
      for (int i = 0; i < 2; ++i) {
        const int64_t off = i ? L.b[l] : L.w[l], cnt = i ? L.bn[l] : L.wn[l];
        if ((off | cnt) & 3)   // the kernel's float4 path (it has a scalar one: slow, not wrong)
          return fail(c, DDQ_ESTATE, "monitor: blob %d.%d at %lld + %lld is no multiple of 4 floats",
                      l, i, (long long)off, (long long)cnt);
        MonitorBlob& b = blobs[t * 10 + 2 * l + i];
        b.first = (int32_t)chunks.size();
        b.count = cnt;
        for (int64_t o = 0; o < cnt; o += kMonChunk)
          chunks.push_back({t, 2 * l + i, (uint32_t)(off + o),
                            (int32_t)std::min<int64_t>(kMonChunk, cnt - o)});
        b.n = (int32_t)chunks.size() - b.first;
      }
  MonitorEnv m{};
  m.nchunks = (int)chunks.size();
  MonitorChunk* dch = nullptr;
  MonitorBlob* dbl = nullptr;
  const int rc = [&]() -> int {
    TRY(dalloc(c, &dch, chunks.size()));
    m.chunks = dch;
    TRY(dalloc(c, &dbl, blobs.size()));
    m.blobs = dbl;
    TRY(dalloc(c, &m.psum, chunks.size()));
    TRY(dalloc(c, &m.pnf, chunks.size()));
    TRY(dalloc(c, &m.ticket, 4));
    TRY(dalloc(c, &m.count, 2));
    TRY(dalloc(c, &m.ring, (size_t)capacity));
    HIP_TRY(c, scopy(c, dch, chunks.data(), chunks.size() * sizeof(MonitorChunk),
                     hipMemcpyHostToDevice));
    HIP_TRY(c, scopy(c, dbl, blobs.data(), blobs.size() * sizeof(MonitorBlob),
                     hipMemcpyHostToDevice));
    return DDQ_OK;
  }();
  m.t[0] = c->nb.theta[0];
  m.t[1] = c->nb.theta[1];
  m.t[2] = c->nb.grad;
  m.capacity = capacity;
  m.iter = c->nb.iter;
  m.loss = c->nb.loss;
  m.q_out = c->nb.q_out;
  m.B = c->nb.B;
  c->mon = m;
  if (rc != DDQ_OK) {
    const std::string msg = c->err;
    monitor_release(c);
    c->err = msg;
    return rc;
  }
  c->mon_period = period;
  return DDQ_OK;
}

int ddq_monitor_record_async(ddq_ctx* c, int64_t tag) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->mon.ring) return fail(c, DDQ_ESTATE, "monitor not enabled (ddq_monitor_enable)");
  TRY(set_dev(c));
  HIP_TRY(c, launch_monitor(c->mon, 0, tag, c->stream));
  return DDQ_OK;
}

int ddq_monitor_read(ddq_ctx* c, int64_t first, int64_t n, ddq_monitor_record* out,
                     int64_t* total) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->mon.ring) return fail(c, DDQ_ESTATE, "monitor not enabled (ddq_monitor_enable)");
  if (n < 0 || (n > 0 && !out)) return fail(c, DDQ_EINVAL, "bad argument");
  TRY(set_dev(c));
  int64_t cnt = 0;
  HIP_TRY(c, scopy(c, &cnt, c->mon.count, sizeof(cnt), hipMemcpyDeviceToHost));
  if (total) *total = cnt;
  if (n == 0) return DDQ_OK;
  const int64_t cap = c->mon.capacity;
  if (first < 0 || first + n > cnt || cnt - first > cap)
    return fail(c, DDQ_EINVAL, "records [%lld, %lld) not in the ring (taken %lld, capacity %lld)",
                (long long)first, (long long)(first + n), (long long)cnt, (long long)cap);
  for (int64_t k = first; k < first + n;) {   // at most two spans of the ring
    const int64_t slot = k % cap, run = std::min(first + n - k, cap - slot);
    HIP_TRY(c, hipMemcpyAsync(out + (k - first), c->mon.ring + slot,
                              (size_t)run * sizeof(MonitorRecord), hipMemcpyDeviceToHost,
                              c->stream));
    k += run;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

// ---------------- measurement ----------------
// A mark names the kernel launched next: arm that launch's own start / stop
// events (common.h ddq_launch).  A mark no kernel follows (an RCCL call, the
// fused step's empty "apply") is still armed at the next mark: dropped.
static void mark_settle(ddq_ctx* c) {
  if (g_ext_timing.start && !c->marks.empty()) c->marks.pop_back();   // not launched
  g_ext_timing = ExtTiming{};
}

static void mark_cb(void* arg, const char* name) {
  ddq_ctx* c = reinterpret_cast<ddq_ctx*>(arg);
  mark_settle(c);
  while (c->ev_used + 2 > c->ev_pool.size()) {
    hipEvent_t e;
    hipEventCreate(&e);
    c->ev_pool.push_back(e);
  }
  hipEvent_t e0 = c->ev_pool[c->ev_used++], e1 = c->ev_pool[c->ev_used++];
  g_ext_timing = ExtTiming{e0, e1};
  c->marks.push_back({name, e0, e1});
}

int ddq_profile_step(ddq_ctx* c, const ddq_step_cfg* cfg, char* names, float* usec, int32_t cap,
                     int32_t* n) {
  TRY(check_step(c, cfg));
  TRY(check_monitor_step(c, cfg));
  if (!n) return fail(c, DDQ_EINVAL, "null n");
  if (is_async(c, cfg)) return fail(c, DDQ_EINVAL, "profile steps take no async exchange");
  TRY(check_not_async(c));
  TRY(set_dev(c));
  c->marks.clear();
  c->ev_used = 0;
  if (c->steps == 0) TRY(initial_target_sync(c, cfg));
  g_profiling = true;
  g_unmarked = 0;
  const int rc = enqueue_step(c, cfg, Marks{mark_cb, c});
  g_profiling = false;
  mark_settle(c);
  TRY(rc);
  count_steps(c, cfg, 1);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (g_unmarked)   // (the step itself ran and counts)
    return fail(c, DDQ_ESTATE, "profile: %d kernel launch(es) of the step ran without a mark "
                "(their time is in no entry)", g_unmarked);
  const int k = (int)c->marks.size();
  *n = k;
  for (int i = 0; i < k && i < cap; ++i) {
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->marks[i].start, c->marks[i].stop));
    if (usec) usec[i] = ms * 1000.f;
    if (names) {
      memset(names + 16 * i, 0, 16);
      strncpy(names + 16 * i, c->marks[i].name.c_str(), 15);
    }
  }
  return DDQ_OK;
}

int ddq_time_layer(ddq_ctx* c, const char* name, int32_t reps, float* usec) {
  if (!c) return DDQ_EINVAL;
  if (!name || !usec || reps < 1) return fail(c, DDQ_EINVAL, "time_layer: bad arguments");
  int l = 0;
  if (!strcmp(name, "conv1_fwd")) l = 1;
  else if (!strcmp(name, "conv2_fwd")) l = 2;
  else if (!strcmp(name, "conv3_fwd")) l = 3;
  else return fail(c, DDQ_EINVAL, "time_layer: unknown layer %s", name);
  TRY(set_dev(c));
  const NetBuffers& nb = c->nb;
  hipEvent_t e0, e1;
  HIP_TRY(c, hipEventCreate(&e0));
  HIP_TRY(c, hipEventCreate(&e1));
  hipError_t e = launch_forward(nb, 2, c->stream, {}, true, l);   // warm
  if (e == hipSuccess) e = hipEventRecord(e0, c->stream);
  for (int i = 0; i < reps && e == hipSuccess; ++i) e = launch_forward(nb, 2, c->stream, {}, true, l);
  if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  HIP_TRY(c, e);
  *usec = ms * 1000.f / reps;
  return DDQ_OK;
}

double ddq_step_flops(const ddq_ctx* c) { return c ? step_flops(c->nb.B, c->nb.S) : 0.0; }

}  // extern "C"

// ---------------- checkpoint and resume ----------------
// The training state as named sections (include/ddq_hip.h): device buffers
// read and written in place, and two small structs assembled on the host --
// "config", a fingerprint that is only ever compared, and "counters", which a
// restore holds in c->st_ctr until ddq_state_commit pushes it.
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
  const int64_t P4 = nb.L.total * 4, cap = c->capacity;
  int n = 0;
  t[n++] = {"config", (int64_t)sizeof(ddq_state_config), nullptr};
  t[n++] = {"theta_q", P4, nb.theta[0]};
  t[n++] = {"theta_p", P4, nb.theta[1]};
  t[n++] = {"opt", P4, nb.opt};
  if (c->adam_on) t[n++] = {"opt2", P4, nb.opt2};
  t[n++] = {"counters", (int64_t)sizeof(ddq_state_counters), nullptr};
  if (c->ring.state) {
    t[n++] = {"ring_state", cap * 4 * nb.S * nb.S, c->ring.state};
    t[n++] = {"ring_action", cap, c->ring.action};
    t[n++] = {"ring_reward", 2 * cap, c->ring.reward};
    t[n++] = {"ring_nonterm", cap, c->ring.nonterm};
  }
  if (c->prio_on) t[n++] = {"prio_leaf", 4 * cap, nb.prio.leaf};
  if (c->a_env.n) t[n++] = {"actor", (int64_t)sizeof(ActorState), c->a_env.games};
  if (c->p_env.n) t[n++] = {"pool", (int64_t)c->p_env.n * (int64_t)sizeof(ActorState), c->p_env.games};
  return n;
}

static ddq_state_config state_config(const ddq_ctx* c) {
  const NetBuffers& nb = c->nb;
  ddq_state_config k;
  memset(&k, 0, sizeof(k));
  k.batch = (int16_t)nb.B;
  k.frame = (int16_t)nb.S;
  memcpy(&k.gamma_bits, &nb.gamma, 4);
  const bool ring = c->ring.state != nullptr;
  k.capacity = ring ? c->capacity : 0;
  k.lanes = ring ? c->lanes : 1;
  k.nstep = (uint8_t)(ring ? c->nstep : 1);
  if (c->prio_on) {
    k.prio_enabled = 1;
    k.prio_alpha = c->prio_cfg.alpha; k.prio_beta = c->prio_cfg.beta; k.prio_eps = c->prio_cfg.eps;
  }
  k.obj_target = (uint8_t)nb.obj_target;
  k.obj_loss = (uint8_t)nb.obj_loss;
  k.huber_delta = nb.huber_delta;
  if (c->adam_on) {
    k.adam_on = 1;
    k.adam_beta1 = nb.adam_beta1; k.adam_beta2 = nb.adam_beta2;
    k.adam_eps = nb.adam_eps; k.adam_max_grad_norm = nb.adam_clip;
  }
  k.actor = c->a_env.n ? 1 : 0;
  k.pool_games = (int16_t)c->p_env.n;
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
  if (c->ring.state) {
    ReplayMeta m;
    HIP_TRY(c, scopy(c, &m, c->ring.meta, sizeof(m), hipMemcpyDeviceToHost));
    k->head = m.head;
    k->valid = m.valid;
    k->draws = m.counter;
    k->ring_err = m.err;
    k->batch_ctr = c->batch_ctr;
  }
  if (c->p_env.n) {
    k->pool_h0 = c->p_h0;
    k->pool_v0 = c->p_v0;
    k->pool_moves = c->p_moves;
  }
  if (c->prio_on) {
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
  if (c->async_on)
    return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx: its state is spread "
                               "over the owners' shards");
  TRY(set_dev(c));
  if (c->cs) HIP_TRY(c, hipStreamSynchronize(c->cs));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (!c->st_dev) TRY(dalloc(c, &c->st_dev, (size_t)kStateParts + kStateMax + 16 + 2));
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
  if (c->restoring) k = c->st_ctr;
  else TRY(state_counters_now(c, &k));
  memcpy(buf, &k, sizeof(k));
  return DDQ_OK;
}

// enqueue section s's digest into digest word `slot` of the scratch; stage: its
// 64-byte-aligned slice of the scratch for a host-assembled section
static int state_enqueue_digest(ddq_ctx* c, const StateSec& s, int slot) {
  uint64_t* part = c->st_dev;
  uint64_t* dig = c->st_dev + kStateParts;
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

extern "C" {

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
  HIP_TRY(c, scopy(c, dig, c->st_dev + kStateParts, sizeof(dig), hipMemcpyDeviceToHost));
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
  HIP_TRY(c, scopy(c, digest, c->st_dev + kStateParts, 8, hipMemcpyDeviceToHost));
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
  if (!c->restoring) {
    TRY(state_counters_now(c, &c->st_ctr));
    c->restoring = true;
  }
  if (!s.dev) {
    memcpy(reinterpret_cast<uint8_t*>(&c->st_ctr) + offset, src, (size_t)bytes);
    return DDQ_OK;
  }
  HIP_TRY(c, scopy(c, (uint8_t*)s.dev + offset, src, (size_t)bytes, hipMemcpyHostToDevice));
  return DDQ_OK;
}

int ddq_state_commit(ddq_ctx* c) {
  TRY(state_begin(c));
  if (!c->restoring) return DDQ_OK;
  const ddq_state_counters k = c->st_ctr;
  const bool ring = c->ring.state != nullptr;
  const int64_t L = c->lane_len;
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
  if (c->p_env.n ? (k.pool_h0 < 0 || k.pool_h0 >= L || k.pool_v0 < 0 || k.pool_v0 > L ||
                    k.pool_moves < 0 || k.head != (k.pool_h0 + k.pool_moves % L) % L ||
                    k.valid != std::min(L, k.pool_v0 + std::min(k.pool_moves, L)))
                 : (k.pool_h0 != 0 || k.pool_v0 != 0 || k.pool_moves != 0))
    return fail(c, DDQ_EINVAL, "counters: the pool's h0 %lld, v0 %lld, moves %lld do not give the "
                               "ring's head %lld / valid %lld",
                (long long)k.pool_h0, (long long)k.pool_v0, (long long)k.pool_moves,
                (long long)k.head, (long long)k.valid);
  // the games: boards the environment kernel can play, the pool in lock step
  for (int role = 0; role < 2; ++role) {
    const EnvBufs<ActorState>& b = role ? c->p_env : c->a_env;
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
  if (c->prio_on) {
    if (k.pmax < kPrioOne || k.pmax > kPrioMax)
      return fail(c, DDQ_EINVAL, "counters: pmax %u outside [65536, 2^24]", k.pmax);
    int32_t* bad = reinterpret_cast<int32_t*>(c->st_dev + kStateParts + kStateMax + 16);
    int32_t hb[2] = {0, INT32_MAX};
    HIP_TRY(c, scopy(c, bad, hb, sizeof(hb), hipMemcpyHostToDevice));
    HIP_TRY(c, launch_state_check_leaves(c->nb.prio, L, k.head, k.valid, c->nstep, bad, c->stream));
    HIP_TRY(c, scopy(c, hb, bad, sizeof(hb), hipMemcpyDeviceToHost));
    if (hb[0])
      return fail(c, DDQ_EINVAL, "prio_leaf: %d leaves are above 2^24 or break \"zero <=> slot unfilled "
                                 "or forbidden\" under head %lld, valid %lld, n %d (first: slot %d)",
                  hb[0], (long long)k.head, (long long)k.valid, c->nstep, hb[1]);
  } else if (k.pmax != 0) {
    return fail(c, DDQ_EINVAL, "counters: pmax %u while prioritized replay is off", k.pmax);
  }
  // ---- push: device memory, then the host mirrors ----
  HIP_TRY(c, hipMemcpyAsync(c->nb.iter, &k.iteration, 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->nb.opt_init, &k.opt_init, 4, hipMemcpyHostToDevice, c->stream));
  if (ring) {
    char* m = reinterpret_cast<char*>(c->ring.meta);
    const int64_t hv[2] = {k.head, k.valid};
    HIP_TRY(c, hipMemcpyAsync(m, hv, sizeof(hv), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(m + offsetof(ReplayMeta, counter), &k.draws, 8, hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, hipMemcpyAsync(m + offsetof(ReplayMeta, err), &k.ring_err, 4, hipMemcpyHostToDevice,
                              c->stream));
  }
  if (c->prio_on) {
    HIP_TRY(c, hipMemcpyAsync(&c->nb.prio.st->pmax, &k.pmax, 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_prio_resum(c->nb.prio, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (k is this frame's: copied before it goes)
  c->applied = k.iteration;
  c->steps = k.steps;
  c->head = k.head;
  c->valid = k.valid;
  c->batch_ctr = k.batch_ctr;
  c->p_h0 = k.pool_h0;
  c->p_v0 = k.pool_v0;
  c->p_moves = k.pool_moves;
  // ---- derived: the conv weights' copies of both towers, the games' rendered states ----
  for (int z = 0; z < 2; ++z) HIP_TRY(c, launch_relayout(c->nb, z, c->stream));
  if (c->a_env.n)
    HIP_TRY(c, launch_env(actor_role(c), env_io(c, c->a_env), c->act_q, 0, 0, c->stream));
  if (c->p_env.n)
    HIP_TRY(c, launch_env(pool_role(c), env_io(c, c->p_env), c->act_q, 0, 0, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);
  c->idx_bound = false;
  c->restoring = false;
  return DDQ_OK;
}

}  // extern "C"
