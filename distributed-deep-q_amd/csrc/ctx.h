// The one internal header of the host side (api*.hip): ddq_ctx, its fields
// grouped by the subsystem that owns them, the error macros, allocation, and
// the helpers more than one unit calls.  Private to csrc/.
#pragma once
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ddq_hip.h"
#include "kernels.h"
#include "param_noise.h"

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
  ddq::NetBuffers nb{};
  std::vector<void*> allocs;
  std::string err;
  bool adam_on = false;            // ddq_set_adam was called: nb.opt2 / gn_part / gnorm exist
  // ddq_inject_fault: armed failpoint, consumed by the next eager step
  int fault = 0;
  std::string small_off;           // why the small-map step is off at S = 16 (empty: on)
  StepGraphs graphs;
  // minibatch sets: [0] the ctx's own (nb.mb is its copy), [1] the twin of
  // pipelined stepping (ensure_pipe allocates it)
  ddq::Minibatch mb[2] = {};
  int64_t steps = 0;
  int64_t applied = 0;               // host mirror of the device iteration counter

  // api_replay.hip
  struct Replay {
    // replay ring: the view every launch takes (state == nullptr: not created;
    // meta: device; prio follows d_prio, nullptr while prioritization is off)
    ddq::ReplayRing ring{};
    uint32_t* r_bitmap = nullptr;    // large-batch sampler scratch (lazy)
    int32_t* r_blk = nullptr;
    uint64_t batch_ctr = 0;          // large-batch draws so far (RNG stream position)
    int64_t head = 0, valid = 0, capacity = 0;
    int32_t lanes = 1;               // laned ring (ddq_replay_set_lanes): head / valid per lane
    int64_t lane_len = 0;            // capacity / lanes
    int32_t nstep = 1;               // n-step returns (ddq_replay_set_nstep)
    int32_t aug_pad = 0;             // random-shift augmentation (ddq_replay_set_augment): 0 = off
    bool idx_bound = false;          // nb.mb.idx holds the bound minibatch's slots
    // index log (ddq_index_log_enable)
    int32_t* log_buf = nullptr;
    int64_t log_buf_cap = 0;
    int64_t log_first = 0;           // first draw the log holds (the counter at enable)
  } replay;

  // api_replay.hip
  struct Prio {
    // prioritized replay (ddq_replay_set_priority): nb.prio and the sets' isw are bound while on
    bool prio_on = false;
    ddq_priority_cfg prio_cfg{0, 0.f, 0.f, 0.f};
    ddq::PrioTree* d_prio = nullptr; // device copy of nb.prio: the ring writers' argument
    int32_t* pset_idx = nullptr;     // ddq_replay_set_priorities staging (grown on demand)
    uint32_t* pset_q = nullptr;
    int32_t pset_cap = 0;
  } prio;

  // api.hip
  struct Act {
    // acting scratch
    uint8_t* act_u8 = nullptr;
    float *act_in = nullptr, *act_p3 = nullptr;
    float *act_h4 = nullptr, *act_part = nullptr, *act_q = nullptr;
    __bf16 *act_p1s = nullptr, *act_p2s = nullptr;
    int32_t* act_out = nullptr;
    // ddq_set_acting_path: which convs every launch_act of the ctx launches
    int32_t act_path = DDQ_ACT_BATCH;
  } act;

  // api_param_noise.hip
  struct ParamNoise {
    // parameter-space noise (ddq_set_param_noise): w = (theta~, wks~), allocated by
    // the first enable and kept; cfg.sigma mirrors *d_sigma as of the last
    // ddq_synchronize; epoch: resamples since the enable; moves: acting moves
    // since the enable (resample_every); q: (2, B, 4) Q and Q~ of the last adapt
    // (blob "Qa_out" is the second half); kl: (B) blob "pn_kl"
    bool on = false;
    ddq_param_noise_cfg cfg{};
    ddq::ActWeights w{nullptr, nullptr};
    float *d_sigma = nullptr, *q = nullptr, *kl = nullptr;
    uint64_t epoch = 0;
    int64_t moves = 0;
  } pn;

  // api_env.hip
  struct Envs {
    // device-resident Snake environments (env_create): the single actor
    // (ddq_actor_create, one game), the evaluator (ddq_eval_create) and the actor
    // pool (ddq_actors_create), each with room for B games
    EnvBufs<ddq::ActorState> a_env, p_env;
    EnvBufs<ddq::EvalGame> e_env;
    // evaluator: the per-game episode logs (grown on demand)
    int32_t* e_log = nullptr;
    size_t e_log_cap = 0;            // int32 elements allocated
    int e_max_moves = 0, e_max_ep = 0;
    uint64_t e_thresh = 0;
    int64_t e_moves = 0;             // lock-step moves enqueued since create
    // pool: the ring's per-lane head / valid at create, moves enqueued since
    int64_t p_h0 = 0, p_v0 = 0, p_moves = 0;
  } envs;

  // api_exchange.hip
  struct Comm {
    // comm (RCCL ranks, or an in-process group of ctxs exchanging by device copies)
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    bool local = false;              // member of an in-process group (ddq_group_init)
    hipStream_t cs = nullptr;        // comm stream of the overlapped all-reduce
    hipEvent_t cev[3] = {};
    int64_t shard_len = 0;           // parameters owned per rank (multiple of 64)
    float* gsl = nullptr;            // [W][shard_len] received gradient slices
    float* gstage = nullptr;         // [W][P] in-process all-reduce staging
    std::string comm_err;
  } comm;

  // api_exchange.hip
  struct Async {
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
  } async;

  // api_monitor.hip
  struct Mon {
    // training monitor (ddq_monitor_enable): mon.ring == nullptr while off
    ddq::MonitorEnv mon{};
    int32_t mon_period = 0;          // > 0: every single-ctx step ends with the monitor launch
  } mon;

  // api_state.hip
  struct State {
    // checkpoint and resume (ddq_state_*): restoring from the first ddq_state_write
    // of a section other than "config" until ddq_state_commit; st_ctr: the
    // "counters" section as written, pushed by the commit; st_dev: device scratch
    // (kStateParts digest partials, kStateMax digests, a 128-byte stage, bad[2])
    bool restoring = false;
    ddq_state_counters st_ctr{};
    uint64_t* st_dev = nullptr;
  } state;

  // api.hip (measurement)
  struct ProfileMarks {
    // profiling marks: a kernel's own dispatch start / stop events
    struct Mark {
      std::string name;
      hipEvent_t start, stop;
    };
    std::vector<Mark> marks;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
  } marks;
};

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

#define TRY(x)                \
  do {                        \
    int r_ = (x);             \
    if (r_ != DDQ_OK) return r_; \
  } while (0)

// The helpers below are defined once, without `static`, in the unit named;
// none of them is exported from the library.
#pragma GCC visibility push(hidden)
namespace ddq {

// api.hip
int fail(ddq_ctx* c, int code, const char* fmt, ...);
hipError_t scopy(ddq_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
int set_dev(ddq_ctx* c);
int not_restoring(ddq_ctx* c);
int guard(ddq_ctx* c);
void invalidate_graph(ddq_ctx* c);
int mb_alloc(ddq_ctx* c, Minibatch* out);
void mb_bind_weights(ddq_ctx* c, bool on);
// api_replay.hip
int prio_refuse(ddq_ctx* c, const char* what);
bool too_few_slots(const ddq_ctx* c, int64_t batch);
// api_param_noise.hip: one acting move of ddq_select_action, the device actor or
// the pool is about to be enqueued -- the resample_every rule; *over <- the
// perturbed set (nullptr while the feature is off)
int param_noise_move(ddq_ctx* c, const ActWeights** over);
// api_env.hip
const char* actor_board_error(const int8_t* b);
ActorRole actor_role(const ddq_ctx* c);
PoolRole pool_role(const ddq_ctx* c);

template <class Game>
static EnvIO env_io(const ddq_ctx* c, const EnvBufs<Game>& b) {
  return EnvIO{b.maps, b.in, c->nb.S, b.n};
}

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

}  // namespace ddq
#pragma GCC visibility pop
