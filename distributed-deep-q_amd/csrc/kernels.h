// Host-side launch wrappers for the deepq step kernels (implemented in
// kernels.hip).  All launches are asynchronous on the given stream and
// graph-capture safe (no allocation, no synchronisation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"   // ddq_launch / ExtTiming (kernel timing)
#include "step_plan.h"

namespace ddq {

// Flat parameter layout of one tower (pycaffe order), element offsets.
struct ParamLayout {
  int S, S2, S3, S4;
  int64_t w[5], b[5];      // offsets of layer weights / biases
  int64_t wn[5], bn[5];    // counts
  int64_t total;
  int64_t wks_off[3];      // offsets of the split (3 x bf16) forward weights in a wks plane
  int64_t wkst_off;        // conv2 data-gradient split weights [ci][tap'][co] (Q only)
  int64_t wkst3_off;       // conv3 data-gradient split weights [ci][tap'][co] (Q only)
  int64_t wks_total;       // elements per wks plane (conv1 padded to kx = 8)
};
ParamLayout make_layout(int S);

// Replay ring bookkeeping kept in device memory so captured graphs see the
// live head/valid and a fresh RNG counter on every replay.
//
// Laned ring (ddq_replay_set_lanes): lanes > 1 contiguous lanes of lane_len =
// capacity / lanes slots, lane g = slots [g lane_len, (g + 1) lane_len), each a
// ring of its own.  Lock-step writers fill it (env.h: PoolRole), so the lanes share one
// head in [0, lane_len) and one valid in [0, lane_len]: head / valid are then
// the per-lane values.  lanes 0 or 1: one ring, lane_len == capacity.
constexpr int kNstepMax = 8;   // DDQ_NSTEP_MAX
struct ReplayMeta {
  int64_t head, valid, capacity;   // head, valid: the first 16 bytes (push_meta)
  uint64_t counter;        // device index-stream draws so far
  int32_t err;             // sticky: 1 = stored action >= num_actions seen,
                           //         2 = a draw found no distinct index set
  int32_t lanes;
  int64_t lane_len;
  // n-step returns (ddq_replay_set_nstep): the window length in [1, DDQ_NSTEP_MAX]
  // and ddq_net_desc.gamma.  Here, not in a launch argument, so a captured
  // graph's draw and gather workgroups read them like head / valid.
  int32_t nstep;
  float gamma;
};

// The update rule's scalars (ddq_update_cfg) and the target period as given.
struct UpdateRule {
  int rule, period;
  float lr, decay, eps, momentum, wd;
};

struct Prefetch;
// What the launches of one step take besides the buffers: the plan
// (step_plan.h) and what its sites need.  plan.fused(): the slab-reduce launch
// computes fc4's weight gradient tile by tile and updates every parameter
// where its gradient becomes final.  plan.ext() (RCCL all-reduce with
// overlap): fc4_bwd computes fc4's weight gradient, the comm stream sums it
// over the ranks under the conv backward (fc4_wait), the slab-reduce launch
// applies fc4's weights from it, and launch_apply the rest after their (small)
// all-reduce.
struct StepLaunch {
  StepPlan plan;
  UpdateRule u{};
  ReplayMeta* meta = nullptr;       // the draw counter, for plan.bump / plan.draw
  const Prefetch* next = nullptr;   // the next step's set, for plan.draw / plan.gather
  hipEvent_t fc4_wait = nullptr;    // plan.ext(): the slab-reduce launch waits for it
};

// Prioritized replay (prio.hip, prio.h, ddq_replay_set_priority): a radix-64 sum tree over
// the ring's slots in device memory.  Leaves are uint32 fixed-point priorities
// (16 fraction bits; 0 = unfilled or forbidden slot, else in [1, 2^24]); level
// k >= 1 holds the exact uint64 sums of 64 nodes of level k - 1; every level is
// padded with zeros to a multiple of 64 nodes and the top level has <= 64.  The
// scalars a captured graph must read live sit in PrioState, never in a launch
// argument.
constexpr int kPrioLevels = 6;          // sum levels: 64^6 > 2^31 slots
constexpr uint32_t kPrioOne = 65536u;   // p = 1.0
constexpr uint32_t kPrioMax = 1u << 24;
struct PrioState {
  float alpha, beta, eps;
  uint32_t pmax;
  unsigned long long total;             // sum of all leaves (the root)
};
struct PrioTree {
  uint32_t* leaf;                       // nullptr: prioritization off
  unsigned long long* sum[kPrioLevels]; // sum[k - 1]: level k
  int64_t padded[kPrioLevels + 1];      // nodes per level with padding ([0]: leaves)
  int32_t nlev;                         // sum levels K >= 1
  int64_t capacity;
  PrioState* st;
};

// The replay ring in device memory: every launch that reads or adds to it
// takes this view.  A member of ActorRole / PoolRole (kernel arguments): the
// layout is fixed.
struct ReplayRing {
  uint8_t* state;
  uint8_t* action;
  int16_t* reward;
  uint8_t* nonterm;
  ReplayMeta* meta;
  const PrioTree* prio;             // device copy of the tree; nullptr: prioritization off
};

// One minibatch set: NHWC frames, action one-hot (B,4), reward / non_terminal
// (B), the ring slots they were gathered from.  isw: the importance-sampling
// weights (B) of prioritized replay, bound only while it is on and then always
// reward + B, the second half of the reward buffer (the head then runs its
// objective instantiation, reads them there and scales dQ and the loss terms
// by them).
struct Minibatch {
  float *state, *next_state, *action, *reward, *nonterm;
  int32_t* idx;
  float* isw;
};

// The profile marks of a step (ddq_profile_step): m(name) names the kernel
// launched next; without fn (every other caller) it does nothing.
struct Marks {
  void (*fn)(void*, const char*) = nullptr;
  void* arg = nullptr;
  void operator()(const char* name) const {
    if (fn) fn(arg, name);
  }
};
// Called right after the fc4 weight gradient is enqueued (the overlapped
// all-reduce starts there); without fn it does nothing.
struct Fc4Done {
  hipError_t (*fn)(void*) = nullptr;
  void* arg = nullptr;
  hipError_t operator()() const { return fn ? fn(arg) : hipSuccess; }
};

struct NetBuffers {
  int B, S;
  Minibatch mb;                     // the set the launches train on and draw into
  // activations per tower z (0 = Q on state, 1 = P on next_state): pool1 /
  // pool2 in one buffer each, sized for their split form (3 bf16 planes,
  // NHWC) -- the S = 16 small-map step keeps the Q tower's split there (its K4
  // reads them split); the general kernels keep fp32 NHWC in the same bytes
  // (pool1f / pool2f: the next conv and the Q weight gradients split them
  // while staging); pool3 fp32 in Caffe order (fc4's input)
  float *pool3[2], *h4[2];
  __bf16 *pool1s[2], *pool2s[2];    // split pool1 / pool2 (3 planes, NHWC): small-map step
  float *pool1f[2], *pool2f[2];     // the same bytes, fp32 NHWC: general kernels
  uint8_t *mask1, *mask2, *mask3;   // Q tower only
  float* fc4_part;                  // [splits][2][B][512]
  int fc4_splits;
  // optional device index log: draw d's sorted indices at [(d % log_cap) * B]
  int32_t* idx_log;
  int64_t log_cap;
  // blobs
  float *q_out, *p_out, *q_sa, *p_sa, *target, *loss;
  // backward scratch
  float *dh4, *dconv3;               // dh4 (B,512); dconv3: fp32 pooled dpool3 (fc4 dgrad)
  __bf16* dconv2s;                  // split pooled dpool2 (conv3's data gradient)
  __bf16* dconv3s;                  // split expanded dconv3 (B,S/4,S/4,64): conv3's weight gradient
  float* wpart;                     // conv wgrad slabs (3 layers, disjoint)
  int64_t wpart_off[3];
  int wsplits[3];
  int wnp[3];
  // parameters: theta[z] flat Caffe layout; wks[z] split kernel layouts (the
  // forward convs; Q's also the data gradients' transposed copies); grad; opt
  // state
  float *theta[2], *grad, *opt;
  __bf16* wks[2];
  float *dqbuf, *lpart;             // head: per-sample dQ (B,4) and squared error (B)
  int32_t* opt_init;                // 0 until the first apply after a reset
  int64_t* iter;                    // applied updates (param-server iteration)
  // side stream + events: the next step's sample + gather beside a step whose
  // apply launch cannot carry them (pipelined stepping, B > 256)
  hipStream_t side;
  hipEvent_t ev[8];
  ParamLayout L;
  float gamma;
  int nstep = 1;                    // the ring's n-step length: >= 2 launches the n-step
                                    // instantiations of the kernels that draw or gather
  // selectable objective (ddq_set_objective): target 0 = max_a P, 1 = P at the
  // first maximum of qn_out (Q(s',.) under theta_Q, (B,4), the pass's first
  // launch group); loss 0 = Euclidean, 1 = Huber with band huber_delta
  int obj_target = 0, obj_loss = 0;
  float huber_delta = 0.f;
  float* qn_out = nullptr;
  PrioTree prio{};                  // prioritized replay: the tree (leaf == nullptr: off)
  // Adam (ddq_set_adam, adam.h): opt holds the first moment, opt2 the second;
  // gn_part: the gradient-norm launch's partials; gnorm: the last pre-clip norm
  float* opt2 = nullptr;
  double* gn_part = nullptr;
  float* gnorm = nullptr;
  float adam_beta1 = 0.f, adam_beta2 = 0.f, adam_eps = 0.f, adam_clip = 0.f;
  // soft target updates (ddq_set_target_tau): < 1, every due P <- Q sync of a
  // step writes P + tau (Q - P) instead (ApplyArgs::tau, target_blend)
  float target_tau = 1.f;
  // deepq16 step (small.h, small_bwd.h): fc4 chain partials and its fan-in words
  int small;                        // S == 16, B <= 256: the four-launch step
  int small_G = 1;                  // its fc4 chain's image chunks (B > 32: ceil(B / 32))
  float* upart = nullptr;           // [G][32][96] unit-sum partials (G > 1)
  float* w4part = nullptr;          // [G][512][256] fc4 weight-gradient partials (G > 1)
  float *qpart, *dpart;             // [32][2][B][4] Q_out / P_out partials, [32][B][256] dpool3
  int32_t* csync;                   // meeting words: K2 [0..2] (64-bit counter, timeout),
                                    // K4 [8..40) (a 64-bit counter per tile, timeout at
                                    // 40), K1's split form: timeout at 48
  __bf16* dconv2x;                  // split expanded dconv2 NHWC (B, 8, 8, 64) (K3 -> K4)
  float *slab2, *slab3;             // K4's per-group slabs of conv2 / conv3 tiles
  __bf16* xchg;                     // K1 split form: pool2 halves [B][2][2][1536]
  uint64_t* pairc;                  // K1 split form: meeting counters [B][2]
};

// fused device draw + gather for the step (B <= 256); the step moves the
// counter on (StepPlan::bump)
hipError_t launch_sample_gather(const NetBuffers& nb, const ReplayRing& ring, uint64_t seed,
                                hipStream_t s);
hipError_t launch_gather(const NetBuffers& nb, const ReplayRing& ring, hipStream_t s);
hipError_t launch_sample(const NetBuffers& nb, ReplayMeta* meta, uint64_t seed, hipStream_t s);
// only: 0 = every layer, l + 1 = conv layer l alone (ddq_time_layer)
hipError_t launch_forward(const NetBuffers& nb, int nz, hipStream_t s, Marks M = {},
                          bool out = true, int only = 0);
// deepq16 (nb.small): K1 (towers + the head's bookkeeping, as launch_head's)
// and K2 (fc4 chain) in place of launch_forward + launch_head
// Every meeting launch of the small-map step has all of its meeting
// workgroups resident at once on this device (meet() spins on the others):
// *ok = 0 and why set otherwise (the ctx then runs the general kernels)
hipError_t small_coresident(int B, int* ok, char* why, int nwhy);
hipError_t launch_small_fwd_head(const NetBuffers& nb, const StepLaunch& sl, hipStream_t s,
                                 Marks M = {});
hipError_t launch_head(const NetBuffers& nb, const StepLaunch& sl, hipStream_t s);
bool fused_apply_ok(const ParamLayout& L);
// deepq16 (nb.small): K3 (data gradients, conv1's weight gradient slabs)
// and K4 (conv weight gradients + fused apply + bookkeeping + next gather) in
// place of launch_backward (same arguments)
hipError_t launch_small_bwd(const NetBuffers& nb, const StepLaunch& sl, hipStream_t s,
                            Marks M = {}, Fc4Done fc4_done = {});
void small_groups(int B, int* G2, int* G3);
hipError_t launch_backward(const NetBuffers& nb, const StepLaunch& sl, hipStream_t s,
                           Marks M = {}, Fc4Done fc4_done = {});
// The next step's draw + gather as extra blocks of the launch StepPlan::gather
// names (pipelined stepping)
struct Prefetch {
  const uint8_t* st;
  const uint8_t* act;
  const int16_t* rew;
  const uint8_t* nt;
  ReplayMeta* meta;
  uint64_t seed;
  int B, S, gx, ng;                 // ng = 0: no prefetch blocks
  int predrawn;                     // 1: an earlier launch drew the set into idx already
                                    // (StepPlan::predrawn)
  int32_t* idx;
  int32_t* idx_log;                 // NetBuffers::idx_log / log_cap of the step
  int64_t log_cap;
  float *sQ, *sP, *action, *reward, *nonterm;
};
// next: the buffers of the step that trains on the prefetched set (next.mb)
Prefetch make_prefetch(const NetBuffers& next, const ReplayRing& ring, uint64_t seed);
// sl.u.period > 0: also copy Q -> P when the next pull sees iteration % period == 0.
hipError_t launch_apply(const NetBuffers& nb, const StepLaunch& sl, hipStream_t s);
// rule DDQ_RULE_ADAM (4): launch_apply launches adam_apply_kernel (adam.h) in
// the apply kernel's place, with nb's Adam constants and lr; the fused apply
// must be off.  With nb.adam_clip > 0 the caller launches launch_grad_norm
// first: the gradient buffer's sum of squares as kGnBlocks double partials
constexpr int kRuleAdam = 4;
constexpr int kGnBlocks = 128;
hipError_t launch_grad_norm(const NetBuffers& nb, hipStream_t s);
hipError_t launch_relayout(const NetBuffers& nb, int z, hipStream_t s);
// owner apply of shard [off, off+len) with W gradient slices (stride `slice`)
// applied in rank order; then, after the theta all-gather, launch_refresh
// rebuilds the conv kernel layouts and performs a latched P <- Q sync.
struct ShardOpts {
  float* theta = nullptr;         // the parameters updated: nb.theta[0], or the async
                                  // exchange's owner copy
  int first = -1;                 // >= 0: the rules' first-call flag from the host and the
                                  // apply's bookkeeping (iteration += 1) done by the launch
                                  // itself (async owner applies); -1: the flags latched by
                                  // the step's bookkeeping
  const Prefetch* pre = nullptr;  // the next step's draw + gather as extra blocks
  float* mirror = nullptr;        // a second copy of the updated shard
  int refresh_own = 0;            // != 0: the launch also does launch_refresh's work for its
                                  // own shard (conv kernel layouts of nb.wks[0]; the P <- Q
                                  // copy into nb.theta[1] / nb.wks[1] when a sync is due: -1
                                  // the latched flag decides, 1 no sync, 2 sync), from the
                                  // values it applied; the refresh after the all-gather /
                                  // pull then skips that shard
  int own_w = -1;                 // with own_g: slice own_w is read from there (the rank's
  const float* own_g = nullptr;   // own gradient in place) instead of gsl
};
hipError_t launch_apply_shard(const NetBuffers& nb, const UpdateRule& u, const float* gsl,
                              int64_t off, int64_t len, int64_t slice, int W, hipStream_t s,
                              const ShardOpts& o = {});
// force_sync >= 0: P <- Q decided by the host instead of the latched flag.
// [skip_lo, skip_hi): a range already refreshed (an owner's refresh_own
// apply); nothing is launched when it covers every parameter
hipError_t launch_refresh(const NetBuffers& nb, hipStream_t s, int force_sync = -1,
                          int64_t skip_lo = 0, int64_t skip_hi = 0);
// one apply's bookkeeping (first-call / sync latches, iteration += 1)
hipError_t launch_book(const NetBuffers& nb, int period, hipStream_t s);
hipError_t launch_sum_slices(float* out, const float* in, int W, int64_t len, int64_t slice,
                             hipStream_t s);
// Q-tower forward of n states (NHWC f32 in `in`) into scratch, argmax into out.
// M: the launches' profile names (ddq_profile_step).
hipError_t launch_act(const NetBuffers& nb, const float* in, int n, float* pool3, float* h4,
                      float* part, float* qout, int32_t* actions, __bf16* pool1s,
                      __bf16* pool2s, hipStream_t s, Marks M = {});
// Device-resident Snake environment (env.h): one kernel body, three roles.
// ActorState: one acting game.  boards: the 4-frame history of 10x10 board
// codes [x*10+y] (SnakeGame.encode_state), oldest first, then init_board;
// draws: position in the game's RNG stream splitmix64(seed ^ splitmix64(k)).
struct ActorState {
  uint64_t seed, draws;
  int64_t steps, games, reward_sum;
  int8_t boards[5 * 100];
  int8_t pad[4];
};
// EvalGame: one evaluated game's RNG stream (as the actor's), its lock-step move
// counter, the records in its log, the running episode's score / moves and its
// boards (4-frame history, then its start board).
struct EvalGame {
  uint64_t seed, draws;
  int64_t reward_sum;
  int32_t move, episodes, score, moves;
  int8_t boards[5 * 100];
  int8_t pad[4];
};
// What every role's launch has: ngames workgroups, game g reading q[4g..4g+4)
// and rendering its next state into slice g of `in`.
struct EnvIO {
  const uint8_t* maps;              // row_map[S] then col_map[S], entries in [0,10)
  float* in;                        // [ngames] states as f32 NHWC (S,S,4): the forward's input
  int S, ngames;
};
// A role is the launch argument that says what its games differ in: the state
// type, whether the coin is drawn even at thresh == 0, whether a ring slot is
// rendered, and (env.h) env_idle / env_commit.
// Single actor (ddq_actor_*): one game, the transition into ring slot
// meta->head read on the device, head / valid advanced there.
struct ActorRole {
  using Game = ActorState;
  static constexpr bool kCoinAlways = true, kRing = true;
  ActorState* games;
  ReplayRing ring;                  // the ring the role adds into
};
// Actor pool (ddq_actors_*): ngames == lanes games, game g adding into lane g of
// a laned ring at slot g lane_len + (h0 + steps_g) mod lane_len; h0 / v0: the
// ring's per-lane head / valid when the pool was created (launch constants);
// workgroup 0 publishes the per-lane head / valid.
struct PoolRole {
  using Game = ActorState;
  static constexpr bool kCoinAlways = true, kRing = true;
  ActorState* games;
  ReplayRing ring;                  // the ring the role adds into
  int64_t lane_len, h0, v0;
};
// Policy evaluation (ddq_eval_*): the episode record when the game is over or
// max_moves is reached; a game whose log is full does nothing.
struct EvalRole {
  using Game = EvalGame;
  static constexpr bool kCoinAlways = false, kRing = false;
  EvalGame* games;                  // [ngames]
  int32_t* log;                     // [ngames][max_episodes][4]: end_move, score, moves, ended_by
  int max_moves, max_episodes;
};
// ngames workgroups of the role's kernel: (play != 0) game g's epsilon-greedy
// action from its row of q and the coin against thresh = ceil(epsilon * 2^53),
// one game step, the role's commit; then the render of its next state into the
// ring slot (ring roles, not after a game over) and into its slice of io.in.
hipError_t launch_env(const ActorRole& r, const EnvIO& io, const float* q, uint64_t thresh,
                      int play, hipStream_t s);
hipError_t launch_env(const EvalRole& r, const EnvIO& io, const float* q, uint64_t thresh, int play,
                      hipStream_t s);
hipError_t launch_env(const PoolRole& r, const EnvIO& io, const float* q, uint64_t thresh, int play,
                      hipStream_t s);
// Device-resident training monitor (monitor.h).  MonitorRecord is
// ddq_monitor_record (include/ddq_hip.h), field for field.
struct MonitorRecord {
  int64_t iteration, tag;
  float loss, q_max_mean;
  int32_t nonfinite[3], reserved;
  float param_rms[2][10], grad_rms[10];
};
constexpr int kMonChunk = 8192;     // floats per chunk: one workgroup's share
constexpr int kMonBlobs = 30;       // (theta_Q, theta_P, grad) x the layout's 10 blobs
// one workgroup's floats: [off, off + count) of tensor `tensor`, inside one blob
struct MonitorChunk {
  int32_t tensor, blob;
  uint32_t off;
  int32_t count;
};
// blob tensor * 10 + b: its chunks are chunks[first .. first + n), in offset order
struct MonitorBlob {
  int32_t first, n;
  int64_t count;
};
struct MonitorEnv {
  const float* t[3];                // theta_Q, theta_P, grad
  const MonitorChunk* chunks;
  const MonitorBlob* blobs;         // [kMonBlobs]
  int nchunks;
  double* psum;                     // [nchunks] sums of squares
  int32_t* pnf;                     // [nchunks] non-finite counts
  int32_t* ticket;                  // arrivals of this launch (0 between launches)
  int64_t* count;                   // records taken since enable
  MonitorRecord* ring;
  int64_t capacity;
  const int64_t* iter;
  const float* loss;
  const float* q_out;
  int B;
};
// One record (chunks' workgroups, the last to finish writes it); period > 0:
// only when *iter % period == 0 (every workgroup returns at once otherwise).
hipError_t launch_monitor(const MonitorEnv& e, int32_t period, int64_t tag, hipStream_t s);
// large-batch device draw (bitmap claim + ordered compaction) into idx[0..n)
// and the Caffe-layout (n,4,S,S) f32 gather of replay.py:167-183
hipError_t launch_sample_batch(ReplayMeta* meta, int64_t valid, int n, uint64_t seed,
                               uint64_t ctr, uint32_t* bm, int32_t* blk, int32_t* idx,
                               hipStream_t s, int nstep);
// out: the n transitions' buffers (its idx / isw are not read)
hipError_t launch_gather_nchw(const ReplayRing& ring, const int32_t* idx, int n, int S,
                              const Minibatch& out, hipStream_t s, int nstep);
hipError_t launch_tile(uint8_t* dst, const uint8_t* src, uint64_t pool_bytes, uint64_t total,
                       hipStream_t s);
hipError_t launch_u8_to_nhwc(const uint8_t* src, int n, int S, float* dst, hipStream_t s);

// Prioritized replay launches (prio.hip).  All one stream-ordered launch each, no
// allocation, graph-capture safe.
// every filled, allowed slot <- st->pmax, the rest 0, then the sums bottom-up
hipError_t launch_prio_rebuild(const PrioTree& t, const ReplayMeta* meta, hipStream_t s);
// one workgroup: the draw counter's stratified sample into nb.mb.idx / nb.mb.isw (and
// the index log); advance: the counter moves on afterwards (a step's own
// launch_prio_commit_draw does that otherwise)
hipError_t launch_prio_sample(const NetBuffers& nb, ReplayMeta* meta, uint64_t seed, hipStream_t s,
                              bool advance = false);
// one workgroup, after the launch that wrote nb.q_sa / nb.target: commit |TD| of
// nb.mb.idx.  bump: the draw counter advances by one; next != nullptr: then draw
// the advanced counter's sample into next->mb.idx / next->mb.isw and log it
hipError_t launch_prio_commit_draw(const NetBuffers& nb, ReplayMeta* bump, const NetBuffers* next,
                                   uint64_t seed, hipStream_t s);
// the commit alone (ddq_replay_update_priorities_async)
hipError_t launch_prio_commit(const NetBuffers& nb, ReplayMeta* meta, hipStream_t s);
// the writer rule for one add at lane-local slot h of lane `lane` (host adds)
hipError_t launch_prio_add(const PrioTree& t, const ReplayMeta* meta, int64_t lane, int64_t h,
                           hipStream_t s);
// leaves idx[0..n) <- q[0..n) (device arrays), sums fixed, pmax raised
hipError_t launch_prio_set(const PrioTree& t, const int32_t* idx, const uint32_t* q, int n,
                           hipStream_t s);
// fill n floats with 1.0f (the weights of a host-given minibatch)
hipError_t launch_fill_ones(float* dst, int n, hipStream_t s);
// the sums bottom-up and the total from the leaves as they are (ddq_state_commit)
hipError_t launch_prio_resum(const PrioTree& t, hipStream_t s);

// Checkpoint and resume (state.hip, ddq_state_*).
constexpr int kStateThreads = 256;
constexpr int kStateParts = 2048;   // the digest launch's workgroups at most: its partials
// *out <- the digest (include/ddq_hip.h) of the n bytes at p, an allocation's
// base (16-byte aligned); part: kStateParts words of scratch.  Two launches.
hipError_t launch_state_digest(const void* p, uint64_t n, uint64_t* part, uint64_t* out,
                               hipStream_t s);
// bad[0] += the leaves that are above 2^24 or break "q == 0 <=> slot unfilled or
// forbidden" under (head, valid, nstep) per lane of lane_len slots; bad[1] = min
// with the lowest such slot
hipError_t launch_state_check_leaves(const PrioTree& t, int64_t lane_len, int64_t head,
                                     int64_t valid, int nstep, int32_t* bad, hipStream_t s);

double step_flops(int B, int S);

extern thread_local const char* g_launch_where;

}  // namespace ddq
