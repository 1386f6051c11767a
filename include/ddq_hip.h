/*
 * ddq_hip.h -- C-ABI of libddq_hip.so, the MI355X (gfx950) implementation of
 * distributed-deep-q's data-parallel DQN training step.
 *
 * The reference's hot path sits behind pycaffe (Boost.Python -> C++ caffe::Net)
 * plus numpy/h5py/Flask host code.  Every entry point below names the reference
 * interface it replaces (file:line in defc0n1/distributed-deep-q).  The Python
 * drop-ins in distributed-deep-q_amd/ddq bind these symbols with ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Every function returns int: DDQ_OK (0) or a negative DDQ_E* code; no C++
 *    exception and no exit() crosses the ABI.  ddq_last_error(ctx) returns the
 *    message of the last failure on that ctx (ctx == NULL: last global error).
 *  - The library owns all device memory.  Host pointers are borrowed for the
 *    duration of the call; a call that takes host buffers copies and
 *    synchronises before returning unless its name ends in _async.  A
 *    "*_on_device" flag != 0 means the pointer is a device pointer (e.g. a
 *    torch tensor's data_ptr()) and the copy is device-to-device.
 *  - One ddq_ctx per (process, GPU), bound to one HIP stream.  Calls on one
 *    ctx must be serialised by the caller; different ctxs are independent.
 *  - Float tensors cross the ABI in the reference's Caffe shapes/orders:
 *    parameters as one flat fp32 buffer in pycaffe net.params order
 *    (Qconv1.w, Qconv1.b, ..., Q_out.b), conv W (Cout,Cin,k,k), minibatch
 *    state/next_state (B,4,S,S), action (B,4,1,1) one-hot, reward and
 *    non_terminal (B,1,1,1).  Internal device layouts are private.
 */
#ifndef DDQ_HIP_H
#define DDQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDQ_ABI_VERSION 6   /* 5: ddq_step_cfg.reserved -> flags; ddq_synchronize reports a
                              small-map step's spin timeout as DDQ_ESTATE.
                              6: DDQ_STEP_REPEAT_CONV2_FWD removed (flag 2 is refused);
                              a timed-out step applies nothing; ddq_inject_fault,
                              ddq_small_path.  ABI 6 later gained the device actor
                              (ddq_actor_create, ddq_actor_step_async, ddq_actor_read):
                              new symbols only, nothing else changed; and then the
                              device evaluator (ddq_eval_create, ddq_eval_run_async,
                              ddq_eval_read), again new symbols only; and the
                              training monitor (ddq_monitor_enable,
                              ddq_monitor_record_async, ddq_monitor_read), likewise;
                              and the laned ring and actor pool (ddq_replay_set_lanes,
                              ddq_replay_lanes, ddq_actors_create,
                              ddq_actors_step_async, ddq_actors_read), likewise;
                              and the selectable objective (ddq_set_objective,
                              ddq_get_objective; blobs "Qn_out", "Q_out.diff"),
                              likewise; and n-step returns (ddq_replay_set_nstep,
                              ddq_replay_nstep), likewise; and prioritized replay
                              (ddq_replay_set_priority, ddq_replay_get_priority,
                              ddq_replay_priorities, ddq_replay_set_priorities,
                              ddq_replay_update_priorities_async; blob "is_weight"),
                              likewise; and the Adam rule (DDQ_RULE_ADAM, ddq_set_adam,
                              ddq_get_adam, ddq_adam_state; blob "grad_norm"),
                              likewise; and soft target updates (ddq_set_target_tau,
                              ddq_get_target_tau, ddq_soft_sync_target), likewise; and
                              checkpoint and resume (ddq_state_sections, ddq_state_read,
                              ddq_state_write, ddq_state_commit, ddq_state_digest),
                              likewise */

enum ddq_status {
  DDQ_OK = 0,
  DDQ_EINVAL = -1,   /* bad argument (sizes, names, B >= valid ...)          */
  DDQ_ENOMEM = -2,   /* device allocation failed                             */
  DDQ_EHIP = -3,     /* HIP runtime error                                    */
  DDQ_ERCCL = -4,    /* RCCL error                                           */
  DDQ_ESTATE = -5,   /* call not valid in the current state (no replay ...)  */
  DDQ_ERANGE = -6    /* data out of range (e.g. stored action >= num_actions) */
};

typedef struct ddq_ctx ddq_ctx;

/* Network description.  Replaces train_val.prototxt's MEMORY_DATA dims
 * (models/deepq/train_val.prototxt:2-37) and the GAMMA coefficient (:473). */
typedef struct ddq_net_desc {
  int32_t batch;        /* B, memory_data_param.batch_size (32)               */
  int32_t frame;        /* S, height == width (16 in deepq16); multiple of 8  */
  int32_t channels;     /* must be 4 (4-frame history, expgain.py:9)          */
  int32_t actions;      /* must be 4 (barista/constants.py:8)                 */
  float gamma;          /* 0.85 (train_val.prototxt:473)                      */
} ddq_net_desc;

/* One parameter blob of the flat layout (one tower).  Replaces iteration over
 * pycaffe net.params (messaging.py:57-66, server.py:238-244). */
typedef struct ddq_blob_desc {
  char name[16];        /* "Qconv1" ... "Q_out" (P tower: same with 'P')      */
  int32_t index;        /* 0 = weight, 1 = bias                               */
  int32_t shape[4];     /* Caffe-2014 4-D blob shape                          */
  int64_t offset;       /* element offset in the flat tower buffer            */
  int64_t count;        /* element count                                      */
} ddq_blob_desc;

/* Update rules of param-server/server.py:81-124 (+ Caffe SGDSolver momentum). */
enum ddq_rule {
  DDQ_RULE_SGD = 0,            /* server.py:81-83   theta -= lr*g             */
  DDQ_RULE_RMSPROP = 1,        /* server.py:86-105  lagged cache (default)    */
  DDQ_RULE_ADAGRAD = 2,        /* server.py:108-124                           */
  DDQ_RULE_MOMENTUM_CAFFE = 3, /* solver.prototxt:4-11 semantics (optional)   */
  DDQ_RULE_ADAM = 4            /* Adam + global-norm clip (ddq_set_adam below) */
};

typedef struct ddq_update_cfg {
  int32_t rule;          /* enum ddq_rule; DDQ_RULE_ADAM reads only lr below  */
  float lr;              /* server.py:268 default 1e-4 (momentum: base_lr)    */
  float decay;           /* rmsprop decay, server.py:270 default 0.9          */
  float eps;             /* 1e-8 inside the sqrt, server.py:105,124           */
  float momentum;        /* momentum rule only (0.9)                          */
  float weight_decay;    /* momentum rule only (0.0005)                       */
} ddq_update_cfg;

/* Gradient exchange of a data-parallel step (replaces the HTTP gradient POST
 * + server apply + model GET round trip, baristanet.py:85-133,
 * server.py:181-209).  Used when the ctx has a communicator (ddq_comm_init)
 * or belongs to an in-process group (ddq_group_init); ignored otherwise. */
enum ddq_exchange {
  DDQ_EXCHANGE_NONE = 0,
  /* W gradients computed at the same theta, summed, applied once (replicated
   * apply on every rank).  Equals the server applying W equally-stale SGD
   * gradients; a documented deviation for rmsprop/adagrad. */
  DDQ_EXCHANGE_ALLREDUCE = 1,
  /* Same semantics, sharded: reduce-scatter(sum) -> each rank applies its
   * 1/W shard (optimizer state sharded) -> all-gather of theta. */
  DDQ_EXCHANGE_SHARDED = 2,
  /* Param-server semantics (server.py:196-209): every rank owns a 1/W shard
   * and its optimizer state; gradient slices go all-to-all and the owner
   * applies the W gradients one by one in rank (ticket) order, exactly as
   * the server applies gradients on arrival; iteration += W per step; then
   * all-gather of theta.  Staleness within a step: 0..W-1 updates. */
  DDQ_EXCHANGE_SERVER = 3,
  /* Asynchronous param server (server.py:181-209 with free-running workers,
   * main.py:61-112): rank r owns shard r of the central model (and its
   * optimizer state).  A TICK is one push: worker w sends the gradient it
   * computed on the model it last pulled, the owners apply it on arrival
   * (iteration += 1), worker w pulls the owners' shards (and the central P
   * tower when a special-update pull happened since its last pull) and
   * immediately computes its next gradient while later ticks proceed.  The
   * arrival order is either round-robin (the deterministic schedule: one
   * step of ddq_step_async / ddq_step_graph_async / ddq_group_step = W ticks,
   * staleness W-1) or ticket order (ddq_async_tick with the worker whose
   * gradient was ready first, ddq_group_async_run): a fast worker pushes
   * more often than a slow one, as in the reference.  Once begun on a ctx,
   * only async steps / ticks run there. */
  DDQ_EXCHANGE_ASYNC = 4
};

/* One fused training step (main.py:61-103 debug_process_connection body,
 * minus acting): sample B indices (device RNG) -> gather -> P/Q forward ->
 * Bellman target + loss -> Q backward -> [exchange] -> apply ->
 * [P <- Q when the next pull sees iteration % target_period == 0]. */
typedef struct ddq_step_cfg {
  ddq_update_cfg update;
  int32_t target_period;   /* server.py:274 --special-update (10); 0 = never */
  int32_t exchange;        /* enum ddq_exchange                              */
  uint64_t seed;           /* device index-stream seed (per rank)            */
  int32_t overlap;         /* ALLREDUCE over RCCL: reduce the fc4 weight
                              bucket on a comm stream under the conv backward */
  int32_t flags;           /* DDQ_STEP_* bits, 0 = none                      */
} ddq_step_cfg;

/* Exchange-free steps: fc4's weight gradient (96 % of the parameters) is
 * computed and applied tile by tile inside the slab-reduce launch and NOT
 * stored to the gradient buffer (8.4 MB of writes per step at 64x64), so
 * ddq_get_grads after such a step returns that block of an earlier step
 * (at S = 16 the block is stored regardless: the fused step's last launch
 * applies it from there).
 * The update is unchanged, bit for bit.  No effect on exchanged steps (their
 * gradient is what is exchanged) nor on DDQ_RULE_ADAM steps (the gradient
 * buffer is the Adam launch's input). */
#define DDQ_STEP_NO_GRAD_STORE 1

/* ---------------- context ---------------------------------------------- */
/* caffe.Net(prototxt, model) + set_mode_gpu + set_phase_test
 * (baristanet.py:16, main.py:147-151).  Dropout is identity (TEST phase).
 * DDQ_EINVAL unless desc->frame is a multiple of 8 in [16, 128] (the backward
 * pass has no form for wider maps) and desc->batch is in [1, 1024]; checked
 * before any device is looked for. */
int ddq_create(ddq_ctx** out, int device, const ddq_net_desc* desc);
int ddq_destroy(ddq_ctx* ctx);
const char* ddq_last_error(const ddq_ctx* ctx);
int ddq_abi_version(void);
/* Use an external HIP stream (e.g. torch.cuda.current_stream().cuda_stream). */
int ddq_set_stream(ddq_ctx* ctx, void* hip_stream);
/* The ctx's HIP stream (e.g. for torch.cuda.ExternalStream events). */
int ddq_get_stream(const ddq_ctx* ctx, void** hip_stream);
/* Wait for the ctx's streams.  DDQ_ESTATE when a small-map (S = 16) step's
 * inter-workgroup meeting timed out since the last call.  The launches went
 * on (no hang) but wrote no parameter, optimizer state, P copy or iteration
 * from that step on (a fused-apply step; an exchanged step's gradient is
 * invalid); this call clears the flag, restarts the meeting counters and
 * takes the device iteration back, so the ctx steps on from the last good
 * update. */
int ddq_synchronize(ddq_ctx* ctx);

/* Failpoints for the error paths' tests (no reference counterpart). */
enum ddq_fault {
  DDQ_FAULT_NONE = 0,          /* disarm                                        */
  /* the next eager step (ddq_step_async) launches its fc4 chain one workgroup
   * short, so the fan-in meeting times out: ddq_synchronize must then return
   * DDQ_ESTATE with the model unchanged.  Small-map ctxs only (DDQ_ESTATE
   * otherwise). */
  DDQ_FAULT_MEET_TIMEOUT = 1
};
int ddq_inject_fault(ddq_ctx* ctx, int32_t fault);

/* 1 when the ctx runs the four-launch small-map step (S = 16, B <= 256, and
 * every meeting launch's workgroups fit the device at once: checked with the
 * occupancy API at ddq_create), 0 when it runs the general kernels; why
 * (nullable, cap bytes) receives the reason it is off. */
int ddq_small_path(const ddq_ctx* ctx, char* why, int32_t cap);

/* ---------------- parameters ------------------------------------------- */
/* Number of fp32 parameters of ONE tower (228,132 at S=16,
 * results/cost-vs-image-size.txt:2). */
int64_t ddq_num_params(const ddq_ctx* ctx);
/* net.params names/shapes/offsets (Q tower; P identical with prefix 'P'). */
int ddq_param_layout(const ddq_ctx* ctx, ddq_blob_desc* out, int32_t cap, int32_t* n);
/* .data / .diff .flat[:] access (messaging.py:66,111).  which: 0 = Q, 1 = P. */
int ddq_set_params(ddq_ctx* ctx, int32_t which, const float* src, int64_t n, int32_t src_on_device);
int ddq_get_params(ddq_ctx* ctx, int32_t which, float* dst, int64_t n, int32_t dst_on_device);
int ddq_get_grads(ddq_ctx* ctx, float* dst, int64_t n, int32_t dst_on_device);
int ddq_set_grads(ddq_ctx* ctx, const float* src, int64_t n, int32_t src_on_device);
/* special_update_transform_model (server.py:127-137): P <- Q. */
int ddq_sync_target(ddq_ctx* ctx);
/* Soft target updates (Polyak averaging).  tau in (0, 1], default 1; DDQ_EINVAL
 * for tau <= 0, tau > 1 or NaN.  With tau < 1 every target sync a step performs
 * (the update after which iteration % target_period == 0) writes
 *   P' = P + tau * (Q' - P)
 * instead of P' = Q': three fp32 operations, each rounded on its own, Q' the
 * value the step just gave theta_Q; the conv weights' derived copies of P follow
 * the blended value.  tau = 1 is the hard copy, exactly as before.  The
 * iteration-0 sync of the first step and ddq_sync_target stay hard copies.
 * target_period = 1 is the usual every-update Polyak rule; period k blends on
 * every k-th update.  Holds for eager, graph and pipelined steps, for no
 * exchange, all-reduce, sharded and server; DDQ_EXCHANGE_ASYNC refuses tau < 1
 * with DDQ_EINVAL (its P travels by pulls).  tau is a launch argument: setting
 * it drops every captured graph. */
int ddq_set_target_tau(ddq_ctx* ctx, float tau);
int ddq_get_target_tau(const ddq_ctx* ctx, float* tau);
/* The host-driven soft update beside ddq_sync_target: one launch blends all of
 * P towards Q with the context's tau (the same rounding) and rewrites P's
 * derived conv-weight copies.  With tau = 1 it is ddq_sync_target. */
int ddq_soft_sync_target(ddq_ctx* ctx);

/* ---------------- replay (replay.py) ----------------------------------- */
/* ReplayDataset.__init__ storage (replay.py:48-61), HBM resident, zeroed. */
int ddq_replay_create(ddq_ctx* ctx, int64_t capacity);
/* add_experience (replay.py:70-92); state == NULL marks a terminal step and
 * leaves the slot stale.  state: 4*S*S uint8 (C,H,W). */
int ddq_replay_add(ddq_ctx* ctx, int32_t action, int32_t reward, const uint8_t* state);
int ddq_replay_info(const ddq_ctx* ctx, int64_t* head, int64_t* valid, int64_t* capacity);
/* Laned ring: the capacity slots become `lanes` contiguous lanes of lane_len =
 * capacity / lanes slots; lane g is slots [g lane_len, (g + 1) lane_len) and a
 * ring of its own, so the ring holds `lanes` trajectories (s' of slot i is the
 * next slot within i's lane, the lane's last slot wrapping to its first).
 * Only lock-step writers fill a laned ring (ddq_actors_*), so all lanes share
 * one head in [0, lane_len) and one valid in [0, lane_len]: on a laned ring
 * ddq_replay_info returns these per-lane values (and the total capacity), and
 * ddq_replay_import takes them (head < lane_len, valid <= lane_len; data in
 * slot order, as ddq_replay_export writes it).  Sampling draws uniformly over
 * the lanes * valid filled slots without every lane's slot head - 1 (head >= 1),
 * and needs B <= lanes * (valid - 1) (DDQ_EINVAL otherwise; at lanes == 1 this
 * is B < valid).  ddq_replay_sample accepts slot i iff i mod lane_len < valid.
 * The ring must exist and be empty (DDQ_ESTATE); capacity % lanes == 0 and
 * lane_len >= 2 (DDQ_EINVAL).  lanes == 1 is the plain ring and changes
 * nothing.  With lanes > 1, ddq_replay_add, ddq_replay_fill_tiled,
 * ddq_replay_sample_batch_async, ddq_replay_gather_batch_async and
 * ddq_actor_create return DDQ_ESTATE. */
int ddq_replay_set_lanes(ddq_ctx* ctx, int32_t lanes);
int ddq_replay_lanes(const ddq_ctx* ctx, int32_t* lanes, int64_t* lane_len);
/* n-step returns.  The ring's n-step length n (1 by default, reset to 1 by
 * ddq_replay_create) changes which slots a draw may pick and what the gather
 * assembles; the head, the step modes and the exchanges are the same, because
 * the head's target gamma * (P_sel * non_terminal) + reward is the n-step
 * target when the gather hands it the discounted reward sum as reward, the
 * remaining discount as non_terminal and s_{t+m} as next_state.  At n = 1 every
 * launch and every bit is what it is without this call.
 *
 * Per lane: L = lane_len, v = valid, h = head, x = the lane-local index of a
 * sample's slot, base = lane * L (a plain ring: base 0, L = capacity).
 *
 * Allowed start slots.  For x in [0, v):
 *     d = h - 1 - x
 *     if (d < 0 && n >= 2 && v == L) d += L      full ring: the window wraps onto the head
 *     forbidden(x)  <=>  0 <= d < n
 * n = 1: x == h - 1, nothing at h == 0 (the reference's rule).  n >= 2: no
 * window reaches the write head, also across the wrap of a full ring.  Allowed
 * slots per lane, A: v - 1 at n = 1; L - n at n >= 2, v == L; at n >= 2, v < L:
 * v - |[max(0, h - n), h - 1] n [0, v)|.  Every draw needs B <= lanes * A
 * (DDQ_EINVAL otherwise; the large-batch sampler n_batch <= A as well as
 * n_batch <= valid / 2).
 *
 * The window of x.  s_k = base + (x + k) mod L, k = 1..n (s_1 is the next slot).
 *     m = the smallest k in 1..n with non_terminal[s_k] == 0, else n
 *     g = 1.0f;  R = (float)reward[s_1]
 *     for k = 2..m:  g = g * gamma;  R = R + g * (float)reward[s_k]
 *     w = 0.0f if a terminal was found, else gamma^(n-1), n - 1 repeated
 *         multiplications from 1.0f
 * every * and + an fp32 operation rounded on its own (no fused multiply-add),
 * gamma = ddq_net_desc.gamma.  The minibatch is
 *     state <- S[base + x]        next_state <- S[s_m]
 *     action <- one-hot of action[s_1] (>= 4: the sticky error of ddq_replay_status)
 *     reward[b] <- R              non_terminal[b] <- w
 * so ddq_read_minibatch's non_terminal is w and its reward is R, blob "P_sa"
 * carries the factor w, and "target_Q_sa" = gamma * (P_sel * w) + R.  A start
 * slot that is itself a terminal slot stays drawable, as in the reference.
 *
 * ddq_replay_set_nstep synchronises and drops captured graphs; it is legal on
 * a filled ring.  DDQ_ESTATE: no ring, or the async exchange has begun.
 * DDQ_EINVAL: n < 1, n > DDQ_NSTEP_MAX or n >= lane_len.  ddq_replay_set_lanes
 * refuses (DDQ_EINVAL) a lane count that would make lane_len <= n.
 * ddq_replay_sample at n >= 2 refuses a forbidden index (DDQ_EINVAL); at n = 1
 * it accepts what it always did.  n is a property of sampling, not of the data:
 * it is not stored with the ring. */
#define DDQ_NSTEP_MAX 8
int ddq_replay_set_nstep(ddq_ctx* ctx, int32_t n);
int ddq_replay_nstep(const ddq_ctx* ctx, int32_t* n);
/* Proportional prioritized replay (Schaul et al. 2016; no reference counterpart).
 * Off by default; while off every launch and every bit is what it is without
 * this section.  While on, the device draws (the step modes,
 * ddq_replay_sample_device_async) pick slots in proportion to a per-slot
 * priority kept in a device sum tree, the head scales each sample's dQ and loss
 * term by an importance-sampling weight, and every step commits |TD| back.
 *
 * Priorities are integers.  Slot i has a leaf q[i], a uint32: 0, or a value in
 * [1, 2^24] read as fixed point with 16 fraction bits (65536 = 1.0).  All sums
 * are uint64 and exact, so nothing depends on the tree's shape, the order of a
 * reduction or of the atomics.
 *
 * Invariant, after every call or launch that changes the ring or n:
 *     q[i] == 0  <=>  slot i is unfilled or forbidden
 * with `forbidden` the n-step rule above on the ring's current head, valid,
 * lane_len and n, per lane.  A zero leaf is never drawn, so the prioritized draw
 * has no rejection and no redraw rounds.
 *
 * Writers.  After an add at lane-local slot h (lane length L, n-step length n),
 * with head' and valid' the lane's values after the add: q[h] <- 0 if h is
 * forbidden under head' / valid' (always, except at n = 1 when head' wrapped to
 * 0: the n = 1 rule forbids nothing there and the slot is allowed at once, so it
 * takes pmax); x = h - n, taken mod L when valid' == L; if x >= 0 and q[x] == 0,
 * q[x] <- pmax (x is the slot whose window just left the head).  pmax is the
 * largest priority ever committed or set since the last rebuild, at least
 * 65536.  ddq_replay_add, the device actor and the actor pool follow it.
 * A rebuild sets pmax = 65536, every filled, allowed slot to pmax and the rest
 * to 0: on enabling, ddq_replay_import, ddq_replay_fill_tiled,
 * ddq_replay_set_nstep and ddq_replay_set_lanes.  Priorities are a property of
 * sampling, like n: they are not stored with the ring or in the HDF5 file.
 *
 * Draw ctr with seed `seed`: B samples, possibly with duplicates (idx, the index
 * log and ddq_read_indices may repeat a slot), sorted by construction.
 *     T    = sum of all leaves              (B <= lanes * A as for every draw, so T >= B)
 *     lo_j = (T * j) / B      j = 0..B      uint64 floor division
 *     r_j  = splitmix64(seed ^ splitmix64(ctr * 0x100000001B3 + j * 0x9E37))
 *     u_j  = lo_j + mulhi64(r_j, lo_{j+1} - lo_j)
 *     idx_j = the slot i with C(i) <= u_j < C(i+1), C the exclusive prefix sum
 *             of q over slots 0..capacity-1
 *     qmin = min_j q[idx_j];  isw_j = powf((float)qmin / (float)q[idx_j], beta)
 * (N and T cancel under the batch-max normalisation; beta == 0 gives exactly
 * 1.0f.)  isw is a per-minibatch buffer right behind reward, blob "is_weight" (B).
 * ddq_replay_sample (host indices) and ddq_write_minibatch set it to 1.0f.  The
 * large-batch sampler stays uniform.
 *
 * Head, per image b, with c = d (or clamp(d) under Huber) as above:
 *     t = c / (float)B;  dQ scale = isw_b * t;  loss term = isw_b * le_b
 * each product rounded on its own; with isw == 1.0f the pass is bit for bit the
 * unweighted one.
 *
 * Commit, after a pass, for b = 0..B-1 and i = idx[b]:
 *     d = Q_sa[b] - target_Q_sa[b];  p = powf(fabsf(d) + eps, alpha)
 *     v = clamp(rintf(p * 65536.0f), 1, 2^24)       (non-finite p: 2^24)
 * q[i] <- v only if q[i] != 0 (a slot an actor has since made forbidden is not
 * resurrected); a slot that appears more than once takes its highest b;
 * pmax <- max(pmax, v) over the values written.  Every step mode commits its
 * own step (one one-workgroup launch after the head, "prio_commit" in
 * ddq_profile_step, which in a pipelined chain also draws the next step's set):
 * draw d+1 sees the commits of every step <= d and every add enqueued before
 * it, in eager, graph and pipelined mode alike.  An eager step begins with
 * "prio_sample" and "gather".
 *
 * ddq_replay_set_priority, enabled 0 -> 1: synchronises, drops captured graphs,
 * allocates the tree and rebuilds.  1 -> 0 frees it.  Called while enabled it
 * only rewrites alpha, beta and eps in device memory, stream-ordered (no
 * synchronisation, no rebuild, no graph drop: the beta-annealing path; captured
 * graphs read them live).  DDQ_EINVAL: alpha or beta outside [0, 1] or not
 * finite, eps <= 0 or not finite, B > 256.  DDQ_ESTATE: no ring, a communicator
 * or group is attached, the async exchange has begun.  While enabled,
 * exchanged steps, ddq_group_step, ddq_group_async_*, ddq_async_begin,
 * ddq_comm_init and ddq_group_init return DDQ_ESTATE. */
typedef struct ddq_priority_cfg { int32_t enabled; float alpha, beta, eps; } ddq_priority_cfg; /* 16 B */
int ddq_replay_set_priority(ddq_ctx* ctx, const ddq_priority_cfg* cfg);
int ddq_replay_get_priority(const ddq_ctx* ctx, ddq_priority_cfg* cfg);
/* The commit above for the bound minibatch after ddq_forward_backward: enqueued,
 * no sync.  DDQ_ESTATE when disabled or when no device-side index set is bound
 * (the minibatch came from ddq_write_minibatch, or the ring was rebuilt). */
int ddq_replay_update_priorities_async(ddq_ctx* ctx);
/* Synchronise and read: leaves (n == capacity), the root, pmax; any pointer may
 * be NULL.  DDQ_ESTATE while disabled. */
int ddq_replay_priorities(ddq_ctx* ctx, uint32_t* leaves, int64_t n, uint64_t* total, uint32_t* pmax);
/* Synchronise, overwrite leaves idx[k] <- q[k] and fix the sums; pmax rises to
 * the largest value set.  DDQ_EINVAL: a nonzero value on a zero leaf, zero on a
 * nonzero leaf, q > 2^24, idx out of range. */
int ddq_replay_set_priorities(ddq_ctx* ctx, const int32_t* idx, const uint32_t* q, int32_t n);
/* Bulk load / store of the ring (the HDF5 datasets of replay.py:48-61,
 * persisted by __del__ :185-192). */
int ddq_replay_import(ddq_ctx* ctx, const uint8_t* state, const uint8_t* action,
                      const int16_t* reward, const uint8_t* non_terminal,
                      int64_t n, int64_t head, int64_t valid);
int ddq_replay_export(ddq_ctx* ctx, uint8_t* state, uint8_t* action, int16_t* reward,
                      uint8_t* non_terminal, int64_t n);
/* sample_direct (replay.py:144-183) given the sorted index list the host
 * drew (replay.py:152-159): assembles the device minibatch bit-exactly.
 * Returns DDQ_EINVAL if B >= valid (replay.py:147-150). */
int ddq_replay_sample(ddq_ctx* ctx, const int32_t* sorted_idx, int32_t batch);
/* Device-RNG draw of B distinct indices in [0,valid) \ {head-1}, sorted,
 * then the same gather (perf mode).  Enqueued, no sync. */
int ddq_replay_sample_device_async(ddq_ctx* ctx, uint64_t seed);
/* Copy the current device minibatch out in Caffe shapes (baristanet.py:30-34). */
int ddq_read_minibatch(ddq_ctx* ctx, float* state, float* action, float* reward,
                       float* next_state, float* non_terminal);
/* Set the minibatch directly (set_input_arrays binding, baristanet.py:41-43;
 * dummy_load_minibatch :70-83). */
int ddq_write_minibatch(ddq_ctx* ctx, const float* state, const float* action,
                        const float* reward, const float* next_state,
                        const float* non_terminal);
/* Fill the whole ring by tiling `pool` transitions (slot i <- pool entry
 * i % pool) on the device, then set head/valid: the 1M-slot HBM replay of
 * SURVEY 8(d) C5 without a 16 GB host image.  Host arrays of `pool` entries. */
int ddq_replay_fill_tiled(ddq_ctx* ctx, const uint8_t* state, const uint8_t* action,
                          const int16_t* reward, const uint8_t* non_terminal, int64_t pool,
                          int64_t head, int64_t valid);
/* Large-batch sample_direct (replay.py:144-183) for n <= valid/2 (any n, not
 * tied to the net batch): device draw of n distinct indices uniform over
 * [0,valid) \ {head-1}, sorted, written to idx; then s <- S[idx],
 * s' <- S[idx+1] (N-1 wraps to 0) as f32 (n,4,S,S), one-hot action (n,4),
 * reward (n), non_terminal (n) of idx+1.  ALL pointers are device pointers
 * (e.g. torch tensors).  The first call allocates the sampler's bitmap
 * (capacity/8 bytes).  Enqueued, no sync; ddq_replay_status reports a
 * stored action >= 4 or a failed draw. */
int ddq_replay_sample_batch_async(ddq_ctx* ctx, int32_t n, uint64_t seed, int32_t* idx,
                                  float* state, float* action, float* reward,
                                  float* next_state, float* non_terminal);
/* The same Caffe-layout gather for a caller-given sorted index list (device). */
int ddq_replay_gather_batch_async(ddq_ctx* ctx, const int32_t* idx, int32_t n, float* state,
                                  float* action, float* reward, float* next_state,
                                  float* non_terminal);
/* Synchronise and report (then clear) the replay's sticky device error flag. */
int ddq_replay_status(ddq_ctx* ctx);
/* Last sorted index list used by the gather (device -> host). */
int ddq_read_indices(ddq_ctx* ctx, int32_t* idx, int32_t batch);
/* Device index draws made so far (the device RNG stream position; reset by
 * ddq_replay_create).  Draw d is the minibatch of the (d+1)-th device-drawn
 * step of this ctx. */
int ddq_replay_draws(ddq_ctx* ctx, int64_t* draws);
/* Debug / parity log of the device draws: every device-drawn sorted index
 * set d (sample kernels, fused step draws, pipelined prefetches) is also
 * written to a device ring of `draws` entries of B int32 (0 disables).  Lets a
 * checker replay exactly the minibatches a graph-captured chain trained on
 * (the role of replay.py:152-159's host index list).  Invalidates graphs. */
int ddq_index_log_enable(ddq_ctx* ctx, int64_t draws);
/* Copy draws [first, first+n) (each B sorted int32) out of the log; they must
 * be among the last `draws` made. */
int ddq_index_log_read(ddq_ctx* ctx, int64_t first, int64_t n, int32_t* out);

/* ---------------- compute ---------------------------------------------- */
/* net.forward(); net.backward() (baristanet.py:138-140).  loss may be NULL. */
int ddq_forward_backward(ddq_ctx* ctx, float* loss);
int ddq_forward_backward_async(ddq_ctx* ctx);
/* forward(end='Q_out') over the bound minibatch (baristanet.py:144). */
int ddq_forward_q(ddq_ctx* ctx);
/* net.blobs[name].data for name in {"Q_out","P_out","Q_sa","P_sa",
 * "target_Q_sa","loss"} (B*4, B*4, B, B, B, 1 floats); and, with no reference
 * counterpart, "Q_out.diff" (B*4): the head's dQ of the last pass (the diff the
 * loss layer hands to Q_out), and "Qn_out" (B*4): Q(s',.) under theta_Q of the
 * last pass with the double target (DDQ_ESTATE under DDQ_TARGET_MAX: nothing
 * computed it), and "grad_norm" (1): the pre-clip gradient norm of the last
 * clipped Adam apply (DDQ_ESTATE unless ddq_set_adam turned clipping on). */
int ddq_read_blob(ddq_ctx* ctx, const char* name, float* dst, int64_t n);
/* Argmax/ReLU routing bytes of pool layer 1..3 of the Q tower for the last
 * forward_backward, in Caffe (B,C,H/2,W/2) order: 0..3 = first-max position
 * in the 2x2 window (row-major), 4 = window max <= 0 (no gradient). */
int ddq_read_pool_mask(ddq_ctx* ctx, int32_t layer, uint8_t* dst, int64_t n);
/* select_action (baristanet.py:142-146) for n states (n <= B, uint8 C,H,W):
 * argmax_a Q(s,a), first max wins.  Does not touch the bound minibatch. */
int ddq_select_action(ddq_ctx* ctx, const uint8_t* states, int32_t n, int32_t* actions);

/* ---------------- selectable TD objective (no reference counterpart) ------- */
/* The reference trains on target = r + gamma max_a P(s',a) nt under a Euclidean
 * loss (train_val.prototxt:385-483); that is the default, {MAX, EUCLIDEAN}, and
 * with it every launch and every bit is what it is without this section.
 * Per image b, in fp32 as the head computes:
 *   MAX     P_sa = max_a P_out[b][a] * nt
 *   DOUBLE  a* = first maximum of Qn_out[b][0..3] (select_action's rule), where
 *           Qn_out = Q(s',.) under theta_Q; P_sa = P_out[b][a*] * nt
 *   target = gamma P_sa + r,  d = Q_sa - target
 *   EUCLIDEAN  dQ[b][a] = act[b][a] d / B;  loss = sum_b d^2 / (2B)
 *   HUBER      dQ[b][a] = act[b][a] clamp(d, -delta, delta) / B;
 *              loss = sum_b h(d_b) / B, h(d) = d^2/2 for |d| <= delta, else
 *              delta (|d| - delta/2)
 * With DOUBLE every pass begins with a forward-only run of the Q tower over the
 * minibatch's next_state (ddq_forward_q's kernels at n = B, on the ctx stream,
 * in the acting scratch) into a buffer of its own, "Qn_out".  The objective is a
 * property of the ctx, honoured by every call that computes a gradient
 * (ddq_forward_backward[_async], the step modes, ddq_profile_step -- the extra
 * forward's kernels are listed as "qn_<name>" --, the group and exchanged steps,
 * and the async exchange for an objective set before ddq_async_begin). */
enum ddq_target { DDQ_TARGET_MAX = 0, DDQ_TARGET_DOUBLE = 1 };
enum ddq_loss   { DDQ_LOSS_EUCLIDEAN = 0, DDQ_LOSS_HUBER = 1 };
typedef struct ddq_objective {      /* 16 bytes */
  int32_t target;        /* enum ddq_target */
  int32_t loss;          /* enum ddq_loss */
  float   huber_delta;   /* HUBER: finite, > 0; ignored otherwise */
  int32_t reserved;      /* 0 */
} ddq_objective;
/* Synchronises, invalidates graphs, and does the extra forward's one-time
 * set-up (so none of it happens inside a capture).  DDQ_EINVAL: unknown enum
 * value, huber_delta not finite or <= 0 with HUBER, reserved != 0.  DDQ_ESTATE:
 * the async exchange has begun on the ctx. */
int ddq_set_objective(ddq_ctx* ctx, const ddq_objective* obj);
int ddq_get_objective(const ddq_ctx* ctx, ddq_objective* obj);

/* ---------------- device-resident actor (expgain.py, gamesim/SnakeGame.py) -- */
/* The worker's "act once, add the transition" (main.py:61-103) without the
 * host in it: one actor per ctx = one Snake game + the ctx's ring + its Q tower
 * (a ring holds one trajectory: sample_direct takes s' from slot idx+1).
 * Random numbers: draw k (k = 0, 1, ...) of an actor is
 * r_k = splitmix64(seed ^ splitmix64(k)); random() = (r >> 11) * 2^-53,
 * randrange(n) = high 64 bits of r * n, choice(seq) = seq[randrange(len)];
 * one draw each, in program order: coin, action when exploring, apple when
 * eaten (ddq.actor.ActorRng is the same stream on the host).  Actions are
 * the reference's ["w","a","s","d"] = 0..3; the stored action is that index. */
/* ExpGain.__init__ / reset_game (expgain.py:30-66) on the device.
 * init_board: 100 int8 board codes [x*10+y] as SnakeGame.encode_state writes
 * them (-1 empty, -2 apple, k = k-th cell from the head); the start of every
 * game (the reference resets to the same init_state, apple included).
 * row_map/col_map: S entries each in [0,10): frame pixel (i,j) shows board
 * cell (row_map[i], col_map[j]) -- the nearest-neighbour zoom of
 * expgain.py:12-18, computed by the caller from its own preprocessor.
 * Needs a replay ring (DDQ_ESTATE otherwise).  Calling it again resets. */
int ddq_actor_create(ddq_ctx* ctx, const int8_t* init_board, const int32_t* row_map,
                     const int32_t* col_map, uint64_t seed);
/* nsteps x generate_experience(iter_num) (expgain.py:82-111): Q forward of the
 * current 4-frame state, epsilon-greedy action at epsilon(iter_num), one game step,
 * add_experience into the ring.  Enqueued on the ctx stream, no sync; the
 * ring's head / valid (ddq_replay_info) advance by nsteps at once. */
int ddq_actor_step_async(ddq_ctx* ctx, int32_t nsteps, int64_t iter_num);
/* Synchronise; boards: 4*100 int8, oldest frame first; stats[4]: steps taken,
 * games ended, sum of rewards, RNG draws consumed.  Either may be NULL. */
int ddq_actor_read(ddq_ctx* ctx, int8_t* boards, int64_t* stats);

/* ---------------- device-resident policy evaluation (evaluation.py:10-51) -- */
/* PolicyEvaluator.evaluate without the host between the moves: ngames <= B
 * independent Snake games in lock step on this ctx.  One move of all games is
 * the Q forward of their states at n = ngames and one environment kernel (one
 * workgroup per game); no copy, no synchronisation.  No replay ring is needed
 * or touched, nor the bound minibatch, the actor or the step counters.
 * Random numbers: game i has the actor's kind of stream on
 * game_seed(seed, i) = splitmix64(splitmix64(seed) ^ i).  Draws per move, in
 * program order: the coin (only when epsilon > 0: epsilon = 0 is the
 * reference's greedy evaluation and draws none), the action when exploring
 * ((r >> 11) < ceil(epsilon * 2^53)), the apple when one is eaten.  The greedy
 * action is the first maximum of the game's own four Q values.
 * An episode of game i ends when the game is over, or (max_moves > 0) with its
 * max_moves-th move; game over wins when both happen at once; the final -1 is
 * part of the score.  The game then restarts from its own init board
 * (init_boards: ngames * 100 board codes as ddq_actor_create's, checked alike)
 * and appends one record of four int32 to its own log of max_episodes entries:
 * end_move (the lock-step move index, from 0, counted per game on the device),
 * score, moves, ended_by (0 game over, 1 max_moves).  A game whose log is full
 * is idle: it plays, draws and renders nothing more.  The evaluator's result
 * is defined on the logs: all records sorted by (end_move, game index), the
 * first num_trials of them -- the order in which the host evaluator counts.
 * Calling it again resets the evaluator. */
int ddq_eval_create(ddq_ctx* ctx, int32_t ngames, const int8_t* init_boards,
                    const int32_t* row_map, const int32_t* col_map, uint64_t seed,
                    double epsilon, int32_t max_moves, int32_t max_episodes);
/* nmoves lock-step moves, enqueued on the ctx stream, no sync. */
int ddq_eval_run_async(ddq_ctx* ctx, int32_t nmoves);
/* Synchronise.  stats[4]: lock-step moves enqueued, episodes logged, sum of
 * all rewards, RNG draws over all games; episodes: ngames record counts; log:
 * ngames * max_episodes * 4 int32 (unused entries 0); boards: ngames * 4 * 100
 * int8, oldest frame first; draws: ngames stream positions.  Every output
 * pointer may be NULL. */
int ddq_eval_read(ddq_ctx* ctx, int64_t* stats, int32_t* episodes, int32_t* log,
                  int8_t* boards, uint64_t* draws);

/* ---------------- device actor pool: N lock-step actors, one ring lane each -- */
/* ngames actors (each ddq_actor_create's game, rules and draws: the coin is
 * always drawn) play in lock step and add into a laned ring, game g into lane
 * g.  One move of all games is the Q forward of their states at n = ngames and
 * one environment kernel (one workgroup per game): ngames transitions for about
 * the price of one; no copy, no synchronisation.  Game i's stream is the
 * actor's on game_seed(seed, i), as the evaluator's.  Needs a ring with
 * lanes == ngames (DDQ_EINVAL otherwise; DDQ_ESTATE without a ring) and
 * ngames <= B.  init_boards: ngames * 100 board codes; boards and maps as
 * ddq_actor_create's, checked alike.  The games write from the ring's per-lane
 * head / valid at this call.  Calling it again resets the games and leaves the
 * ring as it is. */
int ddq_actors_create(ddq_ctx* ctx, int32_t ngames, const int8_t* init_boards,
                      const int32_t* row_map, const int32_t* col_map, uint64_t seed);
/* nmoves lock-step moves at epsilon(iter_num), enqueued on the ctx stream, no
 * sync; the ring's per-lane head / valid (ddq_replay_info) advance by nmoves
 * at once. */
int ddq_actors_step_async(ddq_ctx* ctx, int32_t nmoves, int64_t iter_num);
/* Synchronise.  boards: ngames * 4 * 100 int8, oldest frame first; stats:
 * ngames * 4, per game ddq_actor_read's (steps, games ended, reward sum, RNG
 * draws); totals[4]: their sums over the games.  Every pointer may be NULL. */
int ddq_actors_read(ddq_ctx* ctx, int8_t* boards, int64_t* stats, int64_t* totals);

/* ---------------- apply (param server) --------------------------------- */
/* apply_descent + update_fn (server.py:49-124) on the Q tower with the
 * current gradient buffer.  Optimizer state lives on device. */
int ddq_apply(ddq_ctx* ctx, const ddq_update_cfg* cfg);
int ddq_apply_async(ddq_ctx* ctx, const ddq_update_cfg* cfg);
/* Forget rmsprop/adagrad/momentum/Adam state (server.py:229-231 clear()). */
int ddq_reset_optimizer(ddq_ctx* ctx);
int ddq_get_optimizer_state(ddq_ctx* ctx, float* dst, int64_t n);

/* ---------------- Adam with global-norm gradient clipping ------------------ */
/* (Kingma & Ba 2015; torch.optim.Adam without amsgrad or weight decay; no
 * reference counterpart.)  DDQ_RULE_ADAM keeps two state words per parameter:
 * the first moment m in the buffer every rule uses (ddq_get_optimizer_state
 * returns it) and the second moment v in a buffer ddq_set_adam allocates.
 * Per element, in fp32, every operation rounded on its own (no fused
 * multiply-add), with lr from ddq_update_cfg and the rest from ddq_adam_cfg:
 *     omb1 = (float)(1.0 - (double)beta1)          omb2 likewise
 *     c1   = (float)(1.0 - pow((double)beta1, (double)t))   c2 likewise
 *     g'   = s * g                       (only when clipping is on)
 *     m    = beta1 * m + omb1 * g'       (first apply after a reset: m = v = 0)
 *     v    = beta2 * v + omb2 * (g' * g')
 *     theta = theta - (lr * (m / c1)) / (sqrtf(v / c2) + eps)
 * t is the device iteration counter after the apply's bookkeeping: the number of
 * updates applied since ddq_reset_optimizer, this one included.  The Adam launch
 * reads it from device memory, so captured graphs replay it.  A ctx that changes
 * its rule should call ddq_reset_optimizer: the other rules read m as their
 * state word, and t counts every rule's updates.
 * Clipping (max_grad_norm = c > 0): one launch before the apply ("grad_norm" in
 * ddq_profile_step) sums the squares of the gradient buffer in double, a fixed
 * number of partials in a fixed order, no atomics; the Adam launch ("adam_apply")
 * adds the partials in index order, nrm = (float)sqrt(total),
 * s = nrm > c ? c / nrm : 1.0f.  The gradient buffer is not modified
 * (ddq_get_grads and the monitor see g); under DDQ_EXCHANGE_ALLREDUCE the norm is
 * that of the summed gradient.  ddq_read_blob("grad_norm", 1) returns the last
 * nrm (DDQ_ESTATE with clipping off).
 * An Adam step runs the gradient launches and then the apply launch, the
 * sequencing of an exchanged step (no update inside the slab-reduce launch), in
 * eager, graph and pipelined mode, with every objective, n and prioritized
 * replay.  DDQ_RULE_ADAM before ddq_set_adam: DDQ_ESTATE.  With
 * DDQ_EXCHANGE_SHARDED, DDQ_EXCHANGE_SERVER or DDQ_EXCHANGE_ASYNC (they shard
 * one state buffer and apply W gradients per launch; not supported here) and in
 * ddq_async_begin: DDQ_EINVAL, nothing changes.  DDQ_EXCHANGE_NONE and
 * DDQ_EXCHANGE_ALLREDUCE (RCCL and the in-process group) work. */
typedef struct ddq_adam_cfg {   /* 16 bytes */
  float beta1, beta2;           /* in [0, 1)                                    */
  float eps;                    /* finite, > 0; added outside the sqrt          */
  float max_grad_norm;          /* 0 = no clipping; else finite, > 0            */
} ddq_adam_cfg;
/* The first call synchronises, drops captured graphs and allocates v (zeroed);
 * later calls only change the constants, and also drop graphs.  DDQ_EINVAL: a
 * value out of range.  DDQ_ESTATE: the async exchange has begun. */
int ddq_set_adam(ddq_ctx* ctx, const ddq_adam_cfg* cfg);
/* DDQ_ESTATE before ddq_set_adam. */
int ddq_get_adam(const ddq_ctx* ctx, ddq_adam_cfg* cfg);
/* Synchronise and read m and v (n == ddq_num_params) and t; any pointer may be
 * NULL.  DDQ_ESTATE before ddq_set_adam.  ddq_reset_optimizer zeroes all three. */
int ddq_adam_state(ddq_ctx* ctx, float* m, float* v, int64_t n, int64_t* t);

/* ---------------- communication (RCCL over xGMI) ----------------------- */
/* Replace the HTTP/Redis gradient round trip (baristanet.py:105-123,
 * server.py:196-209) with a sum all-reduce of the flat gradient buffer. */
int ddq_comm_get_unique_id(uint8_t id[128]);
int ddq_comm_init(ddq_ctx* ctx, const uint8_t id[128], int32_t nranks, int32_t rank);
int ddq_allreduce_grads(ddq_ctx* ctx);
int ddq_allreduce_grads_async(ddq_ctx* ctx);

/* ---------------- fused step + graphs ---------------------------------- */
int ddq_step_async(ddq_ctx* ctx, const ddq_step_cfg* cfg);
/* Capture one step into a hipGraph (re-captured when cfg changes) and replay
 * it nsteps times back to back.  Enqueued, no sync. */
int ddq_step_graph_async(ddq_ctx* ctx, const ddq_step_cfg* cfg, int32_t nsteps);
/* nsteps steps as graph replays with step t+1's replay sample + gather
 * overlapped with step t (double-buffered minibatch).  Same results, indices
 * and counters as nsteps sequential ddq_step_async calls.  Enqueued, no sync. */
int ddq_step_pipelined_async(ddq_ctx* ctx, const ddq_step_cfg* cfg, int32_t nsteps);
/* Capture + instantiate (and upload) the graphs of a step mode without
 * launching anything: mode 0 = eager (no-op), 1 = ddq_step_graph_async,
 * 2 = ddq_step_pipelined_async.  Lets multi-rank callers agree on a mode
 * (every rank prepared it) before any rank enters a collective. */
int ddq_step_prepare(ddq_ctx* ctx, const ddq_step_cfg* cfg, int32_t mode);
/* In-process data parallelism: W ctxs (W workers sharing a GPU, or peer-
 * enabled devices) exchange through device copies instead of RCCL, with the
 * same exchanges, shard layout and kernels as ddq_comm_init ranks.  The
 * group step is synchronous and runs phase by phase over the members. */
int ddq_group_init(ddq_ctx** ctxs, int32_t nranks);
int ddq_group_step(ddq_ctx** ctxs, int32_t nranks, const ddq_step_cfg* cfg);
/* Steps taken so far (drives the target-sync period). */
int64_t ddq_step_count(const ddq_ctx* ctx);

/* ---------------- asynchronous param server in arrival order ------------ */
/* (DDQ_EXCHANGE_ASYNC, server.py:196-209 applying pushes as they arrive.)
 * ddq_async_begin: the central model's shards start from this replica and the
 * worker computes its first gradient (implicit in the calls below).
 * ddq_async_ready: *ready = 1 once this worker's gradient is computed (it may
 * take the next ticket).  ddq_async_tick: enqueue tick `worker` -- every rank
 * calls it with the same worker sequence (the tickets, e.g. from a TCP store:
 * ddq/dist.py AsyncTicketLoop); enqueued, no sync (ddq_synchronize waits for
 * the owner duties too). */
int ddq_async_begin(ddq_ctx* ctx, const ddq_step_cfg* cfg);
int ddq_async_ready(ddq_ctx* ctx, int32_t* ready);
int ddq_async_tick(ddq_ctx* ctx, const ddq_step_cfg* cfg, int32_t worker);
/* In-process group in ticket order: npush ticks, each given to the first
 * member (after the previous ticket's holder) whose gradient is ready, polled
 * on the host; order[t] (nullable) receives tick t's worker.  Synchronous. */
int ddq_group_async_run(ddq_ctx** ctxs, int32_t nranks, const ddq_step_cfg* cfg, int32_t npush,
                        int32_t* order);
/* The same ticks in a given worker order (deterministic replay of a ticket
 * run, or any schedule).  Synchronous. */
int ddq_group_async_ticks(ddq_ctx** ctxs, int32_t nranks, const ddq_step_cfg* cfg, int32_t n,
                          const int32_t* order);
/* Straggler emulation (fault injection, cf. the dummy driver's injected
 * failures, baristanet.py:125-133): every gradient this worker computes
 * becomes pushable (ddq_async_ready, ticket runs) usec of host time after it
 * is computed -- a slow worker loop, without occupying the GPU.  0 disables. */
int ddq_set_straggle(ddq_ctx* ctx, int64_t usec);

/* ---------------- training monitor (barista/netutils.py NetLogger) ------- */
/* The quantities net.log() appends after every step (baristanet.py:148-149,
 * netutils.py:72-96): the loss, and the RMS of every blob's gradient and
 * parameters, np.linalg.norm(ravel(x)) / sqrt(x.size) (netutils.py:15-17),
 * taken on the device by one deterministic reduction launch and appended to a
 * device ring of fixed-size records; the host reads the ring whenever it likes.
 * A record is a snapshot of the ctx at the point in stream order where it is
 * taken: the current theta_Q and theta_P, the gradient buffer, the loss blob
 * and Q_out.  Squares are summed in double in a fixed order (no float atomics),
 * each RMS is rounded to fp32 once. */
typedef struct ddq_monitor_record {
  int64_t iteration;        /* device applied-updates counter when taken            */
  int64_t tag;              /* caller's tag (explicit record); -1 for a step's own  */
  float   loss;             /* the loss blob, as ddq_read_blob("loss") returns it   */
  float   q_max_mean;       /* mean over the B images of max_a Q_out[b][a]          */
  int32_t nonfinite[3];     /* count of non-finite values in theta_Q, theta_P, grads */
  int32_t reserved;         /* 0 */
  float   param_rms[2][10]; /* [Q,P][blob]: sqrt(sum x^2 / count), ddq_param_layout order */
  float   grad_rms[10];     /* the gradient buffer's blobs (what ddq_get_grads returns)   */
} ddq_monitor_record;       /* 160 bytes */

/* Allocate a device ring of `capacity` records and reset the record count;
 * capacity == 0 disables the monitor and frees the ring.  Invalidates graphs.
 * period == 0: explicit records only (ddq_monitor_record_async).  period > 0:
 * every single-ctx step (ddq_step_async, ddq_step_graph_async,
 * ddq_step_pipelined_async, ddq_profile_step: kernel "monitor") ends with the
 * monitor launch, which takes a record (tag -1) when the device iteration after
 * the step's update satisfies iteration % period == 0; the kernel makes that
 * test itself, so captured steps replay it.  Such a record holds the step's
 * loss_t and gradient g_t and the parameters AFTER update t (theta_P after the
 * step's P <- Q copy when one was due).  While period > 0 a step with
 * DDQ_STEP_NO_GRAD_STORE is refused (DDQ_EINVAL: its gradient block would be
 * stale) and so is ddq_async_begin (DDQ_ESTATE); ddq_group_step and the async
 * ticks take no records of their own.  With the monitor off (the default)
 * every step is launch for launch what it was. */
int ddq_monitor_enable(ddq_ctx* ctx, int64_t capacity, int32_t period);
/* One record now, with `tag`: enqueued on the ctx stream, no sync.  After a
 * worker's forward_backward it holds the reference's quantities exactly (the
 * fetched theta, this step's gradient and loss).  DDQ_ESTATE while disabled. */
int ddq_monitor_record_async(ddq_ctx* ctx, int64_t tag);
/* Synchronise; *total (nullable) = records taken since enable; copy records
 * [first, first+n), which must be among the last `capacity` taken (DDQ_EINVAL
 * otherwise).  out may be NULL with n == 0. */
int ddq_monitor_read(ddq_ctx* ctx, int64_t first, int64_t n, ddq_monitor_record* out,
                     int64_t* total);

/* ---------------- checkpoint and bit-exact resume ----------------------- */
/* The whole training state of a ctx as named byte sections, so that a ctx
 * restored from them continues exactly -- bit for bit, draw for draw -- as the
 * ctx that was read.  No reference counterpart (the reference persists the
 * ring's HDF5 file and the model snapshots only).
 *
 * Sections, in this fixed order; a section is listed only when what it holds
 * exists on the ctx:
 *   "config"       64                    ddq_state_config: a fingerprint, not state
 *   "theta_q"      4 P                   the flat Q tower, as ddq_get_params(0)
 *   "theta_p"      4 P                   the flat P tower
 *   "opt"          4 P                   the state word every rule uses (Adam: m); under
 *                                        a sharded exchange the rank's own buffer
 *   "opt2"         4 P                   Adam's v (once ddq_set_adam was called)
 *   "counters"     96                    ddq_state_counters
 *   "ring_state"   capacity 4 S S        the ring's arrays in slot order, as
 *   "ring_action"  capacity              ddq_replay_export writes them (once
 *   "ring_reward"  2 capacity            ddq_replay_create was called)
 *   "ring_nonterm" capacity
 *   "prio_leaf"    4 capacity            the leaves (while prioritization is on);
 *                                        the sums are derived and not stored
 *   "actor"        544                   the single actor's game (ddq_actor_create)
 *   "pool"         544 games             the pool's games (ddq_actors_create)
 * A game is: uint64 seed, draws; int64 steps, games ended, reward sum; int8
 * boards[5][100] (the 4-frame history, oldest first, then the start board); 4
 * zero bytes.  The zoom maps come from the create call.
 *
 * NOT state: the evaluator (ddq_eval_*: create it again), the monitor ring, the
 * index log, captured graphs, the small-map step's meeting counters,
 * communicators and groups, the gradient buffer and every blob, and the bound
 * minibatch: after ddq_state_commit none is bound (ddq_replay_update_priorities_async
 * returns DDQ_ESTATE until the next draw) and the step modes draw their own.
 *
 * Reading.  ddq_state_sections synchronises the ctx's streams, computes every
 * section's digest on the device and fills out[0..*n) (out == NULL: *n only;
 * cap < *n: DDQ_EINVAL).  ddq_state_read copies bytes [offset, offset + bytes)
 * of a section to the host: a ring of any size goes to disk through a small
 * staging buffer.  ddq_state_digest: one section's digest.
 *
 * Digest of a section of n bytes: w_k = the little-endian uint64 of bytes
 * 8k .. 8k+7, zero-padded past n; K = ceil(n / 8);
 *   digest = splitmix64(n) + sum_{k<K} splitmix64(w_k ^ ((k + 1) * 0x9E3779B97F4A7C15))
 * every operation mod 2^64, splitmix64 the hash of the index draws.  The sum
 * wraps, so it is the same in any order; it is not cryptographic: it catches
 * torn or corrupted files and lets two ctxs or ranks compare their state
 * without copying it.
 *
 * Restoring.  The caller first configures a ctx as the writer was configured,
 * with the existing calls (create, ring, lanes, n-step, priority, objective,
 * Adam, tau, actor or pool), then writes the sections and commits:
 *  - writing "config" compares it with the ctx and changes nothing; on a
 *    difference DDQ_EINVAL, the message names the first differing field;
 *  - writing any other section needs bytes > 0 and [offset, offset + bytes)
 *    inside the section (DDQ_EINVAL otherwise; nothing is written);
 *  - from the first such write on the ctx is "restoring": every call that
 *    launches work reading the state (the step modes, ddq_forward_backward,
 *    ddq_forward_q, ddq_select_action, the applies, the actor, pool and
 *    evaluator steps, the replay samplers and adds) returns DDQ_ESTATE
 *    ("restore not committed") until ddq_state_commit succeeds;
 *  - "counters" written while restoring is held on the host until the commit
 *    (ddq_state_read returns what was written).
 * ddq_state_commit validates the counters against the ring (head < lane_len,
 * valid <= lane_len, counts >= 0, reserved == 0, pmax in [65536, 2^24] while
 * prioritization is on) and the leaves (every leaf 0 or in [1, 2^24], and the
 * invariant q[i] == 0 <=> slot unfilled or forbidden under the restored head,
 * valid and n); on a failure DDQ_EINVAL and the ctx stays restoring.  Then it
 * pushes the counters to device memory and the host mirrors, rebuilds both
 * towers' derived conv-weight copies, the sum tree's levels and total from the
 * leaves (exact integers: order does not matter) and the actors' rendered
 * states, and drops every captured graph.  Without a preceding write it is a
 * no-op.
 * While the async exchange has begun every state call returns DDQ_ESTATE (the
 * central model lives in the owners' shards).  Members of a communicator or a
 * group are fine: each rank writes its own file. */
typedef struct ddq_state_section { char name[16]; int64_t bytes; uint64_t digest; } ddq_state_section; /* 32 B */

typedef struct ddq_state_config {   /* 64 bytes, no padding */
  int16_t  batch, frame;            /* ddq_net_desc                                  */
  uint32_t gamma_bits;              /* ddq_net_desc.gamma's bits                     */
  int64_t  capacity;                /* ring capacity; 0: no ring                     */
  int32_t  lanes;                   /* 1 without a ring                              */
  uint8_t  nstep;                   /* 1 without a ring                              */
  uint8_t  prio_enabled;            /* 0 / 1                                         */
  uint8_t  obj_target, obj_loss;    /* enum ddq_target, enum ddq_loss                */
  float    prio_alpha, prio_beta, prio_eps;   /* 0 while prioritization is off       */
  float    huber_delta;             /* 0 unless DDQ_LOSS_HUBER                       */
  uint8_t  adam_on;                 /* ddq_set_adam was called                       */
  uint8_t  actor;                   /* ddq_actor_create was called (0 / 1)           */
  int16_t  pool_games;              /* ddq_actors_create's games; 0: no pool         */
  float    adam_beta1, adam_beta2, adam_eps, adam_max_grad_norm;   /* 0 unless adam_on */
  float    target_tau;
} ddq_state_config;                 /* floats are compared by their bits             */

typedef struct ddq_state_counters { /* 96 bytes, no padding */
  int64_t  iteration;               /* the device iteration counter (Adam's t)       */
  int64_t  steps;                   /* ddq_step_count                                */
  int64_t  head, valid;             /* the ring's (per lane on a laned ring); 0 without */
  uint64_t draws;                   /* the ring's draw counter (ddq_replay_draws)    */
  uint64_t batch_ctr;               /* the large-batch sampler's counter             */
  int64_t  pool_h0, pool_v0;        /* the pool's ring head / valid at its create    */
  int64_t  pool_moves;              /* the pool's moves since                        */
  int32_t  opt_init;                /* 0 until the first apply after a reset, then 1 */
  int32_t  ring_err;                /* the ring's sticky error (ddq_replay_status)   */
  uint32_t pmax;                    /* prioritized replay's pmax; 0 while it is off  */
  int32_t  reserved[3];             /* 0 */
} ddq_state_counters;

int ddq_state_sections(ddq_ctx* ctx, ddq_state_section* out, int32_t cap, int32_t* n);
int ddq_state_read(ddq_ctx* ctx, const char* name, int64_t offset, void* dst, int64_t bytes);
int ddq_state_write(ddq_ctx* ctx, const char* name, int64_t offset, const void* src, int64_t bytes);
int ddq_state_commit(ddq_ctx* ctx);
int ddq_state_digest(ddq_ctx* ctx, const char* name, uint64_t* digest);

/* ---------------- measurement ------------------------------------------ */
/* Kernel ids for ddq_profile_step. */
#define DDQ_MAX_KERNELS 32
/* Run one eager step; every kernel is launched with start / stop events of
 * its own (hipExtLaunchKernel: the dispatch's timestamps, no marker packets
 * between the kernels); fills names (16 chars each, NUL padded) and each
 * kernel's device microseconds, in step order (RCCL calls are not timed). */
int ddq_profile_step(ddq_ctx* ctx, const ddq_step_cfg* cfg, char* names, float* usec,
                     int32_t cap, int32_t* n);
/* Launch one forward conv layer ("conv1_fwd", "conv2_fwd" or "conv3_fwd",
 * both towers, the step's own kernel and arguments) reps times back to back
 * between two HIP events on the ctx stream; *usec = average device time per
 * launch (no per-launch event overhead: the roofline's kernel time). */
int ddq_time_layer(ddq_ctx* ctx, const char* name, int32_t reps, float* usec);
/* Algorithmic FLOPs of one step (SURVEY.md 8(d) model, for the roofline). */
double ddq_step_flops(const ddq_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* DDQ_HIP_H */
