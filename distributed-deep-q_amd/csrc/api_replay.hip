// libddq_hip C-ABI: the replay ring, prioritized replay, batch sample and
// gather, the index log, reading and writing the minibatch.
#include <cmath>

#include "ctx.h"

using namespace ddq;
// (the ddq_* definitions take their C linkage from include/ddq_hip.h)

// ---------------- prioritized replay: tree set-up ----------------
static void prio_release(ddq_ctx* c) {
  PrioTree& t = c->nb.prio;
  dfree(c, t.leaf);
  for (auto& p : t.sum) dfree(c, p);
  dfree(c, t.st);
  t = PrioTree{};
  mb_bind_weights(c, false);
  c->replay.ring.prio = nullptr;
  c->prio.prio_on = false;
  c->prio.prio_cfg.enabled = 0;
}

// every filled, allowed slot <- pmax = 1.0, the rest 0, sums bottom-up
// (enable, import, fill_tiled, set_nstep, set_lanes); synchronises
static int prio_rebuild(ddq_ctx* c) {
  if (!c->prio.prio_on) return DDQ_OK;
  const uint32_t one = kPrioOne;
  HIP_TRY(c, hipMemcpyAsync(&c->nb.prio.st->pmax, &one, 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_prio_rebuild(c->nb.prio, c->replay.ring.meta, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->replay.idx_bound = false;
  return DDQ_OK;
}

// the enable path's device work: the scalars, the writers' copy of the tree,
// weights of 1 for a minibatch bound before any draw, the first rebuild
static int prio_enable_fill(ddq_ctx* c, const float abe[3]) {
  const PrioTree& t = c->nb.prio;
  HIP_TRY(c, hipMemcpyAsync(t.st, abe, 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->prio.d_prio, &t, sizeof(t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_fill_ones(c->nb.mb.isw, c->nb.B, c->stream));
  return prio_rebuild(c);
}

int ddq::prio_refuse(ddq_ctx* c, const char* what) {
  if (c && c->prio.prio_on)
    return fail(c, DDQ_ESTATE, "%s while prioritized replay is on: priorities are kept per ring, "
                               "not across ranks (ddq_replay_set_priority with enabled = 0 first)",
                what);
  return DDQ_OK;
}

// ---------------- replay ----------------
static int push_meta(ddq_ctx* c, bool prio_add = false, int64_t h = 0) {
  int64_t hv[2] = {c->replay.head, c->replay.valid};
  HIP_TRY(c, hipMemcpyAsync(c->replay.ring.meta, hv, sizeof(hv), hipMemcpyHostToDevice, c->stream));
  // prioritized replay: the writer rule on the slot just added, after the new
  // head / valid (stream order)
  if (prio_add) HIP_TRY(c, launch_prio_add(c->nb.prio, c->replay.ring.meta, 0, h, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_replay_create(ddq_ctx* c, int64_t capacity) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (capacity < 2 || capacity > (int64_t)INT32_MAX)
    return fail(c, DDQ_EINVAL, "capacity must be in [2, 2^31) (got %lld)", (long long)capacity);
  if (c->replay.ring.state) return fail(c, DDQ_ESTATE, "replay already created");
  TRY(set_dev(c));
  const size_t slot = (size_t)4 * c->nb.S * c->nb.S;
  TRY(dalloc(c, &c->replay.ring.state, slot * capacity));
  TRY(dalloc(c, &c->replay.ring.action, (size_t)capacity));
  TRY(dalloc(c, &c->replay.ring.reward, (size_t)capacity));
  TRY(dalloc(c, &c->replay.ring.nonterm, (size_t)capacity));
  c->replay.capacity = capacity;
  c->replay.head = c->replay.valid = 0;
  c->replay.lanes = 1;
  c->replay.lane_len = capacity;
  c->replay.nstep = 1;
  c->nb.nstep = 1;
  c->replay.aug_pad = 0;
  prio_release(c);
  ReplayMeta m{};
  m.capacity = capacity;
  m.lanes = 1;
  m.lane_len = capacity;
  m.nstep = 1;
  m.gamma = c->nb.gamma;
  HIP_TRY(c, scopy(c, c->replay.ring.meta, &m, sizeof(m), hipMemcpyHostToDevice));
  invalidate_graph(c);
  return DDQ_OK;
}

int ddq_replay_add(ddq_ctx* c, int32_t action, int32_t reward, const uint8_t* state) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->replay.lanes > 1) return fail(c, DDQ_ESTATE, "ddq_replay_add on a laned ring (%d lanes)", c->replay.lanes);
  if (action < 0 || action > 255) return fail(c, DDQ_EINVAL, "action must fit uint8");
  if (reward < -32768 || reward > 32767) return fail(c, DDQ_EINVAL, "reward must fit int16");
  TRY(guard(c));
  const size_t slot = (size_t)4 * c->nb.S * c->nb.S;
  const int64_t h = c->replay.head;
  uint8_t a = (uint8_t)action, nt = state ? 1 : 0;
  int16_t r = (int16_t)reward;
  HIP_TRY(c, hipMemcpyAsync(c->replay.ring.action + h, &a, 1, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->replay.ring.reward + h, &r, 2, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->replay.ring.nonterm + h, &nt, 1, hipMemcpyHostToDevice, c->stream));
  if (state)
    HIP_TRY(c, hipMemcpyAsync(c->replay.ring.state + h * slot, state, slot, hipMemcpyHostToDevice, c->stream));
  c->replay.head = (c->replay.head + 1) % c->replay.capacity;
  c->replay.valid = std::min(c->replay.capacity, c->replay.valid + 1);
  return push_meta(c, c->prio.prio_on, h);
}

int ddq_replay_info(const ddq_ctx* c, int64_t* head, int64_t* valid, int64_t* capacity) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (head) *head = c->replay.head;
  if (valid) *valid = c->replay.valid;
  if (capacity) *capacity = c->replay.capacity;
  return DDQ_OK;
}

// n-step returns (include/ddq_hip.h): forbidden start slots and the allowed
// count A per lane, on the host mirror of head / valid
static bool slot_forbidden(const ddq_ctx* c, int64_t x) {
  int64_t d = c->replay.head - 1 - x;
  if (d < 0 && c->replay.nstep >= 2 && c->replay.valid == c->replay.lane_len) d += c->replay.lane_len;
  return d >= 0 && d < c->replay.nstep;
}

static int64_t allowed_slots(const ddq_ctx* c) {
  if (c->replay.nstep < 2) return c->replay.valid - 1;
  if (c->replay.valid == c->replay.lane_len) return c->replay.lane_len - c->replay.nstep;
  const int64_t lo = std::max<int64_t>(0, c->replay.head - c->replay.nstep);
  const int64_t hi = std::min(c->replay.head - 1, c->replay.valid - 1);
  return c->replay.valid - std::max<int64_t>(0, hi - lo + 1);
}

// fewest filled, allowed slots a draw of B needs: B <= lanes * A, which is
// B <= lanes * (valid - 1) at n = 1 (B < valid on a plain ring)
bool ddq::too_few_slots(const ddq_ctx* c, int64_t batch) {
  return batch > c->replay.lanes * allowed_slots(c);
}

int ddq_replay_set_lanes(ddq_ctx* c, int32_t lanes) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->replay.valid != 0) return fail(c, DDQ_ESTATE, "set_lanes needs an empty ring (valid = %lld)",
                                 (long long)c->replay.valid);
  if (lanes < 1 || c->replay.capacity % lanes != 0 || c->replay.capacity / lanes < 2)
    return fail(c, DDQ_EINVAL, "lanes must divide capacity %lld into lanes of >= 2 slots (got %d)",
                (long long)c->replay.capacity, lanes);
  if (c->replay.capacity / lanes <= c->replay.nstep)
    return fail(c, DDQ_EINVAL, "%d lanes of %lld slots cannot hold the ring's %d-step windows",
                lanes, (long long)(c->replay.capacity / lanes), c->replay.nstep);
  if (lanes == c->replay.lanes) return DDQ_OK;
  TRY(set_dev(c));
  c->replay.lanes = lanes;
  c->replay.lane_len = c->replay.capacity / lanes;
  c->replay.head = 0;
  c->envs.p_env.n = 0;                    // a pool or an actor belongs to the lanes it was
  c->envs.a_env.n = 0;                    // created on
  char* m = reinterpret_cast<char*>(c->replay.ring.meta);
  HIP_TRY(c, scopy(c, m + offsetof(ReplayMeta, lanes), &c->replay.lanes, 4, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, m + offsetof(ReplayMeta, lane_len), &c->replay.lane_len, 8, hipMemcpyHostToDevice));
  TRY(push_meta(c));
  return prio_rebuild(c);
}

int ddq_replay_lanes(const ddq_ctx* c, int32_t* lanes, int64_t* lane_len) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->replay.ring.state) return fail(const_cast<ddq_ctx*>(c), DDQ_ESTATE, "no replay buffer");
  if (lanes) *lanes = c->replay.lanes;
  if (lane_len) *lane_len = c->replay.lane_len;
  return DDQ_OK;
}

static_assert(kNstepMax == DDQ_NSTEP_MAX, "the window loops unroll to DDQ_NSTEP_MAX");

int ddq_replay_set_nstep(ddq_ctx* c, int32_t n) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->async.async_on)
    return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx: set the n-step "
                               "length before ddq_async_begin");
  if (n < 1 || n > DDQ_NSTEP_MAX || n >= c->replay.lane_len)
    return fail(c, DDQ_EINVAL, "n-step length must be in [1, %d] and below lane_len %lld (got %d)",
                DDQ_NSTEP_MAX, (long long)c->replay.lane_len, n);
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);   // a pipelined chain holds a minibatch gathered under the old n
  c->replay.nstep = n;
  c->nb.nstep = n;   // n >= 2: the n-step instantiations of the drawing / gathering kernels
  HIP_TRY(c, scopy(c, reinterpret_cast<char*>(c->replay.ring.meta) + offsetof(ReplayMeta, nstep), &c->replay.nstep,
                   4, hipMemcpyHostToDevice));
  return prio_rebuild(c);
}

int ddq_replay_nstep(const ddq_ctx* c, int32_t* n) {
  if (!c || !n) return fail(nullptr, DDQ_EINVAL, "null argument");
  if (!c->replay.ring.state) return fail(const_cast<ddq_ctx*>(c), DDQ_ESTATE, "no replay buffer");
  *n = c->replay.nstep;
  return DDQ_OK;
}

static_assert(kAugPadMax == DDQ_AUGMENT_PAD_MAX, "a run's window covers pad <= DDQ_AUGMENT_PAD_MAX");

int ddq_replay_set_augment(ddq_ctx* c, int32_t pad) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->async.async_on)
    return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx: it takes no "
                               "augmentation");
  if (pad < 0 || pad > DDQ_AUGMENT_PAD_MAX || 4 * pad > c->nb.S)
    return fail(c, DDQ_EINVAL, "augmentation pad must be in [0, %d] and at most frame / 4 = %d "
                               "(got %d)", DDQ_AUGMENT_PAD_MAX, c->nb.S / 4, pad);
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);   // captured steps hold the fused gather blocks, or the shifting launch
  c->replay.aug_pad = pad;
  return DDQ_OK;
}

int ddq_replay_get_augment(const ddq_ctx* c, int32_t* pad) {
  if (!c || !pad) return fail(nullptr, DDQ_EINVAL, "null argument");
  if (!c->replay.ring.state) return fail(const_cast<ddq_ctx*>(c), DDQ_ESTATE, "no replay buffer");
  *pad = c->replay.aug_pad;
  return DDQ_OK;
}

// ---------------- prioritized replay: entry points ----------------
static bool unit_interval(float x) { return std::isfinite(x) && x >= 0.f && x <= 1.f; }

int ddq_replay_set_priority(ddq_ctx* c, const ddq_priority_cfg* p) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!p) return fail(c, DDQ_EINVAL, "null priority cfg");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  TRY(set_dev(c));
  if (!p->enabled) {
    if (!c->prio.prio_on) return DDQ_OK;
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
  if (c->async.async_on) return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx");
  if (c->comm.comm || c->comm.local)
    return fail(c, DDQ_ESTATE, "prioritized replay on a ctx with a communicator or in a group: "
                               "priorities are kept per ring, not across ranks");
  const float abe[3] = {p->alpha, p->beta, p->eps};
  if (c->prio.prio_on) {
    // the annealing path: three scalars in device memory, stream-ordered; captured
    // graphs read them live.  No synchronisation, no rebuild, no graph drop.
    HIP_TRY(c, hipMemcpyAsync(c->nb.prio.st, abe, sizeof(abe), hipMemcpyHostToDevice, c->stream));
    c->prio.prio_cfg = ddq_priority_cfg{1, p->alpha, p->beta, p->eps};
    return DDQ_OK;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);
  PrioTree t{};
  t.capacity = c->replay.capacity;
  t.padded[0] = (c->replay.capacity + 63) / 64 * 64;
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
  if (rc == DDQ_OK && !c->prio.d_prio) rc = dalloc(c, &c->prio.d_prio, 1);
  c->nb.prio = t;
  mb_bind_weights(c, true);
  c->replay.ring.prio = c->prio.d_prio;
  c->prio.prio_on = true;
  if (rc == DDQ_OK) rc = prio_enable_fill(c, abe);
  if (rc != DDQ_OK) { prio_release(c); return rc; }   // all or nothing: no half-bound tree
  c->prio.prio_cfg = ddq_priority_cfg{1, p->alpha, p->beta, p->eps};
  return DDQ_OK;
}

int ddq_replay_get_priority(const ddq_ctx* c, ddq_priority_cfg* p) {
  if (!c || !p) return fail(nullptr, DDQ_EINVAL, "null argument");
  *p = c->prio.prio_cfg;
  return DDQ_OK;
}

int ddq_replay_priorities(ddq_ctx* c, uint32_t* leaves, int64_t n, uint64_t* total, uint32_t* pmax) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->prio.prio_on) return fail(c, DDQ_ESTATE, "prioritized replay is off");
  if (leaves && n != c->replay.capacity)
    return fail(c, DDQ_EINVAL, "the ring has %lld leaves (got n = %lld)", (long long)c->replay.capacity,
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
  if (!c->prio.prio_on) return fail(c, DDQ_ESTATE, "prioritized replay is off");
  if (n < 0 || (n > 0 && (!idx || !q))) return fail(c, DDQ_EINVAL, "bad argument");
  if (n == 0) return DDQ_OK;
  TRY(set_dev(c));
  std::vector<uint32_t> leaf((size_t)c->replay.capacity);
  HIP_TRY(c, scopy(c, leaf.data(), c->nb.prio.leaf, leaf.size() * 4, hipMemcpyDeviceToHost));
  for (int k = 0; k < n; ++k) {
    if (idx[k] < 0 || idx[k] >= c->replay.capacity) return fail(c, DDQ_EINVAL, "index %d out of range", idx[k]);
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
  if (m > c->prio.pset_cap) {
    dfree(c, c->prio.pset_idx);
    dfree(c, c->prio.pset_q);
    c->prio.pset_cap = 0;
    TRY(dalloc(c, &c->prio.pset_idx, (size_t)m));
    TRY(dalloc(c, &c->prio.pset_q, (size_t)m));
    c->prio.pset_cap = m;
  }
  HIP_TRY(c, hipMemcpyAsync(c->prio.pset_idx, hi.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->prio.pset_q, hq.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_prio_set(c->nb.prio, c->prio.pset_idx, c->prio.pset_q, m, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

int ddq_replay_update_priorities_async(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->prio.prio_on) return fail(c, DDQ_ESTATE, "prioritized replay is off");
  if (!c->replay.idx_bound)
    return fail(c, DDQ_ESTATE, "no device-side index set is bound (the minibatch was not drawn from "
                               "the ring)");
  TRY(set_dev(c));
  HIP_TRY(c, launch_prio_commit(c->nb, c->replay.ring.meta, c->stream));
  return DDQ_OK;
}

int ddq_replay_import(ddq_ctx* c, const uint8_t* state, const uint8_t* action,
                      const int16_t* reward, const uint8_t* nonterm, int64_t n, int64_t head,
                      int64_t valid) {
  if (!c || !state || !action || !reward || !nonterm) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (n != c->replay.capacity) return fail(c, DDQ_EINVAL, "import size %lld != capacity %lld",
                                    (long long)n, (long long)c->replay.capacity);
  if (head < 0 || head >= c->replay.lane_len || valid < 0 || valid > c->replay.lane_len)
    return fail(c, DDQ_EINVAL, "head/valid out of range");
  TRY(set_dev(c));
  const size_t slot = (size_t)4 * c->nb.S * c->nb.S;
  HIP_TRY(c, scopy(c, c->replay.ring.state, state, slot * n, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, c->replay.ring.action, action, n, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, c->replay.ring.reward, reward, 2 * n, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, c->replay.ring.nonterm, nonterm, n, hipMemcpyHostToDevice));
  c->replay.head = head;
  c->replay.valid = valid;
  TRY(push_meta(c));
  return prio_rebuild(c);
}

int ddq_replay_export(ddq_ctx* c, uint8_t* state, uint8_t* action, int16_t* reward,
                      uint8_t* nonterm, int64_t n) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (n != c->replay.capacity) return fail(c, DDQ_EINVAL, "export size mismatch");
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t slot = (size_t)4 * c->nb.S * c->nb.S;
  if (state) HIP_TRY(c, scopy(c, state, c->replay.ring.state, slot * n, hipMemcpyDeviceToHost));
  if (action) HIP_TRY(c, scopy(c, action, c->replay.ring.action, n, hipMemcpyDeviceToHost));
  if (reward) HIP_TRY(c, scopy(c, reward, c->replay.ring.reward, 2 * n, hipMemcpyDeviceToHost));
  if (nonterm) HIP_TRY(c, scopy(c, nonterm, c->replay.ring.nonterm, n, hipMemcpyDeviceToHost));
  return DDQ_OK;
}

static int check_err_flag(ddq_ctx* c) {
  ReplayMeta m;
  HIP_TRY(c, hipMemcpyAsync(&m, c->replay.ring.meta, sizeof(m), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (m.err) {
    int32_t z = 0;
    HIP_TRY(c, scopy(c, reinterpret_cast<char*>(c->replay.ring.meta) + offsetof(ReplayMeta, err), &z, 4,
                         hipMemcpyHostToDevice));
    if (m.err == 2) return fail(c, DDQ_ERANGE, "batch sampler could not find distinct indices");
    return fail(c, DDQ_ERANGE, "stored action index out of range for %d actions", 4);
  }
  return DDQ_OK;
}

int ddq_replay_sample(ddq_ctx* c, const int32_t* idx, int32_t batch) {
  if (!c || !idx) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (too_few_slots(c, batch))
    return fail(c, DDQ_EINVAL, "Can't draw sample of size %d from replay dataset of size %lld",
                batch, (long long)(c->replay.lanes * c->replay.valid));
  if (batch != c->nb.B)
    return fail(c, DDQ_EINVAL, "sample size %d != net batch %d", batch, c->nb.B);
  for (int i = 0; i < batch; ++i) {
    if (idx[i] < 0 || idx[i] >= c->replay.capacity || idx[i] % c->replay.lane_len >= c->replay.valid)
      return fail(c, DDQ_EINVAL, "index %d out of [0,valid)", idx[i]);
    if (c->replay.nstep >= 2 && slot_forbidden(c, idx[i] % c->replay.lane_len))
      return fail(c, DDQ_EINVAL, "index %d: its %d-step window reaches the write head", idx[i],
                  c->replay.nstep);
    if (i && idx[i] <= idx[i - 1]) return fail(c, DDQ_EINVAL, "indices must be sorted and distinct");
  }
  TRY(guard(c));
  HIP_TRY(c, hipMemcpyAsync(c->nb.mb.idx, idx, batch * 4, hipMemcpyHostToDevice, c->stream));
  if (c->nb.mb.isw) HIP_TRY(c, launch_fill_ones(c->nb.mb.isw, batch, c->stream));   // host-given set
  HIP_TRY(c, launch_gather(c->nb, c->replay.ring, c->stream));
  c->replay.idx_bound = true;
  return check_err_flag(c);
}

int ddq_replay_sample_device_async(ddq_ctx* c, uint64_t seed) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (too_few_slots(c, c->nb.B))
    return fail(c, DDQ_EINVAL, "Can't draw sample of size %d from replay dataset of size %lld",
                c->nb.B, (long long)(c->replay.lanes * c->replay.valid));
  TRY(guard(c));
  if (c->prio.prio_on) {   // the prioritized draw (one workgroup), then its counter's advance
    HIP_TRY(c, launch_prio_sample(c->nb, c->replay.ring.meta, seed, c->stream, true));
  } else {
    HIP_TRY(c, launch_sample(c->nb, c->replay.ring.meta, seed, c->stream));
  }
  if (c->replay.aug_pad > 0)   // (both draws above moved the counter on: back = 1)
    HIP_TRY(c, launch_gather_shift(c->nb, c->replay.ring, seed, c->replay.aug_pad, 1, c->stream));
  else
    HIP_TRY(c, launch_gather(c->nb, c->replay.ring, c->stream));
  c->replay.idx_bound = true;
  return DDQ_OK;
}

int ddq_replay_fill_tiled(ddq_ctx* c, const uint8_t* state, const uint8_t* action,
                          const int16_t* reward, const uint8_t* nonterm, int64_t pool,
                          int64_t head, int64_t valid) {
  if (!c || !state || !action || !reward || !nonterm) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (c->replay.lanes > 1)
    return fail(c, DDQ_ESTATE, "ddq_replay_fill_tiled on a laned ring (%d lanes)", c->replay.lanes);
  const int64_t n = c->replay.capacity;
  if (pool < 1 || pool > n) return fail(c, DDQ_EINVAL, "pool must be in [1, capacity]");
  if (head < 0 || head >= n || valid < 0 || valid > n)
    return fail(c, DDQ_EINVAL, "head/valid out of range");
  TRY(set_dev(c));
  const size_t slot = (size_t)4 * c->nb.S * c->nb.S;
  HIP_TRY(c, scopy(c, c->replay.ring.state, state, slot * pool, hipMemcpyHostToDevice));
  if (pool < n)
    HIP_TRY(c, launch_tile(c->replay.ring.state + slot * pool, c->replay.ring.state, slot * pool,
                           slot * (n - pool), c->stream));
  std::vector<uint8_t> a(n), t(n);
  std::vector<int16_t> r(n);
  for (int64_t i = 0; i < n; ++i) {
    a[i] = action[i % pool]; r[i] = reward[i % pool]; t[i] = nonterm[i % pool];
  }
  HIP_TRY(c, scopy(c, c->replay.ring.action, a.data(), n, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, c->replay.ring.reward, r.data(), 2 * n, hipMemcpyHostToDevice));
  HIP_TRY(c, scopy(c, c->replay.ring.nonterm, t.data(), n, hipMemcpyHostToDevice));
  c->replay.head = head;
  c->replay.valid = valid;
  TRY(push_meta(c));
  return prio_rebuild(c);
}

static int check_batch_out(ddq_ctx* c, int32_t n, const Minibatch& out) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!out.state || !out.action || !out.reward || !out.next_state || !out.nonterm)
    return fail(c, DDQ_EINVAL, "null output buffer");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (c->replay.lanes > 1)
    return fail(c, DDQ_ESTATE, "the large-batch sampler does not read a laned ring (%d lanes)",
                c->replay.lanes);
  if (n < 1) return fail(c, DDQ_EINVAL, "n must be >= 1");
  if ((int64_t)n * c->nb.S * c->nb.S >= (int64_t)1 << 31)
    return fail(c, DDQ_EINVAL, "n * S^2 must be < 2^31 (n=%d)", n);
  if (too_few_slots(c, n))   // n > A; n >= valid at nstep == 1
    return fail(c, DDQ_EINVAL, "Can't draw sample of size %d from replay dataset of size %lld",
                n, (long long)c->replay.valid);
  return DDQ_OK;
}

int ddq_replay_sample_batch_async(ddq_ctx* c, int32_t n, uint64_t seed, int32_t* idx,
                                  float* state, float* action, float* reward, float* next_state,
                                  float* nonterm) {
  const Minibatch out{state, next_state, action, reward, nonterm};
  TRY(check_batch_out(c, n, out));
  if (!idx) return fail(c, DDQ_EINVAL, "null idx");
  if (2 * (int64_t)n > c->replay.valid)
    return fail(c, DDQ_EINVAL, "batch sampler needs n <= valid/2 (n=%d, valid=%lld)", n,
                (long long)c->replay.valid);
  TRY(guard(c));
  if (!c->replay.r_bitmap) {   // sized for the full ring: valid never exceeds capacity
    const int64_t nblk = ((c->replay.capacity + 31) / 32 + 1023) / 1024;
    TRY(dalloc(c, &c->replay.r_bitmap, (size_t)nblk * 1024));
    TRY(dalloc(c, &c->replay.r_blk, (size_t)nblk));
  }
  HIP_TRY(c, launch_sample_batch(c->replay.ring.meta, c->replay.valid, n, seed, c->replay.batch_ctr++, c->replay.r_bitmap,
                                 c->replay.r_blk, idx, c->stream, c->replay.nstep));
  HIP_TRY(c, launch_gather_nchw(c->replay.ring, idx, n, c->nb.S, out, c->stream, c->replay.nstep));
  return DDQ_OK;
}

int ddq_replay_gather_batch_async(ddq_ctx* c, const int32_t* idx, int32_t n, float* state,
                                  float* action, float* reward, float* next_state,
                                  float* nonterm) {
  const Minibatch out{state, next_state, action, reward, nonterm};
  TRY(check_batch_out(c, n, out));
  if (!idx) return fail(c, DDQ_EINVAL, "null idx");
  TRY(guard(c));
  HIP_TRY(c, launch_gather_nchw(c->replay.ring, idx, n, c->nb.S, out, c->stream, c->replay.nstep));
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
  HIP_TRY(c, scopy(c, &m, c->replay.ring.meta, sizeof(m), hipMemcpyDeviceToHost));
  c->replay.log_first = (int64_t)m.counter;
  if (draws == 0) {
    c->nb.idx_log = nullptr;
    c->nb.log_cap = 0;
  } else if (draws > c->replay.log_buf_cap) {
    TRY(dalloc(c, &c->replay.log_buf, (size_t)draws * c->nb.B));
    c->replay.log_buf_cap = draws;
    c->nb.idx_log = c->replay.log_buf;
    c->nb.log_cap = draws;
  } else {
    c->nb.idx_log = c->replay.log_buf;
    c->nb.log_cap = draws;
  }
  invalidate_graph(c);   // captured kernels hold the log pointer
  return DDQ_OK;
}

int ddq_replay_draws(ddq_ctx* c, int64_t* draws) {
  if (!c || !draws) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
  TRY(set_dev(c));
  ReplayMeta m;
  HIP_TRY(c, hipMemcpyAsync(&m, c->replay.ring.meta, sizeof(m), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *draws = (int64_t)m.counter;
  return DDQ_OK;
}

int ddq_index_log_read(ddq_ctx* c, int64_t first, int64_t n, int32_t* out) {
  if (!c || !out) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->nb.idx_log) return fail(c, DDQ_ESTATE, "index log not enabled");
  int64_t drawn = 0;
  TRY(ddq_replay_draws(c, &drawn));
  if (first < c->replay.log_first || n < 0 || first + n > drawn || drawn - first > c->nb.log_cap)
    return fail(c, DDQ_EINVAL,
                "draws [%lld, %lld) not in the log (logged from draw %lld, drawn %lld, cap %lld)",
                (long long)first, (long long)(first + n), (long long)c->replay.log_first,
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
  if (!c->replay.ring.state) return fail(c, DDQ_ESTATE, "no replay buffer");
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

// index of the first of n floats that bf16 does not hold exactly (low 16 bits
// of the fp32 pattern set, or not finite), -1 if none
static int64_t first_not_bf16(const float* v, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    uint32_t u;
    memcpy(&u, v + i, 4);
    if ((u & 0xFFFFu) || (u & 0x7F800000u) == 0x7F800000u) return i;
  }
  return -1;
}

int ddq_write_minibatch(ddq_ctx* c, const float* state, const float* action, const float* reward,
                        const float* next_state, const float* nonterm) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(set_dev(c));
  const int B = c->nb.B, SS = c->nb.S * c->nb.S;
  // conv1 reads a frame as ONE bf16 plane (split.h), so a value with more than
  // 8 significant bits would lose them without a word: refuse it here, before
  // anything of the bound minibatch is touched
  for (int which = 0; which < 2; ++which) {
    const float* src = which ? next_state : state;
    if (!src) continue;
    const int64_t bad = first_not_bf16(src, (int64_t)B * 4 * SS);
    if (bad >= 0)
      return fail(c, DDQ_EINVAL, "%s[%lld] = %.9g is not exactly representable in bf16",
                  which ? "next_state" : "state", (long long)bad, (double)src[bad]);
  }
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
  c->replay.idx_bound = false;
  return DDQ_OK;
}
