// libddq_hip C-ABI (include/ddq_hip.h), core unit: the context and its device
// memory, parameters, the compute and acting calls, apply and Adam,
// measurement.  The other subsystems: api_replay.hip, api_env.hip,
// api_step.hip, api_exchange.hip, api_monitor.hip, api_state.hip.
#include <cmath>
#include <cstdarg>

#include "step.h"

namespace ddq {
int fc4_splits_for(int S);
int wgrad_splits_for(int layer, int B, int S, int* np);
}  // namespace ddq

using namespace ddq;
// (the ddq_* definitions take their C linkage from include/ddq_hip.h)

static thread_local std::string g_last_error;

int ddq::fail(ddq_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  g_last_error = buf;
  return code;
}

// One minibatch set's buffers, all or none.  The reward buffer holds 2 * B
// floats: the B rewards, then the B importance-sampling weights of prioritized
// replay (mb_bind_weights).
int ddq::mb_alloc(ddq_ctx* c, Minibatch* out) {
  const size_t B = c->nb.B, frames = B * c->nb.S * c->nb.S * 4;
  Minibatch m{};
  TRY(dalloc(c, &m.state, frames));
  TRY(dalloc(c, &m.next_state, frames));
  TRY(dalloc(c, &m.action, B * 4));
  TRY(dalloc(c, &m.reward, 2 * B));
  TRY(dalloc(c, &m.nonterm, B));
  TRY(dalloc(c, &m.idx, B));
  TRY(dalloc(c, &m.shift, B * 4));
  *out = m;
  return DDQ_OK;
}

// The weights of every allocated set: the second half of its reward buffer
// while prioritization is on, none otherwise.  nb.mb follows set 0.
void ddq::mb_bind_weights(ddq_ctx* c, bool on) {
  for (Minibatch& m : c->mb) m.isw = on && m.reward ? m.reward + c->nb.B : nullptr;
  c->nb.mb = c->mb[0];
}

// Blocking copy ordered on the ctx stream.
hipError_t ddq::scopy(ddq_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(c->stream);
}

int ddq::set_dev(ddq_ctx* c) {
  HIP_TRY(c, hipSetDevice(c->device));
  return DDQ_OK;
}

// The guard of every call that launches work reading the training state:
// between the first ddq_state_write and ddq_state_commit the state is partly
// the checkpoint's and its derived copies are stale.
int ddq::not_restoring(ddq_ctx* c) {
  if (c->state.restoring)
    return fail(c, DDQ_ESTATE, "restore not committed: sections were written with ddq_state_write, "
                               "call ddq_state_commit first");
  return DDQ_OK;
}
int ddq::guard(ddq_ctx* c) {
  TRY(not_restoring(c));
  return set_dev(c);
}

void ddq::invalidate_graph(ddq_ctx* c) { c->graphs.reset(); }

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
    TRY(dalloc(c, &c->act.act_u8, (size_t)B * 4 * S * S));
    TRY(dalloc(c, &c->act.act_in, (size_t)B * S * S * 4));
    TRY(dalloc(c, &c->act.act_p1s, (size_t)3 * B * S2 * S2 * 32));
    TRY(dalloc(c, &c->act.act_p2s, (size_t)3 * B * S3 * S3 * 64));
    TRY(dalloc(c, &c->act.act_p3, (size_t)B * S4 * S4 * 64));
    TRY(dalloc(c, &c->act.act_h4, (size_t)B * 512));
    TRY(dalloc(c, &c->act.act_part, (size_t)nb.fc4_splits * 2 * B * 512));
    TRY(dalloc(c, &c->act.act_q, (size_t)B * 4));
    TRY(dalloc(c, &c->act.act_out, (size_t)B));
    TRY(dalloc(c, &c->replay.ring.meta, 1));
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
  if (c->comm.cs) hipStreamSynchronize(c->comm.cs);
  if (c->stream) hipStreamSynchronize(c->stream);
  invalidate_graph(c);   // (every graph exec: the step, pipelined, async ones)
  for (auto& e : c->marks.ev_pool) hipEventDestroy(e);
  if (c->comm.comm) ncclCommDestroy(c->comm.comm);
  for (void* p : c->allocs) hipFree(p);
  if (c->stream && c->own_stream) hipStreamDestroy(c->stream);
  for (auto& e : c->nb.ev)
    if (e) hipEventDestroy(e);
  if (c->nb.side) hipStreamDestroy(c->nb.side);
  if (c->comm.cs) hipStreamDestroy(c->comm.cs);
  if (c->async.grad_ev) hipEventDestroy(c->async.grad_ev);
  if (c->async.tick_ev) hipEventDestroy(c->async.tick_ev);
  for (auto& e : c->comm.cev)
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
  if (c->comm.cs) HIP_TRY(c, hipStreamSynchronize(c->comm.cs));   // owner duties of async ticks
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->pn.on)                       // the adapted sigma's host mirror (ddq_get_param_noise)
    HIP_TRY(c, hipMemcpy(&c->pn.cfg.sigma, c->pn.d_sigma, sizeof(float), hipMemcpyDeviceToHost));
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
  if (c->async.async_on && tau < 1.f)
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
  HIP_TRY(c, launch_act(nb, nb.mb.next_state, nb.B, c->act.act_p3, c->act.act_h4, c->act.act_part, nb.qn_out,
                        nullptr, c->act.act_p1s, c->act.act_p2s, c->stream, qn, c->act.act_path));
  return DDQ_OK;
}

// Munchausen target (ddq_set_munchausen) with alpha != 0: P(s,.) under theta_P for
// the minibatch view the pass trains on, the pass's first launch group -- the
// acting forward's kernels at n = B over nb.mb.state with the P tower's
// parameters and split copies (launch_act's tower argument), in the acting
// scratch, into the ctx's Pc_out buffer.  It depends on theta_P and the bound
// view only: stream order after the previous step's apply -- which is also what
// writes P on a sync or Polyak step -- is enough.  Profile names: "pc_<kernel>".
static void pc_mark(void* a, const char* name) {
  const std::string s = std::string("pc_") + name;
  (*reinterpret_cast<const Marks*>(a))(s.c_str());
}
static hipError_t launch_pc_forward(ddq_ctx* c, const NetBuffers& nb, Marks m) {
  return launch_act(nb, nb.mb.state, nb.B, c->act.act_p3, c->act.act_h4, c->act.act_part, nb.pc_out,
                    nullptr, c->act.act_p1s, c->act.act_p2s, c->stream, m, c->act.act_path, 1);
}
static int enqueue_pc_forward(ddq_ctx* c, const NetBuffers& nb, Marks m) {
  if (!nb.m_on || nb.m_alpha == 0.f) return DDQ_OK;
  const Marks pc = m.fn ? Marks{pc_mark, &m} : Marks{};
  HIP_TRY(c, launch_pc_forward(c, nb, pc));
  return DDQ_OK;
}

// The gradient launches of a step as sl.plan has them; fc4_done: the
// overlapped all-reduce's start, its argument the ctx (launch_backward).
// (one stream: forking the weight-gradient kernels onto a side stream cost
// more in cross-stream graph edges (6-14 us idle each, measured) than the
// overlap returned, as every kernel here fills the GPU on its own)
int ddq::enqueue_fwd_bwd(ddq_ctx* c, const NetBuffers& nb, const StepLaunch& sl, Marks m,
                         Fc4Done fc4_done, const NetBuffers* prio_next, uint64_t prio_seed) {
  TRY(enqueue_qn_forward(c, nb, m));
  TRY(enqueue_pc_forward(c, nb, m));
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
    // augmented: the shifting gather of the set the commit launch just drew (under the
    // counter it advanced: back = 0)
    if (sl.plan.gather == Site::PrioCommit) {
      m("gather_shift");
      HIP_TRY(c, launch_gather_shift(*prio_next, c->replay.ring, prio_seed, c->replay.aug_pad, 0, c->stream));
    }
  }
  hipError_t e = nb.small ? launch_small_bwd(nb, sl, c->stream, m, fc4_done)
                          : launch_backward(nb, sl, c->stream, m, fc4_done);
  if (e != hipSuccess && !c->comm.comm_err.empty()) {
    std::string m = c->comm.comm_err;
    c->comm.comm_err.clear();
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
  if (o->target == DDQ_TARGET_DOUBLE && c->nb.m_on)
    return fail(c, DDQ_EINVAL, "the double target with the Munchausen target on: turn that off "
                               "first (ddq_set_munchausen)");
  if (c->async.async_on)
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
    HIP_TRY(c, launch_act(nb, nb.mb.next_state, nb.B, c->act.act_p3, c->act.act_h4, c->act.act_part, nb.qn_out,
                          nullptr, c->act.act_p1s, c->act.act_p2s, c->stream, {}, c->act.act_path));
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

// ---------------- Munchausen / soft-Q target ----------------
int ddq_set_munchausen(ddq_ctx* c, const ddq_munchausen_cfg* m) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!m) return fail(c, DDQ_EINVAL, "null munchausen cfg");
  if (m->enabled != 0 && m->enabled != 1)
    return fail(c, DDQ_EINVAL, "enabled must be 0 or 1 (got %d)", (int)m->enabled);
  if (m->enabled) {
    if (!(m->alpha >= 0.f && m->alpha <= 1.f))
      return fail(c, DDQ_EINVAL, "alpha must be in [0, 1] (got %g)", (double)m->alpha);
    if (!(std::isfinite(m->tau) && m->tau > 0.f))
      return fail(c, DDQ_EINVAL, "tau must be finite and > 0 (got %g)", (double)m->tau);
    if (!(std::isfinite(m->clip_lo) && m->clip_lo < 0.f))
      return fail(c, DDQ_EINVAL, "clip_lo must be finite and < 0 (got %g)", (double)m->clip_lo);
    if (c->nb.obj_target == DDQ_TARGET_DOUBLE)
      return fail(c, DDQ_EINVAL, "the Munchausen target with the double target: set "
                                 "DDQ_TARGET_MAX first (ddq_set_objective)");
  }
  if (c->async.async_on)
    return fail(c, DDQ_ESTATE, "the async exchange is in progress on this ctx: set the Munchausen "
                               "target before ddq_async_begin");
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);   // captured steps hold (or lack) the extra forward and the head's constants
  NetBuffers& nb = c->nb;
  if (!m->enabled) {
    nb.m_on = 0;
    nb.m_alpha = nb.m_tau = nb.m_clip = 0.f;
    return DDQ_OK;
  }
  if (!nb.pc_out) TRY(dalloc(c, &nb.pc_out, (size_t)nb.B * 4));
  if (!nb.m_bonus) TRY(dalloc(c, &nb.m_bonus, (size_t)nb.B));
  if (m->alpha != 0.f) {
    // one run of the extra forward now: its kernels' function attributes are set
    // outside any capture (the result is overwritten by the first pass)
    HIP_TRY(c, launch_pc_forward(c, nb, {}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  nb.m_on = 1;
  nb.m_alpha = m->alpha; nb.m_tau = m->tau; nb.m_clip = m->clip_lo;
  return DDQ_OK;
}

int ddq_get_munchausen(const ddq_ctx* c, ddq_munchausen_cfg* m) {
  if (!c || !m) return fail(nullptr, DDQ_EINVAL, "null argument");
  *m = ddq_munchausen_cfg{c->nb.m_on, c->nb.m_alpha, c->nb.m_tau, c->nb.m_clip};
  return DDQ_OK;
}

// ---------------- acting path ----------------
int ddq_set_acting_path(ddq_ctx* c, int32_t path) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (path != DDQ_ACT_BATCH && path != DDQ_ACT_SPREAD && path != DDQ_ACT_AUTO)
    return fail(c, DDQ_EINVAL, "unknown acting path %d", (int)path);
  TRY(set_dev(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  invalidate_graph(c);   // captured steps hold the Qn_out / Pc_out forward's launches
  NetBuffers& nb = c->nb;
  c->act.act_path = path;
  if (path != DDQ_ACT_BATCH && !nb.small) {
    // one run at n = 1 and at n = B into the acting scratch: the kernels'
    // function attributes are set outside any capture
    for (int n : {1, nb.B})
      HIP_TRY(c, launch_act(nb, c->act.act_in, n, c->act.act_p3, c->act.act_h4, c->act.act_part, c->act.act_q, nullptr,
                            c->act.act_p1s, c->act.act_p2s, c->stream, {}, c->act.act_path));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return DDQ_OK;
}

int ddq_get_acting_path(const ddq_ctx* c, int32_t* path) {
  if (!c || !path) return fail(nullptr, DDQ_EINVAL, "null argument");
  *path = c->act.act_path;
  return DDQ_OK;
}

int ddq_forward_q(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  TRY(guard(c));
  HIP_TRY(c, launch_act(c->nb, c->nb.mb.state, c->nb.B, c->act.act_p3, c->act.act_h4, c->act.act_part,
                        c->nb.q_out, nullptr, c->act.act_p1s, c->act.act_p2s, c->stream, {}, c->act.act_path));
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
      {"is_weight", c->nb.mb.isw, B},       {"grad_norm", c->nb.gnorm, 1},
      {"aug_shift", c->nb.mb.shift, 4ll * B}, {"Pc_out", c->nb.pc_out, 4ll * B},
      {"m_bonus", c->nb.m_bonus, B},       {"Qa_out", c->pn.q ? c->pn.q + 4ll * B : nullptr, 4ll * B},
      {"pn_kl", c->pn.kl, B},               {"pn_sigma", c->pn.d_sigma, 1}};
  for (auto& e : t) {
    if (strcmp(e.nm, name) == 0) {
      if (n != e.cnt) return fail(c, DDQ_EINVAL, "blob %s has %lld elements", name, (long long)e.cnt);
      if (!strcmp(name, "grad_norm") && !(c->adam_on && c->nb.adam_clip > 0.f))
        return fail(c, DDQ_ESTATE, "blob grad_norm exists while Adam's gradient clipping is on");
      if (!strcmp(name, "Qn_out") && c->nb.obj_target != DDQ_TARGET_DOUBLE)
        return fail(c, DDQ_ESTATE, "blob Qn_out exists under the double target only");
      if (!strcmp(name, "m_bonus") && !c->nb.m_on)
        return fail(c, DDQ_ESTATE, "blob m_bonus exists while the Munchausen target is on");
      if (!strcmp(name, "Pc_out") && !(c->nb.m_on && c->nb.m_alpha != 0.f))
        return fail(c, DDQ_ESTATE, "blob Pc_out exists while the Munchausen target is on with "
                                   "alpha != 0");
      if ((!strcmp(name, "Qa_out") || !strncmp(name, "pn_", 3)) && !c->pn.on)
        return fail(c, DDQ_ESTATE, "blob %s exists while parameter-space noise is on "
                                   "(ddq_set_param_noise)", name);
      if (!strcmp(name, "aug_shift") && c->replay.aug_pad == 0)
        return fail(c, DDQ_ESTATE, "blob aug_shift exists while augmentation is on "
                                   "(ddq_replay_set_augment)");
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
  const ActWeights* over = nullptr;
  TRY(param_noise_move(c, &over));
  const size_t bytes = (size_t)n * 4 * c->nb.S * c->nb.S;
  HIP_TRY(c, hipMemcpyAsync(c->act.act_u8, states, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_u8_to_nhwc(c->act.act_u8, n, c->nb.S, c->act.act_in, c->stream));
  HIP_TRY(c, launch_act(c->nb, c->act.act_in, n, c->act.act_p3, c->act.act_h4, c->act.act_part, c->act.act_q,
                        c->act.act_out, c->act.act_p1s, c->act.act_p2s, c->stream, {}, c->act.act_path, 0, over));
  HIP_TRY(c, hipMemcpyAsync(actions, c->act.act_out, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}

// ---------------- apply ----------------
int ddq::check_cfg(ddq_ctx* c, const ddq_update_cfg* u) {
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
UpdateRule ddq::rule_of(const ddq_update_cfg& u, int period) {
  return UpdateRule{u.rule, period, u.lr, u.decay, u.eps, u.momentum, u.weight_decay};
}
int ddq::enqueue_apply(ddq_ctx* c, const NetBuffers& nb, const StepLaunch& sl, Marks m) {
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
  if (c->async.async_on)
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

// ---------------- measurement ----------------
// A mark names the kernel launched next: arm that launch's own start / stop
// events (common.h ddq_launch).  A mark no kernel follows (an RCCL call, the
// fused step's empty "apply") is still armed at the next mark: dropped.
static void mark_settle(ddq_ctx* c) {
  if (g_ext_timing.start && !c->marks.marks.empty()) c->marks.marks.pop_back();   // not launched
  g_ext_timing = ExtTiming{};
}

static void mark_cb(void* arg, const char* name) {
  ddq_ctx* c = reinterpret_cast<ddq_ctx*>(arg);
  mark_settle(c);
  while (c->marks.ev_used + 2 > c->marks.ev_pool.size()) {
    hipEvent_t e;
    hipEventCreate(&e);
    c->marks.ev_pool.push_back(e);
  }
  hipEvent_t e0 = c->marks.ev_pool[c->marks.ev_used++], e1 = c->marks.ev_pool[c->marks.ev_used++];
  g_ext_timing = ExtTiming{e0, e1};
  c->marks.marks.push_back({name, e0, e1});
}

int ddq_profile_step(ddq_ctx* c, const ddq_step_cfg* cfg, char* names, float* usec, int32_t cap,
                     int32_t* n) {
  TRY(check_step(c, cfg));
  TRY(check_monitor_step(c, cfg));
  if (!n) return fail(c, DDQ_EINVAL, "null n");
  if (is_async(c, cfg)) return fail(c, DDQ_EINVAL, "profile steps take no async exchange");
  TRY(check_not_async(c));
  TRY(set_dev(c));
  c->marks.marks.clear();
  c->marks.ev_used = 0;
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
  const int k = (int)c->marks.marks.size();
  *n = k;
  for (int i = 0; i < k && i < cap; ++i) {
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->marks.marks[i].start, c->marks.marks[i].stop));
    if (usec) usec[i] = ms * 1000.f;
    if (names) {
      memset(names + 16 * i, 0, 16);
      strncpy(names + 16 * i, c->marks.marks[i].name.c_str(), 15);
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
