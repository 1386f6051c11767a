// libddq_hip C-ABI: parameter-space noise (param_noise.h has the kernels).
#include <cmath>

#include "ctx.h"

using namespace ddq;
// (the ddq_* definitions take their C linkage from include/ddq_hip.h)

// theta~ is not a derived copy of theta_Q that writers maintain (DESIGN.md
// section 4): ddq_set_params, updates and syncs leave it alone, and it is
// stale by design until the next resample.

static int pn_draw(ddq_ctx* c) {
  HIP_TRY(c, launch_param_noise_draw(c->nb, c->pn.w.theta, c->pn.w.wks, c->pn.d_sigma,
                                     c->pn.cfg.seed, c->pn.epoch, c->stream));
  return DDQ_OK;
}

int ddq::param_noise_move(ddq_ctx* c, const ActWeights** over) {
  *over = nullptr;
  if (!c->pn.on) return DDQ_OK;
  const int64_t K = c->pn.cfg.resample_every;
  if (K > 0 && c->pn.moves > 0 && c->pn.moves % K == 0) {
    c->pn.epoch++;
    TRY(pn_draw(c));
  }
  c->pn.moves++;
  *over = &c->pn.w;
  return DDQ_OK;
}

int ddq_set_param_noise(ddq_ctx* c, const ddq_param_noise_cfg* p) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!p) return fail(c, DDQ_EINVAL, "null param noise cfg");
  if (p->enabled != 0 && p->enabled != 1)
    return fail(c, DDQ_EINVAL, "enabled must be 0 or 1 (got %d)", (int)p->enabled);
  if (p->reserved != 0) return fail(c, DDQ_EINVAL, "reserved must be 0");
  if (p->enabled) {
    if (!(std::isfinite(p->sigma) && p->sigma >= 0.f))
      return fail(c, DDQ_EINVAL, "sigma must be finite and >= 0 (got %g)", (double)p->sigma);
    if (!(std::isfinite(p->delta) && p->delta > 0.f))
      return fail(c, DDQ_EINVAL, "delta must be finite and > 0 (got %g)", (double)p->delta);
    if (!(std::isfinite(p->adapt_coef) && p->adapt_coef > 1.f))
      return fail(c, DDQ_EINVAL, "adapt_coef must be finite and > 1 (got %g)", (double)p->adapt_coef);
    if (p->resample_every < 0)
      return fail(c, DDQ_EINVAL, "resample_every must be >= 0 (got %d)", (int)p->resample_every);
  }
  TRY(guard(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  ddq_ctx::ParamNoise& n = c->pn;
  if (!p->enabled) {               // the buffers stay: nothing the default path uses
    n.on = false;
    n.cfg = ddq_param_noise_cfg{};
    return DDQ_OK;
  }
  const NetBuffers& nb = c->nb;
  if (!n.w.theta) TRY(dalloc(c, &n.w.theta, (size_t)nb.L.total));
  if (!n.w.wks) TRY(dalloc(c, &n.w.wks, (size_t)3 * nb.L.wks_total));
  if (!n.d_sigma) TRY(dalloc(c, &n.d_sigma, 1));
  if (!n.q) TRY(dalloc(c, &n.q, (size_t)2 * nb.B * 4));
  if (!n.kl) TRY(dalloc(c, &n.kl, (size_t)nb.B));
  n.cfg = *p;
  n.epoch = 0;
  n.moves = 0;
  HIP_TRY(c, hipMemcpyAsync(n.d_sigma, &n.cfg.sigma, sizeof(float), hipMemcpyHostToDevice, c->stream));
  TRY(pn_draw(c));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  n.on = true;
  return DDQ_OK;
}

int ddq_get_param_noise(const ddq_ctx* c, ddq_param_noise_cfg* p) {
  if (!c || !p) return fail(nullptr, DDQ_EINVAL, "null argument");
  *p = c->pn.cfg;
  return DDQ_OK;
}

static int pn_on(ddq_ctx* c, const char* what) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->pn.on)
    return fail(c, DDQ_ESTATE, "%s: parameter-space noise is off (ddq_set_param_noise)", what);
  return guard(c);
}

int ddq_param_noise_resample_async(ddq_ctx* c) {
  TRY(pn_on(c, "ddq_param_noise_resample_async"));
  c->pn.epoch++;
  return pn_draw(c);
}

int ddq_param_noise_adapt_async(ddq_ctx* c) {
  TRY(pn_on(c, "ddq_param_noise_adapt_async"));
  const NetBuffers& nb = c->nb;
  const ddq_ctx::ParamNoise& n = c->pn;
  c->pn.epoch++;
  TRY(pn_draw(c));
  float* q[2] = {n.q, n.q + 4ll * nb.B};
  for (int z = 0; z < 2; ++z)
    HIP_TRY(c, launch_act(nb, nb.mb.state, nb.B, c->act.act_p3, c->act.act_h4, c->act.act_part, q[z],
                          nullptr, c->act.act_p1s, c->act.act_p2s, c->stream, {}, c->act.act_path, 0,
                          z ? &n.w : nullptr));
  HIP_TRY(c, launch_param_noise_adapt(q[0], q[1], nb.B, n.cfg.delta, n.cfg.adapt_coef, n.kl, n.d_sigma,
                                      c->stream));
  return DDQ_OK;
}

int ddq_param_noise_params(ddq_ctx* c, float* dst, int64_t n) {
  if (c && !dst) return fail(c, DDQ_EINVAL, "null argument");
  TRY(pn_on(c, "ddq_param_noise_params"));
  if (n != c->nb.L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  HIP_TRY(c, hipMemcpyAsync(dst, c->pn.w.theta, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}
