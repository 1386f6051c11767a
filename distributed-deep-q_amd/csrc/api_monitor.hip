// libddq_hip C-ABI: the training monitor.
#include "ctx.h"

using namespace ddq;
// (the ddq_* definitions take their C linkage from include/ddq_hip.h)

static_assert(sizeof(MonitorRecord) == sizeof(ddq_monitor_record) && sizeof(MonitorRecord) == 160 &&
                  offsetof(MonitorRecord, grad_rms) == offsetof(ddq_monitor_record, grad_rms),
              "MonitorRecord is ddq_monitor_record");

// ---------------- training monitor ----------------
static void monitor_release(ddq_ctx* c) {
  MonitorEnv& m = c->mon.mon;
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
  c->mon.mon_period = 0;
}

int ddq_monitor_enable(ddq_ctx* c, int64_t capacity, int32_t period) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (capacity < 0 || capacity > (1ll << 24))
    return fail(c, DDQ_EINVAL, "capacity must be in [0, 2^24] (got %lld)", (long long)capacity);
  if (period < 0) return fail(c, DDQ_EINVAL, "period must be >= 0 (got %d)", period);
  if (period > 0 && capacity > 0 && c->async.async_on)
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
  c->mon.mon = m;
  if (rc != DDQ_OK) {
    const std::string msg = c->err;
    monitor_release(c);
    c->err = msg;
    return rc;
  }
  c->mon.mon_period = period;
  return DDQ_OK;
}

int ddq_monitor_record_async(ddq_ctx* c, int64_t tag) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->mon.mon.ring) return fail(c, DDQ_ESTATE, "monitor not enabled (ddq_monitor_enable)");
  TRY(set_dev(c));
  HIP_TRY(c, launch_monitor(c->mon.mon, 0, tag, c->stream));
  return DDQ_OK;
}

int ddq_monitor_read(ddq_ctx* c, int64_t first, int64_t n, ddq_monitor_record* out,
                     int64_t* total) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->mon.mon.ring) return fail(c, DDQ_ESTATE, "monitor not enabled (ddq_monitor_enable)");
  if (n < 0 || (n > 0 && !out)) return fail(c, DDQ_EINVAL, "bad argument");
  TRY(set_dev(c));
  int64_t cnt = 0;
  HIP_TRY(c, scopy(c, &cnt, c->mon.mon.count, sizeof(cnt), hipMemcpyDeviceToHost));
  if (total) *total = cnt;
  if (n == 0) return DDQ_OK;
  const int64_t cap = c->mon.mon.capacity;
  if (first < 0 || first + n > cnt || cnt - first > cap)
    return fail(c, DDQ_EINVAL, "records [%lld, %lld) not in the ring (taken %lld, capacity %lld)",
                (long long)first, (long long)(first + n), (long long)cnt, (long long)cap);
  for (int64_t k = first; k < first + n;) {   // at most two spans of the ring
    const int64_t slot = k % cap, run = std::min(first + n - k, cap - slot);
    HIP_TRY(c, hipMemcpyAsync(out + (k - first), c->mon.mon.ring + slot,
                              (size_t)run * sizeof(MonitorRecord), hipMemcpyDeviceToHost,
                              c->stream));
    k += run;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return DDQ_OK;
}
