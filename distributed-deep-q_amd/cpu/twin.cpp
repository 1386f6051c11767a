// libddq_cpu.so -- the CPU-mode twin of libddq_hip.so (include/ddq_hip.h).
//
// The reference runs its Barista worker in Caffe CPU mode when asked
// (`--mode cpu`, main.py:128,149-151; BASELINE.json configs[0]: "Caffe CPU
// mode, single Barista worker driven by barista.dummy_client (plumbing, no
// GPU)").  This library exports every ddq_* symbol of the C-ABI so the same
// host layer (ddq.DeepQNet(mode="cpu"), the Barista worker, the param server)
// runs on a machine without a GPU.  It computes what the HIP library computes
// -- the deepq network of models/deepq/train_val.prototxt:38-483 (both
// towers, Q(s,a), the Bellman target 0.85 max_a P + r, the Euclidean loss, the
// Q backward), the replay ring of replay.py, the Snake actor of expgain.py +
// gamesim/SnakeGame.py (ddq_actor_*), the lock-step policy evaluation of
// evaluation.py with per-game streams (ddq_eval_*) and the update rules of
// server.py:49-124 -- with plain C++ loops over NCHW fp32 tensors,
// accumulating every dot product in double and rounding once per layer
// output (so it is no less exact than the GPU's fp32-exact split products).
// The update rules round exactly as the HIP library's apply_rule (built with
// -ffp-contract=off): the same fp32 operations in the same order.
//
// What needs a GPU stream or a communicator (device index draws, large-batch
// gathers, hipGraph steps, RCCL exchanges, in-process groups, the async param
// server, kernel timing) returns DDQ_ESTATE ("CPU mode") -- the reference's
// CPU mode has none of those either.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ddq_hip.h"

namespace {

thread_local std::string g_err;

constexpr int kA = 4;          // actions (barista/constants.py:8)
constexpr int kC = 4;          // frames per state (expgain.py:9)
constexpr int kH4 = 512;       // fc4 units (train_val.prototxt:165)

struct Layout {
  int S;
  int64_t w[5], b[5], wn[5], bn[5], total;
};

Layout make_layout(int S) {
  Layout L{};
  L.S = S;
  const int64_t s4 = S / 8;
  const int64_t wn[5] = {32ll * 4 * 49, 64ll * 32 * 25, 64ll * 64 * 9, kH4 * 64 * s4 * s4, kA * kH4};
  const int64_t bn[5] = {32, 64, 64, kH4, kA};
  int64_t o = 0;
  for (int i = 0; i < 5; ++i) {
    L.w[i] = o; L.wn[i] = wn[i]; o += wn[i];
    L.b[i] = o; L.bn[i] = bn[i]; o += bn[i];
  }
  L.total = o;
  return L;
}

// conv layer geometry: (cin, cout, k, pad) of train_val.prototxt:39-158
struct Conv { int cin, cout, k, pad; };
constexpr Conv kConv[3] = {{4, 32, 7, 3}, {32, 64, 5, 2}, {64, 64, 3, 1}};

// One tower's activations for a batch (NCHW fp32).
struct Tower {
  std::vector<float> x[3];       // input of conv l (x[0]: the frames)
  std::vector<uint8_t> route[3]; // pool l routing: 0..3 first max in window order, 4: ReLU'd
  std::vector<float> pool3;      // (B, 64, S/8, S/8) = fc4's input, Caffe flatten order
  std::vector<float> h4, out;    // (B, 512), (B, 4)
};

}  // namespace

struct ddq_ctx {
  int B = 0, S = 0;
  float gamma = 0.85f;
  Layout L{};
  std::vector<float> theta[2], grad, opt;
  int first = 1;                 // the next apply is the first since a reset
  int64_t iter = 0;
  float target_tau = 1.f;        // ddq_set_target_tau (ddq_soft_sync_target blends with it)
  // Adam (ddq_set_adam): opt holds m, opt2 v; gnorm: the last pre-clip norm
  bool adam_on = false;
  ddq_adam_cfg adam{0.f, 0.f, 0.f, 0.f};
  std::vector<float> opt2;
  float gnorm = 0.f;
  // minibatch (Caffe shapes)
  std::vector<float> state, next_state, action, reward, nonterm;
  std::vector<int32_t> idx;
  // blobs of the last forward
  std::vector<float> q_out, p_out, q_sa, p_sa, target;
  float loss = 0.f;
  Tower tw[3];                   // Q on state, P on next_state, Q on next_state (DOUBLE)
  // selectable objective (ddq_set_objective) and its two blobs
  ddq_objective obj{DDQ_TARGET_MAX, DDQ_LOSS_EUCLIDEAN, 0.f, 0};
  std::vector<float> qn_out, dq_out;
  // replay ring (replay.py:23-68)
  std::vector<uint8_t> r_state, r_action, r_nonterm;
  std::vector<int16_t> r_reward;
  int64_t head = 0, valid = 0, capacity = 0;
  // laned ring (ddq_replay_set_lanes): lanes rings of lane_len slots, head /
  // valid per lane
  int32_t lanes = 1;
  int64_t lane_len = 0;
  int32_t nstep = 1;               // n-step returns (ddq_replay_set_nstep)
  // prioritized replay (ddq_replay_set_priority): a flat leaf array, the draw is
  // a linear prefix scan; isw: the bound minibatch's weights
  bool prio_on = false;
  ddq_priority_cfg prio_cfg{0, 0.f, 0.f, 0.f};
  std::vector<uint32_t> prio_q;
  uint32_t prio_pmax = 65536u;
  uint64_t prio_ctr = 0;           // prioritized draws so far (the draw counter)
  std::vector<float> isw;
  bool idx_bound = false;
  int64_t steps = 0;
  // Snake environments.  A game: its RNG stream and position, its counters, the
  // 4-board history (oldest first) and its start board
  struct Game {
    uint64_t seed = 0, draws = 0;
    int64_t steps = 0, games = 0, reward = 0;
    int8_t boards[4][100], init[100];
  };
  // an evaluated game also has its lock-step move counter, the running
  // episode's score / moves and its episode log
  struct EvalGame : Game {
    int32_t move = 0, score = 0, moves = 0;
    std::vector<int32_t> log;      // 4 per record: end_move, score, moves, ended_by
  };
  template <class G>
  struct Env {
    std::vector<G> games;          // empty: not created
    std::vector<int32_t> row, col; // the zoom maps
  };
  Env<Game> a_env;                 // Snake actor (ddq_actor_*): one game
  Env<EvalGame> e_env;             // policy evaluation (ddq_eval_*): games in lock step
  Env<Game> p_env;                 // actor pool (ddq_actors_*): one game per ring lane
  double e_eps = 0.0;
  int32_t e_max_moves = 0, e_max_ep = 0;
  int64_t e_moves = 0;
  // training monitor (ddq_monitor_*): the ring (empty: off) and the records taken
  std::vector<ddq_monitor_record> m_ring;
  int64_t m_total = 0;
  // pool: the ring's per-lane head / valid at create, moves made since (the
  // HIP library's launch constants; here only the "counters" section has them)
  int64_t p_h0 = 0, p_v0 = 0, p_moves = 0;
  // checkpoint and resume (ddq_state_*): restoring from the first
  // ddq_state_write of a section other than "config" until ddq_state_commit;
  // the counters and the games as written (the games in the sections' layout)
  bool restoring = false;
  ddq_state_counters st_ctr{};
  std::vector<uint8_t> st_actor, st_pool;
  std::string err;
};

namespace {

int fail(ddq_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  g_err = buf;
  return code;
}

// The guard of every call that computes on the training state: not between
// the first ddq_state_write and ddq_state_commit.
int not_restoring(ddq_ctx* c) {
  if (c->restoring)
    return fail(c, DDQ_ESTATE, "restore not committed: sections were written with ddq_state_write, "
                               "call ddq_state_commit first");
  return DDQ_OK;
}

int cpu_only(ddq_ctx* c, const char* what) {
  return fail(c, DDQ_ESTATE, "%s: not available in CPU mode (libddq_cpu.so); use libddq_hip.so",
              what);
}

// ---- forward ----
// out[b][co][y][x] = bias[co] + sum_{ci,ky,kx} W[co][ci][ky][kx] in[b][ci][y+ky-p][x+kx-p]
void conv_fwd(const float* in, int B, int H, const Conv& cv, const float* W, const float* bias,
              float* out) {
  const int k = cv.k, p = cv.pad, HW = H * H;
#pragma omp parallel for collapse(2) schedule(static)
  for (int b = 0; b < B; ++b)
    for (int co = 0; co < cv.cout; ++co) {
      std::vector<double> acc(HW, (double)bias[co]);
      for (int ci = 0; ci < cv.cin; ++ci) {
        const float* src = in + ((size_t)b * cv.cin + ci) * HW;
        const float* w = W + ((size_t)co * cv.cin + ci) * k * k;
        for (int ky = 0; ky < k; ++ky)
          for (int kx = 0; kx < k; ++kx) {
            const double wv = w[ky * k + kx];
            const int y0 = std::max(0, p - ky), y1 = std::min(H, H + p - ky);
            const int x0 = std::max(0, p - kx), x1 = std::min(H, H + p - kx);
            for (int y = y0; y < y1; ++y) {
              const float* row = src + (y + ky - p) * H + (kx - p);
              double* a = acc.data() + y * H;
              for (int x = x0; x < x1; ++x) a[x] += wv * row[x];
            }
          }
      }
      float* dst = out + ((size_t)b * cv.cout + co) * HW;
      for (int i = 0; i < HW; ++i) dst[i] = (float)acc[i];
    }
}

// ReLU (in place, train_val.prototxt RELU layers) + 2x2 / 2 max pool with the
// first maximum of the window in (0,0) (0,1) (1,0) (1,1) order; route 4 when
// the window's maximum is not positive (no gradient passes the ReLU there)
void relu_pool(const float* pre, int B, int C, int H, float* out, uint8_t* route) {
  const int Ho = H / 2;
#pragma omp parallel for collapse(2) schedule(static)
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c) {
      const float* s = pre + ((size_t)b * C + c) * H * H;
      for (int y = 0; y < Ho; ++y)
        for (int x = 0; x < Ho; ++x) {
          const float v[4] = {s[(2 * y) * H + 2 * x], s[(2 * y) * H + 2 * x + 1],
                              s[(2 * y + 1) * H + 2 * x], s[(2 * y + 1) * H + 2 * x + 1]};
          int arg = 0;
          float mx = v[0];
          for (int q = 1; q < 4; ++q)
            if (v[q] > mx) { mx = v[q]; arg = q; }
          const size_t o = (((size_t)b * C + c) * Ho + y) * Ho + x;
          out[o] = mx > 0.f ? mx : 0.f;
          route[o] = (uint8_t)(mx > 0.f ? arg : 4);
        }
    }
}

// y[b][n] = bias[n] + sum_k W[n][k] x[b][k]
void dense(const float* x, int B, int K, int N, const float* W, const float* bias, float* y,
           bool relu) {
#pragma omp parallel for collapse(2) schedule(static)
  for (int b = 0; b < B; ++b)
    for (int n = 0; n < N; ++n) {
      double a = bias[n];
      const float* w = W + (size_t)n * K;
      const float* xb = x + (size_t)b * K;
      for (int k = 0; k < K; ++k) a += (double)w[k] * xb[k];
      const float v = (float)a;
      y[(size_t)b * N + n] = relu ? (v > 0.f ? v : 0.f) : v;
    }
}

// tower slot z with the weights of tower zw (slot 2: Q's weights on next_state)
void tower_fwd(ddq_ctx* c, int z, const float* frames, int B, int zw = -1) {
  const Layout& L = c->L;
  const float* th = c->theta[zw < 0 ? z : zw].data();
  Tower& t = c->tw[z];
  int H = c->S;
  t.x[0].assign(frames, frames + (size_t)B * kC * H * H);
  std::vector<float> pre;
  for (int l = 0; l < 3; ++l) {
    const Conv& cv = kConv[l];
    pre.assign((size_t)B * cv.cout * H * H, 0.f);
    conv_fwd(t.x[l].data(), B, H, cv, th + L.w[l], th + L.b[l], pre.data());
    const size_t np = (size_t)B * cv.cout * (H / 2) * (H / 2);
    std::vector<float>& nxt = l < 2 ? t.x[l + 1] : t.pool3;
    nxt.assign(np, 0.f);
    t.route[l].assign(np, 4);
    relu_pool(pre.data(), B, cv.cout, H, nxt.data(), t.route[l].data());
    H /= 2;
  }
  const int K4 = 64 * H * H;
  t.h4.assign((size_t)B * kH4, 0.f);
  dense(t.pool3.data(), B, K4, kH4, th + L.w[3], th + L.b[3], t.h4.data(), true);
  t.out.assign((size_t)B * kA, 0.f);
  dense(t.h4.data(), B, kH4, kA, th + L.w[4], th + L.b[4], t.out.data(), false);
}

// ---- backward (Q tower) ----
// gW[co][ci][ky][kx] = sum_{b,y,x} d[b][co][y][x] in[b][ci][y+ky-p][x+kx-p]; gb[co] = sum d.
// Per (co, ci) the products accumulate elementwise into one double row per
// tap ([tap][x]: independent lanes, so the inner loop vectorises), summed
// over x at the end.
void conv_wgrad(const float* in, const float* d, int B, int H, const Conv& cv, float* gW,
                float* gb) {
  const int k = cv.k, p = cv.pad, HW = H * H;
#pragma omp parallel for collapse(2) schedule(dynamic)
  for (int co = 0; co < cv.cout; ++co)
    for (int ci = 0; ci < cv.cin; ++ci) {
      std::vector<double> acc((size_t)k * k * H, 0.0);
      for (int b = 0; b < B; ++b) {
        const float* src = in + ((size_t)b * cv.cin + ci) * HW;
        const float* dd = d + ((size_t)b * cv.cout + co) * HW;
        for (int ky = 0; ky < k; ++ky)
          for (int kx = 0; kx < k; ++kx) {
            const int y0 = std::max(0, p - ky), y1 = std::min(H, H + p - ky);
            const int x0 = std::max(0, p - kx), x1 = std::min(H, H + p - kx);
            double* a = acc.data() + (size_t)(ky * k + kx) * H;
            for (int y = y0; y < y1; ++y) {
              const float* row = src + (y + ky - p) * H + (kx - p);
              const float* dr = dd + y * H;
              for (int x = x0; x < x1; ++x) a[x] += (double)dr[x] * row[x];
            }
          }
      }
      float* g = gW + ((size_t)co * cv.cin + ci) * k * k;
      for (int t = 0; t < k * k; ++t) {
        double v = 0.0;
        for (int x = 0; x < H; ++x) v += acc[(size_t)t * H + x];
        g[t] = (float)v;
      }
    }
#pragma omp parallel for schedule(static)
  for (int co = 0; co < cv.cout; ++co) {
    double a = 0.0;
    for (int b = 0; b < B; ++b) {
      const float* dd = d + ((size_t)b * cv.cout + co) * HW;
      for (int i = 0; i < HW; ++i) a += dd[i];
    }
    gb[co] = (float)a;
  }
}

// dx[b][ci][iy][ix] = sum_{co,ky,kx} d[b][co][iy-ky+p][ix-kx+p] W[co][ci][ky][kx]
void conv_dgrad(const float* d, int B, int H, const Conv& cv, const float* W, float* dx) {
  const int k = cv.k, p = cv.pad, HW = H * H;
#pragma omp parallel for collapse(2) schedule(static)
  for (int b = 0; b < B; ++b)
    for (int ci = 0; ci < cv.cin; ++ci) {
      std::vector<double> acc(HW, 0.0);
      for (int co = 0; co < cv.cout; ++co) {
        const float* dd = d + ((size_t)b * cv.cout + co) * HW;
        const float* w = W + ((size_t)co * cv.cin + ci) * k * k;
        for (int ky = 0; ky < k; ++ky)
          for (int kx = 0; kx < k; ++kx) {
            const double wv = w[ky * k + kx];
            // input pixel iy receives output pixel y = iy - ky + p
            const int iy0 = std::max(0, ky - p), iy1 = std::min(H, H + ky - p);
            const int ix0 = std::max(0, kx - p), ix1 = std::min(H, H + kx - p);
            for (int iy = iy0; iy < iy1; ++iy) {
              const float* row = dd + (iy - ky + p) * H + (p - kx);
              double* a = acc.data() + iy * H;
              for (int ix = ix0; ix < ix1; ++ix) a[ix] += wv * row[ix];
            }
          }
      }
      float* dst = dx + ((size_t)b * cv.cin + ci) * HW;
      for (int i = 0; i < HW; ++i) dst[i] = (float)acc[i];
    }
}

// the pooled gradient routed to its window's first maximum (0 elsewhere and
// for ReLU'd windows): the pre-activation gradient of the conv below
void unpool(const float* dpool, const uint8_t* route, int B, int C, int Ho, float* dpre) {
  const int H = 2 * Ho;
  std::fill(dpre, dpre + (size_t)B * C * H * H, 0.f);
#pragma omp parallel for collapse(2) schedule(static)
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c)
      for (int y = 0; y < Ho; ++y)
        for (int x = 0; x < Ho; ++x) {
          const size_t o = (((size_t)b * C + c) * Ho + y) * Ho + x;
          const int r = route[o];
          if (r < 4)
            dpre[(((size_t)b * C + c) * H + 2 * y + (r >> 1)) * H + 2 * x + (r & 1)] = dpool[o];
        }
}

int forward_backward(ddq_ctx* c) {
  const int B = c->B, S = c->S;
  const Layout& L = c->L;
  tower_fwd(c, 0, c->state.data(), B);
  tower_fwd(c, 1, c->next_state.data(), B);
  const bool dbl = c->obj.target == DDQ_TARGET_DOUBLE, huber = c->obj.loss == DDQ_LOSS_HUBER;
  if (dbl) {   // Q(s', .) under theta_Q: the Double-DQN action choice
    tower_fwd(c, 2, c->next_state.data(), B, 0);
    c->qn_out = c->tw[2].out;
  }
  const Tower& q = c->tw[0];
  const Tower& p = c->tw[1];
  c->q_out = q.out;
  c->p_out = p.out;
  c->dq_out.assign((size_t)B * kA, 0.f);
  const double delta = c->obj.huber_delta;
  c->q_sa.assign(B, 0.f); c->p_sa.assign(B, 0.f); c->target.assign(B, 0.f);
  // head: ELTWISE PROD + SLICE + SUM (Q(s,a)), SLICE + MAX * non_terminal (max_a
  // P), SUM with coefficients (gamma, 1), EUCLIDEAN_LOSS (train_val.prototxt:385-483)
  std::vector<double> dq((size_t)B * kA, 0.0);
  double loss = 0.0;
  for (int b = 0; b < B; ++b) {
    double qs = 0.0, pm = p.out[(size_t)b * kA];
    for (int a = 0; a < kA; ++a) {
      qs += (double)q.out[(size_t)b * kA + a] * c->action[(size_t)b * kA + a];
      pm = std::max(pm, (double)p.out[(size_t)b * kA + a]);
    }
    if (dbl) {   // P at the first maximum of Qn_out[b] (argmax rule: first max wins)
      const float* qn = c->qn_out.data() + (size_t)b * kA;
      int best = 0;
      for (int a = 1; a < kA; ++a)
        if (qn[a] > qn[best]) best = a;
      pm = p.out[(size_t)b * kA + best];
    }
    const float qsf = (float)qs;
    const float psf = (float)(pm * c->nonterm[b]);
    const float tg = (float)((double)c->gamma * psf + 1.0 * c->reward[b]);
    c->q_sa[b] = qsf; c->p_sa[b] = psf; c->target[b] = tg;
    const double diff = (double)qsf - tg;
    double dc = diff;
    if (huber) {   // h(d) scaled by 2: d^2 inside the band, delta (2|d| - delta) outside
      const double ad = std::fabs(diff);
      dc = std::min(std::max(diff, -delta), delta);
      loss += ad <= delta ? diff * diff : delta * (2.0 * ad - delta);
    } else {
      loss += diff * diff;
    }
    if (c->prio_on) {   // importance-sampling weight on dQ and on the loss term
      const double w = c->isw[b], le = huber ? (std::fabs(diff) <= delta
                                                    ? diff * diff
                                                    : delta * (2.0 * std::fabs(diff) - delta))
                                             : diff * diff;
      loss += (w - 1.0) * le;          // (w == 1: adds 0, the unweighted sum)
    }
    const double wt = c->prio_on ? (double)c->isw[b] : 1.0;
    for (int a = 0; a < kA; ++a) {
      dq[(size_t)b * kA + a] = c->action[(size_t)b * kA + a] * dc / B * wt;
      c->dq_out[(size_t)b * kA + a] = (float)dq[(size_t)b * kA + a];
    }
  }
  c->loss = (float)(loss / B / 2.0);
  float* g = c->grad.data();
  const float* th = c->theta[0].data();
  const int s4 = S / 8, K4 = 64 * s4 * s4;
  // Q_out (IP 512 -> 4)
  for (int a = 0; a < kA; ++a) {
    double gb = 0.0;
    for (int b = 0; b < B; ++b) gb += dq[(size_t)b * kA + a];
    g[L.b[4] + a] = (float)gb;
    for (int n = 0; n < kH4; ++n) {
      double gw = 0.0;
      for (int b = 0; b < B; ++b) gw += dq[(size_t)b * kA + a] * q.h4[(size_t)b * kH4 + n];
      g[L.w[4] + (size_t)a * kH4 + n] = (float)gw;
    }
  }
  // dh4 = (dQ W5) masked by the ReLU
  std::vector<float> dh4((size_t)B * kH4, 0.f);
  for (int b = 0; b < B; ++b)
    for (int n = 0; n < kH4; ++n) {
      if (!(q.h4[(size_t)b * kH4 + n] > 0.f)) continue;
      double v = 0.0;
      for (int a = 0; a < kA; ++a) v += dq[(size_t)b * kA + a] * th[L.w[4] + (size_t)a * kH4 + n];
      dh4[(size_t)b * kH4 + n] = (float)v;
    }
  // fc4 (IP K4 -> 512)
#pragma omp parallel for schedule(static)
  for (int n = 0; n < kH4; ++n) {
    double gb = 0.0;
    for (int b = 0; b < B; ++b) gb += dh4[(size_t)b * kH4 + n];
    g[L.b[3] + n] = (float)gb;
    for (int k = 0; k < K4; ++k) {
      double gw = 0.0;
      for (int b = 0; b < B; ++b) gw += (double)dh4[(size_t)b * kH4 + n] * q.pool3[(size_t)b * K4 + k];
      g[L.w[3] + (size_t)n * K4 + k] = (float)gw;
    }
  }
  std::vector<float> dpool((size_t)B * K4, 0.f);
#pragma omp parallel for collapse(2) schedule(static)
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < K4; ++k) {
      double v = 0.0;
      for (int n = 0; n < kH4; ++n)
        v += (double)dh4[(size_t)b * kH4 + n] * th[L.w[3] + (size_t)n * K4 + k];
      dpool[(size_t)b * K4 + k] = (float)v;
    }
  // conv3 -> conv1
  std::vector<float> dpre, dx;
  int Ho = s4;
  for (int l = 2; l >= 0; --l) {
    const Conv& cv = kConv[l];
    const int H = 2 * Ho;
    dpre.assign((size_t)B * cv.cout * H * H, 0.f);
    unpool(dpool.data(), q.route[l].data(), B, cv.cout, Ho, dpre.data());
    conv_wgrad(q.x[l].data(), dpre.data(), B, H, cv, g + L.w[l], g + L.b[l]);
    if (l > 0) {
      dx.assign((size_t)B * cv.cin * H * H, 0.f);
      conv_dgrad(dpre.data(), B, H, cv, th + L.w[l], dx.data());
      dpool.swap(dx);
    }
    Ho = H;
  }
  return DDQ_OK;
}

// server.py:81-124 + Caffe SGDSolver momentum, the HIP library's apply_rule
// operation for operation (fp32, no contraction: -ffp-contract=off)
float apply_rule(const ddq_update_cfg& u, bool first, bool is_bias, float th, float g, float& st) {
  switch (u.rule) {
    case DDQ_RULE_SGD:
      return th - u.lr * g;
    case DDQ_RULE_RMSPROP: {
      const float g2 = g * g;
      const float c_use = first ? g2 : st;
      st = first ? g2 : (u.decay * st + (1.0f - u.decay) * g2);
      return th - (u.lr * g) / sqrtf(c_use + u.eps);
    }
    case DDQ_RULE_ADAGRAD: {
      const float acc = first ? g * g : st + g * g;
      st = acc;
      return th - (u.lr * g) / sqrtf(acc + u.eps);
    }
    default: {
      const float lr = u.lr * (is_bias ? 2.f : 1.f);
      const float wd = is_bias ? 0.f : u.weight_decay;
      const float v = u.momentum * (first ? 0.f : st) + lr * (g + wd * th);
      st = v;
      return th - v;
    }
  }
}

// n-step returns (include/ddq_hip.h): forbidden start slots, the allowed count
// per lane
bool slot_forbidden(const ddq_ctx* c, int64_t x) {
  int64_t d = c->head - 1 - x;
  if (d < 0 && c->nstep >= 2 && c->valid == c->lane_len) d += c->lane_len;
  return d >= 0 && d < c->nstep;
}

int64_t allowed_slots(const ddq_ctx* c) {
  if (c->nstep < 2) return c->valid - 1;
  if (c->valid == c->lane_len) return c->lane_len - c->nstep;
  const int64_t lo = std::max<int64_t>(0, c->head - c->nstep);
  const int64_t hi = std::min(c->head - 1, c->valid - 1);
  return c->valid - std::max<int64_t>(0, hi - lo + 1);
}

// ---- prioritized replay (include/ddq_hip.h): the contract on a flat array ----
constexpr uint32_t kPrioOne = 65536u, kPrioMax = 1u << 24;

uint64_t prio_mix64(uint64_t x) {   // splitmix64
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

bool prio_forbidden(int64_t x, int64_t head, int64_t valid, int64_t L, int n) {
  int64_t d = head - 1 - x;
  if (d < 0 && n >= 2 && valid == L) d += L;
  return d >= 0 && d < n;
}

// every filled, allowed slot <- pmax = 1.0, the rest 0
void prio_rebuild(ddq_ctx* c) {
  if (!c->prio_on) return;
  c->prio_pmax = kPrioOne;
  c->prio_q.assign((size_t)c->capacity, 0u);
  for (int64_t i = 0; i < c->capacity; ++i) {
    const int64_t x = i % c->lane_len;
    if (x < c->valid && !prio_forbidden(x, c->head, c->valid, c->lane_len, c->nstep))
      c->prio_q[i] = c->prio_pmax;
  }
  c->idx_bound = false;
}

// the writer rule, after an add at lane-local slot h of the lane at `base`;
// c->head / c->valid are already the values after the add
void prio_on_add(ddq_ctx* c, int64_t base, int64_t h) {
  if (!c->prio_on) return;
  const int64_t L = c->lane_len;
  c->prio_q[base + h] = prio_forbidden(h, c->head, c->valid, L, c->nstep) ? 0u : c->prio_pmax;
  int64_t x = h - c->nstep;
  if (x < 0 && c->valid == L) x += L;
  if (x >= 0 && x != h && c->prio_q[base + x] == 0u) c->prio_q[base + x] = c->prio_pmax;
}

void prio_draw(ddq_ctx* c, uint64_t seed, uint64_t ctr) {
  const int B = c->B;
  unsigned long long T = 0;
  for (uint32_t v : c->prio_q) T += v;
  std::vector<uint32_t> qs(B, 1u);
  int64_t i = 0;                       // u_j is nondecreasing in j: one pass over the leaves
  unsigned long long C = 0;            // exclusive prefix sum at slot i
  uint32_t qmin = 0xFFFFFFFFu;
  for (int j = 0; j < B; ++j) {
    const unsigned long long lo = T * (unsigned long long)j / B, hi = T * (unsigned long long)(j + 1) / B;
    const uint64_t r = prio_mix64(seed ^ prio_mix64(ctr * 0x100000001B3ull + (uint64_t)j * 0x9E37ull));
    const unsigned long long u = lo + (unsigned long long)(((unsigned __int128)r * (hi - lo)) >> 64);
    while (i + 1 < c->capacity && C + c->prio_q[i] <= u) C += c->prio_q[i++];
    c->idx[j] = (int32_t)i;
    qs[j] = c->prio_q[i] ? c->prio_q[i] : 1u;
    qmin = std::min(qmin, qs[j]);
  }
  for (int j = 0; j < B; ++j) c->isw[j] = powf((float)qmin / (float)qs[j], c->prio_cfg.beta);
}

uint32_t prio_leaf_of(float d, float eps, float alpha) {
  const float p = powf(fabsf(d) + eps, alpha);
  if (!std::isfinite(p)) return kPrioMax;
  const float v = rintf(p * 65536.0f);
  if (!(v >= 1.0f)) return 1u;
  if (v >= (float)kPrioMax) return kPrioMax;
  return (uint32_t)v;
}

void prio_commit(ddq_ctx* c) {
  for (int b = 0; b < c->B; ++b) {     // ascending b: the highest b of a repeated slot wins
    const int64_t i = c->idx[b];
    if (i < 0 || i >= c->capacity || c->prio_q[i] == 0u) continue;
    bool later = false;
    for (int o = b + 1; o < c->B && !later; ++o) later = c->idx[o] == i;
    if (later) continue;
    const uint32_t v = prio_leaf_of(c->q_sa[b] - c->target[b], c->prio_cfg.eps, c->prio_cfg.alpha);
    c->prio_q[i] = v;
    c->prio_pmax = std::max(c->prio_pmax, v);
  }
}

void gather(ddq_ctx* c) {
  const int B = c->B, SS = c->S * c->S;
  const size_t slot = (size_t)kC * SS;
  const int64_t L = c->lane_len;
  const int n = c->nstep;
  for (int b = 0; b < B; ++b) {
    const int64_t i = c->idx[b];
    // replay.py:159-183 at n = 1; the n-step window s_k = base + (x + k) mod L
    // within the lane (one lane: the ring), cut at its first terminal slot
    const int64_t base = i - i % L, x = i - base;
    auto sk = [&](int k) { return base + (x + k) % L; };
    const int64_t nxt = sk(1);
    int m = n;
    bool term = false;
    for (int k = 1; k <= n; ++k)
      if (!c->r_nonterm[sk(k)]) { m = k; term = true; break; }
    const int64_t sm = sk(m);
    for (size_t e = 0; e < slot; ++e) {
      c->state[(size_t)b * slot + e] = c->r_state[(size_t)i * slot + e];
      c->next_state[(size_t)b * slot + e] = c->r_state[(size_t)sm * slot + e];
    }
    const int a = c->r_action[nxt];
    for (int k = 0; k < kA; ++k) c->action[(size_t)b * kA + k] = k == a ? 1.f : 0.f;
    // fp32, each * and + rounded on its own (-ffp-contract=off), in the device's order
    float g = 1.0f, w = 1.0f, R = (float)c->r_reward[nxt];
    for (int k = 2; k <= n; ++k) w = w * c->gamma;
    for (int k = 2; k <= m; ++k) {
      g = g * c->gamma;
      const float gr = g * (float)c->r_reward[sk(k)];
      R = R + gr;
    }
    c->reward[b] = R;
    c->nonterm[b] = term ? 0.0f : w;
  }
}

}  // namespace

extern "C" {

int ddq_abi_version(void) { return DDQ_ABI_VERSION; }

const char* ddq_last_error(const ddq_ctx* c) { return c ? c->err.c_str() : g_err.c_str(); }

int ddq_create(ddq_ctx** out, int device, const ddq_net_desc* d) {
  (void)device;
  if (!out || !d) return fail(nullptr, DDQ_EINVAL, "null argument");
  *out = nullptr;
  if (d->channels != 4 || d->actions != 4)
    return fail(nullptr, DDQ_EINVAL, "channels and actions must be 4 (got %d, %d)", d->channels,
                d->actions);
  if (d->frame < 16 || d->frame % 8 != 0 || d->frame > 1024)
    return fail(nullptr, DDQ_EINVAL, "frame side must be a multiple of 8 in [16,1024] (got %d)",
                d->frame);
  if (d->batch < 1 || d->batch > 1024)
    return fail(nullptr, DDQ_EINVAL, "batch must be in [1,1024] (got %d)", d->batch);
  ddq_ctx* c = new ddq_ctx();
  c->B = d->batch; c->S = d->frame; c->gamma = d->gamma;
  c->L = make_layout(c->S);
  const int64_t P = c->L.total;
  for (auto& t : c->theta) t.assign(P, 0.f);
  c->grad.assign(P, 0.f);
  c->opt.assign(P, 0.f);
  const size_t img = (size_t)c->B * kC * c->S * c->S;
  c->state.assign(img, 0.f); c->next_state.assign(img, 0.f);
  c->action.assign((size_t)c->B * kA, 0.f);
  c->reward.assign(c->B, 0.f); c->nonterm.assign(c->B, 0.f);
  c->idx.assign(c->B, 0);
  c->q_out.assign((size_t)c->B * kA, 0.f); c->p_out.assign((size_t)c->B * kA, 0.f);
  c->q_sa.assign(c->B, 0.f); c->p_sa.assign(c->B, 0.f); c->target.assign(c->B, 0.f);
  c->qn_out.assign((size_t)c->B * kA, 0.f); c->dq_out.assign((size_t)c->B * kA, 0.f);
  *out = c;
  return DDQ_OK;
}

int ddq_destroy(ddq_ctx* c) {
  delete c;
  return DDQ_OK;
}

int ddq_set_stream(ddq_ctx* c, void* s) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  return s ? cpu_only(c, "ddq_set_stream") : DDQ_OK;
}

int ddq_get_stream(const ddq_ctx* c, void** s) {
  if (!c || !s) return fail(nullptr, DDQ_EINVAL, "null argument");
  *s = nullptr;   // no stream: every call completes before it returns
  return DDQ_OK;
}

int ddq_synchronize(ddq_ctx* c) { return c ? DDQ_OK : fail(nullptr, DDQ_EINVAL, "null ctx"); }

int ddq_inject_fault(ddq_ctx* c, int32_t fault) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  return fault == DDQ_FAULT_NONE ? DDQ_OK
                                 : fail(c, DDQ_ESTATE, "no small-map step on this ctx (CPU mode)");
}

int ddq_small_path(const ddq_ctx* c, char* why, int32_t cap) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (why && cap > 0) snprintf(why, (size_t)cap, "%s", "CPU mode");
  return 0;
}

int64_t ddq_num_params(const ddq_ctx* c) { return c ? c->L.total : -1; }

int ddq_param_layout(const ddq_ctx* c, ddq_blob_desc* out, int32_t cap, int32_t* n) {
  if (!c || !n) return fail(nullptr, DDQ_EINVAL, "null argument");
  const char* names[5] = {"Qconv1", "Qconv2", "Qconv3", "Qfc4", "Q_out"};
  *n = 10;
  if (!out) return DDQ_OK;
  if (cap < 10) return fail(const_cast<ddq_ctx*>(c), DDQ_EINVAL, "layout needs 10 entries");
  const int s4 = c->S / 8;
  for (int l = 0; l < 5; ++l)
    for (int i = 0; i < 2; ++i) {
      ddq_blob_desc& d = out[2 * l + i];
      memset(&d, 0, sizeof(d));
      snprintf(d.name, sizeof(d.name), "%s", names[l]);
      d.index = i;
      if (i == 0) {
        if (l < 3) {
          d.shape[0] = kConv[l].cout; d.shape[1] = kConv[l].cin;
          d.shape[2] = d.shape[3] = kConv[l].k;
        } else {
          d.shape[0] = d.shape[1] = 1;
          d.shape[2] = l == 3 ? kH4 : kA;
          d.shape[3] = l == 3 ? 64 * s4 * s4 : kH4;
        }
        d.offset = c->L.w[l]; d.count = c->L.wn[l];
      } else {
        d.shape[0] = d.shape[1] = d.shape[2] = 1;
        d.shape[3] = (int)c->L.bn[l];
        d.offset = c->L.b[l]; d.count = c->L.bn[l];
      }
    }
  return DDQ_OK;
}

int ddq_set_params(ddq_ctx* c, int32_t which, const float* src, int64_t n, int32_t on_dev) {
  if (!c || !src) return fail(c, DDQ_EINVAL, "null argument");
  if (on_dev) return cpu_only(c, "device pointers");
  if (which != 0 && which != 1) return fail(c, DDQ_EINVAL, "which must be 0 (Q) or 1 (P)");
  if (n != c->L.total)
    return fail(c, DDQ_EINVAL, "expected %lld params, got %lld", (long long)c->L.total, (long long)n);
  std::copy(src, src + n, c->theta[which].begin());
  return DDQ_OK;
}

int ddq_get_params(ddq_ctx* c, int32_t which, float* dst, int64_t n, int32_t on_dev) {
  if (!c || !dst) return fail(c, DDQ_EINVAL, "null argument");
  if (on_dev) return cpu_only(c, "device pointers");
  if (which != 0 && which != 1) return fail(c, DDQ_EINVAL, "which must be 0 (Q) or 1 (P)");
  if (n != c->L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  std::copy(c->theta[which].begin(), c->theta[which].end(), dst);
  return DDQ_OK;
}

int ddq_get_grads(ddq_ctx* c, float* dst, int64_t n, int32_t on_dev) {
  if (!c || !dst) return fail(c, DDQ_EINVAL, "null argument");
  if (on_dev) return cpu_only(c, "device pointers");
  if (n != c->L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  std::copy(c->grad.begin(), c->grad.end(), dst);
  return DDQ_OK;
}

int ddq_set_grads(ddq_ctx* c, const float* src, int64_t n, int32_t on_dev) {
  if (!c || !src) return fail(c, DDQ_EINVAL, "null argument");
  if (on_dev) return cpu_only(c, "device pointers");
  if (n != c->L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  std::copy(src, src + n, c->grad.begin());
  return DDQ_OK;
}

int ddq_sync_target(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  c->theta[1] = c->theta[0];
  return DDQ_OK;
}

// ---- soft target updates ----
int ddq_set_target_tau(ddq_ctx* c, float tau) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!(tau > 0.f && tau <= 1.f))
    return fail(c, DDQ_EINVAL, "target tau must be in (0, 1] (got %g)", (double)tau);
  c->target_tau = tau;
  return DDQ_OK;
}

int ddq_get_target_tau(const ddq_ctx* c, float* tau) {
  if (!c || !tau) return fail(nullptr, DDQ_EINVAL, "null argument");
  *tau = c->target_tau;
  return DDQ_OK;
}

// P' = P + tau (Q - P): the device's target_blend, three fp32 operations each
// rounded on its own (this file is built with -ffp-contract=off, as the
// update rules need)
int ddq_soft_sync_target(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->target_tau >= 1.f) return ddq_sync_target(c);
  const float tau = c->target_tau;
  const float* q = c->theta[0].data();
  float* p = c->theta[1].data();
  for (int64_t i = 0; i < c->L.total; ++i) {
    const float d = q[i] - p[i];
    const float s = tau * d;
    p[i] = p[i] + s;
  }
  return DDQ_OK;
}

// ---- replay (replay.py) ----
int ddq_replay_create(ddq_ctx* c, int64_t capacity) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (capacity < 2 || capacity > (int64_t)INT32_MAX)
    return fail(c, DDQ_EINVAL, "capacity must be in [2, 2^31) (got %lld)", (long long)capacity);
  if (c->capacity) return fail(c, DDQ_ESTATE, "replay already created");
  c->r_state.assign((size_t)capacity * kC * c->S * c->S, 0);
  c->r_action.assign(capacity, 0);
  c->r_reward.assign(capacity, 0);
  c->r_nonterm.assign(capacity, 0);
  c->capacity = capacity;
  c->head = c->valid = 0;
  c->lanes = 1;
  c->lane_len = capacity;
  c->nstep = 1;
  c->prio_on = false;
  c->prio_cfg = ddq_priority_cfg{0, 0.f, 0.f, 0.f};
  return DDQ_OK;
}

int ddq_replay_set_lanes(ddq_ctx* c, int32_t lanes) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->capacity) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->valid != 0)
    return fail(c, DDQ_ESTATE, "set_lanes needs an empty ring (valid = %lld)", (long long)c->valid);
  if (lanes < 1 || c->capacity % lanes != 0 || c->capacity / lanes < 2)
    return fail(c, DDQ_EINVAL, "lanes must divide capacity %lld into lanes of >= 2 slots (got %d)",
                (long long)c->capacity, lanes);
  if (c->capacity / lanes <= c->nstep)
    return fail(c, DDQ_EINVAL, "%d lanes of %lld slots cannot hold the ring's %d-step windows",
                lanes, (long long)(c->capacity / lanes), c->nstep);
  if (lanes == c->lanes) return DDQ_OK;
  c->lanes = lanes;
  c->lane_len = c->capacity / lanes;
  c->head = 0;
  c->p_env.games.clear();            // a pool or an actor belongs to the lanes it was
  c->a_env.games.clear();            // created on
  prio_rebuild(c);
  return DDQ_OK;
}

int ddq_replay_lanes(const ddq_ctx* c, int32_t* lanes, int64_t* lane_len) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->capacity) return fail(const_cast<ddq_ctx*>(c), DDQ_ESTATE, "no replay buffer");
  if (lanes) *lanes = c->lanes;
  if (lane_len) *lane_len = c->lane_len;
  return DDQ_OK;
}

int ddq_replay_set_nstep(ddq_ctx* c, int32_t n) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->capacity) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (n < 1 || n > DDQ_NSTEP_MAX || n >= c->lane_len)
    return fail(c, DDQ_EINVAL, "n-step length must be in [1, %d] and below lane_len %lld (got %d)",
                DDQ_NSTEP_MAX, (long long)c->lane_len, n);
  c->nstep = n;
  prio_rebuild(c);
  return DDQ_OK;
}

static bool unit_interval(float x) { return std::isfinite(x) && x >= 0.f && x <= 1.f; }

int ddq_replay_set_priority(ddq_ctx* c, const ddq_priority_cfg* p) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!p) return fail(c, DDQ_EINVAL, "null priority cfg");
  if (!c->capacity) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (!p->enabled) {
    c->prio_on = false;
    c->prio_cfg = ddq_priority_cfg{0, 0.f, 0.f, 0.f};
    c->prio_q.clear();
    return DDQ_OK;
  }
  if (!unit_interval(p->alpha)) return fail(c, DDQ_EINVAL, "alpha must be in [0, 1] (got %g)", (double)p->alpha);
  if (!unit_interval(p->beta)) return fail(c, DDQ_EINVAL, "beta must be in [0, 1] (got %g)", (double)p->beta);
  if (!(std::isfinite(p->eps) && p->eps > 0.f))
    return fail(c, DDQ_EINVAL, "eps must be finite and > 0 (got %g)", (double)p->eps);
  if (c->B > 256)
    return fail(c, DDQ_EINVAL, "prioritized replay draws B <= 256 in one workgroup (B = %d)", c->B);
  const bool was = c->prio_on;
  c->prio_cfg = ddq_priority_cfg{1, p->alpha, p->beta, p->eps};
  if (was) return DDQ_OK;            // the annealing path: the scalars only
  c->prio_on = true;
  c->isw.assign(c->B, 1.0f);
  prio_rebuild(c);
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
  if (leaves) std::copy(c->prio_q.begin(), c->prio_q.end(), leaves);
  if (total) {
    uint64_t T = 0;
    for (uint32_t v : c->prio_q) T += v;
    *total = T;
  }
  if (pmax) *pmax = c->prio_pmax;
  return DDQ_OK;
}

int ddq_replay_set_priorities(ddq_ctx* c, const int32_t* idx, const uint32_t* q, int32_t n) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->prio_on) return fail(c, DDQ_ESTATE, "prioritized replay is off");
  if (n < 0 || (n > 0 && (!idx || !q))) return fail(c, DDQ_EINVAL, "bad argument");
  for (int k = 0; k < n; ++k) {
    if (idx[k] < 0 || idx[k] >= c->capacity) return fail(c, DDQ_EINVAL, "index %d out of range", idx[k]);
    if (q[k] > kPrioMax) return fail(c, DDQ_EINVAL, "priority %u above 2^24", q[k]);
    if ((q[k] == 0) != (c->prio_q[idx[k]] == 0))
      return fail(c, DDQ_EINVAL, "slot %d: a zero leaf (unfilled or forbidden slot) stays zero and "
                                 "a nonzero leaf stays nonzero", idx[k]);
  }
  for (int k = 0; k < n; ++k) {
    c->prio_q[idx[k]] = q[k];
    c->prio_pmax = std::max(c->prio_pmax, q[k]);
  }
  return DDQ_OK;
}

int ddq_replay_update_priorities_async(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->prio_on) return fail(c, DDQ_ESTATE, "prioritized replay is off");
  if (!c->idx_bound || (int)c->q_sa.size() != c->B)
    return fail(c, DDQ_ESTATE, "no device-side index set is bound (the minibatch was not drawn from "
                               "the ring, or no pass has run on it)");
  prio_commit(c);
  return DDQ_OK;
}

int ddq_replay_nstep(const ddq_ctx* c, int32_t* n) {
  if (!c || !n) return fail(nullptr, DDQ_EINVAL, "null argument");
  if (!c->capacity) return fail(const_cast<ddq_ctx*>(c), DDQ_ESTATE, "no replay buffer");
  *n = c->nstep;
  return DDQ_OK;
}

int ddq_replay_add(ddq_ctx* c, int32_t action, int32_t reward, const uint8_t* state) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->capacity) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->lanes > 1) return fail(c, DDQ_ESTATE, "ddq_replay_add on a laned ring (%d lanes)", c->lanes);
  if (action < 0 || action > 255) return fail(c, DDQ_EINVAL, "action must fit uint8");
  if (reward < -32768 || reward > 32767) return fail(c, DDQ_EINVAL, "reward must fit int16");
  if (not_restoring(c) != DDQ_OK) return DDQ_ESTATE;
  const size_t slot = (size_t)kC * c->S * c->S;
  const int64_t h = c->head;
  c->r_action[h] = (uint8_t)action;
  c->r_reward[h] = (int16_t)reward;
  c->r_nonterm[h] = state ? 1 : 0;   // a terminal transition keeps the slot's old frames
  if (state) std::copy(state, state + slot, c->r_state.begin() + h * slot);
  c->head = (c->head + 1) % c->capacity;
  c->valid = std::min(c->capacity, c->valid + 1);
  prio_on_add(c, 0, h);
  return DDQ_OK;
}

int ddq_replay_info(const ddq_ctx* c, int64_t* head, int64_t* valid, int64_t* capacity) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (head) *head = c->head;
  if (valid) *valid = c->valid;
  if (capacity) *capacity = c->capacity;
  return DDQ_OK;
}

int ddq_replay_import(ddq_ctx* c, const uint8_t* state, const uint8_t* action,
                      const int16_t* reward, const uint8_t* nonterm, int64_t n, int64_t head,
                      int64_t valid) {
  if (!c || !state || !action || !reward || !nonterm) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->capacity) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (n != c->capacity)
    return fail(c, DDQ_EINVAL, "import size %lld != capacity %lld", (long long)n,
                (long long)c->capacity);
  if (head < 0 || head >= c->lane_len || valid < 0 || valid > c->lane_len)
    return fail(c, DDQ_EINVAL, "head/valid out of range");
  const size_t slot = (size_t)kC * c->S * c->S;
  std::copy(state, state + slot * n, c->r_state.begin());
  std::copy(action, action + n, c->r_action.begin());
  std::copy(reward, reward + n, c->r_reward.begin());
  std::copy(nonterm, nonterm + n, c->r_nonterm.begin());
  c->head = head;
  c->valid = valid;
  prio_rebuild(c);
  return DDQ_OK;
}

int ddq_replay_export(ddq_ctx* c, uint8_t* state, uint8_t* action, int16_t* reward,
                      uint8_t* nonterm, int64_t n) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->capacity) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (n != c->capacity) return fail(c, DDQ_EINVAL, "export size mismatch");
  if (state) std::copy(c->r_state.begin(), c->r_state.end(), state);
  if (action) std::copy(c->r_action.begin(), c->r_action.end(), action);
  if (reward) std::copy(c->r_reward.begin(), c->r_reward.end(), reward);
  if (nonterm) std::copy(c->r_nonterm.begin(), c->r_nonterm.end(), nonterm);
  return DDQ_OK;
}

int ddq_replay_sample(ddq_ctx* c, const int32_t* idx, int32_t batch) {
  if (!c || !idx) return fail(c, DDQ_EINVAL, "null argument");
  if (!c->capacity) return fail(c, DDQ_ESTATE, "no replay buffer");
  if (not_restoring(c) != DDQ_OK) return DDQ_ESTATE;
  if (batch > c->lanes * allowed_slots(c))   // B < valid on a plain ring at n = 1
    return fail(c, DDQ_EINVAL, "Can't draw sample of size %d from replay dataset of size %lld",
                batch, (long long)(c->lanes * c->valid));
  if (batch != c->B) return fail(c, DDQ_EINVAL, "sample size %d != net batch %d", batch, c->B);
  for (int i = 0; i < batch; ++i) {
    if (idx[i] < 0 || idx[i] >= c->capacity || idx[i] % c->lane_len >= c->valid)
      return fail(c, DDQ_EINVAL, "index %d out of [0,valid)", idx[i]);
    if (c->nstep >= 2 && slot_forbidden(c, idx[i] % c->lane_len))
      return fail(c, DDQ_EINVAL, "index %d: its %d-step window reaches the write head", idx[i],
                  c->nstep);
    if (i && idx[i] <= idx[i - 1]) return fail(c, DDQ_EINVAL, "indices must be sorted and distinct");
  }
  for (int i = 0; i < batch; ++i) {
    const int64_t j = idx[i] + 1, nxt = j % c->lane_len == 0 ? j - c->lane_len : j;
    if (c->r_action[nxt] >= kA)
      return fail(c, DDQ_ERANGE, "stored action index out of range for %d actions", kA);
  }
  std::copy(idx, idx + batch, c->idx.begin());
  gather(c);
  if (c->prio_on) c->isw.assign(c->B, 1.0f);   // host-given set
  c->idx_bound = true;
  return DDQ_OK;
}

// (the uniform device index stream is the HIP library's; the prioritized draw
// is defined on integers and restated here)
int ddq_replay_sample_device_async(ddq_ctx* c, uint64_t seed) {
  if (!c || !c->prio_on)
    return cpu_only(c, "ddq_replay_sample_device_async (device index stream)");
  if (not_restoring(c) != DDQ_OK) return DDQ_ESTATE;
  if (c->B > c->lanes * allowed_slots(c))
    return fail(c, DDQ_EINVAL, "Can't draw sample of size %d from replay dataset of size %lld",
                c->B, (long long)(c->lanes * c->valid));
  prio_draw(c, seed, c->prio_ctr++);
  for (int b = 0; b < c->B; ++b) {
    const int64_t j = (int64_t)c->idx[b] + 1, nxt = j % c->lane_len == 0 ? j - c->lane_len : j;
    if (c->r_action[nxt] >= kA)
      return fail(c, DDQ_ERANGE, "stored action index out of range for %d actions", kA);
  }
  gather(c);
  c->idx_bound = true;
  return DDQ_OK;
}

int ddq_read_minibatch(ddq_ctx* c, float* state, float* action, float* reward, float* next_state,
                       float* nonterm) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (state) std::copy(c->state.begin(), c->state.end(), state);
  if (next_state) std::copy(c->next_state.begin(), c->next_state.end(), next_state);
  if (action) std::copy(c->action.begin(), c->action.end(), action);
  if (reward) std::copy(c->reward.begin(), c->reward.end(), reward);
  if (nonterm) std::copy(c->nonterm.begin(), c->nonterm.end(), nonterm);
  return DDQ_OK;
}

int ddq_write_minibatch(ddq_ctx* c, const float* state, const float* action, const float* reward,
                        const float* next_state, const float* nonterm) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (state) std::copy(state, state + c->state.size(), c->state.begin());
  if (next_state) std::copy(next_state, next_state + c->next_state.size(), c->next_state.begin());
  if (action) std::copy(action, action + c->action.size(), c->action.begin());
  if (reward) std::copy(reward, reward + c->reward.size(), c->reward.begin());
  if (nonterm) std::copy(nonterm, nonterm + c->nonterm.size(), c->nonterm.begin());
  if (c->prio_on) c->isw.assign(c->B, 1.0f);
  c->idx_bound = false;
  return DDQ_OK;
}

int ddq_replay_fill_tiled(ddq_ctx* c, const uint8_t*, const uint8_t*, const int16_t*,
                          const uint8_t*, int64_t, int64_t, int64_t) {
  if (c && c->lanes > 1)
    return fail(c, DDQ_ESTATE, "ddq_replay_fill_tiled on a laned ring (%d lanes)", c->lanes);
  return cpu_only(c, "ddq_replay_fill_tiled");
}

int ddq_replay_sample_batch_async(ddq_ctx* c, int32_t, uint64_t, int32_t*, float*, float*, float*,
                                  float*, float*) {
  if (c && c->lanes > 1)
    return fail(c, DDQ_ESTATE, "the large-batch sampler does not read a laned ring (%d lanes)",
                c->lanes);
  return cpu_only(c, "ddq_replay_sample_batch_async");
}

int ddq_replay_gather_batch_async(ddq_ctx* c, const int32_t*, int32_t, float*, float*, float*,
                                  float*, float*) {
  if (c && c->lanes > 1)
    return fail(c, DDQ_ESTATE, "the large-batch sampler does not read a laned ring (%d lanes)",
                c->lanes);
  return cpu_only(c, "ddq_replay_gather_batch_async");
}

int ddq_replay_status(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  return c->capacity ? DDQ_OK : fail(c, DDQ_ESTATE, "no replay buffer");
}

int ddq_read_indices(ddq_ctx* c, int32_t* idx, int32_t batch) {
  if (!c || !idx || batch != c->B) return fail(c, DDQ_EINVAL, "bad argument");
  std::copy(c->idx.begin(), c->idx.end(), idx);
  return DDQ_OK;
}

int ddq_replay_draws(ddq_ctx* c, int64_t*) { return cpu_only(c, "ddq_replay_draws"); }
int ddq_index_log_enable(ddq_ctx* c, int64_t) { return cpu_only(c, "ddq_index_log_enable"); }
int ddq_index_log_read(ddq_ctx* c, int64_t, int64_t, int32_t*) {
  return cpu_only(c, "ddq_index_log_read");
}

// ---- compute ----
int ddq_forward_backward_async(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (not_restoring(c) != DDQ_OK) return DDQ_ESTATE;
  return forward_backward(c);
}

int ddq_forward_backward(ddq_ctx* c, float* loss) {
  const int rc = ddq_forward_backward_async(c);
  if (rc == DDQ_OK && loss) *loss = c->loss;
  return rc;
}

// ---- selectable objective ----
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
  c->obj = *o;
  if (o->loss != DDQ_LOSS_HUBER) c->obj.huber_delta = 0.f;
  return DDQ_OK;
}

int ddq_get_objective(const ddq_ctx* c, ddq_objective* o) {
  if (!c || !o) return fail(nullptr, DDQ_EINVAL, "null argument");
  *o = c->obj;
  return DDQ_OK;
}

int ddq_forward_q(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (not_restoring(c) != DDQ_OK) return DDQ_ESTATE;
  tower_fwd(c, 0, c->state.data(), c->B);
  c->q_out = c->tw[0].out;
  return DDQ_OK;
}

int ddq_read_blob(ddq_ctx* c, const char* name, float* dst, int64_t n) {
  if (!c || !name || !dst) return fail(c, DDQ_EINVAL, "null argument");
  struct { const char* nm; const float* p; int64_t cnt; } t[] = {
      {"Q_out", c->q_out.data(), 4ll * c->B}, {"P_out", c->p_out.data(), 4ll * c->B},
      {"Q_sa", c->q_sa.data(), c->B},         {"P_sa", c->p_sa.data(), c->B},
      {"target_Q_sa", c->target.data(), c->B}, {"loss", &c->loss, 1},
      {"Qn_out", c->qn_out.data(), 4ll * c->B}, {"Q_out.diff", c->dq_out.data(), 4ll * c->B},
      {"is_weight", c->isw.data(), c->B},       {"grad_norm", &c->gnorm, 1}};
  for (auto& e : t)
    if (strcmp(e.nm, name) == 0) {
      if (n != e.cnt) return fail(c, DDQ_EINVAL, "blob %s has %lld elements", name, (long long)e.cnt);
      if (!strcmp(name, "grad_norm") && !(c->adam_on && c->adam.max_grad_norm > 0.f))
        return fail(c, DDQ_ESTATE, "blob grad_norm exists while Adam's gradient clipping is on");
      if (!strcmp(name, "is_weight") && !c->prio_on)
        return fail(c, DDQ_ESTATE, "blob is_weight exists while prioritized replay is on");
      if (!strcmp(name, "Qn_out") && c->obj.target != DDQ_TARGET_DOUBLE)
        return fail(c, DDQ_ESTATE, "blob Qn_out exists under the double target only");
      std::copy(e.p, e.p + n, dst);
      return DDQ_OK;
    }
  return fail(c, DDQ_EINVAL, "unknown blob '%s'", name);
}

int ddq_read_pool_mask(ddq_ctx* c, int32_t layer, uint8_t* dst, int64_t n) {
  if (!c || !dst) return fail(c, DDQ_EINVAL, "null argument");
  if (layer < 1 || layer > 3) return fail(c, DDQ_EINVAL, "layer must be 1..3");
  const int C = layer == 1 ? 32 : 64, Hp = c->S >> layer;
  const int64_t cnt = (int64_t)c->B * C * Hp * Hp;
  if (n != cnt) return fail(c, DDQ_EINVAL, "mask %d has %lld elements", layer, (long long)cnt);
  const std::vector<uint8_t>& r = c->tw[0].route[layer - 1];
  if ((int64_t)r.size() != cnt) return fail(c, DDQ_ESTATE, "no forward pass yet");
  std::copy(r.begin(), r.end(), dst);
  return DDQ_OK;
}

int ddq_select_action(ddq_ctx* c, const uint8_t* states, int32_t n, int32_t* actions) {
  if (!c || !states || !actions) return fail(c, DDQ_EINVAL, "null argument");
  if (n < 1 || n > c->B) return fail(c, DDQ_EINVAL, "n must be in [1,B]");
  if (not_restoring(c) != DDQ_OK) return DDQ_ESTATE;
  const size_t e = (size_t)n * kC * c->S * c->S;
  std::vector<float> in(states, states + e);
  Tower keep = c->tw[0];            // acting does not touch the last training pass
  tower_fwd(c, 0, in.data(), n);
  for (int b = 0; b < n; ++b) {     // first maximum (the GPU's argmax)
    const float* q = c->tw[0].out.data() + (size_t)b * kA;
    int best = 0;
    for (int a = 1; a < kA; ++a)
      if (q[a] > q[best]) best = a;
    actions[b] = best;
  }
  c->tw[0] = std::move(keep);
  return DDQ_OK;
}

// ---- Snake environments (expgain.py:30-111 + gamesim/SnakeGame.py on this ctx):
// the actor, the evaluator and the actor pool on one render, one validation,
// one per-game stream and one move ----
}  // extern "C"

namespace {

uint64_t mix64(uint64_t x) {   // splitmix64
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// seed of game g's stream among a create call's games (ddq.actor.game_seed)
uint64_t game_seed(uint64_t seed, int g) { return mix64(mix64(seed) ^ (uint64_t)g); }

// A game's stream: draw k is splitmix64(seed ^ splitmix64(k)), k = draws
struct Stream {
  uint64_t seed;
  uint64_t& draws;
  uint64_t next() { return mix64(seed ^ mix64(draws++)); }
  uint64_t randrange(uint64_t n) {   // high 64 bits of r * n
    return (uint64_t)(((unsigned __int128)next() * n) >> 64);
  }
  bool coin(double eps) { return (double)(next() >> 11) * 0x1.0p-53 < eps; }   // random() < eps
};

// expgain.epsilon (expgain.py:55-60)
double actor_eps(int64_t it) {
  if (it > 50000) return 0.1;
  return 0.1 + (1.0 - 0.1) * (double)std::max<int64_t>(50000 - it, 0) / 50000.0;
}

struct Cell { int x, y; };

// SnakeGame.set_state: the body, head first; false when the codes are not 0..k-1
bool snake_body(const int8_t* b, std::vector<Cell>* body) {
  int k = 0;
  for (int i = 0; i < 100; ++i) {
    if (b[i] < -2) return false;
    k += b[i] >= 0;
  }
  body->assign(k, Cell{-1, -1});
  for (int i = 0; i < 100; ++i)
    if (b[i] >= 0) {
      if (b[i] >= k || (*body)[b[i]].x >= 0) return false;
      (*body)[b[i]] = Cell{i / 10, i % 10};
    }
  return true;
}

// a create call's zoom maps and n start boards; single: ddq_actor_create's
// one init_board
int env_check(ddq_ctx* c, const int32_t* row_map, const int32_t* col_map, const int8_t* boards,
              int n, bool single) {
  for (int i = 0; i < c->S; ++i)
    if (row_map[i] < 0 || row_map[i] >= 10 || col_map[i] < 0 || col_map[i] >= 10)
      return fail(c, DDQ_EINVAL, "zoom map entry %d outside [0,10)", i);
  for (int g = 0; g < n; ++g) {
    char who[32] = "init_board";
    if (!single) snprintf(who, sizeof(who), "init_boards[%d]", g);
    std::vector<Cell> body;
    if (!snake_body(boards + 100 * g, &body) || body.size() < 2)
      return fail(c, DDQ_EINVAL, "%s: snake cells must be the codes 0..k-1, k >= 2", who);
    if (std::abs(body[0].x - body[1].x) + std::abs(body[0].y - body[1].y) != 1)
      return fail(c, DDQ_EINVAL, "%s: head and neck are not neighbours", who);
  }
  return DDQ_OK;
}

// n fresh games on their start boards, and the maps; the seeds are the caller's
template <class G>
void env_reset(ddq_ctx::Env<G>* e, int n, const int8_t* boards, const int32_t* row_map,
               const int32_t* col_map, int S) {
  e->games.assign(n, G{});
  for (int g = 0; g < n; ++g) {
    memcpy(e->games[g].init, boards + 100 * g, 100);
    for (auto& b : e->games[g].boards) memcpy(b, e->games[g].init, 100);
  }
  e->row.assign(row_map, row_map + S);
  e->col.assign(col_map, col_map + S);
}

// the preprocessor: gray_scale, then the nearest-neighbour zoom through the
// maps; out: u8 (4,S,S)
void env_render(const int8_t boards[4][100], const std::vector<int32_t>& row,
                const std::vector<int32_t>& col, int S, uint8_t* out) {
  for (int f = 0; f < kC; ++f)
    for (int i = 0; i < S; ++i)
      for (int j = 0; j < S; ++j) {
        const int v = boards[f][row[i] * 10 + col[j]];
        out[((size_t)f * S + i) * S + j] = v == -1 ? 0 : (v == -2 ? 255 : 200);
      }
}

// every game's state (idle ones included) in one batched forward: the greedy actions
template <class G>
int env_greedy(ddq_ctx* c, const ddq_ctx::Env<G>& e, std::vector<int32_t>* greedy) {
  const int n = (int)e.games.size();
  const size_t fs = (size_t)kC * c->S * c->S;
  std::vector<uint8_t> frames(n * fs);
  for (int g = 0; g < n; ++g)
    env_render(e.games[g].boards, e.row, e.col, c->S, frames.data() + g * fs);
  greedy->resize(n);
  return ddq_select_action(c, frames.data(), n, greedy->data());
}

// SnakeGame.cpu_play on board cur: the board after the move into next (not
// when the game is over); returns the reward (-1: game over).  The new apple's
// place among the n empty cells is rng.randrange(n).
int snake_play(const int8_t* cur, int act, int8_t* next, Stream& rng) {
  std::vector<Cell> body;
  snake_body(cur, &body);
  const int hdx = body[0].x - body[1].x, hdy = body[0].y - body[1].y;
  static const int step[4][2] = {{0, 1}, {-1, 0}, {0, -1}, {1, 0}};   // w a s d
  int dx = step[act][0], dy = step[act][1];
  if (dx == -hdx && dy == -hdy) { dx = hdx; dy = hdy; }
  const Cell to{body[0].x + dx, body[0].y + dy};
  bool over = to.x < 0 || to.x >= 10 || to.y < 0 || to.y >= 10;
  for (const Cell& b : body) over = over || (b.x == to.x && b.y == to.y);
  if (over) return -1;
  const bool eat = cur[to.x * 10 + to.y] == -2;
  body.insert(body.begin(), to);
  if (!eat) body.pop_back();
  for (int i = 0; i < 100; ++i) next[i] = cur[i] == -2 ? -2 : -1;
  for (size_t k = 0; k < body.size(); ++k) next[body[k].x * 10 + body[k].y] = (int8_t)k;
  if (eat) {   // _add_apple: empty cells x-major then y
    std::vector<int> empty;
    for (int i = 0; i < 100; ++i)
      if (next[i] == -1) empty.push_back(i);
    if (!empty.empty()) next[empty[rng.randrange(empty.size())]] = -2;
  }
  return eat ? 1 : 0;
}

// One move of a game: cpu_play on the newest board, then the next state's
// boards -- the history shifted by one, or four start boards when the episode
// ends (reset_game): a game over, or `last`, the caller's move limit reached
// with this move.  Returns the reward.
int env_move(ddq_ctx::Game& g, int act, bool last = false) {
  Stream rng{g.seed, g.draws};
  int8_t next[100];
  const int reward = snake_play(g.boards[3], act, next, rng);
  if (reward < 0 || last) {
    for (auto& b : g.boards) memcpy(b, g.init, 100);
  } else {
    memmove(g.boards[0], g.boards[1], 300);
    memcpy(g.boards[3], next, 100);
  }
  g.steps += 1;
  g.games += reward < 0;
  g.reward += reward;
  return reward;
}

}  // namespace

extern "C" {

int ddq_actor_create(ddq_ctx* c, const int8_t* init_board, const int32_t* row_map,
                     const int32_t* col_map, uint64_t seed) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!init_board || !row_map || !col_map) return fail(c, DDQ_EINVAL, "null argument");
  const int rc = env_check(c, row_map, col_map, init_board, 1, true);
  if (rc != DDQ_OK) return rc;
  if (!c->capacity) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (c->lanes > 1)
    return fail(c, DDQ_ESTATE, "ddq_actor_create on a laned ring (%d lanes): use ddq_actors_create",
                c->lanes);
  env_reset(&c->a_env, 1, init_board, row_map, col_map, c->S);
  c->a_env.games[0].seed = seed;     // the one game's stream takes the seed verbatim
  return DDQ_OK;
}

// one generate_experience (expgain.py:82-111) per step
int ddq_actor_step_async(ddq_ctx* c, int32_t nsteps, int64_t iter_num) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->a_env.games.empty()) return fail(c, DDQ_ESTATE, "no actor (call ddq_actor_create)");
  if (nsteps < 1) return fail(c, DDQ_EINVAL, "nsteps must be >= 1 (got %d)", nsteps);
  if (not_restoring(c) != DDQ_OK) return DDQ_ESTATE;
  const double eps = actor_eps(iter_num);
  ddq_ctx::Game& g = c->a_env.games[0];
  std::vector<uint8_t> frames((size_t)kC * c->S * c->S);
  for (int i = 0; i < nsteps; ++i) {
    // ExpGain.select_action: the coin first; the net is asked only when greedy
    Stream rng{g.seed, g.draws};
    int32_t act = 0;
    if (rng.coin(eps)) {
      act = (int32_t)rng.randrange(kA);
    } else {
      env_render(g.boards, c->a_env.row, c->a_env.col, c->S, frames.data());
      const int rc = ddq_select_action(c, frames.data(), 1, &act);
      if (rc != DDQ_OK) return rc;
    }
    const int reward = env_move(g, act);
    // add_experience: the next state's frames, none after a game over
    if (reward >= 0) env_render(g.boards, c->a_env.row, c->a_env.col, c->S, frames.data());
    const int rc = ddq_replay_add(c, act, reward, reward < 0 ? nullptr : frames.data());
    if (rc != DDQ_OK) return rc;
  }
  return DDQ_OK;
}

int ddq_actor_read(ddq_ctx* c, int8_t* boards, int64_t* stats) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->a_env.games.empty()) return fail(c, DDQ_ESTATE, "no actor (call ddq_actor_create)");
  const ddq_ctx::Game& g = c->a_env.games[0];
  if (boards) memcpy(boards, g.boards, 400);
  if (stats) {
    stats[0] = g.steps; stats[1] = g.games; stats[2] = g.reward;
    stats[3] = (int64_t)g.draws;
  }
  return DDQ_OK;
}

// ---- policy evaluation (evaluation.py:10-51 with per-game streams) ----
int ddq_eval_create(ddq_ctx* c, int32_t ngames, const int8_t* init_boards, const int32_t* row_map,
                    const int32_t* col_map, uint64_t seed, double epsilon, int32_t max_moves,
                    int32_t max_episodes) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!init_boards || !row_map || !col_map) return fail(c, DDQ_EINVAL, "null argument");
  if (ngames < 1 || ngames > c->B)
    return fail(c, DDQ_EINVAL, "ngames must be in [1,B] (got %d, B = %d)", ngames, c->B);
  if (!(epsilon >= 0.0 && epsilon <= 1.0))
    return fail(c, DDQ_EINVAL, "epsilon must be in [0,1] (got %g)", epsilon);
  if (max_moves < 0) return fail(c, DDQ_EINVAL, "max_moves must be >= 0 (got %d)", max_moves);
  if (max_episodes < 1)
    return fail(c, DDQ_EINVAL, "max_episodes must be >= 1 (got %d)", max_episodes);
  const int rc = env_check(c, row_map, col_map, init_boards, ngames, false);
  if (rc != DDQ_OK) return rc;
  env_reset(&c->e_env, ngames, init_boards, row_map, col_map, c->S);
  for (int g = 0; g < ngames; ++g) c->e_env.games[g].seed = game_seed(seed, g);
  c->e_eps = epsilon;
  c->e_max_moves = max_moves;
  c->e_max_ep = max_episodes;
  c->e_moves = 0;
  return DDQ_OK;
}

int ddq_eval_run_async(ddq_ctx* c, int32_t nmoves) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->e_env.games.empty()) return fail(c, DDQ_ESTATE, "no evaluator (call ddq_eval_create)");
  if (nmoves < 1) return fail(c, DDQ_EINVAL, "nmoves must be >= 1 (got %d)", nmoves);
  if (not_restoring(c) != DDQ_OK) return DDQ_ESTATE;
  std::vector<int32_t> greedy;
  for (int m = 0; m < nmoves; ++m) {
    const int rc = env_greedy(c, c->e_env, &greedy);
    if (rc != DDQ_OK) return rc;
    for (size_t g = 0; g < c->e_env.games.size(); ++g) {
      ddq_ctx::EvalGame& eg = c->e_env.games[g];
      if ((int32_t)eg.log.size() >= 4 * c->e_max_ep) continue;   // its log is full: idle
      Stream rng{eg.seed, eg.draws};
      int act = greedy[g];
      if (c->e_eps > 0.0 && rng.coin(c->e_eps)) act = (int)rng.randrange(kA);   // greedy: no coin
      eg.moves += 1;
      const bool last = c->e_max_moves > 0 && eg.moves >= c->e_max_moves;
      const int reward = env_move(eg, act, last);
      eg.score += reward;
      if (reward < 0 || last) {      // game over wins over max_moves on the same move
        eg.log.insert(eg.log.end(), {eg.move, eg.score, eg.moves, reward < 0 ? 0 : 1});
        eg.score = eg.moves = 0;
      }
      eg.move += 1;
    }
  }
  c->e_moves += nmoves;
  return DDQ_OK;
}

int ddq_eval_read(ddq_ctx* c, int64_t* stats, int32_t* episodes, int32_t* log, int8_t* boards,
                  uint64_t* draws) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->e_env.games.empty()) return fail(c, DDQ_ESTATE, "no evaluator (call ddq_eval_create)");
  int64_t eps = 0, rew = 0, dr = 0;
  const size_t per = 4 * (size_t)c->e_max_ep;
  for (size_t g = 0; g < c->e_env.games.size(); ++g) {
    const ddq_ctx::EvalGame& eg = c->e_env.games[g];
    eps += (int64_t)eg.log.size() / 4;
    rew += eg.reward;
    dr += (int64_t)eg.draws;
    if (episodes) episodes[g] = (int32_t)(eg.log.size() / 4);
    if (log) {
      std::fill(log + g * per, log + (g + 1) * per, 0);
      std::copy(eg.log.begin(), eg.log.end(), log + g * per);
    }
    if (boards) memcpy(boards + 400 * g, eg.boards, 400);
    if (draws) draws[g] = eg.draws;
  }
  if (stats) { stats[0] = c->e_moves; stats[1] = eps; stats[2] = rew; stats[3] = dr; }
  return DDQ_OK;
}

// ---- actor pool: ngames lock-step actors, game g adding into ring lane g ----
int ddq_actors_create(ddq_ctx* c, int32_t ngames, const int8_t* init_boards,
                      const int32_t* row_map, const int32_t* col_map, uint64_t seed) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!init_boards || !row_map || !col_map) return fail(c, DDQ_EINVAL, "null argument");
  if (ngames < 1 || ngames > c->B)
    return fail(c, DDQ_EINVAL, "ngames must be in [1,B] (got %d, B = %d)", ngames, c->B);
  const int rc = env_check(c, row_map, col_map, init_boards, ngames, false);
  if (rc != DDQ_OK) return rc;
  if (!c->capacity) return fail(c, DDQ_ESTATE, "no replay buffer (call ddq_replay_create)");
  if (ngames != c->lanes)
    return fail(c, DDQ_EINVAL, "ngames %d != the ring's %d lanes (ddq_replay_set_lanes)", ngames,
                c->lanes);
  env_reset(&c->p_env, ngames, init_boards, row_map, col_map, c->S);
  for (int g = 0; g < ngames; ++g) c->p_env.games[g].seed = game_seed(seed, g);
  c->p_h0 = c->head;
  c->p_v0 = c->valid;
  c->p_moves = 0;
  return DDQ_OK;
}

int ddq_actors_step_async(ddq_ctx* c, int32_t nmoves, int64_t iter_num) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->p_env.games.empty()) return fail(c, DDQ_ESTATE, "no actor pool (call ddq_actors_create)");
  if (nmoves < 1) return fail(c, DDQ_EINVAL, "nmoves must be >= 1 (got %d)", nmoves);
  if (not_restoring(c) != DDQ_OK) return DDQ_ESTATE;
  const double eps = actor_eps(iter_num);
  const int n = (int)c->p_env.games.size();
  const size_t fs = (size_t)kC * c->S * c->S;
  std::vector<int32_t> greedy;
  for (int m = 0; m < nmoves; ++m) {
    const int rc = env_greedy(c, c->p_env, &greedy);
    if (rc != DDQ_OK) return rc;
    const int64_t h = c->head;
    for (int g = 0; g < n; ++g) {
      ddq_ctx::Game& pg = c->p_env.games[g];
      Stream rng{pg.seed, pg.draws};
      int act = greedy[g];
      if (rng.coin(eps)) act = (int)rng.randrange(kA);   // always a coin
      const int reward = env_move(pg, act);
      // add_experience into lane g's slot h; after a game over the slot keeps
      // its old frames
      const int64_t slot = (int64_t)g * c->lane_len + h;
      c->r_action[slot] = (uint8_t)act;
      c->r_reward[slot] = (int16_t)reward;
      c->r_nonterm[slot] = reward < 0 ? 0 : 1;
      if (reward >= 0)
        env_render(pg.boards, c->p_env.row, c->p_env.col, c->S,
                   c->r_state.data() + (size_t)slot * fs);
    }
    c->head = (h + 1) % c->lane_len;
    c->valid = std::min(c->lane_len, c->valid + 1);
    for (int g = 0; g < n; ++g) prio_on_add(c, (int64_t)g * c->lane_len, h);
    c->p_moves++;
  }
  return DDQ_OK;
}

int ddq_actors_read(ddq_ctx* c, int8_t* boards, int64_t* stats, int64_t* totals) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->p_env.games.empty()) return fail(c, DDQ_ESTATE, "no actor pool (call ddq_actors_create)");
  int64_t tot[4] = {0, 0, 0, 0};
  for (size_t g = 0; g < c->p_env.games.size(); ++g) {
    const ddq_ctx::Game& pg = c->p_env.games[g];
    const int64_t st[4] = {pg.steps, pg.games, pg.reward, (int64_t)pg.draws};
    for (int k = 0; k < 4; ++k) {
      tot[k] += st[k];
      if (stats) stats[4 * g + k] = st[k];
    }
    if (boards) memcpy(boards + 400 * g, pg.boards, 400);
  }
  if (totals) memcpy(totals, tot, sizeof(tot));
  return DDQ_OK;
}

// ---- Adam with global-norm clipping (include/ddq_hip.h; csrc/adam.h on the device) ----
// (-ffp-contract=off: every operation rounds on its own, as the kernel's)
static int adam_apply(ddq_ctx* c, float lr) {
  const ddq_adam_cfg& a = c->adam;
  const int64_t n = c->L.total;
  c->iter++;                     // the bookkeeping first: t counts this update
  const double t = (double)c->iter;
  const float omb1 = (float)(1.0 - (double)a.beta1), omb2 = (float)(1.0 - (double)a.beta2);
  const float c1 = (float)(1.0 - std::pow((double)a.beta1, t));
  const float c2 = (float)(1.0 - std::pow((double)a.beta2, t));
  const bool clip = a.max_grad_norm > 0.f;
  float s = 1.0f;
  if (clip) {
    double tot = 0.0;
    for (int64_t i = 0; i < n; ++i) tot += (double)c->grad[i] * (double)c->grad[i];
    const float nrm = (float)std::sqrt(tot);
    s = nrm > a.max_grad_norm ? a.max_grad_norm / nrm : 1.0f;
    c->gnorm = nrm;
  }
  float* th = c->theta[0].data();
  float* m = c->opt.data();
  float* v = c->opt2.data();
  if (c->first) {                // first apply after a reset: m = v = 0
    std::fill(c->opt.begin(), c->opt.end(), 0.f);
    std::fill(c->opt2.begin(), c->opt2.end(), 0.f);
  }
  for (int64_t i = 0; i < n; ++i) {
    const float g = clip ? s * c->grad[i] : c->grad[i];
    m[i] = a.beta1 * m[i] + omb1 * g;
    v[i] = a.beta2 * v[i] + omb2 * (g * g);
    th[i] = th[i] - (lr * (m[i] / c1)) / (sqrtf(v[i] / c2) + a.eps);
  }
  c->first = 0;
  return DDQ_OK;
}

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
  if (!c->adam_on) c->opt2.assign(c->opt.size(), 0.f);
  c->adam_on = true;
  c->adam = *a;
  return DDQ_OK;
}

int ddq_get_adam(const ddq_ctx* c, ddq_adam_cfg* a) {
  if (!c || !a) return fail(nullptr, DDQ_EINVAL, "null argument");
  if (!c->adam_on) return fail(nullptr, DDQ_ESTATE, "ddq_get_adam before ddq_set_adam");
  *a = c->adam;
  return DDQ_OK;
}

int ddq_adam_state(ddq_ctx* c, float* m, float* v, int64_t n, int64_t* t) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->adam_on) return fail(c, DDQ_ESTATE, "ddq_adam_state before ddq_set_adam");
  if ((m || v) && n != c->L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  if (m) std::copy(c->opt.begin(), c->opt.begin() + n, m);
  if (v) std::copy(c->opt2.begin(), c->opt2.begin() + n, v);
  if (t) *t = c->iter;
  return DDQ_OK;
}

// ---- apply (server.py:49-124) ----
int ddq_apply_async(ddq_ctx* c, const ddq_update_cfg* u) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!u) return fail(c, DDQ_EINVAL, "null update cfg");
  if (u->rule < 0 || u->rule > DDQ_RULE_ADAM)
    return fail(c, DDQ_EINVAL, "unknown update rule %d", u->rule);
  if (not_restoring(c) != DDQ_OK) return DDQ_ESTATE;
  if (u->rule == DDQ_RULE_ADAM) {
    if (!c->adam_on) return fail(c, DDQ_ESTATE, "DDQ_RULE_ADAM before ddq_set_adam");
    return adam_apply(c, u->lr);
  }
  const Layout& L = c->L;
  const bool first = c->first != 0;
  float* th = c->theta[0].data();
  for (int l = 0; l < 5; ++l)
    for (int bias = 0; bias < 2; ++bias) {
      const int64_t o = bias ? L.b[l] : L.w[l], cnt = bias ? L.bn[l] : L.wn[l];
      for (int64_t i = o; i < o + cnt; ++i) {
        float st = c->opt[i];
        th[i] = apply_rule(*u, first, bias != 0, th[i], c->grad[i], st);
        if (u->rule != DDQ_RULE_SGD) c->opt[i] = st;
      }
    }
  c->first = 0;
  c->iter++;
  return DDQ_OK;
}

int ddq_apply(ddq_ctx* c, const ddq_update_cfg* u) { return ddq_apply_async(c, u); }

int ddq_reset_optimizer(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  std::fill(c->opt.begin(), c->opt.end(), 0.f);
  std::fill(c->opt2.begin(), c->opt2.end(), 0.f);
  c->first = 1;
  c->iter = 0;
  c->steps = 0;
  return DDQ_OK;
}

int ddq_get_optimizer_state(ddq_ctx* c, float* dst, int64_t n) {
  if (!c || !dst) return fail(c, DDQ_EINVAL, "null argument");
  if (n != c->L.total) return fail(c, DDQ_EINVAL, "size mismatch");
  std::copy(c->opt.begin(), c->opt.end(), dst);
  return DDQ_OK;
}

// ---- training monitor (netutils.py:72-96 NetLogger quantities) ----
// period > 0 is accepted and has no effect here: the twin refuses step calls.
int ddq_monitor_enable(ddq_ctx* c, int64_t capacity, int32_t period) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (capacity < 0 || capacity > (1ll << 24))
    return fail(c, DDQ_EINVAL, "capacity must be in [0, 2^24] (got %lld)", (long long)capacity);
  if (period < 0) return fail(c, DDQ_EINVAL, "period must be >= 0 (got %d)", period);
  c->m_ring.assign((size_t)capacity, ddq_monitor_record{});
  c->m_ring.shrink_to_fit();
  c->m_total = 0;
  return DDQ_OK;
}

int ddq_monitor_record_async(ddq_ctx* c, int64_t tag) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->m_ring.empty()) return fail(c, DDQ_ESTATE, "monitor not enabled (ddq_monitor_enable)");
  ddq_monitor_record r{};
  r.iteration = c->iter;
  r.tag = tag;
  r.loss = c->loss;
  double qs = 0.0;
  for (int b = 0; b < c->B; ++b) {
    float m = 0.f;
    if ((int64_t)c->q_out.size() >= (int64_t)(b + 1) * kA) {
      const float* q = &c->q_out[(size_t)b * kA];
      m = q[0];
      for (int a = 1; a < kA; ++a)
        if (q[a] > m || std::isnan(q[a])) m = q[a];
    }
    qs += m;
  }
  r.q_max_mean = (float)(qs / c->B);
  const Layout& L = c->L;
  const std::vector<float>* src[3] = {&c->theta[0], &c->theta[1], &c->grad};
  for (int t = 0; t < 3; ++t) {
    int32_t bad = 0;
    for (int j = 0; j < 10; ++j) {
      const int l = j / 2;
      const int64_t o = (j & 1) ? L.b[l] : L.w[l], n = (j & 1) ? L.bn[l] : L.wn[l];
      const float* x = src[t]->data() + o;
      double ss = 0.0;
      for (int64_t i = 0; i < n; ++i) {
        const double v = x[i];
        ss += v * v;
        if (!std::isfinite(x[i])) ++bad;
      }
      const float rms = (float)std::sqrt(ss / (double)n);
      if (t < 2) r.param_rms[t][j] = rms;
      else r.grad_rms[j] = rms;
    }
    r.nonfinite[t] = bad;
  }
  c->m_ring[(size_t)(c->m_total % (int64_t)c->m_ring.size())] = r;
  c->m_total++;
  return DDQ_OK;
}

int ddq_monitor_read(ddq_ctx* c, int64_t first, int64_t n, ddq_monitor_record* out,
                     int64_t* total) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (c->m_ring.empty()) return fail(c, DDQ_ESTATE, "monitor not enabled (ddq_monitor_enable)");
  if (n < 0 || (n > 0 && !out)) return fail(c, DDQ_EINVAL, "bad argument");
  if (total) *total = c->m_total;
  if (n == 0) return DDQ_OK;
  const int64_t cap = (int64_t)c->m_ring.size();
  if (first < 0 || first + n > c->m_total || c->m_total - first > cap)
    return fail(c, DDQ_EINVAL, "records [%lld, %lld) not in the ring (taken %lld, capacity %lld)",
                (long long)first, (long long)(first + n), (long long)c->m_total, (long long)cap);
  for (int64_t k = 0; k < n; ++k) out[k] = c->m_ring[(size_t)((first + k) % cap)];
  return DDQ_OK;
}

// ---- what needs a GPU: RCCL, graphs, groups, async exchange, timing ----
int ddq_comm_get_unique_id(uint8_t id[128]) {
  (void)id;
  return cpu_only(nullptr, "ddq_comm_get_unique_id (RCCL)");
}
int ddq_comm_init(ddq_ctx* c, const uint8_t[128], int32_t, int32_t) {
  return cpu_only(c, "ddq_comm_init (RCCL)");
}
int ddq_allreduce_grads(ddq_ctx* c) { return cpu_only(c, "ddq_allreduce_grads (RCCL)"); }
int ddq_allreduce_grads_async(ddq_ctx* c) { return cpu_only(c, "ddq_allreduce_grads_async (RCCL)"); }
int ddq_step_async(ddq_ctx* c, const ddq_step_cfg*) {
  return cpu_only(c, "ddq_step_async (device index stream)");
}
int ddq_step_graph_async(ddq_ctx* c, const ddq_step_cfg*, int32_t) {
  return cpu_only(c, "ddq_step_graph_async (hipGraph)");
}
int ddq_step_pipelined_async(ddq_ctx* c, const ddq_step_cfg*, int32_t) {
  return cpu_only(c, "ddq_step_pipelined_async (hipGraph)");
}
int ddq_step_prepare(ddq_ctx* c, const ddq_step_cfg*, int32_t) {
  return cpu_only(c, "ddq_step_prepare (hipGraph)");
}
int ddq_group_init(ddq_ctx** ctxs, int32_t) {
  return cpu_only(ctxs ? ctxs[0] : nullptr, "ddq_group_init");
}
int ddq_group_step(ddq_ctx** ctxs, int32_t, const ddq_step_cfg*) {
  return cpu_only(ctxs ? ctxs[0] : nullptr, "ddq_group_step");
}
int64_t ddq_step_count(const ddq_ctx* c) { return c ? c->steps : -1; }
int ddq_async_begin(ddq_ctx* c, const ddq_step_cfg*) { return cpu_only(c, "ddq_async_begin"); }
int ddq_async_ready(ddq_ctx* c, int32_t*) { return cpu_only(c, "ddq_async_ready"); }
int ddq_async_tick(ddq_ctx* c, const ddq_step_cfg*, int32_t) { return cpu_only(c, "ddq_async_tick"); }
int ddq_group_async_run(ddq_ctx** ctxs, int32_t, const ddq_step_cfg*, int32_t, int32_t*) {
  return cpu_only(ctxs ? ctxs[0] : nullptr, "ddq_group_async_run");
}
int ddq_group_async_ticks(ddq_ctx** ctxs, int32_t, const ddq_step_cfg*, int32_t, const int32_t*) {
  return cpu_only(ctxs ? ctxs[0] : nullptr, "ddq_group_async_ticks");
}
int ddq_set_straggle(ddq_ctx* c, int64_t) { return cpu_only(c, "ddq_set_straggle"); }
int ddq_profile_step(ddq_ctx* c, const ddq_step_cfg*, char*, float*, int32_t, int32_t*) {
  return cpu_only(c, "ddq_profile_step");
}
int ddq_time_layer(ddq_ctx* c, const char*, int32_t, float*) { return cpu_only(c, "ddq_time_layer"); }

double ddq_step_flops(const ddq_ctx* c) {
  if (!c) return 0.0;
  const double s1 = c->S, s2 = c->S / 2, s3 = c->S / 4, s4 = c->S / 8;
  const double F = (double)c->B * (6272 * s1 * s1 + 51200 * s2 * s2 + 36864 * s3 * s3 +
                                   32768 * s4 * s4 + 2048);
  return 2.0 * (4.0 * F - (double)c->B * 6272 * s1 * s1);
}

}  // extern "C"

// ---- checkpoint and resume (include/ddq_hip.h ddq_state_*) ----
// The same sections, byte for byte, as the HIP library's: the vectors in
// place, the games in the device struct's layout (544 bytes each), the two
// fixed structs assembled here.  The digest is the plain loop of its definition.
namespace {

constexpr int kStateMax = 16;
constexpr int64_t kGameBytes = 544;   // ActorState of the HIP library

struct StateSec {
  const char* name;
  int64_t bytes;
  uint8_t* mem;     // nullptr: assembled (config, counters, actor, pool)
};

int state_table(ddq_ctx* c, StateSec* t) {
  const int64_t P4 = c->L.total * 4, cap = c->capacity;
  auto u8 = [](auto& v) { return reinterpret_cast<uint8_t*>(v.data()); };
  int n = 0;
  t[n++] = {"config", (int64_t)sizeof(ddq_state_config), nullptr};
  t[n++] = {"theta_q", P4, u8(c->theta[0])};
  t[n++] = {"theta_p", P4, u8(c->theta[1])};
  t[n++] = {"opt", P4, u8(c->opt)};
  if (c->adam_on) t[n++] = {"opt2", P4, u8(c->opt2)};
  t[n++] = {"counters", (int64_t)sizeof(ddq_state_counters), nullptr};
  if (cap) {
    t[n++] = {"ring_state", cap * kC * c->S * c->S, u8(c->r_state)};
    t[n++] = {"ring_action", cap, u8(c->r_action)};
    t[n++] = {"ring_reward", 2 * cap, u8(c->r_reward)};
    t[n++] = {"ring_nonterm", cap, u8(c->r_nonterm)};
  }
  if (c->prio_on) t[n++] = {"prio_leaf", 4 * cap, u8(c->prio_q)};
  if (!c->a_env.games.empty()) t[n++] = {"actor", kGameBytes, nullptr};
  if (!c->p_env.games.empty())
    t[n++] = {"pool", kGameBytes * (int64_t)c->p_env.games.size(), nullptr};
  return n;
}

ddq_state_config state_config(const ddq_ctx* c) {
  ddq_state_config k;
  memset(&k, 0, sizeof(k));
  k.batch = (int16_t)c->B;
  k.frame = (int16_t)c->S;
  memcpy(&k.gamma_bits, &c->gamma, 4);
  k.capacity = c->capacity;
  k.lanes = c->capacity ? c->lanes : 1;
  k.nstep = (uint8_t)(c->capacity ? c->nstep : 1);
  if (c->prio_on) {
    k.prio_enabled = 1;
    k.prio_alpha = c->prio_cfg.alpha; k.prio_beta = c->prio_cfg.beta; k.prio_eps = c->prio_cfg.eps;
  }
  k.obj_target = (uint8_t)c->obj.target;
  k.obj_loss = (uint8_t)c->obj.loss;
  k.huber_delta = c->obj.huber_delta;
  if (c->adam_on) {
    k.adam_on = 1;
    k.adam_beta1 = c->adam.beta1; k.adam_beta2 = c->adam.beta2;
    k.adam_eps = c->adam.eps; k.adam_max_grad_norm = c->adam.max_grad_norm;
  }
  k.actor = c->a_env.games.empty() ? 0 : 1;
  k.pool_games = (int16_t)c->p_env.games.size();
  k.target_tau = c->target_tau;
  return k;
}

const char* state_config_diff(const ddq_state_config& a, const ddq_state_config& b) {
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

ddq_state_counters state_counters_now(const ddq_ctx* c) {
  ddq_state_counters k;
  memset(&k, 0, sizeof(k));
  k.iteration = c->iter;
  k.steps = c->steps;
  k.opt_init = c->first ? 0 : 1;
  if (c->capacity) {
    k.head = c->head;
    k.valid = c->valid;
    k.draws = c->prio_ctr;
  }
  if (!c->p_env.games.empty()) {
    k.pool_h0 = c->p_h0;
    k.pool_v0 = c->p_v0;
    k.pool_moves = c->p_moves;
  }
  if (c->prio_on) k.pmax = c->prio_pmax;
  return k;
}

// a game <-> its 544 bytes: seed, draws, steps, games, reward sum, the four
// history boards, the start board, four zero bytes
void game_pack(const ddq_ctx::Game& g, uint8_t* out) {
  memset(out, 0, (size_t)kGameBytes);
  const uint64_t w[5] = {g.seed, g.draws, (uint64_t)g.steps, (uint64_t)g.games, (uint64_t)g.reward};
  memcpy(out, w, 40);
  memcpy(out + 40, g.boards, 400);
  memcpy(out + 440, g.init, 100);
}
void game_unpack(const uint8_t* in, ddq_ctx::Game* g) {
  uint64_t w[5];
  memcpy(w, in, 40);
  g->seed = w[0]; g->draws = w[1];
  g->steps = (int64_t)w[2]; g->games = (int64_t)w[3]; g->reward = (int64_t)w[4];
  memcpy(g->boards, in + 40, 400);
  memcpy(g->init, in + 440, 100);
}
std::vector<uint8_t> games_pack(const std::vector<ddq_ctx::Game>& gs) {
  std::vector<uint8_t> out(gs.size() * (size_t)kGameBytes);
  for (size_t i = 0; i < gs.size(); ++i) game_pack(gs[i], out.data() + i * kGameBytes);
  return out;
}

bool board_ok(const int8_t* b) {
  std::vector<Cell> body;
  if (!snake_body(b, &body) || body.size() < 2) return false;
  return std::abs(body[0].x - body[1].x) + std::abs(body[0].y - body[1].y) == 1;
}

// an assembled section's bytes: as written while restoring, as the ctx has them otherwise
std::vector<uint8_t> state_assembled(ddq_ctx* c, const StateSec& s) {
  std::vector<uint8_t> out((size_t)s.bytes);
  if (!strcmp(s.name, "config")) {
    const ddq_state_config k = state_config(c);
    memcpy(out.data(), &k, sizeof(k));
  } else if (!strcmp(s.name, "counters")) {
    const ddq_state_counters k = c->restoring ? c->st_ctr : state_counters_now(c);
    memcpy(out.data(), &k, sizeof(k));
  } else if (!strcmp(s.name, "actor")) {
    out = c->restoring ? c->st_actor : games_pack(c->a_env.games);
  } else {
    out = c->restoring ? c->st_pool : games_pack(c->p_env.games);
  }
  return out;
}

uint64_t state_digest_bytes(const uint8_t* p, uint64_t n) {
  uint64_t d = mix64(n);
  const uint64_t K = (n + 7) / 8;
  for (uint64_t k = 0; k < K; ++k) {
    uint64_t w = 0;
    const uint64_t have = std::min<uint64_t>(8, n - 8 * k);
    for (uint64_t b = 0; b < have; ++b) w |= (uint64_t)p[8 * k + b] << (8 * b);
    d += mix64(w ^ ((k + 1) * 0x9E3779B97F4A7C15ull));
  }
  return d;
}

uint64_t state_section_digest(ddq_ctx* c, const StateSec& s) {
  if (s.mem) return state_digest_bytes(s.mem, (uint64_t)s.bytes);
  const std::vector<uint8_t> b = state_assembled(c, s);
  return state_digest_bytes(b.data(), b.size());
}

int state_find(ddq_ctx* c, const char* name, StateSec* out) {
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

int state_range(ddq_ctx* c, const StateSec& s, int64_t offset, int64_t bytes) {
  if (offset < 0 || bytes <= 0 || offset > s.bytes || bytes > s.bytes - offset)
    return fail(c, DDQ_EINVAL, "section '%s' has %lld bytes: [%lld, %lld + %lld) is not inside it",
                s.name, (long long)s.bytes, (long long)offset, (long long)offset, (long long)bytes);
  return DDQ_OK;
}

}  // namespace

extern "C" {

int ddq_state_sections(ddq_ctx* c, ddq_state_section* out, int32_t cap, int32_t* n) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!n) return fail(c, DDQ_EINVAL, "null argument");
  StateSec t[kStateMax];
  const int k = state_table(c, t);
  *n = k;
  if (!out) return DDQ_OK;
  if (cap < k) return fail(c, DDQ_EINVAL, "the ctx has %d sections (cap = %d)", k, cap);
  for (int i = 0; i < k; ++i) {
    memset(&out[i], 0, sizeof(out[i]));
    snprintf(out[i].name, sizeof(out[i].name), "%s", t[i].name);
    out[i].bytes = t[i].bytes;
    out[i].digest = state_section_digest(c, t[i]);
  }
  return DDQ_OK;
}

int ddq_state_digest(ddq_ctx* c, const char* name, uint64_t* digest) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!digest) return fail(c, DDQ_EINVAL, "null argument");
  StateSec s{};
  int rc = state_find(c, name, &s);
  if (rc != DDQ_OK) return rc;
  *digest = state_section_digest(c, s);
  return DDQ_OK;
}

int ddq_state_read(ddq_ctx* c, const char* name, int64_t offset, void* dst, int64_t bytes) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!dst) return fail(c, DDQ_EINVAL, "null argument");
  StateSec s{};
  int rc = state_find(c, name, &s);
  if (rc == DDQ_OK) rc = state_range(c, s, offset, bytes);
  if (rc != DDQ_OK) return rc;
  if (s.mem) {
    memcpy(dst, s.mem + offset, (size_t)bytes);
    return DDQ_OK;
  }
  const std::vector<uint8_t> b = state_assembled(c, s);
  memcpy(dst, b.data() + offset, (size_t)bytes);
  return DDQ_OK;
}

int ddq_state_write(ddq_ctx* c, const char* name, int64_t offset, const void* src, int64_t bytes) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!src) return fail(c, DDQ_EINVAL, "null argument");
  StateSec s{};
  int rc = state_find(c, name, &s);
  if (rc == DDQ_OK) rc = state_range(c, s, offset, bytes);
  if (rc != DDQ_OK) return rc;
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
    c->st_ctr = state_counters_now(c);
    c->st_actor = games_pack(c->a_env.games);
    c->st_pool = games_pack(c->p_env.games);
    c->restoring = true;
  }
  uint8_t* to = s.mem;
  if (!to)
    to = !strcmp(s.name, "counters") ? reinterpret_cast<uint8_t*>(&c->st_ctr)
         : !strcmp(s.name, "actor")  ? c->st_actor.data()
                                     : c->st_pool.data();
  memcpy(to + offset, src, (size_t)bytes);
  return DDQ_OK;
}

int ddq_state_commit(ddq_ctx* c) {
  if (!c) return fail(nullptr, DDQ_EINVAL, "null ctx");
  if (!c->restoring) return DDQ_OK;
  const ddq_state_counters k = c->st_ctr;
  const bool ring = c->capacity != 0;
  const int64_t L = c->lane_len;
  if (k.iteration < 0 || k.steps < 0 || (k.opt_init != 0 && k.opt_init != 1) || k.ring_err < 0 ||
      k.ring_err > 2 || k.reserved[0] || k.reserved[1] || k.reserved[2])
    return fail(c, DDQ_EINVAL, "counters: iteration %lld, steps %lld, opt_init %d, ring_err %d or a "
                               "reserved word out of range",
                (long long)k.iteration, (long long)k.steps, k.opt_init, k.ring_err);
  if (ring ? (k.head < 0 || k.head >= L || k.valid < 0 || k.valid > L)
           : (k.head != 0 || k.valid != 0 || k.draws != 0 || k.batch_ctr != 0))
    return fail(c, DDQ_EINVAL, "counters: head %lld / valid %lld outside the ring's lane length %lld",
                (long long)k.head, (long long)k.valid, (long long)(ring ? L : 0));
  const bool pool = !c->p_env.games.empty();
  if (pool ? (k.pool_h0 < 0 || k.pool_h0 >= L || k.pool_v0 < 0 || k.pool_v0 > L ||
              k.pool_moves < 0 || k.head != (k.pool_h0 + k.pool_moves % L) % L ||
              k.valid != std::min(L, k.pool_v0 + std::min(k.pool_moves, L)))
           : (k.pool_h0 != 0 || k.pool_v0 != 0 || k.pool_moves != 0))
    return fail(c, DDQ_EINVAL, "counters: the pool's h0 %lld, v0 %lld, moves %lld do not give the "
                               "ring's head %lld / valid %lld",
                (long long)k.pool_h0, (long long)k.pool_v0, (long long)k.pool_moves,
                (long long)k.head, (long long)k.valid);
  for (int role = 0; role < 2; ++role) {
    const std::vector<uint8_t>& blob = role ? c->st_pool : c->st_actor;
    const int n = (int)(blob.size() / (size_t)kGameBytes);
    for (int g = 0; g < n; ++g) {
      ddq_ctx::Game gm;
      game_unpack(blob.data() + (size_t)g * kGameBytes, &gm);
      for (int f = 0; f < 5; ++f)
        if (!board_ok(f < 4 ? gm.boards[f] : gm.init))
          return fail(c, DDQ_EINVAL, "%s: game %d, board %d is not a Snake board", role ? "pool" : "actor",
                      g, f);
      if (gm.steps < 0 || (role && gm.steps != k.pool_moves))
        return fail(c, DDQ_EINVAL, "%s: game %d made %lld steps (the pool's moves: %lld)",
                    role ? "pool" : "actor", g, (long long)gm.steps, (long long)k.pool_moves);
    }
  }
  if (c->prio_on) {
    if (k.pmax < kPrioOne || k.pmax > kPrioMax)
      return fail(c, DDQ_EINVAL, "counters: pmax %u outside [65536, 2^24]", k.pmax);
    int64_t bad = 0, first = -1;
    for (int64_t i = 0; i < c->capacity; ++i) {
      const int64_t x = i % L;
      const bool zero = !(x < k.valid) || prio_forbidden(x, k.head, k.valid, L, c->nstep);
      if (c->prio_q[i] > kPrioMax || (c->prio_q[i] == 0) != zero) {
        if (!bad) first = i;
        ++bad;
      }
    }
    if (bad)
      return fail(c, DDQ_EINVAL, "prio_leaf: %lld leaves are above 2^24 or break \"zero <=> slot unfilled "
                                 "or forbidden\" under head %lld, valid %lld, n %d (first: slot %lld)",
                  (long long)bad, (long long)k.head, (long long)k.valid, c->nstep, (long long)first);
  } else if (k.pmax != 0) {
    return fail(c, DDQ_EINVAL, "counters: pmax %u while prioritized replay is off", k.pmax);
  }
  c->iter = k.iteration;
  c->steps = k.steps;
  c->first = k.opt_init ? 0 : 1;
  c->head = k.head;
  c->valid = k.valid;
  c->prio_ctr = k.draws;
  c->p_h0 = k.pool_h0;
  c->p_v0 = k.pool_v0;
  c->p_moves = k.pool_moves;
  if (c->prio_on) c->prio_pmax = k.pmax;
  for (size_t g = 0; g < c->a_env.games.size(); ++g)
    game_unpack(c->st_actor.data() + g * kGameBytes, &c->a_env.games[g]);
  for (size_t g = 0; g < c->p_env.games.size(); ++g)
    game_unpack(c->st_pool.data() + g * kGameBytes, &c->p_env.games[g]);
  c->idx_bound = false;
  c->restoring = false;
  return DDQ_OK;
}

}  // extern "C"
