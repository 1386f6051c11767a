"""The large-batch regime on the device: B > 256, where ddq_create still accepts
the batch (up to 1024) and the code takes other branches in a dozen places.

a. The two-launch draw (sample_kernel at 512 / 1024 threads, then gather_kernel)
   against tests/_nstep_ref.draw element for element: one over the boundary, the
   1024-thread launch with B < P2 and B == P2, a ring with exactly B allowed
   slots, a laned and a plain n = 3 ring (tests/_large_batch.DRAW_CASES).
b. Eager, graph and pipelined chains of 11 steps are one sequence, bit for bit,
   at (S, B) = (16, 264) and (24, 288): the head and the slab reduce leave the
   draw counter to sample_kernel, the pipelined chain replays eleven single-step
   graphs whose prefetch runs on the side stream.  Plain rmsprop, and n = 3 +
   Double + Huber + Adam with clipping (prioritized replay refuses B > 256).
c. One context through eager, graph and both pipelined parities, then another
   lr, against a context that only takes eager steps.
d. Eager steps teacher-forced against the float64 oracle (tests/_parity.py's
   bounds, unchanged), up to one step at B = 1024.
e. The exchanges at B = 264: a one-member group under all-reduce against plain
   steps, W = 3 groups under server / sharded / all-reduce, a W = 2 async group
   tick by tick, and a one-rank RCCL communicator under every exchange.
f. The monitor's image loop and select_action past 256 images.

tests/test_large_batch.py checks on the CPU that every draw expected here is a
legal set the restatement finds in at most 1024 rounds.
"""
import numpy as np
import pytest

import _large_batch as lb
import _monitor_ref as mr
import _nstep_ref as nr
from _parity import check_full_pass, close

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


_RING = {}


def ring_for(S, N=lb.N):
    """N slots of synthetic Snake play (bench.py's frames), terminals included."""
    if (S, N) not in _RING:
        from ddq.expgain import synthetic_transitions
        st, ac, rw, nt = synthetic_transitions(N, S, seed=77)
        assert 2 <= int((~np.asarray(nt, bool)).sum()) < N // 3
        _RING[(S, N)] = (st, ac, rw, np.asarray(nt, np.uint8))
    return _RING[(S, N)]


def theta0(S):
    from ddq.params import init_params_flat
    return init_params_flat(S, seed=42)


def make_net(ddq, S, B, ring, head, valid, lanes=1, n=None):
    net = ddq.DeepQNet(batch=B, frame=S)
    assert not net.small_path()[0]                 # B > 256: the general kernels at S = 16 too
    th = theta0(S)
    net.set_flat(0, th)
    net.set_flat(1, th)
    net.replay_create(len(ring[1]))
    if lanes > 1:
        net.replay_set_lanes(lanes)
    net.replay_import(ring[0], ring[1], ring[2], np.asarray(ring[3], np.uint8), head, valid)
    if n is not None:
        net.replay_set_nstep(n)
    return net


def done(*nets):
    for net in nets:
        net.synchronize()
        net.close()


def code_of(call):
    from ddq import _lib
    with pytest.raises(_lib.DDQError) as ei:
        call()
    return ei.value.code


# ------------------------------------------------------------------ a. the draw
@pytest.mark.parametrize("case", lb.DRAW_CASES, ids=lb.case_id)
def test_device_draw_is_the_restatement(ddq, case):
    B, cap, lanes, head, valid, n = case
    L, S = cap // lanes, 16
    ring = nr.build_ring(np.random.default_rng(cap), cap, S, [s for s in range(cap) if s % 5 == 3])
    net = make_net(ddq, S, B, ring, head, valid, lanes, n if n > 1 else None)
    net.index_log_enable(lb.DRAWS)
    assert net.replay_draws() == 0
    want = [nr.draw(lb.SEED, d, B, head, valid, lanes, L, n) for d in range(lb.DRAWS)]
    for d in range(lb.DRAWS):
        net.replay_sample_device(lb.SEED)
    net.synchronize()
    assert net.replay_draws() == lb.DRAWS
    log = net.index_log(0, lb.DRAWS)
    for d in range(lb.DRAWS):
        np.testing.assert_array_equal(log[d], want[d], "draw %d" % d)
    np.testing.assert_array_equal(net.read_indices(), want[-1])
    net._check(net.lib.ddq_replay_status(net.ctx))
    # the host gather: nr.gather is the per-lane gather (ph.lane_gather) at n = 1
    # and the windowed one on the two n = 3 rings, the laned one among them
    nr.assert_minibatch(net.read_minibatch(), nr.gather(ring, want[-1], L, n))
    if n == 1:
        import _pool_host as ph
        nr.assert_minibatch(net.read_minibatch(), ph.lane_gather(ring, want[-1], L))
    done(net)


# ------------------------------------------------------------------ b. step modes
MODE_SHAPES = [(16, 264), (24, 288)]
# rmsprop as the other suites run it at these frames (1e-4 on the small frame,
# 1e-6 on the general-kernel frames); Adam as tests/test_gpu_adam.py, whose
# general-kernel frame is 32
RMS_LR = {16: 1e-4, 24: 1e-6}
CLIP = 1e-3
_CHAINS = {}


def adam_lr(S):
    from test_gpu_adam import LR
    return LR[16] if S == 16 else LR[32]


def chain(ddq, S, B, mode, full):
    """lb.MODES_STEPS steps from the same start on a fresh ctx: eager 11 x 1,
    step_graph(11) (one 8-step exec and three singles) or step_pipelined(11)
    (eleven single-step graphs, the two minibatch sets alternating).  full: n = 3,
    Double + Huber, Adam with clipping."""
    key = (S, B, mode, full)
    if key in _CHAINS:
        return _CHAINS[key]
    T = lb.MODES_STEPS
    net = make_net(ddq, S, B, ring_for(S), lb.MODES_HEAD, lb.N, n=3 if full else None)
    if full:
        net.set_objective("double", "huber", 0.5)
        net.set_adam(max_grad_norm=CLIP)
    net.index_log_enable(32)                       # (room for a counter that ran ahead)
    cfg = net.step_cfg("adam" if full else "rmsprop", lr=adam_lr(S) if full else RMS_LR[S],
                       target_period=3, seed=lb.MODES_SEED)
    if mode == "eager":
        for _ in range(T):
            net.step(cfg)
    elif mode == "graph":
        net.step_graph(cfg, T)
    else:
        net.step_pipelined(cfg, T)
    net.synchronize()
    out = {"state": [net.get_flat(0), net.get_flat(1), net.optimizer_state()],
           "log": net.index_log(0, T), "idx": net.read_indices(), "mb": net.read_minibatch(),
           "draws": net.replay_draws(), "loss": net.blob("loss")}
    if full:
        m, v, t = net.adam_state()
        out["state"] += [m, v]
        out["t"] = t
        out["grad_norm"] = float(net.blob("grad_norm"))
    assert all(np.isfinite(s).all() for s in out["state"]) and np.isfinite(out["loss"])
    net._check(net.lib.ddq_replay_status(net.ctx))
    # prioritized replay draws B <= 256 in one workgroup: refused here
    assert code_of(lambda: net.replay_set_priority(alpha=0.6, beta=0.4, eps=0.01)) == EINVAL
    done(net)
    _CHAINS[key] = out
    return out


@pytest.mark.parametrize("full", [False, True], ids=["rmsprop", "n3-double-huber-adam"])
@pytest.mark.parametrize("S,B", MODE_SHAPES)
def test_step_modes_are_one_sequence(ddq, S, B, full):
    T, n = lb.MODES_STEPS, 3 if full else 1
    eager = chain(ddq, S, B, "eager", full)
    ring = ring_for(S)
    # one draw a step (sample_kernel advances the counter; the head and the slab
    # reduce must not), each the restatement's
    off = [d for d in range(T) if not np.array_equal(
        eager["log"][d], nr.draw(lb.MODES_SEED, d, B, lb.MODES_HEAD, lb.N, 1, lb.N, n))]
    assert (eager["draws"], off) == (T, []), "draws made, logged sets that are not the restatement's"
    np.testing.assert_array_equal(eager["idx"], eager["log"][-1])
    nr.assert_minibatch(eager["mb"], nr.gather(ring, eager["log"][-1], lb.N, n))
    assert eager["state"][0].tobytes() != theta0(S).tobytes()
    assert eager["state"][1].tobytes() != eager["state"][0].tobytes()   # P: the step-9 model
    if full:
        assert eager["t"] == T and eager["grad_norm"] > CLIP            # the last step clipped
    for mode in ("graph", "pipelined"):
        other = chain(ddq, S, B, mode, full)
        assert other["draws"] == T, mode
        assert eager["log"].tobytes() == other["log"].tobytes(), mode
        assert eager["idx"].tobytes() == other["idx"].tobytes(), mode
        for a, b in zip(eager["state"], other["state"]):
            assert a.tobytes() == b.tobytes(), mode
        for a, b in zip(eager["mb"], other["mb"]):
            assert a.tobytes() == b.tobytes(), mode
        assert eager["loss"].tobytes() == other["loss"].tobytes(), mode
        if full:
            assert other["t"] == T, mode


# ------------------------------------------------------------------ c. one context
def test_one_context_through_the_modes_matches_eager_steps(ddq):
    """Net A: eager 2, step_graph(9) (an 8-step exec and a single), step_pipelined
    of 3 and of 4 (the chain starts on set 0, then on set 1), another lr (every
    exec recaptured), step_pipelined(2).  Net B: the same 20 steps eagerly."""
    from test_gpu_step_modes import assert_same_state, eager
    S, B = 16, 264
    a, b = [make_net(ddq, S, B, ring_for(S), 0, lb.N) for _ in range(2)]
    for n in (a, b):
        n.index_log_enable(32)
    # (the second rate is the lower one: twenty lagged-rmsprop steps stay finite)
    cfg1 = a.step_cfg("rmsprop", lr=1e-4, target_period=3, seed=lb.SWITCH_SEED)
    cfg2 = a.step_cfg("rmsprop", lr=5e-5, target_period=3, seed=lb.SWITCH_SEED)
    eager(a, cfg1, 2)
    a.step_graph(cfg1, 9)
    a.step_pipelined(cfg1, 3)
    a.step_pipelined(cfg1, 4)
    a.step_pipelined(cfg2, 2)
    eager(b, cfg1, 18)
    eager(b, cfg2, 2)
    assert_same_state(a, b, 0, lb.SWITCH_STEPS)
    for x, y in zip(a.read_minibatch(), b.read_minibatch()):
        assert x.tobytes() == y.tobytes()
    assert a.get_flat(0).tobytes() != theta0(S).tobytes()
    done(a, b)


# ------------------------------------------------------------------ d. the oracle
@pytest.mark.parametrize("S,B,N,rule,lr,steps", lb.TEACHER_CASES,
                         ids=["%d-%d-%s" % (c[0], c[1], c[3]) for c in lb.TEACHER_CASES])
def test_eager_steps_teacher_forced(ddq, ref, S, B, N, rule, lr, steps):
    """Every eager step, started from the GPU's own state, against the oracle's
    step on the logged minibatch: blobs and all ten gradient tensors under the
    three rules of tests/_parity.py, theta_Q and the cache after the oracle's
    update rule, theta_P exactly (P <- Q every 3)."""
    from test_gpu_chain import oracle_rule
    period = 3
    ring = ring_for(S, N)
    net = make_net(ddq, S, B, ring, 0, N)
    net.index_log_enable(8)
    cfg = net.step_cfg(rule, lr=lr, target_period=period, seed=lb.TEACHER_SEED)
    r = ref.ReplayRef((4, S, S), N)
    r.state, r.action, r.reward, r.non_terminal = ring[0], ring[1], ring[2], ring[3].astype(bool)
    r.head, r.valid = 0, N
    thq, thp = theta0(S), theta0(S)
    state, ties = None, 0
    for t in range(steps):
        net.step(cfg)
        net.synchronize()
        idx = net.read_indices()
        np.testing.assert_array_equal(idx, nr.draw(lb.TEACHER_SEED, t, B, 0, N, 1, N, 1))
        p_pull = thq if t % period == 0 else thp              # the pull's P <- Q
        mb = r.gather(idx)
        nr.assert_minibatch(net.read_minibatch(), mb, "step %d" % t)
        _, grads, n = check_full_pass(ref, net, ref.unflatten(thq, S, "Q"),
                                      ref.unflatten(p_pull, S, "P"), mb, what="step %d " % t,
                                      quiet=t not in (0, steps - 1))
        ties += n
        g = ref.flatten(grads).astype(np.float32)
        th_ref, st_ref = oracle_rule(ref, rule, thq, g, state, lr)
        gq, gp = net.get_flat(0), net.get_flat(1)
        close(gq, th_ref, what="step %d theta_Q" % t, quiet=t not in (0, steps - 1))
        np.testing.assert_array_equal(gp, gq if (t + 1) % period == 0 else p_pull)
        if rule != "sgd":
            gst = net.optimizer_state()
            close(gst, st_ref, what="step %d cache" % t, quiet=t not in (0, steps - 1))
            state = gst
        thq, thp = gq, gp
    assert net.replay_draws() == steps and not np.array_equal(thq, theta0(S))
    np.testing.assert_array_equal(net.index_log(0, steps)[-1], idx)
    print("%dx%d B=%d %s: %d teacher-forced steps, %d near-tie routings adopted"
          % (S, S, B, rule, steps, ties))
    done(net)


# ------------------------------------------------------------------ e. exchanges
EB, EN = lb.EXCHANGE_B, lb.N


def moved_and_finite(theta, out):
    assert np.isfinite(out).all() and not np.array_equal(out, theta)


def test_one_member_allreduce_group_equals_plain_steps(ddq, ref):
    """The group step's null bump and its separate apply launch against eager +
    pipelined + graph plain steps (which take the separate apply too above 256)."""
    from test_gpu_parity import fused_vs_separate_apply
    assert np.isfinite(fused_vs_separate_apply(ddq, ref, "rmsprop", EB, EN)).all()


@pytest.mark.parametrize("exchange", ["server", "sharded", "allreduce"])
def test_group_exchange_semantics(ddq, ref, exchange):
    from test_gpu_exchange import group_exchange_semantics
    assert np.isfinite(group_exchange_semantics(ddq, ref, exchange, "rmsprop", EB, EN)).all()


def test_group_async_any_order_matches_server_replay(ddq, ref):
    """async_compute with one == false: the worker's draw advances the counter
    itself, the head kernel must not."""
    from _async_check import run_checked
    from test_gpu_async import make_group, minibatch_fn
    W, lr, period = 2, 1e-4, 4
    order = [0, 1, 1, 0, 1, 0]
    nets, arr, theta, data = make_group(ddq, W, log=16, B=EB, N=EN)
    try:
        cfg = nets[0].step_cfg("rmsprop", lr=lr, target_period=period, exchange="async", seed=5)
        # every tick's central model, owner state and P are checked; the oracle's
        # full pass (a second each at this batch) on both first gradients, on
        # worker 1's second push in a row and on the last tick
        central = run_checked(ddq, ref, nets, arr, cfg, order, minibatch_fn(nets, data),
                              "rmsprop", lr, period, theta,
                              grad_check=lambda t, w: t in (-1, 2, 5), what="B%d " % EB)
        moved_and_finite(theta, central)
        for w, n in enumerate(nets):
            n.synchronize()
            assert n.replay_draws() == 1 + order.count(w)
            for d in range(n.replay_draws()):
                np.testing.assert_array_equal(n.index_log(d, 1)[0],
                                              nr.draw(5, d, EB, 0, EN, 1, EN, 1))
    finally:
        for n in nets:
            n.close()


@pytest.mark.parametrize("exchange,overlap", [("allreduce", False), ("allreduce", True),
                                              ("sharded", False), ("server", False)])
def test_rccl_world1_exchange_equals_plain_step(ddq, ref, exchange, overlap):
    from test_gpu_exchange import rccl_world1_exchange_equals_plain_step
    # (lr 1e-6: at that test's own 1e-3 these 18 lagged-rmsprop steps on its x3
    # weights leave the finite range at B = 264, and two nets of NaN are equal)
    moved_and_finite(*rccl_world1_exchange_equals_plain_step(ddq, ref, exchange, overlap, EB, EN,
                                                             lr=1e-6))


def test_rccl_world1_async_ticks_and_graph_equal_plain_steps(ddq):
    """rccl_async_tick with draw == false: the owner apply launch carries no draw,
    the worker draws with the two launches."""
    from test_gpu_async import world1_async_ticks_and_graph_equal_plain_steps
    moved_and_finite(*world1_async_ticks_and_graph_equal_plain_steps(ddq, 3, EB, EN))


# ------------------------------------------------------------------ f. loops past 256
def test_monitor_record_and_select_action_past_256_images(ddq, ref):
    S, B = 16, 300
    net = make_net(ddq, S, B, ring_for(S), 0, lb.N)
    rng = np.random.default_rng(2)
    pQ = ref.init_params(S, seed=21)
    for k in pQ:
        pQ[k][0] = (pQ[k][0] * 3).astype(np.float32)
        pQ[k][1] = rng.normal(0, 0.05, pQ[k][1].shape).astype(np.float32)
    net.set_params(pQ)
    net.set_flat(1, (rng.standard_normal(net.num_params) * 0.02).astype(np.float32))
    net.replay_sample_device(5)
    net.forward_backward()
    net.monitor_enable(4)
    net.monitor_record(tag=7)
    recs, total = net.monitor_read()
    assert total == 1
    want = mr.expected(net, iteration=0, tag=7)
    q = net.blob("Q_out").reshape(B, 4).max(axis=1)
    # the images past the first 256 count: their mean alone is another number
    assert want["loss"] > 0 and np.float32(q[:256].mean()) != want["q_max_mean"]
    mr.assert_record(recs[0], want)
    states = rng.integers(0, 256, (B, 4, S, S)).astype(np.uint8)
    a = net.select_action(states)
    np.testing.assert_array_equal(a, ref.select_action(states.astype(np.float32), pQ))
    assert len(set(a[256:].tolist())) > 1
    done(net)


def test_monitor_inside_pipelined_steps_equals_eager(ddq):
    S, B, T = 16, 300, 3
    runs = []
    for mode in ("eager", "pipelined"):
        net = make_net(ddq, S, B, ring_for(S), 0, lb.N)
        net.monitor_enable(8, 1)
        cfg = net.step_cfg("rmsprop", lr=1e-5, target_period=3, seed=5)
        if mode == "eager":
            for k in range(T):
                net.step(cfg)
                net.synchronize()
                recs, total = net.monitor_read()
                assert total == k + 1
                mr.assert_record(recs[-1], mr.expected(net, iteration=k + 1, tag=-1))
        else:
            net.step_pipelined(cfg, T)
        net.synchronize()
        recs, total = net.monitor_read()
        assert total == T and (recs["nonfinite"] == 0).all() and np.isfinite(recs["loss"]).all()
        runs.append((recs.tobytes(), net.get_flat(0).tobytes()))
        done(net)
    assert runs[0] == runs[1]
