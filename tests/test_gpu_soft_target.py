"""GPU: soft target updates (ddq_set_target_tau) at every update site.

With tau < 1 a due target sync writes P' = P + tau (Q' - P) -- three fp32
operations, tests/_soft_target_ref.py's ``blend`` -- wherever a launch used to
copy Q' into thetaP, and the conv weights' split copies of P (wksP) follow the
blended value.  Every comparison here is of bytes.

Shapes (S, B) as tests/test_gpu_coherence.py's: (16, 8) the small-map step whose
K2 applies the unit sums, (16, 40) the one whose K4 does (two image chunks),
(24, 4) the general kernels.  Ring of 256 slots, seed 11, rmsprop at co.LR (Adam
at 1e-4).
"""
import numpy as np
import pytest

import _coherence as co
from _soft_target_ref import blend, targets

pytestmark = pytest.mark.gpu

SMALL, SMALL40, GENERAL = (16, 8), (16, 40), (24, 4)
THREE = [SMALL, SMALL40, GENERAL]
TWO = [SMALL, GENERAL]
SEED = 11
K = 4
RICH = dict(nstep=3, objective=("double", "huber", 0.5), prio=True)


def sid(shape):
    return "S%d-B%d" % shape


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


# ---------------------------------------------------------------- runs
def make(ddq, S, B, tau, rule="rmsprop", nstep=None, objective=None, prio=False, comm=False,
         ring_seed=0):
    net = co.make_net(ddq, S, B, ring_seed=ring_seed)
    if nstep:
        net.replay_set_nstep(nstep)
    if objective:
        net.set_objective(*objective)
    if prio:
        net.replay_set_priority(alpha=0.6, beta=0.4, eps=0.01)
    if rule == "adam":
        net.set_adam()
    if comm:
        net.comm_init(ddq.DeepQNet.comm_unique_id(), 1, 0)
    if tau is not None:
        net.set_target_tau(tau)
    return net


def cfg_of(net, rule="rmsprop", period=1, **kw):
    return net.step_cfg(rule, lr=1e-4 if rule == "adam" else co.LR, target_period=period,
                        seed=SEED, **kw)


def state(net, rule="rmsprop"):
    """(Q, P, optimizer state ...) as bytes-comparable arrays."""
    net.synchronize()
    out = [net.get_flat(0), net.get_flat(1)]
    if rule == "adam":
        m, v, t = net.adam_state()
        out += [m, v, np.asarray([t])]
    else:
        out.append(net.optimizer_state())
    return out


def same(a, b, what):
    names = ("Q", "P", "state", "state 2", "t")
    for n, x, y in zip(names, a, b):
        assert np.isfinite(x).all(), "%s: %s" % (what, n)
        assert x.tobytes() == y.tobytes(), "%s: %s differs in %d elements" % (what, n, int((x != y).sum()))


_CHAINS = {}


def chain(ddq, shape, tau, period, rule="rmsprop", **kw):
    """K eager steps one at a time: [(Q_t, P_t)] for t = 0..K and the final state."""
    key = (shape, tau, period, rule, tuple(sorted(kw)))
    if key not in _CHAINS:
        net = make(ddq, *shape, tau, rule, **kw)
        try:
            cfg = cfg_of(net, rule, period)
            qp = [(net.get_flat(0), net.get_flat(1))]
            for _ in range(K):
                net.step(cfg)
                net.synchronize()
                qp.append((net.get_flat(0), net.get_flat(1)))
            _CHAINS[key] = (qp, state(net, rule))
        finally:
            co.close_all([net])
    return _CHAINS[key]


# ---------------------------------------------------------------- 1. P is the blend, step by step
@pytest.mark.parametrize("tau", [0.01, 0.5])
@pytest.mark.parametrize("period", [1, 2])
@pytest.mark.parametrize("rule,shape", [("rmsprop", s) for s in THREE] + [("adam", s) for s in TWO],
                         ids=lambda v: v if isinstance(v, str) else sid(v))
def test_p_is_the_blend_step_by_step(ddq, rule, shape, period, tau):
    qp, _ = chain(ddq, shape, tau, period, rule)
    assert qp[0][1].tobytes() == qp[0][0].tobytes()
    want = targets(qp[0][1], [q for q, _ in qp[1:]], tau, period)
    for t in range(1, K + 1):
        q, p = qp[t]
        what = "%s %s tau %g period %d, update %d" % (rule, sid(shape), tau, period, t)
        assert np.isfinite(q).all() and q.tobytes() != qp[t - 1][0].tobytes(), what + ": Q"
        if t % period:
            assert p.tobytes() == qp[t - 1][1].tobytes(), what + ": P moved without a sync"
        else:
            assert p.tobytes() not in (qp[t - 1][1].tobytes(), q.tobytes()), what + ": no blend"
        assert p.tobytes() == want[t - 1].tobytes(), \
            "%s: P is not blend(P, Q, tau) (%d elements differ)" % (what, int((p != want[t - 1]).sum()))


# ---------------------------------------------------------------- 2. the modes agree
@pytest.mark.parametrize("mode", ["graph", "pipelined"])
@pytest.mark.parametrize("rich,shape", [(False, s) for s in THREE] + [(True, s) for s in TWO],
                         ids=lambda v: sid(v) if isinstance(v, tuple) else ("rich" if v else "plain"))
def test_modes_agree_with_the_eager_chain(ddq, rich, shape, mode):
    kw = RICH if rich else {}
    _, want = chain(ddq, shape, 0.5, 1, **kw)
    net = make(ddq, *shape, 0.5, **kw)
    try:
        cfg = cfg_of(net)
        (net.step_graph if mode == "graph" else net.step_pipelined)(cfg, K)
        same(state(net), want, "%s %s %s" % (mode, sid(shape), "rich" if rich else "plain"))
    finally:
        co.close_all([net])


# ---------------------------------------------------------------- 3. coherence
TAU = 0.5


def run_step(ddq, S, B, k, mode, rule="rmsprop", store_grads=True, comm=False, exchange="none",
             overlap=False):
    net = make(ddq, S, B, TAU, rule, comm=comm)
    cfg = cfg_of(net, rule, 1, store_grads=store_grads, exchange=exchange, overlap=overlap)
    if mode == "eager":
        for _ in range(k):
            net.step(cfg)
    elif mode == "graph":
        net.step_graph(cfg, k)
    else:
        net.step_pipelined(cfg, k)
    net.synchronize()
    return [net]


def run_group(ddq, S, B, k, exchange):
    nets = [make(ddq, S, B, TAU, ring_seed=r) for r in range(2)]
    arr = ddq.DeepQNet.group_init(nets)
    cfg = cfg_of(nets[0], exchange=exchange)
    for _ in range(k):
        ddq.DeepQNet.group_step(nets, cfg, arr)
    return nets


def run_host_loop(ddq, S, B, k):
    """Updates driven from the host: forward_backward, the apply launch and
    soft_sync_target() after every one."""
    net = make(ddq, S, B, TAU)
    rng = np.random.default_rng(5)
    for _ in range(k):
        net.replay_sample(np.sort(rng.choice(np.arange(8, co.N - 8), B, replace=False)).astype(np.int32))
        net.forward_backward()
        net.apply("rmsprop", lr=co.LR)
        net.soft_sync_target()
    return [net]


REGIMES = {
    "eager-rmsprop": lambda d, S, B, k: run_step(d, S, B, k, "eager"),
    "graph-rmsprop": lambda d, S, B, k: run_step(d, S, B, k, "graph"),
    "pipelined-rmsprop": lambda d, S, B, k: run_step(d, S, B, k, "pipelined"),
    "eager-adam": lambda d, S, B, k: run_step(d, S, B, k, "eager", rule="adam"),
    "eager-nostore": lambda d, S, B, k: run_step(d, S, B, k, "eager", store_grads=False),
    "host-loop": run_host_loop,
}
for _mode in ("eager", "pipelined"):
    for _ex, _ov in (("allreduce", True), ("allreduce", False), ("sharded", False), ("server", False)):
        REGIMES["comm1-%s-%s%s" % (_mode, _ex, "-overlap" if _ov else "")] = (
            lambda d, S, B, k, m=_mode, e=_ex, o=_ov: run_step(d, S, B, k, m, comm=True, exchange=e,
                                                               overlap=o))
for _ex in ("allreduce", "sharded", "server"):
    REGIMES["group-" + _ex] = lambda d, S, B, k, e=_ex: run_group(d, S, B, k, e)
WIDE = ["eager-rmsprop", "graph-rmsprop", "pipelined-rmsprop"]


def coherence_cases():
    out = []
    for name in REGIMES:
        for shape in (THREE if name in WIDE else TWO):
            for k in co.PROBES:
                out.append(pytest.param(name, shape, k, id="%s-%s-k%d" % (name, sid(shape), k)))
    return out


_QS = {}


def q_after(ddq, name, shape, t, nets=None):
    """[Q of member r] after t updates of the regime (the runs are deterministic:
    a probe point's own run fills its entry, the earlier ones run once)."""
    key = (name, shape, t)
    if key not in _QS:
        own = nets is None
        if own:
            nets = REGIMES[name](ddq, *shape, t)
        try:
            _QS[key] = [n.get_flat(0) for n in nets]
        finally:
            if own:
                co.close_all(nets)
    return _QS[key]


@pytest.mark.parametrize("name,shape,k", coherence_cases())
def test_coherent_after_soft_updates(ddq, name, shape, k):
    """The probe after 2, 3 and 4 soft updates (tau 0.5, period 1): the context
    must multiply by split3 of the blended P.  want_p: test 1's recursion over
    the regime's own Q_1 .. Q_k."""
    nets = REGIMES[name](ddq, *shape, k)
    try:
        q_after(ddq, name, shape, k, nets)
        for r, net in enumerate(nets):
            qs = [q_after(ddq, name, shape, t)[r] for t in range(1, k + 1)]
            want_p = targets(co.theta0(shape[0]), qs, TAU, 1)[-1]
            assert want_p.tobytes() != qs[-1].tobytes()
            what = "soft %s %s, %d updates, member %d" % (name, sid(shape), k, r)
            assert net.get_flat(0).tobytes() == qs[-1].tobytes(), what + ": the run is not deterministic"
            co.check(ddq, net, want_p, what)
    finally:
        co.close_all(nets)


# ---------------------------------------------------------------- 4. the probe can see a miss
@pytest.mark.parametrize("shape", TWO, ids=sid)
def test_probe_sees_a_stale_target(ddq, shape):
    """After 3 soft updates (tau 0.5, co.LR, probe seed 0) a fresh context given
    (Q, P of one update earlier) -- what a site that forgot wksP would multiply
    by -- is told from the coherent one.  Nothing had to be raised: tau 0.5 at
    co.LR and probe seed 0 are seen at both shapes."""
    qp, _ = chain(ddq, shape, TAU, 1)
    (q, p), (_, p_prev) = qp[3], qp[2]
    assert p.tobytes() != p_prev.tobytes()
    net, = run_step(ddq, *shape, 3, "eager")
    try:
        assert net.get_flat(1).tobytes() == p.tobytes()
        mb, states = co.probe_inputs(net.batch, net.frame, 0)
        got, want = co.probe(ddq, net, mb, states)
        co.assert_coherent(got, want, "soft eager %s, 3 updates" % sid(shape))
        d = co.detected(ddq, net, want, mb, states, q, p_prev)
        print("stale P: %s" % ("detected in " + d if d else "NOT DETECTED"))
        assert d is not None, "the probe does not see a P one soft update stale"
    finally:
        co.close_all([net])


# ---------------------------------------------------------------- 5. off is off, tau re-captures
def stepper(net, mode):
    if mode == "eager":
        return lambda cfg, n: [net.step(cfg) for _ in range(n)]
    return net.step_graph if mode == "graph" else net.step_pipelined


@pytest.mark.parametrize("mode", ["eager", "graph", "pipelined"])
@pytest.mark.parametrize("shape", THREE, ids=sid)
def test_tau_1_is_the_hard_copy(ddq, shape, mode):
    got = []
    for tau in (None, 1.0):
        net = make(ddq, *shape, tau)
        try:
            stepper(net, mode)(cfg_of(net, period=3), K)
            got.append(state(net))
        finally:
            co.close_all([net])
    same(got[1], got[0], "tau 1 %s %s" % (mode, sid(shape)))
    assert got[0][1].tobytes() != got[0][0].tobytes()      # (P lags after 4 updates at period 3)


@pytest.mark.parametrize("shape", THREE, ids=sid)
def test_setting_tau_recaptures(ddq, shape):
    got = []
    for mode in ("eager", "graph"):
        net = make(ddq, *shape, None)
        try:
            cfg, go = cfg_of(net), stepper(net, mode)
            go(cfg, 2)
            net.synchronize()
            assert net.get_flat(1).tobytes() == net.get_flat(0).tobytes()
            net.set_target_tau(0.5)
            go(cfg, 2)
            got.append(state(net))
        finally:
            co.close_all([net])
    same(got[1], got[0], "tau change %s" % sid(shape))
    assert got[0][1].tobytes() != got[0][0].tobytes()      # (the last two syncs blended)


# ---------------------------------------------------------------- 6. the async exchange refuses
def test_async_refuses_soft_targets(ddq):
    from ddq import _lib
    net = make(ddq, *SMALL, 0.5, comm=True)
    try:
        cfg = cfg_of(net, period=co.PERIOD, exchange="async")
        for call in (lambda: net.async_begin(cfg), lambda: net.step(cfg), lambda: net.async_tick(cfg, 0)):
            with pytest.raises(_lib.DDQError) as ei:
                call()
            assert ei.value.code == _lib.DDQ_EINVAL
            assert "tau" in str(ei.value) and "ASYNC" in str(ei.value).upper()
        net.set_target_tau(1.0)            # the same calls work as before
        net.async_begin(cfg)
        while not net.async_ready():
            pass
        net.async_tick(cfg, 0)
        net.synchronize()
        assert net.get_flat(0).tobytes() != co.theta0(SMALL[0]).tobytes()
        with pytest.raises(_lib.DDQError) as ei:      # and tau < 1 is refused once it began
            net.set_target_tau(0.5)
        assert ei.value.code == _lib.DDQ_EINVAL and net.target_tau() == 1.0
    finally:
        co.close_all([net])


# ---------------------------------------------------------------- 7. ddq_soft_sync_target
@pytest.mark.parametrize("tau", [0.5, 0.01])
@pytest.mark.parametrize("shape", TWO, ids=sid)
def test_soft_sync_target_on_the_device(ddq, shape, tau):
    S, B = shape
    q, p = co.theta0(S), co.theta0(S, seed=43)
    net = co.make_net(ddq, S, B, theta_p=p)
    try:
        net.set_target_tau(tau)
        want = p
        for n in (1, 2):
            net.soft_sync_target()
            want = blend(want, q, tau)
            assert net.get_flat(0).tobytes() == q.tobytes()
            co.check(ddq, net, want, "soft_sync_target x%d %s tau %g" % (n, sid(shape), tau))
        net.set_target_tau(1.0)
        net.soft_sync_target()
        co.check(ddq, net, q, "soft_sync_target at tau 1 %s" % sid(shape))
    finally:
        co.close_all([net])
