"""DDQ_RULE_ADAM on the device (csrc/adam.h) against tests/_adam_ref.py: the
apply launch alone, teacher-forced steps, the three step modes byte-identical
(plain, and with n = 3, Double + Huber and prioritized replay on), a step
against its parts, clipping inside steps, the in-process group under
all-reduce, and off is off.  S = 16 runs the small-map step, S = 32 the general
kernels; B = 8.
"""
import numpy as np
import pytest

import _adam_ref as ar
import _coherence as co
import _nstep_ref as nr
from _parity import close

pytestmark = pytest.mark.gpu

B = 8
CAP, HEAD = 130, 7
EINVAL, ESTATE = -1, -5
# Adam moves every weight by about lr in its first steps whatever the gradient's
# size; at S = 32 (half a million fc4 weights at B = 8) chains stay finite at
# 1e-6, as the rmsprop chains of the other suites do
LR = {16: 1e-4, 32: 1e-6}
_RING = {}


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


def ring_for(S, seed=CAP):
    if (S, seed) not in _RING:
        _RING[(S, seed)] = nr.build_ring(np.random.default_rng(seed), CAP, S)
    return _RING[(S, seed)]


def theta0(S):
    from ddq.params import init_params_flat
    return init_params_flat(S, seed=42)


def make_net(ddq, S, adam=None, full=False, ring_seed=CAP):
    """A net on a filled ring; adam: set_adam's keywords (None: never called);
    full: n = 3, Double + Huber and prioritized replay on."""
    net = ddq.DeepQNet(batch=B, frame=S)
    assert net.small_path()[0] == (S == 16)
    th = theta0(S)
    net.set_flat(0, th)
    net.set_flat(1, th)
    ring = ring_for(S, ring_seed)
    net.replay_create(CAP)
    net.replay_import(ring[0], ring[1], ring[2], np.asarray(ring[3], np.uint8), HEAD, CAP)
    if full:
        net.replay_set_nstep(3)
        net.set_objective("double", "huber", 0.5)
        net.replay_set_priority(alpha=0.6, beta=0.4, eps=0.01)
    if adam is not None:
        net.set_adam(**adam)
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


def state_of(net):
    m, v, t = net.adam_state()
    return net.get_flat(0), m, v, t


def check_update(net, before, k, lr, what):
    """The net's state against the reference update of `before` with the
    gradient buffer the net holds now.  Returns the pre-clip norm."""
    th0, m0, v0, t0 = before
    g = net.get_grads_flat()
    th, m, v, nrm = ar.step(th0, g, m0 if t0 else None, v0 if t0 else None, t0 + 1, ar.f32(lr), **k)
    gth, gm, gv, gt = state_of(net)
    assert gt == t0 + 1, what
    close(gth, th, what=what + " theta")
    close(gm, m, what=what + " m")
    close(gv, v, what=what + " v")
    return nrm


# 1 ---------------------------------------------------------------- the apply launch
@pytest.mark.parametrize("S", [16, 32])
def test_apply_parity(ddq, S):
    net = ddq.DeepQNet(batch=B, frame=S)
    theta = theta0(S)
    theta_p = co.theta0(S, seed=43)
    net.set_flat(0, theta)
    net.set_flat(1, theta_p)
    net.reset_optimizer()
    assert code_of(lambda: net.apply("adam", lr=1e-3)) == ESTATE
    net.set_adam()
    k = ar.constants()
    rng = np.random.default_rng(11)
    for t in range(1, 5):
        g = rng.normal(0, 1e-2, theta.size).astype(np.float32)
        net.set_grads_flat(g)
        before = state_of(net)
        assert before[3] == t - 1
        net.apply("adam", lr=1e-3)
        check_update(net, before, k, 1e-3, "S%d apply %d" % (S, t))
        assert net.optimizer_state().tobytes() == net.adam_state()[0].tobytes()
        assert net.get_grads_flat().tobytes() == g.tobytes()
    assert code_of(lambda: net.blob("grad_norm")) == ESTATE
    # the conv weights' split layouts were refreshed, and P's (another
    # initialisation, set before the applies) left alone: both towers' forward,
    # the backward and the actions on this net are those of a fresh net given the
    # same parameters, byte for byte (tests/_coherence.py)
    assert net.get_flat(1).tobytes() == theta_p.tobytes()
    mb, states = co.probe_inputs(B, S)
    got, want = co.probe(ddq, net, mb, states)
    co.assert_coherent(got, want, "S%d after four Adam applies" % S)
    # reset: m, v, t back to zero
    net.reset_optimizer()
    m, v, t = net.adam_state()
    assert t == 0 and not m.any() and not v.any()
    done(net)


@pytest.mark.parametrize("S", [16, 32])
def test_apply_clipping(ddq, S):
    rng = np.random.default_rng(12)
    theta = theta0(S)
    g = rng.normal(0, 1e-2, theta.size).astype(np.float32)
    nrm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    out = []
    for c in (0.5 * nrm, 0.0, 2.0 * nrm):
        net = ddq.DeepQNet(batch=B, frame=S)
        net.set_flat(0, theta)
        net.set_adam(max_grad_norm=c)
        net.set_grads_flat(g)
        before = state_of(net)
        net.apply("adam", lr=1e-3)
        if c > 0:
            got = float(net.blob("grad_norm"))
            assert abs(got - nrm) <= 2 * 2.0 ** -23 * nrm, (got, nrm)
        if c == 0.5 * nrm:
            check_update(net, before, ar.constants(max_grad_norm=c), 1e-3, "S%d clipped" % S)
            assert net.get_grads_flat().tobytes() == g.tobytes()
        else:
            net.set_grads_flat(g * np.float32(0.5))
            net.apply("adam", lr=1e-3)
            out.append([x.tobytes() for x in state_of(net)[:3]])
        done(net)
    assert out[0] == out[1]       # a threshold above the norm: the same bits as clipping off


# 2 ---------------------------------------------------------------- teacher-forced steps
@pytest.mark.parametrize("S", [16, 32])
def test_teacher_forced_chain(ddq, S):
    net = make_net(ddq, S, adam={})
    k = ar.constants()
    cfg = net.step_cfg("adam", lr=LR[S], target_period=3, seed=11, store_grads=False)
    p0 = net.get_flat(1)
    for t in range(1, 7):
        before = state_of(net)
        net.step(cfg)
        net.synchronize()
        check_update(net, before, k, LR[S], "S%d step %d" % (S, t))
        p = net.get_flat(1)
        if t % 3 == 0:            # the sync step's apply launch copied Q -> P
            assert p.tobytes() == net.get_flat(0).tobytes(), t
        else:
            assert p.tobytes() == p0.tobytes(), t
        p0 = p
    assert net.replay_draws() == 6
    done(net)


# 3 ---------------------------------------------------------------- step modes
STEPS = 12
_CHAINS = {}


def chain(ddq, S, mode, full, rule="adam", adam=None):
    key = (S, mode, full, rule, str(adam))
    if key in _CHAINS:
        return _CHAINS[key]
    net = make_net(ddq, S, adam=adam, full=full)
    net.index_log_enable(16)
    cfg = net.step_cfg(rule, lr=LR[S], target_period=5, seed=11)
    if mode == "eager":
        for _ in range(STEPS):
            net.step(cfg)
    elif mode == "graph":
        net.step_graph(cfg, STEPS)
    else:
        net.step_pipelined(cfg, STEPS)        # one 8-step graph and a 4-step tail
    net.synchronize()
    out = {"state": [net.get_flat(0), net.get_flat(1), net.optimizer_state()],
           "log": net.index_log(0, STEPS), "draws": net.replay_draws(),
           "idx": net.read_indices()}
    if adam is not None:
        m, v, t = net.adam_state()
        out["state"] += [m, v]
        out["t"] = t
    if full:
        out["prio"] = net.replay_priorities()
    assert all(np.isfinite(s).all() for s in out["state"])
    net._check(net.lib.ddq_replay_status(net.ctx))
    done(net)
    _CHAINS[key] = out
    return out


@pytest.mark.parametrize("S", [16, 32])
@pytest.mark.parametrize("full", [False, True])
def test_step_modes_agree(ddq, S, full):
    eager = chain(ddq, S, "eager", full, adam={})
    assert eager["draws"] == STEPS and eager["t"] == STEPS
    assert eager["state"][0].tobytes() != theta0(S).tobytes()
    assert eager["state"][1].tobytes() != eager["state"][0].tobytes()   # P: the step-10 model
    assert eager["state"][3].any() and eager["state"][4].any()
    if full:
        q, total, pmax = eager["prio"]
        assert total == int(q.astype(np.int64).sum())
        assert len(set(q.tolist())) > B                 # the chain committed
    for mode in ("graph", "pipelined"):
        other = chain(ddq, S, mode, full, adam={})
        for a, b in zip(eager["state"], other["state"]):
            assert a.tobytes() == b.tobytes(), mode
        assert eager["log"].tobytes() == other["log"].tobytes(), mode
        assert eager["idx"].tobytes() == other["idx"].tobytes(), mode
        assert other["draws"] == STEPS and other["t"] == STEPS, mode
        if full:
            assert eager["prio"][0].tobytes() == other["prio"][0].tobytes(), mode
            assert eager["prio"][1:] == other["prio"][1:], mode


# 4 ---------------------------------------------------------------- a step and its parts
@pytest.mark.parametrize("S", [16, 32])
def test_step_equals_its_parts(ddq, S):
    """Four Adam steps (target period 2) on one net; a second net is given every
    step's minibatch and P tower and runs forward_backward + apply("adam").  The
    step after a sync step reads the P layouts the Adam launch wrote."""
    a = make_net(ddq, S, adam={})
    b = make_net(ddq, S, adam={})
    cfg = a.step_cfg("adam", lr=LR[S], target_period=2, seed=5)
    for t in range(1, 5):
        b.set_flat(1, a.get_flat(1))
        a.step(cfg)
        a.synchronize()
        b.replay_sample(a.read_indices())
        b.forward_backward()
        assert a.get_grads_flat().tobytes() == b.get_grads_flat().tobytes(), t
        b.apply("adam", lr=LR[S])
        for x, y in zip(state_of(a), state_of(b)):
            assert x == y if isinstance(x, int) else x.tobytes() == y.tobytes(), t
        assert (a.get_flat(1).tobytes() == a.get_flat(0).tobytes()) == (t % 2 == 0), t
    done(a, b)


# 5 ---------------------------------------------------------------- clipping inside steps
@pytest.mark.parametrize("S", [16, 32])
def test_clipping_inside_steps(ddq, S):
    probe = make_net(ddq, S, adam=dict(max_grad_norm=1e30))
    cfg = probe.step_cfg("adam", lr=LR[S], target_period=5, seed=11)
    probe.step(cfg)
    probe.synchronize()
    nrm = float(probe.blob("grad_norm"))
    g = probe.get_grads_flat().astype(np.float64)
    want = float(np.sqrt(np.sum(g * g)))
    assert abs(nrm - want) <= 2 * 2.0 ** -23 * want, (nrm, want)
    done(probe)
    c = ar.f32(0.5 * nrm)
    net = make_net(ddq, S, adam=dict(max_grad_norm=c))
    k = ar.constants(max_grad_norm=c)
    before = state_of(net)
    names = [n for n, _ in net.profile_step(cfg)]
    assert "grad_norm" in names and "adam_apply" in names and "apply" not in names, names
    assert names.index("grad_norm") + 1 == names.index("adam_apply"), names
    got = check_update(net, before, k, LR[S], "S%d clipped step" % S)
    assert got > c and abs(float(net.blob("grad_norm")) - got) <= 2 * 2.0 ** -23 * got
    before = state_of(net)
    net.step(cfg)                     # and a second, non-first step
    net.synchronize()
    check_update(net, before, k, LR[S], "S%d clipped step 2" % S)
    done(net)


# 6 ---------------------------------------------------------------- in-process group
@pytest.mark.parametrize("S", [16, 32])
def test_group_allreduce(ddq, S):
    nets = [make_net(ddq, S, adam=dict(max_grad_norm=1e30), ring_seed=CAP + r) for r in range(2)]
    arr = ddq.DeepQNet.group_init(nets)
    cfg = nets[0].step_cfg("adam", lr=LR[S], target_period=5, seed=3, exchange="allreduce")
    c = 1e30
    for t in range(1, 3):
        k = ar.constants(max_grad_norm=c)
        before = state_of(nets[0])
        ddq.DeepQNet.group_step(nets, cfg, arr)
        # (the members' gradient buffers hold the sum)
        assert nets[0].get_grads_flat().tobytes() == nets[1].get_grads_flat().tobytes()
        nrm = check_update(nets[0], before, k, LR[S], "S%d group step %d" % (S, t))
        for x, y in zip(state_of(nets[0]), state_of(nets[1])):
            assert x == y if isinstance(x, int) else x.tobytes() == y.tobytes(), t
        got = float(nets[0].blob("grad_norm"))
        assert abs(got - nrm) <= 2 * 2.0 ** -23 * nrm
        c = ar.f32(0.5 * nrm)         # the second step clips the summed gradient
        for n in nets:
            n.set_adam(max_grad_norm=c)
    th = [n.get_flat(0).tobytes() for n in nets]
    for ex in ("sharded", "server", "async"):
        bad = nets[0].step_cfg("adam", lr=LR[S], target_period=5, seed=3, exchange=ex)
        assert code_of(lambda: ddq.DeepQNet.group_step(nets, bad, arr)) == EINVAL, ex
    assert code_of(lambda: nets[0].async_begin(bad)) == EINVAL
    assert [n.get_flat(0).tobytes() for n in nets] == th
    assert nets[0].adam_state()[2] == 2
    done(*nets)


# 7 ---------------------------------------------------------------- off is off
@pytest.mark.parametrize("S", [16, 32])
def test_off_is_off(ddq, S):
    plain = chain(ddq, S, "pipelined", False, rule="rmsprop", adam=None)
    conf = chain(ddq, S, "pipelined", False, rule="rmsprop", adam=dict(max_grad_norm=1.0))
    for a, b in zip(plain["state"], conf["state"][:3]):
        assert a.tobytes() == b.tobytes()
    assert plain["log"].tobytes() == conf["log"].tobytes() and conf["draws"] == STEPS
    assert not conf["state"][4].any()             # v was never touched
    names = []
    for adam in (None, dict(max_grad_norm=1.0)):
        net = make_net(ddq, S, adam=adam)
        names.append([n for n, _ in net.profile_step(net.step_cfg("rmsprop", lr=LR[S], seed=11))])
        done(net)
    assert names[0] == names[1] and "adam_apply" not in names[0]
