"""Selectable TD objective on the device (ddq_set_objective): the Double-DQN
target's extra Q forward, the head's target / clamp / loss in both head kernels
(fc4_head_kernel and the small-map fc4 chain, one and two towers a workgroup),
every step mode, and the default objective left bit for bit as it was.

The cases and their float64 oracle are tests/_objective_ref.py's; each case's
inputs are well separated on the oracle (asserted there before the device is
touched), so the fp32 argmax and every clip decision must agree with it
outright.  fp32 head arithmetic is checked bit for bit from the net's own
blobs; oracle parity uses tests/_parity.py's rule unchanged.
"""
import ctypes

import numpy as np
import pytest

import _objective_ref as objr

pytestmark = pytest.mark.gpu

NAMES = ("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss", "Q_out.diff")
NAMES_D = NAMES + ("Qn_out",)


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


_RUNS = {}


def run(ddq, ref, key):
    """One {DOUBLE, HUBER} pass of a case (the net kept open, not changed)."""
    if key not in _RUNS:
        c = objr.case(ref, *key)
        net = objr.make_net(ddq, c)
        assert net.small_path()[0] == (key[0] == 16)
        net.set_objective("double", "huber", c["o"]["delta"])
        loss = net.forward_backward()
        _RUNS[key] = dict(c=c, net=net, loss=loss, got=objr.blobs_of(net, NAMES_D),
                          grads=net.get_grads_flat())
    return _RUNS[key]


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("key", objr.CASES)
def test_qn_out_is_the_q_forward(ddq, ref, key):
    c = objr.case(ref, *key)
    net = objr.make_net(ddq, c)
    net.set_objective("double")
    net.forward_backward()
    qn = net.blob("Qn_out")
    net.write_minibatch(state=c["mb"][3])          # next_state as state
    net.forward_q()
    assert qn.tobytes() == net.blob("Q_out").tobytes()
    assert qn.tobytes() == net.blob("Qn_out").tobytes()   # a buffer of its own: still there
    net.close()


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("key", objr.CASES)
def test_target_from_the_blobs(ddq, ref, key):
    r = run(ddq, ref, key)
    o, got = r["c"]["o"], r["got"]
    e = objr.expected_head_f32(got, o["act"], o["nt"], o["r"], ref.GAMMA, "double", o["delta"])
    assert got["P_sa"].tobytes() == e["P_sa"].tobytes()
    ulp = np.spacing(np.abs(e["target64"]).astype(np.float32)).astype(np.float64)
    err = np.abs(got["target_Q_sa"].astype(np.float64) - e["target64"])
    print("target: max error %.3g ulp" % float(np.max(err / ulp)))
    assert np.all(err <= ulp)
    assert np.any(got["P_sa"] != got["P_out"].max(axis=1) * o["nt"].astype(np.float32))


# 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("key", objr.CASES)
def test_dq_and_loss_from_the_blobs(ddq, ref, key):
    r = run(ddq, ref, key)
    o, got = r["c"]["o"], r["got"]
    e = objr.expected_head_f32(got, o["act"], o["nt"], o["r"], ref.GAMMA, "double", o["delta"])
    assert got["Q_out.diff"].tobytes() == e["dQ"].tobytes()
    assert (np.abs(e["d"]) > o["delta"]).sum() == o["B"] // 2
    print("loss %.9g, from the blobs %.9g" % (float(got["loss"][0]), e["loss"]))
    np.testing.assert_allclose(float(got["loss"][0]), e["loss"], rtol=1e-4)
    assert r["loss"] == float(got["loss"][0])


# 4 ------------------------------------------------------------------------
@pytest.mark.parametrize("key", objr.CASES)
def test_double_target_changes_only_the_target(ddq, ref, key):
    c = objr.case(ref, *key)
    B = key[1]
    net = objr.make_net(ddq, c)
    net.set_objective("double", "euclidean")
    net.forward_backward()
    g1, b1 = net.get_grads_flat(), objr.blobs_of(net, NAMES)
    net.set_objective("max", "euclidean")
    net.forward_backward()
    assert net.get_grads_flat().tobytes() != g1.tobytes()      # the max target is another one
    net.write_minibatch(reward=b1["target_Q_sa"], non_terminal=np.zeros(B, np.float32))
    net.forward_backward()
    b2 = objr.blobs_of(net, NAMES)
    assert b2["target_Q_sa"].tobytes() == b1["target_Q_sa"].tobytes()
    assert net.get_grads_flat().tobytes() == g1.tobytes()
    for k in ("Q_out", "P_out", "Q_sa", "loss", "Q_out.diff"):
        assert b2[k].tobytes() == b1[k].tobytes(), k
    net.close()


# 5 ------------------------------------------------------------------------
@pytest.mark.parametrize("key", objr.CASES)
def test_wide_band_is_the_euclidean_loss(ddq, ref, key):
    c = objr.case(ref, *key)
    net = objr.make_net(ddq, c)
    net.set_objective("double", "euclidean")
    net.forward_backward()
    b0, g0 = objr.blobs_of(net, NAMES_D), net.get_grads_flat()
    d = b0["Q_sa"] - b0["target_Q_sa"]
    net.set_objective("double", "huber", 2.0 * float(np.max(np.abs(d))))
    net.forward_backward()
    b1, g1 = objr.blobs_of(net, NAMES_D), net.get_grads_flat()
    assert g0.tobytes() == g1.tobytes()
    for k in NAMES_D:
        assert b0[k].tobytes() == b1[k].tobytes(), k
    assert g0.tobytes() != run(ddq, ref, key)["grads"].tobytes()   # the case's band clips
    net.close()


# 6 ------------------------------------------------------------------------
@pytest.mark.parametrize("S", [16, 24])
def test_exact_scaling_at_batch_one(ddq, ref, S):
    """B = 1, delta = |d| / 2: the clamped error is d / 2, and scaling by a power
    of two commutes with fp32 rounding and the bf16 split (flushed denormals
    aside), so every gradient element is half the plain one."""
    for seed in range(900, 932):
        pQ, pP, mb = objr.draw(ref, S, 1, seed)
        c = dict(pQ=pQ, pP=pP, mb=mb)
        net = objr.make_net(ddq, c)
        net.forward_backward()
        b = objr.blobs_of(net, NAMES)
        d = float(np.float32(b["Q_sa"][0]) - np.float32(b["target_Q_sa"][0]))
        if abs(d) >= 1e-3:
            break
        net.close()
    else:
        raise AssertionError("no seed with |d| >= 1e-3")
    g_plain = net.get_grads_flat()
    net.set_objective("max", "huber", abs(d) / 2)
    net.forward_backward()
    g = net.get_grads_flat()
    loss = float(net.blob("loss"))
    big = np.abs(g_plain) >= 2.0 ** -60
    print("S %d seed %d: d %.6g, %d/%d elements >= 2^-60" % (S, seed, d, int(big.sum()), g.size))
    assert big.sum() > g.size // 100
    assert g[big].tobytes() == (np.float32(0.5) * g_plain[big]).tobytes()
    assert np.all(np.abs(g[~big].astype(np.float64) - 0.5 * g_plain[~big].astype(np.float64))
                  <= 2.0 ** -80)
    np.testing.assert_allclose(loss, 3.0 * d * d / 8.0, rtol=1e-4)
    net.close()


# 7 ------------------------------------------------------------------------
@pytest.mark.parametrize("key", objr.CASES)
def test_oracle_parity_double_huber(ddq, ref, key):
    r = run(ddq, ref, key)
    counts = objr.check_objective_pass(ref, r["net"], r["c"], r["c"]["o"], what="%s " % (key,))
    print("head tensors, elements >= 1e-2 of max (held to rtol 1e-4): Q_out W %d, b %d"
          % (counts["Q_out[0]"], counts["Q_out[1]"]))


# 8 - 10: step modes ---------------------------------------------------------
STEP_B, STEP_N, STEPS = 4, 64, 12
_RING, _CHAINS = {}, {}


def ring_for(S):
    if S not in _RING:
        from ddq.expgain import synthetic_transitions
        _RING[S] = synthetic_transitions(STEP_N, S, seed=77)
    return _RING[S]


def theta_for(ref, S):
    pQ, _, _ = objr.draw(ref, S, 1, 903)
    return ref.flatten(pQ)


def step_net(ddq, ref, S):
    net = ddq.DeepQNet(batch=STEP_B, frame=S)
    th = theta_for(ref, S)
    net.set_flat(0, th)
    net.set_flat(1, th)
    st, ac, rw, nt = ring_for(S)
    net.replay_create(STEP_N)
    net.replay_import(st, ac, rw, nt, 0, STEP_N)
    net.index_log_enable(16)
    return net


def step_cfg(net):
    # lr: the "x3" parameters on 0..255 frames give gradients of O(100), and the
    # reference's lagged-cache rmsprop takes steps of lr g / |g_prev|: at 1e-4 any
    # objective's chain overflows within 12 steps, at 1e-6 |d| stays around 1..3
    # (so the band of 1 clips)
    return net.step_cfg("rmsprop", lr=1e-6, target_period=5, seed=11)


def chain(ddq, ref, S, mode, objective, toggled=False):
    """STEPS steps of one step mode on a fresh ctx under an objective (None: never
    set; toggled: set to {DOUBLE, HUBER} and back to the default first); its
    final state, index log and, after the chain, one profiled step's names."""
    key = (S, mode, objective, toggled)
    if key not in _CHAINS:
        net = step_net(ddq, ref, S)
        if toggled:
            net.set_objective("double", "huber", 1.0)
            net.set_objective()
        if objective is not None:
            net.set_objective(*objective)
        cfg = step_cfg(net)
        if mode == "eager":
            for _ in range(STEPS):
                net.step(cfg)
        elif mode == "graph":
            net.step_graph(cfg, STEPS)
        else:
            net.step_pipelined(cfg, STEPS)
        net.synchronize()
        state = [net.get_flat(0), net.get_flat(1), net.optimizer_state()]
        assert all(np.isfinite(s).all() for s in state)
        log = net.index_log(0, STEPS)
        names = [n for n, _ in net.profile_step(cfg)]
        _CHAINS[key] = dict(state=state, log=log, names=names)
        net.close()
    return _CHAINS[key]


DH = ("double", "huber", 1.0)


@pytest.mark.parametrize("S", [16, 24])
def test_step_modes_agree(ddq, ref, S):
    eager = chain(ddq, ref, S, "eager", DH)
    for mode in ("graph", "pipelined"):
        other = chain(ddq, ref, S, mode, DH)
        for a, b in zip(eager["state"], other["state"]):
            assert a.tobytes() == b.tobytes(), mode
        assert eager["log"].tobytes() == other["log"].tobytes()
    plain = chain(ddq, ref, S, "pipelined", None)
    assert plain["log"].tobytes() == eager["log"].tobytes()
    assert plain["state"][0].tobytes() != eager["state"][0].tobytes()
    assert eager["state"][0].tobytes() != theta_for(ref, S).tobytes()


@pytest.mark.parametrize("S", [16, 24])
def test_off_is_off(ddq, ref, S):
    never = chain(ddq, ref, S, "pipelined", None)
    back = chain(ddq, ref, S, "pipelined", None, toggled=True)
    for a, b in zip(never["state"], back["state"]):
        assert a.tobytes() == b.tobytes()
    assert never["log"].tobytes() == back["log"].tobytes()
    assert never["names"] == back["names"]
    assert not any(n.startswith("qn_") for n in never["names"])


@pytest.mark.parametrize("S", [16, 24])
def test_profile_lists_the_extra_forward(ddq, ref, S):
    plain = chain(ddq, ref, S, "pipelined", None)["names"]
    huber = chain(ddq, ref, S, "pipelined", ("max", "huber", 1.0))["names"]
    double = chain(ddq, ref, S, "eager", DH)["names"]
    print("plain  %s\ndouble %s" % (plain, double))
    assert huber == plain
    extra = [n for n in double if n.startswith("qn_")]
    assert [n for n in double if not n.startswith("qn_")] == plain
    assert len(extra) >= 2 and len(set(extra)) == len(extra) and len(double) <= 32
    head = double.index("fc4_chain" if S == 16 else "head")
    first = double.index(extra[0])
    assert double[first:first + len(extra)] == extra and first + len(extra) <= head
    # the first launch group of the pass: right after the draw + gather
    assert double[:first] == plain[:first] and all("fwd" not in n for n in plain[:first])


def test_error_cases(ddq):
    from ddq import _lib
    net = ddq.DeepQNet(batch=2, frame=16)
    net.set_objective("double", "huber", 0.5)
    bad = [(2, 0, 0.0, 0), (-1, 0, 0.0, 0), (0, 2, 1.0, 0), (0, -1, 1.0, 0), (0, 1, 0.0, 0),
           (0, 1, -1.0, 0), (1, 1, float("nan"), 0), (1, 1, float("inf"), 0), (0, 0, 0.0, 1)]
    for t, l, d, r in bad:
        o = _lib.Objective(t, l, d, r)
        assert net.lib.ddq_set_objective(net.ctx, ctypes.byref(o)) == _lib.DDQ_EINVAL, (t, l, d, r)
        assert net.objective() == {"target": "double", "loss": "huber", "huber_delta": 0.5}
    assert net.lib.ddq_set_objective(net.ctx, None) == _lib.DDQ_EINVAL
    net.set_objective("max", "huber", 2.0)
    with pytest.raises(_lib.DDQError) as ei:
        net.blob("Qn_out")
    assert ei.value.code == _lib.DDQ_ESTATE
    assert net.blob("Q_out.diff").shape == (2, 4, 1, 1)
    net.set_objective()
    assert net.objective() == {"target": "max", "loss": "euclidean", "huber_delta": 0.0}
    net.close()


def test_refused_once_the_async_exchange_began(ddq):
    from ddq import _lib
    from ddq.expgain import synthetic_transitions
    net = ddq.DeepQNet(batch=4, frame=16)
    st, ac, rw, nt = synthetic_transitions(32, 16, seed=77)
    net.replay_create(32)
    net.replay_import(st, ac, rw, nt, 0, 32)
    net.comm_init(net.comm_unique_id(), 1, 0)      # the async exchange needs a communicator
    net.set_objective("double", "huber", 1.0)      # set before the exchange begins: honoured
    net.async_begin(net.step_cfg("rmsprop", lr=1e-5, target_period=3, seed=5, exchange="async"))
    net.synchronize()
    with pytest.raises(_lib.DDQError) as ei:
        net.set_objective()
    assert ei.value.code == _lib.DDQ_ESTATE
    assert net.objective() == {"target": "double", "loss": "huber", "huber_delta": 1.0}
    assert np.isfinite(net.blob("Qn_out")).all()
    net.close()
