"""Munchausen / soft-Q target on the device (ddq_set_munchausen): the P(s,.) pass,
the Munchausen build of both heads, eager and graph-captured, against
tests/_munchausen_ref.py under tests/_parity.py's bounds; no extra launch at
alpha 0; off left bit for bit; composition with Huber, n-step and prioritized
replay.  Each case's inputs meet the conditions asserted on the reference alone."""
import numpy as np
import pytest

import _munchausen_ref as mr
import _nstep_ref as nr
import _objective_ref as objr
from _parity import NORM_RTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


def ring_net(ddq, c, S, B, n=None, prio=None):
    """A net on the case's parameters with mr.ring_for(S) imported from the host."""
    net = ddq.DeepQNet(batch=B, frame=S)
    params = dict(c["pQ"])
    params.update(c["pP"])
    net.set_params(params)
    ring = mr.ring_for(S)
    net.replay_create(mr.RING_N)
    net.replay_import(*ring, 0, mr.RING_N)
    if n is not None:
        net.replay_set_nstep(n)
    if prio is not None:
        net.replay_set_priority(**prio)
    return net


def step_cfg(net, period=5):
    """period 0: no target sync, so the first step does not begin with P <- Q."""
    return net.step_cfg("sgd", lr=1e-6, target_period=period, seed=mr.STEP_SEED)


def code_of(call):
    from ddq import _lib
    with pytest.raises(_lib.DDQError) as ei:
        call()
    return ei.value.code


@pytest.mark.parametrize("alpha", [0.0, 0.9])
@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("key", mr.CASES)
def test_parity(ddq, ref, key, mode, alpha):
    from ddq import _lib
    S, B, _ = key
    c = mr.case(ref, *key, drawn=mode == "graph")
    o = mr.oracle_head(ref, c, alpha)               # the conditions, on the reference alone
    if mode == "eager":
        net = objr.make_net(ddq, c)
        net.set_munchausen(alpha, **c["cfg"])
        net.forward_backward()
    else:                                           # one graph-captured step on the ring
        net = ring_net(ddq, c, S, B)
        net.set_munchausen(alpha, **c["cfg"])
        net.step_graph(step_cfg(net, 0), 1)
        net.synchronize()
        nr.assert_minibatch(net.read_minibatch(), c["mb"])
    assert net.small_path()[0] == (S == 16)
    what = "%s %s a=%g " % (key, mode, alpha)
    if alpha:
        pc = net.blob("Pc_out").reshape(B, 4).astype(np.float64)
        err = np.linalg.norm(pc - c["Pc"]) / np.linalg.norm(c["Pc"])
        print("%sPc_out normwise %.3g" % (what, err))
        assert err <= NORM_RTOL
    else:
        assert code_of(lambda: net.blob("Pc_out")) == _lib.DDQ_ESTATE
    mr.check_head(net, c["mb"], ref.GAMMA, alpha, what=what, **c["cfg"])
    mr.check_grads(ref, net, c, o["Q_sa"] - o["target"], what=what)
    net.close()


@pytest.mark.parametrize("S", [16, 24])
def test_alpha_zero_launches_no_extra_pass(ddq, ref, S):
    c = mr.case(ref, S, 4 if S == 16 else 3, 901, drawn=True)
    net = ring_net(ddq, c, S, len(c["mb"][0]))
    cfg = step_cfg(net)
    plain = [n for n, _ in net.profile_step(cfg)]
    net.set_munchausen(0.0, **c["cfg"])
    assert [n for n, _ in net.profile_step(cfg)] == plain
    net.set_munchausen(0.9, **c["cfg"])
    names = [n for n, _ in net.profile_step(cfg)]
    extra = [n for n in names if n.startswith("pc_")]
    print(names)
    assert len(extra) >= 2 and [n for n in names if not n.startswith("pc_")] == plain
    first = names.index(extra[0])                   # one group, ahead of the step's forward
    assert names[first:first + len(extra)] == extra
    assert first + len(extra) <= names.index("tower_fwd" if S == 16 else "conv1_fwd")
    net.close()


@pytest.mark.parametrize("key", mr.CASES)
def test_off_is_untouched(ddq, ref, key):
    c = mr.case(ref, *key)
    names = ("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss", "Q_out.diff")
    fresh = objr.make_net(ddq, c)
    fresh.forward_backward()
    b0, g0 = objr.blobs_of(fresh, names), fresh.get_grads_flat()
    net = objr.make_net(ddq, c)
    net.set_munchausen(0.9, **c["cfg"])
    net.forward_backward()
    assert net.get_grads_flat().tobytes() != g0.tobytes()
    net.set_munchausen(None)
    net.forward_backward()
    b1 = objr.blobs_of(net, names)
    assert net.get_grads_flat().tobytes() == g0.tobytes()
    for k in names:
        assert b1[k].tobytes() == b0[k].tobytes(), k
    fresh.close()
    net.close()


@pytest.mark.parametrize("key", [mr.CASES[0], mr.CASES[2]])
def test_small_tau_is_the_hard_max(ddq, ref, key):
    """expf underflows to 0 below -103.98 (2^-150, under half the smallest fp32
    denormal): with every gap of P' to its maximum above 104 tau the sum is
    expf(0) alone, lse' = logf(1) = 0 and V' = m' exactly.  The P tower's Q_out
    bias is spread to steps of 40 (the x3 fillers' P' stay within +-15), tau 0.1."""
    c = dict(mr.case(ref, *key))
    name = [k for k in c["pP"] if k.endswith("_out")][0]
    bias = np.asarray([0.0, 40.0, 80.0, 120.0], np.float32).reshape(c["pP"][name][1].shape)
    c["pP"] = dict(c["pP"], **{name: [c["pP"][name][0], bias]})
    net = objr.make_net(ddq, c)
    net.forward_backward()
    top = np.sort(objr.blobs_of(net)["P_out"].astype(np.float64), axis=1)
    tau = 0.1
    assert np.min(top[:, -1] - top[:, -2]) / tau > 104
    p_max = net.blob("P_sa")
    net.set_munchausen(0.0, tau, -1.0)
    net.forward_backward()
    assert net.blob("P_sa").tobytes() == p_max.tobytes() and p_max.any()
    net.close()


def test_composition_huber_nstep_prioritized(ddq, ref):
    S, B, n = 16, 4, 3
    c = mr.case(ref, S, B, 901)
    cfg_m = mr.CFG[True]
    nets = []
    for _ in range(2):
        net = ring_net(ddq, c, S, B, n=n, prio=dict(alpha=0.6, beta=0.4, eps=0.01))
        net.set_objective("max", "huber", 1.0)
        net.set_munchausen(0.9, **cfg_m)
        nets.append(net)
    eager, graph = nets
    cfg = step_cfg(eager)
    th0 = eager.get_flat(0)
    eager.step(cfg)
    eager.synchronize()
    mb = eager.read_minibatch()                     # the gathered R and w
    assert len(set(mb[4].reshape(-1).tolist())) > 1 and (mb[4] < 1).all()
    mr.check_head(eager, mb, ref.GAMMA, 0.9, diff=False, what="n3 ", **cfg_m)
    eager.step(cfg)
    eager.step(cfg)
    graph.step_graph(cfg, 3)
    for net in nets:
        net.synchronize()
    for z in (0, 1):
        assert eager.get_flat(z).tobytes() == graph.get_flat(z).tobytes()
    assert eager.get_flat(0).tobytes() != th0.tobytes()
    for net in nets:
        net.close()
