"""DDQ_RULE_ADAM on the CPU twin (cpu/twin.cpp) against tests/_adam_ref.py, and
_adam_ref itself against torch.optim.Adam + torch.nn.utils.clip_grad_norm_ in
float64: the formula is pinned independently of the code under test."""
import numpy as np
import pytest

import _adam_ref as ar
from _parity import close
from _twin import ddq_with_cpu_lib

S, B = 16, 8
EINVAL, ESTATE = -1, -5


@pytest.fixture(scope="module")
def ddq():
    return ddq_with_cpu_lib()


def cpu_net(ddq, seed=3):
    from ddq.params import init_params_flat
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    theta = init_params_flat(S, seed=seed)
    net.set_flat(0, theta)
    net.reset_optimizer()
    return net, theta


def code_of(call):
    from ddq import _lib
    with pytest.raises(_lib.DDQError) as ei:
        call()
    return ei.value.code


# ------------------------------------------------------------------ the formula
@pytest.mark.parametrize("clip", [0.0, 1.5])
def test_reference_is_torch_adam(clip):
    """Five steps of _adam_ref against torch in float64, to 1e-12 relative.

    clip_grad_norm_ scales by max_norm / (norm + 1e-6), the rule by
    max_norm / norm.  So that torch computes the rule's factor, it is given
    max_norm * (norm + 1e-6) / norm, with the norm torch itself reports (its
    clamp of the factor at 1 then fires exactly when norm <= max_norm, as the
    rule's does)."""
    import torch
    rng = np.random.default_rng(7)
    n, lr = 257, 1e-3
    k = dict(beta1=0.9, beta2=0.999, eps=1e-8)
    theta = rng.normal(0, 0.1, n)
    p = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(k["beta1"], k["beta2"]), eps=k["eps"])
    m = v = None
    clipped = 0
    for t in range(1, 6):
        # (norms on both sides of the threshold)
        g = rng.normal(0, 0.05 * t, n)
        p.grad = torch.tensor(g, dtype=torch.float64)
        if clip > 0:
            nrm_t = float(torch.nn.utils.clip_grad_norm_([p], float("inf")))
            torch.nn.utils.clip_grad_norm_([p], clip * (nrm_t + 1e-6) / nrm_t)
        opt.step()
        theta, m, v, nrm = ar.step(theta, g, m, v, t, lr, max_grad_norm=clip, **k)
        if clip > 0:
            assert abs(nrm - nrm_t) <= 1e-12 * nrm_t
            clipped += nrm > clip
        st = opt.state[p]
        for got, want, what in ((theta, p.detach().numpy(), "theta"),
                                (m, st["exp_avg"].numpy(), "m"), (v, st["exp_avg_sq"].numpy(), "v")):
            err = np.max(np.abs(got - want) / np.abs(want))
            assert err <= 1e-12, (what, t, err)
    if clip > 0:
        assert 0 < clipped < 5


# ------------------------------------------------------------------ the twin
def test_apply_parity(ddq):
    net, theta = cpu_net(ddq)
    net.set_adam()
    k = ar.constants()
    lr = ar.f32(1e-3)
    rng = np.random.default_rng(11)
    th, m, v = theta.astype(np.float64), None, None
    for t in range(1, 5):
        g = rng.normal(0, 1e-2, theta.size).astype(np.float32)
        net.set_grads_flat(g)
        net.apply("adam", lr=1e-3)
        th, m, v, _ = ar.step(th, g, m, v, t, lr, **k)
        gm, gv, gt = net.adam_state()
        assert gt == t
        close(net.get_flat(0), th, what="theta %d" % t)
        close(gm, m, what="m %d" % t)
        close(gv, v, what="v %d" % t)
        assert net.optimizer_state().tobytes() == gm.tobytes()
    assert net.get_adam() == {kk: float(np.float32(vv)) for kk, vv in ar.DEFAULTS.items()}
    assert code_of(lambda: net.blob("grad_norm")) == ESTATE       # clipping is off
    net.close()


def test_clipping(ddq):
    rng = np.random.default_rng(12)
    net, theta = cpu_net(ddq)
    g = rng.normal(0, 1e-2, theta.size).astype(np.float32)
    nrm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    c = ar.f32(0.5 * nrm)
    net.set_adam(max_grad_norm=c)
    net.set_grads_flat(g)
    net.apply("adam", lr=1e-3)
    got = float(net.blob("grad_norm"))
    assert abs(got - nrm) <= 2 * 2.0 ** -23 * nrm, (got, nrm)
    k = ar.constants(max_grad_norm=c)
    th, m, v, _ = ar.step(theta, g, None, None, 1, ar.f32(1e-3), **k)
    gm, gv, _ = net.adam_state()
    close(net.get_flat(0), th, what="clipped theta")
    close(gm, m, what="clipped m")            # m = (1 - beta1) s g: the scale is in it
    close(gv, v, what="clipped v")
    assert net.get_grads_flat().tobytes() == g.tobytes()          # the buffer keeps g
    net.close()
    # a threshold above the norm changes nothing, bit for bit
    out = []
    for c in (0.0, 2.0 * nrm):
        net, theta = cpu_net(ddq)
        net.set_adam(max_grad_norm=c)
        for t in range(2):
            net.set_grads_flat(g * np.float32(1 + t))
            net.apply("adam", lr=1e-3)
        out.append([net.get_flat(0).tobytes()] + [x.tobytes() for x in net.adam_state()[:2]])
        net.close()
    assert out[0] == out[1]


def test_refusals_leave_the_state(ddq):
    net, theta = cpu_net(ddq)
    g = np.full(theta.size, 1e-2, np.float32)
    net.set_grads_flat(g)
    assert code_of(lambda: net.apply("adam", lr=1e-3)) == ESTATE  # before set_adam
    assert code_of(net.get_adam) == ESTATE and code_of(net.adam_state) == ESTATE
    assert net.get_flat(0).tobytes() == theta.tobytes()
    net.set_adam(beta1=0.8, beta2=0.99, eps=1e-6, max_grad_norm=2.0)
    net.apply("adam", lr=1e-3)
    before = (net.get_adam(), net.get_flat(0).tobytes(),
              [x if isinstance(x, int) else x.tobytes() for x in net.adam_state()])
    for bad in (dict(beta1=1.0), dict(beta2=1.0), dict(beta1=-0.1), dict(eps=0.0),
                dict(eps=float("inf")), dict(max_grad_norm=-1.0),
                dict(max_grad_norm=float("nan")), dict(max_grad_norm=float("inf")),
                dict(beta2=float("nan"))):
        assert code_of(lambda: net.set_adam(**bad)) == EINVAL, bad
    after = (net.get_adam(), net.get_flat(0).tobytes(),
             [x if isinstance(x, int) else x.tobytes() for x in net.adam_state()])
    assert before == after
    assert before[0] == {k: float(np.float32(x)) for k, x in
                         dict(beta1=0.8, beta2=0.99, eps=1e-6, max_grad_norm=2.0).items()}
    net.close()


def test_reset_zeroes_m_v_t(ddq):
    net, theta = cpu_net(ddq)
    net.set_adam()
    g = np.full(theta.size, 1e-2, np.float32)
    net.set_grads_flat(g)
    net.apply("adam", lr=1e-3)
    net.apply("adam", lr=1e-3)
    m, v, t = net.adam_state()
    assert t == 2 and m.any() and v.any()
    net.reset_optimizer()
    m, v, t = net.adam_state()
    assert t == 0 and not m.any() and not v.any()
    # and the next apply is a first one again: the same bits as a fresh net's
    net.set_flat(0, theta)
    net.apply("adam", lr=1e-3)
    fresh, _ = cpu_net(ddq)
    fresh.set_adam()
    fresh.set_grads_flat(g)
    fresh.apply("adam", lr=1e-3)
    assert net.get_flat(0).tobytes() == fresh.get_flat(0).tobytes()
    assert net.adam_state()[2] == 1
    net.close()
    fresh.close()


def test_param_server_adam(ddq):
    from ddq.barista import messaging
    from ddq.param_server import ParamServer
    adam = dict(beta1=0.9, beta2=0.99, eps=1e-7, max_grad_norm=1.0)
    ps = ParamServer(frame=S, batch=B, update="adam", lr=1e-3, adam=adam, mode="cpu")
    ps.init_params(seed=5)
    theta = ps.net.get_flat(0)
    k = ar.constants(**adam)
    rng = np.random.default_rng(13)
    th, m, v = theta.astype(np.float64), None, None
    clipped = 0
    for t in range(1, 4):
        # norms about 0.7, 2.1, 6.4: on both sides of the threshold
        g = rng.normal(0, 5e-4 * 3 ** t, theta.size).astype(np.float32)
        msg = messaging.create_net_message(ps.net.split(g, "Q"), "diff")
        assert ps.update_params(msg) == b"Updated"
        th, m, v, nrm = ar.step(th, g, m, v, t, ar.f32(1e-3), **k)
        clipped += nrm > k["max_grad_norm"]
    assert ps.iteration == 3 and ps.net.adam_state()[2] == 3 and 0 < clipped < 3
    close(ps.net.get_flat(0), th, what="server model")
    ps.net.close()
    with pytest.raises(ValueError):
        ParamServer(frame=S, batch=B, update="adamw", mode="cpu")
