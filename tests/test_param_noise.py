"""Parameter-space noise (ddq_set_param_noise) on the CPU twin: the draw against
tests/_param_noise_ref.py, the adaptation and its margins, who acts on theta~,
the resample_every rule, the binding and the error table."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _param_noise_ref as pr
from oracle import ref_numpy as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    from ddq import _lib
    if not os.path.exists(_lib.CPU_LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "distributed-deep-q_amd"),
                        "ddq/_lib/libddq_cpu.so"], check=True)
    return m


@pytest.mark.parametrize("sigma", [0.01, 0.5])
@pytest.mark.parametrize("S", [16, 24])
def test_draw(ddq, S, sigma):
    net, th = pr.make_net(ddq, ref, S, B, mode="cpu")
    pr.check_draws(net, th, sigma, "twin S%d" % S)
    net.close()


@pytest.mark.parametrize("S", [16, 24])
def test_adapt_and_margins(ddq, S):
    """sigma 1e-4 / 1.0 put the mean KL more than 10 x below / above delta, on the
    reference alone and on the twin: the branch never hangs on rounding."""
    states = pr.states_of(B, S)
    net, th = pr.make_net(ddq, ref, S, B, states, mode="cpu")
    q = pr.q_oracle(ref, th, S, states)
    for sigma, epoch in ((1e-4, 1), (1.0, 1)):
        qn = pr.q_oracle(ref, th.astype(np.float64) + sigma * pr.eps(th.size, epoch), S, states)
        means = (pr.kl(q, qn).mean(), pr.check_adapt(net, ref, S, states, sigma))
        print("S%d sigma %g mean KL: reference %.3g, twin %.3g, delta %.3g" % ((S, sigma) + means + (pr.DELTA,)))
        assert all(m < pr.DELTA / 10 if sigma < 1 else m > 10 * pr.DELTA for m in means)
    net.close()


def test_consumers_and_resample_every(ddq):
    from ddq import _lib
    S = 16
    states = pr.states_of(B, S)
    net, th = pr.make_net(ddq, ref, S, B, states, mode="cpu")
    plain = net.select_action(states)
    net.forward_q()
    q = net.blob("Q_out").copy()
    net.set_param_noise(0.0, seed=pr.SEED)                  # sigma 0 acts as off
    assert np.array_equal(net.select_action(states), plain)
    assert np.array_equal(net.param_noise_params(), th)
    net.set_param_noise(0.5, seed=pr.SEED)
    net.param_noise_resample()
    net.param_noise_resample()
    e2 = net.param_noise_params()
    net.forward_q()                                         # never on theta~
    assert np.array_equal(net.blob("Q_out"), q)
    net.set_flat(0, th)                                     # writers leave theta~ alone
    assert np.array_equal(net.param_noise_params(), e2)
    net.set_param_noise(0.5, seed=pr.SEED, resample_every=3)
    for _ in range(7):                                      # resamples before moves 3 and 6
        net.select_action(states)
    assert np.array_equal(net.param_noise_params(), e2)
    net.set_param_noise(None)
    assert net.param_noise is None
    assert np.array_equal(net.select_action(states), plain)
    for call in (net.param_noise_resample, net.param_noise_adapt, net.param_noise_params,
                 lambda: net.blob("Qa_out"), lambda: net.blob("pn_kl"), lambda: net.blob("pn_sigma")):
        with pytest.raises(_lib.DDQError) as ei:
            call()
        assert ei.value.code == _lib.DDQ_ESTATE
    net.close()


def test_binding_and_error_table(ddq):
    from ddq import _lib
    assert ctypes.sizeof(_lib.ParamNoiseCfg) == 32 and _lib.ParamNoiseCfg.seed.offset == 24
    assert {"ddq_set_param_noise", "ddq_get_param_noise", "ddq_param_noise_resample_async",
            "ddq_param_noise_adapt_async", "ddq_param_noise_params"} <= set(_lib.EXPORTED)
    net = ddq.DeepQNet(batch=2, frame=16, mode="cpu")
    net.set_param_noise(0.25, delta=0.5, adapt_coef=1.5, resample_every=2, seed=9)
    on = {"sigma": 0.25, "delta": 0.5, "adapt_coef": 1.5, "resample_every": 2, "seed": 9}
    assert net.param_noise == on
    nan, inf = float("nan"), float("inf")
    good = (1, 0.25, 0.5, 1.5, 2, 0, 9)
    bad = [(0, 2), (0, -1), (5, 1), (1, -0.1), (1, nan), (1, inf), (2, 0.0), (2, -1.0), (2, nan),
           (2, inf), (3, 1.0), (3, 0.5), (3, nan), (3, inf), (4, -1)]
    for field, v in bad:
        cfg = list(good)
        cfg[field] = v
        p = _lib.ParamNoiseCfg(*cfg)
        assert net.lib.ddq_set_param_noise(net.ctx, ctypes.byref(p)) == _lib.DDQ_EINVAL, cfg
        assert net.param_noise == on
    assert net.lib.ddq_set_param_noise(net.ctx, None) == _lib.DDQ_EINVAL
    net.close()


def test_restore_turns_it_off_and_a_worker_sets_it_again(ddq, tmp_path):
    import _coherence as co
    from ddq.barista.baristanet import BaristaNet
    from ddq.replay import ReplayDataset
    S, path = 16, str(tmp_path / "worker.ckpt")

    def worker(**kw):
        net = BaristaNet({"batch": B, "frame": S}, None, None, mode="cpu",
                         param_noise={"sigma": 0.05, "seed": 3, "adapt_every": 2}, **kw)
        dset = ReplayDataset(None, (4, S, S), dset_size=64, batch_size=B, net=net.dqn, mode="cpu")
        if "resume" not in kw:
            net.dqn.replay_import(*co.ring(S, 64, 3), 0, 64)
        net.add_dataset(dset)
        return net
    a = worker()
    a.save_checkpoint(path)
    a.dqn.load_checkpoint(path)                             # the context's own restore: off
    assert a.dqn.param_noise is None
    a.dqn.close()
    b = worker(resume=path)                                 # the worker's: set again
    assert b.dqn.param_noise["sigma"] == np.float32(0.05)
    for _ in range(2):                                      # the second pass adapts
        b.load_minibatch()
        b.full_pass()
    b.dqn.synchronize()
    assert np.float32(b.dqn.param_noise["sigma"]) in (np.float32(0.05) * np.float32(1.01),
                                                      np.float32(0.05) / np.float32(1.01))
    b.dqn.close()
