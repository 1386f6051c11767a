"""Parameter-space noise on the device (csrc/param_noise.hip): the one-launch draw
against tests/_param_noise_ref.py, the split copies through the acting forward,
the distance / adaptation launch, who acts on theta~, and off left bit for bit."""
import numpy as np
import pytest

import _actor_host as ah
import _param_noise_ref as pr
from oracle import ref_numpy as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.mark.parametrize("sigma", [0.01, 0.5])
@pytest.mark.parametrize("S", [16, 24])
def test_draw(ddq, S, sigma):
    net, th = pr.make_net(ddq, ref, S, 4)
    pr.check_draws(net, th, sigma, "S%d" % S)
    net.close()


@pytest.mark.parametrize("sigma", [1e-4, 1.0])
@pytest.mark.parametrize("S,B", [(16, 4), (24, 4), (24, 1)])
def test_adapt(ddq, S, B, sigma):
    """Qa_out on the oracle's forward of theta~ (a wrong wks~ layout -- conv1's zero
    tap, the tap order, a plane -- shows here), pn_kl, sigma's step, select_action."""
    states = pr.states_of(B, S)
    net, _ = pr.make_net(ddq, ref, S, B, states)
    assert net.small_path()[0] == (S == 16)
    pr.check_adapt(net, ref, S, states, sigma)
    net.close()


def run_actor(net, S, moves=32):
    from ddq.actor import zoom_maps
    rm, cm = zoom_maps((S, S), S)
    net.replay_create(ah.CAPACITY)
    net.actor_create(ah.init_boards()["coiled"], rm, cm, 77)
    net.actor_step(moves, 60000)
    boards, stats = net.actor_read()
    ring = net.replay_export()
    net.step(net.step_cfg("rmsprop", lr=1e-4, target_period=10, seed=5))
    net.synchronize()
    return [boards, stats, *ring, net.get_flat(0)]


@pytest.mark.parametrize("S", [16, 24])
def test_off_and_sigma_zero_are_untouched(ddq, S):
    want = None
    for how in ("untouched", "zero", "disabled"):
        net, _ = pr.make_net(ddq, ref, S, 4)
        if how != "untouched":
            net.set_param_noise(0.0 if how == "zero" else 0.5, seed=pr.SEED, resample_every=5)
        if how == "disabled":
            net.set_param_noise(None)
        got = run_actor(net, S)
        net.close()
        want = want or got
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), how


@pytest.mark.parametrize("S", [16, 24])
def test_who_acts_on_it(ddq, S, tmp_path):
    from ddq.actor import zoom_maps
    rm, cm = zoom_maps((S, S), S)
    states = pr.states_of(4, S)
    init = np.stack([ah.init_boards()[k] for k in ("start", "coiled")])
    out = []
    for on in (False, True):
        net, _ = pr.make_net(ddq, ref, S, 4, states)
        if on:
            net.set_param_noise(0.5, seed=pr.SEED)
        net.forward_q()
        net.eval_create(init, rm, cm, 5, max_moves=8, max_episodes=4)
        net.eval_run(24)
        ev = net.eval_read()
        out.append([net.blob("Q_out"), ev["log"], ev["boards"], ev["stats"]])
        if on:                                              # resample_every: before moves 3 and 6
            net.param_noise_resample()
            net.param_noise_resample()
            e2 = net.param_noise_params()
            net.set_param_noise(0.5, seed=pr.SEED, resample_every=3)
            for _ in range(7):
                net.select_action(states)
            assert np.array_equal(net.param_noise_params(), e2)
            net.replay_create(ah.CAPACITY)                  # a restore turns it off
            net.save_checkpoint(str(tmp_path / "net.ckpt"))
            net.load_checkpoint(str(tmp_path / "net.ckpt"))
            assert net.param_noise is None
        net.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out))

