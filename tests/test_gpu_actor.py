"""The device-resident Snake actor (csrc/actor.h, ddq_actor_*) on the GPU.

* Bit identity with the host loop (tests/_actor_host.py: unmodified ``ExpGain`` +
  ``SnakeGame.cpu_play`` on ``ActorRng(seed)``, ``ReplayRef`` ring) on two
  contexts holding identical parameters: the device actor on one, the host
  loop's ``select_action`` on the other.  Both run the same forward kernels at
  n = 1, so the Q values, hence every decision, are expected to be equal; no
  tolerance.  S = 16 (small-map ctx) and S = 24 (general kernels), B = 4,
  capacity 37, 200 steps at epsilon(0), epsilon(60000) and the knee ramp;
  S = 40 and S = 64 once each at epsilon(60000).  That forward itself is held
  to the float64 oracle by tests/test_gpu_acting.py.
* The sampler sees the device adds without a synchronise; the host mirror of
  head / valid follows them.
* ``act_and_step``: acting interleaved with graph training steps.
"""
import numpy as np
import pytest

import _actor_host as ah

pytestmark = pytest.mark.gpu

B, STEPS = 4, 200
CASES = [(16, "eps1", "coiled"), (16, "eps01", "start"), (16, "ramp", "apple_ahead"),
         (24, "eps1", "apple_ahead"), (24, "eps01", "coiled"), (24, "ramp", "start"),
         # past S = 24 (general kernels; tests/test_gpu_acting.py holds their Q
         # values to the oracle): a frame with partial edge tiles, the bench's own
         (40, "eps01", "start"), (64, "eps01", "coiled")]


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


def make_net(ddq, S, ring=True, theta=None):
    net = ddq.DeepQNet(batch=B, frame=S)
    th = ah.seeded_theta(S) if theta is None else theta
    net.set_flat(0, th)
    net.set_flat(1, th)
    if ring:
        net.replay_create(ah.CAPACITY)
    return net


@pytest.mark.parametrize("S,reg,bn", CASES, ids=["%d-%s-%s" % c for c in CASES])
def test_device_actor_equals_host_loop(ddq, S, reg, bn):
    from ddq.actor import DeviceActor
    init = ah.init_boards()[bn]
    seed = 101 + CASES.index((S, reg, bn))
    iters = [ah.REGIMES[reg](k) for k in range(STEPS)]
    dev, hostnet = make_net(ddq, S), make_net(ddq, S, ring=False)
    assert dev.small_path()[0] == (S == 16)
    actor = DeviceActor(dev, init, seed)
    if reg == "ramp":
        for it in iters:
            actor.generate_experience(it)
    else:
        dev.actor_step(3, iters[0])
        dev.actor_step(STEPS - 3, iters[0])
    host = ah.HostLoop(hostnet, init, seed, S)
    host.run(iters)
    ah.assert_same(dev, host)
    assert host.counts["games"] >= 1
    dev.synchronize()
    hostnet.synchronize()
    dev.close()
    hostnet.close()


@pytest.mark.parametrize("S", [16, 24])
def test_sampler_sees_device_adds(ddq, S):
    from ddq.actor import DeviceActor
    init = ah.init_boards()["start"]
    dev, hostnet = make_net(ddq, S), make_net(ddq, S, ring=False)
    DeviceActor(dev, init, 7)
    dev.actor_step(40, 0)
    # no synchronise: the draw reads the device head / valid the actor advanced
    dev.replay_sample_device(13)
    idx = dev.read_indices()
    host = ah.HostLoop(hostnet, init, 7, S)
    host.run([0] * 40)
    head, valid, cap = dev.replay_info()
    assert (head, valid, cap) == (host.ring.head, host.ring.valid, ah.CAPACITY) == (3, 37, 37)
    assert idx.shape == (B,) and (np.diff(idx) > 0).all()
    assert idx.min() >= 0 and idx.max() < ah.CAPACITY and (head - 1) not in idx
    # the gathered minibatch is the ring's, as the oracle gathers it
    want = host.ring.gather(idx)
    for g, w in zip(dev.read_minibatch(), want):
        np.testing.assert_array_equal(g, w.reshape(g.shape))
    ah.assert_same(dev, host)
    dev.synchronize()
    hostnet.synchronize()
    dev.close()
    hostnet.close()


@pytest.mark.parametrize("S", [16, 24])
def test_act_and_step(ddq, S):
    from ddq.actor import DeviceActor
    from ddq.params import init_params_flat
    # the prototxt fillers: with the bit-identity tests' scaled-up weights the
    # reference's lagged-cache rmsprop (server.py:86-105) diverges within five
    # updates on any implementation (a gradient that is zero in one step and
    # not in the next is divided by sqrt(eps))
    dev = make_net(ddq, S, theta=init_params_flat(S, seed=42))
    actor = DeviceActor(dev, ah.init_boards()["start"], 21)
    actor.fill(20)
    cfg = dev.step_cfg("rmsprop", lr=1e-4, target_period=10, seed=5)
    theta0 = dev.get_flat(0)
    steps0, (head0, valid0, _) = dev.lib.ddq_step_count(dev.ctx), dev.replay_info()
    actor.act_and_step(cfg, 5, 0)
    dev.synchronize()
    assert dev.lib.ddq_step_count(dev.ctx) == steps0 + 5
    head, valid, cap = dev.replay_info()
    assert (head, valid) == ((head0 + 5) % cap, min(cap, valid0 + 5)) == (25, 25)
    dev._check(dev.lib.ddq_replay_status(dev.ctx))
    st = actor.stats()
    assert st["steps"] == 25
    theta = dev.get_flat(0)
    assert np.isfinite(theta).all() and (theta != theta0).any()
    # the last step drew from the ring the acts had filled: 25 valid slots
    idx = dev.read_indices()
    assert idx.max() < 25 and (head - 1) not in idx
    dev.synchronize()
    dev.close()


def test_argument_errors(ddq):
    from ddq import _lib
    from ddq.actor import zoom_maps
    S = 16
    net = make_net(ddq, S, ring=False)
    rm, cm = zoom_maps((S, S), S)
    good = ah.init_boards()["start"]

    def code(fn, *a):
        with pytest.raises(_lib.DDQError) as ei:
            fn(*a)
        return ei.value.code

    assert code(net.actor_create, good, rm, cm, 1) == _lib.DDQ_ESTATE     # no ring
    assert code(net.actor_step, 1, 0) == _lib.DDQ_ESTATE
    net.replay_create(8)
    assert code(net.actor_step, 1, 0) == _lib.DDQ_ESTATE                   # no actor
    bad = rm.copy()
    bad[5] = 10
    assert code(net.actor_create, good, bad, cm, 1) == _lib.DDQ_EINVAL
    assert code(net.actor_create, good, rm, -bad, 1) == _lib.DDQ_EINVAL
    far = ah.board([(6, 5), (4, 5)], (0, 0))
    gap = ah.board([(6, 5)], (0, 0))
    gap[5, 5] = 2
    for b in (far, gap, np.full((10, 10), -1)):
        assert code(net.actor_create, b, rm, cm, 1) == _lib.DDQ_EINVAL
    p = _lib.ptr
    b8 = np.ascontiguousarray(good, np.int8)
    assert net.lib.ddq_actor_create(net.ctx, None, p(rm), p(cm), 1) == _lib.DDQ_EINVAL
    assert net.lib.ddq_actor_create(net.ctx, p(b8), None, p(cm), 1) == _lib.DDQ_EINVAL
    assert net.lib.ddq_actor_create(None, p(b8), p(rm), p(cm), 1) == _lib.DDQ_EINVAL
    net.actor_create(good, rm, cm, 1)
    assert code(net.actor_step, 0, 0) == _lib.DDQ_EINVAL
    boards, stats = net.actor_read()
    assert (boards == good).all() and list(stats) == [0, 0, 0, 0]
    assert net.replay_info()[:2] == (0, 0)
    net.synchronize()
    net.close()
