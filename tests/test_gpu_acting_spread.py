"""The spread acting forward (csrc/act_spread.h, ``set_acting_path("spread")``)
on the GPU, by the recipe of tests/_acting_ref.py: values against the float64
oracle, an image's row independent of the batch around it, spread against
batch, the device actor against the host loop, and the setting itself."""
import numpy as np
import pytest

import _acting_ref as ar
import _actor_host as ah
from _parity import NORM_RTOL

pytestmark = pytest.mark.gpu

# (S, n, kind): 24 -- maps 24 / 12 / 6, ragged tiles in every layer; 40 -- maps
# 20 / 10; 64 -- the tuned shape; 120 -- maps 60 / 30, pool3 15 x 15; 128 -- the
# limit frame; (24, 33) -- many images, fc4's switch after 32
VALUES = [(24, 1, "s"), (24, 3, "u"), (40, 3, "s"), (64, 1, "u"), (64, 3, "u"), (120, 3, "s"),
          (128, 2, "u"), (24, 33, "s")]


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


def spread_net(ddq, B, S, params, path="spread"):
    net = ar.make_net(ddq, B, S, params)
    net.set_acting_path(path)
    assert net.acting_path == path
    return net


def q_of(net, states):
    net.write_minibatch(state=states)
    net.forward_q()
    return ar.q_out(net)


@pytest.mark.parametrize("S,n,kind", VALUES, ids=ar.ids(VALUES))
def test_values(ddq, ref, S, n, kind):
    c = ar.case(ref, S, n, kind, mags=True)
    net = spread_net(ddq, n, S, c["pQ"])
    err = ar.forward_values(net, c, what="spread (%d, %d, %s) " % (S, n, kind))
    print("spread parity | %d | %d | %s | %.3g |" % (S, n, kind, err))
    net.close()


@pytest.mark.parametrize("S,B,n", [(24, 8, 3), (64, 8, 1)])
def test_row_independent_of_batch(ddq, ref, S, B, n):
    c = ar.case(ref, S, n, "u")
    small, big = spread_net(ddq, n, S, c["pC"]), spread_net(ddq, B, S, c["pC"])
    q = q_of(small, c["states"])
    a_n = small.select_action(c["states"])
    mixed = ar.other_states(S, B, n)
    big.select_action(mixed)                       # the scratch holds another batch
    a_b = big.select_action(c["states"])
    mixed[:n] = c["states"]
    np.testing.assert_array_equal(q_of(big, mixed)[:n].view(np.uint32), q.view(np.uint32))
    np.testing.assert_array_equal(a_n, ar.first_max(q))
    np.testing.assert_array_equal(a_b, a_n)
    ar.check_decided(a_b, c)
    small.close()
    big.close()


@pytest.mark.parametrize("S,n", [(24, 3), (64, 3)])
def test_spread_against_batch(ddq, ref, S, n):
    c = ar.case(ref, S, n, "u")
    net = ar.make_net(ddq, n, S, c["pC"])
    q, a = {}, {}
    for path in ("batch", "spread"):
        net.set_acting_path(path)
        q[path] = q_of(net, c["states"]).astype(np.float64)
        a[path] = net.select_action(c["states"])
    diff = np.linalg.norm((q["spread"] - q["batch"]).ravel()) / np.linalg.norm(c["Qc"].ravel())
    print("spread vs batch (%d, %d): %.3g" % (S, n, diff))
    assert diff <= 2 * NORM_RTOL
    dec = c["decided"]
    np.testing.assert_array_equal(a["spread"][dec], a["batch"][dec])
    net.close()


def test_device_actor_equals_host_loop(ddq):
    from ddq.actor import DeviceActor
    S, steps, seed = 24, 50, 211
    init, th = ah.init_boards()["coiled"], ah.seeded_theta(24)
    nets = []
    for ring in (True, False):
        net = ddq.DeepQNet(batch=4, frame=S)
        net.set_flat(0, th)
        net.set_flat(1, th)
        if ring:
            net.replay_create(ah.CAPACITY)
        net.set_acting_path("spread")
        nets.append(net)
    dev, hostnet = nets
    DeviceActor(dev, init, seed)
    dev.actor_step(steps, 60000)
    host = ah.HostLoop(hostnet, init, seed, S)
    host.run([60000] * steps)
    ah.assert_same(dev, host)
    dev.close()
    hostnet.close()


def test_off_is_off(ddq, ref):
    c = ar.case(ref, 24, 3, "u")
    plain, toggled = ar.make_net(ddq, 3, 24, c["pQ"]), ar.make_net(ddq, 3, 24, c["pQ"])
    assert plain.acting_path == "batch"
    toggled.set_acting_path("spread")
    toggled.set_acting_path("batch")
    np.testing.assert_array_equal(q_of(toggled, c["states"]).view(np.uint32),
                                  q_of(plain, c["states"]).view(np.uint32))
    plain.close()
    toggled.close()


@pytest.mark.parametrize("n,same", [(1, "spread"), (65, "batch")])
def test_auto(ddq, ref, n, same):
    """n = 1 is below every crossover of kernels.hip act_spread_max_n, 65 above."""
    c = ar.case(ref, 24, n, "s" if n == 1 else "u")
    q = {}
    for path in ("auto", same):
        net = spread_net(ddq, n, 24, c["pQ"], path)
        q[path] = q_of(net, c["states"])
        net.close()
    np.testing.assert_array_equal(q["auto"].view(np.uint32), q[same].view(np.uint32))
