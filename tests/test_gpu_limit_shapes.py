"""The full pass at the largest shapes ddq_create accepts (B = 1024 at the
largest frames), checked by an oracle that sees k images of the batch
(tests/_limit_shapes.py: all other images add exactly zero to every gradient).

Per case, on one context:
  * forward_backward through tests/_parity.check_full_pass (its rules
    unchanged): the per-image blobs and the pool routing at the live rows, the
    loss and every gradient tensor times B / k; Q_sa and target_Q_sa of the
    silent rows exactly zero;
  * the acting path's copy of the convs: forward_q's Q_out at the live rows
    under the same rule, and select_action over all B states against it;
  * one rmsprop update from the device's own gradient against
    ref.rmsprop_update, as test_gpu_parity.test_apply_rules_parity holds it;
  * the coherence probe (tests/_coherence.py) on the updated context.

CASES: the corner of the domain, B S^2 = 2^24 (the other parity suites reach
2^22); the largest frame with odd maps (60 / 30 / 15: partial edge tiles in
every layer) at B = 1024; and a frame whose third map is odd (36 / 18 / 9).
Wall times on an MI355X: 4.8, 4.9 and 2.7 s, of which the oracle 1.8, 1.4 and
0.3 s (each case prints its own).

The former domain's larger shapes -- (256 .. 360, 1024), (1016, 128), where
fp32 pool1 and the split dpool2 planes pass 2^31 bytes -- are not here:
ddq_create refuses frames past 128, which the backward pass never could run
(tests/test_limit_shapes.py keeps their arithmetic).
"""
import time

import numpy as np
import pytest

import _coherence as co
import _limit_shapes as ls
from _parity import check_full_pass, close, full_pass_reference

pytestmark = pytest.mark.gpu

# (S, B, k, frames)
CASES = [(128, 1024, 8, "uniform"), (120, 1024, 8, "snake"), (72, 1024, 4, "uniform")]


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


@pytest.mark.parametrize("S,B,k,frames", CASES)
def test_limit_shape(ddq, ref, S, B, k, frames):
    t0 = time.perf_counter()
    c = ls.make_case(ref, S, B, k, frames)
    silent = np.setdiff1d(np.arange(B), c.live)
    net = ddq.DeepQNet(batch=B, frame=S)
    try:
        ls.bind(net, c)
        loss = net.forward_backward()
        assert loss == float(net.blob("loss"))
        view = ls.LiveRows(net, c.live)
        g = view.get_grads_flat()
        t1 = time.perf_counter()
        oracle = full_pass_reference(ref, view, c.pQ, c.pP, c.mb, g)
        t_oracle = time.perf_counter() - t1
        what = "(%d, %d) " % (S, B)
        blobs, _, nties = check_full_pass(ref, view, c.pQ, c.pP, c.mb, grads_gpu=g, what=what,
                                          reference=oracle)
        print("near-tie routings adopted: %d" % nties)
        for name in ("Q_sa", "P_sa", "target_Q_sa"):
            assert not net.blob(name).ravel()[silent].any(), name

        # the acting forward over the same B states
        q_train = net.blob("Q_out").reshape(B, 4)
        net.forward_q()
        q_act = net.blob("Q_out").reshape(B, 4)
        close(q_act[c.live], blobs["Q_out"], what=what + "acting Q_out", mag=oracle[3]["Q_out"],
              tensor="Q_out")
        assert np.isfinite(q_act).all() and not q_act[:, 3].any()
        actions = net.select_action(c.ring[0][:B])
        np.testing.assert_array_equal(actions, np.argmax(q_act, axis=1))
        print("%sacting vs training Q_out: max |d| %.3g" % (what, np.abs(q_act - q_train).max()))

        # one rmsprop update from the device's own gradient
        th0, g_raw = net.get_flat(0), net.get_grads_flat()
        net.reset_optimizer()
        net.apply("rmsprop", lr=1e-3)
        th, state = ref.rmsprop_update(th0, g_raw, None, 1e-3, 0.9)
        close(net.get_flat(0), th, what=what + "theta after rmsprop")
        close(net.optimizer_state(), state, what=what + "rmsprop state")
        assert not np.array_equal(net.get_flat(0), th0)

        # the derived weight copies after that update
        st = c.ring[0]
        act = np.zeros((B, 4, 1, 1), np.float32)
        act[np.arange(B), c.ring[1][1:]] = 1
        mb = (st[:B].astype(np.float32), act, c.ring[2][1:].astype(np.float32),
              st[1:].astype(np.float32), c.ring[3][1:].astype(np.float32))
        got, want = co.probe(ddq, net, mb, st[1:])
        co.assert_coherent(got, want, what + "after one rmsprop update")
    finally:
        net.close()
    print("%swall %.1f s, of which the oracle %.1f s" % (what, time.perf_counter() - t0, t_oracle))
