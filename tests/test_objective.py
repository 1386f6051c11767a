"""Selectable TD objective (ddq_set_objective) on the CPU twin: the binding, the
error cases, the head's semantics from its own blobs, the wide band, oracle
parity of {DOUBLE, HUBER}, and the worker's --double-q / --huber-delta round.
The twin sums in double and rounds once, so where the GPU suite
(test_gpu_objective.py) asks "bit for bit" of fp32 arithmetic, these tests use
the full-pass rule of test_cpu_twin.py (tests/_parity.py ``close``).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _objective_ref as objr
from _parity import close
from oracle import ref_numpy as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    from ddq import _lib
    if not os.path.exists(_lib.CPU_LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "distributed-deep-q_amd"),
                        "ddq/_lib/libddq_cpu.so"], check=True)
    return m


_RUNS = {}


def run(ddq, key):
    """One {DOUBLE, HUBER} pass of a case on the twin (kept open, not changed)."""
    if key not in _RUNS:
        c = objr.case(ref, *key)
        net = objr.make_net(ddq, c, mode="cpu")
        net.set_objective("double", "huber", c["o"]["delta"])
        loss = net.forward_backward()
        names = ("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss", "Q_out.diff", "Qn_out")
        _RUNS[key] = dict(c=c, net=net, loss=loss, got=objr.blobs_of(net, names),
                          grads=net.get_grads_flat())
    return _RUNS[key]


def test_objective_struct_and_binding(ddq):
    from ddq import _lib
    assert ctypes.sizeof(_lib.Objective) == 16
    assert {"ddq_set_objective", "ddq_get_objective"} <= set(_lib.EXPORTED)
    assert _lib.TARGETS == {"max": 0, "double": 1} and _lib.LOSSES == {"euclidean": 0, "huber": 1}
    net = ddq.DeepQNet(batch=2, frame=16, mode="cpu")
    assert net.objective() == {"target": "max", "loss": "euclidean", "huber_delta": 0.0}
    net.set_objective("double", "huber", 0.25)
    assert net.objective() == {"target": "double", "loss": "huber", "huber_delta": 0.25}
    net.set_objective(loss="huber")
    assert net.objective() == {"target": "max", "loss": "huber", "huber_delta": 1.0}
    net.set_objective()
    assert net.objective() == {"target": "max", "loss": "euclidean", "huber_delta": 0.0}
    net.close()


def test_error_cases(ddq):
    from ddq import _lib
    net = ddq.DeepQNet(batch=2, frame=16, mode="cpu")
    net.set_objective("double", "huber", 0.5)
    bad = [(2, 0, 0.0, 0), (-1, 0, 0.0, 0), (0, 2, 1.0, 0), (0, -1, 1.0, 0), (0, 1, 0.0, 0),
           (0, 1, -1.0, 0), (1, 1, float("nan"), 0), (1, 1, float("inf"), 0), (0, 0, 0.0, 1),
           (1, 1, 1.0, -3)]
    for t, l, d, r in bad:
        o = _lib.Objective(t, l, d, r)
        assert net.lib.ddq_set_objective(net.ctx, ctypes.byref(o)) == _lib.DDQ_EINVAL, (t, l, d, r)
        assert net.objective() == {"target": "double", "loss": "huber", "huber_delta": 0.5}
    assert net.lib.ddq_set_objective(net.ctx, None) == _lib.DDQ_EINVAL
    with pytest.raises(ValueError):
        net.set_objective(target="triple")
    with pytest.raises(ValueError):
        net.set_objective(loss="l1")
    # the band is ignored (and need not be finite) without HUBER
    o = _lib.Objective(1, 0, float("nan"), 0)
    assert net.lib.ddq_set_objective(net.ctx, ctypes.byref(o)) == _lib.DDQ_OK
    assert net.blob("Qn_out").shape == (2, 4, 1, 1)
    net.set_objective("max", "huber", 2.0)
    with pytest.raises(_lib.DDQError) as ei:
        net.blob("Qn_out")
    assert ei.value.code == _lib.DDQ_ESTATE
    assert net.blob("Q_out.diff").shape == (2, 4, 1, 1)
    with pytest.raises(_lib.DDQError) as ei:
        out = np.empty(3, np.float32)
        net._check(net.lib.ddq_read_blob(net.ctx, b"Q_out.diff", _lib.ptr(out), 3))
    assert ei.value.code == _lib.DDQ_EINVAL
    net.close()


@pytest.mark.parametrize("key", objr.CPU_CASES)
def test_target_from_the_blobs(ddq, key):
    r = run(ddq, key)
    o, got = r["c"]["o"], r["got"]
    e = objr.expected_head_f32(got, o["act"], o["nt"], o["r"], ref.GAMMA, "double", o["delta"])
    np.testing.assert_array_equal(got["P_sa"], e["P_sa"])
    ulp = np.spacing(np.abs(e["target64"]).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got["target_Q_sa"].astype(np.float64) - e["target64"]) <= ulp)
    # the double target is not the max target on these inputs
    assert np.any(got["P_sa"] != got["P_out"].max(axis=1) * o["nt"].astype(np.float32))


@pytest.mark.parametrize("key", objr.CPU_CASES)
def test_dq_and_loss_from_the_blobs(ddq, key):
    r = run(ddq, key)
    o, got = r["c"]["o"], r["got"]
    B = o["B"]
    e = objr.expected_head_f32(got, o["act"], o["nt"], o["r"], ref.GAMMA, "double", o["delta"])
    mag = o["act"] * ((np.abs(got["Q_sa"]) + np.abs(got["target_Q_sa"])) / B)[:, None]
    close(got["Q_out.diff"], e["dQ"], what="Q_out.diff", mag=mag)
    clipped = np.abs(e["d"]) > o["delta"]
    assert clipped.sum() == B // 2
    np.testing.assert_allclose(float(got["loss"][0]), e["loss"], rtol=1e-4)
    assert r["loss"] == float(got["loss"][0])


@pytest.mark.parametrize("key", objr.CPU_CASES)
def test_wide_band_is_the_euclidean_loss(ddq, key):
    c = objr.case(ref, *key)
    net = objr.make_net(ddq, c, mode="cpu")
    names = ("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss", "Q_out.diff", "Qn_out")
    net.set_objective("double", "euclidean")
    net.forward_backward()
    b0, g0 = objr.blobs_of(net, names), net.get_grads_flat()
    d = b0["Q_sa"] - b0["target_Q_sa"]
    net.set_objective("double", "huber", 2.0 * float(np.max(np.abs(d))))
    net.forward_backward()
    b1, g1 = objr.blobs_of(net, names), net.get_grads_flat()
    assert g0.tobytes() == g1.tobytes()
    for k in names:
        assert b0[k].tobytes() == b1[k].tobytes(), k
    # and the narrow band of the case is not
    assert g0.tobytes() != run(ddq, key)["grads"].tobytes()
    net.close()


@pytest.mark.parametrize("key", objr.CPU_CASES)
def test_oracle_parity_double_huber(ddq, key):
    r = run(ddq, key)
    counts = objr.check_objective_pass(ref, r["net"], r["c"], r["c"]["o"], what="%s " % (key,))
    print("head tensors, elements >= 1e-2 of max (held to rtol 1e-4): Q_out W %d, b %d"
          % (counts["Q_out[0]"], counts["Q_out[1]"]))


def test_worker_flags_select_the_objective(ddq, tmp_path):
    """--double-q / --huber-delta reach the net in --mode cpu; one training step
    (full pass + apply) under them changes theta."""
    from ddq.barista import main as bm
    from ddq.barista.baristanet import BaristaNet
    base = ["arch", "none", "--mode", "cpu", "--driver", "None", "--overwrite",
            "--dset-size", "24", "--initial-replay", "12"]
    want = {(): {"target": "max", "loss": "euclidean", "huber_delta": 0.0},
            ("--double-q",): {"target": "double", "loss": "euclidean", "huber_delta": 0.0},
            ("--huber-delta", "0.5"): {"target": "max", "loss": "huber", "huber_delta": 0.5},
            ("--double-q", "--huber-delta", "0.5"):
                {"target": "double", "loss": "huber", "huber_delta": 0.5}}
    for i, (extra, obj) in enumerate(want.items()):
        args = bm.get_args(base + list(extra) + ["--dataset", str(tmp_path / ("r%d.hdf5" % i))])
        assert args.double_q == ("--double-q" in extra)
        assert bm.objective_of(args) == (None if not extra else
                                         {k: v for k, v in obj.items()
                                          if k != "huber_delta" or obj["loss"] == "huber"})
        if i not in (0, 3):
            continue
        args.architecture = {"batch": 4, "frame": 16}
        net, replay, xp = bm.build_worker(args)
        assert net.dqn.objective() == obj
        it = net.fetch_model()
        xp.generate_experience(it)
        net.load_minibatch()
        before = net.dqn.get_flat(0)
        net.full_pass()
        assert np.any(net.dqn.get_grads_flat() != 0)
        net.dqn.apply("rmsprop", lr=1e-3)
        assert np.any(net.dqn.get_flat(0) != before)
        if i == 3:
            assert net.dqn.blob("Qn_out").shape == (4, 4, 1, 1)
        replay.close()
    with pytest.raises(SystemExit):
        bm.get_args(base + ["--huber-delta", "0"])
    net = BaristaNet({"batch": 2, "frame": 16}, None, None, mode="cpu",
                     objective={"target": "double", "loss": "huber", "huber_delta": 0.75})
    assert net.dqn.objective() == {"target": "double", "loss": "huber", "huber_delta": 0.75}
