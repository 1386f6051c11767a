"""Munchausen / soft-Q target (ddq_set_munchausen) on the CPU twin: the binding,
the error table, the exclusion of the double target in both directions, the two
blobs, and one pass against tests/_munchausen_ref.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _munchausen_ref as mr
from oracle import ref_numpy as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON = {"alpha": 0.9, "tau": 0.5, "clip": -2.0}


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    from ddq import _lib
    if not os.path.exists(_lib.CPU_LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "distributed-deep-q_amd"),
                        "ddq/_lib/libddq_cpu.so"], check=True)
    return m


def test_binding_and_error_table(ddq):
    from ddq import _lib
    assert ctypes.sizeof(_lib.MunchausenCfg) == 16
    assert {"ddq_set_munchausen", "ddq_get_munchausen"} <= set(_lib.EXPORTED)
    net = ddq.DeepQNet(batch=2, frame=16, mode="cpu")
    assert net.munchausen() is None
    net.set_munchausen()
    assert net.munchausen() == pytest.approx({"alpha": 0.9, "tau": 0.03, "clip": -1.0})
    net.set_munchausen(**ON)
    nan, inf = float("nan"), float("inf")
    bad = [(2, 0.5, 0.5, -1.0), (-1, 0.5, 0.5, -1.0), (1, -0.1, 0.5, -1.0), (1, 1.5, 0.5, -1.0),
           (1, nan, 0.5, -1.0), (1, 0.5, 0.0, -1.0), (1, 0.5, -1.0, -1.0), (1, 0.5, inf, -1.0),
           (1, 0.5, nan, -1.0), (1, 0.5, 0.5, 0.0), (1, 0.5, 0.5, 1.0), (1, 0.5, 0.5, -inf),
           (1, 0.5, 0.5, nan)]
    for cfg in bad:
        m = _lib.MunchausenCfg(*cfg)
        assert net.lib.ddq_set_munchausen(net.ctx, ctypes.byref(m)) == _lib.DDQ_EINVAL, cfg
        assert net.munchausen() == pytest.approx(ON)
    assert net.lib.ddq_set_munchausen(net.ctx, None) == _lib.DDQ_EINVAL
    # the double target is refused while it is on, and the objective stays
    with pytest.raises(_lib.DDQError) as ei:
        net.set_objective("double", "huber", 0.5)
    assert ei.value.code == _lib.DDQ_EINVAL
    assert net.objective() == {"target": "max", "loss": "euclidean", "huber_delta": 0.0}
    net.set_objective("max", "huber", 0.5)
    # and it is refused under the double target, staying off
    net.set_munchausen(None)
    net.set_objective("double")
    with pytest.raises(_lib.DDQError) as ei:
        net.set_munchausen(**ON)
    assert ei.value.code == _lib.DDQ_EINVAL and net.munchausen() is None
    net.set_munchausen(None)                       # turning it off is always allowed
    for name in ("Pc_out", "m_bonus"):             # off: no such blob
        with pytest.raises(_lib.DDQError) as ei:
            net.blob(name)
        assert ei.value.code == _lib.DDQ_ESTATE
    net.set_objective()
    net.set_munchausen(alpha=0.0, tau=0.5)         # Soft-DQN: a bonus of zeros, no P(s,.)
    assert net.blob("m_bonus").shape == (2, 1, 1, 1)
    with pytest.raises(_lib.DDQError) as ei:
        net.blob("Pc_out")
    assert ei.value.code == _lib.DDQ_ESTATE
    net.close()


@pytest.mark.parametrize("alpha", [0.0, 0.9])
def test_one_pass_against_the_reference(ddq, alpha):
    import _objective_ref as objr
    c = mr.case(ref, 16, 4, 901)
    mr.oracle_head(ref, c, alpha)                  # the case's conditions
    net = objr.make_net(ddq, c, mode="cpu")
    net.set_munchausen(alpha, **c["cfg"])
    net.forward_backward()
    h = mr.check_head(net, c["mb"], ref.GAMMA, alpha, **c["cfg"])
    assert np.any(h["P_sa"] != objr.blobs_of(net)["P_out"].max(axis=1) * c["mb"][4].reshape(-1))
    mr.check_grads(ref, net, c, h["d"])
    net.close()
