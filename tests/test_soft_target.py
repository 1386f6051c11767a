"""Soft target updates (ddq_set_target_tau, ddq_soft_sync_target) without a GPU:
the C-ABI surface, the setter's argument check, the CPU twin's blend against
tests/_soft_target_ref.py byte for byte, the parameter server's rule and the
worker's --target-tau.  The device sites are tests/test_gpu_soft_target.py's.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _soft_target_ref import blend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ddq_hip.h")
CALLS = ("ddq_set_target_tau", "ddq_get_target_tau", "ddq_soft_sync_target")
S = 16


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    from ddq import _lib
    if not (os.path.exists(_lib.CPU_LIB_PATH) and os.path.exists(_lib.LIB_PATH)):
        subprocess.run(["make", "-C", os.path.join(ROOT, "distributed-deep-q_amd")], check=True)
    return m


def towers():
    from ddq.params import init_params_flat
    return init_params_flat(S, seed=42), init_params_flat(S, seed=43)


def twin(ddq, tau=None):
    net = ddq.DeepQNet(batch=2, frame=S, mode="cpu")
    q, p = towers()
    net.set_flat(0, q)
    net.set_flat(1, p)
    if tau is not None:
        net.set_target_tau(tau)
    return net


def test_header_and_both_libraries_have_the_calls(ddq):
    from ddq import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+ddq_set_target_tau\s*\(\s*ddq_ctx\s*\*\s*\w+\s*,\s*float\s+\w+\s*\)", txt)
    assert re.search(r"\bint\s+ddq_get_target_tau\s*\(\s*const\s+ddq_ctx\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)", txt)
    assert re.search(r"\bint\s+ddq_soft_sync_target\s*\(\s*ddq_ctx\s*\*\s*\w+\s*\)", txt)
    assert "#define DDQ_ABI_VERSION 6" in open(HEADER).read()
    assert set(CALLS) <= set(_lib.EXPORTED)
    for path in (_lib.LIB_PATH, _lib.CPU_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert [c for c in CALLS if not hasattr(lib, c)] == [], path


def test_setter_and_getter(ddq):
    from ddq import _lib
    net = twin(ddq)
    assert net.target_tau() == 1.0
    for tau in (0.5, 0.01, 1.0, 0.25):
        net.set_target_tau(tau)
        assert net.target_tau() == float(np.float32(tau))
    for bad in (0.0, -0.1, 1.5, float("nan")):
        assert net.lib.ddq_set_target_tau(net.ctx, bad) == _lib.DDQ_EINVAL, bad
        assert net.target_tau() == 0.25
        with pytest.raises(_lib.DDQError) as ei:
            net.set_target_tau(bad)
        assert ei.value.code == _lib.DDQ_EINVAL
    t = ctypes.c_float()
    assert net.lib.ddq_get_target_tau(net.ctx, None) == _lib.DDQ_EINVAL
    assert net.lib.ddq_get_target_tau(None, ctypes.byref(t)) == _lib.DDQ_EINVAL
    assert net.lib.ddq_set_target_tau(None, 0.5) == _lib.DDQ_EINVAL
    assert net.lib.ddq_soft_sync_target(None) == _lib.DDQ_EINVAL
    net.close()


@pytest.mark.parametrize("tau", [0.5, 0.01])
def test_twin_soft_sync_is_the_blend(ddq, tau):
    q, p = towers()
    net = twin(ddq, tau)
    net.soft_sync_target()
    p1 = blend(p, q, tau)
    assert p1.tobytes() not in (p.tobytes(), q.tobytes())
    assert net.get_flat(1).tobytes() == p1.tobytes()
    assert net.get_flat(0).tobytes() == q.tobytes()
    net.soft_sync_target()                           # two in a row compound
    p2 = blend(p1, q, tau)
    assert p2.tobytes() != p1.tobytes()
    assert net.get_flat(1).tobytes() == p2.tobytes()
    net.close()


def test_twin_soft_sync_at_tau_1_is_sync_target(ddq):
    q, p = towers()
    a, b = twin(ddq, 1.0), twin(ddq)
    a.soft_sync_target()
    b.sync_target()
    assert a.get_flat(1).tobytes() == b.get_flat(1).tobytes() == q.tobytes()
    # (the blend at tau = 1 is not the copy in fp32: p + (q - p) rounds)
    assert blend(p, q, 1.0).tobytes() != q.tobytes()
    a.close()
    b.close()


def test_param_server_blends_once_a_target_exists(ddq):
    from ddq.barista import messaging
    from ddq.param_server import ParamServer
    tau = 0.25
    ps = ParamServer(frame=S, batch=2, mode="cpu", target_tau=tau, special_update=2,
                     snapshot_freq=0, stats_freq=0)
    assert ps.net.target_tau() == tau
    ps.init_params(seed=42)
    rng = np.random.default_rng(3)
    q0 = ps.net.get_flat(0)
    model = lambda: messaging.load_model_params(ps.get_model_params())  # noqa: E731

    def p_of(msg_params):
        return ps.net.join(msg_params, "P")

    m = model()                                      # iteration 0: the first special update copies
    assert ps.has_target and ps.net.get_flat(1).tobytes() == q0.tobytes()
    assert m[0] == 0 and p_of(m[1]).tobytes() == q0.tobytes()    # (and P* is in the message)
    want = q0
    for it in range(1, 7):
        g = rng.normal(0, 1e-2, ps.net.num_params).astype(np.float32)
        assert ps.update_params(messaging.create_net_message(ps.net.split(g, "Q"))) == b"Updated"
        q = ps.net.get_flat(0)
        model()                                      # a pull after every push
        if it % 2 == 0:
            nxt = blend(want, q, tau)
            assert nxt.tobytes() not in (want.tobytes(), q.tobytes())
            want = nxt
        assert ps.net.get_flat(1).tobytes() == want.tobytes(), it
        assert ps.net.get_flat(0).tobytes() == q.tobytes(), it
    # without target_tau the special update stays the copy
    hard = ParamServer(frame=S, batch=2, mode="cpu", special_update=1, snapshot_freq=0, stats_freq=0)
    hard.init_params(seed=42)
    hard.get_model_params()
    g = rng.normal(0, 1e-2, hard.net.num_params).astype(np.float32)
    hard.update_params(messaging.create_net_message(hard.net.split(g, "Q")))
    hard.get_model_params()
    assert hard.net.get_flat(1).tobytes() == hard.net.get_flat(0).tobytes() != q0.tobytes()


def test_worker_flag_reaches_the_net(ddq, tmp_path):
    from ddq.barista import main as bm
    from ddq.barista.baristanet import BaristaNet
    base = ["arch", "none", "--mode", "cpu", "--driver", "None", "--overwrite",
            "--dset-size", "24", "--initial-replay", "12"]
    assert bm.get_args(base).target_tau is None
    args = bm.get_args(base + ["--target-tau", "0.005", "--dataset", str(tmp_path / "r.hdf5")])
    assert args.target_tau == 0.005
    args.architecture = {"batch": 4, "frame": S}
    net, replay, xp = bm.build_worker(args)
    assert net.target_tau == 0.005 and net.dqn.target_tau() == float(np.float32(0.005))
    # the construction's own P <- Q stays a copy
    assert net.dqn.get_flat(1).tobytes() == net.dqn.get_flat(0).tobytes()
    replay.close()
    for bad in ("0", "1.5", "-0.1"):
        with pytest.raises(SystemExit):
            bm.get_args(base + ["--target-tau", bad])
    plain = BaristaNet({"batch": 2, "frame": S}, None, None, mode="cpu")
    assert plain.target_tau is None and plain.dqn.target_tau() == 1.0
    soft = BaristaNet({"batch": 2, "frame": S}, None, None, mode="cpu", target_tau=0.5)
    assert soft.dqn.target_tau() == 0.5
