"""The training monitor on the CPU twin (cpu/twin.cpp ddq_monitor_*) and the
Python surface above it: DeepQNet.monitor_*, netutils' norm helpers and
NetLogger, BaristaNet.log(), ParamServer(on_stats=...).

Expected records are recomputed in numpy float64 from the getters
(tests/_monitor_ref.py, where the tolerance 2 * 2^-23 is derived)."""
import ctypes
import glob
import os

import numpy as np
import pytest

import _monitor_ref as mr

B = 8


def make_net(S, seed=0, applies=2):
    """A twin ctx with random theta_Q, theta_P and gradient, a forward_backward's
    loss and Q_out, and ``applies`` applied updates behind it."""
    import ddq
    rng = np.random.default_rng(seed)
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    P = net.num_params
    for _ in range(applies):
        net.apply("sgd", lr=1e-3)
    net.set_flat(0, (rng.standard_normal(P) * 0.05).astype(np.float32))
    net.set_flat(1, (rng.standard_normal(P) * 0.03).astype(np.float32))
    act = np.zeros((B, 4), np.float32)
    act[np.arange(B), rng.integers(0, 4, B)] = 1
    net.write_minibatch(rng.integers(0, 256, (B, 4, S, S)).astype(np.float32), act,
                        rng.integers(-1, 2, B).astype(np.float32),
                        rng.integers(0, 256, (B, 4, S, S)).astype(np.float32),
                        rng.integers(0, 2, B).astype(np.float32))
    net.forward_backward()
    g = (rng.standard_normal(P) * 1e-3).astype(np.float32)
    lo, cnt = mr.blobs_of(net)[5]            # Qconv3's bias gradient: all zeros
    g[lo:lo + cnt] = 0
    net.set_grads_flat(g)
    return net


@pytest.mark.parametrize("S", [16, 24])
def test_explicit_record_matches_numpy(S):
    net = make_net(S)
    net.monitor_enable(4)
    net.monitor_record(tag=1234567890123)
    recs, total = net.monitor_read()
    assert total == 1 and len(recs) == 1
    want = mr.expected(net, iteration=2, tag=1234567890123)
    assert np.isfinite(want["loss"]) and want["q_max_mean"] != 0
    assert want["grad_rms"][5] == 0 and (np.delete(want["grad_rms"], 5) > 0).all()
    mr.assert_record(recs[0], want)
    net.close()


def test_nonfinite_counts():
    net = make_net(16)
    net.monitor_enable(4)
    net.monitor_record(7)
    blobs = mr.blobs_of(net)
    g, thp = net.get_grads_flat(), net.get_flat(1)
    g[blobs[2][0] + np.array([0, 17, blobs[2][1] - 1])] = np.nan      # Qconv2.w: 3 NaN
    g[blobs[6][0] + np.array([5, 100000])] = [np.inf, -np.inf]          # Qfc4.w: 2 Inf
    thp[blobs[9][0] + 3] = np.nan                                       # P_out.b: 1 NaN
    net.set_grads_flat(g)
    net.set_flat(1, thp)
    net.monitor_record(7)
    (r0, r1), total = net.monitor_read()
    assert total == 2
    assert list(r1["nonfinite"]) == [0, 1, 5] and list(r0["nonfinite"]) == [0, 0, 0]
    assert np.isnan(r1["grad_rms"][2]) and np.isinf(r1["grad_rms"][6])
    assert np.isnan(r1["param_rms"][1][9])
    # every other field is what it was
    fixed = r1.copy()
    fixed["nonfinite"] = 0
    fixed["grad_rms"][[2, 6]] = r0["grad_rms"][[2, 6]]
    fixed["param_rms"][1][9] = r0["param_rms"][1][9]
    assert fixed.tobytes() == r0.tobytes()
    mr.assert_record(r1, mr.expected(net, 2, 7))
    net.close()


def test_ring_wrap_and_arguments():
    from ddq import _lib
    net = make_net(16, applies=0)
    with pytest.raises(_lib.DDQError) as ei:          # disabled by default
        net.monitor_record(0)
    assert ei.value.code == _lib.DDQ_ESTATE
    with pytest.raises(_lib.DDQError) as ei:
        net.monitor_read()
    assert ei.value.code == _lib.DDQ_ESTATE
    for cap, period in ((-1, 0), (4, -1)):
        with pytest.raises(_lib.DDQError) as ei:
            net.monitor_enable(cap, period)
        assert ei.value.code == _lib.DDQ_EINVAL
    net.monitor_enable(3)
    for tag in range(5):
        net.monitor_record(tag)
    recs, total = net.monitor_read()
    assert total == 5 and list(recs["tag"]) == [2, 3, 4]
    recs, _ = net.monitor_read(3, 2)
    assert list(recs["tag"]) == [3, 4]
    for first, n in ((1, 1), (1, 4), (4, 2), (-1, 1)):
        with pytest.raises(_lib.DDQError) as ei:
            net.monitor_read(first, n)
        assert ei.value.code == _lib.DDQ_EINVAL, (first, n)
    # out may be NULL with n == 0
    total = ctypes.c_int64()
    assert net.lib.ddq_monitor_read(net.ctx, 0, 0, None, ctypes.byref(total)) == 0
    assert total.value == 5
    net.monitor_enable(3, 5)        # re-enable resets the count; a period is accepted
    assert net.monitor_read()[1] == 0
    net.monitor_record(9)
    assert net.monitor_read()[1] == 1
    net.monitor_enable(0)           # capacity 0 disables
    with pytest.raises(_lib.DDQError) as ei:
        net.monitor_record(0)
    assert ei.value.code == _lib.DDQ_ESTATE
    net.close()


def test_record_layout_matches_header():
    from ddq import _lib
    from ddq.net import MONITOR_DTYPE
    R = _lib.MonitorRecord
    assert MONITOR_DTYPE.itemsize == ctypes.sizeof(R) == 160
    # offsets of include/ddq_hip.h ddq_monitor_record (x86-64 SysV)
    want = {"iteration": 0, "tag": 8, "loss": 16, "q_max_mean": 20, "nonfinite": 24,
            "reserved": 36, "param_rms": 40, "grad_rms": 120}
    for name, off in want.items():
        assert getattr(R, name).offset == off, name
        assert MONITOR_DTYPE.fields[name][1] == off, name
    assert MONITOR_DTYPE.names == tuple(f[0] for f in R._fields_)


def test_netlogger_files_and_norm_helpers(tmp_path):
    from ddq.barista import netutils
    from ddq.barista.baristanet import BaristaNet
    np.random.seed(3)
    net = BaristaNet({"batch": B, "frame": 16}, None, None, logpath=str(tmp_path / "run"),
                     mode="cpu")
    recs = []
    for _ in range(2):
        net.dummy_load_minibatch()
        net.full_pass()
        recs.append(net.log())
        mr.assert_record(recs[-1], mr.expected(net.dqn, 0, 0))
    dirs = glob.glob(str(tmp_path / "run-*"))
    assert len(dirs) == 1 and os.path.isdir(dirs[0])
    names = net.dqn.q_names + net.dqn.p_names
    assert len(names) == 10
    assert sorted(os.listdir(dirs[0])) == sorted(
        ["loss"] + [n + ".gradnorm" for n in names] + [n + ".norm" for n in names])

    def lines(fname):
        with open(os.path.join(dirs[0], fname)) as fp:
            out = fp.read().splitlines()
        assert len(out) == 2, fname
        return out

    for k, rec in enumerate(recs):
        assert np.float32(lines("loss")[k]) == rec["loss"]
        for z, tower in enumerate((net.dqn.q_names, net.dqn.p_names)):
            for l, name in enumerate(tower):
                w, b = (np.float32(x) for x in lines(name + ".norm")[k].split(","))
                assert (w, b) == (rec["param_rms"][z][2 * l], rec["param_rms"][z][2 * l + 1])
                w, b = (np.float32(x) for x in lines(name + ".gradnorm")[k].split(","))
                want = (rec["grad_rms"][2 * l], rec["grad_rms"][2 * l + 1]) if z == 0 else (0, 0)
                assert (w, b) == want
    assert recs[0]["loss"] != recs[1]["loss"]

    # ord=None (a device record) against the reference's host computation
    for fn in (netutils.compute_gradient_norms, netutils.compute_param_norms):
        dev, host = fn(net), fn(net, ord=2)
        assert sorted(dev) == sorted(host) == sorted(names)
        for name in names:
            mr.assert_floats(dev[name], np.array(host[name]).astype(np.float32), name)
    sub = netutils.compute_param_norms(net, params=["Qfc4"], ord=np.inf)
    assert list(sub) == ["Qfc4"] and len(sub["Qfc4"]) == 2
    netutils.pretty_print(sub)

    # flush: the same lines from records taken elsewhere
    net.logger.flush(recs)
    with open(os.path.join(dirs[0], "loss")) as fp:
        out = fp.read().splitlines()
    assert len(out) == 4 and out[2:] == out[:2]
    # no logpath: log() does nothing
    plain = BaristaNet({"batch": B, "frame": 16}, None, None, mode="cpu")
    assert plain.logger is None and plain.log() is None
    plain.dqn.close()
    net.dqn.close()


def test_param_server_stats_hook():
    from ddq import _lib
    from ddq.barista import messaging
    from ddq.param_server import ParamServer
    seen = []
    ps = ParamServer(frame=16, batch=B, update="rmsprop", lr=1e-3, stats_freq=2, mode="cpu",
                     on_stats=lambda it, rec: seen.append((it, rec.copy(),
                                                           mr.expected(ps.net, it, it))))
    ps.init_params(seed=5)
    rng = np.random.default_rng(1)
    for _ in range(5):
        g = (rng.standard_normal(ps.net.num_params) * 1e-2).astype(np.float32)
        ps.update_params(messaging.create_net_message(ps.net.split(g, "Q")))
    assert [it for it, _, _ in seen] == [2, 4]
    for it, rec, want in seen:
        mr.assert_record(rec, want)
    assert seen[0][1]["param_rms"][0][0] != seen[1][1]["param_rms"][0][0]
    ps.net.close()

    quiet = ParamServer(frame=16, batch=B, stats_freq=2, mode="cpu")
    quiet.init_params(seed=5)
    with pytest.raises(_lib.DDQError) as ei:
        quiet.net.monitor_read()
    assert ei.value.code == _lib.DDQ_ESTATE
    quiet.net.close()
