"""The device-resident training monitor (csrc/monitor.h, ddq_monitor_*) on the GPU.

S = 16, B = 8 (the small-map step) and S = 24, B = 8 (the general kernels), a
64-slot ring of synthetic Snake transitions.  At S = 16 the blob sizes cover
every chunking case of the 8192-float chunks: blobs far below a chunk (4, 32,
64), one just under a chunk (6272), ragged multi-chunk blobs (51200 = 6.25
chunks, 36864 = 4.5 chunks) and an exact multiple (131072 = 16 chunks).

Expected records are recomputed in numpy float64 from the existing getters
(tests/_monitor_ref.py, where the tolerance 2 * 2^-23 is derived); records of
the same training run taken in different step modes must be equal byte for
byte."""
import numpy as np
import pytest

import _monitor_ref as mr

pytestmark = pytest.mark.gpu

B, N, STEPS = 8, 64, 11
SHAPES = [16, 24]

_RING, _RUNS = {}, {}


def ring_for(S):
    if S not in _RING:
        from ddq.expgain import synthetic_transitions
        _RING[S] = synthetic_transitions(N, S, seed=77)
    return _RING[S]


def theta0(S):
    from ddq import params
    return params.init_params_flat(S, seed=42)


def make_net(S, ring=True, mode="gpu"):
    import ddq
    net = ddq.DeepQNet(batch=B, frame=S, mode=mode)
    net.set_flat(0, theta0(S))
    net.set_flat(1, theta0(S))
    if ring:
        st, ac, rw, nt = ring_for(S)
        net.replay_create(N)
        net.replay_import(st, ac, rw, nt, 0, N)
    return net


def cfg_of(net, **kw):
    return net.step_cfg("rmsprop", lr=1e-5, target_period=3, seed=5, **kw)


def final_state(net):
    return [net.get_flat(0), net.get_flat(1), net.optimizer_state()]


def chain(S, mode, capacity=16, period=1):
    """STEPS steps of one step mode on a fresh ctx; its records and final state.
    Computed once per (S, mode, capacity, period) and not changed afterwards."""
    key = (S, mode, capacity, period)
    if key not in _RUNS:
        net = make_net(S)
        assert net.small_path()[0] == (S == 16)
        if capacity:
            net.monitor_enable(capacity, period)
        cfg = cfg_of(net)
        checked = 0
        if mode == "eager":
            prev = None
            for k in range(STEPS):
                net.step(cfg)
                net.synchronize()
                recs, total = net.monitor_read()
                assert total == k + 1
                mr.assert_record(recs[-1], mr.expected(net, iteration=k + 1, tag=-1))
                # theta_P changes exactly when the step ends on a P <- Q sync
                p = recs[-1]["param_rms"][1]
                if (k + 1) % 3 == 0:
                    assert p.tobytes() == recs[-1]["param_rms"][0].tobytes()
                    assert p.tobytes() != prev.tobytes()
                elif prev is not None:
                    assert p.tobytes() == prev.tobytes()
                else:
                    assert p.tobytes() == mr.rms_of(net, theta0(S)).tobytes()
                prev = p.copy()
                checked += 1
        elif mode == "graph":
            net.step_graph(cfg, STEPS)
        else:
            net.step_pipelined(cfg, STEPS)
        net.synchronize()
        recs, total = net.monitor_read() if capacity else (None, 0)
        if capacity:     # the run stayed finite: the comparisons below compare numbers
            assert (recs["nonfinite"] == 0).all() and np.isfinite(recs["loss"]).all()
        _RUNS[key] = {"records": recs, "total": total, "state": final_state(net),
                      "checked": checked}
        net.close()
    return _RUNS[key]


@pytest.mark.parametrize("S", SHAPES)
def test_explicit_record_after_forward_backward(S):
    net = make_net(S)
    rng = np.random.default_rng(2)
    net.set_flat(1, (rng.standard_normal(net.num_params) * 0.02).astype(np.float32))
    net.replay_sample(np.sort(rng.choice(N - 2, B, replace=False)).astype(np.int32))
    net.forward_backward()
    net.monitor_enable(4)
    net.monitor_record(tag=-(2 ** 40))
    recs, total = net.monitor_read()
    assert total == 1
    want = mr.expected(net, iteration=0, tag=-(2 ** 40))
    assert want["loss"] > 0 and (want["grad_rms"][::2] > 0).all()
    mr.assert_record(recs[0], want)
    # a blob of zeros gives exactly 0; planted non-finite values are counted
    blobs = mr.blobs_of(net)
    g = net.get_grads_flat()
    g[blobs[3][0]:blobs[3][0] + blobs[3][1]] = 0
    g[blobs[6][0] + np.array([1, blobs[6][1] - 1])] = [np.nan, np.inf]
    net.set_grads_flat(g)
    net.monitor_record(1)
    recs, total = net.monitor_read()
    assert total == 2 and recs[1]["grad_rms"][3] == 0 and np.isnan(recs[1]["grad_rms"][6])
    assert list(recs[1]["nonfinite"]) == [0, 0, 2]
    mr.assert_record(recs[1], mr.expected(net, 0, 1))
    net.close()


@pytest.mark.parametrize("S", SHAPES)
def test_eager_steps_record_every_step(S):
    run = chain(S, "eager")
    assert run["checked"] == STEPS and run["total"] == STEPS
    assert list(run["records"]["iteration"]) == list(range(1, STEPS + 1))
    assert (run["records"]["tag"] == -1).all()


@pytest.mark.parametrize("mode", ["graph", "pipelined"])
@pytest.mark.parametrize("S", SHAPES)
def test_step_modes_take_the_same_records(S, mode):
    eager, other = chain(S, "eager"), chain(S, mode)
    assert other["total"] == STEPS
    assert other["records"].tobytes() == eager["records"].tobytes()


@pytest.mark.parametrize("S", SHAPES)
def test_period_four_records_iterations_four_and_eight(S):
    eager = chain(S, "eager")["records"]
    for mode in ("graph", "pipelined"):
        run = chain(S, mode, period=4)
        assert run["total"] == 2 and list(run["records"]["iteration"]) == [4, 8]
        assert run["records"].tobytes() == eager[[3, 7]].tobytes()


@pytest.mark.parametrize("S", SHAPES)
def test_monitor_does_not_perturb_training(S):
    on, off = chain(S, "pipelined"), chain(S, "pipelined", capacity=0)
    for a, b in zip(on["state"], off["state"]):
        assert a.tobytes() == b.tobytes()
    assert not np.array_equal(on["state"][0], theta0(S))


@pytest.mark.parametrize("S", SHAPES)
def test_ring_wraps(S):
    full, small = chain(S, "pipelined"), chain(S, "pipelined", capacity=4)
    assert small["total"] == STEPS and len(small["records"]) == 4
    assert small["records"].tobytes() == full["records"][-4:].tobytes()


@pytest.mark.parametrize("S", SHAPES)
def test_refusals_while_recording_steps(S):
    from ddq import _lib
    net = make_net(S)
    net.comm_init(net.comm_unique_id(), 1, 0)      # the async exchange needs a communicator
    net.monitor_enable(4, 1)
    nostore = cfg_of(net, store_grads=False)
    for call in (lambda: net.step(nostore), lambda: net.step_graph(nostore, 1),
                 lambda: net.step_pipelined(nostore, 2)):
        with pytest.raises(_lib.DDQError) as ei:
            call()
        assert ei.value.code == _lib.DDQ_EINVAL
    with pytest.raises(_lib.DDQError) as ei:
        net.async_begin(cfg_of(net, exchange="async"))
    assert ei.value.code == _lib.DDQ_ESTATE
    net.synchronize()
    assert net.monitor_read()[1] == 0 and net.lib.ddq_step_count(net.ctx) == 0
    net.monitor_enable(0)
    net.step(nostore)
    net.async_begin(cfg_of(net, exchange="async"))
    net.synchronize()
    net.close()


@pytest.mark.parametrize("S", SHAPES)
def test_profile_step_lists_the_monitor(S):
    net = make_net(S)
    cfg = cfg_of(net)
    assert "monitor" not in [n for n, _ in net.profile_step(cfg)]
    net.monitor_enable(4, 1)
    prof = net.profile_step(cfg)
    assert prof[-1][0] == "monitor" and prof[-1][1] > 0
    assert [n for n, _ in prof].count("monitor") == 1
    recs, total = net.monitor_read()
    assert total == 1
    mr.assert_record(recs[0], mr.expected(net, iteration=2, tag=-1))
    net.monitor_enable(0)
    assert "monitor" not in [n for n, _ in net.profile_step(cfg)]
    net.close()


def test_interleaved_with_actor_and_evaluator():
    from ddq.actor import DeviceActor, zoom_maps
    from ddq.snake import SnakeGame
    S = 16
    net = make_net(S, ring=False)
    net.replay_create(N)
    init = SnakeGame().encode_state()
    actor = DeviceActor(net, init, 31)
    actor.fill(40)
    net.monitor_enable(16, 1)
    cfg = cfg_of(net)
    actor.act_and_step(cfg, 3, 60000)
    rm, cm = zoom_maps((S, S), S)
    net.eval_create(np.stack([init] * 4), rm, cm, 7, 0.25, 20, 4)
    net.eval_run(5)
    net.monitor_record(tag=5)
    net.synchronize()
    recs, total = net.monitor_read()
    assert total == 4 and list(recs["tag"]) == [-1, -1, -1, 5]
    assert list(recs["iteration"]) == [1, 2, 3, 3]
    mr.assert_record(recs[2], mr.expected(net, 3, -1))
    mr.assert_record(recs[3], mr.expected(net, 3, 5))
    actor.act_and_step(cfg, 2, 60003)
    net.eval_run(3)
    net.synchronize()
    recs, total = net.monitor_read()
    assert total == 6
    mr.assert_record(recs[5], mr.expected(net, 5, -1))
    assert net.eval_read()["stats"][0] == 8 and net.actor_read()[1][0] == 45
    net.close()


@pytest.mark.parametrize("S", SHAPES)
def test_device_record_against_the_cpu_twin(S):
    rng = np.random.default_rng(4)
    dev, twin = make_net(S, ring=False), make_net(S, ring=False, mode="cpu")
    P = dev.num_params
    thp = (rng.standard_normal(P) * 0.02).astype(np.float32)
    g = (rng.standard_normal(P) * 1e-3).astype(np.float32)
    got = []
    for net in (dev, twin):
        net.set_flat(1, thp)
        net.set_grads_flat(g)
        net.monitor_enable(2)
        net.monitor_record(3)
        recs, _ = net.monitor_read()
        mr.assert_record(recs[0], mr.expected(net, 0, 3))
        got.append(recs[0])
    mr.assert_record(got[0], got[1])
    dev.close()
    twin.close()
