"""GPU: checkpoint and bit-exact resume (ddq_state_*, ddq.checkpoint).

A context restored from a checkpoint must continue exactly as the context that
wrote it: every comparison here is of bytes.  Shapes (S, B) as
tests/test_gpu_coherence.py's: (16, 8) and (16, 40) the two small-map apply
sites, (24, 4) the general kernels.  Ring of 256 slots, seed 11.
"""
import ctypes

import numpy as np
import pytest

import _actor_host as ah
import _checkpoint_ref as ref
import _coherence as co
import _pool_host as ph

pytestmark = pytest.mark.gpu

SMALL, SMALL40, GENERAL = (16, 8), (16, 40), (24, 4)
THREE = [SMALL, SMALL40, GENERAL]
TWO = [SMALL, GENERAL]
SEED = 11
CAPS = (2, 3, 9, 257, 4099)
MODES = ("eager", "graph", "pipelined")


def sid(shape):
    return "S%d-B%d" % shape


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ck():
    from ddq import checkpoint
    return checkpoint


# ---------------------------------------------------------------- 5. the digest kernel
def ring_net(ddq, S, B, cap, mode):
    """Both towers, Adam's v, a ring of `cap` seeded slots and (a draw of B needs
    room: cap >= 257) the priority leaves."""
    net = ddq.DeepQNet(batch=B, frame=S, mode=mode)
    rng = np.random.default_rng(cap)
    net.set_flat(0, co.theta0(S))
    net.set_flat(1, co.theta0(S, seed=43))
    net.set_adam()
    net.replay_create(cap)
    net.replay_import(rng.integers(0, 256, (cap, 4, S, S)).astype(np.uint8),
                      rng.integers(0, 4, cap).astype(np.uint8),
                      rng.integers(-1, 2, cap).astype(np.int16),
                      (rng.random(cap) > 0.1).astype(np.uint8), cap // 2, cap)
    if cap >= 257:
        net.replay_set_priority(alpha=0.6, beta=0.4, eps=0.01)
    return net


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("shape", [SMALL, GENERAL], ids=sid)
def test_device_digest_equals_reference_and_twin(ddq, ck, shape, cap):
    S, B = shape
    gpu, cpu = ring_net(ddq, S, B, cap, "gpu"), ring_net(ddq, S, B, cap, "cpu")
    try:
        secs, twin = gpu.state_sections(), cpu.state_sections()
        assert [(n, b) for n, b, _ in secs] == [(n, b) for n, b, _ in twin]
        sizes = dict((n, b) for n, b, _ in secs)
        assert sizes["ring_action"] == cap and sizes["ring_reward"] == 2 * cap
        assert ("prio_leaf" in sizes) == (cap >= 257)
        for (name, nbytes, dig), (_, _, tdig) in zip(secs, twin):
            data = ck.state_read(gpu, name, 0, nbytes)
            print("%-12s %10d bytes  device %016x  reference %016x  twin %016x"
                  % (name, nbytes, dig, ref.digest(data), tdig))
            assert dig == ref.digest(data), name
            assert dig == tdig, name
            assert ck.state_digest(gpu, name) == dig, name
    finally:
        co.close_all([gpu, cpu])


# ---------------------------------------------------------------- 6. resume is exact
RICH = dict(nstep=3, objective=("double", "huber", 0.5), prio=True)


def make(ddq, S, B, rich):
    net = co.make_net(ddq, S, B)
    if rich:
        net.replay_set_nstep(RICH["nstep"])
        net.set_objective(*RICH["objective"])
        net.replay_set_priority(alpha=0.6, beta=0.4, eps=0.01)
        net.set_adam(max_grad_norm=1.0)
        net.set_target_tau(0.5)
    return net


def cfg_of(net, rich):
    if rich:
        return net.step_cfg("adam", lr=1e-4, target_period=1, seed=SEED)
    return net.step_cfg("rmsprop", lr=co.LR, target_period=3, seed=SEED)


def run(net, cfg, mode, k):
    if mode == "eager":
        for _ in range(k):
            net.step(cfg)
    elif mode == "graph":
        net.step_graph(cfg, k)
    else:
        net.step_pipelined(cfg, k)
    net.synchronize()


def train_state(net, rich):
    """What test 6 compares, with the state's own sections on top."""
    out = ref.full_state(net, adam=rich, prio=rich)
    out["iteration"] = ck_counters(net)["iteration"].reshape(1)
    out["read_indices"] = net.read_indices()
    out["loss"] = np.asarray(net.blob("loss"))
    return out


def ck_counters(net):
    from ddq import _lib, checkpoint
    return checkpoint.state_read(net, "counters").view(_lib.STATE_COUNTERS_DTYPE)[0]


_RUNS = {}


def writer(ddq, shape, rich, mode, tmp_path_factory):
    """2 updates in `mode`, the checkpoint, 5 more: (path, state after 7), once
    per case."""
    key = (shape, rich, mode)
    if key not in _RUNS:
        path = str(tmp_path_factory.mktemp("ckpt") / "w.ckpt")
        net = make(ddq, *shape, rich)
        try:
            cfg = cfg_of(net, rich)
            run(net, cfg, mode, 2)
            net.save_checkpoint(path, meta={"iteration": 2, "mode": mode})
            at_save = train_state(net, rich)
            run(net, cfg, mode, 5)
            _RUNS[key] = (path, at_save, train_state(net, rich))
        finally:
            co.close_all([net])
    return _RUNS[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rich,shape", [(False, s) for s in THREE] + [(True, s) for s in TWO],
                         ids=lambda v: sid(v) if isinstance(v, tuple) else ("rich" if v else "plain"))
def test_resume_is_exact(ddq, ck, tmp_path_factory, rich, shape, mode):
    path, at_save, a = writer(ddq, shape, rich, mode, tmp_path_factory)
    what = "%s %s %s" % (mode, sid(shape), "rich" if rich else "plain")
    net, meta = ck.restore(path)
    try:
        assert meta == {"iteration": 2, "mode": mode}
        got = ref.full_state(net, adam=rich, prio=rich)
        for name in got:                       # (no minibatch is bound after a load)
            assert got[name].tobytes() == at_save[name].tobytes(), "%s: %s after the load" % (what, name)
        assert at_save["theta_q"].tobytes() != a["theta_q"].tobytes(), what
        # the segment straddles rmsprop's first-call lag and the first target sync
        assert ck_counters(net)["iteration"] == 2 and ck_counters(net)["opt_init"] == 1
        run(net, cfg_of(net, rich), mode, 5)
        ref.assert_same_state(train_state(net, rich), a, what)
        assert net.replay_draws() == 7
    finally:
        co.close_all([net])


def test_saved_pipelined_resumed_eager(ddq, ck, tmp_path_factory):
    path, _, _ = writer(ddq, SMALL, False, "pipelined", tmp_path_factory)
    _, _, eager = writer(ddq, SMALL, False, "eager", tmp_path_factory)
    net, _ = ck.restore(path)
    try:
        run(net, cfg_of(net, False), "eager", 5)
        ref.assert_same_state(train_state(net, False), eager, "pipelined file, eager resume")
    finally:
        co.close_all([net])


# ---------------------------------------------------------------- 7. derived copies
@pytest.mark.parametrize("shape", THREE, ids=sid)
def test_derived_copies_after_load(ddq, ck, tmp_path_factory, shape):
    """Right after load_checkpoint, before any step: the conv weights' split
    copies of both towers are those of the restored theta (a commit without the
    relayout leaves the fresh net's initial ones)."""
    path, at_save, _ = writer(ddq, shape, False, "eager", tmp_path_factory)
    S, B = shape
    net = ddq.DeepQNet(batch=B, frame=S)
    try:
        net.set_flat(0, co.theta0(S, seed=44))      # other towers, other copies
        net.set_flat(1, co.theta0(S, seed=45))
        net.replay_create(co.ring_slots(B))
        net.load_checkpoint(path)
        assert net.get_flat(0).tobytes() == at_save["theta_q"].tobytes()
        co.check(ddq, net, at_save["theta_p"], "after load_checkpoint, " + sid(shape))
    finally:
        co.close_all([net])


# ---------------------------------------------------------------- 8. actors
def pool_net(ddq):
    S, B = SMALL
    net = ddq.DeepQNet(batch=B, frame=S)
    th = co.theta0(S)
    net.set_flat(0, th)
    net.set_flat(1, th)
    net.replay_create(256)
    net.replay_set_lanes(4)
    return net


def test_actor_pool_resumes(ddq, ck, tmp_path):
    from ddq.actor import DeviceActorPool
    path = str(tmp_path / "pool.ckpt")
    net = pool_net(ddq)
    try:
        pool = DeviceActorPool(net, ph.four_boards(), 5)
        pool.fill(16)
        cfg = net.step_cfg("rmsprop", lr=co.LR, target_period=3, seed=SEED)
        pool.act_and_train(cfg, 3, 0)
        net.synchronize()
        net.save_checkpoint(path)
        pool.act_and_train(cfg, 3, 12)
        a = ref.full_state(net, pool=True)
    finally:
        co.close_all([net])
    made = []

    def setup(n):
        made.append(DeviceActorPool(n, ph.four_boards(), 999))   # another seed: the file's wins
    fresh, _ = ck.restore(path, setup=setup)
    try:
        assert fresh.replay_lanes() == (4, 64)
        made[0].act_and_train(fresh.step_cfg("rmsprop", lr=co.LR, target_period=3, seed=SEED), 3, 12)
        ref.assert_same_state(ref.full_state(fresh, pool=True), a, "actor pool")
    finally:
        co.close_all([fresh])


def test_single_actor_resumes(ddq, ck, tmp_path):
    from ddq.actor import DeviceActor
    S, B = SMALL
    init = ah.init_boards()["apple_ahead"]
    path = str(tmp_path / "actor.ckpt")

    def make_actor_net():
        net = ddq.DeepQNet(batch=B, frame=S)
        th = co.theta0(S)
        net.set_flat(0, th)
        net.set_flat(1, th)
        net.replay_create(256)
        return net
    net = make_actor_net()
    try:
        actor = DeviceActor(net, init, 7)
        actor.fill(40)
        cfg = net.step_cfg("rmsprop", lr=co.LR, target_period=3, seed=SEED)
        actor.act_and_step(cfg, 3, 0)
        net.synchronize()
        net.save_checkpoint(path)
        actor.act_and_step(cfg, 3, 3)
        a = ref.full_state(net, actor=True)
    finally:
        co.close_all([net])
    made = []
    fresh, _ = ck.restore(path, setup=lambda n: made.append(DeviceActor(n, init, 1234)))
    try:
        made[0].act_and_step(fresh.step_cfg("rmsprop", lr=co.LR, target_period=3, seed=SEED), 3, 3)
        ref.assert_same_state(ref.full_state(fresh, actor=True), a, "single actor")
    finally:
        co.close_all([fresh])


# ---------------------------------------------------------------- 9. across the libraries
def host_updates(net, k):
    rng = np.random.default_rng(5)
    for _ in range(k):
        net.replay_sample(np.sort(rng.choice(np.arange(8, co.N - 8), net.batch, replace=False))
                          .astype(np.int32))
        net.forward_backward()
        net.apply("adam", lr=1e-4)


@pytest.mark.parametrize("src,dst", [("cpu", "gpu"), ("gpu", "cpu")])
def test_files_travel_between_the_libraries(ddq, ck, tmp_path, src, dst):
    S, B = SMALL
    path = str(tmp_path / "x.ckpt")
    net = co.make_net(ddq, S, B, src)
    try:
        net.set_adam(max_grad_norm=1.0)
        host_updates(net, 2)
        net.save_checkpoint(path)
        a = ref.full_state(net, adam=True, device=False)
    finally:
        co.close_all([net])
    hdr, secs = ref.parse(path)
    assert hdr["mode"] == src
    fresh, _ = ck.restore(path, mode=dst)
    try:
        assert fresh.mode == dst
        b = ref.full_state(fresh, adam=True, device=False)
        ref.assert_same_state(b, a, "%s file on %s" % (src, dst))     # the sections' digests among them
        for name in ("theta_q", "theta_p", "opt", "opt2", "ring_state", "ring_action", "ring_reward",
                     "ring_nonterm", "counters"):
            assert ck.state_read(fresh, name).tobytes() == secs[name].tobytes(), name
    finally:
        co.close_all([fresh])


# ---------------------------------------------------------------- 10. refusals
def test_step_before_commit_is_refused(ddq, ck):
    net = co.make_net(ddq, *SMALL)
    try:
        cfg = net.step_cfg("rmsprop", lr=co.LR, target_period=3, seed=SEED)
        net.step(cfg)
        net.synchronize()
        q = net.get_flat(0)
        ck.state_write(net, "theta_q", q)
        calls = [lambda: net.step(cfg), lambda: net.step_graph(cfg, 1),
                 lambda: net.step_pipelined(cfg, 2), net.forward_backward, net.forward_q,
                 lambda: net.apply("rmsprop"), lambda: net.replay_sample_device(1),
                 lambda: net.replay_add(0, 0, None),
                 lambda: net.select_action(np.zeros((1, 4, 16, 16), np.uint8))]
        for call in calls:
            with pytest.raises(ddq._lib.DDQError) as ei:
                call()
            assert ei.value.code == ddq._lib.DDQ_ESTATE and "restore not committed" in ei.value.msg
        ck.state_commit(net)
        net.step(cfg)
        net.synchronize()
        assert net.get_flat(0).tobytes() != q.tobytes()
    finally:
        co.close_all([net])


def test_state_calls_refused_after_async_begin(ddq, ck):
    net = co.make_net(ddq, *SMALL)
    nets = [net]
    try:
        net.comm_init(net.comm_unique_id(), 1, 0)  # the async exchange needs a communicator
        assert net.state_sections()                # members of a communicator are fine
        net.async_begin(net.step_cfg("rmsprop", lr=1e-5, target_period=3, seed=SEED, exchange="async"))
        net.synchronize()
        E = ddq._lib.DDQ_ESTATE
        buf = np.zeros(64, np.uint8)
        p = buf.ctypes.data_as(ctypes.c_void_p)
        n, d = ctypes.c_int32(), ctypes.c_uint64()
        assert net.lib.ddq_state_sections(net.ctx, None, 0, ctypes.byref(n)) == E
        assert net.lib.ddq_state_read(net.ctx, b"config", 0, p, 64) == E
        assert net.lib.ddq_state_write(net.ctx, b"config", 0, p, 64) == E
        assert net.lib.ddq_state_digest(net.ctx, b"config", ctypes.byref(d)) == E
        assert net.lib.ddq_state_commit(net.ctx) == E
    finally:
        co.close_all(nets)


def test_corrupted_file_is_caught_by_the_device_digest(ddq, ck, tmp_path_factory, tmp_path):
    path, _, _ = writer(ddq, SMALL, False, "eager", tmp_path_factory)
    hdr, _ = ref.parse(path)
    raw = bytearray(open(path, "rb").read())
    for name in ("theta_q", "ring_state"):
        e = next(e for e in hdr["sections"] if e["name"] == name)
        bad = bytearray(raw)
        bad[e["offset"] + e["bytes"] - 3] ^= 0x01
        p = str(tmp_path / (name + ".ckpt"))
        open(p, "wb").write(bytes(bad))
        with pytest.raises(ck.CheckpointError, match=name):
            ck.restore(p)
