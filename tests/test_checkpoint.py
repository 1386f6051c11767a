"""Checkpoint and resume on the CPU twin (ddq_state_*, ddq.checkpoint): the
digest against its numpy restatement, a save / restore round trip that must
continue bit for bit, the file format and the refusals.  No GPU.
"""
import ctypes
import os

import numpy as np
import pytest

import _checkpoint_ref as ref
import _coherence as co

S, B = 16, 8
CAPS = (2, 3, 9, 257, 4099)


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ck():
    from ddq import checkpoint
    return checkpoint


def small_ring_net(ddq, cap, mode="cpu", S=S, B=B):
    """A net on a ring of `cap` slots filled with seeded bytes, with Adam and
    (cap >= 9: a draw of B needs B allowed slots) nothing else."""
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
    if cap >= 9:
        net.replay_set_priority(alpha=0.6, beta=0.4, eps=0.01)
    return net


# ---------------------------------------------------------------- 1. digest
def test_reference_digest_is_the_definition():
    ref.check_vectors()


@pytest.mark.parametrize("cap", CAPS)
def test_twin_digest_equals_the_reference(ddq, ck, cap):
    net = small_ring_net(ddq, cap)
    try:
        secs = net.state_sections()
        names = [n for n, _, _ in secs]
        assert names[:6] == ["config", "theta_q", "theta_p", "opt", "opt2", "counters"]
        assert names[6:10] == ["ring_state", "ring_action", "ring_reward", "ring_nonterm"]
        assert ("prio_leaf" in names) == (cap >= 9)
        sizes = dict((n, b) for n, b, _ in secs)
        assert sizes["config"] == 64 and sizes["counters"] == 96
        assert sizes["ring_action"] == cap and sizes["ring_reward"] == 2 * cap
        assert sizes["ring_state"] == cap * 4 * S * S and sizes["theta_q"] == 4 * net.num_params
        for name, nbytes, dig in secs:
            data = ck.state_read(net, name, 0, nbytes)
            assert data.size == nbytes
            assert dig == ref.digest(data), name
            assert ck.state_digest(net, name) == dig, name
        # ranges: an odd offset and length inside a section
        whole = ck.state_read(net, "ring_reward", 0, 2 * cap)
        if cap >= 3:
            assert ck.state_read(net, "ring_reward", 1, 3).tobytes() == whole[1:4].tobytes()
    finally:
        net.close()


def test_state_check_program_under_the_sanitizers(tmp_path):
    """cpu/state_check.cpp: the twin's section walk, range checks and digest over
    odd sizes and offsets, as a program of its own built with the address and
    undefined-behaviour sanitizers (nothing is loaded into this interpreter)."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cpu = os.path.join(root, "distributed-deep-q_amd", "cpu")
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "state_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fopenmp", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Wno-unused-parameter", os.path.join(cpu, "state_check.cpp"),
                    os.path.join(cpu, "twin.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "state check ok" in r.stdout


# ---------------------------------------------------------------- 2. round trip
def host_loop(net, rng, k, rule, lr, prio):
    for _ in range(k):
        net.replay_sample(np.sort(rng.choice(np.arange(8, co.N - 8), net.batch, replace=False))
                          .astype(np.int32))
        net.forward_backward()
        if prio:
            net.replay_update_priorities()
        net.apply(rule, lr=lr)


def configure(ddq, variant, mode="cpu"):
    net = co.make_net(ddq, S, B, mode)
    if variant in ("adam", "rich"):
        net.set_adam(max_grad_norm=1.0)
    if variant == "rich":
        net.replay_set_nstep(3)
        net.set_objective("double", "huber", 0.5)
        net.replay_set_priority(alpha=0.6, beta=0.4, eps=0.01)
        net.set_target_tau(0.5)
    return net


@pytest.mark.parametrize("variant", ["rmsprop", "adam", "rich"])
def test_round_trip_continues_bit_for_bit(ddq, ck, tmp_path, variant):
    rule = "rmsprop" if variant == "rmsprop" else "adam"
    lr = co.LR if rule == "rmsprop" else 1e-4
    kw = dict(adam=rule == "adam", prio=variant == "rich", device=False)
    path = str(tmp_path / "a.ckpt")
    net = configure(ddq, variant)
    try:
        rng = np.random.default_rng(5)
        host_loop(net, rng, 3, rule, lr, kw["prio"])
        if variant == "rich":
            net.soft_sync_target()
        entries = net.save_checkpoint(path, meta={"iteration": 3, "variant": variant})
        saved = ref.full_state(net, **kw)
        rng_state = rng.bit_generator.state
        host_loop(net, rng, 4, rule, lr, kw["prio"])
        a = ref.full_state(net, **kw)
    finally:
        net.close()
    assert not os.path.exists(path + ".tmp")
    assert [e["name"] for e in entries][0] == "config"
    fresh, meta = ck.restore(path, mode="cpu")
    try:
        assert meta == {"iteration": 3, "variant": variant}
        ref.assert_same_state(ref.full_state(fresh, **kw), saved, variant + ": right after the load")
        assert saved["theta_q"].tobytes() != a["theta_q"].tobytes()
        rng = np.random.default_rng(5)
        rng.bit_generator.state = rng_state
        host_loop(fresh, rng, 4, rule, lr, kw["prio"])
        ref.assert_same_state(ref.full_state(fresh, **kw), a, variant + ": 4 updates after the load")
    finally:
        fresh.close()


def test_round_trip_into_a_configured_net_with_an_actor(ddq, ck, tmp_path):
    """load_checkpoint into a net the caller configured; the single actor's game
    and RNG position travel."""
    from ddq.actor import DeviceActor
    board = start_board()

    def make():
        net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
        net.set_flat(0, co.theta0(S))
        net.set_flat(1, co.theta0(S))
        net.replay_create(64)
        DeviceActor(net, board, 77)
        return net
    path = str(tmp_path / "actor.ckpt")
    net = make()
    try:
        net.actor_step(20, 0)
        net.save_checkpoint(path)
        net.actor_step(15, 100)
        a = ref.full_state(net, actor=True, device=False)
    finally:
        net.close()
    fresh = make()
    try:
        assert fresh.load_checkpoint(path) == {}
        fresh.actor_step(15, 100)
        ref.assert_same_state(ref.full_state(fresh, actor=True, device=False), a, "actor")
    finally:
        fresh.close()


def start_board():
    """A (10,10) start board in SnakeGame.encode_state's codes: a three-cell snake
    and one apple."""
    b = np.full((10, 10), -1, np.int8)
    b[5, 5], b[5, 4], b[5, 3] = 0, 1, 2
    b[2, 7] = -2
    return b


# ---------------------------------------------------------------- 3. file
def saved_file(ddq, tmp_path, name="f.ckpt"):
    net = configure(ddq, "adam")
    try:
        rng = np.random.default_rng(5)
        host_loop(net, rng, 1, "adam", 1e-4, False)
        path = str(tmp_path / name)
        net.save_checkpoint(path, meta={"k": 1})
        return path, ref.full_state(net, adam=True, device=False)
    finally:
        net.close()


def test_file_layout(ddq, ck, tmp_path):
    path, state = saved_file(ddq, tmp_path)
    assert not os.path.exists(path + ".tmp")
    hdr, secs = ref.parse(path)
    assert hdr["mode"] == "cpu" and hdr["meta"] == {"k": 1} and hdr["version"] == 1
    assert [e["name"] for e in hdr["sections"]] == [
        "config", "theta_q", "theta_p", "opt", "opt2", "counters", "ring_state", "ring_action",
        "ring_reward", "ring_nonterm"]
    for e in hdr["sections"]:
        assert int(e["digest"]) == ref.digest(secs[e["name"]]), e["name"]
    assert secs["theta_q"].tobytes() == state["theta_q"].tobytes()
    assert secs["opt2"].tobytes() == state["adam_v"].tobytes()
    assert secs["ring_reward"].tobytes() == state["ring_reward"].tobytes()
    from ddq import _lib
    cfg = secs["config"].view(_lib.STATE_CONFIG_DTYPE)[0]
    assert (cfg["batch"], cfg["frame"], cfg["capacity"], cfg["lanes"], cfg["nstep"]) == (B, S, co.N, 1, 1)
    assert cfg["adam_on"] == 1 and cfg["prio_enabled"] == 0 and cfg["target_tau"] == 1.0
    ctr = secs["counters"].view(_lib.STATE_COUNTERS_DTYPE)[0]
    assert ctr["iteration"] == 1 and ctr["opt_init"] == 1 and ctr["valid"] == co.N
    assert not ctr["reserved"].any()
    h2, size = ck.read_header(path)
    assert h2 == hdr and size == os.path.getsize(path)


def test_truncated_file_is_refused(ddq, ck, tmp_path):
    path, _ = saved_file(ddq, tmp_path)
    raw = open(path, "rb").read()
    for cut in (4, 12, 40, len(raw) - 1, len(raw) // 2):
        bad = str(tmp_path / ("cut%d" % cut))
        open(bad, "wb").write(raw[:cut])
        with pytest.raises(ck.CheckpointError):
            ck.restore(bad, mode="cpu")
    bad = str(tmp_path / "magic")
    open(bad, "wb").write(b"DDQCKPT2" + raw[8:])
    with pytest.raises(ck.CheckpointError, match="magic"):
        ck.read_header(bad)


def test_flipped_byte_is_caught_by_the_digest(ddq, ck, tmp_path):
    path, _ = saved_file(ddq, tmp_path)
    hdr, _ = ref.parse(path)
    e = next(e for e in hdr["sections"] if e["name"] == "theta_q")
    raw = bytearray(open(path, "rb").read())
    raw[e["offset"] + e["bytes"] // 2] ^= 0x10
    bad = str(tmp_path / "flipped")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(ck.CheckpointError, match="theta_q.*corrupt|corrupt.*theta_q"):
        ck.restore(bad, mode="cpu")


# ---------------------------------------------------------------- 4. refusals
def test_config_mismatch_names_the_field_and_writes_nothing(ddq, ck, tmp_path):
    path, _ = saved_file(ddq, tmp_path)
    net = configure(ddq, "adam")
    try:
        net.replay_set_nstep(2)                 # the same sizes, another n
        before = ref.full_state(net, adam=True, device=False)
        with pytest.raises(ck.CheckpointError, match="nstep"):
            net.load_checkpoint(path)
        hdr, secs = ref.parse(path)
        rc = net.lib.ddq_state_write(net.ctx, b"config", 0, secs["config"].ctypes.data_as(ctypes.c_void_p), 64)
        assert rc == ddq._lib.DDQ_EINVAL and b"nstep" in net.lib.ddq_last_error(net.ctx)
        ref.assert_same_state(ref.full_state(net, adam=True, device=False), before, "nothing written")
        net.replay_sample(np.arange(8, 8 + B, dtype=np.int32))   # the net is not restoring
    finally:
        net.close()


def test_wrong_byte_count_is_refused(ddq, ck):
    net = configure(ddq, "rmsprop")
    try:
        n = 4 * net.num_params
        buf = np.zeros(n + 8, np.uint8)
        p = buf.ctypes.data_as(ctypes.c_void_p)
        E = ddq._lib.DDQ_EINVAL
        assert net.lib.ddq_state_write(net.ctx, b"theta_q", 0, p, n + 4) == E
        assert net.lib.ddq_state_write(net.ctx, b"theta_q", 8, p, n) == E
        assert net.lib.ddq_state_write(net.ctx, b"theta_q", -1, p, 4) == E
        assert net.lib.ddq_state_write(net.ctx, b"theta_q", 0, p, 0) == E
        assert net.lib.ddq_state_write(net.ctx, b"opt2", 0, p, n) == E          # no Adam: no section
        assert net.lib.ddq_state_write(net.ctx, b"nonsense", 0, p, 4) == E
        assert net.lib.ddq_state_read(net.ctx, b"counters", 90, p, 8) == E
        net.replay_sample(np.arange(8, 8 + B, dtype=np.int32))   # the net is not restoring
    finally:
        net.close()


def test_step_between_write_and_commit_is_refused(ddq, ck):
    net = configure(ddq, "rmsprop")
    try:
        idx = np.arange(8, 8 + B, dtype=np.int32)
        net.replay_sample(idx)
        ck.state_write(net, "theta_q", co.theta0(S, seed=44))
        E = ddq._lib.DDQ_ESTATE
        for call in (lambda: net.replay_sample(idx), net.forward_backward, net.forward_q,
                     lambda: net.apply("rmsprop"), lambda: net.replay_add(0, 0, None),
                     lambda: net.select_action(np.zeros((1, 4, S, S), np.uint8))):
            with pytest.raises(ddq._lib.DDQError) as ei:
                call()
            assert ei.value.code == E and "restore not committed" in ei.value.msg
        ck.state_commit(net)
        assert net.get_flat(0).tobytes() == co.theta0(S, seed=44).tobytes()
        net.replay_sample(idx)
        net.forward_backward()
    finally:
        net.close()


def test_bad_leaf_is_refused_at_commit(ddq, ck):
    net = configure(ddq, "rich")
    try:
        q, _, _ = net.replay_priorities()
        head, valid, cap = net.replay_info()
        forbidden = np.flatnonzero(q == 0)
        assert forbidden.size == 3               # n = 3 on a full ring: the window behind the head
        bad = q.copy()
        bad[forbidden[0]] = 65536                # nonzero on a forbidden slot
        ck.state_write(net, "prio_leaf", bad)
        with pytest.raises(ddq._lib.DDQError) as ei:
            ck.state_commit(net)
        assert ei.value.code == ddq._lib.DDQ_EINVAL and "prio_leaf" in ei.value.msg
        with pytest.raises(ddq._lib.DDQError) as ei:     # still restoring
            net.forward_q()
        assert ei.value.code == ddq._lib.DDQ_ESTATE
        bad = q.copy()
        bad[8] = (1 << 24) + 1                   # above the largest leaf
        ck.state_write(net, "prio_leaf", bad)
        with pytest.raises(ddq._lib.DDQError):
            ck.state_commit(net)
        ck.state_write(net, "prio_leaf", q)
        ck.state_commit(net)
        assert net.replay_priorities()[0].tobytes() == q.tobytes()
    finally:
        net.close()


def test_counters_are_validated_at_commit(ddq, ck):
    net = configure(ddq, "rmsprop")
    try:
        from ddq import _lib
        ctr = ck.state_read(net, "counters").view(_lib.STATE_COUNTERS_DTYPE).copy()
        bad = ctr.copy()
        bad["head"] = co.N                       # head == lane_len
        ck.state_write(net, "counters", bad)
        with pytest.raises(ddq._lib.DDQError) as ei:
            ck.state_commit(net)
        assert ei.value.code == ddq._lib.DDQ_EINVAL and "head" in ei.value.msg
        ctr["head"], ctr["iteration"], ctr["steps"] = 17, 5, 5
        ck.state_write(net, "counters", ctr)
        assert ck.state_read(net, "counters").tobytes() == ctr.tobytes()   # as written
        ck.state_commit(net)
        assert net.replay_info()[0] == 17
        assert ck.state_read(net, "counters").tobytes() == ctr.tobytes()
    finally:
        net.close()


# ---------------------------------------------------------------- 5. the worker and the server
def test_param_server_resumes(ddq, ck, tmp_path):
    from ddq.barista import messaging
    from ddq.param_server import ParamServer
    path = str(tmp_path / "server.ckpt")

    def grad_message(ps, k):
        rng = np.random.default_rng(100 + k)
        g = ps.net.split(rng.normal(0, 1e-2, ps.net.num_params).astype(np.float32), "Q")
        return messaging.create_net_message(g, "diff")

    def push(ps, ks):
        for k in ks:
            ps.get_model_params()
            ps.update_params(grad_message(ps, k))
    a = ParamServer(frame=S, batch=B, update="adam", special_update=2, mode="cpu",
                    checkpoint_path=path, checkpoint_freq=3, adam={"max_grad_norm": 1.0})
    try:
        a.init_params(seed=7)
        push(a, range(3))
        assert os.path.exists(path) and not os.path.exists(path + ".tmp")
        push(a, range(3, 5))
        want, it = a.get_model_params(), a.iteration
        state = ref.full_state(a.net, adam=True, device=False)
    finally:
        a.net.close()
    b = ParamServer(frame=S, batch=B, update="adam", special_update=2, mode="cpu",
                    adam={"max_grad_norm": 1.0}, resume=path)
    try:
        assert (b.iteration, b.has_model, b.has_target) == (3, True, True)
        push(b, range(3, 5))
        assert b.iteration == it and b.get_model_params() == want
        ref.assert_same_state(ref.full_state(b.net, adam=True, device=False), state, "server")
    finally:
        b.net.close()


def test_barista_net_checkpoints_and_resumes(ddq, ck, tmp_path):
    import random

    from ddq.barista.baristanet import BaristaNet
    from ddq.replay import ReplayDataset
    path = str(tmp_path / "worker.ckpt")
    arch = {"batch": B, "frame": S}

    def worker(**kw):
        net = BaristaNet(arch, None, None, mode="cpu", **kw)
        dset = ReplayDataset(None, (4, S, S), dset_size=64, batch_size=B, net=net.dqn, mode="cpu")
        if "resume" not in kw:
            st, ac, rw, nt = co.ring(S, 64, 3)
            net.dqn.replay_import(st, ac, rw, nt, 0, 64)
        net.add_dataset(dset)
        return net

    def steps(net, k):
        for _ in range(k):
            net.iteration += 1
            net.load_minibatch()
            net.full_pass()
            net.dqn.apply("rmsprop", lr=co.LR)
            net.maybe_checkpoint()
    random.seed(3)
    a = worker(checkpoint=path, checkpoint_every=2)
    try:
        steps(a, 2)
        assert os.path.exists(path)
        first = open(path, "rb").read()
        steps(a, 1)
        assert open(path, "rb").read() == first       # iteration 3: no checkpoint
        want = ref.full_state(a.dqn, device=False)
        idx = a.dqn.read_indices()
    finally:
        a.dqn.close()
    random.seed(99)                                    # the file's stream replaces it
    b = worker(resume=path)
    try:
        assert b.iteration == 2
        b.checkpoint = None
        steps(b, 1)
        assert b.dqn.read_indices().tobytes() == idx.tobytes()
        ref.assert_same_state(ref.full_state(b.dqn, device=False), want, "worker")
    finally:
        b.dqn.close()
