"""Prioritized replay (ddq_replay_set_priority) on the CPU twin, against
tests/_per_ref.py: the stratified draw exactly, the weights, the weighted head,
the commit, the invariant under every ring writer and every rebuild, the
refusals, and the host layer (PriorityCfg, ReplayDataset / BaristaNet
``priority=``, the worker's --per-* flags).  S = 16, B = 4.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _actor_host as ah
import _nstep_ref as nr
import _per_ref as pr
import _pool_host as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, B = 16, 4
SEED = 2016


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    from ddq import _lib
    if not os.path.exists(_lib.CPU_LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "distributed-deep-q_amd"),
                        "ddq/_lib/libddq_cpu.so"], check=True)
    return m


def make_net(ddq, ring, head, valid, lanes=1, n=None, prio=None, batch=B):
    net = ddq.DeepQNet(batch=batch, frame=S, mode="cpu")
    th = ah.seeded_theta(S)
    net.set_flat(0, th)
    net.set_flat(1, th)
    st, ac, rw, nt = ring
    net.replay_create(len(ac))
    if lanes > 1:
        net.replay_set_lanes(lanes)
    net.replay_import(st, ac, rw, np.asarray(nt, np.uint8), head, valid)
    if n is not None:
        net.replay_set_nstep(n)
    if prio is not None:
        net.replay_set_priority(**prio)
    return net


def code_of(call):
    from ddq import _lib
    with pytest.raises(_lib.DDQError) as ei:
        call()
    return ei.value.code


PRIO = dict(alpha=0.6, beta=0.4, eps=0.01)
# (name, capacity, lanes, head, valid, n): a small ring; 5000 slots (not a power
# of 64, above 64^2) with an unfilled tail of zero leaves; four lanes with zero
# runs between them; n = 3
RINGS = [("small", 64, 1, 40, 64, 1), ("5000", 5000, 1, 300, 300, 1),
         ("5000 full", 5000, 1, 4990, 5000, 1), ("laned 4x200", 800, 4, 100, 100, 1),
         ("n3", 130, 1, 7, 130, 3)]


def set_leaves(net, leaves):
    idx = np.asarray(sorted(leaves), np.int32)
    net.replay_set_priorities(idx, np.asarray([leaves[int(i)] for i in idx], np.uint32))


# 1 ------------------------------------------------------------------ the draw
@pytest.mark.parametrize("ring", RINGS, ids=[r[0] for r in RINGS])
def test_draw_is_the_restatement(ddq, ring):
    name, cap, lanes, head, valid, n = ring
    L = cap // lanes
    rng = np.random.default_rng(1)
    net = make_net(ddq, nr.build_ring(rng, cap, S), head, valid, lanes, n, PRIO)
    q0, total, pmax = net.replay_priorities()
    pr.check_invariant(q0, total, head, valid, L, n, lanes, name)
    assert pmax == pr.ONE
    ctr = 0
    dup = False
    for cname, leaves in pr.leaf_cases(cap, nr.allowed_slots(head, valid, L, n, lanes)).items():
        set_leaves(net, leaves)
        q, total, got_pmax = net.replay_priorities()
        pmax = max(pmax, max(leaves.values()))       # pmax only rises between rebuilds
        assert total == sum(leaves.values()) and got_pmax == pmax
        for _ in range(3):
            net.replay_sample_device(SEED)
            want, T = pr.draw(q, B, SEED, ctr)
            ctr += 1
            got = net.read_indices()
            np.testing.assert_array_equal(got, want, (name, cname, ctr))
            assert T == total and (np.diff(got) >= 0).all()
            dup |= bool((np.diff(got) == 0).any())
            w = net.blob("is_weight").reshape(B)
            np.testing.assert_allclose(w, pr.isw64(q, got, PRIO["beta"]), rtol=1e-4)
            mb = net.read_minibatch()
            nr.assert_minibatch(mb, nr.gather(nr.build_ring(np.random.default_rng(1), cap, S),
                                              got, L, n), (name, cname))
    assert dup, "the 2^24 leaf must be drawn more than once in a set"
    net.close()


def test_beta_zero_weights_are_exactly_one(ddq):
    rng = np.random.default_rng(2)
    net = make_net(ddq, nr.build_ring(rng, 64, S), 40, 64, prio=dict(alpha=0.5, beta=0.0, eps=0.1))
    set_leaves(net, {i: 1 + 1000 * i for i in range(64) if i != 39})
    net.replay_sample_device(SEED)
    assert net.blob("is_weight").tobytes() == np.ones(B, np.float32).tobytes()
    net.close()


# 3 ------------------------------------------------------------------ the head
@pytest.mark.parametrize("loss", ["euclidean", "huber"])
def test_weighted_head(ddq, loss):
    rng = np.random.default_rng(3)
    ring = nr.build_ring(rng, 64, S)
    net = make_net(ddq, ring, 40, 64, prio=PRIO)
    net.set_objective("max", loss, 0.05)
    set_leaves(net, {i: 1 + 50000 * i for i in range(64) if i != 39})
    net.replay_sample_device(SEED)
    w = net.blob("is_weight").reshape(B)
    assert len(set(w.tolist())) > 1
    lossw = net.forward_backward()
    dqw, gw = net.blob("Q_out.diff").reshape(B, 4), net.get_grads_flat()
    idx = net.read_indices()
    # the same slots unweighted: dQ scales by the weight image by image
    plain = make_net(ddq, ring, 40, 64)
    plain.set_objective("max", loss, 0.05)
    assert len(set(idx.tolist())) == B
    plain.replay_sample(idx)
    loss1 = plain.forward_backward()
    dq1 = plain.blob("Q_out.diff").reshape(B, 4)
    np.testing.assert_allclose(dqw, dq1 * w[:, None], rtol=1e-6)
    assert lossw < loss1 and not np.array_equal(gw, plain.get_grads_flat())
    d = plain.blob("Q_sa").reshape(B).astype(np.float64) - plain.blob("target_Q_sa").reshape(B)
    le = d * d if loss == "euclidean" else 2 * np.where(np.abs(d) <= 0.05, d * d / 2,
                                                        0.05 * (np.abs(d) - 0.025))
    np.testing.assert_allclose(lossw, (w * le).sum() / B / 2, rtol=1e-4)
    # host-given indices carry weight 1: with prioritization on, the pass is the
    # unweighted one byte for byte
    net.replay_set_priority(alpha=0.6, beta=0.0, eps=0.01)
    net.replay_sample(idx)
    assert net.blob("is_weight").tobytes() == np.ones(B, np.float32).tobytes()
    assert net.forward_backward() == loss1
    assert net.get_grads_flat().tobytes() == plain.get_grads_flat().tobytes()
    for name in ("Q_out.diff", "Q_sa", "target_Q_sa", "P_sa"):
        assert net.blob(name).tobytes() == plain.blob(name).tobytes()
    net.close()
    plain.close()


# 4 ------------------------------------------------------------------ the commit
def test_commit_teacher_forced(ddq):
    rng = np.random.default_rng(4)
    ring = nr.build_ring(rng, 64, S)
    net = make_net(ddq, ring, 40, 64, prio=PRIO)
    set_leaves(net, {i: (pr.QMAX if i == 20 else 1) for i in range(64) if i != 39})
    q0, _, pmax0 = net.replay_priorities()
    net.replay_sample_device(SEED)
    idx = net.read_indices()
    assert (np.diff(idx) == 0).any()
    net.forward_backward()
    net.replay_update_priorities()
    q1, total, pmax1 = net.replay_priorities()
    ref = pr.check_commit(q0, q1, total, pmax0, pmax1, idx, net.blob("Q_sa").reshape(B),
                          net.blob("target_Q_sa").reshape(B), PRIO["eps"], PRIO["alpha"])
    assert set(ref) == set(int(i) for i in idx)
    # a slot an add makes forbidden between the draw and the commit stays 0
    net.replay_sample(np.asarray([38, 41, 42, 43], np.int32))
    st = np.zeros((4, S, S), np.uint8)
    net.replay_add(1, 0, st)                     # head 40 -> 41: slot 40 forbidden, 39 released
    net.replay_add(1, 0, st)                     # head 42: slot 41 forbidden, 40 released
    net.forward_backward()
    qa, _, _ = net.replay_priorities()
    assert qa[41] == 0
    net.replay_update_priorities()
    qb, total, _ = net.replay_priorities()
    assert qb[41] == 0 and qb[38] != qa[38] and total == int(qb.astype(np.int64).sum())
    pr.check_invariant(qb, total, 42, 64, 64, 1)
    net.close()


# 5 ------------------------------------------------------------------ writers
@pytest.mark.parametrize("n", [1, 3])
def test_invariant_under_host_adds(ddq, n):
    cap = 8
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    net.replay_create(cap)
    net.replay_set_nstep(n)
    net.replay_set_priority(**PRIO)
    q = [0] * cap
    pmax = pr.ONE
    st = np.zeros((4, S, S), np.uint8)
    for k in range(20):
        if k == 9:                               # a larger pmax: released slots take it
            filled = [i for i in range(cap) if q[i]]
            net.replay_set_priorities(np.asarray(filled[:1], np.int32),
                                      np.asarray([3 * pr.ONE], np.uint32))
            q[filled[0]], pmax = 3 * pr.ONE, 3 * pr.ONE
        h = k % cap
        net.replay_add(k % 4, 0, st if k % 5 else None)
        head, valid, _ = net.replay_info()
        released = pr.writer(q, pmax, 0, h, cap, n, head, valid)
        got, total, gp = net.replay_priorities()
        assert got.tolist() == q and gp == pmax, (k, got.tolist(), q)
        pr.check_invariant(got, total, head, valid, cap, n, 1, "add %d" % k)
        if released is not None:
            assert got[released] == pmax
    net.close()


@pytest.mark.parametrize("n", [1, 3])
def test_invariant_under_the_actor(ddq, n):
    from ddq.actor import zoom_maps
    cap = 8
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    th = ah.seeded_theta(S)
    net.set_flat(0, th)
    net.replay_create(cap)
    net.replay_set_nstep(n)
    net.replay_set_priority(**PRIO)
    rm, cm = zoom_maps((S, S), S)
    net.actor_create(ah.init_boards()["start"], rm, cm, 5)
    q = [0] * cap
    for k in range(20):
        net.actor_step(1, 0)
        head, valid, _ = net.replay_info()
        pr.writer(q, pr.ONE, 0, k % cap, cap, n, head, valid)
        got, total, _ = net.replay_priorities()
        assert got.tolist() == q
        pr.check_invariant(got, total, head, valid, cap, n, 1, "actor step %d" % k)
    net.close()


def test_invariant_under_the_pool(ddq):
    from ddq.actor import zoom_maps
    lanes, L = 4, 8
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    th = ah.seeded_theta(S)
    net.set_flat(0, th)
    net.replay_create(lanes * L)
    net.replay_set_lanes(lanes)
    net.replay_set_priority(**PRIO)
    rm, cm = zoom_maps((S, S), S)
    net.actors_create(ph.four_boards(), rm, cm, 7)
    q = [0] * (lanes * L)
    for k in range(20):
        net.actors_step(1, 0)
        head, valid, _ = net.replay_info()
        for g in range(lanes):
            pr.writer(q, pr.ONE, g * L, k % L, L, 1, head, valid)
        got, total, _ = net.replay_priorities()
        assert got.tolist() == q
        pr.check_invariant(got, total, head, valid, L, 1, lanes, "pool move %d" % k)
    net.close()


def test_rebuilds(ddq):
    rng = np.random.default_rng(5)
    ring = nr.build_ring(rng, 24, S)
    net = make_net(ddq, ring, 5, 24, prio=PRIO)
    set_leaves(net, {7: 9 * pr.ONE})
    assert net.replay_priorities()[2] == 9 * pr.ONE
    net.replay_set_nstep(3)
    q, total, pmax = net.replay_priorities()
    pr.check_invariant(q, total, 5, 24, 24, 3)
    assert pmax == pr.ONE and set(q.tolist()) == {0, pr.ONE}
    set_leaves(net, {7: 9 * pr.ONE})
    net.replay_import(ring[0], ring[1], ring[2], ring[3], 11, 17)
    q, total, pmax = net.replay_priorities()
    pr.check_invariant(q, total, 11, 17, 24, 3)
    assert pmax == pr.ONE and set(q.tolist()) == {0, pr.ONE}
    assert code_of(net.replay_update_priorities) == -5      # the rebuild unbinds the index set
    net.close()


# 8 ------------------------------------------------------------------ refusals
def test_refusals(ddq):
    from ddq import _lib
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    assert code_of(lambda: net.replay_set_priority(**PRIO)) == _lib.DDQ_ESTATE        # no ring
    net.replay_create(16)
    assert net.replay_priority() is None
    for call in (net.replay_priorities, net.replay_update_priorities,
                 lambda: net.replay_set_priorities([0], [1]), lambda: net.blob("is_weight")):
        assert code_of(call) == _lib.DDQ_ESTATE                                       # disabled
    for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(beta=-1e-3),
                dict(beta=1.0001), dict(beta=float("inf")), dict(eps=0.0), dict(eps=-1.0),
                dict(eps=float("nan")), dict(eps=float("inf"))):
        assert code_of(lambda: net.replay_set_priority(**dict(PRIO, **bad))) == _lib.DDQ_EINVAL
    for edge in (dict(alpha=0.0), dict(alpha=1.0), dict(beta=0.0), dict(beta=1.0), dict(eps=1e-30)):
        net.replay_set_priority(**dict(PRIO, **edge))
    got = net.replay_priority()
    assert got == {"alpha": pytest.approx(0.6), "beta": pytest.approx(0.4),
                   "eps": pytest.approx(1e-30)}
    st = np.zeros((4, S, S), np.uint8)
    for k in range(10):
        net.replay_add(0, 0, st)
    q, _, _ = net.replay_priorities()
    assert q[9] == 0 and q[8] != 0
    sp = net.replay_set_priorities
    assert code_of(lambda: sp([9], [5])) == _lib.DDQ_EINVAL          # nonzero on a zero leaf
    assert code_of(lambda: sp([8], [0])) == _lib.DDQ_EINVAL          # zero on a nonzero leaf
    assert code_of(lambda: sp([8], [pr.QMAX + 1])) == _lib.DDQ_EINVAL
    assert code_of(lambda: sp([16], [5])) == _lib.DDQ_EINVAL
    assert code_of(lambda: sp([-1], [5])) == _lib.DDQ_EINVAL
    sp([8, 9], [pr.QMAX, 0])
    assert net.replay_priorities()[1:] == (8 * pr.ONE + pr.QMAX, pr.QMAX)
    # the size check at its boundary: 9 allowed slots
    assert code_of(net.replay_update_priorities) == _lib.DDQ_ESTATE   # nothing drawn yet
    net.replay_sample_device(1)
    net.write_minibatch(reward=np.zeros(B, np.float32))
    assert code_of(net.replay_update_priorities) == _lib.DDQ_ESTATE   # a written minibatch
    net.replay_set_priority(enabled=False)
    assert net.replay_priority() is None
    assert code_of(net.replay_priorities) == _lib.DDQ_ESTATE
    net.close()
    big = ddq.DeepQNet(batch=257, frame=S, mode="cpu")
    big.replay_create(600)
    assert code_of(lambda: big.replay_set_priority(**PRIO)) == _lib.DDQ_EINVAL
    big.close()
    ok = ddq.DeepQNet(batch=256, frame=S, mode="cpu")
    ok.replay_create(600)
    ok.replay_set_priority(**PRIO)
    ok.close()
    few = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    few.replay_create(16)
    few.replay_set_priority(**PRIO)
    for k in range(B):
        few.replay_add(0, 0, st)
    assert code_of(lambda: few.replay_sample_device(1)) == _lib.DDQ_EINVAL   # A = B - 1
    few.replay_add(0, 0, st)
    few.replay_sample_device(1)                                               # A = B
    few.close()


# 9 ------------------------------------------------------------------ host layer
def test_priority_cfg_is_16_bytes():
    from ddq import _lib
    assert ctypes.sizeof(_lib.PriorityCfg) == 16
    for name in ("ddq_replay_set_priority", "ddq_replay_get_priority", "ddq_replay_priorities",
                 "ddq_replay_set_priorities", "ddq_replay_update_priorities_async"):
        assert name in _lib.EXPORTED
    hdr = open(os.path.join(ROOT, "include", "ddq_hip.h")).read()
    assert "#define DDQ_ABI_VERSION 6" in hdr and "ddq_priority_cfg" in hdr


def test_baristanet_round_trip(ddq, tmp_path):
    from ddq.barista.baristanet import BaristaNet
    from ddq.replay import ReplayDataset
    net = BaristaNet({"batch": B, "frame": S}, None, None, mode="cpu",
                     priority={"alpha": 0.7, "beta": 0.5})
    dset = ReplayDataset(str(tmp_path / "r.hdf5"), (4, S, S), dset_size=32, overwrite=True,
                         batch_size=B, mode="cpu")
    assert dset.priority is None
    net.add_dataset(dset)
    assert dset.priority == {"alpha": 0.7, "beta": 0.5, "eps": 1e-2}
    assert net.dqn.replay_priority() == {"alpha": pytest.approx(0.7), "beta": pytest.approx(0.5),
                                         "eps": pytest.approx(1e-2)}
    rng = np.random.default_rng(6)
    for k in range(20):
        dset.add_experience(k % 4, k % 3 - 1, rng.integers(0, 256, (4, S, S), dtype=np.uint8))
    q0, _, _ = net.dqn.replay_priorities()
    net.load_minibatch()
    idx = net.dqn.read_indices()
    want, _ = pr.draw(q0, B, net.per_seed, 0)
    np.testing.assert_array_equal(idx, want)
    net.full_pass()
    q1, total, pmax = net.dqn.replay_priorities()
    assert all(q1[i] != q0[i] for i in idx) and total == int(q1.astype(np.int64).sum())
    assert (q1 == q0).sum() == len(q0) - len(set(idx.tolist()))
    # a dataset made with priority= keeps it through attach
    d2 = ReplayDataset(None, (4, S, S), dset_size=16, batch_size=B, mode="cpu",
                       priority={"alpha": 0.3})
    other = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    d2.attach(other)
    assert other.replay_priority()["alpha"] == pytest.approx(0.3)
    dset.set_priority(None)
    assert net.dqn.replay_priority() is None
    with pytest.raises(ValueError):
        ReplayDataset(None, (4, S, S), dset_size=16, batch_size=B, mode="cpu",
                      priority={"gamma": 1})


def test_worker_flags():
    from ddq.barista import main
    a = main.get_args(["arch", "model"])
    assert main.priority_of(a) is None
    a = main.get_args(["arch", "model", "--per-alpha", "0.6"])
    assert main.priority_of(a) == {"alpha": 0.6, "beta": 0.4, "eps": 0.01}
    a = main.get_args(["arch", "model", "--per-alpha", "1", "--per-beta", "0", "--per-eps", "1e-3"])
    assert main.priority_of(a) == {"alpha": 1.0, "beta": 0.0, "eps": 1e-3}
    for bad in (["--per-alpha", "1.5"], ["--per-alpha", "-0.1"], ["--per-beta", "0.4"],
                ["--per-eps", "0.1"], ["--per-alpha", "0.5", "--per-beta", "2"],
                ["--per-alpha", "0.5", "--per-eps", "0"], ["--per-alpha", "0.5", "--per-eps", "-1"]):
        with pytest.raises(SystemExit):
            main.get_args(["arch", "model"] + bad)
