"""n-step returns (ddq_replay_set_nstep) on the CPU twin: the entry points and
their error codes, the windowed gather bit for bit against tests/_nstep_ref.py
on hand-built rings, the allowed start slots (exhaustively), the size check at
its boundary, one full pass on an n = 3 minibatch, and ReplayDataset(n_step=).
S = 16, B = 4 throughout.
"""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import _nstep_ref as nr
import _objective_ref as objr
import _pool_host as ph
from _parity import check_full_pass
from oracle import ref_numpy as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, B = 16, 4


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    from ddq import _lib
    if not os.path.exists(_lib.CPU_LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "distributed-deep-q_amd"),
                        "ddq/_lib/libddq_cpu.so"], check=True)
    return m


def make_net(ddq, ring, head, valid, lanes=1, n=None):
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    st, ac, rw, nt = ring
    net.replay_create(len(ac))
    if lanes > 1:
        net.replay_set_lanes(lanes)
    net.replay_import(st, ac, rw, np.asarray(nt, np.uint8), head, valid)
    if n is not None:
        net.replay_set_nstep(n)
    return net


def code_of(call):
    from ddq import _lib
    with pytest.raises(_lib.DDQError) as ei:
        call()
    return ei.value.code


# ---------------------------------------------------------------- restatement
def test_restated_draw_is_the_pool_hosts_at_n1():
    for seed, ctr, head, valid, lanes in [(5, 0, 0, 40, 1), (5, 3, 17, 40, 1), (9, 11, 3, 7, 3),
                                          (2 ** 63 + 1, 7, 6, 6, 4), (77, 2, 1, 30, 1)]:
        L = valid + 2
        np.testing.assert_array_equal(nr.draw_sorted(seed, ctr, 4, head, valid, lanes, L, 1),
                                      ph.draw_sorted(seed, ctr, 4, head, valid, lanes, L))
    for seed, ctr, head, valid, lanes in [(5, 0, 0, 200, 1), (6, 4, 100, 200, 1), (7, 9, 3, 60, 3),
                                          (8, 1, 1, 90, 1)]:
        L = valid + 1
        np.testing.assert_array_equal(nr.draw_sorted_wide(seed, ctr, 72, head, valid, lanes, L, 1),
                                      ph.draw_sorted_wide(seed, ctr, 72, head, valid, lanes, L))


def test_allowed_count_is_the_predicates():
    for L in (6, 12):
        for n in range(1, 6):
            for v in range(1, L + 1):
                for h in range(0, L):
                    if n == 1 and h > v:
                        continue                      # v - 1 counts slot h - 1 as filled
                    a = len(nr.allowed_slots(h, v, L, n))
                    if n == 1 and h == 0:
                        assert a == v                 # nothing forbidden; A keeps v - 1
                    else:
                        assert a == nr.allowed_count(h, v, L, n), (L, n, v, h)


def test_gather_restatement_at_n1_is_the_lane_gather():
    rng = np.random.default_rng(3)
    ring = nr.build_ring(rng, 18, S, (3, 4, 10, 17), nr.REWARDS)
    for L in (18, 6):
        idx = [0, 5, 11, 17]
        for a, b in zip(nr.gather(ring, idx, L, 1), ph.lane_gather(ring, idx, L)):
            assert np.array_equal(a, b) and a.dtype == b.dtype


# ---------------------------------------------------------------- entry points
def test_set_nstep_round_trip_and_errors(ddq):
    from ddq import _lib
    assert {"ddq_replay_set_nstep", "ddq_replay_nstep"} <= set(_lib.EXPORTED)
    # the binding's copy of DDQ_NSTEP_MAX (the worker's --n-step check reads it) is
    # the header's
    header = open(os.path.join(ROOT, "include", "ddq_hip.h")).read()
    assert int(re.search(r"#define\s+DDQ_NSTEP_MAX\s+(\d+)", header).group(1)) == _lib.NSTEP_MAX
    from ddq.barista import main as bm
    assert bm.NSTEP_MAX is _lib.NSTEP_MAX
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    assert code_of(lambda: net.replay_set_nstep(2)) == _lib.DDQ_ESTATE      # no ring
    assert code_of(net.replay_nstep) == _lib.DDQ_ESTATE
    net.replay_create(12)
    assert net.replay_nstep() == 1                                        # create: n = 1
    for n in (1, 2, 8, 3):
        net.replay_set_nstep(n)
        assert net.replay_nstep() == n
    for bad in (0, -1, 9, 12, 100):
        assert code_of(lambda: net.replay_set_nstep(bad)) == _lib.DDQ_EINVAL, bad
        assert net.replay_nstep() == 3
    # lanes: lane_len must stay above n
    assert code_of(lambda: net.replay_set_lanes(4)) == _lib.DDQ_EINVAL      # lane_len 3 == n
    assert code_of(lambda: net.replay_set_lanes(6)) == _lib.DDQ_EINVAL      # lane_len 2 < n
    net.replay_set_lanes(3)                                               # lane_len 4
    assert net.replay_lanes() == (3, 4) and net.replay_nstep() == 3
    assert code_of(lambda: net.replay_set_nstep(4)) == _lib.DDQ_EINVAL      # n >= lane_len
    net.close()
    # a small ring bounds n by its capacity
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    net.replay_create(5)
    net.replay_set_nstep(4)
    assert code_of(lambda: net.replay_set_nstep(5)) == _lib.DDQ_EINVAL
    net.close()
    # legal on a filled ring
    rng = np.random.default_rng(0)
    net = make_net(ddq, nr.build_ring(rng, 12, S), 5, 12)
    net.replay_set_nstep(5)
    assert net.replay_nstep() == 5
    net.close()


# ---------------------------------------------------------------- the gather
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_gather_is_the_restatement(ddq, n):
    rng = np.random.default_rng(40 + n)
    ms, ws, k_eq_n_terminal, two_terminals, wrapped = set(), set(), 0, 0, set()
    for name, cap, lanes, head, valid, terms in nr.RINGS:
        L = cap // lanes
        if lanes * nr.allowed_count(head, valid, L, n) < B:
            assert (name, n) == ("laned 3x6", 5)
            continue
        ring = nr.build_ring(rng, cap, S, terms, nr.REWARDS)
        net = make_net(ddq, ring, head, valid, lanes, n)
        allowed = nr.allowed_slots(head, valid, L, n, lanes)
        for idx in nr.index_lists(allowed):
            net.replay_sample(np.asarray(idx, np.int32))
            want = nr.gather(ring, idx, L, n, with_m=True)
            nr.assert_minibatch(net.read_minibatch(), want[:5], "%s n %d %s" % (name, n, idx))
            for i, m, w in zip(idx, want[5], want[4].ravel()):
                ms.add(m)
                ws.add(float(w))
                x = i % L
                win = [(i // L) * L + (x + k) % L for k in range(1, n + 1)]
                nterm = sum(ring[3][s] == 0 for s in win)
                k_eq_n_terminal += (m == n and w == 0 and n > 1)
                two_terminals += (nterm >= 2 and ring[3][win[0]] != 0)
                if x + m >= L:
                    wrapped.add(name)
        net.close()
    # every branch was taken: every cut length, both values of w, a terminal at
    # k = n, two terminals in one window (the first wins), windows across the
    # end of the ring and of a lane
    assert ms == set(range(1, n + 1)), ms
    gn = np.float32(1.0)
    for _ in range(n - 1):
        gn = np.float32(gn * nr.GAMMA)
    assert ws == {0.0, float(gn)}, ws
    if n > 1:
        assert k_eq_n_terminal >= 1
        assert "full h5" in wrapped, wrapped
    if n in (2, 3):     # (at n = 5 the terminals 7, 8 cut every window of the h = 1 ring short)
        assert {"full h1", "laned 3x6"} <= wrapped, wrapped
    if n >= 3:
        assert two_terminals >= 1


def test_set_back_to_one_is_a_context_that_never_called_it(ddq):
    rng = np.random.default_rng(8)
    ring = nr.build_ring(rng, 12, S, nr.TERMINALS, nr.REWARDS)
    a, b = make_net(ddq, ring, 5, 12), make_net(ddq, ring, 5, 12, n=3)
    b.replay_set_nstep(1)
    for idx in ([0, 1, 2, 3], [5, 7, 10, 11], [2, 3, 6, 9]):     # 3 = head - 2: fine at n = 1
        a.replay_sample(np.asarray(idx, np.int32))
        b.replay_sample(np.asarray(idx, np.int32))
        for x, y in zip(a.read_minibatch(), b.read_minibatch()):
            assert x.tobytes() == y.tobytes()
    a.close()
    b.close()


# ---------------------------------------------------------------- allowed slots
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("cap,lanes", [(12, 1), (18, 3)])
def test_replay_sample_accepts_exactly_the_allowed_slots(ddq, cap, lanes, n):
    from ddq import _lib
    rng = np.random.default_rng(1)
    ring = nr.build_ring(rng, cap, S)
    L = cap // lanes
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    net.replay_create(cap)
    if lanes > 1:
        net.replay_set_lanes(lanes)
    net.replay_set_nstep(n)
    st, ac, rw, nt = ring
    checked = 0
    for valid in range(1, L + 1):
        for head in range(0, L if valid == L else valid + 1):
            if head >= L:
                continue
            net.replay_import(st, ac, rw, nt, head, valid)
            allowed = nr.allowed_slots(head, valid, L, n, lanes)
            assert len(allowed) == lanes * nr.allowed_count(head, valid, L, n)
            if len(allowed) < B:
                # the size check comes first: every list is refused
                if valid * lanes >= B:
                    idx = np.arange(B, dtype=np.int32)
                    assert code_of(lambda: net.replay_sample(idx)) == _lib.DDQ_EINVAL
                continue
            filled = [g * L + x for g in range(lanes) for x in range(valid)]
            for s in filled:
                others = [a for a in allowed if a != s][:B - 1]
                idx = np.asarray(sorted(others + [s]), np.int32)
                if s in allowed:
                    net.replay_sample(idx)
                else:
                    assert code_of(lambda: net.replay_sample(idx)) == _lib.DDQ_EINVAL, (head, valid, s)
                checked += 1
    assert checked > 50
    net.close()


@pytest.mark.parametrize("cap,lanes,head,valid,n,ok", [
    (12, 1, 7, 7, 3, True),     # partial, A = 7 - 3 = 4 == B
    (12, 1, 6, 6, 3, False),    # A = 3 == B - 1
    (7, 1, 2, 7, 3, True),      # full, A = L - n = 4
    (6, 1, 2, 6, 3, False),     # A = 3
    (8, 2, 1, 4, 2, True),      # 2 lanes x (4 - 2)
    (9, 3, 1, 3, 2, False),     # 3 lanes x (3 - 2) = 3
    (12, 1, 2, 6, 3, True),     # partial with head inside: 6 - |[0, 1]| = 4
    (12, 1, 3, 6, 3, False),    # 6 - |[0, 2]| = 3
])
def test_size_check_at_its_boundary(ddq, cap, lanes, head, valid, n, ok):
    from ddq import _lib
    rng = np.random.default_rng(2)
    L = cap // lanes
    net = make_net(ddq, nr.build_ring(rng, cap, S), head, valid, lanes, n)
    allowed = nr.allowed_slots(head, valid, L, n, lanes)
    assert len(allowed) == (B if ok else B - 1)
    if ok:
        net.replay_sample(np.asarray(allowed, np.int32))
    else:
        idx = np.asarray(sorted(allowed + [min(set(range(valid)) - set(allowed))]), np.int32)
        with pytest.raises(_lib.DDQError) as ei:
            net.replay_sample(idx)
        assert ei.value.code == _lib.DDQ_EINVAL and "Can't draw sample" in ei.value.msg
    net.close()


# ---------------------------------------------------------------- the pass
def test_forward_backward_on_an_n3_minibatch(ddq):
    rng = np.random.default_rng(77)
    pQ = ref.init_params(S, seed=7, prefix="Q")
    pP = ref.init_params(S, seed=8, prefix="P")
    for p in (pQ, pP):
        for k in p:
            p[k][0] = (p[k][0] * 3).astype(np.float32)
            p[k][1] = rng.normal(0, 0.05, p[k][1].shape).astype(np.float32)
    cap = 12
    st = rng.choice(np.array([0, 200, 255], np.uint8), (cap, 4, S, S), p=[0.9, 0.08, 0.02])
    ring = (st,) + nr.build_ring(rng, cap, S, (4,), {2: 3, 3: -2, 9: 5})[1:]
    net = make_net(ddq, ring, 0, cap, n=3)
    params = dict(pQ)
    params.update(pP)
    net.set_params(params)
    idx = [0, 2, 5, 7]                 # 2: the terminal 4 mid-window (m = 2); 0: none of its slots
    net.replay_sample(np.asarray(idx, np.int32))
    want = nr.gather(ring, idx, cap, 3, with_m=True)
    assert want[5] == [3, 2, 3, 3] and want[4].ravel()[1] == 0 and want[4].ravel()[0] != 0
    mb = net.read_minibatch()
    nr.assert_minibatch(mb, want[:5])
    loss = net.forward_backward()
    got = objr.blobs_of(net)
    act = mb[1].reshape(B, 4)
    w, R = mb[4].reshape(B), mb[2].reshape(B)
    e = objr.expected_head_f32(got, act, w, R, ref.GAMMA, "max", None)
    # P_sa carries w; target_Q_sa = gamma * (P_sel * w) + R, one rounding of the
    # double sum (the twin's head); the loss from the twin's own Q_sa and target
    assert got["P_sa"].tobytes() == e["P_sa"].tobytes()
    assert got["target_Q_sa"].tobytes() == e["target64"].astype(np.float32).tobytes()
    acc = 0.0
    for b in range(B):
        d = float(got["Q_sa"][b]) - float(got["target_Q_sa"][b])
        acc += d * d
    assert got["loss"][0] == np.float32(acc / B / 2.0) and loss == float(got["loss"][0])
    # the target is the 3-step one: not what the single-step scalars give
    assert np.any(got["target_Q_sa"] != np.float32(ref.GAMMA) * got["P_out"].max(axis=1)
                  * ring[3][np.asarray(idx) + 1] + ring[2][np.asarray(idx) + 1])
    check_full_pass(ref, net, pQ, pP, mb)
    net.close()


# ---------------------------------------------------------------- ReplayDataset
def test_replay_dataset_n_step_draw(ddq, tmp_path):
    from ddq.replay import ReplayDataset
    rng = np.random.default_rng(4)
    cap = 12
    ring = nr.build_ring(rng, cap, S, nr.TERMINALS)
    ds = ReplayDataset(None, (4, S, S), dset_size=cap, batch_size=B, mode="cpu", n_step=3)
    assert ds._net.replay_nstep() == 3
    ds._net.replay_import(ring[0], ring[1], ring[2], ring[3], 5, cap)
    forbidden = lambda x: nr.forbidden(x, 5, cap, cap, 3)       # noqa: E731
    random.seed(11)
    drawn, redraws = [ds.draw_indices(B) for _ in range(20)], 0
    random.seed(11)
    for got in drawn:                      # the reference's whole-list redraw, restated
        idx = random.sample(range(0, cap), B)
        while any(forbidden(x) for x in idx):
            idx = random.sample(range(0, cap), B)
            redraws += 1
        assert got == sorted(idx)
        nr.check_allowed(got, 5, cap, 1, cap, 3)
    assert redraws >= 1
    st = ds.sample(B)
    assert st[0].shape == (B, 4, S, S)
    # too few allowed slots: the reference's ValueError
    ds._net.replay_import(ring[0], ring[1], ring[2], ring[3], 6, 6)   # A = 3
    with pytest.raises(ValueError, match="Can't draw sample of size 4"):
        ds.draw_indices(B)
    # attach carries n to the new context
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    ds.attach(net)
    assert net.replay_nstep() == 3 and net.replay_info() == (6, 6, cap)
    net.close()


def test_worker_n_step_flag(ddq, tmp_path):
    from ddq.barista import main as bm
    from ddq.barista.baristanet import BaristaNet
    from ddq.replay import ReplayDataset
    base = ["arch", "none", "--mode", "cpu", "--driver", "None", "--overwrite",
            "--dset-size", "24", "--initial-replay", "12", "--dataset", str(tmp_path / "r.hdf5")]
    assert bm.get_args(base).n_step == 1
    for bad in ("0", "9", "24", "-1"):          # < 1, > DDQ_NSTEP_MAX, >= --dset-size
        with pytest.raises(SystemExit):
            bm.get_args(base + ["--n-step", bad])
    assert bm.get_args(base + ["--n-step", "8"]).n_step == 8
    args = bm.get_args(base + ["--n-step", "3"])
    args.architecture = {"batch": B, "frame": S}
    net, replay, xp = bm.build_worker(args)
    assert net.dqn.replay_nstep() == 3
    xp.generate_experience(net.fetch_model())
    net.load_minibatch()
    head, valid, cap = net.dqn.replay_info()
    nr.check_allowed(net.dqn.read_indices(), head, valid, 1, cap, 3)
    net.full_pass()
    assert np.any(net.dqn.get_grads_flat() != 0)
    replay.close()
    bn = BaristaNet({"batch": B, "frame": S}, None, None, mode="cpu", n_step=2)
    ds = ReplayDataset(None, (4, S, S), dset_size=12, batch_size=B, mode="cpu")
    bn.add_dataset(ds)
    assert bn.dqn.replay_nstep() == 2 and ds.n_step == 2


# ---------------------------------------------------------------- device actors
def test_device_actors_feed_n_step_rings(ddq):
    """DeviceActor / DeviceActorPool need no change: they write the ring the same
    at any n, and the windows run along what they wrote (one trajectory a ring,
    or a lane)."""
    import _actor_host as ah
    from ddq.actor import DeviceActor, DeviceActorPool
    rings = {}
    for n in (1, 3):
        net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
        th = ah.seeded_theta(S)
        net.set_flat(0, th)
        net.set_flat(1, th)
        net.replay_create(24)
        net.replay_set_nstep(n)
        DeviceActor(net, ah.init_boards()["start"], seed=9).fill(30)     # wraps: head 6
        rings[n] = net.replay_export()
        if n == 3:
            assert net.replay_info() == (6, 24, 24)
            assert (~rings[n][3]).any()                                   # a game ended
            for idx in nr.index_lists(nr.allowed_slots(6, 24, 24, 3)):
                net.replay_sample(np.asarray(idx, np.int32))
                nr.assert_minibatch(net.read_minibatch(), nr.gather(rings[n], idx, 24, 3))
        net.close()
    for a, b in zip(rings[1], rings[3]):
        np.testing.assert_array_equal(a, b)
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    th = ah.seeded_theta(S)
    net.set_flat(0, th)
    net.set_flat(1, th)
    net.replay_create(21)
    net.replay_set_lanes(3)
    net.replay_set_nstep(2)
    pool = DeviceActorPool(net, ph.three_boards(), 21)
    pool.fill(9)                                                          # wraps: head 2
    assert net.replay_info() == (2, 7, 21)
    ring = net.replay_export()
    for idx in nr.index_lists(nr.allowed_slots(2, 7, 7, 2, 3)):
        net.replay_sample(np.asarray(idx, np.int32))
        nr.assert_minibatch(net.read_minibatch(), nr.gather(ring, idx, 7, 2))
    net.close()
