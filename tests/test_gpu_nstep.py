"""n-step returns on the device (ddq_replay_set_nstep): the windowed gather and
the head-aware index draw at every call site -- the eager launches, the graph
and pipelined chains' own draw / gather workgroups (S = 16 small-map path and
S = 24 general kernels), the large-batch sampler -- against tests/_nstep_ref.py,
bit for bit; the three step modes byte-identical at n = 3; n = 1 left as it was.
"""
from fractions import Fraction

import numpy as np
import pytest

import _nstep_ref as nr
import _objective_ref as objr
from _parity import check_full_pass, close as pclose

pytestmark = pytest.mark.gpu

B = 4
SEED = 13


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


def make_net(ddq, S, ring, head, valid, lanes=1, n=None, batch=B, theta=None):
    from ddq.params import init_params_flat
    net = ddq.DeepQNet(batch=batch, frame=S)
    th = init_params_flat(S, seed=42) if theta is None else theta
    net.set_flat(0, th)
    net.set_flat(1, th)
    net.replay_create(len(ring[1]))
    if lanes > 1:
        net.replay_set_lanes(lanes)
    net.replay_import(ring[0], ring[1], ring[2], np.asarray(ring[3], np.uint8), head, valid)
    if n is not None:
        net.replay_set_nstep(n)
    return net


def done(*nets):
    for net in nets:
        net.synchronize()
        net.close()


# ------------------------------------------------------------------ the gather
@pytest.mark.parametrize("S", [16, 24])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_gather_is_the_restatement(ddq, S, n):
    rng = np.random.default_rng(40 + n)
    ms, ws = set(), set()
    for name, cap, lanes, head, valid, terms in nr.RINGS:
        L = cap // lanes
        if lanes * nr.allowed_count(head, valid, L, n) < B:
            continue
        ring = nr.build_ring(rng, cap, S, terms, nr.REWARDS)
        net = make_net(ddq, S, ring, head, valid, lanes, n)
        assert net.small_path()[0] == (S == 16)
        for idx in nr.index_lists(nr.allowed_slots(head, valid, L, n, lanes)):
            net.replay_sample(np.asarray(idx, np.int32))
            want = nr.gather(ring, idx, L, n, with_m=True)
            nr.assert_minibatch(net.read_minibatch(), want[:5], "%s n %d %s" % (name, n, idx))
            ms |= set(want[5])
            ws |= {float(w) for w in want[4].ravel()}
        done(net)
    assert ms == set(range(1, n + 1)) and len(ws) == 2 and 0.0 in ws


def test_refusals_on_the_device_library(ddq):
    from ddq import _lib
    rng = np.random.default_rng(0)
    ring = nr.build_ring(rng, 12, 16)

    def code_of(call):
        with pytest.raises(_lib.DDQError) as ei:
            call()
        return ei.value.code

    net = ddq.DeepQNet(batch=B, frame=16)
    assert code_of(lambda: net.replay_set_nstep(2)) == _lib.DDQ_ESTATE
    net.close()
    net = make_net(ddq, 16, ring, 5, 12)
    assert net.replay_nstep() == 1
    for bad in (0, 9, 12):
        assert code_of(lambda: net.replay_set_nstep(bad)) == _lib.DDQ_EINVAL
    net.replay_set_nstep(3)
    assert net.replay_nstep() == 3
    for s in range(12):                         # forbidden at h = 5: slots 4, 3, 2
        idx = np.asarray(sorted({s} | set([6, 7, 8, 9][:3] if s not in (6, 7, 8) else [9, 10, 11])),
                         np.int32)
        if s in (2, 3, 4):
            assert code_of(lambda: net.replay_sample(idx)) == _lib.DDQ_EINVAL
        else:
            net.replay_sample(idx)
    done(net)
    # the size check at its boundary (A = 7 - 3 == B; A = 6 - 3 == B - 1)
    net = make_net(ddq, 16, ring, 7, 7, n=3)
    net.replay_sample_device(SEED)
    net.step(net.step_cfg("sgd", lr=1e-6, seed=SEED))
    net.synchronize()
    net.replay_import(ring[0], ring[1], ring[2], ring[3], 6, 6)
    cfg = net.step_cfg("sgd", lr=1e-6, seed=SEED)
    for call in (lambda: net.replay_sample_device(SEED), lambda: net.step(cfg),
                 lambda: net.step_graph(cfg, 2), lambda: net.step_pipelined(cfg, 2)):
        assert code_of(call) == _lib.DDQ_EINVAL
    done(net)
    net = ddq.DeepQNet(batch=B, frame=16)
    net.replay_create(12)
    net.replay_set_nstep(3)
    assert code_of(lambda: net.replay_set_lanes(4)) == _lib.DDQ_EINVAL
    net.replay_set_lanes(3)
    done(net)


# ------------------------------------------------------------------ the draw
# (name, capacity, lanes, head, valid, batch, sample_device draws, eager steps)
DRAW_CASES = [("partial", 24, 1, 14, 14, B, 24, 8), ("full h1", 24, 1, 1, 24, B, 40, 8),
              ("laned 3x7", 21, 3, 2, 7, B, 24, 8), ("wide", 200, 1, 57, 200, 72, 24, 4)]


def planned_draws(case, first=0, n=3):
    _, cap, lanes, head, valid, batch, nd, ne = case
    L = cap // lanes
    return [nr.draw(SEED, first + d, batch, head, valid, lanes, L, n) for d in range(nd + ne)]


@pytest.mark.parametrize("case", DRAW_CASES, ids=[c[0] for c in DRAW_CASES])
def test_restatement_alone_covers_every_allowed_slot(case):
    """On the CPU first: the planned draws hit every allowed slot and no other."""
    _, cap, lanes, head, valid, batch, nd, ne = case
    L = cap // lanes
    seen = set()
    for idx in planned_draws(case):
        nr.check_allowed(idx, head, valid, lanes, L, 3)
        seen |= {int(i) for i in idx}
    assert seen == set(nr.allowed_slots(head, valid, L, 3, lanes))


# the bitonic draw (B = 72) is one code path: S = 16 runs it
DEVICE_DRAWS = [(S, c) for c in DRAW_CASES for S in (16, 24) if c[5] <= 64 or S == 16]


@pytest.mark.parametrize("S,case", DEVICE_DRAWS, ids=["%d-%s" % (S, c[0]) for S, c in DEVICE_DRAWS])
def test_device_draws_are_the_restatement(ddq, S, case):
    name, cap, lanes, head, valid, batch, nd, ne = case
    L = cap // lanes
    rng = np.random.default_rng(cap)
    ring = nr.build_ring(rng, cap, S, [s for s in range(cap) if s % 5 == 3])
    net = make_net(ddq, S, ring, head, valid, lanes, 3, batch=batch)
    net.index_log_enable(nd + ne)
    first = net.replay_draws()
    want = planned_draws(case, first)
    for d in range(nd):
        net.replay_sample_device(SEED)
        if d % 8 == 0:
            np.testing.assert_array_equal(net.read_indices(), want[d])
            nr.assert_minibatch(net.read_minibatch(), nr.gather(ring, want[d], L, 3))
    cfg = net.step_cfg("sgd", lr=1e-6, target_period=10, seed=SEED)
    for _ in range(ne):
        net.step(cfg)
    net.synchronize()
    assert net.replay_draws() == first + nd + ne
    log = net.index_log(first, nd + ne)
    seen = set()
    for d in range(nd + ne):
        np.testing.assert_array_equal(log[d], want[d])
        seen |= {int(i) for i in log[d]}
    assert seen == set(nr.allowed_slots(head, valid, L, 3, lanes))
    # the last step's minibatch is still bound
    np.testing.assert_array_equal(net.read_indices(), want[-1])
    nr.assert_minibatch(net.read_minibatch(), nr.gather(ring, want[-1], L, 3))
    net._check(net.lib.ddq_replay_status(net.ctx))
    done(net)


# ------------------------------------------------------------------ step modes
STEP_N, STEPS = 48, 9
_RING, _CHAINS = {}, {}


def ring_for(S):
    if S not in _RING:
        from ddq.expgain import synthetic_transitions
        st, ac, rw, nt = synthetic_transitions(STEP_N, S, seed=77)
        assert 2 <= int((~nt).sum()) < STEP_N // 3           # windows with and without a terminal
        _RING[S] = (st, ac, rw, nt)
    return _RING[S]


def theta_for(S):
    """The prototxt fillers (bench.py's weights): rmsprop at the bench's 1e-4 is
    stable on them, which it is not on the parity tests' scaled-up weights."""
    from ddq.params import init_params_flat
    return init_params_flat(S, seed=42)


LR = 1e-4


def chain(ddq, ref, S, mode, nsteps):
    """Nine steps (eager: 1 + 8; graph / pipelined: an 8-step graph and a tail)
    on a fresh ctx; nsteps None: never set, (3, 1): set to 3 and back."""
    key = (S, mode, nsteps)
    if key in _CHAINS:
        return _CHAINS[key]
    ring = ring_for(S)
    th = theta_for(S)
    net = make_net(ddq, S, ring, 5, STEP_N, theta=th)
    for n in (nsteps if isinstance(nsteps, tuple) else () if nsteps is None else (nsteps,)):
        net.replay_set_nstep(n)
    net.index_log_enable(16)
    cfg = net.step_cfg("rmsprop", lr=LR, target_period=5, seed=11)
    out = {}
    if mode == "eager":
        net.step(cfg)
        net.synchronize()
        out["first"] = dict(idx=net.read_indices(), mb=net.read_minibatch(),
                            grads=net.get_grads_flat(), theta=net.get_flat(0))
        if nsteps == 3:
            # the first step against the oracle's, on the restatement's minibatch
            idx = out["first"]["idx"]
            np.testing.assert_array_equal(idx, nr.draw(11, 0, B, 5, STEP_N, 1, STEP_N, 3))
            mb = nr.gather(ring, idx, STEP_N, 3)
            nr.assert_minibatch(out["first"]["mb"], mb)
            check_full_pass(ref, net, ref.unflatten(th, S, "Q"), ref.unflatten(th, S, "P"), mb,
                            grads_gpu=out["first"]["grads"], what="n=3 step 1 ")
            th_ref, _ = ref.rmsprop_update(th, out["first"]["grads"], None, LR)
            pclose(out["first"]["theta"], th_ref, what="theta after step 1")
        for _ in range(STEPS - 1):
            net.step(cfg)
    elif mode == "graph":
        net.step_graph(cfg, 8)
        net.step_graph(cfg, 1)
    else:
        net.step_pipelined(cfg, 8)
        net.step_pipelined(cfg, 1)
    net.synchronize()
    out["state"] = [net.get_flat(0), net.get_flat(1), net.optimizer_state()]
    assert all(np.isfinite(s).all() for s in out["state"])
    out["log"] = net.index_log(0, STEPS)
    out["mb"] = net.read_minibatch()
    net._check(net.lib.ddq_replay_status(net.ctx))
    done(net)
    _CHAINS[key] = out
    return out


@pytest.mark.parametrize("S", [16, 24])
def test_step_modes_agree_at_n3(ddq, ref, S):
    eager = chain(ddq, ref, S, "eager", 3)
    ring = ring_for(S)
    ms = set()
    for d in range(STEPS):
        np.testing.assert_array_equal(eager["log"][d],
                                      nr.draw(11, d, B, 5, STEP_N, 1, STEP_N, 3))
        ms |= set(nr.gather(ring, eager["log"][d], STEP_N, 3, with_m=True)[5])
    assert ms == {1, 2, 3}                               # the chain saw cut and whole windows
    for mode in ("graph", "pipelined"):
        other = chain(ddq, ref, S, mode, 3)
        for a, b in zip(eager["state"], other["state"]):
            assert a.tobytes() == b.tobytes(), mode
        assert eager["log"].tobytes() == other["log"].tobytes()
        nr.assert_minibatch(other["mb"], nr.gather(ring, other["log"][-1], STEP_N, 3), mode)
    plain = chain(ddq, ref, S, "pipelined", None)
    assert plain["state"][0].tobytes() != eager["state"][0].tobytes()
    assert eager["state"][0].tobytes() != theta_for(S).tobytes()


@pytest.mark.parametrize("S", [16, 24])
def test_off_is_off(ddq, ref, S):
    never = chain(ddq, ref, S, "pipelined", None)
    one = chain(ddq, ref, S, "pipelined", 1)
    back = chain(ddq, ref, S, "pipelined", (3, 1))
    for other in (one, back):
        for a, b in zip(never["state"], other["state"]):
            assert a.tobytes() == b.tobytes()
        assert never["log"].tobytes() == other["log"].tobytes()
        for a, b in zip(never["mb"], other["mb"]):
            assert a.tobytes() == b.tobytes()
    import _pool_host as ph
    for d in range(STEPS):
        np.testing.assert_array_equal(never["log"][d], ph.draw_sorted(11, d, B, 5, STEP_N))


# ------------------------------------------------------------------ large batch
def test_large_batch_sampler_and_gather(ddq):
    import torch
    from ddq import _lib
    S, N, n = 16, 400, 64
    rng = np.random.default_rng(5)
    ring = nr.build_ring(rng, N, S, [s for s in range(N) if s % 7 == 2 or s % 31 == 3])
    ring[2][:] = rng.integers(-3, 4, N)
    net = make_net(ddq, S, ring, 123, N, n=3)
    bufs = net.batch_buffers(n)
    seen_m = set()
    for _ in range(3):
        net.replay_sample_batch(bufs, seed=77)
        out = {k: v.cpu().numpy() for k, v in bufs.items()}
        idx = out["idx"].astype(np.int64)
        assert idx.size == n
        nr.check_allowed(idx, 123, N, 1, N, 3)
        want = nr.gather(ring, idx, N, 3, with_m=True)
        nr.assert_minibatch([out[k] for k in ("state", "action", "reward", "next_state",
                                              "non_terminal")], want[:5])
        seen_m |= set(want[5])
    assert seen_m == {1, 2, 3}
    # a given list: the allowed slots around the wrap and the head
    idx = np.asarray(sorted(set(range(390, 400)) | set(range(0, 12)) | set(range(100, 120))
                            | set(range(123, 145)))[:n], np.int32)
    assert idx.size == n
    nr.check_allowed(idx, 123, N, 1, N, 3)
    bufs["idx"].copy_(torch.from_numpy(idx))
    torch.cuda.current_stream(bufs["idx"].device).synchronize()
    net.replay_gather_batch(bufs)
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    nr.assert_minibatch([out[k] for k in ("state", "action", "reward", "next_state",
                                          "non_terminal")], nr.gather(ring, idx, N, 3))
    # the sampler's own bound still comes after the slot count
    with pytest.raises(_lib.DDQError, match="n <= valid/2"):
        net.replay_sample_batch(net.batch_buffers(201), seed=1)
    done(net)


# ------------------------------------------------------------------ actor pool
@pytest.mark.parametrize("S", [16, 24])
def test_actor_pool_feeds_two_step_windows(ddq, S):
    """DeviceActorPool needs no change: its lanes are the trajectories the
    windows run along."""
    import _eval_host as eh
    import _pool_host as ph
    from ddq.actor import DeviceActorPool
    lanes, L, n = 3, 7, 2
    net = ddq.DeepQNet(batch=B, frame=S)
    th = eh.theta(S)
    net.set_flat(0, th)
    net.set_flat(1, th)
    net.replay_create(lanes * L)
    net.replay_set_lanes(lanes)
    net.replay_set_nstep(n)
    pool = DeviceActorPool(net, ph.three_boards(), 21)
    pool.fill(6)                                         # head 6, valid 6: the rounds wrap
    net.index_log_enable(2 * lanes)
    cfg = net.step_cfg("sgd", lr=1e-6, target_period=5, seed=5)
    first = net.replay_draws()
    pool.act_and_train(cfg, 2, 0)
    net.synchronize()
    assert net.replay_info() == (1, L, lanes * L)
    net._check(net.lib.ddq_replay_status(net.ctx))
    log = net.index_log(first, 2 * lanes)
    for r, (h, v) in enumerate(((0, 7), (1, 7))):        # the ring as round r's move left it
        for d in range(lanes):
            k = r * lanes + d
            nr.check_allowed(log[k], h, v, lanes, L, n)
            np.testing.assert_array_equal(log[k], nr.draw(5, first + k, B, h, v, lanes, L, n))
    ring = net.replay_export()
    np.testing.assert_array_equal(net.read_indices(), log[-1])
    nr.assert_minibatch(net.read_minibatch(), nr.gather(ring, log[-1], L, n))
    done(net)


# ------------------------------------------------------------------ the head
def _round_f32(x):
    """The fp32 nearest (ties to even) to the Fraction x."""
    c = np.float32(float(x))
    cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    err = [abs(Fraction(float(v)) - x) for v in cands]
    best = min(err)
    pick = [v for v, e in zip(cands, err) if e == best]
    if len(pick) > 1:
        pick = [v for v in pick if int(np.float32(v).view(np.uint32)) & 1 == 0]
    return np.float32(pick[0])


@pytest.mark.parametrize("S", [16, 24])
def test_double_target_on_an_n3_minibatch(ddq, ref, S):
    ring = ring_for(S)
    net = make_net(ddq, S, ring, 5, STEP_N, n=3, theta=theta_for(S))
    net.set_objective("double")
    nt = ring[3]
    term = [s for s in range(8, 40) if not nt[s]][0]
    idx = sorted({term - 2, term - 1, term + 2, 44})       # terminal at k = 2 and k = 1; none
    assert len(idx) == B
    net.replay_sample(np.asarray(idx, np.int32))
    mb = net.read_minibatch()
    want = nr.gather(ring, idx, STEP_N, 3, with_m=True)
    nr.assert_minibatch(mb, want[:5])
    assert {1, 2} <= set(want[5])
    net.forward_backward()
    got = objr.blobs_of(net, ("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "Qn_out"))
    w, R = mb[4].reshape(B), mb[2].reshape(B)
    assert (w == 0).any() and (w != 0).any()
    e = objr.expected_head_f32(got, mb[1].reshape(B, 4), w, R, ref.GAMMA, "double", None)
    assert got["P_sa"].tobytes() == e["P_sa"].tobytes()
    # target_Q_sa = gamma * P_sa + 1.0f * R: both head kernels are compiled with
    # floating-point contraction on, so this is one fused multiply-add -- the
    # exact gamma * P_sa + R rounded to fp32 once
    g = np.float32(ref.GAMMA)
    fused = np.array([_round_f32(Fraction(float(g)) * Fraction(float(p)) + Fraction(float(r)))
                      for p, r in zip(got["P_sa"], R)], np.float32)
    assert got["target_Q_sa"].astype(np.float32).tobytes() == fused.tobytes()
    done(net)


@pytest.mark.parametrize("batch", [4, 32])
def test_small_path_stays_on(ddq, batch):
    rng = np.random.default_rng(1)
    ring = nr.build_ring(rng, 64, 16)
    net = make_net(ddq, 16, ring, 0, 64, batch=batch)
    assert net.small_path()[0]
    net.replay_set_nstep(3)
    assert net.small_path()[0] and net.replay_nstep() == 3
    net.step_pipelined(net.step_cfg("sgd", lr=1e-6, seed=3), 2)
    done(net)
