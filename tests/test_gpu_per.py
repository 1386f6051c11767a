"""Prioritized replay on the device (ddq_replay_set_priority) against
tests/_per_ref.py: the sum-tree draw exactly (rings of 64 to 5000 slots: three
tree levels with ragged nodes, unfilled tails, four lanes, n = 3), the weights,
the weighted head on the S = 16 four-launch step and the general kernels, the
commit, the invariant under the host adds, the device actor and the actor pool,
the three step modes byte-identical, off is off, the refusals.  Batches of more
than one wave (B = 72 at S = 24, B = 100 and 256 at S = 16; rings of 5000 slots,
four lanes and 600 slots at n = 3): the draw and the weights exactly, the commit
with one slot repeated in every wave; the step modes and off-is-off at B = 100.
"""
import numpy as np
import pytest

import _nstep_ref as nr
import _per_ref as pr
import _pool_host as ph

pytestmark = pytest.mark.gpu

SEED = 2016
PRIO = dict(alpha=0.6, beta=0.4, eps=0.01)
SHAPES = [(16, 4), (16, 32), (32, 4), (32, 32)]
# (name, capacity, lanes, head, valid, n)
RINGS = [("small", 64, 1, 40, 64, 1), ("5000", 5000, 1, 300, 300, 1),
         ("5000 full", 5000, 1, 4990, 5000, 1), ("laned 4x200", 800, 4, 100, 100, 1),
         ("n3", 130, 1, 7, 130, 3)]
# batches of more than one wave (the draw's cross-wave minimum, the commit's scan
# for a later b on the same slot, the 256-thread descent) and the small-map
# step's four image chunks, on rings with room for them
WIDE_SHAPES = [(16, 100), (16, 256), (24, 72)]
WIDE_RINGS = [r for r in RINGS if r[0] in ("5000 full", "laned 4x200")] + \
    [("n3 600", 600, 1, 7, 600, 3)]
_RING = {}


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


def ring_for(cap, S):
    if (cap, S) not in _RING:
        _RING[(cap, S)] = nr.build_ring(np.random.default_rng(cap), cap, S)
    return _RING[(cap, S)]


def make_net(ddq, S, batch, ring, head, valid, lanes=1, n=None, prio=None):
    from ddq.params import init_params_flat
    net = ddq.DeepQNet(batch=batch, frame=S)
    th = init_params_flat(S, seed=42)
    net.set_flat(0, th)
    net.set_flat(1, th)
    net.replay_create(len(ring[1]))
    if lanes > 1:
        net.replay_set_lanes(lanes)
    net.replay_import(ring[0], ring[1], ring[2], np.asarray(ring[3], np.uint8), head, valid)
    if n is not None:
        net.replay_set_nstep(n)
    if prio is not None:
        net.replay_set_priority(**prio)
    return net


def done(*nets):
    for net in nets:
        net.synchronize()
        net.close()


def code_of(call):
    from ddq import _lib
    with pytest.raises(_lib.DDQError) as ei:
        call()
    return ei.value.code


def set_leaves(net, leaves):
    idx = np.asarray(sorted(leaves), np.int32)
    net.replay_set_priorities(idx, np.asarray([leaves[int(i)] for i in idx], np.uint32))


def spread_leaves(allowed):
    """Leaves from 1 to about 2^21 over the allowed slots: distinct weights."""
    return {int(i): 1 + (37 * k * k * 13) % (1 << 21) for k, i in enumerate(allowed)}


# 1, 2 --------------------------------------------------------------- draw, weights
@pytest.mark.parametrize("S,batch", SHAPES)
def test_draw_and_weights_are_the_restatement(ddq, S, batch):
    draw_and_weights(ddq, S, batch, RINGS)


@pytest.mark.parametrize("S,batch", WIDE_SHAPES)
def test_draw_and_weights_across_waves(ddq, S, batch):
    """The descent on 128 and 256 threads, the minimum leaf taken across waves."""
    draw_and_weights(ddq, S, batch, WIDE_RINGS)


def draw_and_weights(ddq, S, batch, rings):
    dup = False
    for name, cap, lanes, head, valid, n in rings:
        L = cap // lanes
        ring = ring_for(cap, S)
        net = make_net(ddq, S, batch, ring, head, valid, lanes, n, PRIO)
        assert net.small_path()[0] == (S == 16)
        q0, total, pmax = net.replay_priorities()
        pr.check_invariant(q0, total, head, valid, L, n, lanes, name)
        assert pmax == pr.ONE
        net.index_log_enable(16)
        ctr = 0
        for cname, leaves in pr.leaf_cases(cap, nr.allowed_slots(head, valid, L, n, lanes)).items():
            set_leaves(net, leaves)
            q, total, got_pmax = net.replay_priorities()
            pmax = max(pmax, max(leaves.values()))
            assert total == sum(leaves.values()) and got_pmax == pmax, (name, cname)
            for _ in range(2):
                net.replay_sample_device(SEED)
                want, T = pr.draw(q, batch, SEED, ctr)
                got = net.read_indices()
                np.testing.assert_array_equal(got, want, (name, cname, ctr))
                np.testing.assert_array_equal(net.index_log(ctr, 1)[0], want)
                ctr += 1
                assert T == total and net.replay_draws() == ctr
                dup |= bool((np.diff(got) == 0).any())
                w = net.blob("is_weight").reshape(batch)
                np.testing.assert_allclose(w, pr.isw64(q, got, PRIO["beta"]), rtol=1e-4)
            nr.assert_minibatch(net.read_minibatch(), nr.gather(ring, got, L, n), (name, cname))
        done(net)
    assert dup, "the 2^24 leaf must be drawn more than once in a set"


def test_beta_zero_weights_are_exactly_one(ddq):
    net = make_net(ddq, 16, 32, ring_for(64, 16), 40, 64, prio=dict(alpha=0.5, beta=0.0, eps=0.1))
    set_leaves(net, spread_leaves([i for i in range(64) if i != 39]))
    net.replay_sample_device(SEED)
    assert net.blob("is_weight").tobytes() == np.ones(32, np.float32).tobytes()
    # the annealing path: the scalars move with no rebuild and no new draw counter
    net.replay_set_priority(alpha=0.5, beta=1.0, eps=0.1)
    q, _, _ = net.replay_priorities()
    net.replay_sample_device(SEED)
    w = net.blob("is_weight").reshape(32)
    np.testing.assert_allclose(w, pr.isw64(q, net.read_indices(), 1.0), rtol=1e-4)
    assert net.replay_draws() == 2 and len(set(w.tolist())) > 4
    done(net)


# 3 ------------------------------------------------------------------ the head
@pytest.mark.parametrize("S,batch", SHAPES)
@pytest.mark.parametrize("loss", ["euclidean", "huber"])
def test_weighted_head_from_the_blobs(ddq, S, batch, loss):
    from oracle import ref_numpy as ref
    ring = ring_for(130, S)
    net = make_net(ddq, S, batch, ring, 7, 130, prio=PRIO)
    set_leaves(net, spread_leaves(nr.allowed_slots(7, 130, 130, 1)))
    net.replay_sample_device(SEED)
    net.forward_backward()
    delta = None
    if loss == "huber":                          # half the images clipped
        d = np.abs(net.blob("Q_sa").reshape(batch).astype(np.float64)
                   - net.blob("target_Q_sa").reshape(batch))
        s = np.sort(d)
        delta = float(np.float32(0.5 * (s[(batch - 1) // 2] + s[batch // 2])))
        net.set_objective("max", "huber", delta)
        net.forward_backward()
    _, w = pr.check_weighted_head(net, ref.GAMMA, "max", delta, "S%d B%d %s " % (S, batch, loss))
    assert len(set(w.tolist())) > 1 and w.max() == 1.0
    done(net)


@pytest.mark.parametrize("S,batch", [(16, 32), (32, 4)])
def test_weight_one_is_the_unweighted_pass(ddq, S, batch):
    ring = ring_for(130, S)
    idx = np.arange(10, 10 + 3 * batch, 3, dtype=np.int32)
    out = []
    for prio in (None, dict(alpha=0.6, beta=0.0, eps=0.01)):
        net = make_net(ddq, S, batch, ring, 7, 130, prio=prio)
        net.replay_sample(idx)
        loss = net.forward_backward()
        out.append([np.float32(loss).tobytes(), net.get_grads_flat().tobytes()] +
                   [net.blob(k).tobytes() for k in ("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa",
                                                    "Q_out.diff")])
        if prio:
            assert net.blob("is_weight").tobytes() == np.ones(batch, np.float32).tobytes()
        done(net)
    assert out[0] == out[1]


# 4 ------------------------------------------------------------------ the commit
@pytest.mark.parametrize("S,batch", SHAPES)
def test_commit_of_one_eager_step(ddq, S, batch):
    commit_of_one_eager_step(ddq, S, batch, 130)


@pytest.mark.parametrize("S,batch", WIDE_SHAPES)
def test_commit_across_waves(ddq, S, batch):
    """One slot fills most of the batch in every wave: the commit's scan for a
    later b on the same slot crosses waves (the copies carry the same TD error,
    so what pr.check_commit holds is one leaf written once, total and pmax
    consistent), and the draw's minimum leaf is taken across the waves."""
    idx = commit_of_one_eager_step(ddq, S, batch, 600)
    waves = {b // 64 for b in range(batch) if idx[b] == 50}
    assert waves == set(range((batch + 63) // 64)), waves


def commit_of_one_eager_step(ddq, S, batch, cap):
    ring = ring_for(cap, S)
    net = make_net(ddq, S, batch, ring, 7, cap, prio=PRIO)
    allowed = nr.allowed_slots(7, cap, cap, 1)
    set_leaves(net, {i: (pr.QMAX if i == 50 else 1) for i in allowed})
    q0, _, pmax0 = net.replay_priorities()
    net.step(net.step_cfg("sgd", lr=1e-6, target_period=5, seed=SEED))
    idx = net.read_indices()
    np.testing.assert_array_equal(idx, pr.draw(q0, batch, SEED, 0)[0])
    assert (np.diff(idx) == 0).any() and net.replay_draws() == 1
    q1, total, pmax1 = net.replay_priorities()
    pr.check_commit(q0, q1, total, pmax0, pmax1, idx, net.blob("Q_sa").reshape(batch),
                    net.blob("target_Q_sa").reshape(batch), PRIO["eps"], PRIO["alpha"],
                    "S%d B%d" % (S, batch))
    done(net)
    return idx


def test_commit_does_not_resurrect_a_forbidden_slot(ddq):
    S = 16
    net = make_net(ddq, S, 4, ring_for(64, S), 40, 64, prio=PRIO)
    net.replay_sample(np.asarray([38, 41, 42, 43], np.int32))
    st = np.zeros((4, S, S), np.uint8)
    net.replay_add(1, 0, st)                     # head 41: slot 40 forbidden, 39 released
    net.replay_add(1, 0, st)                     # head 42: slot 41 forbidden, 40 released
    net.forward_backward()
    qa, _, pa = net.replay_priorities()
    assert qa[41] == 0 and qa[39] == pr.ONE and qa[40] == pr.ONE
    net.replay_update_priorities()
    qb, total, pb = net.replay_priorities()
    pr.check_commit(qa, qb, total, pa, pb, [38, 41, 42, 43], net.blob("Q_sa").reshape(4),
                    net.blob("target_Q_sa").reshape(4), PRIO["eps"], PRIO["alpha"])
    assert qb[41] == 0 and qb[38] != qa[38]
    pr.check_invariant(qb, total, 42, 64, 64, 1)
    done(net)


# 5 ------------------------------------------------------------------ writers
@pytest.mark.parametrize("n", [1, 3])
def test_invariant_under_host_adds(ddq, n):
    cap, S = 8, 16
    net = ddq.DeepQNet(batch=4, frame=S)
    net.replay_create(cap)
    net.replay_set_nstep(n)
    net.replay_set_priority(**PRIO)
    q, pmax = [0] * cap, pr.ONE
    st = np.zeros((4, S, S), np.uint8)
    for k in range(20):
        if k == 9:                               # a larger pmax: released slots take it
            filled = [i for i in range(cap) if q[i]]
            net.replay_set_priorities(np.asarray(filled[:1], np.int32),
                                      np.asarray([3 * pr.ONE], np.uint32))
            q[filled[0]], pmax = 3 * pr.ONE, 3 * pr.ONE
        net.replay_add(k % 4, 0, st if k % 5 else None)
        head, valid, _ = net.replay_info()
        released = pr.writer(q, pmax, 0, k % cap, cap, n, head, valid)
        got, total, gp = net.replay_priorities()
        assert got.tolist() == q and gp == pmax, (k, got.tolist(), q)
        pr.check_invariant(got, total, head, valid, cap, n, 1, "add %d" % k)
        if released is not None:
            assert got[released] == pmax
    done(net)


@pytest.mark.parametrize("n", [1, 3])
def test_invariant_under_the_device_actor(ddq, n):
    import _actor_host as ah
    from ddq.actor import zoom_maps
    cap, S = 8, 16
    net = ddq.DeepQNet(batch=4, frame=S)
    net.set_flat(0, ah.seeded_theta(S))
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
        assert got.tolist() == q, (k, got.tolist(), q)
        pr.check_invariant(got, total, head, valid, cap, n, 1, "actor step %d" % k)
    done(net)


def test_invariant_under_the_actor_pool(ddq):
    import _actor_host as ah
    from ddq.actor import zoom_maps
    lanes, L, S = 4, 8, 16
    net = ddq.DeepQNet(batch=4, frame=S)
    net.set_flat(0, ah.seeded_theta(S))
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
        assert got.tolist() == q, (k, got.tolist(), q)
        pr.check_invariant(got, total, head, valid, L, 1, lanes, "pool move %d" % k)
    done(net)


def test_rebuilds(ddq):
    S = 16
    ring = ring_for(130, S)
    net = make_net(ddq, S, 4, ring, 5, 130, prio=PRIO)

    def rebuilt(head, valid, n):
        q, total, pmax = net.replay_priorities()
        pr.check_invariant(q, total, head, valid, 130, n)
        assert pmax == pr.ONE and set(q.tolist()) == {0, pr.ONE}
        set_leaves(net, {60: 9 * pr.ONE})
        assert net.replay_priorities()[2] == 9 * pr.ONE

    rebuilt(5, 130, 1)
    net.replay_set_nstep(3)
    rebuilt(5, 130, 3)
    net.replay_import(ring[0], ring[1], ring[2], ring[3], 70, 100)
    rebuilt(70, 100, 3)
    net.replay_fill_tiled(ring[0][:9], ring[1][:9], ring[2][:9], ring[3][:9], 3, 130)
    rebuilt(3, 130, 3)
    assert code_of(net.replay_update_priorities) == -5      # a rebuild unbinds the index set
    done(net)


# 6 ------------------------------------------------------------------ step modes
STEPS = 19
_CHAINS = {}
# rmsprop at the bench's 1e-4 is stable on the prototxt fillers at S = 16; at
# S = 32 and B = 4 the same chain overflows within six steps with or without
# prioritization (its first update moves a million weights by lr each), so the
# chain runs at 1e-6 there
LR = {16: 1e-4, 32: 1e-6}


def chain(ddq, S, batch, mode, prio):
    """19 steps from the same start: eager 19 x 1; graph and pipelined 8 + 8 and
    a 3-step tail.  prio: a dict, None (never enabled), or "off" (enabled, then
    disabled)."""
    key = (S, batch, mode, str(prio))
    if key in _CHAINS:
        return _CHAINS[key]
    net = make_net(ddq, S, batch, ring_for(130, S), 7, 130, prio=PRIO if prio == "off" else prio)
    if prio == "off":
        net.replay_set_priority(enabled=False)
    elif prio:
        set_leaves(net, spread_leaves(nr.allowed_slots(7, 130, 130, 1)))
    net.index_log_enable(32)
    cfg = net.step_cfg("rmsprop", lr=LR[S], target_period=5, seed=11)
    if mode == "eager":
        for _ in range(STEPS):
            net.step(cfg)
    elif mode == "graph":
        net.step_graph(cfg, STEPS)
    else:
        net.step_pipelined(cfg, STEPS)
    net.synchronize()
    out = {"state": [net.get_flat(0), net.get_flat(1), net.optimizer_state()],
           "log": net.index_log(0, STEPS), "idx": net.read_indices(),
           "mb": net.read_minibatch(), "draws": net.replay_draws()}
    assert all(np.isfinite(s).all() for s in out["state"])
    if prio and prio != "off":
        out["prio"] = net.replay_priorities()
        out["isw"] = net.blob("is_weight")
    net._check(net.lib.ddq_replay_status(net.ctx))
    done(net)
    _CHAINS[key] = out
    return out


# (16, 100): the small-map step's four image chunks, then prio_commit on two waves
@pytest.mark.parametrize("S,batch", [(16, 32), (32, 4), (16, 100)])
def test_step_modes_agree(ddq, S, batch):
    eager = chain(ddq, S, batch, "eager", PRIO)
    q, total, pmax = eager["prio"]
    assert total == int(q.astype(np.int64).sum()) and eager["draws"] == STEPS
    pr.check_invariant(q, total, 7, 130, 130, 1)
    # the chain committed (B = 100: the ring has 129 leaves, half of them distinct)
    assert len(set(q.tolist())) > min(3 * batch // 2, 64)
    for mode in ("graph", "pipelined"):
        other = chain(ddq, S, batch, mode, PRIO)
        for a, b in zip(eager["state"], other["state"]):
            assert a.tobytes() == b.tobytes(), mode
        assert eager["log"].tobytes() == other["log"].tobytes(), mode
        assert eager["prio"][0].tobytes() == other["prio"][0].tobytes(), mode
        assert eager["prio"][1:] == other["prio"][1:] and other["draws"] == STEPS, mode
        assert eager["idx"].tobytes() == other["idx"].tobytes(), mode
        assert eager["isw"].tobytes() == other["isw"].tobytes(), mode
        for a, b in zip(eager["mb"], other["mb"]):
            assert a.tobytes() == b.tobytes(), mode
    # later draws saw the earlier commits: uniform sampling trains elsewhere
    plain = chain(ddq, S, batch, "pipelined", None)
    assert plain["log"].tobytes() != eager["log"].tobytes()


def test_act_and_train_is_the_eager_sequence(ddq):
    import _actor_host as ah
    from ddq.actor import DeviceActorPool
    lanes, L, S, rounds = 4, 8, 16, 3
    out = []
    for fused in (True, False):
        net = ddq.DeepQNet(batch=4, frame=S)
        th = ah.seeded_theta(S)
        net.set_flat(0, th)
        net.set_flat(1, th)
        net.replay_create(lanes * L)
        net.replay_set_lanes(lanes)
        net.replay_set_priority(**PRIO)
        pool = DeviceActorPool(net, ph.four_boards(), 21)
        pool.fill(7)                                  # the rounds wrap the lanes
        net.index_log_enable(16)
        cfg = net.step_cfg("rmsprop", lr=1e-4, target_period=5, seed=5)
        if fused:
            pool.act_and_train(cfg, rounds, 0)
        else:
            for r in range(rounds):
                net.actors_step(1, r * lanes)
                for _ in range(lanes):
                    net.step(cfg)
        net.synchronize()
        q, total, pmax = net.replay_priorities()
        head, valid, _ = net.replay_info()
        pr.check_invariant(q, total, head, valid, L, 1, lanes)
        out.append([net.get_flat(0).tobytes(), net.optimizer_state().tobytes(), q.tobytes(),
                    total, pmax, net.index_log(0, rounds * lanes).tobytes()])
        done(net)
    assert out[0] == out[1]


# 7 ------------------------------------------------------------------ off is off
@pytest.mark.parametrize("S,batch", [(16, 32), (32, 4), (16, 100)])
def test_off_is_off(ddq, S, batch):
    for mode in ("eager", "graph", "pipelined"):
        never, back = chain(ddq, S, batch, mode, None), chain(ddq, S, batch, mode, "off")
        for a, b in zip(never["state"], back["state"]):
            assert a.tobytes() == b.tobytes(), mode
        assert never["log"].tobytes() == back["log"].tobytes(), mode
        for a, b in zip(never["mb"], back["mb"]):
            assert a.tobytes() == b.tobytes(), mode
    draw = ph.draw_sorted if batch <= 64 else ph.draw_sorted_wide
    for d in range(STEPS):
        np.testing.assert_array_equal(never["log"][d], draw(11, d, batch, 7, 130))
    names = []
    for toggle in (False, True):
        net = make_net(ddq, S, batch, ring_for(130, S), 7, 130)
        if toggle:
            net.replay_set_priority(**PRIO)
            cfg = net.step_cfg("sgd", lr=1e-6, seed=3)
            on = [k for k, _ in net.profile_step(cfg)]
            assert on[:2] == ["prio_sample", "gather"] and on.count("prio_commit") == 1
            head_at = on.index("fc4_chain" if S == 16 else "head")
            assert on[head_at + 1] == "prio_commit"
            assert net.small_path()[0] == (S == 16)
            net.replay_set_priority(enabled=False)
        assert net.small_path()[0] == (S == 16)
        names.append([k for k, _ in net.profile_step(net.step_cfg("sgd", lr=1e-6, seed=3))])
        done(net)
    assert names[0] == names[1] and not any("prio" in k for k in names[0])


# 8 ------------------------------------------------------------------ refusals
def test_refusals_on_the_device_library(ddq):
    from ddq import _lib
    S = 16
    net = ddq.DeepQNet(batch=4, frame=S)
    assert code_of(lambda: net.replay_set_priority(**PRIO)) == _lib.DDQ_ESTATE        # no ring
    net.close()
    ring = ring_for(64, S)
    net = make_net(ddq, S, 4, ring, 5, 5)
    assert net.replay_priority() is None
    for call in (net.replay_priorities, net.replay_update_priorities,
                 lambda: net.replay_set_priorities([0], [1]), lambda: net.blob("is_weight")):
        assert code_of(call) == _lib.DDQ_ESTATE
    for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(beta=-1e-3),
                dict(beta=1.0001), dict(beta=float("inf")), dict(eps=0.0), dict(eps=-1.0),
                dict(eps=float("nan")), dict(eps=float("inf"))):
        assert code_of(lambda: net.replay_set_priority(**dict(PRIO, **bad))) == _lib.DDQ_EINVAL
    net.replay_set_priority(**PRIO)
    for bad in (dict(alpha=2.0), dict(eps=0.0)):                  # while enabled too
        assert code_of(lambda: net.replay_set_priority(**dict(PRIO, **bad))) == _lib.DDQ_EINVAL
    assert net.replay_priority() == {k: pytest.approx(v) for k, v in PRIO.items()}
    sp = net.replay_set_priorities
    assert code_of(lambda: sp([4], [5])) == _lib.DDQ_EINVAL          # nonzero on a zero leaf
    assert code_of(lambda: sp([3], [0])) == _lib.DDQ_EINVAL          # zero on a nonzero leaf
    assert code_of(lambda: sp([3], [pr.QMAX + 1])) == _lib.DDQ_EINVAL
    assert code_of(lambda: sp([64], [5])) == _lib.DDQ_EINVAL
    assert code_of(lambda: sp([-1], [5])) == _lib.DDQ_EINVAL
    sp([3, 4, 3], [7, 0, pr.QMAX])                                # a repeated slot: the last value
    assert net.replay_priorities()[1:] == (3 * pr.ONE + pr.QMAX, pr.QMAX)
    # the size check at its boundary: A = 4 == B; then A = 3
    cfg = net.step_cfg("sgd", lr=1e-6, seed=SEED)
    assert code_of(net.replay_update_priorities) == _lib.DDQ_ESTATE   # nothing drawn yet
    net.replay_sample_device(SEED)
    net.step(cfg)
    net.synchronize()
    net.replay_import(ring[0], ring[1], ring[2], ring[3], 4, 4)
    for call in (lambda: net.replay_sample_device(SEED), lambda: net.step(cfg),
                 lambda: net.step_graph(cfg, 2), lambda: net.step_pipelined(cfg, 2)):
        assert code_of(call) == _lib.DDQ_EINVAL
    # exchanges
    lib = net.lib
    uid = (np.zeros(128, np.uint8)).tobytes()
    assert code_of(lambda: net.comm_init(uid, 1, 0)) == _lib.DDQ_ESTATE
    other = make_net(ddq, S, 4, ring, 5, 5)
    with pytest.raises(_lib.DDQError) as ei:
        ddq.DeepQNet.group_init([net, other])
    assert ei.value.code == _lib.DDQ_ESTATE
    acfg = net.step_cfg("sgd", lr=1e-6, seed=SEED, exchange="async")
    assert code_of(lambda: net.async_begin(acfg)) == _lib.DDQ_ESTATE
    import ctypes
    arr = (ctypes.c_void_p * 1)(net.ctx.value)
    assert lib.ddq_group_step(arr, 1, ctypes.byref(cfg)) == _lib.DDQ_ESTATE
    assert lib.ddq_group_async_ticks(arr, 1, ctypes.byref(acfg), 0, None) == _lib.DDQ_ESTATE
    assert lib.ddq_group_async_run(arr, 1, ctypes.byref(acfg), 0, None) == _lib.DDQ_ESTATE
    net.replay_set_priority(enabled=False)
    pair = [net, other]
    ddq.DeepQNet.group_init(pair)
    assert code_of(lambda: net.replay_set_priority(**PRIO)) == _lib.DDQ_ESTATE   # a group member
    done(net, other)
    # a communicator attached; then the async exchange begun on it (the exchange
    # needs a communicator, so the second state includes the first: the message
    # tells which of the two refused)
    solo = make_net(ddq, S, 4, ring, 5, 5)
    solo.comm_init(solo.comm_unique_id(), 1, 0)
    with pytest.raises(_lib.DDQError) as ei:
        solo.replay_set_priority(**PRIO)
    assert ei.value.code == _lib.DDQ_ESTATE and "communicator" in str(ei.value)
    solo.async_begin(solo.step_cfg("sgd", lr=1e-6, seed=SEED, exchange="async"))
    solo.synchronize()
    with pytest.raises(_lib.DDQError) as ei:
        solo.replay_set_priority(**PRIO)
    assert ei.value.code == _lib.DDQ_ESTATE and "async" in str(ei.value)
    assert solo.replay_priority() is None
    done(solo)
    big = ddq.DeepQNet(batch=257, frame=S)
    big.replay_create(600)
    assert code_of(lambda: big.replay_set_priority(**PRIO)) == _lib.DDQ_EINVAL
    done(big)
    ok = ddq.DeepQNet(batch=256, frame=S)
    ok.replay_create(600)
    ok.replay_set_priority(**PRIO)
    done(ok)
