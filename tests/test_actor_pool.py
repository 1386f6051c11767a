"""The laned replay ring and the actor pool of the C-ABI (ddq_replay_set_lanes,
ddq_replay_lanes, ddq_actors_create / _step_async / _read) on the CPU twin, no
GPU needed.  Everything is bit equality.

* The pool equals the host loop of tests/_pool_host.py (N unmodified ``ExpGain``
  engines, one batched ``select_action`` per move, one ``ReplayRef`` lane each):
  N = 3, lane length 7 (capacity 21), S = 16, B = 4, 60 moves so every lane
  wraps eight times, three distinct start boards, three epsilon regimes.  The
  seeds were chosen with the host loop alone so that every run meets every
  rule (``check_covered``).
* A pool of one game on a plain ring is the single actor on ``game_seed(s, 0)``.
* The laned host-index gather against a numpy gather with the per-lane wrap.
* The Python restatement of the device draw keeps its own invariants.
* Argument and state errors, each code checked.
"""
import os
import subprocess

import numpy as np
import pytest

import _actor_host as ah
import _pool_host as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, B, N, L, MOVES = 16, 4, 3, 7, 60
SEEDS = {"eps1": 1, "eps01": 1, "ramp": 1}


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    from ddq import _lib
    if not os.path.exists(_lib.CPU_LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "distributed-deep-q_amd"),
                        "ddq/_lib/libddq_cpu.so"], check=True)
    return m


def make_net(ddq, capacity=N * L, lanes=N, batch=B):
    net = ddq.DeepQNet(batch=batch, frame=S, mode="cpu")
    th = ah.seeded_theta(S)
    net.set_flat(0, th)
    net.set_flat(1, th)
    if capacity:
        net.replay_create(capacity)
        if lanes:
            net.replay_set_lanes(lanes)
    return net


def maps():
    from ddq.actor import zoom_maps
    return zoom_maps((S, S), S)


@pytest.fixture(scope="module")
def runs(ddq):
    """regime -> (twin net after the run, host loop after the run), computed once."""
    done = {}

    def get(reg):
        if reg not in done:
            from ddq.actor import DeviceActorPool
            seed = SEEDS[reg]
            iters = [ah.REGIMES[reg](k) for k in range(MOVES)]
            net = make_net(ddq)
            pool = DeviceActorPool(net, ph.three_boards(), seed)
            if reg == "ramp":                       # call by call
                for it in iters:
                    pool.generate_experience(it)
            else:                                   # several moves per call
                net.actors_step(3, iters[0])
                net.actors_step(MOVES - 3, iters[0])
            host = ph.PoolHost(net, ph.three_boards(), seed, S, L)
            host.run(iters)
            done[reg] = (net, host, pool)
        return done[reg]

    return get


# ------------------------------------------------------------- bit identity
@pytest.mark.parametrize("reg", list(ah.REGIMES))
def test_twin_pool_equals_host_loop(runs, reg):
    net, host, pool = runs(reg)
    ph.assert_same(net, host)
    assert host.head_valid() == (MOVES % L, L)
    host.check_covered()
    st = pool.stats()
    assert st["steps"] == N * MOVES and st["draws"] == int(host.stats()[:, 3].sum())
    assert st["per_game"].shape == (N, 4) and st["boards"].shape == (N, 4, 10, 10)


def test_pool_of_one_is_the_single_actor(ddq):
    from ddq.actor import game_seed
    rm, cm = maps()
    init = ah.init_boards()["apple_ahead"]
    s = 17
    one = make_net(ddq, capacity=ah.CAPACITY, lanes=1)
    act = make_net(ddq, capacity=ah.CAPACITY, lanes=0)
    one.actors_create(init[None], rm, cm, s)
    act.actor_create(init, rm, cm, game_seed(s, 0))
    for net, step in ((one, one.actors_step), (act, act.actor_step)):
        step(5, 0)
        step(60, 60000)
        for k in range(30):
            step(1, ah.REGIMES["ramp"](k))
    assert one.replay_lanes() == (1, ah.CAPACITY)
    assert one.replay_info() == act.replay_info() == (95 % ah.CAPACITY, ah.CAPACITY, ah.CAPACITY)
    for a, b in zip(one.replay_export(), act.replay_export()):
        np.testing.assert_array_equal(a, b)
    boards, stats, totals = one.actors_read()
    b1, s1 = act.actor_read()
    np.testing.assert_array_equal(boards[0], b1)
    assert list(stats[0]) == list(s1) == list(totals)
    assert s1[1] >= 1                                # a game ended on the way
    one.close()
    act.close()


# ------------------------------------------------------------ laned gather
@pytest.mark.parametrize("valid,head", [(5, 2), (5, 0), (3, 3)])
def test_laned_host_index_gather(ddq, valid, head):
    n, ll = 3, 5
    net = make_net(ddq, capacity=n * ll, lanes=n)
    ring = ph.random_ring(np.random.default_rng(valid), n * ll, S)
    net.replay_import(*ring, head=head, valid=valid)
    assert net.replay_info() == (head, valid, n * ll)
    last = [g * ll + valid - 1 for g in range(n)]    # every lane's last filled slot
    lists = [last + [0], [0] + last, [1, 2] + last[1:], [ll, ll + 1, 2 * ll, 2 * ll + 1]]
    for idx in lists:
        idx = sorted(idx)
        net.replay_sample(idx)
        np.testing.assert_array_equal(net.read_indices(), idx)
        for got, want in zip(net.read_minibatch(), ph.lane_gather(ring, idx, ll)):
            np.testing.assert_array_equal(got, want.reshape(got.shape))
    if valid == ll:                                  # the wrap stays inside the lane
        assert list(ph.lane_next(last, ll)) == [0, ll, 2 * ll]
    net.close()


# ------------------------------------------------------- the draw restated
@pytest.mark.parametrize("lanes,ll,head,valid", [(1, 37, 0, 37), (1, 37, 9, 20), (3, 8, 0, 8),
                                                 (3, 8, 0, 5), (3, 8, 3, 8), (3, 8, 5, 5),
                                                 (3, 8, 1, 3)])
def test_draw_restatement_invariants(lanes, ll, head, valid):
    seen = set()
    for ctr in range(128):
        idx = ph.draw_sorted(13, ctr, B, head, valid, lanes, ll)
        ph.check_draw(idx, B, head, valid, lanes, ll)
        seen |= set(int(i) for i in idx)
    allowed = {g * ll + k for g in range(lanes) for k in range(valid)
               if not (head >= 1 and k == head - 1)}
    assert seen == allowed                           # every allowed slot is reachable
    # the tightest ring a draw of B accepts: B == lanes * (valid - 1)
    if lanes == 3:
        idx = ph.draw_sorted(5, 0, 6, 2, 3, 3, ll)
        assert list(idx) == [0, 2, ll, ll + 2, 2 * ll, 2 * ll + 2]


@pytest.mark.parametrize("lanes,ll,head,valid", [(1, 192, 5, 150), (3, 64, 5, 64), (3, 64, 0, 40)])
def test_wide_draw_restatement_invariants(lanes, ll, head, valid):
    for ctr in range(8):
        idx = ph.draw_sorted_wide(13, ctr, 96, head, valid, lanes, ll)
        ph.check_draw(idx, 96, head, valid, lanes, ll)


# ------------------------------------------------------------ errors
def test_lane_and_pool_errors(ddq):
    from ddq import _lib
    lib = _lib.load(mode="cpu")
    p = _lib.ptr
    rm, cm = maps()
    three = np.ascontiguousarray(ph.three_boards(), np.int8)

    def code(fn, *a, **k):
        with pytest.raises(_lib.DDQError) as ei:
            fn(*a, **k)
        return ei.value.code

    def create(ctx, n=N, b=three, r=rm, c=cm):
        return lib.ddq_actors_create(ctx, n, p(b) if b is not None else None,
                                     p(r) if r is not None else None,
                                     p(c) if c is not None else None, 5)

    net = make_net(ddq, capacity=0)
    # null ctx; no ring
    assert lib.ddq_replay_set_lanes(None, 3) == _lib.DDQ_EINVAL
    assert lib.ddq_replay_lanes(None, None, None) == _lib.DDQ_EINVAL
    assert create(None) == _lib.DDQ_EINVAL
    assert lib.ddq_actors_step_async(None, 1, 0) == _lib.DDQ_EINVAL
    assert lib.ddq_actors_read(None, None, None, None) == _lib.DDQ_EINVAL
    assert code(net.replay_set_lanes, 3) == _lib.DDQ_ESTATE
    assert code(net.replay_lanes) == _lib.DDQ_ESTATE
    assert create(net.ctx) == _lib.DDQ_ESTATE
    # step / read before create
    assert code(net.actors_step, 1, 0) == _lib.DDQ_ESTATE
    assert code(net.actors_read) == _lib.DDQ_ESTATE
    net.replay_create(N * L)
    assert net.replay_lanes() == (1, N * L)
    # capacity % lanes != 0, lanes < 1, lane length < 2
    for bad in (2, 4, 0, -1, N * L, 11):
        assert code(net.replay_set_lanes, bad) == _lib.DDQ_EINVAL
    assert net.replay_lanes() == (1, N * L)
    net.replay_set_lanes(1)                          # allowed, changes nothing
    assert net.replay_lanes() == (1, N * L)
    # ngames != lanes
    assert create(net.ctx) == _lib.DDQ_EINVAL
    assert b"lanes" in lib.ddq_last_error(net.ctx)
    net.replay_set_lanes(N)
    assert net.replay_lanes() == (N, L) and net.replay_info() == (0, 0, N * L)
    assert create(net.ctx, n=2) == _lib.DDQ_EINVAL
    # ngames outside [1, B]
    for n in (0, -1, B + 1):
        assert create(net.ctx, n=n) == _lib.DDQ_EINVAL
        assert b"ngames" in lib.ddq_last_error(net.ctx)
    # null boards / maps; map entries outside [0,10)
    assert create(net.ctx, b=None) == _lib.DDQ_EINVAL
    assert create(net.ctx, r=None) == _lib.DDQ_EINVAL
    assert create(net.ctx, c=None) == _lib.DDQ_EINVAL
    for bad in (-1, 10):
        r2, c2 = rm.copy(), cm.copy()
        r2[3], c2[S - 1] = bad, bad
        assert create(net.ctx, r=r2) == _lib.DDQ_EINVAL
        assert create(net.ctx, c=c2) == _lib.DDQ_EINVAL
    # a bad board in any place: no snake, head and neck apart
    for g in range(N):
        b = three.copy()
        b[g] = -1
        assert create(net.ctx, b=b) == _lib.DDQ_EINVAL
        b[g] = ah.board([(6, 5), (4, 5)], (0, 0))
        assert create(net.ctx, b=b) == _lib.DDQ_EINVAL
    # nothing above made a pool
    assert code(net.actors_step, 1, 0) == _lib.DDQ_ESTATE
    # the refusals on a laned ring
    frame = np.zeros((4, S, S), np.uint8)
    assert code(net.replay_add, 1, 0, frame) == _lib.DDQ_ESTATE
    assert b"laned" in lib.ddq_last_error(net.ctx)
    ring = ph.random_ring(np.random.default_rng(0), N * L, S)
    assert code(net.replay_fill_tiled, *ring, head=0, valid=L) == _lib.DDQ_ESTATE
    assert b"laned" in lib.ddq_last_error(net.ctx)
    out = np.zeros(8, np.float32)
    i32 = np.zeros(8, np.int32)
    assert lib.ddq_replay_sample_batch_async(net.ctx, 2, 0, p(i32), p(out), p(out), p(out), p(out),
                                             p(out)) == _lib.DDQ_ESTATE
    assert b"laned" in lib.ddq_last_error(net.ctx)
    assert lib.ddq_replay_gather_batch_async(net.ctx, p(i32), 2, p(out), p(out), p(out), p(out),
                                             p(out)) == _lib.DDQ_ESTATE
    assert b"laned" in lib.ddq_last_error(net.ctx)
    assert code(net.actor_create, three[0], rm, cm, 1) == _lib.DDQ_ESTATE
    assert b"laned" in lib.ddq_last_error(net.ctx)
    # import takes per-lane head / valid
    assert code(net.replay_import, *ring, head=L, valid=L) == _lib.DDQ_EINVAL
    assert code(net.replay_import, *ring, head=0, valid=L + 1) == _lib.DDQ_EINVAL
    # create, step arguments, read with any output null
    assert create(net.ctx) == _lib.DDQ_OK
    for n in (0, -3):
        assert lib.ddq_actors_step_async(net.ctx, n, 0) == _lib.DDQ_EINVAL
        assert b"nmoves" in lib.ddq_last_error(net.ctx)
    boards = np.empty((N, 4, 10, 10), np.int8)
    stats = np.empty((N, 4), np.int64)
    totals = np.empty(4, np.int64)
    assert lib.ddq_actors_read(net.ctx, p(boards), None, None) == _lib.DDQ_OK
    assert lib.ddq_actors_read(net.ctx, None, p(stats), None) == _lib.DDQ_OK
    assert lib.ddq_actors_read(net.ctx, None, None, p(totals)) == _lib.DDQ_OK
    assert (boards == three[:, None]).all() and not stats.any() and not totals.any()
    # the B-versus-valid check at its boundary: B = 4 needs 3 (v - 1) >= 4, v >= 3
    net.actors_step(2, 0)
    assert net.replay_info()[:2] == (2, 2)
    assert code(net.replay_sample, [0, 1, L, L + 1]) == _lib.DDQ_EINVAL
    assert b"Can't draw sample" in lib.ddq_last_error(net.ctx)
    net.actors_step(1, 0)
    net.replay_sample([0, 1, L, L + 1])
    assert code(net.replay_sample, [0, 1, 3, L]) == _lib.DDQ_EINVAL      # 3 >= valid in lane 0
    assert code(net.replay_sample, [0, 1, L + 3, 2 * L]) == _lib.DDQ_EINVAL
    # set_lanes on a non-empty ring
    assert code(net.replay_set_lanes, 1) == _lib.DDQ_ESTATE
    assert code(net.replay_set_lanes, N) == _lib.DDQ_ESTATE
    # create again resets the games, not the ring
    assert net.actors_read()[2][0] == 3 * N
    assert create(net.ctx) == _lib.DDQ_OK
    assert not net.actors_read()[2].any()
    assert net.replay_info()[:2] == (3, 3)
    net.actors_step(1, 0)
    assert net.replay_info()[:2] == (4, 4)
    net.close()
