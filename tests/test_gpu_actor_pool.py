"""The laned replay ring and the device actor pool (csrc/pool.h, ddq_actors_*,
ddq_replay_set_lanes) on the GPU.  Everything is bit equality.

* The device pool equals the host loop of tests/_pool_host.py on two contexts
  holding identical parameters (the pool on one, the host loop's batched
  ``select_action`` on the other; both run the same forward kernels at
  n = ngames): S = 16 (small-map ctx) and S = 24 (general kernels), B = 4,
  N = 3 and N = B = 4, lane length 7, 40 moves as one call of 3 and one of 37;
  S = 64 once at N = 3.
  A pool of one game on a plain ring is the single actor.
* The draw, exactly: tests/_pool_host.py restates ``draw_sorted`` for B <= 64.
  It is checked first against the index log of a plain ring (code this feature
  must not alter), then against laned rings set up by import, through
  ``replay_sample_device`` and through pipelined steps, at S = 16 and S = 24 so
  the K1 / K4 and head_draw / prefetch_body call sites are all exercised.
* The gather: after every ``replay_sample_device``, ``read_minibatch`` is the
  numpy lane gather of the imported ring at the indices read back.
* The pool feeds the pipelined chain: ``act_and_train`` against the same moves
  each followed by plain graph steps.
* The pool interleaved with ``select_action``, the evaluator and a monitor
  record on one ctx: its results do not change.
"""
import numpy as np
import pytest

import _actor_host as ah
import _eval_host as eh
import _pool_host as ph

pytestmark = pytest.mark.gpu

B, L, MOVES = 4, 7, 40
# (S, N, regime, seed): seeds chosen with the host loop alone (check_covered)
POOL_CASES = [(16, 3, "eps1", 2), (16, 4, "eps01", 1), (24, 3, "ramp", 2), (24, 4, "eps1", 2),
              (64, 3, "eps01", 2)]
# (N, L, h, v)
LANED = [(3, 8, 0, 8), (3, 8, 0, 5), (3, 8, 3, 8), (3, 8, 5, 5)]
DRAWS = 32


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


def boards(n):
    return ph.three_boards() if n == 3 else ph.four_boards()


def make_net(ddq, S, capacity=0, lanes=0, theta=None):
    net = ddq.DeepQNet(batch=B, frame=S)
    th = eh.theta(S) if theta is None else theta
    net.set_flat(0, th)
    net.set_flat(1, th)
    if capacity:
        net.replay_create(capacity)
        if lanes:
            net.replay_set_lanes(lanes)
    return net


def close(*nets):
    for net in nets:
        net.synchronize()
        net.close()


# ------------------------------------------------------------- bit identity
@pytest.mark.parametrize("S,n,reg,seed", POOL_CASES, ids=["%d-%d-%s-%d" % c for c in POOL_CASES])
def test_device_pool_equals_host_loop(ddq, S, n, reg, seed):
    from ddq.actor import DeviceActorPool
    iters = [ah.REGIMES[reg](k) for k in range(MOVES)]
    dev, hostnet = make_net(ddq, S, n * L, n), make_net(ddq, S)
    assert dev.small_path()[0] == (S == 16)
    pool = DeviceActorPool(dev, boards(n), seed)
    if reg == "ramp":
        for it in iters:
            pool.generate_experience(it)
    else:
        dev.actors_step(3, iters[0])
        dev.actors_step(MOVES - 3, iters[0])
    assert dev.replay_info() == (MOVES % L, L, n * L)     # the host mirror, no sync
    host = ph.PoolHost(hostnet, boards(n), seed, S, L)
    host.run(iters)
    ph.assert_same(dev, host)
    host.check_covered()
    dev._check(dev.lib.ddq_replay_status(dev.ctx))
    close(dev, hostnet)


@pytest.mark.parametrize("S", [16, 24])
def test_pool_of_one_is_the_single_actor(ddq, S):
    from ddq.actor import game_seed, zoom_maps
    rm, cm = zoom_maps((S, S), S)
    init = ah.init_boards()["apple_ahead"]
    s = 17
    one, act = make_net(ddq, S, ah.CAPACITY, 1), make_net(ddq, S, ah.CAPACITY)
    one.actors_create(init[None], rm, cm, s)
    act.actor_create(init, rm, cm, game_seed(s, 0))
    for step in (one.actors_step, act.actor_step):
        step(3, 0)
        step(37, 60000)
        step(20, 0)
    assert one.replay_info() == act.replay_info() == (60 % ah.CAPACITY, ah.CAPACITY, ah.CAPACITY)
    for a, b in zip(one.replay_export(), act.replay_export()):
        np.testing.assert_array_equal(a, b)
    brd, stats, totals = one.actors_read()
    b1, s1 = act.actor_read()
    np.testing.assert_array_equal(brd[0], b1)
    assert list(stats[0]) == list(s1) == list(totals) and s1[0] == 60 and s1[1] >= 1
    close(one, act)


# ------------------------------------------------------------------ the draw
def logged_draws(net, seed, n):
    """n x replay_sample_device(seed): the index log's sets and, per draw, the
    indices read back and the minibatch."""
    first = net.replay_draws()
    idx, mbs = [], []
    for _ in range(n):
        net.replay_sample_device(seed)
        idx.append(net.read_indices())
        mbs.append(net.read_minibatch())
    assert net.replay_draws() == first + n
    log = net.index_log(first, n)
    np.testing.assert_array_equal(log, np.stack(idx))
    return first, log, mbs


@pytest.mark.parametrize("S", [16, 24])
def test_restated_draw_equals_the_plain_ring_index_log(ddq, S):
    """Validates tests/_pool_host.draw_sorted against the unlaned device draw."""
    from ddq.params import init_params_flat
    cap = 24
    net = make_net(ddq, S, cap, theta=init_params_flat(S, seed=42))
    ring = ph.random_ring(np.random.default_rng(S), cap, S)
    cfg = net.step_cfg("sgd", lr=1e-6, target_period=10, seed=9)
    for head, valid in ((0, cap), (7, 19), (1, 6)):      # valid 6: redraws in most draws
        net.replay_import(*ring, head=head, valid=valid)
        net.index_log_enable(DRAWS + 8)
        first, log, _ = logged_draws(net, 13, DRAWS)
        for d in range(DRAWS):
            np.testing.assert_array_equal(log[d], ph.draw_sorted(13, first + d, B, head, valid))
        net.step_pipelined(cfg, 8)
        assert net.replay_draws() == first + DRAWS + 8
        log = net.index_log(first + DRAWS, 8)
        for d in range(8):
            np.testing.assert_array_equal(
                log[d], ph.draw_sorted(9, first + DRAWS + d, B, head, valid))
    close(net)


@pytest.mark.parametrize("S", [16, 24])
@pytest.mark.parametrize("n,ll,head,valid", LANED, ids=["%d-%d-%d-%d" % c for c in LANED])
def test_laned_draw_and_gather(ddq, S, n, ll, head, valid):
    from ddq.params import init_params_flat
    net = make_net(ddq, S, n * ll, n, theta=init_params_flat(S, seed=42))
    assert net.small_path()[0] == (S == 16)
    ring = ph.random_ring(np.random.default_rng(S + head), n * ll, S)
    net.replay_import(*ring, head=head, valid=valid)
    assert net.replay_info() == (head, valid, n * ll)
    net.index_log_enable(DRAWS + 8)
    first, log, mbs = logged_draws(net, 13, DRAWS)
    seen = set()
    for d in range(DRAWS):
        want = ph.draw_sorted(13, first + d, B, head, valid, n, ll)
        ph.check_draw(want, B, head, valid, n, ll)
        np.testing.assert_array_equal(log[d], want)
        seen |= {int(i) // ll for i in want}
        for got, ref in zip(mbs[d], ph.lane_gather(ring, log[d], ll)):
            np.testing.assert_array_equal(got, ref.reshape(got.shape))
    assert seen == set(range(n))                          # every lane was drawn from
    if valid == ll:                                       # and a lane's last slot: the wrap
        assert any((int(i) + 1) % ll == 0 for d in range(DRAWS) for i in log[d])
    # the step's own call sites: 8 pipelined steps with the log on
    cfg = net.step_cfg("sgd", lr=1e-6, target_period=10, seed=9)
    net.step_pipelined(cfg, 8)
    assert net.replay_draws() == first + DRAWS + 8
    log = net.index_log(first + DRAWS, 8)
    for d in range(8):
        np.testing.assert_array_equal(
            log[d], ph.draw_sorted(9, first + DRAWS + d, B, head, valid, n, ll))
    # the last step's minibatch is still bound: its gather, too
    np.testing.assert_array_equal(net.read_indices(), log[7])
    for got, ref in zip(net.read_minibatch(), ph.lane_gather(ring, log[7], ll)):
        np.testing.assert_array_equal(got, ref.reshape(got.shape))
    net._check(net.lib.ddq_replay_status(net.ctx))
    close(net)


@pytest.mark.parametrize("S", [16, 24])
def test_multi_wave_draw_plain_and_laned(ddq, S):
    """B = 96 > 64 takes ``draw_sorted``'s sort-network path: its restatement
    against the plain ring first, then a laned ring (3 lanes of 64, 189 allowed
    slots for 96 draws, so redraw rounds happen), gather included."""
    from ddq.params import init_params_flat
    wide, n, ll, head = 96, 3, 64, 5
    ring = ph.random_ring(np.random.default_rng(S), n * ll, S)
    for lanes, valid in ((1, 150), (n, ll)):
        net = ddq.DeepQNet(batch=wide, frame=S)
        th = init_params_flat(S, seed=42)
        net.set_flat(0, th)
        net.set_flat(1, th)
        net.replay_create(n * ll)
        if lanes > 1:
            net.replay_set_lanes(lanes)
        lane_len = n * ll // lanes
        net.replay_import(*ring, head=head, valid=valid)
        net.index_log_enable(12)
        first = net.replay_draws()
        for d in range(8):
            net.replay_sample_device(13)
            idx = net.read_indices()
            want = ph.draw_sorted_wide(13, first + d, wide, head, valid, lanes, lane_len)
            ph.check_draw(want, wide, head, valid, lanes, lane_len)
            np.testing.assert_array_equal(idx, want)
            for got, ref in zip(net.read_minibatch(), ph.lane_gather(ring, idx, lane_len)):
                np.testing.assert_array_equal(got, ref.reshape(got.shape))
        net.step_pipelined(net.step_cfg("sgd", lr=1e-6, target_period=10, seed=9), 4)
        log = net.index_log(first + 8, 4)
        for d in range(4):
            np.testing.assert_array_equal(
                log[d], ph.draw_sorted_wide(9, first + 8 + d, wide, head, valid, lanes, lane_len))
        net._check(net.lib.ddq_replay_status(net.ctx))
        close(net)


# ------------------------------------------------- pool + pipelined chain
@pytest.mark.parametrize("S", [16, 24])
def test_pool_feeds_the_pipelined_chain(ddq, S):
    from ddq.actor import DeviceActorPool
    from ddq.params import init_params_flat
    # sgd and the prototxt fillers: see test_gpu_actor.test_act_and_step on why
    # rmsprop with the bit-identity tests' scaled-up weights diverges
    n, rounds = 4, 3
    nets = [make_net(ddq, S, n * L, n, theta=init_params_flat(S, seed=42)) for _ in range(2)]
    pools = [DeviceActorPool(net, boards(n), 21) for net in nets]
    for net, pool in zip(nets, pools):
        pool.fill(3)
        net.index_log_enable(n * rounds)
    a, b = nets
    cfg = a.step_cfg("sgd", lr=1e-4, target_period=5, seed=5)
    first = a.replay_draws()
    assert first == b.replay_draws()
    pools[0].act_and_train(cfg, rounds, 0)
    for r in range(rounds):
        pools[1].generate_experience(r * n)
        for _ in range(n):
            b.step_graph(cfg, 1)
    close_later = []
    for net in nets:
        net.synchronize()
        assert net.lib.ddq_step_count(net.ctx) == n * rounds
        assert net.replay_info() == (3 + rounds, 3 + rounds, n * L)
        net._check(net.lib.ddq_replay_status(net.ctx))
        close_later.append(net)
    np.testing.assert_array_equal(a.index_log(first, n * rounds), b.index_log(first, n * rounds))
    log = a.index_log(first, n * rounds)
    for r in range(rounds):                               # drawn against the ring after move r
        for d in range(n):
            np.testing.assert_array_equal(
                log[r * n + d], ph.draw_sorted(5, first + r * n + d, B, 4 + r, 4 + r, n, L))
    th0 = init_params_flat(S, seed=42)
    for which in (0, 1):
        ta, tb = a.get_flat(which), b.get_flat(which)
        assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
        assert np.isfinite(ta).all() and (ta != th0).any()
    for x, y in zip(a.replay_export(), b.replay_export()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.actors_read()[1], b.actors_read()[1])
    close(*close_later)


# ------------------------------------------------------------ shared scratch
def test_pool_shares_the_ctx_with_acting_evaluation_and_monitor(ddq):
    """select_action, evaluator moves and a monitor record between the pool's
    moves (the act_* scratch is shared; calls on a ctx are serialised) against
    the pool alone."""
    from ddq.actor import DeviceActorPool
    S, n = 16, 3
    both, alone = make_net(ddq, S, n * L, n), make_net(ddq, S, n * L, n)
    states = np.random.default_rng(0).integers(0, 256, (B, 4, S, S)).astype(np.uint8)
    pb, pa = DeviceActorPool(both, boards(n), 9), DeviceActorPool(alone, boards(n), 9)
    rm, cm = pb.row_map, pb.col_map
    both.monitor_enable(4)
    pb.fill(5)
    picked = both.select_action(states)
    both.actors_step(4, 60000)
    both.eval_create(eh.six_boards()[:B], rm, cm, eh.SEED, eh.EPS, eh.MAX_MOVES, eh.TRIALS)
    both.eval_run(6)
    both.actors_step(3, 60000)
    both.monitor_record(7)
    both.eval_run(2)
    both.actors_step(8, 0)
    pa.fill(5)
    alone.actors_step(7, 60000)
    alone.actors_step(8, 0)
    assert both.replay_info() == alone.replay_info() == (20 % L, L, n * L)
    for x, y in zip(both.replay_export(), alone.replay_export()):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(both.actors_read(), alone.actors_read()):
        np.testing.assert_array_equal(x, y)
    assert pb.stats()["steps"] == 20 * n
    # and the others kept their own results
    np.testing.assert_array_equal(picked, alone.select_action(states))
    assert both.eval_read()["stats"][0] == 8
    recs, total = both.monitor_read()
    assert total == 1 and recs["tag"][0] == 7
    close(both, alone)
