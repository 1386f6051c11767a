"""The device-resident policy evaluator (csrc/eval.h, ddq_eval_*) on the GPU.

* Bit identity with the host loop of tests/_eval_host.py on two contexts
  holding identical parameters: the device evaluator on one, the host loop's
  batched ``select_action`` on the other.  Both run the same forward kernels
  at the same n, so the Q values, hence every decision, are expected to be
  equal; no tolerance.  S = 16 (small-map ctx) and S = 24 (general kernels),
  B = 8, N = 6 games on six different start boards; epsilon 0.25 and 0
  (S = 40 and S = 64: epsilon 0),
  ``max_episodes`` = 2 (idle games), chunked runs; N = B and N = 1 once each.
* Non-interference on a ctx that also holds a ring and a device actor.
* ``DevicePolicyEvaluator.evaluate`` against the host ``streams="per_game"``
  evaluator, twice with two models.
"""
import numpy as np
import pytest

import _actor_host as ah
import _eval_host as eh

pytestmark = pytest.mark.gpu

B, N = 8, 6
CASES = [(S, eps) for S in (16, 24) for eps in (eh.EPS, 0.0)]
# past S = 24, greedy: a frame with partial edge tiles and the bench's own (their
# Q values are held to the oracle by tests/test_gpu_acting.py)
CASES += [(40, 0.0), (64, 0.0)]


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


def make_net(ddq, S, theta=None):
    net = ddq.DeepQNet(batch=B, frame=S)
    th = eh.theta(S) if theta is None else theta
    net.set_flat(0, th)
    net.set_flat(1, th)
    return net


def create(net, S, epsilon, max_moves, max_episodes, boards=None, seed=eh.SEED):
    from ddq.actor import zoom_maps
    rm, cm = zoom_maps((S, S), S)
    net.eval_create(eh.six_boards() if boards is None else boards, rm, cm, seed, epsilon,
                    max_moves, max_episodes)


@pytest.fixture(scope="module")
def hosts(ddq):
    """(S, epsilon) -> (host loop after TRIALS episodes, its moves), each
    computed once on a ctx of its own; the loops are not changed afterwards."""
    nets, done = {}, {}

    def get(S, eps):
        if (S, eps) not in done:
            if S not in nets:
                nets[S] = make_net(ddq, S)
            host = eh.EvalHost(nets[S], eh.six_boards(), eh.SEED, S, eps, eh.MAX_MOVES, eh.TRIALS)
            moves = host.run_until(eh.TRIALS, limit=400)
            host.check_covered()
            done[(S, eps)] = (host, moves)
        return done[(S, eps)]

    yield get
    for net in nets.values():
        net.synchronize()
        net.close()


@pytest.mark.parametrize("S,eps", CASES, ids=["S%d-eps%g" % c for c in CASES])
def test_device_evaluator_equals_host_loop(ddq, hosts, S, eps):
    from ddq.evaluation import select_trials
    host, moves = hosts(S, eps)
    dev = make_net(ddq, S)
    assert dev.small_path()[0] == (S == 16)
    create(dev, S, eps, eh.MAX_MOVES, eh.TRIALS)
    dev.eval_run(moves)
    out = eh.assert_same(dev, host)
    logs = [out["log"][i, :k] for i, k in enumerate(out["episodes"])]
    assert select_trials(logs, eh.TRIALS) == eh.select_trials(host.logs, eh.TRIALS)
    dev.synchronize()
    dev.close()


@pytest.mark.parametrize("S", [16, 24])
def test_chunked_run_equals_host_loop(ddq, hosts, S):
    host, moves = hosts(S, eh.EPS)
    assert moves > 8
    dev = make_net(ddq, S)
    create(dev, S, eh.EPS, eh.MAX_MOVES, eh.TRIALS)
    for n in (3, 5, moves - 8):
        dev.eval_run(n)
    eh.assert_same(dev, host)
    dev.synchronize()
    dev.close()


@pytest.mark.parametrize("S,eps", [(16, eh.EPS), (24, 0.0)])
def test_full_log_makes_a_game_idle(ddq, S, eps):
    dev, hostnet = make_net(ddq, S), make_net(ddq, S)
    host = eh.EvalHost(hostnet, eh.six_boards(), eh.SEED, S, eps, eh.MAX_MOVES, 2)
    host.run(12)
    create(dev, S, eps, eh.MAX_MOVES, 2)
    dev.eval_run(12)
    out = eh.assert_same(dev, host)
    assert len(host.logs[2]) == 2 and host.logs[2][-1][0] < 10     # idle for two moves at least
    assert out["episodes"].min() < 2                                # while another plays on
    host.run(40)
    dev.eval_run(40)
    out = eh.assert_same(dev, host)
    assert list(out["episodes"]) == [2] * N
    for net in (dev, hostnet):
        net.synchronize()
        net.close()


@pytest.mark.parametrize("n", [B, 1])
def test_full_batch_and_single_game(ddq, n):
    S = 16
    six = eh.six_boards()
    boards = np.concatenate([six, six[[1, 0]]])[:n] if n > 1 else six[2:3]
    dev, hostnet = make_net(ddq, S), make_net(ddq, S)
    host = eh.EvalHost(hostnet, boards, 23, S, eh.EPS, eh.MAX_MOVES, 10)
    host.run(25)
    assert host.done() >= 3
    create(dev, S, eh.EPS, eh.MAX_MOVES, 10, boards=boards, seed=23)
    dev.eval_run(25)
    out = eh.assert_same(dev, host)
    assert out["log"].shape == (n, 10, 4)
    for net in (dev, hostnet):
        net.synchronize()
        net.close()


def test_evaluator_leaves_ring_actor_and_training_alone(ddq):
    """Actor steps, evaluator moves, actor steps, one graph training step on
    one ctx, against the same sequence without the evaluator moves; and the
    evaluator's logs against an evaluator that ran alone.  A ``select_action``
    between two evaluator chunks changes nothing in its results."""
    from ddq.actor import DeviceActor
    S = 16
    init = ah.init_boards()["start"]
    both, plain, alone = make_net(ddq, S), make_net(ddq, S), make_net(ddq, S)
    states = np.random.default_rng(0).integers(0, 256, (B, 4, S, S)).astype(np.uint8)
    picked = {}
    for net in (both, plain):
        net.replay_create(ah.CAPACITY)
        DeviceActor(net, init, 31)
        net.actor_step(25, 60000)
        if net is both:
            create(net, S, eh.EPS, eh.MAX_MOVES, eh.TRIALS)
            net.eval_run(7)
        picked[net] = net.select_action(states)
        if net is both:
            net.eval_run(9)
        net.actor_step(25, 60000)
        net.step_graph(net.step_cfg("rmsprop", lr=1e-4, target_period=10, seed=5), 1)
        net.synchronize()
    create(alone, S, eh.EPS, eh.MAX_MOVES, eh.TRIALS)
    alone.eval_run(16)
    np.testing.assert_array_equal(picked[both], picked[plain])
    # the ring, the actor and the step
    assert both.replay_info() == plain.replay_info()
    for a, b in zip(both.replay_export(), plain.replay_export()):
        np.testing.assert_array_equal(a, b)
    (ba, sa), (bb, sb) = both.actor_read(), plain.actor_read()
    np.testing.assert_array_equal(ba, bb)
    assert list(sa) == list(sb) and sa[0] == 50
    np.testing.assert_array_equal(both.read_indices(), plain.read_indices())
    np.testing.assert_array_equal(both.get_flat(0), plain.get_flat(0))
    assert both.lib.ddq_step_count(both.ctx) == plain.lib.ddq_step_count(plain.ctx) == 1
    # the evaluator: untouched by the actor, select_action and the training step
    got, want = both.eval_read(), alone.eval_read()
    for k in ("stats", "episodes", "log", "boards", "draws"):
        np.testing.assert_array_equal(got[k], want[k])
    assert got["stats"][0] == 16 and got["stats"][1] >= 2
    # and it plays on after them: the parameters changed on both alike
    alone.set_flat(0, both.get_flat(0))
    both.eval_run(5)
    alone.eval_run(5)
    got, want = both.eval_read(), alone.eval_read()
    for k in ("stats", "episodes", "log", "boards", "draws"):
        np.testing.assert_array_equal(got[k], want[k])
    for net in (both, plain, alone):
        net.synchronize()
        net.close()


def test_device_policy_evaluator_equals_per_game_host(ddq):
    from ddq import evaluation as ev
    from ddq.barista.baristanet import BaristaNet
    S = 16
    net = BaristaNet({"batch": B, "frame": S}, None, None)
    assert net.dqn.small_path()[0]
    boards = eh.six_boards()
    kw = dict(net=net, seed=eh.SEED, max_moves=eh.MAX_MOVES, epsilon=eh.EPS)
    dev = ev.DevicePolicyEvaluator(None, None, init_state=boards, games=N, chunk=8,
                                   move_limit=400, **kw)
    host = ev.PolicyEvaluator(None, None, streams="per_game", init_states=boards, **kw)
    seen = []
    for seed in (eh.THETA_SEED[S], 7):
        model = net.dqn.split(ah.seeded_theta(S, seed=seed), "Q")
        a = dev.evaluate(model, eh.TRIALS)
        b = host.evaluate(model, eh.TRIALS)
        assert isinstance(a, float) and a == b
        assert dev.episodes == host.episodes and len(dev.episodes) == eh.TRIALS
        assert dev.stats[0] % 8 == 0
        seen.append(dev.episodes)
    assert seen[0] != seen[1]
    net.dqn.synchronize()
    net.dqn.close()


def test_argument_errors(ddq):
    from ddq import _lib
    from ddq.actor import zoom_maps
    S = 16
    net = make_net(ddq, S)
    rm, cm = zoom_maps((S, S), S)
    good = eh.six_boards()

    def code(fn, *a):
        with pytest.raises(_lib.DDQError) as ei:
            fn(*a)
        return ei.value.code

    assert code(net.eval_run, 1) == _lib.DDQ_ESTATE
    assert code(net.eval_read) == _lib.DDQ_ESTATE
    bad = rm.copy()
    bad[5] = 10
    assert code(net.eval_create, good, bad, cm, 1) == _lib.DDQ_EINVAL
    assert code(net.eval_create, good, rm, -bad, 1) == _lib.DDQ_EINVAL
    far = good.copy()
    far[4] = ah.board([(6, 5), (4, 5)], (0, 0))
    assert code(net.eval_create, far, rm, cm, 1) == _lib.DDQ_EINVAL
    assert b"init_boards[4]" in net.lib.ddq_last_error(net.ctx)
    nine = np.concatenate([good, good[:3]])
    assert code(net.eval_create, nine, rm, cm, 1) == _lib.DDQ_EINVAL          # > B games
    assert code(net.eval_create, good, rm, cm, 1, 1.5) == _lib.DDQ_EINVAL
    assert code(net.eval_create, good, rm, cm, 1, 0.5, -1) == _lib.DDQ_EINVAL
    assert code(net.eval_create, good, rm, cm, 1, 0.5, 0, 0) == _lib.DDQ_EINVAL
    p = _lib.ptr
    b8 = np.ascontiguousarray(good, np.int8)
    lib = net.lib
    assert lib.ddq_eval_create(net.ctx, N, None, p(rm), p(cm), 1, 0.0, 0, 1) == _lib.DDQ_EINVAL
    assert lib.ddq_eval_create(net.ctx, N, p(b8), None, p(cm), 1, 0.0, 0, 1) == _lib.DDQ_EINVAL
    assert lib.ddq_eval_create(None, N, p(b8), p(rm), p(cm), 1, 0.0, 0, 1) == _lib.DDQ_EINVAL
    assert code(net.eval_run, 1) == _lib.DDQ_ESTATE                            # still none
    net.eval_create(good, rm, cm, 1, 0.0, 0, 3)
    assert code(net.eval_run, 0) == _lib.DDQ_EINVAL
    assert lib.ddq_eval_read(net.ctx, None, None, None, None, None) == _lib.DDQ_OK
    out = net.eval_read()
    assert list(out["stats"]) == [0, 0, 0, 0] and not out["log"].any()
    assert (out["boards"] == good[:, None]).all()
    # a longer log after a shorter one
    net.eval_create(good, rm, cm, 1, 0.0, 4, 9)
    net.eval_run(8)
    out = net.eval_read()
    assert out["log"].shape == (N, 9, 4) and out["episodes"].min() >= 2
    assert net.replay_info()[2] == 0
    net.synchronize()
    net.close()
