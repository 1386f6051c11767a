"""Device-resident policy evaluation of the C-ABI (ddq_eval_create /
ddq_eval_run_async / ddq_eval_read) on the CPU twin, no GPU needed.

* The twin equals the host loop of tests/_eval_host.py with no tolerance: the
  per-game logs, draws and boards, ``stats``, the selected trials and their
  average.  N = 6 games on six different start boards in a B = 8 ctx, S = 16
  and 24, epsilon 0.25 and 0, ``max_moves`` 8 and 0, ``max_episodes`` = 2 (games
  go idle while others play on), one call against chunks of 3, 5 and the rest.
  The host loop asserts on itself that the games were told apart and that
  every rule was met (``check_covered``).
* ``DevicePolicyEvaluator.evaluate`` equals ``PolicyEvaluator(streams=
  "per_game").evaluate``; ``PolicyEvaluator`` with default keywords returns
  what the loop it had before returns.
* The argument and state errors of include/ddq_hip.h.
"""
import os
import random
import subprocess

import numpy as np
import pytest

import _actor_host as ah
import _eval_host as eh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N = 8, 6
# (S, epsilon, max_moves)
CASES = [(S, eps, mm) for S in (16, 24) for eps, mm in ((eh.EPS, eh.MAX_MOVES),
                                                        (0.0, eh.MAX_MOVES), (eh.EPS, 0),
                                                        (0.0, 0))]


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    from ddq import _lib
    if not os.path.exists(_lib.CPU_LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "distributed-deep-q_amd"),
                        "ddq/_lib/libddq_cpu.so"], check=True)
    return m


def make_net(ddq, S):
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    th = eh.theta(S)
    net.set_flat(0, th)
    net.set_flat(1, th)
    return net


def create(net, S, epsilon, max_moves, max_episodes, boards=None, seed=eh.SEED):
    from ddq.actor import zoom_maps
    rm, cm = zoom_maps((S, S), S)
    net.eval_create(eh.six_boards() if boards is None else boards, rm, cm, seed, epsilon,
                    max_moves, max_episodes)


@pytest.fixture(scope="module")
def runs(ddq):
    """case -> (twin net after the run, host loop after the run, moves), each
    computed once: the host plays until TRIALS episodes are logged (within
    2000 moves, asserted), the twin the same number of moves in one call."""
    done = {}

    def get(case):
        if case not in done:
            S, eps, mm = case
            net = make_net(ddq, S)
            host = eh.EvalHost(net, eh.six_boards(), eh.SEED, S, eps, mm, eh.TRIALS)
            moves = host.run_until(eh.TRIALS, limit=2000)
            create(net, S, eps, mm, eh.TRIALS)
            net.eval_run(moves)
            done[case] = (net, host, moves)
        return done[case]

    return get


def test_game_seed_is_the_documented_mix():
    from ddq.actor import ActorRng, game_seed, splitmix64
    assert game_seed(0, 0) == splitmix64(0xE220A8397B1DCDAF)
    for seed in (0, 11, (1 << 64) - 1):
        seeds = [game_seed(seed, i) for i in range(32)]
        assert len(set(seeds)) == 32
        assert seeds[5] == splitmix64(splitmix64(seed) ^ 5)
    # game i's draw k is the actor's draw k on that seed
    r = ActorRng(game_seed(11, 3))
    assert r._next() == splitmix64(game_seed(11, 3) ^ splitmix64(0))


@pytest.mark.parametrize("case", CASES, ids=["S%d-eps%g-max%d" % c for c in CASES])
def test_twin_evaluator_equals_host_loop(runs, case):
    from ddq.evaluation import select_trials
    net, host, moves = runs(case)
    host.check_covered()
    out = eh.assert_same(net, host)
    assert out["stats"][0] == moves and out["stats"][1] >= eh.TRIALS
    logs = [out["log"][i, :k] for i, k in enumerate(out["episodes"])]
    got = select_trials(logs, eh.TRIALS)
    want = eh.select_trials(host.logs, eh.TRIALS)
    assert got == want
    assert sum(r[2] for r in got) / eh.TRIALS == sum(r[2] for r in want) / eh.TRIALS
    # the trials are the first TRIALS episodes in lock-step order
    assert [r[:2] for r in got] == sorted(r[:2] for r in got)
    assert got[-1][0] == moves - 1


@pytest.mark.parametrize("S,eps", [(16, eh.EPS), (24, 0.0)])
def test_full_log_makes_a_game_idle(ddq, S, eps):
    """max_episodes = 2: the coiled game (two first moves, two deaths) fills
    its log at once and idles while the others play on."""
    net = make_net(ddq, S)
    host = eh.EvalHost(net, eh.six_boards(), eh.SEED, S, eps, eh.MAX_MOVES, 2)
    host.run(12)
    create(net, S, eps, eh.MAX_MOVES, 2)
    net.eval_run(12)
    out = eh.assert_same(net, host)
    assert len(host.logs[2]) == 2 and host.logs[2][-1][0] < 10     # idle for two moves at least
    assert out["episodes"].min() < 2                                # while another plays on
    # the idle game neither drew nor moved after its second episode
    assert (out["boards"][2] == eh.six_boards()[2]).all()
    # and on to the end: every log full, every game idle, nothing moves any more
    host.run(40)
    net.eval_run(40)
    out = eh.assert_same(net, host)
    assert list(out["episodes"]) == [2] * N
    net.eval_run(3)
    again = net.eval_read()
    assert again["stats"][0] == 55 and list(again["stats"][1:]) == list(out["stats"][1:])
    np.testing.assert_array_equal(again["log"], out["log"])
    np.testing.assert_array_equal(again["draws"], out["draws"])


@pytest.mark.parametrize("S", [16, 24])
def test_chunked_run_equals_one_call(ddq, runs, S):
    net, host, moves = runs((S, eh.EPS, eh.MAX_MOVES))
    assert moves > 8
    other = make_net(ddq, S)
    create(other, S, eh.EPS, eh.MAX_MOVES, eh.TRIALS)
    for n in (3, 5, moves - 8):
        other.eval_run(n)
    eh.assert_same(other, host)
    other.close()


def test_create_again_resets(ddq):
    S = 16
    net = make_net(ddq, S)
    create(net, S, eh.EPS, eh.MAX_MOVES, 4)
    net.eval_run(9)
    assert net.eval_read()["stats"][0] == 9
    # fewer games, a longer log, another seed
    boards = eh.six_boards()[[2, 0, 5]]
    create(net, S, eh.EPS, eh.MAX_MOVES, 7, boards=boards, seed=5)
    out = net.eval_read()
    assert list(out["stats"]) == [0, 0, 0, 0] and out["log"].shape == (3, 7, 4)
    assert not out["log"].any() and not out["draws"].any()
    np.testing.assert_array_equal(out["boards"], np.repeat(boards[:, None], 4, axis=1))
    host = eh.EvalHost(net, boards, 5, S, eh.EPS, eh.MAX_MOVES, 7)
    host.run(15)
    net.eval_run(15)
    eh.assert_same(net, host)
    net.close()


# ------------------------------------------------------------ the evaluators
def barista(ddq, S, theta):
    from ddq.barista.baristanet import BaristaNet
    net = BaristaNet({"batch": B, "frame": S}, None, None, mode="cpu")
    net.dqn.set_flat(0, theta)
    net.dqn.set_flat(1, theta)
    return net


@pytest.mark.parametrize("eps,mm", [(eh.EPS, eh.MAX_MOVES), (0.0, None)])
def test_device_policy_evaluator_equals_per_game_host(ddq, eps, mm):
    from ddq import evaluation as ev
    S = 16
    net = barista(ddq, S, eh.theta(S))
    boards = eh.six_boards()
    dev = ev.DevicePolicyEvaluator(None, None, net=net, seed=eh.SEED, max_moves=mm, epsilon=eps,
                                   init_state=boards, games=N, chunk=7, move_limit=2000)
    host = ev.PolicyEvaluator(None, None, net=net, seed=eh.SEED, max_moves=mm,
                              streams="per_game", epsilon=eps, init_states=boards)
    models = [None, net.dqn.split(ah.seeded_theta(S, seed=7), "Q")]
    for model in models:
        a = dev.evaluate(model, eh.TRIALS)
        b = host.evaluate(model, eh.TRIALS)
        assert isinstance(a, float) and a == b
        assert dev.episodes == host.episodes and len(dev.episodes) == eh.TRIALS
        assert dev.stats[0] % 7 == 0 and dev.stats[1] >= eh.TRIALS
    # the first model's result is the test host loop's too
    if mm:
        ref = eh.EvalHost(make_net(ddq, S), boards, eh.SEED, S, eps, mm, eh.TRIALS)
        ref.run_until(eh.TRIALS)
        dev.evaluate(net.dqn.split(eh.theta(S), "Q"), eh.TRIALS)
        assert dev.episodes == eh.select_trials(ref.logs, eh.TRIALS)


def test_one_start_board_is_replicated_and_move_limit_raises(ddq):
    from ddq import evaluation as ev
    from ddq.snake import SnakeGame
    S = 16
    net = barista(ddq, S, eh.theta(S))
    dev = ev.DevicePolicyEvaluator(None, None, net=net, seed=4, max_moves=6, epsilon=0.5)
    assert dev.games == B and dev.boards.shape == (B, 10, 10)
    assert (dev.boards == SnakeGame(random.Random(4)).encode_state()).all()
    host = ev.PolicyEvaluator(None, None, net=net, seed=4, max_moves=6, streams="per_game",
                              epsilon=0.5)
    assert dev.evaluate(None, 20) == host.evaluate(None, 20)
    assert dev.episodes == host.episodes
    # the streams differ from game to game although the boards do not
    assert len({r[2:] for r in dev.episodes}) > 1
    slow = ev.DevicePolicyEvaluator(None, None, net=net, seed=4, max_moves=50, chunk=2,
                                    move_limit=4)
    with pytest.raises(RuntimeError):
        slow.evaluate(None, 10 * B)
    with pytest.raises(ValueError):
        ev.PolicyEvaluator(None, None, net=net, streams="each")
    with pytest.raises(ValueError):
        ev.PolicyEvaluator(None, None, net=net, epsilon=0.5)


def test_start_builds_the_device_evaluator(ddq, tmp_path, monkeypatch):
    from ddq import evaluation as ev
    from oracle import ref_numpy as ref
    ev.save_snapshot("centralModel-000500", ref.init_params(16, seed=2), str(tmp_path))
    built = []

    class Fake:
        def __init__(self, arch, model):
            built.append((type(self).__name__, arch, model))

        def evaluate(self, model, num_trials):
            return float(num_trials)

    monkeypatch.setattr(ev, "DevicePolicyEvaluator", type("Dev", (Fake,), {}))
    monkeypatch.setattr(ev, "PolicyEvaluator", type("Host", (Fake,), {}))
    pat = str(tmp_path / "centralModel-*")
    assert list(ev.start("a", "m", pat, num_trials=3, device=True).values()) == [3.0]
    assert list(ev.start("a", "m", pat, num_trials=4).values()) == [4.0]
    assert built == [("Dev", "a", "m"), ("Host", "a", "m")]


def _todays_loop(pe, num_trials):
    """PolicyEvaluator.evaluate as it was before the streams keyword."""
    for eg in pe.engines:
        eg.reset_game()
    total_score = 0
    trials_completed = 0
    scores = [0] * pe.batch_size
    moves = [0] * pe.batch_size
    while trials_completed < num_trials:
        states = np.stack([eg.get_preprocessed_state() for eg in pe.engines])
        actions = pe.net.select_action(states, batch_size=pe.batch_size)
        for i, (action, eg) in enumerate(zip(actions, pe.engines)):
            scores[i] += eg.play_action(eg.actions[int(action)])
            moves[i] += 1
            if eg.game_over or (pe.max_moves is not None and moves[i] >= pe.max_moves):
                total_score += scores[i]
                trials_completed += 1
                if trials_completed == num_trials:
                    break
                eg.reset_game()
                scores[i] = 0
                moves[i] = 0
    return float(total_score) / num_trials


def test_default_policy_evaluator_is_unchanged(ddq):
    from ddq import evaluation as ev
    from ddq.expgain import ExpGain
    S = 16
    net = barista(ddq, S, eh.theta(S))
    for seed, mm in ((5, 20), (6, None)):
        a = ev.PolicyEvaluator(None, None, net=net, seed=seed, max_moves=mm)
        b = ev.PolicyEvaluator(None, None, net=net, seed=seed, max_moves=mm)
        assert len(a.engines) == B and all(type(e) is ExpGain for e in a.engines)
        # one game object and one start board for all engines, as before
        assert len({id(e.game.__self__) for e in a.engines}) == 1
        assert all((e.init_state == a.engines[0].init_state).all() for e in a.engines)
        assert a.evaluate(None, 13) == _todays_loop(b, 13)


# ------------------------------------------------------------ argument errors
def test_argument_errors(ddq):
    from ddq import _lib
    from ddq.actor import zoom_maps
    S = 16
    lib = _lib.load(mode="cpu")
    rm, cm = zoom_maps((S, S), S)
    good = np.ascontiguousarray(eh.six_boards(), np.int8)
    p = _lib.ptr

    def cr(ctx, n=N, b=good, r=rm, c=cm, eps=0.25, mm=8, me=4):
        return lib.ddq_eval_create(ctx, n, p(np.ascontiguousarray(b, np.int8)) if b is not None
                                   else None, p(r) if r is not None else None,
                                   p(c) if c is not None else None, 5, eps, mm, me)

    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    assert cr(None) == _lib.DDQ_EINVAL
    assert lib.ddq_eval_run_async(None, 1) == _lib.DDQ_EINVAL
    assert lib.ddq_eval_read(None, None, None, None, None, None) == _lib.DDQ_EINVAL
    # run / read before create
    assert lib.ddq_eval_run_async(net.ctx, 1) == _lib.DDQ_ESTATE
    assert lib.ddq_eval_read(net.ctx, None, None, None, None, None) == _lib.DDQ_ESTATE
    # null board / maps
    assert cr(net.ctx, b=None) == _lib.DDQ_EINVAL
    assert cr(net.ctx, r=None) == _lib.DDQ_EINVAL
    assert cr(net.ctx, c=None) == _lib.DDQ_EINVAL
    # ngames, epsilon, max_moves, max_episodes
    for n in (0, -1, B + 1):
        assert cr(net.ctx, n=n) == _lib.DDQ_EINVAL
        assert b"ngames" in lib.ddq_last_error(net.ctx)
    for eps in (-0.01, 1.01, float("nan")):
        assert cr(net.ctx, eps=eps) == _lib.DDQ_EINVAL
        assert b"epsilon" in lib.ddq_last_error(net.ctx)
    assert cr(net.ctx, mm=-1) == _lib.DDQ_EINVAL
    assert cr(net.ctx, me=0) == _lib.DDQ_EINVAL
    # map entries outside [0,10)
    for bad in (-1, 10):
        r2, c2 = rm.copy(), cm.copy()
        r2[3], c2[S - 1] = bad, bad
        assert cr(net.ctx, r=r2) == _lib.DDQ_EINVAL
        assert cr(net.ctx, c=c2) == _lib.DDQ_EINVAL
    # a bad board in any game: no snake, one cell, a gap in the codes, a code
    # twice, head and neck apart
    none = np.full((10, 10), -1, np.int8)
    one = none.copy()
    one[6, 5] = 0
    gap = one.copy()
    gap[5, 5] = 2
    twice = one.copy()
    twice[5, 5] = 0
    far = ah.board([(6, 5), (4, 5)], (0, 0))
    diag = ah.board([(6, 5), (5, 4)], (0, 0))
    for bad in (none, one, gap, twice, far, diag):
        for at in (0, N - 1):
            b = good.copy()
            b[at] = bad
            assert cr(net.ctx, b=b) == _lib.DDQ_EINVAL
            assert b"init_boards[%d]" % at in lib.ddq_last_error(net.ctx)
    # a bad board past ngames is not looked at
    b = good.copy()
    b[N - 1] = none
    assert cr(net.ctx, n=N - 1, b=b) == _lib.DDQ_OK
    # nothing above but the last call made an evaluator; create again resets
    assert cr(net.ctx, eps=0.0, mm=0, me=1) == _lib.DDQ_OK
    assert cr(net.ctx, eps=1.0) == _lib.DDQ_OK
    for n in (0, -3):
        assert lib.ddq_eval_run_async(net.ctx, n) == _lib.DDQ_EINVAL
        assert b"nmoves" in lib.ddq_last_error(net.ctx)
    # read with every output null, and with one at a time
    assert lib.ddq_eval_read(net.ctx, None, None, None, None, None) == _lib.DDQ_OK
    stats = np.full(4, -1, np.int64)
    eps_ = np.full(N, -1, np.int32)
    log = np.full((N, 4, 4), -1, np.int32)
    boards = np.zeros((N, 4, 10, 10), np.int8)
    draws = np.full(N, 9, np.uint64)
    assert lib.ddq_eval_read(net.ctx, p(stats), None, None, None, None) == _lib.DDQ_OK
    assert lib.ddq_eval_read(net.ctx, None, p(eps_), None, None, None) == _lib.DDQ_OK
    assert lib.ddq_eval_read(net.ctx, None, None, p(log), None, None) == _lib.DDQ_OK
    assert lib.ddq_eval_read(net.ctx, None, None, None, p(boards), None) == _lib.DDQ_OK
    assert lib.ddq_eval_read(net.ctx, None, None, None, None, p(draws)) == _lib.DDQ_OK
    assert list(stats) == [0, 0, 0, 0] and not eps_.any() and not log.any() and not draws.any()
    assert (boards == good[:, None]).all()
    # epsilon = 1: two draws per move and game (no apple without ... an apple)
    net.eval_run(1)
    assert lib.ddq_eval_read(net.ctx, p(stats), None, None, None, p(draws)) == _lib.DDQ_OK
    assert stats[0] == 1 and stats[3] == draws.sum() and (draws >= 2).all()
    # through the wrapper
    with pytest.raises(_lib.DDQError) as ei:
        net.eval_run(0)
    assert ei.value.code == _lib.DDQ_EINVAL
    with pytest.raises(ValueError):
        net.eval_create(good.ravel()[:150], rm, cm, 1)
    with pytest.raises(ValueError):
        net.eval_create(good, rm[:5], cm, 1)
    fresh = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    with pytest.raises(_lib.DDQError) as ei:
        fresh.eval_read()
    assert ei.value.code == _lib.DDQ_ESTATE
    # no replay ring was needed, and none was made
    assert net.replay_info()[2] == 0
    net.close()
    fresh.close()
