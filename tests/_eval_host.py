"""The host loop the device evaluator (ddq_eval_*) is checked against: N
unmodified ``ExpGain`` engines, each with its own ``SnakeGame`` on
``ActorRng(game_seed(seed, i))``, one batched ``net.select_action`` of the N
states per move, and the contract of include/ddq_hip.h applied by hand: the
coin only when epsilon > 0, then the action when exploring, then the apple;
an episode ends with the game or with its ``max_moves``-th move (game over
wins); one record (end_move, score, moves, ended_by) per episode in the game's
own log; a game whose log is full is idle.  Shared by tests/test_eval_device.py
(CPU twin) and tests/test_gpu_eval.py.

The loop counts what its run covered, and ``check_covered`` asserts it: a test
whose games all did the same thing would pass with Q indexed by the wrong game.
"""
import random

import numpy as np

import _actor_host as ah

ACTIONS = ah.ACTIONS
SEED, EPS, MAX_MOVES, TRIALS = 11, 0.25, 8, 30
# (at S = 24 seed 3 picks one action on every move; 40 and 64: chosen with the
# host loop alone at epsilon 0, check_covered)
THETA_SEED = {16: 3, 24: 5, 40: 9, 64: 7}


def six_boards():
    b = ah.init_boards()
    return np.stack([b["start"], b["apple_ahead"], b["coiled"],
                     ah.board([(2, 2), (2, 3), (2, 4)], (2, 1)),
                     ah.board([(8, 8), (7, 8), (6, 8), (5, 8)], (9, 8)),
                     ah.board([(1, 7), (2, 7)], (5, 2))])


def theta(S):
    return ah.seeded_theta(S, seed=THETA_SEED[S])


def select_trials(logs, num_trials):
    """All records sorted by (end_move, game), the first num_trials."""
    recs = sorted((int(r[0]), i, int(r[1]), int(r[2]), int(r[3]))
                  for i, log in enumerate(logs) for r in log)
    assert len(recs) >= num_trials, (len(recs), num_trials)
    return recs[:num_trials]


class EvalHost:
    def __init__(self, net, boards, seed, S, epsilon=0.0, max_moves=0, max_episodes=TRIALS):
        from ddq import expgain as eg
        from ddq.actor import ActorRng, game_seed
        from ddq.snake import SnakeGame, gray_scale
        self.net, self.S = net, S
        self.epsilon, self.max_moves, self.max_episodes = epsilon, max_moves, max_episodes
        pre = eg.generate_preprocessor((S, S), gray_scale)
        self.games, self.engines = [], []
        for i, b in enumerate(np.asarray(boards).reshape(-1, 10, 10)):
            g = SnakeGame(random.Random(0))        # (its start apple is never seen)
            g.rng = ActorRng(game_seed(seed, i))
            self.games.append(g)
            self.engines.append(eg.ExpGain(None, ACTIONS, pre, self._player(g), None,
                                           np.array(b, np.int64), rng=g.rng))
        n = len(self.engines)
        self.logs = [[] for _ in range(n)]
        self.scores, self.nmoves = [0] * n, [0] * n
        self.move = 0
        self.reward_sum = 0
        self.counts = {"wall": 0, "self": 0, "apple": 0, "max_moves": 0, "explored": 0,
                       "differ": 0}
        self.greedy = set()

    def _player(self, g):
        """SnakeGame.cpu_play of game g, counted: what kind of move this was."""
        from ddq import snake

        def play(state, direction):
            g.set_state(state)
            rev = snake._OPPOSITE[direction] == g.heading
            dx, dy = snake._STEP[g.heading if rev else direction]
            nx, ny = g.body[0][0] + dx, g.body[0][1] + dy
            new, r, over = g.cpu_play(state, direction)
            self.counts["apple"] += r == 1
            if over:
                self.counts["wall" if not (0 <= nx < 10 and 0 <= ny < 10) else "self"] += 1
            return new, r, over
        return play

    def done(self):
        return sum(len(log) for log in self.logs)

    def run(self, nmoves):
        for _ in range(nmoves):
            states = np.stack([e.get_preprocessed_state() for e in self.engines])
            actions = self.net.select_action(states)
            active = [i for i in range(len(self.engines))
                      if len(self.logs[i]) < self.max_episodes]
            chosen = {int(actions[i]) for i in active}
            self.greedy |= chosen
            self.counts["differ"] += len(chosen) > 1
            for i in active:
                e = self.engines[i]
                act = int(actions[i])
                if self.epsilon > 0 and e.rng.random() < self.epsilon:
                    act = e.rng.randrange(4)
                    self.counts["explored"] += 1
                r = e.play_action(ACTIONS[act])
                self.reward_sum += r
                self.scores[i] += r
                self.nmoves[i] += 1
                if e.game_over or (self.max_moves > 0 and self.nmoves[i] >= self.max_moves):
                    self.logs[i].append((self.move, self.scores[i], self.nmoves[i],
                                         0 if e.game_over else 1))
                    self.counts["max_moves"] += not e.game_over
                    e.reset_game()
                    self.scores[i] = self.nmoves[i] = 0
            self.move += 1

    def run_until(self, num_trials, limit=2000):
        """Move by move until num_trials episodes are logged; the moves made."""
        while self.done() < num_trials:
            assert self.move < limit, "no %d trials within %d moves" % (num_trials, limit)
            self.run(1)
        return self.move

    # ---- what ddq_eval_read returns
    def boards(self):
        return np.stack([np.stack(list(e.sequence)) for e in self.engines]).astype(np.int8)

    def draws(self):
        return np.array([g.rng.draws for g in self.games], np.uint64)

    def episodes(self):
        return np.array([len(log) for log in self.logs], np.int32)

    def log(self):
        out = np.zeros((len(self.logs), self.max_episodes, 4), np.int32)
        for i, log in enumerate(self.logs):
            if log:
                out[i, :len(log)] = log
        return out

    def stats(self):
        return [self.move, self.done(), self.reward_sum, int(self.draws().sum())]

    def check_covered(self):
        """The preconditions on the inputs: the run told the games apart and
        met every rule the kernel implements."""
        c = self.counts
        assert c["differ"] >= 1, c
        assert len(self.greedy) >= 3, self.greedy
        assert c["apple"] >= 1 and c["wall"] >= 1 and c["self"] >= 1, c
        assert max(len(log) for log in self.logs) >= 2, self.episodes()
        if self.epsilon > 0:
            assert c["explored"] >= 1, c
            if self.max_moves > 0:
                assert c["max_moves"] >= 1, c
        else:
            assert c["explored"] == 0 and int(self.draws().sum()) == c["apple"], c


def assert_same(net, host):
    """ddq_eval_read of the net against the host loop, no tolerance."""
    out = net.eval_read()
    np.testing.assert_array_equal(out["episodes"], host.episodes())
    np.testing.assert_array_equal(out["log"], host.log())
    np.testing.assert_array_equal(out["draws"], host.draws())
    np.testing.assert_array_equal(out["boards"], host.boards())
    assert list(out["stats"]) == host.stats()
    assert np.array_equal(net.eval_read(full=False), host.episodes())
    return out
