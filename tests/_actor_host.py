"""The host acting loop the device actor is checked against: unmodified
``ExpGain`` + ``SnakeGame.cpu_play`` with ``rng = ActorRng(seed)``, greedy
actions from the given net's ``select_action``, the oracle's ``ReplayRef`` as
the ring.  Shared by tests/test_actor.py (CPU twin) and tests/test_gpu_actor.py.
"""
import random

import numpy as np

from oracle import ref_numpy as ref

ACTIONS = ["w", "a", "s", "d"]
CAPACITY = 37                      # the ring wraps more than once in every run
RAMP = (49990, 50010)              # the epsilon schedule's knee

# epsilon regimes: iteration number of call k
REGIMES = {
    "eps1": lambda k: 0,                                   # epsilon = 1: every action random
    "eps01": lambda k: 60000,                              # epsilon = 0.1: mostly greedy
    "ramp": lambda k: RAMP[0] + k % (RAMP[1] - RAMP[0] + 1),
}


def board(body, apple):
    """Board codes of SnakeGame.encode_state for a body (head first) and an apple."""
    b = np.full((10, 10), -1, np.int64)
    b[apple] = -2
    for k, cell in enumerate(body):
        b[cell] = k
    return b


def init_boards():
    from ddq.snake import SnakeGame
    return {
        # the reference start: head (6,5), tail (5,5), heading east, one apple
        "start": SnakeGame(random.Random(0)).encode_state(),
        # apple directly ahead: the first non-turning move eats it
        "apple_ahead": board([(6, 5), (5, 5)], (7, 5)),
        # coiled, length 7, heading south into its own body: of the four first
        # moves only 'a' survives ('w' is a reversal and keeps the heading)
        "coiled": board([(4, 4), (4, 5), (5, 5), (5, 4), (5, 3), (4, 3), (3, 3)], (0, 0)),
    }


def seeded_theta(S, seed=3):
    """Non-zero weights: the fillers scaled up so Q depends on the frames."""
    pq = ref.init_params(S, seed=seed)
    for k in pq:
        pq[k][0] = (pq[k][0] * 3).astype(np.float32)
    return ref.flatten(pq)


class _Greedy:
    """The net as ExpGain sees it: select_action of one state -> one index."""

    def __init__(self, net):
        self.net = net

    def select_action(self, pstate):
        return int(self.net.select_action(pstate)[0])


class HostLoop:
    def __init__(self, net, init_state, seed, S, capacity=CAPACITY):
        from ddq import expgain as eg
        from ddq.actor import ActorRng
        from ddq.snake import SnakeGame, gray_scale
        self.rng = ActorRng(seed)
        self.game = SnakeGame(random.Random(0))   # (its start apple is not the actor's draw)
        self.game.rng = self.rng
        self.ring = ref.ReplayRef((4, S, S), capacity)
        self.counts = {"wall": 0, "self": 0, "apple": 0, "reversed": 0, "steps": 0, "games": 0,
                       "reward_sum": 0}
        pre = eg.generate_preprocessor((S, S), gray_scale)
        self.xp = eg.ExpGain(_Greedy(net), ACTIONS, pre, self._play, self.ring,
                             np.array(init_state, np.int64), rng=self.rng)

    def _play(self, state, direction):
        """SnakeGame.cpu_play, counted: what kind of move this was."""
        from ddq import snake
        g = self.game
        g.set_state(state)
        rev = snake._OPPOSITE[direction] == g.heading
        dx, dy = snake._STEP[g.heading if rev else direction]
        nx, ny = g.body[0][0] + dx, g.body[0][1] + dy
        new, r, over = g.cpu_play(state, direction)
        c = self.counts
        c["steps"] += 1
        c["reward_sum"] += r
        c["reversed"] += rev
        c["apple"] += r == 1
        if over:
            c["games"] += 1
            c["wall" if not (0 <= nx < 10 and 0 <= ny < 10) else "self"] += 1
        return new, r, over

    def run(self, iters):
        for it in iters:
            self.xp.generate_experience(it)

    def boards(self):
        return np.stack(list(self.xp.sequence)).astype(np.int8)

    def stats(self):
        c = self.counts
        return [c["steps"], c["games"], c["reward_sum"], self.rng.draws]


def assert_same(net, host):
    """The net's ring, head / valid, boards and stats against the host loop's."""
    st, ac, rw, nt = net.replay_export()
    r = host.ring
    head, valid, cap = net.replay_info()
    assert (head, valid, cap) == (r.head, r.valid, r.N)
    np.testing.assert_array_equal(ac, r.action)
    np.testing.assert_array_equal(rw, r.reward)
    np.testing.assert_array_equal(nt, r.non_terminal)
    np.testing.assert_array_equal(st, r.state)
    boards, stats = net.actor_read()
    np.testing.assert_array_equal(boards, host.boards())
    assert list(stats) == host.stats()
