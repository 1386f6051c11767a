"""Device-resident Snake actor: the worker's "act once, add the transition"
(main.py:61-103, ``ExpGain.generate_experience`` expgain.py:82-111) without the
host in it.  ``ddq_actor_step_async`` runs the Q forward of the current
4-frame state, the ε-greedy choice, one Snake move by the rules of
``ddq/snake.py`` and ``add_experience`` into the ctx's ring as two launches on
the ctx stream: no host-to-device copy, no synchronisation.

The random numbers are a contract, so the host loop (unmodified ``ExpGain`` +
``SnakeGame.cpu_play`` with ``rng = ActorRng(seed)``) and the device actor make
the same decisions bit for bit: draw k is ``splitmix64(seed ^ splitmix64(k))``,
one draw per ``random()`` / ``randrange()`` / ``choice()``, in program order
(coin, action when exploring, apple when eaten).

One actor per ctx, as one reference worker is one game + one ring + one net:
``sample_direct`` takes s' from slot idx+1, so a ring holds one trajectory.
A laned ring (``replay_set_lanes``) holds one per lane: ``DeviceActorPool``
plays N games in lock step, one lane each.
"""
from __future__ import annotations

import numpy as np

from . import expgain as eg

_M64 = (1 << 64) - 1
BOARD = 10              # SnakeGame.py: 10x10 board


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def game_seed(seed, i):
    """Seed of game i's stream in a batch of games on one ``seed`` (the device
    evaluator, ``ddq_eval_create``): splitmix64(splitmix64(seed) ^ i)."""
    return splitmix64(splitmix64(int(seed) & _M64) ^ (int(i) & _M64))


class ActorRng:
    """The actor's random stream with the ``random.Random`` methods ``ExpGain``
    and ``SnakeGame`` use; ``draws`` counts the numbers consumed."""

    def __init__(self, seed):
        self.seed = int(seed) & _M64
        self.draws = 0

    def _next(self):
        r = splitmix64(self.seed ^ splitmix64(self.draws))
        self.draws += 1
        return r

    def random(self):
        return (self._next() >> 11) * 2.0 ** -53

    def randrange(self, n):
        if n < 1:
            raise ValueError("empty range for randrange()")
        return (self._next() * int(n)) >> 64

    def choice(self, seq):
        return seq[self.randrange(len(seq))]


def zoom_maps(preprocessor_or_size, S):
    """(row_map, col_map), int32 (S,) each: frame pixel (i, j) shows board cell
    (row_map[i], col_map[j]).  Given a size (int or pair) the maps are read off
    ``expgain.resampler`` applied to index ramps, so they are scipy's
    ``zoom(order=0)`` by construction; given a preprocessor (gray-scale + zoom,
    ``expgain.generate_preprocessor``) they are read off its images of boards
    with one row / one column lit, and checked to reproduce them."""
    S = int(S)
    if callable(preprocessor_or_size):
        probe = np.full((2 * BOARD, BOARD, BOARD), -1, np.int64)
        for k in range(BOARD):
            probe[k, k, :] = -2                    # row k: apples
            probe[BOARD + k, :, k] = -2            # column k
        out = np.asarray(preprocessor_or_size(probe))
        if out.shape != (2 * BOARD, S, S):
            raise ValueError("preprocessor maps (20,10,10) to %s, not (20,%d,%d)"
                             % (out.shape, S, S))
        lit = out != 0
        row_map = np.argmax(lit[:BOARD, :, 0], axis=0).astype(np.int32)
        col_map = np.argmax(lit[BOARD:, 0, :], axis=0).astype(np.int32)
        k = np.arange(BOARD)[:, None, None]
        want = np.concatenate([np.broadcast_to(k == row_map[None, :, None], (BOARD, S, S)),
                               np.broadcast_to(k == col_map[None, None, :], (BOARD, S, S))])
        if not np.array_equal(lit, want):
            raise ValueError("preprocessor is not a separable nearest-neighbour zoom")
        return row_map, col_map
    size = preprocessor_or_size
    size = (int(size), int(size)) if np.isscalar(size) else tuple(int(v) for v in size)
    if size != (S, S):
        raise ValueError("size %s is not the %dx%d frame" % (size, S, S))
    ramps = np.stack([np.repeat(np.arange(BOARD)[:, None], BOARD, axis=1),
                      np.repeat(np.arange(BOARD)[None, :], BOARD, axis=0)]).astype(np.int64)
    out = eg.resampler(size)(ramps)
    return out[0, :, 0].astype(np.int32), out[1, 0, :].astype(np.int32)


class DeviceActor:
    """Drop-in for ``ExpGain`` in the worker loop (``generate_experience``) with
    the game, the preprocessor and the replay add on the device.

    ``net``: a ``DeepQNet`` (or a ``BaristaNet``) whose ctx already holds the
    replay ring; ``init_state``: the (10,10) start board
    (``SnakeGame.encode_state()``), to which every game resets.

    The actor writes the ring the same at any n-step length
    (``net.replay_set_nstep``): the ring is its one trajectory, which is what
    the n-step windows run along, so it needs nothing for them."""

    def __init__(self, net, init_state, seed, preprocessor=None):
        self.net = getattr(net, "dqn", net)
        S = self.net.frame
        self.row_map, self.col_map = zoom_maps(preprocessor if preprocessor is not None
                                               else (S, S), S)
        self.init_state = np.array(init_state, np.int64).reshape(BOARD, BOARD)
        self.seed = int(seed) & _M64
        self.net.actor_create(self.init_state, self.row_map, self.col_map, self.seed)

    def get_epsilon(self, iter_num):
        return eg.epsilon(iter_num)

    def generate_experience(self, iter_num):
        """One act + add at ε(iter_num); enqueued, no synchronisation."""
        self.net.actor_step(1, iter_num)

    def fill(self, n):
        """The initial replay (main.py:176-178): n experiences at ε(0)."""
        if n > 0:
            self.net.actor_step(n, 0)

    def stats(self):
        """Synchronises.  Steps, games ended, reward sum, RNG draws, and the
        4-board history (oldest first)."""
        boards, st = self.net.actor_read()
        return {"steps": int(st[0]), "games": int(st[1]), "reward_sum": int(st[2]),
                "draws": int(st[3]), "boards": boards}

    def act_and_step(self, cfg, n, iter0):
        """n x (one experience at ε(iter0 + k), then one training step), all
        enqueued on the ctx stream; the caller synchronises.

        The training step is the plain graph step (``step_graph(cfg, 1)``), not
        the pipelined one: within a pipelined chain step t+1's minibatch is
        gathered under step t, that is before an act between the two, so it
        would be drawn against the ring as it was before that act's transition.
        That holds per single act.  A chain's first step draws and gathers for
        itself, so a whole chain can follow a move of N lock-step actors:
        ``DeviceActorPool.act_and_train``.

        With prioritized replay on (``net.replay_set_priority``) the act also
        keeps the priority tree (the new slot becomes undrawable, the one
        leaving the head's reach gets the largest priority) and every step
        commits its |TD| before the next draw."""
        for k in range(int(n)):
            self.net.actor_step(1, iter0 + k)
            self.net.step_graph(cfg, 1)


class DeviceActorPool:
    """N lock-step device actors on one ctx, actor i filling lane i of a laned
    ring (``net.replay_set_lanes(N)`` on the empty ring first): one move is one
    batched Q forward and one environment launch and adds N transitions.

    ``init_states``: (N,10,10) start boards, one per game; game i draws from
    ``ActorRng(game_seed(seed, i))`` and otherwise is ``DeviceActor``'s game.

    Nothing here depends on the ring's n-step length (``net.replay_set_nstep``):
    a lane holds one game's trajectory, an n-step window stays inside its lane,
    and ``act_and_train``'s chains draw against the head the round's move left."""

    def __init__(self, net, init_states, seed, preprocessor=None):
        self.net = getattr(net, "dqn", net)
        S = self.net.frame
        self.row_map, self.col_map = zoom_maps(preprocessor if preprocessor is not None
                                               else (S, S), S)
        self.init_states = np.array(init_states, np.int64).reshape(-1, BOARD, BOARD)
        self.ngames = self.init_states.shape[0]
        self.seed = int(seed) & _M64
        self.net.actors_create(self.init_states, self.row_map, self.col_map, self.seed)

    def get_epsilon(self, iter_num):
        return eg.epsilon(iter_num)

    def generate_experience(self, iter_num):
        """One move of all games at ε(iter_num): N transitions; enqueued, no
        synchronisation."""
        self.net.actors_step(1, iter_num)

    def fill(self, nmoves):
        """The initial replay: nmoves moves (N · nmoves experiences) at ε(0)."""
        if nmoves > 0:
            self.net.actors_step(nmoves, 0)

    def stats(self):
        """Synchronises.  The games' totals (steps, games ended, reward sum,
        RNG draws), the same per game (N,4), and the 4-board histories."""
        boards, per_game, tot = self.net.actors_read()
        return {"steps": int(tot[0]), "games": int(tot[1]), "reward_sum": int(tot[2]),
                "draws": int(tot[3]), "per_game": per_game, "boards": boards}

    def act_and_train(self, cfg, rounds, iter0):
        """rounds x (one move at ε(iter0 + r·N), then N training steps as one
        pipelined chain), all enqueued on the ctx stream; the caller
        synchronises.  Act and train stay 1:1.  The chain's first step draws and
        gathers after the move, so every minibatch of a round is drawn against
        the ring as the round's move left it.  With prioritized replay on
        (``net.replay_set_priority``) the move keeps the priority tree lane by
        lane, and inside the chain each step's commit precedes the next step's
        draw, exactly as in the same sequence issued eagerly."""
        n = self.ngames
        for r in range(int(rounds)):
            self.net.actors_step(1, iter0 + r * n)
            self.net.step_pipelined(cfg, n)
