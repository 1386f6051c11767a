"""The host loop the device actor pool (ddq_actors_*) is checked against, and a
Python restatement of the device index draw on plain and laned rings.  Shared by
tests/test_actor_pool.py (CPU twin) and tests/test_gpu_actor_pool.py.

``PoolHost``: N unmodified ``ExpGain`` engines, each with its own ``SnakeGame``
on ``ActorRng(game_seed(seed, i))`` and its own ``ReplayRef`` of one lane's
length; per move one batched ``net.select_action`` of the N states, then every
engine's unmodified ``generate_experience``: the coin (always), the action when
exploring, the apple when eaten, ``add_experience`` into its own lane.  The
laned ring is the lanes concatenated in slot order; head / valid are any
lane's (they move in lock step).

The loop counts what its run covered and ``check_covered`` asserts it: a run
whose games all did the same thing would pass with Q indexed by the wrong game.

``draw_sorted``: include/ddq_hip.h's draw for B <= 64 as kernels.hip computes
it -- the hash, the rank by (value, position), the redraw of forbidden values
and of the later entries of a duplicate group with the rank as position -- on
x in [0, lanes * valid), forbidden iff head >= 1 and x mod valid == head - 1,
the final sorted x mapped to slots (x div valid) * lane_len + x mod valid.

``wide_rounds``: the B > 64 (sort, redraw, sort again) loop, once, for this
module's and tests/_nstep_ref.py's ``draw_sorted_wide``; it returns the round
that found the set, which tests/test_large_batch.py holds to a cap.
"""
import random

import numpy as np

import _actor_host as ah
from oracle import ref_numpy as ref

ACTIONS = ah.ACTIONS
M64 = (1 << 64) - 1


def three_boards():
    b = ah.init_boards()
    return np.stack([b["start"], b["apple_ahead"], b["coiled"]])


def four_boards():
    return np.concatenate([three_boards(), ah.board([(2, 2), (2, 3), (2, 4)], (2, 1))[None]])


class _Batched:
    """The net as engine i sees it: the action the batched forward gave its state."""

    def __init__(self):
        self.action = 0
        self.asked = 0

    def select_action(self, pstate):
        self.asked += 1
        return self.action


class PoolHost:
    def __init__(self, net, boards, seed, S, lane_len, seeds=None):
        from ddq import expgain as eg
        from ddq.actor import ActorRng, game_seed
        from ddq.snake import SnakeGame, gray_scale
        self.net, self.S, self.L = net, S, lane_len
        pre = eg.generate_preprocessor((S, S), gray_scale)
        boards = np.asarray(boards).reshape(-1, 10, 10)
        self.games, self.engines, self.stubs, self.lanes = [], [], [], []
        self.counts = {"wall": 0, "self": 0, "apple": 0, "differ": 0, "games": 0}
        self.per_game = [[0, 0, 0] for _ in boards]      # steps, games, reward sum
        self.greedy = set()
        for i, b in enumerate(boards):
            g = SnakeGame(random.Random(0))              # (its start apple is never seen)
            g.rng = ActorRng(game_seed(seed, i) if seeds is None else seeds[i])
            stub, lane = _Batched(), ref.ReplayRef((4, S, S), lane_len)
            self.games.append(g)
            self.stubs.append(stub)
            self.lanes.append(lane)
            self.engines.append(eg.ExpGain(stub, ACTIONS, pre, self._player(g, i), lane,
                                           np.array(b, np.int64), rng=g.rng))

    def _player(self, g, i):
        """SnakeGame.cpu_play of game g, counted: what kind of move this was."""
        from ddq import snake

        def play(state, direction):
            g.set_state(state)
            rev = snake._OPPOSITE[direction] == g.heading
            dx, dy = snake._STEP[g.heading if rev else direction]
            nx, ny = g.body[0][0] + dx, g.body[0][1] + dy
            new, r, over = g.cpu_play(state, direction)
            self.counts["apple"] += r == 1
            pg = self.per_game[i]
            pg[0] += 1
            pg[1] += bool(over)
            pg[2] += r
            if over:
                self.counts["games"] += 1
                self.counts["wall" if not (0 <= nx < 10 and 0 <= ny < 10) else "self"] += 1
            return new, r, over
        return play

    def run(self, iters):
        for it in iters:
            states = np.stack([e.get_preprocessed_state() for e in self.engines])
            actions = self.net.select_action(states)
            chosen = {int(a) for a in actions}
            self.greedy |= chosen
            self.counts["differ"] += len(chosen) > 1
            for e, stub, a in zip(self.engines, self.stubs, actions):
                stub.action = int(a)
                e.generate_experience(it)

    # ---- what the ring and ddq_actors_read hold
    def ring(self):
        cat = lambda f: np.concatenate([getattr(r, f) for r in self.lanes])
        return cat("state"), cat("action"), cat("reward"), cat("non_terminal")

    def head_valid(self):
        hv = {(r.head, r.valid) for r in self.lanes}
        assert len(hv) == 1, hv
        return hv.pop()

    def boards(self):
        return np.stack([np.stack(list(e.sequence)) for e in self.engines]).astype(np.int8)

    def stats(self):
        return np.array([pg + [g.rng.draws] for pg, g in zip(self.per_game, self.games)],
                        np.int64)

    def check_covered(self):
        c = self.counts
        assert c["differ"] >= 1, c
        assert len(self.greedy) >= 2, self.greedy
        assert c["apple"] >= 1 and c["wall"] >= 1 and c["self"] >= 1 and c["games"] >= 1, c


def assert_same(net, host):
    """The net's laned ring, per-lane head / valid, boards, per-game stats and
    draws against the host loop's, no tolerance."""
    st, ac, rw, nt = net.replay_export()
    hs, ha, hr, hn = host.ring()
    n = len(host.engines)
    assert net.replay_info() == host.head_valid() + (n * host.L,)
    assert net.replay_lanes() == (n, host.L)
    np.testing.assert_array_equal(ac, ha)
    np.testing.assert_array_equal(rw, hr)
    np.testing.assert_array_equal(nt, hn)
    np.testing.assert_array_equal(st, hs)
    boards, stats, totals = net.actors_read()
    np.testing.assert_array_equal(boards, host.boards())
    np.testing.assert_array_equal(stats, host.stats())
    np.testing.assert_array_equal(totals, host.stats().sum(axis=0))


# ---------------------------------------------------------------- the gather
def lane_next(idx, lane_len):
    """The next slot within the lane of every slot in idx."""
    j = np.asarray(idx, np.int64) + 1
    return np.where(j % lane_len == 0, j - lane_len, j)


def lane_gather(ring, idx, lane_len):
    """sample_direct's gather (replay.py:159-183) with the per-lane wrap, in
    read_minibatch's shapes: state, action, reward, next_state, non_terminal."""
    st, ac, rw, nt = ring
    idx = np.asarray(idx, np.int64)
    nxt = lane_next(idx, lane_len)
    B = len(idx)
    action = np.zeros((B, 4, 1, 1), np.float32)
    action[np.arange(B), ac[nxt]] = 1
    return (st[idx].astype(np.float32), action,
            rw[nxt].astype(np.float32).reshape(B, 1, 1, 1), st[nxt].astype(np.float32),
            np.asarray(nt)[nxt].astype(np.float32).reshape(B, 1, 1, 1))


def random_ring(rng, cap, S):
    """A ring whose slots differ pairwise (frames and scalars)."""
    st = rng.integers(0, 256, (cap, 4, S, S), dtype=np.uint8)
    st[:, 0, 0, 0] = np.arange(cap)                      # pairwise different for sure
    ac = (np.arange(cap) * 3 % 4).astype(np.uint8)
    rw = (np.arange(cap) - 7).astype(np.int16)
    nt = (np.arange(cap) % 3 != 0)
    return st, ac, rw, nt


# ------------------------------------------------------------------ the draw
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


ROUNDS = 4096


def _draw_fns(seed, ctr, head, valid, lanes):
    V = lanes * valid

    def draw_at(rnd, pos):
        r = splitmix64(seed ^ splitmix64((ctr * 0x100000001B3 + pos * 0x9E37 + (rnd << 40)) & M64))
        return (r * V) >> 64

    def forbidden(x):
        if lanes > 1:
            return head >= 1 and x % valid == head - 1
        return x == head - 1                             # head 0: -1 matches no draw

    return draw_at, forbidden


def wide_rounds(draw_at, forbidden, B):
    """The B > 64 loop itself: (the sorted distinct x, the round that found them).
    Round r is the r-th check of a sorted candidate set; the kernel gives up
    after ROUNDS of them."""
    assert B > 64
    cand = [draw_at(0, t) for t in range(B)]
    for rnd in range(1, ROUNDS + 1):
        cand.sort()
        bad = [forbidden(cand[t]) or (t > 0 and cand[t] == cand[t - 1]) for t in range(B)]
        if not any(bad):
            break
        assert rnd < ROUNDS, "no distinct set"
        cand = [draw_at(rnd, t) if bad[t] else cand[t] for t in range(B)]
    return cand, rnd


def draw_sorted_wide(seed, ctr, B, head, valid, lanes=1, lane_len=None, with_rounds=False):
    """The same draw as the kernel's B > 64 path computes it: sort, redraw the
    forbidden entries and the later ones of equal neighbours with their sorted
    position as the hash's position input, sort again.  with_rounds: (slots,
    rounds taken)."""
    draw_at, forbidden = _draw_fns(seed, ctr, head, valid, lanes)
    cand, rounds = wide_rounds(draw_at, forbidden, B)
    if lanes > 1:
        cand = [(x // valid) * lane_len + x % valid for x in cand]
    out = np.array(cand, np.int32)
    return (out, rounds) if with_rounds else out


def draw_sorted(seed, ctr, B, head, valid, lanes=1, lane_len=None):
    """Draw number ctr of the device index stream on ``seed``: B <= 64 sorted
    slots.  head / valid per lane."""
    assert 1 <= B <= 64
    draw_at, forbidden = _draw_fns(seed, ctr, head, valid, lanes)
    v = [draw_at(0, t) for t in range(B)]
    for rnd in range(1, ROUNDS + 1):
        rank = [sum(o < v[t] for o in v) + sum(v[k] == v[t] for k in range(t)) for t in range(B)]
        bad = [forbidden(v[t]) or any(v[k] == v[t] for k in range(t)) for t in range(B)]
        if not any(bad):
            break
        assert rnd < ROUNDS, "no distinct set"
        v = [draw_at(rnd, rank[t]) if bad[t] else v[t] for t in range(B)]
    out = [0] * B
    for t in range(B):
        out[rank[t]] = v[t]
    if lanes > 1:
        out = [(x // valid) * lane_len + x % valid for x in out]
    return np.array(out, np.int32)


def check_draw(idx, B, head, valid, lanes, lane_len):
    """The invariants of a drawn set: sorted, distinct, no forbidden slot, every
    slot in its lane's valid prefix."""
    idx = np.asarray(idx, np.int64)
    assert idx.shape == (B,) and (np.diff(idx) > 0).all(), idx
    assert idx.min() >= 0 and idx.max() < lanes * lane_len, idx
    assert (idx % lane_len < valid).all(), idx
    if head >= 1:
        assert not (idx % lane_len == head - 1).any(), idx
