"""n-step returns (ddq_replay_set_nstep, include/ddq_hip.h) restated in numpy /
Python: the allowed start slots, the window and the gather over an exported
ring, and the device index draw with the n-step predicate (the B > 64 form on
_pool_host.wide_rounds, which also counts its rounds).  Shared by
tests/test_nstep.py (CPU twin), tests/test_gpu_nstep.py and the large-batch
tests (tests/test_large_batch.py, tests/test_gpu_large_batch.py).

Per lane: L = lane_len, v = valid, h = head, x = the lane-local slot.  A plain
ring is one lane of L = capacity.  R, g and w are np.float32 values and every
* and + is one np.float32 operation, in the header's order.
"""
import numpy as np

import _pool_host as ph

GAMMA = np.float32(0.85)


def forbidden(x, h, v, L, n):
    d = h - 1 - x
    if d < 0 and n >= 2 and v == L:
        d += L
    return 0 <= d < n


def allowed_slots(h, v, L, n, lanes=1):
    """Every allowed global slot, ascending."""
    return [g * L + x for g in range(lanes) for x in range(v) if not forbidden(x, h, v, L, n)]


def allowed_count(h, v, L, n):
    """A of the header, by its closed forms (checked against the predicate in
    test_nstep.py)."""
    if n == 1:
        return v - 1
    if v == L:
        return L - n
    lo, hi = max(0, h - n), min(h - 1, v - 1)
    return v - max(0, hi - lo + 1)


def window(ring, i, L, n, gamma=GAMMA):
    """(m, R, w, s1, sm) of global slot i."""
    _, _, rw, nt = ring
    gamma = np.float32(gamma)
    base = (i // L) * L
    x = i - base
    s = [None] + [base + (x + k) % L for k in range(1, n + 1)]
    m, term = n, False
    for k in range(1, n + 1):
        if not nt[s[k]]:
            m, term = k, True
            break
    g, R = np.float32(1.0), np.float32(rw[s[1]])
    for k in range(2, m + 1):
        g = np.float32(g * gamma)
        R = np.float32(R + np.float32(g * np.float32(rw[s[k]])))
    w = np.float32(1.0)
    for _ in range(n - 1):
        w = np.float32(w * gamma)
    if term:
        w = np.float32(0.0)
    return m, R, w, s[1], s[m]


def gather(ring, idx, L, n, gamma=GAMMA, with_m=False):
    """The n-step minibatch of the sorted slots idx in read_minibatch's shapes:
    state, action, reward, next_state, non_terminal."""
    st, ac, _, _ = ring
    idx = np.asarray(idx, np.int64)
    B = len(idx)
    ws = [window(ring, int(i), L, n, gamma) for i in idx]
    s1 = np.array([w[3] for w in ws])
    sm = np.array([w[4] for w in ws])
    action = np.zeros((B, 4, 1, 1), np.float32)
    action[np.arange(B), ac[s1]] = 1
    out = (st[idx].astype(np.float32), action,
           np.array([w[1] for w in ws], np.float32).reshape(B, 1, 1, 1),
           st[sm].astype(np.float32),
           np.array([w[2] for w in ws], np.float32).reshape(B, 1, 1, 1))
    return out + ([w[0] for w in ws],) if with_m else out


def assert_minibatch(got, want, what=""):
    names = ("state", "action", "reward", "next_state", "non_terminal")
    for name, g, w in zip(names, got, want):
        g = np.asarray(g)
        assert g.dtype == np.float32, (what, name, g.dtype)
        assert np.array_equal(g.reshape(np.shape(w)), w), (what, name)


def build_ring(rng, cap, S, terminals=(), rewards=None):
    """A ring whose slots differ pairwise; non_terminal is 0 exactly at
    ``terminals``; rewards cycle through {-1, 0, 1} unless given."""
    st = rng.integers(0, 256, (cap, 4, S, S), dtype=np.uint8)
    st[:, 0, 0, 0] = np.arange(cap)
    ac = (np.arange(cap) * 3 % 4).astype(np.uint8)
    rw = ((np.arange(cap) * 2 + 1) % 3 - 1).astype(np.int16)
    for k, v in (rewards or {}).items():
        rw[k] = v
    nt = np.ones(cap, np.uint8)
    nt[list(terminals)] = 0
    return st, ac, rw, nt


# ------------------------------------------------- the gather cases (B = 4)
NB = 4


def index_lists(allowed):
    """Sorted lists of NB allowed slots that together cover every allowed slot."""
    out = [allowed[i:i + NB] for i in range(0, len(allowed), NB)]
    if len(out[-1]) < NB:
        out[-1] = sorted(set(out[-1]) | set(allowed[:NB - len(out[-1])]))
    assert all(len(x) == NB for x in out)
    return out


# the rings of the gather cases: (name, capacity, lanes, head, valid, terminal slots)
TERMINALS = (3, 7, 8)                       # 7, 8: two terminals in one window
REWARDS = {1: 32767, 6: -32767, 10: 32767, 11: -32767}
RINGS = [("partial", 12, 1, 9, 9, TERMINALS), ("full h5", 12, 1, 5, 12, TERMINALS),
         ("full h1", 12, 1, 1, 12, TERMINALS), ("laned 3x6", 18, 3, 2, 6, (3, 4, 10, 17))]


# ------------------------------------------------------------------ the draw
def _draw_fns(seed, ctr, head, valid, lanes, lane_len, n):
    V = lanes * valid

    def draw_at(rnd, pos):
        r = ph.splitmix64(seed ^ ph.splitmix64(
            (ctr * 0x100000001B3 + pos * 0x9E37 + (rnd << 40)) & ph.M64))
        return (r * V) >> 64

    def bad(x):
        return forbidden(x % valid if lanes > 1 else x, head, valid, lane_len, n)

    return draw_at, bad


def _slots(cand, valid, lanes, lane_len):
    if lanes > 1:
        cand = [(x // valid) * lane_len + x % valid for x in cand]
    return np.array(cand, np.int32)


def draw_sorted(seed, ctr, B, head, valid, lanes, lane_len, n):
    """Draw ctr of the device index stream, B <= 64 (the one-wave form: rank by
    (value, position), redraw the forbidden entries and the later ones of a
    duplicate group with the rank as the hash's position)."""
    assert 1 <= B <= 64
    draw_at, bad_x = _draw_fns(seed, ctr, head, valid, lanes, lane_len, n)
    v = [draw_at(0, t) for t in range(B)]
    for rnd in range(1, ph.ROUNDS + 1):
        rank = [sum(o < v[t] for o in v) + sum(v[k] == v[t] for k in range(t)) for t in range(B)]
        bad = [bad_x(v[t]) or any(v[k] == v[t] for k in range(t)) for t in range(B)]
        if not any(bad):
            break
        assert rnd < ph.ROUNDS, "no distinct set"
        v = [draw_at(rnd, rank[t]) if bad[t] else v[t] for t in range(B)]
    out = [0] * B
    for t in range(B):
        out[rank[t]] = v[t]
    return _slots(out, valid, lanes, lane_len)


def draw_sorted_wide(seed, ctr, B, head, valid, lanes, lane_len, n, with_rounds=False):
    """The B > 64 form: sort, redraw the forbidden entries and the later ones of
    equal neighbours with their sorted position, sort again (ph.wide_rounds, the
    one loop).  with_rounds: (slots, rounds taken)."""
    draw_at, bad_x = _draw_fns(seed, ctr, head, valid, lanes, lane_len, n)
    cand, rounds = ph.wide_rounds(draw_at, bad_x, B)
    out = _slots(cand, valid, lanes, lane_len)
    return (out, rounds) if with_rounds else out


def draw(seed, ctr, B, head, valid, lanes, lane_len, n):
    f = draw_sorted if B <= 64 else draw_sorted_wide
    return f(seed, ctr, B, head, valid, lanes, lane_len, n)


def check_allowed(idx, head, valid, lanes, lane_len, n):
    """Sorted, distinct, in the lanes' valid prefixes, none forbidden."""
    idx = np.asarray(idx, np.int64)
    assert (np.diff(idx) > 0).all(), idx
    assert idx.min() >= 0 and idx.max() < lanes * lane_len, idx
    assert (idx % lane_len < valid).all(), idx
    assert not any(forbidden(int(i) % lane_len, head, valid, lane_len, n) for i in idx), idx
