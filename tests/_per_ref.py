"""Prioritized replay (ddq_replay_set_priority, include/ddq_hip.h) restated in
numpy and Python integers: the invariant, the writer rule, the stratified draw,
the importance-sampling weights and the commit in float64, and the weighted
head recomputed from a net's own blobs (the method of tests/_objective_ref.py).
Shared by tests/test_per.py (CPU twin) and tests/test_gpu_per.py.

Leaves are Python ints / np.uint32; every sum is a Python int, so the draw is
exact whatever the device's tree looks like.
"""
import numpy as np

import _nstep_ref as nr
import _objective_ref as objr
import _pool_host as ph

ONE, QMAX = 1 << 16, 1 << 24


# ------------------------------------------------------------------ invariant
def expected_zero(head, valid, L, n, lanes=1):
    """Bool per slot: unfilled or forbidden (nr.forbidden per lane)."""
    z = np.ones(lanes * L, bool)
    for g in range(lanes):
        for x in range(valid):
            z[g * L + x] = nr.forbidden(x, head, valid, L, n)
    return z


def check_invariant(q, total, head, valid, L, n, lanes=1, what=""):
    q = np.asarray(q)
    want = expected_zero(head, valid, L, n, lanes)
    assert np.array_equal(q == 0, want), (what, q.tolist(), want.tolist())
    assert total == sum(int(v) for v in q), (what, total)
    assert q.max(initial=0) <= QMAX


# ------------------------------------------------------------------ writer rule
def writer(q, pmax, base, h, L, n, head2, valid2):
    """One add at lane-local slot h of the lane at `base`; head2 / valid2 are the
    lane's values after the add.  Returns the slot released (or None)."""
    q[base + h] = 0 if nr.forbidden(h, head2, valid2, L, n) else pmax
    x = h - n
    if x < 0 and valid2 == L:
        x += L
    if x >= 0 and x != h and q[base + x] == 0:
        q[base + x] = pmax
        return base + x
    return None


# ------------------------------------------------------------------ draw
def draw(q, B, seed, ctr):
    """(idx int32[B], total): draw `ctr` of the prioritized index stream."""
    q = [int(v) for v in q]
    T = sum(q)
    C = [0]
    for v in q:
        C.append(C[-1] + v)                 # C[i]: exclusive prefix sum at slot i
    lo = [T * j // B for j in range(B + 1)]
    idx = []
    for j in range(B):
        r = ph.splitmix64(seed ^ ph.splitmix64((ctr * 0x100000001B3 + j * 0x9E37) & ph.M64))
        u = lo[j] + ((r * (lo[j + 1] - lo[j])) >> 64)
        i = int(np.searchsorted(np.asarray(C[1:], dtype=object), u, side="right"))
        assert C[i] <= u < C[i + 1] and q[i] > 0
        idx.append(i)
    return np.asarray(idx, np.int32), T


def isw64(q, idx, beta):
    """The weights in float64 from the leaves the draw saw."""
    qs = np.asarray([int(q[i]) for i in idx], np.float64)
    return (qs.min() / qs) ** float(beta)


# ------------------------------------------------------------------ commit
def leaf_of64(d, eps, alpha):
    p = (abs(float(d)) + float(np.float32(eps))) ** float(np.float32(alpha))
    if not np.isfinite(p):
        return QMAX
    return int(min(max(np.rint(p * 65536.0), 1), QMAX))


def commit64(q_before, idx, q_sa, tgt, eps, alpha):
    """{slot: float64 reference leaf} of the slots a commit writes: nonzero
    leaves only, the highest b of a repeated slot."""
    out = {}
    for b, i in enumerate(idx):
        if int(q_before[i]) == 0:
            continue
        d = np.float32(np.float32(q_sa[b]) - np.float32(tgt[b]))
        out[int(i)] = leaf_of64(d, eps, alpha)
    return out


def check_commit(q_before, q_after, total, pmax_before, pmax_after, idx, q_sa, tgt, eps, alpha,
                 what=""):
    """Untouched leaves unchanged; a touched leaf v within one rounding quantum
    plus the project's rtol of the float64 reference (powf differs between the
    device and numpy); pmax and total consistent with the leaves."""
    ref = commit64(q_before, idx, q_sa, tgt, eps, alpha)
    for i in range(len(q_before)):
        if i not in ref:
            assert int(q_after[i]) == int(q_before[i]), (what, i)
        else:
            v, r = int(q_after[i]), ref[i]
            assert abs(v - r) <= 1 + 1e-4 * r, (what, i, v, r)
    assert total == sum(int(v) for v in q_after), what
    wrote = [int(q_after[i]) for i in ref]
    assert pmax_after == max([pmax_before] + wrote), (what, pmax_before, pmax_after, wrote)
    return ref


# ------------------------------------------------------------------ head
def expected_weighted_head(got, isw, act, nt, r, gamma, target="max", delta=None):
    """objr.expected_head_f32 with the weight: t = c / (float)B; dQ scale =
    isw * t; loss term = isw * le, each product one np.float32 operation."""
    e = objr.expected_head_f32(got, act, nt, r, gamma, target, delta)
    B = act.shape[0]
    w = np.asarray(isw, np.float32).reshape(B)
    d = e["d"]
    if delta is None:
        dc = d
        le = (d * d).astype(np.float32)
    else:
        dl = np.float32(delta)
        dc = np.minimum(np.maximum(d, -dl), dl).astype(np.float32)
        ad = np.abs(d)
        le = np.where(ad <= dl, (d * d).astype(np.float32),
                      (dl * (np.float32(2.0) * ad - dl).astype(np.float32)).astype(np.float32))
    t = (dc / np.float32(B)).astype(np.float32)
    gsc = (w * t).astype(np.float32)
    e["dQ"] = (act.astype(np.float32) * gsc[:, None]).astype(np.float32)
    e["loss"] = float((w.astype(np.float64) * le.astype(np.float64)).sum() / B / 2.0)
    return e


def check_weighted_head(net, gamma, target="max", delta=None, what=""):
    """The net's last pass: P_sa and Q_out.diff bit for bit in fp32 from its own
    blobs and weights, the target within one ulp of its float64 value, the loss
    within the project's rtol (the head's two-term target may contract to an FMA
    and the loss is a sum: _objective_ref's rule for both)."""
    B = net.batch
    names = ["Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss", "Q_out.diff"]
    if target == "double":
        names.append("Qn_out")
    got = objr.blobs_of(net, names)
    isw = net.blob("is_weight").reshape(B)
    _, act, rw, _, nt = net.read_minibatch()
    act, rw, nt = act.reshape(B, 4), rw.reshape(B), nt.reshape(B)
    e = expected_weighted_head(got, isw, act, nt, rw, gamma, target, delta)
    assert got["P_sa"].tobytes() == e["P_sa"].tobytes(), what
    ulp = np.spacing(np.abs(e["target64"]).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got["target_Q_sa"].astype(np.float64) - e["target64"]) <= ulp), what
    assert got["Q_out.diff"].tobytes() == e["dQ"].tobytes(), what
    print("%sloss %.9g, from the blobs %.9g" % (what, float(got["loss"][0]), e["loss"]))
    np.testing.assert_allclose(float(got["loss"][0]), e["loss"], rtol=1e-4)
    return got, isw


# ------------------------------------------------------------------ hand-built leaves
def leaf_cases(cap, allowed):
    """{name: {slot: leaf}} over the allowed slots of a ring: uniform; one leaf
    at 2^24 among leaves of 1 (forces duplicates); a run of more than 64 leaves
    of 1 between heavy ends (the draw must skip it -- a zero leaf cannot be set on
    a filled slot, the zero runs are the ring's unfilled tail); mass only in the
    last (ragged) 64-slot node."""
    allowed = list(allowed)
    out = {"uniform": {i: ONE for i in allowed}}
    big = allowed[len(allowed) // 3]
    out["one big"] = {i: (QMAX if i == big else 1) for i in allowed}
    if len(allowed) > 80:
        out["light run"] = {i: (1 if 3 <= k < len(allowed) - 3 else 5 * ONE)
                            for k, i in enumerate(allowed)}
        last = (allowed[-1] // 64) * 64
        out["last node"] = {i: (ONE + i if i >= last else 1) for i in allowed}
    return out
