"""The recipe the acting forward (launch_act: ddq_forward_q, ddq_select_action,
the device environments) is checked by, on the unmodified float64 oracle
(oracle/ref_numpy.py).  Plain numpy; shared by tests/test_acting_ref.py (the
oracle alone and the CPU twin) and tests/test_gpu_acting.py.

Inputs of a case ``(S, n, kind)``: ``rng = default_rng(500 + S + n)``, then the
"x3" parameters as test_gpu_parity.make_params draws them (seed-7 fillers x 3,
N(0, 0.05) biases), then ``n`` uint8 states: kind "u" uniform 0..255, kind "s"
sparse {0, 200, 255} with p = .9 / .08 / .02.

Values: ``check_values`` holds a Q_out to the oracle's under the three rules of
tests/_parity.py (``close(..., mag=M)``) with their constants unchanged.

Actions: under the x3 parameters nearly every state picks one action (all 33
uniform states at S = 16 pick action 2), and an argmax test on such data cannot
see two images swapped.  ``centred`` keeps the parameters and moves Q_out's bias
to float32(b5 - mean_b Q0), which spreads the states over the four actions
(n = 1 keeps its bias: one state is its own mean).
``margin(Q0) = 2e-5 * ||Q0||_2`` is derived: rule 2 of ``close`` holds a Q_out
normwise to NORM_RTOL = 1e-5 of ||Q0||, which bounds every element's error;
centring changes one bias add only, so each of the two Q values an argmax
compares lies within 1e-5 * ||Q0|| of the oracle's.  A state whose top-two gap
in the oracle (under the centred bias) exceeds the margin is *decided*: a
forward that passes ``check_values`` must pick the oracle's action there.

``conditions`` asserts on the oracle alone, before any result is looked at,
that a case can tell images apart: at most floor(0.02 n) undecided states, at
least min(n, 2) distinct oracle actions, all four for n >= 16.
"""
import numpy as np

from _parity import NORM_RTOL, close

# ---- the cases ---------------------------------------------------------------
# values, ctx batch = n: (S, n), kinds alternating "u" / "s" down the list.
VALUE_SN = [
    # every frame of the sweep 16..128 / 8 at a tiny n
    (16, 1), (24, 1), (32, 2), (40, 3), (48, 2), (56, 1), (64, 3), (72, 3), (80, 2), (88, 1),
    (96, 2), (104, 3), (112, 1), (120, 3), (128, 2),
    # launch_fc4_fwd's switch after n = 32 from the one-tile kernel to 64-image
    # tiles, ragged last tiles, on the general kernels
    (24, 31), (24, 32), (24, 33), (24, 64), (24, 65), (64, 33),
    # the small-map tower at nz = 1: the two-workgroup split form through
    # n = 128, the whole form after it, the general kernels past 256
    (16, 2), (16, 64), (16, 65), (16, 128), (16, 129), (16, 256), (16, 257),
]
# actions, n states on a ctx of batch B >= n: (S, B, n), kinds alternating too
ACTION_SBN = [
    (16, 256, 1), (16, 256, 5), (16, 256, 65), (16, 256, 128), (16, 256, 129), (16, 256, 256),
    (16, 300, 7), (16, 300, 257),
    (24, 65, 1), (24, 65, 33), (24, 65, 65),
    (40, 8, 7), (64, 33, 5), (64, 33, 33), (72, 8, 5), (104, 8, 5), (120, 8, 5),
    (128, 4, 1), (128, 4, 4),
]
# the CPU twin's cases (tests/test_acting_ref.py): n states on a ctx of batch 8
TWIN_SBN = [(16, 8, 5), (24, 8, 3)]
TIE_CASES = [(16, 33, "u"), (24, 33, "s")]
TWIN_TIE_CASES = [(16, 5, "u"), (24, 3, "u")]
MUTATION_SN = (64, 33)             # on the GPU's own Q_out


def _kinds(cases):
    return [c + ("us"[i % 2],) for i, c in enumerate(cases)]


VALUE_CASES = _kinds(VALUE_SN)             # (S, n, kind)
ACTION_CASES = _kinds(ACTION_SBN)          # (S, B, n, kind)
MUTATION_CASE = next(c for c in VALUE_CASES if c[:2] == MUTATION_SN)


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def oracle_cases():
    """Every (S, n, kind) the GPU tests put to the oracle, once each."""
    seen = []
    for c in VALUE_CASES + [(S, n, k) for (S, B, n, k) in ACTION_CASES]:
        if c not in seen:
            seen.append(c)
    return seen


# ---- the recipe ----------------------------------------------------------------
def f64(a):
    return np.asarray(a, np.float64)


def draw(ref, S, n, kind):
    """(pQ, pP, states) of a case; pP only feeds ref.magnitudes' other tower."""
    from test_gpu_parity import make_params
    rng = np.random.default_rng(500 + S + n)
    pQ, pP = make_params(ref, rng, S, "x3")
    if kind == "u":
        states = rng.integers(0, 256, (n, 4, S, S)).astype(np.uint8)
    else:
        states = rng.choice(np.array([0, 200, 255], np.uint8), (n, 4, S, S), p=[0.9, 0.08, 0.02])
    return pQ, pP, states


def other_states(S, B, n):
    """B states that are not the case's: what the shared acting scratch holds
    before the n states are put to a ctx of batch B."""
    return np.random.default_rng(7000 + S + B + n).integers(0, 256, (B, 4, S, S)).astype(np.uint8)


def forward64(ref, pQ, states):
    return ref.net_forward(f64(states), {k: [f64(w) for w in v] for k, v in pQ.items()},
                           "Q")["out"]


def oracle_q(ref, pQ, states, pP=None):
    """(Q0, M): the float64 Q_out of the states and its routed forward
    magnitudes (per-element sum of |terms|), from ref.magnitudes with dummy
    action, reward and non-terminal arrays as tests/_objective_ref.py gets
    Qn_out's."""
    n = np.asarray(states).shape[0]
    Q0 = forward64(ref, pQ, states)
    if pP is None:
        pP = {"P" + k[1:]: v for k, v in pQ.items()}
    st = f64(states)
    dummy = np.zeros((n, 4, 1, 1)), np.zeros((n, 1, 1, 1)), st, np.ones((n, 1, 1, 1))
    M = ref.magnitudes(pQ, pP, st, *dummy)[0]["Q_out"]
    return Q0, M


def centred(pQ, Q0):
    """pQ with Q_out's bias moved to float32(b5 - mean_b Q0).  A single state
    is its own mean: centring would leave it four zeros, nothing decided, so at
    n = 1 (where there are no two images to swap) the bias stays."""
    out = {k: [w.copy() for w in v] for k, v in pQ.items()}
    b5 = out["Q_out"][1]
    if Q0.shape[0] == 1:
        return out
    out["Q_out"][1] = (f64(b5) - Q0.mean(axis=0).reshape(b5.shape)).astype(np.float32)
    return out


def centred_q(pQ, pC, Q0):
    """The oracle's Q_out under centred()'s parameters: one bias add differs."""
    return Q0 + (f64(pC["Q_out"][1]) - f64(pQ["Q_out"][1])).reshape(1, 4)


def margin(Q0):
    return 2 * NORM_RTOL * float(np.linalg.norm(f64(Q0).ravel()))


def decided(Qc, m):
    """The states whose top-two gap in Qc exceeds m."""
    top = np.sort(Qc, axis=1)
    return (top[:, -1] - top[:, -2]) > m


def conditions(Q0, Qc):
    """The recipe's conditions on the oracle alone.  Returns (decided mask,
    oracle actions)."""
    n = Q0.shape[0]
    dec = decided(Qc, margin(Q0))
    acts = np.argmax(Qc, axis=1)
    undecided = int((~dec).sum())
    assert undecided <= int(np.floor(0.02 * n)), ("undecided states", undecided, n)
    distinct = len(set(acts.tolist()))
    assert distinct >= min(n, 2), ("distinct oracle actions", distinct, n)
    if n >= 16:
        assert distinct == 4, ("distinct oracle actions", distinct, n)
    return dec, acts


_CACHE = {}


def case(ref, S, n, kind, mags=False):
    """A case's parameters, states and oracle, computed once, shared by the
    tests and left unchanged: pQ, pP, states, Q0, pC (centred), Qc, margin,
    decided, actions (the conditions asserted), and M with ``mags``."""
    key = (S, n, kind)
    if key not in _CACHE:
        pQ, pP, states = draw(ref, S, n, kind)
        Q0 = forward64(ref, pQ, states)
        pC = centred(pQ, Q0)
        Qc = centred_q(pQ, pC, Q0)
        dec, acts = conditions(Q0, Qc)
        _CACHE[key] = dict(pQ=pQ, pP=pP, states=states, Q0=Q0, pC=pC, Qc=Qc, margin=margin(Q0),
                           decided=dec, actions=acts)
    c = _CACHE[key]
    if mags and "M" not in c:
        c["M"] = oracle_q(ref, c["pQ"], c["states"], c["pP"])[1]
    return c


# ---- the checks ------------------------------------------------------------------
def make_net(ddq, B, S, pQ, mode="gpu"):
    net = ddq.DeepQNet(batch=B, frame=S, mode=mode)
    net.set_params(pQ)
    return net


def q_out(net):
    return net.blob("Q_out").reshape(net.batch, 4)


def check_values(q, Q0, M, what="", quiet=False):
    """A Q_out against the oracle's: _parity.close's three rules."""
    q = np.asarray(q)
    assert q.shape == Q0.shape, (what, q.shape, Q0.shape)
    close(q, Q0, what=what + "Q_out", mag=M, tensor="Q_out", quiet=quiet)
    return float(np.linalg.norm((f64(q) - Q0).ravel()) / np.linalg.norm(Q0.ravel()))


def first_max(q):
    """argmax_kernel restated: the first maximum of each row."""
    return np.argmax(np.asarray(q), axis=1).astype(np.int32)


def check_decided(actions, c, what=""):
    """Rule b.3: every decided state's action is the oracle's."""
    a = np.asarray(actions)
    assert a.shape == c["actions"].shape, (what, a.shape)
    bad = np.flatnonzero(c["decided"] & (a != c["actions"]))
    assert bad.size == 0, "%s%d decided states off the oracle's action, first %d: got %d want %d" % (
        what, bad.size, bad[0], a[bad[0]], c["actions"][bad[0]])


def forward_values(net, c, what=""):
    """2a on a ctx of batch n: write the states, forward_q, check Q_out."""
    net.write_minibatch(state=c["states"])
    net.forward_q()
    return check_values(q_out(net), c["Q0"], c["M"], what=what)


def check_actions(ddq, c, S, B, mode="gpu", what=""):
    """2b: the n states of a case on a ctx of batch n and on a ctx of batch B
    whose acting scratch holds another batch, both under the centred
    parameters.  In order: the n-ctx's actions are the first maxima of its own
    Q_out, exactly; the B-ctx's actions equal the n-ctx's, exactly (every grid
    of the acting forward comes from n); every decided state's action is the
    oracle's.  Returns the actions."""
    states = c["states"]
    n = states.shape[0]
    small, big = make_net(ddq, n, S, c["pC"], mode), make_net(ddq, B, S, c["pC"], mode)
    try:
        small.write_minibatch(state=states)
        small.forward_q()
        q = q_out(small)
        a_n = small.select_action(states)
        np.testing.assert_array_equal(a_n, first_max(q), err_msg=what + "argmax of own Q_out")
        big.select_action(other_states(S, B, n))
        a_b = big.select_action(states)
        np.testing.assert_array_equal(a_b, a_n, err_msg=what + "n states on the batch-%d ctx" % B)
        check_decided(a_b, c, what)
    finally:
        small.close()
        big.close()
    return a_b


def tied_params(c):
    """pQ with Q_out's row 0 copied into row 2 and both biases raised equally
    until that pair is the oracle's maximum, by more than the margin, for about
    half the states.  Returns (params, mask of the states the pair wins)."""
    pQ, Q0 = c["pQ"], c["Q0"]
    out = {k: [w.copy() for w in v] for k, v in pQ.items()}
    W5, b5 = out["Q_out"][0].reshape(4, -1), out["Q_out"][1]    # (views)
    W5[2] = W5[0]
    need = np.maximum(Q0[:, 1], Q0[:, 3]) - Q0[:, 0]       # the raise at which state b ties
    lift = np.float32(np.median(need) + 4 * c["margin"])
    b5 = b5.reshape(-1)
    b5[0] = b5[0] + lift
    b5[2] = b5[0]
    out["Q_out"][1] = b5.reshape(out["Q_out"][1].shape)
    Qt = Q0.copy()
    Qt[:, 0] = Q0[:, 0] + (float(b5[0]) - float(pQ["Q_out"][1].reshape(-1)[0]))
    Qt[:, 2] = Qt[:, 0]
    wins = (Qt[:, 0] - np.maximum(Qt[:, 1], Qt[:, 3])) > c["margin"]
    return out, wins


def check_ties(ddq, c, S, mode="gpu"):
    """2c: at an exact tie the first maximum wins."""
    states = c["states"]
    n = states.shape[0]
    pT, wins = tied_params(c)
    assert wins.sum() >= 1, "no state has the tied pair on top"
    net = make_net(ddq, n, S, pT, mode)
    try:
        net.write_minibatch(state=states)
        net.forward_q()
        q = q_out(net)
        np.testing.assert_array_equal(q[:, 0].view(np.uint32), q[:, 2].view(np.uint32))
        a = net.select_action(states)
        np.testing.assert_array_equal(a, first_max(q))
        assert not (a == 2).any(), a
        np.testing.assert_array_equal(a[wins], 0)
        zero = {k: [w.copy() for w in v] for k, v in c["pQ"].items()}
        zero["Q_out"] = [np.zeros_like(w) for w in zero["Q_out"]]
        net.set_params(zero)
        np.testing.assert_array_equal(net.select_action(states), 0)
    finally:
        net.close()
    return int(wins.sum())


def check_mutations(q, c, actions=None):
    """2e: the harness on an output it accepts.  Two rows swapped, one row
    scaled by 1.001, one row zeroed: each is rejected by the value check; the
    actions of two decided states whose oracle actions differ, swapped, are
    rejected by rule b.3.  Returns the number of rejections."""
    import pytest
    Q0, M = c["Q0"], c["M"]
    q = np.array(q, np.float32).reshape(Q0.shape)
    check_values(q, Q0, M, quiet=True)
    i = int(np.argmax(np.linalg.norm(Q0, axis=1)))
    j = int(np.argmax(np.linalg.norm(Q0 - Q0[i], axis=1)))
    assert i != j
    rejected = 0
    for label in ("swapped", "x1.001", "zeroed"):
        bad = q.copy()
        if label == "swapped":
            bad[[i, j]] = bad[[j, i]]
        elif label == "x1.001":
            bad[i] *= np.float32(1.001)
        else:
            bad[i] = 0
        with pytest.raises(AssertionError):
            check_values(bad, Q0, M, what=label + " ", quiet=True)
        rejected += 1
    if actions is not None:
        a = np.array(actions)
        check_decided(a, c)
        dec = np.flatnonzero(c["decided"])
        k = dec[0]
        others = dec[c["actions"][dec] != c["actions"][k]]
        assert others.size, "every decided state has one oracle action"
        bad = a.copy()
        bad[[k, others[0]]] = bad[[others[0], k]]
        with pytest.raises(AssertionError):
            check_decided(bad, c)
        rejected += 1
    return rejected
