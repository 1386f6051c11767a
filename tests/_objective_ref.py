"""Float64 oracle of the selectable TD objective (ddq_set_objective), built on
the unmodified oracle (oracle/ref_numpy.py).

The backward pass is linear in dQ.  ``oracle`` computes Q, Qn = Q-net(s'), P,
the Double-DQN action a*, the objective's target, d = Q_sa - target and the
clamped d_c in float64 with ``ref.net_forward``; ``substituted`` then builds a
minibatch with reward := Q_sa - d_c and non_terminal := 0, on which the
oracle's plain Euclidean ``diff`` is d_c -- so ``ref.full_pass`` /
``ref.magnitudes`` on it give the objective's gradients and their |terms|.
Comparisons use tests/_parity.py's rules with their constants unchanged.

Inputs: ``rng = default_rng(seed)``, then the parameters, then the inputs, drawn
as test_gpu_parity.make_params(ref, rng, S, "x3") and make_inputs(rng, B, S,
"snake") draw them.
"""
import numpy as np

from _parity import close, floor_count, full_pass_gpu_routing

# (S, B, seed): K2 with one tower per workgroup; K2 with two towers and a ragged
# second chunk; the smallest group split; the general kernels with partial
# tiles; the 64x64 tilings
CASES = [(16, 32, 910), (16, 40, 910), (16, 2, 901), (24, 8, 901), (64, 4, 900)]
CPU_CASES = [(16, 32, 910), (24, 8, 901)]

_CACHE = {}


def f64(a):
    return np.asarray(a, np.float64)


def draw(ref, S, B, seed):
    """(pQ, pP, mb) of a case."""
    from test_gpu_parity import make_inputs, make_params
    rng = np.random.default_rng(seed)
    pQ, pP = make_params(ref, rng, S, "x3")
    mb = make_inputs(rng, B, S, "snake")
    return pQ, pP, mb


def huber(d, delta):
    a = np.abs(d)
    return np.where(a <= delta, d * d / 2.0, delta * (a - delta / 2.0))


def oracle(ref, pQ, pP, mb, target="double", loss="huber", delta=None):
    """The objective's head in float64.  delta None (Huber): the midpoint of the
    two middle values of |d|, so half the images are clipped."""
    st, act, rw, ns, nt = mb
    B = np.asarray(st).shape[0]
    p64 = lambda p: {k: [f64(w) for w in v] for k, v in p.items()}
    Q = ref.net_forward(f64(st), p64(pQ), "Q")["out"]
    Qn = ref.net_forward(f64(ns), p64(pQ), "Q")["out"]
    P = ref.net_forward(f64(ns), p64(pP), "P")["out"]
    a = f64(act).reshape(B, 4)
    r, n = f64(rw).reshape(B), f64(nt).reshape(B)
    astar = Qn.argmax(axis=1)                       # first maximum
    p_pick = P[np.arange(B), astar] if target == "double" else P.max(axis=1)
    p_sa = p_pick * n
    tgt = ref.GAMMA * p_sa + r
    q_sa = (Q * a).sum(axis=1)
    d = q_sa - tgt
    if loss == "huber":
        if delta is None:
            s = np.sort(np.abs(d))
            delta = 0.5 * (s[(B - 1) // 2] + s[B // 2])
        d_c = np.clip(d, -delta, delta)
        lv = float(huber(d, delta).sum() / B)
    else:
        delta, d_c = None, d
        lv = float(d @ d) / B / 2.0
    return dict(Q=Q, Qn=Qn, P=P, astar=astar, P_sa=p_sa, target=tgt, Q_sa=q_sa, d=d, d_c=d_c,
                delta=delta, loss=lv, act=a, r=r, nt=n, B=B)


def assert_well_separated(o):
    """The oracle's decisions are far from fp32 rounding: the fp32 argmax and
    every clip decision must then agree with it outright (no near-tie rule)."""
    B = o["B"]
    top = np.sort(o["Qn"], axis=1)
    gap = float(np.min(top[:, -1] - top[:, -2]) / np.max(np.abs(o["Qn"])))
    assert gap >= 1e-2, ("Qn top-two gap", gap)
    differs = (o["nt"] == 1) & (np.abs(o["P"][np.arange(B), o["astar"]] - o["P"].max(axis=1))
                                > 1e-3 * np.max(np.abs(o["P"])))
    need = max(1, B // 4)
    assert differs.sum() >= need and (~differs).sum() >= need, (int(differs.sum()), B)
    sep = float(np.min(np.abs(np.abs(o["d"]) - o["delta"])) / o["delta"])
    assert sep >= 1e-3, ("|d| - delta separation", sep)
    return gap, sep


def case(ref, S, B, seed):
    """A case's parameters, minibatch and {DOUBLE, HUBER} oracle: computed once,
    shared by the tests and left unchanged."""
    key = (S, B, seed)
    if key not in _CACHE:
        pQ, pP, mb = draw(ref, S, B, seed)
        o = oracle(ref, pQ, pP, mb, "double", "huber")
        gap, sep = assert_well_separated(o)
        print("case %s: Qn gap %.3g of max|Qn|, |d| / delta separation %.3g, delta %.6g"
              % (key, gap, sep, o["delta"]))
        _CACHE[key] = dict(pQ=pQ, pP=pP, mb=mb, o=o)
    return _CACHE[key]


def substituted(mb, o):
    """The minibatch on which the oracle's plain diff is the objective's d_c."""
    st, act, rw, ns, nt = mb
    B = o["B"]
    return (st, act, (o["Q_sa"] - o["d_c"]).reshape(B, 1, 1, 1), ns,
            np.zeros((B, 1, 1, 1), np.float64))


def make_net(ddq, c, mode="gpu"):
    st = c["mb"][0]
    net = ddq.DeepQNet(batch=st.shape[0], frame=st.shape[2], mode=mode)
    params = dict(c["pQ"])
    params.update(c["pP"])
    net.set_params(params)
    net.write_minibatch(*c["mb"])
    return net


def blobs_of(net, names=("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss", "Q_out.diff")):
    B = net.batch
    return {k: net.blob(k).reshape(B, 4) if k in ("Q_out", "P_out", "Qn_out", "Q_out.diff")
            else net.blob(k).reshape(-1) for k in names}


def check_objective_pass(ref, net, c, o, what=""):
    """The net's last pass under the objective of ``o`` against the substituted
    oracle pass: Q_out, P_out, Qn_out, the head's blobs and every gradient
    tensor, _parity.close's three rules (|terms|, normwise, floored elementwise).
    The fp32 argmax and clip decisions must equal the oracle's.  Returns
    {tensor: count of elements >= 1e-2 of its max, held to rtol 1e-4}."""
    pQ, pP, mb = c["pQ"], c["pP"], c["mb"]
    B = o["B"]
    sub = substituted(mb, o)
    blobs, grads, nties, h4_mask = full_pass_gpu_routing(ref, net, pQ, pP, sub, with_mask=True)
    routes = {i: net.pool_mask(i) for i in (1, 2, 3)}
    mblobs, mgrads = ref.magnitudes(pQ, pP, *sub, routes=routes, h4_mask=h4_mask)
    got = blobs_of(net)
    for name in ("Q_out", "P_out"):
        close(got[name], blobs[name], what=what + name, mag=mblobs[name], tensor=name)
    mP = mblobs["P_out"]
    if net.objective()["target"] == "double":
        mQn = ref.magnitudes(pQ, pP, mb[3], mb[1], mb[2], mb[3], mb[4])[0]["Q_out"]
        qn = net.blob("Qn_out").reshape(B, 4)
        close(qn, o["Qn"], what=what + "Qn_out", mag=mQn, tensor="Qn_out")
        # every image's argmax agrees outright (first maximum)
        np.testing.assert_array_equal(np.argmax(qn, axis=1), o["astar"])
        m_psa = mP[np.arange(B), o["astar"]] * o["nt"]
    else:
        m_psa = mP[np.arange(B), o["P"].argmax(axis=1)] * o["nt"]
    m_tgt = ref.GAMMA * m_psa + np.abs(o["r"])
    m_diff = mblobs["Q_sa"] + m_tgt
    close(got["Q_sa"], o["Q_sa"], what=what + "Q_sa", mag=mblobs["Q_sa"], tensor="Q_sa")
    close(got["P_sa"], o["P_sa"], what=what + "P_sa", mag=m_psa, tensor="P_sa")
    close(got["target_Q_sa"], o["target"], what=what + "target_Q_sa", mag=m_tgt,
          tensor="target_Q_sa")
    # every clip decision agrees outright
    d32 = f64(got["Q_sa"]) - f64(got["target_Q_sa"])
    if o["delta"] is not None:
        np.testing.assert_array_equal(np.abs(d32) > o["delta"], np.abs(o["d"]) > o["delta"])
    close(got["Q_out.diff"], o["act"] * (o["d_c"] / B)[:, None], what=what + "Q_out.diff",
          mag=o["act"] * (m_diff / B)[:, None], tensor="Q_out.diff")
    close(float(got["loss"][0]), o["loss"], what=what + "loss",
          mag=float((np.abs(o["d_c"]) * m_diff).sum() / B), tensor="loss")
    counts = {}
    g = net.split(net.get_grads_flat(), "Q")
    for name in grads:
        for i in range(2):
            key = "%s[%d]" % (name, i)
            close(g[name][i], grads[name][i], what=what + key, mag=mgrads[name][i], tensor=key)
            counts[key] = floor_count(grads[name][i])
    print("%snear-tie routings adopted: %d" % (what, nties))
    return counts


def expected_head_f32(got, act, nt, r, gamma, target, delta):
    """The head's blobs recomputed from the net's own blobs: P_sa and dQ in
    np.float32 (what the fp32 head computes, operation for operation), the
    target and the loss in float64."""
    B = act.shape[0]
    P, Q_sa, tq = got["P_out"], got["Q_sa"], got["target_Q_sa"]
    if target == "double":
        qn = got["Qn_out"]
        best = np.zeros(B, np.int64)
        for a in range(1, 4):                       # argmax_kernel: first max wins
            best = np.where(qn[np.arange(B), a] > qn[np.arange(B), best], a, best)
        pick = P[np.arange(B), best]
    else:
        pick = P.max(axis=1)
    p_sa = (pick.astype(np.float32) * nt.astype(np.float32)).astype(np.float32)
    tgt64 = float(np.float32(gamma)) * f64(got["P_sa"]) + f64(r)
    d = (Q_sa.astype(np.float32) - tq.astype(np.float32)).astype(np.float32)
    if delta is None:
        dc, lv = d, float((f64(d) ** 2).sum() / B / 2.0)
    else:
        dl = np.float32(delta)
        dc = np.minimum(np.maximum(d, -dl), dl).astype(np.float32)
        lv = float(huber(f64(d), float(dl)).sum() / B)
    dq = ((act.astype(np.float32) * dc[:, None]).astype(np.float32) / np.float32(B)).astype(np.float32)
    return dict(P_sa=p_sa, target64=tgt64, d=d, dQ=dq, loss=lv)
