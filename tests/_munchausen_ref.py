"""Float64 reference of the Munchausen / soft-Q target (ddq_set_munchausen): the
head formulas of include/ddq_hip.h on given P_out, Pc_out, action, r and nt.

The towers are oracle/ref_numpy.py's, the cases tests/_objective_ref.py's draws
and the bounds tests/_parity.py's, all unchanged.  The gradients come from the
oracle's own backward pass on the substituted minibatch (reward := Q_sa - d,
non_terminal := 0: its plain Euclidean diff is then d), as for the selectable
objective.
"""
import numpy as np

import _objective_ref as objr
from _parity import close, full_pass_gpu_routing

f64 = objr.f64

# (S, B, seed): the small path with one and two image chunks; the general
# kernels at an odd-map frame
CASES = [(16, 4, 901), (16, 40, 910), (24, 3, 901)]
# tau of the order of the x3 fillers' P gaps, so the soft value is no hard max;
# l0 inside the range tau ln pi takes over each case's images (the ring's uniform
# frames spread P(s,.) further than the draws' sparse ones), so the clip is
# active for some images only.  Keyed by case()'s ``drawn``.
CFG = {False: dict(tau=2.0, clip=-2.0), True: dict(tau=2.0, clip=-6.3)}
_CACHE = {}


def lse(v, tau):
    m = v.max(axis=1)
    return m, np.log(np.exp((v - m[:, None]) / tau).sum(axis=1))


def head(P, Pc, act, r, nt, gamma, alpha, tau, clip):
    """P_sa, bonus and target (and the sum of |terms| of each) from P(s',.),
    P(s,.), the one-hot, r and nt.  Pc is not read when alpha == 0."""
    P, act, r, nt = f64(P), f64(act).reshape(-1, 4), f64(r).reshape(-1), f64(nt).reshape(-1)
    m, l = lse(P, tau)
    v = m + tau * l
    out = dict(m=m, V=v, P_sa=v * nt, mag_P_sa=(np.abs(m) + tau * l) * nt,
               bonus=np.zeros_like(r), mag_bonus=np.zeros_like(r), tlp=np.zeros_like(r))
    if alpha != 0:
        Pc = f64(Pc)
        mc, lc = lse(Pc, tau)
        pa = Pc[np.arange(len(r)), act.argmax(axis=1)]
        out["tlp"] = tau * ((pa - mc) / tau - lc)
        out["bonus"] = alpha * np.minimum(np.maximum(out["tlp"], clip), 0.0)
        out["mag_bonus"] = np.where(out["tlp"] > clip, alpha * (np.abs(pa) + np.abs(mc) + tau * lc),
                                    alpha * abs(clip))
    out["target"] = gamma * out["P_sa"] + (r + out["bonus"])
    out["mag_target"] = gamma * out["mag_P_sa"] + np.abs(r) + out["mag_bonus"]
    return out


RING_N, STEP_SEED = 64, 11


def ring_for(S):
    """The ring of the step-mode cases: tests/_nstep_ref.py's, every seventh slot terminal."""
    import _nstep_ref as nr
    return nr.build_ring(np.random.default_rng(5), RING_N, S, terminals=range(2, RING_N, 7))


def case(ref, S, B, seed, drawn=False):
    """A case's parameters, minibatch and float64 towers Q(s,.), P(s',.), P(s,.):
    computed once, shared and left unchanged.  The minibatch is the draw's own
    with image 0 made terminal, or (drawn) what the first device draw of
    STEP_SEED gathers from ring_for(S), by tests/_nstep_ref.py's restatement."""
    key = (S, B, seed, drawn)
    if key not in _CACHE:
        pQ, pP, mb = objr.draw(ref, S, B, seed)
        mb[4][0] = 0.0
        if drawn:
            import _nstep_ref as nr
            idx = nr.draw(STEP_SEED, 0, B, 0, RING_N, 1, RING_N, 1)
            mb = nr.gather(ring_for(S), idx, RING_N, 1)
        p64 = lambda p: {k: [f64(w) for w in v] for k, v in p.items()}
        fwd = lambda x, p, z: ref.net_forward(f64(x), p64(p), z)["out"]
        _CACHE[key] = dict(pQ=pQ, pP=pP, mb=mb, cfg=CFG[drawn], Q=fwd(mb[0], pQ, "Q"), P=fwd(mb[3], pP, "P"),
                           Pc=fwd(mb[0], pP, "P"))
    return _CACHE[key]


def oracle_head(ref, c, alpha):
    """The whole head on the oracle's own towers, with the conditions the case
    has to meet on the reference alone (alpha != 0: the clip ones too)."""
    _, act, rw, _, nt = c["mb"]
    tau, clip = c["cfg"]["tau"], c["cfg"]["clip"]
    h = head(c["P"], c["Pc"], act, rw, nt, ref.GAMMA, alpha, tau, clip)
    B = len(h["V"])
    assert (f64(nt).reshape(-1) == 0).any()
    soft = h["V"] - h["m"] > 1e-3 * np.abs(h["m"])
    assert 2 * soft.sum() >= B, ("the soft value is the hard max in disguise", int(soft.sum()), B)
    if alpha != 0:
        on = h["tlp"] < clip
        assert on.any() and (~on).any(), ("clip active / inactive", int(on.sum()), B)
        # no clip decision within fp32 rounding of l0
        assert np.min(np.abs(h["tlp"] - clip)) >= 1e-3 * abs(clip)
    h["Q_sa"] = (c["Q"] * f64(act).reshape(B, 4)).sum(axis=1)
    return h


def check_head(net, mb, gamma, alpha, tau, clip, diff=True, what=""):
    """P_sa, m_bonus, target_Q_sa and (diff: under the Euclidean, unweighted
    loss) Q_out.diff of the net's last pass on minibatch mb against the
    reference evaluated on the net's own P_out / Pc_out, under _parity.close
    with mag the sum of |terms| of each.  Returns the reference head."""
    B = net.batch
    _, act, rw, _, nt = mb
    got = objr.blobs_of(net)
    pc = net.blob("Pc_out").reshape(B, 4) if alpha != 0 else None
    h = head(got["P_out"], pc, act, rw, nt, gamma, alpha, tau, clip)
    close(got["P_sa"], h["P_sa"], what=what + "P_sa", mag=h["mag_P_sa"], tensor="P_sa")
    bonus = net.blob("m_bonus").reshape(B)
    if alpha != 0:
        close(bonus, h["bonus"], what=what + "m_bonus", mag=h["mag_bonus"], tensor="m_bonus")
    else:
        assert not bonus.any()
    close(got["target_Q_sa"], h["target"], what=what + "target_Q_sa", mag=h["mag_target"],
          tensor="target_Q_sa")
    a = f64(act).reshape(B, 4)
    d = f64(got["Q_sa"]) - h["target"]
    if diff:
        close(got["Q_out.diff"], a * (d / B)[:, None], what=what + "Q_out.diff",
              mag=a * ((np.abs(f64(got["Q_sa"])) + h["mag_target"]) / B)[:, None],
              tensor="Q_out.diff")
    h["d"], h["Q_sa"] = d, f64(got["Q_sa"])
    return h


def check_grads(ref, net, c, d, what=""):
    """Every gradient tensor of the net's last pass against the oracle's
    backward from dQ = act d / B (the substituted pass), under the full-pass
    rules of _parity.close."""
    pQ, pP = c["pQ"], c["pP"]
    q_sa = (c["Q"] * f64(c["mb"][1]).reshape(-1, 4)).sum(axis=1)   # the oracle's own Q_sa
    sub = objr.substituted(c["mb"], dict(B=len(d), Q_sa=q_sa, d_c=d))
    _, grads, nties, h4_mask = full_pass_gpu_routing(ref, net, pQ, pP, sub, with_mask=True)
    routes = {i: net.pool_mask(i) for i in (1, 2, 3)}
    _, mgrads = ref.magnitudes(pQ, pP, *sub, routes=routes, h4_mask=h4_mask)
    g = net.split(net.get_grads_flat(), "Q")
    for name in grads:
        for i in range(2):
            key = "%s[%d]" % (name, i)
            close(g[name][i], grads[name][i], what=what + key, mag=mgrads[name][i], tensor=key)
    return nties
