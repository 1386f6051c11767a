"""The coherence probe: does a context multiply by what its parameters say?

The step kernels never read theta.  They read copies derived from it: the split
[co][tap][ci] bf16 planes of the conv weights (wks[0] for Q, wks[1] for P), the
transposed data-gradient layouts rebuilt from them, the target tower's thetaP /
wksP written on a P <- Q sync, the pipelined mode's second buffer set and the
async exchange's mirror of a shard.  Many launches keep them up to date
("Derived copies and who writes them").  ``get_flat`` reads
theta, so a chain compared through it cannot see a stale copy.

``probe`` can: it gives a fresh context the net's two towers through
``set_flat`` (one relayout launch writes every copy from theta), binds one
minibatch to both, and runs ``forward_backward`` and ``select_action`` on both.
Both run the same deterministic kernels on the same inputs, so every blob, every
gradient tensor, every pool mask and every action is compared byte for byte: a
difference means the net multiplied by something that is not split3(theta).

tests/test_gpu_coherence.py runs it after every update site of the step plan;
tests/test_coherence.py runs the same harness on the CPU twin, which keeps no
copies: a check of the harness itself.
"""
import collections

import numpy as np

PERIOD = 3                 # target_period of every regime
PROBES = (2, 3, 4)         # updates before a probe: before the first sync, right after it, P lagging
N = 256                    # ring slots
# rmsprop's lr.  One update must change the bf16 high term of some weight in
# every conv blob (check_regime asserts it), and 3e-4 does.  1e-3 does too, but
# its lagged cache then throws single weights by 3e-2 within three updates and
# a third of conv3's channels die: a dead channel's weights reach no output, so
# neither a stale copy of them nor a mutant in them can be seen by any probe.
LR = 3e-4
CONV = ("Qconv1", "Qconv2", "Qconv3")
BLOBS = ("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss")
_RINGS = {}


def theta0(S, seed=42):
    from ddq.params import init_params_flat
    return init_params_flat(S, seed=seed)


def ring(S, n=N, seed=0):
    """n transitions of random-policy Snake as replay_import takes them."""
    if (S, n, seed) not in _RINGS:
        from ddq.expgain import synthetic_transitions
        st, ac, rw, nt = synthetic_transitions(n, S, seed=seed)
        _RINGS[(S, n, seed)] = (st, ac, rw, np.asarray(nt, np.uint8))
    return _RINGS[(S, n, seed)]


def ring_slots(B):
    """N, or the next multiple of N that leaves a B-draw room beside the slots
    around the write head that no draw may take (B = 257 needs more than 256)."""
    return N if B + 8 <= N else -(-(B + 8) // N) * N


def make_net(ddq, S, B, mode="gpu", ring_seed=0, theta_p=None):
    """A context holding theta0 in both towers (theta_p: another P tower) on a
    filled ring."""
    net = ddq.DeepQNet(batch=B, frame=S, mode=mode)
    th = theta0(S)
    net.set_flat(0, th)
    net.set_flat(1, th if theta_p is None else theta_p)
    n = ring_slots(B)
    net.replay_create(n)
    net.replay_import(*ring(S, n, ring_seed), 0, n)
    return net


def probe_inputs(B, S, seed=0):
    """(mb, states_u8).  Frames: uniform in [0, 256) as tests/test_cpu_twin.py's
    make_inputs(..., "uniform") draws them, every other sample dense -- every
    conv1 weight then meets a non-zero pixel -- and the rest under random masks
    that keep 1/2, 1/4 or 1/8 of the pixels: a conv channel whose weights sum
    below zero is dead at every position of a dense uniform frame whatever the
    seed, and its weights reach the output only where few pixels are lit.
    non_terminal flags of both kinds, so that P_out reaches target_Q_sa in some
    samples and the reward alone does in others."""
    rng = np.random.default_rng(1000 + seed)

    def frames():
        x = rng.integers(0, 256, (B, 4, S, S)).astype(np.float32)
        for b in range(1, B, 2):
            x[b] *= rng.random((4, S, S)) < 0.5 ** (1 + (b // 2) % 3)
        return x
    st, ns = frames(), frames()
    act = np.zeros((B, 4, 1, 1), np.float32)
    act[np.arange(B), rng.integers(0, 4, B)] = 1
    rw = rng.integers(-1, 2, (B, 1, 1, 1)).astype(np.float32)
    nt = (rng.random((B, 1, 1, 1)) > 0.2).astype(np.float32)
    nt.ravel()[0], nt.ravel()[B - 1] = 1.0, 0.0
    states = frames().astype(np.uint8)
    return (st, act, rw, ns, nt), states


def read(net, mb, states_u8):
    """Bind mb, run forward_backward and select_action; every compared tensor
    by name, in a fixed order."""
    net.synchronize()
    net.write_minibatch(*mb)
    net.forward_backward()
    out = collections.OrderedDict()
    names = BLOBS + (("Qn_out",) if net.objective()["target"] == "double" else ())
    for name in names:
        out[name] = net.blob(name)
    for lname, blobs in net.split(net.get_grads_flat()).items():
        out["grad " + lname + ".W"], out["grad " + lname + ".b"] = blobs
    for layer in (1, 2, 3):
        out["pool_mask%d" % layer] = net.pool_mask(layer)
    out["actions"] = net.select_action(states_u8)
    return out


def fresh_like(ddq, net, q=None, p=None):
    """A new context of the net's batch, frame, mode and objective holding the
    towers q and p (default: the net's own)."""
    fresh = ddq.DeepQNet(batch=net.batch, frame=net.frame, mode=net.mode)
    o = net.objective()
    if (o["target"], o["loss"]) != ("max", "euclidean"):
        fresh.set_objective(o["target"], o["loss"], o["huber_delta"] or 1.0)
    fresh.set_flat(0, net.get_flat(0) if q is None else q)
    fresh.set_flat(1, net.get_flat(1) if p is None else p)
    return fresh


def probe(ddq, net, mb, states_u8):
    """(got, want): the net's tensors and those of a fresh context given its
    parameters."""
    fresh = fresh_like(ddq, net)
    try:
        return read(net, mb, states_u8), read(fresh, mb, states_u8)
    finally:
        fresh.close()


def first_difference(got, want):
    """The name of the first tensor whose bytes differ (with how many elements
    do), or None."""
    for name in want:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        if a.tobytes() != b.tobytes():
            return "%s (%d of %d elements differ, max |d| %.3g)" % (
                name, int((a != b).sum()), a.size,
                float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))))
    return None


def assert_coherent(got, want, what):
    assert list(got) == list(want), what
    for name, a in got.items():
        if np.asarray(a).dtype.kind == "f":
            assert np.isfinite(a).all(), "%s: %s is not finite" % (what, name)
    d = first_difference(got, want)
    assert d is None, "%s: the context and a fresh one given its theta differ in %s" % (what, d)


def check(ddq, net, want_p, what, seed=0):
    """The probe on net, and its P tower against want_p byte for byte."""
    p = net.get_flat(1)
    assert np.isfinite(p).all() and np.isfinite(net.get_flat(0)).all(), what + ": theta"
    assert p.tobytes() == np.asarray(want_p, np.float32).tobytes(), \
        "%s: tower 1 is not the expected one (%d elements differ)" % (what, int((p != want_p).sum()))
    mb, states = probe_inputs(net.batch, net.frame, seed)
    got, want = probe(ddq, net, mb, states)
    assert_coherent(got, want, what)


def stuck_high_terms(net, before, after):
    """The conv blobs in which the update before -> after changed no weight's
    bf16 high term (the upper 16 bits).  A regime's lr is large enough when there
    is none: a plane left stale then differs from a fresh one in its first
    term."""
    hi = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16  # noqa: E731
    a, b = net.split(before), net.split(after)
    return [name for name in CONV if not (hi(a[name][0]) != hi(b[name][0])).any()]


# ---------------------------------------------------------------- regimes
_STATES = {}


def states_after(key, run, k):
    """[(theta Q, theta P) per member] after k updates of regime `key`; the runs
    are deterministic, so a probe point may take an earlier one's towers."""
    if (key, k) not in _STATES:
        nets = run(k)
        try:
            _STATES[(key, k)] = [(n.get_flat(0), n.get_flat(1)) for n in nets]
        finally:
            close_all(nets)
    return _STATES[(key, k)]


def close_all(nets):
    for n in nets:
        n.synchronize()
        n.close()


def check_regime(ddq, key, run, k, p_fixed=None, lr_check=True):
    """run(k) -> the regime's contexts after k updates, each probed.  Tower 1
    must be the initial theta at 2 updates, tower 0 at 3 (the sync has just run)
    and the 3-update run's tower 0 at 4 (p_fixed: the regime never syncs, tower
    1 stays p_fixed)."""
    nets = run(k)
    try:
        _STATES[(key, k)] = [(n.get_flat(0), n.get_flat(1)) for n in nets]
        for r, net in enumerate(nets):
            what = "%s, %d updates, member %d" % (key, k, r)
            if p_fixed is not None:
                want_p = p_fixed
            elif k == 2:
                want_p = theta0(net.frame)
            elif k == 3:
                want_p = net.get_flat(0)
            else:
                want_p = states_after(key, run, 3)[r][0]
            q = net.get_flat(0)
            if lr_check and k > PROBES[0]:      # (the earlier probe point's run is at hand)
                prev = states_after(key, run, k - 1)[r][0]
                assert stuck_high_terms(net, prev, q) == [], what + ": lr too small for the probe"
            if p_fixed is None and k == 4:
                assert want_p.tobytes() != q.tobytes(), what + ": P does not lag"
            check(ddq, net, want_p, what)
    finally:
        close_all(nets)


def random_grad(rng, n):
    return rng.normal(0, 1e-2, n).astype(np.float32)


APPLY_RULES = ("sgd", "rmsprop", "adagrad", "momentum", "adam", "adam-clip")


def run_apply(ddq, S, B, rule, k, mode="gpu"):
    """k separate apply launches of random gradients.  The P tower starts from
    another initialisation: ddq_apply carries no target period, so P and its
    layouts must stay exactly that."""
    net = make_net(ddq, S, B, mode, theta_p=theta0(S, seed=43))
    if rule.startswith("adam"):
        net.set_adam(max_grad_norm=0.5 if rule == "adam-clip" else 0.0)   # |g| is about 1e-2 sqrt(P) > 1
    rng = np.random.default_rng(7)
    for _ in range(k):
        net.set_grads_flat(random_grad(rng, net.num_params))
        net.apply(rule.split("-")[0], lr=1e-2 if rule == "momentum" else 1e-3)   # (the twin's rule tests' rates)
    return [net]


def run_host_loop(ddq, S, B, k, mode="gpu", objective=None, rule="rmsprop", lr=LR):
    """k updates driven from the host, as the param server's worker does them:
    a host-drawn index set, forward_backward, apply, and sync_target() after
    every PERIOD-th."""
    net = make_net(ddq, S, B, mode)
    if objective:
        net.set_objective(*objective)
    rng = np.random.default_rng(5)
    for t in range(1, k + 1):
        net.replay_sample(np.sort(rng.choice(np.arange(8, N - 8), B, replace=False)).astype(np.int32))
        net.forward_backward()
        net.apply(rule, lr=lr)
        if t % PERIOD == 0:
            net.sync_target()
    return [net]


HOST_PATHS = ("set_flat0", "set_flat1", "sync_target", "set_params")


def check_host_path(ddq, net, path, what):
    """A trained net (P lagging Q) through one host path: the probe must be
    coherent and tower 1 exactly what the path says."""
    S = net.frame
    a, b = theta0(S, seed=44), theta0(S, seed=45)
    q, p = net.get_flat(0), net.get_flat(1)
    assert q.tobytes() != p.tobytes(), what
    if path == "set_flat0":          # P's copies untouched
        net.set_flat(0, a)
        want_q, want_p = a, p
    elif path == "set_flat1":
        net.set_flat(1, b)
        want_q, want_p = q, b
    elif path == "sync_target":
        net.sync_target()
        want_q, want_p = q, q
    else:
        params = net.split(a, "Q")
        params.update(net.split(b, "P"))
        net.set_params(params)
        want_q, want_p = a, b
    assert net.get_flat(0).tobytes() == want_q.tobytes(), what + ": tower 0"
    check(ddq, net, want_p, what)


# ---------------------------------------------------------------- mutants
def conv_slice(net, name):
    (shape, off, cnt) = net.layout[name][0]
    return off, cnt


def mutants(net, q, p, q_prev, p_prev):
    """The towers (q, p) with one conv weight put back to what it was one update
    (P: one sync) earlier: [(id, q', p')].  Six single elements -- the one of
    largest |delta| in each conv blob of each tower, the first such on a tie --
    and, per tower, the float4 group of conv3's last four weights, where
    refresh_kernel's early return of a step without a sync cuts."""
    out = []
    for t, (cur, prev) in enumerate(((q, q_prev), (p, p_prev))):
        for name in CONV:
            off, cnt = conv_slice(net, name)
            d = np.abs(cur[off:off + cnt].astype(np.float64) - prev[off:off + cnt])
            assert d.max() > 0, "%s of tower %d did not move" % (name, t)
            picks = [("one", [off + int(np.argmax(d))])]
            if name == "Qconv3":
                tail = list(range(off + cnt - 4, off + cnt))
                # (a weight whose gradient is exactly zero does not move: one of
                # the four moving is what makes the group a mutant)
                assert (off + cnt) % 4 == 0 and d[-4:].max() > 0
                picks.append(("last4", tail))
            for kind, idx in picks:
                m = cur.copy()
                m[idx] = prev[idx]
                out.append(("%s%s-%s" % ("QP"[t], name[1:], kind),
                            m if t == 0 else q, m if t == 1 else p))
    return out


def detected(ddq, net, want, mb, states_u8, q, p):
    """Does the probe tell a context holding (q, p) from the coherent one?  The
    name of the first differing tensor, or None."""
    mutant = fresh_like(ddq, net, q, p)
    try:
        return first_difference(read(mutant, mb, states_u8), want)
    finally:
        mutant.close()


def check_mutants(ddq, key, run, seed=0):
    """Every mutant of the regime's towers right after its first sync (3
    updates; one update earlier: the 2-update run's Q, and the P from before the
    sync) must be told from the coherent context by the probe."""
    q_prev, p_prev = states_after(key, run, 2)[0]
    net, = run(3)
    try:
        q, p = net.get_flat(0), net.get_flat(1)
        assert q.tobytes() == p.tobytes() and p_prev.tobytes() != p.tobytes(), key
        mb, states = probe_inputs(net.batch, net.frame, seed)
        got, want = probe(ddq, net, mb, states)
        assert_coherent(got, want, key + ", 3 updates")
        report = [(name, detected(ddq, net, want, mb, states, mq, mp))
                  for name, mq, mp in mutants(net, q, p, q_prev, p_prev)]
    finally:
        close_all([net])
    for name, d in report:
        print("mutant %-14s %s" % (name, "detected in " + d if d else "NOT DETECTED"))
    assert len(report) == 8
    missed = [name for name, d in report if d is None]
    assert not missed, "%s: the probe (seed %d) does not see the mutants %s" % (key, seed, missed)
