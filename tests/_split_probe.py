"""Exact-value probes of the split-bf16 products (csrc/split.h).

The step kernels form every convolution product from three bf16 planes per
operand, a.b ~= a0b0 + (a1b0 + a0b1 + a2b0 + a1b1 + a0b2).  The float64-oracle
bounds of tests/_parity.py are a budget for fp32 rounding and barely see one of
those six terms lost.  Here the inputs are built so that NOTHING rounds: every
product and every partial sum of the whole pass is exactly representable in
fp32.  Any correct implementation, in any accumulation order, then returns the
float64 oracle's value bit for bit, and a lost or misplaced term flips a known
bit.

Construction
------------
* One-path net.  Up to four probing images per pass, image j alone in frame
  channel j, each with ONE nonzero pixel and its own path: one tap / input
  channel / output channel per convolution, one fc4 weight, one Q_out weight,
  all four paths disjoint in every layer.  Biases 0, path values positive, so
  ReLU and max-pool are exact selections and nothing sums but zeros.
  non_terminal = 0 (target = reward); the P tower holds the Q parameters and
  next_state = state, so P_out is probed with Q_out.  The gamma passes
  (build_pass(..., gamma = 0.5), check_fused_sites) set non_terminal = 1 on a
  net created with that gamma: the target then carries gamma . max_a P_out.
* Operand shapes.  With three planes on BOTH operands the exact product also
  holds a1b2, a2b1 and a2b2, so the float64 oracle is not an fp32 number: a
  six-term kernel would differ from it by design.  The probes therefore use the
  three operand shapes whose exact product IS the sum of kept terms only, and
  which together own every kept term:
      3 x 1  a = 1 + 2^-10 + 2^-20, b a power of two   a0b0 a1b0 a2b0
      1 x 3  a a power of two, b = 1 + 2^-11 + 2^-22   a0b0 a0b1 a0b2
      2 x 2  a = 1 + 2^-10, b = 1 + 2^-11              a0b0 a1b0 a0b1 a1b1
  Each kept term owns one bit of the 24.
* Kinds (what sits on a path; everything else on it is a power of two):
      K<k>  w_k = 1 + 2^-11 + 2^-22: layer k forward 1 x 3, layer k+1.. forward
            and weight gradient 3 x 1 (the activation arrives as 1 . w_k), layer
            k data gradient 1 x 3
      P<k>  w_k = 1 + 2^-10, w_k+1 = 1 + 2^-11: layer k+1 forward 2 x 2
      D     dQ = 1 + 2^-10 + 2^-20 (times a power of two): every data gradient
            3 x 1, every weight gradient 1 x 3.  loss holds dQ^2, which is not an
            fp32 number: it is not compared for this kind
      B<k>  dQ = 1 + 2^-10, w_k = 1 + 2^-11: layer k data gradient 2 x 2, layer
            k+1 weight gradient 2 x 2 (loss again not compared)
  Layers 1..5 = conv1, conv2, conv3, fc4, Q_out.  conv1's activation operand
  is the frame: one plane by contract (include/ddq_hip.h, ddq_write_minibatch),
  so conv1 forward / weight gradient only ever have the 1 x 3 terms.
* dQ = (Q_sa - reward) / B is a true division in every implementation; the
  reward is chosen as Q_sa - B . dQ, which the builder checks is an fp32 number
  (B . dQ needs the bits of B's odd part on top of dQ's: at B = 129 and 260 no
  three-plane dQ fits 24 bits, and kind D there carries 1 + 2^-10, two planes;
  a third-plane dQ reaches those kernels' families at B = 128 and at S = 24).
"""
import collections

import numpy as np

from oracle import ref_numpy as ref

X3 = 1 + 2.0 ** -10 + 2.0 ** -20
X3C = 1 + 2.0 ** -9 + 2.0 ** -18       # the narrowest value with three planes
Y3 = 1 + 2.0 ** -11 + 2.0 ** -22
X2 = 1 + 2.0 ** -10
Y2 = 1 + 2.0 ** -11

TERMS = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))     # split.h: i + j <= 2
LAYERS = ("conv1", "conv2", "conv3", "fc4", "_out")
KINDS = (["K%d" % k for k in range(1, 6)] + ["P%d" % k for k in range(1, 5)] + ["D"]
         + ["B%d" % k for k in range(1, 6)])
BLOBS = ("Q_out", "P_out", "Q_sa", "target_Q_sa", "loss")

# the (S, B) of tests/test_gpu_split_probe.py and the kernel family each reaches
CASES = ((16, 4), (16, 40), (16, 128), (16, 129), (24, 4), (40, 2), (64, 2), (16, 260))


def exact32(x):
    x = np.asarray(x, np.float64)
    return bool(np.all(x.astype(np.float32).astype(np.float64) == x))


def bf16(x):
    """float64 -> the bf16 nearest the value's fp32, ties to even (as the
    device's (__bf16)x), returned as float64."""
    u = np.asarray(x, np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def split3(x):
    """split.h:45: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)."""
    x = np.asarray(x, np.float64)
    h = bf16(x)
    r = x - h
    m = bf16(r)
    return h, m, bf16(r - m)


def split_dot(a, b, terms=TERMS, zero_a=(), zero_b=()):
    """sum_k sum_{(i, j) in terms} a_i[k] b_j[k] in float64 (exact for probe
    operands), the planes in zero_a / zero_b cleared first; as float32."""
    pa = [p * (i not in zero_a) for i, p in enumerate(split3(np.atleast_1d(a)))]
    pb = [p * (j not in zero_b) for j, p in enumerate(split3(np.atleast_1d(b)))]
    return np.float32(sum(float(np.sum(pa[i] * pb[j])) for (i, j) in terms))


def mutants():
    """name -> kwargs of split_dot: each kept term lost, each lower plane of
    either operand lost."""
    out = collections.OrderedDict()
    for t in TERMS:
        out["no a%d*b%d" % t] = dict(terms=tuple(u for u in TERMS if u != t))
    for p in (1, 2):
        out["a plane %d zero" % p] = dict(zero_a=(p,))
        out["b plane %d zero" % p] = dict(zero_b=(p,))
    return out


def kind_values(kind, B):
    """(w[1..5] factors, dQ factor) of a kind at batch B."""
    w = [1.0] * 6
    dq = 1.0
    k = int(kind[1:]) if kind != "D" else 0
    if kind[0] == "K":
        w[k] = Y3
    elif kind[0] == "P":
        w[k], w[k + 1] = X2, Y2
    elif kind == "D":
        lead = B / 2.0 ** int(np.floor(np.log2(B)))
        dq = next(v for v in (X3, X3C, X2) if exact32(lead * v))
    else:
        dq, w[k] = X2, Y2
    return w, dq


# pixels / taps are given per frame side; centre taps are (3, 3), (2, 2), (1, 1)
def placements(S):
    """(pixel, taps of conv1 / conv2 / conv3): corners, the last pixel,
    interior, both sides of the 8- and 16-pixel seams, corner taps landing on
    corner outputs (their halo is all padding), and where S is no multiple of
    16 (24, 40, 72) a pixel of the partial edge tile."""
    C = ((3, 3), (2, 2), (1, 1))
    out = [((0, 0), C), ((S - 1, S - 1), C),
           ((3, 3), ((6, 6), (0, 0), (2, 2))),              # conv1 / conv3 output (0, 0)
           ((S - 4, S - 4), ((0, 0), (4, 4), (0, 0))),      # conv1 / conv3 output last
           ((5, 7), C), ((5, 8), C), ((9, S - 1), C), ((S - 1, 6), C),
           ((6, 10), ((0, 6), (4, 0), (1, 1)))]
    if S > 16:
        out += [((7, 15), C), ((7, 16), C), ((15, 9), C), ((16, 9), C),
                ((15, 16), ((6, 0), (2, 2), (0, 2)))]
    if S % 16:
        out += [((S - 3, S - 6), C), ((S - 6, 17), ((3, 3), (0, 0), (1, 1)))]
    if S > 32:
        out += [((31, 32), C), ((32, 31), C)]
    return out


# channels per image slot j: first, last, and one in each 8-channel half of a
# 16-channel k-group (split.h: a lane reads channels [16 g + 8 h, +8))
CH1 = (0, 11, 19, 31)
CH2 = (0, 19, 43, 63)
CH3 = (3, 27, 40, 63)
UNIT = (0, 9, 300, 511)
SCALE = ((1.0, 2.0, 0.5, 1.0, 2.0), (2.0, 0.5, 1.0, 1.0, 0.5),
         (0.5, 1.0, 2.0, 2.0, 1.0), (1.0, 1.0, 1.0, 0.5, 2.0))


def walk(S, pixel, taps):
    """Output pixel of each convolution and the pooled position after it."""
    pos, H, outs = pixel, S, []
    for (_, _, k, pad), tap in zip(ref.CONVS, taps):
        o = (pos[0] - tap[0] + pad, pos[1] - tap[1] + pad)
        assert 0 <= o[0] < H and 0 <= o[1] < H, (S, pixel, taps, o)
        outs.append(o)
        pos, H = (o[0] // 2, o[1] // 2), H // 2
    return outs, pos


def image_slots(B):
    """Which images of the batch carry probes: first, last, middle, and one in
    the second 32-image chunk when there is one."""
    cand = [0, B - 1, B // 2, 33 if B > 34 else 1]
    out = []
    for b in cand:
        if 0 <= b < B and b not in out:
            out.append(b)
    return out


Probe = collections.namedtuple("Probe", "S B kinds params neutral mb compared operands where")


def build_pass(S, B, kinds, first=0, gamma=None):
    """One pass: kinds[j] on image slot j (at most four), placement
    ``first + j`` of placements(S), channels rotated by ``first``.  Returns a
    Probe: params (Q names; the P tower takes the same), neutral (the same
    paths with every factor 1: the partner of the update / blend tests), the
    minibatch in the oracle's shapes, the compared blob names, the operand
    pairs {site: [(a, b)]} and where[j] = the path's weight indices.

    gamma (a power of two, for a net created with it): non_terminal = 1 in
    every image, so the target is reward + gamma . max_a P_out with the P tower
    holding the Q parameters; the reward is moved so that dQ stays the designed
    one.  The parameters are those of the gamma = None pass."""
    imgs = image_slots(B)
    assert len(kinds) <= len(imgs)
    pl = placements(S)
    s4 = S // 8
    shapes = ref.param_shapes(S, "Q")
    P = collections.OrderedDict((n, [np.zeros(s, np.float32) for s in sh])
                                for n, sh in shapes.items())
    N = collections.OrderedDict((n, [np.zeros(s, np.float32) for s in sh])
                                for n, sh in shapes.items())
    st = np.zeros((B, 4, S, S), np.float32)
    ac = np.zeros((B, 4, 1, 1), np.float32)
    ac[:, 0] = 1
    rw = np.zeros((B, 1, 1, 1), np.float32)
    nt = np.full((B, 1, 1, 1), 0.0 if gamma is None else 1.0, np.float32)
    operands = collections.defaultdict(list)
    where, lossy = [], False
    for j, kind in enumerate(kinds):
        pixel, taps = pl[(first + j) % len(pl)]
        r = (first + j + first // 4) % 4                    # (moves on with every fourth probe)
        f, act = j, (j + first) % 4
        c = (CH1[r], CH2[(r + 1) % 4], CH3[(r + 2) % 4])
        unit = UNIT[(r + 3) % 4]
        fac, dqf = kind_values(kind, B)
        sc = SCALE[r]
        w = [None] + [fac[k] * sc[k - 1] for k in range(1, 6)]
        p = float(1 + (first + j) % 2)                      # pixel value 1 or 2
        _, pos3 = walk(S, pixel, taps)
        flat = c[2] * s4 * s4 + pos3[0] * s4 + pos3[1]
        idx = [("Qconv1", (c[0], f) + taps[0]), ("Qconv2", (c[1], c[0]) + taps[1]),
               ("Qconv3", (c[2], c[1]) + taps[2]), ("Qfc4", (0, 0, unit, flat)),
               ("Q_out", (0, 0, act, unit))]
        for k, (name, ix) in enumerate(idx, 1):
            assert P[name][0][ix] == 0, "paths overlap"
            P[name][0][ix] = w[k]
            N[name][0][ix] = sc[k - 1]
            assert P[name][0][ix] == w[k]
        b = imgs[j]
        st[b, f, pixel[0], pixel[1]] = p
        ac[b] = 0
        ac[b, act] = 1
        # the chain: a[k] leaves layer k, d[k] arrives at layer k's output
        a = [p]
        for k in range(1, 6):
            a.append(a[-1] * w[k])
        dq = dqf * 2.0 ** -int(np.floor(np.log2(B)))
        mine = a[5] - (gamma or 0.0) * a[5]   # Q_sa less the target's P share
        if mine == B * dq:            # reward would be 0: a degenerate target
            dq = -dq
        delta = B * dq
        reward = mine - delta
        assert exact32(delta) and exact32(reward) and exact32(dq), (kind, B, delta, reward)
        assert exact32(mine) and reward != 0 and a[5] - delta != 0
        rw[b] = reward
        d = [None] * 6
        d[5] = dq
        for k in (4, 3, 2, 1):
            d[k] = d[k + 1] * w[k + 1]
        for k, name in enumerate(LAYERS, 1):
            operands[name + ".fwd"].append((a[k - 1], w[k]))
            operands[name + ".wgrad"].append((a[k - 1], d[k]))
            if k > 1:
                operands[name + ".dgrad"].append((d[k], w[k]))
        where.append(dict(image=b, kind=kind, idx=idx, a=a, d=d, w=w,
                          placement=(first + j) % len(pl)))
        lossy = lossy or kind == "D" or kind[0] == "B"
    compared = tuple(n for n in BLOBS if not (lossy and n == "loss"))
    return Probe(S, B, tuple(kinds), P, N, (st, ac, rw, st.copy(), nt), compared,
                 dict(operands), where)


# B >= 128 (the oracle's cost grows with B): three passes of the kinds that put
# every operand shape on every convolution direction -- nine, one for each
# placement of S = 16; the fc-layer kinds run at the smaller batches
LARGE_B_KINDS = ["K1", "K2", "K3", "D", "P1", "P2", "B1", "B2", "B3"]


def kinds_for(B):
    return LARGE_B_KINDS if B >= 128 else KINDS


def expected_gaps(B):
    """{site: the mutants() names no probe of batch B can tell there}: what
    each case does NOT own, stated ahead of the probes and held to them by
    tests/test_split_probe.py.
    * conv1's activation operand is the frame, one plane by contract: no term
      with a1 or a2 exists in its forward and weight gradient, at any B.
    * B >= 128 runs no fc kind (K4, K5, P3, P4, B4, B5): fc4 and Q_out meet a
      multi-plane activation (from K3) and a multi-plane dQ, but their own
      weight is a power of two, so no term with b1 or b2 in their forward and
      data gradient.
    * B = 129, 260: dQ has two planes (B . dQ must fit 24 bits).  A third plane
      on the gradient side then comes only from a three-plane weight below it
      (K3 for conv2, K2 for conv1's weight gradient): conv3, fc4 and Q_out have
      no a2*b0 in the data gradient and no a0*b2 in the weight gradient."""
    a_low = {"a plane 1 zero", "a plane 2 zero", "no a1*b0", "no a1*b1", "no a2*b0"}
    b_low = {"b plane 1 zero", "b plane 2 zero", "no a0*b1", "no a0*b2", "no a1*b1"}
    gaps = collections.defaultdict(set)
    gaps["conv1.fwd"] |= a_low
    gaps["conv1.wgrad"] |= a_low
    if B >= 128:
        for layer in ("fc4", "_out"):
            gaps[layer + ".fwd"] |= b_low
            gaps[layer + ".dgrad"] |= b_low
    if B >= 128 and B & (B - 1):
        for layer in ("conv3", "fc4", "_out"):
            gaps[layer + ".dgrad"] |= {"a plane 2 zero", "no a2*b0"}
            gaps[layer + ".wgrad"] |= {"b plane 2 zero", "no a0*b2"}
    return gaps


def probe_kinds(S, B):
    """kinds_for(B), its head repeated until there is a probe for every
    placement of placements(S): probe m sits on placement m."""
    kinds, n = kinds_for(B), len(placements(S))
    return [kinds[m % len(kinds)] for m in range(max(n, len(kinds)))]


def passes(S, B, gamma=None):
    """Every kind of kinds_for(B) at least once and every placement of
    placements(S) at least once, four (or B) probes to a pass, channels moving
    with the pass."""
    n, kinds = min(4, len(image_slots(B))), probe_kinds(S, B)
    return [build_pass(S, B, kinds[i:i + n], first=i, gamma=gamma)
            for i in range(0, len(kinds), n)]


def with_p(params, pparams=None):
    """{Q..., P...} for set_params / the oracle's pP."""
    src = params if pparams is None else pparams
    return collections.OrderedDict(("P" + k[1:], v) for k, v in src.items())


def oracle(probe, pP=None, gamma=None):
    """The float64 oracle's compared blobs and all ten gradients (gamma: that
    of a build_pass(..., gamma) probe; the reference's otherwise)."""
    pP = with_p(probe.params) if pP is None else pP
    blobs, grads = ref.full_pass(probe.params, pP, *probe.mb,
                                 **({} if gamma is None else {"gamma": gamma}))
    blobs = dict(blobs)
    blobs["loss"] = np.float64(blobs["loss"])
    return blobs, grads


def outputs(net, probe):
    """The same tensors read from a net (either library) after forward_backward."""
    B = probe.B
    blobs = {n: np.asarray(net.blob(n)).reshape((B, 4) if n.endswith("_out") else
                                                (B,) if n != "loss" else ())
             for n in probe.compared}
    return blobs, net.split(net.get_grads_flat(), "Q")


def explain(got, want, probe):
    """Which lost term a wrong element looks like: the kept terms whose share
    of their product is within a factor 1.5 of the element's relative error."""
    rel = abs(float(got) - float(want)) / max(abs(float(want)), 1e-300)
    hits = []
    for site, pairs in probe.operands.items():
        for (a, b) in pairs:
            pa, pb = split3(a), split3(b)
            for (i, j) in TERMS[1:]:
                t = abs(float(pa[i] * pb[j])) / abs(a * b)
                if t > 0 and 1 / 1.5 <= rel / t <= 1.5:
                    hits.append("%s a%d*b%d" % (site, i, j))
    return "relative error %.3g = 2^%.1f; terms of that size: %s" % (
        rel, np.log2(rel) if rel > 0 else -np.inf, ", ".join(sorted(set(hits))) or "none")


def assert_bits(got_blobs, got_grads, want_blobs, want_grads, probe, what=""):
    """np.array_equal on the float32 bits of every compared tensor."""
    def one(name, got, want):
        got = np.asarray(got, np.float32).reshape(np.shape(want))
        w32 = np.asarray(want, np.float64).astype(np.float32)
        if np.array_equal(got.view(np.uint32), w32.view(np.uint32)):
            return
        bad = np.argwhere(np.atleast_1d(got != w32) | np.atleast_1d(np.isnan(got)))
        i = tuple(bad[0]) if got.ndim else ()
        g, w = np.atleast_1d(got)[i] if got.ndim else got, np.atleast_1d(w32)[i] if got.ndim else w32
        raise AssertionError(
            "%s%s (S %d, B %d, kinds %s): %d elements differ; first at %s: got %.9g (0x%08x), "
            "oracle %.9g (0x%08x); %s" % (
                what, name, probe.S, probe.B, ",".join(probe.kinds), len(bad), i, g,
                np.float32(g).view(np.uint32), w, np.float32(w).view(np.uint32),
                explain(g, w, probe)))
    for n in probe.compared:
        one(n, got_blobs[n], want_blobs[n])
    for n in want_grads:
        for k in range(2):
            one("%s[%d]" % (n, k), got_grads[n][k], want_grads[n][k])


def run_pass(net, probe, pP=None):
    """Bind the probe's parameters (P tower: pP or the same) and minibatch,
    run forward_backward, return outputs()."""
    params = collections.OrderedDict(probe.params)
    params.update(with_p(probe.params) if pP is None else pP)
    net.set_params(params)
    net.write_minibatch(*probe.mb)
    net.forward_backward()
    return outputs(net, probe)


def check_update_and_blend(net, probe, lr=0.5):
    """The planes an update rebuilds: start from the neutral paths, reach the
    probe's parameters by apply("sgd", lr) on a designed gradient (theta - lr g
    exact), pass; then blend the target tower half way (tau = 0.5, exact) and
    pass again.  Both passes bit-exact, P_out included."""
    N, Pq, mb = probe.neutral, probe.params, probe.mb
    fn, fp = ref.flatten(N).astype(np.float64), ref.flatten(Pq).astype(np.float64)
    g = (fn - fp) / lr
    assert exact32(g) and np.array_equal(fn - lr * g, fp)
    both = collections.OrderedDict(N)
    both.update(with_p(N))
    net.set_params(both)
    net.set_grads_flat(g.astype(np.float32))
    net.apply("sgd", lr=lr)
    assert np.array_equal(net.get_flat(0), fp.astype(np.float32)), "sgd apply is not exact"
    net.write_minibatch(*mb)
    net.forward_backward()
    blobs, grads = ref.full_pass(Pq, with_p(N), *mb)
    assert_bits(*outputs(net, probe), blobs, grads, probe, what="after apply: ")
    assert np.any(blobs["P_out"] != 0)
    net.set_target_tau(0.5)
    try:
        net.soft_sync_target()
    finally:
        net.set_target_tau(1.0)
    half = collections.OrderedDict(
        (n, [(np.asarray(N[n][i], np.float64) + Pq[n][i]) / 2 for i in range(2)]) for n in N)
    assert all(exact32(v[0]) for v in half.values())
    assert np.array_equal(net.get_flat(1), ref.flatten(half).astype(np.float32)), "blend is not exact"
    net.forward_backward()
    blobs, grads = ref.full_pass(Pq, with_p(half), *mb)
    assert exact32(blobs["P_out"]) and np.any(blobs["P_out"] != 0)
    assert_bits(*outputs(net, probe), blobs, grads, probe, what="after blend: ")


GAMMA = 0.5          # of the nets of the target probes: gamma . P_out is then exact


def fill_ring(net):
    """Any ring: the lr = 0 steps of check_fused_sites draw from it."""
    import _coherence as co
    n = co.ring_slots(net.batch)
    net.replay_create(n)
    net.replay_import(*co.ring(net.frame, n), 0, n)


def host_step(net):
    """What step(sgd, lr = 0, target_period = 1) does, driven from the host (the
    CPU twin has no step of its own)."""
    net.replay_sample(np.arange(8, 8 + net.batch, dtype=np.int32))
    net.forward_backward()
    net.apply("sgd", lr=0.0)
    net.soft_sync_target()


def check_fused_sites(net, p0, p1, step=None):
    """The update sites fused into step() (the slab reduce, K2, K4) and the
    hard P <- Q copy, on a net of gamma = GAMMA over a filled ring.  step: what
    runs in place of net.step(cfg) (host_step, on the twin).

    A step with the sgd rule at lr = 0 leaves theta - 0 . g = theta exact
    whatever the ring held, and still rewrites every derived plane from it;
    with target_period = 1 it also copies Q to P, which held the neutral paths
    until then.  The pass after it must be bit-exact, and under non_terminal =
    1 (p1: the gamma pass of p0's parameters) the target carries gamma . max_a
    P_out, so the copied tower's planes reach target_Q_sa and every gradient.
    First the same pass after the eager sync_target(); last a second step with
    tau = 0.5 from a neutral P: the blend written by the fused site."""
    N, Pq = p0.neutral, p0.params
    fq, fn = ref.flatten(Pq), ref.flatten(N)
    assert np.array_equal(fq, ref.flatten(p1.params)) and not np.array_equal(fq, fn)
    want = oracle(p1, gamma=GAMMA)
    assert all(exact32(want[0][n]) for n in p1.compared)
    for w in p1.where:                                   # P_out's share is in the target
        b = w["image"]
        assert want[0]["target_Q_sa"][b] == p1.mb[2].reshape(-1)[b] + GAMMA * w["a"][5]
    both = collections.OrderedDict(Pq)
    both.update(with_p(N))

    def passes_exactly(probe, blobs, grads, what):
        net.write_minibatch(*probe.mb)
        net.forward_backward()
        assert_bits(*outputs(net, probe), blobs, grads, probe, what=what)

    net.set_params(both)
    net.sync_target()
    assert np.array_equal(net.get_flat(1), fq), "sync_target is not a copy"
    passes_exactly(p1, *want, what="after sync_target: ")

    net.set_params(both)
    cfg = net.step_cfg("sgd", lr=0.0, target_period=1, seed=3)
    step = step or (lambda: net.step(cfg))
    step()
    net.synchronize()
    assert np.array_equal(net.get_flat(0), fq), "a step at lr = 0 moved theta"
    assert np.array_equal(net.get_flat(1), fq), "the step's P <- Q is not a copy"
    passes_exactly(p1, *want, what="after step: ")

    net.set_flat(1, fn)
    net.set_target_tau(0.5)
    try:
        step()
        net.synchronize()
    finally:
        net.set_target_tau(1.0)
    half = collections.OrderedDict(
        (n, [(np.asarray(N[n][i], np.float64) + Pq[n][i]) / 2 for i in range(2)]) for n in N)
    assert np.array_equal(net.get_flat(0), fq), "a step at lr = 0 moved theta"
    assert np.array_equal(net.get_flat(1), ref.flatten(half).astype(np.float32)), \
        "the step's blend is not exact"
    blobs, grads = ref.full_pass(Pq, with_p(half), *p0.mb)
    assert exact32(blobs["P_out"]) and np.any(blobs["P_out"] != 0)
    passes_exactly(p0, blobs, grads, what="after blended step: ")


# ---------------------------------------------------------------- frames contract
def contract_inputs(S, B, seed=3):
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 256, (B, 4, S, S)).astype(np.float32)
    ns = rng.integers(0, 256, (B, 4, S, S)).astype(np.float32)
    ac = np.zeros((B, 4, 1, 1), np.float32)
    ac[np.arange(B), rng.integers(0, 4, B)] = 1
    rw = rng.integers(-1, 2, (B, 1, 1, 1)).astype(np.float32)
    nt = (rng.random((B, 1, 1, 1)) > 0.3).astype(np.float32)
    return st, ac, rw, ns, nt


def check_frames_contract(net, S, B):
    """Either library: refusal, message, minibatch unchanged."""
    import pytest
    from ddq import _lib
    mb = contract_inputs(S, B)
    net.write_minibatch(*mb)
    before = net.read_minibatch()
    other = contract_inputs(S, B, seed=4)
    for which, name in ((0, "state"), (3, "next_state")):
        for bad in (other[which] / 3, None):
            arrs = list(other)
            if bad is None:                                   # one value, 9 significant bits
                arrs[which] = other[which].copy()
                arrs[which].reshape(-1)[777] = 200.5
                first, val = 777, 200.5
            else:
                arrs[which] = bad
                first = int(np.flatnonzero(bad.view(np.uint32).reshape(-1) & 0xFFFF)[0])
                val = float(bad.reshape(-1)[first])
            with pytest.raises(_lib.DDQError) as ei:
                net.write_minibatch(*arrs)
            assert ei.value.code == _lib.DDQ_EINVAL
            assert "%s[%d] = %.9g is not exactly representable in bf16" % (name, first, val) \
                in ei.value.msg, ei.value.msg
            for x, y in zip(net.read_minibatch(), before):
                np.testing.assert_array_equal(x, y)
    for v in (np.inf, np.nan):
        arrs = list(other)
        arrs[0] = other[0].copy()
        arrs[0].reshape(-1)[5] = v
        with pytest.raises(_lib.DDQError):
            net.write_minibatch(*arrs)
    for x, y in zip(net.read_minibatch(), before):
        np.testing.assert_array_equal(x, y)


def half_integer_inputs(S, B):
    mb = list(contract_inputs(S, B, seed=6))
    for i in (0, 3):
        mb[i] = (np.minimum(mb[i], 127.0) + 0.5 * (mb[i] % 2)).astype(np.float32)   # .. 127.5: 8 bits
        mb[i].reshape(-1)[0] = 100.5
    return tuple(mb)
