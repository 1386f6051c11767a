"""The parity harness itself (tests/_parity.py ``close(..., mag=M)``), on the
CPU with the float64 oracle alone: it accepts an honest fp32 result and
rejects every wrong one.

Before the normwise and floored-elementwise rules the harness held blobs and
gradients only to  rtol * |ref| + COND * M,  M the oracle's pass on absolute
values.  M compounds through every layer, so that rule accepts an all-zero
gradient for most tensors (``test_terms_rule_alone_accepts_zero_gradients``
keeps that fact executable).  Here every tensor of three cases is mutated the
way a broken kernel would mutate it and each mutation has to raise.

Cases, drawn as tests/test_gpu_parity.py::test_full_pass_parity draws them
(seed 100 + S + B): S = 16 B = 32 x3 fillers on uniform frames; the bench's
initialisation on the bench's frames at S = 16 B = 32 and at S = 64 B = 4.

Headroom of an honest fp32 pass (the CPU twin, cpu/twin.cpp) on these cases
under the three bounds normwise 1e-5 / rtol 1e-4 above 1e-2 of max|ref| /
1e-6 of max|ref| below, worst over the ten gradient tensors and the blobs:
  (16, 32, uniform, x3)     normwise 1.01e-7, rel 3.08e-6, abs 6.62e-8
  (16, 32, bench, bench)    normwise 6.35e-8, rel 2.53e-6, abs 3.63e-8
  (64, 4, bench, bench)     normwise 9.50e-8, rel 5.06e-6, abs 6.07e-8
(``test_accepts_the_cpu_twin`` prints them): at least 99x, 19x and 15x inside.
"""
import numpy as np
import pytest

from _parity import ELEM_ATOL, NORM_RTOL, RTOL, check_full_pass, close, error_figures
from _twin import ddq_with_cpu_lib
from oracle import ref_numpy as ref
from test_gpu_parity import FORM_SWITCH_CASES, FULL_PASS_CASES, make_inputs, make_params

CASES = [(16, 32, "uniform", "x3"), (16, 32, "bench", "bench"), (64, 4, "bench", "bench")]
CONV = {"Qconv1": 1, "Qconv2": 2, "Qconv3": 3}
WEIGHTS = ("Qconv1", "Qconv2", "Qconv3", "Qfc4", "Q_out")
# (P_sa: the one tensor with an entry in _parity.OVERRIDES; its mutations have
# to be rejected with the override in force)
BLOBS = ("Q_out", "P_out", "Q_sa", "target_Q_sa", "P_sa", "loss")

_CACHE = {}


def f64(a):
    return np.asarray(a, np.float64)


def draw(S, B, frames, init, seed=None):
    rng = np.random.default_rng(100 + S + B if seed is None else seed)
    pQ, pP = make_params(ref, rng, S, init)
    return pQ, pP, make_inputs(rng, B, S, frames)


def conv_top_diffs(pQ, cq, blobs, mb):
    """The top diffs of conv1..3 (after the pool and ReLU backward) of the
    oracle's pass: what ref.full_pass feeds ref.conv_backward."""
    B = cq["out"].shape[0]
    act = f64(mb[1]).reshape(B, 4)
    dQ = act * ((blobs["Q_sa"] - blobs["target_Q_sa"]) / B)[:, None]
    dh4 = (dQ @ f64(pQ["Q_out"][0]).reshape(4, -1)) * (cq["h4"] > 0)
    dpool = (dh4 @ f64(pQ["Qfc4"][0]).reshape(ref.FC4, -1)).reshape(cq["pool3"].shape)
    tops = {}
    for i in (3, 2, 1):
        a = cq["act%d" % i]
        tops[i] = ref.maxpool_backward(dpool, cq["arg%d" % i], a.shape[2], a.shape[3]) * (a > 0)
        if i > 1:
            dpool = ref.conv_backward(cq["x%d" % (i - 1)], f64(pQ["Qconv%d" % i][0]), tops[i],
                                      ref.CONVS[i - 1][3])[2]
    return tops


def case(key):
    """A case's inputs, oracle pass, magnitudes and conv top diffs: computed
    once, shared by the tests and left unchanged."""
    if key not in _CACHE:
        S, B, frames, init = key
        pQ, pP, mb = draw(*key)
        blobs, grads, cq = ref.full_pass(pQ, pP, *mb, return_cache=True)
        mblobs, mgrads = ref.magnitudes(pQ, pP, *mb)
        tops = conv_top_diffs(pQ, cq, blobs, mb)
        for name, i in CONV.items():     # the restated backward is the oracle's
            gW, gb, _ = ref.conv_backward(cq["x%d" % (i - 1)], f64(pQ[name][0]), tops[i],
                                          ref.CONVS[i - 1][3], need_bottom=False)
            np.testing.assert_allclose(gW.ravel(), grads[name][0].ravel(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(gb.ravel(), grads[name][1].ravel(), rtol=1e-12, atol=0)
        tensors = {}
        for name in grads:
            for i in range(2):
                tensors["%s[%d]" % (name, i)] = (f64(grads[name][i]), f64(mgrads[name][i]))
        for name in BLOBS:
            tensors[name] = (f64(blobs[name]), f64(mblobs[name]))
        _CACHE[key] = dict(S=S, B=B, pQ=pQ, pP=pP, mb=mb, blobs=blobs, grads=grads, cq=cq,
                           tops=tops, tensors=tensors)
    return _CACHE[key]


def rejected(c, name, cand, **kw):
    r, m = c["tensors"][name]
    try:
        close(cand, r, what=name, tensor=name, mag=m, quiet=True, **kw)
    except AssertionError:
        return True
    return False


def f32(a):
    return np.array(a, np.float32)


@pytest.fixture(scope="module")
def ddq():
    return ddq_with_cpu_lib()


@pytest.mark.parametrize("key", CASES)
def test_accepts_the_rounded_reference(key):
    c = case(key)
    for name, (r, m) in c["tensors"].items():
        close(r.astype(np.float32), r, what=name, tensor=name, mag=m, quiet=True)


@pytest.mark.parametrize("key", CASES)
def test_accepts_the_cpu_twin(ddq, key):
    """An honest fp32 implementation passes with room: its figures are printed
    (the headroom of the module docstring)."""
    c = case(key)
    net = ddq.DeepQNet(batch=c["B"], frame=c["S"], mode="cpu")
    params = dict(c["pQ"])
    params.update(c["pP"])
    net.set_params(params)
    net.write_minibatch(*c["mb"])
    net.forward_backward()
    g_twin = net.get_grads_flat()
    blobs, grads, _ = check_full_pass(ref, net, c["pQ"], c["pP"], c["mb"], grads_gpu=g_twin)
    g = net.split(g_twin, "Q")
    worst = [0.0, 0.0, 0.0]
    for name in grads:
        for i in range(2):
            fig = error_figures(g[name][i], grads[name][i])
            worst = [max(a, b) for a, b in zip(worst, fig[:3])]
    for name in BLOBS:
        fig = error_figures(net.blob(name), blobs[name])
        worst = [max(a, b) for a, b in zip(worst, fig[:3])]
    print("twin %s: worst normwise %.3g, rel above the floor %.3g, abs below %.3g of max"
          % (key, worst[0], worst[1], worst[2]))
    net.close()
    # the documented headroom does not drift unseen: an honest fp32 pass at
    # these small shapes stays five times inside each bound
    assert worst[0] <= NORM_RTOL / 5 and worst[1] <= RTOL / 5 and worst[2] <= ELEM_ATOL / 5, worst


def generic_mutations(r):
    """(label, candidate, required) of the mutations every tensor must reject."""
    base = r.astype(np.float32)
    a = np.abs(r).ravel()
    yield "zero", np.zeros_like(base), True
    yield "negated", -base, True
    yield "x1.001", (r * 1.001).astype(np.float32), True
    hi = f32(base).ravel()
    hi[np.argmax(a)] *= 2
    yield "largest x2", hi.reshape(base.shape), True
    j = np.argsort(a, kind="stable")[a.size // 2]
    med = f32(base).ravel()
    med[j] *= 2
    yield "median x2", med.reshape(base.shape), bool(a[j] >= 1e-4 * a.max())


@pytest.mark.parametrize("key", CASES)
def test_rejects_generic_mutations(key):
    c = case(key)
    missed, optional = [], 0
    for name, (r, _) in c["tensors"].items():
        for label, cand, required in generic_mutations(r):
            if not required:
                optional += 1
            elif not rejected(c, name, cand):
                missed.append((name, label))
    print("%s: %d median-element mutations below 1e-4 of max|ref| not required" % (key, optional))
    assert not missed, missed


def busiest(x, axis):
    """Index along ``axis`` of the slice with the largest norm."""
    other = tuple(k for k in range(x.ndim) if k != axis)
    return int(np.argmax(np.sqrt((x * x).sum(axis=other))))


def kernel_mutations(c):
    """(tensor, label, candidate) of what a broken kernel would write."""
    S, B, pQ, mb, grads, cq, tops = (c[k] for k in ("S", "B", "pQ", "mb", "grads", "cq", "tops"))
    # gradients from B - 1 of the B images, dQ still divided by B: the oracle's
    # pass on the sub-batch divides by B - 1, and the backward is linear in dQ
    for drop in (0, B - 1):
        keep = np.array([b for b in range(B) if b != drop])
        _, gsub = ref.full_pass(pQ, c["pP"], *[np.asarray(t)[keep] for t in mb])
        for name in gsub:
            for i in range(2):
                yield ("%s[%d]" % (name, i), "image %d dropped" % drop,
                       f32(gsub[name][i] * ((B - 1.0) / B)))
    for name, i in CONV.items():
        gW = f64(grads[name][0])
        k = gW.shape[2]
        x, pad = cq["x%d" % (i - 1)], ref.CONVS[i - 1][3]
        tap = f32(gW)
        tap[:, :, k // 2, k - 1] = 0
        yield name + "[0]", "tap (%d, %d) zeroed" % (k // 2, k - 1), tap
        shifted = np.zeros_like(x)
        shifted[..., 1:] = x[..., :-1]
        yield (name + "[0]", "input shifted one pixel in x",
               f32(ref.conv_backward(shifted, f64(pQ[name][0]), tops[i], pad,
                                     need_bottom=False)[0]))
        if i > 1:
            # one image's top-diff row: of the rows that carry any gradient,
            # the one of median norm
            rows = np.sqrt((tops[i] ** 2).sum(axis=(1, 3)))
            live = np.argwhere(rows > 0)
            b, y = live[np.argsort(rows[rows > 0], kind="stable")[len(live) // 2]]
            td = tops[i].copy()
            td[b, :, y, :] = 0
            gWr, gbr, _ = ref.conv_backward(x, f64(pQ[name][0]), td, pad, need_bottom=False)
            yield name + "[0]", "top-diff row (%d, %d) dropped" % (b, y), f32(gWr)
            yield name + "[1]", "top-diff row (%d, %d) dropped" % (b, y), f32(gbr)
    for name in WEIGHTS:
        gW = f64(grads[name][0])
        rows = gW.reshape(gW.shape[0], -1) if gW.ndim == 4 and gW.shape[0] > 1 else \
            gW.reshape(gW.shape[2], -1)
        ch = busiest(rows, 0)
        nb = ch + 1 if ch + 1 < rows.shape[0] else ch - 1
        dup = f32(rows)
        dup[nb] = dup[ch]
        yield name + "[0]", "channel %d duplicated into %d" % (ch, nb), dup
    s4 = S // 8
    gW4 = f64(grads["Qfc4"][0]).reshape(ref.FC4, 64, s4, s4)
    yield "Qfc4[0]", "flatten order transposed", f32(gW4.transpose(0, 1, 3, 2))
    q = f32(c["blobs"]["Q_out"])
    q[[0, 1]] = q[[1, 0]]
    yield "Q_out", "rows of images 0 and 1 exchanged", q
    yield "loss", "x B / (B - 1)", f32(c["blobs"]["loss"] * B / (B - 1.0))


@pytest.mark.parametrize("key", CASES)
def test_rejects_kernel_shaped_mutations(key):
    c = case(key)
    missed, n = [], 0
    for name, label, cand in kernel_mutations(c):
        n += 1
        r = c["tensors"][name][0]
        assert not np.array_equal(f32(r).ravel(), cand.ravel()), (name, label, "no-op mutation")
        if not rejected(c, name, cand):
            missed.append((name, label))
    print("%s: %d kernel-shaped mutations" % (key, n))
    assert not missed, missed


def test_terms_rule_alone_accepts_zero_gradients():
    """Why the normwise and floored rules exist: rtol * |ref| + COND * M alone
    (strict=False) accepts an all-zero conv1 and Q_out weight gradient on the
    x3 case; the full rule rejects both."""
    c = case(CASES[0])
    for name in ("Qconv1[0]", "Q_out[0]"):
        zero = np.zeros_like(c["tensors"][name][0], dtype=np.float32)
        assert not rejected(c, name, zero, strict=False), name
        assert rejected(c, name, zero), name


def test_nan_and_inf_are_mismatches():
    c = case(CASES[0])
    for name in ("Qconv2[0]", "Q_out", "loss"):
        for bad in (np.nan, np.inf):
            cand = f32(c["tensors"][name][0])
            cand.ravel()[0] = bad
            assert rejected(c, name, cand), (name, bad)


# ------------------------------------------------------------ the zero-norm cap
# ``close`` itself refuses a zero-norm reference for any tensor but P_sa, so
# every caller on every case is held to the cap when it runs -- the chains'
# device-drawn minibatches and the exchanges included, which depend on device
# state and cannot be drawn here.  The seeded cases are also checked ahead of
# time with the oracle: every FULL_PASS_CASES and pair case of at most
# 16 * 16 * 300 input pixels per tower (about half a second each).  Left to the
# assertion in ``close`` alone: FULL_PASS_CASES (64, 32, uniform), (64, 32,
# bench), the seven B = 256 cases at S >= 24 and the three B > 256 cases there.
def cheap(S, B):
    return S * S * B <= 16 * 16 * 300


def seeded_cases():
    from test_gpu_pair_bias import PARENT_ERRS
    from test_gpu_wgrad_pair import CASES as PAIR
    out = [(k, None) for k in CASES]
    out += [((S, B, fr, init), None) for (S, B, fr, init) in FULL_PASS_CASES
            if cheap(S, B) and (S, B, fr, init) not in FORM_SWITCH_CASES]
    out += [((S, B, "uniform", "x3"), 700 + S + B) for (S, B) in PAIR]
    out += [((S, B, "uniform", "x3"), 800 + S + B) for (S, B) in sorted(PARENT_ERRS)]
    # (last: the ids above are positions in this list and stay what they were)
    out += [(k, None) for k in FORM_SWITCH_CASES if cheap(k[0], k[1])]
    return out


def test_seeded_case_lists_are_covered():
    left = sorted((S, B, fr) for (S, B, fr, _) in FULL_PASS_CASES if not cheap(S, B))
    assert left == [(24, 256, "snake"), (24, 257, "snake"), (40, 256, "snake"),
                    (40, 320, "uniform"), (64, 32, "bench"), (64, 32, "uniform"),
                    (64, 256, "bench"), (64, 288, "bench"), (72, 256, "uniform"),
                    (104, 256, "snake"), (120, 256, "snake"), (128, 256, "snake")]
    assert all(cheap(S, B) for (S, B, _, _), seed in seeded_cases() if seed is not None)


def zero_norm_tensors(blobs, grads):
    zero = [k for k, v in blobs.items() if not np.any(f64(v))]
    zero += ["%s[%d]" % (k, i) for k in grads for i in range(2) if not np.any(f64(grads[k][i]))]
    return zero


@pytest.mark.parametrize("key,seed", seeded_cases())
def test_no_zero_norm_reference_but_p_sa(key, seed):
    if seed is None and key in CASES:
        c = case(key)
        blobs, grads = c["blobs"], c["grads"]
    else:
        pQ, pP, mb = draw(*key, seed=seed)
        blobs, grads = ref.full_pass(pQ, pP, *mb)
    assert set(zero_norm_tensors(blobs, grads)) <= {"P_sa"}, (key, seed)


def test_close_caps_the_zero_norm_escape(capsys):
    """A zero-norm reference: for P_sa the |terms| rule alone, announced even
    when quiet; for any other tensor, or none named, an error -- also for a
    candidate of zeros, which the |terms| rule would accept."""
    c = case(CASES[0])
    m = c["tensors"]["Q_sa"][1]
    zeros = np.zeros(m.shape)
    capsys.readouterr()
    close(zeros.astype(np.float32), zeros, what="r3 P_sa", tensor="P_sa", mag=m, quiet=True)
    assert "zero-norm reference" in capsys.readouterr().out
    with pytest.raises(AssertionError):     # the |terms| rule still holds there
        close(np.ones(m.shape, np.float32), zeros, what="P_sa", tensor="P_sa", mag=m, quiet=True)
    for tensor in ("Q_sa", "Qconv1[0]", None):
        with pytest.raises(AssertionError, match="zero-norm reference"):
            close(zeros.astype(np.float32), zeros, what="r3 P_sa", tensor=tensor, mag=m,
                  quiet=True)
    # the label does not select the override either: P_sa's looser normwise
    # bound is not granted to a tensor whose label merely ends in "P_sa"
    r, mg = c["tensors"]["P_sa"]
    off = (r * (1 + 1.5e-5)).astype(np.float64)
    close(off, r, what="P_sa", tensor="P_sa", mag=mg, quiet=True)
    with pytest.raises(AssertionError, match="normwise"):
        close(off, r, what="not P_sa", tensor="Q_sa", mag=mg, quiet=True)
