"""Shared fp32-vs-float64 comparison for the GPU parity tests.

north_star: "Q-values, targets, gradients and post-update weights must match
within fp32 rtol 1e-4".  What runs:

* blobs and gradients (``close(..., mag=M)``, ``check_full_pass``) are held to
  three rules at once; a tensor passes only if it passes all of them.

  1. |terms| rule, elementwise:  |gpu - ref| <= rtol * |ref| + COND * M,
     rtol = 1e-4, COND = 2e-7, where M is the oracle's per-element sum of
     |terms| (``oracle.ref_numpy.magnitudes``: the whole forward and backward
     re-run on absolute values).  M compounds through every layer, so for most
     gradient tensors COND * M exceeds the gradient itself by orders of
     magnitude: ON ITS OWN THIS RULE ACCEPTS AN ALL-ZERO OR NEGATED GRADIENT
     (tests/test_parity_harness.py keeps that executable).  It is kept because
     it bounds the error of heavily cancelled elements by their own terms
     (worst measured 3.2e-8 * M), which the other two do not.
  2. normwise:  ||gpu - ref||_2 / ||ref||_2 <= NORM_RTOL = 1e-5.  The CPU
     twin measures 2e-8 .. 2e-7 here, the GPU over its whole suite at most
     2.0e-6 (P_sa apart, see OVERRIDES); a dropped image at B = 32 moves the
     norm by ~3e-2, a x1.001 scale by 1e-3.
  3. floored elementwise: rtol 1e-4 for every element with |ref| >=
     ELEM_FLOOR = 1e-2 of the tensor's max|ref|; below that floor an absolute
     ELEM_ATOL = 1e-6 of max|ref|.  The GPU's worst over its suite: 5.3e-5
     and 6.1e-7 (B = 256 at S = 128; DESIGN.md section 4 has the table).

  Rules 2 and 3 need ||ref||_2 > 0.  Only P_sa (an all-terminal batch;
  ZERO_NORM_ALLOWED) may have a zero-norm reference: it falls back to rule 1
  alone and ``close`` prints that it did, quiet or not.  For any other tensor
  a zero-norm reference is an AssertionError in ``close`` itself, so every
  caller on every case (the chains' device-drawn minibatches included) is
  held to it; tests/test_parity_harness.py asserts the same ahead of time on
  the seeded cases the float64 oracle can run quickly.  OVERRIDES holds
  per-tensor exceptions to rules 2 and 3 (measured on the GPU, justified
  against the CPU twin; never looser than normwise 1e-4 / rtol 1e-3 / floor
  1e-1); every entry says why it is there.
* parameters and optimizer state (``close`` without ``mag``; no cancellation
  structure): rtol 1e-4 for every element with |ref| >= 1e-3 of the tensor's
  max, and an absolute 1e-6 of that max (~16 ulps of the largest element)
  below it.

NaN / inf count as mismatches.  Per tensor ``close`` prints the normwise error,
the largest relative error above the floor, the largest absolute error (per
max|ref|) below it, and the 50th / 99th / 100th percentiles of the plain
relative error over the elements with ref != 0.
"""
import numpy as np

RTOL = 1e-4
FLOOR = 1e-3
ATOL = 1e-6
COND = 2e-7     # fp32 rounding allowance per unit of |terms| (~3.4 ulps; measured max 3.2e-8)
NORM_RTOL = 1e-5    # rule 2
ELEM_FLOOR = 1e-2   # rule 3: rtol applies from this fraction of max|ref| up
ELEM_ATOL = 1e-6    # rule 3: absolute bound (per max|ref|) below the floor

# The tensors whose reference may be all zeros (close's ``tensor`` argument).
ZERO_NORM_ALLOWED = ("P_sa",)

# Per-tensor exceptions to rules 2 and 3, keyed by close's ``tensor`` argument
# ("Qfc4[0]", "Q_out", ...; never by the label).  Values: a dict with any of
# norm_rtol, rtol, floor, atol.  An entry needs, in a comment: the value the
# GPU measured and its case, the CPU twin's value on that case, and why the
# difference is inherent to the kernel's documented arithmetic.  Bound = 2x the
# measured value; never beyond HARD_LIMITS.
OVERRIDES = {
    # P_sa, normwise 2.24e-5 = 2 x 1.118e-5, the GPU's value at
    # test_gpu_pair_bias.py::test_pair_bias_units[64-2] (S = 64, B = 2, x3
    # fillers, seed 866).  Image 1 is terminal, so P_sa is the one number
    # max_a P_out[0, a] = 0.0509 -- the only positive of a row whose other
    # entries are -1.5 .. -3.9 -- and the tensor's normwise error is that
    # element's relative error.  It is fc5's sum of 512 products with
    # sum|h4||W5| = 121: cancelled 2400-fold, so one fp32 rounding of the sum
    # (2^-24 * 121) is already 1.4e-4 of it.  The GPU's absolute error there,
    # 5.7e-7, is 4.7e-9 of those terms; the CPU twin's on the same case is
    # 1.2e-7 on this element (normwise 2.3e-6, it passes) and 1.05e-6 = 9.8e-9
    # of the terms on the element next to it, which selected by the max would
    # have read 2.1e-5.  Not a loss of accuracy of the kernel: fp32 does not
    # resolve a cancelled sum to 1e-5 of its value.  P_out itself passes all
    # three rules on that case (normwise 9.2e-7, the element 8.6e-8 of the max).
    "P_sa": dict(norm_rtol=2.24e-5),
}
HARD_LIMITS = dict(norm_rtol=1e-4, rtol=1e-3, floor=1e-1, atol=ELEM_ATOL)


def floor_count(ref, floor=ELEM_FLOOR):
    """How many elements rule 3 holds to its relative bound."""
    a = np.abs(np.asarray(ref, np.float64))
    return int((a >= floor * a.max()).sum()) if a.size and a.max() > 0 else 0


def error_figures(gpu, ref, floor=ELEM_FLOOR):
    """(normwise error, max relative error above the floor, max absolute error
    per max|ref| below it, [p50, p99, p100] of the relative error over
    ref != 0) of a tensor with a non-zero reference."""
    gpu = np.asarray(gpu, np.float64).reshape(np.shape(ref))
    ref = np.asarray(ref, np.float64)
    err, a = np.abs(gpu - ref), np.abs(ref)
    scale = float(a.max())
    above = a >= floor * scale
    nz = a > 0
    return (float(np.linalg.norm(err.ravel()) / np.linalg.norm(ref.ravel())),
            float(np.max(err[above] / a[above])),
            float(np.max(err[~above]) / scale) if (~above).any() else 0.0,
            [float(v) for v in np.percentile(err[nz] / a[nz], [50, 99, 100])])


def close(gpu, ref, rtol=RTOL, what="", floor=FLOOR, atol=ATOL, quiet=False, mag=None,
          cond=COND, strict=True, tensor=None):
    """With mag (the oracle's magnitudes(): per-element sum of |terms|): the
    three rules of the module docstring -- every element within rtol * |ref| +
    cond * mag, and the normwise and the floored elementwise bound
    (strict=False leaves those two out: only for showing what rule 1 alone
    accepts).  ``tensor`` names what is compared ("P_sa", "Qfc4[0]", ...): the
    key of OVERRIDES and of ZERO_NORM_ALLOWED; ``what`` is only the label.  A
    zero-norm reference is an error unless ``tensor`` is in ZERO_NORM_ALLOWED,
    where rule 1 alone applies and a line says so.  Without mag: the floor
    rule for parameters of the module docstring.  Returns the largest relative
    error over the well-conditioned elements (|ref| >= 0.1 * mag; without mag:
    the elements above the floor)."""
    gpu = np.asarray(gpu, np.float64)
    ref = np.asarray(ref, np.float64)
    assert gpu.shape == ref.shape or gpu.size == ref.size, (what, gpu.shape, ref.shape)
    gpu = gpu.reshape(ref.shape)
    if ref.size == 0:
        return 0.0
    scale = float(np.max(np.abs(ref)))
    err = np.abs(gpu - ref)
    if mag is not None:
        m = np.asarray(mag, np.float64).reshape(ref.shape)
        tol = rtol * np.abs(ref) + cond * m + 1e-30
        lim = dict(norm_rtol=NORM_RTOL, rtol=RTOL, floor=ELEM_FLOOR, atol=ELEM_ATOL)
        lim.update(OVERRIDES.get(tensor, {}))
        assert all(lim[k] <= HARD_LIMITS[k] for k in lim), (what, lim)
        above = np.abs(ref) >= lim["floor"] * scale
        big = (np.abs(ref) >= 0.1 * m) & (ref != 0)   # well-conditioned (< 10x cancellation)
        if strict and scale == 0:
            # the escape from rules 2 and 3 is capped: a reference that is all
            # zeros tests nothing under rule 1 (it accepts zeros)
            assert tensor in ZERO_NORM_ALLOWED, (
                "%s: zero-norm reference; only %s may have one (change the case's seed)"
                % (what, ", ".join(ZERO_NORM_ALLOWED)))
            print("%-28s zero-norm reference: only rtol %g + %g * |terms| applies"
                  % (what, rtol, cond))
    else:
        big = np.abs(ref) >= floor * scale
        tol = np.where(big, rtol * np.abs(ref), atol * scale) + 1e-30
    bad = ~(err <= tol)
    max_rel = float(np.max(err[big] / np.abs(ref[big]))) if big.any() and scale > 0 else 0.0
    if not quiet:
        if mag is not None:
            cm = float(np.max(err / (m + 1e-300)))
            if scale > 0:
                nerr, rel_hi, abs_lo, pct = error_figures(gpu, ref, lim["floor"])
                print("%-28s normwise %.3g, max rel %.3g over %d/%d >= %.0e of max, below: max "
                      "abs %.3g of max, rel p50/p99/p100 %.3g/%.3g/%.3g, max err/|terms| %.3g"
                      % (what, nerr, rel_hi, int(above.sum()), ref.size, lim["floor"], abs_lo,
                         pct[0], pct[1], pct[2], cm))
            else:
                print("%-28s max err/|terms| %.3g" % (what, cm))
        else:
            small_abs = float(np.max(err[~big]) / scale) if (~big).any() and scale > 0 else 0.0
            print("%-28s max rel err %.3g (%d/%d elements >= %.0e of scale %.3g), below: max "
                  "abs err %.3g of scale" % (what, max_rel, int(big.sum()), ref.size, floor,
                                             scale, small_abs))
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / tol, 0)), ref.shape)
        raise AssertionError("%s: %d/%d elements off (%s); worst at %s: gpu %.9g ref %.9g%s" % (
            what, int(bad.sum()), bad.size,
            "rtol %g + %g * |terms|" % (rtol, cond) if mag is not None else
            "rtol %g above %g of scale %.3g, atol %g of scale below" % (rtol, floor, scale, atol),
            i, gpu[i], ref[i], "" if mag is None else " |terms| %.3g" % np.asarray(mag).reshape(
                ref.shape)[i]))
    if mag is not None and strict and scale > 0:
        nerr = float(np.linalg.norm(err.ravel()) / np.linalg.norm(ref.ravel()))
        if not nerr <= lim["norm_rtol"]:
            raise AssertionError("%s: normwise error %.4g above %g (||ref|| %.6g)" % (
                what, nerr, lim["norm_rtol"], float(np.linalg.norm(ref.ravel()))))
        tol3 = np.where(above, lim["rtol"] * np.abs(ref), lim["atol"] * scale)
        bad3 = ~(err <= tol3)
        if bad3.any():
            i = np.unravel_index(np.argmax(np.where(bad3, err / tol3, 0)), ref.shape)
            raise AssertionError(
                "%s: %d/%d elements off (rtol %g above %g of max|ref| %.3g, atol %g of it "
                "below); worst at %s: gpu %.9g ref %.9g" % (
                    what, int(bad3.sum()), bad3.size, lim["rtol"], lim["floor"], scale,
                    lim["atol"], i, gpu[i], ref[i]))
    return max_rel


def fc4_near_ties(ref, net, cache, grads, blobs, pQ, mb, g_gpu=None, tie4=COND, max_frac=1e-4):
    """fc4's ReLU (train_val.prototxt:186-191) at a genuine fp32-vs-fp64
    near-tie: a unit (b, n) whose float64 pre-activation lies within tie4 of
    its own sum of |terms| (COND: the fp32 rounding bound of the blobs) of 0
    may be live on the GPU and dead in the oracle
    (or the reverse).  Its side is read off the GPU's fc4 bias gradient
    (db4[n] = sum_b dh4[b][n]: that unit's dh4 is in it or not -- the two
    candidates differ by |dQ . W5[:, n]|, far above fp32 rounding) and adopted
    for that unit only.  Returns (h4 mask or None, adopted count)."""
    pre4, flat = cache["pre4"], cache["flat"]
    W4 = np.asarray(pQ["Qfc4"][0], np.float64).reshape(512, -1)
    b4 = np.asarray(pQ["Qfc4"][1], np.float64).reshape(-1)
    m4 = np.abs(flat) @ np.abs(W4).T + np.abs(b4)
    near = np.argwhere((np.abs(pre4) <= tie4 * m4) & (m4 > 0))   # (exact zeros agree)
    if len(near) == 0:
        return None, 0
    assert len(near) <= max(4, max_frac * pre4.size), ("too many fc4 near-ties", len(near))
    if g_gpu is None:
        g_gpu = net.get_grads_flat()
    db4_gpu = np.asarray(net.split(g_gpu, "Q")["Qfc4"][1], np.float64).reshape(-1)
    db4_ref = np.asarray(grads["Qfc4"][1], np.float64).reshape(-1)
    B = pre4.shape[0]
    act = np.asarray(mb[1], np.float64).reshape(B, 4)
    dq = act * ((blobs["Q_sa"] - blobs["target_Q_sa"]) / B)[:, None]
    W5 = np.asarray(pQ["Q_out"][0], np.float64).reshape(4, 512)
    full = dq @ W5                                   # dh4 before the ReLU mask
    mask = pre4 > 0
    adopted = 0
    for (b, n) in near:
        d = full[b, n] * (-1.0 if mask[b, n] else 1.0)   # what flipping does to db4[n]
        if abs(db4_gpu[n] - (db4_ref[n] + d)) < abs(db4_gpu[n] - db4_ref[n]):
            mask[b, n] = not mask[b, n]
            db4_ref = db4_ref.copy()
            db4_ref[n] += d
            adopted += 1
    return (mask if adopted else None), adopted


def full_pass_gpu_routing(ref, net, pQ, pP, mb, max_frac=1e-4, tie=2e-5, g_gpu=None,
                          with_mask=False):
    """The oracle's full pass on minibatch ``mb`` with max-pool routing taken
    from the GPU's last forward (``net.pool_mask``) wherever the two differ --
    and only there, after proving every difference is a genuine fp32-vs-fp64
    near-tie: both candidate values (or the max vs 0 for a ReLU'd window)
    agree to ``tie`` of the layer's activation scale, and at most ``max_frac``
    of the windows differ -- and fc4's ReLU mask likewise at proven near-ties
    (fc4_near_ties).  Returns (blobs, grads, n_ties) (+ the fc4 mask with
    with_mask)."""
    blobs, grads, cache = ref.full_pass(pQ, pP, *mb, return_cache=True)
    routes, nties = {}, 0
    for i in (1, 2, 3):
        g_code = net.pool_mask(i)
        r_code = ref.route_codes(cache["act%d" % i], cache["arg%d" % i])
        a = cache["act%d" % i]
        Bn, C, H, W = a.shape
        win = a.reshape(Bn, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(
            Bn, C, H // 2, W // 2, 4)
        scale = a.max()
        dis = np.argwhere(g_code != r_code)
        assert len(dis) <= max(2, max_frac * g_code.size), ("too many routing differences", i,
                                                            len(dis))
        for (b, c, y, x) in dis:
            w = win[b, c, y, x]
            vals = [w[k] if k < 4 else 0.0 for k in (g_code[b, c, y, x], r_code[b, c, y, x])]
            assert abs(vals[0] - vals[1]) <= tie * scale, ("non-tie routing mismatch", i, w)
        nties += len(dis)
        routes[i] = g_code
    if nties:
        blobs, grads = ref.full_pass(pQ, pP, *mb, routes=routes)
    h4_mask, n4 = fc4_near_ties(ref, net, cache, grads, blobs, pQ, mb, g_gpu)
    if n4:
        blobs, grads = ref.full_pass(pQ, pP, *mb, routes=routes, h4_mask=h4_mask)
        nties += n4
    if with_mask:
        return blobs, grads, nties, h4_mask
    return blobs, grads, nties


def full_pass_reference(ref, net, pQ, pP, mb, grads_gpu=None):
    """What check_full_pass compares with: the oracle's blobs and gradients
    under the GPU's routing at proven near-ties, the adopted count, and the
    magnitudes of both.  (blobs, grads, nties, mblobs, mgrads)."""
    blobs, grads, nties, h4_mask = full_pass_gpu_routing(ref, net, pQ, pP, mb, g_gpu=grads_gpu,
                                                         with_mask=True)
    routes = {i: net.pool_mask(i) for i in (1, 2, 3)}
    mblobs, mgrads = ref.magnitudes(pQ, pP, *mb, routes=routes, h4_mask=h4_mask)
    return blobs, grads, nties, mblobs, mgrads


def check_full_pass(ref, net, pQ, pP, mb, grads_gpu=None, quiet=False, what="", reference=None,
                    with_mags=False):
    """Blobs and Q gradients of the GPU's last forward/backward on ``mb``
    against the oracle (GPU routing at proven near-ties), every tensor under
    the three rules of ``close(..., mag=M)``: elementwise rtol 1e-4 + COND
    (2e-7) * (its sum of |terms|), normwise 1e-5, and rtol 1e-4 above 1e-2 of
    the tensor's max with 1e-6 of the max below.  ``reference``: a
    full_pass_reference() of the same pass, to compare several candidate
    gradients without re-running the oracle.  Returns (blobs, grads, near-tie
    count), with_mags: + the gradients' magnitudes."""
    if reference is None:
        reference = full_pass_reference(ref, net, pQ, pP, mb, grads_gpu)
    blobs, grads, nties, mblobs, mgrads = reference
    B = net.batch
    for name, shape in (("Q_out", (B, 4)), ("P_out", (B, 4)), ("Q_sa", (B,)), ("P_sa", (B,)),
                        ("target_Q_sa", (B,))):
        close(net.blob(name).reshape(shape), blobs[name], what=what + name, mag=mblobs[name],
              quiet=quiet, tensor=name)
    close(float(net.blob("loss")), blobs["loss"], what=what + "loss", mag=mblobs["loss"],
          quiet=quiet, tensor="loss")
    g = net.split(net.get_grads_flat() if grads_gpu is None else grads_gpu, "Q")
    for name in grads:
        for i in range(2):
            close(g[name][i], grads[name][i], what="%s%s[%d]" % (what, name, i),
                  mag=mgrads[name][i], quiet=quiet, tensor="%s[%d]" % (name, i))
    if with_mags:
        return blobs, grads, nties, mgrads
    return blobs, grads, nties
