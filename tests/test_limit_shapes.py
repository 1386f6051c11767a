"""The limit-shape construction (tests/_limit_shapes.py) on the CPU, with the
float64 oracle alone, at S = 16, B = 32, k = 4.

* Silent images add nothing: the oracle's pass over all 32 images gives k / B
  times the gradients of its pass over the 4 live ones, and the same per-image
  blobs at the live rows.
* The harness (tests/_parity.check_full_pass through LiveRows) accepts the
  oracle's own 32-image pass and rejects two mutants of it in which conv2 reads
  another image's values where it should read zero padding -- what a halo
  vector returns whose out-of-range offset kOOB = 2^31 lies inside the tensor:
  in conv2's forward, and in conv2's data gradient, which only conv1's weight
  and bias gradients can show.
* The extent table: every shape ddq_create accepts keeps every 32-bit
  descriptor in range, the GPU cases are accepted shapes, and the five shapes
  of the former domain at which an extent crosses 2^31 or 2^32 sit on the side
  of their threshold that the reading of the kernels predicts -- all of them now
  refused by ddq_create's frame limit.
"""
import ctypes

import numpy as np
import pytest

import _limit_shapes as ls
from _parity import check_full_pass, close
from oracle import ref_numpy as ref

S, B, K = 16, 32, 4
DOWNSTREAM_OF_CONV2 = ("Q_out", "Q_sa", "loss", "Qconv1", "Qconv2", "Qconv3", "Qfc4")
_CACHE = {}


def case():
    """The case, the oracle's pass over the live rows and over all rows:
    computed once, left unchanged."""
    if not _CACHE:
        c = ls.make_case(ref, S, B, K, "uniform")
        full = ls.full_minibatch(ref, c)
        _CACHE.update(c=c, full=full, live=ref.full_pass(c.pQ, c.pP, *c.mb),
                      all=ref.full_pass(c.pQ, c.pP, *full))
    return _CACHE


def test_live_positions():
    live = case()["c"].live
    assert len(live) == K and len(set(live)) == K and live[0] == 0 and live[-1] == B - 1
    # where byte 2^31 of fp32 pool1 / of the split dpool2 planes falls inside the batch
    assert (2 ** 26) // (264 * 264) == 962
    assert {0, 1023, 962, 963}.issubset(ls.live_positions(264, 1024, 8, 1))
    p3 = (2 ** 31 // (8 * 304 * 304)) % 1024
    assert {0, 1023, p3}.issubset(ls.live_positions(304, 1024, 8, 1)) and p3 == 856
    assert {0, 127, 65, 66}.issubset(ls.live_positions(1016, 128, 4, 1))


def test_minibatch_is_the_ring_gather():
    c, full = case()["c"], case()["full"]
    st, act, rw, ns, nt = full
    np.testing.assert_array_equal(st, c.ring[0][:B])
    np.testing.assert_array_equal(ns, c.ring[0][1:])
    silent = np.setdiff1d(np.arange(B), c.live)
    assert (act.reshape(B, 4)[silent] == [0, 0, 0, 1]).all()
    assert not rw.ravel()[silent].any() and not nt.ravel()[silent].any()
    assert not act.reshape(B, 4)[c.live, 3].any()
    for a, b in zip(c.mb, full):
        np.testing.assert_array_equal(a, np.asarray(b)[c.live])
    assert len({f.tobytes() for f in c.ring[0]}) == B + 1      # distinct frames


def test_silent_images_add_nothing():
    t = case()
    c = t["c"]
    (blobs_k, grads_k), (blobs_b, grads_b) = t["live"], t["all"]
    silent = np.setdiff1d(np.arange(B), c.live)
    for name in ("Q_sa", "P_sa", "target_Q_sa"):
        assert not blobs_b[name][silent].any(), name        # exactly zero
        np.testing.assert_array_equal(blobs_b[name][c.live], blobs_k[name])
    for name in ("Q_out", "P_out"):
        np.testing.assert_array_equal(blobs_b[name][c.live], blobs_k[name])
        assert blobs_b[name][silent].any() and not blobs_b[name][:, 3].any()
    assert blobs_b["loss"] == pytest.approx(blobs_k["loss"] * K / B, rel=1e-14)
    for name in grads_k:
        for i in range(2):
            a, b = grads_b[name][i], grads_k[name][i] * (K / B)
            assert np.abs(b).max() > 0
            # float64 round-off of sums taken in another order
            assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), (name, i)


def harness(net):
    c = case()["c"]
    view = ls.LiveRows(net, c.live)
    return check_full_pass(ref, view, c.pQ, c.pP, c.mb, grads_gpu=view.get_grads_flat(),
                           quiet=True)


def test_harness_accepts_the_oracle_on_all_rows():
    t = case()
    c = t["c"]
    harness(ls.OracleNet(ref, c.pQ, c.pP, t["full"]))
    # and the adapter hands over what it says
    net = ls.OracleNet(ref, c.pQ, c.pP, t["full"])
    view = ls.LiveRows(net, c.live)
    assert view.batch == K and view.scale == B / K
    np.testing.assert_array_equal(view.blob("Q_out"), net.blob("Q_out")[c.live])
    assert view.pool_mask(2).shape == (K, 64, S // 4, S // 4)
    assert float(view.blob("loss")) == float(net.blob("loss")) * (B / K)
    np.testing.assert_array_equal(view.get_grads_flat(), net.get_grads_flat() * np.float32(B / K))


def test_harness_rejects_a_conv2_forward_that_reads_another_image():
    t = case()
    c = t["c"]
    with ls.mutant(ref, "forward", lambda n: (n + 1) % B):
        net = ls.OracleNet(ref, c.pQ, c.pP, t["full"])
    # conv1 is untouched: the mutant's pool1 routing is the oracle's
    with pytest.raises(AssertionError) as ei:
        harness(net)
    arg, msg = ei.value.args[0], str(ei.value)
    if isinstance(arg, tuple) and "routing" in arg[0]:   # full_pass_gpu_routing: (text, layer, ..)
        assert arg[1] in (2, 3), msg                     # pool2's or pool3's routing
    else:
        assert any(n in msg for n in DOWNSTREAM_OF_CONV2), msg
    # the values themselves, not only the routing: Q_out at the live rows
    mq = ref.magnitudes(c.pQ, c.pP, *c.mb)[0]["Q_out"]
    with pytest.raises(AssertionError, match="Q_out"):
        close(net.blob("Q_out")[c.live], t["live"][0]["Q_out"], what="Q_out", tensor="Q_out",
              mag=mq, quiet=True)


def test_harness_sees_a_wrong_conv2_data_gradient_through_conv1_alone():
    t = case()
    c = t["c"]
    live = [int(p) for p in c.live]
    # the restated data gradient is the oracle's
    rng = np.random.default_rng(0)
    x, td = rng.normal(size=(2, 32, 8, 8)), rng.normal(size=(2, 64, 8, 8))
    W = rng.normal(size=(64, 32, 5, 5))
    zeros = lambda n: np.zeros((64, 12, 12))  # noqa: E731
    np.testing.assert_allclose(ls.data_gradient(td, W, 2, zeros),
                               ref.conv_backward(x, W, td, 2)[2], rtol=1e-12, atol=1e-12)
    # the halo of image n gets a live image's gradient (a silent one's is zero)
    src = lambda n: live[1] if n == live[0] else live[0]  # noqa: E731
    with ls.mutant(ref, "dgrad", src):
        net = ls.OracleNet(ref, c.pQ, c.pP, t["full"])
    honest = ls.OracleNet(ref, c.pQ, c.pP, t["full"])
    for name in ("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss"):
        np.testing.assert_array_equal(net.blob(name), honest.blob(name))
    g, h = net.split(net.get_grads_flat()), honest.split(honest.get_grads_flat())
    for name in g:
        same = all(np.array_equal(a, b) for a, b in zip(g[name], h[name]))
        assert same == (name != "Qconv1"), name
    with pytest.raises(AssertionError) as ei:
        harness(net)
    assert "Qconv1[0]" in str(ei.value) or "Qconv1[1]" in str(ei.value), str(ei.value)


# ------------------------------------------------------------- the extent table
def gpu_cases():
    from test_gpu_limit_shapes import CASES
    return CASES


# (S, B): the shapes ddq_create accepted before the frame limit at which an
# extent crosses 2^31 or 2^32, and the descriptors the table must fault there
FORMER = {
    (256, 1024): {"conv2 dgrad w1 rs"},      # fp32 pool1 exactly 2^31: kOOB still outside
    (264, 1024): {"conv2 fwd rin32: fp32 pool1", "conv2 dgrad w1 rs"},
    (304, 1024): {"conv2 fwd rin32: fp32 pool1", "conv2 dgrad w1 rs", "conv2 fwd rx",
                  "conv2 dgrad rin"},
    (360, 1024): {"conv2 fwd rin32: fp32 pool1", "conv2 dgrad w1 rs", "conv2 fwd rx",
                  "conv2 dgrad rin"},
    (1016, 128): {"conv2 fwd rin32: fp32 pool1", "conv2 dgrad w1 rs", "conv2 fwd rx",
                  "conv2 dgrad rin"},
}


def test_gpu_cases_are_accepted_and_in_range():
    cases = gpu_cases()
    assert (ls.MAX_FRAME, ls.MAX_BATCH) in [(s, b) for s, b, _, _ in cases]
    for s, b, k, _ in cases:
        assert ls.accepted(s, b) and b % k == 0, (s, b, k)
        assert ls.descriptor_faults(s, b) == [], (s, b)
        assert max(ls.extents(s, b).values()) < 2 ** 31


def test_every_accepted_shape_keeps_its_descriptors_in_range():
    n = 0
    for s in range(16, 1025, 8):
        for b in (1, 2, 31, 32, 33, 128, 256, 257, 512, 1023, 1024):
            if ls.accepted(s, b):
                n += 1
                assert ls.descriptor_faults(s, b) == [], (s, b)
    assert n == 15 * 11
    # the frame limit is what does it: the 32-bit guard alone lets these through
    for (s, b), want in FORMER.items():
        assert ls.refusal(s, b) == "frame", (s, b)
        got = [name for name, _, _ in ls.descriptor_faults(s, b)]
        assert len(got) == len(want) and all(any(g.startswith(w) for g in got) for w in want), \
            (s, b, got)
    e = ls.extents(256, 1024)
    assert e["pool1f: fp32 pool1 (each tower)"] == 2 ** 31
    assert e["wpart[0]: conv1's weight-gradient slabs"] == 2 ** 32
    assert ls.extents(264, 1024)["pool1f: fp32 pool1 (each tower)"] > 2 ** 31
    assert ls.extents(288, 1024)["dconv2s: split dpool2, three planes"] < 2 ** 31 < \
        ls.extents(296, 1024)["dconv2s: split dpool2, three planes"]
    assert 16 * 1024 * 360 * 360 < 2 ** 31 <= 16 * 1024 * 368 * 368
    assert ls.extents(1016, 128)["theta = W4 + the rest (each tower)"] < 2 ** 31


@pytest.mark.parametrize("s,b", [(128, 1024), (136, 1), (136, 1024), (256, 1024), (1016, 128),
                                 (1024, 1), (512, 1024), (128, 1025), (16, 1), (12, 4)])
def test_accepted_restates_ddq_create(s, b):
    """ddq_create checks the shape before it looks for a device: a refused shape
    is DDQ_EINVAL on any host, with the reason ``refusal`` names."""
    from ddq import _lib
    lib = _lib.load()
    desc = _lib.NetDesc(b, s, 4, 4, 0.85)
    ctx = ctypes.c_void_p()
    rc = lib.ddq_create(ctypes.byref(ctx), 0, ctypes.byref(desc))
    err = lib.ddq_last_error(None) or b""
    if rc == 0:
        lib.ddq_destroy(ctx)
    why = ls.refusal(s, b)
    if why is None:
        assert rc != _lib.DDQ_EINVAL, err
    else:
        assert rc == _lib.DDQ_EINVAL
        assert {"32-bit": b"32-bit", "frame": b"backward pass handles frames up to 128",
                "range": b"must be"}[why] in err, err
