"""The training monitor's record recomputed in numpy float64 from what the
existing getters return (tests/test_monitor.py, tests/test_gpu_monitor.py).

Tolerance, derived: the monitor sums exact products (fp32 x fp32 is exact in
double) in double, so a sum of n <= 2^21 terms is off by at most n 2^-53
< 3e-10 relative, whatever the order; numpy's float64 sum likewise.  The only
fp32 rounding is the final one, on both sides, so two correct values differ by
at most one fp32 rounding step each way: relative difference <= 2 * 2^-23.  A
blob of zeros gives exactly 0; the loss is a copy, bit for bit."""
import numpy as np

RTOL = 2.0 * 2.0 ** -23


def blobs_of(net):
    """[(offset, count)] of the ten blobs in ddq_param_layout order."""
    return [(o, c) for blobs in net.layout.values() for (_, o, c) in blobs]


def rms_of(net, flat):
    out = np.zeros(10, np.float32)
    x = np.asarray(flat, np.float32)
    with np.errstate(all="ignore"):
        for j, (o, c) in enumerate(blobs_of(net)):
            v = x[o:o + c].astype(np.float64)
            out[j] = np.float32(np.sqrt(np.sum(v * v) / c))
    return out


def expected(net, iteration, tag):
    """The record the monitor must take of ``net`` as it is now."""
    from ddq.net import MONITOR_DTYPE
    rec = np.zeros((), MONITOR_DTYPE)
    thq, thp, g = net.get_flat(0), net.get_flat(1), net.get_grads_flat()
    rec["iteration"], rec["tag"] = iteration, tag
    rec["loss"] = net.blob("loss")
    q = net.blob("Q_out").reshape(net.batch, 4).astype(np.float64)
    rec["q_max_mean"] = np.float32(q.max(axis=1).mean())
    rec["param_rms"][0], rec["param_rms"][1] = rms_of(net, thq), rms_of(net, thp)
    rec["grad_rms"] = rms_of(net, g)
    rec["nonfinite"] = [int((~np.isfinite(x)).sum()) for x in (thq, thp, g)]
    return rec


def assert_floats(got, want, what):
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    for k, (a, b) in enumerate(zip(got, want)):
        if not np.isfinite(b):
            assert (np.isnan(a) and np.isnan(b)) or a == b, (what, k, a, b)
        elif b == 0:
            assert a == 0, (what, k, a, b)
        else:
            rel = abs(float(a) - float(b)) / abs(float(b))
            assert rel <= RTOL, (what, k, a, b, rel)


def assert_record(got, want):
    for f in ("iteration", "tag", "reserved"):
        assert int(got[f]) == int(want[f]), (f, got[f], want[f])
    assert list(got["nonfinite"]) == list(want["nonfinite"])
    assert np.float32(got["loss"]).tobytes() == np.float32(want["loss"]).tobytes()
    for f in ("q_max_mean", "param_rms", "grad_rms"):
        assert_floats(got[f], want[f], f)
