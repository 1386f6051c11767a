"""The conv2 + conv3 weight-gradient pair (csrc/wgrads.h) at the group shapes
where its split of a row group over the workgroup's row lanes can go wrong:
one-row groups (most lanes idle), groups that straddle images, ragged last
groups, lanes with unequal row counts, rows with a zero tail, and the wide-row
instantiation of frames above 64.

A slab is the sum of its group's rows, lane by lane, so a lane that drops or
doubles a row, or a cross-lane sum that skips a lane, moves the weight
gradient by a whole row's contribution.  The elementwise rule of _parity.py
bounds every element by the sum of its |terms|, which such an error can stay
under, so the cases are also held to a normwise bound against the float64
oracle.
"""
import numpy as np
import pytest

from _parity import check_full_pass
from test_gpu_parity import make_inputs, make_params

pytestmark = pytest.mark.gpu

# (S, B), all on uniform frames with the x3 fillers of test_gpu_parity
CASES = [
    (24, 2),   # every row group is a single row: all lanes but one idle, both layers
    (40, 3),   # row width 20 (zero tail to 32), three-row groups across images, conv3 one-row groups
    (64, 2),   # the bench's instantiation, three-row groups, ragged last group
    (64, 8),   # the bench's instantiation, 11-row groups: unequal rows per lane, groups across images
    (72, 1),   # row width 36: the wide-row instantiation
]

# Normwise bound on ||gpu - ref||_2 / ||ref||_2 of the Qconv2 / Qconv3 weight
# and bias gradients: twice the worst value the kernel gave on these cases
# before its bias sum was restructured (an fp32 sum of the same terms in
# another order stays within a factor of two; a dropped or doubled row moves
# the norm by orders of magnitude more).  Measured then, worst of Qconv2 w, b,
# Qconv3 w, b per case: (24, 2) 1.73e-7, (40, 3) 2.04e-7, (64, 2) 6.33e-7,
# (64, 8) 2.43e-7, (72, 1) 1.88e-7.
PARENT_WORST = 6.329e-7
NORM_BOUND = 2 * PARENT_WORST


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


def run_case(ddq, ref, S, B):
    rng = np.random.default_rng(700 + S + B)
    pQ, pP = make_params(ref, rng, S, "x3")
    net = ddq.DeepQNet(batch=B, frame=S)
    params = dict(pQ)
    params.update(pP)
    net.set_params(params)
    mb = make_inputs(rng, B, S, "uniform")
    net.write_minibatch(*mb)
    net.forward_backward()
    return net, pQ, pP, mb


@pytest.mark.parametrize("S,B", CASES)
def test_pair_parity_and_norm(ddq, ref, S, B):
    net, pQ, pP, mb = run_case(ddq, ref, S, B)
    g_gpu = net.get_grads_flat()
    _, grads, _ = check_full_pass(ref, net, pQ, pP, mb, grads_gpu=g_gpu)
    g = net.split(g_gpu, "Q")
    worst = 0.0
    for name in ("Qconv2", "Qconv3"):
        for i in range(2):
            r = np.asarray(grads[name][i], np.float64).reshape(-1)
            d = np.asarray(g[name][i], np.float64).reshape(-1) - r
            e = float(np.linalg.norm(d) / np.linalg.norm(r))
            print("S %d B %d %s[%d] normwise err %.4g" % (S, B, name, i, e))
            worst = max(worst, e)
    assert worst <= NORM_BOUND, (S, B, worst, NORM_BOUND)


def test_pair_deterministic(ddq, ref):
    net, _, _, _ = run_case(ddq, ref, 64, 8)
    g0 = net.get_grads_flat().copy()
    net.forward_backward()
    g1 = net.get_grads_flat()
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
