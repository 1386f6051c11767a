"""The conv2 + conv3 weight-gradient pair (csrc/wgrads.h) after conv2's bias
column moved to bias units of its own (a third block range behind conv3's
workgroups) and rows whose input row lies outside the image are no longer
staged or multiplied.

Both changes keep every add and its order, so the gradients are the parent's
bit for bit.  Each case is one full pass at a small shape, compared against the
float64 oracle with the elementwise rule of _parity.py, held to the parent
build's own normwise error ||gpu - ref||_2 / ||ref||_2 per tensor (no larger:
equal by construction, so any drift shows), and run twice for equal bits.

Shapes: the three pair instantiations (row width <= 16, <= 32, <= 64), row
counts B * H the group count does not divide, a single image, and (24, 1),
whose 12 conv2 rows are fewer than the 24 row groups aimed for: every group is
one row and three of a bias unit's four waves have none.

Normwise errors of the parent build on these cases, measured with this
file's pair_errors() (Qconv2 w, b, Qconv3 w, b; full precision in PARENT_ERRS):
(24, 1) 1.618e-7 1.485e-7 1.821e-7 1.135e-7; (24, 2) 2.617e-7 2.638e-7 2.601e-7
2.210e-7; (40, 3) 3.211e-7 3.251e-7 3.143e-7 2.730e-7; (64, 2) 2.708e-7
2.580e-7 2.596e-7 1.927e-7; (72, 1) 9.940e-7 9.999e-7 1.013e-6 9.959e-7.
"""
import numpy as np
import pytest

from _parity import check_full_pass
from test_gpu_parity import make_inputs, make_params

pytestmark = pytest.mark.gpu

TENSORS = (("Qconv2", 0), ("Qconv2", 1), ("Qconv3", 0), ("Qconv3", 1))

# (S, B) -> the parent build's normwise error of Qconv2 w, b, Qconv3 w, b
PARENT_ERRS = {
    (24, 1): (1.6179357160040713e-07, 1.4849324358893527e-07, 1.8212328489232898e-07, 1.1345183199865338e-07),
    (24, 2): (2.616946100848251e-07, 2.638139387502135e-07, 2.600887574123255e-07, 2.2102962359399472e-07),
    (40, 3): (3.211077286653952e-07, 3.251248531989051e-07, 3.142704616398823e-07, 2.7300363412704983e-07),
    (64, 2): (2.708483969981981e-07, 2.5802895580618564e-07, 2.5960382509482155e-07, 1.9270031772838498e-07),
    (72, 1): (9.940419268997876e-07, 9.99946638161268e-07, 1.012637271547505e-06, 9.959339031678899e-07),
}


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


def pair_errors(ddq, ref, S, B):
    """One full pass on uniform frames with the x3 fillers of test_gpu_parity:
    the elementwise check against the oracle, then the four tensors' normwise
    errors and whether a second pass gave the same bits."""
    rng = np.random.default_rng(800 + S + B)
    pQ, pP = make_params(ref, rng, S, "x3")
    net = ddq.DeepQNet(batch=B, frame=S)
    params = dict(pQ)
    params.update(pP)
    net.set_params(params)
    mb = make_inputs(rng, B, S, "uniform")
    net.write_minibatch(*mb)
    net.forward_backward()
    g_gpu = net.get_grads_flat().copy()
    _, grads, _ = check_full_pass(ref, net, pQ, pP, mb, grads_gpu=g_gpu)
    g = net.split(g_gpu, "Q")
    errs = []
    for name, i in TENSORS:
        r = np.asarray(grads[name][i], np.float64).reshape(-1)
        d = np.asarray(g[name][i], np.float64).reshape(-1) - r
        errs.append(float(np.linalg.norm(d) / np.linalg.norm(r)))
    net.forward_backward()
    same = np.array_equal(g_gpu.view(np.uint32), net.get_grads_flat().view(np.uint32))
    return errs, same


@pytest.mark.parametrize("S,B", sorted(PARENT_ERRS))
def test_pair_bias_units(ddq, ref, S, B):
    errs, same = pair_errors(ddq, ref, S, B)
    for (name, i), e, p in zip(TENSORS, errs, PARENT_ERRS[(S, B)]):
        print("S %d B %d %s[%d] normwise err %r (parent %r)" % (S, B, name, i, e, p))
    assert same, "two passes gave different bits"
    for (name, i), e, p in zip(TENSORS, errs, PARENT_ERRS[(S, B)]):
        assert e <= p, (S, B, name, i, e, p)
