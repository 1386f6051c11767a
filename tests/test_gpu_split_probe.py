"""The exact-value probes of tests/_split_probe.py on the MI355X: every compared
tensor of every pass must equal the float64 oracle on the float32 BITS.  The
inputs are built so that no product and no partial sum rounds (proved on the
CPU, tests/test_split_probe.py), so the bound is derived, not measured: a
kernel that loses one of the six split terms, or one plane of an operand,
flips a known bit.  A mismatch reports the terms of that size.

Kernel families by (S, B): (16, 4) the small-map step K1-K4; (16, 40) K4
applying the unit sums; (16, 128) / (16, 129) either side of K3's form switch
(tests/test_split_probe.py holds the pair to the threshold in the source; no
call reports the form that ran); (24, 4) the general kernels; (40, 2) partial
edge tiles; (64, 2) the wide-row weight-gradient pair; (16, 260) the general
kernels at S = 16.  Every case visits every placement of sp.placements(S).

After an update: the eager sgd apply on a designed gradient, then a soft blend
of the target tower with tau = 0.5, each followed by a bit-exact pass -- the
planes those launches rebuild (P_out holds the target tower's).  The update
sites fused into step() (the slab reduce, K2, K4): a step at lr = 0 leaves
theta exact and still rewrites every plane; with target_period = 1 it copies
Q over a P tower that held other values, and on a net of gamma = 0.5 under
non_terminal = 1 that tower reaches the target and every gradient; a second
step blends with tau = 0.5.  The eager sync_target() likewise.  What this does
not see: a fused site whose rewrite depends on a nonzero lr . g.

The acting forward (forward_q, Q_out bit-exact for the forward kinds): the
small-path tower kernel at S = 16 (n = 1, 3), and on general contexts both
conv families, spread and batch, at (24, 1), (24, 3) and (40, 2).

The frames contract of ddq_write_minibatch is held here as on the CPU twin.
"""
import numpy as np
import pytest

import _split_probe as sp
from _parity import check_full_pass

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


@pytest.mark.parametrize("S,B", sp.CASES)
def test_full_pass_bit_exact(ddq, S, B):
    net = ddq.DeepQNet(batch=B, frame=S)
    assert net.small_path()[0] == (S == 16 and B <= 256)
    for p in sp.passes(S, B):
        blobs, grads = sp.oracle(p)
        sp.assert_bits(*sp.run_pass(net, p), blobs, grads, p)
    net.close()


@pytest.mark.parametrize("S,B", [(16, 4), (24, 4)])
def test_bit_exact_after_apply_and_blend(ddq, S, B):
    net = ddq.DeepQNet(batch=B, frame=S)
    for p in sp.passes(S, B):
        sp.check_update_and_blend(net, p)
    net.close()


@pytest.mark.parametrize("S,B", [(16, 4), (16, 40), (24, 4)])
def test_bit_exact_after_fused_update_sites(ddq, S, B):
    """step(sgd, lr = 0, target_period = 1): K2 / K4 (S = 16; K4 applying the
    unit sums at B = 40) and the slab reduce (S = 24) rewrite every derived
    plane and copy, then blend, the target tower (sp.check_fused_sites)."""
    net = ddq.DeepQNet(batch=B, frame=S, gamma=sp.GAMMA)
    assert net.small_path()[0] == (S == 16)
    sp.fill_ring(net)
    for p0, p1 in zip(sp.passes(S, B), sp.passes(S, B, gamma=sp.GAMMA)):
        sp.check_fused_sites(net, p0, p1)
    net.close()


FORWARD_KINDS = [k for k in sp.KINDS if k[0] in "KP"]

# "tower": a small-path context (S = 16) acts with the tower kernel whatever
# the acting path says.  "spread" / "batch": the two conv families of a
# general context; 24 and 40 leave ragged edge tiles in the spread conv2
# (8 x 8 tiles on 12 / 20) and conv3 (4 x 4 on 6 / 10).
ACTING = ([("tower", 16, 1), ("tower", 16, 3)]
          + [(path, S, n) for path in ("spread", "batch") for S, n in ((24, 1), (24, 3), (40, 2))])


@pytest.mark.parametrize("path,S,n", ACTING)
def test_acting_forward_bit_exact(ddq, path, S, n):
    net = ddq.DeepQNet(batch=n, frame=S)
    assert net.small_path()[0] == (path == "tower")
    if path != "tower":
        net.set_acting_path(path)
        assert net.acting_path == path
    npl = len(sp.placements(S))
    for i in range(0, max(npl, len(FORWARD_KINDS)), n):
        kinds = [FORWARD_KINDS[m % len(FORWARD_KINDS)] for m in range(i, i + n)]
        p = sp.build_pass(S, n, kinds, first=i)
        want = sp.oracle(p)[0]["Q_out"]
        assert sp.exact32(want) and np.count_nonzero(want) == len(p.kinds)
        net.set_params(p.params)
        net.write_minibatch(*p.mb)
        net.forward_q()
        got = np.asarray(net.blob("Q_out")).reshape(n, 4)
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), (
            p.kinds, got, want, [sp.explain(g, w, p) for g, w in zip(got.ravel(), want.ravel())
                                 if g != w])
    net.close()


# ---------------------------------------------------------------- frames contract
@pytest.mark.parametrize("S,B", [(16, 4), (24, 2)])
def test_write_minibatch_refuses_frames_bf16_cannot_hold(ddq, S, B):
    """frames / 3 through write_minibatch: conv1 would read one bf16 plane of
    them (an error of 2^-9 per value, no error code); the call refuses."""
    net = ddq.DeepQNet(batch=B, frame=S)
    sp.check_frames_contract(net, S, B)
    net.close()


@pytest.mark.parametrize("S,B", [(16, 4), (24, 2)])
def test_bf16_exact_half_integers_pass(ddq, ref, S, B):
    pQ, pP = ref.init_params(S, seed=7, prefix="Q"), ref.init_params(S, seed=8, prefix="P")
    for p in (pQ, pP):
        for k in p:
            p[k][0] = (p[k][0] * 3).astype(np.float32)
    net = ddq.DeepQNet(batch=B, frame=S)
    params = dict(pQ)
    params.update(pP)
    net.set_params(params)
    mb = sp.half_integer_inputs(S, B)
    net.write_minibatch(*mb)
    net.forward_backward()
    check_full_pass(ref, net, pQ, pP, mb, quiet=True)
    net.close()
