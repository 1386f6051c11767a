"""The acting forward (launch_act in csrc/kernels.hip: ddq_forward_q,
ddq_select_action, the Double-DQN Qn_out pass, the device environments) on the
GPU against the float64 oracle, by the recipe of tests/_acting_ref.py.

It is a path of its own: one tower (nz = 1) at n <= B images in the shared
act_* scratch, every grid derived from n, ending in fc4_reduce_out_kernel,
which no training step runs; at S = 16 the small-map tower kernel at nz = 1
(two-workgroup split form through n = 128, whole form through 256).

a. Values on a ctx of batch n: Q_out after ``forward_q`` under the three rules
   of tests/_parity.py, at every frame 16..128 / 8, across launch_fc4_fwd's
   switch after n = 32 with ragged 64-image tiles, and across the tower forms.
b. Actions of n states on a ctx of batch B > n whose scratch holds another
   batch: the argmax kernel exact on the ctx's own Q_out, the B-ctx bit-equal
   to the n-ctx, every decided state on the oracle's action.
c. The first maximum wins an exact tie.
d. Acting changes nothing a training pass left behind.
e. The harness rejects swapped, scaled and zeroed rows of the GPU's own output
   and swapped actions.
"""
import numpy as np
import pytest

import _acting_ref as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


# ----------------------------------------------------------------- a. values
@pytest.mark.parametrize("S,n,kind", ar.VALUE_CASES, ids=ar.ids(ar.VALUE_CASES))
def test_forward_q_values(ddq, ref, S, n, kind):
    c = ar.case(ref, S, n, kind, mags=True)
    net = ar.make_net(ddq, n, S, c["pQ"])
    assert net.small_path()[0] == (S == 16 and n <= 256)
    err = ar.forward_values(net, c, what="(%d, %d, %s) " % (S, n, kind))
    print("acting parity | %d | %d | %s | %.3g |" % (S, n, kind, err))
    net.synchronize()
    net.close()


# ---------------------------------------------------------------- b. actions
@pytest.mark.parametrize("S,B,n,kind", ar.ACTION_CASES, ids=ar.ids(ar.ACTION_CASES))
def test_select_action_n_below_batch(ddq, ref, S, B, n, kind):
    c = ar.case(ref, S, n, kind)
    a = ar.check_actions(ddq, c, S, B, what="(%d, %d, %d, %s) " % (S, B, n, kind))
    print("actions (%d, %d, %d, %s): %s, %d undecided"
          % (S, B, n, kind, np.bincount(a, minlength=4).tolist(), int((~c["decided"]).sum())))


# ------------------------------------------------------------------- c. ties
@pytest.mark.parametrize("S,n,kind", ar.TIE_CASES, ids=ar.ids(ar.TIE_CASES))
def test_first_max_wins_a_tie(ddq, ref, S, n, kind):
    wins = ar.check_ties(ddq, ar.case(ref, S, n, kind), S)
    print("tie (%d, %d): the tied pair on top for %d states" % (S, n, wins))
    assert wins >= 2


# --------------------------------------------------- d. training left alone
def snapshot(net):
    out = {k: net.blob(k).copy() for k in ("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss",
                                           "Q_out.diff")}
    out["grads"] = net.get_grads_flat()
    for i in (1, 2, 3):
        out["mask%d" % i] = net.pool_mask(i)
    for k, v in zip(("state", "action", "reward", "next_state", "non_terminal"),
                    net.read_minibatch()):
        out[k] = v
    out["theta_Q"], out["theta_P"] = net.get_flat(0), net.get_flat(1)
    return out


@pytest.mark.parametrize("S,B", [(16, 8), (64, 4)])
def test_acting_leaves_training_alone(ddq, ref, S, B):
    from test_gpu_parity import make_inputs, make_params
    rng = np.random.default_rng(600 + S + B)
    pQ, pP = make_params(ref, rng, S, "x3")
    mb = make_inputs(rng, B, S, "uniform")
    acted, plain = [ddq.DeepQNet(batch=B, frame=S) for _ in range(2)]
    for net in (acted, plain):
        params = dict(pQ)
        params.update(pP)
        net.set_params(params)
        net.reset_optimizer()
        net.write_minibatch(*mb)
        net.forward_backward()
    before = snapshot(acted)
    assert np.count_nonzero(before["grads"]) > before["grads"].size // 10
    a_full = acted.select_action(ar.other_states(S, B, B))
    a_part = acted.select_action(ar.other_states(S, B, B - 1)[:B - 1])
    assert a_full.shape == (B,) and a_part.shape == (B - 1,)
    after = snapshot(acted)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    for net in (acted, plain):
        net.apply("rmsprop", lr=1e-4)
    np.testing.assert_array_equal(acted.get_flat(0), plain.get_flat(0))
    np.testing.assert_array_equal(acted.get_flat(1), plain.get_flat(1))
    np.testing.assert_array_equal(acted.optimizer_state(), plain.optimizer_state())
    assert not np.array_equal(acted.get_flat(0), before["theta_Q"])
    for net in (acted, plain):
        net.synchronize()
        net.close()


# --------------------------------------------------- e. the harness can fail
def test_harness_rejects_mutated_output(ddq, ref):
    """On the GPU's own Q_out and actions of case (64, 33): accepted as they
    are; two rows swapped, a row x 1.001, a row zeroed and two actions swapped
    are each rejected."""
    S, n, kind = ar.MUTATION_CASE
    c = ar.case(ref, S, n, kind, mags=True)
    net = ar.make_net(ddq, n, S, c["pQ"])
    ar.forward_values(net, c, what="(%d, %d, %s) " % (S, n, kind))
    q = ar.q_out(net)
    net.set_params(c["pC"])
    a = net.select_action(c["states"])
    assert ar.check_mutations(q, c, actions=a) == 4
    net.synchronize()
    net.close()
