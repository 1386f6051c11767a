"""The acting recipe (tests/_acting_ref.py) without a GPU.

* Its conditions hold for every case tests/test_gpu_acting.py puts to the
  oracle -- few undecided states, the oracle's actions spread over the four --
  asserted on the float64 oracle alone.
* The checks themselves run through the CPU twin (``DeepQNet(mode="cpu")``) at
  (16, 5) and (24, 3), each beside a ctx of batch 8: the values under the three
  rules of tests/_parity.py, the three action rules, the exact tie, and the
  mutations the harness must reject.
"""
import numpy as np
import pytest

import _acting_ref as ar
from _twin import ddq_with_cpu_lib
from oracle import ref_numpy as ref


@pytest.fixture(scope="module")
def ddq():
    return ddq_with_cpu_lib()


@pytest.mark.parametrize("S,n,kind", ar.oracle_cases(), ids=ar.ids(ar.oracle_cases()))
def test_recipe_conditions_hold(S, n, kind):
    c = ar.case(ref, S, n, kind)          # (asserts them)
    dec, acts = c["decided"], c["actions"]
    print("case (%d, %d, %s): %d undecided, actions %s, margin %.3g, smallest decided gap %.3g"
          % (S, n, kind, int((~dec).sum()), np.bincount(acts, minlength=4).tolist(), c["margin"],
             float(np.min((np.sort(c["Qc"], axis=1)[:, -1] - np.sort(c["Qc"], axis=1)[:, -2])[dec]))
             if dec.any() else float("nan")))
    # centring moved one bias add and nothing else
    np.testing.assert_allclose(ar.forward64(ref, c["pC"], c["states"]), c["Qc"], rtol=0, atol=1e-9)
    if n > 1:
        assert abs(c["Qc"].mean(axis=0)).max() <= 1e-6 * max(1.0, abs(c["Q0"]).max())


def test_uncentred_parameters_cannot_tell_images_apart():
    """Why the action tests centre the bias: under the x3 parameters the 33
    uniform states of (16, 33) all pick one action."""
    pQ, _, states = ar.draw(ref, 16, 33, "u")
    assert len(set(np.argmax(ar.forward64(ref, pQ, states), axis=1).tolist())) == 1


def test_conditions_reject_a_case_that_cannot_see_a_swap():
    Q0 = np.tile(np.array([[0.0, 1.0, 3.0, 2.0]]), (20, 1))
    with pytest.raises(AssertionError):
        ar.conditions(Q0, Q0)                                  # one action
    Qc = Q0.copy()
    Qc[:5] = Qc[:5, ::-1]
    with pytest.raises(AssertionError):
        ar.conditions(Q0, Qc)                                  # two of four at n >= 16
    Qc = np.eye(4)[np.arange(20) % 4] * 1e-9
    with pytest.raises(AssertionError):
        ar.conditions(Q0, Qc)                                  # nothing decided


@pytest.mark.parametrize("S,B,n", ar.TWIN_SBN, ids=ar.ids(ar.TWIN_SBN))
def test_twin_values_and_mutations(ddq, S, B, n):
    c = ar.case(ref, S, n, "u", mags=True)
    net = ar.make_net(ddq, n, S, c["pQ"], mode="cpu")
    err = ar.forward_values(net, c, what="twin (%d, %d) " % (S, n))
    print("twin (%d, %d): normwise %.3g" % (S, n, err))
    assert net.small_path()[0] is False
    a = ar.check_actions(ddq, c, S, B, mode="cpu")
    assert ar.check_mutations(ar.q_out(net), c, actions=a if n >= 2 else None) == 4
    net.close()


@pytest.mark.parametrize("S,B,n", ar.TWIN_SBN, ids=ar.ids(ar.TWIN_SBN))
def test_twin_actions_n_below_batch(ddq, S, B, n):
    c = ar.case(ref, S, n, "u")
    a = ar.check_actions(ddq, c, S, B, mode="cpu", what="twin (%d, %d, %d) " % (S, B, n))
    assert len(set(a.tolist())) >= 2


@pytest.mark.parametrize("S,n,kind", ar.TWIN_TIE_CASES, ids=ar.ids(ar.TWIN_TIE_CASES))
def test_twin_first_max_wins_a_tie(ddq, S, n, kind):
    assert ar.check_ties(ddq, ar.case(ref, S, n, kind), S, mode="cpu") >= 1
