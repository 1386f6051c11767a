"""The restatement of the device index draw alone, at the large-batch cases of
tests/_large_batch.py: every set the GPU tests expect (the seven draw cases and
every draw of the step, exchange and monitor chains at B > 256) is sorted,
distinct, in the valid prefix and free of forbidden slots; the restatement finds
it within ROUND_CAP = 1024 rounds (the kernel gives up after 4096); and the
n-step and the actor-pool restatements agree at n = 1 for B = 257 and 1024.
"""
import numpy as np
import pytest

import _large_batch as lb
import _nstep_ref as nr
import _pool_host as ph


def check(seed, ctr, B, cap, lanes, head, valid, n):
    L = cap // lanes
    idx, rounds = nr.draw_sorted_wide(seed, ctr, B, head, valid, lanes, L, n, with_rounds=True)
    assert idx.shape == (B,) and idx.dtype == np.int32
    nr.check_allowed(idx, head, valid, lanes, L, n)
    assert 1 <= rounds <= lb.ROUND_CAP, (seed, ctr, rounds)
    np.testing.assert_array_equal(nr.draw(seed, ctr, B, head, valid, lanes, L, n), idx)
    return idx, rounds


@pytest.mark.parametrize("case", lb.DRAW_CASES, ids=lb.case_id)
def test_draw_cases_are_legal_and_within_the_round_cap(case):
    B, cap, lanes, head, valid, n = case
    seen, rounds = set(), []
    for ctr in range(lb.DRAWS):
        idx, r = check(lb.SEED, ctr, B, cap, lanes, head, valid, n)
        seen |= {int(i) for i in idx}
        rounds.append(r)
    print("B %d valid %d x %d n %d: %d..%d rounds" % (B, lanes, valid, n, min(rounds), max(rounds)))
    allowed = set(nr.allowed_slots(head, valid, cap // lanes, n, lanes))
    assert seen <= allowed
    if len(allowed) == B:                      # (300, 301): every allowed slot, every draw
        assert seen == allowed
    else:
        assert len(seen) > B                   # the draws differ


@pytest.mark.parametrize("chain", lb.CHAINS, ids=[c[0] for c in lb.CHAINS])
def test_chain_draws_are_legal_and_within_the_round_cap(chain):
    _, seed, first, draws, B, cap, lanes, head, valid, n = chain
    assert B > 256 and lanes * valid >= 2 * B
    for ctr in range(first, first + draws):
        check(seed, ctr, B, cap, lanes, head, valid, n)


def test_round_count_is_the_loop_of_the_draw():
    """with_rounds changes nothing about the set, in either restatement, and a
    population with nothing to redraw takes exactly one (checking) round."""
    for f, extra in ((ph.draw_sorted_wide, ()), (nr.draw_sorted_wide, (1,))):
        a = f(3, 0, 72, 5, 200, 1, 200, *extra)
        b, rounds = f(3, 0, 72, 5, 200, 1, 200, *extra, with_rounds=True)
        np.testing.assert_array_equal(a, b)
        assert rounds >= 1
    idx, rounds = ph.draw_sorted_wide(3, 0, 65, 0, 1 << 30, with_rounds=True)
    assert rounds == 1 and (np.diff(idx) > 0).all()


@pytest.mark.parametrize("B", [257, 1024])
def test_restatements_agree_at_n1(B):
    for seed, ctr, head, valid, lanes in [(5, 0, 0, 2 * B, 1), (6, 4, 100, 2 * B + 3, 1),
                                          (7, 9, 3, B, 3), (8, 1, 1, B + 76, 1)]:
        L = valid + 1
        np.testing.assert_array_equal(nr.draw_sorted_wide(seed, ctr, B, head, valid, lanes, L, 1),
                                      ph.draw_sorted_wide(seed, ctr, B, head, valid, lanes, L))
