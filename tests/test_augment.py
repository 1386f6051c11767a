"""ddq_replay_set_augment on the CPU twin (its device draw is the prioritized one); the async
exchange's refusal is the device library's: tests/test_gpu_augment.py."""
import numpy as np
import pytest

import _augment_ref as ar
import _nstep_ref as nr
from test_nstep import code_of, ddq  # noqa: F401  (the twin's fixture: builds it if missing)

B, CAP, SEED = 4, 12, 77


def test_argument_checks(ddq):
    from ddq import _lib
    net = ddq.DeepQNet(batch=B, frame=16, mode="cpu")
    assert code_of(lambda: net.replay_set_augment(2)) == _lib.DDQ_ESTATE      # no ring
    assert code_of(net.replay_augment) == _lib.DDQ_ESTATE
    net.replay_create(CAP)
    assert net.replay_augment() == 0
    assert code_of(lambda: net.blob("aug_shift")) == _lib.DDQ_ESTATE          # off
    for bad in (-1, 9, 5):                                                     # 5 > 16 / 4
        assert code_of(lambda: net.replay_set_augment(bad)) == _lib.DDQ_EINVAL
    net.replay_set_augment(4)
    assert net.replay_augment() == 4
    net.close()


@pytest.mark.parametrize("pad", [1, 4])
@pytest.mark.parametrize("S", [16, 24])
def test_twin_gather_is_the_edge_padded_crop(ddq, S, pad):
    ring = (ar.pattern_ring(CAP, S),) + nr.build_ring(np.random.default_rng(S), CAP, S, nr.TERMINALS)[1:]
    net = ddq.DeepQNet(batch=B, frame=S, mode="cpu")
    net.replay_create(CAP)
    net.replay_import(*ring, 5, CAP)
    net.replay_set_priority()
    net.replay_set_augment(pad)
    for d in range(6):
        net.replay_sample_device(SEED)
        sh = net.blob("aug_shift").reshape(B, 4)
        assert np.array_equal(sh, ar.shifts(SEED, d, B, pad)), d
        want = nr.gather(ring, net.read_indices(), CAP, 1)
        state, nxt = ar.augmented(want[0], want[3], sh)
        nr.assert_minibatch(net.read_minibatch(), (state, want[1], want[2], nxt, want[4]), d)
    net.close()
