"""ddq_replay_set_augment (csrc/gather_shift.h) against numpy's edge pad + crop."""
import numpy as np
import pytest

import _augment_ref as ar
import _nstep_ref as nr
from test_gpu_nstep import ddq, done, make_net as base_net  # noqa: F401  (fixture and helpers)

pytestmark = pytest.mark.gpu

CAP, DRAWS = 12, 6
# 16: one run a row; 24, 40: rows only 8-byte aligned, a partial last run; 64: four runs
CASES = [(S, B, pad) for S, B in ((16, 4), (24, 3), (40, 2), (64, 2)) for pad in (1, 4)] + [(64, 2, 8)]


def make_net(ddq, S, B, ring, head, valid, pad=0, lanes=1, n=None, prio=False):
    net = base_net(ddq, S, ring, head, valid, lanes, n, batch=B)
    if prio:
        net.replay_set_priority()
    if pad:
        net.replay_set_augment(pad)
    return net


def seed_covering(B, pad):
    """The first seed whose shifts show both signs and a zero of dy and of dx (formula alone)."""
    def covers(s):
        sh = np.reshape([ar.shifts(s, d, B, pad) for d in range(DRAWS)], (-1, 2))
        return all({-1, 0, 1} <= set(np.sign(sh[:, k])) for k in (0, 1))
    return next(s for s in range(1, 4096) if covers(s))


def pattern(S, cap=CAP, terminals=nr.TERMINALS):
    _, ac, rw, nt = nr.build_ring(np.random.default_rng(S), cap, S, terminals)
    return ar.pattern_ring(cap, S), ac, rw, nt


@pytest.mark.parametrize("S,B,pad", CASES)
def test_gather_matches_reference(ddq, S, B, pad):
    ring, seed = pattern(S), seed_covering(B, pad)
    net, plain = make_net(ddq, S, B, ring, 5, CAP, pad), make_net(ddq, S, B, ring, 5, CAP)
    for d in range(DRAWS):
        net.replay_sample_device(seed)
        plain.replay_sample_device(seed)
        sh = net.blob("aug_shift").reshape(B, 4)
        assert np.array_equal(sh, ar.shifts(seed, d, B, pad)), d
        idx = net.read_indices()
        state, _, _, nxt, _ = nr.gather(ring, idx, CAP, 1)
        state, nxt = ar.augmented(state, nxt, sh)
        base = plain.read_minibatch()
        nr.assert_minibatch(net.read_minibatch(), (state, base[1], base[2], nxt, base[4]), d)
    done(net, plain)


def test_indices_unchanged(ddq):
    ring = pattern(16, cap=40, terminals=())
    nets = [make_net(ddq, 16, 4, ring, 7, 40, pad=p) for p in (4, 0)]
    for d in range(8):
        idx = [net.replay_sample_device(9) or net.read_indices() for net in nets]
        assert np.array_equal(idx[0], idx[1]) and nets[0].replay_draws() == d + 1
    done(*nets)


def test_nstep_and_lanes(ddq):
    S, B, pad, L = 16, 4, 4, 8
    ring = pattern(S, cap=2 * L, terminals=(3, 12))
    net = make_net(ddq, S, B, ring, 0, L, pad, lanes=2, n=3)
    ms = set()
    for d in range(DRAWS):
        net.replay_sample_device(5)
        sh = net.blob("aug_shift").reshape(B, 4)
        assert np.array_equal(sh, ar.shifts(5, d, B, pad)), d
        want = nr.gather(ring, net.read_indices(), L, 3, with_m=True)
        state, nxt = ar.augmented(want[0], want[3], sh)
        nr.assert_minibatch(net.read_minibatch(), (state, want[1], want[2], nxt, want[4]), d)
        ms |= set(want[5])
    assert min(ms) < 3 and 3 in ms
    done(net)


@pytest.mark.parametrize("S,B,prio", [(16, 8, False), (64, 4, False), (16, 8, True)])
def test_step_modes_identical(ddq, S, B, prio):
    ring = nr.build_ring(np.random.default_rng(3), 40, S, (9, 30))
    nets = [make_net(ddq, S, B, ring, 11, 40, pad=2, prio=prio) for _ in range(3)]
    cfg = nets[0].step_cfg("rmsprop", lr=1e-4, seed=21, target_period=4)
    for _ in range(6):
        nets[0].step(cfg)
    nets[1].step_graph(cfg, 6)
    nets[2].step_pipelined(cfg, 6)
    out = [(net.get_flat(0), net.get_flat(1), net.blob("aug_shift"), net.read_indices())
           + net.read_minibatch() for net in nets]
    assert np.array_equal(out[0][2].reshape(B, 4), ar.shifts(21, 5, B, 2))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes()
    done(*nets)


def test_off_is_off(ddq):
    from ddq import _lib
    ring = nr.build_ring(np.random.default_rng(4), 40, 16, (9,))
    never, back = (make_net(ddq, 16, 8, ring, 11, 40, pad=p) for p in (0, 2))
    cfg = never.step_cfg("rmsprop", lr=1e-4, seed=21, target_period=4)
    with pytest.raises(_lib.DDQError) as ei:            # the async exchange takes no augmentation
        back.async_begin(back.step_cfg(exchange="async"))
    assert ei.value.code == _lib.DDQ_EINVAL and "augmentation" in str(ei.value)
    back.replay_set_augment(0)
    assert [n for n, _ in back.profile_step(cfg)] == [n for n, _ in never.profile_step(cfg)]
    for net in (never, back):
        net.step(cfg)
        net.step_graph(cfg, 2)
        net.step_pipelined(cfg, 3)
    assert never.get_flat(0).tobytes() == back.get_flat(0).tobytes()
    for a, b in zip(never.read_minibatch(), back.read_minibatch()):
        assert a.tobytes() == b.tobytes()
    done(never, back)
