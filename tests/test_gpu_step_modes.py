"""One context through every single-ctx step mode, a cfg change and the events
that invalidate its captured graphs, against a context that only ever takes
eager steps.

The other GPU suites pin each mode against another on separate contexts.  Here
net A switches between ``step``, ``step_graph`` and ``step_pipelined`` under one
cfg, then under a second cfg (another lr: every exec is recaptured), then after
``index_log_enable`` or ``set_objective`` (the captured kernels held the old log
pointer / lacked the extra forward: every exec is dropped).  Net B takes the same
steps with ``step(cfg)`` alone.  The graph modes replay the launches of the eager
step on device-side counters, so the two nets are held bit-identical, as
tests/test_gpu_chain.py holds the pipelined chain to eager steps.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, B, N = 16, 16, 300


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


def two_nets(ddq, ref, S=S, B=B):
    rng = np.random.default_rng(21)
    nets = [ddq.DeepQNet(batch=B, frame=S) for _ in range(2)]
    theta = ref.flatten(ref.init_params(S, seed=6))
    st = rng.integers(0, 256, (N, 4, S, S)).astype(np.uint8)
    acts = rng.integers(0, 4, N).astype(np.uint8)
    rws = rng.integers(-1, 2, N).astype(np.int16)
    nts = (rng.random(N) > 0.1).astype(np.uint8)
    for n in nets:
        n.set_flat(0, theta)
        n.set_flat(1, theta)
        n.replay_create(N)
        n.replay_import(st, acts, rws, nts, 0, N)
    return nets


def eager(net, cfg, k):
    for _ in range(k):
        net.step(cfg)


def assert_same_state(a, b, first, ndraws):
    """theta Q and P, the optimizer state, the bound indices and the ndraws index
    sets logged from draw `first`, bit for bit."""
    for n in (a, b):
        n.synchronize()
        assert n.replay_draws() == first + ndraws
    for which in (0, 1):
        th = a.get_flat(which)
        assert np.all(np.isfinite(th))
        np.testing.assert_array_equal(th, b.get_flat(which))
    np.testing.assert_array_equal(a.optimizer_state(), b.optimizer_state())
    np.testing.assert_array_equal(a.read_indices(), b.read_indices())
    np.testing.assert_array_equal(a.index_log(first, ndraws), b.index_log(first, ndraws))


def test_mode_switches_cfg_change_and_index_log_match_eager_steps(ddq, ref):
    """39 steps: P <- Q every 3, so syncs fall inside the 8-step execs and tails."""
    a, b = two_nets(ddq, ref)
    cfg1 = a.step_cfg("rmsprop", lr=1e-4, target_period=3, seed=5)
    cfg2 = a.step_cfg("rmsprop", lr=2e-4, target_period=3, seed=5)
    eager(a, cfg1, 2)
    a.step_graph(cfg1, 9)        # one 8-step exec plus a single
    a.step_pipelined(cfg1, 11)   # an 8-step exec plus a 3-step tail
    a.step_graph(cfg1, 1)        # recaptured: capturing the pipelined execs dropped it
    a.step_pipelined(cfg2, 2)    # the cfg changed: nothing captured under cfg1 may replay
    a.step_graph(cfg2, 3)
    eager(b, cfg1, 23)
    eager(b, cfg2, 5)
    for n in (a, b):
        assert n.replay_draws() == 28
        n.index_log_enable(64)   # the captured kernels hold the old (null) log pointer
    a.step_pipelined(cfg2, 10)
    eager(a, cfg2, 1)
    eager(b, cfg2, 11)
    assert_same_state(a, b, 28, 11)


def test_objective_change_between_graph_steps_matches_eager_steps(ddq, ref):
    """The graph captured after set_objective holds the Double target's extra
    forward and the Huber head; the one captured before it is gone."""
    a, b = two_nets(ddq, ref)
    cfg = a.step_cfg("rmsprop", lr=1e-4, target_period=3, seed=5)
    for n in (a, b):
        n.index_log_enable(64)
    a.step_graph(cfg, 2)
    eager(b, cfg, 2)
    for n in (a, b):
        n.set_objective(target="double", loss="huber")
    a.step_graph(cfg, 9)
    eager(b, cfg, 9)
    assert_same_state(a, b, 0, 11)


# Regimes of the step plan (csrc/step_plan.h, DESIGN.md "The step plan") that no
# other GPU suite runs.  (S, B, exchange, overlap): the general kernels with the
# one-launch draw under the overlapped all-reduce of a 1-rank communicator --
# fc4 applied by the slab-reduce launch after its bucket's all-reduce, the rest
# by the apply launch, the next draw in the head launch (the other suites run
# the overlap on the small path, or past 256 images with the side-stream draw).
PLAN_REGIMES = [(24, 8, "allreduce", True)]


@pytest.mark.parametrize("S,B,exchange,overlap", PLAN_REGIMES)
def test_exchanged_regime_through_the_modes_matches_eager_steps(ddq, ref, S, B, exchange, overlap):
    """Net A: the exchange over its 1-rank communicator, through every mode.  Net
    B: no exchange, eager steps alone (a sum over one rank is the identity)."""
    a, b = two_nets(ddq, ref, S, B)
    a.comm_init(ddq.DeepQNet.comm_unique_id(), 1, 0)
    for n in (a, b):
        n.index_log_enable(64)
    # (lr: rmsprop at 1e-4 leaves float32 range within four steps at S = 24, with
    # or without the exchange; tests/test_gpu_large_batch.py steps that frame at 1e-6)
    cfg_a = a.step_cfg("rmsprop", lr=1e-6, target_period=3, exchange=exchange, overlap=overlap,
                       seed=5)
    cfg_b = b.step_cfg("rmsprop", lr=1e-6, target_period=3, seed=5)
    eager(a, cfg_a, 2)
    a.step_graph(cfg_a, 9)        # one 8-step exec plus a single
    a.step_pipelined(cfg_a, 11)   # an 8-step exec plus a 3-step tail
    eager(a, cfg_a, 1)
    eager(b, cfg_b, 23)
    assert_same_state(a, b, 0, 23)
    assert a.get_flat(0).tobytes() != a.get_flat(1).tobytes()   # steps 22, 23 after the sync at 21
    for n in (a, b):
        n.close()
