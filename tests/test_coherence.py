"""The coherence harness (tests/_coherence.py) on the CPU twin.

The twin keeps theta alone, no split planes, so nothing can go stale there: this
pass checks the harness itself -- the probe's plumbing, the tower-1 expectations
at 2, 3 and 4 updates, the host paths, and that the mutants are told apart -- and
keeps it importable and exercised without a GPU.  The regimes are the ones the
twin has (tests/test_cpu_twin.py, tests/test_adam.py): the separate apply under
every rule, updates driven from the host (replay_sample, forward_backward, apply,
sync_target: the twin takes no ddq_step), the Double + Huber objective, and the
host paths.  The step modes, the exchanges and device-drawn prioritized replay
are GPU-only calls (they refuse with DDQ_ESTATE, test_gpu_only_calls_refuse) and
run in tests/test_gpu_coherence.py.
"""
import pytest

import _coherence as co
from _twin import ddq_with_cpu_lib

SHAPES = [(16, 8), (24, 4)]
SHAPE_IDS = ["S%d-B%d" % s for s in SHAPES]


@pytest.fixture(scope="module")
def ddq():
    return ddq_with_cpu_lib()


@pytest.mark.parametrize("k", co.PROBES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("rule", co.APPLY_RULES)
def test_apply(ddq, rule, shape, k):
    S, B = shape
    key = "cpu apply %s S%d B%d" % (rule, S, B)
    co.check_regime(ddq, key, lambda n: co.run_apply(ddq, S, B, rule, n, "cpu"), k,
                    p_fixed=co.theta0(S, seed=43))


@pytest.mark.parametrize("k", co.PROBES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("objective", [None, ("double", "huber", 0.5)], ids=["max", "double-huber"])
def test_host_loop(ddq, objective, shape, k):
    S, B = shape
    key = "cpu host loop %s S%d B%d" % (objective, S, B)
    co.check_regime(ddq, key, lambda n: co.run_host_loop(ddq, S, B, n, "cpu", objective), k)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("path", co.HOST_PATHS)
def test_host_paths(ddq, path, shape):
    S, B = shape
    net, = co.run_host_loop(ddq, S, B, 4, "cpu")
    try:
        co.check_host_path(ddq, net, path, "cpu %s S%d B%d" % (path, S, B))
    finally:
        net.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mutants_are_detected(ddq, shape):
    co.check_mutants(ddq, "cpu host loop None S%d B%d" % shape,
                     lambda n: co.run_host_loop(ddq, shape[0], shape[1], n, "cpu"))
