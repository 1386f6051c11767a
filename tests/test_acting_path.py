"""``set_acting_path`` on the CPU twin: stored, validated, and without effect on
what the twin computes."""
import numpy as np
import pytest

import _acting_ref as ar
from _twin import ddq_with_cpu_lib
from oracle import ref_numpy as ref


@pytest.fixture(scope="module")
def ddq():
    return ddq_with_cpu_lib()


def test_acting_path_on_the_twin(ddq):
    c = ar.case(ref, 24, 3, "u")
    net = ar.make_net(ddq, 3, 24, c["pQ"], mode="cpu")
    net.write_minibatch(state=c["states"])
    net.forward_q()
    q0 = ar.q_out(net).copy()
    assert net.acting_path == "batch"
    for path in ("spread", "auto", "batch"):
        net.set_acting_path(path)
        assert net.acting_path == path
        net.forward_q()
        np.testing.assert_array_equal(ar.q_out(net).view(np.uint32), q0.view(np.uint32))
    for bad in (3, -1):
        assert net.lib.ddq_set_acting_path(net.ctx, bad) == -1      # DDQ_EINVAL
    assert net.acting_path == "batch"
    with pytest.raises(ValueError):
        net.set_acting_path("wide")
    net.close()
