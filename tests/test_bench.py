"""bench.py's command line: --dump-outputs (what the last timed step left, as
.npy files, identical from run to run) and the plain / --full split of the
result line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"theta_q", "theta_p", "grads", "optimizer_state",
         "Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss"}


class FakeNet:
    """The reads dump_outputs makes, on host arrays of P parameters."""

    def __init__(self, P, B=4):
        r = np.random.default_rng(7)
        self.flat = {k: r.standard_normal(P).astype(np.float32)
                     for k in ("theta_q", "theta_p", "grads", "optimizer_state")}
        self.blobs = {"Q_out": (B, 4, 1, 1), "P_out": (B, 4, 1, 1), "Q_sa": (B, 1, 1, 1),
                      "P_sa": (B, 1, 1, 1), "target_Q_sa": (B, 1, 1, 1), "loss": ()}
        self.blobs = {k: r.standard_normal(s).astype(np.float32) for k, s in self.blobs.items()}

    def get_flat(self, which):
        return self.flat["theta_p" if which else "theta_q"]

    def get_grads_flat(self):
        return self.flat["grads"]

    def optimizer_state(self):
        return self.flat["optimizer_state"]

    def blob(self, name):
        return self.blobs[name]


def load_dir(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path)}


def test_dump_outputs_whole_arrays(tmp_path):
    import bench
    net = FakeNet(1000)
    bench.dump_outputs(net, str(tmp_path / "d"))
    got = load_dir(str(tmp_path / "d"))
    assert set(got) == NAMES
    for k, a in got.items():
        want = net.flat[k] if k in net.flat else net.blobs[k]
        assert a.dtype == np.float32 and np.array_equal(a, want), k


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    """Past the budget every large array is the same seeded sample of its
    elements, in index order; small arrays stay whole."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4 * 2000)
    net = FakeNet(1000)
    bench.dump_outputs(net, str(tmp_path / "a"))
    bench.dump_outputs(net, str(tmp_path / "b"))
    a, b = load_dir(str(tmp_path / "a")), load_dir(str(tmp_path / "b"))
    assert set(a) == NAMES
    assert sum(v.nbytes for v in a.values()) <= 4 * 2000
    for k in NAMES:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
        if k in net.blobs:
            assert np.array_equal(a[k], net.blobs[k]), k
            continue
        assert 400 <= a[k].size < 1000, (k, a[k].size)
        src, j = net.flat[k], 0
        for v in a[k]:              # a subsequence of the source, in its order
            while j < src.size and src[j] != v:
                j += 1
            assert j < src.size, k
            j += 1


def run_bench(*extra):
    env = dict(os.environ)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "9", "--warmup", "2", *extra],
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """A plain run: the headline fields, none of the --full legs, and the same
    outputs bit for bit from two runs with the same arguments."""
    a = run_bench("--dump-outputs", str(tmp_path / "a"))
    b = run_bench("--dump-outputs", str(tmp_path / "b"))
    assert a["steps"] == 9 and a["warmup"] == 2
    assert a["unit"] == "updates/s" and a["higher_is_better"] is True and a["dtype"] == "f32"
    assert a["ms_per_step"] > 0
    assert abs(a["value"] * a["ms_per_step"] / 1e3 - 1) < 0.01      # one GPU: value = 1 / step time
    for leg in ("roofline", "kernels_us", "kernel_roofline", "step_ms_distribution",
                "gather_stress", "deepq16", "frame_sweep", "messaging", "cpu_baseline",
                "exchange_paths"):
        assert leg not in a, leg
    da, db = load_dir(str(tmp_path / "a")), load_dir(str(tmp_path / "b"))
    assert set(da) == NAMES
    assert sum(v.nbytes for v in da.values()) <= 64e6
    for k in NAMES:
        assert da[k].dtype == np.float32 and np.isfinite(da[k]).all(), k
        assert np.array_equal(da[k], db[k]), k
    assert float(da["loss"].reshape(())) == a["final_loss"] == b["final_loss"]
    assert np.any(da["grads"] != 0) and np.any(da["theta_q"] != da["theta_p"])
