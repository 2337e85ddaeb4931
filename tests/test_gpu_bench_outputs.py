"""GPU: `bench.py --dump-outputs DIR` writes what the timed path returned in its last timed step,
and those arrays are the ones the result line was computed from."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dumped_outputs_are_those_of_the_timed_step(tmp_path):
    d = tmp_path / "out"
    # one timed step: the statistics of the timed region are those of the dumped estimates alone
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
           "--no-cpu-baseline", "--no-f32-line", "--no-other-configs", "--no-large-stencil",
           "--dump-outputs", str(d)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip())
    assert line["steps"] == 1 and line["ms_per_step"] > 0.0
    names = sorted(os.listdir(d))
    assert names == ["estimates.npy", "iterations_coarse.npy", "iterations_fine.npy", "trace_estimate.npy",
                     "trace_statistics.npy"]
    arrays = {n[:-4]: np.load(d / n) for n in names}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    est = arrays["estimates"]
    nb = line["config"]["probes_per_step_per_gpu"]
    assert est.shape == (nb, 2) and np.isfinite(est).all() and np.abs(est).max() > 0.0
    assert arrays["iterations_fine"].shape == (nb,)
    assert arrays["iterations_fine"].max() == line["config"]["outer_iterations_max"]
    stats = arrays["trace_statistics"]
    assert stats[3] == nb
    scale = np.abs(est).sum()
    assert abs(stats[0] - est[:, 0].sum()) <= 1e-13 * scale
    assert abs(stats[1] - est[:, 1].sum()) <= 1e-13 * scale
    tr = arrays["trace_estimate"]
    assert tr[:2].tolist() == line["config"]["trace_estimate"] and tr[2] == line["config"]["std_dev"]
