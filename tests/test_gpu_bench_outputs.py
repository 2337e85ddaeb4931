"""GPU: `bench.py --dump-outputs DIR` writes what the timed path returned in its last timed step,
and those arrays are the ones the result line was computed from; a plain run prints the headline
alone within its time budget, `--full` adds the records that take runs of their own."""
import json
import os
import subprocess
import sys
import time

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


HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup",
                 "n_gpus", "config"}
# what takes runs of its own after the timed region: only with --full
FULL_KEYS = {"value_reference_stopping_point", "value_probes_resident", "value_pcie_inclusive_this_rank",
             "probe_generation_ms_per_batch", "f32_preconditioner", "roofline", "stencil_roofline",
             "kernel_rooflines", "step_breakdown_ms", "stencil_roofline_1024", "cpu_baseline", "other_configs"}


def _bench(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"]
    t0 = time.perf_counter()
    out = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1                      # one JSON line on stdout, whatever the mode
    return json.loads(lines[0]), wall


def test_plain_run_is_lean_and_full_adds_the_rest(tmp_path):
    """A plain run carries the headline and none of the records that take runs of their own, and spends at
    most 30 s outside its warm-up and timed steps (whole process, start to exit); --full adds those records
    to the same headline keys."""
    plain, wall = _bench(tmp_path)
    assert HEADLINE_KEYS <= set(plain) and not FULL_KEYS & set(plain)
    assert plain["full"] is False
    assert plain["metric"] == "hutchinson_probe_samples_per_sec_schwinger128"
    assert plain["unit"] == "probe-samples/s" and plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert plain["value"] > 0.0 and plain["ms_per_step"] > 0.0
    outside = wall - (plain["steps"] + plain["warmup"]) * plain["ms_per_step"] * 1e-3
    print("plain run: %.2f s from start to exit, %.2f s outside its steps" % (wall, outside))
    assert outside <= 30.0
    # the CPU baseline alone takes minutes: the other records show that --full still fills the line
    full, _ = _bench(tmp_path, "--full", "--no-cpu-baseline")
    assert full["full"] is True
    assert set(plain) <= set(full) and FULL_KEYS - {"cpu_baseline"} <= set(full)
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert full[key] == plain[key]
    # the same timed steps: the same probes solved to 1e-13 relative residual in both runs
    assert np.allclose(full["config"]["trace_estimate"], plain["config"]["trace_estimate"], rtol=0.0,
                       atol=1e-9 * plain["config"]["std_dev"])
    assert full["kernel_rooflines"] and full["roofline"] == full["kernel_rooflines"][0]
    assert full["value_reference_stopping_point"] > 0.0 and full["f32_preconditioner"]["value"] > 0.0
    assert not any("error" in v for v in full["other_configs"].values() if isinstance(v, dict))
