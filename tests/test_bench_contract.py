"""CPU: bench.py keeps its command-line contract and refuses to run without a GPU (no CPU path)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_flags_and_no_gpu_exit():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--streams", "--workload", "--dump-outputs"):
        assert flag in out.stdout
    import torch
    if torch.cuda.is_available():
        return
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert "no CPU path" in (out.stderr + out.stdout)
    assert out.stdout.strip() == ""          # nothing but the JSON line ever goes to stdout


def test_probe_blocks_partition_the_stream_in_single_gpu_order():
    """bench.first_probe (BASELINE config 4's sharding): over all (rank, stream) of a round the blocks are
    disjoint, contiguous and in stream order, rounds follow each other without gaps, and the union over
    ranks is what one GPU with world * streams engines would have drawn."""
    sys.path.insert(0, ROOT)
    import bench
    for world, streams, nb in ((1, 3, 256), (8, 3, 256), (4, 2, 64), (2, 1, 100)):
        starts = []
        for step in range(3):
            for rank in range(world):
                for e in range(streams):
                    starts.append(bench.first_probe(step, world, rank, streams, e, nb))
        assert starts == [k * nb for k in range(3 * world * streams)]
        one_gpu = [bench.first_probe(step, 1, 0, world * streams, e, nb)
                   for step in range(3) for e in range(world * streams)]
        assert one_gpu == starts


def test_steps_below_one_are_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2
    assert "--steps must be at least 1" in out.stderr
    assert out.stdout.strip() == ""


def test_dump_outputs_writes_float64_arrays_within_the_budget(tmp_path):
    """bench.dump_outputs: one DIR/<name>.npy per array, float64, values unchanged; more than the
    64 MB budget in all is refused before anything is written."""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    e = np.array([1.5 - 2.0j, -0.25 + 0.125j])
    bench.dump_outputs(str(tmp_path / "d"), {"estimates": np.stack([e.real, e.imag], axis=1),
                                             "iterations_fine": np.array([7, 9], dtype=np.int32)})
    assert sorted(os.listdir(tmp_path / "d")) == ["estimates.npy", "iterations_fine.npy"]
    est = np.load(tmp_path / "d" / "estimates.npy")
    its = np.load(tmp_path / "d" / "iterations_fine.npy")
    assert est.dtype == np.float64 and its.dtype == np.float64
    assert np.array_equal(est[:, 0] + 1j * est[:, 1], e) and its.tolist() == [7.0, 9.0]
    big = np.zeros(bench.DUMP_BUDGET_BYTES // 8 + 1)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": big})
    assert not os.path.exists(tmp_path / "big")


def test_full_is_an_option_and_off_by_default(monkeypatch):
    """--full gates everything beyond the headline (bench.run: full_records); a plain command line leaves
    it off, and the switches that trim a --full run stay accepted without it."""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--no-cpu-baseline", "--no-f32-line", "--no-other-configs",
                                      "--no-large-stencil"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--steps", "3"])
    args = bench.parse()
    assert args.full is True and args.steps == 3
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout
