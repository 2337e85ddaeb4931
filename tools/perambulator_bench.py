#!/usr/bin/env python3
"""Cost of the perambulators (sw_perambulators) in one process on schwinger128: HIP-event time (the engine's
per-launch event buckets, summed) and wall time of one 256-column block at N = 32 (four source timeslices) and at
N = 128 (one), the tuned solver hierarchy of the drop-in flow, median of --reps.  The distillation kernels' own class
(k_laph_sources + k_laph_project) is reported with its share of the block's device time and held against the bar
of 10 % that DESIGN 4d set for a mode's own kernels.  k_laph_project alone on a 256-column block (sw_apply_laph_project,
one launch) is timed against the 30 us that one read of the 134 MB block takes at the stencil's 4.4 TB/s; the ratio is
recorded, not asserted.  Last, the wall time of all 128 source timeslices at N = 32 (8192 columns in 32 calls of
four timeslices, as distilled_two_point() issues them), profiling off.
python tools/perambulator_bench.py [--reps 7] [--out FILE]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_NUM_THREADS", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--t0", type=int, default=5)
    ap.add_argument("--stop-factor", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from deflatedmlmc_schwinger_amd import gateway, matrix, utils
    from deflatedmlmc_schwinger_amd.engine import KCLASS_LAPH, TIMER_NAMES
    from deflatedmlmc_schwinger_amd.hierarchy import detect_lattice
    from deflatedmlmc_schwinger_amd.multigrid import MG
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "hutchinson")
    mg = MG(A)
    with contextlib.redirect_stdout(io.StringIO()):
        mg.setup(dof=tp['dof'], aggrs=tp['aggrs'], max_levels=tp['max_nr_levels'], dim=2,
                 acc_eigvs=tp['accuracy_mg_eigvs'], sys_type='schwinger', params=tp)
    eng = mg.engine
    n, L = A.shape[0], 128
    eng.set_option("stop_factor", args.stop_factor)
    Vall, _ = utils.laplacian_eigenvectors(detect_lattice(A)[2], L, L)
    tol, maxiter = 1e-12, 1000
    rng = np.random.default_rng(7)
    Z = rng.standard_normal((256, n)) + 1j * rng.standard_normal((256, n))
    block_mb = 256 * n * 16 / 1e6
    read_us = block_mb / 4.4                                  # MB / (TB/s) = us
    out = {"lattice": "schwinger128", "reps": args.reps, "stop_factor": args.stop_factor, "tol": tol,
           "block_columns": 256, "block_MB": block_mb, "one_read_at_4.4_TB_per_s_us": read_us}
    eng.set_profiling(True)
    for nev in (32, 128):
        V = np.ascontiguousarray(Vall[:, :nev])
        eng.set_distillation(V)
        t0s = [(args.t0 + s) % L for s in range(256 // (2 * nev))]
        dev, wall, cls, proj = [], [], [], []
        buckets, launches, iters = None, None, None
        for rep in range(args.warmup + args.reps):
            eng.timers_reset()
            t1 = time.perf_counter()
            _, it = eng.perambulators(t0s, tol, maxiter)
            eng.sync()
            w = (time.perf_counter() - t1) * 1e3
            t = eng.timers()
            ms, cnt = eng.kernel_stats(KCLASS_LAPH)
            eng.timers_reset()
            eng.apply_laph_project(Z)
            pms, pcnt = eng.kernel_stats(KCLASS_LAPH)
            work = eng.kernel_work(KCLASS_LAPH)
            assert cnt == 2 and pcnt == 1
            if rep >= args.warmup:
                dev.append(sum(t.values()))
                wall.append(w)
                cls.append(ms)
                proj.append(pms)
                buckets, launches, iters = t, cnt, it
        d, p = float(np.median(dev)), float(np.median(proj))
        out["N%d" % nev] = {
            "source_timeslices": t0s, "device_ms": d, "device_ms_all": [round(v, 4) for v in dev],
            "wall_ms": float(np.median(wall)), "iters_min": int(iters.min()), "iters_max": int(iters.max()),
            "buckets_ms": {k: round(buckets[k], 4) for k in TIMER_NAMES}, "laph_launches": launches,
            "laph_ms": float(np.median(cls)), "laph_share": float(np.median(cls)) / d,
            "project_ms": p, "project_ms_all": [round(v, 4) for v in proj],
            "project_over_one_read": p * 1e3 / read_us, "project_share": p / d,
            "project_flops": work, "project_TF_per_s": work / (p * 1e-3) / 1e12,
            "eigenvector_MB": V.size * 16 / 1e6}
    eng.set_profiling(False)

    # all 128 source timeslices at N = 32: 32 calls of four timeslices, as the flow issues them
    eng.set_distillation(np.ascontiguousarray(Vall[:, :32]))
    eng.perambulators([0, 1, 2, 3], tol, maxiter)
    walls = []
    for _ in range(3):
        eng.sync()
        t1 = time.perf_counter()
        total = 0
        for first in range(0, L, 4):
            _, it = eng.perambulators(list(range(first, first + 4)), tol, maxiter)
            total += int(it.sum())
        walls.append(time.perf_counter() - t1)
    out["all_128_sources_N32"] = {"columns": 2 * 32 * L, "calls": L // 4, "wall_s": float(np.median(walls)),
                                  "wall_s_all": [round(v, 4) for v in walls], "iterations": total,
                                  "extrapolated_s": 32 * 7.1e-3}
    eng.set_distillation(None)
    out["bars"] = {"laph_share_max": 0.10,
                   "met": bool(max(out["N32"]["laph_share"], out["N128"]["laph_share"]) <= 0.10)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
