#!/usr/bin/env python3
"""Cost of the displaced traces next to the plain deflated Hutchinson batch, in one process on schwinger128:
HIP-event time (the engine's per-launch event buckets, summed) and wall time of a SW_MODE_HUTCHINSON batch and
of SW_MODE_HUTCHINSON_SHIFTS batches with S = 1, 16 and 128 shifts, nb probes resident in HBM, the tuned
solver hierarchy of the drop-in flow.  python tools/shift_dots_bench.py [--nb 256] [--reps 7] [--out FILE]"""
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
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stop-factor", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from deflatedmlmc_schwinger_amd import gateway, matrix, utils
    from deflatedmlmc_schwinger_amd.engine import MODE_HUTCHINSON, MODE_HUTCHINSON_SHIFTS, TIMER_NAMES
    from deflatedmlmc_schwinger_amd.multigrid import MG
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "hutchinson")
    mg = MG(A)
    with contextlib.redirect_stdout(io.StringIO()):
        mg.setup(dof=tp['dof'], aggrs=tp['aggrs'], max_levels=tp['max_nr_levels'], dim=2,
                 acc_eigvs=tp['accuracy_mg_eigvs'], sys_type='schwinger', params=tp)
        Ux, _ = utils.deflation_pre_computations(A, tp['nr_deflat_vctrs'], tp['defl_eigvs_tol_Hutch'],
                                                 "hutchinson", mg.timer, tp, mg)
    eng = mg.engine
    n, L = A.shape[0], int(tp['latt_dims'][0])
    W = np.asarray(mg.ml.levels[0].Pperm.transpose() * Ux)      # the vectors before Pperm
    eng.set_option("stop_factor", args.stop_factor)
    np.random.seed(123456)
    eng.probes_upload(0, utils.draw_probes(args.nb, n))
    tol, maxiter = 1e-12, 1000

    def measure(mode):
        dev, wall, buckets = [], [], None
        for rep in range(args.warmup + args.reps):
            eng.timers_reset()
            t0 = time.perf_counter()
            eng.hutch_run(mode, 0, tol, maxiter)
            eng.sync()
            w = (time.perf_counter() - t0) * 1e3
            t = eng.timers()
            if rep >= args.warmup:
                dev.append(sum(t.values()))
                wall.append(w)
                buckets = t
        _, itf, _ = eng.hutch_fetch()
        return {"device_ms": float(np.median(dev)), "device_ms_all": [round(v, 4) for v in dev],
                "wall_ms": float(np.median(wall)), "iters_max": int(itf.max()),
                "buckets_ms": {k: round(buckets[k], 4) for k in TIMER_NAMES}}

    eng.set_profiling(True)
    out = {"lattice": "schwinger128", "nb": args.nb, "reps": args.reps, "stop_factor": args.stop_factor,
           "k_defl": int(tp['nr_deflat_vctrs']), "mode0": measure(MODE_HUTCHINSON), "mode4": {}}
    eng.set_deflation(W)
    for S in (1, 16, 128):
        eng.set_shifts([2 * L * d for d in range(S)])
        out["mode4"][str(S)] = measure(MODE_HUTCHINSON_SHIFTS)
        out["mode4"][str(S)]["over_mode0"] = out["mode4"][str(S)]["device_ms"] / out["mode0"]["device_ms"] - 1.0
    eng.set_profiling(False)
    # the launches of the S = 128 batch without per-launch events around them
    t0 = time.perf_counter()
    for _ in range(args.reps):
        eng.hutch_run(MODE_HUTCHINSON_SHIFTS, 0, tol, maxiter)
    eng.sync()
    out["mode4"]["128"]["wall_ms_unprofiled"] = (time.perf_counter() - t0) * 1e3 / args.reps
    eng.set_shifts(None)
    eng.set_deflation(np.asarray(Ux))
    t0 = time.perf_counter()
    for _ in range(args.reps):
        eng.hutch_run(MODE_HUTCHINSON, 0, tol, maxiter)
    eng.sync()
    out["mode0"]["wall_ms_unprofiled"] = (time.perf_counter() - t0) * 1e3 / args.reps
    out["bar"] = {"S128_over_mode0_max": 0.25, "met": bool(out["mode4"]["128"]["over_mode0"] <= 0.25)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
