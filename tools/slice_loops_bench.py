#!/usr/bin/env python3
"""Cost of the timeslice loops next to the plain deflated Hutchinson batch, in one process on schwinger128:
HIP-event time (the engine's per-launch event buckets, summed) and wall time of a SW_MODE_HUTCHINSON batch and
of SW_MODE_HUTCHINSON_LOOPS batches with the momentum 0 alone and with eight momenta, nb probes resident in HBM,
the tuned solver hierarchy of the drop-in flow.  The configurations alternate (mode 0, [0], eight, mode 0, ...)
so that drift of the shared machine lands on all of them alike.
python tools/slice_loops_bench.py [--nb 256] [--reps 7] [--out FILE]"""
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
    from deflatedmlmc_schwinger_amd.engine import MODE_HUTCHINSON, MODE_HUTCHINSON_LOOPS, TIMER_NAMES
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
    n = A.shape[0]
    W = np.asarray(mg.ml.levels[0].Pperm.transpose() * Ux)      # the vectors before Pperm
    eng.set_option("stop_factor", args.stop_factor)
    np.random.seed(123456)
    eng.probes_upload(0, utils.draw_probes(args.nb, n))
    tol, maxiter = 1e-12, 1000

    EIGHT = [0, 1, 2, 3, 4, 5, 6, 7]
    configs = [("mode0", MODE_HUTCHINSON, None), ("p0", MODE_HUTCHINSON_LOOPS, [0]),
               ("eight", MODE_HUTCHINSON_LOOPS, EIGHT)]
    Uperm = np.asarray(Ux)

    def select(mode, momenta):
        # mode 0 projects with Pperm W (and gathers by Pperm), mode 5 with W itself
        eng.set_deflation(Uperm if momenta is None else W)
        eng.set_loop_momenta(momenta)

    def one(mode):
        eng.timers_reset()
        t0 = time.perf_counter()
        eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        w = (time.perf_counter() - t0) * 1e3
        return w, eng.timers()

    eng.set_profiling(True)
    acc = {name: {"dev": [], "wall": [], "buckets": None, "iters_max": 0} for name, _, _ in configs}
    for rep in range(args.warmup + args.reps):
        for name, mode, momenta in configs:
            select(mode, momenta)
            w, t = one(mode)
            if rep >= args.warmup:
                acc[name]["dev"].append(sum(t.values()))
                acc[name]["wall"].append(w)
                acc[name]["buckets"] = t
                acc[name]["iters_max"] = int(eng.hutch_fetch()[1].max())
    eng.set_profiling(False)
    out = {"lattice": "schwinger128", "nb": args.nb, "reps": args.reps, "stop_factor": args.stop_factor,
           "k_defl": int(tp['nr_deflat_vctrs']), "momenta": {"p0": [0], "eight": EIGHT}}
    for name, _, _ in configs:
        a = acc[name]
        out[name] = {"device_ms": float(np.median(a["dev"])), "device_ms_all": [round(v, 4) for v in a["dev"]],
                     "wall_ms": float(np.median(a["wall"])), "iters_max": a["iters_max"],
                     "buckets_ms": {k: round(a["buckets"][k], 4) for k in TIMER_NAMES}}
    for name in ("p0", "eight"):
        out[name]["over_mode0"] = out[name]["device_ms"] / out["mode0"]["device_ms"] - 1.0
    # the same launches without per-launch events around them
    for name, mode, momenta in configs:
        select(mode, momenta)
        eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        out[name]["wall_ms_unprofiled"] = (time.perf_counter() - t0) * 1e3 / args.reps
    eng.set_loop_momenta(None)
    eng.set_deflation(Uperm)
    out["bars"] = {"p0_over_mode0_max": 0.03, "eight_over_mode0_max": 0.10,
                   "met": bool(out["p0"]["over_mode0"] <= 0.03 and out["eight"]["over_mode0"] <= 0.10)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
