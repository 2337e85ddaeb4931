#!/usr/bin/env python3
"""Cost of the one-end-trick two-point batches next to the plain deflated Hutchinson batch, in one process on
schwinger128: HIP-event time (the engine's per-launch event buckets, summed) and wall time of a SW_MODE_HUTCHINSON
batch of 256 probes and of SW_MODE_TWO_POINT batches of 128 noises x momenta [0] and of 64 noises x momenta [0, 1]
(256 solve columns each), probes resident in HBM, the tuned solver hierarchy of the drop-in flow.  Timeslice sources
need another number of outer iterations than random probes, so the comparison is device time per outer iteration;
the new kernels' own classes (sources; pair dots + total) are reported and their share of the mode-6 batch is held
against the bar of 10 %.  The configurations alternate (mode 0, [0], [0, 1], mode 0, ...) so that drift of the shared
machine lands on all of them alike.
python tools/two_point_bench.py [--reps 7] [--out FILE]"""
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
    from deflatedmlmc_schwinger_amd.engine import (KCLASS_TP_DOTS, KCLASS_TP_SOURCES, MODE_HUTCHINSON,
                                                   MODE_TWO_POINT, TIMER_NAMES)
    from deflatedmlmc_schwinger_amd.multigrid import MG
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "hutchinson")
    mg = MG(A)
    with contextlib.redirect_stdout(io.StringIO()):
        mg.setup(dof=tp['dof'], aggrs=tp['aggrs'], max_levels=tp['max_nr_levels'], dim=2,
                 acc_eigvs=tp['accuracy_mg_eigvs'], sys_type='schwinger', params=tp)
        utils.deflation_pre_computations(A, tp['nr_deflat_vctrs'], tp['defl_eigvs_tol_Hutch'], "hutchinson",
                                         mg.timer, tp, mg)
    eng = mg.engine
    n = A.shape[0]
    eng.set_option("stop_factor", args.stop_factor)
    np.random.seed(123456)
    probes = utils.draw_probes(256, n)
    # slot per configuration: 256 probes, 128 noises, 64 noises
    configs = [("mode0", MODE_HUTCHINSON, None, 256), ("p0_128", MODE_TWO_POINT, [0], 128),
               ("p01_64", MODE_TWO_POINT, [0, 1], 64)]
    for slot, (_, _, _, nb) in enumerate(configs):
        eng.probes_upload_slot(slot, 0, probes[:nb])
    tol, maxiter = 1e-12, 1000

    def select(slot, momenta):
        eng.probes_select(slot)
        if momenta is not None:
            eng.set_two_point(args.t0, momenta)

    def one(mode):
        eng.timers_reset()
        t0 = time.perf_counter()
        eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        w = (time.perf_counter() - t0) * 1e3
        return w, eng.timers(), eng.kernel_stats(KCLASS_TP_SOURCES), eng.kernel_stats(KCLASS_TP_DOTS)

    eng.set_profiling(True)
    acc = {c[0]: {"dev": [], "wall": [], "src": [], "dots": [], "buckets": None, "iters_max": 0} for c in configs}
    for rep in range(args.warmup + args.reps):
        for slot, (name, mode, momenta, _) in enumerate(configs):
            select(slot, momenta)
            w, t, src, dots = one(mode)
            if rep >= args.warmup:
                a = acc[name]
                a["dev"].append(sum(t.values()))
                a["wall"].append(w)
                a["src"].append(src[0])
                a["dots"].append(dots[0])
                a["buckets"] = t
                a["launches"] = {"sources": src[1], "pair_dots_total": dots[1]}
                a["iters_max"] = int(eng.hutch_fetch()[1].max())
    eng.set_profiling(False)
    out = {"lattice": "schwinger128", "reps": args.reps, "stop_factor": args.stop_factor, "source_timeslice": args.t0,
           "solve_columns": 256, "momenta": {"p0_128": [0], "p01_64": [0, 1]}}
    for name, _, _, nb in configs:
        a = acc[name]
        dev = float(np.median(a["dev"]))
        out[name] = {"nb": nb, "device_ms": dev, "device_ms_all": [round(v, 4) for v in a["dev"]],
                     "wall_ms": float(np.median(a["wall"])), "iters_max": a["iters_max"],
                     "device_ms_per_outer_iteration": dev / max(1, a["iters_max"]),
                     "buckets_ms": {k: round(a["buckets"][k], 4) for k in TIMER_NAMES}}
        if name != "mode0":
            src, dots = float(np.median(a["src"])), float(np.median(a["dots"]))
            out[name].update({"sources_ms": src, "pair_dots_total_ms": dots, "launches": a["launches"],
                              "new_kernels_share": (src + dots) / dev,
                              "per_iteration_over_mode0": out[name]["device_ms_per_outer_iteration"]
                              / out["mode0"]["device_ms_per_outer_iteration"] - 1.0})
    # the same launches without per-launch events around them
    for slot, (name, mode, momenta, _) in enumerate(configs):
        select(slot, momenta)
        eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        out[name]["wall_ms_unprofiled"] = (time.perf_counter() - t0) * 1e3 / args.reps
    eng.set_two_point(0, None)
    eng.probes_select(0)
    out["bars"] = {"new_kernels_share_max": 0.10,
                   "met": bool(max(out[c]["new_kernels_share"] for c in ("p0_128", "p01_64")) <= 0.10)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
