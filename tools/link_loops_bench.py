#!/usr/bin/env python3
"""Cost of the point-split link loops next to the timeslice-loop batch, in one process on schwinger128: HIP-event
time (the engine's per-launch event buckets, summed), the time of k_slice_link_dots alone (its kernel class) and
wall time of SW_MODE_HUTCHINSON_LOOPS and SW_MODE_HUTCHINSON_LINK_LOOPS batches at the momentum 0 alone and at
eight momenta, nb probes resident in HBM, k = 8 deflation vectors, the tuned solver hierarchy of the drop-in flow.
The four configurations alternate batch by batch (mode 5 [0], mode 12 [0], mode 5 eight, mode 12 eight, ...) so
that drift of the shared machine lands on all of them alike.  Mode 5 is code this mode does not touch: it is the
batch as it was before the link loops existed.
python tools/link_loops_bench.py [--nb 256] [--reps 7] [--out FILE]"""
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

BAR = 0.10      # DESIGN 4c's bar for its widest case: at most +10 % over the batch it is compared with


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
    from deflatedmlmc_schwinger_amd.engine import (KCLASS_LINK_DOTS, MODE_HUTCHINSON_LINK_LOOPS,
                                                   MODE_HUTCHINSON_LOOPS, TIMER_NAMES)
    from deflatedmlmc_schwinger_amd.multigrid import MG
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params['link_loops'] = [0]
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "hutchinson")
    tp['nr_deflat_vctrs'] = 8
    mg = MG(A)
    with contextlib.redirect_stdout(io.StringIO()):
        mg.setup(dof=tp['dof'], aggrs=tp['aggrs'], max_levels=tp['max_nr_levels'], dim=2,
                 acc_eigvs=tp['accuracy_mg_eigvs'], sys_type='schwinger', params=tp)
        # with the key present the vectors W = gamma_3 V sgn(lambda) are registered without Pperm, as both modes want
        utils.deflation_pre_computations(A, tp['nr_deflat_vctrs'], tp['defl_eigvs_tol_Hutch'], "hutchinson",
                                         mg.timer, tp, mg)
    eng = mg.engine
    n = A.shape[0]
    eng.set_option("stop_factor", args.stop_factor)
    np.random.seed(123456)
    eng.probes_upload(0, utils.draw_probes(args.nb, n))
    tol, maxiter = 1e-12, 1000

    EIGHT = [0, 1, 2, 3, 4, 5, 6, 7]
    configs = [("loops_p0", MODE_HUTCHINSON_LOOPS, [0]), ("link_p0", MODE_HUTCHINSON_LINK_LOOPS, [0]),
               ("loops_eight", MODE_HUTCHINSON_LOOPS, EIGHT), ("link_eight", MODE_HUTCHINSON_LINK_LOOPS, EIGHT)]

    def one(mode):
        eng.timers_reset()
        t0 = time.perf_counter()
        eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        w = (time.perf_counter() - t0) * 1e3
        return w, eng.timers(), eng.kernel_stats(KCLASS_LINK_DOTS)

    eng.set_profiling(True)
    acc = {name: {"dev": [], "wall": [], "link": [], "buckets": None, "iters_max": 0, "link_launches": 0}
           for name, _, _ in configs}
    for rep in range(args.warmup + args.reps):
        for name, mode, momenta in configs:
            eng.set_loop_momenta(momenta)
            w, t, (link_ms, link_launches) = one(mode)
            if rep >= args.warmup:
                a = acc[name]
                a["dev"].append(sum(t.values()))
                a["wall"].append(w)
                a["link"].append(link_ms)
                a["buckets"] = t
                a["link_launches"] = link_launches
                a["iters_max"] = int(eng.hutch_fetch()[1].max())
    eng.set_profiling(False)
    out = {"lattice": "schwinger128", "nb": args.nb, "reps": args.reps, "stop_factor": args.stop_factor,
           "k_defl": int(tp['nr_deflat_vctrs']), "momenta": {"p0": [0], "eight": EIGHT}}
    for name, _, _ in configs:
        a = acc[name]
        out[name] = {"device_ms": float(np.median(a["dev"])), "device_ms_min": float(np.min(a["dev"])),
                     "device_ms_max": float(np.max(a["dev"])), "device_ms_all": [round(v, 4) for v in a["dev"]],
                     "wall_ms": float(np.median(a["wall"])), "iters_max": a["iters_max"],
                     "link_dots_ms": float(np.median(a["link"])), "link_dots_ms_all": [round(v, 4) for v in a["link"]],
                     "link_dots_launches": a["link_launches"],
                     "buckets_ms": {k: round(a["buckets"][k], 4) for k in TIMER_NAMES}}
    for which in ("p0", "eight"):
        base, link = out["loops_" + which], out["link_" + which]
        link["over_loops"] = link["device_ms"] / base["device_ms"] - 1.0
        diff = link["device_ms"] - base["device_ms"]
        spread = max(base["device_ms_max"] - base["device_ms_min"], link["device_ms_max"] - link["device_ms_min"])
        link["difference_ms"] = diff
        link["spread_ms"] = spread
        link["resolved"] = bool(abs(diff) > spread)
    # the same launches without per-launch events around them
    for name, mode, momenta in configs:
        eng.set_loop_momenta(momenta)
        eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        out[name]["wall_ms_unprofiled"] = (time.perf_counter() - t0) * 1e3 / args.reps
    eng.set_loop_momenta(None)
    out["bars"] = {"link_over_loops_max": BAR,
                   "met": bool(out["link_p0"]["over_loops"] <= BAR and out["link_eight"]["over_loops"] <= BAR)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
