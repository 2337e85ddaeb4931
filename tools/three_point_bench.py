#!/usr/bin/env python3
"""Cost of the three-point batches next to the two-point batch, in one process on schwinger128: HIP-event time (the
engine's per-launch event buckets, summed) and wall time of a SW_MODE_TWO_POINT batch of 128 noises x momenta [0] and
of SW_MODE_THREE_POINT batches of 128 noises with the insertion momenta [0], [0, 1] and eight momenta -- 256 solve
columns per solve in each, probes resident in HBM, the tuned solver hierarchy of the drop-in flow.  Mode 6 is code
this mode does not touch; a mode-13 batch holds two such solves.  The new kernels' own classes (sources + c_k; the
field x field sums) are reported, their share of the mode-13 batch's device time is held against the bar of 10 % at
[0] and [0, 1], and the sums' time against the byte model -- each of the 5 M branch passes reads zeta and z once,
2 n 2 nq 16 B -- as an effective read rate.  The configurations alternate batch by batch (mode 6, [0], mode 6,
[0, 1], mode 6, eight, ...) so that drift of the shared machine lands on all of them alike.
python tools/three_point_bench.py [--reps 7] [--out FILE]"""
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

EIGHT = [0, 1, 2, 3, 5, 8, 13, 127]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--t0", type=int, default=5)
    ap.add_argument("--tf", type=int, default=21)
    ap.add_argument("--nb", type=int, default=128)
    ap.add_argument("--stop-factor", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from deflatedmlmc_schwinger_amd import gateway, matrix, utils
    from deflatedmlmc_schwinger_amd.engine import (KCLASS_3PT_DOTS, KCLASS_3PT_SOURCES, MODE_THREE_POINT,
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
    eng = mg.engine
    n = A.shape[0]
    nb = args.nb
    eng.set_option("stop_factor", args.stop_factor)
    np.random.seed(123456)
    eng.probes_upload(0, utils.draw_probes(nb, n))
    eng.set_two_point(args.t0, [0])
    configs = [("q0", [0]), ("q01", [0, 1]), ("q8", EIGHT)]
    tol, maxiter = 1e-12, 1000

    def one(mode):
        eng.timers_reset()
        t0 = time.perf_counter()
        eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        w = (time.perf_counter() - t0) * 1e3
        return w, eng.timers(), eng.kernel_stats(KCLASS_3PT_SOURCES), eng.kernel_stats(KCLASS_3PT_DOTS)

    eng.set_profiling(True)
    names = ["mode6"] + [c[0] for c in configs]
    acc = {k: {"dev": [], "wall": [], "src": [], "dots": [], "buckets": None, "iters_max": 0} for k in names}

    def record(name, res):
        w, t, src, dots = res
        a = acc[name]
        a["dev"].append(sum(t.values()))
        a["wall"].append(w)
        a["src"].append(src[0])
        a["dots"].append(dots[0])
        a["buckets"] = t
        a["launches"] = {"sources_total": src[1], "seq_dots": dots[1]}
        a["iters_max"] = int(eng.hutch_fetch()[1].max())

    for rep in range(args.warmup + args.reps):
        for name, momenta in configs:
            res6 = one(MODE_TWO_POINT)
            if rep >= args.warmup:
                record("mode6", res6)
            eng.set_three_point(args.t0, args.tf, 'g3', 0, momenta)
            res = one(MODE_THREE_POINT)
            if rep >= args.warmup:
                record(name, res)
    eng.set_profiling(False)
    pass_bytes = 2 * n * 2 * nb * 16                    # zeta and z, once
    out = {"lattice": "schwinger128", "reps": args.reps, "stop_factor": args.stop_factor, "source_timeslice": args.t0,
           "sink_timeslice": args.tf, "sink_gamma": "g3", "sink_momentum": 0, "noises": nb, "solve_columns": 2 * nb,
           "momenta": dict(configs), "bytes_per_branch_pass": pass_bytes}
    for name in names:
        a = acc[name]
        dev = float(np.median(a["dev"]))
        out[name] = {"device_ms": dev, "device_ms_all": [round(v, 4) for v in a["dev"]],
                     "wall_ms": float(np.median(a["wall"])), "iters_max": a["iters_max"],
                     "buckets_ms": {k: round(a["buckets"][k], 4) for k in TIMER_NAMES}}
        if name != "mode6":
            M = len(dict(configs)[name])
            src, dots = float(np.median(a["src"])), float(np.median(a["dots"]))
            out[name].update({"sources_total_ms": src, "seq_dots_ms": dots, "launches": a["launches"],
                              "new_kernels_share": (src + dots) / dev,
                              "device_ms_over_two_mode6": dev / (2.0 * out["mode6"]["device_ms"]),
                              "seq_dots_model_bytes": 5 * M * pass_bytes,
                              "seq_dots_effective_TBps": 5 * M * pass_bytes / (dots * 1e-3) / 1e12})
    # the same launches without per-launch events around them
    for name, momenta in [("mode6", None)] + configs:
        mode = MODE_TWO_POINT if momenta is None else MODE_THREE_POINT
        if momenta is not None:
            eng.set_three_point(args.t0, args.tf, 'g3', 0, momenta)
        eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        out[name]["wall_ms_unprofiled"] = (time.perf_counter() - t0) * 1e3 / args.reps
    eng.set_two_point(0, None)
    eng.set_three_point(0, 1, 'g3', 0, None)
    out["bars"] = {"new_kernels_share_max": 0.10,
                   "met": bool(max(out[c]["new_kernels_share"] for c in ("q0", "q01")) <= 0.10)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
