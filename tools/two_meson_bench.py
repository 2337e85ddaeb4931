#!/usr/bin/env python3
"""Cost of the two-meson building blocks on the device (sw_distilled_two_meson) in one process on
schwinger128, by the method of distilled_contract_bench.py: HIP-event time (the engine's per-launch event buckets,
summed), median of --reps with min-max, the tuned solver hierarchy of the drop-in flow, tol 1e-12.  For N = 32 (four
source timeslices) and N = 128 (one), one 256-column block, the momenta 0 and 1 and 2 x 2 operators ((g3, 0), (g3, 1) at
both ends): the block's device time, the time and the counted flops of the two-meson class (k_laph_sink,
k_laph_sandwich, k_laph_source, k_laph_trace1, k_laph_trace2) and its rate, next to the rate of the two-point
contraction's class (k_laph_left, k_laph_right, k_laph_reduce; sw_distilled_two_point) on the same block in the same
run.  Then the wall clock of the chunk loop of distilled_two_meson(), elementals included and the set-up excluded,
distilled_contraction = "host" (NumPy on OMP_NUM_THREADS threads, 16 by default) against "device" at both workloads.
The condition is that the device path is the faster one at both.
python tools/two_meson_bench.py [--reps 7] [--out FILE]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_NUM_THREADS", "16")
MFMA_F64_TF = 48.1
OPERATORS = [('g3', 0), ('g3', 1)]


def _spread(values):
    import numpy as np
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values)),
            "all": [round(float(v), 4) for v in values]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--t0", type=int, default=5)
    ap.add_argument("--stop-factor", type=float, default=0.1)
    ap.add_argument("--flow-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from deflatedmlmc_schwinger_amd import gateway, matrix, utils
    from deflatedmlmc_schwinger_amd.engine import KCLASS_LAPH_CONTRACT, KCLASS_LAPH_TWO_MESON, TIMER_NAMES
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
    L = 128
    eng.set_option("stop_factor", args.stop_factor)
    Vall, _ = utils.laplacian_eigenvectors(detect_lattice(A)[2], L, L)
    tol, maxiter, momenta = 1e-12, 1000, [0, 1]
    G, H = utils.two_meson_folded(OPERATORS, OPERATORS)
    out = {"lattice": "schwinger128", "reps": args.reps, "stop_factor": args.stop_factor, "tol": tol,
           "block_columns": 256, "momenta": momenta, "operators": [list(op) for op in OPERATORS],
           "mfma_f64_TF_per_s": MFMA_F64_TF, "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}

    # one block: the two-meson class against the block's device time, and the two-point contraction's class beside it
    eng.set_profiling(True)
    for nev in (32, 128):
        V = np.ascontiguousarray(Vall[:, :nev])
        eng.set_distillation(V)
        eng.set_distillation_momenta(momenta)
        t0s = [(args.t0 + s) % L for s in range(256 // (2 * nev))]
        dev, cls, cls27 = [], [], []
        buckets = work = work27 = iters = None
        for rep in range(args.warmup + args.reps):
            eng.timers_reset()
            _, _, it = eng.distilled_two_meson(t0s, G, H, tol, maxiter)
            eng.sync()
            t = eng.timers()
            ms, cnt = eng.kernel_stats(KCLASS_LAPH_TWO_MESON)
            assert cnt == 2 * 2 + 3
            w29 = eng.kernel_work(KCLASS_LAPH_TWO_MESON)
            eng.timers_reset()
            eng.distilled_two_point(t0s, tol, maxiter, keep=False)
            eng.sync()
            ms27, cnt27 = eng.kernel_stats(KCLASS_LAPH_CONTRACT)
            assert cnt27 == 3 * len(momenta)
            if rep >= args.warmup:
                dev.append(sum(t.values()))
                cls.append(ms)
                cls27.append(ms27)
                buckets, work, work27, iters = t, w29, eng.kernel_work(KCLASS_LAPH_CONTRACT), it
        d, c, c27 = _spread(dev), _spread(cls), _spread(cls27)
        rate = lambda flops, s: {"median": flops / (s["median"] * 1e-3) / 1e12, "min": flops / (s["max"] * 1e-3) / 1e12,
                                 "max": flops / (s["min"] * 1e-3) / 1e12}
        traces = 8.0 * (4 * L * len(t0s) * 5 * nev * nev + 16 * L * len(t0s) * (2 * nev) ** 2)
        out["N%d" % nev] = {
            "source_timeslices": t0s, "device_ms": d, "iters_min": int(iters.min()), "iters_max": int(iters.max()),
            "buckets_ms": {k: round(buckets[k], 4) for k in TIMER_NAMES},
            "two_meson_ms": c, "two_meson_share": c["median"] / d["median"], "two_meson_flops": work,
            "two_meson_matrix_flops": work - traces, "two_meson_TF_per_s": rate(work, c),
            "two_point_contract_ms": c27, "two_point_contract_flops": work27,
            "two_point_contract_TF_per_s": rate(work27, c27),
            "workspace_MB": (2 + 4 + 1) * len(t0s) * L * (2 * ((nev + 15) // 16 * 16)) ** 2 * 16 / 1e6}
    eng.set_profiling(False)

    # the chunk loop of distilled_two_meson(), host against device
    sink_ops = source_ops = list(OPERATORS)          # the momenta are their own indices in [0, 1]

    def host(V, t0s, nev):
        M = utils.laph_elementals(V, L, momenta)
        chunk = max(1, 256 // (2 * nev))
        parts = []
        for first in range(0, len(t0s), chunk):
            part = t0s[first:first + chunk]
            tau, _ = eng.perambulators(part, tol, maxiter)
            parts.append(utils.two_meson_sums(tau, M, part, sink_ops, source_ops))
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def device(V, t0s, nev):
        eng.set_distillation_momenta(momenta)
        chunk = max(1, 256 // (2 * nev))
        parts = []
        for first in range(0, len(t0s), chunk):
            parts.append(eng.distilled_two_meson(t0s[first:first + chunk], G, H, tol, maxiter))
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    for name, nev, t0s in (("flow_N32_four_sources", 32, [(args.t0 + s) % L for s in range(4)]),
                           ("flow_N128_one_source", 128, [args.t0])):
        V = np.ascontiguousarray(Vall[:, :nev])
        eng.set_distillation(V)
        rec = {"sources": len(t0s), "momenta": momenta, "columns": 2 * nev * len(t0s)}
        results = {}
        for where, run in (("host", host), ("device", device)):
            run(V, t0s, nev)                                               # warm-up
            walls = []
            for _ in range(args.flow_reps):
                eng.sync()
                t1 = time.perf_counter()
                results[where] = run(V, t0s, nev)
                eng.sync()
                walls.append(time.perf_counter() - t1)
            rec[where + "_wall_s"] = _spread(walls)
        rec["host_over_device"] = rec["host_wall_s"]["median"] / rec["device_wall_s"]["median"]
        rec["max_rel_difference_C1"] = float(np.max(np.abs(results["host"][0] - results["device"][0]))
                                             / np.max(np.abs(results["host"][0])))
        rec["max_rel_difference_C2"] = float(np.max(np.abs(results["host"][1] - results["device"][1]))
                                             / np.max(np.abs(results["host"][1])))
        out[name] = rec
    eng.set_distillation(None)
    out["bars"] = {"device_faster": bool(min(out["flow_N32_four_sources"]["host_wall_s"]["min"]
                                             / out["flow_N32_four_sources"]["device_wall_s"]["max"],
                                             out["flow_N128_one_source"]["host_wall_s"]["min"]
                                             / out["flow_N128_one_source"]["device_wall_s"]["max"]) > 1.0)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
