#!/usr/bin/env python3
"""Cost of contracting the distilled two-point functions on the device (sw_distilled_two_point) in one
process on schwinger128, by the method of perambulator_bench.py: HIP-event time (the engine's per-launch event buckets,
summed), median of --reps, the tuned solver hierarchy of the drop-in flow.  For N = 32 (four source timeslices) and
N = 128 (one), one 256-column block and one momentum: the time of the contraction's own class (k_laph_left,
k_laph_right, k_laph_reduce), its share of the block's device time held against the bar of 10 % that DESIGN 4d set for
a mode's own kernels, and its rate against the 48.1 TFlop/s of profiles/r01_mfma_f64_rate.txt; the elementals'
launch (k_laph_elementals) on its own.  Then the wall clock of the chunk loop of distilled_two_point() with
keep_perambulators = False, elementals included and the set-up excluded, distilled_contraction = "host" against
"device": all 128 source timeslices at N = 32 and four at N = 128, both with the momenta 0 and 1.  The condition is
that the device path is the faster one at both.
python tools/distilled_contract_bench.py [--reps 7] [--out FILE]"""
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
MFMA_F64_TF = 48.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--t0", type=int, default=5)
    ap.add_argument("--momentum", type=int, default=1)
    ap.add_argument("--stop-factor", type=float, default=0.1)
    ap.add_argument("--flow-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from deflatedmlmc_schwinger_amd import gateway, matrix, utils
    from deflatedmlmc_schwinger_amd.engine import KCLASS_LAPH_CONTRACT, TIMER_NAMES
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
    tol, maxiter = 1e-12, 1000
    out = {"lattice": "schwinger128", "reps": args.reps, "stop_factor": args.stop_factor, "tol": tol,
           "block_columns": 256, "momentum": args.momentum, "mfma_f64_TF_per_s": MFMA_F64_TF,
           "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}

    # one block, one momentum: the contraction's class against the block's device time
    eng.set_profiling(True)
    for nev in (32, 128):
        V = np.ascontiguousarray(Vall[:, :nev])
        eng.set_distillation(V)
        eng.timers_reset()
        eng.set_distillation_momenta([args.momentum])
        elem_ms, elem_cnt = eng.kernel_stats(KCLASS_LAPH_CONTRACT)
        elem_work = eng.kernel_work(KCLASS_LAPH_CONTRACT)
        t0s = [(args.t0 + s) % L for s in range(256 // (2 * nev))]
        dev, wall, cls = [], [], []
        buckets = work = iters = None
        for rep in range(args.warmup + args.reps):
            eng.timers_reset()
            t1 = time.perf_counter()
            _, _, _, it = eng.distilled_two_point(t0s, tol, maxiter, keep=False)
            eng.sync()
            w = (time.perf_counter() - t1) * 1e3
            t = eng.timers()
            ms, cnt = eng.kernel_stats(KCLASS_LAPH_CONTRACT)
            assert cnt == 3
            if rep >= args.warmup:
                dev.append(sum(t.values()))
                wall.append(w)
                cls.append(ms)
                buckets, work, iters = t, eng.kernel_work(KCLASS_LAPH_CONTRACT), it
        d, c = float(np.median(dev)), float(np.median(cls))
        out["N%d" % nev] = {
            "source_timeslices": t0s, "device_ms": d, "device_ms_all": [round(v, 4) for v in dev],
            "wall_ms": float(np.median(wall)), "iters_min": int(iters.min()), "iters_max": int(iters.max()),
            "buckets_ms": {k: round(buckets[k], 4) for k in TIMER_NAMES},
            "contract_ms": c, "contract_ms_all": [round(v, 4) for v in cls], "contract_share": c / d,
            "contract_flops": work, "contract_TF_per_s": work / (c * 1e-3) / 1e12,
            "contract_over_mfma_rate": work / (c * 1e-3) / 1e12 / MFMA_F64_TF,
            "elementals_ms": elem_ms, "elementals_launches": elem_cnt, "elementals_flops": elem_work,
            "block_MB": L * 2 * nev * 256 * 16 / 1e6}
    eng.set_profiling(False)

    # the chunk loop of distilled_two_point(), keep_perambulators = False, host against device
    momenta = [0, 1]

    def host(V, t0s, nev):
        M = utils.laph_elementals(V, L, momenta)
        chunk = max(1, 256 // (2 * nev))
        T = np.zeros((len(t0s), 2, 2, 2, 2, 2, L), dtype=np.complex128)
        loops = np.full((2, 2, 2, L), np.nan + 0j)
        for first in range(0, len(t0s), chunk):
            part = t0s[first:first + chunk]
            tau, _ = eng.perambulators(part, tol, maxiter)
            T[first:first + len(part)] = utils.distilled_pair_sums(tau, M, part)
            loops[..., part] = utils.distilled_loops(tau, M, part)[..., part]
        return T, loops

    def device(V, t0s, nev):
        eng.set_distillation_momenta(momenta)
        chunk = max(1, 256 // (2 * nev))
        T = np.zeros((len(t0s), 2, 2, 2, 2, 2, L), dtype=np.complex128)
        loops = np.full((2, 2, 2, L), np.nan + 0j)
        for first in range(0, len(t0s), chunk):
            part = t0s[first:first + chunk]
            Tp, lp, _, _ = eng.distilled_two_point(part, tol, maxiter, keep=False)
            T[first:first + len(part)] = Tp
            loops[..., part] = lp.transpose(1, 2, 3, 0)
        return T, loops

    for name, nev, t0s in (("flow_N32_all_128_sources", 32, list(range(L))),
                           ("flow_N128_four_sources", 128, [(args.t0 + s) % L for s in range(4)])):
        V = np.ascontiguousarray(Vall[:, :nev])
        eng.set_distillation(V)
        rec = {"sources": len(t0s), "momenta": momenta, "columns": 2 * nev * len(t0s)}
        results = {}
        for where, run in (("host", host), ("device", device)):
            run(V, t0s[:max(1, 256 // (2 * nev))], nev)                    # warm-up: one chunk
            walls = []
            for _ in range(args.flow_reps):
                eng.sync()
                t1 = time.perf_counter()
                results[where] = run(V, t0s, nev)
                eng.sync()
                walls.append(time.perf_counter() - t1)
            rec[where + "_wall_s"] = float(np.median(walls))
            rec[where + "_wall_s_all"] = [round(v, 4) for v in walls]
        rec["host_over_device"] = rec["host_wall_s"] / rec["device_wall_s"]
        rec["max_rel_difference"] = float(np.max(np.abs(results["host"][0] - results["device"][0]))
                                          / np.max(np.abs(results["host"][0])))
        out[name] = rec
    eng.set_distillation(None)
    out["bars"] = {"contract_share_max": 0.10,
                   "share_met": bool(max(out["N32"]["contract_share"], out["N128"]["contract_share"]) <= 0.10),
                   "device_faster": bool(min(out["flow_N32_all_128_sources"]["host_over_device"],
                                             out["flow_N128_four_sources"]["host_over_device"]) > 1.0)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
