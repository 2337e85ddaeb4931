#!/usr/bin/env python3
"""Cost of the generalized perambulators (sw_generalized_perambulators) in one process on schwinger128, the tuned
solver hierarchy of the drop-in flow, tol 1e-12, median of --reps:

  * one call at N = 32 and N = 128, all 128 insertion timeslices, at one and at two momenta: HIP-event time (the
    engine's per-launch buckets, summed) and wall time, the share of k_laph_generalized (class 28) and its rate;
  * k_laph_project alone on a 256-column block in the same run: the other kernel on the same matrix cores;
  * the device against the host from the same solutions: sw_apply_laph_generalized (kernel time, and wall time with
    both transfers) against utils.generalized_perambulators_from_solutions in complex128 on the threads NumPy is
    given (OMP_NUM_THREADS), at N = 32 on all timeslices and at N = 128 on eight.

python tools/generalized_perambulator_bench.py [--reps 7] [--out FILE]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--t0", type=int, default=5)
    ap.add_argument("--tf", type=int, default=21)
    ap.add_argument("--stop-factor", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from deflatedmlmc_schwinger_amd import gateway, matrix, utils
    from deflatedmlmc_schwinger_amd.engine import KCLASS_LAPH, KCLASS_LAPH_GENERALIZED, TIMER_NAMES
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
    _, _, U1, U2 = detect_lattice(A)
    eng.set_option("stop_factor", args.stop_factor)
    Vall, _ = utils.laplacian_eigenvectors(U1, L, L)
    tol, maxiter = 1e-12, 1000
    rng = np.random.default_rng(7)
    out = {"lattice": "schwinger128", "reps": args.reps, "stop_factor": args.stop_factor, "tol": tol,
           "source_timeslice": args.t0, "sink_timeslice": args.tf,
           "host_threads": os.environ.get("OMP_NUM_THREADS", "unset")}
    med = lambda v: float(np.median(v))
    eng.set_profiling(True)

    # one call, all insertion timeslices
    for nev in (32, 128):
        eng.set_distillation(np.ascontiguousarray(Vall[:, :nev]))
        for momenta in ([0], [0, 1]):
            dev, wall, cls = [], [], []
            for rep in range(args.warmup + args.reps):
                eng.timers_reset()
                t1 = time.perf_counter()
                G, _, it = eng.generalized_perambulators(args.t0, args.tf, list(range(L)), momenta, tol, maxiter,
                                                         keep_tau=False)
                w = (time.perf_counter() - t1) * 1e3
                t = eng.timers()
                ms, cnt = eng.kernel_stats(KCLASS_LAPH_GENERALIZED)
                work = eng.kernel_work(KCLASS_LAPH_GENERALIZED)
                if rep >= args.warmup:
                    dev.append(sum(t.values()))
                    wall.append(w)
                    cls.append(ms)
            out["N%d_q%d" % (nev, len(momenta))] = {
                "momenta": momenta, "device_ms": med(dev), "device_ms_all": [round(v, 3) for v in dev],
                "wall_ms": med(wall), "iters_min": int(it.min()), "iters_max": int(it.max()),
                "buckets_ms": {k: round(t[k], 3) for k in TIMER_NAMES}, "generalized_launches": cnt,
                "generalized_ms": med(cls), "generalized_share": med(cls) / med(dev), "generalized_flops": work,
                "generalized_TF_per_s": work / (med(cls) * 1e-3) / 1e12, "G_MB": G.nbytes / 1e6}
            del G

    # k_laph_project on a 256-column block, the same matrix cores
    Z = rng.standard_normal((256, n)) + 1j * rng.standard_normal((256, n))
    proj = []
    for rep in range(args.warmup + args.reps):
        eng.timers_reset()
        eng.apply_laph_project(Z)
        pms, _ = eng.kernel_stats(KCLASS_LAPH)
        pwork = eng.kernel_work(KCLASS_LAPH)
        if rep >= args.warmup:
            proj.append(pms)
    out["project_N128"] = {"project_ms": med(proj), "project_flops": pwork,
                           "project_TF_per_s": pwork / (med(proj) * 1e-3) / 1e12}
    eng.set_distillation(None)

    # the device against the host from the same solutions of the eigenvector sources (solved here once, on the device)
    for nev, ts in ((32, list(range(L))), (128, [4, 5, 6, 13, 20, 21, 22, 70])):
        src = utils.laph_sources(np.ascontiguousarray(Vall[:, :nev]), L, [args.t0, args.tf])
        sol = np.concatenate([mg.solve_batch(0, src[c:c + 256], tol)[0] for c in range(0, src.shape[0], 256)])
        Z0, Zf = sol[:2 * nev], sol[2 * nev:]
        kern, wall = [], []
        for rep in range(args.warmup + args.reps):
            eng.timers_reset()
            t1 = time.perf_counter()
            G = eng.apply_laph_generalized(Zf, Z0, ts, [0, 1])
            w = (time.perf_counter() - t1) * 1e3
            ms, _ = eng.kernel_stats(KCLASS_LAPH_GENERALIZED)
            if rep >= args.warmup:
                kern.append(ms)
                wall.append(w)
        host = []
        for rep in range(args.reps):
            t1 = time.perf_counter()
            ref = utils.generalized_perambulators_from_solutions(Zf, Z0, U1, U2, L, ts, [0, 1])
            host.append((time.perf_counter() - t1) * 1e3)
        out["device_against_host_N%d" % nev] = {
            "timeslices": len(ts), "momenta": [0, 1], "device_kernel_ms": med(kern), "device_wall_ms": med(wall),
            "host_ms": med(host), "host_ms_all": [round(v, 1) for v in host],
            "host_over_device_wall": med(host) / med(wall), "host_over_device_kernel": med(host) / med(kern),
            "max_abs_diff_over_max": float(np.max(np.abs(G - ref)) / np.max(np.abs(ref)))}
    eng.set_profiling(False)
    out["condition"] = {"device_faster_than_host": bool(all(
        out["device_against_host_N%d" % nev]["host_over_device_wall"] > 1.0 for nev in (32, 128)))}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            rows = [" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in out.items()]      # one record per line
            f.write("{\n" + ",\n".join(rows) + "\n}\n")


if __name__ == "__main__":
    main()
