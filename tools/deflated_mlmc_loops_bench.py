#!/usr/bin/env python3
"""Cost and value of the deflated MLMC loops, in one process on schwinger128, by the protocol of
tools/mlmc_loops_bench.py: with k vectors of the difference operators registered on the levels 0 (level 1 skipped)
and 2, HIP-event time and wall time of a SW_MODE_MLMC_SKIP batch at level 0 and a SW_MODE_MLMC batch at level 2 next
to the SW_MODE_MLMC_DEFL_LOOPS_SKIP / SW_MODE_MLMC_DEFL_LOOPS batches with eight momenta, nb probes resident in HBM,
the two configurations of a level alternating batch by batch; the spread of the per-repetition differences decides
whether a difference is resolved.  Then the seconds of sw_level_deflation_loops (second call) next to
sw_coarsest_loops, and (--flows) deflated_mlmc_loops(), mlmc_loops() and hutchinson() at equal tol: per-entry variance
of the mean times the wall time of the probe loops for p = 0 and gamma_3, 1, and the sample variance of each level's
control column with and without the vectors (every flow is run twice and the second run is the one reported).
python tools/deflated_mlmc_loops_bench.py [--nb 256] [--reps 7] [--k 16] [--flows] [--out FILE]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("OMP_NUM_THREADS", "1")

from mlmc_loops_bench import EIGHT, byte_model_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=16, help="vectors per deflated level")
    ap.add_argument("--stop-factor", type=float, default=0.1)
    ap.add_argument("--flows", action="store_true")
    ap.add_argument("--flow-tol", type=float, default=3e-3)
    ap.add_argument("--hbm-tbs", type=float, default=4.4, help="rate of the byte model: what the stencil sustains")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from scipy.sparse.linalg import LinearOperator
    from deflatedmlmc_schwinger_amd import gateway, matrix, stoch_trace, utils
    from deflatedmlmc_schwinger_amd.engine import (MODE_MLMC, MODE_MLMC_DEFL_LOOPS, MODE_MLMC_DEFL_LOOPS_SKIP,
                                                   MODE_MLMC_SKIP, TIMER_NAMES)
    from deflatedmlmc_schwinger_amd.multigrid import MG
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params['use_permuted'] = False          # the scalar modes then solve for the plain probe too: equal work
    params['mlmc_defl_setup'] = 'device'
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "mlmc")
    mg = MG(A)
    with contextlib.redirect_stdout(io.StringIO()):
        mg.setup(dof=tp['dof'], aggrs=tp['aggrs'], max_levels=tp['max_nr_levels'], dim=2,
                 acc_eigvs=tp['accuracy_mg_eigvs'], sys_type='schwinger', params=tp)
    mg.total_levels = len(mg.ml.levels)
    mg.skip_level = True
    eng = mg.engine
    sizes = [lev.A.shape[0] for lev in mg.ml.levels]
    L = int(tp['latt_dims'][0])
    eng.set_option("stop_factor", args.stop_factor)
    tol, maxiter = 1e-12, 1000
    out = {"lattice": "schwinger128", "level_sizes": sizes, "nb": args.nb, "reps": args.reps, "vectors": args.k,
           "stop_factor": args.stop_factor, "byte_model_tbs": args.hbm_tbs, "momenta": EIGHT, "levels": {},
           "vector_setup_s": {}}

    for level in (0, 2):
        mg.level_for_diff_op = level
        lop = LinearOperator((sizes[level],) * 2, dtype=np.complex128,
                             matvec=lambda v: mg.diff_op_Q(np.array(v, dtype=np.complex128)))
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            utils.deflation_pre_computations(A, args.k, tp['defl_eigvs_tol_MLMC'], "mlmc", mg.timer, tp, mg, lop,
                                             level_nr=level)
        out["vector_setup_s"][str(level)] = time.perf_counter() - t0

    eng.set_profiling(True)
    for level, scalar, loops in ((0, MODE_MLMC_SKIP, MODE_MLMC_DEFL_LOOPS_SKIP), (2, MODE_MLMC, MODE_MLMC_DEFL_LOOPS)):
        np.random.seed(123456 + level)
        eng.probes_upload(level, utils.draw_probes(args.nb, sizes[level]))
        configs = [("scalar", scalar, [0]), ("eight", loops, EIGHT)]
        acc = {name: {"dev": [], "wall": [], "buckets": None} for name, _, _ in configs}
        for rep in range(args.warmup + args.reps):
            for name, mode, momenta in configs:
                eng.set_loop_momenta(momenta)
                eng.timers_reset()
                t0 = time.perf_counter()
                eng.hutch_run(mode, level, tol, maxiter)
                eng.sync()
                w = (time.perf_counter() - t0) * 1e3
                t = eng.timers()
                if rep >= args.warmup:
                    acc[name]["dev"].append(sum(t.values()))
                    acc[name]["wall"].append(w)
                    acc[name]["buckets"] = t
        rec = {}
        for name, _, _ in configs:
            a = acc[name]
            rec[name] = {"device_ms": float(np.median(a["dev"])), "device_ms_all": [round(v, 4) for v in a["dev"]],
                         "wall_ms": float(np.median(a["wall"])),
                         "buckets_ms": {k: round(a["buckets"][k], 4) for k in TIMER_NAMES}}
        # the pairs of one repetition ran back to back: their differences carry the spread of the comparison
        d = np.array(acc["eight"]["dev"]) - np.array(acc["scalar"]["dev"])
        e = rec["eight"]
        e["added_ms"] = float(np.median(d))
        e["added_ms_min_max"] = [float(d.min()), float(d.max())]
        e["over_scalar"] = e["added_ms"] / rec["scalar"]["device_ms"]
        e["over_scalar_min_max"] = [float(d.min() / rec["scalar"]["device_ms"]),
                                    float(d.max() / rec["scalar"]["device_ms"])]
        e["resolved"] = bool(d.min() > 0.0 or d.max() < 0.0)
        if level > 0:
            chain = [(sizes[l + 1], sizes[l]) for l in range(level - 1, -1, -1)]
            e["byte_model_ms"], e["byte_model_bytes"] = byte_model_ms(sizes[0], sizes[level], L, args.nb, len(EIGHT),
                                                                      chain, args.hbm_tbs)
        out["levels"][str(level)] = rec
    eng.set_profiling(False)
    out["bars"] = {"level0_eight_over_scalar_max": 0.10,
                   "met": bool(out["levels"]["0"]["eight"]["over_scalar"] <= 0.10)}

    eng.set_loop_momenta(EIGHT)
    for level in (0, 2):
        eng.level_deflation_loops(level, level == 0, tol, maxiter)
        eng.sync()
        t0 = time.perf_counter()
        eng.level_deflation_loops(level, level == 0, tol, maxiter)
        out.setdefault("level_deflation_loops_s", {})[str(level)] = time.perf_counter() - t0
    eng.coarsest_loops()
    eng.sync()
    t0 = time.perf_counter()
    eng.coarsest_loops()
    out["coarsest_loops_s"] = time.perf_counter() - t0
    out["coarsest_columns"] = sizes[-1]
    eng.set_loop_momenta(None)
    for level in (0, 2):
        eng.set_level_deflation(level, None)

    if args.flows:
        def flow(which):
            p = gateway.set_params('schwinger128')
            p['function_tol'] = 1e-12
            p['timeslice_loops'] = [0]
            p['stop_factor'] = args.stop_factor
            p['mlmc_defl_setup'] = 'device'
            f = utils.trace_params_from_params(p, "hutchinson" if which == "hutchinson" else "mlmc")
            f['tol'] = args.flow_tol
            if which == "deflated_mlmc":
                f['mlmc_deflat_vctrs'] = [args.k, 0, args.k, 0]
            elif which == "mlmc":
                f['mlmc_deflat_vctrs'] = [0, 0, 0, 0]
            fn = {"deflated_mlmc": stoch_trace.deflated_mlmc_loops, "mlmc": stoch_trace.mlmc_loops,
                  "hutchinson": stoch_trace.hutchinson}[which]
            # the second of two identical runs: the first pays the workspace allocations of its batch shapes
            with contextlib.redirect_stdout(io.StringIO()):
                fn(A, dict(f))
                return fn(A, f)

        rec = {"tol": args.flow_tol}
        for which in ("deflated_mlmc", "mlmc"):
            r = flow(which)
            stoch = [i for i in range(r['nr_levels'] - 1) if r['results'][i]['nr_ests'] > 0]
            secs = sum(r['results'][i]['probe_loop_s'] for i in stoch)
            rec[which] = {"probe_loop_s": secs, "levels": stoch,
                          "nr_ests": [r['results'][i]['nr_ests'] + 1 for i in stoch],
                          "control_sample_var": [float(np.var(r['results'][i]['ests'])) for i in stoch],
                          "trace": [float(np.real(r['trace'])), float(np.imag(r['trace']))]}
            for g in ("g3", "1"):
                v = sum(np.var(utils.loop_gamma(r['results'][i]['loop_ests'][:, 0], g), axis=0)
                        / (r['results'][i]['nr_ests'] + 1) for i in stoch)
                rec[which]["var_x_s_" + g] = float(np.mean(v) * secs)
        rh = flow("hutchinson")
        rec["hutchinson"] = {"probe_loop_s": rh['probe_loop_s'], "nr_ests": rh['nr_ests'] + 1}
        for g in ("g3", "1"):
            vh = np.var(utils.loop_gamma(rh['loop_ests'][:, 0], g), axis=0) / (rh['nr_ests'] + 1)
            rec["hutchinson"]["var_x_s_" + g] = float(np.mean(vh) * rh['probe_loop_s'])
        out["flows"] = rec

    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
