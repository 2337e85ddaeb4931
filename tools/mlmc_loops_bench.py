#!/usr/bin/env python3
"""Cost of the MLMC loop batches next to the scalar MLMC batches, in one process on schwinger128: HIP-event time (the
engine's per-launch event buckets, summed) and wall time of a SW_MODE_MLMC_SKIP batch at level 0 and a SW_MODE_MLMC
batch at level 2, and of the SW_MODE_MLMC_LOOPS_SKIP / SW_MODE_MLMC_LOOPS batches at the same levels with the
momentum 0 alone and with eight momenta, nb probes resident in HBM.  The configurations of a level alternate batch by
batch so that drift of the shared machine lands on all of them alike.  Then the seconds of sw_coarsest_loops, and
(--flows) one mlmc_loops() and one hutchinson() loops run at equal tol: per-entry variance of the mean times the wall
time of the probe loops, for p = 0 and gamma_3, 1.
python tools/mlmc_loops_bench.py [--nb 256] [--reps 7] [--flows] [--out FILE]"""
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

EIGHT = [0, 1, 2, 3, 64, 65, 126, 127]


def byte_model_ms(n0, n_lev, L, nb, nmom, chain_rows, hbm_tbs):
    """What a coarse-level loop batch adds to the scalar one, in bytes at 16 per complex number: the two prolongation
    chains (read the source, write the target, per hop; chain_rows = the (source, target) row counts), the two
    lattice blocks k_slice_cdots reads and the loops it writes; less the two dots of the scalar mode (4 reads of
    n_lev rows); the time at hbm_tbs TB/s."""
    b = 0
    for src, dst in chain_rows:
        b += 2 * (src + dst) * nb * 16
    b += 2 * n0 * nb * 16 + nmom * 4 * L * nb * 16
    b -= 4 * n_lev * nb * 16
    return b / (hbm_tbs * 1e12) * 1e3, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stop-factor", type=float, default=0.1)
    ap.add_argument("--flows", action="store_true")
    ap.add_argument("--flow-tol", type=float, default=3e-3)
    ap.add_argument("--hbm-tbs", type=float, default=4.4, help="rate of the byte model: what the stencil sustains")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from deflatedmlmc_schwinger_amd import gateway, matrix, stoch_trace, utils
    from deflatedmlmc_schwinger_amd.engine import (MODE_MLMC, MODE_MLMC_LOOPS, MODE_MLMC_LOOPS_SKIP, MODE_MLMC_SKIP,
                                                   TIMER_NAMES)
    from deflatedmlmc_schwinger_amd.multigrid import MG
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params['use_permuted'] = False          # the scalar modes then solve for the plain probe too: equal work
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "mlmc")
    mg = MG(A)
    with contextlib.redirect_stdout(io.StringIO()):
        mg.setup(dof=tp['dof'], aggrs=tp['aggrs'], max_levels=tp['max_nr_levels'], dim=2,
                 acc_eigvs=tp['accuracy_mg_eigvs'], sys_type='schwinger', params=tp)
    eng = mg.engine
    sizes = [lev.A.shape[0] for lev in mg.ml.levels]
    L = int(tp['latt_dims'][0])
    eng.set_option("stop_factor", args.stop_factor)
    tol, maxiter = 1e-12, 1000
    out = {"lattice": "schwinger128", "level_sizes": sizes, "nb": args.nb, "reps": args.reps,
           "stop_factor": args.stop_factor, "byte_model_tbs": args.hbm_tbs, "momenta": {"p0": [0], "eight": EIGHT},
           "levels": {}}

    eng.set_profiling(True)
    for level, scalar, loops in ((0, MODE_MLMC_SKIP, MODE_MLMC_LOOPS_SKIP), (2, MODE_MLMC, MODE_MLMC_LOOPS)):
        np.random.seed(123456 + level)
        eng.probes_upload(level, utils.draw_probes(args.nb, sizes[level]))
        configs = [("scalar", scalar, [0]), ("p0", loops, [0]), ("eight", loops, EIGHT)]
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
        for name in ("p0", "eight"):
            rec[name]["added_ms"] = rec[name]["device_ms"] - rec["scalar"]["device_ms"]
            rec[name]["over_scalar"] = rec[name]["device_ms"] / rec["scalar"]["device_ms"] - 1.0
            if level > 0:
                chain = [(sizes[l + 1], sizes[l]) for l in range(level - 1, -1, -1)]
                ms, nbytes = byte_model_ms(sizes[0], sizes[level], L, args.nb, len(out["momenta"][name]), chain,
                                           args.hbm_tbs)
                rec[name]["byte_model_ms"] = ms
                rec[name]["byte_model_bytes"] = nbytes
        out["levels"][str(level)] = rec
    eng.set_profiling(False)
    out["bars"] = {"level0_eight_over_scalar_max": 0.10,
                   "met": bool(out["levels"]["0"]["eight"]["over_scalar"] <= 0.10)}

    for name, momenta in (("p0", [0]), ("eight", EIGHT)):
        eng.set_loop_momenta(momenta)
        eng.coarsest_loops()
        eng.sync()
        t0 = time.perf_counter()
        eng.coarsest_loops()
        out.setdefault("coarsest_loops_s", {})[name] = time.perf_counter() - t0
    out["coarsest_columns"] = sizes[-1]
    eng.set_loop_momenta(None)

    if args.flows:
        def flow(which):
            p = gateway.set_params('schwinger128')
            p['function_tol'] = 1e-12
            p['timeslice_loops'] = [0]
            p['stop_factor'] = args.stop_factor
            f = utils.trace_params_from_params(p, which)
            f['tol'] = args.flow_tol
            with contextlib.redirect_stdout(io.StringIO()):
                return (stoch_trace.mlmc_loops if which == "mlmc" else stoch_trace.hutchinson)(A, f)

        rm, rh = flow("mlmc"), flow("hutchinson")
        stoch = [i for i in range(rm['nr_levels'] - 1) if rm['results'][i]['nr_ests'] > 0]
        secs_m = sum(rm['results'][i]['probe_loop_s'] for i in stoch)
        secs_h = rh['probe_loop_s']
        rec = {"tol": args.flow_tol, "mlmc": {"probe_loop_s": secs_m,
                                               "nr_ests": [rm['results'][i]['nr_ests'] + 1 for i in stoch]},
               "hutchinson": {"probe_loop_s": secs_h, "nr_ests": rh['nr_ests'] + 1}}
        for g in ("g3", "1"):
            vm = sum(np.var(utils.loop_gamma(rm['results'][i]['loop_ests'][:, 0], g), axis=0)
                     / (rm['results'][i]['nr_ests'] + 1) for i in stoch)
            vh = np.var(utils.loop_gamma(rh['loop_ests'][:, 0], g), axis=0) / (rh['nr_ests'] + 1)
            rec["mlmc"]["var_x_s_" + g] = float(np.mean(vm) * secs_m)
            rec["hutchinson"]["var_x_s_" + g] = float(np.mean(vh) * secs_h)
            rec["hutchinson_over_mlmc_" + g] = rec["hutchinson"]["var_x_s_" + g] / rec["mlmc"]["var_x_s_" + g]
        out["flows"] = rec

    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
