#!/usr/bin/env python3
"""Cost of the smeared two-point batch next to the plain one, in one process on schwinger128: HIP-event time (the
engine's per-launch event buckets, summed) and wall time of SW_MODE_TWO_POINT and SW_MODE_TWO_POINT_SMEARED batches of
128 noises x momenta [0] (256 solve columns), t0 = 5, kappa = 0.25, 32 source steps, sink levels [0, 32], probes
resident in HBM, the tuned solver hierarchy of the drop-in flow.  The two modes alternate batch by batch so that drift
of the shared machine lands on both alike; the smearing launches' own class is reported and its share of the mode-14
batch is held against the bar of 10 %.  The same file holds the fused 32-step smearing of a 256-column block
(k_smear_fused, one launch) against the chain of 32 one-step launches it replaces (k_smear_step), both through
sw_apply_smearing in the same run, HIP-event time of the smearing class alone.
python tools/smeared_two_point_bench.py [--reps 7] [--out FILE]"""
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
    ap.add_argument("--kappa", type=float, default=0.25)
    ap.add_argument("--source-steps", type=int, default=32)
    ap.add_argument("--sink-steps", type=int, nargs="+", default=[0, 32])
    ap.add_argument("--stop-factor", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from deflatedmlmc_schwinger_amd import gateway, matrix, utils
    from deflatedmlmc_schwinger_amd.engine import (KCLASS_SMEAR, KCLASS_TP_DOTS, KCLASS_TP_SOURCES, MODE_TWO_POINT,
                                                   MODE_TWO_POINT_SMEARED, TIMER_NAMES)
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
    nb = 128
    eng.set_option("stop_factor", args.stop_factor)
    np.random.seed(123456)
    eng.probes_upload_slot(0, 0, utils.draw_probes(nb, n))
    eng.probes_select(0)
    eng.set_two_point(args.t0, [0])
    eng.set_smearing(args.kappa, args.source_steps, args.sink_steps)
    tol, maxiter = 1e-12, 1000
    classes = {"sources": KCLASS_TP_SOURCES, "pair_dots_total": KCLASS_TP_DOTS, "smearing": KCLASS_SMEAR}
    configs = [("mode6", MODE_TWO_POINT), ("mode14", MODE_TWO_POINT_SMEARED)]

    def one(mode):
        eng.timers_reset()
        t0 = time.perf_counter()
        eng.hutch_run(mode, 0, tol, maxiter)
        eng.sync()
        w = (time.perf_counter() - t0) * 1e3
        return w, eng.timers(), {k: eng.kernel_stats(c) for k, c in classes.items()}

    eng.set_profiling(True)
    acc = {name: {"dev": [], "wall": [], "cls": {k: [] for k in classes}} for name, _ in configs}
    for rep in range(args.warmup + args.reps):
        for name, mode in configs:
            w, t, cls = one(mode)
            if rep >= args.warmup:
                a = acc[name]
                a["dev"].append(sum(t.values()))
                a["wall"].append(w)
                for k in classes:
                    a["cls"][k].append(cls[k][0])
                a["buckets"] = t
                a["launches"] = {k: cls[k][1] for k in classes}
                a["iters_max"] = int(eng.hutch_fetch()[1].max())
    out = {"lattice": "schwinger128", "reps": args.reps, "stop_factor": args.stop_factor, "source_timeslice": args.t0,
           "noises": nb, "solve_columns": 2 * nb, "momenta": [0], "smearing_kappa": args.kappa,
           "source_smearing_steps": args.source_steps, "sink_smearing_steps": list(args.sink_steps)}
    for name, _ in configs:
        a = acc[name]
        dev = float(np.median(a["dev"]))
        out[name] = {"device_ms": dev, "device_ms_all": [round(v, 4) for v in a["dev"]],
                     "wall_ms": float(np.median(a["wall"])), "iters_max": a["iters_max"],
                     "device_ms_per_outer_iteration": dev / max(1, a["iters_max"]),
                     "buckets_ms": {k: round(a["buckets"][k], 4) for k in TIMER_NAMES},
                     "launches": a["launches"]}
        for k in classes:
            out[name][k + "_ms"] = float(np.median(a["cls"][k]))
    out["mode14"]["smearing_share"] = out["mode14"]["smearing_ms"] / out["mode14"]["device_ms"]
    out["mode14"]["over_mode6"] = out["mode14"]["device_ms"] / out["mode6"]["device_ms"] - 1.0

    # the sink smearing of one 256-column block alone: fused against the chain it replaces, alternating
    steps = max(args.sink_steps)
    rng = np.random.default_rng(7)
    X = rng.standard_normal((2 * nb, n)) + 1j * rng.standard_normal((2 * nb, n))
    kinds = {"fused": True, "chain": False}
    ms = {k: [] for k in kinds}
    launches = {}
    same = None
    for rep in range(args.warmup + args.reps):
        res = {}
        for k, fused in kinds.items():
            eng.timers_reset()
            res[k] = eng.apply_smearing(X, steps, fused=fused)
            t, cnt = eng.kernel_stats(KCLASS_SMEAR)
            launches[k] = cnt
            if rep >= args.warmup:
                ms[k].append(t)
        same = bool(np.array_equal(res["fused"], res["chain"]))
    eng.set_profiling(False)
    field_mb = 2 * nb * n * 16 / 1e6
    out["sink_smearing_256_columns"] = {
        "steps": steps, "field_MB": field_mb, "bit_identical": same,
        "fused_ms": float(np.median(ms["fused"])), "fused_ms_all": [round(v, 4) for v in ms["fused"]],
        "chain_ms": float(np.median(ms["chain"])), "chain_ms_all": [round(v, 4) for v in ms["chain"]],
        "launches": launches,
        "chain_TB_per_s": 2 * field_mb * steps / 1e6 / (float(np.median(ms["chain"])) / 1e3),
        "fused_over_one_read_one_write_at_4.4_TB_per_s": float(np.median(ms["fused"])) / (2 * field_mb / 4.4e3)}
    out["sink_smearing_256_columns"]["speedup"] = (out["sink_smearing_256_columns"]["chain_ms"]
                                                   / out["sink_smearing_256_columns"]["fused_ms"])
    eng.set_smearing(1.0, 0, None)
    eng.set_two_point(0, None)
    out["bars"] = {"smearing_share_max": 0.10, "met": bool(out["mode14"]["smearing_share"] <= 0.10),
                   "fused_faster_than_chain": bool(out["sink_smearing_256_columns"]["speedup"] > 1.0)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
