#!/usr/bin/env python3
"""Cost of the low-mode averaging on schwinger128, in one process, median of --reps, HIP-event time, configurations
alternating:
  kernel  k_meson_field (sw_kernel_stats class 20) at k = 16, 64, 256 vectors and p = 0 / p = 1: time, the fraction of
          8 * 4 * L^2 * ld^2 flops over the engine's measured v_mfma_f64 issue rate (48.1 TFLOP/s,
          profiles/r01_mfma_f64_rate.txt) and the bytes -- the dense output, 64 L k^2, plus one read of U, 32 L^2 ld --
          over the stencil's stream rate (4.4 TB/s); the larger of the two model times is the bound.
  batch   a SW_MODE_TWO_POINT_LMA batch (128 noises x momenta [0], k = 16 and 64) next to a SW_MODE_TWO_POINT batch of
          the same width: the added device time against its byte model -- the projection passes (one read of the
          sources for U^H eta, one write of z_L, U read by both: 2 * 16 n ncols + 2 * 16 n ld bytes) plus one more
          pair-dot pass (16 n ncols) at the stream rate.
The vectors are random (orthonormalised) and G is the identity: neither the kernels' time nor the solve depends on
their values.
python tools/meson_fields_bench.py [--reps 7] [--out profiles/meson_fields_128.json]"""
import argparse
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_NUM_THREADS", "1")

MFMA_F64_TFLOPS = 48.1
STREAM_TBS = 4.4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--t0", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from deflatedmlmc_schwinger_amd import gateway, matrix, utils
    from deflatedmlmc_schwinger_amd.engine import (KCLASS_MESON_FIELD, KCLASS_TP_DOTS, MODE_TWO_POINT,
                                                   MODE_TWO_POINT_LMA, TIMER_NAMES)
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
    L = int(tp['latt_dims'][0])
    rng = np.random.default_rng(1)
    basis = {}
    for k in (16, 64, 256):
        Q, _ = np.linalg.qr(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))
        basis[k] = np.ascontiguousarray(Q)
    out = {"lattice": "schwinger128", "reps": args.reps, "mfma_f64_tflops": MFMA_F64_TFLOPS,
           "stream_tbs": STREAM_TBS, "kernel": {}, "batch": {}}

    # ---- the kernel ----
    eng.set_profiling(True)
    times = {(k, p): [] for k in (16, 64, 256) for p in (0, 1)}
    for rep in range(args.warmup + args.reps):
        for k in (16, 64, 256):
            eng.set_deflation(basis[k])
            for p in (0, 1):
                eng.timers_reset()
                eng.meson_fields(p, k)
                ms, launches = eng.kernel_stats(KCLASS_MESON_FIELD)
                assert launches == 1
                if rep >= args.warmup:
                    times[(k, p)].append(ms)
    for (k, p), v in times.items():
        ld = (k + 15) // 16 * 16
        ms = float(np.median(v))
        flops = 32.0 * L * L * ld * ld
        nbytes = 64.0 * L * k * k + 32.0 * L * L * ld
        t_mfma = flops / (MFMA_F64_TFLOPS * 1e12) * 1e3
        t_bytes = nbytes / (STREAM_TBS * 1e12) * 1e3
        out["kernel"]["k%d_p%d" % (k, p)] = {
            "ms": ms, "ms_all": [round(x, 5) for x in v], "flops": flops, "bytes": nbytes,
            "mfma_model_ms": t_mfma, "bytes_model_ms": t_bytes, "fraction_of_mfma_rate": t_mfma / ms,
            "fraction_of_stream_rate": t_bytes / ms, "bound": "mfma" if t_mfma > t_bytes else "bytes"}

    # ---- the batch ----
    np.random.seed(123456)
    probes = utils.draw_probes(128, n)
    eng.probes_upload_slot(0, 0, probes)
    eng.probes_select(0)
    eng.set_two_point(args.t0, [0])
    eng.set_option("stop_factor", 0.1)
    configs = [("mode6", MODE_TWO_POINT, None), ("lma_k16", MODE_TWO_POINT_LMA, 16),
               ("lma_k64", MODE_TWO_POINT_LMA, 64)]
    acc = {c[0]: {"dev": [], "defl": [], "dots": [], "buckets": None} for c in configs}
    for rep in range(args.warmup + args.reps):
        for name, mode, k in configs:
            if k is not None:
                eng.set_deflation(basis[k])
                eng.set_low_mode_inverse(np.eye(k))
            eng.timers_reset()
            eng.hutch_run(mode, 0, 1e-12, 1000)
            eng.sync()
            t = eng.timers()
            if rep >= args.warmup:
                acc[name]["dev"].append(sum(t.values()))
                acc[name]["defl"].append(t["defl"])
                acc[name]["dots"].append(eng.kernel_stats(KCLASS_TP_DOTS)[0])
                acc[name]["buckets"] = t
                acc[name]["iters_max"] = int(eng.hutch_fetch()[1].max())
    eng.set_profiling(False)
    ncols = 2 * 128
    for name, _, k in configs:
        a = acc[name]
        rec = {"device_ms": float(np.median(a["dev"])), "device_ms_all": [round(x, 4) for x in a["dev"]],
               "defl_ms": float(np.median(a["defl"])), "pair_dots_ms": float(np.median(a["dots"])),
               "iters_max": a["iters_max"], "buckets_ms": {q: round(a["buckets"][q], 4) for q in TIMER_NAMES}}
        if k is not None:
            ld = (k + 15) // 16 * 16
            base = out["batch"]["mode6"]
            added = rec["device_ms"] - base["device_ms"]
            model_bytes = 2 * 16.0 * n * ncols + 2 * 16.0 * n * ld + 16.0 * n * ncols
            rec.update({"k": k, "added_ms": added, "added_share": added / base["device_ms"],
                        "added_kernels_ms": rec["defl_ms"] + rec["pair_dots_ms"] - base["pair_dots_ms"],
                        "model_bytes": model_bytes, "model_ms": model_bytes / (STREAM_TBS * 1e12) * 1e3})
            rec["added_kernels_over_model"] = rec["added_kernels_ms"] / rec["model_ms"]
        out["batch"][name] = rec
    eng.set_two_point(0, None)
    eng.set_deflation(None)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
