#!/usr/bin/env python3
"""Cost of the low-mode two-point functions of one momentum on schwinger128, in one process, median of --reps, the two
paths alternating:
  host    eng.meson_fields(p, k) followed by utils.low_mode_two_point(Phi[None], G): the fields read back, the triple
          products and the contraction in NumPy with the thread count of the environment; wall-clock time.
  device  eng.low_mode_two_point(p): wall-clock time, and the HIP-event time of its kernel class (k_cgemm_nt and
          k_lm_two_point_reduce, sw_kernel_stats class 21; k_meson_field is class 20) as a fraction of
          8 (2 * 4L * ld^3 + (4L)^2 k^2) flops over the engine's measured v_mfma_f64 issue rate (48.1 TFLOP/s,
          profiles/r01_mfma_f64_rate.txt) and against its byte model at the stencil's stream rate (4.4 TB/s): Phi
          read by the first product and by the contraction, W^T written and read, Psi written and read
          (6 * 64 L k^2), the split-K partial sums written and read and the result written (16 (4L)^2 (2 S + 1)).
k = 16, 64, 256 and p = 0, 1; random orthonormal vectors and a random G (the timings do not depend on the values).  The
largest difference between the two paths relative to the largest entry is recorded per configuration.
python tools/low_mode_two_point_bench.py [--reps 7] [--out profiles/low_mode_two_point_128.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F64_TFLOPS = 48.1
STREAM_TBS = 4.4


def splits(L, k):
    """The number of K splits sw_low_mode_two_point uses (shapes only)."""
    tiles = ((4 * L + 63) // 64) ** 2
    steps = (k * k + 15) // 16
    want = min(steps, 64, max(1, 1024 // tiles))
    kchunk = 16 * ((steps + want - 1) // want)
    return (k * k + kchunk - 1) // kchunk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ranks", default="16,64,256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from deflatedmlmc_schwinger_amd import gateway, matrix, utils
    from deflatedmlmc_schwinger_amd.engine import KCLASS_LM_CONTRACT, KCLASS_MESON_FIELD
    from deflatedmlmc_schwinger_amd.multigrid import MG, REF_HID, _new_engine
    params = gateway.set_params('schwinger128')
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    lat = MG(A)._lattice()
    L, n = int(lat[0]), A.shape[0]
    eng = _new_engine(0)
    eng.hier_begin(REF_HID, 1)
    eng.set_lattice(REF_HID, lat[0], lat[1], lat[2], lat[3])
    eng.hier_end(REF_HID)
    ranks = [int(x) for x in args.ranks.split(",")]
    rng = np.random.default_rng(1)
    out = {"lattice": "schwinger128", "reps": args.reps, "mfma_f64_tflops": MFMA_F64_TFLOPS,
           "stream_tbs": STREAM_TBS, "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "configs": {}}
    eng.set_profiling(True)
    for k in ranks:
        Q, _ = np.linalg.qr(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))
        G = rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k))
        eng.set_deflation(np.ascontiguousarray(Q))
        eng.set_low_mode_inverse(G)
        for p in (0, 1):
            host_s, dev_s, ev_ms, mf_ms = [], [], [], []
            diff = None
            for rep in range(args.warmup + args.reps):
                t = time.perf_counter()
                Eh = utils.low_mode_two_point(eng.meson_fields(p, k)[None], G)[0]
                th = time.perf_counter() - t
                eng.timers_reset()
                t = time.perf_counter()
                Ed = eng.low_mode_two_point(p)
                td = time.perf_counter() - t
                ms, launches = eng.kernel_stats(KCLASS_LM_CONTRACT)
                assert launches == 4
                if rep >= args.warmup:
                    host_s.append(th)
                    dev_s.append(td)
                    ev_ms.append(ms)
                    mf_ms.append(eng.kernel_stats(KCLASS_MESON_FIELD)[0])
                diff = float(np.max(np.abs(Ed - Eh)) / np.max(np.abs(Eh)))
                flops = eng.kernel_work(KCLASS_LM_CONTRACT)
            S = splits(L, k)
            nbytes = 6 * 64.0 * L * k * k + 16.0 * (4 * L) ** 2 * (2 * S + 1)
            ms = float(np.median(ev_ms))
            t_mfma = flops / (MFMA_F64_TFLOPS * 1e12) * 1e3
            t_bytes = nbytes / (STREAM_TBS * 1e12) * 1e3
            rec = {"host_s": float(np.median(host_s)), "host_s_all": [round(x, 5) for x in host_s],
                   "device_s": float(np.median(dev_s)), "device_s_all": [round(x, 5) for x in dev_s],
                   "host_over_device": float(np.median(host_s) / np.median(dev_s)),
                   "contract_event_ms": ms, "contract_event_ms_all": [round(x, 5) for x in ev_ms],
                   "meson_field_event_ms": float(np.median(mf_ms)), "splits": S, "flops": flops, "bytes": nbytes,
                   "mfma_model_ms": t_mfma, "bytes_model_ms": t_bytes, "fraction_of_mfma_rate": t_mfma / ms,
                   "fraction_of_stream_rate": t_bytes / ms, "bound": "mfma" if t_mfma > t_bytes else "bytes",
                   "max_rel_diff_device_host": diff}
            out["configs"]["k%d_p%d" % (k, p)] = rec
            print("k=%d p=%d: host %.4f s, device %.4f s (contraction kernels %.3f ms, %.2f of the MFMA rate)"
                  % (k, p, rec["host_s"], rec["device_s"], ms, rec["fraction_of_mfma_rate"]), flush=True)
    eng.set_profiling(False)
    eng.set_deflation(None)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
