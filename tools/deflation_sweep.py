"""Deflated Hutchinson on schwinger128 against the number of deflation vectors (GPU only).

For each k: the device eigensolve of gamma_3 A (block width 64 ceil(2k/64)) and, with --host-max >= k, host
ARPACK; the time of one 256-probe batch with and without the k-vector projection (host clock around a
synchronised batch), the engine's `defl` timer bucket per batch, the sample standard deviation of the
per-probe estimates, and variance x batch time (the cost to a fixed error).  One JSON object on stdout.

    python tools/deflation_sweep.py [--ks 0,8,32,64,128,256] [--probes 2048] [--host-max 64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402
import scipy.sparse.linalg as spla  # noqa: E402

from deflatedmlmc_schwinger_amd import gateway, matrix, setup_gpu, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import MODE_HUTCHINSON  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG  # noqa: E402

BATCH = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="0,8,32,64,128,256")
    ap.add_argument("--probes", type=int, default=2048, help="probes per k (a multiple of 256)")
    ap.add_argument("--host-max", type=int, default=64, help="largest k also solved by host ARPACK")
    ap.add_argument("--tol", type=float, default=1e-9, help="eigensolver tolerance")
    ap.add_argument("--function-tol", type=float, default=1e-12, help="probe solve tolerance")
    a = ap.parse_args()
    ks = [int(v) for v in a.ks.split(",")]
    nbatch = max(1, a.probes // BATCH)

    params = gateway.set_params('schwinger128')
    params['function_tol'] = a.function_tol
    params['use_permuted'] = False
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "hutchinson")
    tp['nr_deflat_vctrs'] = 0
    mg = MG(A)
    mg.setup(dof=tp['dof'], aggrs=tp['aggrs'], max_levels=tp['max_nr_levels'], dim=2,
             acc_eigvs=tp['accuracy_mg_eigvs'], sys_type='schwinger', params=tp)
    eng = mg.engine
    n = A.shape[0]
    g3 = mg.ml.levels[0].g3
    ftol = params['function_tol']

    def batches(seed):
        """per-probe estimates and median per-batch seconds over nbatch batches (one warm-up), then the `defl`
        timer bucket (ms) of one more batch with the HIP-event timers on (kept out of the timed batches)"""
        np.random.seed(seed)
        warm = utils.draw_probes(BATCH, n)
        eng.hutch_batch(MODE_HUTCHINSON, 0, warm, ftol, 1000)
        ests, secs = [], []
        for _ in range(nbatch):
            probes = utils.draw_probes(BATCH, n)
            eng.sync()
            t0 = time.perf_counter()
            e, _, _ = eng.hutch_batch(MODE_HUTCHINSON, 0, probes, ftol, 1000)
            eng.sync()
            secs.append(time.perf_counter() - t0)
            ests.append(np.asarray(e))
        eng.set_profiling(True)
        eng.timers_reset()
        eng.hutch_batch(MODE_HUTCHINSON, 0, warm, ftol, 1000)
        defl = eng.timers()["defl"]
        eng.set_profiling(False)
        return np.concatenate(ests), float(np.median(secs)), float(defl)

    eng.set_deflation(None)
    _, t_plain, _ = batches(777)
    rows = []
    for k in ks:
        row = {"k": k}
        tr1 = 0.0
        if k > 0:
            t0 = time.time()
            lam, X = mg.device_eigenpairs(k, a.tol, hermitian=True, width=setup_gpu.eig_width_for(k))
            row["eigsolve_device_s"] = round(time.time() - t0, 3)
            if k <= a.host_max:
                Q = (g3 * A).tocsc()
                t0 = time.time()
                spla.eigsh(Q, k=k, which='LM', tol=a.tol, sigma=0.0)
                row["eigsolve_host_arpack_s"] = round(time.time() - t0, 3)
            sgn = np.where(lam > 0, 1.0, -1.0)
            U = g3 @ (X * sgn[None, :])
            tr1 = float(np.real(np.sum(np.einsum("ik,ik->k", U.conj(), X) / np.abs(lam))))
            eng.set_deflation(U)
        else:
            eng.set_deflation(None)
        ests, t_batch, defl_ms = batches(1000 + k)
        var = float(np.var(ests.real, ddof=1))
        row.update({"batch_s_undeflated": round(t_plain, 5), "batch_s": round(t_batch, 5),
                    "defl_ms_per_batch": round(defl_ms, 4), "probes": int(ests.size),
                    "std_dev": float(np.sqrt(var)), "trace": float(np.mean(ests.real)) + tr1,
                    "variance_x_batch_s": var * t_batch})
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    eng.set_deflation(None)
    print(json.dumps({"lattice": "schwinger128", "batch": BATCH, "function_tol": ftol, "rows": rows}))


if __name__ == "__main__":
    main()
