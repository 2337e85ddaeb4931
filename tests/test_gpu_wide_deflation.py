"""GPU: deflation with up to 256 vectors.  The registered projection (sw_apply_deflation: the fp64-MFMA pair
k_defl_gemm_dots / k_defl_gemm_apply above 64 vectors, and under defl_gemm = 1 at every rank) against NumPy,
the eigen kernels of blocks wider than 64 (k_block_gram_wide, k_block_rotate_wide) against NumPy, the device
eigensolver at k = 64 / 128 against ARPACK, deflated probes with 128 / 96 vectors against the sparse-LU
oracle, and the hutchinson flow with 128 device deflation vectors against the exact trace."""
import contextlib
import io
import json
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import gateway, hierarchy, matrix, setup_gpu, stoch_trace, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import MODE_HUTCHINSON, MODE_MLMC_SKIP  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG, SOLVER_HID  # noqa: E402
from oracle import ref_path as rp  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden.json")


@pytest.fixture(scope="module")
def p128():
    """The MLMC reference hierarchy of schwinger128 on the engine (hierarchy 0 with all its levels)."""
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "mlmc")
    mg = MG(A)
    mg.setup(dof=tp['dof'], aggrs=tp['aggrs'], max_levels=tp['max_nr_levels'], dim=2,
             acc_eigvs=tp['accuracy_mg_eigvs'], sys_type='schwinger', params=tp)
    mg.total_levels = len(mg.ml.levels)
    return A, tp, mg


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _orthonormal(n, k, seed):
    Q, _ = np.linalg.qr(_rand((n, k), seed))
    return Q


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _restore_perm(mg):
    shift = int(getattr(mg.ml.levels[0], "perm_shift", 0) or 0)
    mg.engine.set_perm(0, shift if shift > 0 else -1)


def test_apply_deflation_against_numpy(p128):
    """Both forms for kd in {65, 128, 256} (the MFMA kernels), the Hutchinson form with and without the
    Pperm^T gather, 70 vectors (a padded probe chunk)."""
    A, tp, mg = p128
    eng = mg.engine
    n0 = A.shape[0]
    shift = 128 * 2 * 2
    X = _rand((70, n0), 1)
    try:
        for kd in (65, 128, 256):
            U = _rand((n0, kd), 10 + kd)
            eng.set_deflation(U)
            proj = (X.T - U @ (U.conj().T @ X.T)).T
            eng.set_perm(0, -1)
            err = _rel(eng.apply_deflation(0, 0, X), proj)
            eng.set_perm(0, shift)
            # Pperm^T: (Pperm^T v)[r] = v[(r - shift) mod n]
            err_p = _rel(eng.apply_deflation(0, 0, X), np.roll(proj, shift, axis=1))
            print("hutchinson form kd %d: rel err %.2e, permuted %.2e" % (kd, err, err_p))
            assert err < 1e-13 and err_p < 1e-13, (kd, err, err_p)
            for level in (0, 1):
                n = mg.ml.levels[level].A.shape[0]
                V = _rand((n, kd), 20 + kd + level)
                Xl = _rand((9, n), 30 + level)
                eng.set_level_deflation(level, V)
                ref = (Xl.T - V @ (V.conj().T @ Xl.T)).T
                err = _rel(eng.apply_deflation(1, level, Xl), ref)
                print("MLMC form level %d kd %d: rel err %.2e" % (level, kd, err))
                assert err < 1e-13, (level, kd, err)
                eng.set_level_deflation(level, None)
    finally:
        eng.set_deflation(None)
        _restore_perm(mg)


def test_mfma_deflation_agrees_with_the_dot_kernels_at_small_rank(p128):
    """defl_gemm = 1 runs the MFMA kernels where the default runs k_defl_dots / k_defl_apply."""
    A, tp, mg = p128
    eng = mg.engine
    n0 = A.shape[0]
    X = _rand((64, n0), 2)
    saved = eng.get_option("defl_gemm")
    try:
        eng.set_perm(0, 128 * 2 * 2)
        for kd in (8, 64):
            U = _orthonormal(n0, kd, 40 + kd)
            eng.set_deflation(U)
            eng.set_option("defl_gemm", 0)
            a = eng.apply_deflation(0, 0, X)
            eng.set_option("defl_gemm", 1)
            b = eng.apply_deflation(0, 0, X)
            err = _rel(b, a)
            print("kd %d: defl_gemm 1 against 0: rel diff %.2e" % (kd, err))
            assert err < 1e-13, (kd, err)
    finally:
        eng.set_option("defl_gemm", saved)
        eng.set_deflation(None)
        _restore_perm(mg)


def _solver_only():
    params = gateway.set_params('schwinger128')
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    lat = hierarchy.detect_lattice(A)
    mg = MG(A)
    mg.setup_solver_only(hierarchy.auto_solver_cfg(lat[0]), device=0, engines=1)
    return A, mg


@pytest.mark.parametrize("width", [128, 512])
def test_wide_block_kernels_against_numpy(width):
    A, mg = _solver_only()
    eng = mg.engine
    n = A.shape[0]
    V = _rand((width, n), 3)
    W = _rand((width, n), 4)
    Y = _rand((width, width), 5)
    eng.eig_begin(SOLVER_HID, 0, width=width)
    try:
        eng.eig_load(0, V)
        eng.eig_load(1, W)
        G = eng.eig_gram(0, 1)
        ref = V.conj() @ W.T
        assert G.shape == (width, width)
        assert np.abs(G - ref).max() / np.abs(ref).max() < 1e-13
        eng.eig_rotate(0, Y, 2)
        out = eng.eig_fetch(2, width)
        ref = (V.T @ Y).T
        assert np.abs(out - ref).max() / np.abs(ref).max() < 1e-13
        eng.eig_rotate(0, Y, 2, sub=1)
        out = eng.eig_fetch(2, width)
        assert np.abs(out - (W - ref)).max() / np.abs(ref).max() < 1e-13
        # fewer columns than the block: the rest of the loaded buffer is zero
        eng.eig_load(0, V[:70])
        assert np.abs(eng.eig_fetch(0, 70) - V[:70]).max() == 0.0
    finally:
        eng.eig_end()
    eng.close()


def test_device_eigsh_with_64_and_128_pairs():
    """eigsh(gamma_3 A, k, sigma=0) on the GPU with blocks of 128 and 256 vectors against ARPACK (k = 64),
    and ARPACK's shift-invert criterion plus orthonormality at k = 128."""
    A, mg = _solver_only()
    eng = mg.engine
    n = A.shape[0]
    g3 = np.ones(n)
    g3[n // 2:] = -1.0
    Q = (sp.diags(g3) @ A).tocsc()
    lu = spla.splu(Q)
    tol = 1e-9
    for k in (64, 128):
        log = []
        t0 = time.time()
        lam, X = setup_gpu.device_eigenpairs(eng, SOLVER_HID, 0, k, tol, hermitian_g3=True, log=log,
                                             width=setup_gpu.eig_width_for(k))
        t_dev = time.time() - t0
        assert X.shape == (n, k)
        assert np.abs(X.conj().T @ X - np.eye(k)).max() < 1e-12
        res = np.linalg.norm(lu.solve(X) - X / lam[None, :], axis=0) * np.abs(lam)
        print("k %d: device %.2f s, %d steps, shift-invert residual max %.2e" % (k, t_dev, len(log), res.max()))
        # the solver measured this with its own inexact solves; the LU solves here are exact
        assert res.max() <= 10 * tol
        if k == 64:
            t0 = time.time()
            # the reference iterated well below tol, so that the angle measures the device vectors' error
            S, Vq = spla.eigsh(Q, k=k, which='LM', tol=1e-12, sigma=0.0)
            print("k %d: host ARPACK %.2f s" % (k, time.time() - t0))
            assert np.max(np.abs(np.sort(S) - np.sort(lam)) / np.abs(np.sort(S))) < 1e-8
            # sine of the largest principal angle, ||(I - X X^H) Vq||_2 (not sqrt(1 - cos^2): that loses half the digits)
            sine = np.linalg.norm(Vq - X @ (X.conj().T @ Vq), 2)
            print("k %d: subspace sine %.2e" % (k, sine))
            assert sine < 1e-7
    eng.close()


def test_device_difference_eigenpairs_with_48_pairs(p128):
    """eigsh(Q_0, 48, which='LM') of the level-0 difference operator (with level skipping) on a block of 128."""
    A, tp, mg = p128
    lv = mg.ml.levels
    cinv = np.asarray(mg.coarsest_inv)
    lus = {}

    def solve(level, B):
        if level not in lus:
            lus[level] = rp.LUSolver(lv[level].A)
        return lus[level](B)

    def diff(X):
        X = np.array(X, dtype=np.complex128)
        X[X.shape[0] // 2:] *= -1.0
        Z = solve(0, X)
        Xc = lv[1].R @ (lv[0].R @ X)
        Yc = cinv @ Xc if len(lv) == 3 else solve(2, Xc)
        return Z - lv[0].P @ (lv[1].P @ np.asarray(Yc))

    mg.solve_tol = 1e-11
    mg.skip_level = True
    try:
        k = 48
        log = []
        t0 = time.time()
        lam, X = mg.device_diff_eigenpairs(0, k, 1e-6, log=log, width=setup_gpu.eig_width_for(k))
        print("difference operator k %d: device %.2f s, %d steps" % (k, time.time() - t0, len(log)))
        QX = diff(X)
        res = np.linalg.norm(QX - X * lam[None, :], axis=0) / np.abs(lam)
        assert res.max() <= 1e-5, res
        assert np.abs(X.conj().T @ X - np.eye(k)).max() < 1e-12
        n = A.shape[0]
        op = spla.LinearOperator((n, n), dtype=np.complex128, matvec=lambda v: diff(v.reshape(-1, 1))[:, 0])
        ref = spla.eigsh(op, k=k, which='LM', tol=1e-10, return_eigenvectors=False)
        assert np.max(np.abs(np.sort(lam) - np.sort(ref)) / np.abs(np.sort(ref))) < 1e-6
    finally:
        mg.skip_level = False
        mg.solve_tol = tp['function_params']['tol']


def test_deflated_probes_with_128_and_96_vectors_match_lu(p128):
    """256 Hutchinson probes with 128 deflation vectors (with the Pperm^T gather) at 1e-10, and MLMC_SKIP probes
    with 96 level-0 vectors at 1e-9, against the sparse-LU oracle."""
    A, tp, mg = p128
    eng = mg.engine
    lv = mg.ml.levels
    n = A.shape[0]
    lu = rp.LUSolver(A)
    shift = 128 * 2 * 2
    PpermT = sp.csr_matrix((np.ones(n), (np.arange(n), (np.arange(n) - shift) % n)), shape=(n, n))
    U = _orthonormal(n, 128, 7)
    np.random.seed(5151)
    probes = utils.draw_probes(256, n)
    try:
        eng.set_deflation(U)
        eng.set_perm(0, shift)
        ests, _, _ = eng.hutch_batch(MODE_HUTCHINSON, 0, probes, 1e-12, 1000)
        worst = 0.0
        for j in range(256):
            x = probes[j].astype(np.complex128)
            ref = rp.hutch_probe(x, lu, U, PpermT)
            worst = max(worst, abs(ests[j] - ref) / abs(ref))
        print("hutchinson, 128 vectors, 256 probes: max rel err %.2e" % worst)
        assert worst < 1e-10
    finally:
        eng.set_deflation(None)
        _restore_perm(mg)
    cinv = np.asarray(mg.coarsest_inv)
    lus = {0: lu}

    def solve(level, B):
        if level not in lus:
            lus[level] = rp.LUSolver(lv[level].A)
        return lus[level](B)

    Vx = _orthonormal(n, 96, 8)
    try:
        for e in utils._engines(mg):
            e.set_level_deflation(0, Vx)
        probes = utils.draw_probes(8, n)
        ests, _, _ = eng.hutch_batch(MODE_MLMC_SKIP, 0, probes, 1e-12, 1000)
        for j in range(8):
            x0 = probes[j].astype(np.complex128)
            ref = rp.mlmc_probe(x0, 0, lv, True, solve, cinv, tp['use_permuted'], Vx=Vx)
            xd = x0 - Vx @ (Vx.conj().T @ x0)
            scale = max(abs(np.vdot(x0, solve(0, xd))), abs(ref), 1.0)
            assert abs(ests[j] - ref) / scale < 1e-9, (j, ests[j], ref)
    finally:
        for e in utils._engines(mg):
            e.set_level_deflation(0, None)


def test_hutchinson_flow_with_128_device_deflation_vectors():
    g = json.load(open(GOLDEN))
    exact = complex(*g["exact_trace_128_plain"])
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params['use_permuted'] = False
    params['nr_deflat_vctrs'] = 128
    params['defl_setup'] = "device"
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "hutchinson")
    assert tp['defl_setup'] == "device"
    with contextlib.redirect_stdout(io.StringIO()):
        res = stoch_trace.hutchinson(A, tp)
    err = res['std_dev'] / np.sqrt(res['nr_ests'])
    print("hutchinson 128^2, 128 device vectors: trace %r, exact %r, per-probe std %.4g, %d probes"
          % (res['trace'], exact, res['std_dev'], res['nr_ests']))
    assert abs(res['trace'] - exact) < 4.0 * err + 1e-9
