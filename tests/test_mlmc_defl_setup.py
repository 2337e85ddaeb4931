"""CPU: the block eigensolver of the MLMC difference-level deflation (setup_gpu.block_eigenpairs in its
largest-magnitude mode) driven through a NumPy stand-in of the engine's eigen buffers, and the plumbing of
the build-only key mlmc_defl_setup."""
import numpy as np
import pytest

from deflatedmlmc_schwinger_amd import gateway, matrix, setup_gpu, stoch_trace, utils
from deflatedmlmc_schwinger_amd.multigrid import MG


class FakeEigenEngine:
    """The sw_eig_* calls of the engine on a dense Hermitian matrix Q: three [n][64] blocks,
    eig_apply_diff = Q (the difference operator), eig_solve = Q^-1 (the shift-invert)."""

    def __init__(self, Q, seed=5):
        self.Q = Q
        self.Qinv = np.linalg.inv(Q)
        self.n = Q.shape[0]
        self.rng = np.random.default_rng(seed)
        self.buf = None
        self.applies = 0

    def eig_begin(self, hid, level, seed=11):
        self.buf = [np.zeros((self.n, 64), dtype=np.complex128) for _ in range(3)]
        self.buf[0] = self.rng.standard_normal((self.n, 64)) + 1j * self.rng.standard_normal((self.n, 64))

    def eig_load(self, dst, X):
        X = np.atleast_2d(X)
        self.buf[dst][:, :X.shape[0]] = X.T

    def eig_apply_diff(self, src, dst, skip, g3, tol, maxiter=1000):
        assert src != dst
        self.buf[dst] = self.Q @ self.buf[src]
        self.applies += 1
        return 3

    def eig_solve(self, src, dst, mode, tol, maxiter=1000):
        assert src != dst
        self.buf[dst] = self.Qinv @ self.buf[src]
        return 4

    def eig_gram(self, a, b):
        return self.buf[a].conj().T @ self.buf[b]

    def eig_rotate(self, src, Y, dst, sub=-1):
        assert src != dst and Y.shape == (64, 64)
        out = self.buf[src] @ Y
        self.buf[dst] = out if sub < 0 else self.buf[sub] - out

    def eig_fetch(self, src, k):
        return self.buf[src][:, :k].T.copy()

    def eig_end(self):
        self.buf = None


def _designed_matrix(n=512, seed=3):
    """Hermitian, 24 eigenvalues of large modulus and both signs, the rest small (none near zero
    closer than 1e-2, so the shift-invert mode is well conditioned)."""
    rng = np.random.default_rng(seed)
    big = np.geomspace(40.0, 2.0, 24) * np.where(np.arange(24) % 3 == 1, -1.0, 1.0)
    small = np.linspace(0.01, 0.5, n - 24) * rng.choice([-1.0, 1.0], n - 24)
    lam = np.concatenate([big, small])
    U, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    Q = (U * lam[None, :]) @ U.conj().T
    return 0.5 * (Q + Q.conj().T), lam


def _check_pairs(Q, lam, X, want, tol):
    got = np.sort(lam)
    ref = np.sort(want)
    assert np.max(np.abs(got - ref) / np.abs(ref)) < 1e-10, (got, ref)
    R = Q @ X - X * lam[None, :]
    res = np.linalg.norm(R, axis=0) / np.abs(lam)
    assert res.max() <= tol * 1.0001, res
    assert np.abs(X.conj().T @ X - np.eye(X.shape[1])).max() < 1e-12


@pytest.mark.parametrize("k", [8, 16])
def test_largest_magnitude_pairs_of_a_hermitian_operator(k):
    Q, spec = _designed_matrix()
    w = np.linalg.eigvalsh(Q)
    want = w[np.argsort(-np.abs(w))[:k]]
    eng = FakeEigenEngine(Q)
    log = []
    tol = 1e-9
    lam, X = setup_gpu.device_diff_eigenpairs(eng, 0, k, tol, 1e-11, log=log)
    assert lam.dtype == np.float64 and X.shape == (Q.shape[0], k)
    _check_pairs(Q, lam, X, want, tol)
    # both signs among the wanted pairs, one operator application per step
    assert (lam > 0).any() and (lam < 0).any()
    assert eng.applies == len(log) and log[-1]["residual_max"] <= tol
    assert all(r["solve_tol"] == 1e-11 and r["solve_iterations"] == 3 for r in log)


def test_shift_invert_mode_still_returns_the_pairs_nearest_zero():
    Q, _ = _designed_matrix()
    w = np.linalg.eigvalsh(Q)
    k = 8
    want = w[np.argsort(np.abs(w))[:k]]
    tol = 1e-9
    for hermitian in (True, False):
        eng = FakeEigenEngine(Q)
        lam, X = setup_gpu.device_eigenpairs(eng, 1, 0, k, tol, hermitian_g3=hermitian)
        lam = np.real_if_close(lam, tol=1e6)
        assert np.max(np.abs(np.sort(lam.real) - np.sort(want)) / np.abs(np.sort(want))) < 1e-10
        assert eng.applies == 0
        # the shift-invert criterion |Q^-1 x - x / lambda| <= tol / |lambda|
        R = eng.Qinv @ X - X / lam[None, :]
        assert (np.linalg.norm(R, axis=0) * np.abs(lam)).max() <= tol * 1.0001


def test_block_width_limits_the_number_of_pairs():
    Q, _ = _designed_matrix(n=128)
    with pytest.raises(Exception, match="outside 1..32"):
        setup_gpu.device_diff_eigenpairs(FakeEigenEngine(Q), 0, 33, 1e-6, 1e-8)
    with pytest.raises(Exception, match="outside 1..32"):
        setup_gpu.device_diff_eigenpairs(FakeEigenEngine(Q), 0, 0, 1e-6, 1e-8)
    # the MG entry point refuses before it needs an engine
    p = gateway.set_params('schwinger16')
    A = matrix.loadMatrix(p['matrix'], p['matrix_params'])
    with pytest.raises(Exception, match="outside 1..32"):
        MG(A).device_diff_eigenpairs(0, 33, 1e-3)


def test_mlmc_defl_setup_key_is_passed_through_and_checked():
    params = gateway.set_params('schwinger16')
    params['function_tol'] = 1e-12
    tp = utils.trace_params_from_params(params, "mlmc")
    assert 'mlmc_defl_setup' not in tp
    assert utils.mlmc_defl_setup_of(tp) == "host"
    for how in ("host", "device"):
        params['mlmc_defl_setup'] = how
        tp = utils.trace_params_from_params(params, "mlmc")
        assert tp['mlmc_defl_setup'] == how
        assert utils.mlmc_defl_setup_of(tp) == how
    params['mlmc_defl_setup'] = "gpu"
    tp = utils.trace_params_from_params(params, "mlmc")
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    with pytest.raises(Exception, match="mlmc_defl_setup"):
        stoch_trace.mlmc(A, tp)


def test_refinement_below_tol_while_the_residual_still_falls():
    Q, _ = _designed_matrix()
    loose, refined = [], []
    setup_gpu.device_diff_eigenpairs(FakeEigenEngine(Q), 0, 8, 1e-1, 1e-11, log=loose)
    lam, X = setup_gpu.device_diff_eigenpairs(FakeEigenEngine(Q), 0, 8, 1e-1, 1e-11, log=refined, refine_to=1e-9)
    assert loose[-1]["residual_max"] <= 1e-1 and loose[-1]["residual_max"] > 1e-9
    assert refined[-1]["residual_max"] <= 1e-9 and len(refined) > len(loose)
    w = np.linalg.eigvalsh(Q)
    _check_pairs(Q, lam, X, w[np.argsort(-np.abs(w))[:8]], 1e-9)
