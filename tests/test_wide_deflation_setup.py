"""CPU: the block eigensolver on blocks wider than 64 vectors (setup_gpu.block_eigenpairs with `width`)
driven through a NumPy stand-in of the engine's eigen buffers, the plumbing of the build-only key
defl_setup (which route computes the Hutchinson deflation pairs), and the register use of the new kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from deflatedmlmc_schwinger_amd import gateway, matrix, setup_gpu, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class WideFakeEngine:
    """The sw_eig_* calls on a dense matrix Q with blocks of `width` columns (sw_eig_begin_wide):
    eig_solve = Q^-1 (shift-invert), eig_apply_diff = Q."""

    def __init__(self, Q, seed=5):
        self.Q = Q
        self.Qinv = np.linalg.inv(Q)
        self.n = Q.shape[0]
        self.rng = np.random.default_rng(seed)
        self.buf = None
        self.width = None

    def eig_begin(self, hid, level, seed=11, width=64):
        self.width = width
        shape = (self.n, width)
        self.buf = [np.zeros(shape, dtype=np.complex128) for _ in range(3)]
        self.buf[0] = self.rng.standard_normal(shape) + 1j * self.rng.standard_normal(shape)

    def eig_load(self, dst, X):
        X = np.atleast_2d(X)
        self.buf[dst][:, :X.shape[0]] = X.T

    def eig_apply_diff(self, src, dst, skip, g3, tol, maxiter=1000):
        self.buf[dst] = self.Q @ self.buf[src]
        return 3

    def eig_solve(self, src, dst, mode, tol, maxiter=1000):
        self.buf[dst] = self.Qinv @ self.buf[src]
        return 4

    def eig_gram(self, a, b):
        return self.buf[a].conj().T @ self.buf[b]

    def eig_rotate(self, src, Y, dst, sub=-1):
        assert src != dst and Y.shape == (self.width, self.width)
        out = self.buf[src] @ Y
        self.buf[dst] = out if sub < 0 else self.buf[sub] - out

    def eig_fetch(self, src, k):
        assert k <= self.width
        return self.buf[src][:, :k].T.copy()

    def eig_end(self):
        self.buf = None


def _matrix(n, hermitian, seed):
    """Eigenvalues spread over two decades (no two closer than a few percent at the ends of the spectrum,
    so both modes converge fast on a 2k-wide block)."""
    rng = np.random.default_rng(seed)
    lam = np.geomspace(0.05, 50.0, n) * rng.choice([-1.0, 1.0], n)
    if hermitian:
        U, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        Q = (U * lam[None, :]) @ U.conj().T
        return 0.5 * (Q + Q.conj().T)
    S = np.eye(n) + 0.1 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(n)
    return (S * lam[None, :]) @ np.linalg.inv(S)


def _pick(w, k, nearest_zero):
    return w[np.argsort(np.abs(w) if nearest_zero else -np.abs(w))[:k]]


def _same(got, want):
    key = lambda z: (round(abs(z), 8), z.imag)  # noqa: E731
    got = np.array(sorted(np.asarray(got, dtype=complex), key=key))
    want = np.array(sorted(np.asarray(want, dtype=complex), key=key))
    return np.max(np.abs(got - want) / np.abs(want))


@pytest.mark.parametrize("k,width", [(48, 128), (100, 256)])
def test_shift_invert_pairs_on_wide_blocks(k, width):
    assert setup_gpu.eig_width_for(k) == width
    for hermitian in (True, False):
        Q = _matrix(600, hermitian, seed=k)
        want = _pick(np.linalg.eig(Q)[0], k, True)
        eng = WideFakeEngine(Q)
        lam, X = setup_gpu.device_eigenpairs(eng, 1, 0, k, 1e-11, hermitian_g3=hermitian, width=width)
        assert eng.width == width and X.shape == (600, k)
        assert _same(lam, want) < 1e-10, hermitian
        res = np.linalg.norm(Q @ X - X * lam[None, :], axis=0) / np.abs(lam)
        assert res.max() < 1e-8


@pytest.mark.parametrize("k,width", [(48, 128), (100, 256)])
def test_largest_magnitude_pairs_on_wide_blocks(k, width):
    Q = _matrix(600, True, seed=7 + k)
    want = _pick(np.linalg.eig(Q)[0], k, False)
    eng = WideFakeEngine(Q)
    lam, X = setup_gpu.device_diff_eigenpairs(eng, 0, k, 1e-11, 1e-12, width=width)
    assert eng.width == width
    assert _same(lam, want) < 1e-10
    assert np.abs(X.conj().T @ X - np.eye(k)).max() < 1e-12


def test_width_checks():
    Q = _matrix(300, True, seed=1)
    with pytest.raises(Exception, match="outside 1..64"):
        setup_gpu.device_eigenpairs(WideFakeEngine(Q), 1, 0, 65, 1e-6, width=128)
    with pytest.raises(Exception, match="multiple of 64"):
        setup_gpu.device_eigenpairs(WideFakeEngine(Q), 1, 0, 8, 1e-6, width=96)
    with pytest.raises(Exception, match="multiple of 64"):
        setup_gpu.device_diff_eigenpairs(WideFakeEngine(Q), 0, 8, 1e-6, 1e-8, width=576)
    assert [setup_gpu.eig_width_for(k) for k in (1, 32, 33, 64, 65, 128, 200, 256)] == \
        [64, 64, 128, 128, 192, 256, 448, 512]


# ---- defl_setup ---------------------------------------------------------------------------------
class _Level:
    def __init__(self, n):
        import scipy.sparse as sp
        sign = np.ones(n)
        sign[n // 2:] = -1.0
        self.g3 = sp.diags([sign], [0])


class _ML:
    def __init__(self, n):
        self.levels = [_Level(n)]


class StubMG:
    """What deflation_pre_computations reads of an MG, recording which eigensolver route ran."""

    def __init__(self, n, solver_hier=True):
        self.ml = _ML(n)
        self._have_solver_hier = solver_hier
        self._solver_cfg_built = {"setup": "device"}
        self.engine = None
        self.engines = []
        self.calls = []
        self.n = n

    def device_eigenpairs(self, k, tol, hermitian=False, log=None, width=None):
        self.calls.append(("device", k, width))
        rng = np.random.default_rng(k)
        X, _ = np.linalg.qr(rng.standard_normal((self.n, k)) + 0j)
        return np.linspace(0.1, 1.0, k), X


@pytest.fixture
def small():
    params = gateway.set_params('schwinger16')
    params['function_tol'] = 1e-12
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    return params, A


def _route(monkeypatch, params, A, k, how, solver_hier=True):
    host = []

    def fake_eigsh(Q, k=6, **kw):
        host.append(k)
        X, _ = np.linalg.qr(np.random.default_rng(k).standard_normal((Q.shape[0], k)) + 0j)
        return np.linspace(0.1, 1.0, k), X

    monkeypatch.setattr(utils, "eigsh", fake_eigsh)
    p = dict(params)
    if how is not None:
        p['defl_setup'] = how
    tp = utils.trace_params_from_params(p, "hutchinson")
    tp['use_permuted'] = False
    mg = StubMG(A.shape[0], solver_hier)
    utils.deflation_pre_computations(A, k, 1e-9, "hutchinson", utils.CustomTimer(), tp, mg)
    return ["device"] * len(mg.calls) + ["host"] * len(host), mg.calls


def test_defl_setup_key_is_passed_through_and_checked(small):
    params, A = small
    tp = utils.trace_params_from_params(params, "hutchinson")
    assert 'defl_setup' not in tp and utils.defl_setup_of(tp) == "auto"
    for how in ("auto", "device", "host"):
        tp = utils.trace_params_from_params(dict(params, defl_setup=how), "hutchinson")
        assert tp['defl_setup'] == how and utils.defl_setup_of(tp) == how
        assert utils.trace_params_from_params(dict(params, defl_setup=how), "mlmc")['defl_setup'] == how
    tp = utils.trace_params_from_params(dict(params, defl_setup="gpu"), "hutchinson")
    with pytest.raises(Exception, match="defl_setup"):
        utils.defl_setup_of(tp)
    with pytest.raises(Exception, match="defl_setup"):
        utils.deflation_pre_computations(A, 8, 1e-9, "hutchinson", utils.CustomTimer(), tp, StubMG(A.shape[0]))


def test_defl_setup_routes(monkeypatch, small):
    params, A = small
    # "auto" (and no key): today's rule -- the device solver up to 32 pairs with a device-built solver hierarchy
    for how in (None, "auto"):
        assert _route(monkeypatch, params, A, 8, how)[0] == ["device"]
        assert _route(monkeypatch, params, A, 48, how)[0] == ["host"]
        assert _route(monkeypatch, params, A, 100, how)[0] == ["host"]
        assert _route(monkeypatch, params, A, 8, how, solver_hier=False)[0] == ["host"]
    # "device": the block eigensolver on a block of 64 ceil(2 k / 64)
    for k, width in ((8, 64), (48, 128), (100, 256)):
        route, calls = _route(monkeypatch, params, A, k, "device")
        assert route == ["device"] and calls == [("device", k, width)]
    with pytest.raises(Exception, match="solver hierarchy"):
        _route(monkeypatch, params, A, 8, "device", solver_hier=False)
    with pytest.raises(Exception, match="outside 1..256"):
        _route(monkeypatch, params, A, 257, "device")
    # "host": ARPACK always
    for k in (8, 48, 100):
        assert _route(monkeypatch, params, A, k, "host")[0] == ["host"]


# ---- register use of the new kernels -----------------------------------------------------------
NEW_KERNELS = ("k_defl_gemm_dots", "k_defl_gemm_apply", "k_block_gram_wide", "k_block_rotate_wide")


def test_new_kernels_do_not_spill():
    """Compile-only: every accumulator of the MFMA deflation and wide eigen kernels stays in registers."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "deflatedmlmc_schwinger_amd", "csrc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          "-o", os.devnull, "sw_engine.hip", "-Rpass-analysis=kernel-resource-usage"],
                         cwd=csrc, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    scratch = {}
    name = None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    for kern in NEW_KERNELS:
        found = {k: v for k, v in scratch.items() if kern in k}
        assert found, kern
        assert all(v == 0 for v in found.values()), found
