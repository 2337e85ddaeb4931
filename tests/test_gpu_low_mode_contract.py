"""GPU: the low-mode two-point functions contracted on the device (sw_low_mode_two_point: k_meson_field, the two batched
products Psi = G Phi G^H and the split-K contraction of k_cgemm_nt, k_lm_two_point_reduce) against the same three
products evaluated on the host from the device's own meson fields, bit-reproducibility, special values of G, the
refusals and the absence of side effects on the mode-11 buffers.  The lattice operator alone, no multigrid set-up."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import gateway, matrix, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import KCLASS_LM_CONTRACT, MODE_TWO_POINT_LMA, EngineError  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG, REF_HID, _new_engine  # noqa: E402


class Lattice:
    """The lattice operator alone on hierarchy 0 of an engine (the pattern of test_gpu_meson_fields.py)."""

    def __init__(self, A):
        self.mg = MG(A)
        lat = self.mg._lattice()
        self.L = int(lat[0])
        self.n = 2 * self.L * self.L
        self.eng = _new_engine(0)
        self.eng.hier_begin(REF_HID, 1)
        self.eng.set_lattice(REF_HID, lat[0], lat[1], lat[2], lat[3])
        self.eng.hier_end(REF_HID)


def _schwinger(name):
    params = gateway.set_params(name)
    return Lattice(matrix.loadMatrix(params['matrix'], params['matrix_params']))


@pytest.fixture(scope="module")
def p16():
    p = _schwinger('schwinger16')
    yield p
    p.eng.close()


@pytest.fixture(scope="module")
def p32():
    p = Lattice(matrix.synthetic_matrix(32, 0.05, sigma=0.3, seed=132))
    yield p
    p.eng.close()


@pytest.fixture(scope="module")
def p128():
    p = _schwinger('schwinger128')
    yield p
    p.eng.close()


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _contract(Phi, G):
    """The three products in the precision of Phi: Psi = G Phi G^H, E[(c,d,t)][(a,b,t0)] = Phi . conj(Psi), then
    g_a g_b and the layout [a][b][c][d][t][t0]."""
    L, k = Phi.shape[2], Phi.shape[3]
    G = G.astype(Phi.dtype)
    Psi = np.matmul(np.matmul(G, Phi), G.conj().T)
    E = Phi.reshape(4 * L, k * k) @ Psi.reshape(4 * L, k * k).conj().T
    g = np.array([1.0, -1.0])
    E = E.reshape(2, 2, L, 2, 2, L).transpose(3, 4, 0, 1, 2, 5)
    return E * (g[:, None] * g[None, :])[:, :, None, None, None, None]


def _bound(Phi, G):
    """(k^2 + 2 k + 16) 2^-52 sum_{m,m'} |Phi[c,d,t]|_{mm'} (|G| |Phi[a,b,t0]| |G|^T)_{mm'} as [a][b][c][d][t][t0]: a
    chain of 2 k^2 fused multiply-adds per component in any fixed order (k^2), the two 2 k-term chains inside Psi
    (2 k), and 16 for the sign and the additions of the K splits."""
    L, k = Phi.shape[2], Phi.shape[3]
    Pa, Ga = np.abs(Phi), np.abs(G)
    W = Pa.reshape(4 * L, k * k) @ np.matmul(np.matmul(Ga, Pa), Ga.T).reshape(4 * L, k * k).T
    return (k * k + 2 * k + 16) * 2.0 ** -52 * W.reshape(2, 2, L, 2, 2, L).transpose(3, 4, 0, 1, 2, 5)


def _register(p, k, seed):
    V = _rand((p.n, k), seed)
    G = _rand((k, k), seed + 1)                 # non-Hermitian: no symmetry for an error to hide behind
    p.eng.set_deflation(V)
    p.eng.set_low_mode_inverse(G)
    return V, G


def _check_parity(p, k, mom, seed):
    """E = eng.low_mode_two_point(p) against the long-double evaluation from the device's own Phi: every entry
    within _bound."""
    _, G = _register(p, k, seed)
    Phi = p.eng.meson_fields(mom, k)
    E = p.eng.low_mode_two_point(mom)
    assert E.shape == (2, 2, 2, 2, p.L, p.L) and E.dtype == np.complex128
    ref = _contract(Phi.astype(np.clongdouble), G)
    ratio = np.abs(E - ref).astype(np.float64) / _bound(Phi, G)
    print("low-mode contraction n=%d k=%d p=%d: worst |err| / bound = %.4f" % (p.n, k, mom, ratio.max()))
    assert np.max(np.abs(E)) > 0
    assert ratio.max() <= 1.0, "%.3f of the bound" % ratio.max()


@pytest.mark.parametrize("mom", [0, 1, 15])
@pytest.mark.parametrize("k", [5, 20, 70])
def test_parity_16(p16, k, mom):
    """Tails in every dimension: K = 25 / 400 / 4900, 4 L = 64 rows, rank below / above one 64-row block."""
    _check_parity(p16, k, mom, 800 + k)


@pytest.mark.parametrize("mom", [0, 3])
def test_parity_32_several_row_blocks(p32, mom):
    _check_parity(p32, 20, mom, 832)


def test_two_calls_agree_bit_for_bit(p16):
    _register(p16, 20, 840)
    E = p16.eng.low_mode_two_point(1)
    assert np.array_equal(p16.eng.low_mode_two_point(1), E)
    assert not np.array_equal(p16.eng.low_mode_two_point(15), E)


@pytest.mark.parametrize("k", [16, 40])
def test_parity_128_many_row_blocks_and_splits(p128, k):
    """4 L = 512: 8 x 8 workgroup tiles and 16 K splits.  Against the complex128 host contraction of the device's own
    Phi with twice the bound, since both sides round; the launches and the flops of the new kernel class."""
    p = p128
    _, G = _register(p, k, 850 + k)
    Phi = p.eng.meson_fields(1, k)
    p.eng.set_profiling(True)
    p.eng.timers_reset()
    try:
        E = p.eng.low_mode_two_point(1)
        ms, launches = p.eng.kernel_stats(KCLASS_LM_CONTRACT)
        work = p.eng.kernel_work(KCLASS_LM_CONTRACT)
        dots = p.eng.timers()['dots']
    finally:
        p.eng.set_profiling(False)
    ld = (k + 15) // 16 * 16
    assert launches == 4 and ms > 0 and dots >= ms
    assert work == 8.0 * (2.0 * 512 * ld ** 3 + 512.0 ** 2 * k * k)
    ref = utils.low_mode_two_point(Phi[None], G)[0]
    ratio = np.abs(E - ref) / (2.0 * _bound(Phi, G))
    print("low-mode contraction n=%d k=%d p=1 against complex128: worst |err| / (2 bound) = %.4f"
          % (p.n, k, ratio.max()))
    assert ratio.max() <= 1.0
    assert np.array_equal(p.eng.low_mode_two_point(1), E)


def test_zero_inverse_gives_exact_zeros(p16):
    p16.eng.set_deflation(_rand((p16.n, 20), 860))
    p16.eng.set_low_mode_inverse(np.zeros((20, 20)))
    E = p16.eng.low_mode_two_point(1)
    assert E.shape == (2, 2, 2, 2, 16, 16) and np.all(E == 0)


def test_diagonal_inverse_summed_over_the_sink_timeslice(p16):
    """G = diag(1 / lambda) with orthonormal V: sum_t E[a][a][c][c][t][t0] against the device Phi contracted with the
    diagonal G on the host, Psi[m][m'] = Phi[m][m'] / (lambda_m lambda_m')."""
    p, k, mom = p16, 20, 1
    V, _ = np.linalg.qr(_rand((p.n, k), 870))
    lam = np.random.default_rng(871).uniform(0.2, 2.0, k) * np.where(np.arange(k) % 2, -1.0, 1.0)
    p.eng.set_deflation(np.ascontiguousarray(V))
    p.eng.set_low_mode_inverse(np.diag(1.0 / lam))
    Phi = p.eng.meson_fields(mom, k)
    E = p.eng.low_mode_two_point(mom)
    Psi = Phi / (lam[:, None] * lam[None, :])
    worst = 0.0
    for a in range(2):
        for c in range(2):
            host = np.einsum('tmn,smn->s', Phi[c, c], Psi[a, a].conj())          # [t0], summed over t
            worst = max(worst, np.max(np.abs(E[a, a, c, c].sum(axis=0) - host)))
    print("diagonal G: max |sum_t E - host| / max |E| = %.2e" % (worst / np.max(np.abs(E))))
    assert worst <= 1e-12 * np.max(np.abs(E))


def test_refusals_launch_nothing(p16):
    p, eng = p16, p16.eng
    V = _rand((p.n, 5), 880)
    eng.set_deflation(None)
    launches = eng.launch_count()
    try:
        with pytest.raises(EngineError, match="no deflation vectors"):
            eng.low_mode_two_point(0)
        assert eng.launch_count() == launches
        eng.set_deflation(V)
        with pytest.raises(EngineError, match="no low-mode inverse"):
            eng.low_mode_two_point(0)
        assert eng.launch_count() == launches
        eng.set_low_mode_inverse(np.eye(5))
        eng.set_deflation(V)                                                # a new registration drops G
        with pytest.raises(EngineError, match="no low-mode inverse"):
            eng.low_mode_two_point(0)
        assert eng.launch_count() == launches
        eng.set_low_mode_inverse(np.eye(5))
        for mom in (p.L, -1):
            with pytest.raises(EngineError, match="outside"):
                eng.low_mode_two_point(mom)
            assert eng.launch_count() == launches
    finally:
        eng.set_deflation(None)


def test_no_side_effects_on_a_mode_11_batch(p16):
    p, eng = p16, p16.eng
    _register(p, 5, 890)
    eng.set_low_mode_inverse(1e-3 * _rand((5, 5), 891))
    eng.set_solver(16, REF_HID)
    eng.set_two_point(3, [0, 1])
    try:
        np.random.seed(892)
        codes = utils.draw_probes(3, p.n)
        R, _, _ = eng.hutch_batch_resolved(MODE_TWO_POINT_LMA, 0, codes, 1e-10, 1000)
        assert np.max(np.abs(R)) > 0
        E = eng.low_mode_two_point(1)
        assert np.max(np.abs(E)) > 0
        assert np.array_equal(eng.hutch_fetch_two_point_lma(), R)
        assert np.array_equal(eng.low_mode_two_point(1), E)
    finally:
        eng.set_two_point(0, None)
        eng.set_deflation(None)
