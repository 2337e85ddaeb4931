"""GPU: the device meson fields (sw_meson_fields, k_meson_field), the low-mode chain alone (sw_apply_low_mode:
projection dots, k_low_mode_coef, the apply kernel without its subtraction) and the refusals of the low-mode ABI."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import gateway, matrix, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import MODE_TWO_POINT_LMA, EngineError  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG, REF_HID, _new_engine  # noqa: E402

MOMENTA = [0, 1, 15]


class Lattice:
    """The lattice operator alone on hierarchy 0 of an engine: all the meson fields and the low-mode chain need."""

    def __init__(self, A):
        self.mg = MG(A)
        lat = self.mg._lattice()
        self.L = int(lat[0])
        self.n = 2 * self.L * self.L
        self.eng = _new_engine(0)
        self.eng.hier_begin(REF_HID, 1)
        self.eng.set_lattice(REF_HID, lat[0], lat[1], lat[2], lat[3])
        self.eng.hier_end(REF_HID)


@pytest.fixture(scope="module")
def p16():
    params = gateway.set_params('schwinger16')
    return Lattice(matrix.loadMatrix(params['matrix'], params['matrix_params']))


@pytest.fixture(scope="module")
def p32():
    return Lattice(matrix.synthetic_matrix(32, 0.05, sigma=0.3, seed=132))


def _vectors(n, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))


def _check_fields(p, k, momenta, seed):
    """Every entry within (L + 8) 2^-52 sum_x |V_m| |V_m'| of the extended-precision value.  The kernel sums an entry's
    real and imaginary parts as chains of 2 ceil(L / 4) * 4 fused multiply-adds in the fixed order x = 0, 1, ... (the
    matrix core's K = 4 block in sequence, the padded rows exact zeros), two products per x -- the same 2 L-term
    chain per component as the pair dots of DESIGN 4d, one rounding per term instead of two -- and the phased
    operand carries one table entry and one complex multiply, inside the + 8.  Two calls are bit-identical."""
    L = p.L
    V = _vectors(p.n, k, seed)
    p.eng.set_deflation(V)
    ref = utils.meson_fields(V.astype(np.clongdouble), L, momenta)
    Va = np.abs(V).reshape(2, L, L, k)
    W = np.einsum('ctxm,dtxn->cdtmn', Va, Va)
    worst = 0.0
    for j, mom in enumerate(momenta):
        out = p.eng.meson_fields(mom, k)
        assert out.shape == (2, 2, L, k, k)
        ratio = np.abs(out - ref[j]).astype(np.float64) / ((L + 8) * 2.0 ** -52 * W)
        worst = max(worst, ratio.max())
        assert ratio.max() <= 1.0, "p = %d: %.3f of the bound" % (mom, ratio.max())
        assert np.max(np.abs(out)) > 0
        assert np.array_equal(p.eng.meson_fields(mom, k), out)
        assert np.max(np.abs(out - utils.meson_fields(V, L, [mom])[0])) < 1e-12 * np.max(W)
    print("meson fields n=%d k=%d momenta=%s: worst |err| / bound = %.3f" % (p.n, k, momenta, worst))


@pytest.mark.parametrize("k", [5, 20, 70])
def test_meson_fields_16(p16, k):
    _check_fields(p16, k, MOMENTA, 500 + k)


def test_meson_fields_32_several_k_loop_trips(p32):
    _check_fields(p32, 20, [0, 3], 532)


@pytest.mark.parametrize("nb", [3, 70])
@pytest.mark.parametrize("k", [5, 70])
def test_apply_low_mode_16(p16, k, nb):
    """Y = V G V^H X against the long-double evaluation, per column below 1e-13 (k + 8) of the column's norm."""
    p = p16
    V = _vectors(p.n, k, 600 + k) / np.sqrt(p.n)
    G = _vectors(k, k, 601 + k)
    X = _vectors(p.n, nb, 602 + nb).T.copy()
    p.eng.set_deflation(V)
    p.eng.set_low_mode_inverse(G)
    Y = p.eng.apply_low_mode(X)
    assert Y.shape == X.shape
    Vl, Gl, Xl = V.astype(np.clongdouble), G.astype(np.clongdouble), X.astype(np.clongdouble)
    ref = ((Xl @ Vl.conj()) @ Gl.T) @ Vl.T
    rel = (np.linalg.norm((Y - ref).astype(np.complex128), axis=1)
           / np.linalg.norm(ref.astype(np.complex128), axis=1))
    print("apply_low_mode k=%d nb=%d: worst relative error per column %.2e (bar %.2e)"
          % (k, nb, rel.max(), 1e-13 * (k + 8)))
    assert rel.max() < 1e-13 * (k + 8)
    assert np.array_equal(p.eng.apply_low_mode(X), Y)
    one = p.eng.apply_low_mode(X[0])
    assert one.shape == (p.n,) and np.array_equal(one, Y[0])


def test_refusals(p16):
    p = p16
    eng = p.eng
    V = _vectors(p.n, 5, 700)
    np.random.seed(7)
    probes = utils.draw_probes(2, p.n)
    eng.set_deflation(None)
    eng.set_two_point(0, None)
    launches = eng.launch_count()
    try:
        with pytest.raises(EngineError, match="no deflation vectors"):
            eng.meson_fields(0, 5)
        with pytest.raises(EngineError, match="no deflation vectors"):
            eng.set_low_mode_inverse(np.eye(5))
        with pytest.raises(EngineError, match="no deflation vectors"):
            eng.apply_low_mode(np.ones(p.n))
        eng.set_low_mode_inverse(None)                                      # clearing is always allowed
        eng.set_deflation(V)
        with pytest.raises(EngineError, match="outside"):
            eng.meson_fields(p.L, 5)
        with pytest.raises(EngineError, match="outside"):
            eng.meson_fields(-1, 5)
        with pytest.raises(EngineError, match="rank 4"):
            eng.set_low_mode_inverse(np.eye(4))
        with pytest.raises(EngineError, match="no low-mode inverse"):
            eng.apply_low_mode(np.ones(p.n))
        eng.set_low_mode_inverse(np.eye(5))
        eng.set_deflation(V)                                                # a new registration drops G
        with pytest.raises(EngineError, match="no low-mode inverse"):
            eng.apply_low_mode(np.ones(p.n))
        eng.set_low_mode_inverse(np.eye(5))
        with pytest.raises(EngineError, match="no two-point registration"):
            eng.hutch_batch(MODE_TWO_POINT_LMA, 0, probes, 1e-12, 100)
        eng.set_two_point(3, [0, 1])
        with pytest.raises(EngineError, match="no low-mode averaged two-point batch"):
            eng.hutch_fetch_two_point_lma()
        eng.set_low_mode_inverse(None)
        with pytest.raises(EngineError, match="no low-mode inverse"):
            eng.hutch_batch(MODE_TWO_POINT_LMA, 0, probes, 1e-12, 100)
        eng.set_deflation(None)
        with pytest.raises(EngineError, match="no deflation vectors"):
            eng.hutch_batch(MODE_TWO_POINT_LMA, 0, probes, 1e-12, 100)
        assert eng.launch_count() == launches                              # nothing was launched
    finally:
        eng.set_two_point(0, None)
        eng.set_deflation(None)
