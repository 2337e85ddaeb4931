"""GPU: low-mode averaged two-point functions (SW_MODE_TWO_POINT_LMA, lma_two_point()) -- per-noise parity of the
stochastic remainder against sparse LU and the host low-mode solutions, the G = 0 batch against mode 6 bit for bit,
switching between the modes 6, 11 and 5, and the flow against the exact expectation of schwinger128."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import gateway, matrix, stoch_trace, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import MODE_TWO_POINT, MODE_TWO_POINT_LMA  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG  # noqa: E402
from oracle import ref_path as rp  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


class Problem:
    """One lattice with its hierarchy on the GPU, its sparse LU, and k low modes of gamma_3 A with their low-mode
    inverse registered: 16^2 from the dense eigendecomposition, 128^2 from the device eigensolver."""

    def __init__(self, name, k):
        params = gateway.set_params(name)
        params['function_tol'] = 1e-12
        self.A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
        self.tp = utils.trace_params_from_params(params, "hutchinson")
        from deflatedmlmc_schwinger_amd import hierarchy as _h
        self.tp['solver_cfg'] = dict(_h.DEFAULT_SOLVER_CFG)
        self.mg = MG(self.A)
        self.mg.setup(dof=self.tp['dof'], aggrs=self.tp['aggrs'], max_levels=self.tp['max_nr_levels'], dim=2,
                      acc_eigvs=self.tp['accuracy_mg_eigvs'], sys_type='schwinger', params=self.tp)
        self.mg.total_levels = len(self.mg.ml.levels)
        self.L = int(self.tp['latt_dims'][0])
        self.n = self.A.shape[0]
        self.eng = self.mg.engine
        self.lu = rp.LUSolver(self.A)
        g3 = np.where(np.arange(self.n) < self.n // 2, 1.0, -1.0)
        if self.n <= 512:
            lam, W = np.linalg.eigh(g3[:, None] * self.A.toarray())
            self.V = np.ascontiguousarray(W[:, np.argsort(np.abs(lam))[:k]])
        else:
            _, V = self.mg.device_eigenpairs(k, 1e-9, hermitian=True)
            self.V = np.ascontiguousarray(np.asarray(V, dtype=np.complex128))
        self.G = utils.low_mode_inverse(self.V, g3[:, None] * np.asarray(self.A @ self.V))
        self.register(self.G)

    def register(self, G):
        self.eng.set_deflation(self.V)
        self.eng.set_low_mode_inverse(G)

    def solutions(self, codes, t0, momenta):
        src = utils.slice_sources(codes, self.L, t0, momenta)
        G, nb, n = src.shape
        return src, np.asarray(self.lu(src.reshape(G * nb, n).T)).T.reshape(G, nb, n)


@pytest.fixture(scope="module")
def p16():
    return Problem('schwinger16', 5)


@pytest.fixture(scope="module")
def p128():
    return Problem('schwinger128', 16)


def _weights(Z, L, momenta):
    M = len(momenta)
    Za = np.abs(Z).reshape(M, 2, Z.shape[1], 2, L, L)
    return np.einsum('akctx,jbkdtx->kjabcdt', Za[list(momenta).index(0)], Za)


def _tight(p, body):
    saved = p.eng.get_option("stop_factor")
    p.eng.set_option("stop_factor", 0.1)
    try:
        return body()
    finally:
        p.eng.set_option("stop_factor", saved)


def _lma_batch(p, codes):
    R, itf, _ = p.eng.hutch_batch_resolved(MODE_TWO_POINT_LMA, 0, codes, 1e-12, 1000)
    total, itf2, _ = p.eng.hutch_fetch()
    assert np.array_equal(itf, itf2)
    return R, total, itf


def _check_parity(p, codes, t0, momenta, what):
    """A mode-11 batch against pair_dots(z_LU) - pair_dots(z_L), z_LU the sparse-LU solutions of the same sources and
    z_L = utils.low_mode_solutions: 2e-10 of the batch's largest sum_x |z_c| |z_d| (DESIGN 4d's bar; the low-mode
    part carries no solver error).  The fetched total is the sum over the fetched R: the two sums of 4 L terms differ
    by at most 8 L 2^-53 of the terms' moduli."""
    p.register(p.G)
    p.eng.set_two_point(t0, momenta)
    R, total, itf = _tight(p, lambda: _lma_batch(p, codes))
    assert R.shape == (codes.shape[0], len(momenta), 2, 2, 2, 2, p.L) and itf.min() >= 1
    src, Z = p.solutions(codes, t0, momenta)
    ZL = utils.low_mode_solutions(p.V, p.G, src)
    ref = utils.pair_dots(Z, p.L, momenta) - utils.pair_dots(ZL, p.L, momenta)
    worst = np.max(np.abs(R - ref)) / np.max(_weights(Z, p.L, momenta))
    plain = np.max(np.abs(ref)) / np.max(np.abs(utils.pair_dots(Z, p.L, momenta)))
    print("%s n=%d t0=%d momenta=%s: max |R - ref| / max sum|z_c||z_d| = %.2e (max |R| / max |T| = %.3f)"
          % (what, p.n, t0, momenta, worst, plain))
    assert worst < 2e-10
    j0 = list(momenta).index(0)
    host = stoch_trace.two_point_columns(R, j0)[:, -1]
    terms = sum(np.sum(np.abs(R[:, j0, a, a, c, c, :]), axis=1) for a in range(2) for c in range(2))
    assert np.all(np.abs(host - total) <= 8 * p.L * 2.0 ** -53 * terms)
    return R


@pytest.mark.parametrize("kind", ["z2", "z4"])
def test_per_noise_parity_16(p16, kind):
    np.random.seed(51)
    _check_parity(p16, utils.draw_probes(3, p16.n, kind), 3, [0, 1, 15], "lma parity " + kind)


def test_per_noise_parity_128(p128):
    np.random.seed(52)
    _check_parity(p128, utils.draw_probes(8, p128.n, "z2"), 5, [0, 1], "lma parity")


def test_zero_low_mode_inverse_gives_mode_6_bit_for_bit(p16):
    """With G = 0 the low-mode solutions are exact zeros, their pair sums too, and T - 0 = T."""
    p = p16
    np.random.seed(53)
    codes = utils.draw_probes(6, p.n, "z4")
    p.eng.set_two_point(3, [1, 0, 15])
    try:
        p.register(np.zeros_like(p.G))
        R, total, itf = _lma_batch(p, codes)
        T, itf6, _ = p.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
        total6, _, _ = p.eng.hutch_fetch()
        assert np.array_equal(R, T) and np.array_equal(total, total6) and np.array_equal(itf, itf6)
        assert np.max(np.abs(T)) > 0
    finally:
        p.register(p.G)
        p.eng.set_two_point(0, None)


def test_mode_switching_keeps_every_fetch_right(p16):
    p = p16
    np.random.seed(54)
    codes = utils.draw_probes(4, p.n, "z2")
    other = utils.draw_probes(4, p.n, "z2")
    momenta = [0, 15]
    p.register(p.G)
    p.eng.set_two_point(3, momenta)
    p.eng.set_loop_momenta([0, 1])
    try:
        T6, _, _ = p.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
        R11 = _lma_batch(p, other)[0]
        assert np.array_equal(p.eng.hutch_fetch_two_point(), T6)           # mode 6's batch survived mode 11
        assert np.array_equal(p.eng.hutch_fetch_two_point_lma(), R11)
        assert not np.array_equal(R11, T6)
        T6b, _, _ = p.eng.hutch_batch_two_point(0, other, 1e-12, 1000)
        assert np.array_equal(p.eng.hutch_fetch_two_point_lma(), R11)      # mode 11's batch survived mode 6
        assert np.array_equal(p.eng.hutch_fetch_two_point(), T6b) and not np.array_equal(T6b, T6)
        l5, _, _ = p.eng.hutch_batch_loops(0, codes, 1e-12, 1000)          # deflated with the registered vectors
        assert np.array_equal(p.eng.hutch_fetch_two_point_lma(), R11)
        assert np.array_equal(p.eng.hutch_fetch_two_point(), T6b)
        assert np.array_equal(p.eng.hutch_fetch_loops(), l5)
        assert np.array_equal(_lma_batch(p, other)[0], R11)
        assert np.array_equal(p.eng.hutch_fetch_loops(), l5)
    finally:
        p.eng.set_loop_momenta(None)
        p.eng.set_two_point(0, None)


# ---- the flow ---------------------------------------------------------------------------------------------
def _golden():
    with open(os.path.join(HERE, "golden", "two_point128.json")) as f:
        g = json.load(f)
    return np.array([complex(re, im) for re, im in g["two_point128"]]).reshape(g["shape"])


KEYS = {'two_point', 'two_point_devs', 'two_point_ests', 'converged', 'momenta', 'source_timeslice', 'nr_ests',
        'function_iters', 'ests', 'probe_loop_s', 'probes_solved', 'two_point_low', 'two_point_rest',
        'two_point_rest_devs', 'nr_deflat_vctrs'}


def test_fixed_length_flow_128_against_the_exact_expectation(capsys):
    """2048 noises whatever their variance (tol 1e-9 is never met), 16 vectors: every one of the 2 x 16 x 128 entries
    of two_point within 5 dev / sqrt(N) of the exact expectation.  Prints the pion channel's per-timeslice sample
    variance of the remainder next to that of two_point()'s T over the same first 256 stream noises; no
    variance-reduction figure is asserted."""
    golden = _golden()
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params['source_timeslice'] = 5
    params['two_point_momenta'] = [0, 1]
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "hutchinson")
    tp['max_nr_ests'] = 2048
    tp['tol'] = 1e-9
    tp['nr_deflat_vctrs'] = 16
    res = stoch_trace.lma_two_point(A, tp)
    plain = stoch_trace.two_point(A, dict(tp, max_nr_ests=256))
    capsys.readouterr()
    nr = res['nr_ests'] + 1
    assert set(res) == KEYS
    assert nr == 2048 and res['probes_solved'] == 2048 and res['nr_deflat_vctrs'] == 16
    assert res['momenta'] == [0, 1] and res['source_timeslice'] == 5
    shape = (2, 2, 2, 2, 2, 128)
    assert res['two_point'].shape == res['two_point_devs'].shape == res['two_point_rest'].shape == shape
    assert res['two_point_low'].shape == shape + (128,)
    assert res['two_point_ests'].shape == (nr,) + shape and res['ests'].shape == (nr,)
    assert np.array_equal(res['two_point_low'][..., 5] + res['two_point_rest'], res['two_point'])
    diff = np.abs(res['two_point'] - golden)
    bound = 5.0 * res['two_point_devs'] / np.sqrt(nr)
    ratio = diff / bound
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("lma two-point: worst |diff| / bound = %.3f at [p][a][b][c][d][t] = %s (|diff| %.3e, bound %.3e); entries "
          "over 3/5 of the bound: %d of %d" % (ratio[at], at, diff[at], bound[at], int(np.sum(ratio > 0.6)),
                                               ratio.size))
    low = np.abs(res['two_point_low'][..., 5] - golden)
    print("low-mode part alone: max |E_L - E[T]| / max |E[T]| = %.3f" % (np.max(low) / np.max(np.abs(golden))))
    pr = utils.meson_correlator(res['two_point_ests'][:256], 'g3', 'g3')[:, 0].real
    pt = utils.meson_correlator(plain['two_point_ests'][:256], 'g3', 'g3')[:, 0].real
    print("pion channel, 256 noises, |t - t0| : var(R_k) : var(T_k) : ratio")
    for d in (0, 1, 2, 4, 8, 16, 32, 48, 64):
        vr, vt = np.var(pr[:, (5 + d) % 128]), np.var(pt[:, (5 + d) % 128])
        print("  %3d  %.4e  %.4e  %.4f" % (d, vr, vt, vr / vt))
    assert ratio.size == 4096 and np.all(diff < bound)
    for T in (res['two_point'], res['two_point_low'][..., 5]):
        pion = utils.meson_correlator(T, 'g3', 'g3')[0]
        assert np.all(pion.real > 0)
    assert np.max(np.abs(res['two_point_ests'].mean(axis=0) - res['two_point'])) < 1e-9
    assert res['function_iters'] >= nr
