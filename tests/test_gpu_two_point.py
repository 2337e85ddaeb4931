"""GPU: one-end-trick two-point functions (sw_set_two_point, SW_MODE_TWO_POINT, k_slice_sources, k_slice_pair_dots) --
the two kernels alone against their NumPy restatements, the ABI's refusals, per-noise parity against sparse LU, the
pion total against sw_solve, switching between the modes 4, 5 and 6, and the two_point() flow against the exact
expectation of schwinger128."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import gateway, matrix, stoch_trace, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import MODE_TWO_POINT, EngineError  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG, SOLVER_HID  # noqa: E402
from oracle import ref_path as rp  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
EIGHT16 = [1, 2, 0, 3, 5, 8, 13, 15]          # momentum 0 is not the first: j0 = 2


class Problem:
    """One lattice with its hierarchy on the GPU, no deflation vectors (the mode uses none), and its sparse LU."""

    def __init__(self, name):
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

    def solutions(self, codes, t0, momenta):
        src = utils.slice_sources(codes, self.L, t0, momenta)
        G, nb, n = src.shape
        return np.asarray(self.lu(src.reshape(G * nb, n).T)).T.reshape(G, nb, n)


@pytest.fixture(scope="module")
def p16():
    return Problem('schwinger16')


@pytest.fixture(scope="module")
def p128():
    return Problem('schwinger128')


def _weights(Z, L, momenta):
    """W[k][j][a][b][c][d][t] = sum_x |Z[2 j0 + a][k][idx(c,x,t)]| |Z[2 j + b][k][idx(d,x,t)]|."""
    M = len(momenta)
    Za = np.abs(Z).reshape(M, 2, Z.shape[1], 2, L, L)
    return np.einsum('akctx,jbkdtx->kjabcdt', Za[list(momenta).index(0)], Za)


# ---- the source kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("momenta", [[0], [0, 5, 15]], ids=["p0", "three"])
@pytest.mark.parametrize("t0", [0, 15])
@pytest.mark.parametrize("kind", ["z2", "z4"])
@pytest.mark.parametrize("nb", [1, 3, 70])
def test_source_kernel_16(p16, nb, kind, t0, momenta):
    """Equal to utils.slice_sources: exactly at p = 0 and wherever the phase lies on an axis, to 4 * 2^-53 (one
    table entry, one multiply; the entries have modulus 1) elsewhere; zero off the L source rows."""
    p = p16
    np.random.seed(300 + nb)
    codes = utils.draw_probes(nb, p.n, kind)
    p.eng.set_two_point(t0, momenta)
    out = p.eng.apply_slice_sources(codes)
    ref = utils.slice_sources(codes, p.L, t0, momenta)
    assert out.shape == ref.shape == (2 * len(momenta), nb, p.n)
    err = np.max(np.abs(out - ref))
    print("sources nb=%d %s t0=%d momenta=%s: max |diff| = %.2e" % (nb, kind, t0, momenta, err))
    assert err <= 4 * 2.0 ** -53
    assert np.array_equal(out == 0, ref == 0) and np.count_nonzero(out) == 2 * len(momenta) * nb * p.L
    y = np.arange(p.L)
    for j, mom in enumerate(momenta):
        axis = (4 * mom * y) % p.L == 0                   # every y at p = 0
        for a in range(2):
            rows = a * p.L * p.L + t0 * p.L + y[axis]
            assert np.array_equal(out[2 * j + a][:, rows], ref[2 * j + a][:, rows])
    assert np.array_equal(p.eng.apply_slice_sources(codes), out)


# ---- the pair-dot kernels ---------------------------------------------------------------------------------
def _check_pair_dots(p, nb, momenta, seed):
    """Each entry within (L + 8) 2^-52 sum_x |z_c| |z_d| of its value in extended precision: the worst-case
    rounding of an L-term fixed-order sum of phased products.  Two runs are bit-identical."""
    L = p.L
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((2 * len(momenta), nb, p.n)) + 1j * rng.standard_normal((2 * len(momenta), nb, p.n))
    p.eng.set_two_point(1, momenta)
    out = p.eng.apply_pair_dots(Z)
    assert out.shape == (nb, len(momenta), 2, 2, 2, 2, L)
    M = len(momenta)
    Zr = Z.astype(np.clongdouble).reshape(M, 2, nb, 2, L, L)
    x = np.arange(L)
    ang = -2 * np.pi * (np.outer(np.asarray(momenta), x) % L).astype(np.longdouble) / L
    ph = np.cos(ang) + 1j * np.sin(ang)
    ref = np.einsum('jx,akctx,jbkdtx->kjabcdt', ph, Zr[list(momenta).index(0)].conj(), Zr)
    ratio = np.abs(out - ref).astype(np.float64) / ((L + 8) * 2.0 ** -52 * _weights(Z, L, momenta))
    print("pair dots n=%d nb=%d momenta=%s: worst |err| / bound = %.3f" % (p.n, nb, momenta, ratio.max()))
    assert ratio.max() <= 1.0
    assert np.max(np.abs(out)) > 0
    assert np.array_equal(p.eng.apply_pair_dots(Z), out)


@pytest.mark.parametrize("momenta", [[0], [0, 9], EIGHT16], ids=["p0", "two", "eight"])
@pytest.mark.parametrize("nb", [1, 3, 70, 130])
def test_pair_dot_kernel_16(p16, nb, momenta):
    _check_pair_dots(p16, nb, momenta, 400 + nb)


def test_pair_dot_kernel_128_full_noise_group(p128):
    _check_pair_dots(p128, 64, [0, 1], 9)


# ---- the ABI ----------------------------------------------------------------------------------------------
def test_abi_refusals(p16):
    eng, L, n = p16.eng, p16.L, p16.n
    np.random.seed(3)
    probes = utils.draw_probes(2, n)
    eng.set_two_point(3, [0, 1])
    launches = eng.launch_count()
    try:
        with pytest.raises(EngineError, match="source timeslice"):
            eng.set_two_point(L, [0])
        with pytest.raises(EngineError, match="source timeslice"):
            eng.set_two_point(-1, [0])
        with pytest.raises(EngineError, match="contain 0"):
            eng.set_two_point(3, [1, 2])
        with pytest.raises(EngineError, match="outside"):
            eng.set_two_point(3, [0, L])
        with pytest.raises(EngineError, match="listed twice"):
            eng.set_two_point(3, [0, 3, 3])
        with pytest.raises(EngineError, match="at most 8"):
            eng.set_two_point(3, list(range(9)))
        eng.set_two_point(0, None)
        with pytest.raises(EngineError, match="no two-point registration"):
            eng.hutch_batch(MODE_TWO_POINT, 0, probes, 1e-12, 100)
        with pytest.raises(EngineError, match="no two-point registration"):
            eng.apply_slice_sources(probes)
        with pytest.raises(EngineError, match="no two-point batch"):
            eng.hutch_fetch_two_point()
        eng.set_two_point(3, [0, 1])
        with pytest.raises(EngineError, match="no two-point batch"):
            eng.hutch_fetch_two_point()
        n1 = p16.mg.ml.levels[1].A.shape[0]
        with pytest.raises(EngineError, match="level 0"):
            eng.hutch_batch(MODE_TWO_POINT, 1, np.ones((2, n1), dtype=np.int8), 1e-12, 100)
        assert eng.launch_count() == launches                              # nothing was launched
    finally:
        eng.set_two_point(0, None)


def _tight(p, body):
    saved = p.eng.get_option("stop_factor")
    p.eng.set_option("stop_factor", 0.1)
    try:
        return body()
    finally:
        p.eng.set_option("stop_factor", saved)


def _check_parity(p, codes, t0, momenta, what):
    """A mode-6 batch against pair_dots of sparse-LU solutions of the same sources.  T is bilinear in two solutions
    that the solver holds to 1e-10 each: the bar is 2e-10 of the batch's largest sum_x |z_c| |z_d|."""
    p.eng.set_two_point(t0, momenta)
    T, itf, _ = _tight(p, lambda: p.eng.hutch_batch_two_point(0, codes, 1e-12, 1000))
    assert T.shape == (codes.shape[0], len(momenta), 2, 2, 2, 2, p.L) and itf.min() >= 1
    Z = p.solutions(codes, t0, momenta)
    ref = utils.pair_dots(Z, p.L, momenta)
    worst = np.max(np.abs(T - ref)) / np.max(_weights(Z, p.L, momenta))
    print("%s n=%d t0=%d momenta=%s: max |T - ref| / max sum|z_c||z_d| = %.2e" % (what, p.n, t0, momenta, worst))
    assert worst < 2e-10
    return T, Z


@pytest.mark.parametrize("kind", ["z2", "z4"])
def test_per_noise_parity_16(p16, kind):
    np.random.seed(21)
    _check_parity(p16, utils.draw_probes(6, p16.n, kind), 3, [1, 0, 15], "parity " + kind)


def test_per_noise_parity_128(p128):
    np.random.seed(22)
    _check_parity(p128, utils.draw_probes(8, p128.n, "z2"), 5, [0, 1], "parity")


@pytest.mark.parametrize("kind", ["z2", "z4"])
def test_total_is_the_squared_norm_of_the_momentum_zero_solutions_16(p16, kind):
    """sw_hutch_fetch after a mode-6 batch = sum_a ||z^(0,a)||^2 with z from sw_solve on the same sources."""
    p = p16
    np.random.seed(31)
    codes = utils.draw_probes(6, p.n, kind)
    t0, momenta = 7, [2, 0]
    p.eng.set_two_point(t0, momenta)

    def both():
        T, _, _ = p.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
        total, itf, itc = p.eng.hutch_fetch()
        src = p.eng.apply_slice_sources(codes)
        Z, _, _ = p.eng.solve(SOLVER_HID, 0, src[2:4].reshape(-1, p.n), 1e-12, 1000)
        return T, total, itf, Z.reshape(2, -1, p.n)

    T, total, itf, Z = _tight(p, both)
    norm = np.sum(np.abs(Z) ** 2, axis=(0, 2))
    rel = np.max(np.abs(total - norm) / norm)
    host = stoch_trace.two_point_columns(T, 1)[:, -1]
    print("pion total %s: |fetch - sum ||z||^2| / . = %.2e, host sum of T %.2e" % (kind, rel,
                                                                                  np.max(np.abs(host - total) / norm)))
    assert rel < 1e-10
    assert np.max(np.abs(host - total) / norm) < 1e-13
    assert np.max(np.abs(total.imag) / norm) < 1e-13 and itf.min() >= 1


def test_mode_switching_keeps_every_fetch_right(p16):
    p = p16
    np.random.seed(41)
    codes = utils.draw_probes(6, p.n, "z4")
    X = utils.probes_as_complex(codes)
    sols = np.asarray(p.lu(X.T)).T
    shifts, momenta = [0, 2 * p.L], [0, 1, 15]
    p.eng.set_shifts(shifts)
    p.eng.set_loop_momenta(momenta)
    p.eng.set_deflation(None)
    ref4 = np.array([[np.vdot(np.roll(X[k], -s), sols[k]) for s in shifts] for k in range(6)])
    ref5 = np.einsum('px,katx,kbtx->kpabt', utils.slice_phases(p.L, momenta), X.reshape(6, 2, p.L, p.L).conj(),
                     sols.reshape(6, 2, p.L, p.L))

    def run4():
        e, _, _ = _tight(p, lambda: p.eng.hutch_batch_shifts(0, codes, 1e-12, 1000))
        assert np.max(np.abs(e - ref4)) < 1e-10 * np.max(np.abs(ref4))
        return e

    def run5():
        l, _, _ = _tight(p, lambda: p.eng.hutch_batch_loops(0, codes, 1e-12, 1000))
        assert np.max(np.abs(l - ref5)) < 1e-10 * np.max(np.abs(ref5))
        return l

    try:
        e4 = run4()
        T6, _ = _check_parity(p, codes, 3, [0, 15], "mode 6 after 4")
        assert np.array_equal(p.eng.hutch_fetch_shifts(), e4)              # mode 4's batch survived mode 6
        l5 = run5()
        assert np.array_equal(p.eng.hutch_fetch_two_point(), T6)           # mode 6's batch survived mode 5
        assert np.array_equal(p.eng.hutch_fetch_shifts(), e4)
        T6b, _ = _check_parity(p, codes, 3, [0, 15], "mode 6 after 5")
        assert np.array_equal(T6b, T6)
        assert np.array_equal(p.eng.hutch_fetch_loops(), l5)               # mode 5's batch survived mode 6
        assert np.array_equal(run4(), e4) and np.array_equal(run5(), l5)
        assert np.array_equal(p.eng.hutch_fetch_two_point(), T6)
    finally:
        p.eng.set_shifts(None)
        p.eng.set_loop_momenta(None)
        p.eng.set_two_point(0, None)


# ---- the flow ---------------------------------------------------------------------------------------------
def _golden():
    with open(os.path.join(HERE, "golden", "two_point128.json")) as f:
        g = json.load(f)
    return np.array([complex(re, im) for re, im in g["two_point128"]]).reshape(g["shape"])


KEYS = {'two_point', 'two_point_devs', 'two_point_ests', 'converged', 'momenta', 'source_timeslice', 'nr_ests',
        'function_iters', 'ests', 'probe_loop_s', 'probes_solved'}


def test_fixed_length_flow_128_against_the_exact_expectation(capsys):
    """2048 noises whatever their variance (tol 1e-9 is never met): every one of the 2 x 16 x 128 entries within
    5 dev / sqrt(N) of the exact expectation.  The same 2048 stream noises through the sparse-LU oracle on the CPU
    lie within 0.547 of that bound."""
    golden = _golden()
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params['source_timeslice'] = 5
    params['two_point_momenta'] = [0, 1]
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "hutchinson")
    tp['max_nr_ests'] = 2048
    tp['tol'] = 1e-9
    res = stoch_trace.two_point(A, tp)
    capsys.readouterr()
    nr = res['nr_ests'] + 1
    assert set(res) == KEYS
    assert nr == 2048 and res['probes_solved'] == 2048
    assert res['momenta'] == [0, 1] and res['source_timeslice'] == 5
    shape = (2, 2, 2, 2, 2, 128)
    assert res['two_point'].shape == res['two_point_devs'].shape == res['converged'].shape == shape
    assert res['two_point_ests'].shape == (nr,) + shape and res['ests'].shape == (nr,)
    diff = np.abs(res['two_point'] - golden)
    bound = 5.0 * res['two_point_devs'] / np.sqrt(nr)
    ratio = diff / bound
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("two-point: worst |diff| / bound = %.3f at [p][a][b][c][d][t] = %s (|diff| %.3e, bound %.3e); entries over "
          "3/5 of the bound: %d of %d" % (ratio[at], at, diff[at], bound[at], int(np.sum(ratio > 0.6)), ratio.size))
    assert ratio.size == 4096 and np.all(diff < bound)
    pion = utils.meson_correlator(res['two_point'], 'g3', 'g3')[0]
    assert np.all(pion.real > 0)
    assert np.max(np.abs(res['two_point_ests'].mean(axis=0) - res['two_point'])) < 1e-9
    assert np.all(res['ests'].real > 0) and res['function_iters'] >= nr
