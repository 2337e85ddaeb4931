"""GPU: the three routes to the MLMC difference operator d = A_l^-1 x - P A_c^-1 R x (skip: A_0^-1 x - P_0 P_1 A_2^-1
R_1 R_0 x) -- the probe body of modes 7 / 8, sw_eig_apply_diff and sw_level_deflation_loops -- apply the same operator:
on the same 64 columns they agree bit for bit.  Every route keeps all 64 columns of its one column group occupied, so
none of them solves next to padding that another does not have.  Hierarchy and bars are those of
test_gpu_mlmc_loops.py."""
import os

import numpy as np
import pytest

import test_gpu_mlmc_loops as base

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import utils  # noqa: E402

MOMENTA = [0, 3]
TOL = 1e-12


@pytest.fixture(scope="module")
def p16():
    tv = np.load(os.path.join(base.HERE, "golden", "schwinger16_testvectors.npz"))
    p = base.Problem('schwinger16', [tv["tv0"], tv["tv1"]], {'accuracy_mg_eigvs': 'high'})
    assert [l.A.shape[0] for l in p.levels] == [512, 256, 64]
    p.eng.set_loop_momenta(MOMENTA)
    return p


def _eig_difference(p, level, skip, X):
    """D X of the 64 rows of X (64, n_level) through the eigen block: load, sw_eig_apply_diff without gamma_3, fetch."""
    eng = p.eng
    eng.eig_begin(0, level)
    try:
        eng.eig_load(0, X)
        eng.eig_apply_diff(0, 1, skip, 0, TOL)
        return eng.eig_fetch(1, 64)
    finally:
        eng.eig_end()


def _ascending_sum(per_column):
    total = np.zeros(per_column.shape[1:], dtype=np.complex128)
    for c in range(per_column.shape[0]):
        total = total + per_column[c]
    return total


def _tr1(p, level, skip, V):
    p.eng.set_level_deflation(level, V)
    try:
        return p.eng.level_deflation_loops(level, skip, TOL, 1000)
    finally:
        p.eng.set_level_deflation(level, None)


@pytest.mark.parametrize("skip", [False, True], ids=["l0", "l0skip"])
def test_probe_body_equals_eigen_route(p16, skip):
    """Mode 7 (skip: mode 8) on 64 z4 probes = k_slice_cdots of the probes and sw_eig_apply_diff of the probes."""
    p = p16
    np.random.seed(210)
    codes = utils.draw_probes(64, p.n, "z4")
    X = utils.probes_as_complex(codes)

    def body():
        loops, _, _ = p.eng.hutch_batch_mlmc_loops(0, codes, TOL, 1000, skip=skip)
        return loops, p.eng.apply_slice_cdots(X, _eig_difference(p, 0, skip, X))

    loops, routed = base._with_stop_factor(p, body)
    assert loops.shape == routed.shape == (64, len(MOMENTA), 2, 2, p.L)
    print("mode body vs eigen route, skip %s: %d of %d entries differ, max |diff| %.3e"
          % (skip, int(np.sum(loops != routed)), loops.size, np.max(np.abs(loops - routed))))
    assert np.max(np.abs(loops)) > 0
    assert np.array_equal(loops, routed)


@pytest.mark.parametrize("skip", [False, True], ids=["l0", "l0skip"])
def test_tr1_equals_eigen_route(p16, skip):
    """sw_level_deflation_loops of 64 orthonormal vectors at level 0 = the ascending sum over the columns of
    k_slice_cdots of the vectors and sw_eig_apply_diff of the vectors."""
    p = p16
    V = np.linalg.qr(base._rand((p.n, 64), 220))[0]
    X = np.ascontiguousarray(V.T)

    def body():
        return _tr1(p, 0, skip, V), p.eng.apply_slice_cdots(X, _eig_difference(p, 0, skip, X))

    tr1, per_column = base._with_stop_factor(p, body)
    routed = _ascending_sum(per_column)
    assert tr1.shape == routed.shape == (len(MOMENTA), 2, 2, p.L)
    print("tr1 vs eigen route, skip %s: %d of %d entries differ, max |diff| %.3e"
          % (skip, int(np.sum(tr1 != routed)), tr1.size, np.max(np.abs(tr1 - routed))))
    assert np.max(np.abs(tr1)) > 0
    assert np.array_equal(tr1, routed)


def test_tr1_equals_eigen_route_level_1(p16):
    """The same on level 1 (no skip).  The eigen route's block and image are prolonged to the lattice on the host with
    the problem's own P, a different rounding than the device's prolongation: every entry within 2e-10 of the largest
    sum_x |u| |v| of a column, the bar of test_level_deflation_loops_16."""
    p = p16
    n1 = p.levels[1].A.shape[0]
    V = np.linalg.qr(base._rand((n1, 64), 230))[0]
    X = np.ascontiguousarray(V.T)

    def body():
        return _tr1(p, 1, False, V), _eig_difference(p, 1, False, X)

    tr1, D = base._with_stop_factor(p, body)
    P0 = p.levels[0].P
    PiV = np.ascontiguousarray(np.asarray(P0 @ V).T)
    PiD = np.ascontiguousarray(np.asarray(P0 @ D.T).T)
    routed = _ascending_sum(p.eng.apply_slice_cdots(PiV, PiD))
    scale = np.max(base._weights(PiV, PiD, p.L))
    worst = np.max(np.abs(tr1 - routed)) / scale
    print("tr1 vs eigen route, level 1: max |diff| / max sum|u||v| = %.2e (max |tr1| / scale %.2e)"
          % (worst, np.max(np.abs(tr1)) / scale))
    assert worst < 2e-10
    assert np.max(np.abs(tr1)) > 1e-6 * scale
