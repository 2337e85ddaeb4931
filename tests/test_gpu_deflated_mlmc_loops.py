"""GPU: the deflated MLMC loops (SW_MODE_MLMC_DEFL_LOOPS / _SKIP, sw_level_deflation_loops,
stoch_trace.deflated_mlmc_loops) -- the per-probe level terms with a registered projection against sparse LU and the
host transfer operators, the control identity against SW_MODE_MLMC with the same vectors, bit-equality with modes
7 / 8 when no vectors are registered, the sliced tr1 against dense algebra, and the flow on schwinger128 against the
exact loops.  Hierarchy, probes and bars are those of test_gpu_mlmc_loops.py."""
import os

import numpy as np
import pytest

import test_gpu_mlmc_loops as base

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import matrix, stoch_trace, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import (MODE_MLMC, MODE_MLMC_DEFL_LOOPS, MODE_MLMC_SKIP,  # noqa: E402
                                               EngineError)

MOMENTA = [0, 1, 15]
CASES = [(0, False), (1, False), (0, True)]
IDS = ["l0", "l1", "l0skip"]


@pytest.fixture(scope="module")
def p16():
    tv = np.load(os.path.join(base.HERE, "golden", "schwinger16_testvectors.npz"))
    p = base.Problem('schwinger16', [tv["tv0"], tv["tv1"]], {'accuracy_mg_eigvs': 'high'})
    assert [l.A.shape[0] for l in p.levels] == [512, 256, 64]
    return p


def _orthonormal(n, k, seed):
    return np.linalg.qr(base._rand((n, k), seed))[0]


def _projected(X, V):
    """x - V V^H x for the rows x of X."""
    return X - (X @ V.conj()) @ V.T


def _operands(p, level, skip, X, V):
    """(Pi x, Pi D (x - V V^H x)) of the rows of X from the exact level solves."""
    U, _ = p.level_operands(level, skip, X)
    _, W = p.level_operands(level, skip, _projected(X, V))
    return U, W


def _difference(p, level, skip, V):
    """D V on the level itself, V (n_level, k), from the exact level solves."""
    lev = p.levels
    V = np.ascontiguousarray(V, dtype=np.complex128)
    Rv = lev[level].R @ V
    if skip:
        Y = lev[1].P @ p.solve(level + 2, lev[1].R @ Rv)
    else:
        Y = p.solve(level + 1, Rv)
    return np.asarray(p.solve(level, V) - lev[level].P @ Y)


def _registered(p, level, V, body):
    p.eng.set_level_deflation(level, V)
    try:
        return base._with_stop_factor(p, body)
    finally:
        p.eng.set_level_deflation(level, None)


# ---- modes 9 / 10 per probe -------------------------------------------------------------------------------
# k = 65: two 64-column groups of the projection (the matrix-core pair), level 0 only
@pytest.mark.parametrize("kind", ["z2", "z4"])
@pytest.mark.parametrize("level,skip,k", [(0, False, 4), (1, False, 4), (0, True, 4), (0, False, 65), (0, True, 65)],
                         ids=["l0", "l1", "l0skip", "l0-k65", "l0skip-k65"])
def test_per_probe_parity_16(p16, level, skip, k, kind):
    """A mode-9 (skip: mode-10) batch against slice_cdots(Pi x, Pi D (x - V V^H x)) of the oracle's operands: every
    entry within 2e-10 of the batch's largest sum_x |u| |v|."""
    p = p16
    n = p.levels[level].A.shape[0]
    np.random.seed(50 + level)
    codes = utils.draw_probes(6, n, kind)
    V = _orthonormal(n, k, 90 + level)
    p.eng.set_loop_momenta(MOMENTA)
    loops, itf, itc = _registered(
        p, level, V, lambda: p.eng.hutch_batch_mlmc_loops(level, codes, 1e-12, 1000, skip=skip, deflated=True))
    assert loops.shape == (6, len(MOMENTA), 2, 2, p.L) and itf.min() >= 1 and itc.min() >= 1
    U, W = _operands(p, level, skip, utils.probes_as_complex(codes), V)
    ref = utils.slice_cdots(U, W, p.L, MOMENTA)
    scale = np.max(base._weights(U, W, p.L))
    worst = np.max(np.abs(loops - ref)) / scale
    # the projection is not a no-op: the undeflated operands differ from these by far more than the bar
    plain = utils.slice_cdots(*p.level_operands(level, skip, utils.probes_as_complex(codes)), p.L, MOMENTA)
    print("deflated parity level %d skip %s k %d %s: max |l - ref| / max sum|u||v| = %.2e (max |ref| / scale %.2e, "
          "max |undeflated - ref| / scale %.2e)" % (level, skip, k, kind, worst, np.max(np.abs(ref)) / scale,
                                                     np.max(np.abs(plain - ref)) / scale))
    assert worst < 2e-10
    assert np.max(np.abs(ref)) > 1e-6 * scale
    assert np.max(np.abs(plain - ref)) > 1e-6 * scale


@pytest.mark.parametrize("level,skip", CASES, ids=IDS)
def test_control_value_is_the_scalar_mlmc_estimate_16(p16, level, skip):
    """sw_hutch_fetch after a mode-9 / 10 batch = the SW_MODE_MLMC / _SKIP estimate of the same probes with the same
    vectors registered (no perm, no rhsmap), and = the scalar total of the fetched loops."""
    p = p16
    n = p.levels[level].A.shape[0]
    np.random.seed(70 + level)
    codes = utils.draw_probes(6, n, "z4")
    V = _orthonormal(n, 4, 95 + level)
    p.eng.set_loop_momenta([0, 3])

    def both():
        e, _, _ = p.eng.hutch_batch(MODE_MLMC_SKIP if skip else MODE_MLMC, level, codes, 1e-12, 1000)
        loops, _, _ = p.eng.hutch_batch_mlmc_loops(level, codes, 1e-12, 1000, skip=skip, deflated=True)
        first, _, _ = p.eng.hutch_fetch()
        return e, loops, first

    e, loops, first = _registered(p, level, V, both)
    total = np.sum(loops[:, 0, 0, 0, :] + loops[:, 0, 1, 1, :], axis=1)
    scale = np.maximum(np.abs(e), 0.1 * n)
    rel_dev, rel_host = np.max(np.abs(first - e) / scale), np.max(np.abs(total - e) / scale)
    print("deflated control level %d skip %s: sw_hutch_fetch %.2e, host sum %.2e relative"
          % (level, skip, rel_dev, rel_host))
    assert rel_dev < 1e-10 and rel_host < 1e-10


@pytest.mark.parametrize("level,skip", CASES, ids=IDS)
def test_without_vectors_the_batch_is_the_mode_7_batch(p16, level, skip):
    p = p16
    np.random.seed(110 + level)
    codes = utils.draw_probes(6, p.levels[level].A.shape[0], "z4")
    p.eng.set_loop_momenta(MOMENTA)
    p.eng.set_level_deflation(level, None)

    def body():
        plain, _, _ = p.eng.hutch_batch_mlmc_loops(level, codes, 1e-12, 1000, skip=skip)
        e7, _, _ = p.eng.hutch_fetch()
        defl, _, _ = p.eng.hutch_batch_mlmc_loops(level, codes, 1e-12, 1000, skip=skip, deflated=True)
        e9, _, _ = p.eng.hutch_fetch()
        return plain, e7, defl, e9

    plain, e7, defl, e9 = base._with_stop_factor(p, body)
    assert np.max(np.abs(plain)) > 0
    assert np.array_equal(defl, plain) and np.array_equal(e9, e7)


def test_two_runs_agree_and_other_modes_return_the_same_after_a_mode_9_batch(p16):
    p = p16
    np.random.seed(81)
    c0 = utils.draw_probes(6, p.n, "z4")
    c1 = utils.draw_probes(6, 256, "z2")
    p.eng.set_loop_momenta(MOMENTA)
    V0, V1 = _orthonormal(p.n, 4, 120), _orthonormal(256, 4, 121)

    def run():
        e1, _, _ = p.eng.hutch_batch(MODE_MLMC, 1, c1, 1e-12, 1000)
        e2, _, _ = p.eng.hutch_batch(MODE_MLMC_SKIP, 0, c0, 1e-12, 1000)
        l5, _, _ = p.eng.hutch_batch_loops(0, c0, 1e-12, 1000)
        return e1, e2, l5

    def body():
        before = run()
        m9, _, _ = p.eng.hutch_batch_mlmc_loops(1, c1, 1e-12, 1000, deflated=True)
        assert np.array_equal(p.eng.hutch_fetch_loops(), before[2])       # mode 5's buffer survived the mode-9 batch
        m10, _, _ = p.eng.hutch_batch_mlmc_loops(0, c0, 1e-12, 1000, skip=True, deflated=True)
        after = run()
        assert np.array_equal(p.eng.hutch_fetch_mlmc_loops(), m10)        # and the reverse
        again, _, _ = p.eng.hutch_batch_mlmc_loops(1, c1, 1e-12, 1000, deflated=True)
        assert np.array_equal(again, m9)
        return before, after

    p.eng.set_level_deflation(1, V1)
    try:
        before, after = _registered(p, 0, V0, body)
    finally:
        p.eng.set_level_deflation(1, None)
    for b, a in zip(before, after):
        assert np.array_equal(a, b)


# ---- the sliced tr1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,skip,k", [(0, False, 4), (1, False, 4), (0, True, 4), (0, False, 65)],
                         ids=["l0", "l1", "l0skip", "l0-k65"])
def test_level_deflation_loops_16(p16, level, skip, k):
    """sum_j S_q(Pi V_j, Pi D V_j) against sliced_level_tr1 of the oracle's operands: every entry within 2e-10 of
    the largest sum_x |u| |v| of a column; two calls bit-identical; the scalar total = trace(V^H D V)."""
    p = p16
    n = p.levels[level].A.shape[0]
    V = _orthonormal(n, k, 130 + level)
    p.eng.set_loop_momenta(MOMENTA)

    def body():
        a = p.eng.level_deflation_loops(level, skip, 1e-12, 1000)
        return a, p.eng.level_deflation_loops(level, skip, 1e-12, 1000)

    got, again = _registered(p, level, V, body)
    assert got.shape == (len(MOMENTA), 2, 2, p.L)
    PiV, PiDV = p.level_operands(level, skip, V.T)
    ref = utils.sliced_level_tr1(PiV, PiDV, p.L, MOMENTA)
    scale = np.max(base._weights(PiV, PiDV, p.L))
    worst = np.max(np.abs(got - ref)) / scale
    print("level deflation loops level %d skip %s k %d: max |tr1 - ref| / max sum|u||v| = %.2e (max |ref| / scale "
          "%.2e)" % (level, skip, k, worst, np.max(np.abs(ref)) / scale))
    assert worst < 2e-10
    assert np.max(np.abs(ref)) > 1e-6 * scale
    assert np.array_equal(again, got)
    # the prolongations have orthonormal columns (Pi^H Pi = I): the total is trace(V^H D V) on the level itself
    trace = np.sum(V.conj() * _difference(p, level, skip, V))
    total = np.sum(got[0, 0, 0] + got[0, 1, 1])
    print("  scalar total %s, trace(V^H D V) %s" % (total, trace))
    assert abs(total - trace) < 1e-10 * abs(trace)


def test_level_deflation_loops_refusals(p16):
    eng = p16.eng
    V = _orthonormal(256, 4, 140)
    try:
        eng.set_level_deflation(1, V)
        eng.set_loop_momenta(None)
        with pytest.raises(EngineError, match="no momenta registered"):
            eng.level_deflation_loops(1)
        with pytest.raises(EngineError, match="no momenta registered"):
            eng.hutch_batch(MODE_MLMC_DEFL_LOOPS, 1, np.ones((2, 256), dtype=np.int8), 1e-12, 100)
        eng.set_loop_momenta([0, 1])
        with pytest.raises(EngineError, match="no deflation vectors registered at level 0"):
            eng.level_deflation_loops(0)
        with pytest.raises(EngineError, match="level 0 only"):
            eng.level_deflation_loops(1, skip=True)
        with pytest.raises(EngineError, match="no coarse level"):
            eng.level_deflation_loops(2)
        with pytest.raises(EngineError, match="no coarse level"):
            eng.hutch_batch(MODE_MLMC_DEFL_LOOPS, 2, np.ones((2, 64), dtype=np.int8), 1e-12, 100)
        with pytest.raises(EngineError, match="level 0 only"):
            eng.hutch_batch_mlmc_loops(1, np.ones((2, 256), dtype=np.int8), 1e-12, 100, skip=True, deflated=True)
    finally:
        eng.set_level_deflation(1, None)
        eng.set_loop_momenta([0])


# ---- the flow ---------------------------------------------------------------------------------------------
def flow_params():
    """test_gpu_mlmc_loops.flow_params with 8 vectors on the difference levels 0 and 2, computed on the device."""
    params, tp = base.flow_params()
    tp['mlmc_deflat_vctrs'] = [8, 0, 8, 0]
    tp['mlmc_defl_setup'] = 'device'
    return params, tp


def test_flow_128_against_the_exact_loops(capsys):
    """Every one of the 4 x 2 x 2 x 128 entries of `loops` within 5 loop_errs of the exact value, and the trace
    within 5 of its error of the exact scalar total.  Checked before seed, tolerance and probe count were fixed:
    the same stream probes (seed 123456: 5 rough probes, then 256 of level 0, then 256 of level 2) replayed on the CPU
    through sparse LU, the host P and R and the dense coarsest inverse, with the vectors the run registered (8 per
    level from the device eigensolver) and sliced_level_tr1 of their exact D V, meet the same condition on their own
    (worst entry 0.570 of the bound, none of the 2048 over 0.6, trace 0.297 of its bound); the flow's per-probe level
    loops agree with that replay to 1.9e-12 (level 0) and 6.2e-12 (level 2) of the largest entry, its loop_tr1 to
    2.4e-14 and 1.0e-13."""
    golden = base._golden_loops()
    params, tp = flow_params()
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    res = stoch_trace.deflated_mlmc_loops(A, tp)
    capsys.readouterr()
    N = base.FLOW_MAX_NR_ESTS
    assert res['momenta'] == [0, 1, 2, 3] and res['nr_levels'] == 4
    shape = (4, 2, 2, 128)
    assert res['loops'].shape == res['loop_errs'].shape == golden.shape == shape
    for i in (0, 2):
        lev = res['results'][i]
        assert lev['nr_ests'] + 1 == N and lev['probes_solved'] == N
        assert lev['loops'].shape == lev['loop_devs'].shape == lev['converged'].shape == shape
        assert lev['loop_tr1'].shape == shape and np.max(np.abs(lev['loop_tr1'])) > 1e-3
        assert lev['loop_ests'].shape == (N,) + shape
        assert np.max(np.abs(lev['loops'] - lev['loop_ests'].mean(axis=0) - lev['loop_tr1'])) < 1e-9
        total = np.sum(lev['loop_ests'][:, 0, 0, 0, :] + lev['loop_ests'][:, 0, 1, 1, :], axis=1)
        assert np.max(np.abs(total - lev['ests'])) < 1e-9 * np.max(np.abs(lev['ests']))
        t1 = np.sum(lev['loop_tr1'][0, 0, 0] + lev['loop_tr1'][0, 1, 1])
        assert abs(lev['ests_avg'] - np.mean(lev['ests']) - t1) < 1e-9 * abs(lev['ests_avg'])
    assert not np.any(res['results'][1]['loops']) and res['results'][1]['nr_ests'] == 0
    assert res['results'][3]['loops'].shape == shape and np.max(np.abs(res['results'][3]['loops'])) > 1e-3
    diff = np.abs(res['loops'] - golden)
    bound = 5.0 * res['loop_errs']
    ratio = diff / bound
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("loops: worst |diff| / bound = %.3f at [p][a][b][t] = %s (|diff| %.3e, bound %.3e); entries over 3/5 of the "
          "bound: %d of %d" % (ratio[at], at, diff[at], bound[at], int(np.sum(ratio > 0.6)), ratio.size))
    assert np.all(diff < bound)
    err = np.sqrt(sum(res['results'][i]['ests_dev'] ** 2 / (res['results'][i]['nr_ests'] + 1) for i in (0, 2)))
    exact = np.sum(golden[0, 0, 0] + golden[0, 1, 1])
    print("trace %s |diff| %.3e bound %.3e" % (res['trace'], abs(res['trace'] - exact), 5.0 * err))
    assert abs(res['trace'] - exact) < 5.0 * err
