"""CPU: the error bounds of the complex64 kernel tests (oracle/f32_bounds.py) separate right from wrong.

The GPU file tests/test_gpu_f32_kernels.py holds every complex64 kernel to two limits against a complex128
evaluation of the same operation: the worst-case rounding bound (4 K + 16) u S_i and the tight limit
4 c_ref + 4, c_ref being what a sequential NumPy float32 evaluation loses.  Here the same helpers run on the
float32 emulation alone, at the two row lengths of those tests (K = 80: five site blocks, KS = 20, and
K = 1024: a dense 1024-column operator, KS = 256): a correct evaluation in ANOTHER summation order passes
both limits, one that skips a k-step or leaves out a split-K partial sum fails the tight one."""
import numpy as np
import pytest

from oracle import f32_bounds as fb


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _operator(KS, seed):
    """4 row tiles writing tiles 3, 0, 2, 1 of a 16 KS-row vector... of n = max(4 KS, 64) rows: KS distinct
    4-column groups per tile in a scrambled order"""
    n = max(4 * KS, 64)
    rng = np.random.default_rng(seed)
    RT = 4
    kcol = np.stack([rng.permutation(n // 4)[:KS] * 4 for _ in range(RT)]).astype(np.int32)
    vals = fb.c64(_rand((RT, KS, 64), seed + 1))
    tmap = np.array([3, 0, 2, 1], dtype=np.int32)
    return n, tmap, kcol, vals


CASES = {}


def _case(KS):
    if KS not in CASES:
        n, tmap, kcol, vals = _operator(KS, 100 + KS)
        X, B = fb.c64(_rand((n, 5), 7 + KS)), fb.c64(_rand((n, 5), 8 + KS))
        M = fb.packed_matrix(tmap, kcol, vals, n)
        AX, S_ax = M @ X, fb.abs1_matrix(M) @ fb.abs1(X)
        rows = (tmap.astype(np.int64)[:, None] * 16 + np.arange(16)).reshape(-1)
        CASES[KS] = (n, tmap, kcol, vals, X, B, AX, S_ax, rows)
    return CASES[KS]


W = 0.37 - 0.21j


@pytest.mark.parametrize("KS", [20, 256])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_correct_evaluations_pass_both_limits(KS, mode):
    n, tmap, kcol, vals, X, B, AX, S_ax, rows = _case(KS)
    ref, S = fb.mode_reference(AX, S_ax, X, B, mode, W)
    seq = fb.emulate_block_rows(tmap, kcol, vals, X, B, mode, W)
    c_ref = fb.error_ratio(seq, ref, S, rows)
    # a single-precision evaluation loses something, and far less than the worst case
    assert 0.1 < c_ref < 0.05 * fb.hard_limit(4 * KS), c_ref
    # other summation orders of the same sum: four split-K partial sums; the k-steps in reverse
    sk = fb.emulate_block_rows(tmap, kcol, vals, X, B, mode, W, splitk=True)
    rev = fb.emulate_block_rows(tmap, kcol[:, ::-1], vals[:, ::-1], X, B, mode, W)
    for other in (sk, rev):
        r = fb.error_ratio(other, ref, S, rows)
        assert r <= fb.tight_limit(c_ref), (r, c_ref)
        assert r <= fb.hard_limit(4 * KS)
    # rows outside the tile map are not written
    mask = np.ones(n, dtype=bool)
    mask[rows] = False
    assert not seq[mask].any()
    # the row-by-row evaluation (grouped-ELL order: sorted columns) of the same operator agrees as well
    ell = fb.emulate_rows(fb.packed_matrix(tmap, kcol, vals, n), X, B, mode, W)
    assert fb.error_ratio(ell, ref, S, rows) <= fb.tight_limit(c_ref)


@pytest.mark.parametrize("KS", [20, 256])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_a_dropped_kstep_is_rejected(KS, mode):
    """the tail k-step (and one in the middle) left out of the sum: far over the tight limit at both row
    lengths, although at K = 1024 the worst-case bound alone would nearly let it through"""
    n, tmap, kcol, vals, X, B, AX, S_ax, rows = _case(KS)
    ref, S = fb.mode_reference(AX, S_ax, X, B, mode, W)
    c_ref = fb.error_ratio(fb.emulate_block_rows(tmap, kcol, vals, X, B, mode, W), ref, S, rows)
    for drop in (KS - 1, KS // 2):
        bad = fb.emulate_block_rows(tmap, kcol, vals, X, B, mode, W, drop_kstep=drop)
        r = fb.error_ratio(bad, ref, S, rows)
        assert r > 100 * fb.tight_limit(c_ref), (drop, r, c_ref)


@pytest.mark.parametrize("KS", [20, 256])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_a_missing_splitk_partial_sum_is_rejected(KS, mode):
    n, tmap, kcol, vals, X, B, AX, S_ax, rows = _case(KS)
    ref, S = fb.mode_reference(AX, S_ax, X, B, mode, W)
    c_ref = fb.error_ratio(fb.emulate_block_rows(tmap, kcol, vals, X, B, mode, W), ref, S, rows)
    for q in range(4):
        bad = fb.emulate_block_rows(tmap, kcol, vals, X, B, mode, W, splitk=True, drop_partial=q)
        r = fb.error_ratio(bad, ref, S, rows)
        assert r > 100 * fb.tight_limit(c_ref), (q, r, c_ref)


def test_dense_packing_round_trip():
    M = fb.c64(_rand((64, 64), 3))
    tmap, kcol, vals = fb.pack_dense(M)
    assert kcol.shape == (4, 16)
    assert np.array_equal(fb.packed_matrix(tmap, kcol, vals, 64).toarray(), M)


def test_smoother_recurrence_in_both_precisions():
    """the even-odd smoother model: complex64 against complex128 differs at single-precision level, and the
    reduced form is the full form with b_o = 0 on the even rows"""
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    ne = 24
    Aeo = sp.random(ne, ne, density=0.2, random_state=1, data_rvs=rng.standard_normal).tocsr() * (1 + 0.5j)
    Aoe = sp.random(ne, ne, density=0.2, random_state=2, data_rvs=rng.standard_normal).tocsr() * (1 - 0.5j)
    E, O = np.arange(0, 2 * ne, 2), np.arange(1, 2 * ne, 2)
    B, X = fb.c64(_rand((2 * ne, 3), 1)), fb.c64(_rand((2 * ne, 3), 2))
    w = [0.2 + 0.01j, 0.15 - 0.02j, 0.1]
    hi = fb.eo_smoother(Aeo, Aoe, 4.1, w, B, X, E, O, False, np.complex128)
    lo = fb.eo_smoother(Aeo, Aoe, 4.1, w, B, X, E, O, False, np.complex64)
    err = fb.column_errors(lo, hi)
    assert (err > 1e-9).all() and (err < 1e-5).all(), err
    B0 = B.copy()
    B0[O] = 0
    full = fb.eo_smoother(Aeo, Aoe, 4.1, w, B0, X, E, O, False, np.complex128)
    red = fb.eo_smoother(Aeo, Aoe, 4.1, w, B0, X, E, O, True, np.complex128)
    assert np.array_equal(full[E], red[E]) and not red[O].any()
