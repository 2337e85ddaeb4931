"""CPU: the double-double reference and the error bounds of the fp64 kernel tests (oracle/f64_bounds.py) separate
right from wrong.

tests/test_gpu_f64_kernels.py holds every fp64 operator kernel to two limits against a double-double evaluation
of the same operation: the worst-case rounding bound (4 K + 16) u S_i, u = 2^-53, and the tight limit
4 c_ref + 4, c_ref being what the NumPy float64 emulation of the kernel's arithmetic form loses.  Here the same
helpers run on the emulations alone, at the row lengths of those tests (K = 80: KS = 20, whose tail at 8 stages is
four k-steps; K = 16: KS = 4, fewer k-steps than an 8-stage prologue; K = 512: the dense Schur inverse, KS = 128):
the correct evaluations in either form and in another summation order pass both limits, and each defect a wrong
pipeline tail, block map or epilogue would cause fails the tight one by a wide margin."""
import numpy as np
import pytest

from oracle import f64_bounds as fb

W = 0.37 - 0.21j
NB = 35          # three 16-probe chunks, the last one ragged


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _operator(KS, seed):
    """4 row tiles writing tiles 3, 0, 2, 1 of a vector of n = max(4 KS, 64) rows: KS distinct 4-column groups per
    tile in a scrambled order"""
    n = max(4 * KS, 64)
    rng = np.random.default_rng(seed)
    kcol = np.stack([rng.permutation(n // 4)[:KS] * 4 for _ in range(4)]).astype(np.int32)
    return n, np.array([3, 0, 2, 1], dtype=np.int32), kcol, _rand((4, KS, 64), seed + 1)


CASES = {}


def _case(KS):
    if KS not in CASES:
        n, tmap, kcol, vals = _operator(KS, 100 + KS)
        X, B = _rand((n, NB), 7 + KS), _rand((n, NB), 8 + KS)
        AX, rows = fb.dd_block_rows(tmap, kcol, vals, X)
        M = fb.packed_matrix(tmap, kcol, vals, n)
        CASES[KS] = (n, tmap, kcol, vals, X, B, AX, fb.abs1_matrix(M) @ fb.abs1(X), rows, M)
    return CASES[KS]


def _ratio(Y, KS, mode):
    n, tmap, kcol, vals, X, B, AX, S_ax, rows, M = _case(KS)
    ref, low, S = fb.mode_reference(AX, S_ax, X, B, mode, W)
    return fb.error_ratio(Y, ref, S, rows, low)


def _c_ref(KS, mode, form):
    n, tmap, kcol, vals, X, B = _case(KS)[:6]
    return _ratio(fb.emulate_block_rows(tmap, kcol, vals, X, B, mode, W, form=form), KS, mode)


def test_double_double_primitives_are_exact():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(1000) * 2.0 ** rng.integers(-30, 30, 1000)
    b = rng.standard_normal(1000) * 2.0 ** rng.integers(-30, 30, 1000)
    from fractions import Fraction
    s, e = fb.two_sum(a, b)
    p, q = fb.two_prod(a, b)
    for i in range(0, 1000, 7):
        assert Fraction(s[i]) + Fraction(e[i]) == Fraction(a[i]) + Fraction(b[i])
        assert Fraction(p[i]) + Fraction(q[i]) == Fraction(a[i]) * Fraction(b[i])
    assert np.array_equal(s, a + b) and np.array_equal(p, a * b)


def test_double_double_sum_against_exact_rationals():
    """one row of a K = 80 operator against exact rational arithmetic: the double-double result is the correctly
    rounded one and its low part carries the rest to below 2^-100 of the scale"""
    from fractions import Fraction
    n, tmap, kcol, vals, X, B, AX, S_ax, rows, M = _case(20)
    ref, low, S = fb.mode_reference(AX, S_ax, X, B, 3, W)
    Mr = M.tocsr()
    w = complex(W)
    for row, col in ((int(rows[0]), 0), (int(rows[37]), NB - 1)):
        re = im = Fraction(0)
        for j, a in zip(Mr.indices[Mr.indptr[row]:Mr.indptr[row + 1]], Mr.data[Mr.indptr[row]:Mr.indptr[row + 1]]):
            x = X[j, col]
            re += Fraction(a.real) * Fraction(x.real) - Fraction(a.imag) * Fraction(x.imag)
            im += Fraction(a.real) * Fraction(x.imag) + Fraction(a.imag) * Fraction(x.real)
        tr, ti = Fraction(B[row, col].real) - re, Fraction(B[row, col].imag) - im
        yr = Fraction(X[row, col].real) + Fraction(w.real) * tr - Fraction(w.imag) * ti
        yi = Fraction(X[row, col].imag) + Fraction(w.real) * ti + Fraction(w.imag) * tr
        for exact, hi, lo in ((yr, ref[row, col].real, low[row, col].real), (yi, ref[row, col].imag, low[row, col].imag)):
            assert abs(Fraction(hi) + Fraction(lo) - exact) <= Fraction(2) ** -100 * Fraction(S[row, col])
            assert hi == float(exact)


def test_double_double_agrees_with_long_double():
    """a cross-check only where long double is wider than double (the reference itself never depends on it)"""
    if np.finfo(np.longdouble).nmant < 63:
        return
    n, tmap, kcol, vals, X, B, AX, S_ax, rows, M = _case(20)
    Md = M.toarray()
    Y = np.zeros((n, NB), dtype=np.clongdouble)
    Y[:] = (Md.real.astype(np.longdouble) @ X.real.astype(np.longdouble)
            - Md.imag.astype(np.longdouble) @ X.imag.astype(np.longdouble))
    Y += 1j * (Md.real.astype(np.longdouble) @ X.imag.astype(np.longdouble)
               + Md.imag.astype(np.longdouble) @ X.real.astype(np.longdouble))
    d = Y - AX.rounded().astype(np.clongdouble) - AX.low().astype(np.clongdouble)
    err = np.maximum(np.abs(d.real), np.abs(d.imag))[rows] / S_ax[rows]
    # long double: 2 K roundings of 2^-64 at the most
    assert float(err.max()) <= 2 * 80 * 2.0 ** -64


@pytest.mark.parametrize("KS", [4, 20, 128])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_correct_evaluations_pass_both_limits(KS, mode):
    n, tmap, kcol, vals, X, B, AX, S_ax, rows, M = _case(KS)
    hard = fb.hard_limit(4 * KS)
    c = {form: _c_ref(KS, mode, form) for form in ("4m", "3m")}
    for form in ("4m", "3m"):
        # a double-precision evaluation loses something, and far less than the worst case (also in three products)
        assert 0.1 < c[form] < 0.1 * hard, (form, c[form])
        # another order of the same sums: the k-steps in reverse
        rev = fb.emulate_block_rows(tmap, kcol[:, ::-1], vals[:, ::-1], X, B, mode, W, form=form)
        r = _ratio(rev, KS, mode)
        assert r <= fb.tight_limit(c[form]) and r <= hard, (form, r, c[form])
    # rows outside the tile map are not written
    seq = fb.emulate_block_rows(tmap, kcol, vals, X, B, mode, W)
    mask = np.ones(n, dtype=bool)
    mask[rows] = False
    assert not seq[mask].any()
    # the row-by-row evaluation (grouped-ELL order: sorted columns) of the same operator, and its double-double sum
    ell = fb.emulate_rows(M, X, B, mode, W)
    assert _ratio(ell, KS, mode) <= fb.tight_limit(c["4m"])
    rr = fb.dd_rows(M, X)
    assert fb.error_ratio(rr.rounded(), AX.rounded(), S_ax, rows, AX.low() - rr.low()) < 2.0 ** -40


DEFECTS = [
    ("a dropped k-step (the last)", 0, lambda KS: dict(drop_kstep=KS - 1)),
    ("a dropped k-step (in the middle)", 0, lambda KS: dict(drop_kstep=KS // 2)),
    ("a k-step applied twice (wrong tail re-load)", 0, lambda KS: dict(dup_kstep=KS - 1)),
    ("the tile beyond the last whole round of 8 stages dropped", 0, lambda KS: dict(drop_tail_of=8)),
    ("own-X rows of mode 3 from the next row tile", 3, lambda KS: dict(own_x_shift=1)),
    ("the sign of the w.y term flipped", 3, lambda KS: dict(flip_wy=True)),
    ("one (row tile, 16-probe chunk) left zero", 0, lambda KS: dict(zero_tile=(2, 1))),
    ("the ragged last chunk of one row tile left zero", 1, lambda KS: dict(zero_tile=(0, 2))),
]


# (KS = 128 is a multiple of every stage count: it has no tail to drop)
DEFECT_CASES = [(KS,) + d for KS in (4, 20, 128) for d in DEFECTS if not (KS == 128 and "stages dropped" in d[0])]


@pytest.mark.parametrize("form", ["4m", "3m"])
@pytest.mark.parametrize("KS,label,first_mode,make", DEFECT_CASES, ids=["KS %d: %s" % d[:2] for d in DEFECT_CASES])
def test_defects_are_rejected(KS, form, label, first_mode, make):
    """every defect is far over the tight limit in every mode it can occur in, at every row length -- also at
    K = 512, where the worst-case bound alone is three orders of magnitude wider than the kernels' error"""
    n, tmap, kcol, vals, X, B = _case(KS)[:6]
    kw = make(KS)
    for mode in ([3] if first_mode == 3 else [0, 1, 3]):
        bad = fb.emulate_block_rows(tmap, kcol, vals, X, B, mode, W, form=form, **kw)
        r = _ratio(bad, KS, mode)
        assert r > 1e6 * fb.tight_limit(_c_ref(KS, mode, form)), (label, mode, r)
