"""Double-double reference, NumPy float64 emulations and error bounds for the per-kernel tests of the fp64
operator kernels (tests/test_gpu_f64_kernels.py on the GPU, tests/test_f64_bounds_host.py without one); the
complex64 counterpart is oracle/f32_bounds.py, whose operator packing helpers and limits are reused here.

An fp64 kernel computes y_i = sum_j a_ij x_j (plus the terms of its mode) in float64.  The reference evaluates
the same expression on the SAME float64 operands in double-double arithmetic (an unevaluated sum hi + lo of two
doubles: TwoSum for the additions, TwoProd by Veltkamp splitting for the products, no FMA and no long double
needed), unit roundoff about 2^-104: against u = 2^-53 it is exact.  It walks the stored entries of a row as the
emulations do and returns the result rounded to double, its low part and the scale

    S_i = sum_j (|Re a| + |Im a|)(|Re x| + |Im x|)  +  the absolute values of the other terms of the mode.

Limits, as for the complex64 kernels, with K = complex entries stored per row, padding included:

  hard limit    every real and imaginary part within (4 K + 16) u S_i, for any order of the sum.
                Four-product form (k_bsr_mfma, k_ell, the stencil): a part is a sum of 2 K products, each product
                rounded at most once and each partial sum once, so at most 2 K roundings touch any term:
                (1 + u)^(2K) - 1 is about 2 K u, half the limit; the epilogue of a mode adds fewer than eight.
                Three-product form (k_bsr_mfma3, k_dense_mfma3_lds): T1 = Ar Xr, T2 = Ai Xi,
                T3 = (Ar + Ai)(Xr + Xi), Re = T1 - T2, Im = T3 - T1 - T2.  A term of T3 is
                fl(Ar + Ai) fl(Xr + Xi), at most (|Ar| + |Ai|)(|Xr| + |Xi|)(1 + u)^2 -- exactly a term of S_i --
                and carries the two operand roundings plus at most K roundings of its sum of K products: K + 2
                against S_i.  T1 and T2 are sums of K products each; their terms |Ar Xr| and |Ai Xi| are
                DISJOINT parts of S_i, so together they carry K roundings against at most S_i.  The two final
                subtractions add fewer than four more: about (2 K + 6) u S_i in total for Im, less for Re --
                again half the limit.
  tight limit   max_i err / (u S_i) <= 4 c_ref + 4, c_ref the same figure of the float64 emulation of the kernel's
                arithmetic form (every product and every sum rounded, in NumPy: no FMA) against the
                double-double reference.  The factor covers another order of the same sums (the pipeline depth
                does not change it; 4-wide matrix-instruction blocks, fused multiply-adds do) and the epilogue.

Both are set by the arithmetic and the CPU emulation alone, never by what a kernel returned.
"""
import numpy as np
import scipy.sparse as sp

from oracle.f32_bounds import (abs1, abs1_matrix, column_errors, hard_limit, pack_dense,  # noqa: F401
                               packed_matrix, tight_limit)

U64 = 2.0 ** -53
_SPLIT = 134217729.0        # 2^27 + 1


# ---------------------------------------------------------------------------------------------------
# double-double arithmetic on float64 arrays: a value is the pair (hi, lo), |lo| <= ulp(hi) / 2
# ---------------------------------------------------------------------------------------------------
def two_sum(a, b):
    """s + e = a + b exactly, s = fl(a + b) (Knuth)"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _veltkamp(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """p + e = a b exactly, p = fl(a b) (Dekker, Veltkamp splitting; no overflow for |a|, |b| < 2^996)"""
    p = a * b
    ah, al = _veltkamp(a)
    bh, bl = _veltkamp(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_add(x, y):
    """(hi, lo) + (hi, lo)"""
    s, e = two_sum(x[0], y[0])
    e = e + (x[1] + y[1])
    hi = s + e
    return hi, e - (hi - s)


def dd_add_prod(acc, a, b, sign=1.0):
    """acc + sign a b, a and b doubles (sign = +-1: exact)"""
    p, e = two_prod(a, b)
    return dd_add(acc, (sign * p, sign * e))


def dd_mul_d(x, a):
    """(hi, lo) a, a double"""
    p, e = two_prod(x[0], a)
    e = e + x[1] * a
    hi = p + e
    return hi, e - (hi - p)


def dd_neg(x):
    return -x[0], -x[1]


def _dd_zero(shape):
    return np.zeros(shape), np.zeros(shape)


def _dd_of(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, np.zeros_like(a)


class DD:
    """A complex double-double array: re and im are (hi, lo) pairs."""

    def __init__(self, re, im):
        self.re, self.im = re, im

    def rounded(self):
        return self.re[0] + 1j * self.im[0]

    def low(self):
        return self.re[1] + 1j * self.im[1]

    def __getitem__(self, idx):
        return DD((self.re[0][idx], self.re[1][idx]), (self.im[0][idx], self.im[1][idx]))


def _dd_cfma(re, im, vr, vi, xr, xi):
    """(re, im) += (vr + i vi)(xr + i xi), all four products exact"""
    re = dd_add_prod(re, vr, xr)
    re = dd_add_prod(re, vi, xi, -1.0)
    im = dd_add_prod(im, vr, xi)
    im = dd_add_prod(im, vi, xr)
    return re, im


def dd_block_rows(tmap, kcol, vals, X):
    """op X of a block-row operator (tmap[RT], kcol[RT, KS], vals[RT, KS, 64]) in double-double, walking the
    stored entries k-step by k-step: DD arrays [n, nb], zero in the rows no tile writes, and `rows`."""
    RT, KS = kcol.shape
    X = np.asarray(X, dtype=np.complex128)
    n, nb = X.shape
    v = np.asarray(vals, dtype=np.complex128).reshape(RT, KS, 4, 16)
    xr, xi = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)
    re, im = _dd_zero((RT, 16, nb)), _dd_zero((RT, 16, nb))
    for ks in range(KS):
        cols = kcol[:, ks].astype(np.int64)
        for c in range(4):
            a = v[:, ks, c, :, None]
            re, im = _dd_cfma(re, im, a.real, a.imag, xr[cols + c][:, None, :], xi[cols + c][:, None, :])
    rows = (np.asarray(tmap, dtype=np.int64)[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)
    out = DD(_dd_zero((n, nb)), _dd_zero((n, nb)))
    for q in (0, 1):
        out.re[q][rows] = re[q].reshape(RT * 16, nb)
        out.im[q][rows] = im[q].reshape(RT * 16, nb)
    return out, rows


def _ell_of(M):
    """(cols[nr, K], vals[nr, K]) of a sparse matrix, the entries of a row in column order, zero padding"""
    M = sp.csr_matrix(M)
    M.sort_indices()
    nr = M.shape[0]
    cnt = np.diff(M.indptr)
    K = int(cnt.max()) if nr else 0
    cols = np.zeros((nr, K), dtype=np.int64)
    vals = np.zeros((nr, K), dtype=np.complex128)
    pos = np.arange(M.nnz) - np.repeat(M.indptr[:-1], cnt)
    rr = np.repeat(np.arange(nr), cnt)
    cols[rr, pos] = M.indices
    vals[rr, pos] = M.data
    return cols, vals


def dd_rows(M, X):
    """M X of a sparse matrix in double-double, row by row over the stored entries"""
    cols, vals = _ell_of(M)
    X = np.asarray(X, dtype=np.complex128)
    shape = (cols.shape[0], X.shape[1])
    re, im = _dd_zero(shape), _dd_zero(shape)
    for k in range(cols.shape[1]):
        x = X[cols[:, k]]
        a = vals[:, k, None]
        re, im = _dd_cfma(re, im, a.real, a.imag, np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag))
    return DD(re, im)


def mode_reference(AX, S_ax, X, B, mode, w):
    """(y_ref rounded to double, its low part, S) of a mode from the double-double AX = op X and the float64
    S_ax = |op| |X|: 0: op X, 1: B - op X, 3: X + w (B - op X), w in full double precision, all in double-double"""
    if mode == 0:
        return AX.rounded(), AX.low(), S_ax
    B = np.asarray(B, dtype=np.complex128)
    tr = dd_add(_dd_of(B.real), dd_neg(AX.re))
    ti = dd_add(_dd_of(B.imag), dd_neg(AX.im))
    if mode == 1:
        t = DD(tr, ti)
        return t.rounded(), t.low(), abs1(B) + S_ax
    X = np.asarray(X, dtype=np.complex128)
    w = complex(w)
    re = dd_add(dd_add(_dd_of(X.real), dd_mul_d(tr, w.real)), dd_mul_d(ti, -w.imag))
    im = dd_add(dd_add(_dd_of(X.imag), dd_mul_d(ti, w.real)), dd_mul_d(tr, w.imag))
    y = DD(re, im)
    return y.rounded(), y.low(), abs1(X) + (abs(w.real) + abs(w.imag)) * (abs1(B) + S_ax)


def error_ratio(Y, Y_ref, S, rows=None, low=None, u=U64):
    """max over the entries (real and imaginary parts separately) of |y - y_ref| / (u S_i); rows: the rows the
    operation writes (default: all); low: the low part of a double-double reference (y - hi is exact wherever the
    two are close, so the difference is taken against hi + lo).  An entry with S_i = 0 must be exact."""
    Y, Y_ref, S = np.asarray(Y), np.asarray(Y_ref), np.asarray(S)
    low = np.zeros_like(Y_ref) if low is None else np.asarray(low)
    if rows is not None:
        Y, Y_ref, S, low = Y[rows], Y_ref[rows], S[rows], low[rows]
    d = np.maximum(np.abs((Y.real - Y_ref.real) - low.real), np.abs((Y.imag - Y_ref.imag) - low.imag))
    zero = S == 0
    if np.any(d[zero] != 0):
        return np.inf
    if zero.all():
        return 0.0
    return float((d[~zero] / (u * S[~zero])).max())


# ---------------------------------------------------------------------------------------------------
# float64 emulations of the kernels' arithmetic forms (every product and every sum rounded)
# ---------------------------------------------------------------------------------------------------
def _epilogue64(yr, yi, X, B, mode, w, flip_wy=False):
    """the mode arithmetic of the kernels' epilogues in float64: 1: B - y, 3: X + w (B - y), one product and one
    sum after the other; flip_wy: the w.y terms with the wrong sign (a defect)"""
    if mode == 0:
        return yr, yi
    B = np.asarray(B, dtype=np.complex128)
    tr, ti = B.real - yr, B.imag - yi
    if mode == 1:
        return tr, ti
    X = np.asarray(X, dtype=np.complex128)
    w = complex(w)
    wy = -w.imag if flip_wy else w.imag
    return (X.real + w.real * tr) - wy * ti, (X.imag + w.real * ti) + wy * tr


def emulate_block_rows(tmap, kcol, vals, X, B=None, mode=0, w=0.0, form="4m", drop_kstep=None, dup_kstep=None,
                       drop_tail_of=None, own_x_shift=0, flip_wy=False, zero_tile=None):
    """Float64 evaluation of a block-row operator on X[n, nb], the k-steps of a row tile one after the other and
    the four columns of a k-step one after the other.
      form "4m"   k_bsr_mfma: the four real sums Ar Xr, Ai Xi, Ar Xi, Ai Xr accumulated separately (two matrix
                  instructions per k-step, the real and imaginary parts of the probes side by side), then
                  Re = Ar Xr - Ai Xi, Im = Ar Xi + Ai Xr
      form "3m"   k_bsr_mfma3 / k_dense_mfma3_lds: T1 = Ar Xr, T2 = Ai Xi, T3 = fl(Ar + Ai) fl(Xr + Xi),
                  Re = T1 - T2, Im = (T3 - T1) - T2
    The defects the bounds must reject: drop_kstep leaves one k-step out, dup_kstep adds one twice (a wrong tail
    re-load), drop_tail_of = STG leaves out the k-steps beyond the last whole round of STG (a dropped tile when
    KS % STG != 0), own_x_shift takes the own-X rows of mode 3 from the row tile that many tiles on, flip_wy flips
    the sign of the w.y terms, zero_tile = (row tile, 16-probe chunk) leaves that block of the output zero.
    Returns complex128 [n, nb]; rows no tile writes are zero."""
    RT, KS = kcol.shape
    X = np.asarray(X, dtype=np.complex128)
    n, nb = X.shape
    v = np.asarray(vals, dtype=np.complex128).reshape(RT, KS, 4, 16)
    xr, xi = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)
    acc = [np.zeros((RT, 16, nb)) for _ in range(4)]
    steps = []
    for ks in range(KS):
        if ks == drop_kstep or (drop_tail_of and ks >= (KS // drop_tail_of) * drop_tail_of):
            continue
        steps.append(ks)
        if ks == dup_kstep:
            steps.append(ks)
    for ks in steps:
        cols = kcol[:, ks].astype(np.int64)
        for c in range(4):
            ar, ai = v[:, ks, c, :, None].real, v[:, ks, c, :, None].imag
            pr, pi = xr[cols + c][:, None, :], xi[cols + c][:, None, :]
            acc[0] = acc[0] + ar * pr
            acc[1] = acc[1] + ai * pi
            if form == "4m":
                acc[2] = acc[2] + ar * pi
                acc[3] = acc[3] + ai * pr
            else:
                acc[2] = acc[2] + (ar + ai) * (pr + pi)
    re = acc[0] - acc[1]
    im = acc[2] + acc[3] if form == "4m" else (acc[2] - acc[0]) - acc[1]
    tmap = np.asarray(tmap, dtype=np.int64)
    rows = (tmap[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)
    own = (np.roll(tmap, -own_x_shift)[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)
    re, im = re.reshape(RT * 16, nb), im.reshape(RT * 16, nb)
    Xr = None if mode != 3 else X[own]
    Br = None if mode == 0 else np.asarray(B)[rows]
    yr, yi = _epilogue64(re, im, Xr, Br, mode, w, flip_wy)
    if zero_tile is not None:
        rt, ch = zero_tile
        yr, yi = yr.copy(), yi.copy()
        yr[16 * rt:16 * rt + 16, 16 * ch:16 * ch + 16] = 0.0
        yi[16 * rt:16 * rt + 16, 16 * ch:16 * ch + 16] = 0.0
    out = np.zeros((n, nb), dtype=np.complex128)
    out[rows] = yr + 1j * yi
    return out


def emulate_rows(M, X, B=None, mode=0, w=0.0):
    """Float64 evaluation of a sparse operator row by row, the stored entries of a row one after the other in
    column order, four real products per complex term, each rounded (k_ell and, for the limits, the stencil)."""
    cols, vals = _ell_of(M)
    X = np.asarray(X, dtype=np.complex128)
    re = np.zeros((cols.shape[0], X.shape[1]))
    im = np.zeros_like(re)
    for k in range(cols.shape[1]):
        x = X[cols[:, k]]
        vr, vi = vals[:, k, None].real, vals[:, k, None].imag
        re = (re + vr * x.real) - vi * x.imag
        im = (im + vr * x.imag) + vi * x.real
    yr, yi = _epilogue64(re, im, X, B, mode, w)
    return yr + 1j * yi
