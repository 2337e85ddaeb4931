"""Error bounds and NumPy float32 emulations for the per-kernel tests of the complex64 preconditioner
(tests/test_gpu_f32_kernels.py on the GPU, tests/test_f32_bounds_host.py without one).

A complex64 kernel computes y_i = sum_j a_ij x_j (plus the terms of its mode) in float32, four real products
per complex term.  Against the same expression evaluated in complex128 on the SAME complex64-rounded
operands, every real and imaginary part obeys, for any order of the sum,

    |y - y_ref| <= (4 K + 16) u S_i,      u = 2^-24,
    S_i = sum_j (|Re a| + |Im a|)(|Re x| + |Im x|)  +  the absolute values of the other terms of the mode,

K = complex entries stored per row, padding included: a real part is a sum of 2 K products, each product
rounded once and each partial sum once, so at most 2 K roundings touch any term -- (1 + u)^(2K) - 1 is about
2 K u, half the limit, for K u << 1 -- and the epilogue of a mode adds fewer than eight more.  That bound
(`hard_limit`) cannot be missed by a correct kernel but is slack for long rows; the tight criterion measures
what a plain sequential float32 evaluation of the same sum loses, c_ref = max_i err_ref / (u S_i), and allows
the kernel 4 c_ref + 4: the factor for another summation order (4-wide MFMA blocks, split-K partial sums) and
the epilogue.
"""
import numpy as np
import scipy.sparse as sp

U32 = 2.0 ** -24


def c64(a):
    """Round to complex64 (to nearest even, as the device cast does) and widen back: exact complex128 copies
    of what the complex64 kernels read."""
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


def abs1(z):
    z = np.asarray(z)
    return np.abs(z.real) + np.abs(z.imag)


def abs1_matrix(M):
    M = sp.csr_matrix(M)
    return sp.csr_matrix((abs1(M.data), M.indices, M.indptr), shape=M.shape)


def hard_limit(K):
    return 4.0 * K + 16.0


def tight_limit(c_ref):
    return 4.0 * c_ref + 4.0


def mode_reference(AX, S_ax, X, B, mode, w):
    """(y_ref, S) of a mode from AX = op X and S_ax = |op| |X| (rows x columns, complex128 / float64):
    0: op X, 1: B - op X, 3: X + w (B - op X) with w rounded to complex64."""
    if mode == 0:
        return AX, S_ax
    if mode == 1:
        return B - AX, abs1(B) + S_ax
    w = complex(np.complex64(w))
    return X + w * (B - AX), abs1(X) + (abs(w.real) + abs(w.imag)) * (abs1(B) + S_ax)


def error_ratio(Y, Y_ref, S, rows=None):
    """max over the entries (real and imaginary parts separately) of |y - y_ref| / (u S_i); rows: the rows the
    operation writes (default: all).  An entry with S_i = 0 must be exact."""
    Y, Y_ref, S = np.asarray(Y), np.asarray(Y_ref), np.asarray(S)
    if rows is not None:
        Y, Y_ref, S = Y[rows], Y_ref[rows], S[rows]
    d = np.maximum(np.abs(Y.real - Y_ref.real), np.abs(Y.imag - Y_ref.imag))
    zero = S == 0
    if np.any(d[zero] != 0):
        return np.inf
    if zero.all():
        return 0.0
    return float((d[~zero] / (U32 * S[~zero])).max())


# ---------------------------------------------------------------------------------------------------
# block-row operators: (tmap[RT], kcol[RT, KS], vals[RT, KS, 64]), lane = (row & 15) + 16 (col & 3)
# ---------------------------------------------------------------------------------------------------
def packed_matrix(tmap, kcol, vals, n):
    """The n x n sparse matrix of a block-row operator (explicit zeros of the padding dropped)."""
    RT, KS = kcol.shape
    v = np.asarray(vals).reshape(RT, KS, 4, 16)
    rows = (np.asarray(tmap, dtype=np.int64)[:, None, None, None] * 16 + np.arange(16)[None, None, None, :]
            + np.zeros((1, KS, 4, 1), dtype=np.int64))
    cols = (np.asarray(kcol, dtype=np.int64)[:, :, None, None] + np.arange(4)[None, None, :, None]
            + np.zeros((1, 1, 1, 16), dtype=np.int64))
    keep = v != 0
    return sp.csr_matrix((v[keep], (rows[keep], cols[keep])), shape=(n, n))


def pack_dense(M):
    """A dense n x n matrix (n % 16 == 0) in block-row form, every 4-column group of every row tile in order,
    as the engine packs the coarsest inverse."""
    M = np.asarray(M)
    n = M.shape[0]
    RT, KS = n // 16, n // 4
    kcol = np.tile(np.arange(KS, dtype=np.int32) * 4, (RT, 1))
    vals = M.reshape(RT, 16, KS, 4).transpose(0, 2, 3, 1).reshape(RT, KS, 64)
    return np.arange(RT, dtype=np.int32), kcol, np.ascontiguousarray(vals)


def _cfma32(ar, ai, vr, vi, xr, xi):
    """acc += v x in float32, four real products, each product and each sum rounded"""
    ar = ar + vr * xr
    ar = ar - vi * xi
    ai = ai + vr * xi
    ai = ai + vi * xr
    return ar, ai


def _epilogue32(yr, yi, X, B, mode, w):
    """the mode arithmetic of the kernels' epilogues in float32: 1: B - y, 3: X + w (B - y)"""
    if mode == 0:
        return yr, yi
    B = np.asarray(B).astype(np.complex64)
    tr, ti = B.real - yr, B.imag - yi
    if mode == 1:
        return tr, ti
    X = np.asarray(X).astype(np.complex64)
    w = np.complex64(w)
    return _cfma32(X.real.copy(), X.imag.copy(), w.real, w.imag, tr, ti)


def emulate_block_rows(tmap, kcol, vals, X, B=None, mode=0, w=0.0, drop_kstep=None, splitk=False,
                       drop_partial=None):
    """Float32 evaluation of a block-row operator on X[n, nb]: the k-steps of a row tile one after the other,
    the four columns of a k-step one after the other, four real products per complex term (first the two of
    the real part's Re a Re x and the imaginary part's Re a Im x, then -Im a Im x and Im a Re x, as
    k_bsr_mfma_f32 issues its four matrix instructions).  splitk: four partial sums over the k-steps
    q, q + 4, ... added at the end, as k_bsr_mfma_f32_sk.  drop_kstep leaves one k-step out, drop_partial one of
    the four partial sums (the two defects the bounds must reject).  Returns complex128 [n, nb]; rows no tile
    writes are zero."""
    RT, KS = kcol.shape
    X32 = np.asarray(X).astype(np.complex64)
    n, nb = X32.shape
    v = np.asarray(vals).astype(np.complex64).reshape(RT, KS, 4, 16)
    xr, xi = np.ascontiguousarray(X32.real), np.ascontiguousarray(X32.imag)
    nparts = 4 if splitk else 1
    parts = []
    for q in range(nparts):
        re = np.zeros((RT, 16, nb), dtype=np.float32)
        im = np.zeros((RT, 16, nb), dtype=np.float32)
        for ks in range(q, KS, nparts):
            if ks == drop_kstep:
                continue
            cols = kcol[:, ks].astype(np.int64)
            a = v[:, ks]                                       # [RT, 4, 16]
            for c in range(4):
                vr = a[:, c, :, None].real
                re = re + vr * xr[cols + c][:, None, :]
                im = im + vr * xi[cols + c][:, None, :]
            for c in range(4):
                vi = a[:, c, :, None].imag
                re = re + (-vi) * xi[cols + c][:, None, :]
                im = im + vi * xr[cols + c][:, None, :]
        parts.append((re, im))
    re, im = parts[0]
    if splitk and drop_partial == 0:
        re, im = np.zeros_like(re), np.zeros_like(im)
    for q in range(1, nparts):
        if q != drop_partial:
            re = re + parts[q][0]
            im = im + parts[q][1]
    rows = (np.asarray(tmap, dtype=np.int64)[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)
    re, im = re.reshape(RT * 16, nb), im.reshape(RT * 16, nb)
    Xr = None if mode != 3 else np.asarray(X)[rows]
    Br = None if mode == 0 else np.asarray(B)[rows]
    yr, yi = _epilogue32(re, im, Xr, Br, mode, w)
    out = np.zeros((n, nb), dtype=np.complex128)
    out[rows] = yr.astype(np.float64) + 1j * yi.astype(np.float64)
    return out


def emulate_rows(M, X, B=None, mode=0, w=0.0):
    """Float32 evaluation of a sparse operator row by row, the stored entries of a row one after the other in
    column order (the grouped-ELL kernel's order), four real products per complex term."""
    M = sp.csr_matrix(M)
    M.sort_indices()
    X32 = np.asarray(X).astype(np.complex64)
    nb = X32.shape[1]
    nr = M.shape[0]
    cnt = np.diff(M.indptr)
    K = int(cnt.max()) if nr else 0
    cols = np.zeros((nr, K), dtype=np.int64)
    vals = np.zeros((nr, K), dtype=np.complex64)
    pos = np.arange(M.nnz) - np.repeat(M.indptr[:-1], cnt)
    rr = np.repeat(np.arange(nr), cnt)
    cols[rr, pos] = M.indices
    vals[rr, pos] = M.data.astype(np.complex64)
    re = np.zeros((nr, nb), dtype=np.float32)
    im = np.zeros((nr, nb), dtype=np.float32)
    for k in range(K):
        x = X32[cols[:, k]]
        re, im = _cfma32(re, im, vals[:, k, None].real, vals[:, k, None].imag, x.real, x.imag)
    yr, yi = _epilogue32(re, im, X, B, mode, w)
    return yr.astype(np.float64) + 1j * yi.astype(np.float64)


def column_errors(Y, Y_ref):
    """relative l2 error of every column of Y[n, nb]"""
    Y, Y_ref = np.asarray(Y), np.asarray(Y_ref)
    return np.linalg.norm(Y - Y_ref, axis=0) / np.linalg.norm(Y_ref, axis=0)


# ---------------------------------------------------------------------------------------------------
# the lattice level's even-odd kernels: the same expressions in either precision
# ---------------------------------------------------------------------------------------------------
SCHUR_K = 17     # entries of a row of S = D - A_eo A_oe / D on the lattice: its own site's and 8 sites x 2 spins


def schur_apply(Aeo, Aoe, D, X, E, dtype):
    """(S x_e, its scale D |x_e| + |A_eo| (|A_oe| |x_e|) / D) on the rows E of X[n, nb], zero elsewhere; S is applied
    as the kernel applies it, hop after hop: no cancellation between paths enters the scale."""
    real = np.float32 if dtype == np.complex64 else np.float64
    d = real(D)
    di = real(1.0) / d
    xe = np.asarray(X).astype(dtype)[E]
    sx = d * xe - di * (sp.csr_matrix(Aeo).astype(dtype) @ (sp.csr_matrix(Aoe).astype(dtype) @ xe))
    assert sx.dtype == dtype
    out = np.zeros(np.asarray(X).shape, dtype=np.complex128)
    out[E] = sx
    scale = np.zeros(out.shape)
    scale[E] = float(D) * abs1(xe) + (abs1_matrix(Aeo) @ (abs1_matrix(Aoe) @ abs1(xe))) / float(D)
    return out, scale


def eo_smoother(Aeo, Aoe, D, weights, B, X, E, O, reduced, dtype):
    """x_e <- x_e + w_k (b'_e - S x_e), S = D - A_eo A_oe / D, from x_e = X[E]; full form: b'_e = b_e - A_eo b_o / D
    first and x_o = (b_o - A_oe x_e) / D last, reduced form: b'_e = B[E] and the odd rows stay zero.  Evaluated
    in `dtype` (complex128: the reference, complex64: the error level a correct single-precision evaluation
    has); the inverse diagonal is formed once in the dtype's real type and multiplied, as the kernels do."""
    real = np.float32 if dtype == np.complex64 else np.float64
    Aeo = sp.csr_matrix(Aeo).astype(dtype)
    Aoe = sp.csr_matrix(Aoe).astype(dtype)
    d = real(D)
    di = real(1.0) / d
    ws = [dtype(wk) for wk in np.asarray(weights).astype(dtype)]
    B = np.asarray(B).astype(dtype)
    xe = np.asarray(X).astype(dtype)[E]
    bp = B[E] if reduced else B[E] - di * (Aeo @ B[O])
    for wk in ws:
        sx = d * xe - di * (Aeo @ (Aoe @ xe))
        xe = xe + wk * (bp - sx)
    out = np.zeros(B.shape, dtype=dtype)
    out[E] = xe
    if not reduced:
        out[O] = di * (B[O] - Aoe @ xe)
    assert out.dtype == dtype
    return out.astype(np.complex128)
