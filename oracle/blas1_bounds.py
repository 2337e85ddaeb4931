"""Double-double references, NumPy float64 emulations and error limits for the per-kernel tests of the Krylov
solver's BLAS-1 kernels and per-probe scalar updates (tests/test_gpu_krylov_kernels.py on the GPU,
tests/test_blas1_bounds_host.py without one).  The double-double primitives are those of oracle/f64_bounds.py.

Layout here: vectors [n, nb] (row r, probe column c), stacks [K, n, nb], per-probe arrays [rows, nb].

Inner products (k_multidot, k_gram, k_reduce_partials, reduce_and_tail / red_sum_block)
--------------------------------------------------------------------------------------
out[k, c] = sum_r conj(V_k[r, c]) W[r, c].  The reference evaluates it in double-double on the SAME float64
operands (complex64 operands are widened first: exact).  Re = sum (vr wr + vi wi), Im = sum (vr wi - vi wr); with
u = 2^-53 and S = the sum of the absolute values of the 2 n real products that form the component (S_re, S_im):

  hard limit    |err| <= (4 n + 16) u S for each real and imaginary part, whatever the order of the sum: a part is
                a sum of 2 n products; each product is rounded at most once and each partial sum once, so at most
                2 n roundings touch any term, (1 + u)^(2n) - 1 ~ 2 n u: half the limit.
  tight limit   max err / (u S) <= 4 c_ref + 4, c_ref the same figure of emulate_multidot: float64 NumPy (every
                product and sum rounded, no FMA) in the kernel's ORDER of summation -- rows r0 + wave, + 4, ... per
                wave within a row block of rows_per_block rows, the four waves in wave order, then the row blocks:
                in-launch form (red_sum_block) groups of 32 blocks, within a group wave w adds p = w, w + 8, ... and
                p = w + 4, w + 12, ... in two chains, the eight chains combine as (a0 + a1) per wave and
                (w0 + w1) + (w2 + w3), the group sums combine the same way in the order of g; two-stage form
                (k_reduce_partials) wave w adds p = w + 16 i, w + 4 + 16 i, w + 8 + 16 i, w + 12 + 16 i in four
                chains (a ragged tail goes to the first), (s0 + s1) + (s2 + s3), the waves in wave order.
row_blocking / fused_ok are Python twins of the engine's; the GPU test asserts they agree with what the entry
points report.

k_multiaxpy
-----------
Wout[r] = Win[r] + sum_k c_k V_k[r], c_k = sign coef_k (sign = +-1: exact): K + 1 terms per component, so the
same two limits with hard limit 4 (K + 1) + 16 and S = |Win part| + sum of the |real products|.  A complex64 W adds
the half-ulp of the final narrowing, 2^-24 |ref|, to each limit.  The complex64 copy must be float32(Wout) bit for
bit.

The fused norm nrm = sum_r |w_r|^2 is an inner product of the float64 values w_r the kernel holds BEFORE
narrowing, compared with the double-double norm N* of the double-double update w*_r.  Write w_r = w*_r + e_r, each
part of e_r within eps_r = F u S_r (F = the update's limit factor, hard or tight).  Then

    | |w_r|^2 - |w*_r|^2 |  =  | 2 Re(conj(w*_r) e_r) + |e_r|^2 |
                           <=  2 (|Re w*_r| eps_re + |Im w*_r| eps_im) + eps_re^2 + eps_im^2,

and the sum of n positive terms |w_r|^2 is itself formed with the inner-product limit against S = sum |w_r|^2 =
nrm.  So, with G the inner-product factor (4 n + 16, or 4 c_ref + 4 of the emulated norm sum against the
double-double norm of ITS OWN float64 values),

    |nrm - N*|  <=  G u N* (1 + 2^-40)  +  P,    P = sum_r [ 2 F u (|Re w*_r| S_re,r + |Im w*_r| S_im,r)
                                                            + (F u)^2 (S_re,r^2 + S_im,r^2) ]

(norm_limit; the 2^-40 covers nrm versus N* in the first term).  P is the propagated update error.

Gram tail (fg_gram_col)
-----------------------
Three evaluations, each for its own check: the device's own Gram values (bit-level checks of the decisions start
from them); emulate_gram_col, a float64 transcription of fg_gram_col applied to emulated Gram values (c_ref);
gram_reference: the double-double M = W^H W and W^H r0 solved by Cholesky in np.longdouble: y*, the nested
residual norms |r_j|^2 = |r0|^2 - sum_{k<=j} |t_k|^2 and cond_2(M).  Limit on the coefficients:
|y - y*| / |y*| in units of u cond_2(M) <= 4 c_ref + 4.  Decisions (iters, truncation, done, notconv) are compared
exactly; the inputs keep every decision at least 10x from its threshold (decision_margins), so the reference alone
decides it.

Arnoldi / Givens scalars (fg_begin_col, fg_hess_col, fg_verify_col, k_fg_solve)
-------------------------------------------------------------------------------
UnnormalisedArnoldi runs the unnormalised-basis Arnoldi process of fg_hess_col's comment on the host in float64
and produces the raw h1, h2, nrm2 of every step; givens_reference rebuilds h_{k,j} = svec_k svec_j d_k and
h_{j+1,j} = svec_j sqrt(nrm2) in np.longdouble and carries the Givens QR in np.longdouble.  A column costs j
rotations of six multiply-adds per entry plus a new rotation of two square roots and three divisions: well below
64 roundings on any entry for m = 6, so H, cs, sn, g must agree to 64 u relative to the column norm (GIVENS_LIMIT;
the measured figures are in DESIGN.md).  emulate_hess_col is the float64 transcription for the CPU check of that
limit and of the seeded defect.

Seeded defects, and the limit that catches each (tests/test_blas1_bounds_host.py):
  last row of a ragged row block dropped ............ hard (and tight)
  a row block, or a group of 32, dropped ............ hard
  one partial added twice ........................... hard
  accumulator k = K - 1 of a KT > K instantiation ... hard (the value is 0: error = the whole sum)
  conjugate on W instead of V ....................... hard (imaginary part: 2 |Im| against u S)
  coef without svec^2 ............................... the coef check (coef = svec^2 out to 2 u)
  sign ignored in the update ........................ hard
  Gram entry (a, b) read at the index of (b, a) ..... the coefficient limit, and the exact decisions
  Givens rotation with sn not conjugated ............ the 64 u limit on H and g
"""
import numpy as np

from oracle.f32_bounds import hard_limit, tight_limit  # noqa: F401
from oracle.f64_bounds import DD, U64, dd_add, dd_add_prod, two_prod, two_sum  # noqa: F401

WAVES = 4                 # SW_WAVES_PER_BLOCK
RED_GROUP = 32            # SW_RED_GROUP
RED_MAXGROUPS = 64        # SW_RED_MAXGROUPS
TICKET_CHUNKS = 128       # SW_TICKET_CHUNKS
GRAM_MAXL = 4             # SW_GRAM_MAXL
HALF_ULP32 = 2.0 ** -24
GIVENS_LIMIT = 64.0


# ---------------------------------------------------------------------------------------------------
# the engine's launch geometry
# ---------------------------------------------------------------------------------------------------
def pad64(nb):
    return (nb + 63) // 64 * 64


def row_blocking(n, nbp, reduce=True, dot_blocks=1024):
    """(P, rows_per_block) of a batched BLAS-1 launch: the twin of row_blocking in sw_engine.hip (option
    dot_blocks sets both the block budget and its cap, at least 64)."""
    nchunks = nbp // 64
    if reduce:
        d = max(64, int(dot_blocks))
        p = max(8, min(d, d // max(1, nchunks)))
        if nchunks >= 4 and d == 1024:
            p = min(p, 128)
    else:
        p = max(8, 4096 // max(1, nchunks))
    r = max(WAVES, (n + p - 1) // p)
    return (n + r - 1) // r, r


def fused_ok(P, nbp, fused_reduce=True):
    """can the reduction be completed inside the launch?  (the twin of fused_ok)"""
    return bool(fused_reduce) and nbp // 64 <= TICKET_CHUNKS and (P + RED_GROUP - 1) // RED_GROUP <= RED_MAXGROUPS


def gram_index(a, b, NV):
    """the kernel's k of entry (a, b), a <= b"""
    return a * NV - (a * (a - 1)) // 2 + (b - a)


# ---------------------------------------------------------------------------------------------------
# double-double inner products
# ---------------------------------------------------------------------------------------------------
def _dd_sum_axis0(x):
    """double-double sum over axis 0 of the pair x = (hi, lo), pairwise"""
    hi, lo = x
    while hi.shape[0] > 1:
        if hi.shape[0] & 1:
            pad = np.zeros((1,) + hi.shape[1:])
            hi, lo = np.concatenate([hi, pad]), np.concatenate([lo, pad])
        h = hi.shape[0] // 2
        hi, lo = dd_add((hi[:h], lo[:h]), (hi[h:], lo[h:]))
    return hi[0], lo[0]


def dd_dots(V, W, lanes=32):
    """sum_r conj(V_k[r]) W[r] in double-double: a DD of shape [K, nb].  `lanes` rows are accumulated side by
    side (the order of a double-double sum does not matter at 2^-104) to keep the Python loop short."""
    V = np.asarray(V, dtype=np.complex128)
    W = np.asarray(W, dtype=np.complex128)
    K, n, nb = V.shape
    steps = (n + lanes - 1) // lanes
    pad = steps * lanes - n
    if pad:          # zero rows: their products are exact zeros
        V = np.concatenate([V, np.zeros((K, pad, nb), dtype=np.complex128)], axis=1)
        W = np.concatenate([W, np.zeros((pad, nb), dtype=np.complex128)], axis=0)
    vr = np.ascontiguousarray(V.real).reshape(K, steps, lanes, nb)
    vi = np.ascontiguousarray(V.imag).reshape(K, steps, lanes, nb)
    wr = np.ascontiguousarray(W.real).reshape(steps, lanes, nb)
    wi = np.ascontiguousarray(W.imag).reshape(steps, lanes, nb)
    shape = (K, lanes, nb)
    re, im = (np.zeros(shape), np.zeros(shape)), (np.zeros(shape), np.zeros(shape))
    for t in range(steps):
        a, b, c, d = vr[:, t], vi[:, t], wr[t][None], wi[t][None]
        re = dd_add_prod(re, a, c)
        re = dd_add_prod(re, b, d)
        im = dd_add_prod(im, a, d)
        im = dd_add_prod(im, b, c, -1.0)
    re = _dd_sum_axis0((np.moveaxis(re[0], 1, 0), np.moveaxis(re[1], 1, 0)))
    im = _dd_sum_axis0((np.moveaxis(im[0], 1, 0), np.moveaxis(im[1], 1, 0)))
    return DD(re, im)


def dot_scales(V, W):
    """(S_re, S_im)[K, nb]: the sums of the absolute values of the real products of each component"""
    V = np.asarray(V, dtype=np.complex128)
    W = np.asarray(W, dtype=np.complex128)
    ar, ai, br, bi = np.abs(V.real), np.abs(V.imag), np.abs(W.real), np.abs(W.imag)
    s_re = np.einsum("krc,rc->kc", ar, br) + np.einsum("krc,rc->kc", ai, bi)
    s_im = np.einsum("krc,rc->kc", ar, bi) + np.einsum("krc,rc->kc", ai, br)
    return s_re, s_im


def part_ratios(Y, ref, S_re, S_im, extra_re=0.0, extra_im=0.0, u=U64):
    """|err| / (u S) of the real and of the imaginary parts against the DD `ref`, after `extra` (an absolute
    allowance, e.g. the narrowing half-ulp) is taken off; an entry with S = 0 must be exact (inf otherwise), and an
    entry that is not finite counts as inf.  Returns an array shaped like Y with the larger of the two."""
    Y = np.asarray(Y, dtype=np.complex128)
    out = []
    for y, (hi, lo), S, extra in ((Y.real, ref.re, S_re, extra_re), (Y.imag, ref.im, S_im, extra_im)):
        d = np.maximum(np.abs((y - hi) - lo) - extra, 0.0)
        S = np.broadcast_to(np.asarray(S, dtype=np.float64), d.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(S > 0, d / (u * np.where(S > 0, S, 1.0)), np.where(d == 0, 0.0, np.inf))
        out.append(np.where(np.isfinite(y), r, np.inf))
    return np.maximum(out[0], out[1])


def dot_ratio(out, ref, S_re, S_im):
    """max over the K x nb values of err / (u S), parts separately"""
    return float(part_ratios(out, ref, S_re, S_im).max())


# ---------------------------------------------------------------------------------------------------
# float64 emulation of the kernels' order of summation
# ---------------------------------------------------------------------------------------------------
def block_partials(V, W, P, rpb, conj_w=False, drop_row=None):
    """partial[p, k, c] as a row block leaves it: per wave the rows r0 + wave, + 4, ... one after the other (four
    real products per complex term, each product and each sum rounded), then the four waves in wave order.
    conj_w: the conjugate on W instead of V (a defect); drop_row: that row is left out (a defect)."""
    V = np.asarray(V, dtype=np.complex128)
    W = np.asarray(W, dtype=np.complex128)
    K, n, nb = V.shape
    vr, vi = np.ascontiguousarray(V.real), np.ascontiguousarray(V.imag)
    wr, wi = np.ascontiguousarray(W.real), np.ascontiguousarray(W.imag)
    re = np.zeros((K, P, WAVES, nb))
    im = np.zeros((K, P, WAVES, nb))
    base = np.arange(P)[:, None] * rpb + np.arange(WAVES)[None, :]
    sgn = -1.0 if conj_w else 1.0
    for t in range((rpb + WAVES - 1) // WAVES):
        idx = base + WAVES * t
        ok = (np.arange(WAVES)[None, :] + WAVES * t < rpb) & (idx < n)
        if drop_row is not None:
            ok = ok & (idx != drop_row)
        ic = np.where(ok, idx, 0)
        m = ok[None, :, :, None]
        a, b = np.where(m, vr[:, ic], 0.0), np.where(m, vi[:, ic], 0.0)
        c, d = wr[ic][None], wi[ic][None]
        re = (re + a * c) + b * d
        im = (im + sgn * (a * d)) - sgn * (b * c)
    pr = ((re[:, :, 0] + re[:, :, 1]) + re[:, :, 2]) + re[:, :, 3]
    pi = ((im[:, :, 0] + im[:, :, 1]) + im[:, :, 2]) + im[:, :, 3]
    return np.moveaxis(pr + 1j * pi, 1, 0)          # [P, K, nb]


def _chain(x, idx):
    s = np.zeros(x.shape[1:], dtype=x.dtype)
    for i in idx:
        s = s + x[i]
    return s


def red_sum_block(x):
    """the sum over axis 0 as red_sum_block forms it"""
    cnt = x.shape[0]
    w = []
    for wave in range(WAVES):
        a0 = _chain(x, range(wave, cnt, 8))
        a1 = _chain(x, range(wave + 4, cnt, 8))
        w.append(a0 + a1)
    return (w[0] + w[1]) + (w[2] + w[3])


def reduce_partials(x):
    """the sum over axis 0 as k_reduce_partials forms it"""
    P = x.shape[0]
    w = []
    for wave in range(WAVES):
        p = wave
        s = [[], [], [], []]
        while p + 12 < P:
            for q in range(4):
                s[q].append(p + 4 * q)
            p += 16
        s[0].extend(range(p, P, 4))
        c = [_chain(x, i) for i in s]
        w.append((c[0] + c[1]) + (c[2] + c[3]))
    return ((w[0] + w[1]) + w[2]) + w[3]


def combine_partials(partial, fused, drop_group=None):
    """the cross-block sum: in-launch (groups of 32 in the order of p, then the group sums in the order of g) or
    two-stage; drop_group: that group's sum is left out (a defect)"""
    P = partial.shape[0]
    if not fused:
        return reduce_partials(partial)
    ngroups = (P + RED_GROUP - 1) // RED_GROUP
    if ngroups == 1:
        return red_sum_block(partial)
    gp = [red_sum_block(partial[g * RED_GROUP:min(P, (g + 1) * RED_GROUP)]) for g in range(ngroups)
          if g != drop_group]
    return red_sum_block(np.stack(gp))


def emulate_multidot(V, W, P, rpb, fused=True, svec=None, defect=None):
    """(out[K, nb], coef[K, nb] or None) in float64 in the kernel's order.  defect = (name, argument):
      ("drop_row", r)  ("drop_block", p)  ("drop_group", g)  ("dup_partial", p)  ("drop_last_acc", None)
      ("conj_w", None)  ("coef_no_svec", None)"""
    name, arg = defect if defect else (None, None)
    part = block_partials(V, W, P, rpb, conj_w=name == "conj_w", drop_row=arg if name == "drop_row" else None)
    if name == "drop_block":
        part = np.delete(part, arg, axis=0)
    if name == "dup_partial":
        part = np.insert(part, arg, part[arg], axis=0)
    out = combine_partials(part, fused, drop_group=arg if name == "drop_group" else None)
    if name == "drop_last_acc":
        out = out.copy()
        out[-1] = 0.0
    coef = None
    if svec is not None:
        q = np.asarray(svec, dtype=np.float64)
        q2 = np.ones_like(q) if name == "coef_no_svec" else q * q
        coef = (q2 * out.real) + 1j * (q2 * out.imag)
    return out, coef


def emulate_gram(U, P, rpb):
    """the NV (NV + 1) / 2 values of k_gram (always completed in the launch) at the kernel's indices"""
    U = np.asarray(U, dtype=np.complex128)
    NV = U.shape[0]
    out = np.zeros((NV * (NV + 1) // 2, U.shape[2]), dtype=np.complex128)
    for b in range(NV):
        col, _ = emulate_multidot(U[:b + 1], U[b], P, rpb, True)
        for a in range(b + 1):
            out[gram_index(a, b, NV)] = col[a]
    return out


def dd_gram(U):
    """(DD [K, nb], S_re, S_im) of all pairs a <= b at the kernel's indices"""
    U = np.asarray(U, dtype=np.complex128)
    NV, _, nb = U.shape
    K = NV * (NV + 1) // 2
    parts = [[np.zeros((K, nb)) for _ in range(2)] for _ in range(2)]
    S = [np.zeros((K, nb)), np.zeros((K, nb))]
    for b in range(NV):
        ref = dd_dots(U[:b + 1], U[b])
        s = dot_scales(U[:b + 1], U[b])
        for a in range(b + 1):
            k = gram_index(a, b, NV)
            for q in (0, 1):
                parts[0][q][k] = ref.re[q][a]
                parts[1][q][k] = ref.im[q][a]
                S[q][k] = s[q][a]
    return DD(tuple(parts[0]), tuple(parts[1])), S[0], S[1]


# ---------------------------------------------------------------------------------------------------
# k_multiaxpy
# ---------------------------------------------------------------------------------------------------
def dd_axpy(V, coef, sign, Win):
    """(DD [n, nb], S_re, S_im) of Win + sum_k (sign coef_k) V_k; S = |Win part| + the |real products|"""
    V = np.asarray(V, dtype=np.complex128)
    Win = np.asarray(Win, dtype=np.complex128)
    c = float(sign) * np.asarray(coef, dtype=np.complex128)
    re = (np.ascontiguousarray(Win.real), np.zeros(Win.shape))
    im = (np.ascontiguousarray(Win.imag), np.zeros(Win.shape))
    s_re, s_im = np.abs(Win.real), np.abs(Win.imag)
    for k in range(V.shape[0]):
        cr, ci = c[k].real[None, :], c[k].imag[None, :]
        vr, vi = np.ascontiguousarray(V[k].real), np.ascontiguousarray(V[k].imag)
        re = dd_add_prod(re, cr, vr)
        re = dd_add_prod(re, ci, vi, -1.0)
        im = dd_add_prod(im, cr, vi)
        im = dd_add_prod(im, ci, vr)
        s_re = s_re + np.abs(cr * vr) + np.abs(ci * vi)
        s_im = s_im + np.abs(cr * vi) + np.abs(ci * vr)
    return DD(re, im), s_re, s_im


def emulate_multiaxpy(V, coef, sign, Win, w_c64=False, ignore_sign=False):
    """(Wout as stored, the float64 values before narrowing) in float64, the K terms one after the other;
    ignore_sign: sign taken as + 1 (a defect)"""
    V = np.asarray(V, dtype=np.complex128)
    Win = np.asarray(Win, dtype=np.complex128)
    c = (1.0 if ignore_sign else float(sign)) * np.asarray(coef, dtype=np.complex128)
    re, im = Win.real.copy(), Win.imag.copy()
    for k in range(V.shape[0]):
        cr, ci = c[k].real[None, :], c[k].imag[None, :]
        re = (re + cr * V[k].real) - ci * V[k].imag
        im = (im + cr * V[k].imag) + ci * V[k].real
    w = re + 1j * im
    return (w.astype(np.complex64).astype(np.complex128) if w_c64 else w), w


def axpy_ratio(Wout, ref, S_re, S_im, w_c64=False):
    """max err / (u S) of the update; complex64 W: after the half-ulp of the narrowing, 2^-24 |ref part|"""
    ex_re = HALF_ULP32 * np.abs(ref.re[0]) if w_c64 else 0.0
    ex_im = HALF_ULP32 * np.abs(ref.im[0]) if w_c64 else 0.0
    return float(part_ratios(Wout, ref, S_re, S_im, ex_re, ex_im).max())


def dd_norms(ref):
    """N*[nb] = sum_r |w*_r|^2 of a DD vector block [n, nb], in double-double on its high and low parts: (hi, lo).
    |w*|^2 = hi^2 + 2 hi lo + lo^2; the last term is below 2^-208 of the first and is dropped."""
    acc = (np.zeros(ref.re[0].shape), np.zeros(ref.re[0].shape))
    for hi, lo in (ref.re, ref.im):
        acc = dd_add_prod(acc, hi, hi)
        acc = dd_add_prod(acc, 2.0 * hi, lo)
    return _dd_sum_axis0(acc)


def norm_limit(F, G, ref, S_re, S_im, u=U64):
    """the limit on |nrm - N*| per column (module docstring): G u N* + the propagated update error at factor F"""
    N = dd_norms(ref)[0]
    e = F * u
    prop = (2.0 * e * (np.abs(ref.re[0]) * S_re + np.abs(ref.im[0]) * S_im) + e * e * (S_re ** 2 + S_im ** 2)).sum(axis=0)
    return G * u * N * (1.0 + 2.0 ** -40) + prop


def norm_ratio(nrm, F, G, ref, S_re, S_im):
    """max over the columns of |nrm - N*| / norm_limit: at most 1 inside the limit"""
    hi, lo = dd_norms(ref)
    nrm = np.asarray(nrm, dtype=np.float64)
    d = np.abs((nrm - hi) - lo)
    lim = norm_limit(F, G, ref, S_re, S_im)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(lim > 0, d / np.where(lim > 0, lim, 1.0), np.where(d == 0, 0.0, np.inf))
    return float(np.where(np.isfinite(nrm), r, np.inf).max())


def emulate_norm(w, P, rpb, fused=True):
    """sum_r |w_r|^2 in float64 in the kernel's order (the real part of the emulated inner product of w with itself)"""
    out, _ = emulate_multidot(np.asarray(w)[None], w, P, rpb, fused)
    return out[0].real


def norm_sum_cref(w, P, rpb, fused=True):
    """c_ref of the norm's own sum: the emulated sum against the double-double norm of the SAME float64 values"""
    w = np.asarray(w, dtype=np.complex128)
    z = np.zeros(w.shape)
    hi, lo = dd_norms(DD((np.ascontiguousarray(w.real), z), (np.ascontiguousarray(w.imag), z)))
    e = emulate_norm(w, P, rpb, fused)
    return float((np.abs((e - hi) - lo) / (U64 * hi)).max())


# ---------------------------------------------------------------------------------------------------
# Gram tail
# ---------------------------------------------------------------------------------------------------
def emulate_gram_col(d, L, normb, iters, tol, tol_stop, iter_base, init, swap=None):
    """fg_gram_col for ONE probe in float64 (Python floats: every operation rounded, no FMA).  d: the K Gram values
    of the probe; swap = (a, b): entry (a, b) is read at the index the kernel's formula gives for (b, a) (a defect).
    Returns dict(ys[L], relres, g, normb, iters, notconv (0 or 1), Leff, done)."""
    NV = L + 1
    K = NV * (NV + 1) // 2

    def G(a, b):
        if swap == (a, b):
            a, b = b, a
        return complex(d[(a * NV - (a * (a - 1)) // 2 + (b - a)) % K])
    g00 = max(G(0, 0).real, 0.0)
    iters = int(iters)
    if init:
        normb = float(np.sqrt(g00))
        iters = -1 if g00 > 0.0 else 0
    nb_ = float(normb)
    rr0 = float(np.sqrt(g00)) / nb_ if nb_ > 0.0 else 0.0
    C = [[0j] * GRAM_MAXL for _ in range(GRAM_MAXL)]
    t = [0j] * GRAM_MAXL
    res2, Leff = g00, 0
    done = (not nb_ > 0.0) or (iters >= 0 and rr0 < 1.0e-2 * tol_stop) or g00 == 0.0
    rr = rr0
    if not done:
        for j in range(L):
            dj = G(j + 1, j + 1).real
            mjj = dj
            for k in range(j):
                v = G(k + 1, j + 1).conjugate()
                vx, vy = v.real, v.imag
                for i in range(k):
                    a_, b_ = C[j][i], C[k][i]
                    vx = vx - (a_.real * b_.real + a_.imag * b_.imag)
                    vy = vy - (a_.imag * b_.real - a_.real * b_.imag)
                ckk = C[k][k].real
                C[j][k] = complex(vx / ckk, vy / ckk)
                dj -= C[j][k].real * C[j][k].real + C[j][k].imag * C[j][k].imag
            if not dj > 1.0e-13 * mjj or not mjj > 0.0:
                break
            cjj = float(np.sqrt(dj))
            C[j][j] = complex(cjj, 0.0)
            tj = G(0, j + 1).conjugate()
            tx, ty = tj.real, tj.imag
            for k in range(j):
                a_, b_ = C[j][k], t[k]
                tx = tx - (a_.real * b_.real - a_.imag * b_.imag)
                ty = ty - (a_.real * b_.imag + a_.imag * b_.real)
            t[j] = complex(tx / cjj, ty / cjj)
            res2 -= t[j].real * t[j].real + t[j].imag * t[j].imag
            Leff = j + 1
            rr = float(np.sqrt(max(res2, 0.0))) / nb_
            if iters < 0 and rr < tol:
                iters = iter_base + j + 1
    y = [0j] * GRAM_MAXL
    for j in range(GRAM_MAXL - 1, -1, -1):
        if j >= Leff:
            continue
        vx, vy = t[j].real, t[j].imag
        for k in range(GRAM_MAXL - 1, 0, -1):
            if k <= j or k >= Leff:
                continue
            a_, b_ = C[k][j], y[k]
            vx = vx - (a_.real * b_.real + a_.imag * b_.imag)
            vy = vy - (a_.real * b_.imag - a_.imag * b_.real)
        cjj = C[j][j].real
        y[j] = complex(vx / cjj, vy / cjj)
    return dict(ys=np.array(y[:L]), relres=rr, g=rr0, normb=nb_, iters=iters,
                notconv=int((not done) and not (rr < tol_stop)), Leff=Leff, done=done)


def gram_reference(U, dd=None):
    """Per probe column, from the double-double Gram values of U = [r0, w_0 .. w_{L-1}] ([NV, n, nb]): the Cholesky
    solution of (W^H W) y = W^H r0 in np.longdouble.  Returns dict(y[L, nb] (complex128), res2[L + 1, nb]: |r0|^2
    and the nested |r_j|^2, cond[nb] = cond_2(M) over the directions that entered, pivot[L, nb]: the Cholesky pivots d_j / M_jj (what the
    truncation test looks at), M[nb, L, L], rhs[nb, L]).  dd: the double-double Gram values of U when the caller
    has them already."""
    ref = dd_gram(U)[0] if dd is None else dd
    NV, _, nb = np.asarray(U).shape
    L = NV - 1
    ld, cld = np.longdouble, np.clongdouble

    def G(a, b, c):
        k = gram_index(a, b, NV)
        return cld(ld(ref.re[0][k, c]) + ld(ref.re[1][k, c])) + cld(1j) * (ld(ref.im[0][k, c]) + ld(ref.im[1][k, c]))
    y = np.zeros((L, nb), dtype=np.complex128)
    res2 = np.zeros((L + 1, nb))
    cond = np.zeros(nb)
    pivot = np.zeros((L, nb))
    Ms = np.zeros((nb, L, L), dtype=np.complex128)
    rhs = np.zeros((nb, L), dtype=np.complex128)
    for c in range(nb):
        M = np.zeros((L, L), dtype=cld)
        b = np.zeros(L, dtype=cld)
        for i in range(L):
            b[i] = np.conj(G(0, i + 1, c))
            for j in range(i, L):
                M[i, j] = G(i + 1, j + 1, c)
                M[j, i] = np.conj(M[i, j])
        Ms[c], rhs[c] = M.astype(np.complex128), b.astype(np.complex128)
        g00 = G(0, 0, c).real
        res2[0, c] = float(g00)
        if not g00 > 0:
            continue
        Cf = np.zeros((L, L), dtype=cld)
        t = np.zeros(L, dtype=cld)
        r2, Leff = g00, 0
        for j in range(L):
            dj = M[j, j].real
            for k in range(j):
                v = M[j, k] - sum((Cf[j, i] * np.conj(Cf[k, i]) for i in range(k)), cld(0))
                Cf[j, k] = v / Cf[k, k]
                dj = dj - abs(Cf[j, k]) ** 2
            pivot[j, c] = float(dj / M[j, j].real) if M[j, j].real > 0 else 0.0
            if not dj > ld(1.0e-13) * M[j, j].real:
                break
            Cf[j, j] = np.sqrt(dj)
            t[j] = (b[j] - sum((Cf[j, k] * t[k] for k in range(j)), cld(0))) / Cf[j, j]
            r2 = r2 - abs(t[j]) ** 2
            res2[j + 1, c] = float(r2)
            Leff = j + 1
        res2[Leff + 1:, c] = res2[Leff, c]
        cond[c] = np.linalg.cond(Ms[c][:Leff, :Leff]) if Leff else 1.0      # (of the directions that entered)
        yy = np.zeros(L, dtype=cld)
        for j in range(Leff - 1, -1, -1):
            v = t[j] - sum((np.conj(Cf[k, j]) * yy[k] for k in range(j + 1, Leff)), cld(0))
            yy[j] = v / Cf[j, j]
        y[:, c] = yy.astype(np.complex128)
    return dict(y=y, res2=res2, cond=cond, pivot=pivot, M=Ms, rhs=rhs)


def coef_ratio(ys, gref, cols=None):
    """max over the probe columns of |y - y*| / |y*| in units of u cond_2(M) (columns with y* = 0 must give 0)"""
    worst = 0.0
    nb = gref["y"].shape[1]
    for c in (range(nb) if cols is None else cols):
        yr = gref["y"][:, c]
        d = np.linalg.norm(np.asarray(ys)[:, c] - yr)
        nr = np.linalg.norm(yr)
        if nr == 0.0:
            r = 0.0 if d == 0.0 else np.inf
        else:
            r = d / nr / (U64 * gref["cond"][c])
        worst = max(worst, r if np.isfinite(r) else np.inf)
    return float(worst)


def decision_margins(gref, normb, tol, tol_stop, entry_iters):
    """The smallest factor by which any decision of fg_gram_col stays away from its threshold, per column, from the
    longdouble reference: every nested relres against tol (and the final one against tol_stop), rr0 against
    1e-2 tol_stop for a probe that enters with iters >= 0, every Cholesky pivot against 1e-13.  A test's inputs
    must keep this at 10 or more."""
    res2, pivot = gref["res2"], gref["pivot"]
    L, nb = pivot.shape
    out = np.full(nb, np.inf)

    def away(x, thr):
        if thr <= 0.0 or x <= 0.0:
            return np.inf
        return max(x / thr, thr / x)
    for c in range(nb):
        nbc = float(np.asarray(normb)[c])
        if not nbc > 0.0 or not res2[0, c] > 0.0:
            continue
        rr0 = np.sqrt(res2[0, c]) / nbc
        m = np.inf
        if np.asarray(entry_iters)[c] >= 0:
            m = min(m, away(rr0, 1.0e-2 * tol_stop))
            if rr0 < 1.0e-2 * tol_stop:
                out[c] = m
                continue
        for j in range(L):
            m = min(m, away(pivot[j, c], 1.0e-13))
            if not pivot[j, c] > 1.0e-13:
                break
            rr = np.sqrt(max(res2[j + 1, c], 0.0)) / nbc
            m = min(m, away(rr, tol))
        m = min(m, away(np.sqrt(max(res2[L, c], 0.0)) / nbc, tol_stop))
        out[c] = m
    return out


def expected_decisions(gref, normb, entry_iters, tol, tol_stop, iter_base, init):
    """(iters[nb], Leff[nb], done[nb], notconv) as the longdouble reference decides them"""
    res2, pivot = gref["res2"], gref["pivot"]
    L, nb = pivot.shape
    iters = np.array(entry_iters, dtype=np.int64).copy()
    Leff = np.zeros(nb, dtype=np.int64)
    done = np.zeros(nb, dtype=bool)
    notconv = 0
    for c in range(nb):
        g00 = res2[0, c]
        nbc = np.sqrt(g00) if init else float(np.asarray(normb)[c])
        if init:
            iters[c] = -1 if g00 > 0 else 0
        rr0 = np.sqrt(g00) / nbc if nbc > 0 else 0.0
        done[c] = (not nbc > 0) or (iters[c] >= 0 and rr0 < 1.0e-2 * tol_stop) or g00 == 0
        rr = rr0
        if not done[c]:
            for j in range(L):
                if not pivot[j, c] > 1.0e-13:
                    break
                Leff[c] = j + 1
                rr = np.sqrt(max(res2[j + 1, c], 0.0)) / nbc
                if iters[c] < 0 and rr < tol:
                    iters[c] = iter_base + j + 1
            if not rr < tol_stop:
                notconv += 1
    return iters, Leff, done, notconv


# ---------------------------------------------------------------------------------------------------
# Arnoldi / Givens scalars
# ---------------------------------------------------------------------------------------------------
def new_state(m, nb):
    """a zero FGMRES state for restart length m: the arrays of Engine.krylov_scalars"""
    z = np.zeros
    return dict(H=z((m + 1, m, nb), dtype=np.complex128), cs=z((m, nb), dtype=np.complex128),
                sn=z((m, nb), dtype=np.complex128), g=z((m + 1, nb), dtype=np.complex128),
                y=z((m, nb), dtype=np.complex128), normb=z(nb, dtype=np.complex128),
                relres=z(nb, dtype=np.complex128), svec=z((m + 1, nb), dtype=np.complex128),
                ys=z((m, nb), dtype=np.complex128), iters=np.full(nb, -1, dtype=np.int32))


def emulate_begin(state, nrm, first_cycle):
    s = {k: np.array(v) for k, v in state.items()}
    beta = np.sqrt(np.maximum(np.asarray(nrm, dtype=np.float64), 0.0))
    pos = beta > 0
    if first_cycle:
        s["normb"] = beta.astype(np.complex128)
        s["iters"] = np.where(pos, -1, 0).astype(np.int32)
        s["relres"] = np.where(pos, 1.0, 0.0).astype(np.complex128)
    s["g"][0] = beta
    s["svec"][0] = np.where(pos, 1.0 / np.where(pos, beta, 1.0), 0.0)
    return s


def emulate_hess_col(state, j, h1, h2, nrm2, tol, tol_stop, iter_base, pyth, sn_not_conj=False):
    """fg_hess_col in float64 for every probe column (Python complex per column: every operation rounded, no FMA).
    sn_not_conj: the rotation applied as [c sn; -sn c] (a defect).  Returns (new state, notconv)."""
    s = {k: np.array(v) for k, v in state.items()}
    m, nb = s["cs"].shape
    notconv = 0
    for c in range(nb):
        sv = s["svec"][:, c].real
        sj = float(sv[j])

        def raw(k):
            return complex(h1[k, c] + h2[k, c]) if h2 is not None else complex(h1[k, c])
        s0 = float(sv[0]) * sj
        hk = complex(s0 * raw(0).real, s0 * raw(0).imag)
        hcol2 = hk.real * hk.real + hk.imag * hk.imag
        for k in range(j):
            sk1 = float(sv[k + 1]) * sj
            hk1 = complex(sk1 * raw(k + 1).real, sk1 * raw(k + 1).imag)
            hcol2 = hk1.real * hk1.real + (hk1.imag * hk1.imag + hcol2)
            cc = float(s["cs"][k, c].real)
            sn = complex(s["sn"][k, c])
            t = cc * hk + sn * hk1
            u = cc * hk1 + (-sn if sn_not_conj else -sn.conjugate()) * hk
            s["H"][k, j, c] = t
            hk = u
        if pyth:
            tot = sj * sj * max(float(np.real(h1[j + 1, c])), 0.0)
            h2v = tot - hcol2
            if not h2v > 1.0e-12 * tot:
                h2v = 0.0
            hn = float(np.sqrt(h2v))
            wn = hn / sj if sj > 0.0 else 0.0
        else:
            wn = float(np.sqrt(max(float(nrm2[c]), 0.0)))
            hn = sj * wn
        habs = float(np.sqrt(hk.real * hk.real + hk.imag * hk.imag))
        dnm = float(np.sqrt(habs * habs + hn * hn))
        if dnm == 0.0:
            cc, sn = 1.0, 0j
        elif habs == 0.0:
            cc, sn = 0.0, 1.0 + 0j
        else:
            cc = habs / dnm
            f = hn / (habs * dnm)
            sn = complex(hk.real * f, hk.imag * f)
        s["cs"][j, c] = cc
        s["sn"][j, c] = sn
        s["H"][j, j, c] = cc * hk + sn * hn
        gj = complex(s["g"][j, c])
        gn = (-sn if sn_not_conj else -sn.conjugate()) * gj
        s["g"][j + 1, c] = gn
        s["g"][j, c] = cc * gj
        nb_ = float(s["normb"][c].real)
        rr = abs(gn) / nb_ if nb_ > 0.0 else 0.0
        dead = hn == 0.0 and hcol2 == 0.0
        if not dead:
            s["relres"][c] = rr
        if s["iters"][c] < 0 and rr < tol:
            s["iters"][c] = iter_base + j + 1
        if not dead and not rr < tol_stop:
            notconv += 1
        frozen = (s["iters"][c] >= 0 and rr < 1.0e-2 * tol_stop) or (hn * hn <= 1.0e-28 * (hcol2 + hn * hn))
        s["svec"][j + 1, c] = 1.0 / wn if (hn > 0.0 and not frozen) else 0.0
    return s, notconv


def emulate_solve(state, k):
    """k_fg_solve in float64"""
    s = {key: np.array(v) for key, v in state.items()}
    for c in range(s["cs"].shape[1]):
        for i in range(k - 1, -1, -1):
            t = complex(s["g"][i, c])
            for l in range(i + 1, k):
                t = t - complex(s["H"][i, l, c]) * complex(s["y"][l, c])
            hii = complex(s["H"][i, i, c])
            dd = hii.real * hii.real + hii.imag * hii.imag
            yi = 0j
            if dd > 0.0:
                yi = complex((t.real * hii.real + t.imag * hii.imag) / dd, (t.imag * hii.real - t.real * hii.imag) / dd)
            s["y"][i, c] = yi
            si = float(s["svec"][i, c].real)
            s["ys"][i, c] = complex(si * yi.real, si * yi.imag)
    return s


class UnnormalisedArnoldi:
    """The host half of one restart cycle of GMRES(m) on a dense A[n, n] with right-hand sides B[n, nb], zero guess,
    no preconditioner, in the unnormalised-basis formulation of fg_hess_col: vtilde_0 = b, vtilde_{j+1} = the
    orthogonalised A vtilde_j as it is, the scales svec come back from the scalar update under test.  step(j, svec)
    returns the float64 inputs of the Hessenberg update of column j."""

    def __init__(self, A, B, m, passes=1):
        self.A = np.asarray(A, dtype=np.complex128)
        self.m, self.passes = m, passes
        self.vt = [np.asarray(B, dtype=np.complex128).copy()]
        self.wn2 = []          # |A vtilde_j|^2 before the orthogonalisation

    def begin(self):
        """nrm[nb] = |b|^2"""
        return np.einsum("rc,rc->c", self.vt[0].conj(), self.vt[0]).real

    def step(self, j, svec, pyth=False):
        """(h1[m + 2, nb], h2 or None, nrm2[nb]); svec[m + 1, nb]: the scales the state holds.  pyth: the last-step
        form -- |w|^2 before the orthogonalisation in row j + 1 of h1, nrm2 is still the explicit |vtilde_{j+1}|^2
        of the orthogonalised vector (for comparison; the update does not read it)."""
        nb = self.vt[0].shape[1]
        V = np.stack(self.vt[:j + 1])
        w = self.A @ self.vt[j]
        q2 = np.asarray(svec)[:j + 1].real ** 2
        h1 = np.zeros((self.m + 2, nb), dtype=np.complex128)
        h1[:j + 1] = np.einsum("krc,rc->kc", V.conj(), w)
        if pyth:
            h1[j + 1] = np.einsum("rc,rc->c", w.conj(), w).real
        w = w - np.einsum("kc,krc->rc", q2 * h1[:j + 1], V)
        h2 = None
        if self.passes == 2:
            h2 = np.zeros_like(h1)
            h2[:j + 1] = np.einsum("krc,rc->kc", V.conj(), w)
            w = w - np.einsum("kc,krc->rc", q2 * h2[:j + 1], V)
        nrm2 = np.einsum("rc,rc->c", w.conj(), w).real
        if len(self.vt) == j + 1:
            self.vt.append(w)
        return h1, h2, nrm2


def givens_reference(svec, raws, m):
    """np.longdouble Givens QR of the Hessenberg columns rebuilt from the raw inputs.  svec[m + 1, nb]: the scales
    (float64 values, as the state holds them after the cycle); raws[j] = (d[j + 1, nb] = h1 + h2 rows, hn2[nb] =
    the squared norm nrm2 that closes the column).  Returns dict(Hraw[m + 1, m, nb] complex128: the unrotated
    Hessenberg matrix, R, cs, sn, g (np.clongdouble / longdouble, g for beta = 1: the right-hand side after the
    last column), gsteps[m, 2, nb]: (g_j, g_{j+1}) as column j leaves them -- |g_{j+1}| is the residual after column j
    --, colnorm[m, nb])."""
    ld, cld = np.longdouble, np.clongdouble
    ncol = len(raws)
    nb = np.asarray(svec).shape[1]
    sv = np.asarray(svec).real.astype(ld)
    Hraw = np.zeros((m + 1, m, nb), dtype=cld)
    R = np.zeros((m + 1, m, nb), dtype=cld)
    cs = np.zeros((m, nb), dtype=ld)
    sn = np.zeros((m, nb), dtype=cld)
    g = np.zeros((m + 1, nb), dtype=cld)
    g[0] = 1
    gsteps = np.zeros((m, 2, nb), dtype=cld)
    for j in range(ncol):
        d, hn2 = raws[j]
        col = np.zeros((j + 2, nb), dtype=cld)
        for k in range(j + 1):
            col[k] = (sv[k] * sv[j]) * np.asarray(d[k]).astype(cld)
        col[j + 1] = sv[j] * np.sqrt(np.maximum(np.asarray(hn2).astype(ld), 0))
        Hraw[:j + 2, j] = col
        hk = col[0]
        for k in range(j):
            t = cs[k] * hk + sn[k] * col[k + 1]
            hk = cs[k] * col[k + 1] - np.conj(sn[k]) * hk
            R[k, j] = t
        hn = col[j + 1].real
        habs = np.abs(hk)
        dnm = np.sqrt(habs * habs + hn * hn)
        ok = (dnm > 0) & (habs > 0)
        safe_d = np.where(dnm > 0, dnm, 1)
        safe_a = np.where(habs > 0, habs, 1)
        cs[j] = np.where(dnm == 0, 1, np.where(habs == 0, 0, habs / safe_d))
        sn[j] = np.where(ok, hk * (hn / (safe_a * safe_d)), np.where(dnm == 0, 0, 1))
        R[j, j] = cs[j] * hk + sn[j] * hn
        g[j + 1] = -np.conj(sn[j]) * g[j]
        g[j] = cs[j] * g[j]
        gsteps[j, 0], gsteps[j, 1] = g[j], g[j + 1]
    colnorm = np.sqrt((np.abs(Hraw) ** 2).sum(axis=0)).astype(np.float64)
    return dict(Hraw=Hraw.astype(np.complex128), R=R, cs=cs, sn=sn, g=g, gsteps=gsteps, colnorm=colnorm)


def givens_ratios(state, gref, j, beta):
    """err / u of column j of a state against givens_reference: (H column relative to the column norm, cs and sn
    (absolute: they are of unit size), g_j and g_{j+1} relative to beta), the largest over the probe columns whose
    column is not zero"""
    cn = gref["colnorm"][j]
    live = cn > 0
    if not live.any():
        return 0.0, 0.0, 0.0
    safe = np.where(live, cn, 1.0)
    dH = np.abs(np.asarray(state["H"])[:j + 1, j].astype(np.clongdouble) - gref["R"][:j + 1, j]).max(axis=0)
    rH = float((dH / safe)[live].max() / U64)
    dc = np.abs(np.asarray(state["cs"])[j].real - gref["cs"][j])
    ds = np.abs(np.asarray(state["sn"])[j].astype(np.clongdouble) - gref["sn"][j])
    rc = float(np.maximum(dc, ds)[live].max() / U64)
    b = np.asarray(beta, dtype=np.float64)
    dg = np.abs(np.asarray(state["g"])[j:j + 2].astype(np.clongdouble) - gref["gsteps"][j] * b).max(axis=0)
    rg = float((dg / np.where(b > 0, b, 1.0))[live & (b > 0)].max() / U64) if (live & (b > 0)).any() else 0.0
    return rH, rc, rg


# ---------------------------------------------------------------------------------------------------
# inputs shared by the host and the GPU tests
# ---------------------------------------------------------------------------------------------------
def c64(a):
    """rounded to complex64 and widened back: what a complex64 kernel reads"""
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


def rand_block(shape, seed):
    """standard normal complex [..., n, nb]; column 1 is scaled by 1e-3 and column 2 by 1e3 (nb >= 3), so that
    only a limit expressed per column holds"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    if shape[-1] >= 3:
        a[..., 1] *= 1.0e-3
        a[..., 2] *= 1.0e3
    return a


# the probe columns of gram_inputs with a decision of their own (nb >= 7)
COL_ZERO_RHS, COL_CONVERGED, COL_PASSES_AT_2, COL_DUPLICATE = 3, 4, 5, 6
GRAM_TOL = 2.0e-2          # every nested residual of gram_inputs is at least 10x away from it (decision_margins)
GRAM_LEFTOVER = 2.0e-5     # what the two-direction problem of COL_PASSES_AT_2 leaves of r0


def gram_inputs(n, nb, seed, production=False, eps=0.2):
    """(U[5, n, nb] = [r0, w_0 .. w_3], Z[4, n, nb], X[n, nb]) of a Gram cycle of up to four directions; a cycle of
    L directions takes U[:L + 1], Z[:L].
      random      independent random directions: cond_2(W^H W) < 1e3
      production  w_j = (I - E)^(j+1) r0 with E = diag(e_r), 0 <= e_r <= eps: the nearly collinear basis of a
                  preconditioned cycle (S M ~ I - E, mean of E 0.1: cond_2 ~ 1e6 at L = 3); z_0 = r0, z_{j+1} = w_j
    Columns 1, 2 carry the scales 1e-3, 1e3.  random only, nb >= 7: column 3 has no right-hand side, column 4 is an
    ordinary column that the caller enters as already converged (through normb and iters), column 5 is
    r0 = w_0 + w_1 + GRAM_LEFTOVER q: its nested residual passes GRAM_TOL with the second direction, column 6 has
    w_2 a bit-identical copy of w_1."""
    U = rand_block((5, n, nb), seed)
    Z = rand_block((4, n, nb), seed + 1)
    X = rand_block((n, nb), seed + 2)
    if production:
        rng = np.random.default_rng(seed + 3)
        e = eps * rng.random((n, 1))
        for j in range(4):
            U[j + 1] = (1.0 - e) * U[j]
            Z[j] = U[j]
        return U, Z, X
    if nb >= 7:
        U[0, :, COL_ZERO_RHS] = 0.0
        q = np.random.default_rng(seed + 4).standard_normal(n)
        U[0, :, COL_PASSES_AT_2] = U[1, :, COL_PASSES_AT_2] + U[2, :, COL_PASSES_AT_2] + GRAM_LEFTOVER * q
        U[3, :, COL_DUPLICATE] = U[2, :, COL_DUPLICATE]
    return U, Z, X


def gram_entry_state(U, tol_stop, init):
    """(normb[nb], iters[nb]) a Gram cycle over gram_inputs is entered with: |r0| and -1 (init: placeholders the
    cycle overwrites), column 4 as already converged at 5e-4 tol_stop (20x below the 1e-2 tol_stop at which a probe
    takes no further part) with a recorded iteration"""
    nb = U.shape[2]
    r0n = np.sqrt(np.einsum("rc,rc->c", U[0].conj(), U[0]).real)
    if init:
        return np.full(nb, 7.0), np.full(nb, 3, dtype=np.int32)
    normb, iters = r0n.copy(), np.full(nb, -1, dtype=np.int32)
    if nb >= 7:
        iters[COL_ZERO_RHS] = 0
        if tol_stop > 0.0:
            normb[COL_CONVERGED] = r0n[COL_CONVERGED] / (5.0e-4 * tol_stop)
            iters[COL_CONVERGED] = 5
    return normb, iters


def sub_gram(full, NVfull, NV):
    """the DD Gram values of the first NV vectors out of those of NVfull"""
    idx = [gram_index(a, b, NVfull) for a in range(NV) for b in range(a, NV)]
    return full[idx]
