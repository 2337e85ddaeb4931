"""GPU: every BLAS-1 kernel and per-probe scalar update of the Krylov solver alone, against double-double and
longdouble references of the same operation.

Engine.krylov_multidot / krylov_gram / krylov_gram_cycle / krylov_multiaxpy / krylov_scalars (sw_krylov_*) run ONE
solver operation through the production host helper (multidot, multigram + multiaxpy, multiaxpy, launch_tail,
launch_fg_solve), so row_blocking, fused_ok, the KT / NV instantiation and the options fused_reduce and dot_blocks
choose the launch exactly as in a solve.  The references and limits are those of oracle/blas1_bounds.py, whose
docstring derives them; tests/test_blas1_bounds_host.py shows on the CPU that they pass the faithful emulations and
reject each seeded defect.  In short, with u = 2^-53 and S the sum of the absolute values of the real products of a
component:

  inner products   hard: every part within (4 n + 16) u S; tight: err / (u S) <= 4 c_ref + 4, c_ref the same figure
                   of the float64 emulation of the kernel's order of summation (in-launch or two-stage)
  k_multiaxpy      the same with K + 1 terms; + 2^-24 |ref| for a complex64 W; the complex64 copy bit for bit;
                   the fused norm within norm_limit (inner-product limit + propagated update error)
  Gram tail        |y - y*| / |y*| <= (4 c_ref + 4) u cond_2(M); relres within the same factor of
                   u cond_2(M) (rr0 / rr)^2 (|r_L|^2 is the difference |r0|^2 - sum |t_k|^2: its relative error is
                   that of the terms times |r0|^2 / |r_L|^2); decisions exactly, every one at least 10x from its
                   threshold by construction (asserted through decision_margins)
  Givens scalars   H, cs, sn, g against the longdouble QR to 64 u of the column norm; relres against
                   np.linalg.lstsq to 64 u cond(H); k_fg_solve to 64 u (|R| |y| + |g|) row by row, ys = svec y exactly

Row counts (default dot_blocks = 1024): n = 3 (one row block, wave 3 has no row), 100 (P = 25: one group, the
in-launch reduction ends at its first level), 133 (rows_per_block 4, P = 34: the last block holds one row; two groups,
the second with two blocks), 5123 (rows_per_block 6: the waves take 2 / 2 / 1 / 1 rows; P = 854, 27 groups, the last
with 22 blocks).  Batch widths nb = 3 (nbp = 64), 70 (two chunks: P halves at n = 5123), 200 (four chunks: the cap of
128 row blocks; n = 5123, K <= 4 only).  dot_blocks = 64 (P <= 64 at n = 5123) and 4096 (n = 16387: P = 3278, 103
groups > SW_RED_MAXGROUPS: the two-stage route; the Gram cycle refuses).  Column 1 of every input carries the scale
1e-3 and column 2 the scale 1e3.

Instantiations reached: k_multidot<KT, complex128 / complex64> for KT = 2, 4, 8, 16, 24, 34, each with K == KT and
K < KT (K = 1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 34: ragged 8-wide cross-wave batches and 6-wide reduction batches);
k_gram<2..5>; k_reduce_partials; reduce_and_tail with one group, two groups, 27 groups; k_multiaxpy<KT, NORM, CV, CW>
for the same K, NORM on / off, (CV, CW) = (complex128, complex128), (complex64, complex64), (complex64, complex128),
with and without the complex64 copy; k_fg_tail with BEGIN / HESS / VERIFY and the Gram tail inside k_gram; k_fg_solve.
Not reached: the BEGIN / HESS / VERIFY tails INSIDE a reducing launch (fg_tail_col is the same device function the
k_fg_tail kernel calls; the in-launch call site is exercised with the Gram tail).

Figures measured on an MI355X are in DESIGN.md, "Per-kernel parity of the Krylov solver kernels"; every assertion
message carries its own.
"""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import engine as EN  # noqa: E402
from oracle import blas1_bounds as bb  # noqa: E402

K_ALL = (1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 34)
U = bb.U64
CACHE = {}
WORST = {}


def _note(key, value):
    """the worst figure per kind, printed by the tests (run with -s) for DESIGN.md"""
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def _report(prefix):
    for k in sorted(WORST):
        if k.startswith(prefix):
            print("%-60s %.4g" % (k, WORST[k]))


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine()
    saved = {k: e.get_option(k) for k in ("fused_reduce", "dot_blocks")}
    yield e
    for k, v in saved.items():
        e.set_option(k, v)
    e.close()


@contextlib.contextmanager
def options(e, **kw):
    """dot_blocks is process-wide, fused_reduce per engine: both are put back whatever happens"""
    saved = {k: e.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            e.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            e.set_option(k, v)


def _dev(a):
    """[..., n, nb] -> the (..., nb, n) host layout of the entry points"""
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))


def _host(a):
    return np.swapaxes(a, -1, -2)


# -------------------------------------------------------------------------------------------------
# k_multidot, k_reduce_partials, reduce_and_tail
# -------------------------------------------------------------------------------------------------
def _dot_case(n, nb, Kmax, c64, dot_blocks=1024):
    """inputs, the double-double reference and the c_ref figures per reduction form, once per shape"""
    key = ("dot", n, nb, Kmax, c64, dot_blocks)
    if key not in CACHE:
        V, W = bb.rand_block((Kmax, n, nb), 1000 + n), bb.rand_block((n, nb), 2000 + n)
        if c64:
            V, W = bb.c64(V), bb.c64(W)
        ref, S = bb.dd_dots(V, W), bb.dot_scales(V, W)
        P, rpb = bb.row_blocking(n, bb.pad64(nb), True, dot_blocks)
        emu = {}
        for fused in (True, False):
            if fused and not bb.fused_ok(P, bb.pad64(nb)):
                continue
            out, _ = bb.emulate_multidot(V, W, P, rpb, fused)
            emu[fused] = bb.part_ratios(out, ref, *S).max(axis=1)        # per k
        svec = 0.5 + np.random.default_rng(n + nb).random((Kmax, nb))
        CACHE[key] = dict(Vd=_dev(V), Wd=_dev(W), ref=ref, S=S, P=P, rpb=rpb, emu=emu, svec=svec)
    return CACHE[key]


def _check_dot(e, case, n, nb, K, c64, fused, with_svec, label):
    svec = case["svec"][:K] if with_svec else None
    out, coef, pad, info = e.krylov_multidot(case["Vd"][:K], case["Wd"], svec, c64)
    assert info[:2] == (case["P"], case["rpb"]), "%s: row blocking %s, the twin gives %s" % (
        label, info[:2], (case["P"], case["rpb"]))
    assert info[2] == int(fused), "%s: reduction form %d, expected %d" % (label, info[2], fused)
    ref, (S_re, S_im) = case["ref"][:K], case["S"]
    r = bb.dot_ratio(out, ref, S_re[:K], S_im[:K])
    c_ref = float(case["emu"][fused][:K].max())
    _note("multidot %s %s n=%d ratio" % ("c64" if c64 else "c128", "fused" if fused else "two-stage", n), r)
    _note("multidot %s %s n=%d c_ref" % ("c64" if c64 else "c128", "fused" if fused else "two-stage", n), c_ref)
    assert r <= bb.hard_limit(n), "%s: err / (u S) = %.3g beyond the hard limit %g" % (label, r, bb.hard_limit(n))
    assert r <= bb.tight_limit(c_ref), "%s: err / (u S) = %.3g, tight limit %.3g (c_ref %.3g)" % (
        label, r, bb.tight_limit(c_ref), c_ref)
    assert pad == 0.0, "%s: pad columns of out up to %g" % (label, pad)
    if with_svec:
        q2 = svec ** 2
        want = q2 * out.real + 1j * (q2 * out.imag)
        d = np.maximum(np.abs(coef.real - want.real), np.abs(coef.imag - want.imag))
        rc = float((d / (U * np.maximum(np.abs(want.real), np.abs(want.imag)))).max())
        # (q q) t: two roundings; the emulation of a missing factor fails this by 1e10 (host test)
        assert rc <= 2.0, "%s: coef against svec^2 out: %.3g u" % (label, rc)
    return out


@pytest.mark.parametrize("n,nb", [(133, 3), (133, 70), (5123, 3), (5123, 70)])
def test_multidot_every_instantiation_against_double_double(eng, n, nb):
    """At n = 5123, nb = 70 the double-double reference and the emulations of K = 34 alone take 5 s on the CPU for the
    two storages: K stops at 9 there; K = 34 runs at n = 5123 with nb = 3 and at n = 133 with both widths."""
    Ks = K_ALL if n == 133 else ((1, 5, 9, 34) if nb == 3 else (1, 5, 9))
    for c64 in (False, True):
        case = _dot_case(n, nb, max(Ks), c64)
        for fr in (1, 0):
            with options(eng, fused_reduce=fr):
                for K in Ks:
                    for with_svec in (False, True):
                        label = "multidot n=%d nb=%d K=%d %s fused_reduce=%d svec=%d" % (
                            n, nb, K, "complex64" if c64 else "complex128", fr, with_svec)
                        out = _check_dot(eng, case, n, nb, K, c64, bool(fr), with_svec, label)
                    if fr:          # a repeated fused call: the order of every sum is fixed
                        again = eng.krylov_multidot(case["Vd"][:K], case["Wd"], case["svec"][:K], c64)[0]
                        assert np.array_equal(out, again), "%s: a repeated call differs" % label
    _report("multidot")


def test_multidot_leaves_the_ticket_counters_zero(eng):
    """the same call gives the same bits after a call of a different shape (other group counts, another chunk count)
    has used the counters"""
    a = _dot_case(133, 3, 34, False)
    b = _dot_case(5123, 70, 9, False)
    first = eng.krylov_multidot(a["Vd"][:9], a["Wd"])[0]
    eng.krylov_multidot(b["Vd"][:5], b["Wd"])
    second = eng.krylov_multidot(a["Vd"][:9], a["Wd"])[0]
    assert np.array_equal(first, second)
    g = eng.krylov_gram(a["Vd"][:3])[0]
    third = eng.krylov_multidot(a["Vd"][:9], a["Wd"])[0]
    assert np.array_equal(first, third) and np.all(np.isfinite(g))


def test_multidot_four_chunks_cap_the_row_blocks(eng):
    n, nb = 5123, 200
    case = _dot_case(n, nb, 4, False)
    assert case["P"] == 125
    for fr in (1, 0):
        with options(eng, fused_reduce=fr):
            for K in (1, 4):
                _check_dot(eng, case, n, nb, K, False, bool(fr), True, "multidot n=%d nb=%d K=%d fused_reduce=%d" % (n, nb, K, fr))


def test_dot_blocks_64_and_the_two_stage_route_beyond_the_group_limit(eng):
    with options(eng, dot_blocks=64):
        case = _dot_case(5123, 3, 5, False, dot_blocks=64)
        assert case["P"] <= 64
        _check_dot(eng, case, 5123, 3, 5, False, True, True, "multidot n=5123 dot_blocks=64")
    with options(eng, dot_blocks=4096):
        n, nb = 16387, 3
        case = _dot_case(n, nb, 4, False, dot_blocks=4096)
        assert case["P"] == 3278 and not bb.fused_ok(case["P"], 64)
        # fused_reduce is on, yet fused_ok turns false: the result comes from k_reduce_partials
        assert eng.get_option("fused_reduce") == 1.0
        _check_dot(eng, case, n, nb, 4, False, False, True, "multidot n=16387 dot_blocks=4096")
        with pytest.raises(EN.EngineError, match="in-launch reductions"):
            eng.krylov_gram(case["Vd"][:2])
        Ud = case["Vd"][:2]
        with pytest.raises(EN.EngineError, match="in-launch reductions"):
            eng.krylov_gram_cycle(Ud, Ud[:1], Ud[0], np.ones(nb), np.full(nb, -1), 1e-3, 1e-3)
    assert eng.get_option("dot_blocks") == 1024.0


# -------------------------------------------------------------------------------------------------
# k_gram without a tail
# -------------------------------------------------------------------------------------------------
def _gram_case(n, nb, NVmax, production=False):
    key = ("gram", n, nb, NVmax, production)
    if key not in CACHE:
        Uv, Z, X = bb.gram_inputs(n, nb, 3000 + n + (7 if production else 0), production)
        Uv, Z = Uv[:NVmax], Z[:NVmax - 1]
        ref, S_re, S_im = bb.dd_gram(Uv)
        P, rpb = bb.row_blocking(n, bb.pad64(nb))
        emu = bb.emulate_gram(Uv, P, rpb)
        CACHE[key] = dict(U=Uv, Z=Z, X=X, Ud=_dev(Uv), Zd=_dev(Z), Xd=_dev(X), ref=ref, S=(S_re, S_im), P=P, rpb=rpb,
                          emu=emu, c_ref=bb.part_ratios(emu, ref, S_re, S_im).max(axis=1))
    return CACHE[key]


def _check_gram_values(case, gram, NV, NVmax, n, label):
    idx = [bb.gram_index(a, b, NVmax) for a in range(NV) for b in range(a, NV)]
    ref = case["ref"][idx]
    r = bb.dot_ratio(gram, ref, case["S"][0][idx], case["S"][1][idx])
    c_ref = float(case["c_ref"][idx].max())
    _note("gram n=%d ratio" % n, r)
    _note("gram n=%d c_ref" % n, c_ref)
    assert r <= bb.hard_limit(n), "%s: err / (u S) = %.3g beyond the hard limit %g" % (label, r, bb.hard_limit(n))
    assert r <= bb.tight_limit(c_ref), "%s: err / (u S) = %.3g, tight limit %.3g (c_ref %.3g)" % (
        label, r, bb.tight_limit(c_ref), c_ref)
    for a in range(NV):
        im = gram[bb.gram_index(a, a, NV)].imag
        assert not np.any(im), "%s: diagonal entry (%d, %d) has an imaginary part up to %g" % (label, a, a, np.abs(im).max())


@pytest.mark.parametrize("n", [3, 100, 133, 5123])
@pytest.mark.parametrize("nb", [3, 70])
def test_gram_every_instantiation_against_double_double(eng, n, nb):
    case = _gram_case(n, nb, 5)
    for NV in (2, 3, 4, 5):
        label = "k_gram<%d> n=%d nb=%d" % (NV, n, nb)
        gram, info = eng.krylov_gram(case["Ud"][:NV])
        assert info[:3] == (case["P"], case["rpb"], 1), "%s: %s against the twin's %s" % (label, info, (case["P"], case["rpb"]))
        _check_gram_values(case, gram, NV, 5, n, label)
        again, _ = eng.krylov_gram(case["Ud"][:NV])
        assert np.array_equal(gram, again), "%s: a repeated call differs" % label
    _report("gram")


def test_gram_four_chunks(eng):
    n, nb = 5123, 200
    case = _gram_case(n, nb, 2)
    assert case["P"] == 125
    gram, info = eng.krylov_gram(case["Ud"])
    assert info[:3] == (125, 41, 1)
    _check_gram_values(case, gram, 2, 2, n, "k_gram<2> n=%d nb=%d" % (n, nb))


# -------------------------------------------------------------------------------------------------
# the Gram cycle: k_gram with the Gram tail (fg_gram_col), then the update of X
# -------------------------------------------------------------------------------------------------
def _gram_refs(case, L, production):
    key = ("gref", id(case), L)
    if key not in CACHE:
        idx = [bb.gram_index(a, b, 5) for a in range(L + 1) for b in range(a, L + 1)]
        CACHE[key] = (bb.gram_reference(case["U"][:L + 1], case["ref"][idx]), case["emu"][idx])
    return CACHE[key]


def _relres_ratio(relres, rr0, gref, normb, live):
    """|rr - rr*| / (u cond_2 rr* (rr0* / rr*)^2), the largest over the live columns"""
    L = gref["pivot"].shape[0]
    worst = 0.0
    for c in live:
        Leff = int((gref["pivot"][:, c] > 1e-13).cumprod().sum())
        want = np.sqrt(max(gref["res2"][Leff, c], 0.0)) / normb[c]
        want0 = np.sqrt(gref["res2"][0, c]) / normb[c]
        if want == 0.0:
            continue
        worst = max(worst, abs(relres[c] - want) / (U * max(gref["cond"][c], 1.0) * want * (want0 / want) ** 2))
    return worst


@pytest.mark.parametrize("production", [False, True], ids=["random", "production"])
@pytest.mark.parametrize("n", [133, 5123])
def test_gram_cycle_coefficients_decisions_and_update(eng, n, production):
    nb = 70
    case = _gram_case(n, nb, 5, production=production)
    Uv, Z, X = case["U"], case["Z"], case["X"]
    tol = 0.0 if production else bb.GRAM_TOL      # (production: as the K-cycle's inner iteration runs it)
    for L in (1, 2, 3, 4):
        gref, emu = _gram_refs(case, L, production)
        for tol_stop in ((0.0,) if production else (tol, tol / 100)):
            for init in (False, True):
                label = "Gram cycle n=%d L=%d %s tol_stop=%g init=%d" % (n, L, "production" if production else "random", tol_stop, init)
                normb, iters = bb.gram_entry_state(Uv, tol_stop, init)
                if production and not init:
                    normb, iters = np.sqrt(gref["res2"][0]), np.full(nb, -1, dtype=np.int32)
                nb_eff = np.sqrt(gref["res2"][0]) if init else normb
                margins = bb.decision_margins(gref, nb_eff, tol, tol_stop, np.full(nb, -1) if init else iters)
                assert margins.min() >= 10.0, "%s: a decision only %.3g from its threshold" % (label, margins.min())
                want_it, want_Leff, want_done, want_nc = bb.expected_decisions(gref, normb, iters, tol, tol_stop, 100, init)
                res = eng.krylov_gram_cycle(case["Ud"][:L + 1], case["Zd"][:L], case["Xd"], normb, iters, tol, tol_stop,
                                            iter_base=100, init=init)
                assert res["info"][:3] == (case["P"], case["rpb"], 1), label
                _check_gram_values(case, res["gram"], L + 1, 5, n, label)
                # decisions, exactly
                assert np.array_equal(res["iters"], want_it), "%s: iters %s, expected %s" % (label, res["iters"], want_it)
                assert res["notconv"] == want_nc, "%s: notconv %d, expected %d" % (label, res["notconv"], want_nc)
                ys = res["ys"]
                for c in range(nb):
                    assert not np.any(ys[want_Leff[c]:, c]), "%s: column %d: y beyond Leff = %d not zero" % (label, c, want_Leff[c])
                    assert want_Leff[c] == 0 or np.all(ys[:want_Leff[c], c] != 0), "%s: column %d truncated early" % (label, c)
                live = [c for c in range(nb) if not want_done[c]]
                # coefficients against the longdouble Cholesky solution of the double-double normal equations
                cyc = [bb.emulate_gram_col(emu[:, c], L, normb[c], iters[c], tol, tol_stop, 100, init) for c in range(nb)]
                c_ref = bb.coef_ratio(np.stack([q["ys"] for q in cyc], axis=1), gref, live)
                r = bb.coef_ratio(ys, gref, live)
                kind = "production" if production else "random"
                _note("gramcycle %s L=%d coef ratio" % (kind, L), r)
                _note("gramcycle %s L=%d coef c_ref" % (kind, L), c_ref)
                _note("gramcycle %s L=%d cond_2" % (kind, L), gref["cond"][live].max())
                assert r <= bb.tight_limit(c_ref), "%s: |y - y*| / |y*| = %.3g u cond_2, limit %.3g (c_ref %.3g)" % (
                    label, r, bb.tight_limit(c_ref), c_ref)
                c_rr = _relres_ratio(np.array([q["relres"] for q in cyc]), None, gref, nb_eff, live)
                r_rr = _relres_ratio(res["relres"], None, gref, nb_eff, live)
                _note("gramcycle %s L=%d relres ratio" % (kind, L), r_rr)
                _note("gramcycle %s L=%d relres c_ref" % (kind, L), c_rr)
                assert r_rr <= bb.tight_limit(c_rr), "%s: relres off by %.3g u cond_2 (rr0 / rr)^2, limit %.3g" % (
                    label, r_rr, bb.tight_limit(c_rr))
                # g = rr0 and normb from the device's own |r0|^2: a square root and a division, within an ulp (2 u) each
                g00 = np.maximum(res["gram"][0].real, 0.0)
                if init:
                    d = np.abs(res["normb"] - np.sqrt(g00))
                    assert np.all(d <= 2 * U * np.sqrt(g00)), "%s: normb off by %g" % (label, d.max())
                else:
                    assert np.array_equal(res["normb"], normb), label
                pos = res["normb"] > 0
                want_g = np.where(pos, np.sqrt(g00) / np.where(pos, res["normb"], 1.0), 0.0)
                assert np.all(np.abs(res["g"] - want_g) <= 4 * U * want_g), "%s: g = rr0 off by %g" % (
                    label, np.abs(res["g"] - want_g).max())
                for c in range(nb):
                    if want_done[c]:          # takes no part: relres = rr0
                        assert res["relres"][c] == res["g"][c], "%s: column %d done, relres != rr0" % (label, c)
                if not production and not init:
                    assert want_done[bb.COL_CONVERGED] and want_done[bb.COL_ZERO_RHS]
                    assert res["iters"][bb.COL_CONVERGED] == 5 and res["iters"][bb.COL_ZERO_RHS] == 0
                if not production and L == 4:
                    assert res["iters"][bb.COL_PASSES_AT_2] == 102, label
                    assert want_Leff[bb.COL_DUPLICATE] == 2, label
                # X + sum_j ys_j z_j with the device's own ys: independent of the coefficient check (once per L: the
                # update does not depend on the tolerances)
                if init or tol_stop != tol:
                    continue
                ref, S_re, S_im = bb.dd_axpy(Z[:L], ys, 1.0, X)
                c_ax = bb.axpy_ratio(bb.emulate_multiaxpy(Z[:L], ys, 1.0, X)[0], ref, S_re, S_im)
                r_ax = bb.axpy_ratio(_host(res["X"]), ref, S_re, S_im)
                _note("gramcycle update ratio", r_ax)
                assert r_ax <= min(bb.tight_limit(c_ax), bb.hard_limit(L + 1)), "%s: X update err / (u S) = %.3g, limit %.3g" % (
                    label, r_ax, bb.tight_limit(c_ax))
    _report("gramcycle")


# -------------------------------------------------------------------------------------------------
# k_multiaxpy
# -------------------------------------------------------------------------------------------------
STORAGE = ((False, False), (True, True), (True, False))          # (V complex64, W complex64): the engine's pairs


def _axpy_case(n, nb, Kmax, v64c, w64c):
    key = ("axpy", n, nb, Kmax, v64c, w64c)
    if key not in CACHE:
        V, Win = bb.rand_block((Kmax, n, nb), 5000 + n), bb.rand_block((n, nb), 6000 + n)
        coef = bb.rand_block((Kmax, nb), 7000 + n)
        coef[:, 0] = 0.0                      # a column whose coefficients are all zero
        if v64c:
            V = bb.c64(V)
        if w64c:
            Win = bb.c64(Win)
        CACHE[key] = dict(V=V, Win=Win, coef=coef, Vd=_dev(V), Wd=_dev(Win), refs={})
    return CACHE[key]


def _axpy_ref(case, K, sign, w64c):
    if (K, sign) not in case["refs"]:
        ref, S_re, S_im = bb.dd_axpy(case["V"][:K], case["coef"][:K], sign, case["Win"])
        _, w = bb.emulate_multiaxpy(case["V"][:K], case["coef"][:K], sign, case["Win"], w64c)
        case["refs"][(K, sign)] = (ref, S_re, S_im, w, bb.axpy_ratio(w, ref, S_re, S_im))
    return case["refs"][(K, sign)]


@pytest.mark.parametrize("n,nb", [(133, 70), (5123, 3)])
def test_multiaxpy_every_instantiation_against_double_double(eng, n, nb):
    Ks = K_ALL if n == 133 else (1, 9, 34)
    nbp = bb.pad64(nb)
    for v64c, w64c in STORAGE:
        case = _axpy_case(n, nb, max(Ks), v64c, w64c)
        name = "V %s W %s" % ("c64" if v64c else "c128", "c64" if w64c else "c128")
        for K in Ks:
            for sign in (1.0, -1.0):
                ref, S_re, S_im, w_emu, c_ax = _axpy_ref(case, K, sign, w64c)
                # norm off; norm on in-launch; norm on two-stage; with the complex64 copy (fp64 W)
                variants = [(False, 1, False), (True, 1, False), (True, 0, False)]
                if not w64c:
                    variants += [(True, 1, True), (False, 1, True)]
                for norm, fr, w32 in variants:
                    label = "multiaxpy n=%d nb=%d K=%d %s sign=%+d norm=%d fused_reduce=%d w32=%d" % (
                        n, nb, K, name, sign, norm, fr, w32)
                    with options(eng, fused_reduce=fr):
                        Wout, nrm, W32, info = eng.krylov_multiaxpy(case["Vd"][:K], case["coef"][:K], sign, case["Wd"],
                                                                    v_c64=v64c, w_c64=w64c, norm=norm, w32=w32)
                    P, rpb = bb.row_blocking(n, nbp, norm)
                    assert info[:3] == (P, rpb, int(norm and bool(fr))), "%s: %s against the twin's %s" % (label, info, (P, rpb))
                    Wout = _host(Wout)
                    r = bb.axpy_ratio(Wout, ref, S_re, S_im, w64c)
                    _note("multiaxpy %s ratio" % name, r)
                    _note("multiaxpy %s c_ref" % name, c_ax)
                    assert r <= bb.hard_limit(K + 1), "%s: err / (u S) = %.3g beyond the hard limit %g" % (
                        label, r, bb.hard_limit(K + 1))
                    assert r <= bb.tight_limit(c_ax), "%s: err / (u S) = %.3g, tight limit %.3g (c_ref %.3g)" % (
                        label, r, bb.tight_limit(c_ax), c_ax)
                    assert np.array_equal(Wout[:, 0], case["Win"][:, 0]), "%s: the zero-coefficient column changed" % label
                    if w32:
                        assert np.array_equal(_host(W32), Wout.astype(np.complex64).astype(np.complex128)), \
                            "%s: the complex64 copy is not float32(Wout)" % label
                    if norm:
                        c_sum = bb.norm_sum_cref(w_emu, P, rpb, bool(fr))
                        rt = bb.norm_ratio(nrm, bb.tight_limit(c_ax), bb.tight_limit(c_sum), ref, S_re, S_im)
                        rh = bb.norm_ratio(nrm, bb.hard_limit(K + 1), bb.hard_limit(n), ref, S_re, S_im)
                        _note("multiaxpy norm %s: err / tight norm_limit" % ("fused" if fr else "two-stage"), rt)
                        _note("multiaxpy norm %s: err / hard norm_limit" % ("fused" if fr else "two-stage"), rh)
                        assert rh <= 1.0, "%s: norm at %.3g of its hard limit" % (label, rh)
                        assert rt <= 1.0, "%s: norm at %.3g of its tight limit (c_sum %.3g, c_ax %.3g)" % (label, rt, c_sum, c_ax)
    _report("multiaxpy")


# -------------------------------------------------------------------------------------------------
# the FGMRES scalars: k_fg_tail (BEGIN, HESS, VERIFY) and k_fg_solve
# -------------------------------------------------------------------------------------------------
def _dense(n, seed, contract=None):
    rng = np.random.default_rng(seed)
    G = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(2 * n)
    return np.eye(n) + contract * G if contract else G + 0.5 * np.eye(n)


def _run_cycle(e, A, B, m, passes, tol, tol_stop, pyth_last=False, iter_base=0):
    """one restart cycle: the host Arnoldi process feeds the device scalar updates.  Returns (state after the cycle,
    state after BEGIN, raws, per-step (state, notconv), the Arnoldi object)"""
    nb = B.shape[1]
    ar = bb.UnnormalisedArnoldi(A, B, m, passes)
    st, _ = e.krylov_scalars(bb.new_state(m, nb), EN.KRYLOV_BEGIN, flag=1, nrm=ar.begin())
    begin = st
    raws, steps = [], []
    for j in range(m):
        pyth = pyth_last and j == m - 1
        h1, h2, nrm2 = ar.step(j, st["svec"], pyth)
        st, nc = e.krylov_scalars(st, EN.KRYLOV_HESS, j=j, flag=int(pyth), tol=tol, tol_stop=tol_stop, iter_base=iter_base,
                                  h1=h1, h2=h2, nrm=nrm2)
        raws.append((h1 if h2 is None else h1 + h2, nrm2))
        steps.append((st, nc))
    return st, begin, raws, steps, ar


def _check_begin(begin, nrm, label):
    beta = np.sqrt(nrm)
    for key in ("normb", "relres"):
        assert not np.any(begin[key].imag)
    assert np.all(np.abs(begin["normb"].real - beta) <= 2 * U * beta), label       # one square root: within an ulp
    assert np.array_equal(begin["g"][0], begin["normb"]), label
    pos = beta > 0
    inv = np.where(pos, 1.0 / np.where(pos, begin["normb"].real, 1.0), 0.0)
    assert np.all(np.abs(begin["svec"][0].real - inv) <= 2 * U * inv), label       # one division: within an ulp
    assert np.array_equal(begin["iters"], np.where(pos, -1, 0)), label
    assert np.array_equal(begin["relres"].real, np.where(pos, 1.0, 0.0)), label


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("nb", [3, 70])
def test_hessenberg_columns_against_longdouble_givens(eng, nb, passes):
    n, m = 64, 6
    A, B = _dense(n, 51), bb.rand_block((n, nb), 52)
    label = "fg scalars nb=%d passes=%d" % (nb, passes)
    st, begin, raws, steps, ar = _run_cycle(eng, A, B, m, passes, 1e-30, 1e-30)
    _check_begin(begin, ar.begin(), label)
    beta = begin["g"][0].real
    gref = bb.givens_reference(st["svec"], raws, m)
    for j, (sj, nc) in enumerate(steps):
        rH, rc, rg = bb.givens_ratios(sj, gref, j, beta)
        _note("fg givens H err / (u colnorm)", rH)
        _note("fg givens cs, sn err / u", rc)
        _note("fg givens g err / (u beta)", rg)
        assert max(rH, rc, rg) <= bb.GIVENS_LIMIT, "%s column %d: H %.3g, cs / sn %.3g, g %.3g u against the limit %g" % (
            label, j, rH, rc, rg, bb.GIVENS_LIMIT)
        assert nc == nb, "%s column %d: notconv %d" % (label, j, nc)          # nothing converges to 1e-30
        # |g_{j+1}| / normb is the residual of the (j + 2) x (j + 1) least-squares problem
        for c in range(nb):
            Hc = gref["Hraw"][:j + 2, :j + 1, c]
            rhs = np.zeros(j + 2, dtype=np.complex128)
            rhs[0] = 1.0
            y = np.linalg.lstsq(Hc, rhs, rcond=None)[0]
            want = np.linalg.norm(rhs - Hc @ y)
            got = sj["relres"][c].real
            r = abs(got - want) / (U * np.linalg.cond(Hc))
            _note("fg relres against lstsq / (u cond)", r)
            assert r <= bb.GIVENS_LIMIT, "%s column %d probe %d: relres %.17g, lstsq %.17g: %.3g u cond(H)" % (label, j, c, got, want, r)
    sol, _ = eng.krylov_scalars(st, EN.KRYLOV_SOLVE, j=m)
    for c in range(nb):
        R = np.triu(st["H"][:m, :, c])
        y, g = sol["y"][:, c], st["g"][:m, c]
        d = np.abs(R @ y - g)
        lim = U * (np.abs(R) @ np.abs(y) + np.abs(g))
        r = float((d / lim).max())
        _note("fg solve residual / (u (|R||y| + |g|))", r)
        assert r <= bb.GIVENS_LIMIT, "%s probe %d: H y = g to %.3g u" % (label, c, r)
    sv = st["svec"][:m].real
    assert np.array_equal(sol["ys"], sv * sol["y"].real + 1j * (sv * sol["y"].imag)), "%s: ys != svec y" % label
    for key in ("H", "cs", "sn", "g", "svec", "normb", "relres"):
        assert np.array_equal(sol[key], st[key]), "%s: the solve changed %s" % (label, key)
    _report("fg")


def test_last_step_from_the_pythagorean_identity(eng):
    """pyth = 1: h_{j+1,j}^2 = svec_j^2 |A z_j|^2 - sum_k |h_{k,j}|^2, a DIFFERENCE of squares: its relative error is
    u |col|^2 / h_{j+1,j}^2, so h_{j+1,j} agrees with the explicit norm of the orthogonalised vector to sqrt(u)
    relative, not to a few u; the rotation and g inherit that."""
    n, m, nb = 64, 6, 70
    A, B = _dense(n, 51), bb.rand_block((n, nb), 52)
    st, begin, raws, steps, ar = _run_cycle(eng, A, B, m, 1, 1e-30, 1e-30, pyth_last=True)
    gref = bb.givens_reference(st["svec"], raws, m)        # (the last column from the explicit |vtilde_m|^2)
    beta = begin["g"][0].real
    for j in range(m - 1):
        assert max(bb.givens_ratios(steps[j][0], gref, j, beta)) <= bb.GIVENS_LIMIT
    rH, rc, rg = bb.givens_ratios(st, gref, m - 1, beta)
    lim = np.sqrt(U) / U
    _note("fg pyth last column: largest err / sqrt(u)", max(rH, rc, rg) / lim)
    assert max(rH, rc, rg) <= lim, "pyth column: H %.3g, cs / sn %.3g, g %.3g u against sqrt(u) / u = %.3g" % (rH, rc, rg, lim)
    assert max(rH, rc, rg) > 0.0
    # the vector is never formed: svec_m is 1 / wn of the identity's own wn, the same sqrt(u)
    hn = np.sqrt(raws[m - 1][1])
    assert np.all(np.abs(st["svec"][m].real * hn - 1.0) <= np.sqrt(U))
    _report("fg pyth")


def test_happy_breakdown_freezes_the_probe(eng):
    """b lies in an invariant subspace of dimension 3 of A (probe 0 does not): after three columns the orthogonalised
    vector is round-off, h_{3,2} <= 1e-14 |A z_2| by more than 10x (asserted), the probe freezes: svec_3 = 0, the later
    columns are exactly zero and k_fg_solve gives y = 0 there."""
    n, m, nb = 64, 6, 5
    rng = np.random.default_rng(61)
    A = np.zeros((n, n), dtype=np.complex128)
    A[:3, :3] = _dense(3, 62) + np.eye(3)
    A[3:, 3:] = _dense(n - 3, 63)
    B = np.zeros((n, nb), dtype=np.complex128)
    B[:3] = rng.standard_normal((3, nb)) + 1j * rng.standard_normal((3, nb))
    B[:, 0] = bb.rand_block((n, 1), 64)[:, 0]
    B[:, 1] *= 1e-3
    B[:, 2] *= 1e3
    st, begin, raws, steps, ar = _run_cycle(eng, A, B, m, 2, 1e-30, 1e-30)
    s2 = steps[2][0]
    hn = s2["svec"][2].real * np.sqrt(raws[2][1])
    col = np.sqrt((np.abs(s2["svec"][:3].real * s2["svec"][2].real * raws[2][0][:3]) ** 2).sum(axis=0) + hn ** 2)
    assert np.all(hn[1:] <= 1e-15 * col[1:]) and hn[0] > 1e-13 * col[0], (hn / col)
    assert np.all(s2["svec"][3, 1:] == 0) and s2["svec"][3, 0].real > 0
    assert np.all(st["svec"][3:, 1:] == 0) and np.all(st["svec"][:, 0].real > 0)
    assert not np.any(st["H"][:, 3:, 1:]) and np.all(st["H"][3, 3, :1] != 0)
    assert not np.any(st["g"][4:, 1:])
    for j in (3, 4, 5):
        assert steps[j][1] == 1, "a frozen probe is not counted: %d" % steps[j][1]
    sol, _ = eng.krylov_scalars(st, EN.KRYLOV_SOLVE, j=m)
    assert not np.any(sol["y"][3:, 1:]) and not np.any(sol["ys"][3:, 1:])
    assert np.all(sol["y"][:3, 1:] != 0) and np.all(sol["y"][:, 0] != 0)
    # relres of a frozen probe stays what the last live column left
    assert np.array_equal(st["relres"][1:], steps[2][0]["relres"][1:])


def test_freeze_two_orders_below_tol_stop_and_the_iteration_count(eng):
    """A = I + 5e-6 G: the residual falls by about 1e-5 per column, so tol = tol_stop = 10 sqrt(rr_1 rr_2) puts rr_1
    above tol and rr_2 below 1e-2 tol_stop, each by more than 10x (asserted on the least-squares residuals): iters = 2
    for every probe, frozen from column 2 on; the zero right-hand side (probe 3) is never counted."""
    n, m, nb = 64, 6, 6
    A, B = _dense(n, 71, contract=5e-6), bb.rand_block((n, nb), 72)
    B[:, 3] = 0.0
    live = [0, 1, 2, 4, 5]
    _, _, raws, steps, _ = _run_cycle(eng, A, B, m, 2, 1e-30, 1e-30)
    gref = bb.givens_reference(steps[-1][0]["svec"], raws, m)
    rr = np.concatenate([np.ones((1, nb)), np.abs(gref["gsteps"][:, 1]).astype(np.float64)])   # rr[j + 1]: after column j
    tol = 10.0 * np.sqrt(rr[1, 0] * rr[2, 0])
    assert np.all(rr[1, live] >= 10 * tol) and np.all(rr[2, live] <= 1e-2 * tol / 10), (rr[1], rr[2], tol)
    st, begin, raws, steps, _ = _run_cycle(eng, A, B, m, 2, tol, tol, iter_base=40)
    assert np.array_equal(st["iters"], [42, 42, 42, 0, 42, 42]), st["iters"]
    assert [nc for _, nc in steps] == [5, 0, 0, 0, 0, 0], [nc for _, nc in steps]
    assert np.all(steps[0][0]["svec"][1, live].real > 0) and np.all(steps[1][0]["svec"][2] == 0)
    assert not np.any(st["H"][:, 2:]) and not np.any(st["svec"][2:])
    assert not np.any(st["H"][:, :, 3]) and not np.any(st["g"][:, 3]) and st["relres"][3] == 0
    sol, _ = eng.krylov_scalars(st, EN.KRYLOV_SOLVE, j=m)
    assert not np.any(sol["y"][2:]) and not np.any(sol["y"][:, 3]) and np.all(sol["y"][:2, live] != 0)
    # with tol_stop = 1e-6 tol the probes pass tol at the same column, are still counted there and stay live
    st2, _, _, steps2, _ = _run_cycle(eng, A, B, m, 2, tol, tol * 1e-6, iter_base=40)
    assert np.array_equal(st2["iters"], st["iters"])
    assert np.all(rr[2, live] >= 10 * tol * 1e-6)
    assert np.all(steps2[1][0]["svec"][2, live].real > 0) and steps2[1][1] == 5


def test_verify_and_begin_updates(eng):
    m, nb = 6, 70
    rng = np.random.default_rng(81)
    st = bb.new_state(m, nb)
    normb = np.exp(rng.uniform(-7, 7, nb))
    st["normb"] = normb.astype(np.complex128)
    st["iters"] = np.arange(nb, dtype=np.int32) + 3
    tol, tol_stop = 1e-6, 1e-8
    # probes 0 mod 3: 10x above tol (lose their iteration, counted); 1 mod 3: between (keep it, counted);
    # 2 mod 3: 10x below tol_stop (keep it, not counted)
    rr = np.where(np.arange(nb) % 3 == 0, 10 * tol, np.where(np.arange(nb) % 3 == 1, 1e-7, tol_stop / 10))
    nrm = (rr * normb) ** 2
    out, nc = eng.krylov_scalars(st, EN.KRYLOV_VERIFY, tol=tol, tol_stop=tol_stop, nrm=nrm)
    want = np.where(np.arange(nb) % 3 == 0, -1, st["iters"])
    assert np.array_equal(out["iters"], want), out["iters"]
    assert nc == int((np.arange(nb) % 3 != 2).sum()), nc
    exact = np.sqrt(nrm) / normb
    assert np.all(np.abs(out["relres"].real - exact) <= 4 * U * exact)      # a square root and a division, an ulp each
    # BEGIN in a later cycle: normb, iters and relres stay, g_0 and svec_0 follow the new residual
    st["relres"] = rr.astype(np.complex128)
    nrm[5] = 0.0
    out, nc = eng.krylov_scalars(st, EN.KRYLOV_BEGIN, flag=0, nrm=nrm)
    for key in ("normb", "relres", "iters"):
        assert np.array_equal(out[key], st[key]), key
    beta = np.sqrt(nrm)
    assert np.all(np.abs(out["g"][0].real - beta) <= 2 * U * beta) and out["svec"][0, 5] == 0 and nc == 0
    # ... and in the first: a zero right-hand side is settled at once
    first, _ = eng.krylov_scalars(st, EN.KRYLOV_BEGIN, flag=1, nrm=nrm)
    _check_begin(first, nrm, "BEGIN first cycle")
    assert first["iters"][5] == 0 and first["relres"][5] == 0 and first["normb"][5] == 0


def test_krylov_entry_argument_errors(eng):
    V = bb.rand_block((2, 3, 8), 91)            # (K, nb, n) as the entries take it
    lib, h = eng._lib, eng._h
    with pytest.raises(EN.EngineError, match="K=35 out of"):
        eng.krylov_multidot(np.zeros((35, 3, 8)), V[0])
    with pytest.raises(EN.EngineError, match="K=35 out of"):
        eng.krylov_multiaxpy(np.zeros((35, 3, 8)), np.zeros((35, 3)), 1.0, V[0])
    z = EN._c128(np.zeros((3, 8)))
    info = np.zeros(4, dtype=np.int32)
    for K in (0, -1):
        assert lib.sw_krylov_multidot(h, 8, 3, K, 0, EN._ptr(z), EN._ptr(z), None, EN._ptr(z), None, EN._ptr(info)) != 0
        assert b"out of" in lib.sw_last_error(h)
    for NV in (1, 6):
        with pytest.raises(EN.EngineError, match="vectors out of"):
            eng.krylov_gram(np.zeros((NV, 3, 8)))
    with pytest.raises(EN.EngineError, match="unsupported storage pair"):
        eng.krylov_multiaxpy(V, np.zeros((2, 3)), 1.0, V[0], v_c64=False, w_c64=True)
    with pytest.raises(EN.EngineError, match="fp64 W"):
        eng.krylov_multiaxpy(V, np.zeros((2, 3)), 1.0, V[0], v_c64=True, w_c64=True, w32=True)
    assert lib.sw_krylov_multidot(h, 8, 3, 2, 7, EN._ptr(z), EN._ptr(z), None, EN._ptr(z), None, None) != 0
    assert b"unsupported storage" in lib.sw_last_error(h)
    # a Gram tail while the in-launch reduction is off
    with options(eng, fused_reduce=0):
        with pytest.raises(EN.EngineError, match="in-launch reductions"):
            eng.krylov_gram_cycle(V, V[:1], V[0], np.ones(3), np.full(3, -1), 1e-3, 1e-3)
        with pytest.raises(EN.EngineError, match="in-launch reductions"):
            eng.krylov_gram(V)
    st = bb.new_state(6, 3)
    with pytest.raises(EN.EngineError, match="unknown operation"):
        eng.krylov_scalars(st, 4)
    with pytest.raises(EN.EngineError, match="out of range"):
        eng.krylov_scalars(st, EN.KRYLOV_HESS, j=6, h1=np.zeros((8, 3)), nrm=np.ones(3))
    with pytest.raises(EN.EngineError, match="needs nrm"):
        eng.krylov_scalars(st, EN.KRYLOV_VERIFY)
    # the engine still works after the refusals
    out = eng.krylov_multidot(V, V[0])[0]
    assert np.all(np.isfinite(out))
