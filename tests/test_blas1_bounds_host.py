"""CPU: the references and limits of the Krylov solver's per-kernel tests (oracle/blas1_bounds.py) separate right
from wrong.

tests/test_gpu_krylov_kernels.py holds k_multidot, k_gram, k_reduce_partials, the in-launch reduction, k_multiaxpy
and the per-probe scalar updates to the limits derived in oracle/blas1_bounds.py.  Here the same helpers run on the
float64 emulations alone, at the smallest shape of the GPU file at which each defect can be seeded (n = 133:
rows_per_block = 4, P = 34 row blocks, the last one with a single row, two groups of the in-launch reduction):

  the double-double inner product equals the exact rational one (fractions) to 2^-100
  the Python twins of row_blocking / fused_ok give the geometry the GPU file relies on
  the faithful emulations -- both reduction forms, both storages, and another order of the sum -- pass both limits
  each seeded defect is rejected, by the limit named:
    last row of a ragged row block dropped, a row block dropped, a group of 32 dropped, one partial added twice,
    the accumulator k = K - 1 of a KT > K instantiation dropped, the conjugate on W instead of V:
                                                 hard limit (4 n + 16) u S (and with it the tight one)
    coef without the svec^2 factor:              coef = svec^2 out to 2 u (two roundings)
    sign ignored in the update:                  hard limit (4 (K + 1) + 16) u S of k_multiaxpy
    Gram entry (a, b) read at the index of (b, a): the coefficient limit 4 c_ref + 4 in units of u cond_2(M), on
                                                 both input sets
    Givens rotation with sn not conjugated:      the 64 u limit on the rotated Hessenberg column and g
  the decisions of the Gram tail on the inputs of the GPU file are at least 10x from their thresholds, and the
  float64 emulation takes them as the longdouble reference does."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import blas1_bounds as bb

N, NB = 133, 5
P, RPB = bb.row_blocking(N, bb.pad64(NB))
CACHE = {}


def _dots(K, c64=False):
    key = ("dots", K, c64)
    if key not in CACHE:
        V, W = bb.rand_block((K, N, NB), 21), bb.rand_block((N, NB), 22)
        if c64:
            V, W = bb.c64(V), bb.c64(W)
        CACHE[key] = (V, W, bb.dd_dots(V, W), bb.dot_scales(V, W))
    return CACHE[key]


def test_double_double_inner_product_against_exact_rationals():
    rng = np.random.default_rng(3)
    V = (rng.standard_normal((2, 9, 2)) + 1j * rng.standard_normal((2, 9, 2))) * 2.0 ** rng.integers(-20, 20, (2, 9, 2))
    W = (rng.standard_normal((9, 2)) + 1j * rng.standard_normal((9, 2))) * 2.0 ** rng.integers(-20, 20, (9, 2))
    ref = bb.dd_dots(V, W, lanes=4)          # (9 rows on 4 lanes: a ragged last step)
    S_re, S_im = bb.dot_scales(V, W)
    F = Fraction
    for k in range(2):
        for c in range(2):
            re = sum(F(V[k, r, c].real) * F(W[r, c].real) + F(V[k, r, c].imag) * F(W[r, c].imag) for r in range(9))
            im = sum(F(V[k, r, c].real) * F(W[r, c].imag) - F(V[k, r, c].imag) * F(W[r, c].real) for r in range(9))
            got_re = F(ref.re[0][k, c]) + F(ref.re[1][k, c])
            got_im = F(ref.im[0][k, c]) + F(ref.im[1][k, c])
            assert abs(got_re - re) <= F(S_re[k, c]) * F(2) ** -100, (k, c, float(got_re - re))
            assert abs(got_im - im) <= F(S_im[k, c]) * F(2) ** -100, (k, c, float(got_im - im))
    assert ref.rounded().shape == (2, 2)


def test_row_blocking_twin_gives_the_geometry_of_the_gpu_cases():
    rb = bb.row_blocking
    assert rb(3, 64) == (1, 4)                       # one row block; wave 3 has no row
    assert rb(100, 64) == (25, 4)                    # one group: the in-launch reduction ends at its first level
    assert rb(133, 64) == (34, 4) and 133 - 33 * 4 == 1            # two groups, the second with two blocks
    assert rb(5123, 64) == (854, 6)                  # waves take 2 / 2 / 1 / 1 rows; 27 groups, the last with 22
    assert (854 + 31) // 32 == 27 and 854 - 26 * 32 == 22
    assert rb(133, 128) == (34, 4) and rb(5123, 128) == (466, 11)  # two chunks: p halves
    assert rb(5123, 256) == (125, 41)                # four chunks: the cap of 128 row blocks
    assert rb(5123, 64, True, 64)[0] <= 64
    Pbig, _ = rb(16387, 64, True, 4096)
    assert Pbig == 3278 and (Pbig + 31) // 32 == 103 and not bb.fused_ok(Pbig, 64)
    assert bb.fused_ok(854, 64) and not bb.fused_ok(854, 64, fused_reduce=False)
    assert rb(5123, 64, False) == (1281, 4)          # no reduction: a budget of 4096 blocks, at least 4 rows each
    assert [bb.gram_index(a, b, 3) for a in range(3) for b in range(a, 3)] == list(range(6))


@pytest.mark.parametrize("c64", [False, True])
def test_faithful_emulations_pass_both_limits(c64):
    V, W, ref, S = _dots(34, c64)
    worst = 0.0
    for fused in (True, False):
        out, _ = bb.emulate_multidot(V, W, P, RPB, fused)
        c_ref = bb.dot_ratio(out, ref, *S)
        worst = max(worst, c_ref)
        assert c_ref <= bb.hard_limit(N), c_ref
    # another order of the same sum (NumPy's own) stays inside the tight limit of either emulation
    other = bb.dot_ratio(np.einsum("krc,rc->kc", V.conj(), W), ref, *S)
    assert other <= bb.tight_limit(0.0) <= bb.tight_limit(worst), (other, worst)


DOT_DEFECTS = [("drop_row", N - 1), ("drop_block", 5), ("drop_group", 1), ("dup_partial", 7), ("drop_last_acc", None),
               ("conj_w", None)]


# (the two-stage reduction has no groups to drop)
DOT_DEFECT_CASES = [(d, f) for d in DOT_DEFECTS for f in (True, False) if f or d[0] != "drop_group"]


@pytest.mark.parametrize("defect,fused", DOT_DEFECT_CASES,
                         ids=["%s-%s" % (d[0], "fused" if f else "two_stage") for d, f in DOT_DEFECT_CASES])
def test_limits_reject_the_seeded_inner_product_defects(defect, fused):
    K = 3                      # KT = 4 > K: the last accumulator in use is not the last of the instantiation
    V, W, ref, S = _dots(K)
    good, _ = bb.emulate_multidot(V, W, P, RPB, fused)
    c_ref = bb.dot_ratio(good, ref, *S)
    bad, _ = bb.emulate_multidot(V, W, P, RPB, fused, defect=defect)
    r = bb.dot_ratio(bad, ref, *S)
    assert r > 1e6 * bb.hard_limit(N) > bb.tight_limit(c_ref), (defect, r, c_ref)


def _coef_ratio(coef, out, svec):
    q2 = np.asarray(svec) ** 2
    want = q2 * out.real + 1j * (q2 * out.imag)
    d = np.maximum(np.abs(coef.real - want.real), np.abs(coef.imag - want.imag))
    return float((d / (bb.U64 * np.maximum(np.abs(want.real), np.abs(want.imag)))).max())


def test_coef_check_rejects_a_missing_svec_factor():
    V, W, ref, S = _dots(3)
    svec = 0.5 + np.random.default_rng(5).random((3, NB))
    out, coef = bb.emulate_multidot(V, W, P, RPB, True, svec=svec)
    assert _coef_ratio(coef, out, svec) <= 2.0
    _, bad = bb.emulate_multidot(V, W, P, RPB, True, svec=svec, defect=("coef_no_svec", None))
    assert _coef_ratio(bad, out, svec) > 1e10


@pytest.mark.parametrize("w_c64", [False, True])
def test_multiaxpy_limits_pass_the_emulation_and_reject_an_ignored_sign(w_c64):
    K = 9
    V, Win = bb.rand_block((K, N, NB), 31), bb.rand_block((N, NB), 32)
    coef = bb.rand_block((K, NB), 33)
    coef[:, 4] = 0.0
    if w_c64:
        V, Win = bb.c64(V), bb.c64(Win)
    for sign in (1.0, -1.0):
        ref, S_re, S_im = bb.dd_axpy(V, coef, sign, Win)
        out, w = bb.emulate_multiaxpy(V, coef, sign, Win, w_c64)
        c_ref = bb.axpy_ratio(out, ref, S_re, S_im, w_c64)
        assert c_ref <= bb.hard_limit(K + 1) / 2 and bb.tight_limit(c_ref) < bb.hard_limit(K + 1), c_ref
        assert np.array_equal(out[:, 4], Win[:, 4])          # a zero coefficient column: bit-identical
        # the fused norm of the values before narrowing, against the double-double norm of the double-double update
        Pn, rpbn = bb.row_blocking(N, bb.pad64(NB), True)
        for fused in (True, False):
            nrm = bb.emulate_norm(w, Pn, rpbn, fused)
            c_sum = bb.norm_sum_cref(w, Pn, rpbn, fused)
            c_ax = bb.axpy_ratio(w, ref, S_re, S_im)
            assert bb.norm_ratio(nrm, bb.tight_limit(c_ax), bb.tight_limit(c_sum), ref, S_re, S_im) <= 1.0
            assert bb.norm_ratio(nrm, bb.hard_limit(K + 1), bb.hard_limit(N), ref, S_re, S_im) <= 1.0
            # ... and it is a limit: a norm that misses its last row is far outside
            short = bb.emulate_norm(np.concatenate([w[:-1], np.zeros((1, NB))]), Pn, rpbn, fused)
            assert bb.norm_ratio(short, bb.hard_limit(K + 1), bb.hard_limit(N), ref, S_re, S_im) > 1e6
    ref, S_re, S_im = bb.dd_axpy(V, coef, -1.0, Win)
    bad, _ = bb.emulate_multiaxpy(V, coef, -1.0, Win, w_c64, ignore_sign=True)
    r = bb.axpy_ratio(bad[:, :4], ref[:, :4], S_re[:, :4], S_im[:, :4], w_c64)
    assert r > 1e6 * bb.hard_limit(K + 1), r


def _gram_case(production):
    key = ("gram", production)
    if key not in CACHE:
        nb = 9
        U, Z, X = bb.gram_inputs(N, nb, 41, production)
        Pg, rpbg = bb.row_blocking(N, bb.pad64(nb))
        CACHE[key] = (U, bb.dd_gram(U)[0], bb.emulate_gram(U, Pg, rpbg))
    return CACHE[key]


def _emulated_cycle(d, L, normb, iters, tol, tol_stop, iter_base, init, swap=None):
    nb = d.shape[1]
    cols = [bb.emulate_gram_col(d[:, c], L, normb[c], iters[c], tol, tol_stop, iter_base, init, swap) for c in range(nb)]
    return (np.stack([c["ys"] for c in cols], axis=1), np.array([c["iters"] for c in cols]),
            np.array([c["Leff"] for c in cols]), np.array([c["done"] for c in cols]), sum(c["notconv"] for c in cols),
            np.array([c["relres"] for c in cols]))


@pytest.mark.parametrize("production", [False, True])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_gram_tail_emulation_meets_the_reference_and_its_decisions(L, production):
    U, full, emu = _gram_case(production)
    NV = L + 1
    gref = bb.gram_reference(U[:NV], bb.sub_gram(full, 5, NV))
    d = bb.sub_gram(emu, 5, NV)
    tol = 0.0 if production else bb.GRAM_TOL
    for tol_stop in ((0.0,) if production else (tol, tol / 100)):
        for init in (False, True):
            normb, iters = bb.gram_entry_state(U, tol_stop, init)
            if production and not init:          # (no special columns in this set)
                normb, iters = np.sqrt(gref["res2"][0]), np.full(U.shape[2], -1, dtype=np.int32)
            margins = bb.decision_margins(gref, np.sqrt(gref["res2"][0]) if init else normb, tol, tol_stop,
                                          np.full(U.shape[2], -1) if init else iters)
            assert margins.min() >= 10.0, margins
            ys, it, Leff, done, notconv, relres = _emulated_cycle(d, L, normb, iters, tol, tol_stop, 100, init)
            want_it, want_Leff, want_done, want_nc = bb.expected_decisions(gref, normb, iters, tol, tol_stop, 100, init)
            assert np.array_equal(it, want_it) and np.array_equal(Leff, want_Leff), (it, want_it, Leff, want_Leff)
            assert np.array_equal(done, want_done) and notconv == want_nc
            live = [c for c in range(U.shape[2]) if not want_done[c]]
            assert not np.any(ys[:, want_done])          # a probe that takes no part: y = 0
            c_ref = bb.coef_ratio(ys, gref, live)
            print("Gram tail L=%d production=%d init=%d: c_ref %.3g, cond_2 up to %.3g" % (L, production, init, c_ref, gref["cond"].max()))
            assert np.isfinite(c_ref)
            if production:
                assert L < 3 or gref["cond"].min() > 1e5, gref["cond"]
            else:
                assert gref["cond"][[0, 1, 2]].max() < 1e3
                assert it[bb.COL_ZERO_RHS] == 0 and not np.any(ys[:, bb.COL_ZERO_RHS])
                if L == 4:
                    assert it[bb.COL_PASSES_AT_2] == 102
                    assert Leff[bb.COL_DUPLICATE] == 2 and not np.any(ys[2:, bb.COL_DUPLICATE])
                if not init:
                    assert done[bb.COL_CONVERGED] and not np.any(ys[:, bb.COL_CONVERGED])
                    assert relres[bb.COL_CONVERGED] < 1.0e-2 * tol_stop
            # entry (0, 1) read at the index the kernel's formula gives for (1, 0): NV - 1, the place of (0, NV - 1)
            # (the same place for NV = 2)
            if L >= 2:
                bad = _emulated_cycle(d, L, normb, iters, tol, tol_stop, 100, init, swap=(0, 1))[0]
                assert bb.coef_ratio(bad, gref, live) > 1e3 * bb.tight_limit(c_ref), bb.coef_ratio(bad, gref, live)


def _dense(n, seed, contract=None):
    rng = np.random.default_rng(seed)
    G = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(2 * n)
    return np.eye(n) + contract * G if contract else G + 0.5 * np.eye(n)


@pytest.mark.parametrize("passes", [1, 2])
def test_givens_limit_passes_the_emulation_and_rejects_an_unconjugated_sn(passes):
    n, m, nb = 64, 6, 5
    A, B = _dense(n, 51), bb.rand_block((n, nb), 52)
    worst = {}
    for defect in (False, True):
        ar = bb.UnnormalisedArnoldi(A, B, m, passes)
        st = bb.emulate_begin(bb.new_state(m, nb), ar.begin(), 1)
        beta = st["g"][0].real.copy()
        raws, ratios = [], []
        for j in range(m):
            h1, h2, nrm2 = ar.step(j, st["svec"])
            st, _ = bb.emulate_hess_col(st, j, h1, h2, nrm2, 1e-30, 1e-30, 0, 0, sn_not_conj=defect)
            raws.append((h1 if h2 is None else h1 + h2, nrm2))
            gref = bb.givens_reference(st["svec"], raws, m)
            ratios.append(bb.givens_ratios(st, gref, j, beta))
        worst[defect] = np.array(ratios).max(axis=0)
    assert worst[False].max() <= bb.GIVENS_LIMIT, worst[False]
    assert max(worst[True][0], worst[True][2]) > 1e6 * bb.GIVENS_LIMIT, worst[True]
    # the solve: H y = g by back substitution, ys = svec y
    sol = bb.emulate_solve(st, m)
    assert np.array_equal(sol["ys"], sol["svec"][:m].real * sol["y"])
