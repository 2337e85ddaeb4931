"""CPU: the host side of the timeslice loops (build-only key timeslice_loops) -- the deflated part tr1[p][a][b][t]
against a dense inverse, the validation, the spin contraction, the unbiased loop-loop correlator and the golden
fixture against the displaced-trace fixture of the same LU."""
import json
import os

import numpy as np
import pytest

from deflatedmlmc_schwinger_amd import gateway, matrix, stoch_trace, utils

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden_loops():
    with open(os.path.join(HERE, "golden", "slice_loops128.json")) as f:
        g = json.load(f)
    return g["momenta"], np.array([complex(re, im) for re, im in g["slice_loops128"]]).reshape(g["shape"])


def _blocks(M, L, momenta):
    """out[p][a][b][t] = sum_x e^{-2 pi i p x / L} M[idx(b,x,t), idx(a,x,t)], idx(s,x,y) = s L^2 + y L + x."""
    out = np.zeros((len(momenta), 2, 2, L), dtype=np.complex128)
    x = np.arange(L)
    for j, p in enumerate(momenta):
        ph = np.exp(-2j * np.pi * p * x / L)
        for a in range(2):
            for b in range(2):
                for t in range(L):
                    out[j, a, b, t] = np.sum(ph * M[b * L * L + t * L + x, a * L * L + t * L + x])
    return out


def test_sliced_tr1_completes_the_projected_blocks_on_16():
    """diag-blocks(A^-1 (I - W W^H)) + tr1 = diag-blocks(A^-1) on every (p, a, b, t), dense algebra, k = 8."""
    params = gateway.set_params('schwinger16')
    A = matrix.loadMatrix(params['matrix'], params['matrix_params']).toarray()
    n, L, k = A.shape[0], 16, 8
    momenta = [0, 1, 15]
    g3 = np.ones(n)
    g3[n // 2:] = -1.0
    lam, V = np.linalg.eigh(g3[:, None] * A)
    low = np.argsort(np.abs(lam))[:k]
    Sy, Vx = lam[low], V[:, low]
    W = g3[:, None] * Vx * np.sign(Sy)[None, :]
    Ainv = np.linalg.inv(A)
    AinvPi = Ainv - (Ainv @ W) @ W.conj().T
    tr1 = utils.sliced_tr1(Vx, Sy, g3, L, momenta)
    assert tr1.shape == (3, 2, 2, L)
    exact = _blocks(Ainv, L, momenta)
    got = _blocks(AinvPi, L, momenta) + tr1
    err = np.max(np.abs(got - exact))
    print("sliced_tr1 on 16^2: max |diff| = %.2e" % err)
    assert err < 2e-11
    assert np.max(np.abs(tr1)) > 1e-3                    # the deflated part is not a rounding-size correction
    # the scalar total at p = 0 is Tr(A^-1)
    total = np.sum(exact[0, 0, 0] + exact[0, 1, 1])
    assert abs(total - 265.8581064657958) < 1e-9 * 265.8581064657958
    # gamma_3 as the sparse matrix the hierarchy holds
    import scipy.sparse as sp
    other = utils.sliced_tr1(Vx, Sy, sp.diags([g3], [0]), L, momenta)
    assert np.max(np.abs(other - tr1)) < 512 * np.finfo(float).eps * np.max(np.abs(tr1))
    with pytest.raises(Exception, match="expected 512"):
        utils.sliced_tr1(Vx[:-1], Sy, g3[:-1], L, momenta)


def _tp(example="hutchinson", **extra):
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params.update(extra)
    return utils.trace_params_from_params(params, example)


def test_key_is_copied_only_when_present():
    assert 'timeslice_loops' not in _tp()
    assert utils.loops_of(_tp()) is None
    assert _tp(timeslice_loops=[0, 3])['timeslice_loops'] == [0, 3]
    assert utils.loops_of(_tp(timeslice_loops=[2, 0, 127])) == [2, 0, 127]


@pytest.mark.parametrize("extra,msg", [
    (dict(timeslice_loops=[1, 2]), "contain the momentum 0"),
    (dict(timeslice_loops=[0, 3, 3]), "listed twice"),
    (dict(timeslice_loops=[0, 128]), "outside"),
    (dict(timeslice_loops=[0, -1]), "outside"),
    (dict(timeslice_loops=[0, 1.5]), "not an integer"),
    (dict(timeslice_loops=list(range(9))), "at most 8"),
    (dict(timeslice_loops=[0, 1], x_displacements=[0, 2]), "x_displacements"),
])
def test_validation_raises_before_any_engine_call(extra, msg):
    tp = _tp(**extra)
    with pytest.raises(Exception, match=msg):
        utils.loops_of(tp)
    with pytest.raises(Exception, match=msg):
        stoch_trace.hutchinson(None, tp)           # no matrix, no engine: the validation comes first


def test_mlmc_rejects_the_key():
    with pytest.raises(Exception, match="timeslice_loops"):
        stoch_trace.mlmc(None, _tp("mlmc", timeslice_loops=[0]))


def test_loop_gamma_against_einsum():
    rng = np.random.default_rng(11)
    loops = rng.standard_normal((5, 3, 2, 2, 7)) + 1j * rng.standard_normal((5, 3, 2, 2, 7))
    pauli = {'1': np.eye(2), 'g3': np.array([[1, 0], [0, -1]]), 's1': np.array([[0, 1], [1, 0]]),
             's2': np.array([[0, -1j], [1j, 0]])}
    for which, G in pauli.items():
        ref = np.einsum('ab,kpabt->kpt', G, loops)
        got = utils.loop_gamma(loops, which)
        assert got.shape == (5, 3, 7)
        assert np.max(np.abs(got - ref)) <= 4 * np.finfo(float).eps * np.max(np.abs(loops))
    assert utils.loop_gamma(loops[0, 0], '1').shape == (7,)
    with pytest.raises(Exception, match="unknown spin matrix"):
        utils.loop_gamma(loops, 'g5')
    with pytest.raises(Exception, match="expected"):
        utils.loop_gamma(np.zeros((3, 2, 7)), '1')


def test_loop_correlator_against_pairs_of_different_probes():
    rng = np.random.default_rng(12)
    N, L = 9, 6
    a = rng.standard_normal((N, L)) + 1j * rng.standard_normal((N, L)) + 3.0
    b = rng.standard_normal((N, L)) + 1j * rng.standard_normal((N, L)) - 2.0j
    ref = np.zeros(L, dtype=np.complex128)
    for D in range(L):
        acc = 0.0
        for t in range(L):
            for k in range(N):
                for m in range(N):
                    if k != m:
                        acc += a[k, (t + D) % L] * b[m, t]
        ref[D] = acc / (N * (N - 1) * L)
    got = utils.loop_correlator(a, b)
    assert got.shape == (L,)
    assert np.max(np.abs(got - ref) / np.abs(ref)) < 1e-12
    # unbiased: with independent unit-variance noise on constant loops the plain product of means would carry
    # the extra sum_k a_k b_k / N^2; the pair form equals the product of means minus exactly that share
    naive = np.array([np.mean(np.roll(a.mean(axis=0), -D) * b.mean(axis=0)) for D in range(L)])
    same = np.array([np.mean(np.sum(np.roll(a, -D, axis=1) * b, axis=0)) for D in range(L)]) / (N * N)
    assert np.max(np.abs(got - (naive - same) * N / (N - 1.0))) < 1e-12 * np.max(np.abs(got))
    with pytest.raises(Exception, match="at least two"):
        utils.loop_correlator(a[:1], b[:1])
    with pytest.raises(Exception, match="two equal"):
        utils.loop_correlator(a, b[:, :-1])


def test_loop_columns_control_is_the_scalar_total():
    rng = np.random.default_rng(13)
    loops = rng.standard_normal((4, 2, 2, 2, 5)) + 1j * rng.standard_normal((4, 2, 2, 2, 5))
    cols = stoch_trace.loop_columns(loops, 1)
    assert cols.shape == (4, 2 * 4 * 5 + 1)
    assert np.array_equal(cols[:, :-1].reshape(loops.shape), loops)
    ref = np.array([sum(loops[k, 1, 0, 0, t] + loops[k, 1, 1, 1, t] for t in range(5)) for k in range(4)])
    assert np.max(np.abs(cols[:, -1] - ref)) < 1e-14 * np.max(np.abs(ref))


def test_golden_loops_agree_with_the_displaced_fixture():
    momenta, G = _golden_loops()
    assert momenta == [0, 1, 2, 3] and G.shape == (4, 2, 2, 128) and G.size == 2048
    with open(os.path.join(HERE, "golden", "displaced_traces128.json")) as f:
        d0 = complex(*json.load(f)["displaced_traces128"][0])
    total = np.sum(G[0, 0, 0] + G[0, 1, 1])
    assert abs(total - d0) < 1e-8
    assert abs(total - 8326.43205953889) < 1e-9 * 8326.43205953889
    assert np.max(np.abs(G[1:])) > 1e-3                  # the momentum blocks carry signal
