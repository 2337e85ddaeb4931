"""CPU: the host side of the point-split link loops (build-only key link_loops) -- the deflated part
against a dense inverse, the Ward identity of the conserved current and the tie to the local loops on the exact
branches, the NumPy statement of the reduction against a literal loop, exactness over a full Hadamard set, the key's
validation and the golden fixture's own consistency."""
import json
import os

import numpy as np
import pytest

from deflatedmlmc_schwinger_amd import gateway, hierarchy, matrix, stoch_trace, utils

HERE = os.path.dirname(os.path.abspath(__file__))
HP = {'x': hierarchy._HOP["+x"], 't': hierarchy._HOP["+y"]}
HM = {'x': hierarchy._HOP["-x"], 't': hierarchy._HOP["-y"]}


def _exact_branches(M, U1, U2, L, momenta):
    """out[d][p][a][b][t] of a dense matrix M in place of A^-1: F_mu = sum_x e^{-2 pi i p x / L} U_mu(n)
    M[idx(b,n+mu), idx(a,n)], B_mu = sum_x e^{-2 pi i p x / L} conj(U_mu(n)) M[idx(b,n), idx(a,n+mu)]."""
    V = L * L
    site = np.arange(V)
    x, t = site % L, site // L
    nxt = (t * L + (x + 1) % L, ((t + 1) % L) * L + x)
    out = np.zeros((4, len(momenta), 2, 2, L), dtype=np.complex128)
    for j, p in enumerate(momenta):
        ph = np.exp(-2j * np.pi * p * x / L)
        for mu, U in enumerate((U1, U2)):
            for a in range(2):
                for b in range(2):
                    f = ph * U * M[b * V + nxt[mu], a * V + site]
                    g = ph * np.conj(U) * M[b * V + site, a * V + nxt[mu]]
                    out[2 * mu, j, a, b] = f.reshape(L, L).sum(axis=1)
                    out[2 * mu + 1, j, a, b] = g.reshape(L, L).sum(axis=1)
    return out


def _local_blocks(M, L, momenta):
    V = L * L
    site = np.arange(V)
    out = np.zeros((len(momenta), 2, 2, L), dtype=np.complex128)
    for j, p in enumerate(momenta):
        ph = np.exp(-2j * np.pi * p * (site % L) / L)
        for a in range(2):
            for b in range(2):
                out[j, a, b] = (ph * M[b * V + site, a * V + site]).reshape(L, L).sum(axis=1)
    return out


def _current(link, mu):
    """J_mu[p][t] written out: sum_ab (H+_mu[a][b] F_mu - H-_mu[a][b] B_mu)."""
    d = 0 if mu == 'x' else 2
    return np.einsum('ab,pabt->pt', HP[mu], link[d]) - np.einsum('ab,pabt->pt', HM[mu], link[d + 1])


def _ward_residual(link, L, momenta):
    """max over p, t of |(1 - omega_p) J_x(t,p) + J_t(t,p) - J_t(t-1,p)|, and max |J|."""
    Jx, Jt = _current(link, 'x'), _current(link, 't')
    om = np.exp(-2j * np.pi * np.asarray(momenta) / L)[:, None]
    res = (1 - om) * Jx + Jt - np.roll(Jt, 1, axis=1)
    return np.max(np.abs(res)), max(np.max(np.abs(Jx)), np.max(np.abs(Jt)))


def _tie_residual(link0, L1, mass, L):
    """max over t of |(m+4) L_1(t) - sum_ab [H+_x F_x + H-_x B_x + H+_t F_t](t) - sum_ab H-_t B_t(t-1) - 2 L| at
    p = 0: link0[d][a][b][t], L1[t]."""
    hop = (np.einsum('ab,abt->t', HP['x'], link0[0]) + np.einsum('ab,abt->t', HM['x'], link0[1])
           + np.einsum('ab,abt->t', HP['t'], link0[2]) + np.roll(np.einsum('ab,abt->t', HM['t'], link0[3]), 1))
    return np.max(np.abs((mass + 4) * L1 - hop - 2 * L))


@pytest.fixture(scope="module")
def dense16():
    params = gateway.set_params('schwinger16')
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    L, mass, U1, U2 = hierarchy.detect_lattice(A)
    assert L == 16
    A = A.toarray()
    n, k = A.shape[0], 8
    g3 = np.ones(n)
    g3[n // 2:] = -1.0
    lam, V = np.linalg.eigh(g3[:, None] * A)
    low = np.argsort(np.abs(lam))[:k]
    Sy, Vx = lam[low], V[:, low]
    W = g3[:, None] * Vx * np.sign(Sy)[None, :]
    Ainv = np.linalg.inv(A)
    AinvPi = Ainv - (Ainv @ W) @ W.conj().T
    return dict(L=L, mass=mass, U1=U1, U2=U2, g3=g3, Sy=Sy, Vx=Vx, Ainv=Ainv, AinvPi=AinvPi, n=n)


def test_link_sliced_tr1_completes_the_projected_branches_on_16(dense16):
    d = dense16
    momenta = [0, 1, 15]
    tr1 = utils.link_sliced_tr1(d['Vx'], d['Sy'], d['g3'], d['U1'], d['U2'], d['L'], momenta)
    assert tr1.shape == (4, 3, 2, 2, 16)
    exact = _exact_branches(d['Ainv'], d['U1'], d['U2'], d['L'], momenta)
    got = _exact_branches(d['AinvPi'], d['U1'], d['U2'], d['L'], momenta) + tr1
    err = np.max(np.abs(got - exact))
    print("link_sliced_tr1 on 16^2: max |diff| = %.2e, max |tr1| = %.3f" % (err, np.max(np.abs(tr1))))
    assert err < 5e-11
    assert np.max(np.abs(tr1)) > 1e-3
    with pytest.raises(Exception, match="expected 512"):
        utils.link_sliced_tr1(d['Vx'][:-1], d['Sy'], d['g3'][:-1], d['U1'], d['U2'], d['L'], momenta)


def test_ward_identity_and_tie_on_the_exact_branches(dense16):
    d = dense16
    L, momenta = d['L'], [0, 1, 5, 15]
    link = _exact_branches(d['Ainv'], d['U1'], d['U2'], L, momenta)
    res, scale = _ward_residual(link, L, momenta)
    print("Ward residual %.2e at max |J| = %.2f" % (res, scale))
    assert res < 1e-11 * scale
    Jt0 = _current(link, 't')[0]
    assert np.min(np.abs(Jt0)) > 0.1                       # a signal, not 0 = 0
    assert np.max(np.abs(Jt0 - Jt0[0])) < 1e-11 * scale    # p = 0: the charge through a timeslice is conserved
    # utils.conserved_current is the same contraction
    for mu in ('x', 't'):
        assert np.max(np.abs(utils.conserved_current(link, mu) - _current(link, mu))) < 1e-13 * scale
    L1 = _local_blocks(d['Ainv'], L, [0])[0]
    L1 = L1[0, 0] + L1[1, 1]
    tie = _tie_residual(link[:, 0], L1, d['mass'], L)
    print("tie residual %.2e at (m+4) max |L_1| = %.2f" % (tie, (d['mass'] + 4) * np.max(np.abs(L1))))
    assert tie < 1e-11 * (d['mass'] + 4) * np.max(np.abs(L1))


@pytest.mark.parametrize("L", [4, 6])
def test_slice_link_dots_against_a_literal_loop(L):
    rng = np.random.default_rng(40 + L)
    n, nb = 2 * L * L, 3
    momenta = [0, 1, L - 1]
    X = rng.standard_normal((nb, n)) + 1j * rng.standard_normal((nb, n))
    Z = rng.standard_normal((nb, n)) + 1j * rng.standard_normal((nb, n))
    U1 = np.exp(2j * np.pi * rng.random(L * L))
    U2 = np.exp(2j * np.pi * rng.random(L * L))
    idx = lambda s, x, y: s * L * L + y * L + x            # noqa: E731
    ref = np.zeros((nb, 4, len(momenta), 2, 2, L), dtype=np.complex128)
    for k in range(nb):
        for d in range(4):
            U = U1 if d < 2 else U2
            for j, p in enumerate(momenta):
                for a in range(2):
                    for b in range(2):
                        for t in range(L):
                            for x in range(L):
                                xn, tn = ((x + 1) % L, t) if d < 2 else (x, (t + 1) % L)
                                ph = np.exp(-2j * np.pi * p * x / L)
                                u = U[t * L + x]
                                if d % 2 == 0:
                                    ref[k, d, j, a, b, t] += ph * u * np.conj(X[k, idx(a, x, t)]) * Z[k, idx(b, xn, tn)]
                                else:
                                    ref[k, d, j, a, b, t] += (ph * np.conj(u) * np.conj(X[k, idx(a, xn, tn)])
                                                              * Z[k, idx(b, x, t)])
    got = utils.slice_link_dots(X, Z, U1, U2, L, momenta)
    assert got.shape == ref.shape
    for k in range(nb):
        assert np.max(np.abs(got[k] - ref[k])) < 1e-13 * np.sum(np.abs(Z[k]))
    assert np.max(np.abs(ref)) > 0.1
    with pytest.raises(Exception, match="two equal"):
        utils.slice_link_dots(X, Z[:, :-1], U1, U2, L, momenta)
    with pytest.raises(Exception, match="links of"):
        utils.slice_link_dots(X, Z, U1[:-1], U2, L, momenta)


def test_hadamard_probes_give_the_projected_branches_exactly(dense16):
    d = dense16
    n, L, momenta = d['n'], d['L'], [0, 1, 15]
    H = np.array([[1.0]])
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])                    # Sylvester: H H^T = n I
    assert H.shape == (n, n)
    Z = (d['AinvPi'] @ H).T                                # row k = A^-1 Pi h_k
    mean = utils.slice_link_dots(H.T, Z, d['U1'], d['U2'], L, momenta).mean(axis=0)
    exact = _exact_branches(d['AinvPi'], d['U1'], d['U2'], L, momenta)
    err = np.max(np.abs(mean - exact))
    print("Hadamard mean against the exact projected branches: %.2e" % err)
    assert err < 1e-12


def _tp(example="hutchinson", **extra):
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params.update(extra)
    return utils.trace_params_from_params(params, example)


def test_key_is_copied_only_when_present():
    assert 'link_loops' not in _tp()
    assert utils.link_loops_of(_tp()) is None
    assert _tp(link_loops=[0, 3])['link_loops'] == [0, 3]
    assert utils.link_loops_of(_tp(link_loops=[2, 0, 127])) == [2, 0, 127]


@pytest.mark.parametrize("extra,msg", [
    (dict(link_loops=[1, 2]), "contain the momentum 0"),
    (dict(link_loops=[0, 3, 3]), "listed twice"),
    (dict(link_loops=[0, 128]), "outside"),
    (dict(link_loops=[0, -1]), "outside"),
    (dict(link_loops=[0, 1.5]), "not an integer"),
    (dict(link_loops=list(range(9))), "at most 8"),
    (dict(link_loops=[0, 1], x_displacements=[0, 2]), "x_displacements"),
    (dict(link_loops=[0, 1], timeslice_loops=[0]), "timeslice_loops"),
    (dict(link_loops=[0, 1], source_timeslice=3), "source_timeslice"),
    (dict(link_loops=[0, 1], two_point_momenta=[0]), "two_point_momenta"),
])
def test_validation_raises_before_any_engine_call(extra, msg):
    tp = _tp(**extra)
    with pytest.raises(Exception, match=msg):
        utils.link_loops_of(tp)
    with pytest.raises(Exception, match=msg):
        stoch_trace.hutchinson(None, tp)           # no matrix, no engine: the validation comes first


def test_a_matrix_that_is_no_lattice_is_refused_before_any_engine_call():
    import scipy.sparse as sp
    A = sp.identity(2 * 128 * 128, dtype=np.complex128, format="csr") * 2.0 + sp.eye(2 * 128 * 128, k=1) * 0.5
    with pytest.raises(Exception, match="lattice operator"):
        stoch_trace.hutchinson(A, _tp(link_loops=[0]))


@pytest.mark.parametrize("flow", ["mlmc", "mlmc_loops", "deflated_mlmc_loops"])
def test_the_mlmc_flows_refuse_the_key(flow):
    extra = dict(link_loops=[0]) if flow == "mlmc" else dict(link_loops=[0], timeslice_loops=[0])
    with pytest.raises(Exception, match="link_loops"):
        getattr(stoch_trace, flow)(None, _tp("mlmc", **extra))


def test_link_loop_gamma_and_conserved_current_on_a_constructed_array():
    rng = np.random.default_rng(21)
    link = rng.standard_normal((3, 4, 2, 2, 2, 5)) + 1j * rng.standard_normal((3, 4, 2, 2, 2, 5))
    pauli = {'1': np.eye(2), 'g3': np.array([[1, 0], [0, -1]]), 's1': np.array([[0, 1], [1, 0]]),
             's2': np.array([[0, -1j], [1j, 0]])}
    for d, branch in enumerate(utils.LINK_BRANCHES):
        for which, G in pauli.items():
            ref = np.einsum('ab,kpabt->kpt', G, link[:, d])
            got = utils.link_loop_gamma(link, branch, which)
            assert got.shape == (3, 2, 5)
            assert np.max(np.abs(got - ref)) <= 8 * np.finfo(float).eps * np.max(np.abs(link))
    sx = np.array([[0, 1], [1, 0]])
    sy = np.array([[0, -1j], [1j, 0]])
    for mu, s, d in (('x', sx, 0), ('t', sy, 2)):
        ref = (np.einsum('ab,kpabt->kpt', np.eye(2) - s, link[:, d])
               - np.einsum('ab,kpabt->kpt', np.eye(2) + s, link[:, d + 1]))
        got = utils.conserved_current(link, mu)
        assert got.shape == (3, 2, 5)
        assert np.max(np.abs(got - ref)) <= 32 * np.finfo(float).eps * np.max(np.abs(link))
    assert utils.conserved_current(link[0], 'x').shape == (2, 5)
    with pytest.raises(Exception, match="unknown spin matrix"):
        utils.link_loop_gamma(link, 'Fx', 'g5')
    with pytest.raises(Exception, match="unknown branch"):
        utils.link_loop_gamma(link, 'Fz', '1')
    with pytest.raises(Exception, match="unknown direction"):
        utils.conserved_current(link, 'y')
    for bad in (np.zeros((3, 2, 2, 2, 5)), np.zeros((4, 2, 2, 5)), np.zeros((4, 2, 2, 3, 5))):
        with pytest.raises(Exception, match="expected"):
            utils.link_loop_gamma(bad, 'Fx', '1')
        with pytest.raises(Exception, match="expected"):
            utils.conserved_current(bad, 't')


def _golden(name, key):
    with open(os.path.join(HERE, "golden", name)) as f:
        g = json.load(f)
    return g["momenta"], np.array([complex(re, im) for re, im in g[key]]).reshape(g["shape"])


def test_golden_link_loops_satisfy_the_ward_identity_and_the_tie_to_the_loop_fixture():
    momenta, G = _golden("link_loops128.json", "link_loops128")
    assert momenta == [0, 1] and G.shape == (4, 2, 2, 2, 128)
    res, scale = _ward_residual(G, 128, momenta)
    print("golden: Ward residual %.2e at max |J| = %.2f" % (res, scale))
    assert res < 1e-9 * scale
    # the conserved charge of this configuration is small (-0.0021 i) but ten orders above the residual
    assert np.min(np.abs(_current(G, 't')[0])) > 1e-3
    lm, loops = _golden("slice_loops128.json", "slice_loops128")
    L1 = loops[lm.index(0), 0, 0] + loops[lm.index(0), 1, 1]
    tie = _tie_residual(G[:, 0], L1, -0.1320, 128)
    print("golden: tie residual %.2e" % tie)
    assert tie < 1e-8 * 2 * 128
    for a in range(4):
        for b in range(a):
            assert not np.array_equal(G[a], G[b])
