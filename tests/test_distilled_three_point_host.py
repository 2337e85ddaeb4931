"""CPU: the host side of the distilled three-point functions (distilled_three_point(), build-only keys
insertion_timeslices and source_momentum) on schwinger16 with the dense inverse -- the generalized
perambulators against seq_dots and three_point_current of the same fields, their Ward identity, the contraction
against the explicit trace with Phi = box diag(omega) box at both ends and against the exact expectation of
three_point() at full rank, the key validation and the refusals of the other flows."""
import os
import re

import numpy as np
import pytest

from deflatedmlmc_schwinger_amd import engine, gateway, hierarchy, matrix, stoch_trace, utils

L = 16
N = 2 * L * L
CHANNELS = ('1', 'g3', 's1', 's2')
SLICES = [(3, 9), (13, 2), (5, 6), (0, 15)]      # as test_three_point_host: plain, wrapped, adjacent, the t + 1 wrap
# (t0, tf, Gamma_f, pf, pi)
CONFIGS = [(3, 9, 's1', 15, 0), (13, 2, 's2', 1, 1), (5, 6, 'g3', 0, 15)]
MOMENTA = [0, 1, 5]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _idx(s, x, t):
    return s * L * L + t * L + x


@pytest.fixture(scope="module")
def dense16():
    params = gateway.set_params('schwinger16')
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    Ld, mass, U1, U2 = hierarchy.detect_lattice(A)
    assert Ld == L
    return dict(Ainv=np.linalg.inv(A.toarray()), U1=np.asarray(U1).reshape(-1), U2=np.asarray(U2).reshape(-1))


def _solutions(dense, V, t0, tf):
    """(Z0, Zf, tau): the solutions of the eigenvector sources on t0 and tf, (2 nev, n) each, and their tau."""
    Z = utils.laph_sources(V, L, [t0, tf]) @ dense['Ainv'].T
    half = Z.shape[0] // 2
    return Z[:half], Z[half:], utils.perambulators_from_solutions(V, Z, L, nsrc=2)


def test_pairs_match_seq_dots_and_the_current():
    """G restricted to the pairs m = n is seq_dots followed by three_point_current of the same fields."""
    rng = np.random.default_rng(11)
    nb = 3
    Zeta = rng.standard_normal((2, nb, N)) + 1j * rng.standard_normal((2, nb, N))
    Z = rng.standard_normal((2, nb, N)) + 1j * rng.standard_normal((2, nb, N))
    U1 = np.exp(2j * np.pi * rng.random(L * L))
    U2 = np.exp(2j * np.pi * rng.random(L * L))
    momenta = [0, 1, 5, 15]
    S = utils.seq_dots(Zeta, Z, U1, U2, L, momenta)                                    # [k][d][j][a][b][f][c][t]
    Jx, Jt = utils.three_point_current(S, 'x'), utils.three_point_current(S, 't')       # [k][j][a][b][t]
    Zf = Zeta.transpose(1, 0, 2).reshape(2 * nb, N)                                    # column (k, a) -> 2 k + a
    Z0 = Z.transpose(1, 0, 2).reshape(2 * nb, N)
    G = utils.generalized_perambulators_from_solutions(Zf, Z0, U1, U2, L, list(range(L)), momenta)
    assert G.shape == (L, len(momenta), 6, 2 * nb, 2 * nb)
    Gr = G.reshape(L, len(momenta), 6, nb, 2, nb, 2)
    scale = np.max(np.abs(G))
    worst = 0.0
    for k in range(nb):
        pair = Gr[:, :, :, k, :, k, :]                                                 # [t][j][comp][a][b]
        local = S[k, 0].transpose(5, 0, 3, 4, 1, 2).reshape(L, len(momenta), 4, 2, 2)   # [t][j][2 f + c][a][b]
        worst = max(worst, np.max(np.abs(pair[:, :, :4] - local)))
        worst = max(worst, np.max(np.abs(pair[:, :, 4] - Jx[k].transpose(3, 0, 1, 2))))
        worst = max(worst, np.max(np.abs(pair[:, :, 5] - Jt[k].transpose(3, 0, 1, 2))))
    print("pairs m = n against seq_dots: max |diff| = %.2e of %.1f" % (worst, scale))
    assert worst < 1e-13 * scale
    # a subset of the timeslices and momenta, in another order, is the same numbers; wide agrees with complex128
    sub = utils.generalized_perambulators_from_solutions(Zf, Z0, U1, U2, L, [15, 0], [5, 0])
    assert np.array_equal(sub, G[[15, 0]][:, [2, 0]])
    wide = utils.generalized_perambulators_from_solutions(Zf, Z0, U1, U2, L, [15, 0], [5, 0], wide=True)
    assert wide.dtype == np.clongdouble and np.max(np.abs(wide - sub)) < 1e-13 * scale
    bound = utils.generalized_perambulator_bounds(Zf, Z0, L, [15, 0])
    assert bound.shape == (2, 6, 2 * nb, 2 * nb) and bound.dtype == np.longdouble and np.all(bound > 0)
    assert np.all(np.abs(wide - sub) <= bound[:, None])


@pytest.mark.parametrize("t0,tf", SLICES)
def test_ward_identity_off_source_and_sink(dense16, t0, tf):
    """W(t) = (1 - omega_q) G[t][4] + G[t][5] - G[t - 1][5] vanishes entry by entry for t outside {t0, tf}."""
    V, _ = utils.laplacian_eigenvectors(dense16['U1'], L, 5)
    Z0, Zf, _ = _solutions(dense16, V, t0, tf)
    G = utils.generalized_perambulators_from_solutions(Zf, Z0, dense16['U1'], dense16['U2'], L, list(range(L)),
                                                       MOMENTA)
    om = np.exp(-2j * np.pi * np.asarray(MOMENTA) / L)[None, :, None, None]
    W = (1 - om) * G[:, :, 4] + G[:, :, 5] - np.roll(G[:, :, 5], 1, axis=0)
    scale = np.max(np.abs(G[:, :, 4:]))
    off = [t for t in range(L) if t not in (t0, tf)]
    print("Ward identity (%d, %d): %.2e off, %.2e on the two slices, max |J| = %.1f"
          % (t0, tf, np.max(np.abs(W[off])), np.max(np.abs(W[[t0, tf]])), scale))
    assert np.max(np.abs(W[off])) < 1e-10 * scale
    assert np.max(np.abs(W[[t0, tf]])) > 1e-3 * scale


def _insertion_matrix(U1, U2, ins, t, q):
    """The insertion of the trace as a dense (n, n) matrix: Gamma x diag(omega_q) on timeslice t for a local one, the
    point-split conserved current H+_mu omega^x U_mu(n) at (n, n + mu) minus H-_mu omega^x conj(U_mu(n)) at (n + mu, n)
    for 'Jx' / 'Jt'."""
    K = np.zeros((N, N), dtype=np.complex128)
    x = np.arange(L)
    om = np.exp(-2j * np.pi * q * x / L)
    if ins in utils._PAULI:
        for f in range(2):
            for c in range(2):
                K[_idx(f, x, t), _idx(c, x, t)] = utils._PAULI[ins][f, c] * om
        return K
    if ins == 'Jx':
        u, xn, tn, hp, hm = U1.reshape(L, L)[t], (x + 1) % L, t, hierarchy._HOP["+x"], hierarchy._HOP["-x"]
    else:
        u, xn, tn, hp, hm = U2.reshape(L, L)[t], x, (t + 1) % L, hierarchy._HOP["+y"], hierarchy._HOP["-y"]
    for f in range(2):
        for c in range(2):
            K[_idx(f, x, t), _idx(c, xn, tn)] += hp[f, c] * om * u
            K[_idx(f, xn, tn), _idx(c, x, t)] -= hm[f, c] * om * u.conj()
    return K


@pytest.mark.parametrize("nev", [1, 5, 16])
def test_contraction_matches_the_explicit_trace(dense16, nev):
    """tr[(Gi x Phi(pi,t0)) A^-1(t0;tf) (Gf x Phi(pf,tf)) A^-1(tf;t) (insertion) A^-1(t;t0)] with Phi(p,t) = box(t)
    diag(omega_p) box(t), all propagators from the dense inverse, for the three configurations, all 16 (Gamma_i, Gamma)
    and both currents; at N = 1 an elemental of non-zero momentum vanishes, so pi = pf = 0 there."""
    Ainv, U1, U2 = dense16['Ainv'], dense16['U1'], dense16['U2']
    V, _ = utils.laplacian_eigenvectors(U1, L, nev)
    x = np.arange(L)
    rows = lambda t: np.concatenate([_idx(0, x, t), _idx(1, x, t)])
    tins = [0, 4, 9, 15]
    for t0, tf, sink, pf, pi in CONFIGS:
        if nev == 1:
            pf = pi = 0
        Z0, Zf, tau = _solutions(dense16, V, t0, tf)
        G = utils.generalized_perambulators_from_solutions(Zf, Z0, U1, U2, L, tins, MOMENTA)
        M = utils.laph_elementals(V, L, [pf, pi])

        def phi(p, t):
            box = V[t].T @ V[t].conj()
            return box @ np.diag(np.exp(-2j * np.pi * p * x / L)) @ box
        mid = Ainv[np.ix_(rows(t0), rows(tf))] @ np.kron(utils._PAULI[sink], phi(pf, tf)) @ Ainv[rows(tf)]
        worst, scale = 0.0, 0.0
        for src in CHANNELS:
            P = Ainv[:, rows(t0)] @ np.kron(utils._PAULI[src], phi(pi, t0)) @ mid           # (n, n)
            for ins in utils.DISTILLED_INSERTIONS:
                got = utils.distilled_three_point_correlator(G, tau[0, tf], M[0, tf], M[1, t0], sink, ins, src)
                assert got.shape == (len(MOMENTA), len(tins))
                for j, q in enumerate(MOMENTA):
                    for i, t in enumerate(tins):
                        ref = np.sum(_insertion_matrix(U1, U2, ins, t, q) * P.T)
                        worst, scale = max(worst, abs(got[j, i] - ref)), max(scale, abs(ref))
        print("N = %d, (%d, %d, %s, %d, %d): max |diff| = %.2e at max |C3| = %.3g"
              % (nev, t0, tf, sink, pf, pi, worst, scale))
        assert scale > 0 and worst < 1e-10 * scale


def test_full_rank_equals_the_exact_expectation_of_three_point(dense16):
    """At N = L the boxes are the identity: with pi = 0 the contraction equals three_point_correlator and
    three_point_current of the exact expectation of three_point() (the L unit noises)."""
    Ainv, U1, U2 = dense16['Ainv'], dense16['U1'], dense16['U2']
    V, _ = utils.laplacian_eigenvectors(U1, L, L)
    for t0, tf, sink, pf in [(3, 9, 's1', 15), (13, 2, 'g3', 0)]:
        codes = np.zeros((L, N), dtype=np.int8)
        codes[np.arange(L), t0 * L + np.arange(L)] = 1
        eta = utils.slice_sources(codes, L, t0, [0])
        z = np.einsum('rc,akc->akr', Ainv, eta)
        zeta = np.einsum('rc,akc->akr', Ainv, utils.seq_sources(z, L, tf, sink, pf))
        S = utils.seq_dots(zeta, z, U1, U2, L, MOMENTA).sum(axis=0)
        Z0, Zf, tau = _solutions(dense16, V, t0, tf)
        G = utils.generalized_perambulators_from_solutions(Zf, Z0, U1, U2, L, list(range(L)), MOMENTA)
        M = utils.laph_elementals(V, L, [pf, 0])
        worst, scale = 0.0, 0.0
        for src in CHANNELS:
            for ins in utils.DISTILLED_INSERTIONS:
                got = utils.distilled_three_point_correlator(G, tau[0, tf], M[0, tf], M[1, t0], sink, ins, src)
                ref = (utils.three_point_correlator(S, ins, src) if ins in utils._PAULI
                       else utils.three_point_current(S, ins[1], src))
                worst, scale = max(worst, np.max(np.abs(got - ref))), max(scale, np.max(np.abs(ref)))
        print("full rank (%d, %d, %s, %d): max |diff| = %.2e at max |C3| = %.3g" % (t0, tf, sink, pf, worst, scale))
        assert worst < 1e-10 * scale


def test_the_correlator_checks_its_arguments():
    G, tau, M = np.zeros((2, 1, 6, 4, 4)), np.zeros((2, 2, 2, 2)), np.zeros((2, 2))
    assert utils.distilled_three_point_correlator(G, tau, M, M, 'g3', 'Jx', '1').shape == (1, 2)
    for bad in (dict(G=np.zeros((2, 1, 5, 4, 4))), dict(tau=np.zeros((2, 2, 3, 2))), dict(M=np.zeros((3, 3))),
                dict(sink='g5'), dict(insertion='Jy'), dict(source='x')):
        a = dict(dict(G=G, tau=tau, M=M, sink='g3', insertion='1', source='1'), **bad)
        with pytest.raises(Exception):
            utils.distilled_three_point_correlator(a['G'], a['tau'], a['M'], a['M'], a['sink'], a['insertion'],
                                                   a['source'])
    with pytest.raises(Exception, match="expected"):
        utils.generalized_perambulators_from_solutions(np.zeros((1, 5)), np.zeros((1, N)), np.ones(L * L),
                                                       np.ones(L * L), L, [0], [0])
    with pytest.raises(Exception, match="links"):
        utils.generalized_perambulators_from_solutions(np.zeros((1, N)), np.zeros((1, N)), np.ones(3), np.ones(L * L),
                                                       L, [0], [0])


# ---- keys and flows -----------------------------------------------------------------------------------------
def _params(**extra):
    params = gateway.set_params('schwinger128')
    params.update(extra)
    return params


BASE = dict(distillation_vectors=32, source_timeslice=5, sink_timeslice=21)


def test_keys_are_validated():
    assert utils.DISTILLED_THREE_POINT_KEYS == ('insertion_timeslices', 'source_momentum')
    assert utils.distilled_three_point_of(_params()) is None
    assert utils.distilled_three_point_of(_params(distillation_vectors=32)) is None
    assert utils.distilled_three_point_of(_params(source_timeslice=5, sink_timeslice=21)) is None
    sel = utils.distilled_three_point_of(_params(**BASE))
    assert sel == dict(nev=32, t0=5, tf=21, sink='g3', pf=0, pi=0, momenta=[0], tins=list(range(128)))
    sel = utils.distilled_three_point_of(_params(**dict(BASE, sink_gamma='s2', sink_momentum=127, source_momentum=3,
                                                        three_point_momenta=[3, 1], insertion_timeslices=[7, 0, 127])))
    assert sel == dict(nev=32, t0=5, tf=21, sink='s2', pf=127, pi=3, momenta=[3, 1], tins=[7, 0, 127])
    assert utils.distilled_three_point_of(_params(**dict(BASE, insertion_timeslices="all")))['tins'] == list(range(128))
    bad = [dict(insertion_timeslices=[]), dict(insertion_timeslices=[3, 3]), dict(insertion_timeslices=[128]),
           dict(insertion_timeslices=[-1]), dict(insertion_timeslices=[2.5]), dict(insertion_timeslices=[True]),
           dict(insertion_timeslices="some"), dict(insertion_timeslices=4), dict(source_momentum=128),
           dict(source_momentum=-1), dict(source_momentum=0.5), dict(source_momentum=True),
           dict(distillation_vectors=129), dict(distillation_vectors=0), dict(distillation_vectors=2.5),
           dict(sink_timeslice=5), dict(sink_gamma='g5'), dict(three_point_momenta=[1, 1]),
           # the loop, displacement and smearing keys and the keys of distilled_two_point()
           dict(timeslice_loops=[0]), dict(link_loops=[0]), dict(x_displacements=[1]), dict(two_point_momenta=[0]),
           dict(smearing_kappa=0.2), dict(source_smearing_steps=2), dict(sink_smearing_steps=[2]),
           dict(source_timeslices=[5]), dict(keep_perambulators=True), dict(distilled_contraction="device")]
    for extra in bad:
        with pytest.raises(Exception):
            utils.distilled_three_point_of(_params(**dict(BASE, **extra)))
    # distillation_of keeps rejecting what it rejects
    with pytest.raises(Exception, match="does not combine with source_timeslice"):
        utils.distillation_of(_params(**dict(BASE, source_timeslices=[5])))


FLOWS = [("hutchinson", {}), ("mlmc", {}), ("two_point", dict(source_timeslice=5)),
         ("three_point", dict(source_timeslice=5, sink_timeslice=9)), ("lma_two_point", dict(source_timeslice=5)),
         ("mlmc_loops", dict(timeslice_loops=[0])), ("deflated_mlmc_loops", dict(timeslice_loops=[0])),
         ("distilled_two_point", dict(distillation_vectors=32, source_timeslices=[5]))]


@pytest.mark.parametrize("flow,extra", FLOWS)
@pytest.mark.parametrize("key,value", [("insertion_timeslices", [4]), ("source_momentum", 1)])
def test_the_other_flows_refuse_the_new_keys(flow, extra, key, value):
    with pytest.raises(Exception, match="%s belongs to distilled_three_point" % key):
        getattr(stoch_trace, flow)(None, _params(**dict(extra, **{key: value})))


def test_distilled_three_point_refuses_before_any_setup():
    with pytest.raises(Exception, match="needs the keys distillation_vectors"):
        stoch_trace.distilled_three_point(None, _params(source_timeslice=5, sink_timeslice=21))
    with pytest.raises(Exception, match="needs the keys distillation_vectors"):
        stoch_trace.distilled_three_point(None, _params(distillation_vectors=32))
    with pytest.raises(Exception, match="does not combine with source_timeslices"):
        stoch_trace.distilled_three_point(None, _params(**dict(BASE, source_timeslices=[5])))
    with pytest.raises(Exception, match="smearing"):
        stoch_trace.distilled_three_point(None, _params(**dict(BASE, smearing_kappa=0.2)))
    with pytest.raises(Exception, match="listed twice"):
        stoch_trace.distilled_three_point(None, _params(**dict(BASE, insertion_timeslices=[1, 1])))
    with pytest.raises(Exception, match="lattice operator"):
        stoch_trace.distilled_three_point(None, _params(**BASE))


def test_the_kernel_class_number():
    header = open(os.path.join(ROOT, "include", "schwinger_hip.h")).read()
    assert re.search(r"#define SW_KCLASS_LAPH_GENERALIZED 28\b", header)
    assert engine.KCLASS_LAPH_GENERALIZED == 28
    for name in ("sw_generalized_perambulators", "sw_apply_laph_generalized"):
        assert name in engine.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % name, header)
