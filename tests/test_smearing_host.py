"""CPU: the host side of the smeared two-point functions (two_point() with the build-only keys smearing_kappa,
source_smearing_steps and sink_smearing_steps) on schwinger16 -- utils.smear against the explicit line matrices and
its symmetries, the exact expectation of the smeared estimator against the trace formula in all 16 channels, the
validation of the keys, the flows that refuse them, and the engine call trace of the method "two_point_smeared"."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from deflatedmlmc_schwinger_amd import gateway, matrix, stoch_trace, utils
from deflatedmlmc_schwinger_amd.engine import MODE_TWO_POINT_SMEARED, RESOLVED_FETCH, Engine, probe_mode
from deflatedmlmc_schwinger_amd.hierarchy import detect_lattice

HERE = os.path.dirname(os.path.abspath(__file__))
L = 16
N = 2 * L * L
T0 = 3
MOMENTA = [0, 1, 15]
KAPPA = 0.25
SOURCE = 3
SINK = [0, 2, 5]
CHANNELS = ('1', 'g3', 's1', 's2')


def _idx(s, x, t):
    return s * L * L + t * L + x


@pytest.fixture(scope="module")
def lat():
    params = gateway.set_params('schwinger16')
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    found = detect_lattice(A)
    assert found is not None and found[0] == L
    return SimpleNamespace(A=A.toarray(), U1=np.asarray(found[2]).reshape(L, L))      # U1[t][x]


def _line_matrix(U1, t, kappa):
    """(1 + kappa H) / (1 + 2 kappa) on timeslice t as an L x L matrix, entry by entry."""
    M = np.zeros((L, L), dtype=np.complex128)
    for x in range(L):
        M[x, x] += 1.0
        M[x, (x + 1) % L] += kappa * U1[t, x]
        M[x, (x - 1) % L] += kappa * np.conj(U1[t, (x - 1) % L])
    return M / (1.0 + 2.0 * kappa)


def _field(seed, *lead):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(lead + (N,)) + 1j * rng.standard_normal(lead + (N,))


# ---- utils.smear ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [0, 1, 4, 20])
@pytest.mark.parametrize("kappa", [0.25, 1.5])
def test_smear_is_the_power_of_the_line_matrices(lat, kappa, steps):
    """steps = 0 is the identity; steps = 20 > L has gone round the torus."""
    psi = _field(1, 2, 3)
    got = utils.smear(psi, lat.U1, L, kappa, steps)
    assert got.shape == psi.shape and got.dtype == np.complex128
    if steps == 0:
        assert np.array_equal(got, psi)
    ref = np.empty_like(psi)
    for t in range(L):
        P = np.linalg.matrix_power(_line_matrix(lat.U1, t, kappa), steps)
        for s in range(2):
            rows = _idx(s, np.arange(L), t)
            ref[..., rows] = psi[..., rows] @ P.T
    err = np.max(np.abs(got - ref))
    print("smear kappa=%g steps=%d: max |diff| against the matrix power = %.2e" % (kappa, steps, err))
    assert err < 1e-13 * np.max(np.abs(psi))
    # a flat link array and a flat field give the same
    assert np.array_equal(utils.smear(psi[0, 0], lat.U1.ravel(), L, kappa, steps), got[0, 0])


def test_every_line_matrix_is_hermitian(lat):
    for kappa in (0.25, 1.5):
        for t in range(L):
            M = _line_matrix(lat.U1, t, kappa)
            assert np.array_equal(M, M.conj().T)
    # ... and so is S_n as utils.smear applies it: <phi, S psi> = <S phi, psi>
    phi, psi = _field(2), _field(3)
    a = np.vdot(phi, utils.smear(psi, lat.U1, L, 0.25, 7))
    b = np.vdot(utils.smear(phi, lat.U1, L, 0.25, 7), psi)
    assert abs(a - b) < 1e-12 * abs(a)


def test_gauge_covariance(lat):
    """S[U^g](g psi) = g S[U] psi with U^g(x,t) = g(x,t) U(x,t) conj(g(x+1,t))."""
    rng = np.random.default_rng(4)
    g = np.exp(2j * np.pi * rng.random((L, L)))                           # g[t][x]
    Ug = g * lat.U1 * np.conj(np.roll(g, -1, axis=1))
    psi = _field(5, 2)
    gfull = np.concatenate([g.ravel(), g.ravel()])
    for steps in (1, 5, 20):
        lhs = utils.smear(gfull * psi, Ug, L, 0.25, steps)
        rhs = gfull * utils.smear(psi, lat.U1, L, 0.25, steps)
        assert np.max(np.abs(lhs - rhs)) < 1e-13
    assert np.max(np.abs(utils.smear(gfull * psi, lat.U1, L, 0.25, 5) - gfull * utils.smear(psi, lat.U1, L, 0.25, 5))) > 1e-3


def test_constant_field_on_unit_links_is_unchanged():
    const = np.full(N, 0.75 - 0.5j)
    for kappa in (0.25, 1.5):
        out = utils.smear(const, np.ones(L * L), L, kappa, 20)
        assert np.max(np.abs(out - const)) < 1e-14


def test_smear_spin_blind_extended_precision_and_refusals(lat):
    psi = _field(6)
    out = utils.smear(psi, lat.U1, L, 0.25, 4)
    swapped = np.concatenate([psi[L * L:], psi[:L * L]])
    assert np.array_equal(utils.smear(swapped, lat.U1, L, 0.25, 4), np.concatenate([out[L * L:], out[:L * L]]))
    wide = utils.smear(psi.astype(np.clongdouble), lat.U1, L, 0.25, 4)
    assert wide.dtype == np.clongdouble and np.max(np.abs(wide - out)) < 1e-14
    # a subset of the timeslices alone: the lines do not talk to each other
    ts = [0, 7, 15]
    sub = np.ascontiguousarray(psi.reshape(2, L, L)[:, ts]).ravel()
    assert np.array_equal(utils.smear(sub, lat.U1[ts], L, 0.25, 4), out.reshape(2, L, L)[:, ts].ravel())
    with pytest.raises(Exception, match="expected"):
        utils.smear(psi[:-1], lat.U1, L, 0.25, 1)
    with pytest.raises(Exception, match="expected"):
        utils.smear(psi, lat.U1[:-1], L, 0.25, 1)
    with pytest.raises(Exception, match="non-negative integer"):
        utils.smear(psi, lat.U1, L, 0.25, -1)
    with pytest.raises(Exception, match="non-negative integer"):
        utils.smear(psi, lat.U1, L, 0.25, 1.5)


# ---- the exact contraction --------------------------------------------------------------------------------
def test_smeared_contraction_matches_the_trace_formula_in_all_16_channels(lat):
    """E[T^(i)] from the 2 L smeared unit-source columns of the dense inverse, contracted by meson_correlator, against
    C(t, p) = tr[Gamma Ps S_s A^-1 S_n Pt0 e^{+ipy} Gamma' e^{-ipy} Pt0 S_n A^-1 S_s e^{-ipx} Ps] with both propagators
    from the dense inverse (no gamma_3 Hermiticity) and S as dense matrices built from the line matrices."""
    Ainv = np.linalg.inv(lat.A)

    def dense_S(steps):
        S = np.zeros((N, N), dtype=np.complex128)
        for t in range(L):
            P = np.linalg.matrix_power(_line_matrix(lat.U1, t, KAPPA), steps)
            for s in range(2):
                rows = _idx(s, np.arange(L), t)
                S[np.ix_(rows, rows)] = P
        return S

    Sn = dense_S(SOURCE)
    # the estimator's exact expectation: the sum over the L unit noises, smeared with utils.smear
    codes = np.zeros((L, N), dtype=np.int8)
    codes[np.arange(L), T0 * L + np.arange(L)] = 1
    src = utils.smear(utils.slice_sources(codes, L, T0, MOMENTA), lat.U1, L, KAPPA, SOURCE)
    assert np.count_nonzero(src) > 0 and np.all(src.reshape(6, L, 2, L, L)[:, :, :, np.arange(L) != T0] == 0)
    Z = np.einsum('rc,gkc->gkr', Ainv, src)
    E = np.stack([utils.pair_dots(utils.smear(Z, lat.U1, L, KAPPA, s), L, MOMENTA).sum(axis=0) for s in SINK])
    assert E.shape == (len(SINK), len(MOMENTA), 2, 2, 2, 2, L)
    x = np.arange(L)
    worst = 0.0
    for i, s in enumerate(SINK):
        Ss = dense_S(s)
        fwd_all = Ss @ Ainv @ Sn                                           # sink <- source
        bwd_all = Sn @ Ainv @ Ss                                           # source <- sink
        for sink in CHANNELS:
            for source in CHANNELS:
                G, Gp = utils._PAULI[sink], utils._PAULI[source]
                got = utils.meson_correlator(E, sink, source)
                assert got.shape == (len(SINK), len(MOMENTA), L)
                for j, p in enumerate(MOMENTA):
                    ph = np.exp(-2j * np.pi * p * (x[:, None] - x[None, :]) / L)        # [x][y]
                    for t in range(L):
                        ref = 0.0
                        for c in range(2):
                            for d in range(2):
                                for b in range(2):
                                    for a in range(2):
                                        if G[c, d] == 0 or Gp[b, a] == 0:
                                            continue
                                        fwd = fwd_all[np.ix_(_idx(d, x, t), _idx(b, x, T0))]      # [x][y]
                                        bwd = bwd_all[np.ix_(_idx(a, x, T0), _idx(c, x, t))]      # [y][x]
                                        ref += G[c, d] * Gp[b, a] * np.sum(ph * fwd * bwd.T)
                        worst = max(worst, abs(got[i, j, t] - ref))
    pion = utils.meson_correlator(E, 'g3', 'g3')[:, 0]
    print("smeared contraction against the trace formula: max |diff| = %.2e, max |C| = %.2f"
          % (worst, np.max(np.abs(pion))))
    assert worst < 1e-10
    # the pion channel stays real and positive at every sink level, and its total is the control column
    assert np.all(pion.real > 0) and np.max(np.abs(pion.imag)) < 1e-12 * np.max(pion.real)
    cols = stoch_trace._TwoPointSmeared(MOMENTA).columns(E[None])
    assert cols.shape == (1, E.size + 1) and abs(cols[0, -1] - pion[0].sum()) < 1e-12 * abs(cols[0, -1])


# ---- the keys ---------------------------------------------------------------------------------------------
def _params(**extra):
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params.update(extra)
    return utils.trace_params_from_params(params, "hutchinson")


def test_smearing_of_validation():
    assert utils.smearing_of(_params()) is None
    assert utils.smearing_of(_params(source_timeslice=5)) is None
    assert utils.smearing_of(_params(source_timeslice=5, smearing_kappa=0.25)) == dict(kappa=0.25, source=0, sink=[0])
    got = utils.smearing_of(_params(source_timeslice=5, smearing_kappa=1, source_smearing_steps=32,
                                    sink_smearing_steps=[0, 8, 1024]))
    assert got == dict(kappa=1.0, source=32, sink=[0, 8, 1024])
    for key in utils.SMEARING_KEYS:
        assert key in utils._BUILD_KEYS
    bad = [(dict(source_smearing_steps=3), "needs smearing_kappa"),
           (dict(source_timeslice=5, sink_smearing_steps=[0]), "needs smearing_kappa"),
           (dict(smearing_kappa=0.25), "needs source_timeslice"),
           (dict(source_timeslice=5, smearing_kappa=0.0), "positive finite"),
           (dict(source_timeslice=5, smearing_kappa=-0.25), "positive finite"),
           (dict(source_timeslice=5, smearing_kappa=float('inf')), "positive finite"),
           (dict(source_timeslice=5, smearing_kappa=float('nan')), "positive finite"),
           (dict(source_timeslice=5, smearing_kappa="0.25"), "positive finite"),
           (dict(source_timeslice=5, smearing_kappa=0.25, source_smearing_steps=-1), "outside"),
           (dict(source_timeslice=5, smearing_kappa=0.25, source_smearing_steps=1025), "outside"),
           (dict(source_timeslice=5, smearing_kappa=0.25, source_smearing_steps=2.5), "not an integer"),
           (dict(source_timeslice=5, smearing_kappa=0.25, sink_smearing_steps=4), "not a list"),
           (dict(source_timeslice=5, smearing_kappa=0.25, sink_smearing_steps=[]), "between 1 and 4"),
           (dict(source_timeslice=5, smearing_kappa=0.25, sink_smearing_steps=[0, 1, 2, 3, 4]), "between 1 and 4"),
           (dict(source_timeslice=5, smearing_kappa=0.25, sink_smearing_steps=[0, 1.5]), "not an integer"),
           (dict(source_timeslice=5, smearing_kappa=0.25, sink_smearing_steps=[0, 2000]), "outside"),
           (dict(source_timeslice=5, smearing_kappa=0.25, sink_smearing_steps=[4, 2]), "ascend"),
           (dict(source_timeslice=5, smearing_kappa=0.25, sink_smearing_steps=[2, 2]), "ascend")]
    for extra, msg in bad:
        with pytest.raises(Exception, match=msg):
            utils.smearing_of(_params(**extra))


@pytest.mark.parametrize("key,value", [("smearing_kappa", 0.25), ("source_smearing_steps", 3),
                                       ("sink_smearing_steps", [0, 2])])
def test_the_other_flows_refuse_the_keys(key, value):
    for flow, extra in [(stoch_trace.hutchinson, {}), (stoch_trace.mlmc, {}),
                        (stoch_trace.three_point, dict(source_timeslice=5, sink_timeslice=9)),
                        (stoch_trace.lma_two_point, dict(source_timeslice=5))]:
        with pytest.raises(Exception, match="%s belongs to two_point" % key):
            flow(None, _params(**dict(extra, **{key: value})))


def test_two_point_refuses_a_bad_smearing_before_any_setup():
    with pytest.raises(Exception, match="ascend"):
        stoch_trace.two_point(None, _params(source_timeslice=5, smearing_kappa=0.25, sink_smearing_steps=[3, 1]))
    with pytest.raises(Exception, match="lattice operator"):
        stoch_trace.two_point(None, _params(source_timeslice=5, smearing_kappa=0.25))


# ---- the engine call trace --------------------------------------------------------------------------------
TOL = 1e-7
SHAPE = (2, 1, 2, 2, 2, 2, 4)                  # [sink level][momentum][a][b][c][d][t]


class FakeEngine:
    """Records every call; probe k of the stream evaluates to k in every entry of the resolved result."""
    hutch_fetch_resolved = Engine.hutch_fetch_resolved

    def __init__(self):
        self.calls = []
        self._slots = {}
        self._first = None

    def stream_set(self, window):
        self.calls.append(("stream_set",))

    def probes_generate(self, slot, level, nb, pos, kind="z2"):
        self.calls.append(("probes_generate", slot, level, nb, pos, kind))
        self._slots[slot] = np.arange(nb) + pos // 2048

    def probes_select(self, slot):
        self.calls.append(("probes_select", slot))
        self._first = self._slots[slot]

    def hutch_run(self, mode, level, tol, maxiter=1000):
        self.calls.append(("hutch_run", mode, level, tol, maxiter))

    def hutch_fetch(self):
        self.calls.append(("hutch_fetch",))
        k = self._first
        return k.astype(np.complex128), k.astype(np.int32), (0 * k).astype(np.int32)

    def hutch_fetch_two_point_smeared(self):
        self.calls.append(("hutch_fetch_two_point_smeared",))
        return self._first.astype(np.complex128).reshape((-1,) + (1,) * len(SHAPE)) * np.ones(SHAPE)


def test_engine_call_trace_of_the_smeared_method():
    assert MODE_TWO_POINT_SMEARED == 14 and probe_mode("two_point_smeared", 0) == 14
    assert probe_mode("two_point_smeared", 0, skip_level=True) == 14
    assert RESOLVED_FETCH[14] == "hutch_fetch_two_point_smeared"
    levels = [SimpleNamespace(A=SimpleNamespace(shape=(2048, 2048)))]
    mg = SimpleNamespace(engines=[FakeEngine()], ml=SimpleNamespace(levels=levels), skip_level=False)
    obs = stoch_trace._TwoPointSmeared([0])
    source = stoch_trace.DeviceProbes(mg, {'function_params': {'tol': TOL}}, obs.method, 0, "z2", obs.columns)
    assert not source.prefetches                                       # a resolved mode: nothing is drawn ahead
    np.random.seed(1)
    width = int(np.prod(SHAPE)) + 1
    loop = stoch_trace.run_probe_loop(source, 2048, np.full(width, 1e-30), 10, 5, control=width - 1)
    batch = lambda first: [("probes_generate", 0, 0, 5, first * 2048, "z2"), ("probes_select", 0),   # noqa: E731
                           ("hutch_run", 14, 0, TOL, 1000), ("hutch_fetch",), ("hutch_fetch_two_point_smeared",)]
    assert mg.engines[0].calls == [("stream_set",)] + batch(0) + batch(5)
    assert loop["ests"].shape == (10, width)
    # probe k: every T entry is k, the control column is the pion total of sink level 0: 4 diagonal entries x 4 t
    assert np.array_equal(loop["ests"][:, 0].real, np.arange(10))
    assert np.array_equal(loop["ests"][:, -1].real, 16 * np.arange(10))


def test_golden_fixture_is_consistent():
    with open(os.path.join(HERE, "golden", "smeared_two_point128.json")) as f:
        g = json.load(f)
    E = np.array([complex(re, im) for re, im in g["smeared_two_point128"]]).reshape(g["shape"])
    assert E.shape == (2, 1, 2, 2, 2, 2, 128) and E.size == 4096
    assert g["momenta"] == [0] and g["source_timeslice"] == 5 and g["smearing_kappa"] == 0.25
    assert g["source_smearing_steps"] == 8 and g["sink_smearing_steps"] == [0, 8]
    pion = utils.meson_correlator(E, 'g3', 'g3')[:, 0]
    assert np.all(pion.real > 0) and np.max(np.abs(pion.imag)) < 1e-10 * np.max(pion.real)
    for i in range(2):
        assert np.max(np.abs(E[i, 0] - np.conj(E[i, 0].transpose(1, 0, 3, 2, 4)))) < 1e-10 * np.max(np.abs(E[i, 0]))
