"""CPU: the host side of the device contraction of the distilled two-point functions -- the key
distilled_contraction and the flows that refuse it, distillation_of() as it was, the extended-precision reference and
the rounding-bound helpers of the GPU tests against brute-force index sums on 16^2 with N = 3, and the C header."""
import os
import re

import numpy as np
import pytest

from deflatedmlmc_schwinger_amd import engine, gateway, stoch_trace, utils

HERE = os.path.dirname(os.path.abspath(__file__))
L, N = 16, 3


def _params(**extra):
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params.update(extra)
    return utils.trace_params_from_params(params, "hutchinson")


# ---- the key ----------------------------------------------------------------------------------------------
def test_the_key_is_validated_by_a_helper_of_its_own():
    assert utils.DISTILLED_CONTRACTIONS == ("host", "device")
    assert 'distilled_contraction' in utils.DISTILLATION_KEYS and 'distilled_contraction' in utils._BUILD_KEYS
    assert utils.distilled_contraction_of(_params()) == "host"
    assert utils.distilled_contraction_of(None) == "host"
    base = dict(distillation_vectors=32, source_timeslices=[5])
    assert utils.distilled_contraction_of(_params(**base)) == "host"
    for where in ("host", "device"):
        assert utils.distilled_contraction_of(_params(distilled_contraction=where, **base)) == where
    for bad in ("gpu", "", "Device", 1, True, ["device"]):
        with pytest.raises(Exception, match="distilled_contraction"):
            utils.distilled_contraction_of(_params(distilled_contraction=bad, **base))


def test_distillation_of_returns_what_it_did():
    base = dict(distillation_vectors=32, source_timeslices=[5])
    want = dict(nev=32, t0s=[5], momenta=[0], keep=True)
    assert utils.distillation_of(_params(**base)) == want
    assert utils.distillation_of(_params(distilled_contraction="device", **base)) == want
    assert utils.distillation_of(_params(distilled_contraction="host", **base)) == want
    with pytest.raises(Exception, match="distilled_contraction needs distillation_vectors"):
        utils.distillation_of(_params(distilled_contraction="device"))


def test_a_bad_value_raises_before_any_setup():
    # A = None: anything that reached the set-up would fail on the missing lattice operator instead
    with pytest.raises(Exception, match="distilled_contraction: 'gpu' is none of host, device"):
        stoch_trace.distilled_two_point(None, _params(distillation_vectors=32, source_timeslices=[5],
                                                      distilled_contraction="gpu"))
    with pytest.raises(Exception, match="lattice operator"):
        stoch_trace.distilled_two_point(None, _params(distillation_vectors=32, source_timeslices=[5],
                                                      distilled_contraction="device"))


FLOWS = [("hutchinson", {}), ("mlmc", {}), ("two_point", dict(source_timeslice=5)),
         ("three_point", dict(source_timeslice=5, sink_timeslice=9)), ("lma_two_point", dict(source_timeslice=5)),
         ("mlmc_loops", dict(timeslice_loops=[0])), ("deflated_mlmc_loops", dict(timeslice_loops=[0]))]


@pytest.mark.parametrize("flow,extra", FLOWS)
def test_the_seven_other_flows_refuse_the_key(flow, extra):
    with pytest.raises(Exception, match="distilled_contraction belongs to distilled_two_point"):
        getattr(stoch_trace, flow)(None, _params(**dict(extra, distilled_contraction="device")))


# ---- the reference and the bounds -------------------------------------------------------------------------
def _random(seed, nsrc):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((L, N, L)) + 1j * rng.standard_normal((L, N, L))
    tau = rng.standard_normal((nsrc, L, 2, N, N, 2)) + 1j * rng.standard_normal((nsrc, L, 2, N, N, 2))
    return V, tau


def test_wide_sums_and_bounds_against_brute_force():
    t0s, momenta = [5, 0], [0, 1, 15]
    V, tau = _random(3, len(t0s))
    M = utils.laph_elementals(V, L, momenta)
    T, loops = utils.distilled_sums_wide(tau, M, t0s)
    bT, bl = utils.distilled_contract_bounds(tau, M, t0s)
    assert T.dtype == np.clongdouble and T.shape == (2, 3, 2, 2, 2, 2, L) and loops.shape == (2, 3, 2, 2)
    assert bT.shape == T.shape and bl.shape == loops.shape and np.all(bT > 0) and np.all(bl > 0)
    tw, Mw = tau.astype(np.clongdouble), M.astype(np.clongdouble)
    ta, Ma = np.abs(tau).astype(np.longdouble), np.abs(M).astype(np.longdouble)
    eps = np.longdouble(2.0) ** -52
    rng = np.random.default_rng(8)
    for _ in range(24):
        s, j, a, b, c, d = (int(rng.integers(k)) for k in (2, 3, 2, 2, 2, 2))
        t, t0 = int(rng.integers(L)), t0s[s]
        ref, w = np.clongdouble(0), np.longdouble(0)
        for m1 in range(N):
            for n1 in range(N):
                for m2 in range(N):
                    for n2 in range(N):
                        ref += np.conj(tw[s, t, c, m1, n1, a]) * Mw[j, t, m1, m2] * tw[s, t, d, m2, n2, b] \
                            * np.conj(Mw[j, t0, n1, n2])
                        w += ta[s, t, c, m1, n1, a] * Ma[j, t, m1, m2] * ta[s, t, d, m2, n2, b] * Ma[j, t0, n1, n2]
        assert abs(T[s, j, a, b, c, d, t] - ref) <= 1e-17 * w
        assert abs(bT[s, j, a, b, c, d, t] - (N * N + 2 * N + 16) * eps * w) <= 1e-15 * bT[s, j, a, b, c, d, t]
    for s, t0 in enumerate(t0s):
        for j in range(3):
            for a in range(2):
                for b in range(2):
                    ref = sum(Mw[j, t0, n, m] * tw[s, t0, b, m, n, a] for m in range(N) for n in range(N))
                    w = sum(Ma[j, t0, n, m] * ta[s, t0, b, m, n, a] for m in range(N) for n in range(N))
                    assert abs(loops[s, j, a, b] - ref) <= 1e-17 * w
                    assert abs(bl[s, j, a, b] - (N * N + 8) * eps * w) <= 1e-15 * bl[s, j, a, b]
    # the complex128 functions of the flow compute the same quantities
    T64 = utils.distilled_pair_sums(tau, M, t0s)
    l64 = utils.distilled_loops(tau, M, t0s)
    assert np.all(np.abs(T64 - T) <= bT)
    for s, t0 in enumerate(t0s):
        assert np.all(np.abs(l64[:, :, :, t0] - loops[s]) <= bl[s])


def test_wide_elementals_and_their_bound_against_brute_force():
    momenta = [0, 1, 15]
    V, _ = _random(5, 1)
    Mw = utils.laph_elementals_wide(V, L, momenta)
    bound = utils.laph_elemental_bounds(V, L)
    assert Mw.dtype == np.clongdouble and Mw.shape == (3, L, N, N) and bound.shape == (L, N, N)
    Vw = V.astype(np.clongdouble)
    eps = np.longdouble(2.0) ** -52
    for j, p in enumerate(momenta):
        for t in (0, 7, 15):
            for m in range(N):
                for n in range(N):
                    ref = sum(np.exp(-2j * np.pi * ((p * x) % L) / L) * np.conj(Vw[t, m, x]) * Vw[t, n, x]
                              for x in range(L))
                    w = sum(abs(V[t, m, x]) * abs(V[t, n, x]) for x in range(L))
                    assert abs(Mw[j, t, m, n] - ref) <= 1e-15 * w           # the phase table is double precision
                    assert abs(bound[t, m, n] - (L + 8) * eps * w) <= 1e-15 * bound[t, m, n]
    assert np.all(np.abs(utils.laph_elementals(V, L, momenta) - Mw) <= bound[None])


# ---- the ABI ----------------------------------------------------------------------------------------------
def test_header_and_wrapper_declare_the_new_symbols():
    with open(os.path.join(HERE, "..", "include", "schwinger_hip.h")) as f:
        header = f.read()
    for name in ("sw_set_distillation_momenta", "sw_apply_laph_elementals", "sw_distilled_two_point",
                 "sw_apply_laph_contract"):
        assert re.search(r"\bint %s\(sw_engine\* h" % name, header), name
        assert name in engine.EXPORTED_SYMBOLS
    assert re.search(r"#define SW_KCLASS_LAPH_CONTRACT 27\b", header)
    assert engine.KCLASS_LAPH_CONTRACT == 27 and engine.KCLASS_LAPH == 26
    for method in ("set_distillation_momenta", "laph_elementals", "distilled_two_point", "apply_laph_contract"):
        assert callable(getattr(engine.Engine, method))
