"""GPU: the distilled three-point functions (sw_generalized_perambulators, sw_apply_laph_generalized,
k_laph_generalized) -- the kernel alone against its NumPy definition within the derived rounding bounds,
the entry point against sparse LU with its perambulators bit for bit those of sw_perambulators and the Ward identity of
the device's currents, the full-rank generalized perambulators of schwinger128 against the existing three-point
fixture, the distilled_three_point() flow against its own fixture, the ABI's refusals and what a call leaves of the
probe modes."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_gpu_distillation as base  # noqa: E402
from deflatedmlmc_schwinger_amd import gateway, matrix, stoch_trace, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import (KCLASS_LAPH, KCLASS_LAPH_GENERALIZED, Engine,  # noqa: E402
                                               EngineError)

HERE = os.path.dirname(os.path.abspath(__file__))
NCLASSES = 29
# the lattices, their engines, eigenvectors and sparse LU, the random fields and the tight stopping of the
# distillation tests; the fixtures are this module's own instances
setup_cache, p16, fresh16, p128 = base.setup_cache, base.p16, base.fresh16, base.p128
_field, _tight = base._field, base._tight


def _host(p, nev, t0, tf, timeslices, momenta):
    """(G, Z0, Zf) of the host definition from sparse-LU solves."""
    Z = p.solve(utils.laph_sources(p.vectors(nev), p.L, [t0, tf]))
    Z0, Zf = Z[:2 * nev], Z[2 * nev:]
    return (utils.generalized_perambulators_from_solutions(Zf, Z0, p.lattice[2], p.lattice[3], p.L, timeslices,
                                                           momenta), Z0, Zf)


def _work(L, nt, nmom, nbf, nb0):
    """The flops class 28 counts: eight complex products per timeslice and momentum, issued tiles."""
    ct = (nb0 + 15) // 16
    ncg = (ct + 7) // 8
    nt_ = (ct + ncg - 1) // ncg
    return 8.0 * 8.0 * nt * nmom * ((L + 3) // 4 * 4) * (16.0 * ((nbf + 15) // 16)) * (16.0 * nt_ * ncg)


# ---- 1. the kernel alone ------------------------------------------------------------------------------------
TS16 = [0, 15, 7]


@pytest.mark.parametrize("nbf,nb0", [(1, 1), (3, 130), (33, 17), (70, 64)],
                         ids=["one-entry", "ragged-two-column-groups", "three-row-tiles", "two-row-groups"])
@pytest.mark.parametrize("momenta", [[0, 1, 15], [5]], ids=["q0-1-15", "q5"])
def test_kernel_16_within_its_bounds(p16, nbf, nb0, momenta):
    """Random complex fields; every entry within its bound of the extended-precision definition; a zero row or column
    (where another one remains) gives exact zeros; one timeslice or one momentum alone, and a column alone, are the
    same bits; two calls agree."""
    p = p16
    Zf, Z0 = _field(100 + nbf, nbf, p.n), _field(200 + nb0, nb0, p.n)
    if nbf > 1:
        Zf[nbf // 2] = 0.0
    if nb0 > 1:
        Z0[nb0 - 1] = 0.0
    out = p.eng.apply_laph_generalized(Zf, Z0, TS16, momenta)
    assert out.shape == (3, len(momenta), 6, nbf, nb0)
    ref = utils.generalized_perambulators_from_solutions(Zf, Z0, p.lattice[2], p.lattice[3], p.L, TS16, momenta,
                                                         wide=True)
    bound = utils.generalized_perambulator_bounds(Zf, Z0, p.L, TS16)[:, None]
    err = np.abs(out - ref)
    live = np.broadcast_to(bound > 0, err.shape)
    assert live.any() and np.all(err[~live] == 0)
    worst = float(np.max((err / np.where(bound > 0, bound, 1))[live]))
    print("generalized kernel n=%d %d x %d q=%s: worst |err| / bound = %.3f" % (p.n, nbf, nb0, momenta, worst))
    assert worst <= 1.0
    assert nbf == 1 or np.all(out[:, :, :, nbf // 2, :] == 0)
    assert nb0 == 1 or np.all(out[:, :, :, :, nb0 - 1] == 0)
    assert np.count_nonzero(out) == out.size * (nbf - (nbf > 1)) * (nb0 - (nb0 > 1)) // (nbf * nb0)
    assert np.array_equal(p.eng.apply_laph_generalized(Zf, Z0, TS16, momenta), out)
    assert np.array_equal(p.eng.apply_laph_generalized(Zf, Z0, [7], momenta), out[2:3])
    if 1 in momenta:
        alone = p.eng.apply_laph_generalized(Zf, Z0, TS16, [1])
        assert np.array_equal(alone[:, 0], out[:, momenta.index(1)])
    if nbf == 70:
        one = p.eng.apply_laph_generalized(Zf[37], Z0, TS16, momenta)
        assert one.shape == (3, len(momenta), 6, 1, nb0) and np.array_equal(one[:, :, :, 0], out[:, :, :, 37])
        col = p.eng.apply_laph_generalized(Zf, Z0[37], TS16, momenta)
        assert np.array_equal(col[..., 0], out[..., 37])


def test_kernel_128_four_row_tiles(p128):
    """nbf = nb0 = 64 on schwinger128, the t + 1 wrap included, against the complex128 definition: twice the bound
    (the reference carries a rounding error of its own, no larger than the device's).  Class 28 counts the launches
    and the work."""
    p = p128
    ts, momenta, nb = [0, 127, 64, 5], [0, 3], 64
    Zf, Z0 = _field(31, nb, p.n), _field(32, nb, p.n)
    p.eng.set_profiling(True)
    p.eng.timers_reset()
    try:
        out = p.eng.apply_laph_generalized(Zf, Z0, ts, momenta)
        ms, launches = p.eng.kernel_stats(KCLASS_LAPH_GENERALIZED)
        work = p.eng.kernel_work(KCLASS_LAPH_GENERALIZED)
        dots = p.eng.timers()['dots']
    finally:
        p.eng.set_profiling(False)
    assert launches == 2 and ms > 0 and dots >= ms
    assert work == _work(p.L, len(ts), len(momenta), nb, nb) == 8.0 * 8 * 4 * 2 * 128 * 64 * 64
    ref = utils.generalized_perambulators_from_solutions(Zf, Z0, p.lattice[2], p.lattice[3], p.L, ts, momenta)
    bound = utils.generalized_perambulator_bounds(Zf, Z0, p.L, ts)[:, None]
    worst = float(np.max(np.abs(out - ref) / bound))
    print("generalized kernel n=%d 64 x 64: worst |err| / bound against complex128 = %.3f" % (p.n, worst))
    assert worst <= 2.0
    assert np.array_equal(p.eng.apply_laph_generalized(Zf, Z0, ts, momenta), out)


# ---- 2. the entry point against sparse LU -----------------------------------------------------------------------
@pytest.mark.parametrize("nev,t0,tf", [(5, 13, 2), (16, 3, 9)], ids=["N5-wrapped", "N16-full-rank"])
def test_generalized_perambulators_16(p16, nev, t0, tf):
    p, L = p16, p16.L
    ts, momenta, tol = list(range(L)), [0, 1, 5], 1e-12
    V = p.vectors(nev)
    p.eng.set_distillation(V)
    p.eng.set_profiling(True)
    p.eng.timers_reset()
    try:
        G, tau, iters = _tight(p, lambda: p.eng.generalized_perambulators(t0, tf, ts, momenta, tol))
        _, launches = p.eng.kernel_stats(KCLASS_LAPH_GENERALIZED)
        work = p.eng.kernel_work(KCLASS_LAPH_GENERALIZED)
        _, launches26 = p.eng.kernel_stats(KCLASS_LAPH)
        work26 = p.eng.kernel_work(KCLASS_LAPH)
        p.eng.timers_reset()
        tau_ref, iters_ref = _tight(p, lambda: p.eng.perambulators([t0, tf], tol))
        _, peramb26 = p.eng.kernel_stats(KCLASS_LAPH)
        peramb_work26 = p.eng.kernel_work(KCLASS_LAPH)
    finally:
        p.eng.set_profiling(False)
    assert G.shape == (L, 3, 6, 2 * nev, 2 * nev)
    assert np.array_equal(tau, tau_ref) and np.array_equal(iters, iters_ref)           # bit for bit
    assert launches == 2 and work == _work(L, L, 3, 2 * nev, 2 * nev)
    assert launches26 == peramb26 == 2 and work26 == peramb_work26
    lean, none, _ = _tight(p, lambda: p.eng.generalized_perambulators(t0, tf, ts, momenta, tol, keep_tau=False))
    assert none is None and np.array_equal(lean, G)
    ref, Z0, Zf = _host(p, nev, t0, tf, ts, momenta)
    err = np.max(np.abs(G - ref)) / np.max(np.abs(ref))
    print("generalized perambulators n=%d N=%d (%d, %d): max |G - LU| / max |G| = %.2e, iterations %d..%d"
          % (p.n, nev, t0, tf, err, iters.min(), iters.max()))
    assert err < 2e-10
    # Ward identity of the device's currents off source and sink.  A z = eta + r with |r| <= tol |eta| = tol, so
    # W(t) = sum_x omega^x (conj(z_f) g3 r_0 - conj(r_f) g3 z_0) on the timeslice: |W| <= tol (|z_f| + |z_0|), plus
    # the rounding of the three entries
    om = np.exp(-2j * np.pi * np.asarray(momenta) / L)[None, :, None, None]
    W = (1 - om) * G[:, :, 4] + G[:, :, 5] - np.roll(G[:, :, 5], 1, axis=0)
    bound = utils.generalized_perambulator_bounds(Zf, Z0, L, ts).astype(np.float64)
    allowed = (tol * (np.linalg.norm(Zf, axis=1)[:, None] + np.linalg.norm(Z0, axis=1)[None, :])[None, None]
               + (np.abs(1 - om) * bound[:, None, 4] + bound[:, None, 5] + np.roll(bound[:, None, 5], 1, axis=0)))
    off = [t for t in range(L) if t not in (t0, tf)]
    ratio = float(np.max(np.abs(W[off]) / allowed[off]))
    print("Ward identity on the device's G: worst |W| / allowed off source and sink = %.3f; on them |W| up to %.2e"
          % (ratio, np.max(np.abs(W[[t0, tf]]))))
    assert ratio <= 1.0


# ---- 3. schwinger128 at full rank against the existing three-point fixture -------------------------------------
def test_full_rank_128_reproduces_the_three_point_fixture(p128):
    """N = L = 128: the boxes are the identity, so the contraction with Gamma_i = Gamma_f = g3, pi = pf = 0 is the exact
    expectation of tests/golden/three_point128.json, all six rows.  Two solve blocks of 256 columns; G is 100 MB."""
    p = p128
    with open(os.path.join(HERE, "golden", "three_point128.json")) as f:
        g = json.load(f)
    golden = np.array([complex(re, im) for re, im in g["three_point128"]]).reshape(g["shape"])
    assert golden.shape == (6, 2, 128) and g["momenta"] == [0, 1] and g["rows"] == list(utils.DISTILLED_INSERTIONS)
    assert (g["source_timeslice"], g["sink_timeslice"], g["sink_gamma"], g["sink_momentum"], g["source_gamma"]) \
        == (5, 21, 'g3', 0, 'g3')
    ts = [4, 5, 6, 13, 20, 21, 22, 70]
    V = p.vectors(128)
    p.eng.set_distillation(V)
    G, tau, iters = _tight(p, lambda: p.eng.generalized_perambulators(5, 21, ts, [0, 1], 1e-12))
    assert G.shape == (8, 2, 6, 256, 256) and tau.shape == (2, 128, 2, 128, 128, 2) and iters.min() >= 1
    M = [np.einsum('mx,nx->mn', V[t].conj(), V[t]) for t in (21, 5)]
    for r, ins in enumerate(utils.DISTILLED_INSERTIONS):
        got = utils.distilled_three_point_correlator(G, tau[0, 21], M[0], M[1], 'g3', ins, 'g3')
        err = np.max(np.abs(got - golden[r][:, ts])) / np.max(np.abs(golden[r]))
        print("full rank n=%d insertion %s: max |C3 - golden| / max |golden row| = %.2e" % (p.n, ins, err))
        assert err < 2e-10


# ---- 4. the flow --------------------------------------------------------------------------------------------
KEYS = {'three_point', 'generalized_perambulators', 'perambulators', 'eigenvalues', 'momenta', 'insertion_timeslices',
        'source_timeslice', 'sink_timeslice', 'sink_gamma', 'sink_momentum', 'source_momentum',
        'distillation_vectors', 'function_iters', 'solves', 'solve_s'}


def _flow(name, **extra):
    params = gateway.set_params(name)
    params['function_tol'] = 1e-12
    params['stop_factor'] = 0.1
    params.update(extra)
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    return stoch_trace.distilled_three_point(A, utils.trace_params_from_params(params, "hutchinson"))


def test_flow_128_against_the_fixture(capsys):
    """C3 is linear in G with weights that depend on Gamma_i through factors of modulus one only, so an error of G
    shows at the same size in all four Gamma_i of an insertion: the bar is 2e-10 of the insertion's largest value."""
    with open(os.path.join(HERE, "golden", "distilled_three_point128.json")) as f:
        g = json.load(f)
    flat = np.array(g["distilled_three_point128"])                                    # re, im, re, im, ...
    golden = (flat[0::2] + 1j * flat[1::2]).reshape(g["shape"])
    assert golden.shape == (6, 4, 2, 128) and g["insertions"] == list(utils.DISTILLED_INSERTIONS)
    res = _flow('schwinger128', distillation_vectors=g["distillation_vectors"],
                source_timeslice=g["source_timeslice"], sink_timeslice=g["sink_timeslice"],
                sink_gamma=g["sink_gamma"], three_point_momenta=g["momenta"])
    capsys.readouterr()
    assert set(res) == KEYS
    assert res['three_point'].shape == (6, 4, 2, 128) and res['insertion_timeslices'] == list(range(128))
    assert res['generalized_perambulators'].shape == (128, 2, 6, 64, 64)
    assert res['perambulators'].shape == (2, 128, 2, 32, 32, 2) and res['eigenvalues'].shape == (128, 32)
    assert (res['source_timeslice'], res['sink_timeslice'], res['sink_gamma'], res['sink_momentum'],
            res['source_momentum'], res['momenta'], res['distillation_vectors']) == (5, 21, 'g3', 0, 0, [0, 1], 32)
    assert res['solves'] == 128 and res['function_iters'] >= 128 and res['solve_s'] > 0
    for i, ins in enumerate(utils.DISTILLED_INSERTIONS):
        err = np.max(np.abs(res['three_point'][i] - golden[i])) / np.max(np.abs(golden[i]))
        print("distilled_three_point N=32 (5, 21) insertion %s: max |C3 - golden| / max |golden| = %.2e" % (ins, err))
        assert err < 2e-10


def test_flow_16_equals_the_host_chain(p16, capsys):
    """schwinger16, N = 5, a wrapped interval, non-zero momenta at both ends, a subset of the timeslices."""
    p, nev, t0, tf, tins, momenta = p16, 5, 13, 2, [1, 13, 0, 15, 2, 7], [1, 0, 5]
    res = _flow('schwinger16', distillation_vectors=nev, source_timeslice=t0, sink_timeslice=tf, sink_gamma='s2',
                sink_momentum=1, source_momentum=15, three_point_momenta=momenta, insertion_timeslices=tins)
    capsys.readouterr()
    assert set(res) == KEYS and res['three_point'].shape == (6, 4, 3, 6) and res['insertion_timeslices'] == tins
    V = p.vectors(nev)
    G, Z0, Zf = _host(p, nev, t0, tf, tins, momenta)
    tau = utils.perambulators_from_solutions(V, np.concatenate([Z0, Zf]), p.L, nsrc=2)
    M = utils.laph_elementals(V, p.L, [1, 15])
    for i, ins in enumerate(utils.DISTILLED_INSERTIONS):
        ref = np.stack([utils.distilled_three_point_correlator(G, tau[0, tf], M[0, tf], M[1, t0], 's2', ins, s)
                        for s in ('1', 'g3', 's1', 's2')])
        err = np.max(np.abs(res['three_point'][i] - ref)) / np.max(np.abs(ref))
        print("distilled_three_point n=%d N=%d insertion %s: max |C3 - host chain| / max = %.2e" % (p.n, nev, ins, err))
        assert err < 2e-10
    assert np.max(np.abs(res['generalized_perambulators'] - G)) < 2e-10 * np.max(np.abs(G))


# ---- 5. refusals and isolation --------------------------------------------------------------------------------
def _counts(eng):
    return [eng.kernel_stats(c)[1] for c in range(NCLASSES)] + [eng.launch_count()]


def test_refusals_launch_nothing(p16):
    p, eng = p16, p16.eng
    ok = dict(t0=3, tf=9, timeslices=[0, 1], momenta=[0, 1], tol=1e-12, maxiter=100)

    def call(**change):
        return eng.generalized_perambulators(**dict(ok, **change))
    Z = _field(1, 2, p.n)
    eng.set_distillation(None)
    eng.set_profiling(True)
    eng.timers_reset()
    try:
        before = _counts(eng)
        assert len(before) == NCLASSES + 1
        with pytest.raises(EngineError, match="out of range"):
            eng.kernel_stats(NCLASSES)
        with pytest.raises(EngineError, match="no distillation registration"):
            call()
        eng.set_distillation(p.vectors(5))
        for change, msg in [(dict(t0=16), "outside"), (dict(t0=-1), "outside"), (dict(tf=16), "outside"),
                            (dict(tf=3), "listed twice"), (dict(timeslices=[]), "outside"),
                            (dict(timeslices=[4, 4]), "listed twice"), (dict(timeslices=[16]), "outside"),
                            (dict(timeslices=[-1]), "outside"), (dict(momenta=[]), "between 1 and"),
                            (dict(momenta=list(range(9))), "between 1 and"), (dict(momenta=[1, 1]), "listed twice"),
                            (dict(momenta=[16]), "outside"), (dict(maxiter=0), "maxiter")]:
            with pytest.raises(EngineError, match=msg):
                call(**change)
        t = np.array([0, 1], dtype=np.int32)
        rc = eng._lib.sw_generalized_perambulators(eng._h, 3, 9, 2, t.ctypes.data, 2, t.ctypes.data, 1e-12, 100, None,
                                                   None, None)
        assert rc != 0 and b"null output" in eng._lib.sw_last_error(eng._h)
        # the kernel alone: the same lists, and the column counts
        for tl, ml, msg in [([], [0], "outside"), ([2, 2], [0], "listed twice"), ([0], [], "between 1 and"),
                            ([0], [3, 3], "listed twice"), ([0], [-1], "outside")]:
            with pytest.raises(EngineError, match=msg):
                eng.apply_laph_generalized(Z, Z, tl, ml)
        with pytest.raises(EngineError, match="columns outside"):
            eng.apply_laph_generalized(_field(2, 257, p.n), Z, [0], [0])
        assert _counts(eng) == before                                      # nothing was launched by any refusal
        G, _, _ = call(maxiter=1000)
        assert G.shape == (2, 2, 6, 10, 10) and _counts(eng)[KCLASS_LAPH_GENERALIZED] == 2
    finally:
        eng.set_profiling(False)


def test_engines_without_a_lattice_or_a_finalised_hierarchy_are_refused(p16):
    Z = _field(1, 2, p16.n)
    eng = Engine(p16.eng.device)
    try:
        eng.hier_begin(0, 1)
        eng.set_csr(0, 0, p16.A)
        launches = eng.launch_count()
        with pytest.raises(EngineError, match="lattice level 0"):
            eng.apply_laph_generalized(Z, Z, [0], [0])
        assert eng.launch_count() == launches
    finally:
        eng.close()
    eng = Engine(p16.eng.device)
    try:
        L, mass, U1, U2 = p16.lattice
        eng.hier_begin(0, 1)
        eng.set_lattice(0, L, mass, U1, U2)
        eng.set_distillation(p16.vectors(5))
        launches = eng.launch_count()
        with pytest.raises(EngineError, match="not finalised"):
            eng.generalized_perambulators(3, 9, [0], [0], 1e-12, 100)
        assert eng.launch_count() == launches
        # the kernel alone needs the lattice and its links only
        out = eng.apply_laph_generalized(Z, Z, [15], [1])
        ref = utils.generalized_perambulators_from_solutions(Z, Z, U1, U2, L, [15], [1])
        assert np.max(np.abs(out - ref)) < 1e-12 * np.max(np.abs(ref))
    finally:
        eng.close()


def test_a_call_leaves_the_probe_modes_alone(p16, fresh16):
    """A mode-6 batch after a call equals, bit for bit, that of an engine with the same hierarchy that never made one;
    the fetches of the other modes still return their own last batches; two calls agree bit for bit."""
    p, fresh = p16, fresh16
    np.random.seed(23)
    codes = utils.draw_probes(5, p.n, "z4")
    fresh.eng.set_two_point(3, [0, 15])
    ref6, itf6, _ = fresh.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
    ts, momenta = list(range(16)), [0, 1]
    try:
        p.eng.set_two_point(3, [0, 15])
        p.eng.set_loop_momenta([0, 1])
        p.eng.set_three_point(3, 9, 'g3', 0, [0, 1])
        before6, _, _ = p.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
        assert np.array_equal(before6, ref6)
        loops5, _, _ = p.eng.hutch_batch_loops(0, utils.draw_probes(5, p.n, "z2"), 1e-12, 1000)
        est = p.eng.hutch_fetch()
        p.eng.set_distillation(p.vectors(16))
        G, tau, iters = p.eng.generalized_perambulators(3, 9, ts, momenta, 1e-12)
        assert np.array_equal(p.eng.hutch_fetch_two_point(), ref6)
        assert np.array_equal(p.eng.hutch_fetch_loops(), loops5)
        for a, b in zip(p.eng.hutch_fetch(), est):
            assert np.array_equal(a, b)
        T6, itf, _ = p.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
        assert np.array_equal(T6, ref6) and np.array_equal(itf, itf6)
        G2, tau2, iters2 = p.eng.generalized_perambulators(3, 9, ts, momenta, 1e-12)
        assert np.array_equal(G2, G) and np.array_equal(tau2, tau) and np.array_equal(iters2, iters)
    finally:
        p.eng.set_two_point(0, None)
        p.eng.set_loop_momenta(None)
        p.eng.set_three_point(0, 1, 'g3', 0, None)
        fresh.eng.set_two_point(0, None)
