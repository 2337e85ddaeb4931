"""GPU: the distilled two-point functions contracted on the device (sw_set_distillation_momenta,
sw_apply_laph_elementals, sw_distilled_two_point, sw_apply_laph_contract) -- the elementals and the three contraction
kernels within their derived rounding bounds of extended precision, bit-for-bit repeatability and independence of a
source from its block, the whole call against sw_perambulators and sparse LU, the ABI's refusals and what a call leaves
of the probe modes, full rank on schwinger128 against the two-point fixture, and the flow with
distilled_contraction = "device" against its fixture and against the host path."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import gateway, hierarchy, matrix, stoch_trace, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import KCLASS_LAPH, KCLASS_LAPH_CONTRACT, Engine, EngineError  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG  # noqa: E402
from oracle import ref_path as rp  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MOMENTA16 = [0, 1, 15]


class Problem:
    """One lattice with its hierarchy on the GPU, no deflation vectors, its Laplacian eigenvectors (all L of them) and
    its sparse LU; cache_dir: the set-up cache, so that two engines compared bit for bit get the same hierarchy."""

    def __init__(self, name, cache_dir=None):
        saved = os.environ.get("SW_CACHE_DIR")
        if cache_dir is not None:
            os.environ["SW_CACHE_DIR"] = str(cache_dir)
        try:
            self._setup(name)
        finally:
            if cache_dir is not None:
                if saved is None:
                    del os.environ["SW_CACHE_DIR"]
                else:
                    os.environ["SW_CACHE_DIR"] = saved

    def _setup(self, name):
        params = gateway.set_params(name)
        params['function_tol'] = 1e-12
        self.A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
        self.tp = utils.trace_params_from_params(params, "hutchinson")
        self.tp['solver_cfg'] = dict(hierarchy.DEFAULT_SOLVER_CFG)
        self.mg = MG(self.A)
        self.mg.setup(dof=self.tp['dof'], aggrs=self.tp['aggrs'], max_levels=self.tp['max_nr_levels'], dim=2,
                      acc_eigvs=self.tp['accuracy_mg_eigvs'], sys_type='schwinger', params=self.tp)
        self.mg.total_levels = len(self.mg.ml.levels)
        self.L = int(self.tp['latt_dims'][0])
        self.n = self.A.shape[0]
        self.eng = self.mg.engine
        self.lattice = hierarchy.detect_lattice(self.A)
        self.V, self.lam = utils.laplacian_eigenvectors(self.lattice[2], self.L, self.L)
        self._lu = None

    def vectors(self, nev):
        return np.ascontiguousarray(self.V[:, :nev])

    def random_vectors(self, nev, seed):
        """Complex and not orthonormal: the engine takes any V, and nothing cancels in the elementals."""
        rng = np.random.default_rng(seed)
        return rng.standard_normal((self.L, nev, self.L)) + 1j * rng.standard_normal((self.L, nev, self.L))

    def solve(self, src):
        if self._lu is None:
            self._lu = rp.LUSolver(self.A)
        return np.asarray(self._lu(np.ascontiguousarray(src.T))).T


@pytest.fixture(scope="module")
def setup_cache(tmp_path_factory):
    return tmp_path_factory.mktemp("setup_cache")


@pytest.fixture(scope="module")
def p16(setup_cache):
    p = Problem('schwinger16', setup_cache)
    yield p
    p.eng.set_distillation(None)


@pytest.fixture(scope="module")
def fresh16(setup_cache, p16):          # after p16: reads the set-up products p16 computed; never runs a contraction
    return Problem('schwinger16', setup_cache)


@pytest.fixture(scope="module")
def p128():
    p = Problem('schwinger128')
    yield p
    p.eng.set_distillation(None)


def _tau(seed, nsrc, L, nev):
    rng = np.random.default_rng(seed)
    shape = (nsrc, L, 2, nev, nev, 2)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _tight(p, body):
    saved = p.eng.get_option("stop_factor")
    p.eng.set_option("stop_factor", 0.1)
    try:
        return body()
    finally:
        p.eng.set_option("stop_factor", saved)


def _fraction(err, bound):
    """max |err| / bound; where the bound is zero nothing may be off."""
    err, bound = np.asarray(err), np.asarray(bound)
    assert np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def _chunks(t0s, nev):
    size = max(1, 256 // (2 * nev))
    return [t0s[i:i + size] for i in range(0, len(t0s), size)]


def _work(L, nev, momenta, blocks):
    """sw_kernel_work(27) of contractions of blocks of ns sources each, as the header states it."""
    ld, K4 = (nev + 15) // 16 * 16, (nev + 3) // 4 * 4
    total = 0.0
    for ns in blocks:
        ncols = (2 * nev * ns + 63) // 64 * 64
        total += len(momenta) * 8.0 * (2 * L * ncols * ld * K4 + 4 * L * ns * ld * ld * K4 + 16 * L * ns * nev * nev
                                       + 4 * ns * nev * nev)
    return total


# ---- 1. the elementals ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nev", [1, 5, 16])
@pytest.mark.parametrize("kind", ["random", "laplacian"])
def test_elementals_16(p16, kind, nev):
    """One padded tile (N = 1, 5) and a full one; momentum 0 (no phase table), 1 and L - 1."""
    p = p16
    V = p.random_vectors(nev, 40 + nev) if kind == "random" else p.vectors(nev)
    p.eng.set_distillation(V)
    p.eng.set_profiling(True)
    p.eng.timers_reset()
    try:
        p.eng.set_distillation_momenta(MOMENTA16)
        _, launches = p.eng.kernel_stats(KCLASS_LAPH_CONTRACT)
        work = p.eng.kernel_work(KCLASS_LAPH_CONTRACT)
    finally:
        p.eng.set_profiling(False)
    assert launches == 3 and work == 3 * 8.0 * p.L * p.L * 16 * 16
    M = p.eng.laph_elementals()
    assert M.shape == (3, p.L, nev, nev)
    ref = utils.laph_elementals_wide(V, p.L, MOMENTA16)
    worst = _fraction(np.abs(M - ref), np.broadcast_to(utils.laph_elemental_bounds(V, p.L), M.shape))
    print("elementals n=%d %s N=%d: worst |err| / bound = %.3f" % (p.n, kind, nev, worst))
    assert worst <= 1.0
    assert np.max(np.abs(M)) > 0
    assert np.array_equal(p.eng.laph_elementals(), M)
    p.eng.set_distillation_momenta(MOMENTA16)                              # computed again: the same bits
    assert np.array_equal(p.eng.laph_elementals(), M)
    p.eng.set_distillation_momenta([15])                                   # a momentum's values do not depend on the list
    assert np.array_equal(p.eng.laph_elementals()[0], M[2])
    p.eng.set_distillation(V)                                              # every registration drops the momenta
    with pytest.raises(EngineError, match="no distillation momenta"):
        p.eng.laph_elementals()


# ---- 2. the contraction kernels alone, schwinger16 --------------------------------------------------------
T0S = {"one": [5], "three": [0, 15, 3], "all": list(range(16))}


@pytest.mark.parametrize("nev", [1, 5, 16])
@pytest.mark.parametrize("which", ["one", "three", "all"])
def test_contract_16(p16, which, nev):
    """N = 16 on all timeslices is two blocks of eight sources; N = 5 on all is 160 columns padded to 192; N = 1 is
    a single term per sum.  The reference is the np.clongdouble evaluation from the device's own elementals."""
    p, t0s = p16, T0S[which]
    nsrc = len(t0s)
    p.eng.set_distillation(p.random_vectors(nev, 70 + nev))
    p.eng.set_distillation_momenta(MOMENTA16)
    M = p.eng.laph_elementals()
    tau = _tau(900 + 16 * nev + nsrc, nsrc, p.L, nev)
    if nsrc > 1:
        tau[1] = 0.0
    p.eng.set_profiling(True)
    p.eng.timers_reset()
    try:
        T, loops = p.eng.apply_laph_contract(tau, t0s)
        _, launches = p.eng.kernel_stats(KCLASS_LAPH_CONTRACT)
        work = p.eng.kernel_work(KCLASS_LAPH_CONTRACT)
    finally:
        p.eng.set_profiling(False)
    assert T.shape == (nsrc, 3, 2, 2, 2, 2, p.L) and loops.shape == (nsrc, 3, 2, 2)
    blocks = [len(c) for c in _chunks(t0s, nev)]
    assert launches == 3 * 3 * len(blocks) and work == _work(p.L, nev, MOMENTA16, blocks)
    Tw, lw = utils.distilled_sums_wide(tau, M, t0s)
    bT, bl = utils.distilled_contract_bounds(tau, M, t0s)
    worst_T, worst_l = _fraction(np.abs(T - Tw), bT), _fraction(np.abs(loops - lw), bl)
    print("contraction n=%d N=%d sources=%d: worst |dT| / bound = %.3f, worst |dloop| / bound = %.3f"
          % (p.n, nev, nsrc, worst_T, worst_l))
    assert worst_T <= 1.0 and worst_l <= 1.0
    assert np.max(np.abs(T[0])) > 0 and np.max(np.abs(loops[0])) > 0
    if nsrc > 1:
        assert np.all(T[1] == 0) and np.all(loops[1] == 0)                 # a zero source comes back exactly zero
    T2, loops2 = p.eng.apply_laph_contract(tau, t0s)
    assert np.array_equal(T2, T) and np.array_equal(loops2, loops)         # two calls agree bit for bit
    if which == "three":
        # a source's values do not depend on the sources it shares the block with, nor on where its columns start
        Ta, la = p.eng.apply_laph_contract(tau[2:3], [3])
        assert np.array_equal(Ta[0], T[2]) and np.array_equal(la[0], loops[2])


# ---- 3. the contraction kernels alone, schwinger128 -------------------------------------------------------
@pytest.mark.parametrize("nev,t0s,momenta", [(40, [5, 127, 64], [0, 3]), (128, [77], [1])],
                         ids=["N40-three-sources", "N128-full-block"])
def test_contract_128(p128, nev, t0s, momenta):
    """N = 40: three row tiles, the last padded, 240 columns of 256; N = 128: eight row tiles, a full 256-column block.
    The reference is complex128 (utils.distilled_pair_sums / distilled_loops with the device's elementals) and carries
    rounding of its own of the same order: the bar is twice the bound, as in the low-mode contraction's test."""
    p = p128
    nsrc = len(t0s)
    p.eng.set_distillation(p.random_vectors(nev, 5))
    p.eng.set_distillation_momenta(momenta)
    M = p.eng.laph_elementals()
    tau = _tau(17, nsrc, p.L, nev)
    T, loops = p.eng.apply_laph_contract(tau, t0s)
    ref = utils.distilled_pair_sums(tau, M, t0s)
    lref = utils.distilled_loops(tau, M, t0s)[..., t0s].transpose(3, 0, 1, 2)          # [s][j][a][b]
    bT, bl = utils.distilled_contract_bounds(tau, M, t0s, wide=False)
    worst_T, worst_l = _fraction(np.abs(T - ref), bT), _fraction(np.abs(loops - lref), bl)
    print("contraction n=%d N=%d sources=%d momenta=%s: worst |dT| / bound = %.3f, worst |dloop| / bound = %.3f"
          % (p.n, nev, nsrc, momenta, worst_T, worst_l))
    assert worst_T <= 2.0 and worst_l <= 2.0
    T2, loops2 = p.eng.apply_laph_contract(tau, t0s)
    assert np.array_equal(T2, T) and np.array_equal(loops2, loops)


# ---- 4. the whole call ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nev,t0s", [(5, [3, 0, 15, 8, 1, 12, 6]), (16, list(range(16)))],
                         ids=["70-columns", "two-blocks"])
def test_distilled_two_point_16(p16, nev, t0s):
    p, momenta = p16, [0, 1]
    V = p.vectors(nev)
    p.eng.set_distillation(V)
    p.eng.set_distillation_momenta(momenta)
    T, loops, tau, iters = _tight(p, lambda: p.eng.distilled_two_point(t0s, 1e-12, 1000))
    nsrc = len(t0s)
    assert T.shape == (nsrc, 2, 2, 2, 2, 2, p.L) and loops.shape == (nsrc, 2, 2, 2)
    assert tau.shape == (nsrc, p.L, 2, nev, nev, 2) and iters.shape == (nsrc, nev, 2) and iters.min() >= 1
    # the solves and the projection are those of sw_perambulators on every chunk
    first = 0
    for part in _chunks(t0s, nev):
        tau_c, it_c = _tight(p, lambda: p.eng.perambulators(part, 1e-12, 1000))
        assert np.array_equal(tau[first:first + len(part)], tau_c)
        assert np.array_equal(iters[first:first + len(part)], it_c)
        first += len(part)
    # ... the contraction is that of the kernels alone
    Tc, lc = p.eng.apply_laph_contract(tau, t0s)
    assert np.array_equal(T, Tc) and np.array_equal(loops, lc)
    # ... and does not depend on whether the perambulators are copied out
    T2, loops2, none, iters2 = _tight(p, lambda: p.eng.distilled_two_point(t0s, 1e-12, 1000, keep=False))
    assert none is None and np.array_equal(T2, T) and np.array_equal(loops2, loops) and np.array_equal(iters2, iters)
    # against sparse LU and the host formulas
    Z = p.solve(utils.laph_sources(V, p.L, t0s))
    M = utils.laph_elementals(V, p.L, momenta)
    tau_ref = utils.perambulators_from_solutions(V, Z, p.L, nsrc=nsrc)
    Tref = utils.distilled_pair_sums(tau_ref, M, t0s)
    lref = utils.distilled_loops(tau_ref, M, t0s)[..., t0s].transpose(3, 0, 1, 2)
    for j in range(2):
        err = np.max(np.abs(T[:, j] - Tref[:, j])) / np.max(np.abs(Tref[:, j]))
        lerr = np.max(np.abs(loops[:, j] - lref[:, j])) / np.max(np.abs(lref[:, j]))
        print("distilled two-point n=%d N=%d sources=%d p=%d: max |T - LU| / max |T| = %.2e, loops %.2e"
              % (p.n, nev, nsrc, momenta[j], err, lerr))
        assert err < 2e-10 and lerr < 2e-10


# ---- 5. refusals ------------------------------------------------------------------------------------------
def _counts(eng):
    return [eng.kernel_stats(c)[1] for c in range(KCLASS_LAPH_CONTRACT + 1)] + [eng.launch_count()]


def test_refusals_launch_nothing(p16):
    p, eng = p16, p16.eng
    V = p.vectors(5)
    tau = _tau(1, 1, p.L, 5)
    t = np.array([3], dtype=np.int32)
    out = np.zeros(2 * 16 * p.L * 2, dtype=np.complex128)
    eng.set_distillation(None)
    eng.set_profiling(True)
    eng.timers_reset()
    try:
        before = _counts(eng)
        for call in (lambda: eng.distilled_two_point([3], 1e-12, 100), lambda: eng.set_distillation_momenta([0]),
                     lambda: eng.laph_elementals(),
                     lambda: eng.apply_laph_contract(np.zeros((1, p.L, 2, 0, 0, 2), dtype=np.complex128), [3])):
            with pytest.raises(EngineError, match="no distillation registration"):
                call()
        eng.set_distillation(V)
        for call in (lambda: eng.distilled_two_point([3], 1e-12, 100), lambda: eng.laph_elementals(),
                     lambda: eng.apply_laph_contract(tau, [3])):
            with pytest.raises(EngineError, match="no distillation momenta"):
                call()
        with pytest.raises(EngineError, match="at most 8"):
            eng.set_distillation_momenta(list(range(9)))
        with pytest.raises(EngineError, match="outside"):
            eng.set_distillation_momenta([0, p.L])
        with pytest.raises(EngineError, match="outside"):
            eng.set_distillation_momenta([-1])
        with pytest.raises(EngineError, match="listed twice"):
            eng.set_distillation_momenta([1, 2, 1])
        assert _counts(eng) == before
        eng.set_distillation_momenta([0, 1])
        eng.set_distillation_momenta(None)                                 # clears
        with pytest.raises(EngineError, match="no distillation momenta"):
            eng.laph_elementals()
        eng.set_distillation_momenta([0, 1])
        registered = _counts(eng)
        assert registered[KCLASS_LAPH_CONTRACT] == before[KCLASS_LAPH_CONTRACT] + 4
        for t0s, msg in [([], "outside"), (list(range(16)) + [0], "outside"), ([16], "outside"), ([-1], "outside"),
                         ([3, 7, 3], "listed twice")]:
            with pytest.raises(EngineError, match=msg):
                eng.distilled_two_point(t0s, 1e-12, 100)
            with pytest.raises(EngineError, match=msg):
                eng.apply_laph_contract(_tau(2, len(t0s), p.L, 5), t0s)
        with pytest.raises(EngineError, match="maxiter"):
            eng.distilled_two_point([3], 1e-12, 0)
        for T_, l_ in ((None, out.ctypes.data), (out.ctypes.data, None)):
            rc = eng._lib.sw_distilled_two_point(eng._h, 1, t.ctypes.data, 1e-12, 100, T_, l_, None, None)
            assert rc != 0 and b"null output" in eng._lib.sw_last_error(eng._h)
        rc = eng._lib.sw_distilled_two_point(eng._h, 1, None, 1e-12, 100, out.ctypes.data, out.ctypes.data, None, None)
        assert rc != 0 and b"null source timeslice list" in eng._lib.sw_last_error(eng._h)
        rc = eng._lib.sw_apply_laph_contract(eng._h, 1, t.ctypes.data, None, out.ctypes.data, out.ctypes.data)
        assert rc != 0 and b"null argument" in eng._lib.sw_last_error(eng._h)
        rc = eng._lib.sw_apply_laph_elementals(eng._h, None)
        assert rc != 0 and b"null output" in eng._lib.sw_last_error(eng._h)
        assert _counts(eng) == registered                                  # nothing was launched by any refusal
        # the registrations survived the refused calls
        T, loops, _, _ = eng.distilled_two_point([3], 1e-12, 1000)
        assert T.shape == (1, 2, 2, 2, 2, 2, 16) and np.max(np.abs(T)) > 0 and np.max(np.abs(loops)) > 0
    finally:
        eng.set_profiling(False)


def test_an_engine_without_a_finalised_hierarchy_is_refused(p16):
    eng = Engine(p16.eng.device)
    try:
        L, mass, U1, U2 = p16.lattice
        eng.hier_begin(0, 1)
        eng.set_lattice(0, L, mass, U1, U2)
        eng.set_distillation(p16.vectors(5))
        eng.set_distillation_momenta([0, 1])                               # needs the lattice only
        assert eng.laph_elementals().shape == (2, 16, 5, 5)
        launches = eng.launch_count()
        with pytest.raises(EngineError, match="not finalised"):
            eng.distilled_two_point([3], 1e-12, 100)
        assert eng.launch_count() == launches
        eng.hier_begin(0, 1)                                               # a new definition of hierarchy 0 drops both
        eng.set_lattice(0, L, mass, U1, U2)
        with pytest.raises(EngineError, match="no distillation registration"):
            eng.laph_elementals()
        eng.set_distillation(p16.vectors(5))
        with pytest.raises(EngineError, match="no distillation momenta"):
            eng.laph_elementals()
    finally:
        eng.close()


# ---- 6. isolation -----------------------------------------------------------------------------------------
def test_a_call_leaves_the_probe_modes_alone(p16, fresh16):
    """A mode-6 batch after a call equals, bit for bit, that of an engine with the same hierarchy that never made one;
    the fetches of the other modes still return their own last batches; the call's launches and work are counted in
    class 27 and leave class 26 what sw_perambulators makes it."""
    p, fresh = p16, fresh16
    np.random.seed(23)
    codes = utils.draw_probes(5, p.n, "z4")
    fresh.eng.set_two_point(3, [0, 15])
    ref6, itf6, _ = fresh.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
    t0s, momenta = list(range(16)), [0, 1]
    try:
        p.eng.set_two_point(3, [0, 15])
        p.eng.set_loop_momenta([0, 1])
        before6, _, _ = p.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
        assert np.array_equal(before6, ref6)
        loops5, _, _ = p.eng.hutch_batch_loops(0, utils.draw_probes(5, p.n, "z2"), 1e-12, 1000)
        est = p.eng.hutch_fetch()
        p.eng.set_distillation(p.vectors(16))
        p.eng.set_distillation_momenta(momenta)
        p.eng.set_profiling(True)
        p.eng.timers_reset()
        try:
            T, loops, tau, _ = p.eng.distilled_two_point(t0s, 1e-12, 1000)  # two blocks: the workspace grows
            ms, launches = p.eng.kernel_stats(KCLASS_LAPH_CONTRACT)
            work = p.eng.kernel_work(KCLASS_LAPH_CONTRACT)
            _, launches26 = p.eng.kernel_stats(KCLASS_LAPH)
            work26 = p.eng.kernel_work(KCLASS_LAPH)
            dots = p.eng.timers()['dots']
        finally:
            p.eng.set_profiling(False)
        assert launches == 2 * 2 * 3 and ms > 0 and dots >= ms
        assert work == _work(p.L, 16, momenta, [8, 8])
        assert launches26 == 2 * 2 and work26 == 2 * 8.0 * 2 * p.L * p.L * 16 * 256
        assert np.array_equal(p.eng.hutch_fetch_two_point(), ref6)
        assert np.array_equal(p.eng.hutch_fetch_loops(), loops5)
        for a, b in zip(p.eng.hutch_fetch(), est):
            assert np.array_equal(a, b)
        T6, itf, _ = p.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
        assert np.array_equal(T6, ref6) and np.array_equal(itf, itf6)
        T2, loops2, tau2, _ = p.eng.distilled_two_point(t0s, 1e-12, 1000)
        assert np.array_equal(T2, T) and np.array_equal(loops2, loops) and np.array_equal(tau2, tau)
        assert np.array_equal(p.eng.laph_elementals().shape, (2, 16, 16, 16))          # the registration survived
    finally:
        p.eng.set_two_point(0, None)
        p.eng.set_loop_momenta(None)
        fresh.eng.set_two_point(0, None)


# ---- 7. schwinger128 at full rank against the existing two-point fixture ----------------------------------
def test_full_rank_128_reproduces_the_undistilled_pair_sums(p128):
    """N = L = 128: box = 1, so the distilled pair sums are the E[T] of tests/golden/two_point128.json.  One full block,
    eight row tiles in every stage.  The bar is 2e-10 of the largest entry of each momentum."""
    p = p128
    with open(os.path.join(HERE, "golden", "two_point128.json")) as f:
        g = json.load(f)
    golden = np.array([complex(re, im) for re, im in g["two_point128"]]).reshape(g["shape"])
    assert g["momenta"] == [0, 1] and g["source_timeslice"] == 5
    p.eng.set_distillation(p.vectors(128))
    p.eng.set_distillation_momenta([0, 1])
    T, loops, none, iters = _tight(p, lambda: p.eng.distilled_two_point([5], 1e-12, 1000, keep=False))
    assert none is None and T.shape == (1, 2, 2, 2, 2, 2, 128) and iters.min() >= 1
    assert T[0].shape == golden.shape and np.all(np.isfinite(loops))
    for j in range(2):
        err = np.max(np.abs(T[0, j] - golden[j])) / np.max(np.abs(golden[j]))
        print("full rank on the device n=%d p=%d: max |T - golden| / max |golden| = %.2e" % (p.n, j, err))
        assert err < 2e-10


# ---- 8. the flow ------------------------------------------------------------------------------------------
KEYS = {'two_point', 'two_point_avg', 'loops', 'perambulators', 'eigenvalues', 'momenta', 'source_timeslices',
        'distillation_vectors', 'function_iters', 'solves', 'solve_s'}


def _flow(name, **extra):
    params = gateway.set_params(name)
    params['function_tol'] = 1e-12
    params['stop_factor'] = 0.1
    params.update(extra)
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    return stoch_trace.distilled_two_point(A, utils.trace_params_from_params(params, "hutchinson"))


def test_flow_128_on_the_device_against_the_fixture(capsys):
    with open(os.path.join(HERE, "golden", "distilled_two_point128.json")) as f:
        g = json.load(f)
    golden = np.array([complex(re, im) for re, im in g["distilled_two_point128"]]).reshape(g["shape"])
    res = _flow('schwinger128', distillation_vectors=32, two_point_momenta=[0, 1], source_timeslices=[5],
                distilled_contraction="device")
    capsys.readouterr()
    assert set(res) == KEYS
    assert res['two_point'].shape == (1, 2, 2, 2, 2, 2, 128) and res['two_point_avg'].shape == (2, 2, 2, 2, 2, 128)
    assert res['perambulators'].shape == (1, 128, 2, 32, 32, 2)
    assert res['momenta'] == [0, 1] and res['source_timeslices'] == [5] and res['distillation_vectors'] == 32
    assert res['solves'] == 64 and res['function_iters'] >= 64 and res['solve_s'] > 0
    for j in range(2):
        err = np.max(np.abs(res['two_point'][0, j] - golden[j])) / np.max(np.abs(golden[j]))
        print("distilled_two_point on the device N=32 t0=5 p=%d: max |T - golden| / max |golden| = %.2e" % (j, err))
        assert err < 2e-10
    assert np.array_equal(res['two_point_avg'], np.roll(res['two_point'][0], -5, axis=-1))
    finite = np.isfinite(res['loops'])
    assert res['loops'].shape == (2, 2, 2, 128) and np.all(finite[..., 5]) and not np.any(np.delete(finite, 5, axis=-1))


def test_flow_16_device_against_host(capsys, tmp_path):
    """The same set-up cache for every run, so that the hierarchies -- and with them the perambulators -- are the same
    bits; the contractions differ by their rounding only."""
    common = dict(distillation_vectors=5, two_point_momenta=[0, 1, 15], source_timeslices=[3, 0, 15],
                  cache_dir=str(tmp_path))
    host = _flow('schwinger16', **common)
    dev = _flow('schwinger16', distilled_contraction="device", **common)
    lean = _flow('schwinger16', distilled_contraction="device", keep_perambulators=False, **common)
    capsys.readouterr()
    assert set(host) == KEYS and set(dev) == KEYS and set(lean) == KEYS
    for key in ('two_point', 'two_point_avg', 'loops'):
        a, b = host[key], dev[key]
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(a)
        err = np.max(np.abs(a[ok] - b[ok])) / np.max(np.abs(a[ok]))
        print("flow on 16^2, %s: max |device - host| / max |host| = %.2e" % (key, err))
        assert err < 2e-10
        assert np.array_equal(lean[key], b, equal_nan=True)
    finite = np.isfinite(dev['loops'])
    assert np.all(finite[..., [3, 0, 15]]) and not np.any(np.delete(finite, [3, 0, 15], axis=-1))
    assert np.array_equal(dev['perambulators'], host['perambulators'])
    assert lean['perambulators'] is None
    for key in ('momenta', 'source_timeslices', 'distillation_vectors', 'solves', 'function_iters'):
        assert dev[key] == host[key] and lean[key] == host[key]
    assert np.array_equal(dev['eigenvalues'], host['eigenvalues'])
