"""GPU: distillation (sw_set_distillation, sw_perambulators, k_laph_sources, k_laph_project) -- the two kernels alone
against their NumPy definitions (the projection within its derived rounding bound of extended precision), the
perambulators against sparse LU, the ABI's refusals and what a call leaves of the probe modes, the full-rank
perambulators of schwinger128 against the existing two-point fixture, and the distilled_two_point() flow against its
own fixture."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import gateway, hierarchy, matrix, stoch_trace, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import KCLASS_LAPH, Engine, EngineError  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG  # noqa: E402
from oracle import ref_path as rp  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


class Problem:
    """One lattice with its hierarchy on the GPU, no deflation vectors (distillation uses none), its links, its
    Laplacian eigenvectors (all L of them: the first N are the N-vector set) and its sparse LU."""

    def __init__(self, name, cache_dir=None):
        """cache_dir: the set-up cache, so that two engines that are compared bit for bit get the same hierarchy."""
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

    @property
    def lu(self):
        if self._lu is None:
            self._lu = rp.LUSolver(self.A)
        return self._lu

    def solve(self, src):
        return np.asarray(self.lu(np.ascontiguousarray(src.T))).T


@pytest.fixture(scope="module")
def setup_cache(tmp_path_factory):
    return tmp_path_factory.mktemp("setup_cache")


@pytest.fixture(scope="module")
def p16(setup_cache):
    p = Problem('schwinger16', setup_cache)
    yield p
    p.eng.set_distillation(None)


@pytest.fixture(scope="module")
def fresh16(setup_cache, p16):          # after p16: reads the set-up products p16 computed; never runs a perambulator
    return Problem('schwinger16', setup_cache)


@pytest.fixture(scope="module")
def p128():
    p = Problem('schwinger128')
    yield p
    p.eng.set_distillation(None)


def _field(seed, nb, n):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nb, n)) + 1j * rng.standard_normal((nb, n))


def _tight(p, body):
    saved = p.eng.get_option("stop_factor")
    p.eng.set_option("stop_factor", 0.1)
    try:
        return body()
    finally:
        p.eng.set_option("stop_factor", saved)


def _weights(V, Z, L):
    """W[t][c][m][k] = sum_x |v_m(x,t)| |Z[k][idx(c,x,t)]| in extended precision."""
    return utils.perambulators_from_solutions(np.abs(V).astype(np.clongdouble), np.abs(Z).astype(np.clongdouble), L).real


def _ratio(out, V, Z, L):
    """|out - ref| in extended precision over (L + 8) 2^-52 sum_x |v_m(x,t)| |Z(x)|: each component of an output is a
    fixed-order chain of 2 L fused multiply-adds on the matrix cores, the constant the one DESIGN 4g derived for the
    same chain with one more multiply."""
    ref = utils.perambulators_from_solutions(V.astype(np.clongdouble), Z.astype(np.clongdouble), L)
    err, bound = np.abs(out - ref), (L + 8) * 2.0 ** -52 * _weights(V, Z, L)
    assert np.all(err[bound == 0] == 0)                                    # a zero column: nothing to be off by
    return float(np.max(err[bound > 0] / bound[bound > 0]))


# ---- 1. the source kernel ---------------------------------------------------------------------------------
def test_laph_sources_16(p16):
    p, t0s = p16, [0, 15, 3]
    V = p.vectors(5)
    p.eng.set_distillation(V)
    out = p.eng.apply_laph_sources(t0s)
    assert out.shape == (3 * 5 * 2, p.n)
    assert np.array_equal(out, utils.laph_sources(V, p.L, t0s))
    assert np.array_equal(p.eng.apply_laph_sources([7]), utils.laph_sources(V, p.L, [7]))
    # more than one 256-column block: 16 vectors on 9 timeslices are 288 columns
    V16 = p.vectors(16)
    p.eng.set_distillation(V16)
    many = [4, 0, 15, 1, 9, 2, 8, 3, 7]
    assert np.array_equal(p.eng.apply_laph_sources(many), utils.laph_sources(V16, p.L, many))


# ---- 2. the projection kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("nev", [1, 5, 16])
@pytest.mark.parametrize("nb", [1, 3, 70])
def test_laph_project_16(p16, nb, nev):
    """One padded column group (nb = 1, 3) and two (70); one row tile, padded (N = 1, 5) and full (16)."""
    p = p16
    V = p.vectors(nev)
    Z = _field(600 + nb, nb, p.n)
    if nb > 1:
        Z[1] = 0.0
    p.eng.set_distillation(V)
    out = p.eng.apply_laph_project(Z)
    assert out.shape == (p.L, 2, nev, nb)
    worst = _ratio(out, V, Z, p.L)
    print("projection n=%d nb=%d N=%d: worst |err| / bound = %.3f" % (p.n, nb, nev, worst))
    assert worst <= 1.0
    assert np.max(np.abs(out[..., 0])) > 0
    if nb > 1:
        assert np.all(out[..., 1] == 0)                                    # a zero column comes back exactly zero
    assert np.array_equal(p.eng.apply_laph_project(Z), out)                # two calls agree bit for bit
    if nb == 70:
        # a column's result does not depend on how many other columns the launch has
        alone = p.eng.apply_laph_project(Z[37])
        assert alone.shape == (p.L, 2, nev, 1) and np.array_equal(alone[..., 0], out[..., 37])


def test_laph_project_128_two_row_tiles(p128):
    p = p128
    L, nb, nev = p.L, 64, 32
    V = p.vectors(nev)
    Z = _field(11, nb, p.n)
    p.eng.set_distillation(V)
    p.eng.set_profiling(True)
    p.eng.timers_reset()
    try:
        out = p.eng.apply_laph_project(Z)
        ms, launches = p.eng.kernel_stats(KCLASS_LAPH)
        work = p.eng.kernel_work(KCLASS_LAPH)
        dots = p.eng.timers()['dots']
    finally:
        p.eng.set_profiling(False)
    assert out.shape == (L, 2, nev, nb)
    assert launches == 1 and ms > 0 and dots >= ms
    assert work == 8.0 * 2 * L * L * 32 * 64
    ts = [0, 5, 77, 127]
    Zs = np.ascontiguousarray(Z.reshape(nb, 2, L, L)[:, :, ts, :])
    worst = 0.0
    for i, t in enumerate(ts):
        # the one timeslice as an L-site problem of its own: utils takes (L, N, L) and (nb, 2 L^2), so compare entry sums
        ref = np.einsum('mx,kcx->cmk', V[t].astype(np.clongdouble).conj(), Zs[:, :, i].astype(np.clongdouble))
        w = np.einsum('mx,kcx->cmk', np.abs(V[t]).astype(np.longdouble), np.abs(Zs[:, :, i]).astype(np.longdouble))
        worst = max(worst, float(np.max(np.abs(out[t] - ref) / ((L + 8) * 2.0 ** -52 * w))))
    print("projection n=%d nb=%d N=%d: worst |err| / bound on the timeslices %s = %.3f" % (p.n, nb, nev, ts, worst))
    assert worst <= 1.0
    assert np.array_equal(p.eng.apply_laph_project(Z), out)


# ---- 3. the perambulators against sparse LU ---------------------------------------------------------------
@pytest.mark.parametrize("nev,t0s", [(5, [3]), (5, [3, 0, 15, 8, 1, 12, 6]), (16, list(range(16)))],
                         ids=["10-columns", "70-columns", "512-columns"])
def test_perambulators_16_against_sparse_lu(p16, nev, t0s):
    """One padded block; 70 columns, past a 64-column pad boundary; 512 columns, two solve blocks.  tau is linear in a
    solution that the solver holds to 1e-10: the bar is mode 6's, 2e-10 of the call's largest sum_x |v_m| |z|."""
    p = p16
    V = p.vectors(nev)
    p.eng.set_distillation(V)
    p.eng.set_profiling(True)
    p.eng.timers_reset()
    try:
        tau, iters = _tight(p, lambda: p.eng.perambulators(t0s, 1e-12, 1000))
        _, launches = p.eng.kernel_stats(KCLASS_LAPH)
        work = p.eng.kernel_work(KCLASS_LAPH)
    finally:
        p.eng.set_profiling(False)
    nsrc, total = len(t0s), 2 * nev * len(t0s)
    assert tau.shape == (nsrc, p.L, 2, nev, nev, 2) and iters.shape == (nsrc, nev, 2)
    assert iters.min() >= 1 and iters.max() <= 1000
    blocks = [min(256, total - c) for c in range(0, total, 256)]
    assert launches == 2 * len(blocks)
    assert work == sum(8.0 * 2 * p.L * p.L * 16 * ((b + 63) // 64 * 64) for b in blocks)
    Z = p.solve(utils.laph_sources(V, p.L, t0s))
    ref = utils.perambulators_from_solutions(V, Z, p.L, nsrc=nsrc)
    worst = np.max(np.abs(tau - ref)) / float(np.max(_weights(V, Z, p.L)))
    print("perambulators n=%d N=%d sources=%d (%d columns): max |tau - ref| / max sum|v||z| = %.2e, iterations %d..%d"
          % (p.n, nev, nsrc, total, worst, iters.min(), iters.max()))
    assert worst < 2e-10
    tau2, iters2 = _tight(p, lambda: p.eng.perambulators(t0s, 1e-12, 1000))
    assert np.array_equal(tau2, tau) and np.array_equal(iters2, iters)     # two calls agree bit for bit


# ---- 4. refusals and isolation ----------------------------------------------------------------------------
def test_refusals_launch_nothing(p16):
    p, eng = p16, p16.eng
    V = p.vectors(5)
    Z = _field(1, 2, p.n)
    eng.set_distillation(None)
    launches = eng.launch_count()
    for call in (lambda: eng.perambulators([3], 1e-12, 100), lambda: eng.apply_laph_sources([3]),
                 lambda: eng.apply_laph_project(Z)):
        with pytest.raises(EngineError, match="no distillation registration"):
            call()
    with pytest.raises(EngineError, match="outside"):
        eng.set_distillation(np.zeros((16, 17, 16), dtype=np.complex128))
    with pytest.raises(EngineError, match="expected"):
        eng.set_distillation(np.zeros((16, 5, 8), dtype=np.complex128))
    eng.set_distillation(V)
    after_set = eng.launch_count()
    assert after_set == launches                                           # the registration is uploads only
    for t0s, msg in [([], "outside"), (list(range(16)) + [0], "outside"), ([16], "outside"), ([-1], "outside"),
                     ([3, 7, 3], "listed twice")]:
        with pytest.raises(EngineError, match=msg):
            eng.perambulators(t0s, 1e-12, 100)
        with pytest.raises(EngineError, match=msg):
            eng.apply_laph_sources(t0s)
    with pytest.raises(EngineError, match="maxiter"):
        eng.perambulators([3], 1e-12, 0)
    t = np.array([3], dtype=np.int32)
    rc = eng._lib.sw_perambulators(eng._h, 1, t.ctypes.data, 1e-12, 100, None, None)
    assert rc != 0 and b"null output" in eng._lib.sw_last_error(eng._h)
    rc = eng._lib.sw_perambulators(eng._h, 1, None, 1e-12, 100, t.ctypes.data, None)
    assert rc != 0 and b"null source timeslice list" in eng._lib.sw_last_error(eng._h)
    assert eng.launch_count() == launches                                  # nothing was launched by any refusal
    # the registration survived the refused calls
    tau, _ = eng.perambulators([3], 1e-12, 1000)
    assert tau.shape == (1, 16, 2, 5, 5, 2) and eng.launch_count() > launches


def test_engines_without_a_lattice_or_a_finalised_hierarchy_are_refused(p16):
    V = p16.vectors(5)
    eng = Engine(p16.eng.device)
    try:
        eng.hier_begin(0, 1)
        eng.set_csr(0, 0, p16.A)
        launches = eng.launch_count()
        with pytest.raises(EngineError, match="lattice level 0"):
            eng.set_distillation(V)
        eng.set_distillation(None)                                         # clearing needs nothing
        assert eng.launch_count() == launches
    finally:
        eng.close()
    eng = Engine(p16.eng.device)
    try:
        L, mass, U1, U2 = p16.lattice
        eng.hier_begin(0, 1)
        eng.set_lattice(0, L, mass, U1, U2)
        eng.set_distillation(V)
        launches = eng.launch_count()
        with pytest.raises(EngineError, match="not finalised"):
            eng.perambulators([3], 1e-12, 100)
        assert eng.launch_count() == launches
    finally:
        eng.close()


def test_a_perambulator_call_leaves_the_probe_modes_alone(p16, fresh16):
    """A mode-6 batch after a perambulator call equals, bit for bit, that of an engine with the same hierarchy that
    never ran one; the fetches of the other modes still return their own last batches."""
    p, fresh = p16, fresh16
    np.random.seed(23)
    codes = utils.draw_probes(5, p.n, "z4")
    fresh.eng.set_two_point(3, [0, 15])
    ref6, itf6, _ = fresh.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
    try:
        p.eng.set_two_point(3, [0, 15])
        p.eng.set_loop_momenta([0, 1])
        before6, _, _ = p.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
        assert np.array_equal(before6, ref6)
        loops, _, _ = p.eng.hutch_batch_loops(0, utils.draw_probes(5, p.n, "z2"), 1e-12, 1000)
        est = p.eng.hutch_fetch()
        p.eng.set_distillation(p.vectors(16))
        tau, _ = p.eng.perambulators(list(range(16)), 1e-12, 1000)          # two 256-column blocks: the workspace grows
        assert np.array_equal(p.eng.hutch_fetch_two_point(), ref6)
        assert np.array_equal(p.eng.hutch_fetch_loops(), loops)
        for a, b in zip(p.eng.hutch_fetch(), est):
            assert np.array_equal(a, b)
        T6, itf, _ = p.eng.hutch_batch_two_point(0, codes, 1e-12, 1000)
        assert np.array_equal(T6, ref6) and np.array_equal(itf, itf6)
        tau2, _ = p.eng.perambulators(list(range(16)), 1e-12, 1000)
        assert np.array_equal(tau2, tau)
    finally:
        p.eng.set_two_point(0, None)
        p.eng.set_loop_momenta(None)
        fresh.eng.set_two_point(0, None)


# ---- 5. schwinger128 at full rank against the existing two-point fixture ----------------------------------
def test_full_rank_128_reproduces_the_undistilled_pair_sums(p128):
    """N = L = 128: box = 1, so the distilled pair sums are the E[T] of tests/golden/two_point128.json.  One 256-column
    block.  The bar is 2e-10 of the largest entry of each momentum."""
    p = p128
    with open(os.path.join(HERE, "golden", "two_point128.json")) as f:
        g = json.load(f)
    golden = np.array([complex(re, im) for re, im in g["two_point128"]]).reshape(g["shape"])
    assert g["momenta"] == [0, 1] and g["source_timeslice"] == 5
    V = p.vectors(128)
    p.eng.set_distillation(V)
    tau, iters = _tight(p, lambda: p.eng.perambulators([5], 1e-12, 1000))
    assert tau.shape == (1, 128, 2, 128, 128, 2) and iters.min() >= 1
    T = utils.distilled_pair_sums(tau, utils.laph_elementals(V, p.L, [0, 1]), [5])[0]
    assert T.shape == golden.shape
    pion = sum(golden[0, a, a, c, c] for a in range(2) for c in range(2)).real       # [t]
    for j in range(2):
        err = np.max(np.abs(T[j] - golden[j])) / np.max(np.abs(golden[j]))
        per_t = np.max(np.abs(T[j] - golden[j]).reshape(16, 128), axis=0) / pion
        print("full rank n=%d p=%d: max |T - golden| / max |golden| = %.2e; worst per-timeslice ratio to the pion "
              "value %.2e (t = %d)" % (p.n, j, err, per_t.max(), int(np.argmax(per_t))))
        assert err < 2e-10


# ---- 6. the flow ------------------------------------------------------------------------------------------
KEYS = {'two_point', 'two_point_avg', 'loops', 'perambulators', 'eigenvalues', 'momenta', 'source_timeslices',
        'distillation_vectors', 'function_iters', 'solves', 'solve_s'}


def _flow(**extra):
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params['stop_factor'] = 0.1
    params['distillation_vectors'] = 32
    params['two_point_momenta'] = [0, 1]
    params.update(extra)
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    return stoch_trace.distilled_two_point(A, utils.trace_params_from_params(params, "hutchinson"))


def test_flow_128_against_the_fixture(capsys):
    with open(os.path.join(HERE, "golden", "distilled_two_point128.json")) as f:
        g = json.load(f)
    golden = np.array([complex(re, im) for re, im in g["distilled_two_point128"]]).reshape(g["shape"])
    res = _flow(source_timeslices=[5])
    capsys.readouterr()
    assert set(res) == KEYS
    assert res['two_point'].shape == (1, 2, 2, 2, 2, 2, 128) and res['two_point_avg'].shape == (2, 2, 2, 2, 2, 128)
    assert res['perambulators'].shape == (1, 128, 2, 32, 32, 2) and res['eigenvalues'].shape == (128, 32)
    assert res['momenta'] == [0, 1] and res['source_timeslices'] == [5] and res['distillation_vectors'] == 32
    assert res['solves'] == 64 and res['function_iters'] >= 64 and res['solve_s'] > 0
    assert np.max(np.abs(res['eigenvalues'][5] - np.array(g["eigenvalues"]))) < 1e-12
    for j in range(2):
        err = np.max(np.abs(res['two_point'][0, j] - golden[j])) / np.max(np.abs(golden[j]))
        print("distilled_two_point N=32 t0=5 p=%d: max |T - golden| / max |golden| = %.2e" % (j, err))
        assert err < 2e-10
    assert np.array_equal(res['two_point_avg'], np.roll(res['two_point'][0], -5, axis=-1))
    finite = np.isfinite(res['loops'])
    assert res['loops'].shape == (2, 2, 2, 128) and np.all(finite[..., 5]) and not np.any(np.delete(finite, 5, axis=-1))


def test_flow_128_two_sources_with_and_without_the_perambulators(capsys):
    res = _flow(source_timeslices=[5, 6])
    lean = _flow(source_timeslices=[5, 6], keep_perambulators=False)
    capsys.readouterr()
    assert set(res) == KEYS and set(lean) == KEYS
    T = res['two_point']
    assert T.shape == (2, 2, 2, 2, 2, 2, 128) and res['perambulators'].shape == (2, 128, 2, 32, 32, 2)
    assert res['source_timeslices'] == [5, 6] and res['solves'] == 128
    mean = np.zeros_like(T[0])
    for dt in range(128):
        mean[..., dt] = 0.5 * (T[0][..., (5 + dt) % 128] + T[1][..., (6 + dt) % 128])
    assert np.max(np.abs(res['two_point_avg'] - mean)) <= 1e-15 * np.max(np.abs(mean))
    finite = np.isfinite(res['loops'])
    assert np.all(finite[..., [5, 6]]) and not np.any(np.delete(finite, [5, 6], axis=-1))
    # the loops are those of the kept perambulators
    M = utils.laph_elementals(np.ascontiguousarray(utils.laplacian_eigenvectors(
        hierarchy.detect_lattice(matrix.loadMatrix(*_matrix_args()))[2], 128, 32)[0]), 128, [0, 1])
    again = utils.distilled_loops(res['perambulators'], M, [5, 6])
    assert np.array_equal(again[..., [5, 6]], res['loops'][..., [5, 6]])
    assert lean['perambulators'] is None
    # the two set-ups build two (equally good) hierarchies: the solutions agree to the solver's tolerance, not bit for bit
    assert np.max(np.abs(lean['two_point'] - T)) < 2e-10 * np.max(np.abs(T))


def _matrix_args():
    params = gateway.set_params('schwinger128')
    return params['matrix'], params['matrix_params']
