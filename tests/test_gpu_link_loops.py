"""GPU: point-split link loops and the conserved vector current per timeslice (SW_MODE_HUTCHINSON_LINK_LOOPS,
k_slice_link_dots) -- the kernel alone against NumPy from the definition, the ABI's refusals, per-probe
parity against sparse LU, the local loops of the same batch bit for bit against mode 5, switching between modes, the
Ward identity and the tie to the local loops through the whole device path on a full Hadamard set, and the
hutchinson() flow against the exact branches of schwinger128."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import gateway, hierarchy, matrix, stoch_trace, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import MODE_HUTCHINSON_LINK_LOOPS, EngineError  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG, REF_HID, _new_engine  # noqa: E402
from oracle import ref_path as rp  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
EIGHT16 = [0, 1, 2, 3, 5, 8, 13, 15]


class Problem:
    """One lattice with its hierarchy on the GPU and the deflation vectors W = gamma_3 V sgn(lambda) registered
    WITHOUT Pperm (key link_loops present)."""

    def __init__(self, name, k_defl):
        params = gateway.set_params(name)
        params['function_tol'] = 1e-12
        params['link_loops'] = [0]
        self.A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
        self.tp = utils.trace_params_from_params(params, "hutchinson")
        self.tp['nr_deflat_vctrs'] = k_defl
        self.tp['solver_cfg'] = dict(hierarchy.DEFAULT_SOLVER_CFG)
        self.mg = MG(self.A)
        self.mg.setup(dof=self.tp['dof'], aggrs=self.tp['aggrs'], max_levels=self.tp['max_nr_levels'], dim=2,
                      acc_eigvs=self.tp['accuracy_mg_eigvs'], sys_type='schwinger', params=self.tp)
        self.mg.total_levels = len(self.mg.ml.levels)
        self.k_defl = k_defl
        self.W, _ = utils.deflation_pre_computations(self.A, k_defl, 1e-9, "hutchinson", self.mg.timer, self.tp,
                                                     self.mg)
        self.L, self.mass, self.U1, self.U2 = self.mg.lattice
        self.n = self.A.shape[0]
        self.eng = self.mg.engine
        self._lu = None

    @property
    def lu(self):
        if self._lu is None:
            self._lu = rp.LUSolver(self.A)
        return self._lu

    def link_ref(self, X, Z, momenta):
        return utils.slice_link_dots(X, Z, self.U1, self.U2, self.L, momenta)

    def projected_solutions(self, X, deflated):
        W = self.W
        return np.array([self.lu(x - W @ (W.conj().T @ x) if deflated else x) for x in X])

    def tr1(self, momenta):
        """(local, link) deflated parts for `momenta`; the vectors they belong to are registered anew."""
        tp = dict(self.tp, link_loops=list(momenta))
        self.W, both = utils.deflation_pre_computations(self.A, self.k_defl, 1e-9, "hutchinson", self.mg.timer, tp,
                                                        self.mg)
        return both


class Lattice:
    """The lattice operator alone on hierarchy 0 of an engine: all the link-dot kernel needs."""

    def __init__(self, A):
        self.L, self.mass, self.U1, self.U2 = hierarchy.detect_lattice(A)
        self.n = 2 * self.L * self.L
        self.eng = _new_engine(0)
        self.eng.hier_begin(REF_HID, 1)
        self.eng.set_lattice(REF_HID, self.L, self.mass, self.U1, self.U2)
        self.eng.hier_end(REF_HID)

    def link_ref(self, X, Z, momenta):
        return utils.slice_link_dots(X, Z, self.U1, self.U2, self.L, momenta)


@pytest.fixture(scope="module")
def p16():
    return Problem('schwinger16', 8)


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _check_kernel(p, nb, kind, momenta, seed):
    np.random.seed(seed)
    codes = utils.draw_probes(nb, p.n, kind)
    X = utils.probes_as_complex(codes)
    Z = _rand((nb, p.n), seed + 1)
    p.eng.set_loop_momenta(momenta)
    out = p.eng.apply_slice_link_dots(codes, Z)
    assert out.shape == (nb, 4, len(momenta), 2, 2, p.L)
    ref = p.link_ref(X, Z, momenta)
    scale = np.sum(np.abs(Z), axis=1)
    worst = np.max(np.abs(out - ref).reshape(nb, -1).max(axis=1) / scale)
    print("link dots n=%d nb=%d %s momenta=%s: max |err| / sum|z| = %.2e" % (p.n, nb, kind, momenta, worst))
    assert worst < 1e-13
    assert np.max(np.abs(ref)) > 0 and np.max(np.abs(out)) > 0
    assert np.array_equal(p.eng.apply_slice_link_dots(codes, Z), out)   # deterministic reduction
    for a in range(4):                                                  # four different branches
        for b in range(a):
            assert not np.array_equal(out[:, a], out[:, b])


# [0]: the no-phase path; [5]: one momentum with phase; [0, 9], [0, 1, 15], eight: 2, 4 and 8 momenta per pass
@pytest.mark.parametrize("momenta", [[0], [5], [0, 9], [0, 1, 15], EIGHT16],
                         ids=["p0", "one", "two", "three", "eight"])
@pytest.mark.parametrize("kind", ["z2", "z4"])
@pytest.mark.parametrize("nb", [1, 3, 70, 130])
def test_link_dots_kernel_16(p16, nb, kind, momenta):
    _check_kernel(p16, nb, kind, momenta, 300 + nb)


def test_link_dots_kernel_L6_unequal_waves():
    """L = 6, the smallest lattice with L % 4 == 2 that hierarchy.detect_lattice admits (L >= 4, even): waves 0 and 1
    hold two sites, waves 2 and 3 one, and the wrap in x falls on wave 1 instead of wave 3.  The kernel needs the
    lattice operator only, so no multigrid set-up is involved (which L = 6 would not admit)."""
    p = Lattice(matrix.synthetic_matrix(6, 0.05, sigma=0.3, seed=106))
    try:
        _check_kernel(p, 3, "z4", [0, 1], 61)
    finally:
        p.eng.close()


def test_link_dots_kernel_128_four_momenta():
    params = gateway.set_params('schwinger128')
    p = Lattice(matrix.loadMatrix(params['matrix'], params['matrix_params']))   # the operator alone: no set-up
    try:
        _check_kernel(p, 5, "z4", [0, 1, 2, 3], 17)
    finally:
        p.eng.close()


def test_abi_refusals(p16):
    eng, n = p16.eng, p16.n
    np.random.seed(3)
    probes = utils.draw_probes(2, n)
    eng.set_loop_momenta([0, 1])                       # a registration drops the batches of the loop modes
    launches = eng.launch_count()
    lib, h = eng._lib, eng._h
    try:
        with pytest.raises(EngineError, match="no link-loop batch to fetch"):
            eng.hutch_fetch_link_loops()
        eng.set_loop_momenta(None)
        with pytest.raises(EngineError, match="no momenta registered"):
            eng.hutch_batch(MODE_HUTCHINSON_LINK_LOOPS, 0, probes, 1e-12, 100)
        with pytest.raises(EngineError, match="no momenta registered"):
            eng.apply_slice_link_dots(probes, np.ones((2, n), dtype=complex))
        with pytest.raises(EngineError, match="no link-loop batch to fetch"):
            eng.hutch_fetch_link_loops()
        eng.set_loop_momenta([0, 1])
        n1 = p16.mg.ml.levels[1].A.shape[0]
        with pytest.raises(EngineError, match="level 0"):
            eng.hutch_batch(MODE_HUTCHINSON_LINK_LOOPS, 1, np.ones((2, n1), dtype=np.int8), 1e-12, 100)
        # null pointers
        Z = np.ones((2, n), dtype=np.complex128)
        out = np.zeros((4, 2, 2, 2, p16.L, 2), dtype=np.complex128)
        ptr = lambda a: a.ctypes.data                  # noqa: E731
        assert lib.sw_hutch_fetch_link_loops(h, None) != 0
        assert lib.sw_apply_slice_link_dots(h, 2, None, ptr(Z), ptr(out)) != 0
        assert lib.sw_apply_slice_link_dots(h, 2, ptr(probes), None, ptr(out)) != 0
        assert lib.sw_apply_slice_link_dots(h, 2, ptr(probes), ptr(Z), None) != 0
        assert lib.sw_apply_slice_link_dots(h, 0, ptr(probes), ptr(Z), ptr(out)) != 0
        assert eng.launch_count() == launches                              # nothing was launched
    finally:
        eng.set_loop_momenta([0])


def _with_solver_state(p, deflated, body):
    saved = p.eng.get_option("stop_factor")
    p.eng.set_option("stop_factor", 0.1)
    if not deflated:
        p.eng.set_deflation(None)
    try:
        return body()
    finally:
        p.eng.set_option("stop_factor", saved)
        if not deflated:
            p.eng.set_deflation(np.asarray(p.W))


def _check_link_parity(p, codes, momenta, deflated, what):
    """A mode-12 batch against sparse LU, per probe; returns (link branches, local loops of the same batch)."""
    X = utils.probes_as_complex(codes)
    p.eng.set_loop_momenta(momenta)

    def body():
        link, itf, _ = p.eng.hutch_batch_link_loops(0, codes, 1e-12, 1000)
        return link, itf, p.eng.hutch_fetch_loops()

    link, itf, local = _with_solver_state(p, deflated, body)
    nb = codes.shape[0]
    assert link.shape == (nb, 4, len(momenta), 2, 2, p.L) and itf.min() >= 1
    ref = p.link_ref(X, p.projected_solutions(X, deflated), momenta)
    err = np.abs(link - ref).reshape(nb, -1).max(axis=1)
    worst = np.max(err / np.abs(ref).reshape(nb, -1).max(axis=1))
    print("%s n=%d momenta=%s deflated=%s: max |link - ref| / max |ref| = %.2e" % (what, p.n, momenta, deflated, worst))
    assert worst < 1e-10
    return link, local


@pytest.mark.parametrize("kind", ["z2", "z4"])
@pytest.mark.parametrize("deflated", [False, True])
def test_per_probe_parity_16(p16, kind, deflated):
    p = p16
    np.random.seed(21)
    codes = utils.draw_probes(6, p.n, kind)
    momenta = [0, 1, 15]
    _, local = _check_link_parity(p, codes, momenta, deflated, "parity")
    # the local loops of the batch are a mode-5 batch's, bit for bit (same probes, same engine state)
    loops5, _, _ = _with_solver_state(p, deflated, lambda: p.eng.hutch_batch_loops(0, codes, 1e-12, 1000))
    assert local.shape == (6, 3, 2, 2, p.L)
    assert np.array_equal(local, loops5)


def test_mode_switching_keeps_every_fetch_right(p16):
    p = p16
    np.random.seed(41)
    codes = utils.draw_probes(6, p.n, "z4")
    other = utils.draw_probes(6, p.n, "z4")
    momenta = [0, 1, 15]
    p.eng.set_shifts([0, 2 * p.L])
    link, local = _check_link_parity(p, codes, momenta, True, "mode 12 first")
    loops5, _, _ = _with_solver_state(p, True, lambda: p.eng.hutch_batch_loops(0, other, 1e-12, 1000))
    ests4, _, _ = _with_solver_state(p, True, lambda: p.eng.hutch_batch_shifts(0, other, 1e-12, 1000))
    assert not np.array_equal(loops5, local)
    assert np.array_equal(p.eng.hutch_fetch_link_loops(), link)          # mode 12's buffer survived modes 5 and 4
    assert np.array_equal(p.eng.hutch_fetch_loops(), loops5)             # mode 5's holds its own last batch
    again, local2 = _check_link_parity(p, codes, momenta, True, "mode 12 again")
    assert np.array_equal(again, link) and np.array_equal(local2, local)
    assert np.array_equal(p.eng.hutch_fetch_shifts(), ests4)             # and the reverse: mode 4's buffer survived
    assert np.array_equal(p.eng.hutch_fetch_link_loops(), link)


def _current(link, mu):
    hp = hierarchy._HOP["+x" if mu == 'x' else "+y"]
    hm = hierarchy._HOP["-x" if mu == 'x' else "-y"]
    d = 0 if mu == 'x' else 2
    return np.einsum('ab,pabt->pt', hp, link[d]) - np.einsum('ab,pabt->pt', hm, link[d + 1])


def test_ward_identity_through_the_device_16(p16):
    """The 512 Sylvester-Hadamard columns as Z2 probes: their mean is the expectation exactly, so probe mean + tr1
    are the branches of A^-1 up to the solver's tolerance, and the Ward identity and the tie to the local loops must
    hold: residuals below 5e-9 max |entry| (the per-entry 1e-10 of the parity test times the at most 48 entries an
    identity combines)."""
    p = p16
    L, n, momenta = p.L, p.n, [0, 1, 15]
    H = np.array([[1]], dtype=np.int8)
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    assert H.shape == (n, n)
    tr1_local, tr1_link = p.tr1(momenta)               # before the batches: they project with these vectors
    p.eng.set_loop_momenta(momenta)

    def body():
        link, local = [], []
        for first in (0, 256):
            lk, _, _ = p.eng.hutch_batch_link_loops(0, np.ascontiguousarray(H[first:first + 256]), 1e-12, 1000)
            link.append(lk)
            local.append(p.eng.hutch_fetch_loops())
        return np.concatenate(link), np.concatenate(local)

    link, local = _with_solver_state(p, True, body)
    link = link.mean(axis=0) + tr1_link                                # [d][p][a][b][t]
    local = local.mean(axis=0) + tr1_local                             # [p][a][b][t]
    scale = max(np.max(np.abs(link)), np.max(np.abs(local)))
    Jx, Jt = _current(link, 'x'), _current(link, 't')
    om = np.exp(-2j * np.pi * np.asarray(momenta) / L)[:, None]
    ward = np.max(np.abs((1 - om) * Jx + Jt - np.roll(Jt, 1, axis=1)))
    hop = hierarchy._HOP
    hop = (np.einsum('ab,abt->t', hop["+x"], link[0, 0]) + np.einsum('ab,abt->t', hop["-x"], link[1, 0])
           + np.einsum('ab,abt->t', hop["+y"], link[2, 0]) + np.roll(np.einsum('ab,abt->t', hop["-y"], link[3, 0]), 1))
    L1 = local[0, 0, 0] + local[0, 1, 1]
    tie = np.max(np.abs((p.mass + 4) * L1 - hop - 2 * L))
    print("device Ward residual %.2e, tie residual %.2e, max |entry| %.2f, J_t(t,0) = %s"
          % (ward, tie, scale, Jt[0, 0]))
    assert ward < 5e-9 * scale
    assert tie < 5e-9 * scale
    assert np.min(np.abs(Jt[0])) > 0.1
    assert np.array_equal(utils.conserved_current(link, 't'), utils.conserved_current(link[None], 't')[0])
    assert np.max(np.abs(utils.conserved_current(link, 't') - Jt)) < 1e-12 * scale


def _golden(name, key):
    with open(os.path.join(HERE, "golden", name)) as f:
        g = json.load(f)
    return g["momenta"], np.array([complex(re, im) for re, im in g[key]]).reshape(g["shape"])


PLAIN_KEYS = {'trace', 'std_dev', 'nr_ests', 'function_iters', 'total_complexity', 'ests', 'rough_trace',
              'level_tol', 'probe_loop_s', 'probes_solved'}
LOOP_KEYS = {'momenta', 'loops', 'loop_devs', 'loop_ests', 'converged'}
LINK_KEYS = {'link_loops', 'link_loop_devs', 'link_loop_ests', 'link_converged'}


def _within(what, got, devs, nr, exact):
    diff = np.abs(got - exact)
    bound = 5.0 * devs / np.sqrt(nr) + 1e-9
    ratio = diff / bound
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%s: worst |diff| / bound = %.3f at %s (|diff| %.3e, bound %.3e); entries over 3/5 of the bound: %d of %d"
          % (what, ratio[at], at, diff[at], bound[at], int(np.sum(ratio > 0.6)), ratio.size))
    assert np.all(diff < bound)


def test_fixed_length_flow_128_against_the_exact_branches(capsys):
    """2048 probes whatever their variance (tol 1e-9 is never met): every one of the 4 x 2 x 2 x 2 x 128 link entries
    and of the 2 x 2 x 2 x 128 local ones within 5 devs / sqrt(n) + 1e-9 of the exact value, the trace likewise."""
    gm, golden = _golden("link_loops128.json", "link_loops128")
    lm, loops = _golden("slice_loops128.json", "slice_loops128")
    assert gm == [0, 1] and lm[:2] == [0, 1]
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    plain = stoch_trace.hutchinson(A, utils.trace_params_from_params(params, "hutchinson"))   # the same call, no key
    params['link_loops'] = [0, 1]
    tp = utils.trace_params_from_params(params, "hutchinson")
    tp['max_nr_ests'] = 2048
    tp['tol'] = 1e-9
    res = stoch_trace.hutchinson(A, tp)
    capsys.readouterr()
    assert set(plain) == PLAIN_KEYS
    assert set(res) == PLAIN_KEYS | LOOP_KEYS | LINK_KEYS
    nr = res['nr_ests'] + 1
    assert nr == 2048 and res['probes_solved'] == 2048
    assert res['momenta'] == [0, 1]
    assert res['loops'].shape == res['loop_devs'].shape == res['converged'].shape == (2, 2, 2, 128)
    assert res['loop_ests'].shape == (nr, 2, 2, 2, 128)
    assert res['link_loops'].shape == res['link_loop_devs'].shape == res['link_converged'].shape == (4, 2, 2, 2, 128)
    assert res['link_loop_ests'].shape == (nr, 4, 2, 2, 2, 128)
    _within("link loops", res['link_loops'], res['link_loop_devs'], nr, golden)
    _within("local loops", res['loops'], res['loop_devs'], nr, loops[:2])
    tb = 5.0 * res['std_dev'] / np.sqrt(nr) + 1e-9
    print("trace %s |diff| %.3e bound %.3e" % (res['trace'], abs(res['trace'] - 8326.43205953889), tb))
    assert abs(res['trace'] - 8326.43205953889) < tb
    # the per-probe series carry tr1 and average to the reported values
    assert np.max(np.abs(res['link_loop_ests'].mean(axis=0) - res['link_loops'])) < 1e-9
    assert np.max(np.abs(res['loop_ests'].mean(axis=0) - res['loops'])) < 1e-9
    assert res['ests'].shape == (nr,)
