"""GPU: timeslice loops from one solve per probe (sw_set_loop_momenta, SW_MODE_HUTCHINSON_LOOPS, k_slice_dots) --
the kernel alone against NumPy from the definition, the ABI's refusals, per-probe parity against sparse LU, the
scalar-sum identity against SW_MODE_HUTCHINSON_SHIFTS, switching between the two modes, and the hutchinson() flow
against the exact loops of schwinger128."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import gateway, matrix, stoch_trace, utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import MODE_HUTCHINSON_LOOPS, EngineError  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG  # noqa: E402
from oracle import ref_path as rp  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
EIGHT = {16: [0, 1, 2, 3, 5, 8, 13, 15], 128: [0, 1, 2, 3, 64, 65, 126, 127]}


class Problem:
    """One lattice with its hierarchy on the GPU and the deflation vectors W = gamma_3 V sgn(lambda) registered
    WITHOUT Pperm (key timeslice_loops present)."""

    def __init__(self, name, k_defl):
        params = gateway.set_params(name)
        params['function_tol'] = 1e-12
        params['timeslice_loops'] = [0]
        self.A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
        self.tp = utils.trace_params_from_params(params, "hutchinson")
        self.tp['nr_deflat_vctrs'] = k_defl
        from deflatedmlmc_schwinger_amd import hierarchy as _h
        self.tp['solver_cfg'] = dict(_h.DEFAULT_SOLVER_CFG)
        self.mg = MG(self.A)
        self.mg.setup(dof=self.tp['dof'], aggrs=self.tp['aggrs'], max_levels=self.tp['max_nr_levels'], dim=2,
                      acc_eigvs=self.tp['accuracy_mg_eigvs'], sys_type='schwinger', params=self.tp)
        self.mg.total_levels = len(self.mg.ml.levels)
        self.W, self.tr1 = utils.deflation_pre_computations(self.A, k_defl, 1e-9, "hutchinson", self.mg.timer,
                                                            self.tp, self.mg)
        self.L = int(self.tp['latt_dims'][0])
        self.n = self.A.shape[0]
        self.eng = self.mg.engine
        self.lu = rp.LUSolver(self.A)

    def loops_ref(self, X, Z, momenta):
        """l[k][p][a][b][t] = sum_x e^{-2 pi i p x / L} conj(X[k][idx(a,x,t)]) Z[k][idx(b,x,t)]."""
        L = self.L
        Xr, Zr = X.reshape(-1, 2, L, L), Z.reshape(-1, 2, L, L)            # [k][s][t][x]
        return np.einsum('px,katx,kbtx->kpabt', utils.slice_phases(L, momenta), Xr.conj(), Zr)

    def projected_solutions(self, X, deflated):
        W = self.W
        return np.array([self.lu(x - W @ (W.conj().T @ x) if deflated else x) for x in X])


@pytest.fixture(scope="module")
def p16():
    return Problem('schwinger16', 8)


@pytest.fixture(scope="module")
def p128():
    return Problem('schwinger128', 8)


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _check_kernel(p, nb, kind, momenta, seed):
    np.random.seed(seed)
    codes = utils.draw_probes(nb, p.n, kind)
    X = utils.probes_as_complex(codes)
    Z = _rand((nb, p.n), seed + 1)
    p.eng.set_loop_momenta(momenta)
    out = p.eng.apply_slice_dots(codes, Z)
    assert out.shape == (nb, len(momenta), 2, 2, p.L)
    ref = p.loops_ref(X, Z, momenta)
    scale = np.sum(np.abs(Z), axis=1)
    worst = np.max(np.abs(out - ref).reshape(nb, -1).max(axis=1) / scale)
    print("slice dots n=%d nb=%d %s momenta=%s: max |err| / sum|z| = %.2e" % (p.n, nb, kind, momenta, worst))
    assert worst < 1e-13
    assert np.max(np.abs(ref)) > 0 and np.max(np.abs(out)) > 0
    assert np.array_equal(p.eng.apply_slice_dots(codes, Z), out)        # deterministic reduction


# [0]: the no-phase path; [5]: one momentum with phase; [0, 9], [0, 1, 15], eight: 2, 4 and 8 momenta per pass
@pytest.mark.parametrize("momenta", [[0], [5], [0, 9], [0, 1, 15], EIGHT[16]],
                         ids=["p0", "one", "two", "three", "eight"])
@pytest.mark.parametrize("kind", ["z2", "z4"])
@pytest.mark.parametrize("nb", [1, 3, 70, 130])
def test_slice_dots_kernel_16(p16, nb, kind, momenta):
    _check_kernel(p16, nb, kind, momenta, 200 + nb)


def test_slice_dots_kernel_128_four_momenta(p128):
    _check_kernel(p128, 5, "z4", [0, 1, 2, 3], 7)


def test_slice_dots_kernel_128_full_batch(p128):
    _check_kernel(p128, 256, "z4", [0], 8)


def test_abi_refusals(p16):
    eng, L, n = p16.eng, p16.L, p16.n
    np.random.seed(3)
    probes = utils.draw_probes(2, n)
    eng.set_loop_momenta([0, 1])
    launches = eng.launch_count()
    try:
        with pytest.raises(EngineError, match="outside"):
            eng.set_loop_momenta([0, L])
        with pytest.raises(EngineError, match="outside"):
            eng.set_loop_momenta([0, -1])
        with pytest.raises(EngineError, match="listed twice"):
            eng.set_loop_momenta([0, 3, 3])
        with pytest.raises(EngineError, match="at most 8"):
            eng.set_loop_momenta(list(range(9)))
        eng.set_loop_momenta(None)
        with pytest.raises(EngineError, match="no momenta registered"):
            eng.hutch_batch(MODE_HUTCHINSON_LOOPS, 0, probes, 1e-12, 100)
        with pytest.raises(EngineError, match="no momenta registered"):
            eng.apply_slice_dots(probes, np.ones((2, n), dtype=complex))
        with pytest.raises(EngineError, match="no loop batch"):
            eng.hutch_fetch_loops()
        eng.set_loop_momenta([0, 1])
        n1 = p16.mg.ml.levels[1].A.shape[0]
        with pytest.raises(EngineError, match="level 0"):
            eng.hutch_batch(MODE_HUTCHINSON_LOOPS, 1, np.ones((2, n1), dtype=np.int8), 1e-12, 100)
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


def _check_loops_parity(p, codes, momenta, deflated, what):
    """A mode-5 batch against sparse LU, per probe; returns the loops."""
    X = utils.probes_as_complex(codes)
    p.eng.set_loop_momenta(momenta)
    loops, itf, _ = _with_solver_state(p, deflated, lambda: p.eng.hutch_batch_loops(0, codes, 1e-12, 1000))
    assert loops.shape == (codes.shape[0], len(momenta), 2, 2, p.L) and itf.min() >= 1
    ref = p.loops_ref(X, p.projected_solutions(X, deflated), momenta)
    err = np.abs(loops - ref).reshape(codes.shape[0], -1).max(axis=1)
    worst = np.max(err / np.abs(ref).reshape(codes.shape[0], -1).max(axis=1))
    print("%s n=%d momenta=%s deflated=%s: max |l - ref| / max |ref| = %.2e" % (what, p.n, momenta, deflated, worst))
    assert worst < 1e-10
    return loops


def _check_shifts_parity(p, codes, deflated, what):
    """A mode-4 batch at the shifts 0 and 2L against sparse LU, per probe; returns the estimates."""
    X = utils.probes_as_complex(codes)
    shifts = [0, 2 * p.L]
    p.eng.set_shifts(shifts)
    ests, _, _ = _with_solver_state(p, deflated, lambda: p.eng.hutch_batch_shifts(0, codes, 1e-12, 1000))
    Zs = p.projected_solutions(X, deflated)
    worst = 0.0
    for k in range(codes.shape[0]):
        ref = np.array([np.vdot(np.roll(X[k], -s), Zs[k]) for s in shifts])
        worst = max(worst, np.max(np.abs(ests[k] - ref)) / np.max(np.abs(ref)))
    print("%s n=%d deflated=%s: max |e - ref| / max_j |ref| = %.2e" % (what, p.n, deflated, worst))
    assert worst < 1e-10
    return ests


@pytest.mark.parametrize("kind", ["z2", "z4"])
@pytest.mark.parametrize("deflated", [False, True])
def test_per_probe_parity_16(p16, kind, deflated):
    np.random.seed(21)
    _check_loops_parity(p16, utils.draw_probes(6, p16.n, kind), [0, 1, 15], deflated, "parity")


def test_per_probe_parity_128(p128):
    np.random.seed(22)
    _check_loops_parity(p128, utils.draw_probes(8, p128.n, "z2"), [0, 1], True, "parity")


@pytest.mark.parametrize("kind", ["z2", "z4"])
def test_scalar_sum_is_the_shift_zero_value_16(p16, kind):
    """sum_t (l[0][0][0][t] + l[0][1][1][t]) = x^H z: the mode-5 output summed on the host and sw_hutch_fetch
    after the batch against the shift-0 estimate of a mode-4 batch, same probes, same engine state."""
    p = p16
    np.random.seed(31)
    codes = utils.draw_probes(6, p.n, kind)
    p.eng.set_shifts([0])
    p.eng.set_loop_momenta([0, 3])

    def both():
        e4, _, _ = p.eng.hutch_batch_shifts(0, codes, 1e-12, 1000)
        l5, _, _ = p.eng.hutch_batch_loops(0, codes, 1e-12, 1000)
        first, _, _ = p.eng.hutch_fetch()
        return e4[:, 0], l5, first

    e4, l5, first = _with_solver_state(p, True, both)
    total = np.sum(l5[:, 0, 0, 0, :] + l5[:, 0, 1, 1, :], axis=1)
    rel_host = np.max(np.abs(total - e4) / np.abs(e4))
    rel_dev = np.max(np.abs(first - e4) / np.abs(e4))
    print("scalar sum %s: host sum %.2e, sw_hutch_fetch %.2e relative to the shift-0 value" % (kind, rel_host, rel_dev))
    assert rel_host < 1e-10 and rel_dev < 1e-10


def test_mode_switching_keeps_both_fetches_right(p16):
    p = p16
    np.random.seed(41)
    codes = utils.draw_probes(6, p.n, "z4")
    first4 = _check_shifts_parity(p, codes, True, "mode 4 first")
    loops = _check_loops_parity(p, codes, [0, 1, 15], True, "mode 5 between")
    assert np.array_equal(p.eng.hutch_fetch_shifts(), first4)            # mode 4's buffer survived the mode-5 batch
    again4 = _check_shifts_parity(p, codes, True, "mode 4 again")
    assert np.array_equal(again4, first4)
    assert np.array_equal(p.eng.hutch_fetch_loops(), loops)              # and the reverse


def _golden_loops():
    with open(os.path.join(HERE, "golden", "slice_loops128.json")) as f:
        g = json.load(f)
    return np.array([complex(re, im) for re, im in g["slice_loops128"]]).reshape(g["shape"])


PLAIN_KEYS = {'trace', 'std_dev', 'nr_ests', 'function_iters', 'total_complexity', 'ests', 'rough_trace',
              'level_tol', 'probe_loop_s', 'probes_solved'}
NEW_KEYS = {'momenta', 'loops', 'loop_devs', 'loop_ests', 'converged'}


def test_fixed_length_flow_128_against_the_exact_loops(capsys):
    """2048 probes whatever their variance (tol 1e-9 is never met): every one of the 2 x 2 x 2 x 128 entries
    within 5 loop_devs / sqrt(n) + 1e-9 of the exact value, and the trace within the same bound."""
    golden = _golden_loops()[:2]
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params['timeslice_loops'] = [0, 1]
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    tp = utils.trace_params_from_params(params, "hutchinson")
    tp['max_nr_ests'] = 2048
    tp['tol'] = 1e-9
    res = stoch_trace.hutchinson(A, tp)
    capsys.readouterr()
    nr = res['nr_ests'] + 1
    assert nr == 2048 and res['probes_solved'] == 2048
    assert res['momenta'] == [0, 1]
    assert res['loops'].shape == res['loop_devs'].shape == res['converged'].shape == (2, 2, 2, 128)
    assert res['loop_ests'].shape == (nr, 2, 2, 2, 128)
    diff = np.abs(res['loops'] - golden)
    bound = 5.0 * res['loop_devs'] / np.sqrt(nr) + 1e-9
    ratio = diff / bound
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("loops: worst |diff| / bound = %.3f at [p][a][b][t] = %s (|diff| %.3e, bound %.3e); entries over 3/5 of the "
          "bound: %d of %d" % (ratio[at], at, diff[at], bound[at], int(np.sum(ratio > 0.6)), ratio.size))
    assert np.all(diff < bound)
    tb = 5.0 * res['std_dev'] / np.sqrt(nr) + 1e-9
    print("trace %s |diff| %.3e bound %.3e" % (res['trace'], abs(res['trace'] - 8326.43205953889), tb))
    assert abs(res['trace'] - 8326.43205953889) < tb
    # the per-probe series carry tr1 and average to the reported loops
    assert np.max(np.abs(res['loop_ests'].mean(axis=0) - res['loops'])) < 1e-9
    assert res['ests'].shape == (nr,)


def test_default_flow_128_key_sets(capsys):
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    plain = stoch_trace.hutchinson(A, utils.trace_params_from_params(params, "hutchinson"))   # the same call, no key
    params['timeslice_loops'] = [0, 1]
    res = stoch_trace.hutchinson(A, utils.trace_params_from_params(params, "hutchinson"))
    capsys.readouterr()
    assert set(plain) == PLAIN_KEYS
    assert set(res) == PLAIN_KEYS | NEW_KEYS
    assert res['nr_ests'] >= 5
    assert res['loop_ests'].shape[0] == res['nr_ests'] + 1
    assert res['ests'].shape == (res['nr_ests'] + 1,)
    assert res['function_iters'] >= res['nr_ests'] + 1
    # the control series is the scalar total at p = 0 of the per-probe loops (tr1 included in both)
    total = np.sum(res['loop_ests'][:, 0, 0, 0, :] + res['loop_ests'][:, 0, 1, 1, :], axis=1)
    assert abs(np.mean(total) - res['trace']) < 1e-9 * abs(res['trace'])
