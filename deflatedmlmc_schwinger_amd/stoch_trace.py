"""``hutchinson`` and ``mlmc`` of the reference's stoch_trace.py on the MI355X engine.

Same call surface and result dictionaries.  The reference evaluates one probe at
a time; here the probes of a round are one multi-RHS batch on the GPU (and, with several
ranks, a contiguous slice of the round per GPU).  The probes come from the same seeded
global NumPy stream in the same order, and the sequential stopping rule is replayed over the
gathered per-probe values, so ``trace``, ``std_dev`` and ``nr_ests`` are what the one-by-one
loop would produce with the same per-probe values.
"""
import time
from math import sqrt

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.linalg import LinearOperator

from . import dist as _dist
from .engine import RESOLVED_FETCH, ProbeStream, probe_mode
from .multigrid import MG
from .utils import (_engines, deflation_pre_computations, displacements_of, draw_probes, flopsV_manual,
                    loops_of, mlmc_defl_setup_of, probe_batch, probe_batch_generated, register_loop_momenta,
                    register_shifts, register_two_point, two_point_of, low_mode_inverse, low_mode_two_point,
                    register_low_modes, low_mode_contraction_of, link_loops_of, three_point_of,
                    register_three_point, refuse_three_point, register_smearing, refuse_smearing, smearing_of,
                    distillation_of, refuse_distillation, refuse_distilled_three_point,
                    refuse_two_meson, two_meson_ops_of, two_meson_sums, two_meson_folded,
                    distilled_three_point_of, distilled_three_point_correlator, DISTILLED_INSERTIONS,
                    laplacian_eigenvectors, laph_elementals,
                    distilled_pair_sums, distilled_loops, source_average, distilled_contraction_of)

DEFAULT_BATCH = 256
NR_ROUGH_PROBES = 5


def _stats(values):
    """Mean and population deviation exactly as stoch_trace.py:143-145 writes them."""
    count = len(values)
    avg = np.sum(values) / count
    dev = sqrt(np.sum(np.square(np.abs(values - avg))) / count)
    return avg, dev


def first_stop_index(ests, first_new, level_tol, min_index=5):
    """The first index i >= first_new at which the reference's loop would break,
    `i >= min_index and dev_i / sqrt(i + 1) < level_tol` with (avg_i, dev_i) = _stats(ests[:i + 1])
    (stoch_trace.py:143-154 / 394-406), or None -- without the reference's O(N^2) re-evaluation of the
    statistics per probe: a running-sum screen (one pass, on estimates shifted by a pivot so the
    variance does not cancel) marks the indices whose error estimate is below level_tol or within a
    relative 1e-9 of it -- many orders above the screen's rounding error --, and only those are
    re-evaluated with the reference's own two-pass formula, in order.  Returns (index, avg, dev) of the
    break, or None when the loop runs on."""
    ests = np.asarray(ests, dtype=np.complex128)
    n = ests.size
    lo = max(int(first_new), int(min_index))
    if n == 0 or lo >= n:
        return None
    pivot = np.mean(ests[:min(n, 64)])
    d = ests - pivot
    cnt = np.arange(1, n + 1, dtype=np.float64)
    m1 = np.cumsum(d) / cnt
    m2 = np.cumsum(d.real * d.real + d.imag * d.imag) / cnt
    var = np.maximum(m2 - (m1.real * m1.real + m1.imag * m1.imag), 0.0)
    err = np.sqrt(var / cnt)
    cand = np.flatnonzero(err[lo:] < level_tol * (1.0 + 1e-9) + 1e-300) + lo
    for i in cand:
        avg, dev = _stats(ests[:i + 1])
        if dev / sqrt(i + 1) < level_tol:
            return int(i), avg, dev
    return None


class HostProbes:
    """Probe source for evaluators that take the probes themselves (int8, (k, n)): this rank's
    slice of a round is produced on the host by the C MT19937 stream at its stream positions
    (jump polynomial, no walk over the other ranks' draws)."""

    def __init__(self, evaluate, n, kind="z2"):
        self.evaluate = evaluate
        self.n = n
        self.kind = kind
        self._entry = None

    def begin(self, entry_stream):
        self._entry = entry_stream

    def __call__(self, first_probe, count):
        g = self._entry.copy()
        g.jump(first_probe * self.n)
        return self.evaluate(g.probes(count, self.n, self.kind))


class DeviceProbes:
    """Probe source of the GPU estimators: the engines generate their probes in HBM at the
    probes' stream positions (k_mt_generate) and evaluate them; nothing of size n touches the host.
    `method`, `level` and `deflated` are those of utils.probe_batch_generated.  For a resolved method each probe
    yields one row; `columns` (None: the row as it is) turns the batch's resolved array into the columns of
    run_probe_loop(control=...): loop_columns(., zero) or two_point_columns(., zero).
    For the scalar methods the probes of the round expected next (`round_stride` probes further down the stream,
    set by the loop) are drawn on the engines' generation streams while the current round is being solved."""

    def __init__(self, mg_solver, params, method, level, kind="z2", columns=None, deflated=False):
        self.mg_solver = mg_solver
        self.params = params
        self.method = method
        self.level = level
        self.kind = kind
        self.columns = columns
        self.deflated = deflated       # MODE_MLMC_DEFL_LOOPS: the level's registered projection on the right
        self.prefetches = probe_mode(method, level, deflated=deflated) not in RESOLVED_FETCH
        self.round_stride = 0          # distance (in probes) to this rank's slice of the next round
        self._ready = None

    def begin(self, entry_stream):
        window = entry_stream.window()
        for eng in _engines(self.mg_solver):
            eng.stream_set(window)
        self._ready = None

    def __call__(self, first_probe, count):
        nxt = (first_probe + self.round_stride, count) if self.prefetches and self.round_stride > 0 else None
        e, f, c, self._ready = probe_batch_generated(self.mg_solver, self.params, self.method, self.level,
                                                     first_probe, count, self.kind, prefetch=nxt,
                                                     ready=self._ready, deflated=self.deflated)
        return (e if self.columns is None else self.columns(e)), f, c


def run_probe_loop(evaluate, n, level_tol, max_nr_ests, batch, comm=None, min_index=5,
                   verbose=False, probe_type="z2", control=None):
    """The probe loop of stoch_trace.py:137-154 / 386-406 in rounds of batched probes.

    `evaluate` is a probe source -- called as source(first_probe, count) for the probes
    [first_probe, first_probe + count) of the loop, counted from the position of the global NumPy
    stream on entry (:class:`DeviceProbes`, :class:`HostProbes`) -- or a plain callable
    evaluate(probes[int8, (k, n)]) -> (ests[k], iters_fine[k], iters_coarse[k]), which is wrapped
    in :class:`HostProbes`.  Every rank evaluates only its contiguous slice of a round.
    Returns dict(index, avg, dev, ests, iters_fine, iters_coarse, rounds) where `index` is the
    loop index at which the reference would have left the loop.  On return the global NumPy
    stream sits exactly where the one-by-one loop would have left it.

    control = j: for estimators that return one value per displacement (or loop entry, ...): `evaluate` yields
    ests of shape (count, S) and `level_tol` holds S tolerances.  The sequential stopping rule is replayed on
    column j against level_tol[j] alone, so that column's index, avg and dev are those of the scalar loop on it;
    every other column is summarised over the same first index + 1 probes.  The dictionary (avg, dev: the control
    column; ests: (index + 1, S)) then also has avgs[S], devs[S] and converged[S] = whether each column met its own
    tolerance at the stopping index.  One rank only."""
    comm = comm or _dist.default_comm()
    width = ()
    if control is not None:
        if comm.world > 1:
            raise Exception("displaced traces (x_displacements) run on one rank; got %d" % comm.world)
        level_tols = np.asarray(level_tol, dtype=float)
        width = (level_tols.size,)
        level_tol = level_tols[control]
    source = evaluate if hasattr(evaluate, "begin") else HostProbes(evaluate, n, probe_type)
    entry = ProbeStream.from_numpy_state()
    source.begin(entry)
    ests = np.zeros((0,) + width, dtype=np.complex128)
    it_f = np.zeros(0, dtype=np.int64)
    it_c = np.zeros(0, dtype=np.int64)
    rounds = 0
    stop_index = None
    avg = dev = 0.0

    def series():
        return ests if control is None else ests[:, control]

    while ests.shape[0] < max_nr_ests:
        round_size = min(batch * comm.world, max_nr_ests - ests.shape[0])
        first_new = ests.shape[0]
        lo, hi = comm.my_slice(round_size)
        if hasattr(source, "round_stride"):
            # the next round (if the loop goes on and is a full one) starts round_size probes further on
            source.round_stride = round_size if first_new + 2 * round_size <= max_nr_ests else 0
        if hi > lo:
            e, f, c = source(first_new + lo, hi - lo)
        else:
            e, f, c = np.zeros(0, complex), np.zeros(0, np.int64), np.zeros(0, np.int64)
        e, f, c = comm.allgather_probe_results(e, f, c, round_size)
        if control is not None and e.shape != (round_size,) + width:
            raise Exception("displaced probe batch of shape %s, expected %s" % (e.shape, (round_size,) + width))
        ests = np.concatenate([ests, e])
        it_f = np.concatenate([it_f, f])
        it_c = np.concatenate([it_c, c])
        rounds += 1
        if verbose:
            # the reference's per-probe debug prints (stoch_trace.py:150-152): its own O(N^2) loop
            for i in range(first_new, ests.shape[0]):
                avg, dev = _stats(series()[:i + 1])
                err = dev / sqrt(i + 1)
                print(dev)
                print(err)
                print(level_tol)
                if i >= min_index and err < level_tol:
                    stop_index = i
                    break
        else:
            hit = first_stop_index(series(), first_new, level_tol, min_index)
            if hit is not None:
                stop_index, avg, dev = hit
        if stop_index is not None:
            break
    if stop_index is None:
        stop_index = ests.shape[0] - 1
        avg, dev = _stats(series())
    k = stop_index + 1
    # leave the global stream where the one-by-one loop leaves it: k probes of n draws each
    entry.jump(k * n)
    np.random.set_state(entry.numpy_state())
    out = {"index": stop_index, "avg": avg, "dev": dev, "ests": ests[:k],
           "iters_fine": it_f[:k], "iters_coarse": it_c[:k], "rounds": rounds,
           "solved": int(ests.shape[0])}
    if control is not None:
        per = [_stats(ests[:k, j]) for j in range(width[0])]
        out["avgs"] = np.array([a for a, _ in per])
        out["devs"] = np.array([d for _, d in per])
        out["converged"] = out["devs"] / sqrt(k) < level_tols
    return out


def loop_columns(loops, zero):
    """The columns of the timeslice-loop estimator for run_probe_loop(control=...): loops[k][p][a][b][t] flattened
    per probe, plus one control column, the scalar total sum_t (l[0][0][t] + l[1][1][t]) of momentum index
    `zero` (p = 0) -- the plain Hutchinson value x^H z of the probe."""
    loops = np.asarray(loops, dtype=np.complex128)
    total = np.sum(loops[:, zero, 0, 0, :] + loops[:, zero, 1, 1, :], axis=1)
    return np.concatenate([loops.reshape(loops.shape[0], -1), total[:, None]], axis=1)


def two_point_columns(T, zero):
    """The columns of the two-point estimator for run_probe_loop(control=...): T[k][j][a][b][c][d][t] flattened per
    noise, plus one control column, the pion total sum_t sum_ac T[zero][a][a][c][c][t] = sum_a ||z^(0,a)||^2 of
    momentum index `zero` (p = 0), which is real and positive."""
    T = np.asarray(T, dtype=np.complex128)
    total = sum(np.sum(T[:, zero, a, a, c, c, :], axis=1) for a in range(2) for c in range(2))
    return np.concatenate([T.reshape(T.shape[0], -1), total[:, None]], axis=1)


def _setup_solver(A, params, announce=True, defer_coarse=False, lattice=None):
    mg_solver = MG(A)
    if lattice is not None:
        mg_solver._lat = lattice       # hierarchy.detect_lattice(A), which the caller already ran
    if defer_coarse and "defer_coarse_levels" not in params:
        # build-only: the flow uses level 0 only until its work model at the very end (MG.finish_setup)
        params = dict(params, defer_coarse_levels=True)
    mg_solver.coarsest_iters = 0
    mg_solver.coarsest_iters_tot = 0
    mg_solver.coarsest_iters_avg = 0
    mg_solver.nr_calls = 0
    print("MG setup phase ...", end='', flush=True)
    t0 = time.time()
    mg_solver.setup(dof=params['dof'], aggrs=params['aggrs'], max_levels=params['max_nr_levels'],
                    dim=2, acc_eigvs=params['accuracy_mg_eigvs'],
                    sys_type=params['problem_name'], params=params)
    print(" done. Time : " + str(time.time() - t0) + " seconds")
    print(mg_solver)
    deferred = getattr(mg_solver, "_pending", None) is not None
    nr_levels = mg_solver.total_levels if deferred else len(mg_solver.ml.levels)
    mg_solver.total_levels = nr_levels
    for i in range(nr_levels):
        mg_solver.coarsest_lev_iters[i] = 0
    if nr_levels < 3:
        raise Exception("Use three or more levels.")
    if not deferred:
        for i in range(nr_levels - 1):
            mg_solver.ml.levels[i].P = csr_matrix(mg_solver.ml.levels[i].P)
            mg_solver.ml.levels[i].R = csr_matrix(mg_solver.ml.levels[i].R)
    return mg_solver, nr_levels


def _rough_estimate(mg_solver, params, n, method="hutchinson", columns=None):
    """stoch_trace.py:103-115 / 288-302: seed 123456, the mean of five probes of `method` at level 0 (of their
    `columns`, if given); the caller adds the deflated part."""
    np.random.seed(123456)
    t0 = time.time()
    probes = draw_probes(NR_ROUGH_PROBES, n, params.get('probe_type', 'z2'))
    e, _, _ = probe_batch(mg_solver, params, method, probes, 0)
    if columns is not None:
        e = columns(e)
    rough = np.sum(e[0:NR_ROUGH_PROBES], axis=0) / NR_ROUGH_PROBES
    print(" done. Time : " + str(time.time() - t0) + " seconds")
    return rough


class _Observable:
    """What a Hutchinson-type flow estimates, as hutchinson() and _estimate_stage need it.  This one is the
    plain trace: one scalar series per probe, any number of ranks.  The resolved ones estimate `columns` of each
    probe's row and stop on the column `control`, on one rank (`one_rank`: the refusal otherwise)."""
    what = "trace"                     # ... in the printed lines
    method = "hutchinson"              # of utils.probe_batch / probe_batch_generated
    columns = None                     # the resolved array of a batch -> the columns of the probe loop
    one_rank = None

    def register(self, mg_solver):
        """What the engines have to know besides the deflation vectors."""

    def tr1_columns(self, tr1):
        """The deflated part as deflation_pre_computations returns it -> one value per column."""
        return tr1

    def control(self, rough):
        """The column the stopping rule runs on (None: the estimates are scalars)."""
        return None

    def fill(self, result, loop, tr1_cols, rough, level_tols):
        """The result keys beyond the reference's, from the loop's avgs / devs / ests / converged."""


class _Displaced(_Observable):
    """x_displacements: Tr(A^-1 D_s) at every listed displacement, one column each; the reference's keys are those
    of the control displacement."""
    what = "traces"
    method = "shifts"
    one_rank = "displaced traces (x_displacements) run on one rank"

    def __init__(self, displaced):
        self.disps, self.shifts, self.control_index = displaced

    def register(self, mg_solver):
        register_shifts(mg_solver, self.shifts)

    def tr1_columns(self, tr1):
        return np.asarray(tr1, dtype=np.complex128)

    def control(self, rough):
        return self.control_index

    def fill(self, result, loop, tr1_cols, rough, level_tols):
        result['ests'] = loop["ests"]                   # (nr_ests + 1, S)
        result['displacements'] = list(self.disps)
        result['traces'] = loop["avgs"] + tr1_cols
        result['std_devs'] = loop["devs"]
        result['rough_traces'] = rough
        result['level_tols'] = level_tols
        result['converged'] = loop["converged"]


class _Loops(_Observable):
    """timeslice_loops: the loops l[p][a][b][t], flattened, plus one control column, the scalar total at p = 0, whose
    expectation plus sum(tr1) is Tr(A^-1): the reference's keys are filled from it."""
    what = "loops"
    method = "loops"
    one_rank = "timeslice loops (timeslice_loops) run on one rank"

    def __init__(self, momenta):
        self.momenta = momenta
        self.zero = momenta.index(0)
        self.tr1 = None                # the deflated part [p][a][b][t]

    def columns(self, loops):
        return loop_columns(loops, self.zero)

    def register(self, mg_solver):
        register_loop_momenta(mg_solver, self.momenta)

    def tr1_columns(self, tr1):
        self.tr1 = np.asarray(tr1, dtype=np.complex128)
        return loop_columns(self.tr1[None], self.zero)[0]

    def control(self, rough):
        return rough.size - 1

    def fill(self, result, loop, tr1_cols, rough, level_tols):
        control, shape = rough.size - 1, self.tr1.shape
        result['momenta'] = list(self.momenta)
        result['loops'] = (loop["avgs"][:control] + tr1_cols[:control]).reshape(shape)
        result['loop_devs'] = loop["devs"][:control].reshape(shape)
        result['loop_ests'] = loop["ests"][:, :control].reshape((-1,) + shape) + self.tr1[None]
        result['converged'] = loop["converged"][:control].reshape(shape)


class _LinkLoops(_Loops):
    """link_loops: per probe the local loops l[p][a][b][t] and the four link branches [d][p][a][b][t] as
    one array [5][p][a][b][t] (index 0: local), flattened, plus _Loops' control column, the scalar total of the local
    loops at p = 0, whose series is the plain Hutchinson series."""
    what = "link loops"
    method = "link_loops"
    one_rank = "link loops (link_loops) run on one rank"

    def columns(self, rows):
        rows = np.asarray(rows, dtype=np.complex128)
        total = loop_columns(rows[:, 0], self.zero)[:, -1]
        return np.concatenate([rows.reshape(rows.shape[0], -1), total[:, None]], axis=1)

    def tr1_columns(self, tr1):
        local, link = tr1
        self.tr1 = np.concatenate([np.asarray(local, dtype=np.complex128)[None],
                                   np.asarray(link, dtype=np.complex128)], axis=0)
        return self.columns(self.tr1[None])[0]

    def fill(self, result, loop, tr1_cols, rough, level_tols):
        control, shape = rough.size - 1, self.tr1.shape
        avgs = (loop["avgs"][:control] + tr1_cols[:control]).reshape(shape)
        devs = loop["devs"][:control].reshape(shape)
        ests = loop["ests"][:, :control].reshape((-1,) + shape) + self.tr1[None]
        conv = loop["converged"][:control].reshape(shape)
        result['momenta'] = list(self.momenta)
        result['loops'], result['link_loops'] = avgs[0], avgs[1:]
        result['loop_devs'], result['link_loop_devs'] = devs[0], devs[1:]
        result['loop_ests'], result['link_loop_ests'] = ests[:, 0], ests[:, 1:]
        result['converged'], result['link_converged'] = conv[0], conv[1:]


class _TwoPoint(_Observable):
    """two_point(): the pair sums T[j][a][b][c][d][t], flattened, plus one control column, the pion total."""
    what = "two-point functions"
    method = "two_point"
    one_rank = "two-point functions (source_timeslice) run on one rank"

    def __init__(self, momenta):
        self.zero = momenta.index(0)

    def columns(self, T):
        return two_point_columns(T, self.zero)

    def control(self, rough):
        return rough.size - 1


class _TwoPointSmeared(_TwoPoint):
    """two_point() with smearing_kappa: the pair sums T[i][j][a][b][c][d][t] of every sink level i, flattened, plus
    the pion total of sink level 0 as the control column (real and positive at any source and sink level)."""
    what = "smeared two-point functions"
    method = "two_point_smeared"

    def columns(self, T):
        T = np.asarray(T, dtype=np.complex128)
        total = two_point_columns(T[:, 0], self.zero)[:, -1]
        return np.concatenate([T.reshape(T.shape[0], -1), total[:, None]], axis=1)


class _TwoPointLMA(_TwoPoint):
    """lma_two_point(): the remainders R[j][a][b][c][d][t] = T(z, z) - T(z_L, z_L), flattened, plus their pion total;
    the exact low-mode part E_L(t0) enters as tr1_cols."""
    what = "low-mode averaged two-point functions"
    method = "two_point_lma"


def _estimate_stage(mg_solver, params, n, obs, tr1_cols=None):
    """The second half of a Hutchinson-type flow: the rough estimate from five probes (plus tr1_cols), the level
    tolerances |tol * rough|, the timers' reset and the probe loop of `obs` at level 0.
    Returns (rough, level_tols, control, loop, loop_s); control None: rough and level_tols are scalars."""
    kind = params.get('probe_type', 'z2')
    print("\nComputing rough estimation of the " + obs.what + " ...", end='', flush=True)
    rough = _rough_estimate(mg_solver, params, n, obs.method, obs.columns)
    if tr1_cols is not None:
        rough = rough + tr1_cols
    level_tols = np.abs(params['tol'] * rough)
    control = obs.control(rough)

    print("\nResetting timer to zero ...", end='')
    mg_solver.timer.reset()
    mg_solver.engine.timers_reset()
    print(" done")
    print("\nComputing the " + obs.what + " stochastically ...", end='', flush=True)
    t0 = time.time()
    source = DeviceProbes(mg_solver, params, obs.method, 0, kind, obs.columns)
    # a round = one batch per engine handle (concurrent HIP streams) per rank
    loop = run_probe_loop(source, n, level_tols, params['max_nr_ests'],
                          int(params.get('batch', DEFAULT_BATCH)) * max(1, len(_engines(mg_solver))),
                          verbose=control is None and bool(params.get('verbose', False)),
                          probe_type=kind, control=control)
    loop_s = time.time() - t0
    print(" done. Time : " + str(loop_s) + " seconds")
    return rough, level_tols, control, loop, loop_s


# compute tr(A^{-1}) via (deflated) Hutchinson                      stoch_trace.py:33-179
def hutchinson(A, params):
    """The build-only keys x_displacements (Tr(A^-1 D_s) at every listed displacement; DESIGN.md, "Displaced
    traces"), timeslice_loops (the spin- and momentum-resolved loops l[p][a][b][t] of every timeslice; DESIGN.md
    4c) and link_loops (those loops plus the four point-split link branches, from which utils.conserved_current
    forms the conserved vector current) resolve the estimate, from one deflation projection and one
    solve per probe: the reference's result keys are then those of the control column, and the stopping rule runs on
    its series alone."""
    refuse_distilled_three_point(params, "hutchinson()")
    refuse_two_meson(params, "hutchinson()")
    refuse_three_point(params, "hutchinson()")
    refuse_smearing(params, "hutchinson()")
    refuse_distillation(params, "hutchinson()")
    if two_point_of(params) is not None:
        raise Exception("source_timeslice belongs to two_point(), not to hutchinson()")
    link = link_loops_of(params)
    momenta = loops_of(params) if link is None else None
    displaced = displacements_of(params) if momenta is None and link is None else None
    lattice = None
    if link is not None:
        obs = _LinkLoops(link)
    elif momenta is not None:
        obs = _Loops(momenta)
    elif displaced is not None:
        obs = _Displaced(displaced)
    else:
        obs = _Observable()
    if obs.one_rank and _dist.default_comm().world > 1:
        raise Exception(obs.one_rank)
    if link is not None:
        # the branches pair sites through the links: the operator has to be the lattice stencil the engine detects
        from .hierarchy import detect_lattice
        lattice = A if isinstance(A, tuple) else (None if A is None else detect_lattice(A))
        if lattice is None:
            raise Exception("link_loops needs a lattice operator (a U(1) Wilson stencil with its links)")
    mg_solver, nr_levels = _setup_solver(A, params, defer_coarse=True, lattice=lattice)
    N = A.shape[0]

    print("\nResetting timer to zero ...", end='')
    mg_solver.timer.reset()
    print(" done\n")
    nr_deflat_vctrs = params['nr_deflat_vctrs']
    print("Computing deflation vectors ...", end='', flush=True)
    t0 = time.time()
    Vx, tr1 = deflation_pre_computations(A, nr_deflat_vctrs, params['defl_eigvs_tol_Hutch'],
                                         "hutchinson", mg_solver.timer, params, mg_solver)
    tr1_cols = obs.tr1_columns(tr1)
    obs.register(mg_solver)
    print(" done. Time : " + str(time.time() - t0) + " seconds")
    print(mg_solver.timer)

    mg_solver.coarsest_lev_iters[0] = 0
    rough, level_tols, control, loop, loop_s = _estimate_stage(mg_solver, params, N, obs, tr1_cols)

    def at_control(v):
        return v if control is None else v[control]

    function_iters = int(np.sum(loop["iters_fine"]))
    mg_solver.coarsest_lev_iters[0] = function_iters
    mg_solver.finish_setup()          # the coarse levels (built beside the probe loop): the work model reads their nnz
    result = dict()
    result['trace'] = loop["avg"] + at_control(tr1_cols)
    result['std_dev'] = loop["dev"]
    result['nr_ests'] = loop["index"]
    result['function_iters'] = function_iters
    levels = mg_solver.ml.levels
    result['total_complexity'] = flopsV_manual(len(levels), levels, 0, mg_solver) * function_iters
    result['total_complexity'] += levels[len(levels) - 1].A.nnz * mg_solver.coarsest_lev_iters[0]
    # stoch_trace.py:173-175 (hard-coded 1/3 kept)
    result['total_complexity'] += result['nr_ests'] * (2 * N * nr_deflat_vctrs) / 3.0
    # build-only extras (not in the reference's dictionary)
    result['ests'] = loop["ests"] if control is None else loop["ests"][:, control]      # (nr_ests + 1,)
    result['rough_trace'] = at_control(rough)
    result['level_tol'] = at_control(level_tols)
    result['probe_loop_s'] = loop_s                 # wall clock of the probe loop and what it solved
    result['probes_solved'] = loop["solved"]        # (whole rounds: >= nr_ests + 1)
    obs.fill(result, loop, tr1_cols, rough, level_tols)
    mg_solver.sync_timer()
    print(mg_solver.timer)
    return result


def two_point(A, params):
    """Connected meson two-point functions by the one-end trick.  The build-only keys
    source_timeslice = t0 and two_point_momenta = [p_0, ...] (default [0]; it has to contain 0) select the sources:
    per noise k one Z2 / Z4 vector xi_k(y) on the timeslice t0 -- the code of probe k of the usual stream at
    idx(0, y, t0) -- is solved for at both spins and every momentum, 2 M solves without deflation, and

        T_k[j][a][b][c][d][t] = sum_x e^{-2 pi i p_j x / L} conj(z_k^(0,a)[idx(c,x,t)]) z_k^(j,b)[idx(d,x,t)]

    averages to sum_{x,y} e^{-2 pi i p_j (x - y) / L} conj(A^-1[idx(c,x,t), idx(a,y,t0)]) A^-1[idx(d,x,t),
    idx(b,y,t0)]; utils.meson_correlator contracts it into any of the 16 channels.  No fermion-loop sign is
    applied.  The columns of the probe loop are the flattened T plus one control column, the pion total
    sum_t C_pi(t, 0), which is real and positive, and the stopping rule runs on it alone.  `batch` counts noises;
    the solve is 2 M batch columns wide.

    With the build-only key smearing_kappa (source_smearing_steps, default 0, and sink_smearing_steps,
    default [0], go with it) the quark fields are smeared with utils.smear: the sources on their timeslice after the
    phase, the solutions on every timeslice at each listed sink level.  The arrays then carry a leading axis over the
    sink levels, the control column is the pion total of the first level, and the result carries the three keys
    back.  The operator has to be the lattice stencil the engine detects.

    Returns two_point (the mean, [p][a][b][c][d][t]), two_point_devs, two_point_ests (per noise), converged,
    momenta, source_timeslice, nr_ests, function_iters (a noise counts the largest iteration number among its
    2 M solves), ests (the control series), probe_loop_s and probes_solved."""
    refuse_distilled_three_point(params, "two_point()")
    refuse_two_meson(params, "two_point()")
    refuse_three_point(params, "two_point()")
    refuse_distillation(params, "two_point()")
    sel = two_point_of(params)
    if sel is None:
        raise Exception("two_point() needs the key source_timeslice")
    t0, momenta = sel
    smearing = smearing_of(params)
    obs = _TwoPoint(momenta) if smearing is None else _TwoPointSmeared(momenta)
    if _dist.default_comm().world > 1:
        raise Exception(obs.one_rank)
    lattice = None
    if smearing is not None:
        # H pairs sites through the links: the operator has to be the lattice stencil the engine detects
        from .hierarchy import detect_lattice
        lattice = A if isinstance(A, tuple) else (None if A is None else detect_lattice(A))
        if lattice is None:
            raise Exception("smearing_kappa needs a lattice operator (a U(1) Wilson stencil with its links)")
    mg_solver, nr_levels = _setup_solver(A, params, defer_coarse=True, lattice=lattice)
    shape = (len(momenta), 2, 2, 2, 2, int(params['latt_dims'][0]))
    register_two_point(mg_solver, t0, momenta)
    if smearing is not None:
        shape = (len(smearing['sink']),) + shape
        register_smearing(mg_solver, smearing)
    _, _, control, loop, loop_s = _estimate_stage(mg_solver, params, A.shape[0], obs)

    mg_solver.finish_setup()
    result = dict()
    result['two_point'] = loop["avgs"][:control].reshape(shape)
    result['two_point_devs'] = loop["devs"][:control].reshape(shape)
    result['two_point_ests'] = loop["ests"][:, :control].reshape((-1,) + shape)
    result['converged'] = loop["converged"][:control].reshape(shape)
    result['momenta'] = list(momenta)
    result['source_timeslice'] = t0
    if smearing is not None:
        result['smearing_kappa'] = smearing['kappa']
        result['source_smearing_steps'] = smearing['source']
        result['sink_smearing_steps'] = list(smearing['sink'])
    result['nr_ests'] = loop["index"]
    result['function_iters'] = int(np.sum(loop["iters_fine"]))
    result['ests'] = loop["ests"][:, control]       # (nr_ests + 1,): sum_t C_pi(t, 0) per noise
    result['probe_loop_s'] = loop_s
    result['probes_solved'] = loop["solved"]
    mg_solver.sync_timer()
    print(mg_solver.timer)
    return result


def distilled_two_point(A, params):
    """Distillation: the quark fields projected onto the distillation_vectors = N lowest eigenvectors
    of the gauge-covariant spatial Laplacian of every timeslice, box(t) = sum_m v_m v_m^H.  For every listed source
    timeslice the engine solves the 2 N eigenvector sources and projects the solutions on the device
    (Engine.perambulators); the perambulators tau(t, t0) are exact -- no noise, no stopping rule -- and every
    connected correlator follows from them, on the host or (distilled_contraction = "device") by the
    engine's contraction kernels with the perambulator blocks staying on the device (Engine.distilled_two_point):

        two_point[s][p][a][b][c][d][t]   utils.distilled_pair_sums: two_point()'s pair sums with box(t) A^-1 box(t0) in
                                         place of A^-1 (utils.meson_correlator applies unchanged)
        two_point_avg[p][a][b][c][d][dt] their mean over the sources at t = t0 + dt mod L
        loops[p][a][b][t]                utils.distilled_loops on the source timeslices, NaN elsewhere

    Keys (utils.distillation_of): distillation_vectors, source_timeslices (a list, or "all"), two_point_momenta
    (default [0]; need not contain 0), keep_perambulators (default True), distilled_contraction ("host", the default,
    or "device"; utils.distilled_contraction_of).  The sources go to the engine in chunks of
    max(1, 256 // (2 N)) timeslices, one 256-column solve block each, and are contracted chunk by chunk: with
    keep_perambulators false nothing of the size of all perambulators is retained.  One rank; the operator has to be the
    lattice stencil the engine detects.

    Returns two_point, two_point_avg, loops, perambulators ([s][t][c][m][n][a], or None), eigenvalues ([t][m]),
    momenta, source_timeslices, distillation_vectors, function_iters (summed over all columns), solves and
    solve_s."""
    refuse_distilled_three_point(params, "distilled_two_point()")
    refuse_two_meson(params, "distilled_two_point()")
    sel = distillation_of(params)
    if sel is None:
        raise Exception("distilled_two_point() needs the key distillation_vectors")
    on_device = distilled_contraction_of(params) == "device"
    if _dist.default_comm().world > 1:
        raise Exception("distilled two-point functions run on one rank")
    # H pairs sites through the links: the operator has to be the lattice stencil the engine detects
    from .hierarchy import detect_lattice
    lattice = A if isinstance(A, tuple) else (None if A is None else detect_lattice(A))
    if lattice is None:
        raise Exception("distillation_vectors needs a lattice operator (a U(1) Wilson stencil with its links)")
    nev, t0s, momenta = sel['nev'], sel['t0s'], sel['momenta']
    L = int(params['latt_dims'][0])
    mg_solver, nr_levels = _setup_solver(A, params, defer_coarse=True, lattice=lattice)
    engs = _engines(mg_solver)
    if not engs:
        raise Exception("no GPU engine attached (run MG.setup first)")
    eng = engs[0]
    V, eigenvalues = laplacian_eigenvectors(lattice[2], L, nev)
    eng.set_distillation(V)
    if on_device:
        eng.set_distillation_momenta(momenta)
    else:
        M = laph_elementals(V, L, momenta)
    n = 2 * L * L
    tol, maxiter = params['function_params']['tol'], (n if n < 1000 else 1000)

    print("\nResetting timer to zero ...", end='')
    mg_solver.timer.reset()
    eng.timers_reset()
    print(" done")
    print("\nComputing the perambulators ...", end='', flush=True)
    T = np.zeros((len(t0s), len(momenta), 2, 2, 2, 2, L), dtype=np.complex128)
    loops = np.full((len(momenta), 2, 2, L), np.nan + 0j, dtype=np.complex128)
    kept = [] if sel['keep'] else None
    iters, solve_s = 0, 0.0
    chunk = max(1, 256 // (2 * nev))
    for first in range(0, len(t0s), chunk):
        part = t0s[first:first + chunk]
        t1 = time.time()
        if on_device:
            Tp, lp, tau, it = eng.distilled_two_point(part, tol, maxiter, keep=sel['keep'])
            solve_s += time.time() - t1
            T[first:first + len(part)] = Tp
            loops[..., part] = lp.transpose(1, 2, 3, 0)                    # [s][p][a][b] -> [p][a][b][t0s[s]]
        else:
            tau, it = eng.perambulators(part, tol, maxiter)
            solve_s += time.time() - t1
            T[first:first + len(part)] = distilled_pair_sums(tau, M, part)
            lp = distilled_loops(tau, M, part)
            loops[..., part] = lp[..., part]
        iters += int(np.sum(it))
        if kept is not None:
            kept.append(tau)
    print(" done. Time : " + str(solve_s) + " seconds")
    eng.set_distillation(None)

    mg_solver.finish_setup()
    result = dict()
    result['two_point'] = T
    result['two_point_avg'] = source_average(T, t0s)
    result['loops'] = loops
    result['perambulators'] = np.concatenate(kept, axis=0) if kept is not None else None
    result['eigenvalues'] = eigenvalues
    result['momenta'] = list(momenta)
    result['source_timeslices'] = list(t0s)
    result['distillation_vectors'] = nev
    result['function_iters'] = iters
    result['solves'] = 2 * nev * len(t0s)
    result['solve_s'] = solve_s
    mg_solver.sync_timer()
    print(mg_solver.timer)
    return result


def distilled_two_meson(A, params):
    """Two-meson correlators in the distilled basis: two mesons at the source timeslice and two at the
    sink (the pi-pi type, isospin-2 channel) need only the source-to-sink perambulators of distilled_two_point() --
    nothing more is solved.  For the sink operators k = (Gamma_k, p_k) and the source operators k' = (Gamma'_k', p_k')

        C1[s][k][k'][t]           tr[Q_k S_k']            the single-meson correlator (utils.two_meson_sums)
        C2[s][k][l][k'][l'][t]    tr[Q_k S_k' Q_l S_l']   the chain of four perambulators
        C1_avg, C2_avg            their utils.source_average over the sources at t = t0 + dt mod L

    from which utils.two_meson_correlator forms the direct and crossed diagrams and their isospin-2 combination.

    Keys (utils.two_meson_ops_of): distillation_vectors, source_timeslices, two_point_momenta and distilled_contraction
    as distilled_two_point() takes them; meson_operators, a list of 1 to 4 pairs (spin matrix out of '1', 'g3', 's1',
    's2', momentum out of two_point_momenta); source_operators, the same form (default: meson_operators).  With
    distilled_contraction = "host" (the default) the perambulators come back chunk by chunk (Engine.perambulators) and
    NumPy contracts them; with "device" the engine's kernels do and no perambulator leaves the device
    (Engine.distilled_two_meson).  One rank; the operator has to be the lattice stencil the engine detects.

    Returns C1, C2, C1_avg, C2_avg, operators, source_operators, momenta, source_timeslices, distillation_vectors,
    eigenvalues, function_iters, solves and solve_s."""
    refuse_distilled_three_point(params, "distilled_two_meson()")
    sel = two_meson_ops_of(params)
    if sel is None:
        raise Exception("distilled_two_meson() needs the keys distillation_vectors and meson_operators")
    on_device = distilled_contraction_of(params) == "device"
    if _dist.default_comm().world > 1:
        raise Exception("distilled two-meson correlators run on one rank")
    from .hierarchy import detect_lattice
    lattice = A if isinstance(A, tuple) else (None if A is None else detect_lattice(A))
    if lattice is None:
        raise Exception("distilled_two_meson() needs a lattice operator (a U(1) Wilson stencil with its links)")
    nev, t0s, momenta = sel['nev'], sel['t0s'], sel['momenta']
    sink_ops, source_ops = sel['sink_ops'], sel['source_ops']
    nk, nkp = len(sink_ops), len(source_ops)
    L = int(params['latt_dims'][0])
    mg_solver, nr_levels = _setup_solver(A, params, defer_coarse=True, lattice=lattice)
    engs = _engines(mg_solver)
    if not engs:
        raise Exception("no GPU engine attached (run MG.setup first)")
    eng = engs[0]
    V, eigenvalues = laplacian_eigenvectors(lattice[2], L, nev)
    n = 2 * L * L
    tol, maxiter = params['function_params']['tol'], (n if n < 1000 else 1000)
    C1 = np.zeros((len(t0s), nk, nkp, L), dtype=np.complex128)
    C2 = np.zeros((len(t0s), nk, nk, nkp, nkp, L), dtype=np.complex128)
    iters, solve_s = 0, 0.0
    try:                                   # the registrations and the deferred set-up do not outlive a failed call
        eng.set_distillation(V)
        if on_device:
            eng.set_distillation_momenta(momenta)
            G, H = two_meson_folded(sink_ops, source_ops, len(momenta), "distilled_two_meson()")
        else:
            M = laph_elementals(V, L, momenta)

        print("\nResetting timer to zero ...", end='')
        mg_solver.timer.reset()
        eng.timers_reset()
        print(" done")
        print("\nComputing the two-meson building blocks ...", end='', flush=True)
        chunk = max(1, 256 // (2 * nev))
        for first in range(0, len(t0s), chunk):
            part = t0s[first:first + chunk]
            t1 = time.time()
            if on_device:
                c1, c2, it = eng.distilled_two_meson(part, G, H, tol, maxiter)
            else:
                tau, it = eng.perambulators(part, tol, maxiter)
                c1, c2 = two_meson_sums(tau, M, part, sink_ops, source_ops)
            solve_s += time.time() - t1
            C1[first:first + len(part)], C2[first:first + len(part)] = c1, c2
            iters += int(np.sum(it))
        print(" done. Time : " + str(solve_s) + " seconds")
    finally:
        eng.set_distillation(None)
        mg_solver.finish_setup()

    result = dict()
    result['C1'], result['C2'] = C1, C2
    result['C1_avg'], result['C2_avg'] = source_average(C1, t0s), source_average(C2, t0s)
    result['operators'] = list(sel['operators'])
    result['source_operators'] = list(sel['source_operators'])
    result['momenta'] = list(momenta)
    result['source_timeslices'] = list(t0s)
    result['distillation_vectors'] = nev
    result['eigenvalues'] = eigenvalues
    result['function_iters'] = iters
    result['solves'] = 2 * nev * len(t0s)
    result['solve_s'] = solve_s
    mg_solver.sync_timer()
    print(mg_solver.timer)
    return result


def distilled_three_point(A, params):
    """Three-point functions in the distilled basis: both outer quark lines are eigenvector sources,
    one on source_timeslice = t0 and one on sink_timeslice = tf, so no sequential solve is needed.  One engine call
    (Engine.generalized_perambulators) solves the 2 x 2 N columns, keeps both solution blocks on the device and sums
    them at every insertion timeslice and momentum into the generalized perambulators G; from G and the perambulator
    tau(tf, t0) every source matrix, sink matrix and momentum is a small host contraction
    (utils.distilled_three_point_correlator) -- nothing is solved again and there is no noise.

    Keys (utils.distilled_three_point_of): distillation_vectors, source_timeslice, sink_timeslice, sink_gamma (default
    'g3'), sink_momentum (default 0), three_point_momenta (default [0]), insertion_timeslices (a list, or "all", the
    default) and source_momentum (default 0).  One rank; the operator has to be the lattice stencil the engine detects.

    Returns three_point ([6 insertions '1', 'g3', 's1', 's2', 'Jx', 'Jt'][4 source matrices '1', 'g3', 's1',
    's2'][momentum][insertion timeslice], for the given sink matrix and momenta), generalized_perambulators
    ([t][q][6][(m,e)][(n,b)]), perambulators (the two tau of [t0, tf], [s][t][c][m][n][a]: utils.distilled_pair_sums
    gives the two-point function of the ratio), eigenvalues, momenta, insertion_timeslices, source_timeslice,
    sink_timeslice, sink_gamma, sink_momentum, source_momentum, distillation_vectors, function_iters, solves and
    solve_s."""
    refuse_two_meson(params, "distilled_three_point()")
    sel = distilled_three_point_of(params)
    if sel is None:
        raise Exception("distilled_three_point() needs the keys distillation_vectors, source_timeslice and "
                        "sink_timeslice")
    if _dist.default_comm().world > 1:
        raise Exception("distilled three-point functions run on one rank")
    from .hierarchy import detect_lattice
    lattice = A if isinstance(A, tuple) else (None if A is None else detect_lattice(A))
    if lattice is None:
        raise Exception("distilled_three_point() needs a lattice operator (a U(1) Wilson stencil with its links)")
    nev, t0, tf, momenta, tins = sel['nev'], sel['t0'], sel['tf'], sel['momenta'], sel['tins']
    L = int(params['latt_dims'][0])
    mg_solver, nr_levels = _setup_solver(A, params, defer_coarse=True, lattice=lattice)
    engs = _engines(mg_solver)
    if not engs:
        raise Exception("no GPU engine attached (run MG.setup first)")
    eng = engs[0]
    V, eigenvalues = laplacian_eigenvectors(lattice[2], L, nev)
    eng.set_distillation(V)
    ends = sorted({sel['pf'], sel['pi']})
    M = laph_elementals(V, L, ends)
    n = 2 * L * L
    tol, maxiter = params['function_params']['tol'], (n if n < 1000 else 1000)

    print("\nResetting timer to zero ...", end='')
    mg_solver.timer.reset()
    eng.timers_reset()
    print(" done")
    print("\nComputing the generalized perambulators ...", end='', flush=True)
    t1 = time.time()
    try:
        G, tau, it = eng.generalized_perambulators(t0, tf, tins, momenta, tol, maxiter)
        solve_s = time.time() - t1
    finally:                               # the registration and the deferred set-up do not outlive a failed call
        eng.set_distillation(None)
        mg_solver.finish_setup()
    print(" done. Time : " + str(solve_s) + " seconds")

    sources = ('1', 'g3', 's1', 's2')
    C3 = np.zeros((len(DISTILLED_INSERTIONS), len(sources), len(momenta), len(tins)), dtype=np.complex128)
    Ms, Mi = M[ends.index(sel['pf']), tf], M[ends.index(sel['pi']), t0]
    for i, insertion in enumerate(DISTILLED_INSERTIONS):
        for s, source in enumerate(sources):
            C3[i, s] = distilled_three_point_correlator(G, tau[0, tf], Ms, Mi, sel['sink'], insertion, source)

    result = dict()
    result['three_point'] = C3
    result['generalized_perambulators'] = G
    result['perambulators'] = tau
    result['eigenvalues'] = eigenvalues
    result['momenta'] = list(momenta)
    result['insertion_timeslices'] = list(tins)
    result['source_timeslice'], result['sink_timeslice'] = t0, tf
    result['sink_gamma'], result['sink_momentum'], result['source_momentum'] = sel['sink'], sel['pf'], sel['pi']
    result['distillation_vectors'] = nev
    result['function_iters'] = int(np.sum(it))
    result['solves'] = 4 * nev
    result['solve_s'] = solve_s
    mg_solver.sync_timer()
    print(mg_solver.timer)
    return result


class _ThreePoint(_Observable):
    """three_point(): the sums S[d][j][a][b][f][c][t], flattened, plus one control column, c_k = the pion two-point value
    at the sink slice (real and positive) -- a batch's row as Engine.hutch_fetch_three_point_resolved returns it."""
    what = "three-point functions"
    method = "three_point"
    one_rank = "three-point functions (sink_timeslice) run on one rank"

    @staticmethod
    def columns(rows):
        return np.asarray(rows, dtype=np.complex128)

    def control(self, rough):
        return rough.size - 1


def three_point(A, params):
    """Three-point functions source -> insertion at t -> sink at tf from sequential one-end-trick solves (DESIGN.md
    4j).  The build-only keys source_timeslice = t0, sink_timeslice = tf != t0, sink_gamma (default 'g3'),
    sink_momentum (default 0) and three_point_momenta = [q_0, ...] (default [0]) select the chain: per noise k the two
    spin sources of two_point() at momentum 0 give z_k^a, the sequential sources through the sink (utils.seq_sources)
    give zeta_k^a, 2 + 2 solves without deflation to the same tolerance, and

        S_k[d][j][a][b][f][c][t],  d = (local, F_x, B_x, F_t, B_t)        (utils.seq_dots)

    is what utils.three_point_correlator (a local insertion, any source matrix) and utils.three_point_current (the
    conserved vector current) contract.  No fermion-loop sign is applied.  The columns of the probe loop are the
    flattened S plus one control column, c_k = sum_{a,c,x} |z_k^a[idx(c,x,tf)]|^2 -- the pion two-point value
    C_2(tf) of the noise, real and positive, the denominator of the usual ratio C_3 / C_2 -- and the stopping rule runs
    on it alone.  `batch` counts noises; each solve is 2 batch columns wide.  One rank; the operator has to be the
    lattice stencil the engine detects (the link branches need its links).

    Returns three_point (the mean, [d][j][a][b][f][c][t]), three_point_devs, three_point_ests (per noise),
    three_point_converged, sink_two_point (mean and deviation of c_k), momenta, source_timeslice, sink_timeslice,
    sink_gamma, sink_momentum, and the reference's keys from the control series: trace (= the mean of c_k), std_dev,
    nr_ests, function_iters (a noise counts its largest stage-1 plus its largest stage-2 iteration number), ests,
    rough_trace, level_tol, probe_loop_s and probes_solved."""
    refuse_distilled_three_point(params, "three_point()")
    refuse_two_meson(params, "three_point()")
    refuse_smearing(params, "three_point()")
    refuse_distillation(params, "three_point()")
    sel = three_point_of(params)
    if sel is None:
        raise Exception("three_point() needs the keys source_timeslice and sink_timeslice")
    obs = _ThreePoint()
    if _dist.default_comm().world > 1:
        raise Exception(obs.one_rank)
    from .hierarchy import detect_lattice
    lattice = A if isinstance(A, tuple) else (None if A is None else detect_lattice(A))
    if lattice is None:
        raise Exception("three_point() needs a lattice operator (a U(1) Wilson stencil with its links)")
    mg_solver, nr_levels = _setup_solver(A, params, defer_coarse=True, lattice=lattice)
    shape = (5, len(sel['momenta']), 2, 2, 2, 2, int(params['latt_dims'][0]))
    register_three_point(mg_solver, sel)
    rough, level_tols, control, loop, loop_s = _estimate_stage(mg_solver, params, A.shape[0], obs)

    mg_solver.finish_setup()
    result = dict()
    result['three_point'] = loop["avgs"][:control].reshape(shape)
    result['three_point_devs'] = loop["devs"][:control].reshape(shape)
    result['three_point_ests'] = loop["ests"][:, :control].reshape((-1,) + shape)
    result['three_point_converged'] = loop["converged"][:control].reshape(shape)
    result['sink_two_point'] = (loop["avg"], loop["dev"])
    result['momenta'] = list(sel['momenta'])
    result['source_timeslice'], result['sink_timeslice'] = sel['t0'], sel['tf']
    result['sink_gamma'], result['sink_momentum'] = sel['sink'], sel['pf']
    result['trace'] = loop["avg"]
    result['std_dev'] = loop["dev"]
    result['nr_ests'] = loop["index"]
    result['function_iters'] = int(np.sum(loop["iters_fine"]))
    result['ests'] = loop["ests"][:, control]       # (nr_ests + 1,): c_k per noise
    result['rough_trace'] = rough[control]
    result['level_tol'] = level_tols[control]
    result['probe_loop_s'] = loop_s
    result['probes_solved'] = loop["solved"]
    mg_solver.sync_timer()
    print(mg_solver.timer)
    return result


def lma_two_point(A, params):
    """two_point() with low-mode averaging: the nr_deflat_vctrs > 0 lowest eigenvectors V of gamma_3 A
    (hutchinson()'s deflation step) give the low-mode inverse A_L^-1 = V G V^H gamma_3, G = (V^H gamma_3 A V)^-1 made
    Hermitian.  Its pair sums E_L[p][a][b][c][d][t][t0] are exact, from the device meson fields of V, for every source
    timeslice; the noises estimate only the remainder R_k = T(z_k, z_k) - T(z_L, z_L), z_L = A_L^-1 eta_k, whose
    expectation is E[T] - E_L(t0) for any V and G.  Keys, sources, probe loop and stopping rule are two_point()'s; the
    level tolerances are relative to E_L(t0) plus the rough remainder, i.e. to the full correlator.  The build-only key
    low_mode_contraction says where E_L is contracted from the fields: "host" (the default: the fields are read back
    and contracted in NumPy) or "device" (Engine.low_mode_two_point, the fields never leave the device; the two differ
    in rounding only).

    Returns two_point()'s keys with two_point = E_L(t0) + the remainder's mean, plus two_point_low (E_L, all t0),
    two_point_rest (the remainder's mean), two_point_rest_devs and nr_deflat_vctrs; two_point_ests are the per-noise
    remainders plus E_L(t0)."""
    refuse_distilled_three_point(params, "lma_two_point()")
    refuse_two_meson(params, "lma_two_point()")
    refuse_three_point(params, "lma_two_point()")
    refuse_smearing(params, "lma_two_point()")
    refuse_distillation(params, "lma_two_point()")
    sel = two_point_of(params)
    if sel is None:
        raise Exception("lma_two_point() needs the key source_timeslice")
    t0, momenta = sel
    contraction = low_mode_contraction_of(params)
    nr_deflat_vctrs = int(params['nr_deflat_vctrs'])
    if nr_deflat_vctrs <= 0:
        raise Exception("lma_two_point() needs nr_deflat_vctrs > 0 (two_point() is the estimator without low modes)")
    obs = _TwoPointLMA(momenta)
    if _dist.default_comm().world > 1:
        raise Exception(obs.one_rank)
    mg_solver, nr_levels = _setup_solver(A, params, defer_coarse=True)
    L = int(params['latt_dims'][0])
    shape = (len(momenta), 2, 2, 2, 2, L)

    print("Computing deflation vectors ...", end='', flush=True)
    t1 = time.time()
    plain = dict(params, use_permuted=False)
    Ux, _ = deflation_pre_computations(A, nr_deflat_vctrs, params['defl_eigvs_tol_Hutch'], "hutchinson",
                                       mg_solver.timer, plain, mg_solver)
    g3 = mg_solver.ml.levels[0].g3
    V = np.ascontiguousarray(g3 * np.asarray(Ux))          # the eigenvectors up to their signs: gamma_3^2 = 1
    eng = mg_solver.engine
    QV = np.asarray(g3 * eng.apply_dirac(0, 0, np.ascontiguousarray(V.T)).T)
    G = low_mode_inverse(V, QV)
    for e in _engines(mg_solver):
        e.set_deflation(V)
    register_low_modes(mg_solver, G)
    low = np.empty(shape + (L,), dtype=np.complex128)
    for j, p in enumerate(momenta):
        if contraction == "device":
            low[j] = eng.low_mode_two_point(p)
        else:
            low[j] = low_mode_two_point(eng.meson_fields(p, nr_deflat_vctrs)[None], G)[0]
    print(" done. Time : " + str(time.time() - t1) + " seconds")
    register_two_point(mg_solver, t0, momenta)
    tr1_cols = obs.columns(low[None, ..., t0])[0]
    _, _, control, loop, loop_s = _estimate_stage(mg_solver, params, A.shape[0], obs, tr1_cols)

    mg_solver.finish_setup()
    result = dict()
    result['two_point_low'] = low
    result['two_point_rest'] = loop["avgs"][:control].reshape(shape)
    result['two_point_rest_devs'] = loop["devs"][:control].reshape(shape)
    result['two_point'] = low[..., t0] + result['two_point_rest']
    result['two_point_devs'] = result['two_point_rest_devs']
    result['two_point_ests'] = loop["ests"][:, :control].reshape((-1,) + shape) + low[None, ..., t0]
    result['converged'] = loop["converged"][:control].reshape(shape)
    result['momenta'] = list(momenta)
    result['source_timeslice'] = t0
    result['nr_deflat_vctrs'] = nr_deflat_vctrs
    result['nr_ests'] = loop["index"]
    result['function_iters'] = int(np.sum(loop["iters_fine"]))
    result['ests'] = loop["ests"][:, control] + tr1_cols[control]
    result['probe_loop_s'] = loop_s
    result['probes_solved'] = loop["solved"]
    mg_solver.sync_timer()
    print(mg_solver.timer)
    return result


# ---- the pieces mlmc() and the MLMC loop flows share -------------------------------------------------------
def _skip_level_of(params):
    """mlmc_levels_to_skip: whether the second level is skipped (the only form allowed)."""
    skip_list = params['mlmc_levels_to_skip']
    if len(skip_list) > 1:
        raise Exception("Only allowed to skip one level for now")
    skip_level = len(skip_list) == 1
    if skip_level and not skip_list[0] == 1:
        raise Exception("Only allowed to skip the second level for now")
    return skip_level


def _level_tol_fctr(i, nr_levels, skip_level):
    """The share of the tolerance that level i takes (stoch_trace.py:327-336, 376-384); i = nr_levels - 1, the
    coarsest level estimated stochastically, takes the share of the last difference level."""
    if nr_levels < 3:
        raise Exception("Number of levels restricted to >2 for now ...")
    if nr_levels == 3:
        frac0, frac1 = 0.8, 0.2
    else:
        frac0, frac1 = 0.45, 0.45
    if skip_level:
        frac0 = frac0 + frac1
    if i == 0:
        return sqrt(frac0)
    if i == 1:
        return sqrt(frac1)
    if nr_levels == 3:                  # the coarsest level of three
        return sqrt(1.0 - frac0) if skip_level else sqrt(frac1)
    if skip_level:
        return sqrt(1.0 - frac0) / sqrt(nr_levels - 3)
    return sqrt(1.0 - frac0 - frac1) / sqrt(nr_levels - 3)


def _diff_operator(mg_solver, ix):
    """The difference operator (A_f^-1 - P A_c^-1 R) g3 of level ix for ARPACK            stoch_trace.py:257-270"""
    mg_solver.level_for_diff_op = ix
    n_ix = mg_solver.ml.levels[ix].A.shape[0]
    return LinearOperator((n_ix, n_ix), dtype=np.complex128,
                          matvec=lambda v: mg_solver.diff_op_Q(np.array(v, dtype=np.complex128)))


def _mlmc_output(nr_levels, rough_trace, per_level=None):
    """The result dictionary of the MLMC flows before any level ran; per_level(): further keys of every level."""
    output_params = {'nr_levels': nr_levels, 'trace': 0.0, 'total_complexity': 0.0,
                     'std_dev': 0.0, 'results': [], 'rough_trace': rough_trace}
    for i in range(nr_levels):
        output_params['results'].append({'function_iters': 0, 'nr_ests': 0, 'ests_avg': 0.0,
                                         'ests_dev': 0.0, 'level_complexity': 0.0})
        if per_level is not None:
            output_params['results'][i].update(per_level())
    return output_params


def _mlmc_work_model(output_params, mg_solver):
    """stoch_trace.py:443-467: the levels' complexities, their total and the total trace."""
    levels = mg_solver.ml.levels
    nr_levels = output_params['nr_levels']
    last = nr_levels - 1
    for i in range(nr_levels - 1):
        res = output_params['results'][i]
        res['level_complexity'] = res['function_iters'] * flopsV_manual(i, levels, i, mg_solver)
        res['level_complexity'] += levels[last].A.nnz * mg_solver.coarsest_lev_iters[i]
    nc = levels[last].A.shape[0]
    output_params['results'][last]['level_complexity'] = \
        pow(nc, 3) + output_params['results'][last]['function_iters'] * pow(nc, 2)
    for i in range(nr_levels):
        output_params['total_complexity'] += output_params['results'][i]['level_complexity']
        output_params['trace'] += output_params['results'][i]['ests_avg']


# compute tr(A^{-1}) via multigrid multilevel Monte Carlo          stoch_trace.py:185-471
def mlmc(A, params):
    refuse_distilled_three_point(params, "mlmc()")
    refuse_two_meson(params, "mlmc()")
    refuse_three_point(params, "mlmc()")
    refuse_smearing(params, "mlmc()")
    refuse_distillation(params, "mlmc()")
    if two_point_of(params) is not None:
        raise Exception("source_timeslice belongs to two_point(), not to mlmc()")
    if loops_of(params) is not None:
        raise Exception("timeslice_loops is implemented for hutchinson() only: the MLMC coarse terms need a "
                        "timeslice projection per level (mlmc_loops() has it)")
    if link_loops_of(params) is not None:
        raise Exception("link_loops is implemented for hutchinson() only: the MLMC levels have no links")
    if displacements_of(params) is not None:
        raise Exception("x_displacements is implemented for hutchinson() only: the MLMC difference levels "
                        "need their own displaced right-hand sides")
    mlmc_defl_setup_of(params)
    skip_level = _skip_level_of(params)

    mg_solver, nr_levels = _setup_solver(A, params)
    N = A.shape[0]
    batch = int(params.get('batch', DEFAULT_BATCH))
    kind = params.get('probe_type', 'z2')
    mg_solver.skip_level = skip_level

    print("\nResetting timer to zero ...", end='')
    mg_solver.timer.reset()
    print(" done\n")
    print("Computing deflation vectors ...", end='', flush=True)
    t0 = time.time()
    nr_deflat_vctrs = params['mlmc_deflat_vctrs']
    tolx = params['defl_eigvs_tol_MLMC']
    tr1s = []
    for ix in range(nr_levels - 1):
        if skip_level and ix == 1:
            tr1s.append(0.0)
            continue
        _, _, tr1 = deflation_pre_computations(A, nr_deflat_vctrs[ix], tolx, "mlmc", mg_solver.timer,
                                               params, mg_solver, _diff_operator(mg_solver, ix), level_nr=ix)
        tr1s.append(tr1)
    print(" done. Time : " + str(time.time() - t0) + " seconds")
    print(mg_solver.timer)

    print("Computing deflation vectors (for rough trace estimation purposes only) ...", end='',
          flush=True)
    t0 = time.time()
    Vx, tr1 = deflation_pre_computations(A, params['nr_deflat_vctrs'],
                                         params['defl_eigvs_tol_Hutch'], "hutchinson",
                                         mg_solver.timer, params, mg_solver)
    print(" done. Time : " + str(time.time() - t0) + " seconds")
    print("\nComputing rough estimation of the trace ...", end='', flush=True)
    rough_trace = _rough_estimate(mg_solver, params, N) + tr1

    output_params = _mlmc_output(nr_levels, rough_trace)

    print("\nResetting timer to zero ...", end='')
    mg_solver.timer.reset()
    mg_solver.engine.timers_reset()
    print(" done\n")
    mg_solver.coarsest_lev_iters[0] = 0
    levels = mg_solver.ml.levels

    for i in range(nr_levels - 1):
        if skip_level and i == 1:
            continue
        t0 = time.time()
        level_trace_tol = abs(params['tol'] * rough_trace * _level_tol_fctr(i, nr_levels, skip_level))
        n_i = levels[i].A.shape[0]
        lc = i + 2 if (skip_level and i == 0) else i + 1
        print("Computing for level " + str(i) + " ...", end='', flush=True)

        source = DeviceProbes(mg_solver, params, "mlmc", i, kind)
        loop = run_probe_loop(source, n_i, level_trace_tol, params['max_nr_ests'],
                              batch * max(1, len(_engines(mg_solver))), probe_type=kind)
        res = output_params['results']
        res[i]['function_iters'] += int(np.sum(loop["iters_fine"]))
        res[lc]['function_iters'] += int(np.sum(loop["iters_coarse"]))
        mg_solver.coarsest_lev_iters[i] += int(np.sum(loop["iters_fine"]))
        res[i]['nr_ests'] += loop["index"]
        res[i]['ests_avg'] = loop["avg"] + tr1s[i]
        res[i]['ests_dev'] = loop["dev"]
        res[i]['ests'] = loop["ests"]              # build-only extras
        res[i]['level_tol'] = level_trace_tol
        res[i]['probe_loop_s'] = time.time() - t0
        res[i]['probes_solved'] = loop["solved"]
        print(" done. Time : " + str(time.time() - t0) + " seconds")

    # coarsest level, computed directly                            stoch_trace.py:418-437
    last = nr_levels - 1
    if levels[last].A.shape[0] == 1:
        raise Exception("your coarsest-level matrix is of size 1 ... is this what you want?")
    if params['coarsest_level_directly'] == True:   # noqa: E712  (as the reference tests it)
        output_params['results'][last]['nr_ests'] += 1
        crst_mat = mg_solver.coarsest_inv
        if params["use_permuted"]:
            crst_mat = levels[last].Pperm.transpose().conjugate() * (crst_mat * levels[last].Bblock_perm)
        output_params['results'][last]['ests_avg'] = np.trace(crst_mat)
        output_params['results'][last]['ests_dev'] = 0
    elif params.get('stochastic_coarsest'):
        # build-only option (the reference raises here): the coarsest term tr(Pperm^H A_c^-1 Bblock)
        # by plain Hutchinson probes on the coarsest level, with the tolerance share of the last
        # difference level
        n_c = levels[last].A.shape[0]
        level_trace_tol = abs(params['tol'] * rough_trace * _level_tol_fctr(last, nr_levels, skip_level))
        source = DeviceProbes(mg_solver, params, "level", last, kind)
        loop = run_probe_loop(source, n_c, level_trace_tol, params['max_nr_ests'], batch, probe_type=kind)
        res = output_params['results'][last]
        res['function_iters'] += int(np.sum(loop["iters_fine"]))
        res['nr_ests'] += loop["index"]
        res['ests_avg'] = loop["avg"]
        res['ests_dev'] = loop["dev"]
        res['ests'] = loop["ests"]
        res['level_tol'] = level_trace_tol
    else:
        raise Exception("Stochastic coarsest-level computation is disabled at the moment.")

    _mlmc_work_model(output_params, mg_solver)
    mg_solver.sync_timer()
    print(mg_solver.timer)
    return output_params


def _mlmc_loops_checks(params, deflated=False):
    """The validation of mlmc_loops() (deflated: of deflated_mlmc_loops()), before any setup: (momenta, skip_level)."""
    who = "deflated_mlmc_loops" if deflated else "mlmc_loops"
    has = hasattr(params, "get")
    refuse_distilled_three_point(params, who + "()")
    refuse_two_meson(params, who + "()")
    refuse_three_point(params, who + "()")
    refuse_distillation(params, who + "()")
    if has and params.get('source_timeslice') is not None:
        raise Exception("source_timeslice belongs to two_point(), not to %s()" % who)
    if has and params.get('x_displacements') is not None:
        raise Exception("x_displacements does not combine with the MLMC loops")
    if has and params.get('link_loops') is not None:
        raise Exception("link_loops is implemented for hutchinson() only: %s() refuses the key" % who)
    momenta = loops_of(params)
    if momenta is None:
        raise Exception("%s() needs the key timeslice_loops" % who)
    if deflated:
        mlmc_defl_setup_of(params)
        if params['defl_type'] in ("inexact_02", "inexact_03"):
            raise Exception("deflated_mlmc_loops() computes the deflated part from applications of the difference "
                            "operators (the inexact_01 form): defl_type %s is not defined for it"
                            % params['defl_type'])
    elif any(int(k) != 0 for k in params['mlmc_deflat_vctrs']):
        raise Exception("mlmc_loops() runs without MLMC-level deflation (mlmc_deflat_vctrs all zero): the deflated "
                        "part would need a sliced tr1 of the difference operators")
    if params['coarsest_level_directly'] != True:   # noqa: E712  (as mlmc() tests it)
        raise Exception("%s() computes the coarsest term exactly: coarsest_level_directly has to be true" % who)
    if _dist.default_comm().world > 1:
        raise Exception("MLMC loops (%s) run on one rank" % who)
    return momenta, _skip_level_of(params)


def mlmc_loops(A, params):
    """The timeslice loops l[p][a][b][t] = Tr(Gamma_q A^-1) by multigrid multilevel Monte Carlo:

        l_q = sum_i E_x[ S_q(Pi_i x, Pi_i D_i x) ] + sum_j S_q(Pi e_j, Pi A_c^-1 e_j)

    with D_i the MLMC difference operator of level i, Pi_i = P_0 ... P_{i-1} and S_q the slice reduction -- mlmc()
    with every level's estimate resolved in momentum, spin and timeslice (MODE_MLMC_LOOPS), the coarsest term exact
    (Engine.coarsest_loops).  Needs the key timeslice_loops (momenta, 0 among them); mlmc_deflat_vctrs all zero,
    coarsest_level_directly true, one rank; use_permuted and x_displacement are ignored, as in the Hutchinson loop
    flow.  Per level the probe loop's columns are the flattened level loops plus one control column, the scalar
    MLMC difference of the probe; the stopping rule runs on it against mlmc()'s tolerance split of the rough trace,
    which comes from five MODE_HUTCHINSON_LOOPS probes with the Hutchinson deflation vectors.

    Returns mlmc()'s dictionary (trace estimates Tr(A^-1)) with, per level, results[i]['loops' | 'loop_devs' |
    'loop_ests' | 'converged'] (the last level's loops are exact), and at top level loops = the sum over the levels,
    loop_errs = sqrt(sum_i loop_devs_i^2 / (nr_ests_i + 1)) and momenta."""
    return _mlmc_loops_flow(A, params, False)


def deflated_mlmc_loops(A, params):
    """mlmc_loops() with MLMC-level deflation of the difference operators: for the vectors V_i of
    level i (mlmc_deflat_vctrs[i] of them, computed and registered as mlmc() does, mlmc_defl_setup honoured)

        Tr(Pi_i^H Gamma_q Pi_i D_i) = E_x[ S_q(Pi_i x, Pi_i D_i (x - V_i V_i^H x)) ] + sum_j S_q(Pi_i V_j, Pi_i D_i V_j)

    the first term from probes through MODE_MLMC_DEFL_LOOPS, the second (results[i]['loop_tr1']) exactly from one
    application of D_i to V_i at function_params['tol'] (Engine.level_deflation_loops) -- never from eigenvalues, so
    the accuracy of the vectors changes the variance only.  results[i]['loops'] = probe mean + loop_tr1 (loop_ests
    stay the per-probe series without it), ests_avg = control mean + the scalar total of loop_tr1.  defl_type
    inexact_02 / inexact_03 raise; everything else as mlmc_loops()."""
    return _mlmc_loops_flow(A, params, True)


def _mlmc_loops_flow(A, params, deflated):
    momenta, skip_level = _mlmc_loops_checks(params, deflated)
    mg_solver, nr_levels = _setup_solver(A, params)
    N = A.shape[0]
    L = int(params['latt_dims'][0])
    batch = int(params.get('batch', DEFAULT_BATCH))
    kind = params.get('probe_type', 'z2')
    zero = momenta.index(0)
    shape = (len(momenta), 2, 2, L)
    mg_solver.skip_level = skip_level

    def columns(loops):
        return loop_columns(loops, zero)

    print("\nResetting timer to zero ...", end='')
    mg_solver.timer.reset()
    print(" done\n")
    register_loop_momenta(mg_solver, momenta)
    loop_tr1 = [np.zeros(shape, dtype=np.complex128) for _ in range(nr_levels)]
    if deflated:
        print("Computing deflation vectors ...", end='', flush=True)
        t0 = time.time()
    for ix in range(nr_levels - 1):
        # mlmc_loops(): no MLMC-level deflation, which clears what an earlier flow on these engines may have
        # registered; deflated_mlmc_loops(): the vectors of mlmc() (stoch_trace.py:257-270), then their sliced tr1
        k_ix = int(params['mlmc_deflat_vctrs'][ix]) if deflated and not (skip_level and ix == 1) else 0
        lop = _diff_operator(mg_solver, ix) if k_ix > 0 else None
        deflation_pre_computations(A, k_ix, params['defl_eigvs_tol_MLMC'], "mlmc", mg_solver.timer, params, mg_solver,
                                   lop, level_nr=ix)
        if k_ix > 0:
            n_ix = mg_solver.ml.levels[ix].A.shape[0]
            loop_tr1[ix] = mg_solver.engine.level_deflation_loops(ix, skip_level and ix == 0,
                                                                  params['function_params']['tol'],
                                                                  n_ix if n_ix < 1000 else 1000)
    if deflated:
        print(" done. Time : " + str(time.time() - t0) + " seconds")
    print("Computing deflation vectors (for rough estimation purposes only) ...", end='', flush=True)
    t0 = time.time()
    Vx, tr1 = deflation_pre_computations(A, params['nr_deflat_vctrs'], params['defl_eigvs_tol_Hutch'], "hutchinson",
                                         mg_solver.timer, params, mg_solver)
    tr1_cols = columns(np.asarray(tr1, dtype=np.complex128)[None])[0]
    print(" done. Time : " + str(time.time() - t0) + " seconds")
    print("\nComputing rough estimation of the loops ...", end='', flush=True)
    rough = _rough_estimate(mg_solver, params, N, "loops", columns) + tr1_cols
    control = rough.size - 1

    output_params = _mlmc_output(nr_levels, rough[control],
                                 lambda: {'loops': np.zeros(shape, dtype=np.complex128),
                                          'loop_devs': np.zeros(shape),
                                          'loop_ests': np.zeros((0,) + shape, dtype=np.complex128),
                                          'converged': np.ones(shape, dtype=bool)})

    print("\nResetting timer to zero ...", end='')
    mg_solver.timer.reset()
    mg_solver.engine.timers_reset()
    print(" done\n")
    mg_solver.coarsest_lev_iters[0] = 0
    levels = mg_solver.ml.levels
    res = output_params['results']

    for i in range(nr_levels - 1):
        if skip_level and i == 1:
            continue
        t0 = time.time()
        level_tols = np.abs(params['tol'] * rough * _level_tol_fctr(i, nr_levels, skip_level))
        n_i = levels[i].A.shape[0]
        lc = i + 2 if (skip_level and i == 0) else i + 1
        print("Computing for level " + str(i) + " ...", end='', flush=True)
        source = DeviceProbes(mg_solver, params, "mlmc_loops", i, kind, columns, deflated)
        loop = run_probe_loop(source, n_i, level_tols, params['max_nr_ests'],
                              batch * max(1, len(_engines(mg_solver))), probe_type=kind, control=control)
        res[i]['function_iters'] += int(np.sum(loop["iters_fine"]))
        res[lc]['function_iters'] += int(np.sum(loop["iters_coarse"]))
        mg_solver.coarsest_lev_iters[i] += int(np.sum(loop["iters_fine"]))
        res[i]['nr_ests'] += loop["index"]
        res[i]['ests_avg'] = loop["avg"]
        res[i]['ests_dev'] = loop["dev"]
        res[i]['ests'] = loop["ests"][:, control]  # build-only extras
        res[i]['level_tol'] = level_tols[control]
        res[i]['probe_loop_s'] = time.time() - t0
        res[i]['probes_solved'] = loop["solved"]
        res[i]['loops'] = loop["avgs"][:control].reshape(shape)
        res[i]['loop_devs'] = loop["devs"][:control].reshape(shape)
        res[i]['loop_ests'] = loop["ests"][:, :control].reshape((-1,) + shape)
        res[i]['converged'] = loop["converged"][:control].reshape(shape)
        if deflated:
            # the exact deflated part: added to the means, the per-probe series stay as the probes gave them
            t1 = columns(loop_tr1[i][None])[0]
            res[i]['ests_avg'] = loop["avg"] + t1[control]
            res[i]['loops'] = res[i]['loops'] + loop_tr1[i]
            res[i]['loop_tr1'] = loop_tr1[i]
        print(" done. Time : " + str(time.time() - t0) + " seconds")

    # coarsest level, computed directly                            stoch_trace.py:418-437
    last = nr_levels - 1
    if levels[last].A.shape[0] == 1:
        raise Exception("your coarsest-level matrix is of size 1 ... is this what you want?")
    res[last]['nr_ests'] += 1
    res[last]['loops'] = mg_solver.engine.coarsest_loops()
    res[last]['ests_avg'] = np.trace(mg_solver.coarsest_inv)
    res[last]['ests_dev'] = 0

    _mlmc_work_model(output_params, mg_solver)
    output_params['loops'] = np.zeros(shape, dtype=np.complex128)
    var = np.zeros(shape)
    for i in range(nr_levels):
        output_params['loops'] = output_params['loops'] + res[i]['loops']
        if i < last:
            var = var + np.square(res[i]['loop_devs']) / (res[i]['nr_ests'] + 1)
    output_params['loop_errs'] = np.sqrt(var)
    output_params['momenta'] = list(momenta)
    mg_solver.sync_timer()
    print(mg_solver.timer)
    return output_params
