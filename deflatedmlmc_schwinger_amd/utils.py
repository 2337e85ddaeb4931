"""Helpers of the reference's ``utils.py`` (same names and call signatures), with the probe
body running on the GPU engine.  Reference lines are cited per function."""
import os
import time

import numpy as np
from scipy.sparse.linalg import eigsh

from . import dist as _dist
from .engine import MAX_MOMENTA, MAX_SHIFTS, RESOLVED_FETCH, EngineError, probe_mode


# ----------------------------------------------------------------------------------------
# reporting / plumbing
# ----------------------------------------------------------------------------------------
def flopsV_manual(bare_level, levels_info, level_id, mg_solver):
    """utils.py:19-31: nnz-weighted work model of one cycle (kept as is, not "fixed")."""
    total = 0
    last = len(levels_info) - 2
    lvl = level_id
    while True:
        weight = 2 * mg_solver.smooth_iters + (2 if lvl == bare_level else 1)
        total += weight * levels_info[lvl].A.nnz
        if lvl == last:
            return total
        lvl += 1


def print_post_results(A, params, result, example):
    """utils.py:36-69."""
    if example not in ("mlmc", "hutchinson"):
        raise Exception("Value for parameter <example> not available.")
    print(" -- matrix : " + params['matrix'])
    print(" -- matrix size : " + str(A.shape[0]) + "x" + str(A.shape[1]))
    print(" -- tr(A^{-1}) = " + str(result['trace']))
    print(" -- total MG complexity = " + str(result['total_complexity'] / (1.0e+6)) + " MFLOPS")
    if example == "mlmc":
        print(" -- std dev = ---")
        for i in range(result['nr_levels']):
            lev = result['results'][i]
            print(" -- level : " + str(i))
            print(" \t-- number of estimates = " + str(lev['nr_ests']))
            print(" \t-- function iters = " + str(lev['function_iters']))
            print(" \t-- trace = " + str(lev['ests_avg']))
            print(" \t-- std dev = " + str(lev['ests_dev']))
            print(" \t-- var = " + str(lev['ests_dev'] * lev['ests_dev']))
            print("\t-- level MG complexity = " + str(lev['level_complexity'] / (1.0e+6)) + " MFLOPS")
    else:
        print(" -- std dev = " + str(result['std_dev']))
        print(" -- var = " + str(result['std_dev'] * result['std_dev']))
        print(" -- number of estimates = " + str(result['nr_ests']))
        print(" -- function iters = " + str(result['function_iters']))


_COMMON_KEYS = ('max_nr_levels', 'nr_deflat_vctrs', 'defl_eigvs_tol_Hutch', 'accuracy_mg_eigvs',
                'aggrs', 'dof', 'use_permuted', 'latt_dims', 'x_displacement', 'check_quality_MG',
                'test_vectors_type')
_MLMC_KEYS = ('mlmc_deflat_vctrs', 'defl_eigvs_tol_MLMC', 'diff_lev_op_tol', 'defl_type',
              'coarsest_level_directly', 'mlmc_levels_to_skip')
# build-only options (all optional; reference presets do not carry them)
_BUILD_KEYS = ('batch', 'device', 'engines', 'cache_dir', 'report_path', 'probe_type', 'solver_cfg', 'use_solver_hierarchy', 'mg_testvectors',
               'solver_testvectors', 'deflation_eigenpairs', 'ref_cycle_post', 'ref_cycle_k', 'ref_smoother',
               'solver_restart', 'stochastic_coarsest', 'stop_factor', 'ref_direct_max_n', 'ref_coarsest',
               'ref_coarse_dofs', 'setup_eigs', 'defer_coarse_levels',
               'verbose', 'probe_rounds_max', 'mlmc_defl_setup', 'defl_setup', 'x_displacements',
               'timeslice_loops', 'source_timeslice', 'two_point_momenta', 'low_mode_contraction', 'link_loops',
               'sink_timeslice', 'sink_gamma', 'sink_momentum', 'three_point_momenta',
               'smearing_kappa', 'source_smearing_steps', 'sink_smearing_steps',
               'distillation_vectors', 'source_timeslices', 'keep_perambulators', 'distilled_contraction',
               'insertion_timeslices', 'source_momentum', 'meson_operators', 'source_operators')
# where the eigenpairs of the MLMC difference operators come from: host ARPACK (the reference's path) or
# the block eigensolver on the GPU (setup_gpu.device_diff_eigenpairs)
MLMC_DEFL_SETUPS = ("host", "device")


# where lma_two_point() contracts the meson fields into E_L: NumPy on the host from the read-back fields, or the
# engine's MFMA products with the fields staying on the device (Engine.low_mode_two_point)
LOW_MODE_CONTRACTIONS = ("host", "device")


def low_mode_contraction_of(params):
    """The build-only key low_mode_contraction ("host" when absent); any other value raises."""
    how = params.get('low_mode_contraction', "host") if hasattr(params, "get") else "host"
    if how not in LOW_MODE_CONTRACTIONS:
        raise Exception("low_mode_contraction: %r is not one of %s" % (how, list(LOW_MODE_CONTRACTIONS)))
    return how


def mlmc_defl_setup_of(params):
    """The build-only key mlmc_defl_setup ("host" when absent); any other value raises."""
    how = params.get('mlmc_defl_setup', "host") if hasattr(params, "get") else "host"
    if how not in MLMC_DEFL_SETUPS:
        raise Exception("mlmc_defl_setup = %r: expected one of %s" % (how, ", ".join(MLMC_DEFL_SETUPS)))
    return how


# where the Hutchinson deflation eigenpairs come from: "auto" (the device block eigensolver for k <= 32 when
# the solver hierarchy was set up on the device, host ARPACK otherwise), "device" (the block eigensolver for
# 1 <= k <= 256, block width 64 ceil(2 k / 64)) or "host" (ARPACK always)
DEFL_SETUPS = ("auto", "device", "host")


def defl_setup_of(params):
    """The build-only key defl_setup ("auto" when absent); any other value raises."""
    how = params.get('defl_setup', "auto") if hasattr(params, "get") else "auto"
    if how not in DEFL_SETUPS:
        raise Exception("defl_setup = %r: expected one of %s" % (how, ", ".join(DEFL_SETUPS)))
    return how


def displacements_of(params):
    """The build-only key x_displacements: None when absent, else (displacements, flat shifts, index of the
    control displacement) after validation.  Displacement d is the flat-index shift latt_dims[0] * 2 * d; the
    control displacement -- the one the reference's own run would estimate -- is x_displacement with
    use_permuted and 0 without, and has to be in the list."""
    if not hasattr(params, "get") or params.get('x_displacements') is None:
        return None
    L = int(params['latt_dims'][0])
    disps = []
    for d in params['x_displacements']:
        if int(d) != d:
            raise Exception("x_displacements: %r is not an integer" % (d,))
        d = int(d)
        if not 0 <= d < L:
            raise Exception("x_displacements: %d outside [0, %d)" % (d, L))
        if d in disps:
            raise Exception("x_displacements: %d listed twice" % d)
        disps.append(d)
    if not disps:
        raise Exception("x_displacements is empty")
    if len(disps) > MAX_SHIFTS:
        raise Exception("x_displacements: %d entries, at most %d" % (len(disps), MAX_SHIFTS))
    control = int(params['x_displacement']) if params['use_permuted'] else 0
    if control not in disps:
        raise Exception("x_displacements has to contain the control displacement %d "
                        "(x_displacement with use_permuted, 0 without)" % control)
    return disps, [L * 2 * d for d in disps], disps.index(control)


def displaced_tr1(Vx, Sy, g3, n, shifts):
    """The deflated part of the displaced traces: tr1_s = sum_i (w_i^H D_s v_i) / |lambda_i| for every flat
    shift s, with (lambda_i, v_i) eigenpairs of gamma_3 A (Sy, columns of Vx), w_i = gamma_3 v_i sgn(lambda_i)
    and (D_s v)[j] = v[(j - s) mod n].  Then Tr(A^-1 D_s) = Tr(D_s A^-1 (I - W W^H)) + tr1_s.  g3: the
    diagonal of gamma_3, or a (sparse) matrix."""
    Vx = np.asarray(Vx, dtype=np.complex128)
    Sy = np.asarray(Sy, dtype=float)
    if Vx.shape[0] != n:
        raise Exception("displaced_tr1: vectors of length %d, expected %d" % (Vx.shape[0], n))
    W = (np.asarray(g3)[:, None] * Vx if np.ndim(g3) == 1 else np.asarray(g3 * Vx)) * np.sign(Sy)[None, :]
    return np.array([np.sum(np.sum(W.conj() * np.roll(Vx, int(s), axis=0), axis=0) / np.abs(Sy))
                     for s in shifts])


def loops_of(params):
    """The build-only key timeslice_loops: None when absent, else the validated list of spatial momenta p (integers
    in [0, L), L = latt_dims[0]) of the loops L_Gamma(t, p).  The list has to contain 0 -- the scalar total at
    p = 0 is the control series that estimates Tr(A^-1) -- and does not combine with x_displacements."""
    if not hasattr(params, "get") or params.get('timeslice_loops') is None:
        return None
    if params.get('x_displacements') is not None:
        raise Exception("timeslice_loops does not combine with x_displacements")
    L = int(params['latt_dims'][0])
    momenta = []
    for p in params['timeslice_loops']:
        if int(p) != p:
            raise Exception("timeslice_loops: %r is not an integer" % (p,))
        p = int(p)
        if not 0 <= p < L:
            raise Exception("timeslice_loops: momentum %d outside [0, %d)" % (p, L))
        if p in momenta:
            raise Exception("timeslice_loops: momentum %d listed twice" % p)
        momenta.append(p)
    if len(momenta) > MAX_MOMENTA:
        raise Exception("timeslice_loops: %d momenta, at most %d" % (len(momenta), MAX_MOMENTA))
    if 0 not in momenta:
        raise Exception("timeslice_loops has to contain the momentum 0 (its scalar total is the control series)")
    return momenta


def link_loops_of(params):
    """The build-only key link_loops: None when absent, else the validated list of spatial momenta p of the
    point-split link loops, checked exactly as timeslice_loops: integers in [0, L), L = latt_dims[0], no
    duplicates, at most MAX_MOMENTA, 0 among them (the scalar total of the local loops at p = 0 is the control
    series).  The key combines with neither x_displacements, timeslice_loops, source_timeslice nor
    two_point_momenta -- the local loops are part of its result anyway."""
    if not hasattr(params, "get") or params.get('link_loops') is None:
        return None
    for other in ('x_displacements', 'timeslice_loops', 'source_timeslice', 'two_point_momenta'):
        if params.get(other) is not None:
            raise Exception("link_loops does not combine with %s" % other)
    L = int(params['latt_dims'][0])
    momenta = []
    for p in params['link_loops']:
        if isinstance(p, bool) or int(p) != p:
            raise Exception("link_loops: %r is not an integer" % (p,))
        p = int(p)
        if not 0 <= p < L:
            raise Exception("link_loops: momentum %d outside [0, %d)" % (p, L))
        if p in momenta:
            raise Exception("link_loops: momentum %d listed twice" % p)
        momenta.append(p)
    if len(momenta) > MAX_MOMENTA:
        raise Exception("link_loops: %d momenta, at most %d" % (len(momenta), MAX_MOMENTA))
    if 0 not in momenta:
        raise Exception("link_loops has to contain the momentum 0 (its scalar total is the control series)")
    return momenta


LINK_BRANCHES = ('Fx', 'Bx', 'Ft', 'Bt')


def slice_link_dots(X, Z, U1, U2, L, momenta):
    """The four link branches d = (F_x, B_x, F_t, B_t) for a batch, out[k, d, p, a, b, t]:

        F_mu = sum_x e^{-2 pi i p x / L} U_mu(n)       conj(X[k, idx(a,n)])    Z[k, idx(b,n+mu)]
        B_mu = sum_x e^{-2 pi i p x / L} conj(U_mu(n)) conj(X[k, idx(a,n+mu)]) Z[k, idx(b,n)]

    with n = (x, t) the site that owns the link (its phase, its timeslice), n + x^ = ((x+1) mod L, t), n + t^ =
    (x, (t+1) mod L), idx(s,x,y) = s L^2 + y L + x and U_x = U1, U_t = U2 in natural site order t L + x.  X, Z:
    complex arrays (nb, 2 L^2) (probes as the vectors they stand for: probes_as_complex); phases as the engine's
    table -- the reduction of MODE_HUTCHINSON_LINK_LOOPS, what Engine.apply_slice_link_dots computes."""
    X = np.atleast_2d(np.asarray(X))
    Z = np.atleast_2d(np.asarray(Z))
    if X.shape != Z.shape or X.shape[1] != 2 * L * L:
        raise Exception("slice_link_dots: X %s and Z %s, expected two equal (nb, %d)" % (X.shape, Z.shape, 2 * L * L))
    U = [np.asarray(u, dtype=np.complex128).reshape(-1) for u in (U1, U2)]
    if any(u.size != L * L for u in U):
        raise Exception("slice_link_dots: links of %d and %d entries, expected %d each" % (U[0].size, U[1].size, L * L))
    ph = _phase_table(L)[np.outer(np.asarray(momenta, dtype=np.int64), np.arange(L)) % L]
    Xc, Zr = X.reshape(-1, 2, L, L).conj(), Z.reshape(-1, 2, L, L)         # [k][s][t][x]
    out = np.empty((X.shape[0], 4, len(momenta), 2, 2, L), dtype=np.complex128)
    for mu, axis in enumerate((3, 2)):                                    # n + mu: one step along x / along t
        u = U[mu].reshape(L, L)                                           # [t][x]
        fwd = u * Xc[:, :, None] * np.roll(Zr, -1, axis=axis)[:, None]    # [k][a][b][t][x]
        bwd = u.conj() * np.roll(Xc, -1, axis=axis)[:, :, None] * Zr[:, None]
        out[:, 2 * mu] = np.moveaxis(fwd @ ph.T, -1, 1)
        out[:, 2 * mu + 1] = np.moveaxis(bwd @ ph.T, -1, 1)
    return out


def link_sliced_tr1(Vx, Sy, g3, U1, U2, L, momenta):
    """The deflated part of the link loops, shape (4, nmom, 2, 2, L): the four branches of slice_link_dots with
    sum_i v_i w_i^H / |lambda_i| = A^-1 W W^H in place of A^-1 (I - W W^H), (lambda_i, v_i) eigenpairs of gamma_3 A
    (Sy, columns of Vx), w_i = gamma_3 v_i sgn(lambda_i) -- as sliced_tr1.  g3: the diagonal of gamma_3, or a (sparse)
    matrix."""
    Vx = np.asarray(Vx, dtype=np.complex128)
    Sy = np.asarray(Sy, dtype=float)
    if Vx.shape[0] != 2 * L * L:
        raise Exception("link_sliced_tr1: vectors of length %d, expected %d" % (Vx.shape[0], 2 * L * L))
    W = (np.asarray(g3)[:, None] * Vx if np.ndim(g3) == 1 else np.asarray(g3 * Vx)) * np.sign(Sy)[None, :]
    return slice_link_dots(W.T, (Vx / np.abs(Sy)[None, :]).T, U1, U2, L, momenta).sum(axis=0)


def _link_branch(link, branch, who):
    link = np.asarray(link)
    if link.ndim < 5 or link.shape[-5] != 4 or link.shape[-3:-1] != (2, 2):
        raise Exception("%s: link loops of shape %s, expected (..., 4, nmom, 2, 2, L)" % (who, link.shape))
    if branch not in LINK_BRANCHES:
        raise Exception("%s: unknown branch %r (one of %s)" % (who, branch, list(LINK_BRANCHES)))
    return link[..., LINK_BRANCHES.index(branch), :, :, :, :]


def link_loop_gamma(link, branch, which):
    """sum_ab Gamma[a][b] link[..., d, :, a, b, :] of one branch d = 'Fx', 'Bx', 'Ft' or 'Bt' of the link loops
    (..., 4, nmom, 2, 2, L), Gamma = '1', 'g3', 's1' or 's2' as loop_gamma: shape (..., nmom, L)."""
    if which not in _PAULI:
        raise Exception("link_loop_gamma: unknown spin matrix %r (one of %s)" % (which, sorted(_PAULI)))
    return loop_gamma(_link_branch(link, branch, "link_loop_gamma"), which)


def conserved_current(link, mu):
    """The conserved (point-split) vector current per timeslice and momentum from the link loops (..., 4, nmom, 2, 2, L):

        J_mu(t, p) = sum_ab ( H+_mu[a][b] F_mu[p][a][b][t] - H-_mu[a][b] B_mu[p][a][b][t] ),    mu = 'x' or 't',

    H+-_mu = 1 -+ sigma_mu the hop matrices of the operator (hierarchy._HOP, no 1/2); shape (..., nmom, L).  For the
    exact inverse it obeys (1 - e^{-2 pi i p / L}) J_x(t, p) + J_t(t, p) - J_t(t - 1, p) = 0 on every configuration."""
    from .hierarchy import _HOP
    if mu not in ('x', 't'):
        raise Exception("conserved_current: unknown direction %r (one of ['t', 'x'])" % (mu,))
    F = _link_branch(link, 'F' + mu, "conserved_current")
    B = _link_branch(link, 'B' + mu, "conserved_current")
    hp, hm = _HOP["+x" if mu == 'x' else "+y"], _HOP["-x" if mu == 'x' else "-y"]
    return sum(hp[a, b] * F[..., a, b, :] - hm[a, b] * B[..., a, b, :] for a in range(2) for b in range(2))


def slice_phases(L, momenta):
    """e^{-2 pi i p x / L} as an array [p][x]."""
    return np.exp(-2j * np.pi * np.outer(np.asarray(momenta, dtype=np.int64), np.arange(L)) / L)


def sliced_tr1(Vx, Sy, g3, L, momenta):
    """The deflated part of the timeslice loops: tr1[p][a][b][t] = sum_i sum_x e^{-2 pi i p x / L}
    conj(w_i[idx(a,x,t)]) v_i[idx(b,x,t)] / |lambda_i| with (lambda_i, v_i) eigenpairs of gamma_3 A (Sy, columns
    of Vx), w_i = gamma_3 v_i sgn(lambda_i) and idx(s,x,y) = s L^2 + y L + x.  Then the diagonal blocks of A^-1
    are those of A^-1 (I - W W^H) plus this.  g3: the diagonal of gamma_3, or a (sparse) matrix."""
    Vx = np.asarray(Vx, dtype=np.complex128)
    Sy = np.asarray(Sy, dtype=float)
    if Vx.shape[0] != 2 * L * L:
        raise Exception("sliced_tr1: vectors of length %d, expected %d" % (Vx.shape[0], 2 * L * L))
    W = (np.asarray(g3)[:, None] * Vx if np.ndim(g3) == 1 else np.asarray(g3 * Vx)) * np.sign(Sy)[None, :]
    k = Vx.shape[1]
    Wc = W.conj().reshape(2, L, L, k)                      # [a][t][x][i]
    Vs = (Vx / np.abs(Sy)[None, :]).reshape(2, L, L, k)    # [b][t][x][i]
    return np.einsum('px,atxi,btxi->pabt', slice_phases(L, momenta), Wc, Vs)


_PAULI = {'1': np.array([[1, 0], [0, 1]], dtype=np.complex128),
          'g3': np.array([[1, 0], [0, -1]], dtype=np.complex128),
          's1': np.array([[0, 1], [1, 0]], dtype=np.complex128),
          's2': np.array([[0, -1j], [1j, 0]], dtype=np.complex128)}


def loop_gamma(loops, which):
    """sum_ab Gamma[a][b] loops[..., a, b, :] for Gamma the unit matrix ('1'), gamma_3 = sigma_3 ('g3'), sigma_1
    ('s1') or sigma_2 ('s2'): the loop L_Gamma(t, p) from the spin-resolved array [..., 2, 2, L]."""
    if which not in _PAULI:
        raise Exception("loop_gamma: unknown spin matrix %r (one of %s)" % (which, sorted(_PAULI)))
    loops = np.asarray(loops)
    if loops.ndim < 3 or loops.shape[-3:-1] != (2, 2):
        raise Exception("loop_gamma: loops of shape %s, expected (..., 2, 2, L)" % (loops.shape,))
    G = _PAULI[which]
    return sum(G[a, b] * loops[..., a, b, :] for a in range(2) for b in range(2) if G[a, b] != 0)


def loop_correlator(per_probe_a, per_probe_b):
    """C[D] = (1/L) sum_t <L_a(t + D)> <L_b(t)>, D = 0..L-1 (t + D mod L), from per-probe series of shape (N, L)
    that already include tr1.  The product of the two means is formed over pairs of different probes only,
    (S_a S_b - sum_k a_k b_k) / (N (N - 1)) with S = the sum over probes: the same probe in both factors would
    add its variance, so this keeps the estimate unbiased."""
    a = np.asarray(per_probe_a, dtype=np.complex128)
    b = np.asarray(per_probe_b, dtype=np.complex128)
    if a.ndim != 2 or a.shape != b.shape:
        raise Exception("loop_correlator: series of shapes %s and %s, expected two equal (N, L)" % (a.shape, b.shape))
    N, L = a.shape
    if N < 2:
        raise Exception("loop_correlator needs at least two probes")
    Sa, Sb = a.sum(axis=0), b.sum(axis=0)
    out = np.empty(L, dtype=np.complex128)
    for D in range(L):
        ar = np.roll(a, -D, axis=1)                        # ar[k, t] = a[k, t + D]
        out[D] = np.sum(np.roll(Sa, -D) * Sb - np.sum(ar * b, axis=0)) / (N * (N - 1.0) * L)
    return out


def slice_cdots(U, V, L, momenta):
    """S_q(u, v) of the MLMC loops for a batch: out[k, p, a, b, t] = sum_x e^{-2 pi i p x / L} conj(U[k, idx(a,x,t)])
    V[k, idx(b,x,t)], idx(s,x,y) = s L^2 + y L + x, for two complex arrays (nb, 2 L^2) -- the reduction of
    MODE_MLMC_LOOPS on the prolonged probe U and the prolonged difference V (phases as the engine's table)."""
    U = np.atleast_2d(np.asarray(U))
    V = np.atleast_2d(np.asarray(V))
    if U.shape != V.shape or U.shape[1] != 2 * L * L:
        raise Exception("slice_cdots: U %s and V %s, expected two equal (nb, %d)" % (U.shape, V.shape, 2 * L * L))
    ph = _phase_table(L)[np.outer(np.asarray(momenta, dtype=np.int64), np.arange(L)) % L]
    ph = ph.astype(np.result_type(U.dtype, V.dtype, np.complex128))
    Ur, Vr = U.reshape(-1, 2, L, L), V.reshape(-1, 2, L, L)               # [k][s][t][x]
    prod = Ur.conj()[:, :, None] * Vr[:, None]                            # [k][a][b][t][x]
    return np.ascontiguousarray(np.moveaxis(prod @ ph.T, -1, 1))


def sliced_level_tr1(PiV, PiDV, L, momenta):
    """The deflated part of one level's term of the MLMC loops: tr1[p][a][b][t] = sum_j S_q(Pi V_j, Pi D V_j) from
    the prolonged vectors PiV and the prolonged D V, both (k, 2 L^2) -- what Engine.level_deflation_loops computes.
    With E_x[S_q(Pi x, Pi D (x - V V^H x))] it adds up to Tr(Pi^H Gamma_q Pi D) for any V."""
    return slice_cdots(PiV, PiDV, L, momenta).sum(axis=0)


def block_loops(M, L, momenta):
    """out[p][a][b][t] = sum_x e^{-2 pi i p x / L} M[idx(b,x,t), idx(a,x,t)] = Tr(Gamma_q M) of a dense 2 L^2 x 2 L^2
    matrix: the loops that a probe average of slice_cdots(x, M x) converges to."""
    M = np.asarray(M)
    V = L * L
    if M.shape != (2 * V, 2 * V):
        raise Exception("block_loops: matrix of shape %s, expected (%d, %d)" % (M.shape, 2 * V, 2 * V))
    ph = _phase_table(L)[np.outer(np.asarray(momenta, dtype=np.int64), np.arange(L)) % L]
    out = np.zeros((len(momenta), 2, 2, L), dtype=np.complex128)
    for a in range(2):
        for b in range(2):
            d = np.diagonal(M[b * V:(b + 1) * V, a * V:(a + 1) * V]).reshape(L, L)      # [t][x]
            out[:, a, b, :] = ph @ d.T
    return out


def mlmc_level_loops_exact(levels, coarsest_inv, L, momenta, skip=False):
    """The exact terms of the telescoping sum of the loops, from dense inverses (small lattices only):
    (terms, coarsest) with terms[i][p][a][b][t] = Tr(Gamma_q Pi_i D_i Pi_i^H) for every level but the last,
    D_i = A_i^-1 - P_i A_{i+1}^-1 R_i and Pi_i = P_0 ... P_{i-1} (skip: D_0 = A_0^-1 - P_0 P_1 A_2^-1 R_1 R_0 and
    terms[1] = 0), and coarsest = Tr(Gamma_q Pi A_c^-1 Pi^H) with A_c^-1 = coarsest_inv.  Their sum is
    block_loops(A_0^-1).  levels: objects with .A and .P (R = P^H), finest first."""
    nl = len(levels)
    if nl < 2:
        raise Exception("mlmc_level_loops_exact needs at least two levels")
    if skip and nl < 3:
        raise Exception("level skipping needs at least three levels")
    dense = lambda X: np.asarray(X.toarray() if hasattr(X, "toarray") else X, dtype=np.complex128)
    P = [dense(levels[i].P) for i in range(nl - 1)]
    inv = [np.linalg.inv(dense(levels[i].A)) for i in range(nl - 1)] + [dense(coarsest_inv)]
    Pi = [np.eye(P[0].shape[0], dtype=np.complex128)]
    for i in range(nl - 1):
        Pi.append(Pi[i] @ P[i])
    terms = []
    for i in range(nl - 1):
        if skip and i == 1:
            terms.append(np.zeros((len(momenta), 2, 2, L), dtype=np.complex128))
            continue
        if skip and i == 0:
            PP = P[0] @ P[1]
            D = inv[0] - PP @ inv[2] @ PP.conj().T
        else:
            D = inv[i] - P[i] @ inv[i + 1] @ P[i].conj().T
        terms.append(block_loops(Pi[i] @ D @ Pi[i].conj().T, L, momenta))
    return terms, block_loops(Pi[nl - 1] @ inv[nl - 1] @ Pi[nl - 1].conj().T, L, momenta)


def mlmc_loop_correlator(level_series_a, level_series_b, exact_a, exact_b):
    """C[D] = (1/L) sum_t <L_a(t + D)> <L_b(t)>, D = 0..L-1, when each loop is a sum over independent MLMC levels:
    level_series_x[i] holds the per-probe series (N_i, L) of level i's term (both loops from the same N_i probes),
    exact_x (L,) is the exact coarsest term, a constant.  Pairs of different levels, and pairs with the constant,
    take the product of the means; pairs within a level take loop_correlator's distinct-probe form, so no probe
    meets itself and the estimate is unbiased."""
    if len(level_series_a) != len(level_series_b):
        raise Exception("mlmc_loop_correlator: %d and %d levels" % (len(level_series_a), len(level_series_b)))
    ea = np.asarray(exact_a, dtype=np.complex128)
    eb = np.asarray(exact_b, dtype=np.complex128)
    if ea.ndim != 1 or ea.shape != eb.shape:
        raise Exception("mlmc_loop_correlator: exact terms of shapes %s and %s, expected two equal (L,)"
                        % (ea.shape, eb.shape))
    L = ea.size

    def of_means(ma, mb):
        return np.array([np.sum(np.roll(ma, -D) * mb) for D in range(L)]) / L

    sa, sb = ea.copy(), eb.copy()
    out = np.zeros(L, dtype=np.complex128)
    for a, b in zip(level_series_a, level_series_b):
        a = np.asarray(a, dtype=np.complex128)
        b = np.asarray(b, dtype=np.complex128)
        if a.ndim != 2 or a.shape != b.shape or a.shape[1] != L:
            raise Exception("mlmc_loop_correlator: level series of shapes %s and %s, expected two equal (N, %d)"
                            % (a.shape, b.shape, L))
        ma, mb = a.mean(axis=0), b.mean(axis=0)
        sa += ma
        sb += mb
        out += loop_correlator(a, b) - of_means(ma, mb)
    return out + of_means(sa, sb)


def two_point_of(params):
    """The build-only keys of two_point(): None when source_timeslice is absent, else (t0, momenta) after
    validation -- t0 an integer in [0, L), L = latt_dims[0]; two_point_momenta ([0] when absent) a list of at most
    MAX_MOMENTA different integers in [0, L) that contains 0 (its solutions are the conjugated factor of every
    momentum).  The keys combine with neither x_displacements nor timeslice_loops."""
    has = hasattr(params, "get")
    if not has or params.get('source_timeslice') is None:
        if has and params.get('two_point_momenta') is not None:
            raise Exception("two_point_momenta needs source_timeslice")
        return None
    if params.get('x_displacements') is not None:
        raise Exception("source_timeslice does not combine with x_displacements")
    if params.get('timeslice_loops') is not None:
        raise Exception("source_timeslice does not combine with timeslice_loops")
    L = int(params['latt_dims'][0])
    t0 = params['source_timeslice']
    if isinstance(t0, bool) or int(t0) != t0:
        raise Exception("source_timeslice: %r is not an integer" % (t0,))
    t0 = int(t0)
    if not 0 <= t0 < L:
        raise Exception("source_timeslice: %d outside [0, %d)" % (t0, L))
    given = params.get('two_point_momenta')
    momenta = []
    for p in ([0] if given is None else given):
        if int(p) != p:
            raise Exception("two_point_momenta: %r is not an integer" % (p,))
        p = int(p)
        if not 0 <= p < L:
            raise Exception("two_point_momenta: momentum %d outside [0, %d)" % (p, L))
        if p in momenta:
            raise Exception("two_point_momenta: momentum %d listed twice" % p)
        momenta.append(p)
    if len(momenta) > MAX_MOMENTA:
        raise Exception("two_point_momenta: %d momenta, at most %d" % (len(momenta), MAX_MOMENTA))
    if 0 not in momenta:
        raise Exception("two_point_momenta has to contain the momentum 0")
    return t0, momenta


def _phase_table(L):
    """omega^j = e^{-2 pi i j / L}, j in [0, L), exact at the multiples of a quarter turn (as the engine's table)."""
    j = np.arange(L)
    tab = np.exp(-2j * np.pi * j / L)
    quarter = (4 * j) % L == 0
    tab[quarter] = np.array([1, -1j, -1, 1j])[(4 * j[quarter]) // L]
    return tab


def slice_sources(probes, L, t0, momenta):
    """The one-end-trick sources of two_point(): out[2 j + a, k, idx(a', y, t)] = delta_aa' delta_{t,t0}
    e^{+2 pi i p_j y / L} xi_k(y) with xi_k(y) = the code of probe k at idx(0, y, t0) -- the same noise for both
    spins and all momenta; idx(s,x,y) = s L^2 + y L + x.  probes: int8 codes (nb, 2 L^2)."""
    probes = np.asarray(probes)
    if probes.ndim != 2 or probes.shape[1] != 2 * L * L:
        raise Exception("slice_sources: probes of shape %s, expected (nb, %d)" % (probes.shape, 2 * L * L))
    xi = probes_as_complex(probes[:, t0 * L:(t0 + 1) * L])                # [k][y]
    tab = _phase_table(L)
    out = np.zeros((2 * len(momenta),) + probes.shape, dtype=np.complex128)
    for j, p in enumerate(momenta):
        ph = np.conj(tab[(int(p) * np.arange(L)) % L])
        for a in range(2):
            first = a * L * L + t0 * L
            out[2 * j + a][:, first:first + L] = xi * ph[None, :]
    return out


def pair_dots(Z, L, momenta):
    """T[k, j, a, b, c, d, t] = sum_x e^{-2 pi i p_j x / L} conj(Z[2 j0 + a, k, idx(c,x,t)]) Z[2 j + b, k, idx(d,x,t)]
    with j0 = the index of momentum 0: the reduction of two_point() on solutions Z of shape (2 M, nb, 2 L^2) in
    the layout of slice_sources."""
    Z = np.asarray(Z, dtype=np.complex128)
    M = len(momenta)
    if Z.ndim != 3 or Z.shape[0] != 2 * M or Z.shape[2] != 2 * L * L:
        raise Exception("pair_dots: Z of shape %s, expected (%d, nb, %d)" % (Z.shape, 2 * M, 2 * L * L))
    j0 = [int(p) for p in momenta].index(0)
    Zr = Z.reshape(M, 2, Z.shape[1], 2, L, L)                             # [j][a][k][c][t][x]
    tab = _phase_table(L)
    ph = tab[np.outer(np.asarray(momenta, dtype=np.int64), np.arange(L)) % L]
    return np.einsum('jx,akctx,jbkdtx->kjabcdt', ph, Zr[j0].conj(), Zr)


def meson_correlator(T, sink, source):
    """C(t, p_j) = sum_abcd Gamma[c][d] Gamma'[b][a] g_a g_c T[..., a, b, c, d, t], Gamma = `sink`, Gamma' = `source`
    out of '1', 'g3', 's1', 's2' and g = (+1, -1) the diagonal of gamma_3: the connected two-point function
    sum_{x,y} e^{-2 pi i p (x - y) / L} tr[Gamma A^-1(x,t; y,t0) Gamma' A^-1(y,t0; x,t)] from the spin-resolved pair
    sums of two_point() (T of shape (..., 2, 2, 2, 2, L); the result keeps the leading axes and t).  gamma_3
    Hermiticity, A^-1 = gamma_3 A^-H gamma_3, supplies the backward propagator.  No fermion-loop sign is applied."""
    for which in (sink, source):
        if which not in _PAULI:
            raise Exception("meson_correlator: unknown spin matrix %r (one of %s)" % (which, sorted(_PAULI)))
    T = np.asarray(T)
    if T.ndim < 5 or T.shape[-5:-1] != (2, 2, 2, 2):
        raise Exception("meson_correlator: T of shape %s, expected (..., 2, 2, 2, 2, L)" % (T.shape,))
    G, Gp, g = _PAULI[sink], _PAULI[source], (1.0, -1.0)
    out = np.zeros(T.shape[:-5] + T.shape[-1:], dtype=np.complex128)
    for a in range(2):
        for b in range(2):
            for c in range(2):
                for d in range(2):
                    w = G[c, d] * Gp[b, a] * g[a] * g[c]
                    if w != 0:
                        out = out + w * T[..., a, b, c, d, :]
    return out


SMEARING_KEYS = ('smearing_kappa', 'source_smearing_steps', 'sink_smearing_steps')
MAX_SINK_LEVELS = 4            # SW_MAX_SINK_LEVELS, SW_MAX_SMEARING_STEPS of the engine
MAX_SMEARING_STEPS = 1024


def smear(field, U1, L, kappa, steps):
    """Gauge-covariant Jacobi (Wuppertal) smearing in the spatial direction, the NumPy definition of what
    Engine.apply_smearing computes: S_steps field with S = (1 + kappa H) / (1 + 2 kappa) and, on every line (spin s,
    timeslice t),

        (H psi)(x, t) = U1(x, t) psi(x + 1, t) + conj(U1(x - 1, t)) psi(x - 1, t)            (x +- 1 mod L).

    field: (..., 2 L^2) in the reference ordering idx(s,x,y) = s L^2 + y L + x, t = y, any leading axes; U1: the L^2
    x-links in the natural site order t L + x.  The lines do not talk to each other, so a subset of nt timeslices may
    be smeared alone: U1 the nt L links of those timeslices, field (..., 2 nt L) as [s][t][x].  S commutes with spin,
    is Hermitian on each timeslice and gauge covariant, and leaves a constant field unchanged on unit links.  A field
    (or links) of extended precision is smeared in that precision."""
    field = np.asarray(field)
    U1 = np.asarray(U1)
    nt = U1.size // L
    if nt == 0 or U1.size != nt * L or field.shape[-1] != 2 * nt * L:
        raise Exception("smear: field of shape %s and %d links, expected (..., 2 nt %d) and nt %d links (nt = %d on the "
                        "whole lattice)" % (field.shape, U1.size, L, L, L))
    if isinstance(steps, bool) or int(steps) != steps or steps < 0:
        raise Exception("smear: steps %r is not a non-negative integer" % (steps,))
    wide = np.clongdouble in (field.dtype.type, U1.dtype.type)
    ctype = np.clongdouble if wide else np.complex128
    rtype = np.longdouble if wide else np.float64
    psi = field.astype(ctype).reshape(field.shape[:-1] + (2, nt, L))      # [...][s][t][x]
    U = U1.astype(ctype).reshape(nt, L)                                   # [t][x]
    Ub = np.roll(U, 1, axis=-1).conj()                                    # conj(U1(x - 1, t))
    kappa = rtype(kappa)
    for _ in range(int(steps)):
        H = U * np.roll(psi, -1, axis=-1) + Ub * np.roll(psi, 1, axis=-1)
        psi = (psi + kappa * H) / (1 + 2 * kappa)
    return psi.reshape(field.shape)


def smearing_of(params):
    """The build-only keys of the smeared two_point(): None when smearing_kappa is absent, else the validated
    dict(kappa, source, sink) -- smearing_kappa positive and finite; source_smearing_steps (0 when absent) an integer
    in [0, MAX_SMEARING_STEPS]; sink_smearing_steps ([0] when absent) between 1 and MAX_SINK_LEVELS strictly ascending
    integers in that range, 0 meaning a local sink.  The keys need source_timeslice."""
    has = hasattr(params, "get")
    if not has or params.get('smearing_kappa') is None:
        for key in SMEARING_KEYS[1:]:
            if has and params.get(key) is not None:
                raise Exception("%s needs smearing_kappa" % key)
        return None
    if params.get('source_timeslice') is None:
        raise Exception("smearing_kappa needs source_timeslice")
    kappa = params['smearing_kappa']
    if isinstance(kappa, (bool, str)) or not np.isreal(kappa) or not np.isfinite(kappa) or not kappa > 0:
        raise Exception("smearing_kappa: %r is not a positive finite number" % (kappa,))

    def steps_of(key, v):
        if isinstance(v, bool) or int(v) != v:
            raise Exception("%s: %r is not an integer" % (key, v))
        if not 0 <= int(v) <= MAX_SMEARING_STEPS:
            raise Exception("%s: %d outside [0, %d]" % (key, int(v), MAX_SMEARING_STEPS))
        return int(v)

    given = params.get('source_smearing_steps')
    source = steps_of('source_smearing_steps', 0 if given is None else given)
    given = params.get('sink_smearing_steps')
    given = [0] if given is None else given
    if isinstance(given, (str, bytes)) or not hasattr(given, '__len__'):
        raise Exception("sink_smearing_steps: %r is not a list" % (given,))
    sink = [steps_of('sink_smearing_steps', v) for v in given]
    if not sink or len(sink) > MAX_SINK_LEVELS:
        raise Exception("sink_smearing_steps: %d levels, between 1 and %d" % (len(sink), MAX_SINK_LEVELS))
    for a, b in zip(sink, sink[1:]):
        if b <= a:
            raise Exception("sink_smearing_steps: %d after %d, the levels have to ascend strictly" % (b, a))
    return dict(kappa=float(kappa), source=source, sink=sink)


def refuse_smearing(params, who):
    """The smearing keys belong to two_point(): every other flow raises on them."""
    for key in SMEARING_KEYS:
        if hasattr(params, "get") and params.get(key) is not None:
            raise Exception("%s belongs to two_point(), not to %s" % (key, who))


DISTILLATION_KEYS = ('distillation_vectors', 'source_timeslices', 'keep_perambulators', 'distilled_contraction')
# where distilled_two_point() contracts the perambulators: NumPy on the host from the read-back blocks, or the engine's
# kernels with the blocks staying on the device (Engine.distilled_two_point)
DISTILLED_CONTRACTIONS = ("host", "device")
MAX_LAPH = 128                 # SW_MAX_LAPH of the engine
LAPH_TIE = 1e-8                # moduli this close (relatively) to the largest are tied in the phase convention


def laplacian_eigenvectors(U1, L, nev):
    """(V, eigenvalues): on every timeslice t the nev eigenvectors of the largest eigenvalues of the Hermitian L x L
    matrix of smear(),

        (H_t psi)(x) = U1(x, t) psi(x + 1) + conj(U1(x - 1, t)) psi(x - 1)                   (x +- 1 mod L),

    i.e. the lowest modes of the gauge-covariant spatial Laplacian 2 - H_t.  V[t, m, x] = v_m(x, t), orthonormal in x,
    eigenvalues[t, m] descending in m.  U1: the L^2 x-links in the natural site order t L + x.  np.linalg.eigh per
    timeslice; the phase of every vector is fixed by making its largest-modulus component real and positive, the
    lowest x on ties.  In one dimension ties are the rule -- H_t is gauge equivalent to uniform links, so a
    non-degenerate eigenvector has the same modulus at every site up to rounding -- hence moduli within the relative
    LAPH_TIE of the largest count as tied: the result is a function of the links alone."""
    U = np.asarray(U1, dtype=np.complex128).reshape(-1)
    if U.size != L * L:
        raise Exception("laplacian_eigenvectors: %d links, expected %d" % (U.size, L * L))
    if isinstance(nev, bool) or int(nev) != nev or not 1 <= int(nev) <= L:
        raise Exception("laplacian_eigenvectors: %r vectors outside [1, %d]" % (nev, L))
    nev = int(nev)
    U = U.reshape(L, L)
    x = np.arange(L)
    V = np.zeros((L, nev, L), dtype=np.complex128)
    lam = np.zeros((L, nev))
    for t in range(L):
        H = np.zeros((L, L), dtype=np.complex128)
        np.add.at(H, (x, (x + 1) % L), U[t])
        np.add.at(H, ((x + 1) % L, x), U[t].conj())
        w, Q = np.linalg.eigh(H)
        w, Q = w[::-1][:nev], Q[:, ::-1][:, :nev].T                       # [m][x], descending
        mod = np.abs(Q)
        big = np.argmax(mod >= (1.0 - LAPH_TIE) * mod.max(axis=1, keepdims=True), axis=1)
        pivot = Q[np.arange(nev), big]
        V[t] = Q * (np.abs(pivot) / pivot)[:, None]
        V[t, np.arange(nev), big] = np.abs(pivot)                         # exactly real
        lam[t] = w
    return V, lam


def _check_laph(V, L, who):
    V = np.asarray(V)
    if V.ndim != 3 or V.shape[0] != L or V.shape[2] != L:
        raise Exception("%s: V of shape %s, expected (%d, nev, %d)" % (who, V.shape, L, L))
    return V


def laph_sources(V, L, t0s):
    """The eigenvector sources of perambulators(), the NumPy definition of what Engine.apply_laph_sources writes:
    out[(s nev + n) 2 + a, idx(a', y, t)] = delta_aa' delta_{t, t0s[s]} V[t0s[s], n, y], shape (nsrc nev 2, 2 L^2)."""
    V = _check_laph(V, L, "laph_sources")
    nev = V.shape[1]
    t0s = [int(t) for t in np.atleast_1d(t0s)]
    out = np.zeros((len(t0s), nev, 2, 2 * L * L), dtype=V.dtype)
    for s, t0 in enumerate(t0s):
        for a in range(2):
            first = a * L * L + t0 * L
            out[s, :, a, first:first + L] = V[t0]
    return out.reshape(len(t0s) * nev * 2, 2 * L * L)


def perambulators_from_solutions(V, Z, L, nsrc=None):
    """out[t, c, m, k] = sum_x conj(V[t, m, x]) Z[k, idx(c, x, t)], shape (L, 2, nev, nb): the NumPy definition of what
    Engine.apply_laph_project computes, for Z of shape (nb, 2 L^2) in the reference ordering.  In np.longdouble when V
    or Z comes in that precision.  nsrc given: Z holds the nsrc nev 2 solutions of laph_sources and the result comes in
    the layout of Engine.perambulators, tau[s, t, c, m, n, a]."""
    V = _check_laph(V, L, "perambulators_from_solutions")
    Z = np.asarray(Z)
    if Z.ndim != 2 or Z.shape[1] != 2 * L * L:
        raise Exception("perambulators_from_solutions: Z of shape %s, expected (nb, %d)" % (Z.shape, 2 * L * L))
    wide = np.clongdouble in (V.dtype.type, Z.dtype.type)
    ctype = np.clongdouble if wide else np.complex128
    Zr = Z.astype(ctype).reshape(Z.shape[0], 2, L, L)                      # [k][c][t][x]
    out = np.einsum('tmx,kctx->tcmk', V.astype(ctype).conj(), Zr)
    if nsrc is None:
        return out
    nev = V.shape[1]
    if Z.shape[0] != nsrc * nev * 2:
        raise Exception("perambulators_from_solutions: %d solutions, expected %d x %d x 2" % (Z.shape[0], nsrc, nev))
    return np.ascontiguousarray(out.reshape(L, 2, nev, nsrc, nev, 2).transpose(3, 0, 1, 2, 4, 5))


def laph_elementals(V, L, momenta):
    """M[j, t, m, m'] = sum_x e^{-2 pi i p_j x / L} conj(V[t, m, x]) V[t, m', x]: the momentum projection in the
    eigenvector basis of every timeslice, shape (nmom, L, nev, nev); the phases are the engine's table."""
    V = _check_laph(V, L, "laph_elementals").astype(np.complex128)
    tab = _phase_table(L)
    ph = tab[np.outer(np.asarray(momenta, dtype=np.int64), np.arange(L)) % L]           # [j][x]
    return np.einsum('tmx,jtnx->jtmn', V.conj(), ph[:, None, None, :] * V[None])


def _check_tau(tau, M, t0s, who):
    tau = np.asarray(tau, dtype=np.complex128)
    M = np.asarray(M, dtype=np.complex128)
    t0s = [int(t) for t in np.atleast_1d(t0s)]
    if tau.ndim != 6 or tau.shape[0] != len(t0s) or tau.shape[2] != 2 or tau.shape[5] != 2 \
            or tau.shape[3] != tau.shape[4]:
        raise Exception("%s: tau of shape %s, expected (%d, L, 2, nev, nev, 2)" % (who, tau.shape, len(t0s)))
    if M.ndim != 4 or M.shape[1:] != (tau.shape[1], tau.shape[3], tau.shape[3]):
        raise Exception("%s: M of shape %s, expected (nmom, %d, %d, %d)"
                        % (who, M.shape, tau.shape[1], tau.shape[3], tau.shape[3]))
    return tau, M, t0s


def distilled_pair_sums(tau, M, t0s):
    """T[s, j, a, b, c, d, t] = sum conj(tau[s, t, c, m1, n1, a]) M[j, t, m1, m2] tau[s, t, d, m2, n2, b]
    conj(M[j, t0s[s], n1, n2]): the pair sums of two_point() with box(t) A^-1 box(t0) in place of A^-1, from the
    perambulators tau[s, t, c, m, n, a] and the elementals M of laph_elementals -- meson_correlator applies to it
    unchanged.  Per (s, j) two batched matrix products X = M_t tau_db M_t0^H and one elementwise sum against conj(tau)."""
    tau, M, t0s = _check_tau(tau, M, t0s, "distilled_pair_sums")
    nsrc, L = tau.shape[:2]
    T = np.zeros((nsrc, M.shape[0], 2, 2, 2, 2, L), dtype=np.complex128)
    for s, t0 in enumerate(t0s):
        ts = np.ascontiguousarray(tau[s].transpose(0, 1, 4, 2, 3))         # [t][c][a][m][n]
        for j in range(M.shape[0]):
            X = np.matmul(np.matmul(M[j][:, None, None], ts), M[j, t0].conj().T)       # [t][d][b][m1][n1]
            T[s, j] = np.einsum('tcamn,tdbmn->abcdt', ts.conj(), X)
    return T


def distilled_loops(tau, M, t0s):
    """loops[j, a, b, t] = sum_{m,n} M[j, t, n, m] tau(t, t)[b, m, n, a] on the source timeslices t = t0s[s], NaN on
    every other timeslice: tr[Gamma e^{-ipx} box A^-1 box] per timeslice in the layout of the timeslice loops, so
    loop_gamma applies to it unchanged."""
    tau, M, t0s = _check_tau(tau, M, t0s, "distilled_loops")
    L = tau.shape[1]
    out = np.full((M.shape[0], 2, 2, L), np.nan + 0j, dtype=np.complex128)
    for s, t0 in enumerate(t0s):
        out[:, :, :, t0] = np.einsum('jnm,bmna->jab', M[:, t0], tau[s, t0])
    return out


def source_average(T, t0s):
    """avg[..., dt] = the mean over the sources s of T[s, ..., (t0s[s] + dt) mod L]: the two_point_avg of
    distilled_two_point(), every source's correlator shifted to its own origin."""
    T = np.asarray(T)
    t0s = [int(t) for t in np.atleast_1d(t0s)]
    if T.ndim < 2 or T.shape[0] != len(t0s):
        raise Exception("source_average: T of shape %s for %d sources" % (T.shape, len(t0s)))
    return np.mean(np.stack([np.roll(T[s], -t0, axis=-1) for s, t0 in enumerate(t0s)]), axis=0)


def distillation_of(params):
    """The build-only keys of distilled_two_point(): None when distillation_vectors is absent, else the validated
    dict(nev, t0s, momenta, keep) -- distillation_vectors an integer in [1, min(L, MAX_LAPH)], L = latt_dims[0];
    source_timeslices a non-empty list of different integers in [0, L) or "all"; two_point_momenta ([0] when absent)
    at most MAX_MOMENTA different integers in [0, L), which need not contain 0; keep_perambulators (True when absent)
    a bool.  The keys combine with none of source_timeslice, sink_timeslice, x_displacements, timeslice_loops,
    link_loops and the smearing keys."""
    has = hasattr(params, "get")
    if not has or params.get('distillation_vectors') is None:
        for key in DISTILLATION_KEYS[1:]:
            if has and params.get(key) is not None:
                raise Exception("%s needs distillation_vectors" % key)
        return None
    for other in ('source_timeslice', 'sink_timeslice', 'x_displacements', 'timeslice_loops', 'link_loops') \
            + SMEARING_KEYS:
        if params.get(other) is not None:
            raise Exception("distillation_vectors does not combine with %s" % other)
    L = int(params['latt_dims'][0])
    nev = params['distillation_vectors']
    if isinstance(nev, (bool, str)) or int(nev) != nev:
        raise Exception("distillation_vectors: %r is not an integer" % (nev,))
    nev = int(nev)
    if not 1 <= nev <= min(L, MAX_LAPH):
        raise Exception("distillation_vectors: %d outside [1, %d]" % (nev, min(L, MAX_LAPH)))
    given = params.get('source_timeslices')
    if given is None:
        raise Exception("distillation_vectors needs source_timeslices (a list, or \"all\")")
    if isinstance(given, str):
        if given != "all":
            raise Exception("source_timeslices: %r is neither a list nor \"all\"" % (given,))
        t0s = list(range(L))
    else:
        if isinstance(given, bytes) or not hasattr(given, '__len__'):
            raise Exception("source_timeslices: %r is not a list" % (given,))
        t0s = []
        for t in given:
            if isinstance(t, bool) or int(t) != t:
                raise Exception("source_timeslices: %r is not an integer" % (t,))
            t = int(t)
            if not 0 <= t < L:
                raise Exception("source_timeslices: %d outside [0, %d)" % (t, L))
            if t in t0s:
                raise Exception("source_timeslices: %d listed twice" % t)
            t0s.append(t)
        if not t0s:
            raise Exception("source_timeslices: the list is empty")
    given = params.get('two_point_momenta')
    momenta = _momentum_list('two_point_momenta', [0] if given is None else given, L)
    keep = params.get('keep_perambulators')
    keep = True if keep is None else keep
    if not isinstance(keep, (bool, np.bool_)):
        raise Exception("keep_perambulators: %r is not a bool" % (keep,))
    return dict(nev=nev, t0s=t0s, momenta=momenta, keep=bool(keep))


def distilled_contraction_of(params):
    """The build-only key distilled_contraction of distilled_two_point(): "host" (also when absent) or "device"."""
    where = params.get('distilled_contraction') if hasattr(params, "get") else None
    where = "host" if where is None else where
    if not isinstance(where, str) or where not in DISTILLED_CONTRACTIONS:
        raise Exception("distilled_contraction: %r is none of %s" % (where, ", ".join(DISTILLED_CONTRACTIONS)))
    return where


def distilled_sums_wide(tau, M, t0s):
    """(T, loops) of distilled_pair_sums and distilled_loops evaluated in np.clongdouble: T[s, j, a, b, c, d, t] and
    loops[s, j, a, b] (per source, the entry of its own timeslice) -- the reference of the device contraction."""
    tau, M, t0s = _check_tau(tau, M, t0s, "distilled_sums_wide")
    return _distilled_sums(tau.astype(np.clongdouble), M.astype(np.clongdouble), t0s)


def _distilled_sums(tau, M, t0s):
    nsrc, L = tau.shape[:2]
    T = np.zeros((nsrc, M.shape[0], 2, 2, 2, 2, L), dtype=tau.dtype)
    loops = np.zeros((nsrc, M.shape[0], 2, 2), dtype=tau.dtype)
    for s, t0 in enumerate(t0s):
        ts = np.ascontiguousarray(tau[s].transpose(0, 1, 4, 2, 3))         # [t][c][a][m][n]
        for j in range(M.shape[0]):
            X = np.matmul(np.matmul(M[j][:, None, None], ts), M[j, t0].conj().T)       # [t][d][b][m1][n1]
            T[s, j] = np.einsum('tcamn,tdbmn->abcdt', ts.conj(), X)
        loops[s] = np.einsum('jnm,bmna->jab', M[:, t0], tau[s, t0])
    return T, loops


def distilled_contract_bounds(tau, M, t0s, wide=True):
    """(bound_T, bound_loops), the rounding bounds of the device contraction, shaped as distilled_sums_wide:
    |dT| <= (N^2 + 2 N + 16) 2^-52 W with W = sum_{m1,n1} |tau_ca| (|M_t| |tau_db| |M_t0|^T), and
    |dloop| <= (N^2 + 8) 2^-52 sum_{m,n} |M_t0| |tau| -- the three stages are chains of N, N and N^2 complex
    multiply-adds.  M: the elementals the device used.  The weights are sums of non-negative terms, evaluated in
    np.longdouble, or (wide false, for large N) in float64, which is off by a relative N^2 2^-53 at most."""
    tau, M, t0s = _check_tau(tau, M, t0s, "distilled_contract_bounds")
    N = tau.shape[3]
    rtype = np.longdouble if wide else np.float64
    W, w = _distilled_sums(np.abs(tau).astype(rtype), np.abs(M).astype(rtype), t0s)
    eps = rtype(2.0) ** -52
    return (N * N + 2 * N + 16) * eps * W, (N * N + 8) * eps * w


def laph_elemental_bounds(V, L):
    """bound[t, m, m'] = (L + 8) 2^-52 sum_x |v_m(x, t)| |v_m'(x, t)|: the rounding bound of a device elemental of any
    momentum (the three-factor chain of 4g)."""
    a = np.abs(_check_laph(V, L, "laph_elemental_bounds")).astype(np.longdouble)
    return (L + 8) * np.longdouble(2.0) ** -52 * np.einsum('tmx,tnx->tmn', a, a)


def laph_elementals_wide(V, L, momenta):
    """laph_elementals evaluated in np.clongdouble (the phases are the engine's table, as there)."""
    V = _check_laph(V, L, "laph_elementals_wide").astype(np.clongdouble)
    ph = _phase_table(L)[np.outer(np.asarray(momenta, dtype=np.int64), np.arange(L)) % L].astype(np.clongdouble)
    return np.einsum('tmx,jtnx->jtmn', V.conj(), ph[:, None, None, :] * V[None])


def refuse_distillation(params, who):
    """The distillation keys belong to distilled_two_point(): every other flow raises on them."""
    for key in DISTILLATION_KEYS:
        if hasattr(params, "get") and params.get(key) is not None:
            raise Exception("%s belongs to distilled_two_point(), not to %s" % (key, who))


def _momentum_list(key, given, L):
    momenta = []
    for p in given:
        if isinstance(p, bool) or int(p) != p:
            raise Exception("%s: %r is not an integer" % (key, p))
        p = int(p)
        if not 0 <= p < L:
            raise Exception("%s: momentum %d outside [0, %d)" % (key, p, L))
        if p in momenta:
            raise Exception("%s: momentum %d listed twice" % (key, p))
        momenta.append(p)
    if not momenta or len(momenta) > MAX_MOMENTA:
        raise Exception("%s: %d momenta, between 1 and %d" % (key, len(momenta), MAX_MOMENTA))
    return momenta


def three_point_of(params):
    """The build-only keys of three_point(): None when sink_timeslice is absent, else the validated
    dict(t0, tf, sink, pf, momenta) -- source_timeslice and sink_timeslice different integers in [0, L), L =
    latt_dims[0]; sink_gamma one of '1', 'g3', 's1', 's2' (default 'g3'); sink_momentum an integer in [0, L) (default
    0); three_point_momenta ([0] when absent) at most MAX_MOMENTA different integers in [0, L), which need not contain
    0.  The keys combine with none of x_displacements, timeslice_loops, link_loops and two_point_momenta."""
    has = hasattr(params, "get")
    if not has or params.get('sink_timeslice') is None:
        for key in ('sink_gamma', 'sink_momentum', 'three_point_momenta'):
            if has and params.get(key) is not None:
                raise Exception("%s needs sink_timeslice" % key)
        return None
    for other in ('x_displacements', 'timeslice_loops', 'link_loops', 'two_point_momenta'):
        if params.get(other) is not None:
            raise Exception("sink_timeslice does not combine with %s" % other)
    if params.get('source_timeslice') is None:
        raise Exception("sink_timeslice needs source_timeslice")
    L = int(params['latt_dims'][0])
    got = {}
    for key, name in (('source_timeslice', 't0'), ('sink_timeslice', 'tf'), ('sink_momentum', 'pf')):
        v = params.get(key)
        v = 0 if v is None else v          # only sink_momentum can be absent here
        if isinstance(v, bool) or int(v) != v:
            raise Exception("%s: %r is not an integer" % (key, v))
        if not 0 <= int(v) < L:
            raise Exception("%s: %d outside [0, %d)" % (key, int(v), L))
        got[name] = int(v)
    if got['tf'] == got['t0']:
        raise Exception("sink_timeslice: %d equals source_timeslice" % got['tf'])
    sink = params.get('sink_gamma')
    sink = 'g3' if sink is None else sink
    if sink not in _PAULI:
        raise Exception("sink_gamma: unknown spin matrix %r (one of %s)" % (sink, sorted(_PAULI)))
    given = params.get('three_point_momenta')
    got['sink'] = sink
    got['momenta'] = _momentum_list('three_point_momenta', [0] if given is None else given, L)
    return got


def refuse_three_point(params, who):
    """sink_timeslice selects three_point(): every other flow raises on it."""
    if hasattr(params, "get") and params.get('sink_timeslice') is not None:
        raise Exception("sink_timeslice belongs to three_point(), not to %s" % who)


def seq_sources(Z, L, tf, sink, pf):
    """The sequential sources of three_point(): out[a, k, idx(e,x,t)] = delta_{t,tf} e^{+2 pi i pf x / L} sum_c
    ((g3 Gf g3)^H)[e][c] Z[a, k, idx(c,x,tf)], Gf = `sink` out of '1', 'g3', 's1', 's2'; Z of shape (2, nb, 2 L^2), the
    solutions z_k^a of the two spin sources.  Every row of (g3 Gf g3)^H holds one entry out of +-1, +-i, so the
    matrix acts as a selection with a quarter turn; the phase is the conjugated entry of the engine's table, and
    pf = 0 multiplies nothing -- what Engine.apply_seq_sources computes."""
    if sink not in _PAULI:
        raise Exception("seq_sources: unknown spin matrix %r (one of %s)" % (sink, sorted(_PAULI)))
    Z = np.asarray(Z, dtype=np.complex128)
    if Z.ndim != 3 or Z.shape[0] != 2 or Z.shape[2] != 2 * L * L:
        raise Exception("seq_sources: Z of shape %s, expected (2, nb, %d)" % (Z.shape, 2 * L * L))
    g3 = _PAULI['g3']
    Mx = (g3 @ _PAULI[sink] @ g3).conj().T
    Zr = Z.reshape(2, Z.shape[1], 2, L, L)                                # [a][k][c][t][x]
    out = np.zeros_like(Zr)
    ph = np.conj(_phase_table(L)[(int(pf) * np.arange(L)) % L])
    for e in range(2):
        c = int(np.flatnonzero(Mx[e])[0])
        v = Mx[e, c] * Zr[:, :, c, tf, :]
        out[:, :, e, tf, :] = v if pf == 0 else ph * v
    return out.reshape(Z.shape)


def seq_dots(Zeta, Z, U1, U2, L, momenta):
    """The field x field sums of three_point() for a batch, out[k, d, j, a, b, f, c, t] over the branches d = (local,
    F_x, B_x, F_t, B_t):

        S[0]    = sum_x e^{-2 pi i q_j x / L}               conj(Zeta[a, k, idx(f,n)])    Z[b, k, idx(c,n)]
        S[F_mu] = sum_x e^{-2 pi i q_j x / L} U_mu(n)       conj(Zeta[a, k, idx(f,n)])    Z[b, k, idx(c,n+mu)]
        S[B_mu] = sum_x e^{-2 pi i q_j x / L} conj(U_mu(n)) conj(Zeta[a, k, idx(f,n+mu)]) Z[b, k, idx(c,n)]

    with n = (x, t) the site that owns the link, n + mu and the links as in slice_link_dots; Zeta, Z of shape
    (2, nb, 2 L^2); phases as the engine's table -- what Engine.apply_seq_dots computes."""
    Zeta, Z = np.asarray(Zeta), np.asarray(Z)
    if Zeta.shape != Z.shape or Z.ndim != 3 or Z.shape[0] != 2 or Z.shape[2] != 2 * L * L:
        raise Exception("seq_dots: Zeta %s and Z %s, expected two equal (2, nb, %d)" % (Zeta.shape, Z.shape, 2 * L * L))
    U = [np.asarray(u, dtype=np.complex128).reshape(-1) for u in (U1, U2)]
    if any(u.size != L * L for u in U):
        raise Exception("seq_dots: links of %d and %d entries, expected %d each" % (U[0].size, U[1].size, L * L))
    ph = _phase_table(L)[np.outer(np.asarray(momenta, dtype=np.int64), np.arange(L)) % L]
    nb = Z.shape[1]
    Zc, Zr = Zeta.reshape(2, nb, 2, L, L).conj(), Z.reshape(2, nb, 2, L, L)      # [a][k][f][t][x], [b][k][c][t][x]
    out = np.empty((nb, 5, len(momenta), 2, 2, 2, 2, L), dtype=Z.dtype if Z.dtype.kind == 'c' else np.complex128)
    out[:, 0] = np.einsum('jx,akftx,bkctx->kjabfct', ph, Zc, Zr)
    for mu, axis in enumerate((4, 3)):                                   # n + mu: one step along x / along t
        u = U[mu].reshape(L, L).astype(out.dtype)                        # [t][x]
        out[:, 1 + 2 * mu] = np.einsum('jx,tx,akftx,bkctx->kjabfct', ph, u, Zc, np.roll(Zr, -1, axis=axis))
        out[:, 2 + 2 * mu] = np.einsum('jx,tx,akftx,bkctx->kjabfct', ph, u.conj(), np.roll(Zc, -1, axis=axis), Zr)
    return out


def _three_point_sums(S, who):
    S = np.asarray(S)
    if S.ndim < 7 or S.shape[-7] != 5 or S.shape[-5:-1] != (2, 2, 2, 2):
        raise Exception("%s: S of shape %s, expected (..., 5, nmom, 2, 2, 2, 2, L)" % (who, S.shape))
    return S


def _source_weights(source, who):
    if source not in _PAULI:
        raise Exception("%s: unknown spin matrix %r (one of %s)" % (who, source, sorted(_PAULI)))
    return _PAULI[source] @ _PAULI['g3']                                  # (Gamma_i g3)[b][a]


def three_point_correlator(S, insertion, source):
    """C3_Gamma(t, q_j) = sum_abfc (Gamma_i g3)[b][a] g_f Gamma[f][c] S[..., 0, j, a, b, f, c, t], Gamma = `insertion`,
    Gamma_i = `source` out of '1', 'g3', 's1', 's2', g = (+1, -1): the three-point function sum_{x,y,w} e^{-2 pi i q x / L}
    e^{-2 pi i pf w / L} tr[Gamma_i A^-1(y,t0; w,tf) Gamma_f A^-1(w,tf; x,t) Gamma A^-1(x,t; y,t0)] from the local
    sums of three_point() (S of shape (..., 5, nmom, 2, 2, 2, 2, L)); shape (..., nmom, L).  No fermion-loop sign."""
    S = _three_point_sums(S, "three_point_correlator")
    if insertion not in _PAULI:
        raise Exception("three_point_correlator: unknown spin matrix %r (one of %s)" % (insertion, sorted(_PAULI)))
    W = _source_weights(source, "three_point_correlator")
    G = _PAULI['g3'] @ _PAULI[insertion]                                  # g_f Gamma[f][c]
    return np.einsum('ba,fc,...jabfct->...jt', W, G, S[..., 0, :, :, :, :, :, :])


def three_point_current(S, mu, source=None):
    """The conserved vector current inserted into the three-point function, from the link sums of three_point():

        J_mu[a][b](t, q_j) = sum_fc g_f ( H+_mu[f][c] S[F_mu] - H-_mu[f][c] S[B_mu] )[j][a][b][f][c][t],  mu = 'x' or 't',

    H+-_mu the hop matrices of the operator (hierarchy._HOP).  source None: J itself, shape (..., nmom, 2, 2, L);
    else C3_{J_mu}(t, q_j) = sum_ab (Gamma_i g3)[b][a] J_mu[a][b], shape (..., nmom, L).  Per noise and exactly,
    W[a][b](t) = (1 - e^{-2 pi i q / L}) J_x(t) + J_t(t) - J_t(t - 1) vanishes off the source and the sink slice."""
    from .hierarchy import _HOP
    S = _three_point_sums(S, "three_point_current")
    if mu not in ('x', 't'):
        raise Exception("three_point_current: unknown direction %r (one of ['t', 'x'])" % (mu,))
    d = 1 if mu == 'x' else 3
    g3 = _PAULI['g3']
    hp, hm = g3 @ _HOP["+x" if mu == 'x' else "+y"], g3 @ _HOP["-x" if mu == 'x' else "-y"]
    J = (np.einsum('fc,...jabfct->...jabt', hp, S[..., d, :, :, :, :, :, :])
         - np.einsum('fc,...jabfct->...jabt', hm, S[..., d + 1, :, :, :, :, :, :]))
    if source is None:
        return J
    return np.einsum('ba,...jabt->...jt', _source_weights(source, "three_point_current"), J)


# ---- distilled three-point functions: generalized perambulators -------------------------------------
DISTILLED_THREE_POINT_KEYS = ('insertion_timeslices', 'source_momentum')
DISTILLED_INSERTIONS = ('1', 'g3', 's1', 's2', 'Jx', 'Jt')


def refuse_distilled_three_point(params, who):
    """insertion_timeslices and source_momentum belong to distilled_three_point(): every other flow raises on them."""
    for key in DISTILLED_THREE_POINT_KEYS:
        if hasattr(params, "get") and params.get(key) is not None:
            raise Exception("%s belongs to distilled_three_point(), not to %s" % (key, who))


def _hop_factors(mu):
    """(l+, r+, l-, r-) with g3 H+-_mu = outer(l, r): the four hop matrices times g3 have rank one."""
    from .hierarchy import _HOP
    out = []
    for key in (("+x", "-x") if mu == 0 else ("+y", "-y")):
        h = _PAULI['g3'] @ _HOP[key]
        l, r = h[:, 0] / h[0, 0], h[0, :]
        if not np.array_equal(np.outer(l, r), h):
            raise Exception("_hop_factors: g3 H%s is not of rank one" % key)
        out += [l, r]
    return out


def _solution_fields(Z, L, who, ctype):
    Z = np.asarray(Z)
    if Z.ndim != 2 or Z.shape[1] != 2 * L * L:
        raise Exception("%s: fields of shape %s, expected (nb, %d)" % (who, Z.shape, 2 * L * L))
    return Z.astype(ctype).reshape(Z.shape[0], 2, L, L)                    # [k][c][t][x]


def generalized_perambulators_from_solutions(Zf, Z0, U1, U2, L, timeslices, momenta, wide=False):
    """G[i, j, k, r, s] for the insertion timeslices t = timeslices[i], the momenta q_j and the fields Zf (nbf, 2 L^2),
    Z0 (nb0, 2 L^2) in the reference ordering, shape (nt, nmom, 6, nbf, nb0): the NumPy definition of what
    Engine.apply_laph_generalized computes,

        k = 2 f + c:   sum_x e^{-2 pi i q x / L} conj(Zf[r, idx(f,x,t)]) Z0[s, idx(c,x,t)]
        k = 4 + mu:    sum_fc (g3 H+_mu)[f][c] F_mu[f][c] - (g3 H-_mu)[f][c] B_mu[f][c],        mu = 0 (x), 1 (t)
            F_mu[f][c] = sum_x e^{-2 pi i q x / L}      U_mu(n)  conj(Zf[r, idx(f,n)])    Z0[s, idx(c,n+mu)]
            B_mu[f][c] = sum_x e^{-2 pi i q x / L} conj(U_mu(n)) conj(Zf[r, idx(f,n+mu)]) Z0[s, idx(c,n)]

    i.e. seq_dots followed by three_point_current(., mu, None) with the noise index replaced by the pair (r, s); links,
    neighbours and hop matrices as there, phases from the engine's table.  The four g3 H+-_mu have rank one, so every
    link branch is one product of spin-projected fields.  wide: evaluated in np.clongdouble."""
    ctype = np.clongdouble if wide else np.complex128
    who = "generalized_perambulators_from_solutions"
    Zf, Z0 = _solution_fields(Zf, L, who, ctype), _solution_fields(Z0, L, who, ctype)
    U = [np.asarray(u, dtype=np.complex128).reshape(-1) for u in (U1, U2)]
    if any(u.size != L * L for u in U):
        raise Exception("%s: links of %d and %d entries, expected %d each" % (who, U[0].size, U[1].size, L * L))
    U = [u.reshape(L, L).astype(ctype) for u in U]                         # [t][x]
    ts = [int(t) for t in np.atleast_1d(timeslices)]
    qs = [int(q) for q in np.atleast_1d(momenta)]
    ph = _phase_table(L)[np.outer(np.asarray(qs, dtype=np.int64), np.arange(L)) % L].astype(ctype)     # [j][x]
    hops = [_hop_factors(mu) for mu in range(2)]
    out = np.zeros((len(ts), len(qs), 6, Zf.shape[0], Z0.shape[0]), dtype=ctype)
    for i, t in enumerate(ts):
        zf, z0 = Zf[:, :, t, :], Z0[:, :, t, :]                            # [k][c][x]
        tn = (t + 1) % L
        # per current the (weight, left field, right field) of the F and the B branch, at the link's own x
        branches = []
        for mu in range(2):
            lp, rp, lm, rm = [v.astype(ctype) for v in hops[mu]]
            if mu == 0:
                zfn, z0n = np.roll(zf, -1, axis=2), np.roll(z0, -1, axis=2)
            else:
                zfn, z0n = Zf[:, :, tn, :], Z0[:, :, tn, :]
            u = U[mu][t]
            branches.append(((u, np.einsum('f,kfx->kx', lp.conj(), zf), np.einsum('c,kcx->kx', rp, z0n)),
                             (-u.conj(), np.einsum('f,kfx->kx', lm.conj(), zfn), np.einsum('c,kcx->kx', rm, z0))))
        for j in range(len(qs)):
            for f in range(2):
                left = zf[:, f, :].conj() * ph[j]
                for c in range(2):
                    out[i, j, 2 * f + c] = left @ z0[:, c, :].T
            for mu in range(2):
                for w, a, b in branches[mu]:
                    out[i, j, 4 + mu] += (a.conj() * (ph[j] * w)) @ b.T
    return out


def generalized_perambulator_bounds(Zf, Z0, L, timeslices):
    """bound[i, k, r, s], the rounding bounds of the device's generalized perambulators at any momentum, in
    np.longdouble:  (L + 12) 2^-52 sum_x |Zf_f| |Z0_c| for the local components k = 2 f + c -- a chain of 2 L
    multiply-adds and one more multiply by the weight -- and (2 L + 16) 2^-52 sum_{branch,f,c} sum_x |Zf_f| |Z0_c| at
    the branch's sites for the currents k = 4, 5: two branches of four spin terms with coefficients of modulus one
    in one accumulator."""
    who = "generalized_perambulator_bounds"
    Af = np.abs(_solution_fields(Zf, L, who, np.complex128)).astype(np.longdouble)
    A0 = np.abs(_solution_fields(Z0, L, who, np.complex128)).astype(np.longdouble)
    ts = [int(t) for t in np.atleast_1d(timeslices)]
    eps = np.longdouble(2.0) ** -52
    out = np.zeros((len(ts), 6, Af.shape[0], A0.shape[0]), dtype=np.longdouble)
    for i, t in enumerate(ts):
        af, a0 = Af[:, :, t, :], A0[:, :, t, :]
        tn = (t + 1) % L
        for f in range(2):
            for c in range(2):
                out[i, 2 * f + c] = (L + 12) * eps * (af[:, f, :] @ a0[:, c, :].T)
        sf, s0 = af.sum(axis=1), a0.sum(axis=1)                            # sum over the spins: [k][x]
        sfx, s0x = np.roll(sf, -1, axis=1), np.roll(s0, -1, axis=1)
        sft, s0t = Af[:, :, tn, :].sum(axis=1), A0[:, :, tn, :].sum(axis=1)
        out[i, 4] = (2 * L + 16) * eps * (sf @ s0x.T + sfx @ s0.T)
        out[i, 5] = (2 * L + 16) * eps * (sf @ s0t.T + sft @ s0.T)
    return out


def distilled_three_point_correlator(G, tau_f0, M_sink, M_source, sink, insertion, source):
    """C3(t_i, q_j), shape (nmom, nt), from the generalized perambulators G[i, j, k, (m,e), (n',b)] of
    Engine.generalized_perambulators, the perambulator tau_f0[e, m, n, a] = tau(tf, t0) (perambulators()[s, tf] of
    the source t0), the sink elemental M_sink = M[pf][tf] and the source elemental M_source = M[pi][t0] (each
    (nev, nev), laph_elementals):

        R[(m,e)][(n,a)] = sum_{m',c} ((g3 Gf g3)^H)[e][c] conj(M_sink[m'][m]) tau_f0[c][m'][n][a]
        C3 = sum (Gi g3)[b][a] X[f][c] conj(R[(m,e)][(n,a)]) M_source[n'][n] G[i][j][2 f + c][(m,e)][(n',b)]

    with X = g3 Gamma for a local insertion Gamma out of '1', 'g3', 's1', 's2', and the component 4 / 5 of G in place
    of the sum over f, c for the conserved current 'Jx' / 'Jt'; Gf = `sink`, Gi = `source`.  It equals
    tr[(Gi x Phi(pi,t0)) A^-1(t0;tf) (Gf x Phi(pf,tf)) A^-1(tf;t) (Gamma x diag omega_q) A^-1(t;t0)] with
    Phi(p,t) = box(t) diag(omega_p) box(t).  No fermion-loop sign, as in three_point_correlator."""
    who = "distilled_three_point_correlator"
    G = np.asarray(G, dtype=np.complex128)
    tau_f0 = np.asarray(tau_f0, dtype=np.complex128)
    if tau_f0.ndim != 4 or tau_f0.shape[0] != 2 or tau_f0.shape[3] != 2 or tau_f0.shape[1] != tau_f0.shape[2]:
        raise Exception("%s: tau_f0 of shape %s, expected (2, nev, nev, 2)" % (who, tau_f0.shape))
    N = tau_f0.shape[1]
    if G.ndim != 5 or G.shape[2:] != (6, 2 * N, 2 * N):
        raise Exception("%s: G of shape %s, expected (nt, nmom, 6, %d, %d)" % (who, G.shape, 2 * N, 2 * N))
    Ms, Mi = np.asarray(M_sink, dtype=np.complex128), np.asarray(M_source, dtype=np.complex128)
    if Ms.shape != (N, N) or Mi.shape != (N, N):
        raise Exception("%s: elementals of shape %s and %s, expected (%d, %d)" % (who, Ms.shape, Mi.shape, N, N))
    if sink not in _PAULI:
        raise Exception("%s: unknown spin matrix %r (one of %s)" % (who, sink, sorted(_PAULI)))
    if insertion not in DISTILLED_INSERTIONS:
        raise Exception("%s: unknown insertion %r (one of %s)" % (who, insertion, list(DISTILLED_INSERTIONS)))
    W = _source_weights(source, who)                                       # (Gi g3)[b][a]
    g3 = _PAULI['g3']
    Mx = (g3 @ _PAULI[sink] @ g3).conj().T
    R = np.einsum('ec,pm,cpna->mena', Mx, Ms.conj(), tau_f0)
    Y = np.einsum('mena,pn,ba->mepb', R.conj(), Mi, W).reshape(2 * N, 2 * N)
    if insertion in _PAULI:
        X = g3 @ _PAULI[insertion]
        Gk = np.einsum('k,ijkrs->ijrs', X.reshape(4), G[:, :, :4])
    else:
        Gk = G[:, :, 4 if insertion == 'Jx' else 5]
    return np.einsum('ijrs,rs->ji', Gk, Y)


def distilled_three_point_of(params):
    """The build-only keys of distilled_three_point(): None when distillation_vectors or sink_timeslice is absent, else
    the validated dict(nev, t0, tf, sink, pf, pi, momenta, tins) -- distillation_vectors an integer in
    [1, min(L, MAX_LAPH)]; source_timeslice, sink_timeslice, sink_gamma, sink_momentum and three_point_momenta as
    three_point_of takes them; insertion_timeslices a non-empty list of different integers in [0, L) or "all" (the
    default); source_momentum an integer in [0, L) (default 0).  The keys combine with none of source_timeslices,
    keep_perambulators, distilled_contraction, two_point_momenta, x_displacements, timeslice_loops, link_loops and the
    smearing keys."""
    has = hasattr(params, "get")
    if not has or params.get('distillation_vectors') is None or params.get('sink_timeslice') is None:
        return None
    for other in DISTILLATION_KEYS[1:] + SMEARING_KEYS:
        if params.get(other) is not None:
            raise Exception("distilled_three_point() does not combine with %s" % other)
    got = three_point_of(params)           # refuses the loop and displacement keys and two_point_momenta
    L = int(params['latt_dims'][0])
    nev = params['distillation_vectors']
    if isinstance(nev, (bool, str)) or int(nev) != nev:
        raise Exception("distillation_vectors: %r is not an integer" % (nev,))
    nev = int(nev)
    if not 1 <= nev <= min(L, MAX_LAPH):
        raise Exception("distillation_vectors: %d outside [1, %d]" % (nev, min(L, MAX_LAPH)))
    pi = params.get('source_momentum')
    pi = 0 if pi is None else pi
    if isinstance(pi, (bool, str)) or int(pi) != pi:
        raise Exception("source_momentum: %r is not an integer" % (pi,))
    if not 0 <= int(pi) < L:
        raise Exception("source_momentum: %d outside [0, %d)" % (int(pi), L))
    given = params.get('insertion_timeslices')
    given = "all" if given is None else given
    if isinstance(given, str):
        if given != "all":
            raise Exception("insertion_timeslices: %r is neither a list nor \"all\"" % (given,))
        tins = list(range(L))
    else:
        if isinstance(given, bytes) or not hasattr(given, '__len__'):
            raise Exception("insertion_timeslices: %r is not a list" % (given,))
        tins = []
        for t in given:
            if isinstance(t, (bool, str)) or int(t) != t:
                raise Exception("insertion_timeslices: %r is not an integer" % (t,))
            t = int(t)
            if not 0 <= t < L:
                raise Exception("insertion_timeslices: %d outside [0, %d)" % (t, L))
            if t in tins:
                raise Exception("insertion_timeslices: %d listed twice" % t)
            tins.append(t)
        if not tins:
            raise Exception("insertion_timeslices: the list is empty")
    return dict(nev=nev, t0=got['t0'], tf=got['tf'], sink=got['sink'], pf=got['pf'], pi=int(pi),
                momenta=got['momenta'], tins=tins)


# ---- two-meson correlators from the perambulators ---------------------------------------------------
TWO_MESON_KEYS = ('meson_operators', 'source_operators')
MAX_MESON_OPS = 4              # SW_MAX_MESON_OPS of the engine


def refuse_two_meson(params, who):
    """meson_operators and source_operators belong to distilled_two_meson(): every other flow raises on them."""
    for key in TWO_MESON_KEYS:
        if hasattr(params, "get") and params.get(key) is not None:
            raise Exception("%s belongs to distilled_two_meson(), not to %s" % (key, who))


def _meson_operator_list(key, given, momenta):
    if isinstance(given, (str, bytes)) or not hasattr(given, '__len__'):
        raise Exception("%s: %r is not a list of (spin matrix, momentum) pairs" % (key, given))
    if not 1 <= len(given) <= MAX_MESON_OPS:
        raise Exception("%s: %d operators, between 1 and %d" % (key, len(given), MAX_MESON_OPS))
    ops = []
    for op in given:
        if isinstance(op, (str, bytes)) or not hasattr(op, '__len__') or len(op) != 2:
            raise Exception("%s: %r is not a (spin matrix, momentum) pair" % (key, op))
        which, p = op
        if not isinstance(which, str) or which not in _PAULI:
            raise Exception("%s: unknown spin matrix %r (one of %s)" % (key, which, sorted(_PAULI)))
        if isinstance(p, (bool, str)) or int(p) != p:
            raise Exception("%s: momentum %r is not an integer" % (key, p))
        if int(p) not in momenta:
            raise Exception("%s: momentum %d is not in two_point_momenta %s" % (key, int(p), list(momenta)))
        ops.append((which, int(p)))
    return ops


def two_meson_ops_of(params):
    """The build-only keys of distilled_two_meson(): None when meson_operators is absent, else the validated
    dict(nev, t0s, momenta, operators, source_operators, sink_ops, source_ops) -- distillation_vectors,
    source_timeslices and two_point_momenta as distillation_of takes them (keep_perambulators is refused: the flow keeps
    no perambulators); meson_operators a list of 1 to MAX_MESON_OPS pairs (spin matrix out of '1', 'g3', 's1', 's2',
    momentum), every momentum one of two_point_momenta; source_operators the same form, meson_operators when absent.
    sink_ops / source_ops: the pairs with the momentum replaced by its index in `momenta`, as two_meson_sums and the
    engine take them."""
    has = hasattr(params, "get")
    if not has or params.get('meson_operators') is None:
        if has and params.get('source_operators') is not None:
            raise Exception("source_operators needs meson_operators")
        return None
    if params.get('keep_perambulators') is not None:
        raise Exception("distilled_two_meson() does not combine with keep_perambulators")
    for key in DISTILLED_THREE_POINT_KEYS:
        if params.get(key) is not None:
            raise Exception("distilled_two_meson() does not combine with %s" % key)
    sel = distillation_of(params)
    if sel is None:
        raise Exception("meson_operators needs distillation_vectors")
    momenta = sel['momenta']
    operators = _meson_operator_list('meson_operators', params['meson_operators'], momenta)
    given = params.get('source_operators')
    source_operators = list(operators) if given is None else _meson_operator_list('source_operators', given, momenta)
    return dict(nev=sel['nev'], t0s=sel['t0s'], momenta=momenta, operators=operators,
                source_operators=source_operators,
                sink_ops=[(g, momenta.index(p)) for g, p in operators],
                source_ops=[(g, momenta.index(p)) for g, p in source_operators])


def _meson_spin(which, who):
    if isinstance(which, str):
        if which not in _PAULI:
            raise Exception("%s: unknown spin matrix %r (one of %s)" % (who, which, sorted(_PAULI)))
        return _PAULI[which]
    g = np.asarray(which, dtype=np.complex128)
    if g.shape != (2, 2):
        raise Exception("%s: spin matrix of shape %s, expected (2, 2)" % (who, g.shape))
    return g


def two_meson_folded(sink_ops, source_ops, nmom=None, who="two_meson_folded"):
    """([(G_k, j_k)], [(H_k', j_k')]) with G = g3 Gamma and H = Gamma' g3: the operators as the engine takes them, from
    pairs (Gamma, momentum index), Gamma a name out of '1', 'g3', 's1', 's2' or a 2 x 2 matrix."""
    g3 = _PAULI['g3']
    out = []
    for ops, sink in ((sink_ops, True), (source_ops, False)):
        ops = list(ops)
        if not 1 <= len(ops) <= MAX_MESON_OPS:
            raise Exception("%s: %d operators, between 1 and %d" % (who, len(ops), MAX_MESON_OPS))
        side = []
        for which, j in ops:
            if isinstance(j, bool) or int(j) != j or int(j) < 0 or (nmom is not None and int(j) >= nmom):
                raise Exception("%s: momentum index %r outside the %s momenta" % (who, j, nmom))
            g = _meson_spin(which, who)
            side.append((g3 @ g if sink else g @ g3, int(j)))
        out.append(side)
    return out[0], out[1]


def _two_meson_sums(tau, M, t0s, G, H, want_Q):
    """C1, C2 (and Q) in the dtype of tau from the folded operators G = [(G_k, j_k)], H = [(H_k', j_k')]: batched
    matrix products over the timeslices on the 2 N x 2 N matrices of one source."""
    nsrc, L, N = tau.shape[0], tau.shape[1], tau.shape[3]
    nk, nkp = len(G), len(H)
    C1 = np.zeros((nsrc, nk, nkp, L), dtype=tau.dtype)
    C2 = np.zeros((nsrc, nk, nk, nkp, nkp, L), dtype=tau.dtype)
    Q = np.zeros((nsrc, nk, L, 2 * N, 2 * N), dtype=tau.dtype) if want_Q else None
    for s, t0 in enumerate(t0s):
        X = tau[s].reshape(L, 2 * N, 2 * N)                                # [t][(c,m)][(n,a)]
        Xh = X.conj().transpose(0, 2, 1)
        R = np.zeros((nk, nkp, L, 2 * N, 2 * N), dtype=tau.dtype)
        for k, (g, j) in enumerate(G):
            Phi = (g.astype(tau.dtype)[None, :, None, :, None] * M[j][:, None, :, None, :]).reshape(L, 2 * N, 2 * N)
            Qk = np.matmul(Xh, np.matmul(Phi, X))                          # [t][rho1][rho2]
            if want_Q:
                Q[s, k] = Qk
            for kp, (hm, jp) in enumerate(H):
                # S[(n2,b)][(n1,a)] = H[b][a] conj(M_t0[n1][n2])
                S = (M[jp, t0].conj().T[:, None, :, None] * hm.astype(tau.dtype)[None, :, None, :]).reshape(2 * N, 2 * N)
                C1[s, k, kp] = np.sum(Qk * S.T[None], axis=(1, 2))
                R[k, kp] = np.matmul(Qk, S)
        for k in range(nk):
            for l in range(nk):
                for kp in range(nkp):
                    for lp in range(nkp):
                        C2[s, k, l, kp, lp] = np.sum(R[k, kp] * R[l, lp].transpose(0, 2, 1), axis=(1, 2))
    return C1, C2, Q


def two_meson_sums(tau, M, t0s, sink_ops, source_ops):
    """(C1[s, k, k', t], C2[s, k, l, k', l', t]), the two-meson building blocks from the perambulators tau[s, t, c, m, n,
    a] and the elementals M of laph_elementals, for the sink operators (Gamma_k, j_k) and the source operators
    (Gamma'_k', j_k') -- spin matrix (a name or 2 x 2) and index into M's momenta: with G = g3 Gamma, H = Gamma' g3 and
    rho = 2 n + a,

        Q[s, k, t][rho1, rho2] = sum conj(tau[s, t, c, m1, n1, a]) G[c, d] M[j_k, t, m1, m2] tau[s, t, d, m2, n2, b]
        S[s, k'][rho2, rho1]   = H[b, a] conj(M[j_k', t0s[s], n1, n2])
        C1 = tr[Q_k S_k'],     C2 = tr[Q_k S_k' Q_l S_l'].

    C1[s, k, k'] is meson_correlator(distilled_pair_sums(...)[s, j], Gamma_k, Gamma'_k') when both momenta are j; C2 is
    the crossed quark-line diagram of two mesons at the sink and two at the source.  No fermion-loop sign."""
    tau, M, t0s = _check_tau(tau, M, t0s, "two_meson_sums")
    G, H = two_meson_folded(sink_ops, source_ops, M.shape[0], "two_meson_sums")
    return _two_meson_sums(tau, M, t0s, G, H, False)[:2]


def two_meson_sums_wide(tau, M, t0s, sink_ops, source_ops):
    """(C1, C2, Q) of two_meson_sums evaluated in np.clongdouble, with the sandwich Q[s, k, t, rho1, rho2] -- the
    reference of the device kernels."""
    tau, M, t0s = _check_tau(tau, M, t0s, "two_meson_sums_wide")
    G, H = two_meson_folded(sink_ops, source_ops, M.shape[0], "two_meson_sums_wide")
    return _two_meson_sums(tau.astype(np.clongdouble), M.astype(np.clongdouble), t0s, G, H, True)


def two_meson_bounds(tau, M, t0s, sink_ops, source_ops, wide=True):
    """(bound_Q, bound_C1, bound_C2), the rounding bounds of the device's two-meson kernels, shaped as
    two_meson_sums_wide's Q, C1, C2: the same formulas on absolute values,

        |dQ|  <= (4 N + 16) 2^-52 |tau|^H (|G| x |M_t|) |tau|
        |dC1| <= (4 N^2 + 4 N + 32) 2^-52 tr[Qabs Sabs]
        |dC2| <= (4 N^2 + 12 N + 64) 2^-52 tr[Qabs_k Sabs_k' Qabs_l Sabs_l']

    -- chains of 2 N (W), 2 N (Q), 2 N (R) and 4 N^2 (the traces) complex multiply-adds plus the spin weights.  M: the
    elementals the device used.  Sums of non-negative terms in np.longdouble, or (wide false, for large N) float64."""
    tau, M, t0s = _check_tau(tau, M, t0s, "two_meson_bounds")
    G, H = two_meson_folded(sink_ops, source_ops, M.shape[0], "two_meson_bounds")
    N = tau.shape[3]
    rtype = np.longdouble if wide else np.float64
    Ga = [(np.abs(g).astype(rtype), j) for g, j in G]
    Ha = [(np.abs(hm).astype(rtype), j) for hm, j in H]
    C1, C2, Q = _two_meson_sums(np.abs(tau).astype(rtype), np.abs(M).astype(rtype), t0s, Ga, Ha, True)
    eps = rtype(2.0) ** -52
    return (4 * N + 16) * eps * Q, (4 * N * N + 4 * N + 32) * eps * C1, (4 * N * N + 12 * N + 64) * eps * C2


def two_meson_correlator(C1, C2, k, l, kp, lp):
    """dict(direct, crossed, isospin2), each of the shape of C1[..., 0, 0, :]: for the sink operators k, l and the source
    operators kp, lp of two_meson_sums' C1[..., k, k', t] and C2[..., k, l, k', l', t],

        direct   = C1[k, kp] C1[l, lp] + C1[k, lp] C1[l, kp]
        crossed  = C2[k, l, kp, lp] + C2[k, l, lp, kp]
        isospin2 = direct - crossed.

    No fermion-loop sign is applied anywhere, as in meson_correlator."""
    C1, C2 = np.asarray(C1), np.asarray(C2)
    if C1.ndim < 3 or C2.ndim != C1.ndim + 2 or C2.shape[-5:-3] != (C1.shape[-3],) * 2 \
            or C2.shape[-3:-1] != (C1.shape[-2],) * 2 or C2.shape[-1] != C1.shape[-1]:
        raise Exception("two_meson_correlator: C1 of shape %s and C2 of shape %s, expected (..., nk, nkp, L) and "
                        "(..., nk, nk, nkp, nkp, L)" % (C1.shape, C2.shape))
    for name, v, n in (('k', k, C1.shape[-3]), ('l', l, C1.shape[-3]), ('kp', kp, C1.shape[-2]),
                       ('lp', lp, C1.shape[-2])):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < n:
            raise Exception("two_meson_correlator: %s = %r outside [0, %d)" % (name, v, n))
    direct = C1[..., k, kp, :] * C1[..., l, lp, :] + C1[..., k, lp, :] * C1[..., l, kp, :]
    crossed = C2[..., k, l, kp, lp, :] + C2[..., k, l, lp, kp, :]
    return dict(direct=direct, crossed=crossed, isospin2=direct - crossed)


def meson_fields(V, L, momenta):
    """Phi[j, c, d, t, m, m'] = sum_x e^{-2 pi i p_j x / L} conj(V[idx(c,x,t), m]) V[idx(d,x,t), m'] for the columns of
    V (2 L^2, k), idx(s,x,y) = s L^2 + y L + x: the meson fields of lma_two_point(), what Engine.meson_fields computes
    one momentum at a time.  Evaluated in V's precision: a numpy.clongdouble V gives the extended-precision
    statement (phases formed in long double), anything else complex128 with the engine's phase table."""
    V = np.asarray(V)
    if V.ndim != 2 or V.shape[0] != 2 * L * L:
        raise Exception("meson_fields: V of shape %s, expected (%d, k)" % (V.shape, 2 * L * L))
    idx = np.outer(np.asarray(momenta, dtype=np.int64), np.arange(L)) % L
    if V.dtype == np.clongdouble:
        j = np.arange(L)
        ang = -2 * (4 * np.arctan(np.longdouble(1))) * j.astype(np.longdouble) / L
        tab = (np.cos(ang) + 1j * np.sin(ang)).astype(np.clongdouble)
        quarter = (4 * j) % L == 0
        tab[quarter] = np.array([1, -1j, -1, 1j], dtype=np.clongdouble)[(4 * j[quarter]) // L]
    else:
        V = V.astype(np.complex128)
        tab = _phase_table(L)
    Vr = V.reshape(2, L, L, V.shape[1])                                   # [s][t][x][m]
    out = np.zeros((len(momenta), 2, 2, L, V.shape[1], V.shape[1]), dtype=V.dtype)
    for j in range(len(momenta)):
        ph = tab[idx[j]]
        for c in range(2):
            left = np.conj(Vr[c]).transpose(0, 2, 1)                      # [t][m][x]
            for d in range(2):
                out[j, c, d] = np.matmul(left, ph[None, :, None] * Vr[d])
    return out


def low_mode_inverse(V, QV):
    """G = (V^H Q V)^-1 made Hermitian, Q V = gamma_3 A V given: the low-mode inverse of lma_two_point(), with which
    A_L^-1 = V G V^H gamma_3.  For exact eigenvectors of Q it is diag(1 / lambda)."""
    V = np.asarray(V, dtype=np.complex128)
    QV = np.asarray(QV, dtype=np.complex128)
    if V.ndim != 2 or V.shape != QV.shape:
        raise Exception("low_mode_inverse: V %s and QV %s, expected two equal (n, k)" % (V.shape, QV.shape))
    G = np.linalg.inv(V.conj().T @ QV)
    return 0.5 * (G + G.conj().T)


def low_mode_two_point(Phi, G):
    """E_L[j, a, b, c, d, t, t0] = g_a g_b sum_{m,m'} Phi[j, c, d, t, m, m'] conj(Psi[j, a, b, t0, m, m']) with
    Psi = G Phi G^H and g = (+1, -1): the pair sums of two_point() with A_L^-1 = V G V^H gamma_3 in place of A^-1,
    for every source timeslice t0, from the meson fields Phi[j, c, d, t, m, m'] of V.  Any G, Hermitian or not."""
    Phi = np.asarray(Phi, dtype=np.complex128)
    G = np.asarray(G, dtype=np.complex128)
    if Phi.ndim != 6 or Phi.shape[1:3] != (2, 2) or Phi.shape[4] != Phi.shape[5] or G.shape != Phi.shape[4:]:
        raise Exception("low_mode_two_point: Phi of shape %s and G of shape %s, expected (M, 2, 2, L, k, k) and (k, k)"
                        % (Phi.shape, G.shape))
    M, L, k = Phi.shape[0], Phi.shape[3], Phi.shape[4]
    g = np.array([1.0, -1.0])
    out = np.empty((M, 2, 2, 2, 2, L, L), dtype=np.complex128)
    for j in range(M):
        Psi = np.matmul(np.matmul(G, Phi[j]), G.conj().T)                # [a][b][t0][m][m']
        E = Phi[j].reshape(4 * L, k * k) @ Psi.reshape(4 * L, k * k).conj().T          # [(c,d,t)][(a,b,t0)]
        E = E.reshape(2, 2, L, 2, 2, L).transpose(3, 4, 0, 1, 2, 5)      # [a][b][c][d][t][t0]
        out[j] = E * (g[:, None] * g[None, :])[:, :, None, None, None, None]
    return out


def lma_correlator(result, sink, source):
    """The source-averaged correlator of a lma_two_point() result, shape (M, L), as a function of the distance
    Delta = (t - t0) mod L:

        C_low[j][Delta]  = (1 / L) sum_t0 meson_correlator(two_point_low[..., t0], sink, source)[j][(t0 + Delta) mod L]
        C_rest[j][Delta] = meson_correlator(two_point_rest, sink, source)[j][(source_timeslice + Delta) mod L]

    and C_low + C_rest is returned.  The low-mode part is exact for every source timeslice and is averaged over all of
    them; the remainder was estimated from the one source timeslice of the run.  Averaging over t0 relies on the
    translation invariance of the ENSEMBLE average, as every low-mode averaging does: on a single configuration the
    correlators from different t0 differ, and only their ensemble means coincide.  Raises on a result without
    two_point_low (two_point() has no low part)."""
    for key in ('two_point_low', 'two_point_rest', 'source_timeslice'):
        if key not in result:
            raise Exception("lma_correlator: the result has no %r (it takes the result of lma_two_point())" % key)
    low = np.asarray(result['two_point_low'])
    if low.ndim != 7 or low.shape[-1] != low.shape[-2]:
        raise Exception("lma_correlator: two_point_low of shape %s, expected (M, 2, 2, 2, 2, L, L)" % (low.shape,))
    L = low.shape[-1]
    t0 = int(result['source_timeslice'])
    shift = (np.arange(L)[:, None] + np.arange(L)[None, :]) % L           # [t0][Delta] -> t
    per_source = meson_correlator(np.moveaxis(low, -1, 0), sink, source)   # [t0][j][t]
    c_low = per_source[np.arange(L)[:, None], :, shift].mean(axis=0).T    # [t0][Delta][j] -> [j][Delta]
    c_rest = meson_correlator(result['two_point_rest'], sink, source)[:, shift[t0]]
    return c_low + c_rest


def low_mode_solutions(V, G, sources):
    """z_L = A_L^-1 eta = V G V^H gamma_3 eta for sources eta of shape (..., 2 L^2) (slice_sources' layout (2 M, nb, n)
    included), gamma_3 = +1 / -1 on the first / second half of the index."""
    V = np.asarray(V, dtype=np.complex128)
    eta = np.asarray(sources, dtype=np.complex128)
    n = V.shape[0]
    if eta.shape[-1] != n:
        raise Exception("low_mode_solutions: sources of length %d, expected %d" % (eta.shape[-1], n))
    g3 = np.where(np.arange(n) < n // 2, 1.0, -1.0)
    c = (eta * g3) @ V.conj()                                             # [...][m] = V^H gamma_3 eta
    return (c @ np.asarray(G, dtype=np.complex128).T) @ V.T


def register_low_modes(mg_solver, G):
    """Hand the low-mode inverse of the registered deflation vectors to every engine handle (None clears)."""
    for eng in _engines(mg_solver):
        eng.set_low_mode_inverse(G)


def trace_params_from_params(params, example):
    """utils.py:73-125: whitelist copy into the dictionary the estimators read."""
    if example not in ("mlmc", "hutchinson"):
        raise Exception("Value for parameter <example> not available.")
    tp = {'function_params': {'tol': params['function_tol']},
          'tol': params['trace_tol'],
          'max_nr_ests': 100000,
          'problem_name': params['matrix_params']['problem_name']}
    for key in _COMMON_KEYS:
        tp[key] = params[key]
    if example == "mlmc":
        for key in _MLMC_KEYS:
            tp[key] = params[key]
    else:
        tp['defl-type'] = params['defl_type']      # key spelled as in utils.py:113
    for key in _BUILD_KEYS:
        if key in params:
            tp[key] = params[key]
    return tp


class CustomTimer:
    """utils.py:366-445: non-reentrant wall-clock buckets.  On this build the buckets are
    additionally fed from HIP-event timings of the engine (MG.sync_timer)."""
    _PARTS = ("mvm", "defl", "P", "R", "mg_setup", "defl_setup", "axpy")

    def __init__(self):
        self.on = 0
        self.reset()

    def reset(self):
        for part in self._PARTS:
            setattr(self, part, 0.0)
        self.dots = 0.0      # Krylov inner products: untimed in the reference
        self.tbuff = 0.0

    def start(self, part):
        if self.on == 1:
            raise Exception("Can't turn timer on, it's already timing")
        self.on = 1
        self.tbuff = time.time()

    def end(self, part):
        if self.on == 0:
            raise Exception("Can't turn timer off, it's already down")
        self.on = 0
        elapsed = time.time() - self.tbuff
        if part not in self._PARTS:
            raise Exception("Uknown part to time")
        setattr(self, part, getattr(self, part) + elapsed)

    def __str__(self):
        acc = self.mvm + self.defl + self.P + self.R + self.mg_setup + self.defl_setup
        lines = ["", "Timings specific to computations:",
                 " -- matrix-vector multiplications : " + str(self.mvm),
                 " -- deflations : " + str(self.defl),
                 " -- applications of P : " + str(self.P),
                 " -- applications of R : " + str(self.R),
                 " -- applications of axpy : " + str(self.axpy),
                 " -- accumulated time : " + str(acc), ""]
        return "\n".join(lines)


def _engines(mg_solver):
    engs = getattr(mg_solver, "engines", None)
    if engs:
        return engs
    return [mg_solver.engine] if getattr(mg_solver, "engine", None) is not None else []


# ----------------------------------------------------------------------------------------
# deflation (setup-time, host)                                          utils.py:130-201
# ----------------------------------------------------------------------------------------
def _explicit_deflation_pairs(how, A, k, tolx, mg_solver, lev0):
    """eigsh(gamma_3 A, k, sigma=0) as defl_setup = "device" (block eigensolver, k <= 256; the pairs the setup
    already computed on the GPU when it had them) or "host" (ARPACK) asks."""
    if how == "host":
        Q = (lev0.g3 * A).tocsc()
        return _dist.default_comm().compute_on_root(lambda: eigsh(Q, k=k, which='LM', tol=tolx, sigma=0.0))
    if not 1 <= k <= 256:
        raise Exception("defl_setup = 'device': nr_deflat_vctrs = %d outside 1..256" % k)
    if not getattr(mg_solver, "_have_solver_hier", False):
        raise Exception("defl_setup = 'device' needs the level-0 solver hierarchy on the GPU "
                        "(the device eigensolver's shift-invert solves)")
    found = getattr(mg_solver, "_device_defl", {}).get((int(k), float(tolx)))
    if found is not None:
        return found
    from .setup_gpu import eig_width_for
    return _dist.default_comm().compute_on_root(
        lambda: mg_solver.device_eigenpairs(k, tolx, hermitian=True, width=eig_width_for(k)))


def deflation_pre_computations(A, nr_deflat_vctrs, tolx, method, timer, params, mg_solver,
                               lop=None, level_nr=0):
    if method not in ("hutchinson", "mlmc"):
        raise Exception("unknown deflation method")
    if nr_deflat_vctrs <= 0:
        if method == "hutchinson":
            for eng in _engines(mg_solver):
                eng.set_deflation(None)
            disp = displacements_of(params)
            link = link_loops_of(params)
            momenta = loops_of(params) if link is None else link
            if momenta is not None:
                L = int(params['latt_dims'][0])
                zero = np.zeros((len(momenta), 2, 2, L), dtype=np.complex128)
                return (None, zero if link is None else (zero, np.zeros((4,) + zero.shape, dtype=np.complex128)))
            return (None, 0.0 if disp is None else np.zeros(len(disp[0]), dtype=np.complex128))
        for eng in _engines(mg_solver):
            eng.set_level_deflation(level_nr, None)
        return (None, None, 0.0)

    lev0 = mg_solver.ml.levels[0]
    displaced = displacements_of(params) if method == "hutchinson" else None
    link = link_loops_of(params) if method == "hutchinson" else None
    momenta = (loops_of(params) if link is None else link) if method == "hutchinson" else None
    if method == "hutchinson":
        pre = params.get("deflation_eigenpairs") if hasattr(params, "get") else None
        how = defl_setup_of(params)
        if pre is not None:
            Sy, Vx = np.array(pre[0], dtype=float), np.array(pre[1], dtype=np.complex128)
        elif how != "auto":
            Sy, Vx = _explicit_deflation_pairs(how, A, nr_deflat_vctrs, tolx, mg_solver, lev0)
        else:
            from . import cache as _cache
            cdir = _cache.cache_dir(params)
            ckey = _cache.matrix_key(A, {"k": nr_deflat_vctrs, "tol": tolx}) if cdir else None
            hit = _cache.load(cdir, "defl", ckey) if cdir else None
            found = getattr(mg_solver, "_device_defl", {}).get((int(nr_deflat_vctrs), float(tolx)))
            if hit is not None:
                Sy, Vx = hit["S"], hit["V"]
            elif found is not None:
                # computed on the GPU during MG.setup, while the host built the coarse levels
                Sy, Vx = found
            else:
                device = (getattr(mg_solver, "_have_solver_hier", False) and nr_deflat_vctrs <= 32
                          and getattr(mg_solver, "_solver_cfg_built", None) is not None
                          and mg_solver._solver_cfg_built.get("setup") == "device"
                          and params.get("setup_eigs", os.environ.get("SW_SETUP_EIGS", "device")) == "device")
                if device:
                    # eigsh(gamma_3 A, k, sigma=0) by block subspace iteration on the GPU (utils.py:137-140)
                    Sy, Vx = _dist.default_comm().compute_on_root(
                        lambda: mg_solver.device_eigenpairs(nr_deflat_vctrs, tolx, hermitian=True))
                else:
                    Q = (lev0.g3 * A).tocsc()                               # utils.py:137-140
                    # (with several ranks: rank 0's eigenpairs everywhere, see dist.compute_on_root)
                    Sy, Vx = _dist.default_comm().compute_on_root(
                        lambda: eigsh(Q, k=nr_deflat_vctrs, which='LM', tol=tolx, sigma=0.0))
            if hit is None and cdir:
                _cache.save(cdir, "defl", ckey, {"S": Sy, "V": Vx})
    else:
        how = mlmc_defl_setup_of(params)
        mg_solver.solve_tol = params['diff_lev_op_tol']                 # utils.py:142-143
        t1 = time.time()
        if how == "device":
            # eigsh(Q_l, k, which='LM') by block subspace iteration on the GPU, 64 columns per operator
            # application (the host path solves one right-hand side per ARPACK mat-vec).  The "exact" tr1 below
            # is sum(lambda_i x_i^H gamma_3 x_i), off by -sum(x_i^H gamma_3 r_i) for residuals r_i.  Subspace
            # iteration stops right at tol (3 steps at 0.1 on schwinger128) where ARPACK's Lanczos usually
            # overshoots it, so the pairs are refined while the residual still halves per step, down to the
            # accuracy of the operator's solves (7 steps there).
            steps = []
            from .setup_gpu import eig_width_for
            Sy, Vx = _dist.default_comm().compute_on_root(
                lambda: mg_solver.device_diff_eigenpairs(level_nr, nr_deflat_vctrs, tolx, log=steps,
                                                         refine_to=params['diff_lev_op_tol'],
                                                         width=eig_width_for(nr_deflat_vctrs)))
            rec = {"method": "device", "seconds": round(time.time() - t1, 4), "steps": steps}
        else:
            Sy, Vx = _dist.default_comm().compute_on_root(
                lambda: eigsh(lop, k=nr_deflat_vctrs, which='LM', tol=tolx))
            rec = {"method": "host", "seconds": round(time.time() - t1, 4)}
        mg_solver.setup_log.setdefault("mlmc_deflation", {})[level_nr] = rec
    sgn = np.where(Sy > 0, 1.0, -1.0)
    Sabs = Sy * sgn
    Ux = Vx * sgn[None, :]
    if method == "hutchinson":
        Ux = lev0.g3 * Ux
        if displaced is not None or momenta is not None:
            # W = gamma_3 V sgn(lambda) as it is: the displacement sits on the probe side of the dots
            # (SW_MODE_HUTCHINSON_SHIFTS), tr1 is one number per displacement; the timeslice loops
            # (SW_MODE_HUTCHINSON_LOOPS) project with the same W, tr1 is the array [p][a][b][t]
            if os.getenv('OMP_NUM_THREADS') is None:                    # utils.py:161-164
                raise Exception("Run : << export OMP_NUM_THREADS=N >>")
            mg_solver.solve_tol = params['function_params']['tol']
            for eng in _engines(mg_solver):
                eng.set_deflation(np.asarray(Ux))
            if link is not None:
                # the link loops project as the timeslice loops do; tr1 = (the local array, the four link branches)
                lat = getattr(mg_solver, "lattice", None)
                if lat is None:
                    raise Exception("link_loops needs a lattice operator (the links of hierarchy.detect_lattice)")
                L = int(lat[0])
                return (Ux, (sliced_tr1(Vx, Sy, lev0.g3, L, link),
                             link_sliced_tr1(Vx, Sy, lev0.g3, lat[2], lat[3], L, link)))
            if momenta is not None:
                return (Ux, sliced_tr1(Vx, Sy, lev0.g3, int(params['latt_dims'][0]), momenta))
            return (Ux, displaced_tr1(Vx, Sy, lev0.g3, Vx.shape[0], displaced[1]))
        if params['use_permuted']:
            Ux = lev0.Pperm * Ux
    else:
        Vx = mg_solver.ml.levels[level_nr].g3 * Vx
        if getattr(mg_solver, "coarse_eo", None) is not None and level_nr >= 1:
            raise Exception("ref_coarsest = 'eo' keeps the coarse level in tile order on the GPU: MLMC-level "
                            "deflation vectors at level %d are not supported in that mode" % level_nr)
        for eng in _engines(mg_solver):
            # the GPU probe body projects with these vectors (utils.py:260-266)
            eng.set_level_deflation(level_nr, np.asarray(Vx))

    if os.getenv('OMP_NUM_THREADS') is None:                            # utils.py:161-164
        raise Exception("Run : << export OMP_NUM_THREADS=N >>")
    mg_solver.solve_tol = params['function_params']['tol']

    overlap = np.dot(Ux.transpose().conjugate(), Vx)
    if method == "hutchinson":
        tr1 = np.sum(np.diag(overlap) / Sabs)                           # utils.py:173,191
        for eng in _engines(mg_solver):
            eng.set_deflation(np.asarray(Ux))
        return (Ux, tr1)
    defl_type = params['defl_type']
    if defl_type == "exact":
        tr1 = np.sum(np.diag(overlap) * Sabs)                           # utils.py:176
    elif defl_type == "inexact_01":
        if mlmc_defl_setup_of(params) == "device":
            Vbuff = mg_solver.diff_op_block(Vx)                         # all k columns in one application
        else:
            Vbuff = np.zeros_like(Vx)
            for i in range(nr_deflat_vctrs):
                Vbuff[:, i] = mg_solver.diff_op(Vx[:, i].copy())
                print('.', end='', flush=True)
        tr1 = np.trace(np.dot(Vx.transpose().conjugate(), Vbuff))
    elif defl_type == "inexact_02":
        raise Exception("deflation type inexact_02 under construction")
    elif defl_type == "inexact_03":
        tr1 = 0.0
    else:
        raise Exception("unknown deflation type")
    return (Vx, Ux, tr1)


# ----------------------------------------------------------------------------------------
# probes
# ----------------------------------------------------------------------------------------
def draw_probes(count, n, kind="z2"):
    """`count` probes from the GLOBAL NumPy stream as int8 codes, shape (count, n).

    kind "z2" (the reference): identical to `count` calls of np.random.randint(2, size=n)
    (utils.py:213-215), entries +-1.  kind "z4" (build-only option, BASELINE config 1; NOT in the
    reference): one draw of np.random.randint(4) per entry, 0,1,2,3 -> 1, i, -1, -i, encoded as
    +1, +2, -1, -2."""
    if kind == "z2":
        bits = np.random.randint(2, size=(count, n))
        return (2 * bits - 1).astype(np.int8)
    if kind == "z4":
        q = np.random.randint(4, size=(count, n))
        return np.array([1, 2, -1, -2], dtype=np.int8)[q]
    raise Exception("unknown probe type")


def probes_as_complex(probes):
    """int8 probe codes -> the complex vectors they stand for."""
    p = np.asarray(probes)
    return np.where(np.abs(p) == 2, 1j * (p // 2), p).astype(np.complex128)


def _batch_args(mg_solver, params, method, level, deflated):
    """(engine handles, mode, solve tolerance, level size, iteration cap) of a probe batch of `method` at `level`."""
    engs = _engines(mg_solver)
    if not engs:
        raise EngineError("no GPU engine attached (run MG.setup first)")
    n = mg_solver.ml.levels[level].A.shape[0]
    mode = probe_mode(method, level, getattr(mg_solver, "skip_level", False), deflated)
    return engs, mode, params['function_params']['tol'], n, (n if n < 1000 else 1000)


def probe_batch(mg_solver, params, method, probes, level=0, deflated=False):
    """Evaluate one batch of probes on the GPU: returns (ests, iters_fine, iters_coarse).

    hutchinson: e = x^H A^-1 Pperm^T (x - U U^H x)            utils.py:210-250
    mlmc      : e = x^H A_f^-1 C x - x^H P A_c^-1 R C x        utils.py:252-361
    (deflation vectors and permutation were registered with the engine at setup).  The resolved methods return
    one row per probe from one projection and one solve per probe, on the first engine handle:
    shifts    : ests[nb, S], e[k, j] = (D_{s_j}^T x_k)^H A^-1 (x_k - W W^H x_k) at every registered shift
    loops     : loops[nb, nmom, 2, 2, L] (MODE_HUTCHINSON_LOOPS)
    link_loops: rows[nb, 5, nmom, 2, 2, L] (MODE_HUTCHINSON_LINK_LOOPS): [:, 0] the local loops, [:, 1:] the four
                link branches (F_x, B_x, F_t, B_t)
    mlmc_loops: loops[nb, nmom, 2, 2, L], the term of `level` (MODE_MLMC_LOOPS, _SKIP at level 0 with
                mg_solver.skip_level; deflated: MODE_MLMC_DEFL_LOOPS / _SKIP, the level's registered projection)
    two_point : T[nb, nmom, 2, 2, 2, 2, L], the probes being the noises: 2 nmom solves per noise, no deflation;
                iters_fine is the largest count among a noise's solves."""
    engs, mode, tol, _, maxiter = _batch_args(mg_solver, params, method, level, deflated)
    probes = np.asarray(probes)
    nb = probes.shape[0]
    if mode in RESOLVED_FETCH:
        return engs[0].hutch_batch_resolved(mode, level, probes, tol, maxiter)
    if len(engs) == 1 or nb < 2 * 64:
        return engs[0].hutch_batch(mode, level, probes, tol, maxiter)
    # several engine handles = several HIP streams on the same GPU: the sub-batches overlap
    # (MFMA-bound coarse kernels of one with HBM-bound fine kernels of the other)
    from concurrent.futures import ThreadPoolExecutor
    parts = np.array_split(np.arange(nb), len(engs))
    with ThreadPoolExecutor(max_workers=len(engs)) as pool:
        futs = [pool.submit(eng.hutch_batch, mode, level, probes[idx], tol, maxiter)
                for eng, idx in zip(engs, parts) if len(idx)]
        res = [f.result() for f in futs]
    return tuple(np.concatenate([r[k] for r in res]) for k in range(3))


def register_shifts(mg_solver, shifts):
    """Hand the flat shifts of the displaced traces to every engine handle (None clears)."""
    for eng in _engines(mg_solver):
        eng.set_shifts(shifts)


def register_loop_momenta(mg_solver, momenta):
    """Hand the momenta of the timeslice loops to every engine handle (None clears)."""
    for eng in _engines(mg_solver):
        eng.set_loop_momenta(momenta)


def register_two_point(mg_solver, t0, momenta):
    """Hand the source timeslice and momenta of two_point() to every engine handle (momenta None clears)."""
    for eng in _engines(mg_solver):
        eng.set_two_point(t0, momenta)


def register_smearing(mg_solver, sel):
    """Hand the registration of the smeared two_point() -- smearing_of's dict, None clears -- to every engine handle."""
    for eng in _engines(mg_solver):
        if sel is None:
            eng.set_smearing(1.0, 0, None)
        else:
            eng.set_smearing(sel['kappa'], sel['source'], sel['sink'])


def register_three_point(mg_solver, sel):
    """Hand the registration of three_point() -- three_point_of's dict, None clears -- to every engine handle."""
    for eng in _engines(mg_solver):
        if sel is None:
            eng.set_three_point(0, 1, 'g3', 0, None)
        else:
            eng.set_three_point(sel['t0'], sel['tf'], sel['sink'], sel['pf'], sel['momenta'])


def probe_batch_generated(mg_solver, params, method, level, first_probe, count, kind="z2",
                          prefetch=None, ready=None, deflated=False):
    """Like probe_batch, for the probes [first_probe, first_probe + count) of the stream the
    engines were handed with Engine.stream_set: each engine GENERATES its contiguous share in
    HBM (k_mt_generate, bit-exact with np.random.randint, utils.py:213-216,255-258) and
    evaluates it; only the 16-byte estimates -- and the rows of a resolved method -- come back.

    Generation is asynchronous on the engines' generation streams.  `prefetch` = (first_probe, count)
    of the batch expected NEXT: its probes are queued into the engines' other slot before this batch is
    solved, so they are drawn while the solve runs; `ready` = the (first_probe, count, slot) a previous
    call prefetched (skips this batch's own generation when it matches).  Returns
    (ests, iters_fine, iters_coarse, prefetched) with prefetched = (first, count, slot) or None."""
    engs, mode, tol, n, maxiter = _batch_args(mg_solver, params, method, level, deflated)
    resolved = mode in RESOLVED_FETCH
    ne = len(engs) if count >= 2 * 64 else 1

    def shares(cnt):
        return [(k * cnt) // ne for k in range(ne + 1)]

    slot = 0
    have = ready is not None and ready[0] == first_probe and ready[1] == count
    if have:
        slot = ready[2]
    bounds = shares(count)
    if not have:
        for k in range(ne):
            if bounds[k + 1] > bounds[k]:
                engs[k].probes_generate(slot, level, bounds[k + 1] - bounds[k],
                                        (first_probe + bounds[k]) * n, kind)
    prefetched = None
    if prefetch is not None and prefetch[1] > 0 and (ne == (len(engs) if prefetch[1] >= 2 * 64 else 1)):
        nslot = 1 - slot
        nb2 = shares(prefetch[1])
        for k in range(ne):
            if nb2[k + 1] > nb2[k]:
                engs[k].probes_generate(nslot, level, nb2[k + 1] - nb2[k], (prefetch[0] + nb2[k]) * n, kind)
        prefetched = (prefetch[0], prefetch[1], nslot)

    def run(eng):
        eng.probes_select(slot)
        eng.hutch_run(mode, level, tol, maxiter)
        ests, itf, itc = eng.hutch_fetch()
        return (eng.hutch_fetch_resolved(mode) if resolved else ests), itf, itc

    active = [engs[k] for k in range(ne) if bounds[k + 1] > bounds[k]]
    if len(active) == 1:
        res = [run(active[0])]
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=len(active)) as pool:
            res = list(pool.map(run, active))
    return tuple(np.concatenate([r[k] for r in res]) for k in range(3)) + (prefetched,)


def one_defl_Hutch_step(Af, Ac, mg_solver, params, method, nr_deflat_vctrs, Vx, Ux, i=0,
                        output_params=None, P=None, R=None, Pn=None, Rn=None):
    """utils.py:207-361, one probe.  The probe comes from the global NumPy stream exactly as in
    the reference; the arithmetic runs on the GPU.  MLMC-level deflation vectors (Vx with
    method == "mlmc") are applied on the host before the batch call."""
    n = Af.shape[0]
    if method == "hutchinson":
        probes = draw_probes(1, n)
        mg_solver.level_nr = 0
        e, itf, _ = probe_batch(mg_solver, params, "hutchinson", probes, 0)
        mg_solver.num_iters = int(itf[0])
        itrs = int(itf[0])
        est = e[0]
    elif method == "mlmc":
        if nr_deflat_vctrs > 0 and params['defl_type'] not in ("exact", "inexact_01"):
            if params['defl_type'] == "inexact_02":
                raise Exception("deflation type inexact_02 under construction")
            if params['defl_type'] == "inexact_03":
                raise Exception("deflation type inexact_03 is not available on the GPU probe path")
            raise Exception("unknown deflation type")
        # with nr_deflat_vctrs > 0 the projection x0 - V V^H x0 (utils.py:266) uses the vectors that
        # deflation_pre_computations registered with the engine for level i
        probes = draw_probes(1, n)
        mg_solver.level_nr = i
        e, itf, itc = probe_batch(mg_solver, params, "mlmc", probes, i)
        lc = i + 2 if (mg_solver.skip_level and i == 0) else i + 1
        output_params['results'][i]['function_iters'] += int(itf[0])
        output_params['results'][lc]['function_iters'] += int(itc[0])
        itrs = 0
        est = e[0]
    else:
        raise Exception("unknown method")
    print('.', end='', flush=True)
    return (est, itrs)
