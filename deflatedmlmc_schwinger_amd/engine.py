"""ctypes binding of the C ABI in ``include/schwinger_hip.h`` (libschwinger_hip.so).

The library is the product's only compute path.  If it is missing, or no HIP
device is visible, construction of :class:`Engine` raises -- there is no CPU
fallback in this package (the NumPy restatement under ``oracle/`` is test
infrastructure and is never imported from here).
"""
import ctypes as C
import os
import sys

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libschwinger_hip.so")

MODE_HUTCHINSON = 0
MODE_MLMC = 1
MODE_MLMC_SKIP = 2
MODE_LEVEL = 3
MODE_HUTCHINSON_SHIFTS = 4
MODE_HUTCHINSON_LOOPS = 5
MODE_TWO_POINT = 6
MODE_MLMC_LOOPS = 7
MODE_MLMC_LOOPS_SKIP = 8
MODE_MLMC_DEFL_LOOPS = 9
MODE_MLMC_DEFL_LOOPS_SKIP = 10
MODE_TWO_POINT_LMA = 11
MODE_HUTCHINSON_LINK_LOOPS = 12
MODE_THREE_POINT = 13
MODE_TWO_POINT_SMEARED = 14
# estimator method -> (mode, mode of the level-skipping form at level 0); "mlmc_defl_loops" is "mlmc_loops" deflated
_METHOD_MODES = {"hutchinson": (MODE_HUTCHINSON, MODE_HUTCHINSON),
                 "mlmc": (MODE_MLMC, MODE_MLMC_SKIP),
                 "level": (MODE_LEVEL, MODE_LEVEL),
                 "shifts": (MODE_HUTCHINSON_SHIFTS, MODE_HUTCHINSON_SHIFTS),
                 "loops": (MODE_HUTCHINSON_LOOPS, MODE_HUTCHINSON_LOOPS),
                 "link_loops": (MODE_HUTCHINSON_LINK_LOOPS, MODE_HUTCHINSON_LINK_LOOPS),
                 "two_point": (MODE_TWO_POINT, MODE_TWO_POINT),
                 "two_point_lma": (MODE_TWO_POINT_LMA, MODE_TWO_POINT_LMA),
                 "two_point_smeared": (MODE_TWO_POINT_SMEARED, MODE_TWO_POINT_SMEARED),
                 "three_point": (MODE_THREE_POINT, MODE_THREE_POINT),
                 "mlmc_loops": (MODE_MLMC_LOOPS, MODE_MLMC_LOOPS_SKIP),
                 "mlmc_defl_loops": (MODE_MLMC_DEFL_LOOPS, MODE_MLMC_DEFL_LOOPS_SKIP)}
# the modes whose batches leave a resolved result beside the scalar estimates -> the Engine method that fetches it
RESOLVED_FETCH = {MODE_HUTCHINSON_SHIFTS: "hutch_fetch_shifts",
                  MODE_HUTCHINSON_LOOPS: "hutch_fetch_loops",
                  MODE_HUTCHINSON_LINK_LOOPS: "hutch_fetch_link_resolved",
                  MODE_TWO_POINT: "hutch_fetch_two_point",
                  MODE_TWO_POINT_LMA: "hutch_fetch_two_point_lma",
                  MODE_TWO_POINT_SMEARED: "hutch_fetch_two_point_smeared",
                  MODE_THREE_POINT: "hutch_fetch_three_point_resolved",
                  MODE_MLMC_LOOPS: "hutch_fetch_mlmc_loops",
                  MODE_MLMC_LOOPS_SKIP: "hutch_fetch_mlmc_loops",
                  MODE_MLMC_DEFL_LOOPS: "hutch_fetch_mlmc_loops",
                  MODE_MLMC_DEFL_LOOPS_SKIP: "hutch_fetch_mlmc_loops"}


def probe_mode(method, level=0, skip_level=False, deflated=False):
    """The engine mode of estimator `method` at `level`: with skip_level (MG.skip_level) the difference methods
    take their level-skipping mode at level 0; deflated selects the MLMC loops with the level's projection."""
    if method == "mlmc_loops" and deflated:
        method = "mlmc_defl_loops"
    if method not in _METHOD_MODES:
        raise Exception("unknown method")
    return _METHOD_MODES[method][1 if (skip_level and level == 0) else 0]


KCLASS_TP_SOURCES = 17     # sw_kernel_stats classes of the two-point kernels
KCLASS_TP_DOTS = 18
KCLASS_SLICE_CDOTS = 19    # ... and of k_slice_cdots (MLMC loops)
KCLASS_MESON_FIELD = 20    # ... and of k_meson_field (low-mode averaging)
KCLASS_LM_CONTRACT = 21    # ... and of k_cgemm_nt / k_lm_two_point_reduce (low_mode_two_point)
KCLASS_LINK_DOTS = 22      # ... and of k_slice_link_dots (link loops)
KCLASS_3PT_SOURCES = 23    # ... and of k_seq_sources / k_pair_slice_total and the stage-1 sources (three-point functions)
KCLASS_3PT_DOTS = 24       # ... and of k_slice_seq_dots
KCLASS_SMEAR = 25          # ... and of k_smear_step / k_smear_fused (smeared two-point functions)
KCLASS_LAPH = 26           # ... and of k_laph_sources / k_laph_project (distillation)
KCLASS_LAPH_CONTRACT = 27  # ... and of k_laph_elementals / k_laph_left / k_laph_right / k_laph_reduce
KCLASS_LAPH_GENERALIZED = 28   # ... and of k_laph_generalized (generalized perambulators)
KCLASS_LAPH_TWO_MESON = 30     # (29 is no class: kernel_stats(29) stays out of range) ... and of k_laph_sink / k_laph_sandwich / k_laph_source / k_laph_trace1 / k_laph_trace2
MAX_MESON_OPS = 4              # SW_MAX_MESON_OPS: sink operators, and source operators, of one two-meson call
MAX_LAPH = 128             # SW_MAX_LAPH
MAX_SINK_LEVELS = 4        # SW_MAX_SINK_LEVELS, SW_MAX_SMEARING_STEPS
MAX_SMEARING_STEPS = 1024
SINK_GAMMAS = ('1', 'g3', 's1', 's2')      # the sink spin matrix codes of set_three_point
MAX_SHIFTS = 128
MAX_MOMENTA = 8
# operations of Engine.apply_op32 / apply_op64 (SW_OP32_* of the header): one kernel of the complex64 / fp64
# cycle at a time
OP32_A = 0
OP32_R = 1
OP32_P = 2
OP32_P_EVEN = 3
OP32_RE = 4
OP32_COARSEST = 5
OP32_EO0 = 6                 # + q: even-odd operator q = 0..4 of a block level
OP32_SCHUR = 11
OP32_EO_SMOOTH = 12
OP32_EO_SMOOTH_REDUCED = 13
OP32_INPLACE = 1
# Engine.krylov_* (SW_KRYLOV_* of the header): one operation of the Krylov solver alone
KRYLOV_C128, KRYLOV_C64 = 0, 1
KRYLOV_INIT, KRYLOV_NOTAIL = 1, 2
KRYLOV_NORM, KRYLOV_W32 = 1, 2
KRYLOV_BEGIN, KRYLOV_HESS, KRYLOV_VERIFY, KRYLOV_SOLVE = 1, 2, 3, 5
# the packed FGMRES state of sw_krylov_scalars: (key, rows of nb complex entries for restart length m)
KRYLOV_STATE = (("H", lambda m: (m + 1) * m), ("cs", lambda m: m), ("sn", lambda m: m), ("g", lambda m: m + 1),
                ("y", lambda m: m), ("normb", lambda m: 1), ("relres", lambda m: 1), ("svec", lambda m: m + 1),
                ("ys", lambda m: m))
PROBES_Z2 = 1
PROBES_Z4 = 2
PROBE_KINDS = {"z2": PROBES_Z2, "z4": PROBES_Z4}

TIMER_NAMES = ("mvm", "defl", "P", "R", "axpy", "dots", "coarsest", "other")


class EngineError(RuntimeError):
    pass


_lib = None


def load_library():
    """Load the C-ABI library (raises EngineError when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            "HIP engine library not built: %s is missing (run `python -c 'import "
            "__graft_entry__ as g; g.build()'` or `make -C deflatedmlmc_schwinger_amd/csrc`)"
            % LIB_PATH)
    if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1 and "torch" not in sys.modules:
        # A multi-rank launch will use torch.distributed (backend nccl = RCCL).  PyTorch bundles its own
        # ROCm runtime: loaded AFTER this library it is mapped as a second HIP / HSA runtime in the process
        # (same sonames, different files: /proc/self/maps shows both), loaded BEFORE it the dynamic loader
        # resolves this library's libamdhip64.so.7 / libhsa-runtime64.so.1 to PyTorch's mapped copies --
        # one runtime serving both.  So: torch first.
        try:
            import torch  # noqa: F401
        except Exception:      # no torch: the engine runs on the system runtime alone
            pass
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the box
        raise EngineError("cannot load %s: %s" % (LIB_PATH, e))
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    P = C.POINTER

    def sig(name, res, *args):
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = list(args)

    sig("sw_create", i32, P(vp), i32)
    sig("sw_destroy", i32, vp)
    sig("sw_last_error", C.c_char_p, vp)
    sig("sw_device_count", i32)
    sig("sw_version", C.c_char_p)
    sig("sw_hier_begin", i32, vp, i32, i32)
    sig("sw_set_lattice", i32, vp, i32, i32, dbl, vp, vp)
    sig("sw_set_csr", i32, vp, i32, i32, i32, vp, vp, vp)
    sig("sw_set_transfer", i32, vp, i32, i32, i32, i32, vp, vp, vp)
    sig("sw_set_coarsest_inv", i32, vp, i32, i32, vp)
    sig("sw_set_cycle", i32, vp, i32, i32, i32, i32, i32)
    sig("sw_set_smoother", i32, vp, i32, i32, i32, vp, i32, vp)
    sig("sw_set_gmres_smoother", i32, vp, i32, i32, i32, i32)
    sig("sw_set_eo_smoother", i32, vp, i32, i32, i32, vp)
    sig("sw_set_eo_operator", i32, vp, i32, i32, i32, i32, i32, vp, vp, vp)
    sig("sw_setup_eo_operators", i32, vp, i32, i32, i32)
    sig("sw_apply_eo_operator", i32, vp, i32, i32, i32, i32, vp, vp)
    sig("sw_get_level_bsr", i32, vp, i32, i32, P(i32), vp, vp)
    sig("sw_setup_testvectors", i32, vp, i32, i32, i32, C.c_uint64, i32, dbl, i32, i32, vp)
    sig("sw_setup_transfer", i32, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp)
    sig("sw_setup_galerkin", i32, vp, i32, i32, i32, vp)
    sig("sw_get_level_dense", i32, vp, i32, i32, vp)
    sig("sw_setup_invert_coarsest", i32, vp, i32)
    sig("sw_setup_direct_level", i32, vp, i32, i32)
    sig("sw_setup_level_inverse", i32, vp, i32, i32)
    sig("sw_setup_arnoldi", i32, vp, i32, i32, i32, i32, C.c_uint64, vp)
    sig("sw_hier_end", i32, vp, i32)
    sig("sw_set_deflation", i32, vp, i32, vp)
    sig("sw_set_level_deflation", i32, vp, i32, i32, vp)
    sig("sw_set_perm", i32, vp, i32, i64)
    sig("sw_set_rhsmap", i32, vp, i32, i32, vp, vp, vp)
    sig("sw_set_solver", i32, vp, i32, i32)
    sig("sw_set_option", i32, vp, C.c_char_p, dbl)
    sig("sw_get_option", i32, vp, C.c_char_p, P(dbl))
    sig("sw_pool_trim", i32)
    sig("sw_get_coarsest_inv", i32, vp, i32, vp)
    sig("sw_eig_begin", i32, vp, i32, i32, C.c_uint64)
    sig("sw_eig_begin_wide", i32, vp, i32, i32, C.c_uint64, i32)
    sig("sw_eig_load", i32, vp, i32, i32, vp)
    sig("sw_eig_solve", i32, vp, i32, i32, i32, dbl, i32, P(i32))
    sig("sw_eig_apply_diff", i32, vp, i32, i32, i32, i32, dbl, i32, P(i32))
    sig("sw_eig_gram", i32, vp, i32, i32, vp)
    sig("sw_eig_rotate", i32, vp, i32, vp, i32, i32)
    sig("sw_eig_fetch", i32, vp, i32, i32, vp)
    sig("sw_eig_end", i32, vp)
    sig("sw_apply_dirac", i32, vp, i32, i32, i32, vp, vp)
    sig("sw_restrict", i32, vp, i32, i32, i32, vp, vp)
    sig("sw_prolong", i32, vp, i32, i32, i32, vp, vp)
    sig("sw_coarsest", i32, vp, i32, i32, vp, vp)
    sig("sw_apply_deflation", i32, vp, i32, i32, i32, vp, vp)
    sig("sw_vcycle", i32, vp, i32, i32, i32, vp, vp)
    sig("sw_apply_op32", i32, vp, i32, i32, i32, i32, i32, vp, vp, dbl, dbl, i32, vp, vp)
    sig("sw_apply_op64", i32, vp, i32, i32, i32, i32, i32, vp, vp, dbl, dbl, i32, vp, vp)
    sig("sw_krylov_multidot", i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp)
    sig("sw_krylov_gram_cycle", i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, dbl, dbl, i32, vp, vp, vp, vp,
        P(i32), vp)
    sig("sw_krylov_multiaxpy", i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, dbl, vp, vp, vp, vp)
    sig("sw_krylov_scalars", i32, vp, i32, i32, i32, i32, i32, dbl, dbl, i32, vp, vp, vp, vp, vp, P(i32))
    sig("sw_solve", i32, vp, i32, i32, i32, vp, vp, dbl, i32, vp, vp)
    sig("sw_hutch_batch", i32, vp, i32, i32, i32, vp, dbl, i32, vp, vp)
    sig("sw_probes_upload", i32, vp, i32, i32, vp)
    sig("sw_probes_upload_slot", i32, vp, i32, i32, i32, vp)
    sig("sw_probes_select", i32, vp, i32)
    sig("sw_kernel_stats", i32, vp, i32, P(dbl), P(i64))
    sig("sw_kernel_work", i32, vp, i32, P(dbl))
    sig("sw_comm_unique_id", i32, vp)
    sig("sw_comm_init", i32, vp, i32, i32, vp)
    sig("sw_allreduce_stats", i32, vp, vp)
    sig("sw_comm_destroy", i32, vp)
    sig("sw_hutch_run", i32, vp, i32, i32, dbl, i32)
    sig("sw_sync", i32, vp)
    sig("sw_hutch_fetch", i32, vp, vp, vp)
    sig("sw_bench_dirac", i32, vp, i32, i32, i32, i32, P(dbl))
    sig("sw_set_profiling", i32, vp, i32)
    sig("sw_timers", i32, vp, P(dbl))
    sig("sw_timers_reset", i32, vp)
    sig("sw_launch_count", i32, vp, P(i64))
    sig("sw_mt_create", vp, C.c_uint32)
    sig("sw_mt_destroy", None, vp)
    sig("sw_mt_skip", None, vp, C.c_uint64)
    sig("sw_mt_raw", None, vp, C.c_uint64, vp)
    sig("sw_mt_rademacher", None, vp, C.c_uint64, vp)
    sig("sw_mt_z4", None, vp, C.c_uint64, vp)
    sig("sw_mt_from_state", vp, vp, i32)
    sig("sw_mt_get_state", None, vp, vp, P(i32))
    sig("sw_mt_window", None, vp, vp)
    sig("sw_mt_jump", i32, vp, C.c_uint64)
    sig("sw_mt_jump_poly", i32, C.c_uint64, vp)
    sig("sw_mt_window_jump", i32, vp, C.c_uint64, vp)
    sig("sw_probes_stream_set", i32, vp, vp)
    sig("sw_probes_generate", i32, vp, i32, i32, i32, i32, C.c_uint64)
    sig("sw_probes_fetch", i32, vp, i32, vp)
    sig("sw_set_shifts", i32, vp, i32, vp)
    sig("sw_hutch_fetch_shifts", i32, vp, vp)
    sig("sw_apply_shift_dots", i32, vp, i32, vp, vp, vp)
    sig("sw_set_loop_momenta", i32, vp, i32, vp)
    sig("sw_hutch_fetch_loops", i32, vp, vp)
    sig("sw_apply_slice_dots", i32, vp, i32, vp, vp, vp)
    sig("sw_set_two_point", i32, vp, i32, i32, vp)
    sig("sw_hutch_fetch_two_point", i32, vp, vp)
    sig("sw_apply_slice_sources", i32, vp, i32, vp, vp)
    sig("sw_apply_pair_dots", i32, vp, i32, vp, vp)
    sig("sw_apply_slice_cdots", i32, vp, i32, vp, vp, vp)
    sig("sw_coarsest_loops", i32, vp, vp)
    sig("sw_hutch_fetch_mlmc_loops", i32, vp, vp)
    sig("sw_level_deflation_loops", i32, vp, i32, i32, dbl, i32, vp)
    sig("sw_meson_fields", i32, vp, i32, vp)
    sig("sw_low_mode_two_point", i32, vp, i32, vp)
    sig("sw_set_low_mode_inverse", i32, vp, i32, vp)
    sig("sw_apply_low_mode", i32, vp, i32, vp, vp)
    sig("sw_hutch_fetch_two_point_lma", i32, vp, vp)
    sig("sw_hutch_fetch_link_loops", i32, vp, vp)
    sig("sw_apply_slice_link_dots", i32, vp, i32, vp, vp, vp)
    sig("sw_set_three_point", i32, vp, i32, i32, i32, i32, i32, vp)
    sig("sw_hutch_fetch_three_point", i32, vp, vp)
    sig("sw_apply_seq_sources", i32, vp, i32, vp, vp)
    sig("sw_apply_seq_dots", i32, vp, i32, vp, vp, vp)
    sig("sw_set_smearing", i32, vp, dbl, i32, i32, vp)
    sig("sw_apply_smearing", i32, vp, i32, i32, i32, vp, vp)
    sig("sw_hutch_fetch_two_point_smeared", i32, vp, vp)
    sig("sw_set_distillation", i32, vp, i32, vp)
    sig("sw_perambulators", i32, vp, i32, vp, dbl, i32, vp, vp)
    sig("sw_apply_laph_sources", i32, vp, i32, vp, vp)
    sig("sw_apply_laph_project", i32, vp, i32, vp, vp)
    sig("sw_set_distillation_momenta", i32, vp, i32, vp)
    sig("sw_apply_laph_elementals", i32, vp, vp)
    sig("sw_distilled_two_point", i32, vp, i32, vp, dbl, i32, vp, vp, vp, vp)
    sig("sw_apply_laph_contract", i32, vp, i32, vp, vp, vp, vp)
    sig("sw_distilled_two_meson", i32, vp, i32, vp, i32, vp, vp, i32, vp, vp, dbl, i32, vp, vp, vp)
    sig("sw_apply_laph_two_meson", i32, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp)
    sig("sw_generalized_perambulators", i32, vp, i32, i32, i32, vp, i32, vp, dbl, i32, vp, vp, vp)
    sig("sw_apply_laph_generalized", i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp)
    _lib = lib
    return lib


EXPORTED_SYMBOLS = (
    "sw_create", "sw_destroy", "sw_last_error", "sw_device_count", "sw_version", "sw_hier_begin",
    "sw_set_lattice", "sw_set_csr", "sw_set_transfer", "sw_set_coarsest_inv", "sw_set_cycle",
    "sw_set_smoother", "sw_set_gmres_smoother", "sw_set_eo_smoother", "sw_set_eo_operator", "sw_setup_eo_operators", "sw_apply_eo_operator",
    "sw_get_level_bsr", "sw_setup_testvectors", "sw_setup_transfer",
    "sw_setup_galerkin", "sw_get_level_dense", "sw_setup_invert_coarsest", "sw_setup_direct_level", "sw_setup_level_inverse", "sw_setup_arnoldi", "sw_hier_end", "sw_set_deflation", "sw_set_level_deflation", "sw_set_perm", "sw_set_rhsmap", "sw_set_solver", "sw_set_option", "sw_get_option",
    "sw_pool_trim", "sw_get_coarsest_inv", "sw_eig_begin", "sw_eig_begin_wide", "sw_eig_load", "sw_eig_solve", "sw_eig_apply_diff", "sw_eig_gram", "sw_eig_rotate", "sw_eig_fetch", "sw_eig_end",
    "sw_apply_dirac", "sw_restrict", "sw_prolong", "sw_coarsest", "sw_apply_deflation", "sw_vcycle", "sw_apply_op32", "sw_apply_op64", "sw_solve",
    "sw_krylov_multidot", "sw_krylov_gram_cycle", "sw_krylov_multiaxpy", "sw_krylov_scalars",
    "sw_hutch_batch", "sw_probes_upload", "sw_probes_upload_slot", "sw_probes_select",
    "sw_kernel_stats", "sw_kernel_work", "sw_hutch_run", "sw_sync", "sw_hutch_fetch",
    "sw_comm_unique_id", "sw_comm_init", "sw_allreduce_stats", "sw_comm_destroy",
    "sw_bench_dirac", "sw_set_profiling", "sw_timers", "sw_timers_reset", "sw_launch_count",
    "sw_mt_create", "sw_mt_destroy", "sw_mt_skip", "sw_mt_raw", "sw_mt_rademacher",
    "sw_mt_z4", "sw_mt_from_state", "sw_mt_get_state", "sw_mt_window", "sw_mt_jump",
    "sw_mt_jump_poly", "sw_mt_window_jump",
    "sw_probes_stream_set", "sw_probes_generate", "sw_probes_fetch",
    "sw_set_shifts", "sw_hutch_fetch_shifts", "sw_apply_shift_dots",
    "sw_set_loop_momenta", "sw_hutch_fetch_loops", "sw_apply_slice_dots",
    "sw_set_two_point", "sw_hutch_fetch_two_point", "sw_apply_slice_sources", "sw_apply_pair_dots",
    "sw_apply_slice_cdots", "sw_coarsest_loops", "sw_hutch_fetch_mlmc_loops", "sw_level_deflation_loops",
    "sw_meson_fields", "sw_low_mode_two_point", "sw_set_low_mode_inverse", "sw_apply_low_mode", "sw_hutch_fetch_two_point_lma",
    "sw_hutch_fetch_link_loops", "sw_apply_slice_link_dots",
    "sw_set_three_point", "sw_hutch_fetch_three_point", "sw_apply_seq_sources", "sw_apply_seq_dots",
    "sw_set_smearing", "sw_apply_smearing", "sw_hutch_fetch_two_point_smeared",
    "sw_set_distillation", "sw_perambulators", "sw_apply_laph_sources", "sw_apply_laph_project",
    "sw_set_distillation_momenta", "sw_apply_laph_elementals", "sw_distilled_two_point", "sw_apply_laph_contract",
    "sw_generalized_perambulators", "sw_apply_laph_generalized",
    "sw_distilled_two_meson", "sw_apply_laph_two_meson",
)


def pool_trim():
    """Release the device memory the engines' process-wide block pool has parked."""
    return load_library().sw_pool_trim()


def device_count():
    return int(load_library().sw_device_count())


def _c128(a):
    return np.ascontiguousarray(a, dtype=np.complex128)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _csr_parts(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    indptr = np.ascontiguousarray(M.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(M.indices, dtype=np.int32)
    data = _c128(M.data)
    return M.shape, indptr, indices, data


class Engine:
    """One handle = one GPU + one stream.  Vectors passed in and out are NumPy arrays in the
    reference ordering, shape (n,) or (nb, n) (one row per right-hand side)."""

    def __init__(self, device=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        rc = self._lib.sw_create(C.byref(self._h), int(device))
        if rc != 0:
            msg = self._lib.sw_last_error(None)
            self._h = None
            raise EngineError("sw_create failed: %s" % (msg.decode() if msg else "unknown"))
        self.device = int(device)
        self.level_sizes = {}

    # -- plumbing --------------------------------------------------------------------------
    def _chk(self, rc, what):
        if rc != 0:
            msg = self._lib.sw_last_error(self._h)
            raise EngineError("%s failed: %s" % (what, msg.decode() if msg else "unknown"))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sw_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- operands --------------------------------------------------------------------------
    def hier_begin(self, hid, nlevels):
        self._chk(self._lib.sw_hier_begin(self._h, hid, nlevels), "sw_hier_begin")
        self.level_sizes[hid] = [0] * nlevels
        if hid == 0:
            self._nshifts = 0          # the engine drops its shift registration with hierarchy 0
            self._nmom = 0             # ... and its loop momenta
            self._t3_nmom = 0          # ... and its three-point registration
            self._lh_nev = 0           # ... and its distillation vectors
            self._lh_nmom = 0          # ... with their momenta

    def set_lattice(self, hid, L, mass, U1, U2):
        U1, U2 = _c128(U1), _c128(U2)
        if U1.size != L * L or U2.size != L * L:
            raise EngineError("link arrays must have L*L entries")
        self._chk(self._lib.sw_set_lattice(self._h, hid, L, float(mass), _ptr(U1), _ptr(U2)),
                  "sw_set_lattice")
        self.level_sizes[hid][0] = 2 * L * L

    def set_csr(self, hid, level, A):
        (n, m), indptr, indices, data = _csr_parts(A)
        if n != m:
            raise EngineError("level operator must be square")
        self._chk(self._lib.sw_set_csr(self._h, hid, level, n, _ptr(indptr), _ptr(indices),
                                       _ptr(data)), "sw_set_csr")
        self.level_sizes[hid][level] = n

    def set_transfer(self, hid, level, P):
        (nf, nc), indptr, indices, data = _csr_parts(P)
        self._chk(self._lib.sw_set_transfer(self._h, hid, level, nf, nc, _ptr(indptr),
                                            _ptr(indices), _ptr(data)), "sw_set_transfer")
        self.level_sizes[hid][level] = nf
        self.level_sizes[hid][level + 1] = nc

    def set_coarsest_inv(self, hid, M):
        M = _c128(np.asarray(M))
        if M.ndim != 2 or M.shape[0] != M.shape[1]:
            raise EngineError("coarsest inverse must be a square dense matrix")
        self._chk(self._lib.sw_set_coarsest_inv(self._h, hid, M.shape[0], _ptr(M)),
                  "sw_set_coarsest_inv")
        self.level_sizes[hid][-1] = M.shape[0]

    def set_cycle(self, hid, level, nu_pre, nu_post, kcycle=0):
        self._chk(self._lib.sw_set_cycle(self._h, hid, level, nu_pre, nu_post, kcycle),
                  "sw_set_cycle")

    def set_smoother(self, hid, level, w_pre, w_post):
        wp = _c128(np.asarray(w_pre if w_pre is not None else [], dtype=np.complex128))
        wq = _c128(np.asarray(w_post if w_post is not None else [], dtype=np.complex128))
        self._chk(self._lib.sw_set_smoother(self._h, hid, level, wp.size,
                                            _ptr(wp) if wp.size else None, wq.size,
                                            _ptr(wq) if wq.size else None), "sw_set_smoother")

    def set_eo_smoother(self, hid, level, w_post):
        wq = _c128(np.asarray(w_post if w_post is not None else [], dtype=np.complex128))
        self._chk(self._lib.sw_set_eo_smoother(self._h, hid, level, wq.size,
                                               _ptr(wq) if wq.size else None), "sw_set_eo_smoother")

    def set_eo_operator(self, hid, level, which, tmap, kcol, vals):
        tmap = np.ascontiguousarray(tmap, dtype=np.int32)
        kcol = np.ascontiguousarray(kcol, dtype=np.int32)
        vals = _c128(vals)
        RT, KS = kcol.shape
        if vals.shape != (RT, KS, 64) or tmap.shape != (RT,):
            raise EngineError("even-odd operator arrays have inconsistent shapes")
        self._chk(self._lib.sw_set_eo_operator(self._h, hid, level, int(which), RT, KS, _ptr(tmap),
                                               _ptr(kcol), _ptr(vals)), "sw_set_eo_operator")

    def setup_eo_operators(self, hid, level, Lc):
        """S, F, G, Hb of block level `level` (Lc x Lc sites) built on the device from its operator."""
        self._chk(self._lib.sw_setup_eo_operators(self._h, hid, level, int(Lc)), "sw_setup_eo_operators")

    def apply_eo_operator(self, hid, level, which, X):
        X2, single = self._io(X, self._n(hid, level))
        Y = np.empty_like(X2)
        self._chk(self._lib.sw_apply_eo_operator(self._h, hid, level, int(which), X2.shape[0], _ptr(X2),
                                                 _ptr(Y)), "sw_apply_eo_operator")
        return Y[0] if single else Y

    def level_bsr(self, hid, level):
        """A (device-built) level operator in MFMA block-row form: (kcol[RT, KS], vals[RT, KS, 64])."""
        ks = C.c_int(0)
        self._chk(self._lib.sw_get_level_bsr(self._h, hid, level, C.byref(ks), None, None),
                  "sw_get_level_bsr")
        RT = self.level_sizes[hid][level] // 16
        kcol = np.empty((RT, ks.value), dtype=np.int32)
        vals = np.empty((RT, ks.value, 64), dtype=np.complex128)
        self._chk(self._lib.sw_get_level_bsr(self._h, hid, level, C.byref(ks), _ptr(kcol), _ptr(vals)),
                  "sw_get_level_bsr")
        return kcol, vals

    def set_gmres_smoother(self, hid, level, m, cycles):
        self._chk(self._lib.sw_set_gmres_smoother(self._h, hid, level, int(m), int(cycles)),
                  "sw_set_gmres_smoother")

    # -- GPU-side setup ---------------------------------------------------------------------
    def setup_testvectors(self, hid, level, nvec, seed, sweeps, tol, maxiter, precond):
        its = np.zeros(max(1, sweeps), dtype=np.int32)
        self._chk(self._lib.sw_setup_testvectors(self._h, hid, level, nvec, int(seed), sweeps,
                                                 float(tol), int(maxiter), 1 if precond else 0,
                                                 _ptr(its)), "sw_setup_testvectors")
        return its[:sweeps].tolist()

    def setup_transfer(self, hid, level, blk_rows, G, pcols, pmap, porder=None):
        blk_rows = np.ascontiguousarray(blk_rows, dtype=np.int32)
        pcols = np.ascontiguousarray(pcols, dtype=np.int32)
        pmap = np.ascontiguousarray(pmap, dtype=np.int64)
        nblocks, rpb = blk_rows.shape
        K = pcols.shape[1]
        if porder is not None:
            porder = np.ascontiguousarray(porder, dtype=np.int32)
        self._chk(self._lib.sw_setup_transfer(self._h, hid, level, nblocks, rpb, _ptr(blk_rows), G, K,
                                              _ptr(pcols), _ptr(pmap),
                                              _ptr(porder) if porder is not None else None),
                  "sw_setup_transfer")
        self.level_sizes[hid][level] = nblocks * rpb
        self.level_sizes[hid][level + 1] = nblocks * 8

    def setup_galerkin(self, hid, level, Lc, nbr):
        nbr = np.ascontiguousarray(nbr, dtype=np.int32)
        self._chk(self._lib.sw_setup_galerkin(self._h, hid, level, int(Lc), _ptr(nbr)),
                  "sw_setup_galerkin")

    def setup_invert_coarsest(self, hid):
        self._chk(self._lib.sw_setup_invert_coarsest(self._h, hid), "sw_setup_invert_coarsest")
        self.level_sizes[hid][-1] = self.level_sizes[hid][-1]

    def get_coarsest_inv(self, hid, n):
        """The dense coarsest inverse the engine holds, as an (n, n) complex128 array."""
        out = np.empty((n, n), dtype=np.complex128)
        self._chk(self._lib.sw_get_coarsest_inv(self._h, hid, _ptr(out)), "sw_get_coarsest_inv")
        return out

    def setup_direct_level(self, hid, level):
        """Dense inverse of block level `level`'s even-odd Schur complement, formed on the device and
        installed as the level's even-odd operator 4 (the level is then solved exactly)."""
        self._chk(self._lib.sw_setup_direct_level(self._h, hid, level), "sw_setup_direct_level")

    def setup_level_inverse(self, hid, level):
        """Dense inverse of a small level's operator (n <= 8192), formed on the device; solves that start
        at this level are then two applications of it around one residual instead of an iteration."""
        self._chk(self._lib.sw_setup_level_inverse(self._h, hid, level), "sw_setup_level_inverse")

    def setup_arnoldi(self, hid, level, which, degree, seed=2024):
        """(degree+1) x degree Hessenberg matrix of `degree` Arnoldi steps of the level operator
        (which = 0) or its even-odd Schur complement (which = 1), computed on the device."""
        Hm = np.zeros((degree + 1, degree), dtype=np.complex128)
        self._chk(self._lib.sw_setup_arnoldi(self._h, hid, level, int(which), int(degree), int(seed),
                                             _ptr(Hm)), "sw_setup_arnoldi")
        return Hm

    def level_dense(self, hid, level):
        n = self.level_sizes[hid][level]
        M = np.empty((n, n), dtype=np.complex128)
        self._chk(self._lib.sw_get_level_dense(self._h, hid, level, _ptr(M)), "sw_get_level_dense")
        return M

    def hier_end(self, hid):
        self._chk(self._lib.sw_hier_end(self._h, hid), "sw_hier_end")

    def set_deflation(self, U):
        if U is None:
            self._chk(self._lib.sw_set_deflation(self._h, 0, None), "sw_set_deflation")
            return
        U = _c128(np.asarray(U))
        self._chk(self._lib.sw_set_deflation(self._h, U.shape[1], _ptr(U)), "sw_set_deflation")

    def set_low_mode_inverse(self, G):
        """The low-mode inverse G (k, k) of the registered deflation vectors, A_L^-1 = U G U^H gamma_3 (None clears;
        every set_deflation drops it)."""
        if G is None:
            self._chk(self._lib.sw_set_low_mode_inverse(self._h, 0, None), "sw_set_low_mode_inverse")
            return
        G = _c128(np.asarray(G))
        if G.ndim != 2 or G.shape[0] != G.shape[1]:
            raise EngineError("low-mode inverse of shape %s, expected (k, k)" % (G.shape,))
        self._chk(self._lib.sw_set_low_mode_inverse(self._h, G.shape[0], _ptr(G)), "sw_set_low_mode_inverse")

    def meson_fields(self, p, k):
        """Meson fields of the k registered deflation vectors for the momentum p: Phi[c, d, t, m, m'] =
        sum_x e^{-2 pi i p x / L} conj(U[idx(c,x,t), m]) U[idx(d,x,t), m'], shape (2, 2, L, k, k)."""
        L = int(round((self._n(0, 0) // 2) ** 0.5))
        out = np.zeros((2, 2, L, int(k), int(k)), dtype=np.complex128)
        self._chk(self._lib.sw_meson_fields(self._h, int(p), _ptr(out)), "sw_meson_fields")
        return out

    def low_mode_two_point(self, p):
        """E_L[a, b, c, d, t, t0] of the momentum p from the registered vectors and low-mode inverse, contracted on the
        device: utils.low_mode_two_point(meson_fields(p, k)[None], G)[0] without the fields leaving the device, shape
        (2, 2, 2, 2, L, L)."""
        L = int(round((self._n(0, 0) // 2) ** 0.5))
        out = np.zeros((2, 2, 2, 2, L, L), dtype=np.complex128)
        self._chk(self._lib.sw_low_mode_two_point(self._h, int(p), _ptr(out)), "sw_low_mode_two_point")
        return out

    def apply_low_mode(self, X):
        """Y = U G U^H X with the registered vectors and low-mode inverse (the low-mode chain of MODE_TWO_POINT_LMA)."""
        X2, single = self._io(X, self._n(0, 0))
        Y = np.empty_like(X2)
        self._chk(self._lib.sw_apply_low_mode(self._h, X2.shape[0], _ptr(X2), _ptr(Y)), "sw_apply_low_mode")
        return Y[0] if single else Y

    def set_level_deflation(self, level, V):
        if V is None:
            self._chk(self._lib.sw_set_level_deflation(self._h, level, 0, None),
                      "sw_set_level_deflation")
            return
        V = _c128(np.asarray(V))
        self._chk(self._lib.sw_set_level_deflation(self._h, level, V.shape[1], _ptr(V)),
                  "sw_set_level_deflation")

    def set_perm(self, level, shift):
        self._chk(self._lib.sw_set_perm(self._h, level, int(shift)), "sw_set_perm")

    def set_shifts(self, shifts):
        """Register the flat-index shifts of MODE_HUTCHINSON_SHIFTS (multiples of 2L in [0, n), no
        duplicates, at most MAX_SHIFTS); None or an empty list clears the registration."""
        s = np.ascontiguousarray([] if shifts is None else shifts, dtype=np.int64).ravel()
        self._chk(self._lib.sw_set_shifts(self._h, s.size, _ptr(s) if s.size else None), "sw_set_shifts")
        self._nshifts = int(s.size)

    def set_loop_momenta(self, momenta):
        """Register the spatial momenta of MODE_HUTCHINSON_LOOPS (integers in [0, L), no duplicates, at most
        MAX_MOMENTA); None or an empty list clears the registration."""
        p = np.ascontiguousarray([] if momenta is None else momenta, dtype=np.int32).ravel()
        self._chk(self._lib.sw_set_loop_momenta(self._h, p.size, _ptr(p) if p.size else None),
                  "sw_set_loop_momenta")
        self._nmom = int(p.size)

    def set_rhsmap(self, level, Cmat):
        (n, m), indptr, indices, data = _csr_parts(Cmat)
        self._chk(self._lib.sw_set_rhsmap(self._h, level, n, _ptr(indptr), _ptr(indices),
                                          _ptr(data)), "sw_set_rhsmap")

    def set_solver(self, restart=24, solver_hid=0):
        self._chk(self._lib.sw_set_solver(self._h, restart, solver_hid), "sw_set_solver")

    def set_option(self, name, value):
        self._chk(self._lib.sw_set_option(self._h, name.encode(), float(value)), "sw_set_option")

    def get_option(self, name):
        """Current value of an engine switch (save before an A/B run, restore afterwards)."""
        v = C.c_double(0.0)
        self._chk(self._lib.sw_get_option(self._h, name.encode(), C.byref(v)), "sw_get_option")
        return float(v.value)

    # -- device eigensolver (block subspace iteration; driver: setup_gpu.device_eigenpairs) ------
    def eig_begin(self, hid, level, seed=11, width=64):
        """Block buffers of `width` vectors (a multiple of 64, at most 512) on (hid, level)."""
        if width == 64:
            self._chk(self._lib.sw_eig_begin(self._h, hid, level, int(seed)), "sw_eig_begin")
        else:
            self._chk(self._lib.sw_eig_begin_wide(self._h, hid, level, int(seed), int(width)),
                      "sw_eig_begin_wide")
        self._eig_n = self._n(hid, level)
        self._eig_w = int(width)

    def eig_load(self, dst, X):
        X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.complex128)
        self._chk(self._lib.sw_eig_load(self._h, dst, X.shape[0], _ptr(X)), "sw_eig_load")

    def eig_solve(self, src, dst, mode, tol, maxiter=1000):
        its = C.c_int32(0)
        self._chk(self._lib.sw_eig_solve(self._h, src, dst, mode, float(tol), int(maxiter), C.byref(its)),
                  "sw_eig_solve")
        return int(its.value)

    def eig_apply_diff(self, src, dst, skip, g3, tol, maxiter=1000):
        """buf_dst = (A_l^-1 - P A_c^-1 R) Gamma buf_src (Gamma = gamma_3 if g3, skip: the level-0 skip form);
        returns the fine solve's iteration count"""
        its = C.c_int32(0)
        self._chk(self._lib.sw_eig_apply_diff(self._h, src, dst, int(bool(skip)), int(bool(g3)), float(tol),
                                              int(maxiter), C.byref(its)), "sw_eig_apply_diff")
        return int(its.value)

    def eig_gram(self, a, b):
        w = self._eig_w
        out = np.empty((w, w), dtype=np.complex128)
        self._chk(self._lib.sw_eig_gram(self._h, a, b, _ptr(out)), "sw_eig_gram")
        return out

    def eig_rotate(self, src, Y, dst, sub=-1):
        """buf_dst = buf_src Y, or (sub >= 0) buf_dst = buf_sub - buf_src Y"""
        Y = np.ascontiguousarray(Y, dtype=np.complex128)
        w = self._eig_w
        if Y.shape != (w, w):
            raise EngineError("rotation matrix must be %d x %d" % (w, w))
        self._chk(self._lib.sw_eig_rotate(self._h, src, _ptr(Y), dst, sub), "sw_eig_rotate")

    def eig_fetch(self, src, k):
        out = np.empty((k, self._eig_n), dtype=np.complex128)
        self._chk(self._lib.sw_eig_fetch(self._h, src, k, _ptr(out)), "sw_eig_fetch")
        return out

    def eig_end(self):
        self._chk(self._lib.sw_eig_end(self._h), "sw_eig_end")

    # -- building blocks -------------------------------------------------------------------
    def _io(self, X, n_in):
        X = _c128(X)
        single = X.ndim == 1
        X2 = X.reshape(1, -1) if single else X
        if X2.shape[1] != n_in:
            raise EngineError("vector length %d, expected %d" % (X2.shape[1], n_in))
        return X2, single

    def _n(self, hid, level):
        return self.level_sizes[hid][level]

    def apply_dirac(self, hid, level, X):
        X2, single = self._io(X, self._n(hid, level))
        Y = np.empty_like(X2)
        self._chk(self._lib.sw_apply_dirac(self._h, hid, level, X2.shape[0], _ptr(X2), _ptr(Y)),
                  "sw_apply_dirac")
        return Y[0] if single else Y

    def restrict(self, hid, level, X):
        X2, single = self._io(X, self._n(hid, level))
        Y = np.empty((X2.shape[0], self._n(hid, level + 1)), dtype=np.complex128)
        self._chk(self._lib.sw_restrict(self._h, hid, level, X2.shape[0], _ptr(X2), _ptr(Y)),
                  "sw_restrict")
        return Y[0] if single else Y

    def prolong(self, hid, level, X):
        X2, single = self._io(X, self._n(hid, level + 1))
        Y = np.empty((X2.shape[0], self._n(hid, level)), dtype=np.complex128)
        self._chk(self._lib.sw_prolong(self._h, hid, level, X2.shape[0], _ptr(X2), _ptr(Y)),
                  "sw_prolong")
        return Y[0] if single else Y

    def coarsest(self, hid, X):
        X2, single = self._io(X, self.level_sizes[hid][-1])
        Y = np.empty_like(X2)
        self._chk(self._lib.sw_coarsest(self._h, hid, X2.shape[0], _ptr(X2), _ptr(Y)),
                  "sw_coarsest")
        return Y[0] if single else Y

    def apply_deflation(self, which, level, X):
        """The registered deflation projection: which = 0, Pperm^T (I - U U^H) X at level 0 (Hutchinson);
        which = 1, (I - V_l V_l^H) X at `level` (MLMC)."""
        X2, single = self._io(X, self._n(0, level))
        Y = np.empty_like(X2)
        self._chk(self._lib.sw_apply_deflation(self._h, int(which), int(level), X2.shape[0], _ptr(X2),
                                               _ptr(Y)), "sw_apply_deflation")
        return Y[0] if single else Y

    def vcycle(self, hid, level0, B):
        B2, single = self._io(B, self._n(hid, level0))
        X = np.empty_like(B2)
        self._chk(self._lib.sw_vcycle(self._h, hid, level0, B2.shape[0], _ptr(B2), _ptr(X)),
                  "sw_vcycle")
        return X[0] if single else X

    def apply_op32(self, hid, level, which, X, B=None, mode=0, w=0.0, in_place=False):
        """One operation of the complex64 cycle alone (sw_apply_op32; which = OP32_*): Y = op X (mode 0),
        B - op X (1) or X + w (B - op X) (3) in complex64 through the cycle's own launcher, widened to complex128;
        in_place: mode 1 with B = Y = X on the device.  Returns (Y, info) with info = (row tiles, k-steps, ELL
        group size G, ELL entries per row K) of the operator applied."""
        return self._apply_op(self._lib.sw_apply_op32, "sw_apply_op32", hid, level, which, X, B, mode, w, in_place)

    def apply_op64(self, hid, level, which, X, B=None, mode=0, w=0.0, in_place=False):
        """One operation of the fp64 cycle alone (sw_apply_op64): as apply_op32 without the casts, through the fp64
        cycle's launcher; OP32_A also on the lattice level (the Wilson stencil), no Schur / even-odd smoother codes."""
        return self._apply_op(self._lib.sw_apply_op64, "sw_apply_op64", hid, level, which, X, B, mode, w, in_place)

    def _apply_op(self, fn, name, hid, level, which, X, B, mode, w, in_place):
        if which in (OP32_R, OP32_P, OP32_P_EVEN, OP32_RE) and not 0 <= level < len(self.level_sizes[hid]) - 1:
            raise EngineError("%s: no transfer from level %d" % (name, level))
        n_in = self._n(hid, level + 1) if which in (OP32_P, OP32_P_EVEN) else self._n(hid, level)
        n_out = self._n(hid, level + 1) if which in (OP32_R, OP32_RE) else self._n(hid, level)
        X2, single = self._io(X, n_in)
        B2 = None
        if B is not None:
            B2, _ = self._io(B, n_out)
            if B2.shape[0] != X2.shape[0]:
                raise EngineError("X and B differ in the number of vectors")
        Y = np.empty((X2.shape[0], n_out), dtype=np.complex128)
        info = np.zeros(4, dtype=np.int32)
        w = complex(w)
        self._chk(fn(self._h, hid, level, int(which), int(mode), X2.shape[0], _ptr(X2),
                     _ptr(B2) if B2 is not None else None, w.real, w.imag, OP32_INPLACE if in_place else 0, _ptr(Y),
                     _ptr(info)), name)
        return (Y[0] if single else Y), tuple(int(v) for v in info)

    # -- one operation of the Krylov solver alone (sw_krylov_*, test-only; no hierarchy needed) -----------------
    # vectors (nb, n) or stacks (K, nb, n), per-probe arrays (rows, nb); info = (row blocks P, rows per block,
    # 1 when the reduction was completed in the launch, groups of 32 row blocks)
    def krylov_multidot(self, V, W, svec=None, c64=False):
        """out[k] = V_k^H W through multidot (k_multidot<KT, complex128 or complex64>).  Returns (out[K, nb],
        coef[K, nb] = svec^2 out or None, largest |pad column entry| of out, info)."""
        V, W = _c128(V), _c128(W)
        K, nb, n = V.shape
        if W.shape != (nb, n):
            raise EngineError("W must be %d x %d" % (nb, n))
        nbp = (nb + 63) // 64 * 64
        out = np.empty((K, nbp), dtype=np.complex128)
        coef = sv = None
        if svec is not None:
            sv = np.ascontiguousarray(svec, dtype=np.float64)
            if sv.shape != (K, nb):
                raise EngineError("svec must be %d x %d" % (K, nb))
            coef = np.empty((K, nb), dtype=np.complex128)
        info = np.zeros(4, dtype=np.int32)
        self._chk(self._lib.sw_krylov_multidot(self._h, n, nb, K, KRYLOV_C64 if c64 else KRYLOV_C128, _ptr(V), _ptr(W),
                                               _ptr(sv) if sv is not None else None, _ptr(out),
                                               _ptr(coef) if coef is not None else None, _ptr(info)),
                  "sw_krylov_multidot")
        pad = out[:, nb:]
        # (a NaN in the pad columns -- an entry no kernel wrote -- must not pass for zero)
        pad_max = float(np.nan_to_num(np.abs(pad), nan=np.inf).max()) if pad.size else 0.0
        return np.ascontiguousarray(out[:, :nb]), coef, pad_max, tuple(int(v) for v in info)

    def krylov_gram(self, U):
        """All inner products of the NV vectors U[NV, nb, n] through multigram without a tail (k_gram<NV>):
        (gram[NV (NV + 1) / 2, nb], info)."""
        U = _c128(U)
        NV, nb, n = U.shape
        gram = np.empty((max(NV * (NV + 1) // 2, 1), nb), dtype=np.complex128)
        info = np.zeros(4, dtype=np.int32)
        self._chk(self._lib.sw_krylov_gram_cycle(self._h, n, nb, NV, KRYLOV_NOTAIL, _ptr(U), None, None, None, None,
                                                 0.0, 0.0, 0, _ptr(gram), None, None, None, None, _ptr(info)),
                  "sw_krylov_gram_cycle")
        return gram, tuple(int(v) for v in info)

    def krylov_gram_cycle(self, U, Z, X, normb, iters, tol, tol_stop, iter_base=0, init=False):
        """The BLAS-1 half of a Gram-matrix restart cycle (gram_cycle after its operator applications): multigram
        over U = [r0, w_0 .. w_{L-1}] with the Gram tail, then X += sum_j ys_j z_j.  Returns a dict: gram, ys,
        relres, g, normb, iters, notconv, X, info."""
        U, Z, X = _c128(U), _c128(Z), _c128(X).copy()
        NV, nb, n = U.shape
        L = NV - 1
        if Z.shape != (L, nb, n) or X.shape != (nb, n):
            raise EngineError("Z must be %d x %d x %d and X %d x %d" % (L, nb, n, nb, n))
        normb = np.array(normb, dtype=np.float64).reshape(nb).copy()
        iters = np.array(iters, dtype=np.int32).reshape(nb).copy()
        gram = np.empty((max(NV * (NV + 1) // 2, 1), nb), dtype=np.complex128)
        ys = np.empty((max(L, 1), nb), dtype=np.complex128)
        relres, g = np.empty(nb), np.empty(nb)
        notconv = C.c_int32(0)
        info = np.zeros(4, dtype=np.int32)
        self._chk(self._lib.sw_krylov_gram_cycle(self._h, n, nb, NV, KRYLOV_INIT if init else 0, _ptr(U), _ptr(Z),
                                                 _ptr(X), _ptr(normb), _ptr(iters), float(tol), float(tol_stop),
                                                 int(iter_base), _ptr(gram), _ptr(ys), _ptr(relres), _ptr(g),
                                                 C.byref(notconv), _ptr(info)), "sw_krylov_gram_cycle")
        return dict(gram=gram, ys=ys, relres=relres, g=g, normb=normb, iters=iters, notconv=int(notconv.value), X=X,
                    info=tuple(int(v) for v in info))

    def krylov_multiaxpy(self, V, coef, sign, W, v_c64=False, w_c64=False, norm=False, w32=False):
        """W + sign sum_k coef[k] V_k in place through multiaxpy (k_multiaxpy<KT, NORM, CV, CW>).  Returns (Wout,
        |Wout|^2 per column or None, the complex64 copy widened or None, info)."""
        V, W = _c128(V), _c128(W).copy()
        K, nb, n = V.shape
        coef = _c128(coef)
        if W.shape != (nb, n) or coef.shape != (K, nb):
            raise EngineError("W must be %d x %d and coef %d x %d" % (nb, n, K, nb))
        nrm = np.empty(nb) if norm else None
        W32 = np.empty_like(W) if w32 else None
        info = np.zeros(4, dtype=np.int32)
        self._chk(self._lib.sw_krylov_multiaxpy(self._h, n, nb, K, KRYLOV_C64 if v_c64 else KRYLOV_C128,
                                                KRYLOV_C64 if w_c64 else KRYLOV_C128,
                                                (KRYLOV_NORM if norm else 0) | (KRYLOV_W32 if w32 else 0), _ptr(V),
                                                _ptr(coef), float(sign), _ptr(W), _ptr(nrm) if norm else None,
                                                _ptr(W32) if w32 else None, _ptr(info)), "sw_krylov_multiaxpy")
        return W, nrm, W32, tuple(int(v) for v in info)

    def krylov_scalars(self, state, op, j=0, flag=0, tol=0.0, tol_stop=0.0, iter_base=0, h1=None, h2=None, nrm=None):
        """One FGMRES scalar update (op = KRYLOV_BEGIN / HESS / VERIFY through k_fg_tail, KRYLOV_SOLVE = k_fg_solve
        with k = j) on `state`, a dict of H[m + 1, m, nb], cs, sn, y, ys[m, nb], g, svec[m + 1, nb], normb,
        relres[nb] (complex or real) and iters[nb].  Returns (new state, notconv)."""
        m, nb = np.asarray(state["cs"]).shape
        parts = []
        for key, rows in KRYLOV_STATE:
            a = _c128(state[key]).reshape(-1, nb)
            if a.shape[0] != rows(m):
                raise EngineError("state[%r] must have %d rows" % (key, rows(m)))
            parts.append(a)
        packed = np.ascontiguousarray(np.concatenate(parts, axis=0))
        iters = np.array(state["iters"], dtype=np.int32).reshape(nb).copy()

        def small(a, rows, dtype):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.shape != (rows, nb):
                raise EngineError("a %d x %d array is needed" % (rows, nb))
            return a
        h1, h2 = small(h1, m + 2, np.complex128), small(h2, m + 2, np.complex128)
        nrm = small(None if nrm is None else np.asarray(nrm).reshape(1, nb), 1, np.float64)
        notconv = C.c_int32(0)
        self._chk(self._lib.sw_krylov_scalars(self._h, m, nb, int(op), int(j), int(flag), float(tol), float(tol_stop),
                                              int(iter_base), *[_ptr(a) if a is not None else None for a in (h1, h2, nrm)],
                                              _ptr(packed), _ptr(iters), C.byref(notconv)), "sw_krylov_scalars")
        new, r = {"iters": iters}, 0
        for key, rows in KRYLOV_STATE:
            new[key] = packed[r:r + rows(m)].reshape(np.asarray(state[key]).shape).copy()
            r += rows(m)
        return new, int(notconv.value)

    def solve(self, hid, level0, B, tol, maxiter=1000):
        B2, single = self._io(B, self._n(hid, level0))
        nb = B2.shape[0]
        X = np.empty_like(B2)
        iters = np.zeros(nb, dtype=np.int32)
        relres = np.zeros(nb, dtype=np.float64)
        self._chk(self._lib.sw_solve(self._h, hid, level0, nb, _ptr(B2), _ptr(X), float(tol),
                                     int(maxiter), _ptr(iters), _ptr(relres)), "sw_solve")
        if single:
            return X[0], int(iters[0]), float(relres[0])
        return X, iters, relres

    # -- probe batches ---------------------------------------------------------------------
    @staticmethod
    def _probes(probes):
        p = np.ascontiguousarray(probes, dtype=np.int8)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        return p

    def _probe_rows(self, what, shape, *args):
        """The resolved result of shape (..., nb) that the C entry `what` writes for `args`, the probe axis first."""
        out = np.zeros(shape, dtype=np.complex128)
        self._chk(getattr(self._lib, what)(self._h, *args, _ptr(out)), what)
        return np.ascontiguousarray(np.moveaxis(out, -1, 0))

    def _fetch_rows(self, what, shape):
        """_probe_rows for the sw_hutch_fetch_* entry `what`: shape(nb) with the probes of the last upload."""
        return self._probe_rows(what, shape(getattr(self, "_nb_uploaded", 0)))

    def hutch_batch(self, mode, level, probes, tol, maxiter=1000):
        p = self._probes(probes)
        nb = self._nb_uploaded = p.shape[0]
        ests = np.zeros(nb, dtype=np.complex128)
        iters = np.zeros(2 * nb, dtype=np.int32)
        self._chk(self._lib.sw_hutch_batch(self._h, mode, level, nb, _ptr(p), float(tol),
                                           int(maxiter), _ptr(ests), _ptr(iters)),
                  "sw_hutch_batch")
        return ests, iters[:nb].copy(), iters[nb:].copy()

    def hutch_batch_resolved(self, mode, level, probes, tol, maxiter=1000):
        """One batch of a mode of RESOLVED_FETCH: (its resolved result, iters_fine[nb], iters_coarse[nb])."""
        _, itf, itc = self.hutch_batch(mode, level, probes, tol, maxiter)
        return self.hutch_fetch_resolved(mode), itf, itc

    def hutch_fetch_resolved(self, mode):
        """The resolved result of the last batch of `mode`, one row per probe (a scalar mode has none: an error)."""
        if mode not in RESOLVED_FETCH:
            raise EngineError("mode %d leaves no resolved result" % mode)
        return getattr(self, RESOLVED_FETCH[mode])()

    def hutch_batch_shifts(self, level, probes, tol, maxiter=1000):
        """One MODE_HUTCHINSON_SHIFTS batch: (ests[nb, S], iters_fine[nb], iters_coarse[nb]) with one
        column per registered shift."""
        return self.hutch_batch_resolved(MODE_HUTCHINSON_SHIFTS, level, probes, tol, maxiter)

    def hutch_fetch_shifts(self):
        """Estimates of the last MODE_HUTCHINSON_SHIFTS batch at every registered shift, shape (nb, S)."""
        return self._fetch_rows("sw_hutch_fetch_shifts", lambda nb: (getattr(self, "_nshifts", 0), nb))

    def apply_shift_dots(self, probes, Z):
        """The shifted-dot kernel alone: out[k, j] = np.vdot(np.roll(x_k, -s_j), Z[k]) for the registered
        shifts; probes int8 (nb, n) codes, Z complex (nb, n), both in the reference ordering."""
        p = self._probes(probes)
        Z2, _ = self._io(Z, self._n(0, 0))
        if p.shape != Z2.shape:
            raise EngineError("probes %s and Z %s differ in shape" % (p.shape, Z2.shape))
        return self._probe_rows("sw_apply_shift_dots", (getattr(self, "_nshifts", 0), p.shape[0]), p.shape[0], _ptr(p),
                                _ptr(Z2))

    def _loop_shape(self, nb):
        n = self._n(0, 0)
        L = int(round((n // 2) ** 0.5))
        return (getattr(self, "_nmom", 0), 2, 2, L, nb)

    def hutch_batch_loops(self, level, probes, tol, maxiter=1000):
        """One MODE_HUTCHINSON_LOOPS batch: (loops[nb, nmom, 2, 2, L], iters_fine[nb], iters_coarse[nb]),
        loops[k, p, a, b, t] = sum_x e^{-2 pi i p x / L} conj(x_k[idx(a,x,t)]) z_k[idx(b,x,t)]."""
        return self.hutch_batch_resolved(MODE_HUTCHINSON_LOOPS, level, probes, tol, maxiter)

    def hutch_fetch_loops(self):
        """Loops of the last MODE_HUTCHINSON_LOOPS batch for every registered momentum, shape
        (nb, nmom, 2, 2, L)."""
        return self._fetch_rows("sw_hutch_fetch_loops", self._loop_shape)

    def apply_slice_dots(self, probes, Z):
        """The slice-dot kernel alone: out[k, p, a, b, t] = sum_x e^{-2 pi i p x / L} conj(x_k[idx(a,x,t)])
        Z[k][idx(b,x,t)] for the registered momenta; probes int8 (nb, n) codes, Z complex (nb, n), both in the
        reference ordering idx(s,x,y) = s L^2 + y L + x."""
        p = self._probes(probes)
        Z2, _ = self._io(Z, self._n(0, 0))
        if p.shape != Z2.shape:
            raise EngineError("probes %s and Z %s differ in shape" % (p.shape, Z2.shape))
        return self._probe_rows("sw_apply_slice_dots", self._loop_shape(p.shape[0]), p.shape[0], _ptr(p), _ptr(Z2))

    def hutch_batch_link_loops(self, level, probes, tol, maxiter=1000):
        """One MODE_HUTCHINSON_LINK_LOOPS batch: (link[nb, 4, nmom, 2, 2, L], iters_fine[nb], iters_coarse[nb]), the
        branches d = (F_x, B_x, F_t, B_t) of every probe:
        F_mu[k, p, a, b, t] = sum_x e^{-2 pi i p x / L} U_mu(n) conj(x_k[idx(a,n)]) z_k[idx(b,n+mu)],
        B_mu[k, p, a, b, t] = sum_x e^{-2 pi i p x / L} conj(U_mu(n)) conj(x_k[idx(a,n+mu)]) z_k[idx(b,n)], n = (x, t).
        hutch_fetch_loops() then returns the local loops of the same batch."""
        _, itf, itc = self.hutch_batch(MODE_HUTCHINSON_LINK_LOOPS, level, probes, tol, maxiter)
        return self.hutch_fetch_link_loops(), itf, itc

    def hutch_fetch_link_resolved(self):
        """Everything a MODE_HUTCHINSON_LINK_LOOPS batch resolves, shape (nb, 5, nmom, 2, 2, L): [:, 0] the local
        loops (hutch_fetch_loops), [:, 1:] the four link branches (hutch_fetch_link_loops)."""
        return np.concatenate([self.hutch_fetch_loops()[:, None], self.hutch_fetch_link_loops()], axis=1)

    def hutch_fetch_link_loops(self):
        """Link branches of the last MODE_HUTCHINSON_LINK_LOOPS batch, shape (nb, 4, nmom, 2, 2, L)."""
        return self._fetch_rows("sw_hutch_fetch_link_loops", lambda nb: (4,) + self._loop_shape(nb))

    def apply_slice_link_dots(self, probes, Z):
        """The link-dot kernel alone: out[k, d, p, a, b, t], the four branches of hutch_batch_link_loops with
        z_k = Z[k], for the registered momenta; probes int8 (nb, n) codes, Z complex (nb, n), both in the reference
        ordering idx(s,x,y) = s L^2 + y L + x."""
        p = self._probes(probes)
        Z2, _ = self._io(Z, self._n(0, 0))
        if p.shape != Z2.shape:
            raise EngineError("probes %s and Z %s differ in shape" % (p.shape, Z2.shape))
        return self._probe_rows("sw_apply_slice_link_dots", (4,) + self._loop_shape(p.shape[0]), p.shape[0], _ptr(p),
                                _ptr(Z2))

    def hutch_batch_mlmc_loops(self, level, probes, tol, maxiter=1000, skip=False, deflated=False):
        """One MODE_MLMC_LOOPS batch (skip: MODE_MLMC_LOOPS_SKIP) at `level`: (loops[nb, nmom, 2, 2, L], iters_fine[nb],
        iters_coarse[nb]), loops[k, p, a, b, t] = S_q(Pi_l x_k, Pi_l d_k) with d_k the MLMC difference of probe k.
        deflated: MODE_MLMC_DEFL_LOOPS / _SKIP, d_k the difference of x_k - V V^H x_k for the level's registered V."""
        # `skip` is the caller's word (the engine refuses it above level 0), so the mode is looked up at level 0
        return self.hutch_batch_resolved(probe_mode("mlmc_loops", 0, skip, deflated), level, probes, tol, maxiter)

    def hutch_fetch_mlmc_loops(self):
        """Level loops of the last MODE_MLMC_LOOPS / _SKIP batch, shape (nb, nmom, 2, 2, L)."""
        return self._fetch_rows("sw_hutch_fetch_mlmc_loops", self._loop_shape)

    def apply_slice_cdots(self, U, V):
        """k_slice_cdots alone: out[k, p, a, b, t] = sum_x e^{-2 pi i p x / L} conj(U[k][idx(a,x,t)]) V[k][idx(b,x,t)]
        for the registered momenta; U, V complex (nb, n) in the reference ordering."""
        U2, _ = self._io(U, self._n(0, 0))
        V2, _ = self._io(V, self._n(0, 0))
        if U2.shape != V2.shape:
            raise EngineError("U %s and V %s differ in shape" % (U2.shape, V2.shape))
        return self._probe_rows("sw_apply_slice_cdots", self._loop_shape(U2.shape[0]), U2.shape[0], _ptr(U2), _ptr(V2))

    def coarsest_loops(self):
        """The exact coarsest term of the MLMC loops, shape (nmom, 2, 2, L): sum_j S_q(Pi e_j, Pi A_c^-1 e_j)."""
        out = np.zeros(self._loop_shape(1)[:-1], dtype=np.complex128)
        self._chk(self._lib.sw_coarsest_loops(self._h, _ptr(out)), "sw_coarsest_loops")
        return out

    def level_deflation_loops(self, level, skip=False, tol=1e-12, maxiter=1000):
        """The deflated part of level `level`'s term of the MLMC loops, shape (nmom, 2, 2, L): sum_j S_q(Pi V_j,
        Pi D V_j) over the vectors registered with set_level_deflation, D applied on the device (solves to `tol`)."""
        out = np.zeros(self._loop_shape(1)[:-1], dtype=np.complex128)
        self._chk(self._lib.sw_level_deflation_loops(self._h, int(level), int(bool(skip)), float(tol), int(maxiter),
                                                     _ptr(out)), "sw_level_deflation_loops")
        return out

    def set_two_point(self, t0, momenta):
        """Source timeslice and momenta of MODE_TWO_POINT (None or an empty list clears)."""
        m = np.ascontiguousarray([] if momenta is None else momenta, dtype=np.int32)
        self._chk(self._lib.sw_set_two_point(self._h, int(t0), m.size, _ptr(m) if m.size else None),
                  "sw_set_two_point")
        self._tp_nmom = int(m.size)

    def _two_point_shape(self, nb):
        n = self._n(0, 0)
        L = int(round((n // 2) ** 0.5))
        return (getattr(self, "_tp_nmom", 0), 2, 2, 2, 2, L, nb)

    def hutch_batch_two_point(self, level, probes, tol, maxiter=1000):
        """One MODE_TWO_POINT batch, the probes being the noises: (T[nb, nmom, 2, 2, 2, 2, L], iters_fine[nb],
        iters_coarse[nb]); iters_fine[k] is the largest count among the 2 nmom solves of noise k."""
        return self.hutch_batch_resolved(MODE_TWO_POINT, level, probes, tol, maxiter)

    def hutch_fetch_two_point(self):
        """Pair sums of the last MODE_TWO_POINT batch, shape (nb, nmom, 2, 2, 2, 2, L): T[k, j, a, b, c, d, t]."""
        return self._fetch_rows("sw_hutch_fetch_two_point", self._two_point_shape)

    def hutch_fetch_two_point_lma(self):
        """Remainders of the last MODE_TWO_POINT_LMA batch, shape (nb, nmom, 2, 2, 2, 2, L): R[k, j, a, b, c, d, t] =
        T(z, z) - T(z_L, z_L)."""
        return self._fetch_rows("sw_hutch_fetch_two_point_lma", self._two_point_shape)

    def apply_slice_sources(self, probes):
        """The source kernel alone: out[2 j + a, k, :] = the source of momentum j, spin a and noise k of the
        registration, reference ordering; probes int8 (nb, n) codes."""
        p = self._probes(probes)
        if p.shape[1] != self._n(0, 0):
            raise EngineError("probes of length %d, expected %d" % (p.shape[1], self._n(0, 0)))
        out = np.zeros((2 * getattr(self, "_tp_nmom", 0),) + p.shape, dtype=np.complex128)
        self._chk(self._lib.sw_apply_slice_sources(self._h, p.shape[0], _ptr(p), _ptr(out)),
                  "sw_apply_slice_sources")
        return out

    def apply_pair_dots(self, Z):
        """The pair-dot kernels alone: Z complex (2 nmom, nb, n) in the layout of apply_slice_sources; returns
        T[k, j, a, b, c, d, t]."""
        Z = _c128(Z)
        if Z.ndim != 3 or Z.shape[0] != 2 * getattr(self, "_tp_nmom", 0) or Z.shape[2] != self._n(0, 0):
            raise EngineError("Z of shape %s, expected (%d, nb, %d)"
                              % (Z.shape, 2 * getattr(self, "_tp_nmom", 0), self._n(0, 0)))
        return self._probe_rows("sw_apply_pair_dots", self._two_point_shape(Z.shape[1]), Z.shape[1], _ptr(Z))

    def set_smearing(self, kappa, source_steps=0, sink_steps=(0,)):
        """kappa, the source steps and the ascending sink levels of MODE_TWO_POINT_SMEARED (sink_steps None or an
        empty list clears)."""
        s = np.ascontiguousarray([] if sink_steps is None else sink_steps, dtype=np.int32)
        self._chk(self._lib.sw_set_smearing(self._h, float(kappa), int(source_steps), s.size,
                                            _ptr(s) if s.size else None), "sw_set_smearing")
        self._sm_nsink = int(s.size)

    def apply_smearing(self, X, steps, fused=False):
        """The smearing kernels alone: S_steps X with the registered kappa on X complex (nb, n) or (n,), reference
        ordering, every timeslice (utils.smear); fused: one launch of k_smear_fused instead of `steps` of
        k_smear_step -- the same bits."""
        X2, single = self._io(X, self._n(0, 0))
        Y = np.empty_like(X2)
        self._chk(self._lib.sw_apply_smearing(self._h, X2.shape[0], int(steps), int(bool(fused)), _ptr(X2), _ptr(Y)),
                  "sw_apply_smearing")
        return Y[0] if single else Y

    def set_distillation(self, V):
        """The Laplacian eigenvectors of perambulators(): V complex (L, nev, L) = v_m(x, t) at [t, m, x] (None or an
        empty array clears).  Orthonormality is not checked: V defines the operator."""
        if V is None or np.size(V) == 0:
            self._chk(self._lib.sw_set_distillation(self._h, 0, None), "sw_set_distillation")
            self._lh_nev = self._lh_nmom = 0
            return
        V = _c128(V)
        if V.ndim != 3 or V.shape[0] != V.shape[2]:
            raise EngineError("set_distillation: V of shape %s, expected (L, nev, L)" % (V.shape,))
        self._lh_nmom = 0              # every registration drops the momenta of set_distillation_momenta
        self._chk(self._lib.sw_set_distillation(self._h, V.shape[1], _ptr(V)), "sw_set_distillation")
        self._lh_nev = int(V.shape[1])

    def _t0s(self, t0s):
        return np.ascontiguousarray(np.atleast_1d(t0s), dtype=np.int32).reshape(-1)

    def perambulators(self, t0s, tol, maxiter=1000):
        """(tau[nsrc, L, 2, nev, nev, 2], iters[nsrc, nev, 2]): tau[s, t, c, m, n, a] = sum_x conj(v_m(x, t))
        z^(s,n,a)[idx(c, x, t)] for the solutions of the eigenvector sources on the timeslices t0s
        (utils.perambulators_from_solutions of utils.laph_sources).  Stateless: no mode buffer is touched."""
        t = self._t0s(t0s)
        nev = getattr(self, "_lh_nev", 0)
        L = int(round((self._n(0, 0) // 2) ** 0.5))
        out = np.zeros((t.size, L, 2, nev, nev, 2), dtype=np.complex128)
        iters = np.zeros((t.size, nev, 2), dtype=np.int32)
        self._chk(self._lib.sw_perambulators(self._h, t.size, _ptr(t) if t.size else None, float(tol), int(maxiter),
                                             _ptr(out) if out.size else None, _ptr(iters) if iters.size else None),
                  "sw_perambulators")
        return out, iters

    def apply_laph_sources(self, t0s):
        """k_laph_sources alone: the sources of perambulators(), shape (nsrc nev 2, n), reference ordering."""
        t = self._t0s(t0s)
        out = np.zeros((t.size * getattr(self, "_lh_nev", 0) * 2, self._n(0, 0)), dtype=np.complex128)
        self._chk(self._lib.sw_apply_laph_sources(self._h, t.size, _ptr(t) if t.size else None,
                                                  _ptr(out) if out.size else None), "sw_apply_laph_sources")
        return out

    def apply_laph_project(self, Z):
        """k_laph_project alone on Z complex (nb, n), reference ordering: out[t, c, m, k] = sum_x conj(v_m(x, t))
        Z[k, idx(c, x, t)], shape (L, 2, nev, nb)."""
        Z2, _ = self._io(Z, self._n(0, 0))
        L = int(round((self._n(0, 0) // 2) ** 0.5))
        out = np.zeros((L, 2, getattr(self, "_lh_nev", 0), Z2.shape[0]), dtype=np.complex128)
        self._chk(self._lib.sw_apply_laph_project(self._h, Z2.shape[0], _ptr(Z2), _ptr(out) if out.size else None),
                  "sw_apply_laph_project")
        return out

    def set_distillation_momenta(self, momenta):
        """The momenta of distilled_two_point(): at most MAX_MOMENTA different integers in [0, L) (None or an empty list
        clears).  Needs set_distillation; the elementals are computed on the device here and stay there until the next
        set_distillation."""
        p = np.ascontiguousarray([] if momenta is None else momenta, dtype=np.int32).reshape(-1)
        self._chk(self._lib.sw_set_distillation_momenta(self._h, p.size, _ptr(p) if p.size else None),
                  "sw_set_distillation_momenta")
        self._lh_nmom = int(p.size)

    def _laph_shape(self):
        return int(round((self._n(0, 0) // 2) ** 0.5)), getattr(self, "_lh_nev", 0), getattr(self, "_lh_nmom", 0)

    def laph_elementals(self):
        """M[nmom, L, nev, nev] = sum_x e^{-2 pi i p_j x / L} conj(v_m(x, t)) v_m'(x, t): the registered elementals as
        the device computed them (utils.laph_elementals)."""
        L, nev, nmom = self._laph_shape()
        out = np.zeros((nmom, L, nev, nev), dtype=np.complex128)
        self._chk(self._lib.sw_apply_laph_elementals(self._h, _ptr(out) if out.size else None),
                  "sw_apply_laph_elementals")
        return out

    def distilled_two_point(self, t0s, tol, maxiter=1000, keep=True):
        """(T[nsrc, nmom, 2, 2, 2, 2, L], loops[nsrc, nmom, 2, 2], tau or None, iters[nsrc, nev, 2]): the perambulators
        of the timeslices t0s solved, projected and contracted on the device (utils.distilled_pair_sums and the
        source-timeslice entries of utils.distilled_loops); tau as perambulators() returns it when keep is set,
        otherwise nothing of its size leaves the device.  Stateless: no mode buffer is touched."""
        t = self._t0s(t0s)
        L, nev, nmom = self._laph_shape()
        T = np.zeros((t.size, nmom, 2, 2, 2, 2, L), dtype=np.complex128)
        loops = np.zeros((t.size, nmom, 2, 2), dtype=np.complex128)
        tau = np.zeros((t.size, L, 2, nev, nev, 2), dtype=np.complex128) if keep else None
        iters = np.zeros((t.size, nev, 2), dtype=np.int32)
        self._chk(self._lib.sw_distilled_two_point(self._h, t.size, _ptr(t) if t.size else None, float(tol),
                                                   int(maxiter), _ptr(T) if T.size else None,
                                                   _ptr(loops) if loops.size else None,
                                                   _ptr(tau) if keep and tau.size else None,
                                                   _ptr(iters) if iters.size else None), "sw_distilled_two_point")
        return T, loops, tau, iters

    def apply_laph_contract(self, tau, t0s):
        """The contraction kernels alone on perambulators tau[nsrc, L, 2, nev, nev, 2]: (T, loops) as
        distilled_two_point() returns them."""
        t = self._t0s(t0s)
        L, nev, nmom = self._laph_shape()
        tau = _c128(tau)
        if tau.shape != (t.size, L, 2, nev, nev, 2):
            raise EngineError("apply_laph_contract: tau of shape %s, expected %s"
                              % (tau.shape, (t.size, L, 2, nev, nev, 2)))
        T = np.zeros((t.size, nmom, 2, 2, 2, 2, L), dtype=np.complex128)
        loops = np.zeros((t.size, nmom, 2, 2), dtype=np.complex128)
        self._chk(self._lib.sw_apply_laph_contract(self._h, t.size, _ptr(t) if t.size else None,
                                                   _ptr(tau) if tau.size else None, _ptr(T) if T.size else None,
                                                   _ptr(loops) if loops.size else None), "sw_apply_laph_contract")
        return T, loops

    @staticmethod
    def _meson_ops(ops, what):
        """(spin complex128[n, 2, 2], mom int32[n]) from a list of (2 x 2 matrix, momentum index) pairs."""
        ops = list(ops)
        spin = np.zeros((len(ops), 2, 2), dtype=np.complex128)
        mom = np.zeros(len(ops), dtype=np.int32)
        for k, op in enumerate(ops):
            g = np.asarray(op[0], dtype=np.complex128)
            if g.shape != (2, 2):
                raise EngineError("%s operator %d: spin matrix of shape %s, expected (2, 2)" % (what, k, g.shape))
            spin[k], mom[k] = g, int(op[1])
        return spin, mom

    def distilled_two_meson(self, t0s, sink_ops, source_ops, tol, maxiter=1000):
        """(C1[nsrc, nk, nkp, L], C2[nsrc, nk, nk, nkp, nkp, L], iters[nsrc, nev, 2]): the perambulators of the
        timeslices t0s solved, projected and contracted into the two-meson building blocks on the device
        (utils.two_meson_sums).  sink_ops: 1 to MAX_MESON_OPS pairs (G, j) of the folded 2 x 2 matrix G = g3 Gamma and
        the index j into the momenta of set_distillation_momenta; source_ops: pairs (H, j), H = Gamma' g3
        (utils.two_meson_folded makes both).  Stateless: no mode buffer is touched."""
        t = self._t0s(t0s)
        L, nev, _ = self._laph_shape()
        G, jk = self._meson_ops(sink_ops, "sink")
        H, jkp = self._meson_ops(source_ops, "source")
        nk, nkp = jk.size, jkp.size
        C1 = np.zeros((t.size, nk, nkp, L), dtype=np.complex128)
        C2 = np.zeros((t.size, nk, nk, nkp, nkp, L), dtype=np.complex128)
        iters = np.zeros((t.size, nev, 2), dtype=np.int32)
        self._chk(self._lib.sw_distilled_two_meson(
            self._h, t.size, _ptr(t) if t.size else None, nk, _ptr(G) if nk else None, _ptr(jk) if nk else None,
            nkp, _ptr(H) if nkp else None, _ptr(jkp) if nkp else None, float(tol), int(maxiter),
            _ptr(C1) if C1.size else None, _ptr(C2) if C2.size else None, _ptr(iters) if iters.size else None),
            "sw_distilled_two_meson")
        return C1, C2, iters

    def apply_laph_two_meson(self, tau, t0s, sink_ops, source_ops, want_Q=False):
        """The two-meson kernels alone on perambulators tau[nsrc, L, 2, nev, nev, 2]: (C1, C2) as
        distilled_two_meson() returns them and, with want_Q, the sandwich Q[nsrc, nk, L, 2 nev, 2 nev] (else None)."""
        t = self._t0s(t0s)
        L, nev, _ = self._laph_shape()
        tau = _c128(tau)
        if tau.shape != (t.size, L, 2, nev, nev, 2):
            raise EngineError("apply_laph_two_meson: tau of shape %s, expected %s"
                              % (tau.shape, (t.size, L, 2, nev, nev, 2)))
        G, jk = self._meson_ops(sink_ops, "sink")
        H, jkp = self._meson_ops(source_ops, "source")
        nk, nkp = jk.size, jkp.size
        C1 = np.zeros((t.size, nk, nkp, L), dtype=np.complex128)
        C2 = np.zeros((t.size, nk, nk, nkp, nkp, L), dtype=np.complex128)
        Q = np.zeros((t.size, nk, L, 2 * nev, 2 * nev), dtype=np.complex128) if want_Q else None
        self._chk(self._lib.sw_apply_laph_two_meson(
            self._h, t.size, _ptr(t) if t.size else None, _ptr(tau) if tau.size else None, nk,
            _ptr(G) if nk else None, _ptr(jk) if nk else None, nkp, _ptr(H) if nkp else None,
            _ptr(jkp) if nkp else None, _ptr(C1) if C1.size else None, _ptr(C2) if C2.size else None,
            _ptr(Q) if want_Q and Q.size else None), "sw_apply_laph_two_meson")
        return C1, C2, Q

    def _insertions(self, timeslices, momenta):
        return (np.ascontiguousarray(np.atleast_1d(timeslices), dtype=np.int32).reshape(-1),
                np.ascontiguousarray(np.atleast_1d(momenta), dtype=np.int32).reshape(-1))

    def generalized_perambulators(self, t0, tf, timeslices, momenta, tol, maxiter=1000, keep_tau=True):
        """(G[nt, nmom, 6, 2 nev, 2 nev], tau[2, L, 2, nev, nev, 2] or None, iters[2, nev, 2]): the generalized
        perambulators between the eigenvector solutions of the sink timeslice tf (rows (m, e) -> 2 m + e) and of the
        source timeslice t0 (columns (n, b) -> 2 n + b) at the insertion timeslices and momenta
        (utils.generalized_perambulators_from_solutions: components 2 f + c local, 4 = J_x, 5 = J_t), and, with
        keep_tau, the perambulators of perambulators([t0, tf]), bit for bit.  Stateless: no mode buffer is touched."""
        t, q = self._insertions(timeslices, momenta)
        L, nev, _ = self._laph_shape()
        G = np.zeros((t.size, q.size, 6, 2 * nev, 2 * nev), dtype=np.complex128)
        tau = np.zeros((2, L, 2, nev, nev, 2), dtype=np.complex128) if keep_tau else None
        iters = np.zeros((2, nev, 2), dtype=np.int32)
        self._chk(self._lib.sw_generalized_perambulators(
            self._h, int(t0), int(tf), t.size, _ptr(t) if t.size else None, q.size, _ptr(q) if q.size else None,
            float(tol), int(maxiter), _ptr(G) if G.size else None, _ptr(tau) if keep_tau and tau.size else None,
            _ptr(iters) if iters.size else None), "sw_generalized_perambulators")
        return G, tau, iters

    def apply_laph_generalized(self, Zf, Z0, timeslices, momenta):
        """k_laph_generalized alone on Zf complex (nbf, n) and Z0 complex (nb0, n), reference ordering, in place of
        the solutions: out[i, j, k, r, s], shape (nt, nmom, 6, nbf, nb0)
        (utils.generalized_perambulators_from_solutions with the links of the lattice level)."""
        Zf2, _ = self._io(Zf, self._n(0, 0))
        Z02, _ = self._io(Z0, self._n(0, 0))
        t, q = self._insertions(timeslices, momenta)
        out = np.zeros((t.size, q.size, 6, Zf2.shape[0], Z02.shape[0]), dtype=np.complex128)
        self._chk(self._lib.sw_apply_laph_generalized(
            self._h, Zf2.shape[0], _ptr(Zf2), Z02.shape[0], _ptr(Z02), t.size, _ptr(t) if t.size else None, q.size,
            _ptr(q) if q.size else None, _ptr(out) if out.size else None), "sw_apply_laph_generalized")
        return out

    def hutch_batch_two_point_smeared(self, level, probes, tol, maxiter=1000):
        """One MODE_TWO_POINT_SMEARED batch: (T[nb, nsink, nmom, 2, 2, 2, 2, L], iters_fine[nb], iters_coarse[nb])."""
        return self.hutch_batch_resolved(MODE_TWO_POINT_SMEARED, level, probes, tol, maxiter)

    def hutch_fetch_two_point_smeared(self):
        """Pair sums of the last MODE_TWO_POINT_SMEARED batch at every sink level, shape (nb, nsink, nmom, 2, 2, 2,
        2, L)."""
        return self._fetch_rows("sw_hutch_fetch_two_point_smeared",
                                lambda nb: (getattr(self, "_sm_nsink", 0),) + self._two_point_shape(nb))

    def set_three_point(self, t0, tf, sink='g3', pf=0, momenta=(0,)):
        """Source and sink timeslice, sink spin matrix ('1', 'g3', 's1', 's2' or its code 0..3), sink momentum and
        insertion momenta of MODE_THREE_POINT (momenta None or an empty list clears)."""
        m = np.ascontiguousarray([] if momenta is None else momenta, dtype=np.int32)
        code = SINK_GAMMAS.index(sink) if sink in SINK_GAMMAS else sink
        if isinstance(code, str):
            raise EngineError("unknown sink spin matrix %r (one of %s)" % (sink, list(SINK_GAMMAS)))
        self._chk(self._lib.sw_set_three_point(self._h, int(t0), int(tf), int(code), int(pf), m.size,
                                               _ptr(m) if m.size else None), "sw_set_three_point")
        self._t3_nmom = int(m.size)

    def _three_point_shape(self, nb):
        n = self._n(0, 0)
        L = int(round((n // 2) ** 0.5))
        return (5, getattr(self, "_t3_nmom", 0), 2, 2, 2, 2, L, nb)

    def hutch_batch_three_point(self, level, probes, tol, maxiter=1000):
        """One MODE_THREE_POINT batch, the probes being the noises: (S[nb, 5, nmom, 2, 2, 2, 2, L], c[nb],
        iters_fine[nb], iters_coarse[nb]); S[k, d, j, a, b, f, c, t] over the branches d = (local, F_x, B_x, F_t, B_t),
        c[k] = sum_{a,c,x} |z_k^a[idx(c,x,tf)]|^2, iters_fine[k] the largest stage-1 plus the largest stage-2 count."""
        c, itf, itc = self.hutch_batch(MODE_THREE_POINT, level, probes, tol, maxiter)
        return self.hutch_fetch_three_point(), c, itf, itc

    def hutch_fetch_three_point(self):
        """Sums of the last MODE_THREE_POINT batch, shape (nb, 5, nmom, 2, 2, 2, 2, L)."""
        return self._fetch_rows("sw_hutch_fetch_three_point", self._three_point_shape)

    def hutch_fetch_three_point_resolved(self):
        """Everything a MODE_THREE_POINT batch resolves, one row per noise: the flattened S followed by c_k."""
        S = self.hutch_fetch_three_point()
        c, _, _ = self.hutch_fetch()
        return np.concatenate([S.reshape(S.shape[0], -1), c[:, None]], axis=1)

    def _pair_fields(self, Z, what):
        Z = _c128(Z)
        if Z.ndim != 3 or Z.shape[0] != 2 or Z.shape[2] != self._n(0, 0):
            raise EngineError("%s of shape %s, expected (2, nb, %d)" % (what, Z.shape, self._n(0, 0)))
        return Z

    def apply_seq_sources(self, Z):
        """The sequential-source kernel alone: Z complex (2, nb, n) = z_k^a in the reference ordering; returns s of
        the same shape for the registration of set_three_point (utils.seq_sources)."""
        Z = self._pair_fields(Z, "Z")
        out = np.zeros_like(Z)
        self._chk(self._lib.sw_apply_seq_sources(self._h, Z.shape[1], _ptr(Z), _ptr(out)), "sw_apply_seq_sources")
        return out

    def apply_seq_dots(self, Zeta, Z):
        """The field x field reduction alone: Zeta, Z complex (2, nb, n); returns S[k, d, j, a, b, f, c, t]
        (utils.seq_dots with the links of the lattice level)."""
        Zeta, Z = self._pair_fields(Zeta, "Zeta"), self._pair_fields(Z, "Z")
        if Zeta.shape != Z.shape:
            raise EngineError("Zeta %s and Z %s differ in shape" % (Zeta.shape, Z.shape))
        return self._probe_rows("sw_apply_seq_dots", self._three_point_shape(Z.shape[1]), Z.shape[1], _ptr(Zeta),
                                _ptr(Z))

    def probes_upload(self, level, probes):
        p = self._probes(probes)
        self._nb_uploaded = p.shape[0]
        self._chk(self._lib.sw_probes_upload(self._h, level, p.shape[0], _ptr(p)),
                  "sw_probes_upload")

    def probes_upload_slot(self, slot, level, probes):
        p = self._probes(probes)
        self._chk(self._lib.sw_probes_upload_slot(self._h, slot, level, p.shape[0], _ptr(p)),
                  "sw_probes_upload_slot")
        self._slot_nb = getattr(self, "_slot_nb", {})
        self._slot_nb[slot] = p.shape[0]

    def probes_select(self, slot):
        self._chk(self._lib.sw_probes_select(self._h, slot), "sw_probes_select")
        self._nb_uploaded = self._slot_nb[slot]

    def stream_set(self, window):
        """Hand the engine a window of the MT19937 probe stream (ProbeStream.window()); it
        becomes stream position 0 of probes_generate()."""
        w = np.ascontiguousarray(window, dtype=np.uint32)
        if w.size != 624:
            raise EngineError("an MT19937 window has 624 words")
        self._chk(self._lib.sw_probes_stream_set(self._h, _ptr(w)), "sw_probes_stream_set")

    def probes_generate(self, slot, level, nb, pos, kind="z2"):
        """Fill `slot` on the device with the nb probes that start at draw `pos` of the stream."""
        self._chk(self._lib.sw_probes_generate(self._h, int(slot), int(level), int(nb),
                                               PROBE_KINDS[kind], int(pos)), "sw_probes_generate")
        self._slot_nb = getattr(self, "_slot_nb", {})
        self._slot_nb[slot] = int(nb)
        self._slot_n = getattr(self, "_slot_n", {})
        self._slot_n[slot] = self.level_sizes[0][level]

    def probes_fetch(self, slot):
        """int8 codes held in `slot`, shape (nb, n) (tests; the estimators never need them)."""
        nb = self._slot_nb[slot]
        n = getattr(self, "_slot_n", {}).get(slot)
        if n is None:
            raise EngineError("slot %d was not generated on the device" % slot)
        out = np.empty((nb, n), dtype=np.int8)
        self._chk(self._lib.sw_probes_fetch(self._h, int(slot), _ptr(out)), "sw_probes_fetch")
        return out

    def kernel_stats(self, which):
        ms = C.c_double(0.0)
        cnt = C.c_int64(0)
        self._chk(self._lib.sw_kernel_stats(self._h, which, C.byref(ms), C.byref(cnt)),
                  "sw_kernel_stats")
        return ms.value, int(cnt.value)

    def kernel_work(self, which):
        w = C.c_double(0.0)
        self._chk(self._lib.sw_kernel_work(self._h, which, C.byref(w)), "sw_kernel_work")
        return w.value

    def hutch_run(self, mode, level, tol, maxiter=1000):
        self._chk(self._lib.sw_hutch_run(self._h, mode, level, float(tol), int(maxiter)),
                  "sw_hutch_run")

    def sync(self):
        self._chk(self._lib.sw_sync(self._h), "sw_sync")

    def hutch_fetch(self):
        nb = self._nb_uploaded
        ests = np.zeros(nb, dtype=np.complex128)
        iters = np.zeros(2 * nb, dtype=np.int32)
        self._chk(self._lib.sw_hutch_fetch(self._h, _ptr(ests), _ptr(iters)), "sw_hutch_fetch")
        return ests, iters[:nb].copy(), iters[nb:].copy()

    # -- the collective behind the C ABI (RCCL) -----------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        if load_library().sw_comm_unique_id(buf) != 0:
            raise EngineError("sw_comm_unique_id failed (RCCL not loadable)")
        return buf.raw

    def comm_init(self, nranks, rank, uid):
        buf = C.create_string_buffer(bytes(uid), 128)
        self._chk(self._lib.sw_comm_init(self._h, int(nranks), int(rank), buf), "sw_comm_init")

    def allreduce_stats(self, stats):
        a = np.ascontiguousarray(stats, dtype=np.float64).copy()
        if a.size != 4:
            raise EngineError("four statistics expected")
        self._chk(self._lib.sw_allreduce_stats(self._h, _ptr(a)), "sw_allreduce_stats")
        return a

    def comm_destroy(self):
        self._chk(self._lib.sw_comm_destroy(self._h), "sw_comm_destroy")

    # -- measurement -----------------------------------------------------------------------
    def bench_dirac(self, hid, level, nb, reps):
        ms = C.c_double(0.0)
        self._chk(self._lib.sw_bench_dirac(self._h, hid, level, nb, reps, C.byref(ms)),
                  "sw_bench_dirac")
        return ms.value

    def set_profiling(self, on):
        self._chk(self._lib.sw_set_profiling(self._h, 1 if on else 0), "sw_set_profiling")

    def timers(self):
        t = (C.c_double * 8)()
        self._chk(self._lib.sw_timers(self._h, t), "sw_timers")
        return dict(zip(TIMER_NAMES, [float(v) for v in t]))

    def timers_reset(self):
        self._chk(self._lib.sw_timers_reset(self._h), "sw_timers_reset")

    def launch_count(self):
        n = C.c_int64(0)
        self._chk(self._lib.sw_launch_count(self._h, C.byref(n)), "sw_launch_count")
        return int(n.value)


class ProbeStream:
    """The reference's probe stream (utils.py:213-216) without NumPy's global state: MT19937
    seeded as ``np.random.seed(seed)``; host-only, needs no GPU.  ``jump`` moves any distance in
    O(1) state refills (GF(2) jump polynomial), ``skip`` walks there (the checker)."""

    def __init__(self, seed=None, _handle=None):
        self._lib = load_library()
        if _handle is not None:
            self._g = _handle
        else:
            self._g = self._lib.sw_mt_create(int(seed) & 0xFFFFFFFF)
        if not self._g:
            raise EngineError("sw_mt_create failed")

    @classmethod
    def from_numpy_state(cls, state=None):
        """Continue the legacy global NumPy stream (np.random.get_state() by default)."""
        lib = load_library()
        st = np.random.get_state() if state is None else state
        if st[0] != 'MT19937':
            raise EngineError("not an MT19937 state")
        key = np.ascontiguousarray(st[1], dtype=np.uint32)
        g = lib.sw_mt_from_state(_ptr(key), int(st[2]))
        return cls(_handle=g)

    def numpy_state(self):
        """State tuple for np.random.set_state (same stream from here on)."""
        key = np.empty(624, dtype=np.uint32)
        pos = C.c_int(0)
        self._lib.sw_mt_get_state(self._g, _ptr(key), C.byref(pos))
        return ('MT19937', key, int(pos.value), 0, 0.0)

    def copy(self):
        return ProbeStream.from_numpy_state(self.numpy_state())

    def skip(self, ndraws):
        self._lib.sw_mt_skip(self._g, int(ndraws))

    def jump(self, ndraws):
        if self._lib.sw_mt_jump(self._g, int(ndraws)) != 0:
            raise EngineError("sw_mt_jump failed")

    def window(self):
        """The 624 raw words at the current position (Engine.stream_set)."""
        out = np.empty(624, dtype=np.uint32)
        self._lib.sw_mt_window(self._g, _ptr(out))
        return out

    def raw(self, n):
        out = np.empty(int(n), dtype=np.uint32)
        self._lib.sw_mt_raw(self._g, int(n), _ptr(out))
        return out

    def rademacher(self, count, n):
        out = np.empty((int(count), int(n)), dtype=np.int8)
        self._lib.sw_mt_rademacher(self._g, int(count) * int(n), _ptr(out))
        return out

    def z4(self, count, n):
        out = np.empty((int(count), int(n)), dtype=np.int8)
        self._lib.sw_mt_z4(self._g, int(count) * int(n), _ptr(out))
        return out

    def probes(self, count, n, kind="z2"):
        return self.rademacher(count, n) if kind == "z2" else self.z4(count, n)

    def __del__(self):  # pragma: no cover
        try:
            if self._g:
                self._lib.sw_mt_destroy(self._g)
                self._g = None
        except Exception:
            pass
