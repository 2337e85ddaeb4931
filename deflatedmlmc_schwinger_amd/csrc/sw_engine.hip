// sw_engine.hip -- host side of the MI355X Schwinger trace engine: operand ingestion, the
// batched flexible-GMRES / multigrid-cycle orchestration on one HIP stream, the probe-batch
// drivers and the C ABI of include/schwinger_hip.h.  gfx950 only; no CPU fallback: every
// compute entry point fails with a message when no HIP device is present.
#include "../../include/schwinger_hip.h"
#include "sw_kernels.hpp"
#include "sw_pack.hpp"
#include "sw_poly.hpp"

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

using swk::cplx;
using swk::cplxf;
using swk::PtrList;

#define SW_MAXM 32  // engine restart cap (<= SW_MAX_KRYLOV)
#define SW_NC_SLOTS 2048
#define SW_TICKET_CHUNKS 128

static std::string g_create_error;
static int (*g_rccl_destroy)(void*) = nullptr;   // set when RCCL has been loaded (sw_comm_*)

struct sw_engine;
static int sw_fail(sw_engine* h, const char* fmt, ...);

#define HIPCHK(call)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return sw_fail(h, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,  \
                     __LINE__);                                                           \
  } while (0)
#define SWCHK(...)              \
  do {                          \
    int rc_ = (__VA_ARGS__);    \
    if (rc_ != 0) return rc_;   \
  } while (0)

enum TimerCat { T_MVM = 0, T_DEFL, T_P, T_R, T_AXPY, T_DOTS, T_COARSEST, T_OTHER,
                T_STENCIL,      // k_stencil<0>  Y = A X
                T_STENCIL_RES,  // k_stencil<1>  Y = B - A X
                T_STENCIL_SM,   // k_stencil<2>  Y = X + w (B - A X)
                T_MFMA_DENSE,   // k_bsr_mfma on the dense coarsest inverse
                T_MFMA_OP,      // k_bsr_mfma on a block-structured level operator
                T_UNUSED13,     // (class 13 was a fused two-step stencil; removed, numbering kept)
                T_MFMA_OP2,     // k_bsr_mfma on level operators below level 1 of the solver hierarchy
                T_SCHUR,        // k_schur_step / k_eo_hop: even-odd smoother of the stencil level
                T_SCHUR_OP,     // k_schur_step<0/1>: operator / residual of the even-odd reduced system
                T_TP_SOURCES,   // k_slice_sources of SW_MODE_TWO_POINT
                T_TP_DOTS,      // k_slice_pair_dots / k_pair_total of SW_MODE_TWO_POINT
                T_SLICE_CDOTS,  // k_slice_cdots of SW_MODE_MLMC_LOOPS / sw_coarsest_loops
                T_MESON_FIELD,  // k_meson_field of sw_meson_fields / sw_low_mode_two_point
                T_LM_CONTRACT,  // k_cgemm_nt / k_lm_two_point_reduce of sw_low_mode_two_point
                T_LINK_DOTS,    // k_slice_link_dots of SW_MODE_HUTCHINSON_LINK_LOOPS
                T_3PT_SOURCES,  // k_seq_sources / k_pair_slice_total of SW_MODE_THREE_POINT
                T_3PT_DOTS,     // k_slice_seq_dots of SW_MODE_THREE_POINT
                T_SMEAR,        // k_smear_step / k_smear_fused of SW_MODE_TWO_POINT_SMEARED / sw_apply_smearing
                T_LAPH,         // k_laph_project of sw_perambulators; SW_KCLASS_LAPH reports it with T_LAPH_SRC
                T_LAPH_CONTRACT,  // k_laph_elementals / k_laph_left / k_laph_right / k_laph_reduce (sw_distilled_two_point)
                T_LAPH_GEN,     // k_laph_generalized (sw_generalized_perambulators, sw_apply_laph_generalized)
                T_LAPH_SRC,     // k_laph_sources (internal: number 29 is no kernel class and stays refused)
                T_LAPH_2M,      // k_laph_sink / k_laph_sandwich / k_laph_source / k_laph_trace1 / k_laph_trace2
                                // (sw_distilled_two_meson, sw_apply_laph_two_meson): SW_KCLASS_LAPH_TWO_MESON = 30
                T_NCAT };
// classes >= T_STENCIL are folded into the mvm / coarsest (two-point and three-point: other / dots; slice cdots,
// meson fields, their contraction and the link dots: dots; smearing: other; distillation: the projection dots, the
// sources other, the contraction, the generalized perambulators and the two-meson blocks dots) buckets by
// sw_timers and reported separately by sw_kernel_stats

struct EllOp {
  int nrows = 0, ncols = 0, K = 0, G = 1, ngroups = 0;
  int* cols = nullptr;
  cplx* vals = nullptr;
  int* order = nullptr;     // processing order of the row groups (NULL: natural), sw_pack.hpp
  // prolongators of even-odd smoothed levels: the row groups of the EVEN sites only, in `order`'s
  // order -- the smoother never reads the odd half of the prolongated iterate (ensure_even_orders)
  int* order_even = nullptr;
  int ngroups_even = 0;
  bool set = false;
  // optional MFMA block-row form (square operators with n % 16 == 0 and dense-ish 16x4 blocks)
  int bsr_KS = 0;
  int* bsr_kcol = nullptr;   // [n/16][KS] first X row of each 4-column group
  cplx* bsr_vals = nullptr;  // [n/16][KS][64] lane-packed
  int* bsr_tmap = nullptr;   // optional: row tile -> tile of the output vector (subset operators)
  int bsr_RT = 0;            // row tiles when != nrows / 16 (subset operators)
  bool bsr_diag_last = false;   // the last four k-steps of every row tile are its own X rows (check_diag_last)
  // dense operator whose row tiles all list the same columns in the same order (kcol rows identical): the
  // LDS-staged dense kernel (k_dense_mfma3_lds) shares the X rows of a k-step between row tiles
  bool dense_uniform = false;
  // complex64 mirrors of the value arrays (same index arrays), made on demand for the
  // single-precision preconditioner (option precond_f32)
  cplxf* vals32 = nullptr;
  cplxf* bsr_vals32 = nullptr;
};

struct KrylovWS {
  int m = 0, n = 0, nbp = 0;
  cplx* V = nullptr;  // m vectors: vtilde_1 .. vtilde_m (vtilde_0 is the residual itself)
  cplx* Z = nullptr;  // m vectors
  // single-precision preconditioner on the lattice level: its m directions stay complex64 (the widening
  // is exact, so A z and x += Z y see the same numbers) and v32 is the complex64 copy of the Krylov
  // vector it is applied to next, written by the kernel that produced that vector
  cplxf* Z32 = nullptr;
  cplxf* v32 = nullptr;
  // option f32_krylov: the whole restart cycle in complex64 storage (basis V32, w = A z written
  // complex64, inner products accumulated in fp64) -- iterative refinement with GMRES(m) cycles: the
  // residual b - A x and the solution update stay fp64, once per restart
  cplxf* V32 = nullptr;
  cplx* xacc = nullptr;
  cplx* rres = nullptr;
  swk::FgScalars sc{};
  cplx* h1 = nullptr;   // [(m+2)][nbp]
  cplx* h2 = nullptr;   // [(m+2)][nbp]
  cplx* c1 = nullptr;   // [(m+2)][nbp] orthogonalisation coefficients svec_k^2 d_k
  cplx* nrm = nullptr;  // [nbp]
  cplx* gram = nullptr; // [15][nbp] inner products of a restart cycle in Gram-matrix form (fgmres_eo_gram)
};

struct Level {
  int n = 0;
  bool stencil = false;
  int L = 0;
  double mass = 0.0;
  cplx* U1 = nullptr;
  cplx* U2 = nullptr;
  EllOp A, P, R;
  EllOp Re;   // stencil level, even-odd reduced outer solve: R restricted to the even-site columns
  // small level solved DIRECTLY (sw_setup_level_inverse): dense inverse of the level operator in block-row
  // form; solve_dev applies it with one step of iterative refinement instead of iterating
  EllOp dinv;
  int nu_pre = 0, nu_post = 3, kcycle = 0;
  // fixed-polynomial (Richardson) smoother: weights 1/theta_k; empty -> adaptive MR steps
  std::vector<std::complex<double>> w_pre, w_post;
  bool rich = false;
  // even-odd post-smoother: Richardson weights for the Schur complement S of the even sites.
  // Stencil level: S is the fused two-hop kernel.  Coarse (block) levels: four subset operators in
  // MFMA block-row form, eo_op[0] = S (even x even, 9-point), [1] = F = A_eo D_oo^-1,
  // [2] = G = D_oo^-1, [3] = Hb = D_oo^-1 A_oe
  std::vector<std::complex<double>> w_eo;
  // the same smoother polynomial in product form (swp::product_form): x + q(S)(b' - S x) with
  // q(z) = (1 - prod_k (1 - w_k z)) / z = q_beta prod_j (1 - q_w[j] z); empty when not available
  std::vector<std::complex<double>> q_w;
  std::complex<double> q_beta;
  EllOp eo_op[5];   // [4] (optional): the DENSE inverse of S over the even sites' rows -- the level's Schur
                    // steps, and everything below the level, are then replaced by one application of it
  std::vector<int> h_rowmap;  // natural -> internal (empty: identity)
  int* rowmap = nullptr;
  // per-level cycle workspace, [n][nbp]
  int ws_nbp = 0;
  cplx *b = nullptr, *x = nullptr, *r = nullptr, *t = nullptr;
  // single-precision preconditioner: link mirrors, cycle workspace and the boundary pair
  // (i32: cast of the fp64 input, o32: result before the cast back)
  cplxf *U1f = nullptr, *U2f = nullptr;
  int ws32_nbp = 0;
  cplxf *b32 = nullptr, *x32 = nullptr, *r32 = nullptr, *t32 = nullptr, *i32 = nullptr, *o32 = nullptr;
  // reference-faithful smoother: gm_cycles restart cycles of unpreconditioned GMRES(gm_m) from a
  // zero guess, the engine's counterpart of lgmres(maxiter=smooth_iters) with inner_m = 30
  // (multigrid.py:393-394,438-439).  gm_m == 0: off
  int gm_m = 0, gm_cycles = 0;
  cplx *g1 = nullptr, *g2 = nullptr;
  KrylovWS gws;   // smoother workspace
  // GPU-side setup: test vectors of this level, [n][64] (column = test vector), and a swap buffer
  cplx *tv = nullptr, *tv2 = nullptr;
  KrylovWS kws;   // K-cycle workspace
  KrylovWS sws;   // outer-solve workspace
};

struct Hier {
  int nlevels = 0;
  Level lv[SW_MAX_LEVELS];
  EllOp cinv;
  bool ready = false;
  bool f32_valid = false;   // the complex64 mirrors match the operators (cleared by every setter)
  bool even_valid = false;  // the even-site group lists of the prolongators match (likewise)
};

struct EventRec {
  int cat;
  hipEvent_t e0, e1;
};

// A resolved result of a probe batch on the device, [rows][stride] with one column per probe.
// result_begin() marks it not fetchable, grows it and records the shape about to be written; done() after the
// batch's last synchronisation makes the first nb columns fetchable; drop() is what a registration that sized it
// does.  result_fetch() copies the recorded rows, whatever is registered by then.
struct ResultBuf {
  cplx* p = nullptr;
  size_t cap = 0, rows = 0;
  int stride = 0;
  int nb = 0;   // probes of the last completed batch (0: nothing to fetch)
  void done(int nb_) { nb = nb_; }
  void drop() { nb = 0; }
};

struct sw_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  // probe generation runs on a stream of its own, so that the next batch's probes are drawn while the
  // current batch is being solved (sw_probes_generate is asynchronous; sw_hutch_run waits for its slot)
  hipStream_t gen_stream = nullptr;
  int pb_slot = -1;
  std::string err;
  Hier hier[SW_MAX_HIER];
  int restart = 24;
  int solver_hid = 0;
  bool use_mfma = true;
  int bsr_stages = 4, dense_stages = 8;   // software-pipeline depth of k_bsr_mfma (k-steps in flight)
  int bsr_map = 1, bsr_sub = 8, dense_map = 0;   // block orderings of k_bsr_mfma (see the kernel)
  bool bsr_nt = true;     // non-temporal B loads / Y stores in k_bsr_mfma on level operators
  bool ell_order = true;   // visit prolongator row groups sorted by column (A/B switch)
  bool bsr_xreg = true;    // smoother step of a block operator: own X rows from the operand registers (A/B switch)
  bool p_even = true;      // prolongate onto the even sites only ahead of an even-odd smoother (A/B switch)
  int bench_what = 0;      // what sw_bench_dirac times: 0 operator, 1 restrict, 2 prolong, 3 coarsest inverse
  int bench_mode = 0;      // operator mode sw_bench_dirac times (0: Y=AX, 1: residual, 2: smoother step)
  bool mfma_ops = true;   // MFMA block-row kernel also for block-structured level operators
  bool mfma_3m = true;    // three real matrix products per complex one (k_bsr_mfma3) instead of four
  int mfma3_tiles = 0;    // tiles of 16 probes per wave in k_bsr_mfma3 (0: by the operator's size)
  int mfma_tiles = 4;
  int f32_tiles = 0;          // tiles of 16 probes per wave in k_bsr_mfma_f32 (0: automatic)
  int f32_stages = 4, f32_dense_stages = 8;
  int f32_splitk = 1;         // split-K block-row kernel: 0 off, 1 dense coarsest inverse, 2 every small operator
  bool f32_krylov = true;     // with precond_f32 on the lattice level: complex64 Krylov basis per restart cycle
  bool f32_pairs = true;      // two probes per lane in the HBM-bound complex64 kernels (A/B switch)
  int mfma_small_tiles = 2;   // tiles per wave for operators too small to fill the chip (0: off)
  // iteration count of the previous outer solve per (hierarchy, level): the convergence flag
  // is only read back from (hint - 2) on, earlier iterations are queued without a host sync
  int sync_hint[SW_MAX_HIER][SW_MAX_LEVELS] = {{0}};
  bool lazy_sync = true;
  // time-skewed order of the even-odd smoother's steps on the stencil level (schur_steps): -1 automatic
  // (strips sized for the Infinity Cache where the smoother's three half vectors exceed it), 0 off,
  // > 0 strip height in lattice rows
  int eo_skew = -1;
  bool eo_skew_chunk = false;   // walk the strips 64-probe chunk by chunk even where the full width is admissible
  // restart cycles of the even-odd reduced outer solve in Gram-matrix form (fgmres_eo_gram)
  bool gram_cycle = true;
  // even-odd smoother of the reduced-system cycle in product form (schur_product_steps): 2 nu + 2 half-vector
  // passes instead of 3 nu
  bool eo_product = true;
  int gj_block = 32;      // panel width of the blocked Gauss-Jordan inverse (0: unblocked)
  // fp64 even-odd kernels of the lattice level from LDS-staged halo tiles double-buffered by LDS-DMA, one
  // persistent workgroup per CU (k_schur_tile; 0 off, 4 / 8 waves per workgroup): the launches without a b'
  // operand (reduced operator, product-form factors) on full-lattice launches
  int eo_tile = 0;
  // dense operators (coarsest inverse, dense Schur inverse of a direct level, direct inverse of a small level)
  // through the LDS-staged three-product kernel k_dense_mfma3_lds (A/B switch)
  int dense_lds = 4;     // row tiles per workgroup (2 or 4); 0: k_bsr_mfma3.  2048^2 on 256 probes, per launch:
                         // k_bsr_mfma3 142 us, 2 tiles 157, 4 tiles 135 (profiles/r04_ab_sessions.txt, r04j)
  int eo_tile_dbg = 0;   // timing diagnostics of k_schur_tile (results are then wrong): 1 no prefetch, 2 no compute
  int num_cus = 256;
  // levels that carry the dense inverse of their operator (sw_setup_level_inverse) are solved with it
  bool direct_small = true;
  bool lgmres_aug = true;   // reference-faithful smoother: LGMRES's augmentation vector in the second cycle
  bool stencil_nt = false;
  int stencil_tile = 0;   // 0: automatic
  int stencil_spw = 0;    // 0: automatic (4)
  // one Gram-Schmidt pass per Arnoldi step instead of two; every outer solve is then verified
  // against its TRUE residual and continued when the recurrence was optimistic
  bool cgs2 = false;
  bool verify = true;
  // second Gram-Schmidt pass in the short inner Krylov cycles (K-cycle, GMRES smoother): they are
  // preconditioners of 2-30 steps whose result feeds a flexible outer iteration, one pass suffices
  bool inner_cgs2 = false;
  // last Arnoldi step of every restart cycle without its orthogonalisation pass: h_{j+1,j} from
  // |A z|^2 - sum |h_{k,j}|^2 (single-pass Gram-Schmidt only; see fgmres)
  bool pyth_last = true;
  // outer solves of an even-odd smoothed stencil level on the even-odd reduced (Schur complement)
  // system: half-length Krylov vectors, see fgmres_eo
  bool eo_solve = true;
  // block levels that carry the dense inverse of their Schur complement (eo_op[4]) are solved with it
  bool eo_direct = true;
  // single-precision preconditioner: every application of a multigrid cycle as the preconditioner of
  // an fp64 flexible GMRES (and sw_vcycle) runs in complex64 on the f32 matrix cores -- operands cast
  // at the boundary, residuals / orthogonalisation / verification stay fp64
  bool precond_f32 = false;
  // deflation
  int kd = 0;
  cplx* U = nullptr;  // [n0][defl_ld(kd)] internal row order, zero beyond column kd
  // deflation kernels: 0 = k_defl_dots / k_defl_apply up to kd = 64 and the MFMA kernels above it,
  // 1 = the MFMA kernels (k_defl_gemm_*) at every kd
  int defl_gemm = 0;
  // MLMC-level deflation vectors V_l (utils.py:260-266), [n_l][defl_ld(k_l)] internal row order
  int lkd[SW_MAX_LEVELS] = {0};
  cplx* lV[SW_MAX_LEVELS] = {nullptr};
  // Pperm^T gathers and MLMC rhs maps (hid 0)
  int* perm_src[SW_MAX_LEVELS] = {nullptr};
  EllOp rhsmap[SW_MAX_LEVELS];
  // scratch
  cplx* partial = nullptr;
  size_t partial_bytes = 0;
  cplx* small = nullptr;  // small per-probe scalars
  size_t small_bytes = 0;
  void* stage = nullptr;  // host<->device staging
  size_t stage_bytes = 0;
  std::vector<std::pair<void*, size_t>> allocs;
  // probe batch state
  int pb_level = -1, pb_nb = 0, pb_nbp = 0;
  int8_t* pb_probes = nullptr;   // currently selected slot
  struct ProbeSlot {
    int8_t* p = nullptr;
    size_t bytes = 0;
    int level = -1, nb = 0;
    hipEvent_t ready = nullptr;   // recorded on gen_stream behind the slot's generation (pending: true)
    bool pending = false;
  };
  std::vector<ProbeSlot> slots;
  // device probe stream (k_mt_jump / k_mt_generate): window = 624 raw MT19937 words at mt_pos
  bool mt_set = false;
  uint32_t* mt_win0 = nullptr;      // window at stream position 0 (as handed to sw_probes_stream_set)
  uint32_t* mt_win = nullptr;       // [2][624] double buffer, mt_win + 624*mt_cur is current
  int mt_cur = 0;
  uint64_t mt_pos = 0;              // stream position (draws) of the current window
  uint32_t* mt_poly = nullptr;      // [624] x^mt_dist mod phi
  uint64_t mt_dist = 0;
  uint32_t* mt_family = nullptr;    // [mt_fam_count][624]: x^(s*mt_fam_seg), s = 1..count
  uint64_t mt_fam_seg = 0;
  int mt_fam_count = 0;
  cplx *pb_x0 = nullptr, *pb_rhs = nullptr, *pb_z = nullptr, *pb_xc = nullptr, *pb_xc2 = nullptr,
       *pb_y = nullptr, *pb_w = nullptr, *pb_w2 = nullptr, *pb_xd = nullptr;
  int pb_ws_nbp = 0;
  cplx* pb_est = nullptr;
  int* pb_iters = nullptr;
  // shifted probe dots (sw_set_shifts, SW_MODE_HUTCHINSON_SHIFTS): the registered flat shifts, their ring
  // displacements d_j = s_j / 2L on the device (padded to a multiple of 16 with d_0), the ring -> internal row
  // table of the lattice level, the probes' int8 codes in the engine layout and the estimates [shift][probe]
  std::vector<int64_t> shifts;
  int* shift_disp = nullptr;
  int* ringrow = nullptr;
  int8_t* pb_codes = nullptr;
  ResultBuf r_shifts;
  // timeslice loops (sw_set_loop_momenta, SW_MODE_HUTCHINSON_LOOPS): the registered momenta (on the device padded
  // to SW_MAX_MOMENTA with the first), the phase table omega^j = e^{-2 pi i j / L}, j in [0, L), the
  // (timeslice, x, spin) -> internal row table of the lattice level and the loops [momentum][a][b][t][probe]
  std::vector<int32_t> momenta;
  int* loop_mom = nullptr;
  cplx* loop_phase = nullptr;
  int* slicerow = nullptr;
  ResultBuf r_loops;
  // MLMC level loops (SW_MODE_MLMC_LOOPS / _SKIP, sw_apply_slice_cdots): the same momenta and tables, results in a
  // buffer of their own so that sw_hutch_fetch_loops keeps returning mode 5's last batch
  ResultBuf r_mloops;
  // point-split link loops (SW_MODE_HUTCHINSON_LINK_LOOPS, sw_apply_slice_link_dots): the same momenta and tables,
  // the four branches [d][momentum][a][b][t][probe] in a buffer of their own
  ResultBuf r_links;
  // one-end-trick two-point functions (sw_set_two_point, SW_MODE_TWO_POINT): a registration of its own (source
  // timeslice, momenta, the index of momentum 0, tables as for the loops), the sources and solutions [n][2 M nq]
  // and the pair sums T[momentum][a][b][c][d][t][noise]
  std::vector<int32_t> tp_momenta;
  int tp_t0 = 0, tp_j0 = 0;
  int* tp_mom = nullptr;
  cplx* tp_phase = nullptr;
  int* tp_slicerow = nullptr;
  cplx *tp_rhs = nullptr, *tp_z = nullptr;
  size_t tp_ws_cap = 0;
  ResultBuf r_tp;
  // smeared sources and sinks (sw_set_smearing, SW_MODE_TWO_POINT_SMEARED): a registration of its own -- kappa with
  // the two coefficients of a step as the kernels take them, the source steps, the ascending sink steps, a
  // (timeslice, x, spin) -> internal row table of its own -- and the pair sums
  // T[sink level][momentum][a][b][c][d][t][noise]
  double sm_kappa = 0.0, sm_c0 = 1.0, sm_c1 = 0.0;
  int sm_source = 0;
  std::vector<int32_t> sm_sink;
  int* sm_slicerow = nullptr;
  ResultBuf r_tps;
  // distillation (sw_set_distillation, sw_perambulators): a registration of its own -- the eigenvectors as
  // swp::laph_pack lays them out, conj(V)[t][lh_Lp][lh_ld], and a (timeslice, x, spin) -> internal row table of its own
  int lh_nev = 0, lh_Lp = 0, lh_ld = 0;
  cplx* lh_V = nullptr;
  int* lh_slicerow = nullptr;
  // ... and its momenta (sw_set_distillation_momenta): the transposed, padded elementals Mt[momentum][t][ld][ld] of
  // k_laph_elementals with the tables they were made from; dropped with the eigenvectors
  std::vector<int32_t> lh_momenta;
  int* lh_mom = nullptr;
  cplx* lh_phase = nullptr;
  cplx* lh_M = nullptr;
  // low-mode averaging (sw_set_low_mode_inverse, sw_meson_fields, SW_MODE_TWO_POINT_LMA): G [lm_k][lm_k] row-major
  // for the registered deflation vectors (lm_k = kd, 0: none), the tables of sw_meson_fields, the coefficients
  // c and c' [2][ld][columns], and the remainder R = T(z, z) - T(z_L, z_L) of the last batch with T(z_L, z_L)'s
  // scratch beside it -- buffers of the mode's own, sw_hutch_fetch_two_point keeps returning mode 6's last batch
  int lm_k = 0;
  cplx* lm_G = nullptr;
  int* lm_mom = nullptr;
  cplx* lm_phase = nullptr;
  int* lm_slicerow = nullptr;
  cplx* lm_coef = nullptr;
  size_t lm_coef_cap = 0;
  ResultBuf r_lma, lma_tmp;
  // three-point functions (sw_set_three_point, SW_MODE_THREE_POINT): a registration of its own (source and sink
  // timeslice, sink spin matrix and momentum, insertion momenta; t3_jz = the index of momentum 0 or -1; t3_mom0 =
  // a zero momentum table for the stage-1 sources), three blocks [n][2 nq] -- the sources of either stage, z and
  // zeta -- and the sums S[branch][momentum][a][b][f][c][t][noise]
  std::vector<int32_t> t3_momenta;
  int t3_t0 = 0, t3_tf = 0, t3_gamma = 0, t3_pf = 0, t3_jz = -1;
  int *t3_mom = nullptr, *t3_mom0 = nullptr;
  cplx* t3_phase = nullptr;
  int* t3_slicerow = nullptr;
  cplx *t3_rhs = nullptr, *t3_z = nullptr, *t3_zeta = nullptr;
  size_t t3_ws_cap = 0;
  ResultBuf r_t3;
  std::vector<int32_t> last_iters_f, last_iters_c;
  // profiling
  bool profiling = false;
  std::vector<EventRec> recs;
  std::vector<hipEvent_t> evpool;
  double tacc[T_NCAT] = {0};
  int64_t tcount[T_NCAT] = {0};
  double twork[T_NCAT] = {0};   // arithmetic issued per class while profiling (flops, MFMA classes)
  int64_t launches = 0;
  // convergence counters: one slot per FGMRES scalar update of an outer solve (no per-iteration reset);
  // the last slot is the sink of the inner solves, which nobody reads
  int* d_notconv = nullptr;  // [SW_NC_SLOTS]
  int nc_next = 0;
  int* h_notconv = nullptr;  // pinned
  // tickets of the in-launch reductions (swk::reduce_and_tail), zero between launches
  int* d_tick = nullptr;     // [SW_TICKET_CHUNKS * (SW_RED_MAXGROUPS + 1)]
  bool fused_reduce = true;
  // the batch is iterated until every probe's residual is below stop_factor * tol; iteration counts are
  // reported at tol (multigrid.py:347-366).  1: the reference's stopping point; 0.1: per-probe estimates
  // to 1e-10 relative even where the estimate cancels to a small number
  double stop_factor = 1.0;
  // directly solved levels (sw_setup_level_inverse): the measured ||b - A x|| / ||b|| of the last such solve
  // per right-hand side, and how often the refinement did not reach the tolerance and the iterative path
  // took over
  std::vector<double> direct_relres;
  int64_t direct_fallbacks = 0;
  // host time spent inside hipMalloc / hipFree, calls and bytes allocated since creation
  double alloc_s = 0.0, alloc_bytes = 0.0;
  int64_t alloc_calls = 0, pool_hits = 0;
  // device eigensolver (sw_eig_*): three [n][64] block buffers on one (hierarchy, level), the gamma_3 signs
  // in that level's row order, the partial sums of the block Gram kernel
  cplx* eig_buf[3] = {nullptr, nullptr, nullptr};
  signed char* eig_sign = nullptr;
  cplx* eig_small = nullptr;     // [w*w] reduced Gram matrix / rotation
  int eig_w = 64;                // block width w: w/64 groups of [n][64] (sw_eig_begin_wide)
  cplx* eig_cs[2] = {nullptr, nullptr};   // sw_eig_apply_diff: two [n_{l+1}][64] coarse blocks (first use)
  int eig_hid = -1, eig_level = -1, eig_n = 0;
  void* comm = nullptr;      // RCCL communicator (sw_comm_init), one rank per engine
  double* d_stats = nullptr; // [4] all-reduce buffer
};
// every fetchable result (a new definition of the reference hierarchy drops them all)
static constexpr ResultBuf sw_engine::* kResults[] = {&sw_engine::r_shifts, &sw_engine::r_loops, &sw_engine::r_mloops,
                                                      &sw_engine::r_links,  &sw_engine::r_tp,    &sw_engine::r_lma,
                                                      &sw_engine::r_t3,    &sw_engine::r_tps};

// ---------------------------------------------------------------------------------------------
// engine options (sw_set_option / sw_get_option): one entry per name.  Bool fields take value != 0, int
// fields (int)value; a validator rejects a value with its message before anything is stored.
// ---------------------------------------------------------------------------------------------
static int g_dot_blocks = 1024, g_dot_pmax = 1024;   // process-wide (row_blocking has no engine)

struct EngineOption {
  const char* name;
  double (*get)(const sw_engine*);
  void (*set)(sw_engine*, double);   // nullptr: a read-only statistic
  bool (*ok)(double) = nullptr;      // the values sw_set_option accepts (nullptr: all)
  const char* msg = nullptr;         // its message for the others
};
template <auto F>
static double get_field(const sw_engine* h) { return (double)(h->*F); }
template <auto F>
static void set_field(sw_engine* h, double v) { h->*F = static_cast<std::remove_reference_t<decltype(h->*F)>>(v); }
template <auto F>
static constexpr EngineOption field(const char* name, bool (*ok)(double) = nullptr, const char* msg = nullptr) {
  return {name, get_field<F>, set_field<F>, ok, msg};
}

static constexpr EngineOption kOptions[] = {
    // kernel choices
    field<&sw_engine::use_mfma>("use_mfma"),   // MFMA block-row kernels where an operator has that form
    field<&sw_engine::mfma_ops>("mfma_ops"),   // ... also for the block-structured level operators
    field<&sw_engine::mfma_3m>("mfma_3m"),     // k_bsr_mfma3 (three real products) instead of k_bsr_mfma
    // k_bsr_mfma probe tiles per wave, and on operators too small to fill the chip (0: off)
    field<&sw_engine::mfma_tiles>("mfma_tiles", [](double v) { return v == 2.0 || v == 4.0; },
                                  "mfma_tiles must be 2 or 4"),
    field<&sw_engine::mfma_small_tiles>("mfma_small_tiles",
                                        [](double v) { return v == 0.0 || v == 2.0 || v == 4.0; },
                                        "mfma_small_tiles must be 0, 2 or 4"),
    // k_bsr_mfma3 probe tiles per wave (0: by the operator's size)
    field<&sw_engine::mfma3_tiles>("mfma3_tiles",
                                   [](double v) { const int t = (int)v; return t == 0 || t == 1 || t == 2 || t == 4; },
                                   "mfma3_tiles must be 0, 1, 2 or 4"),
    // block orderings of k_bsr_mfma on level operators and on the dense coarsest inverse, and their grouping
    field<&sw_engine::bsr_map>("bsr_map", [](double v) { return (int)v >= 0 && (int)v <= 3; },
                               "bsr_map must be 0..3"),
    field<&sw_engine::dense_map>("dense_map", [](double v) { return (int)v >= 0 && (int)v <= 3; },
                                 "dense_map must be 0..3"),
    field<&sw_engine::bsr_sub>("bsr_sub", [](double v) { return (int)v >= 1; }, "bsr_sub must be >= 1"),
    // k-steps in flight in k_bsr_mfma on level operators and on dense ones
    field<&sw_engine::bsr_stages>("bsr_stages", [](double v) { return v == 2.0 || v == 4.0 || v == 8.0; },
                                  "bsr_stages must be 2, 4 or 8 (dense_stages: or 16)"),
    field<&sw_engine::dense_stages>("dense_stages",
                                    [](double v) { return v == 2.0 || v == 4.0 || v == 8.0 || v == 16.0; },
                                    "dense_stages must be 2, 4 or 8 (dense_stages: or 16)"),
    field<&sw_engine::bsr_nt>("bsr_nt"),       // non-temporal loads / stores on level operators
    field<&sw_engine::bsr_xreg>("bsr_xreg"),   // own X rows from the operand registers
    // k_dense_mfma3_lds row tiles per workgroup (1 is stored as 2; 0: k_bsr_mfma3)
    {"dense_lds", get_field<&sw_engine::dense_lds>,
     [](sw_engine* h, double v) { h->dense_lds = v == 1.0 ? 2 : (int)v; },
     [](double v) { return v == 0.0 || v == 1.0 || v == 2.0 || v == 4.0; }, "dense_lds must be 0, 2 or 4"},
    // k_defl_gemm_* at every deflation rank
    field<&sw_engine::defl_gemm>("defl_gemm", [](double v) { return v == 0.0 || v == 1.0; },
                                 "defl_gemm must be 0 or 1"),
    field<&sw_engine::fused_reduce>("fused_reduce"),   // cross-workgroup sums inside the reducing launch
    // row blocks of the reducing BLAS-1 launches (process-wide, at least 64)
    {"dot_blocks", [](const sw_engine*) { return (double)g_dot_blocks; },
     [](sw_engine*, double v) { g_dot_blocks = g_dot_pmax = std::max(64, (int)v); }},
    // panel width of the blocked Gauss-Jordan inverse (0: unblocked)
    field<&sw_engine::gj_block>("gj_block",
                                [](double v) {
                                  const int b = (int)v;
                                  return b == 0 || (b >= 8 && b <= 256 && b % 8 == 0);
                                },
                                "gj_block must be 0 or a multiple of 8 in 8..256"),
    // lattice level: stencil stores, x-tile and x-sites per wave (0: automatic)
    field<&sw_engine::stencil_nt>("stencil_nt"),
    field<&sw_engine::stencil_tile>("stencil_tile"),
    field<&sw_engine::stencil_spw>("stencil_spw",
                                   [](double v) {
                                     const int t = (int)v;
                                     return t == 0 || t == 1 || t == 2 || t == 4 || t == 8;
                                   },
                                   "stencil_spw must be 0,1,2,4,8"),
    // k_schur_tile waves per workgroup (0: off), and its timing diagnostics (two bits)
    field<&sw_engine::eo_tile>("eo_tile", [](double v) { return v == 0.0 || v == 4.0 || v == 8.0; },
                               "eo_tile must be 0 (off), 4 or 8 waves"),
    {"eo_tile_dbg", get_field<&sw_engine::eo_tile_dbg>, [](sw_engine* h, double v) { h->eo_tile_dbg = (int)v & 3; }},
    // time-skewed Schur steps: strip height (-1 automatic, 0 off), walked 64 probes at a time
    field<&sw_engine::eo_skew>("eo_skew", [](double v) { return !(v < -1.0 || v > 65536.0); },
                               "eo_skew must be -1 (automatic), 0 (off) or a strip height"),
    field<&sw_engine::eo_skew_chunk>("eo_skew_chunk"),
    field<&sw_engine::eo_product>("eo_product"),   // even-odd smoother in product form
    // transfers and cycle
    field<&sw_engine::p_even>("p_even"),           // prolongate onto the even sites ahead of an even-odd smoother
    // prolongator row groups in column order (the even-site group lists are rebuilt)
    {"ell_order", get_field<&sw_engine::ell_order>, [](sw_engine* h, double v) {
       h->ell_order = v != 0.0;
       for (Hier& H : h->hier) H.even_valid = false;
     }},
    field<&sw_engine::direct_small>("direct_small"),   // solve levels with a dense inverse directly
    field<&sw_engine::eo_direct>("eo_direct"),         // ... and block levels with a dense Schur inverse
    field<&sw_engine::lgmres_aug>("lgmres_aug"),       // LGMRES augmentation in the GMRES smoother
    // outer solve
    field<&sw_engine::cgs2>("cgs2"),                   // two Gram-Schmidt passes per Arnoldi step
    field<&sw_engine::inner_cgs2>("inner_cgs2"),       // ... in the inner Krylov cycles
    field<&sw_engine::pyth_last>("pyth_last"),         // last Arnoldi step of a cycle without its pass
    field<&sw_engine::verify>("verify"),               // true-residual check of a converged solve
    field<&sw_engine::lazy_sync>("lazy_sync"),         // convergence read back late (sync_hint)
    field<&sw_engine::eo_solve>("eo_solve"),           // outer solve on the even-odd reduced system
    field<&sw_engine::gram_cycle>("gram_cycle"),       // ... in Gram-matrix restart cycles
    field<&sw_engine::stop_factor>("stop_factor", [](double v) { return v > 0.0 && v <= 1.0; },
                                   "stop_factor must be in (0, 1]"),   // iterate to stop_factor * tol
    // single-precision preconditioner
    field<&sw_engine::precond_f32>("precond_f32"),     // complex64 multigrid cycle
    field<&sw_engine::f32_krylov>("f32_krylov"),       // complex64 Krylov basis per restart cycle
    field<&sw_engine::f32_pairs>("f32_pairs"),         // two probes per lane
    // k_bsr_mfma_f32 probe tiles per wave (0: automatic), k-steps in flight, split-K kernel (0 off, 1 dense
    // coarsest inverse, 2 every small operator)
    field<&sw_engine::f32_tiles>("f32_tiles",
                                 [](double v) { const int t = (int)v; return t == 0 || t == 1 || t == 2 || t == 4; },
                                 "f32_tiles must be 0, 1, 2 or 4"),
    field<&sw_engine::f32_stages>("f32_stages"),
    field<&sw_engine::f32_dense_stages>("f32_dense_stages"),
    field<&sw_engine::f32_splitk>("f32_splitk"),
    // what sw_bench_dirac times (0 operator, 1 restrict, 2 prolong, 3 coarsest inverse), in which operator mode
    field<&sw_engine::bench_what>("bench_what", [](double v) { return !(v < 0.0 || v > 3.0); },
                                  "bench_what must be 0..3"),
    field<&sw_engine::bench_mode>("bench_mode", [](double v) { return v == 0.0 || v == 1.0 || v == 2.0; },
                                  "bench_mode must be 0, 1 or 2"),
    // read-only statistics: direct solves that fell back to the iterative path, allocator time, calls, volume,
    // and allocations served from parked blocks
    {"direct_fallbacks", get_field<&sw_engine::direct_fallbacks>, nullptr},
    {"alloc_seconds", get_field<&sw_engine::alloc_s>, nullptr},
    {"alloc_calls", get_field<&sw_engine::alloc_calls>, nullptr},
    {"alloc_gbytes", [](const sw_engine* h) { return h->alloc_bytes * 1e-9; }, nullptr},
    {"pool_hits", get_field<&sw_engine::pool_hits>, nullptr},
};

static int sw_fail(sw_engine* h, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  else g_create_error = buf;
  return 1;
}

// ---------------------------------------------------------------------------------------------
// memory helpers
// ---------------------------------------------------------------------------------------------
// hipMalloc / hipFree with their host time accumulated (option "alloc_seconds" etc.: the setup log splits its
// phases into allocation time and the rest).  Large blocks are PARKED instead of freed and handed out again:
// the device setup allocates and frees multi-GB scratch per level (11.8 GB for one Arnoldi run on the 1024^2
// lattice), and in a process that has already moved ~100 GB through the allocator those calls were measured at
// 2.5-3.4 s per setup where a fresh process needs 0.02 s (profiles/r04_ab_sessions.txt, r04h: the cause of the
// driver-observed 2.4x slower 1024^2 setup of round 3).  The pool is per process (engines come and go), capped
// (SW_POOL_GB, default 128 of the 288 GB: evicting parked blocks is itself a slow hipFree; 0 disables; an
// allocation that fails with blocks parked returns them to the driver and retries), and a block is parked only
// after the freeing engine's streams have drained (hipFree's implicit synchronisation is what made reuse by
// another stream safe before).
namespace {
struct ParkedBlock {
  void* p;
  size_t bytes;
  int device;
};
std::mutex g_pool_mu;
std::vector<ParkedBlock> g_pool;
size_t g_pool_bytes = 0;
const size_t kPoolMinBlock = (size_t)32 << 20;
size_t pool_cap() {
  static const size_t cap = [] {
    const char* e = std::getenv("SW_POOL_GB");
    const double gb = e ? std::atof(e) : 128.0;
    return gb > 0.0 ? (size_t)(gb * 1073741824.0) : (size_t)0;
  }();
  return cap;
}
}  // namespace

static int dev_alloc(sw_engine* h, void** p, size_t bytes) {
  if (bytes == 0) bytes = 16;
  const auto t0 = std::chrono::steady_clock::now();
  *p = nullptr;
  if (bytes >= kPoolMinBlock && pool_cap() > 0) {
    // size classes of 1/8 octave (at most 12.5 % over the request), so that workspaces of similar shapes --
    // Krylov bases of m or m + 1 vectors, the Arnoldi basis, probing blocks -- meet in the pool
    size_t top = (size_t)1 << 25;
    while ((top << 1) <= bytes) top <<= 1;
    const size_t step = top >> 3;
    bytes = ((bytes + step - 1) / step) * step;
  }
  size_t got = bytes;
  if (bytes >= kPoolMinBlock && pool_cap() > 0) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    int best = -1;
    for (size_t i = 0; i < g_pool.size(); ++i)
      if (g_pool[i].device == h->device && g_pool[i].bytes >= bytes && g_pool[i].bytes <= 2 * bytes &&
          (best < 0 || g_pool[i].bytes < g_pool[best].bytes))
        best = (int)i;
    if (best >= 0) {
      *p = g_pool[best].p;
      got = g_pool[best].bytes;
      g_pool_bytes -= got;
      g_pool.erase(g_pool.begin() + best);
      h->pool_hits++;
    }
  }
  if (!*p && hipMalloc(p, bytes) != hipSuccess) {
    // out of device memory with blocks parked: give them back and try once more
    (void)hipGetLastError();
    std::vector<ParkedBlock> blocks;
    {
      std::lock_guard<std::mutex> lk(g_pool_mu);
      blocks.swap(g_pool);
      g_pool_bytes = 0;
    }
    for (auto& b : blocks) (void)hipFree(b.p);
    *p = nullptr;
    HIPCHK(hipMalloc(p, bytes));
  }
  h->alloc_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  h->alloc_calls++;
  h->alloc_bytes += (double)bytes;
  h->allocs.push_back({*p, got});
  return 0;
}
static int dev_free(sw_engine* h, void* p) {
  if (!p) return 0;
  size_t bytes = 0;
  for (size_t i = 0; i < h->allocs.size(); ++i)
    if (h->allocs[i].first == p) {
      bytes = h->allocs[i].second;
      h->allocs.erase(h->allocs.begin() + i);
      break;
    }
  const auto t0 = std::chrono::steady_clock::now();
  if (bytes >= kPoolMinBlock && pool_cap() > 0) {
    // nothing of this engine may still be using the block when another stream gets it; a block whose streams
    // cannot be drained goes back to the driver instead
    auto drain = [&]() -> int {
      if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));
      if (h->gen_stream) HIPCHK(hipStreamSynchronize(h->gen_stream));
      return 0;
    };
    if (drain() != 0) {
      (void)hipFree(p);
      return 1;
    }
    std::vector<void*> evict;
    {
      std::lock_guard<std::mutex> lk(g_pool_mu);
      g_pool.push_back({p, bytes, h->device});
      g_pool_bytes += bytes;
      while (g_pool_bytes > pool_cap() && !g_pool.empty()) {     // oldest first
        evict.push_back(g_pool.front().p);
        g_pool_bytes -= g_pool.front().bytes;
        g_pool.erase(g_pool.begin());
      }
    }
    for (void* q : evict) HIPCHK(hipFree(q));
  } else {
    HIPCHK(hipFree(p));
  }
  h->alloc_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}
template <class T>
static int dev_realloc(sw_engine* h, T** p, size_t count) {
  if (*p) SWCHK(dev_free(h, *p));
  *p = nullptr;
  void* q = nullptr;
  SWCHK(dev_alloc(h, &q, count * sizeof(T)));
  *p = (T*)q;
  return 0;
}
template <class T>
static int upload(sw_engine* h, T** dst, const T* src, size_t count) {
  SWCHK(dev_realloc(h, dst, count));
  if (count) HIPCHK(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
// Owner of a function-local device buffer: allocated through dev_realloc / upload on `p`, released through
// dev_free when it goes out of scope, error returns included.  That release keeps the message already in
// h->err: the first failure is what the caller reports.
template <class T>
struct DevBuf {
  sw_engine* h;
  T* p = nullptr;
  explicit DevBuf(sw_engine* h_) : h(h_) {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : h(o.h), p(o.p) { o.p = nullptr; }
  ~DevBuf() {
    if (!p) return;
    std::string first;
    first.swap(h->err);
    (void)dev_free(h, p);
    h->err.swap(first);
  }
  operator T*() const { return p; }
};
// ResultBuf: about to be written as [rows][stride]
static int result_begin(sw_engine* h, ResultBuf& r, size_t rows, int stride) {
  r.drop();
  if (r.cap < rows * stride) {
    SWCHK(dev_realloc(h, &r.p, rows * stride));
    r.cap = rows * stride;
  }
  r.rows = rows;
  r.stride = stride;
  return 0;
}
// out[rows][nb] = the first nb columns, once the stream has drained
static int result_fetch(sw_engine* h, const ResultBuf& r, int nb, double* out) {
  HIPCHK(hipMemcpy2D(out, sizeof(cplx) * nb, r.p, sizeof(cplx) * r.stride, sizeof(cplx) * nb, r.rows,
                     hipMemcpyDeviceToHost));
  return 0;
}
static int ensure_stage(sw_engine* h, size_t bytes) {
  if (h->stage_bytes >= bytes) return 0;
  if (h->stage) SWCHK(dev_free(h, h->stage));
  h->stage = nullptr;
  SWCHK(dev_alloc(h, &h->stage, bytes));
  h->stage_bytes = bytes;
  return 0;
}
static int ensure_partial(sw_engine* h, size_t bytes) {
  if (h->partial_bytes >= bytes) return 0;
  if (h->partial) SWCHK(dev_free(h, h->partial));
  h->partial = nullptr;
  void* q;
  SWCHK(dev_alloc(h, &q, bytes));
  h->partial = (cplx*)q;
  h->partial_bytes = bytes;
  return 0;
}
static inline int pad64(int nb) { return ((nb + 63) / 64) * 64; }
// row stride of a registered deflation basis: kd rounded up to the 16-column MFMA tile
static inline int defl_ld(int kd) { return ((kd + 15) / 16) * 16; }

// ---------------------------------------------------------------------------------------------
// launch bookkeeping (HIP-event buckets mirror CustomTimer, utils.py:366-445)
// ---------------------------------------------------------------------------------------------
struct LaunchScope {
  sw_engine* h;
  int idx = -1;
  LaunchScope(sw_engine* h_, int cat) : h(h_) {
    h->launches++;
    if (h->profiling) {
      EventRec r;
      r.cat = cat;
      auto get = [&]() {
        hipEvent_t e;
        if (!h->evpool.empty()) {
          e = h->evpool.back();
          h->evpool.pop_back();
        } else {
          (void)hipEventCreate(&e);
        }
        return e;
      };
      r.e0 = get();
      r.e1 = get();
      (void)hipEventRecord(r.e0, h->stream);
      h->recs.push_back(r);
      idx = (int)h->recs.size() - 1;
    }
  }
  ~LaunchScope() {
    if (idx >= 0) (void)hipEventRecord(h->recs[idx].e1, h->stream);
  }
};
static void harvest_events(sw_engine* h) {
  for (auto& r : h->recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
      h->tacc[r.cat] += ms;
      h->tcount[r.cat] += 1;
    }
    h->evpool.push_back(r.e0);
    h->evpool.push_back(r.e1);
  }
  h->recs.clear();
}
static int stream_sync(sw_engine* h) {
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->profiling) harvest_events(h);
  return 0;
}
#define KLAUNCH_CHECK() HIPCHK(hipGetLastError())

// One kernel launch on the engine's stream, counted and (while profiling) timed in class `cat`
template <class... P, class... A>
static int launch(sw_engine* h, int cat, void (*k)(P...), dim3 grid, dim3 block, A&&... a) {
  LaunchScope ls(h, cat);
  k<<<grid, block, 0, h->stream>>>(a...);
  KLAUNCH_CHECK();
  return 0;
}

// Runtime value -> template argument: f(IntC<V>{}) for one V of the list.
// pick: the V equal to v, or the last V when none is.  pick_ge: the first V >= v, or the last V.
template <int V>
using IntC = std::integral_constant<int, V>;
template <int... Vs, class F>
static int pick(int v, F&& f) {
  constexpr int last[] = {Vs...};
  int rc = 0;
  (void)(((v == Vs || Vs == last[sizeof...(Vs) - 1]) && (rc = f(IntC<Vs>{}), true)) || ...);
  return rc;
}
template <int... Vs, class F>
static int pick_ge(int v, F&& f) {
  constexpr int last[] = {Vs...};
  int rc = 0;
  (void)(((v <= Vs || Vs == last[sizeof...(Vs) - 1]) && (rc = f(IntC<Vs>{}), true)) || ...);
  return rc;
}

// One launch of k_slice_dots / k_slice_cdots for the registered momenta: f(momenta per pass, phased) with the
// no-phase instantiation for the single momentum 0, else the smallest instantiation that holds them all (none of
// them spills)
template <class F>
static int pick_momenta(sw_engine* h, F&& f) {
  if (h->momenta.size() == 1 && h->momenta[0] == 0) return f(IntC<1>{}, std::false_type{});
  return pick_ge<1, 2, 4, 8>((int)h->momenta.size(), [&](auto NP) { return f(NP, std::true_type{}); });
}

// ---------------------------------------------------------------------------------------------
// CSR -> grouped ELL / MFMA block-row form: packed on the host (sw_pack.hpp), uploaded here
// ---------------------------------------------------------------------------------------------
static int build_ell(sw_engine* h, EllOp& op, int nrows, int ncols, const int64_t* indptr,
                     const int32_t* indices, const std::complex<double>* data,
                     const std::vector<int>& rows_int, const std::vector<int>& colmap,
                     int forceG = 0, bool sort_by_column = false) {
  swp::EllHost e;
  std::string err;
  if (swp::ell_pack(e, err, nrows, ncols, indptr, indices, data, rows_int, colmap, forceG,
                    sort_by_column) != 0)
    return sw_fail(h, "%s", err.c_str());
  op.nrows = nrows;
  op.ncols = ncols;
  op.K = e.K;
  op.G = e.G;
  op.ngroups = e.ngroups;
  SWCHK(upload(h, &op.cols, e.cols.data(), e.cols.size()));
  SWCHK(upload(h, (std::complex<double>**)&op.vals, e.vals.data(), e.vals.size()));
  if (!e.order.empty()) SWCHK(upload(h, &op.order, e.order.data(), e.order.size()));
  op.set = true;
  return 0;
}

// MFMA block-row form of a square CSR operator in natural order (level >= 1 operators and the
// dense inverse).  Built only when at least `min_fill` of the packed 16x4 groups is non-zero.
static void check_diag_last(EllOp& op, const int32_t* kcol, const int32_t* tmap);
static int build_bsr(sw_engine* h, EllOp& op, int n, const int64_t* indptr, const int32_t* indices,
                     const std::complex<double>* data, double min_fill) {
  swp::BsrHost b;
  swp::bsr_pack(b, n, indptr, indices, data, min_fill);
  op.bsr_KS = 0;
  if (b.KS == 0) return 0;
  SWCHK(upload(h, &op.bsr_kcol, b.kcol.data(), b.kcol.size()));
  SWCHK(upload(h, (std::complex<double>**)&op.bsr_vals, b.vals.data(), b.vals.size()));
  op.bsr_KS = b.KS;
  if (op.nrows == 0) op.nrows = n;
  check_diag_last(op, b.kcol.data(), nullptr);
  return 0;
}

// Does every row tile end with its own diagonal block (k-steps KS-4 .. KS-1 = X rows 16 ot + 4 r)?
// The packers arrange it (sw_pack.hpp, hierarchy.block_rows_from_matrix, setup_gpu.level_geometry);
// the kernel's register shortcut is only taken where this check, on the index array itself, passes.
static void check_diag_last(EllOp& op, const int32_t* kcol, const int32_t* tmap) {
  op.bsr_diag_last = false;
  const int KS = op.bsr_KS;
  const int RT = op.bsr_RT > 0 ? op.bsr_RT : op.nrows / 16;
  if (KS < 4 || KS % 4 || RT <= 0 || !kcol) return;
  for (int rt = 0; rt < RT; ++rt) {
    const int ot = tmap ? tmap[rt] : rt;
    for (int r = 0; r < 4; ++r)
      if (kcol[(size_t)rt * KS + KS - 4 + r] != 16 * ot + 4 * r) return;
  }
  op.bsr_diag_last = true;
}

static int free_op(sw_engine* h, EllOp& op) {
  SWCHK(dev_free(h, op.cols));
  SWCHK(dev_free(h, op.vals));
  SWCHK(dev_free(h, op.order));
  SWCHK(dev_free(h, op.order_even));
  SWCHK(dev_free(h, op.bsr_kcol));
  SWCHK(dev_free(h, op.bsr_vals));
  SWCHK(dev_free(h, op.bsr_tmap));
  SWCHK(dev_free(h, op.vals32));
  SWCHK(dev_free(h, op.bsr_vals32));
  op = EllOp();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// kernel launch wrappers
// ---------------------------------------------------------------------------------------------
static int launch_bsr(sw_engine* h, const EllOp& op, int mode, const cplx* X, const cplx* B, cplx* Y,
                      int nbp, int cat, cplx w) {
  const int RT = op.bsr_RT > 0 ? op.bsr_RT : op.nrows / 16;
  // MFMA column tiles per wave (8 probes each).  Small operators (a 4096-row level on 256 probes is
  // 2048 waves at NT = 4, two per SIMD once) are latency-bound: fewer tiles per wave = more waves
  int NT = h->mfma_tiles;
  if (h->mfma_small_tiles > 0 && (long long)RT * ((2 * nbp) / (16 * NT)) < 4096)
    NT = h->mfma_small_tiles;
  const int bmap = (cat == T_COARSEST) ? h->dense_map : h->bsr_map, msub = h->bsr_sub;
  const int RBn = (RT + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK, NCn = (2 * nbp) / (16 * NT);
  const int want = (cat == T_COARSEST) ? h->dense_stages : h->bsr_stages;
  const int stages = (want >= 8 && op.bsr_KS % 8 == 0) ? 8 : ((want >= 4 && op.bsr_KS % 4 == 0) ? 4 : 2);
  dim3 grid = (bmap == 0) ? dim3(RBn, NCn) : dim3(RBn * NCn);
  // level-1 operator of the solver hierarchy vs. the smaller operators below it (separate stats)
  const int n1 = h->hier[h->solver_hid].nlevels > 1 ? h->hier[h->solver_hid].lv[1].n : 0;
  const int cls = cat == T_COARSEST ? T_MFMA_DENSE
                                    : (cat == T_MVM ? (op.nrows == n1 || n1 == 0 ? T_MFMA_OP : T_MFMA_OP2)
                                                    : cat);
  // 16 rows x 4 columns x nbp probes x 8 flops per complex multiply-add, per (tile, k-step)
  if (h->profiling) h->twork[cls] += 512.0 * (double)RT * (double)op.bsr_KS * (double)nbp;
  const int dl_kb = 4;     // k-steps per LDS stage (8 measured 135.1 us against 136.4: barriers are not the bound)
  if (h->mfma_3m && h->dense_lds > 0 && cat == T_COARSEST && mode == 0 && op.dense_uniform &&
      RT % h->dense_lds == 0 && op.bsr_KS % (dl_kb * SW_DL_DEPTH) == 0 && op.bsr_KS >= 2 * dl_kb * SW_DL_DEPTH &&
      (nbp & 31) == 0 && X != Y) {
    // dense operator: operands shared through LDS (register-staged, double-buffered), one workgroup per
    // (16 dense_lds)-row x 32-probe block -- 1 KiB (0.75 KiB) per wave and k-step through the L2 -> CU path
    // instead of 2
    return pick<4, 2>(h->dense_lds, [&](auto RTW) {
      return launch(h, cls, swk::k_dense_mfma3_lds<RTW, dl_kb>, dim3((RT / RTW) * (nbp / 32)), dim3(128 * RTW),
                    (const cplx*)op.bsr_vals, (const int*)op.bsr_kcol, op.bsr_KS, RT, X, Y, nbp,
                    (const int*)op.bsr_tmap);
    });
  }
  if (h->mfma_3m) {
    // three real products per complex one (k_bsr_mfma3): tiles of 16 probes per wave
    // Measured (gpurun_out r03d): one tile of 16 probes per wave wins wherever it was compared -- the
    // dense 2048^2 Schur inverse 138 us against 234 (two tiles) and 391 (four): more tiles mean more
    // stage registers (204 + 106 at two tiles and eight stages: one wave per SIMD), and the kernel lives on
    // two or three co-resident waves hiding each other's L1 round trips.  Larger level operators (lattices
    // beyond 128^2) keep two tiles per wave when they have the waves to spare.
    int NT3 = 1;
    if (cat != T_COARSEST && (long long)RT * (nbp / 32) >= 16384) NT3 = 2;
    if (h->mfma3_tiles == 1 || h->mfma3_tiles == 2 || h->mfma3_tiles == 4) NT3 = h->mfma3_tiles;
    while (NT3 > 1 && nbp % (16 * NT3)) NT3 >>= 1;
    const int NC3 = nbp / (16 * NT3);
    const dim3 grid3(RBn * NC3);
    const bool ntio3 = h->bsr_nt && cat != T_COARSEST;
    const int xr = (op.bsr_diag_last && h->bsr_xreg) ? 1 : 0;
    const int bm3 = (bmap == 0) ? 0 : bmap;
    auto b3 = [&](auto MD, auto NTT, auto NTB, auto SG) {
      return launch(h, cls, swk::k_bsr_mfma3<MD, NTT, NTB, SG>, grid3, dim3(SW_BLOCK), (const cplx*)op.bsr_vals,
                    (const int*)op.bsr_kcol, op.bsr_KS, RT, X, B, Y, nbp, w, bm3, msub, (const int*)op.bsr_tmap, xr);
    };
    if (!ntio3 && mode == 0 && want >= 16 && NT3 == 1 && op.bsr_KS % 16 == 0)
      return b3(IntC<0>{}, IntC<1>{}, IntC<0>{}, IntC<16>{});
    if (!ntio3 && mode == 0 && want >= 8)
      return pick<4, 2, 1>(NT3, [&](auto NTT) { return b3(IntC<0>{}, NTT, IntC<0>{}, IntC<8>{}); });
    return pick<0, 1, 3>(mode, [&](auto MD) {
      return pick<4, 2, 1>(NT3, [&](auto NTT) {
        return pick<0, 1>(ntio3, [&](auto NTB) { return b3(MD, NTT, NTB, IntC<4>{}); });
      });
    });
  }
  const bool ntio = h->bsr_nt && cat != T_COARSEST;
  const int xr = (op.bsr_diag_last && h->bsr_xreg) ? 1 : 0;
  return pick<0, 1, 3>(mode, [&](auto MD) {
    return pick<2, 4>(NT, [&](auto NTT) {
      return pick<0, 1>(ntio, [&](auto NTB) {
        return pick<8, 4, 2>(stages, [&](auto SG) {
          return launch(h, cls, swk::k_bsr_mfma<MD, NTT, NTB, SG>, grid, dim3(SW_BLOCK), (const cplx*)op.bsr_vals,
                        (const int*)op.bsr_kcol, op.bsr_KS, RT, (const double*)X, (const double*)B, (double*)Y,
                        2 * nbp, nbp, w, bmap, msub, (const int*)op.bsr_tmap, xr);
        });
      });
    });
  });
}

// The grouped-ELL kernel of an operator (T = cplx: fp64 values, cplxf: their complex64 mirror).  even_only:
// write the rows of the even sites only (prolongation before an even-odd smoother)
template <class T>
static int launch_ell_groups(sw_engine* h, const EllOp& op, const T* vals, int mode, const T* X, const T* B, T* Y,
                             int nbp, int cat, T w, bool even_only) {
  const bool ev = even_only && op.order_even && h->p_even;
  const int ng = ev ? op.ngroups_even : op.ngroups;
  const int* ord = ev ? op.order_even : (h->ell_order ? op.order : nullptr);
  const dim3 grid((ng + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK, nbp / 64);
  if (op.G != 1 && op.G != 2 && op.G != 4 && op.G != 8 && op.G != 16)
    return sw_fail(h, "unsupported ELL group size %d", op.G);
  return pick<1, 2, 4, 8, 16>(op.G, [&](auto G) {
    return pick<0, 1, 2, 3>(mode, [&](auto MODE) {
      return launch(h, cat, swk::k_ell<G, MODE, T>, grid, dim3(SW_BLOCK), (const int*)op.cols, vals, op.K, ng, ord,
                    X, B, Y, nbp, w);
    });
  });
}

static int launch_ell(sw_engine* h, const EllOp& op, int mode, const cplx* X, const cplx* B,
                      cplx* Y, int nbp, int cat, cplx w = cplx{0.0, 0.0}, bool even_only = false) {
  if (!op.set) return sw_fail(h, "operator not set");
  if (op.bsr_KS > 0 && (mode == 0 || mode == 1 || mode == 3) && h->use_mfma &&
      (cat == T_COARSEST || h->mfma_ops))
    return launch_bsr(h, op, mode, X, B, Y, nbp, cat, w);
  if (!op.cols || !op.vals)
    return sw_fail(h, "operator exists in MFMA block-row form only (built on the device): it needs "
                      "use_mfma = mfma_ops = 1");
  return launch_ell_groups<cplx>(h, op, op.vals, mode, X, B, Y, nbp, cat, w, even_only);
}

static int launch_bsr(sw_engine* h, const EllOp& op, int mode, const cplx* X, const cplx* B, cplx* Y,
                      int nbp, int cat, cplx w);
static int ensure_level_ws(sw_engine* h, Level& lv, int nbp);

// Y = coarsest_inv X : fp64 MFMA block-row kernel when the size allows, grouped-ELL otherwise.
// A coarsest level that carries the even-odd operators and the dense inverse of its Schur complement
// (sw_set_eo_operator 0..3 + sw_setup_direct_level) is solved in even-odd form instead -- the same exact
// solve at a quarter of the dense flops: b'_e = b_e - F b_o ; x_e = S^-1 b'_e ; x_o = G b_o - Hb x_e
// (X and Y must be different arrays; the level's residual buffer is the scratch for b').
static int apply_coarsest(sw_engine* h, Hier& H, const cplx* X, cplx* Y, int nbp) {
  Level& lc = H.lv[H.nlevels - 1];
  if (h->eo_direct && H.nlevels > 1 && lc.eo_op[4].set && lc.eo_op[1].set && lc.eo_op[2].set &&
      lc.eo_op[3].set && X != Y) {
    SWCHK(ensure_level_ws(h, lc, nbp));
    SWCHK(launch_bsr(h, lc.eo_op[1], 1, X, X, lc.r, nbp, T_MVM, cplx{0.0, 0.0}));
    SWCHK(launch_bsr(h, lc.eo_op[4], 0, lc.r, nullptr, Y, nbp, T_COARSEST, cplx{0.0, 0.0}));
    SWCHK(launch_bsr(h, lc.eo_op[2], 0, X, nullptr, Y, nbp, T_MVM, cplx{0.0, 0.0}));
    return launch_bsr(h, lc.eo_op[3], 1, Y, Y, Y, nbp, T_MVM, cplx{0.0, 0.0});
  }
  if (!H.cinv.set) return sw_fail(h, "coarsest inverse not set");
  return launch_ell(h, H.cinv, 0, X, nullptr, Y, nbp, T_COARSEST);
}

static int stencil_spw(sw_engine* h, int tile_w) {
  // consecutive x-sites per wave (must divide the tile width)
  // measured (profiles/r01_stencil_tiles.txt): one site per wave keeps the most independent
  // loads in flight and beats the register sliding window (SPW 2/4/8) at every lattice size
  int spw = h->stencil_spw > 0 ? h->stencil_spw : 1;
  while (spw > 1 && tile_w % spw) spw >>= 1;
  return spw;
}

// Arguments of the stencil kernels of the lattice level (w = 0).  x-tile: whole rows while three of them
// (2 KiB per site and 64-probe chunk; the even-odd kernels: five rows of half the sites) fit well inside a
// 4-MiB L2, otherwise 256-site (or 64-site) tiles: 3.6 -> 4.6 TB/s on 1024^2; option stencil_tile where it
// divides L.  eo: the even-odd kernels (k_schur_step, k_eo_hop), which need an even tile and store with
// temporal stores.  C = complex64 (cplxf, or cplxf2: two probes per element): the complex64 links and
// diagonal, rows of nbp / (probes per element) elements.
template <class C>
static swk::StencilArgsT<C> stencil_args(sw_engine* h, const Level& lv, int nbp, bool eo) {
  using S = typename swk::scalar_of<C>::type;
  swk::StencilArgsT<C> a;
  a.L = lv.L;
  a.Vh = lv.L * lv.L / 2;
  a.diag = (typename swk::real_of<C>::type)(4.0 + lv.mass);
  if constexpr (std::is_same<C, cplx>::value) {
    a.U1 = lv.U1;
    a.U2 = lv.U2;
  } else {
    a.U1 = lv.U1f;
    a.U2 = lv.U2f;
  }
  a.nbp = nbp / (int)(sizeof(C) / sizeof(S));
  a.w.x = 0;
  a.w.y = 0;
  a.nt_store = (!eo && h->stencil_nt) ? 1 : 0;
  a.tile_w = lv.L;
  if (lv.L > 256) a.tile_w = (lv.L % 256 == 0) ? 256 : ((lv.L % 64 == 0) ? 64 : lv.L);
  if (h->stencil_tile > 0 && lv.L % h->stencil_tile == 0 && (!eo || h->stencil_tile % 2 == 0))
    a.tile_w = h->stencil_tile;
  return a;
}

// the Wilson stencil of the lattice level; CI = complex64: X is a direction stored by the
// single-precision preconditioner (mode 0 only), widened on load
template <class CI, class CO>
static int launch_stencil(sw_engine* h, Level& lv, int mode, const CI* X, const cplx* B, CO* Y,
                          int nbp, cplx w) {
  swk::StencilArgs a = stencil_args<cplx>(h, lv, nbp, false);
  a.w = w;
  const int spw = stencil_spw(h, a.tile_w);
  const int V = lv.L * lv.L;
  const int waves = V / spw;
  const int bpc = (waves + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK;
  const int nchunks = nbp / 64;
  const int cat = mode == 0 ? T_STENCIL : (mode == 1 ? T_STENCIL_RES : T_STENCIL_SM);
  return pick<8, 4, 2, 1>(spw, [&](auto SP) {
    auto go = [&](auto MD) {
      return launch(h, cat, swk::k_stencil<MD, SP, CI, CO>, dim3(bpc * nchunks), dim3(SW_BLOCK), X, B, Y, a, bpc);
    };
    if (mode == 0) return go(IntC<0>{});
    if constexpr (std::is_same<CI, cplx>::value && std::is_same<CO, cplx>::value)
      return pick<1, 2>(mode, go);
    else
      return sw_fail(h, "internal: complex64 stencil input supports Y = A X only");
  });
}

// Y = A X (mode 0), Y = B - A X (mode 1) or Y = X + w (B - A X) (mode 2) at a level
static int apply_op(sw_engine* h, Level& lv, int mode, const cplx* X, const cplx* B, cplx* Y,
                    int nbp, cplx w = cplx{0.0, 0.0}) {
  if (lv.stencil) return launch_stencil<cplx, cplx>(h, lv, mode, X, B, Y, nbp, w);
  return launch_ell(h, lv.A, mode == 2 ? 3 : mode, X, B, Y, nbp, T_MVM, w);
}

// Workgroups of a reducing BLAS-1 launch (row blocks x probe chunks; option dot_blocks).  Round 1's cap of
// 128 row blocks left a 64-probe batch on a 1024^2 lattice with 512 waves for 2 M rows: 1024 blocks took
// its inner products from 61.7 to 20.7 ms and the fused-norm updates from 61.7 to 30.2 ms per batch
// (165 -> 214 probe-samples/s); beyond ~1500 the second reduction stage grows faster than the first shrinks.
// With four or more probe chunks 128 row blocks already make 512+ workgroups, and the second stage
// (k_reduce_partials: 5 us at 128 partials, 17 us at 256) would eat what the first gains.
static void row_blocking(int n, int nbp, bool reduce, int* P, int* rpb) {
  const int nchunks = nbp / 64;
  int p;
  if (reduce) {
    p = std::max(8, std::min(g_dot_pmax, g_dot_blocks / std::max(1, nchunks)));
    if (nchunks >= 4 && g_dot_pmax == 1024) p = std::min(p, 128);
  } else {
    p = std::max(8, 4096 / std::max(1, nchunks));
  }
  int r = (n + p - 1) / p;
  if (r < SW_WAVES_PER_BLOCK) r = SW_WAVES_PER_BLOCK;
  *rpb = r;
  *P = (n + r - 1) / r;
}

// Reduction bookkeeping of the reducing BLAS-1 launches.  fused_reduce (default): the cross-workgroup
// sum is completed inside the launch (last block done, two levels: swk::reduce_and_tail) and an FGMRES
// scalar update (`tail`) may ride along; otherwise a second launch (k_reduce_partials) and, for a tail,
// a third (k_fg_tail).
static const swk::FgTail kNoTail = [] { swk::FgTail t{}; t.kind = SW_TAIL_NONE; return t; }();

static bool fused_ok(sw_engine* h, int P, int nbp) {
  return h->fused_reduce && h->d_tick && nbp / 64 <= SW_TICKET_CHUNKS &&
         (P + SW_RED_GROUP - 1) / SW_RED_GROUP <= SW_RED_MAXGROUPS;
}
static swk::RedArgs red_args(sw_engine* h, bool fused, int P, int K, int nbp, cplx* out, const cplx* svec,
                             cplx* coef) {
  swk::RedArgs ra{};
  if (fused) {
    ra.tick1 = h->d_tick;
    ra.tick2 = h->d_tick + SW_TICKET_CHUNKS * SW_RED_MAXGROUPS;
    ra.gpart = h->partial + (size_t)P * K * nbp;
    ra.out = out;
    ra.svec = svec;
    ra.coef = coef;
  }
  return ra;
}
static int launch_tail(sw_engine* h, const swk::FgTail& tail) {
  const int nbp = tail.s.nbp, tb = 256;
  return launch(h, T_OTHER, swk::k_fg_tail, dim3((nbp + tb - 1) / tb), dim3(tb), tail);
}

// out[k][col] = sum_r conj(V_k[r]) W[r],  k < K
template <class CV>
static int multidot(sw_engine* h, const swk::PtrListT<CV>& V, int K, const CV* W, int n, int nbp,
                    cplx* out, const cplx* svec = nullptr, cplx* coef = nullptr,
                    const swk::FgTail* tail = nullptr) {
  if (K < 1 || K > SW_MAXM + 2) return sw_fail(h, "multidot: K=%d out of range", K);
  int P, rpb;
  row_blocking(n, nbp, true, &P, &rpb);
  const int ngroups = (P + SW_RED_GROUP - 1) / SW_RED_GROUP;
  SWCHK(ensure_partial(h, (size_t)(P + ngroups) * K * nbp * sizeof(cplx)));
  const bool fused = fused_ok(h, P, nbp);
  const swk::RedArgs ra = red_args(h, fused, P, K, nbp, out, svec, coef);
  const swk::FgTail tl = (fused && tail) ? *tail : kNoTail;
  dim3 grid(P, nbp / 64);
  SWCHK(pick_ge<2, 4, 8, 16, 24, 34>(K, [&](auto KT) {
    return launch(h, T_DOTS, swk::k_multidot<KT, CV>, grid, dim3(SW_BLOCK), V, K, W, n, nbp, rpb, h->partial, ra,
                  tl);
  }));
  if (fused) return 0;
  SWCHK(launch(h, T_DOTS, swk::k_reduce_partials, dim3(K, nbp / 64), dim3(SW_BLOCK), h->partial, P, K, nbp, out,
               svec, coef));
  if (tail) SWCHK(launch_tail(h, *tail));
  return 0;
}

// out[k][col] = u_a^H u_b for all pairs a <= b of NV vectors (k = a NV - a (a-1)/2 + (b-a)) in one pass;
// the reduction is completed in the launch and `tail` (the Gram-cycle update) applied
static int multigram(sw_engine* h, const PtrList& U, int NV, int n, int nbp, cplx* out, const swk::FgTail* tail) {
  if (NV < 2 || NV > SW_GRAM_MAXL + 1) return sw_fail(h, "multigram: %d vectors out of range", NV);
  const int K = NV * (NV + 1) / 2;
  int P, rpb;
  row_blocking(n, nbp, true, &P, &rpb);
  const int ngroups = (P + SW_RED_GROUP - 1) / SW_RED_GROUP;
  SWCHK(ensure_partial(h, (size_t)(P + ngroups) * K * nbp * sizeof(cplx)));
  if (!fused_ok(h, P, nbp)) return sw_fail(h, "internal: the Gram cycle needs the in-launch reductions");
  const swk::RedArgs ra = red_args(h, true, P, K, nbp, out, nullptr, nullptr);
  const swk::FgTail tl = tail ? *tail : kNoTail;
  dim3 grid(P, nbp / 64);
  return pick<2, 3, 4, 5>(NV, [&](auto NN) {
    return launch(h, T_DOTS, swk::k_gram<NN>, grid, dim3(SW_BLOCK), U, n, nbp, rpb, h->partial, ra, tl);
  });
}

// Wout = Win + sign * sum_k coef[k] V_k ; optional nrm[col].x = ||Wout||^2
template <class CV, class CW>
static int multiaxpy(sw_engine* h, const swk::PtrListT<CV>& V, int K, const cplx* coef, double sign,
                     const CW* Win, CW* Wout, int n, int nbp, cplx* nrm_out,
                     cplxf* w32 = nullptr, const swk::FgTail* tail = nullptr) {
  if (K < 1 || K > SW_MAXM + 2) return sw_fail(h, "multiaxpy: K=%d out of range", K);
  if (tail && !nrm_out) return sw_fail(h, "internal: a reduction tail needs the fused norm");
  int P, rpb;
  row_blocking(n, nbp, nrm_out != nullptr, &P, &rpb);
  const int ngroups = (P + SW_RED_GROUP - 1) / SW_RED_GROUP;
  if (nrm_out) SWCHK(ensure_partial(h, (size_t)(P + ngroups) * nbp * sizeof(cplx)));
  const bool fused = nrm_out && fused_ok(h, P, nbp);
  const swk::RedArgs ra = red_args(h, fused, P, 1, nbp, nrm_out, nullptr, nullptr);
  const swk::FgTail tl = (fused && tail) ? *tail : kNoTail;
  dim3 grid(P, nbp / 64);
  SWCHK(pick_ge<2, 4, 8, 16, 24, 34>(K, [&](auto KT) {
    if (nrm_out)
      return launch(h, T_AXPY, swk::k_multiaxpy<KT, true, CV, CW>, grid, dim3(SW_BLOCK), V, K, coef, sign, Win, Wout,
                    n, nbp, rpb, h->partial, w32, ra, tl);
    return launch(h, T_AXPY, swk::k_multiaxpy<KT, false, CV, CW>, grid, dim3(SW_BLOCK), V, K, coef, sign, Win, Wout,
                  n, nbp, rpb, h->partial, w32, ra, tl);
  }));
  if (nrm_out && !fused) {
    SWCHK(launch(h, T_DOTS, swk::k_reduce_partials, dim3(1, nbp / 64), dim3(SW_BLOCK), h->partial, P, 1, nbp,
                 nrm_out, (const cplx*)nullptr, (cplx*)nullptr));
  }
  if (tail && !fused) SWCHK(launch_tail(h, *tail));
  return 0;
}

static int zero_vec(sw_engine* h, cplx* p, int n, int nbp) {
  LaunchScope ls(h, T_AXPY);
  HIPCHK(hipMemsetAsync(p, 0, (size_t)n * nbp * sizeof(cplx), h->stream));
  return 0;
}
static int copy_vec(sw_engine* h, cplx* dst, const cplx* src, int n, int nbp) {
  LaunchScope ls(h, T_AXPY);
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)n * nbp * sizeof(cplx), hipMemcpyDeviceToDevice,
                        h->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------------
// workspaces
// ---------------------------------------------------------------------------------------------
static int ensure_small(sw_engine* h, int nbp) {
  const size_t need = (size_t)(SW_MAX_DEFL + 8) * nbp * sizeof(cplx);
  if (h->small_bytes >= need) return 0;
  if (h->small) SWCHK(dev_free(h, h->small));
  h->small = nullptr;
  void* q;
  SWCHK(dev_alloc(h, &q, need));
  h->small = (cplx*)q;
  h->small_bytes = need;
  return 0;
}

static int ensure_level_ws(sw_engine* h, Level& lv, int nbp) {
  if (lv.ws_nbp == nbp && lv.b) return 0;
  const size_t cnt = (size_t)lv.n * nbp;
  SWCHK(dev_realloc(h, &lv.b, cnt));
  SWCHK(dev_realloc(h, &lv.x, cnt));
  SWCHK(dev_realloc(h, &lv.r, cnt));
  SWCHK(dev_realloc(h, &lv.t, cnt));
  lv.ws_nbp = nbp;
  return 0;
}

static int free_krylov(sw_engine* h, KrylovWS& w) {
  SWCHK(dev_free(h, w.V)); w.V = nullptr;
  SWCHK(dev_free(h, w.Z)); w.Z = nullptr;
  SWCHK(dev_free(h, w.Z32)); w.Z32 = nullptr;
  SWCHK(dev_free(h, w.v32)); w.v32 = nullptr;
  SWCHK(dev_free(h, w.V32)); w.V32 = nullptr;
  SWCHK(dev_free(h, w.xacc)); w.xacc = nullptr;
  SWCHK(dev_free(h, w.rres)); w.rres = nullptr;
  SWCHK(dev_free(h, w.sc.H)); w.sc.H = nullptr;
  SWCHK(dev_free(h, w.sc.cs)); w.sc.cs = nullptr;
  SWCHK(dev_free(h, w.sc.sn)); w.sc.sn = nullptr;
  SWCHK(dev_free(h, w.sc.g)); w.sc.g = nullptr;
  SWCHK(dev_free(h, w.sc.y)); w.sc.y = nullptr;
  SWCHK(dev_free(h, w.sc.normb)); w.sc.normb = nullptr;
  SWCHK(dev_free(h, w.sc.relres)); w.sc.relres = nullptr;
  SWCHK(dev_free(h, w.sc.svec)); w.sc.svec = nullptr;
  SWCHK(dev_free(h, w.sc.ys)); w.sc.ys = nullptr;
  SWCHK(dev_free(h, w.c1)); w.c1 = nullptr;
  SWCHK(dev_free(h, w.sc.iters)); w.sc.iters = nullptr;
  SWCHK(dev_free(h, w.h1)); w.h1 = nullptr;
  SWCHK(dev_free(h, w.h2)); w.h2 = nullptr;
  SWCHK(dev_free(h, w.nrm)); w.nrm = nullptr;
  SWCHK(dev_free(h, w.gram)); w.gram = nullptr;
  w.m = w.n = w.nbp = 0;
  return 0;
}

static int ensure_krylov(sw_engine* h, KrylovWS& w, int m, int n, int nbp, bool outer) {
  if (w.m == m && w.n == n && w.nbp == nbp && w.V) return 0;
  SWCHK(free_krylov(h, w));
  const size_t vec = (size_t)n * nbp;
  SWCHK(dev_realloc(h, &w.V, vec * m));
  SWCHK(dev_realloc(h, &w.Z, vec * m));
  if (outer) {
    SWCHK(dev_realloc(h, &w.xacc, vec));
    SWCHK(dev_realloc(h, &w.rres, vec));
  }
  SWCHK(dev_realloc(h, &w.sc.H, (size_t)(m + 1) * m * nbp));
  SWCHK(dev_realloc(h, &w.sc.cs, (size_t)m * nbp));
  SWCHK(dev_realloc(h, &w.sc.sn, (size_t)m * nbp));
  SWCHK(dev_realloc(h, &w.sc.g, (size_t)(m + 1) * nbp));
  SWCHK(dev_realloc(h, &w.sc.y, (size_t)m * nbp));
  SWCHK(dev_realloc(h, &w.sc.normb, (size_t)nbp));
  SWCHK(dev_realloc(h, &w.sc.relres, (size_t)nbp));
  SWCHK(dev_realloc(h, &w.sc.svec, (size_t)(m + 1) * nbp));
  SWCHK(dev_realloc(h, &w.sc.ys, (size_t)m * nbp));
  SWCHK(dev_realloc(h, &w.c1, (size_t)(m + 2) * nbp));
  SWCHK(dev_realloc(h, &w.sc.iters, (size_t)nbp));
  SWCHK(dev_realloc(h, &w.h1, (size_t)(m + 2) * nbp));
  SWCHK(dev_realloc(h, &w.h2, (size_t)(m + 2) * nbp));
  SWCHK(dev_realloc(h, &w.nrm, (size_t)nbp));
  SWCHK(dev_realloc(h, &w.gram, (size_t)((SW_GRAM_MAXL + 1) * (SW_GRAM_MAXL + 2) / 2) * nbp));
  w.sc.m = m;
  w.sc.nbp = nbp;
  w.m = m;
  w.n = n;
  w.nbp = nbp;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// the multigrid cycle (MG.one_mg_step, multigrid.py:369-447) with MR(nu) smoothing
// ---------------------------------------------------------------------------------------------
static int fgmres(sw_engine* h, Hier& H, int level, const cplx* B, cplx* X, double tol, int maxiter,
                  int m, bool outer, KrylovWS& ws, int nbp, int* iters_total,
                  bool use_precond = true, const cplx* aug = nullptr);

// The system a flexible GMRES iterates on (fgmres_loop, gram_cycle): the full system of a level
// (full_system) or the even-odd reduced system of the stencil level (reduced_system)
struct KrylovSys {
  int n = 0;                                                        // vector length
  std::function<int(int mode, const cplx* x, const cplx* b, cplx* y)> apply;   // y = A x (mode 0), b - A x (1)
  std::function<int(const cplx* v, cplx* z)> precond;               // z = M v (empty: no preconditioner)
  // complex64 directions (precond32 empty: none): z = M v, then w = A z into a complex64 basis (op32, option
  // f32_krylov) or into the fp64 basis (op32w)
  std::function<int(const cplxf* v, cplxf* z)> precond32;
  std::function<int(const cplxf* z, cplxf* w)> op32;
  std::function<int(const cplxf* z, cplx* w)> op32w;
  bool normb_set = false;   // ||b|| of the stopping criterion was fixed by the caller (tail_begin)
};
static KrylovSys full_system(sw_engine* h, Hier& H, int level, int nbp, bool use_precond, bool outer);

// nu MR steps on (X, R) with R = B - A X maintained
static int mr_smooth(sw_engine* h, Level& lv, cplx* X, cplx* R, int nu, int nbp) {
  SWCHK(ensure_small(h, nbp));
  cplx* d = h->small;                // [2][nbp]
  cplx* alpha = h->small + 2 * nbp;  // [nbp]
  for (int s = 0; s < nu; ++s) {
    SWCHK(apply_op(h, lv, 0, R, nullptr, lv.t, nbp));
    PtrList pl;
    pl.p[0] = R;
    pl.p[1] = lv.t;
    SWCHK(multidot(h, pl, 2, lv.t, lv.n, nbp, d));
    SWCHK(launch(h, T_DOTS, swk::k_mr_alpha, dim3((nbp + 255) / 256), dim3(256), d, nbp, alpha));
    int P, rpb;
    row_blocking(lv.n, nbp, false, &P, &rpb);
    SWCHK(launch(h, T_AXPY, swk::k_mr_update, dim3(P, nbp / 64), dim3(SW_BLOCK), alpha, X, R, lv.t, lv.n, nbp,
                 rpb));
  }
  return 0;
}

// n fixed-weight Richardson steps  x <- x + w_k (B - A x), ping-ponging between `cur`
// (holding x on entry, ignored when from_zero) and `other`; *result = buffer with the answer
static int rich_steps(sw_engine* h, Level& lv, const cplx* Bin, cplx* cur, cplx* other,
                      const std::vector<std::complex<double>>& w, bool from_zero, int nbp,
                      cplx** result) {
  size_t k = 0;
  if (from_zero && !w.empty()) {
    const size_t count = (size_t)lv.n * nbp;
    SWCHK(launch(h, T_AXPY, swk::k_cscale, dim3(2048), dim3(SW_BLOCK), cplx{w[0].real(), w[0].imag()}, Bin, cur,
                 count));
    k = 1;
  }
  for (; k < w.size(); ++k) {
    SWCHK(apply_op(h, lv, 2, cur, Bin, other, nbp, cplx{w[k].real(), w[k].imag()}));
    std::swap(cur, other);
  }
  *result = cur;
  return 0;
}

static int vcycle_rich(sw_engine* h, Hier& H, int l, const cplx* Bin, cplx* Xout, int nbp);

static int vec_add(sw_engine* h, const cplx* a, const cplx* b, cplx* dst, int n, int nbp) {
  return launch(h, T_AXPY, swk::k_add, dim3(2048), dim3(SW_BLOCK), a, b, dst, (size_t)n * nbp);
}

// E = gm_cycles x GMRES(gm_m) applied to A_l e = R from a zero guess (unpreconditioned).  With two cycles
// and option lgmres_aug (default) the second cycle is LGMRES's: its search space is augmented by the
// first cycle's correction, as SciPy's lgmres(maxiter=2, inner_m=30, outer_k=3) does at
// multigrid.py:393-394,438-439 (the first outer iteration has nothing to augment with).
static int gmres_smooth(sw_engine* h, Hier& H, int l, const cplx* R, cplx* E, int nbp) {
  Level& lv = H.lv[l];
  const int m = lv.gm_m;
  const bool lg = h->lgmres_aug && lv.gm_cycles == 2 && m + 1 <= SW_MAXM;
  SWCHK(ensure_krylov(h, lv.gws, lg ? m + 1 : m, lv.n, nbp, false));
  SWCHK(fgmres(h, H, l, R, E, 0.0, m, m, false, lv.gws, nbp, nullptr, false));
  for (int c = 1; c < lv.gm_cycles; ++c) {
    SWCHK(apply_op(h, lv, 1, E, R, lv.g1, nbp));                       // g1 = R - A E
    SWCHK(fgmres(h, H, l, lv.g1, lv.g2, 0.0, m, m, false, lv.gws, nbp, nullptr, false, lg ? E : nullptr));
    SWCHK(vec_add(h, E, lv.g2, E, lv.n, nbp));
  }
  return 0;
}

static int vcycle(sw_engine* h, Hier& H, int l, const cplx* Bin, cplx* Xout, int nbp);

// MG.one_mg_step as written (multigrid.py:369-447): smooth, residual, restrict, recurse, prolong,
// residual, smooth -- with the GMRES(m) x cycles smoother above in place of lgmres(maxiter=2)
static int vcycle_gmres(sw_engine* h, Hier& H, int l, const cplx* Bin, cplx* Xout, int nbp) {
  Level& lv = H.lv[l];
  Level& lc = H.lv[l + 1];
  SWCHK(ensure_level_ws(h, lv, nbp));
  SWCHK(ensure_level_ws(h, lc, nbp));
  if (!lv.P.set || !lv.R.set) return sw_fail(h, "transfer operators of level %d not set", l);
  if (!lv.g1 || lv.gws.nbp != nbp) {
    SWCHK(dev_realloc(h, &lv.g1, (size_t)lv.n * nbp));
    SWCHK(dev_realloc(h, &lv.g2, (size_t)lv.n * nbp));
  }
  SWCHK(gmres_smooth(h, H, l, Bin, Xout, nbp));                         // :388-399  (x = 0 + e)
  SWCHK(apply_op(h, lv, 1, Xout, Bin, lv.r, nbp));                      // :402
  SWCHK(launch_ell(h, lv.R, 0, lv.r, nullptr, lc.b, nbp, T_R));         // :406
  SWCHK(vcycle(h, H, l + 1, lc.b, lc.x, nbp));                          // :413-416 at the coarsest
  SWCHK(launch_ell(h, lv.P, 2, lc.x, Xout, Xout, nbp, T_P));            // :429
  SWCHK(apply_op(h, lv, 1, Xout, Bin, lv.r, nbp));                      // :433
  SWCHK(gmres_smooth(h, H, l, lv.r, lv.t, nbp));                        // :438
  return vec_add(h, Xout, lv.t, Xout, lv.n, nbp);                       // :444
}

static int vcycle(sw_engine* h, Hier& H, int l, const cplx* Bin, cplx* Xout, int nbp) {
  if (l < H.nlevels - 1 && H.lv[l].gm_m > 0) return vcycle_gmres(h, H, l, Bin, Xout, nbp);
  if (l < H.nlevels - 1 && H.lv[l].rich) return vcycle_rich(h, H, l, Bin, Xout, nbp);
  const int last = H.nlevels - 1;
  if (l == last) {
    return apply_coarsest(h, H, Bin, Xout, nbp);
  }
  Level& lv = H.lv[l];
  Level& lc = H.lv[l + 1];
  SWCHK(ensure_level_ws(h, lv, nbp));
  SWCHK(ensure_level_ws(h, lc, nbp));
  if (!lv.P.set || !lv.R.set) return sw_fail(h, "transfer operators of level %d not set", l);
  const bool pre = lv.nu_pre > 0;
  if (pre) {
    SWCHK(zero_vec(h, Xout, lv.n, nbp));
    SWCHK(copy_vec(h, lv.r, Bin, lv.n, nbp));
    SWCHK(mr_smooth(h, lv, Xout, lv.r, lv.nu_pre, nbp));
    SWCHK(launch_ell(h, lv.R, 0, lv.r, nullptr, lc.b, nbp, T_R));
  } else {
    SWCHK(launch_ell(h, lv.R, 0, Bin, nullptr, lc.b, nbp, T_R));
  }
  if (lv.kcycle > 0 && l + 1 < last) {
    SWCHK(ensure_krylov(h, lc.kws, lv.kcycle, lc.n, nbp, false));
    SWCHK(fgmres(h, H, l + 1, lc.b, lc.x, 0.0, lv.kcycle, lv.kcycle, false, lc.kws, nbp, nullptr));
  } else {
    SWCHK(vcycle(h, H, l + 1, lc.b, lc.x, nbp));
  }
  if (pre) SWCHK(launch_ell(h, lv.P, 2, lc.x, Xout, Xout, nbp, T_P));
  else SWCHK(launch_ell(h, lv.P, 0, lc.x, nullptr, Xout, nbp, T_P));
  if (lv.nu_post > 0) {
    SWCHK(apply_op(h, lv, 1, Xout, Bin, lv.r, nbp));
    SWCHK(mr_smooth(h, lv, Xout, lv.r, lv.nu_post, nbp));
  }
  return 0;
}

// Even-site group lists of the prolongators of the even-odd smoothed levels (rebuilt after any
// operator of the hierarchy changed).  Lattice level: rows are parity-sorted, the even sites are the
// first half; block levels: the 16-row tiles named by the tile map of the Schur operator.
static int ensure_even_orders(sw_engine* h, Hier& H) {
  if (H.even_valid) return 0;
  for (int l = 0; l < H.nlevels - 1; ++l) {
    Level& lv = H.lv[l];
    EllOp& P = lv.P;
    SWCHK(dev_free(h, P.order_even));
    P.order_even = nullptr;
    P.ngroups_even = 0;
    SWCHK(free_op(h, lv.Re));
    if (lv.stencil && !lv.w_eo.empty() && lv.R.set && lv.R.cols && lv.R.vals) {
      // R restricted to the columns of the even sites (the first n / 2 rows of the level), compacted:
      // the restriction of a vector whose odd half is zero, read from a half-length array
      const EllOp& R = lv.R;
      const size_t ng = (size_t)R.ngroups, K = (size_t)R.K, G = (size_t)R.G;
      std::vector<int> rc(ng * K);
      std::vector<std::complex<double>> rv(ng * K * G);
      HIPCHK(hipMemcpy(rc.data(), R.cols, rc.size() * sizeof(int), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(rv.data(), R.vals, rv.size() * sizeof(cplx), hipMemcpyDeviceToHost));
      std::vector<std::vector<size_t>> keep(ng);
      size_t Ke = 1;
      for (size_t g = 0; g < ng; ++g) {
        for (size_t k = 0; k < K; ++k) {
          if (rc[g * K + k] >= lv.n / 2) continue;
          bool nz = false;
          for (size_t q = 0; q < G; ++q) nz = nz || rv[(g * K + k) * G + q] != std::complex<double>(0.0, 0.0);
          if (nz) keep[g].push_back(k);
        }
        Ke = std::max(Ke, keep[g].size());
      }
      std::vector<int> ec(ng * Ke, 0);
      std::vector<std::complex<double>> evv(ng * Ke * G, std::complex<double>(0.0, 0.0));
      for (size_t g = 0; g < ng; ++g)
        for (size_t i = 0; i < keep[g].size(); ++i) {
          const size_t k = keep[g][i];
          ec[g * Ke + i] = rc[g * K + k];
          for (size_t q = 0; q < G; ++q) evv[(g * Ke + i) * G + q] = rv[(g * K + k) * G + q];
        }
      EllOp& E = lv.Re;
      E.nrows = R.nrows;
      E.ncols = lv.n / 2;
      E.K = (int)Ke;
      E.G = R.G;
      E.ngroups = R.ngroups;
      SWCHK(upload(h, &E.cols, ec.data(), ec.size()));
      SWCHK(upload(h, &E.vals, (const cplx*)evv.data(), evv.size()));
      E.set = true;
    }
    if (!P.set || !P.cols || lv.w_eo.empty() || P.G < 1) continue;
    std::vector<char> even_row_tile;     // per 16-row tile (block levels)
    if (!lv.stencil) {
      const EllOp& S = lv.eo_op[0];
      if (!S.set || !S.bsr_tmap || S.bsr_RT <= 0 || 16 % P.G) continue;
      std::vector<int> tm(S.bsr_RT);
      HIPCHK(hipMemcpy(tm.data(), S.bsr_tmap, tm.size() * sizeof(int), hipMemcpyDeviceToHost));
      even_row_tile.assign((size_t)lv.n / 16, 0);
      for (int t : tm)
        if (t >= 0 && (size_t)t < even_row_tile.size()) even_row_tile[t] = 1;
    } else if ((lv.n / 2) % P.G) {
      continue;
    }
    std::vector<int> ord(P.ngroups);
    if (P.order && h->ell_order)
      HIPCHK(hipMemcpy(ord.data(), P.order, ord.size() * sizeof(int), hipMemcpyDeviceToHost));
    else
      for (int g = 0; g < P.ngroups; ++g) ord[g] = g;
    std::vector<int> ev;
    for (int g : ord) {
      const long long row = (long long)g * P.G;
      const bool even = lv.stencil ? (row < lv.n / 2) : (even_row_tile[row / 16] != 0);
      if (even) ev.push_back(g);
    }
    if (ev.empty()) continue;
    SWCHK(upload(h, &P.order_even, ev.data(), ev.size()));
    P.ngroups_even = (int)ev.size();
  }
  H.even_valid = true;
  return 0;
}

static inline int* sink_slot(sw_engine* h);
static bool f32_capable(const Hier& H, int level);

// One restart cycle of L steps in Gram-matrix form (see fgmres_eo_gram) from the residual R: the directions
// z_j = M v_j, w_j = A z_j (v_0 = R, v_j = w_{j-1}) without orthogonalisation, one multigram pass over
// [R, w_0 .. w_{L-1}] whose SW_TAIL_GRAM tail `tg` (tolerances, iteration base, counter, first_cycle set by
// the caller) solves for y, then X += sum_j y_j z_j
// (the cycle's BLAS-1 half, after its operator applications: pu = [R, w_0 .. w_{L-1}], pz = [z_0 .. z_{L-1}])
static int gram_cycle_update(sw_engine* h, const PtrList& pu, const PtrList& pz, int L, int n, int nbp, cplx* X,
                             KrylovWS& ws, swk::FgTail tg) {
  tg.kind = SW_TAIL_GRAM;
  tg.s = ws.sc;
  tg.j = L;
  tg.h1 = ws.gram;
  SWCHK(multigram(h, pu, L + 1, n, nbp, ws.gram, &tg));
  return multiaxpy(h, pz, L, ws.sc.ys, 1.0, X, X, n, nbp, nullptr);
}
static int gram_cycle(sw_engine* h, const KrylovSys& sys, const cplx* R, cplx* X, int L, KrylovWS& ws, int nbp,
                      swk::FgTail tg) {
  const size_t vec = (size_t)sys.n * nbp;
  PtrList pu, pz;
  pu.p[0] = R;
  for (int j = 0; j < L; ++j) {
    cplx* z = ws.Z + vec * j;
    cplx* w = ws.V + vec * j;
    SWCHK(sys.precond(pu.p[j], z));
    SWCHK(sys.apply(0, z, nullptr, w));
    pu.p[j + 1] = w;
    pz.p[j] = z;
  }
  return gram_cycle_update(h, pu, pz, L, sys.n, nbp, X, ws, tg);
}

// The K-cycle's inner iteration -- L steps of flexible GMRES from a zero guess, preconditioned by the cycle
// of `level` -- as one Gram-matrix cycle: 7 vector passes of BLAS-1 instead of 14 for L = 2
static int kcycle_gram(sw_engine* h, Hier& H, int level, const cplx* B, cplx* X, int L, KrylovWS& ws, int nbp) {
  swk::FgTail tg{};      // (tol = 0: nothing to count; the counter is the sink)
  tg.first_cycle = 1;
  tg.notconv = sink_slot(h);
  SWCHK(zero_vec(h, X, H.lv[level].n, nbp));
  return gram_cycle(h, full_system(h, H, level, nbp, true, false), B, X, L, ws, nbp, tg);
}

static int coarse_correction(sw_engine* h, Hier& H, int l, int nbp) {
  Level& lv = H.lv[l];
  Level& lc = H.lv[l + 1];
  const int last = H.nlevels - 1;
  if (lv.kcycle > 0 && l + 1 < last) {
    SWCHK(ensure_krylov(h, lc.kws, lv.kcycle, lc.n, nbp, false));
    int P = 0, rpb = 0;
    row_blocking(lc.n, nbp, true, &P, &rpb);
    if (h->gram_cycle && lv.kcycle <= SW_GRAM_MAXL && fused_ok(h, P, nbp) &&
        !(h->precond_f32 && f32_capable(H, l + 1)))
      return kcycle_gram(h, H, l + 1, lc.b, lc.x, lv.kcycle, lc.kws, nbp);
    return fgmres(h, H, l + 1, lc.b, lc.x, 0.0, lv.kcycle, lv.kcycle, false, lc.kws, nbp, nullptr);
  }
  return vcycle(h, H, l + 1, lc.b, lc.x, nbp);
}

// Into and out of the even-odd reduced system of the stencil level (k_eo_hop):
//   HOP 0:  out_e = b'_e = b_e + H_eo b_o / D   (src = B)
//   HOP 1:  out_o = x_o  = (b_o + H_oe x_e) / D (src = out = the iterate, whose even half is x_e)
template <int HOP>
static int eo_hop(sw_engine* h, Level& lv, const cplx* B, const cplx* src, cplx* out, int nbp) {
  const swk::StencilArgs a = stencil_args<cplx>(h, lv, nbp, true);
  const int bpc = (a.Vh + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK;
  const double di = 1.0 / a.diag;
  if (h->profiling) h->twork[T_SCHUR] += (double)a.Vh * (96.0 * nbp + 64.0);
  return launch(h, T_SCHUR, swk::k_eo_hop<HOP, cplx>, dim3(bpc * (nbp / 64)), dim3(SW_BLOCK), B, src, out, a,
                HOP == 0 ? 1.0 : di, di, bpc);
}

// One k_schur_step launch (class cat) on the stencil level (fp64) on the lattice rows a.row0 .. a.row0 + a.nrows - 1
// (a.nrows = 0: all)
template <int MODE>
static int launch_schur_step(sw_engine* h, int cat, swk::StencilArgs& a, const cplx* src, const cplx* bp, cplx* dst,
                             int nbp) {
  const int items = (a.nrows > 0 ? a.nrows : a.L) * (a.L / 2);
  if (h->eo_tile > 0 && (MODE == 0 || MODE == 3) && a.nrows == 0 && a.L % 8 == 0) {
    // LDS-staged halo tiles in rotated coordinates, double-buffered by LDS-DMA: one persistent workgroup per CU
    constexpr int TM = (MODE == 0) ? 0 : 3;
    const int tiles_v = a.L / 8, ntiles = (a.L / 4) * tiles_v;
    swk::StencilArgs at = a;
    at.row0 = h->eo_tile_dbg;      // (the tile kernel takes no row window: the field carries the diagnostic bits)
    const int njobs = ntiles * (nbp / 64);
    int grid = std::min(h->num_cus, njobs);
    grid = std::max(8, (grid + 7) & ~7);
    if (h->eo_tile == 8)
      return launch(h, cat, swk::k_schur_tile<TM, 8>, dim3(grid), dim3(512), src, dst, at, tiles_v, ntiles, njobs);
    return launch(h, cat, swk::k_schur_tile<TM, 4>, dim3(grid), dim3(256), src, dst, at, tiles_v, ntiles, njobs);
  }
  const int bpc = (items + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK;
  return launch(h, cat, swk::k_schur_step<cplx, MODE>, dim3(bpc * (nbp / 64)), dim3(SW_BLOCK), src, bp, dst, a, bpc);
}

// strip height of the time-skewed order for nu launches that each reach two lattice rows (0: plain order),
// and the probe width the strips are walked with: all nbp probes at once where strips of at least
// 4 (nu - 1) + 2 rows fit the cache at that width, else 64-probe chunk by chunk (the whole schedule once per
// chunk: the same launches per probe, each a quarter as wide at nbp = 256)
static int skew_height(sw_engine* h, Level& lv, int nu, int nbp, int* width) {
  const int L = lv.L;
  *width = nbp;
  if (h->eo_skew == 0 || nu < 2) return 0;
  auto admissible = [&](int H) { return H > 0 && L % H == 0 && L / H >= 2 && H > 4 * (nu - 1) && !(H & 1); };
  for (int w = h->eo_skew_chunk ? 64 : nbp; w >= 64; w = (w > 64 ? 64 : 0)) {
    const double row_bytes = (double)(L / 2) * 2.0 * sizeof(cplx) * w;          // one lattice row of a half vector
    int H = 0;
    if (h->eo_skew > 0) H = h->eo_skew;
    else if (3.0 * row_bytes * L * ((double)nbp / w) > 208.0e6) {
      H = 1;
      while (2 * H <= L / 2 && 3.0 * row_bytes * (2 * H) <= 208.0e6) H *= 2;
    }
    if (admissible(H)) {
      *width = w;
      return H;
    }
    if (H == 0 || h->eo_skew > 0) break;      // nothing to skew (fits the cache), or a fixed height that is not admissible
  }
  return 0;
}

// The nu Schur steps of an even-odd smoothing pass on the stencil level,
//   x_e <- x_e + w_k (bp - S x_e),  k = 0 .. nu-1,
// ping-ponging between `cur` (the iterate on entry) and `nxt`; *result = the buffer the last step wrote.
// On lattices whose three half vectors (both iterates and bp) exceed the 256 MB Infinity Cache every step
// would stream them from HBM (1024^2, 64 probes: 3.2 GB per step at 4.2 TB/s).  There the steps run in a
// TIME-SKEWED order instead (option eo_skew): the lattice rows are cut into strips of H rows; strip by
// strip, all nu steps are applied before the next strip is touched, step k of a strip working on its rows
// shifted down by 2 k (a Schur step reaches two lattice rows), so that everything step k reads from step
// k-1 has been written already -- by the strip itself or by its predecessor:
//   strip 0          step k : rows [2k, H - 2k)            (a shrinking trapezoid: nothing to its left yet)
//   strip s >= 1     step k : rows [sH - 2k, (s+1)H - 2k)  (parallelograms)
//   closing wedge    step k : rows [L - 2k, L + 2k)        (periodic lattice: what the torus still lacks)
// The two ping-pong buffers suffice (rows of step k and of step k-2 that are still needed never overlap).
// A strip's working set is 3 (H + 4) rows: chosen to fit the cache, only the first and the last touch of a
// strip reach HBM.  Same arithmetic per site in another order: results are bit-identical.
static int schur_steps(sw_engine* h, Level& lv, cplx* cur, cplx* nxt, const cplx* bp, int nbp, cplx** result) {
  swk::StencilArgs a = stencil_args<cplx>(h, lv, nbp, true);
  const int nu = (int)lv.w_eo.size();
  const int L = lv.L;
  int c0 = 0, cw = nbp;      // probe columns of the current launches
  auto launch = [&](int k, int row0, int nrows, const cplx* src, cplx* dst) -> int {
    a.w = cplx{lv.w_eo[k].real(), lv.w_eo[k].imag()};
    a.row0 = row0;
    a.nrows = nrows;
    const int items = (nrows > 0 ? nrows : L) * (L / 2);
    // algorithmic bytes: three half-vector rows per even site and spin (x_e, b'_e in, x_e out) + links
    if (h->profiling) h->twork[T_SCHUR] += (double)items * (96.0 * cw + 64.0);
    return launch_schur_step<2>(h, T_SCHUR, a, src + c0, bp + c0, dst + c0, cw);
  };
  const int H = skew_height(h, lv, nu, nbp, &cw);      // 0 = no skewing
  if (H == 0) {
    for (int k = 0; k < nu; ++k) {
      SWCHK(launch(k, 0, 0, cur, nxt));
      std::swap(cur, nxt);
    }
    *result = cur;
    return 0;
  }
  // buf[k & 1] receives step k; step k reads buf[(k + 1) & 1] (step 0: the iterate on entry, in `cur`)
  cplx* buf[2] = {nxt, cur};
  const int ns = L / H;
  for (c0 = 0; c0 < nbp; c0 += cw) {
    for (int sidx = 0; sidx < ns; ++sidx)
      for (int k = 0; k < nu; ++k) {
        const int row0 = (sidx == 0) ? 2 * k : sidx * H - 2 * k;
        const int nrows = (sidx == 0) ? H - 4 * k : H;
        SWCHK(launch(k, row0, nrows, buf[(k + 1) & 1], buf[k & 1]));
      }
    for (int k = 1; k < nu; ++k) SWCHK(launch(k, L - 2 * k, 4 * k, buf[(k + 1) & 1], buf[k & 1]));
  }
  *result = buf[(nu - 1) & 1];
  return 0;
}

// The same smoothing pass in PRODUCT FORM.  The nu steps above give x + q(S)(b' - S x) with the polynomial
// q(z) = (1 - prod_k (1 - w_k z)) / z of degree nu - 1; written as q(z) = beta prod_j (1 - u_j z) (Level::q_w,
// swp::product_form) the pass becomes
//   v = b' - S x              (k_schur_step<1>: x, b' in, v out     -- 3 half-vector passes)
//   v <- v - u_j S v          (k_schur_step<3>, j = 0 .. nu-3       -- 2 passes each: b' is not read)
//   x <- x + beta (v - u S v) (k_schur_step<4>, the last factor     -- 3 passes, in place in x)
// nu launches as before, 2 nu + 2 passes instead of 3 nu (nu = 8: 18 instead of 24).  Same polynomial, other
// arithmetic: equal to the step form to round-off (tests), not bit for bit.  `x` holds the iterate on entry
// and the smoothed iterate on exit; va, vb are two half-vector scratch arrays.  Time-skewed order as above
// (launch k reads what launch k-1 wrote, two rows further out; x is read by launch 0 and written by the
// last one, whose rows lie behind everything launch 0 still has to read).
static int schur_product_steps(sw_engine* h, Level& lv, cplx* x, cplx* va, cplx* vb, const cplx* bp, int nbp) {
  swk::StencilArgs a = stencil_args<cplx>(h, lv, nbp, true);
  const int nu = (int)lv.w_eo.size();
  const int L = lv.L;
  cplx* buf[2] = {va, vb};
  int c0 = 0, cw = nbp;      // probe columns of the current launches
  auto launch = [&](int k, int row0, int nrows) -> int {
    a.row0 = row0;
    a.nrows = nrows;
    const int items = (nrows > 0 ? nrows : L) * (L / 2);
    if (k == 0) {
      if (h->profiling) h->twork[T_SCHUR] += (double)items * (96.0 * cw + 64.0);
      return launch_schur_step<1>(h, T_SCHUR, a, x + c0, bp + c0, buf[0] + c0, cw);
    }
    const std::complex<double> u = lv.q_w[k - 1];
    a.w = cplx{u.real(), u.imag()};
    if (k < nu - 1) {
      if (h->profiling) h->twork[T_SCHUR] += (double)items * (64.0 * cw + 64.0);
      return launch_schur_step<3>(h, T_SCHUR, a, buf[(k + 1) & 1] + c0, nullptr, buf[k & 1] + c0, cw);
    }
    a.w2 = cplx{lv.q_beta.real(), lv.q_beta.imag()};
    if (h->profiling) h->twork[T_SCHUR] += (double)items * (96.0 * cw + 64.0);
    return launch_schur_step<4>(h, T_SCHUR, a, buf[(k + 1) & 1] + c0, x + c0, x + c0, cw);
  };
  const int H = skew_height(h, lv, nu, nbp, &cw);
  if (H == 0) {
    for (int k = 0; k < nu; ++k) SWCHK(launch(k, 0, 0));
    return 0;
  }
  const int ns = L / H;
  for (c0 = 0; c0 < nbp; c0 += cw) {
    for (int sidx = 0; sidx < ns; ++sidx)
      for (int k = 0; k < nu; ++k) {
        const int row0 = (sidx == 0) ? 2 * k : sidx * H - 2 * k;
        const int nrows = (sidx == 0) ? H - 4 * k : H;
        SWCHK(launch(k, row0, nrows));
      }
    for (int k = 1; k < nu; ++k) SWCHK(launch(k, L - 2 * k, 4 * k));
  }
  return 0;
}

// Even-odd post-smoothing of the stencil level (k_schur_step): on entry `start` holds the iterate
// after the coarse correction (only its even half is used), on exit Xout the smoothed iterate.
// `start` and `other` are the ping-pong pair chosen by the caller so that the last step lands in Xout.
static int eo_smooth(sw_engine* h, Level& lv, const cplx* Bin, cplx* start, cplx* other, cplx* Xout,
                     int nbp) {
  cplx* bp = lv.r;   // b'_e lives in the even half of the level's residual buffer
  SWCHK(eo_hop<0>(h, lv, Bin, Bin, bp, nbp));
  cplx* cur = nullptr;
  SWCHK(schur_steps(h, lv, start, other, bp, nbp, &cur));
  SWCHK(eo_hop<1>(h, lv, Bin, cur, cur, nbp));
  if (cur != Xout) return sw_fail(h, "internal: even-odd smoother ended in the wrong buffer");
  return 0;
}

// cycle with the fixed-polynomial smoother (weights set by sw_set_smoother)
static int vcycle_rich(sw_engine* h, Hier& H, int l, const cplx* Bin, cplx* Xout, int nbp) {
  Level& lv = H.lv[l];
  Level& lc = H.lv[l + 1];
  SWCHK(ensure_level_ws(h, lv, nbp));
  SWCHK(ensure_level_ws(h, lc, nbp));
  SWCHK(ensure_even_orders(h, H));
  if (!lv.P.set || !lv.R.set) return sw_fail(h, "transfer operators of level %d not set", l);
  const size_t npost = lv.w_post.size();
  if (!lv.stencil && lv.eo_op[4].set && lv.eo_op[1].set && lv.eo_op[2].set && lv.eo_op[3].set &&
      lv.w_pre.empty() && h->eo_direct) {
    // exact solve of this block level in even-odd reduced form: b'_e = b_e - F b_o ; x_e = S^-1 b'_e
    // (dense, matrix cores) ; x_o = G b_o - Hb x_e -- four launches, nothing below this level is visited
    SWCHK(launch_bsr(h, lv.eo_op[1], 1, Bin, Bin, lv.r, nbp, T_MVM, cplx{0.0, 0.0}));
    SWCHK(launch_bsr(h, lv.eo_op[4], 0, lv.r, nullptr, Xout, nbp, T_COARSEST, cplx{0.0, 0.0}));
    SWCHK(launch_bsr(h, lv.eo_op[2], 0, Bin, nullptr, Xout, nbp, T_MVM, cplx{0.0, 0.0}));
    return launch_bsr(h, lv.eo_op[3], 1, Xout, Xout, Xout, nbp, T_MVM, cplx{0.0, 0.0});
  }
  cplx* xpre = nullptr;
  if (!lv.w_pre.empty()) {
    SWCHK(rich_steps(h, lv, Bin, Xout, lv.t, lv.w_pre, true, nbp, &xpre));
    SWCHK(apply_op(h, lv, 1, xpre, Bin, lv.r, nbp));
    SWCHK(launch_ell(h, lv.R, 0, lv.r, nullptr, lc.b, nbp, T_R));
  } else {
    SWCHK(launch_ell(h, lv.R, 0, Bin, nullptr, lc.b, nbp, T_R));
  }
  SWCHK(coarse_correction(h, H, l, nbp));
  if (!lv.stencil && !lv.w_eo.empty() && !xpre && lv.eo_op[0].set) {
    // even-odd post-smoother of a block level, all four pieces on the MFMA block-row kernel:
    //   b'_e = b_e - F b_o ;  x_e <- x_e + w_k (b'_e - S x_e) ;  x_o = G b_o - Hb x_e
    const bool odd_steps = (lv.w_eo.size() & 1) != 0;
    cplx* cur = odd_steps ? lv.t : Xout;
    cplx* nxt = odd_steps ? Xout : lv.t;
    SWCHK(launch_ell(h, lv.P, 0, lc.x, nullptr, cur, nbp, T_P, cplx{0.0, 0.0}, true));
    SWCHK(launch_bsr(h, lv.eo_op[1], 1, Bin, Bin, lv.r, nbp, T_MVM, cplx{0.0, 0.0}));
    for (size_t k = 0; k < lv.w_eo.size(); ++k) {
      SWCHK(launch_bsr(h, lv.eo_op[0], 3, cur, lv.r, nxt, nbp, T_MVM,
                       cplx{lv.w_eo[k].real(), lv.w_eo[k].imag()}));
      std::swap(cur, nxt);
    }
    SWCHK(launch_bsr(h, lv.eo_op[2], 0, Bin, nullptr, Xout, nbp, T_MVM, cplx{0.0, 0.0}));
    return launch_bsr(h, lv.eo_op[3], 1, Xout, Xout, Xout, nbp, T_MVM, cplx{0.0, 0.0});
  }
  if (lv.stencil && !lv.w_eo.empty() && !xpre) {
    // even-odd post-smoother: prolongate into the buffer from which nu steps end in Xout
    const bool odd_steps = (lv.w_eo.size() & 1) != 0;
    cplx* start = odd_steps ? lv.t : Xout;
    cplx* other = odd_steps ? Xout : lv.t;
    SWCHK(launch_ell(h, lv.P, 0, lc.x, nullptr, start, nbp, T_P, cplx{0.0, 0.0}, true));
    return eo_smooth(h, lv, Bin, start, other, Xout, nbp);
  }
  // place the prolongated iterate so that the ping-pong launches of the post-smoother end in Xout
  const size_t nlaunch = npost;
  cplx* start = (nlaunch % 2 == 0) ? Xout : lv.t;
  cplx* other = (nlaunch % 2 == 0) ? lv.t : Xout;
  if (xpre) SWCHK(launch_ell(h, lv.P, 2, lc.x, xpre, start, nbp, T_P));
  else SWCHK(launch_ell(h, lv.P, 0, lc.x, nullptr, start, nbp, T_P));
  cplx* res = start;
  SWCHK(rich_steps(h, lv, Bin, start, other, lv.w_post, false, nbp, &res));
  if (res != Xout) SWCHK(copy_vec(h, Xout, res, lv.n, nbp));
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Single-precision preconditioner (option precond_f32).  The cycle below is vcycle_rich's even-odd /
// fixed-polynomial cycle on complex64 mirrors of the operators: half the bytes on every HBM-bound
// kernel and the f32 matrix cores (twice the fp64 rate on gfx950) for the block operators.  It is only
// ever used INSIDE an fp64 flexible GMRES, whose residuals, orthogonalisation and true-residual
// verification are untouched, so the solve converges to the same fp64 tolerance.
// Supported: fixed-polynomial (Richardson) levels without pre-smoothing and without K-cycles, the
// stencil level smoothed even-odd -- i.e. the tuned configurations; anything else fails loudly.
// ---------------------------------------------------------------------------------------------
template <class CI, class CO>
static int cast_vec(sw_engine* h, const CI* src, CO* dst, size_t count, int cat = T_OTHER) {
  return launch(h, cat, swk::k_cast<CI, CO>, dim3((unsigned)((count + SW_BLOCK - 1) / SW_BLOCK)), dim3(SW_BLOCK),
                src, dst, count);
}

static int mirror_op32(sw_engine* h, EllOp& op) {
  if (!op.set) return 0;
  if (op.vals && !op.vals32) {
    const size_t cnt = (size_t)op.ngroups * op.K * op.G;
    SWCHK(dev_realloc(h, &op.vals32, cnt));
    SWCHK(cast_vec(h, (const cplx*)op.vals, op.vals32, cnt));
  }
  if (op.bsr_vals && op.bsr_KS > 0 && !op.bsr_vals32) {
    const int RT = op.bsr_RT > 0 ? op.bsr_RT : op.nrows / 16;
    const size_t cnt = (size_t)RT * op.bsr_KS * 64;
    SWCHK(dev_realloc(h, &op.bsr_vals32, cnt));
    SWCHK(cast_vec(h, (const cplx*)op.bsr_vals, op.bsr_vals32, cnt));
  }
  return 0;
}

static int drop_op32(sw_engine* h, EllOp& op) {
  SWCHK(dev_free(h, op.vals32));
  op.vals32 = nullptr;
  SWCHK(dev_free(h, op.bsr_vals32));
  op.bsr_vals32 = nullptr;
  return 0;
}

// (re)build every complex64 mirror of a hierarchy after its operators changed
static int ensure_f32(sw_engine* h, Hier& H) {
  if (H.f32_valid) return 0;
  for (int l = 0; l < H.nlevels; ++l) {
    Level& lv = H.lv[l];
    EllOp* ops[8] = {&lv.A, &lv.P, &lv.R, &lv.eo_op[0], &lv.eo_op[1], &lv.eo_op[2], &lv.eo_op[3], &lv.eo_op[4]};
    for (EllOp* op : ops) {
      SWCHK(drop_op32(h, *op));
      SWCHK(mirror_op32(h, *op));
    }
    if (lv.stencil && lv.U1) {
      const size_t V = (size_t)lv.L * lv.L;
      SWCHK(dev_realloc(h, &lv.U1f, V));
      SWCHK(dev_realloc(h, &lv.U2f, V));
      SWCHK(cast_vec(h, (const cplx*)lv.U1, lv.U1f, V));
      SWCHK(cast_vec(h, (const cplx*)lv.U2, lv.U2f, V));
    }
  }
  SWCHK(drop_op32(h, H.cinv));
  SWCHK(mirror_op32(h, H.cinv));
  H.f32_valid = true;
  return 0;
}

static int ensure_level_ws32(sw_engine* h, Level& lv, int nbp) {
  if (lv.ws32_nbp == nbp && lv.b32) return 0;
  const size_t cnt = (size_t)lv.n * nbp;
  SWCHK(dev_realloc(h, &lv.b32, cnt));
  SWCHK(dev_realloc(h, &lv.x32, cnt));
  SWCHK(dev_realloc(h, &lv.r32, cnt));
  SWCHK(dev_realloc(h, &lv.t32, cnt));
  SWCHK(dev_free(h, lv.i32)); lv.i32 = nullptr;   // boundary pair: made on demand for this width
  SWCHK(dev_free(h, lv.o32)); lv.o32 = nullptr;
  lv.ws32_nbp = nbp;
  return 0;
}

static int launch_bsr32(sw_engine* h, const EllOp& op, int mode, const cplxf* X, const cplxf* B, cplxf* Y,
                        int nbp, int cat, cplxf w) {
  if (!op.bsr_vals32) return sw_fail(h, "internal: complex64 mirror of a block-row operator missing");
  const int RT = op.bsr_RT > 0 ? op.bsr_RT : op.nrows / 16;
  // tiles of 16 probes per wave: 4 (64 probes) unless the operator is too small to fill the chip
  int NT = 4;
  if ((long long)RT * (nbp / 64) < 4096) NT = 2;
  if (h->f32_tiles == 1 || h->f32_tiles == 2 || h->f32_tiles == 4) NT = h->f32_tiles;
  const int RBn = (RT + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK, NCn = nbp / (16 * NT);
  const int bmap = (cat == T_COARSEST) ? 0 : 1;
  const int n1 = h->hier[h->solver_hid].nlevels > 1 ? h->hier[h->solver_hid].lv[1].n : 0;
  const int cls = cat == T_COARSEST ? T_MFMA_DENSE
                                    : (cat == T_MVM ? (op.nrows == n1 || n1 == 0 ? T_MFMA_OP : T_MFMA_OP2)
                                                    : cat);
  if (h->profiling) h->twork[cls] += 512.0 * (double)RT * (double)op.bsr_KS * (double)nbp;
  if ((h->f32_splitk == 1 && cat == T_COARSEST) ||
      (h->f32_splitk == 2 && (long long)RT * (nbp / 64) < 4096 && op.bsr_KS >= 16)) {
    // few (tile, chunk) pairs: four waves per pair, each a quarter of the k-steps
    const int NTs = (h->f32_tiles == 1) ? 1 : 2;
    const dim3 gsk(RT * (nbp / (16 * NTs)));
    return pick<1, 2>(NTs, [&](auto NTT) {
      return pick<0, 1, 3>(mode, [&](auto MD) {
        return launch(h, cls, swk::k_bsr_mfma_f32_sk<MD, NTT>, gsk, dim3(SW_BLOCK), (const cplxf*)op.bsr_vals32,
                      (const int*)op.bsr_kcol, op.bsr_KS, RT, X, B, Y, nbp, w, (const int*)op.bsr_tmap);
      });
    });
  }
  const dim3 grid(RBn * NCn);
  const int stg = (cat == T_COARSEST) ? h->f32_dense_stages : h->f32_stages;
  return pick<4, 2, 1>(NT, [&](auto NTT) {
    return pick<0, 1, 3>(mode, [&](auto MD) {
      return pick<8, 4, 2>(stg >= 8 ? 8 : (stg >= 4 ? 4 : 2), [&](auto SG) {
        return launch(h, cls, swk::k_bsr_mfma_f32<MD, NTT, SG>, grid, dim3(SW_BLOCK), (const cplxf*)op.bsr_vals32,
                      (const int*)op.bsr_kcol, op.bsr_KS, RT, X, B, Y, nbp, w, bmap, (const int*)op.bsr_tmap);
      });
    });
  });
}

static int launch_ell32(sw_engine* h, const EllOp& op, int mode, const cplxf* X, const cplxf* B,
                        cplxf* Y, int nbp, int cat, cplxf w = cplxf{0.f, 0.f}, bool even_only = false) {
  if (!op.set) return sw_fail(h, "operator not set");
  if (op.bsr_KS > 0 && (mode == 0 || mode == 1 || mode == 3) && op.bsr_vals32)
    return launch_bsr32(h, op, mode, X, B, Y, nbp, cat, w);
  if (!op.cols || !op.vals32)
    return sw_fail(h, "internal: complex64 mirror of a grouped-ELL operator missing");
  return launch_ell_groups<cplxf>(h, op, op.vals32, mode, X, B, Y, nbp, cat, w, even_only);
}

// even-odd post-smoothing of the stencil level in complex64 (eo_smooth's twin).  C = cplxf2: two probes
// per lane (16-B accesses, rows of nbp / 2 elements), used whenever nbp is a multiple of 128
template <class C>
// reduced: smoothing of the even-odd reduced system itself (vcycle32_even): Bin IS b'_e (no hop before the
// steps) and only the even half of the iterate is wanted (no hop after them); all arrays half-length
static int eo_smooth32_t(sw_engine* h, Level& lv, const cplxf* Bin_, cplxf* start_, cplxf* other_,
                         cplxf* Xout_, int nbp, bool reduced) {
  const C* Bin = (const C*)Bin_;
  C* start = (C*)start_;
  C* other = (C*)other_;
  C* Xout = (C*)Xout_;
  swk::StencilArgsT<C> a = stencil_args<C>(h, lv, nbp, true);
  const int bpc = (a.Vh + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK;
  const dim3 grid(bpc * (a.nbp / 64));
  const float di = (float)(1.0 / (4.0 + lv.mass));
  const C* bp = reduced ? Bin : (const C*)lv.r32;
  if (!reduced) {
    SWCHK(launch(h, T_SCHUR, swk::k_eo_hop<0, C>, grid, dim3(SW_BLOCK), Bin, Bin, (C*)lv.r32, a, 1.0f, di, bpc));
  }
  C* cur = start;
  C* nxt = other;
  for (size_t k = 0; k < lv.w_eo.size(); ++k) {
    a.w = cplxf{(float)lv.w_eo[k].real(), (float)lv.w_eo[k].imag()};
    SWCHK(launch(h, T_SCHUR, swk::k_schur_step<C>, grid, dim3(SW_BLOCK), (const C*)cur, (const C*)bp, nxt, a, bpc));
    std::swap(cur, nxt);
  }
  if (cur != Xout) return sw_fail(h, "internal: even-odd smoother ended in the wrong buffer");
  if (!reduced) {
    SWCHK(launch(h, T_SCHUR, swk::k_eo_hop<1, C>, grid, dim3(SW_BLOCK), Bin, (const C*)Xout, Xout, a, di, di, bpc));
  }
  return 0;
}

static int eo_smooth32(sw_engine* h, Level& lv, const cplxf* Bin, cplxf* start, cplxf* other, cplxf* Xout,
                       int nbp, bool reduced = false) {
  if (nbp % 128 == 0 && h->f32_pairs)
    return eo_smooth32_t<swk::cplxf2>(h, lv, Bin, start, other, Xout, nbp, reduced);
  return eo_smooth32_t<cplxf>(h, lv, Bin, start, other, Xout, nbp, reduced);
}

// Y_e = S X_e on complex64 half vectors (operator of the even-odd reduced system, complex64 Krylov basis)
template <class C>
static int schur_apply32_t(sw_engine* h, Level& lv, const cplxf* X_, cplxf* Y_, int nbp) {
  const swk::StencilArgsT<C> a = stencil_args<C>(h, lv, nbp, true);
  const int bpc = (a.Vh + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK;
  const dim3 grid(bpc * (a.nbp / 64));
  return launch(h, T_SCHUR_OP, swk::k_schur_step<C, 0>, grid, dim3(SW_BLOCK), (const C*)X_, (const C*)nullptr,
                (C*)Y_, a, bpc);
}
static int schur_apply32(sw_engine* h, Level& lv, const cplxf* X, cplxf* Y, int nbp) {
  if (nbp % 128 == 0 && h->f32_pairs) return schur_apply32_t<swk::cplxf2>(h, lv, X, Y, nbp);
  return schur_apply32_t<cplxf>(h, lv, X, Y, nbp);
}

static int vcycle32(sw_engine* h, Hier& H, int l, const cplxf* Bin, cplxf* Xout, int nbp) {
  const int last = H.nlevels - 1;
  if (l == last) {
    if (!H.cinv.set) return sw_fail(h, "coarsest inverse not set");
    return launch_ell32(h, H.cinv, 0, Bin, nullptr, Xout, nbp, T_COARSEST);
  }
  Level& lv = H.lv[l];
  Level& lc = H.lv[l + 1];
  if (!lv.rich || lv.gm_m > 0 || !lv.w_pre.empty())
    return sw_fail(h, "precond_f32 supports fixed-polynomial post-smoothing cycles only "
                      "(level %d is configured otherwise)", l);
  SWCHK(ensure_level_ws32(h, lv, nbp));
  SWCHK(ensure_level_ws32(h, lc, nbp));
  SWCHK(ensure_even_orders(h, H));
  if (!lv.P.set || !lv.R.set) return sw_fail(h, "transfer operators of level %d not set", l);
  if (!lv.stencil && lv.eo_op[4].set && lv.eo_op[4].bsr_vals32 && lv.eo_op[1].set && lv.eo_op[2].set &&
      lv.eo_op[3].set && h->eo_direct) {
    const cplxf z0{0.f, 0.f};
    SWCHK(launch_bsr32(h, lv.eo_op[1], 1, Bin, Bin, lv.r32, nbp, T_MVM, z0));
    SWCHK(launch_bsr32(h, lv.eo_op[4], 0, lv.r32, nullptr, Xout, nbp, T_COARSEST, z0));
    SWCHK(launch_bsr32(h, lv.eo_op[2], 0, Bin, nullptr, Xout, nbp, T_MVM, z0));
    return launch_bsr32(h, lv.eo_op[3], 1, Xout, Xout, Xout, nbp, T_MVM, z0);
  }
  SWCHK(launch_ell32(h, lv.R, 0, Bin, nullptr, lc.b32, nbp, T_R));
  if (lv.kcycle > 0 && l + 1 < last) {
    // K-cycle: the few-step inner FGMRES of the coarse system stays fp64 (its Hessenberg solve and
    // orthogonalisation are precision-sensitive and small); its preconditioner is complex64 again
    const size_t cc = (size_t)lc.n * nbp;
    SWCHK(ensure_level_ws(h, lc, nbp));
    SWCHK(cast_vec(h, (const cplxf*)lc.b32, lc.b, cc, T_AXPY));
    SWCHK(ensure_krylov(h, lc.kws, lv.kcycle, lc.n, nbp, false));
    SWCHK(fgmres(h, H, l + 1, lc.b, lc.x, 0.0, lv.kcycle, lv.kcycle, false, lc.kws, nbp, nullptr, true));
    SWCHK(cast_vec(h, (const cplx*)lc.x, lc.x32, cc, T_AXPY));
  } else {
    SWCHK(vcycle32(h, H, l + 1, lc.b32, lc.x32, nbp));
  }
  const cplxf z{0.f, 0.f};
  if (!lv.stencil && !lv.w_eo.empty() && lv.eo_op[0].set) {
    const bool odd_steps = (lv.w_eo.size() & 1) != 0;
    cplxf* cur = odd_steps ? lv.t32 : Xout;
    cplxf* nxt = odd_steps ? Xout : lv.t32;
    SWCHK(launch_ell32(h, lv.P, 0, lc.x32, nullptr, cur, nbp, T_P, z, true));
    SWCHK(launch_bsr32(h, lv.eo_op[1], 1, Bin, Bin, lv.r32, nbp, T_MVM, z));
    for (size_t k = 0; k < lv.w_eo.size(); ++k) {
      SWCHK(launch_bsr32(h, lv.eo_op[0], 3, cur, lv.r32, nxt, nbp, T_MVM,
                         cplxf{(float)lv.w_eo[k].real(), (float)lv.w_eo[k].imag()}));
      std::swap(cur, nxt);
    }
    SWCHK(launch_bsr32(h, lv.eo_op[2], 0, Bin, nullptr, Xout, nbp, T_MVM, z));
    return launch_bsr32(h, lv.eo_op[3], 1, Xout, Xout, Xout, nbp, T_MVM, z);
  }
  if (lv.stencil) {
    if (lv.w_eo.empty())
      return sw_fail(h, "precond_f32 needs the even-odd smoother on the stencil level (sw_set_eo_smoother)");
    const bool odd_steps = (lv.w_eo.size() & 1) != 0;
    cplxf* start = odd_steps ? lv.t32 : Xout;
    cplxf* other = odd_steps ? Xout : lv.t32;
    SWCHK(launch_ell32(h, lv.P, 0, lc.x32, nullptr, start, nbp, T_P, z, true));
    return eo_smooth32(h, lv, Bin, start, other, Xout, nbp);
  }
  // block level with the plain polynomial post-smoother: x <- x + w_k (b - A x)
  const size_t npost = lv.w_post.size();
  cplxf* cur = (npost % 2 == 0) ? Xout : lv.t32;
  cplxf* nxt = (npost % 2 == 0) ? lv.t32 : Xout;
  SWCHK(launch_ell32(h, lv.P, 0, lc.x32, nullptr, cur, nbp, T_P));
  for (size_t k = 0; k < npost; ++k) {
    SWCHK(launch_ell32(h, lv.A, 3, cur, Bin, nxt, nbp, T_MVM,
                       cplxf{(float)lv.w_post[k].real(), (float)lv.w_post[k].imag()}));
    std::swap(cur, nxt);
  }
  if (cur != Xout) return sw_fail(h, "internal: polynomial smoother ended in the wrong buffer");
  return 0;
}

// can the cycle that starts at `level` run on the complex64 path?  (otherwise the fp64 cycle is used)
static bool f32_capable(const Hier& H, int level) {
  for (int l = level; l < H.nlevels - 1; ++l) {
    const Level& lv = H.lv[l];
    if (!lv.rich || lv.gm_m > 0 || !lv.w_pre.empty()) return false;
    if (lv.stencil && lv.w_eo.empty()) return false;
  }
  return level < H.nlevels - 1;
}

// the preconditioner as the fp64 solver sees it: Xout = (fp64) cycle32((complex64) Bin)
static int vcycle_f32_boundary(sw_engine* h, Hier& H, int l, const cplx* Bin, cplx* Xout, int nbp) {
  SWCHK(ensure_f32(h, H));
  Level& lv = H.lv[l];
  SWCHK(ensure_level_ws32(h, lv, nbp));
  const size_t cnt = (size_t)lv.n * nbp;
  if (!lv.i32) {
    SWCHK(dev_realloc(h, &lv.i32, cnt));
    SWCHK(dev_realloc(h, &lv.o32, cnt));
  }
  SWCHK(cast_vec(h, Bin, lv.i32, cnt, T_AXPY));
  SWCHK(vcycle32(h, H, l, lv.i32, lv.o32, nbp));
  return cast_vec(h, (const cplxf*)lv.o32, Xout, cnt, T_AXPY);
}

// ---------------------------------------------------------------------------------------------
// convergence counters and the FGMRES scalar updates that ride on the reductions
// ---------------------------------------------------------------------------------------------
static int reset_slots(sw_engine* h) {
  HIPCHK(hipMemsetAsync(h->d_notconv, 0, SW_NC_SLOTS * sizeof(int), h->stream));
  h->nc_next = 0;
  return 0;
}
// a zeroed counter for the next scalar update of an outer solve
static int take_slot(sw_engine* h, int** slot) {
  if (h->nc_next >= SW_NC_SLOTS - 1) SWCHK(reset_slots(h));
  *slot = h->d_notconv + h->nc_next++;
  return 0;
}
static inline int* sink_slot(sw_engine* h) { return h->d_notconv + SW_NC_SLOTS - 1; }
// number of probes the update that owned `slot` left above tol_stop (drains the stream)
static int read_slot(sw_engine* h, const int* slot, int* count) {
  HIPCHK(hipMemcpyAsync(h->h_notconv, slot, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  SWCHK(stream_sync(h));
  *count = *h->h_notconv;
  return 0;
}
// y = H(0:k,0:k)^-1 g(0:k) and ys = svec y per probe, at the end of a restart cycle of k columns
static int launch_fg_solve(sw_engine* h, const swk::FgScalars& sc, int k) {
  const int tb = 256;
  return launch(h, T_OTHER, swk::k_fg_solve, dim3((sc.nbp + tb - 1) / tb), dim3(tb), sc, k);
}
static swk::FgTail tail_begin(const KrylovWS& ws, int first_cycle) {
  swk::FgTail t{};
  t.kind = SW_TAIL_BEGIN;
  t.s = ws.sc;
  t.h1 = ws.nrm;
  t.first_cycle = first_cycle;
  return t;
}
static swk::FgTail tail_hess(const KrylovWS& ws, int j, bool two_pass, bool pyth, double tol, double tol_stop,
                             int iter_base, int* slot) {
  swk::FgTail t{};
  t.kind = SW_TAIL_HESS;
  t.s = ws.sc;
  t.j = j;
  t.h1 = ws.h1;
  t.h2 = two_pass ? ws.h2 : nullptr;
  t.nrm2 = pyth ? ws.h1 + (size_t)(j + 1) * ws.nbp : ws.nrm;
  t.tol = tol;
  t.tol_stop = tol_stop;
  t.iter_base = iter_base;
  t.pyth = pyth ? 1 : 0;
  t.notconv = slot;
  return t;
}
static swk::FgTail tail_verify(const KrylovWS& ws, double tol, double tol_stop, int* slot) {
  swk::FgTail t{};
  t.kind = SW_TAIL_VERIFY;
  t.s = ws.sc;
  t.h1 = ws.nrm;
  t.tol = tol;
  t.tol_stop = tol_stop;
  t.notconv = slot;
  return t;
}

// ---------------------------------------------------------------------------------------------
// batched right-preconditioned flexible GMRES(m) (MG.solve -> fgmres, multigrid.py:347-366) on the system
// `sys` with right-hand side B (of length sys.n); one classical Gram-Schmidt pass per step (two with option
// cgs2), true-residual verification
//  outer == true : restarted, converges every probe to stop_factor * tol (one host read-back per
//                  iteration once the expected count is near)
//  outer == false: exactly `maxiter` (= m, or m + 1 with `aug`) steps from a zero guess, no host
//                  synchronisation
//  aug (inner, unpreconditioned only): LGMRES's augmentation vector (multigrid.py:393-394, SciPy
//                  lgmres with outer_k >= 1): after the m Arnoldi steps one more step whose direction
//                  is `aug` instead of the next Krylov vector, so the cycle minimises the residual over
//                  K_m(A, r) + span{aug}; ws must have room for m + 1 vectors
// ---------------------------------------------------------------------------------------------
static int fgmres_loop(sw_engine* h, Hier& H, int level, const KrylovSys& sys, const cplx* B, cplx* X,
                       double tol, int maxiter, int m, bool outer, KrylovWS& ws, int nbp, int* iters_total,
                       const cplx* aug = nullptr) {
  const int hid_idx = (int)(&H - &h->hier[0]);
  const int check_from = (outer && h->lazy_sync) ? std::max(0, h->sync_hint[hid_idx][level] - 2) : 0;
  const int n = sys.n;
  const size_t vec = (size_t)n * nbp;
  const double tol_stop = outer ? tol * h->stop_factor : tol;
  // complex64 directions: the input copy of each Krylov vector is written by its producer
  const bool z32 = (bool)sys.precond32;
  const bool k32 = z32 && h->f32_krylov;
  if (aug && (outer || sys.precond || ws.m < m + 1)) return sw_fail(h, "internal: augmented cycle misused");
  if (z32 && !(k32 ? (bool)sys.op32 : (bool)sys.op32w))
    return sw_fail(h, "internal: complex64 operator of the Krylov system missing");
  int done = 0;
  bool first = true;
  bool converged = false;
  if (outer) SWCHK(reset_slots(h));
  SWCHK(zero_vec(h, X, n, nbp));
  const cplx* Rcur = B;
  if (z32) {
    Level& lv = H.lv[level];
    SWCHK(ensure_f32(h, H));
    SWCHK(ensure_level_ws32(h, lv, nbp));
    // full length of the level: its full and reduced systems share the workspace
    const size_t full = (size_t)lv.n * nbp;
    if (!ws.Z32) {
      SWCHK(dev_realloc(h, &ws.Z32, full * m));
      SWCHK(dev_realloc(h, &ws.v32, full));
    }
    if (k32 && !ws.V32) SWCHK(dev_realloc(h, &ws.V32, full * m));
  }
  while (done < maxiter && !converged) {
    // beta = ||r||
    {
      PtrList pl;
      pl.p[0] = Rcur;
      const swk::FgTail tbeg = tail_begin(ws, (first && !sys.normb_set) ? 1 : 0);
      SWCHK(multidot(h, pl, 1, Rcur, n, nbp, ws.nrm, nullptr, nullptr, &tbeg));
    }
    // the basis is kept unnormalised (fg_hess_col): vtilde_0 is the residual where it lies,
    // vtilde_{j+1} the orthogonalised A M vtilde_j -- no normalisation passes over the vectors
    auto vt = [&](int k) -> const cplx* { return k == 0 ? Rcur : ws.V + vec * (k - 1); };
    auto vt32 = [&](int k) -> const cplxf* { return k == 0 ? ws.v32 : ws.V32 + vec * (k - 1); };
    if (z32) SWCHK(cast_vec(h, Rcur, ws.v32, vec, T_AXPY));
    const bool two_pass = h->cgs2 || (!outer && h->inner_cgs2);
    int j = 0;
    const int jmax = std::min(m, maxiter - done) + (aug ? 1 : 0);
    for (; j < jmax; ++j) {
      const cplx* vj = vt(j);
      cplx* zj = ws.Z + vec * j;
      cplx* w = ws.V + vec * j;          // becomes vtilde_{j+1}
      cplxf* zj32 = z32 ? ws.Z32 + vec * j : nullptr;
      const bool aug_step = aug && j == jmax - 1;
      // Last step of a cycle: vtilde_{j+1} is never used (the next cycle starts from the true
      // residual), only h_{j+1,j} is.  With one Gram-Schmidt pass that is
      // sqrt(|w|^2 - sum_k |h_{k,j}|^2): |w|^2 rides along in the same multidot pass over w and the
      // orthogonalisation pass (j + 3 vector passes) is not run at all (fg_hess_col, pyth).
      const bool last = h->pyth_last && !two_pass && j == jmax - 1 && m <= 8;   // (short cycles only:
      // a single-pass basis of 30 vectors has lost too much orthogonality for the identity)
      int* slot = sink_slot(h);
      if (outer) SWCHK(take_slot(h, &slot));
      const swk::FgTail th = tail_hess(ws, j, two_pass, last, tol, tol_stop, done, slot);
      if (k32) {
        // complex64 cycle: vtilde_j -> z_j -> w = A z_j -> orthogonalised vtilde_{j+1}, all stored
        // complex64 (the arithmetic of A z and of the inner products is fp64 on widened operands)
        cplxf* w32 = ws.V32 + vec * j;
        SWCHK(sys.precond32(vt32(j), zj32));
        SWCHK(sys.op32(zj32, w32));
        swk::PtrListT<cplxf> pv32;
        for (int k = 0; k <= j; ++k) pv32.p[k] = vt32(k);
        pv32.p[j + 1] = w32;
        SWCHK(multidot(h, pv32, last ? j + 2 : j + 1, (const cplxf*)w32, n, nbp, ws.h1, ws.sc.svec, ws.c1,
                       last ? &th : nullptr));
        if (last) {
          // (nothing: h_{j+1,j} comes from the dots alone)
        } else if (two_pass) {
          SWCHK(multiaxpy(h, pv32, j + 1, ws.c1, -1.0, (const cplxf*)w32, w32, n, nbp, nullptr));
          SWCHK(multidot(h, pv32, j + 1, (const cplxf*)w32, n, nbp, ws.h2, ws.sc.svec, ws.c1));
          SWCHK(multiaxpy(h, pv32, j + 1, ws.c1, -1.0, (const cplxf*)w32, w32, n, nbp, ws.nrm, nullptr, &th));
        } else {
          SWCHK(multiaxpy(h, pv32, j + 1, ws.c1, -1.0, (const cplxf*)w32, w32, n, nbp, ws.nrm, nullptr, &th));
        }
      } else {
      if (z32) {
        SWCHK(sys.precond32(ws.v32, zj32));
        SWCHK(sys.op32w(zj32, w));
      } else {
        if (aug_step) SWCHK(copy_vec(h, zj, aug, n, nbp));
        else if (sys.precond) SWCHK(sys.precond(vj, zj));
        else SWCHK(copy_vec(h, zj, vj, n, nbp));
        SWCHK(sys.apply(0, zj, nullptr, w));
      }
      PtrList pv;
      for (int k = 0; k <= j; ++k) pv.p[k] = vt(k);
      pv.p[j + 1] = w;
      // pass 1: raw dots d1 = Vt^H w, coefficients c = svec^2 d1 ; w -= Vt c
      SWCHK(multidot(h, pv, last ? j + 2 : j + 1, w, n, nbp, ws.h1, ws.sc.svec, ws.c1, last ? &th : nullptr));
      if (last) {
        // (nothing: h_{j+1,j} comes from the dots alone)
      } else if (two_pass) {
        SWCHK(multiaxpy(h, pv, j + 1, ws.c1, -1.0, w, w, n, nbp, nullptr));
        // pass 2 (re-orthogonalisation): d2 = Vt^H w ; w -= Vt (svec^2 d2) ; ||w||^2
        SWCHK(multidot(h, pv, j + 1, w, n, nbp, ws.h2, ws.sc.svec, ws.c1));
        SWCHK(multiaxpy(h, pv, j + 1, ws.c1, -1.0, w, w, n, nbp, ws.nrm, z32 ? ws.v32 : nullptr, &th));
      } else {
        SWCHK(multiaxpy(h, pv, j + 1, ws.c1, -1.0, w, w, n, nbp, ws.nrm, z32 ? ws.v32 : nullptr, &th));
      }
      }   // fp64 basis
      // read the flag back from the hinted iteration on, at the end of the budget, and in any
      // case every 8th iteration (a stale hint must never cost more than a few iterations)
      // (tol = 0: a fixed number of iterations, e.g. the relaxation sweeps of the setup -- nothing to poll)
      if (outer && tol_stop > 0.0 && (done + j + 1 >= check_from || done + j + 1 >= maxiter ||
                                      ((done + j + 1) & 7) == 0)) {
        int left = 0;
        SWCHK(read_slot(h, slot, &left));
        if (left == 0) {
          converged = true;
          ++j;
          break;
        }
      }
    }
    const int k = j;  // columns built in this cycle
    SWCHK(launch_fg_solve(h, ws.sc, k));
    if (z32) {
      swk::PtrListT<cplxf> pz;
      for (int q = 0; q < k; ++q) pz.p[q] = ws.Z32 + vec * q;
      SWCHK(multiaxpy(h, pz, k, ws.sc.ys, 1.0, X, X, n, nbp, nullptr));
    } else {
      PtrList pz;
      for (int q = 0; q < k; ++q) pz.p[q] = ws.Z + vec * q;
      SWCHK(multiaxpy(h, pz, k, ws.sc.ys, 1.0, X, X, n, nbp, nullptr));
    }
    done += k;
    first = false;
    if (!outer) break;
    if (converged && h->verify) {
      // (also at done == maxiter: a solve that is flagged converged on its last permitted
      // iteration is still checked, and reported as not converged when the check fails)
      // true residual of every probe; continue when the Arnoldi recurrence was optimistic
      SWCHK(sys.apply(1, X, B, ws.rres));
      PtrList pr;
      pr.p[0] = ws.rres;
      int* slot = nullptr;
      SWCHK(take_slot(h, &slot));
      const swk::FgTail tv = tail_verify(ws, tol, tol_stop, slot);
      SWCHK(multidot(h, pr, 1, ws.rres, n, nbp, ws.nrm, nullptr, nullptr, &tv));
      int left = 0;
      SWCHK(read_slot(h, slot, &left));
      if (left != 0) {
        converged = false;
        Rcur = ws.rres;
        continue;
      }
    } else if (!converged && done < maxiter) {
      SWCHK(sys.apply(1, X, B, ws.rres));
      Rcur = ws.rres;
    }
  }
  if (iters_total) *iters_total = done;
  if (outer) h->sync_hint[hid_idx][level] = converged ? done : 0;
  return 0;
}

// A X = B at a level, preconditioned by its multigrid cycle (use_precond, above the coarsest level): fp64,
// fp64 with the complex64 cycle cast at its boundary (precond_f32), or -- in the outer solve on the lattice
// level -- with complex64 directions whose input copies are written by the producers of the Krylov vectors
static KrylovSys full_system(sw_engine* h, Hier& H, int level, int nbp, bool use_precond, bool outer) {
  Level& lv = H.lv[level];
  const bool precond = use_precond && (level < H.nlevels - 1);
  const bool pf32 = precond && h->precond_f32 && f32_capable(H, level);
  KrylovSys s;
  s.n = lv.n;
  s.apply = [h, &lv, nbp](int mode, const cplx* x, const cplx* b, cplx* y) {
    return apply_op(h, lv, mode, x, b, y, nbp);
  };
  if (pf32)
    s.precond = [h, &H, level, nbp](const cplx* v, cplx* z) { return vcycle_f32_boundary(h, H, level, v, z, nbp); };
  else if (precond)
    s.precond = [h, &H, level, nbp](const cplx* v, cplx* z) { return vcycle(h, H, level, v, z, nbp); };
  if (pf32 && outer && lv.stencil) {
    s.precond32 = [h, &H, level, nbp](const cplxf* v, cplxf* z) { return vcycle32(h, H, level, v, z, nbp); };
    s.op32 = [h, &lv, nbp](const cplxf* z, cplxf* w) {
      return launch_stencil<cplxf, cplxf>(h, lv, 0, z, nullptr, w, nbp, cplx{0.0, 0.0});
    };
    s.op32w = [h, &lv, nbp](const cplxf* z, cplx* w) {
      return launch_stencil<cplxf, cplx>(h, lv, 0, z, nullptr, w, nbp, cplx{0.0, 0.0});
    };
  }
  return s;
}

static int fgmres(sw_engine* h, Hier& H, int level, const cplx* B, cplx* X, double tol, int maxiter,
                  int m, bool outer, KrylovWS& ws, int nbp, int* iters_total, bool use_precond,
                  const cplx* aug) {
  return fgmres_loop(h, H, level, full_system(h, H, level, nbp, use_precond, outer), B, X, tol, maxiter, m,
                     outer, ws, nbp, iters_total, aug);
}

// ---------------------------------------------------------------------------------------------
// host <-> device vector movement in the reference layout
// ---------------------------------------------------------------------------------------------
// host (nb, n) <-> device [n][nbp] (pad columns zero), rows through `rowmap` when there is one
static int pack_rows(sw_engine* h, int n, const int* rowmap, int nb, const double* Xhost, cplx* dst, int nbp) {
  const size_t bytes = (size_t)nb * n * sizeof(cplx);
  SWCHK(ensure_stage(h, bytes));
  HIPCHK(hipMemcpyAsync(h->stage, Xhost, bytes, hipMemcpyHostToDevice, h->stream));
  return launch(h, T_OTHER, swk::k_pack_c, dim3((n + 63) / 64, nbp / 64), dim3(SW_BLOCK), (const cplx*)h->stage,
                nb, n, rowmap, dst, nbp);
}
static int unpack_rows(sw_engine* h, int n, const int* rowmap, int nb, const cplx* src, double* Yhost, int nbp) {
  const size_t bytes = (size_t)nb * n * sizeof(cplx);
  SWCHK(ensure_stage(h, bytes));
  SWCHK(launch(h, T_OTHER, swk::k_unpack_c, dim3((n + 63) / 64, nbp / 64), dim3(SW_BLOCK), src, nbp, n, rowmap,
               (cplx*)h->stage, nb));
  HIPCHK(hipMemcpyAsync(Yhost, h->stage, bytes, hipMemcpyDeviceToHost, h->stream));
  SWCHK(stream_sync(h));
  return 0;
}
static int pack_host(sw_engine* h, Level& lv, int nb, const double* Xhost, cplx* dst, int nbp) {
  return pack_rows(h, lv.n, (const int*)lv.rowmap, nb, Xhost, dst, nbp);
}
static int unpack_host(sw_engine* h, Level& lv, int nb, const cplx* src, double* Yhost, int nbp) {
  return unpack_rows(h, lv.n, (const int*)lv.rowmap, nb, src, Yhost, nbp);
}

static int check_hier(sw_engine* h, int hid, int level, bool need_ready) {
  if (!h) return 1;
  if (hid < 0 || hid >= SW_MAX_HIER) return sw_fail(h, "hierarchy id %d out of range", hid);
  Hier& H = h->hier[hid];
  if (H.nlevels <= 0) return sw_fail(h, "hierarchy %d not defined", hid);
  if (level < 0 || level >= H.nlevels) return sw_fail(h, "level %d out of range", level);
  if (need_ready && !H.ready) return sw_fail(h, "hierarchy %d not finalised (sw_hier_end)", hid);
  return 0;
}

// two scratch vectors per level for the building-block entry points
static int io_vectors(sw_engine* h, Level& lv, int nbp, cplx** a, cplx** b) {
  SWCHK(ensure_level_ws(h, lv, nbp));
  // the cycle never uses lv.b / lv.x of its own start level, so they are free for I/O
  *a = lv.b;
  *b = lv.x;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// What the sw_krylov_* entry points share (one operation of the Krylov solver alone on host data, for the
// per-kernel tests): small per-probe arrays host [rows][nb] <-> device [rows][nbp] with the pad columns zero
// (cx: complex entries, otherwise the real parts alone), a Krylov workspace with the life of one call, and the
// row blocking the production helper is about to choose.
// ---------------------------------------------------------------------------------------------
static int put_cols(sw_engine* h, cplx* dst, const double* src, int rows, int nb, int nbp, bool cx = true) {
  std::vector<cplx> t((size_t)rows * nbp, cplx{0.0, 0.0});
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < nb; ++c) {
      const size_t i = (size_t)r * nb + c;
      t[(size_t)r * nbp + c] = cx ? cplx{src[2 * i], src[2 * i + 1]} : cplx{src[i], 0.0};
    }
  HIPCHK(hipMemcpyAsync(dst, t.data(), t.size() * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
  return stream_sync(h);
}
static int get_cols(sw_engine* h, const cplx* src, double* dst, int rows, int nb, int nbp, bool cx = true) {
  std::vector<cplx> t((size_t)rows * nbp);
  HIPCHK(hipMemcpyAsync(t.data(), src, t.size() * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
  SWCHK(stream_sync(h));
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < nb; ++c) {
      const size_t i = (size_t)r * nb + c;
      const cplx v = t[(size_t)r * nbp + c];
      if (cx) { dst[2 * i] = v.x; dst[2 * i + 1] = v.y; }
      else dst[i] = v.x;
    }
  return 0;
}
static int put_ints(sw_engine* h, int* dst, const int32_t* src, int nb, int nbp) {
  std::vector<int> t((size_t)nbp, 0);
  for (int c = 0; c < nb; ++c) t[c] = src[c];
  HIPCHK(hipMemcpyAsync(dst, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  return stream_sync(h);
}
static int get_ints(sw_engine* h, const int* src, int32_t* dst, int nb) {
  std::vector<int> t((size_t)nb);
  HIPCHK(hipMemcpyAsync(t.data(), src, t.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  SWCHK(stream_sync(h));
  for (int c = 0; c < nb; ++c) dst[c] = t[c];
  return 0;
}
struct KrylovScope {
  sw_engine* h;
  KrylovWS ws;
  explicit KrylovScope(sw_engine* h_) : h(h_) {}
  KrylovScope(const KrylovScope&) = delete;
  KrylovScope& operator=(const KrylovScope&) = delete;
  ~KrylovScope() {
    std::string first;
    first.swap(h->err);
    (void)free_krylov(h, ws);
    h->err.swap(first);
  }
};
// info = {row blocks P, rows per block, 1 when the reduction is completed in the launch, groups of row blocks}
static void blocking_info(sw_engine* h, int n, int nbp, bool reduce, int32_t* info) {
  if (!info) return;
  int P = 0, rpb = 0;
  row_blocking(n, nbp, reduce, &P, &rpb);
  info[0] = P;
  info[1] = rpb;
  info[2] = (reduce && fused_ok(h, P, nbp)) ? 1 : 0;
  info[3] = (P + SW_RED_GROUP - 1) / SW_RED_GROUP;
}
// cnt host vectors (nb, n) -> device [cnt][n][nbp]
static int pack_vectors(sw_engine* h, int n, int nb, int nbp, int cnt, const double* src, cplx* dst) {
  for (int k = 0; k < cnt; ++k)
    SWCHK(pack_rows(h, n, nullptr, nb, src + (size_t)k * nb * n * 2, dst + (size_t)n * nbp * k, nbp));
  return 0;
}
// ... in storage C: the fp64 block itself, or its complex64 copy (k_cast: rounded to nearest) in `v32`
template <class C>
static int stored_as(sw_engine* h, cplx* v64, size_t count, DevBuf<cplxf>& v32, C** out) {
  if constexpr (std::is_same<C, cplx>::value) {
    *out = v64;
  } else {
    SWCHK(dev_realloc(h, &v32.p, count));
    SWCHK(cast_vec(h, (const cplx*)v64, v32.p, count));
    *out = v32.p;
  }
  return 0;
}
template <class CV>
static int krylov_multidot(sw_engine* h, int n, int nb, int nbp, int K, const double* V, const double* W,
                           const cplx* svec, cplx* out, cplx* coef) {
  const size_t vec = (size_t)n * nbp;
  DevBuf<cplx> v64(h);
  DevBuf<cplxf> v32(h);
  SWCHK(dev_realloc(h, &v64.p, vec * (K + 1)));       // (the K vectors and W in one block)
  SWCHK(pack_vectors(h, n, nb, nbp, K, V, v64.p));
  SWCHK(pack_vectors(h, n, nb, nbp, 1, W, v64.p + vec * K));
  CV* v = nullptr;
  SWCHK(stored_as<CV>(h, v64.p, vec * (K + 1), v32, &v));
  swk::PtrListT<CV> pl;
  for (int k = 0; k < K; ++k) pl.p[k] = v + vec * k;
  SWCHK(multidot(h, pl, K, (const CV*)(v + vec * K), n, nbp, out, svec, coef));
  return stream_sync(h);
}
template <class CV, class CW>
static int krylov_multiaxpy(sw_engine* h, int n, int nb, int nbp, int K, const double* V, const cplx* coef,
                            double sign, double* W, cplx* nrm, double* W32) {
  const size_t vec = (size_t)n * nbp;
  DevBuf<cplx> v64(h), w64(h);
  DevBuf<cplxf> v32(h), w32s(h), wcopy(h);
  SWCHK(dev_realloc(h, &v64.p, vec * K));
  SWCHK(dev_realloc(h, &w64.p, vec));
  CV* v = nullptr;
  CW* w = nullptr;
  SWCHK(pack_vectors(h, n, nb, nbp, K, V, v64.p));
  SWCHK(pack_vectors(h, n, nb, nbp, 1, W, w64.p));
  SWCHK(stored_as<CV>(h, v64.p, vec * K, v32, &v));
  SWCHK(stored_as<CW>(h, w64.p, vec, w32s, &w));
  if (W32) {
    SWCHK(dev_realloc(h, &wcopy.p, vec));
    HIPCHK(hipMemsetAsync(wcopy.p, 0xFF, vec * sizeof(cplxf), h->stream));
  }
  swk::PtrListT<CV> pl;
  for (int k = 0; k < K; ++k) pl.p[k] = v + vec * k;
  SWCHK(multiaxpy(h, pl, K, coef, sign, (const CW*)w, w, n, nbp, nrm, W32 ? wcopy.p : nullptr));   // in place
  if constexpr (!std::is_same<CW, cplx>::value) SWCHK(cast_vec(h, (const cplxf*)w, w64.p, vec));
  SWCHK(unpack_rows(h, n, nullptr, nb, w64.p, W, nbp));
  if (W32) {
    SWCHK(cast_vec(h, (const cplxf*)wcopy.p, w64.p, vec));
    SWCHK(unpack_rows(h, n, nullptr, nb, w64.p, W32, nbp));
  }
  return 0;
}

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* sw_version(void) { return "schwinger-hip 0.1 (gfx950)"; }

int sw_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* sw_last_error(sw_engine* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// Return the device memory the process-wide block pool has parked (dev_free) to the driver.
int sw_pool_trim(void) {
  std::vector<ParkedBlock> blocks;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    blocks.swap(g_pool);
    g_pool_bytes = 0;
  }
  int rc = 0;
  for (auto& b : blocks) {
    if (hipSetDevice(b.device) != hipSuccess || hipFree(b.p) != hipSuccess) rc = 1;
  }
  return rc;
}

int sw_create(sw_engine** out, int device_id) {
  if (!out) return 1;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return sw_fail(nullptr, "no HIP device available (%s); the engine has no CPU fallback",
                   e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device_id < 0 || device_id >= n)
    return sw_fail(nullptr, "device id %d out of range (have %d)", device_id, n);
  sw_engine* h = new sw_engine();
  h->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess) {
    delete h;
    return sw_fail(nullptr, "hipSetDevice(%d) failed", device_id);
  }
  if (hipStreamCreate(&h->stream) != hipSuccess || hipStreamCreate(&h->gen_stream) != hipSuccess) {
    delete h;
    return sw_fail(nullptr, "hipStreamCreate failed");
  }
  void* q = nullptr;
  void* q2 = nullptr;
  const size_t tick_bytes = (size_t)SW_TICKET_CHUNKS * (SW_RED_MAXGROUPS + 1) * sizeof(int);
  if (hipMalloc(&q, SW_NC_SLOTS * sizeof(int)) != hipSuccess || hipMalloc(&q2, tick_bytes) != hipSuccess ||
      hipMemset(q, 0, SW_NC_SLOTS * sizeof(int)) != hipSuccess || hipMemset(q2, 0, tick_bytes) != hipSuccess ||
      hipHostMalloc((void**)&h->h_notconv, sizeof(int)) != hipSuccess) {
    delete h;
    return sw_fail(nullptr, "allocation of the convergence counters failed");
  }
  h->d_notconv = (int*)q;
  h->d_tick = (int*)q2;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0)
      h->num_cus = cus;
  }
  *out = h;
  return 0;
}

int sw_destroy(sw_engine* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  if (h->gen_stream) (void)hipStreamSynchronize(h->gen_stream);
  for (auto& sl : h->slots)
    if (sl.ready) (void)hipEventDestroy(sl.ready);
  if (h->comm && g_rccl_destroy) g_rccl_destroy(h->comm);
  while (!h->allocs.empty()) (void)dev_free(h, h->allocs.back().first);     // (large blocks: parked for the next engine)
  for (auto& r : h->recs) {
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  for (auto& e : h->evpool) (void)hipEventDestroy(e);
  if (h->d_notconv) (void)hipFree(h->d_notconv);
  if (h->d_tick) (void)hipFree(h->d_tick);
  if (h->h_notconv) (void)hipHostFree(h->h_notconv);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  if (h->gen_stream) (void)hipStreamDestroy(h->gen_stream);
  delete h;
  return 0;
}

int sw_hier_begin(sw_engine* h, int hid, int nlevels) {
  if (!h) return 1;
  if (hid < 0 || hid >= SW_MAX_HIER) return sw_fail(h, "hierarchy id %d out of range", hid);
  if (nlevels < 1 || nlevels > SW_MAX_LEVELS) return sw_fail(h, "nlevels %d out of range", nlevels);
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  for (int l = 0; l < SW_MAX_LEVELS; ++l) h->sync_hint[hid][l] = 0;
  // release what the previous definition held
  for (int l = 0; l < SW_MAX_LEVELS; ++l) {
    Level& lv = H.lv[l];
    SWCHK(dev_free(h, lv.U1)); SWCHK(dev_free(h, lv.U2));
    SWCHK(free_op(h, lv.A));
    SWCHK(free_op(h, lv.P));
    SWCHK(free_op(h, lv.R));
    SWCHK(free_op(h, lv.Re));
    SWCHK(free_op(h, lv.dinv));
    for (int q = 0; q < 5; ++q) SWCHK(free_op(h, lv.eo_op[q]));
    SWCHK(dev_free(h, lv.rowmap));
    SWCHK(dev_free(h, lv.b)); SWCHK(dev_free(h, lv.x)); SWCHK(dev_free(h, lv.r));
    SWCHK(dev_free(h, lv.t));
    SWCHK(dev_free(h, lv.U1f)); SWCHK(dev_free(h, lv.U2f));
    SWCHK(dev_free(h, lv.b32)); SWCHK(dev_free(h, lv.x32)); SWCHK(dev_free(h, lv.r32));
    SWCHK(dev_free(h, lv.t32)); SWCHK(dev_free(h, lv.i32)); SWCHK(dev_free(h, lv.o32));
    SWCHK(free_krylov(h, lv.kws));
    SWCHK(free_krylov(h, lv.sws));
    SWCHK(free_krylov(h, lv.gws));
    SWCHK(dev_free(h, lv.g1)); SWCHK(dev_free(h, lv.g2));
    SWCHK(dev_free(h, lv.tv)); SWCHK(dev_free(h, lv.tv2));
    lv = Level();
  }
  SWCHK(free_op(h, H.cinv));
  H.nlevels = nlevels;
  H.ready = false;
  H.f32_valid = H.even_valid = false;
  if (hid == 0) {
    // everything that was sized or indexed by the previous definition of the reference
    // hierarchy: deflation vectors, permutations, rhs maps, probe slots and the probe workspace
    h->kd = 0;
    SWCHK(dev_free(h, h->U));
    h->U = nullptr;
    for (int l = 0; l < SW_MAX_LEVELS; ++l) {
      h->lkd[l] = 0;
      SWCHK(dev_free(h, h->lV[l]));
      h->lV[l] = nullptr;
      SWCHK(dev_free(h, h->perm_src[l]));
      h->perm_src[l] = nullptr;
      SWCHK(free_op(h, h->rhsmap[l]));
    }
    HIPCHK(hipStreamSynchronize(h->gen_stream));
    for (auto& sl : h->slots) {
      SWCHK(dev_free(h, sl.p));
      if (sl.ready) (void)hipEventDestroy(sl.ready);
    }
    h->slots.clear();
    h->pb_slot = -1;
    h->pb_probes = nullptr;
    h->pb_level = -1;
    h->pb_nb = h->pb_nbp = 0;
    h->pb_ws_nbp = 0;
    h->shifts.clear();
    h->momenta.clear();
    h->tp_momenta.clear();
    h->lm_k = 0;
    h->t3_momenta.clear();
    h->sm_sink.clear();
    h->lh_nev = 0;
    h->lh_momenta.clear();
    SWCHK(dev_free(h, h->lh_M));
    h->lh_M = nullptr;
    for (auto r : kResults) (h->*r).drop();
  }
  return 0;
}

int sw_set_lattice(sw_engine* h, int hid, int L, double mass, const double* U1, const double* U2) {
  SWCHK(check_hier(h, hid, 0, false));
  if (L < 2 || (L & 1)) return sw_fail(h, "lattice extent L=%d must be even and >= 2", L);
  if (!U1 || !U2) return sw_fail(h, "null link arrays");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[hid].lv[0];
  h->hier[hid].f32_valid = h->hier[hid].even_valid = false;
  lv.stencil = true;
  lv.L = L;
  lv.mass = mass;
  lv.n = 2 * L * L;
  SWCHK(upload(h, (double**)&lv.U1, U1, (size_t)2 * L * L));
  SWCHK(upload(h, (double**)&lv.U2, U2, (size_t)2 * L * L));
  // natural idx(s,x,y) = s*L*L + y*L + x  ->  internal ((par*Vh + ((y*L+x)>>1))*2 + s)
  const int V = L * L, Vh = V / 2;
  lv.h_rowmap.resize(lv.n);
  for (int s = 0; s < 2; ++s)
    for (int y = 0; y < L; ++y)
      for (int x = 0; x < L; ++x) {
        const int par = (x + y) & 1, sh = (y * L + x) >> 1;
        lv.h_rowmap[s * V + y * L + x] = (par * Vh + sh) * 2 + s;
      }
  SWCHK(upload(h, &lv.rowmap, lv.h_rowmap.data(), lv.h_rowmap.size()));
  return 0;
}

int sw_set_csr(sw_engine* h, int hid, int level, int n, const int64_t* indptr,
               const int32_t* indices, const double* data) {
  SWCHK(check_hier(h, hid, level, false));
  if (n <= 0 || !indptr || !indices || !data) return sw_fail(h, "sw_set_csr: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[hid].lv[level];
  h->hier[hid].f32_valid = h->hier[hid].even_valid = false;
  if (lv.stencil) {
    if (lv.n != n) return sw_fail(h, "sw_set_csr: n=%d differs from the lattice size %d", n, lv.n);
    return 0;  // the stencil is the operator; the CSR is redundant
  }
  if (lv.n && lv.n != n) return sw_fail(h, "sw_set_csr: level %d already has n=%d", level, lv.n);
  lv.n = n;
  std::vector<int> none;
  SWCHK(free_op(h, lv.A));
  SWCHK(free_op(h, lv.dinv));      // an inverse of the previous operator is stale
  SWCHK(build_ell(h, lv.A, n, n, indptr, indices, (const std::complex<double>*)data, none, none));
  return build_bsr(h, lv.A, n, indptr, indices, (const std::complex<double>*)data, 0.6);
}

int sw_set_transfer(sw_engine* h, int hid, int level, int n_f, int n_c, const int64_t* indptr,
                    const int32_t* indices, const double* data) {
  SWCHK(check_hier(h, hid, level, false));
  Hier& H = h->hier[hid];
  H.f32_valid = H.even_valid = false;
  if (level + 1 >= H.nlevels) return sw_fail(h, "no level below %d to transfer to", level);
  if (!indptr || !indices || !data) return sw_fail(h, "sw_set_transfer: null arrays");
  HIPCHK(hipSetDevice(h->device));
  Level& lf = H.lv[level];
  Level& lc = H.lv[level + 1];
  if (lf.n == 0) lf.n = n_f;
  if (lc.n == 0) lc.n = n_c;
  if (lf.n != n_f || lc.n != n_c)
    return sw_fail(h, "sw_set_transfer: shape %dx%d does not match levels (%d,%d)", n_f, n_c, lf.n,
                   lc.n);
  if (!lc.h_rowmap.empty()) return sw_fail(h, "coarse level with a row permutation unsupported");
  const std::complex<double>* cd = (const std::complex<double>*)data;
  // P: rows = fine rows in INTERNAL order
  std::vector<int> rows_int;
  if (!lf.h_rowmap.empty()) {
    rows_int.resize(n_f);
    for (int i = 0; i < n_f; ++i) rows_int[lf.h_rowmap[i]] = i;
  }
  std::vector<int> none;
  SWCHK(build_ell(h, lf.P, n_f, n_c, indptr, indices, cd, rows_int, none, 0, true));
  // R = P^H as CSR (rows = coarse), columns mapped to the fine internal order
  const int64_t nnz = indptr[n_f];
  std::vector<int64_t> rp(n_c + 1, 0);
  for (int64_t q = 0; q < nnz; ++q) rp[indices[q] + 1]++;
  for (int c = 0; c < n_c; ++c) rp[c + 1] += rp[c];
  std::vector<int32_t> ri(nnz);
  std::vector<std::complex<double>> rv(nnz);
  std::vector<int64_t> fill(rp.begin(), rp.end() - 1);
  for (int r = 0; r < n_f; ++r)
    for (int64_t q = indptr[r]; q < indptr[r + 1]; ++q) {
      const int64_t pos = fill[indices[q]]++;
      ri[pos] = r;
      rv[pos] = std::conj(cd[q]);
    }
  SWCHK(build_ell(h, lf.R, n_c, n_f, rp.data(), ri.data(), rv.data(), none, lf.h_rowmap));
  return 0;
}

int sw_set_coarsest_inv(sw_engine* h, int hid, int n, const double* dense) {
  SWCHK(check_hier(h, hid, 0, false));
  Hier& H = h->hier[hid];
  H.f32_valid = H.even_valid = false;
  Level& lv = H.lv[H.nlevels - 1];
  if (!dense || n <= 0) return sw_fail(h, "sw_set_coarsest_inv: bad arguments");
  if (lv.n == 0) lv.n = n;
  if (lv.n != n) return sw_fail(h, "coarsest inverse size %d != level size %d", n, lv.n);
  HIPCHK(hipSetDevice(h->device));
  const std::complex<double>* M = (const std::complex<double>*)dense;
  int G = 1;
  for (int g : {16, 8, 4, 2})
    if (n % g == 0) {
      G = g;
      break;
    }
  const int ng = n / G;
  std::vector<int> hc((size_t)ng * n);
  std::vector<std::complex<double>> hv((size_t)ng * n * G);
  for (int gi = 0; gi < ng; ++gi)
    for (int k = 0; k < n; ++k) {
      hc[(size_t)gi * n + k] = k;
      for (int g = 0; g < G; ++g) hv[((size_t)gi * n + k) * G + g] = M[(size_t)(gi * G + g) * n + k];
    }
  SWCHK(free_op(h, H.cinv));
  EllOp& op = H.cinv;
  op.nrows = op.ncols = n;
  op.K = n;
  op.G = G;
  op.ngroups = ng;
  SWCHK(upload(h, &op.cols, hc.data(), hc.size()));
  SWCHK(upload(h, (std::complex<double>**)&op.vals, hv.data(), hv.size()));
  op.set = true;
  if (n % 16 == 0) {
    // dense -> MFMA block-row form: every 4-column group of every 16-row tile
    const int KS = n / 4, RT = n / 16;
    std::vector<int> kcol((size_t)RT * KS);
    std::vector<std::complex<double>> pk((size_t)RT * KS * 64);
    for (int rt = 0; rt < RT; ++rt)
      for (int ks = 0; ks < KS; ++ks) {
        kcol[(size_t)rt * KS + ks] = ks * 4;
        for (int lane = 0; lane < 64; ++lane)
          pk[((size_t)rt * KS + ks) * 64 + lane] =
              M[(size_t)(rt * 16 + (lane & 15)) * n + ks * 4 + (lane >> 4)];
      }
    SWCHK(upload(h, &op.bsr_kcol, kcol.data(), kcol.size()));
    SWCHK(upload(h, (std::complex<double>**)&op.bsr_vals, pk.data(), pk.size()));
    op.bsr_KS = KS;
    op.dense_uniform = true;
  }
  return 0;
}

int sw_set_cycle(sw_engine* h, int hid, int level, int nu_pre, int nu_post, int kcycle) {
  SWCHK(check_hier(h, hid, level, false));
  if (nu_pre < 0 || nu_post < 0 || kcycle < 0 || kcycle > SW_MAXM)
    return sw_fail(h, "sw_set_cycle: bad parameters");
  Level& lv = h->hier[hid].lv[level];
  lv.nu_pre = nu_pre;
  lv.nu_post = nu_post;
  lv.kcycle = kcycle;
  return 0;
}

int sw_set_smoother(sw_engine* h, int hid, int level, int n_pre, const double* w_pre, int n_post,
                    const double* w_post) {
  SWCHK(check_hier(h, hid, level, false));
  if (n_pre < 0 || n_post < 0 || n_pre > 64 || n_post > 64)
    return sw_fail(h, "sw_set_smoother: bad step counts");
  if ((n_pre > 0 && !w_pre) || (n_post > 0 && !w_post)) return sw_fail(h, "null weights");
  Level& lv = h->hier[hid].lv[level];
  lv.w_pre.clear();
  lv.w_post.clear();
  for (int i = 0; i < n_pre; ++i) lv.w_pre.emplace_back(w_pre[2 * i], w_pre[2 * i + 1]);
  for (int i = 0; i < n_post; ++i) lv.w_post.emplace_back(w_post[2 * i], w_post[2 * i + 1]);
  lv.rich = (n_pre + n_post) > 0;
  return 0;
}

// ---- GPU-side setup of a hierarchy ------------------------------------------
int sw_setup_testvectors(sw_engine* h, int hid, int level, int nvec, uint64_t seed, int sweeps,
                         double tol, int maxiter, int precond, int32_t* iters_out) {
  SWCHK(check_hier(h, hid, level, precond != 0));
  if (nvec != SW_TV) return sw_fail(h, "the device setup works with %d test vectors per half", SW_TV);
  if (sweeps < 0 || maxiter < 1) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  Level& lv = H.lv[level];
  if (lv.n <= 0 || (!lv.stencil && !lv.A.set)) return sw_fail(h, "level %d has no operator yet", level);
  const int nbp = 64;
  const size_t cnt = (size_t)lv.n * nbp;
  if (!lv.tv2) SWCHK(dev_realloc(h, &lv.tv2, cnt));
  if (!lv.tv || seed != 0) {
    if (!lv.tv) SWCHK(dev_realloc(h, &lv.tv, cnt));
    SWCHK(launch(h, T_OTHER, swk::k_fill_random, dim3((lv.n + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK),
                 dim3(SW_BLOCK), lv.tv, lv.n, nbp, nvec, (unsigned long long)(seed ? seed : 7)));
  }
  // the solver's own restart in both modes: ONE Krylov workspace (2 m + 2 vectors of 64 columns, tens
  // of GB on a 1024^2 lattice) serves the setup and the solves that follow
  const int m = std::min(h->restart, maxiter);
  for (int sw = 0; sw < sweeps; ++sw) {
    SWCHK(ensure_krylov(h, lv.sws, m, lv.n, nbp, true));
    int total = 0;
    // V <- A_l^-1 V (inexact): inverse iteration amplifies the near-kernel the coarse space must hold
    SWCHK(fgmres(h, H, level, lv.tv, lv.tv2, tol, maxiter, m, true, lv.sws, nbp, &total, precond != 0));
    SWCHK(stream_sync(h));
    std::swap(lv.tv, lv.tv2);
    if (iters_out) iters_out[sw] = total;
  }
  return 0;
}

int sw_setup_transfer(sw_engine* h, int hid, int level, int nblocks, int rpb, const int32_t* blk_rows,
                      int G, int K, const int32_t* pcols, const int64_t* pmap, const int32_t* porder) {
  SWCHK(check_hier(h, hid, level, false));
  Hier& H = h->hier[hid];
  H.f32_valid = H.even_valid = false;
  if (level + 1 >= H.nlevels) return sw_fail(h, "no level below %d", level);
  if (!blk_rows || !pcols || !pmap || nblocks <= 0 || rpb <= 0) return sw_fail(h, "bad arguments");
  if (rpb > 512) return sw_fail(h, "aggregate blocks of %d rows exceed the QR kernel's 512", rpb);
  if (G != 1 && G != 2 && G != 4 && G != 8 && G != 16) return sw_fail(h, "bad group size %d", G);
  HIPCHK(hipSetDevice(h->device));
  Level& lf = H.lv[level];
  Level& lc = H.lv[level + 1];
  const int n_f = lf.n, n_c = nblocks * SW_TV;
  if ((long long)nblocks * rpb != n_f) return sw_fail(h, "blocks do not tile level %d", level);
  if (n_f % G) return sw_fail(h, "group size %d does not divide n = %d", G, n_f);
  if (!lf.tv) return sw_fail(h, "level %d has no test vectors (sw_setup_testvectors)", level);
  if (lc.n != 0 && lc.n != n_c) return sw_fail(h, "level %d already has n = %d", level + 1, lc.n);
  if (!lc.h_rowmap.empty()) return sw_fail(h, "coarse level with a row permutation unsupported");
  lc.n = n_c;
  for (size_t i = 0; i < (size_t)nblocks * rpb; ++i)
    if (blk_rows[i] < 0 || blk_rows[i] >= n_f) return sw_fail(h, "block member row out of range");
  const int ng = n_f / G;
  for (size_t i = 0; i < (size_t)ng * K; ++i)
    if (pcols[i] < 0 || pcols[i] >= n_c) return sw_fail(h, "prolongator column out of range");
  const long long qcount = (long long)nblocks * rpb * SW_TV;
  for (size_t i = 0; i < (size_t)ng * K * G; ++i)
    if (pmap[i] >= qcount) return sw_fail(h, "prolongator value map out of range");
  SWCHK(free_op(h, lf.R));
  SWCHK(free_op(h, lf.P));
  // R = P^H in grouped-ELL form: group = block, G = SW_TV rows (the block's coarse dofs), K = rpb
  EllOp& R = lf.R;
  R.nrows = n_c;
  R.ncols = n_f;
  R.K = rpb;
  R.G = SW_TV;
  R.ngroups = nblocks;
  SWCHK(upload(h, &R.cols, (const int*)blk_rows, (size_t)nblocks * rpb));
  SWCHK(dev_realloc(h, &R.vals, (size_t)qcount));
  DevBuf<cplx> Q(h);
  SWCHK(dev_realloc(h, &Q.p, (size_t)qcount));
  // rows per lane 1, 2, 4 or 8 (8 x 8 aggregates of a block level: BASELINE config 5's 3-level hierarchy)
  SWCHK(pick_ge<64, 128, 256, 512>(rpb, [&](auto RPB) {
    return launch(h, T_OTHER, swk::k_block_qr<RPB / 64>,
                  dim3((nblocks + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK), dim3(SW_BLOCK), (const cplx*)lf.tv,
                  64, (const int*)R.cols, nblocks, rpb, Q, R.vals);
  }));
  R.set = true;
  // P: structure from the host (geometry), values gathered from Q
  EllOp& P = lf.P;
  P.nrows = n_f;
  P.ncols = n_c;
  P.K = K;
  P.G = G;
  P.ngroups = ng;
  SWCHK(upload(h, &P.cols, (const int*)pcols, (size_t)ng * K));
  if (porder) {
    std::vector<char> seen(ng, 0);
    for (int i = 0; i < ng; ++i) {
      if (porder[i] < 0 || porder[i] >= ng || seen[porder[i]]) return sw_fail(h, "porder is not a permutation");
      seen[porder[i]] = 1;
    }
    SWCHK(upload(h, &P.order, (const int*)porder, (size_t)ng));
  }
  const size_t pv = (size_t)ng * K * G;
  SWCHK(dev_realloc(h, &P.vals, pv));
  DevBuf<long long> dmap(h);
  SWCHK(upload(h, &dmap.p, (const long long*)pmap, pv));
  SWCHK(launch(h, T_OTHER, swk::k_fill_from_map, dim3(4096), dim3(SW_BLOCK), (const long long*)dmap,
               (const cplx*)Q, P.vals, pv));
  P.set = true;
  // the coarse image of the test vectors is the starting guess one level down
  if (!lc.tv) SWCHK(dev_realloc(h, &lc.tv, (size_t)n_c * 64));
  SWCHK(launch_ell(h, R, 0, lf.tv, nullptr, lc.tv, 64, T_R));
  return stream_sync(h);
}

int sw_setup_galerkin(sw_engine* h, int hid, int level, int Lc, const int32_t* nbr) {
  SWCHK(check_hier(h, hid, level, false));
  Hier& H = h->hier[hid];
  H.f32_valid = H.even_valid = false;
  if (level + 1 >= H.nlevels) return sw_fail(h, "no level below %d", level);
  if (!nbr || Lc < 4 || (Lc & 3)) return sw_fail(h, "coarse lattice extent %d must be a multiple of 4", Lc);
  if (!h->use_mfma || !h->mfma_ops) return sw_fail(h, "the device setup needs use_mfma = mfma_ops = 1");
  HIPCHK(hipSetDevice(h->device));
  Level& lf = H.lv[level];
  Level& lc = H.lv[level + 1];
  const int ncs = Lc * Lc, n_c = ncs * 16, n_f = lf.n;
  if (lc.n != n_c) return sw_fail(h, "level %d has n = %d, expected %d sites x 16", level + 1, lc.n, ncs);
  if (!lf.P.set || !lf.R.set) return sw_fail(h, "transfer operators of level %d not set", level);
  for (int i = 0; i < ncs * 5; ++i)
    if (nbr[i] < 0 || nbr[i] >= ncs) return sw_fail(h, "neighbour site out of range");
  for (int I = 0; I < ncs; ++I)
    for (int a = 1; a < 5; ++a)
      for (int b = 0; b < a; ++b)
        if (nbr[I * 5 + a] == nbr[I * 5 + b]) return sw_fail(h, "neighbour lists must hold five distinct sites");
  const int nbp = 256;
  DevBuf<cplx> Y(h), X(h), E(h);     // released E, X, Y: the block pool hands X's block out first
  SWCHK(dev_realloc(h, &E.p, (size_t)n_c * nbp));
  SWCHK(dev_realloc(h, &X.p, (size_t)n_f * nbp));
  SWCHK(dev_realloc(h, &Y.p, (size_t)n_f * nbp));
  SWCHK(launch(h, T_OTHER, swk::k_probe_unit, dim3((n_c + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK),
               dim3(SW_BLOCK), E, Lc, nbp));
  SWCHK(launch_ell(h, lf.P, 0, E, nullptr, X, nbp, T_P));          // X = P E
  SWCHK(apply_op(h, lf, 0, X, nullptr, Y, nbp));                   // Y = A X
  SWCHK(launch_ell(h, lf.R, 0, Y, nullptr, E, nbp, T_R));          // Z = R Y  (over E)
  DevBuf<int> dnbr(h);
  SWCHK(upload(h, &dnbr.p, (const int*)nbr, (size_t)ncs * 5));
  SWCHK(free_op(h, lc.A));
  EllOp& A = lc.A;
  A.nrows = A.ncols = n_c;
  A.bsr_KS = 20;
  SWCHK(dev_realloc(h, &A.bsr_vals, (size_t)ncs * 20 * 64));
  SWCHK(dev_realloc(h, &A.bsr_kcol, (size_t)ncs * 20));
  SWCHK(launch(h, T_OTHER, swk::k_bsr_from_probe, dim3((ncs * 20 + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK),
               dim3(SW_BLOCK), (const cplx*)E, nbp, (const int*)dnbr, Lc, A.bsr_vals, A.bsr_kcol));
  A.set = true;
  SWCHK(stream_sync(h));
  {
    // the k-step columns are 16 nbr + 4 g: the own-site-last property can be read off nbr
    bool last = Lc > 1;
    for (int I = 0; I < ncs && last; ++I) last = nbr[I * 5 + 4] == I;
    A.bsr_diag_last = last;
  }
  return 0;
}

// In-place inverse of the dense row-major n x n matrix D on the device: Gauss-Jordan with partial
// pivoting (the device counterpart of np.linalg.inv at multigrid.py:342-344); hand-written kernels, no
// library handle involved.  Four small launches per pivot step.
// In-place inverse of the dense row-major [n][n] matrix D: Gauss-Jordan with partial pivoting.  Blocked
// (option gj_block, default 32 columns; n a multiple of 64): the pivot steps of a panel update the panel
// only (n x nb), after which the panel is N = G E -- the panel's composite transformation applied to the unit
// columns -- and every other column c becomes a[:, c] (pivot rows zeroed) + N a[pivot rows, c]: one rank-nb
// update on the fp64 matrix cores (k_bsr_mfma3 in residual mode on the negated panel, the matrix as nbp = n
// "probes").  n = 4096: 0.355 s -> see profiles/r03_ab_sessions.txt (r03ab).
static int gj_invert(sw_engine* h, cplx* D, int n) {
  DevBuf<cplx> colk(h), pvinv(h);
  DevBuf<int> pivs(h);
  SWCHK(dev_realloc(h, &colk.p, (size_t)n));
  SWCHK(dev_realloc(h, &pvinv.p, (size_t)1));
  SWCHK(dev_realloc(h, &pivs.p, (size_t)n + 1));
  int* info = pivs + n;
  HIPCHK(hipMemsetAsync(info, 0, sizeof(int), h->stream));
  const int nb = (h->gj_block >= 8 && h->gj_block % 8 == 0 && n % 64 == 0 && n % h->gj_block == 0 &&
                  n >= 4 * h->gj_block && h->use_mfma && h->mfma_3m) ? h->gj_block : 0;
  const dim3 g1((n + SW_BLOCK - 1) / SW_BLOCK);
  auto pivot_step = [&](int k, int c0, int cn) {
    const dim3 gu((cn + 63) / 64, (n + 16 * SW_WAVES_PER_BLOCK - 1) / (16 * SW_WAVES_PER_BLOCK));
    hipLaunchKernelGGL(swk::k_gj_pivot, dim3(1), dim3(1024), 0, h->stream, (const cplx*)D, n, k, pivs, pvinv,
                       info);
    hipLaunchKernelGGL(swk::k_gj_swap_rows, dim3((cn + SW_BLOCK - 1) / SW_BLOCK), dim3(SW_BLOCK), 0, h->stream, D,
                       n, k, (const int*)pivs, c0, cn);
    hipLaunchKernelGGL(swk::k_gj_column_and_scale, g1, dim3(SW_BLOCK), 0, h->stream, D, n, k,
                       (const cplx*)pvinv, colk, c0, cn);
    hipLaunchKernelGGL(swk::k_gj_update, gu, dim3(SW_BLOCK), 0, h->stream, D, n, k, (const cplx*)colk, c0, cn);
    h->launches += 4;
  };
  if (nb == 0) {
    for (int k = 0; k < n; ++k) {
      pivot_step(k, 0, n);
      // keep the queue shallow: thousands of back-to-back launches without a host sync overran
      // rocprofv3's per-dispatch counter buffers (FETCH_SIZE pass, n = 2048: segmentation fault inside
      // the tool); a drain every 256 pivot steps costs nothing measurable
      if ((k & 255) == 255) HIPCHK(hipStreamSynchronize(h->stream));
    }
  } else {
    DevBuf<cplx> T(h), pvals(h);
    DevBuf<int> pkcol(h);
    SWCHK(dev_realloc(h, &T.p, (size_t)nb * n));
    SWCHK(dev_realloc(h, &pvals.p, (size_t)(n / 16) * (nb / 4) * 64));
    SWCHK(dev_realloc(h, &pkcol.p, (size_t)(n / 16) * (nb / 4)));
    EllOp pn;                       // -N of the current panel in block-row form
    pn.nrows = n;
    pn.ncols = nb;
    pn.bsr_KS = nb / 4;
    pn.bsr_vals = pvals;
    pn.bsr_kcol = pkcol;
    pn.set = true;
    const size_t items = (size_t)(n / 16) * pn.bsr_KS;
    for (int k0 = 0; k0 < n; k0 += nb) {
      if (nb <= 64) {
        for (int k = k0; k < k0 + nb; ++k) {
          hipLaunchKernelGGL(swk::k_gj_pivot_panel, dim3(1), dim3(1024), 0, h->stream, D, n, k, k0, nb, pivs, info);
          hipLaunchKernelGGL(swk::k_gj_update_panel, dim3((n + 16 * SW_WAVES_PER_BLOCK - 1) / (16 * SW_WAVES_PER_BLOCK)),
                             dim3(SW_BLOCK), 0, h->stream, D, n, k, k0, nb);
        }
        h->launches += 2 * nb;
      } else {
        for (int k = k0; k < k0 + nb; ++k) pivot_step(k, k0, nb);
      }
      hipLaunchKernelGGL(swk::k_gj_block_rows, g1, dim3(SW_BLOCK), 0, h->stream, D, n, k0, nb, (const int*)pivs, T);
      hipLaunchKernelGGL(swk::k_gj_panel_to_bsr, dim3((unsigned)((items + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK)),
                         dim3(SW_BLOCK), 0, h->stream, (const cplx*)D, n, k0, nb, pn.bsr_vals, pn.bsr_kcol);
      KLAUNCH_CHECK();
      h->launches += 2;
      SWCHK(launch_bsr(h, pn, 1, T, D, D, n, T_OTHER, cplx{0.0, 0.0}));
      if (((k0 / nb) & 7) == 7) HIPCHK(hipStreamSynchronize(h->stream));      // (shallow queue, as above)
    }
    SWCHK(stream_sync(h));
  }
  hipLaunchKernelGGL(swk::k_gj_unpermute, g1, dim3(SW_BLOCK), 0, h->stream, D, n, (const int*)pivs);
  KLAUNCH_CHECK();
  h->launches += 1;
  int hinfo = 0;
  HIPCHK(hipMemcpyAsync(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  SWCHK(stream_sync(h));
  if (hinfo != 0) return sw_fail(h, "Gauss-Jordan inverse: the matrix is singular");
  return 0;
}

// Zero the dense row-major [n][n] matrix D and expand op into it: its block-row form over all n / 16 row tiles, or
// over a subset of them (bsr_tmap) with colrank[site tile] the dense tile of each column, where it has one; else
// its grouped-ELL form (sw_set_csr builds both from one CSR: each kernel writes every non-zero once and skips zeros).
static int op_to_dense(sw_engine* h, const EllOp& op, int n, cplx* D, const int* colrank) {
  HIPCHK(hipMemsetAsync(D, 0, (size_t)n * n * sizeof(cplx), h->stream));
  if (op.bsr_KS > 0 && (!op.bsr_tmap || colrank)) {
    const int items = (n / 16) * op.bsr_KS;
    return launch(h, T_OTHER, swk::k_bsr_to_dense, dim3((items + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK),
                  dim3(SW_BLOCK), (const cplx*)op.bsr_vals, (const int*)op.bsr_kcol, n / 16, op.bsr_KS, n, D, colrank,
                  (const int*)nullptr);
  }
  if (op.cols && op.vals) {
    const size_t total = (size_t)op.ngroups * op.K * op.G;
    return launch(h, T_OTHER, swk::k_ell_to_dense, dim3((unsigned)((total + SW_BLOCK - 1) / SW_BLOCK)),
                  dim3(SW_BLOCK), (const int*)op.cols, (const cplx*)op.vals, op.K, op.G, op.ngroups, n, D);
  }
  return sw_fail(h, "operator in neither grouped-ELL nor block-row form");
}

// op <- the block-row form of the dense row-major [n][n] matrix D, as an operator of `rows` rows: every 4-column
// group of each of its n / 16 row tiles.  tmap (optional, with its device copy d_tmap): dense tile t is the
// level's site tile tmap[t], for rows and columns.
static int dense_to_bsr(sw_engine* h, EllOp& op, int rows, const cplx* D, int n, const std::vector<int>* tmap,
                        const int* d_tmap) {
  SWCHK(free_op(h, op));
  op.nrows = op.ncols = rows;
  op.bsr_RT = n / 16;
  op.bsr_KS = n / 4;
  if (tmap) SWCHK(upload(h, &op.bsr_tmap, tmap->data(), tmap->size()));
  const size_t items = (size_t)op.bsr_RT * op.bsr_KS;
  SWCHK(dev_realloc(h, &op.bsr_vals, items * 64));
  SWCHK(dev_realloc(h, &op.bsr_kcol, items));
  SWCHK(launch(h, T_OTHER, swk::k_dense_to_bsr, dim3((unsigned)((items + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK)),
               dim3(SW_BLOCK), D, n, op.bsr_vals, op.bsr_kcol, d_tmap));
  op.set = true;
  op.dense_uniform = true;     // k_dense_to_bsr: the column list depends on the k-step only
  return 0;
}

int sw_setup_invert_coarsest(sw_engine* h, int hid) {
  SWCHK(check_hier(h, hid, 0, false));
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  H.f32_valid = H.even_valid = false;
  Level& lv = H.lv[H.nlevels - 1];
  if (H.nlevels < 2 || !lv.A.set) return sw_fail(h, "coarsest level has no operator");
  const int n = lv.n;
  if (n % 16) return sw_fail(h, "coarsest size %d is not a multiple of 16", n);
  if (n > 8192) return sw_fail(h, "coarsest size %d too large for the in-engine dense inverse", n);
  DevBuf<cplx> D(h);
  SWCHK(dev_realloc(h, &D.p, (size_t)n * n));
  SWCHK(op_to_dense(h, lv.A, n, D, nullptr));
  SWCHK(gj_invert(h, D, n));
  SWCHK(dense_to_bsr(h, H.cinv, n, D, n, nullptr, nullptr));
  return stream_sync(h);
}

// The dense coarsest inverse the engine holds (set by the caller or formed on the device) as a row-major
// complex128[n*n] host array: multigrid.py:342-344's coarsest_inv for callers that read the attribute
// (stoch_trace.py:428-435 traces it directly).
int sw_get_coarsest_inv(sw_engine* h, int hid, double* dense) {
  SWCHK(check_hier(h, hid, 0, false));
  if (!dense) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  const EllOp& op = h->hier[hid].cinv;
  if (!op.set) return sw_fail(h, "coarsest inverse missing");
  const int n = op.nrows;
  DevBuf<cplx> D(h);
  SWCHK(dev_realloc(h, &D.p, (size_t)n * n));
  SWCHK(op_to_dense(h, op, n, D, nullptr));
  HIPCHK(hipMemcpyAsync(dense, D, (size_t)n * n * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
  return stream_sync(h);
}

static int schur_apply(sw_engine* h, Level& lv, int mode, const cplx* X, const cplx* Bp, cplx* Y, int nbp);
static int dot_into(sw_engine* h, const cplx* A, const cplx* Bv, int n, int nbp, cplx* out);

// The dense inverse of a block level's even-odd Schur complement, formed ON THE DEVICE from the level's
// Schur operator (eo_op[0], 9-point in 16 x 16 blocks over the even sites): S -> dense (ne*16)^2 ->
// Gauss-Jordan -> block-row form over the even sites' tiles = even-odd operator 4, with which the cycle
// solves the level exactly (vcycle_rich) instead of smoothing it.  Counterpart of np.linalg.inv at
// multigrid.py:342-344 one level up.
int sw_setup_direct_level(sw_engine* h, int hid, int level) {
  SWCHK(check_hier(h, hid, level, false));
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  H.f32_valid = false;
  Level& lv = H.lv[level];
  const EllOp& S = lv.eo_op[0];
  if (lv.stencil || !S.set || !S.bsr_tmap || S.bsr_RT <= 0 || !lv.eo_op[1].set || !lv.eo_op[2].set ||
      !lv.eo_op[3].set)
    return sw_fail(h, "level %d has no even-odd operators (sw_setup_eo_operators / sw_set_eo_operator)", level);
  const int ne = S.bsr_RT, n = ne * 16, ns = lv.n / 16;
  if (n > 8192) return sw_fail(h, "Schur complement of %d rows too large for the in-engine dense inverse", n);
  std::vector<int> E(ne), erank(ns, -1);
  HIPCHK(hipMemcpy(E.data(), S.bsr_tmap, (size_t)ne * sizeof(int), hipMemcpyDeviceToHost));
  for (int r = 0; r < ne; ++r) {
    if (E[r] < 0 || E[r] >= ns || erank[E[r]] >= 0) return sw_fail(h, "level %d: bad tile map of the Schur operator", level);
    erank[E[r]] = r;
  }
  std::vector<int> kc((size_t)ne * S.bsr_KS);
  HIPCHK(hipMemcpy(kc.data(), S.bsr_kcol, kc.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int c : kc)
    if (erank[c >> 4] < 0) return sw_fail(h, "level %d: the Schur operator reaches an odd site", level);
  DevBuf<int> d_rank(h), d_E(h);
  SWCHK(upload(h, &d_rank.p, erank.data(), erank.size()));
  SWCHK(upload(h, &d_E.p, E.data(), E.size()));
  DevBuf<cplx> D(h);
  SWCHK(dev_realloc(h, &D.p, (size_t)n * n));
  SWCHK(op_to_dense(h, S, n, D, d_rank));
  SWCHK(gj_invert(h, D, n));
  SWCHK(dense_to_bsr(h, lv.eo_op[4], lv.n, D, n, &E, d_E));
  return stream_sync(h);
}

// Dense inverse of a small level's operator (n <= 8192, n % 16 == 0; grouped-ELL operator from sw_set_csr, or the
// block-row operator of a device-built level), formed on the device and kept as the level's direct solver:
// solves that START at this level (the MLMC coarse solves A_c^-1 R x of utils.py:306-329 on the reference
// hierarchy's small levels, the fine solves of its coarse difference levels) are then two applications of the
// inverse around one residual -- x = A^-1 b, x += A^-1 (b - A x) -- instead of a multigrid-preconditioned FGMRES
// of hundreds of tiny launches.  The refinement step takes the Gauss-Jordan inverse's residual (eps cond(A),
// ~1e-11) below the solver tolerance.  The level keeps its operator, transfers and smoother for cycles
// that merely pass through it.
int sw_setup_level_inverse(sw_engine* h, int hid, int level) {
  SWCHK(check_hier(h, hid, level, false));
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  Level& lv = H.lv[level];
  const int n = lv.n;
  if (lv.stencil) return sw_fail(h, "level %d is the lattice level", level);
  if (n <= 0 || n % 16 || n > 8192) return sw_fail(h, "level %d: size %d not a multiple of 16 or above 8192", level, n);
  if (!lv.A.set) return sw_fail(h, "level %d has no operator", level);
  DevBuf<cplx> D(h);
  SWCHK(dev_realloc(h, &D.p, (size_t)n * n));
  SWCHK(op_to_dense(h, lv.A, n, D, nullptr));
  SWCHK(gj_invert(h, D, n));
  SWCHK(dense_to_bsr(h, lv.dinv, n, D, n, nullptr, nullptr));
  H.f32_valid = false;
  return stream_sync(h);
}

// Arnoldi relation of a level's operator for the smoother polynomial (hierarchy.smoother_weights fits
// the weights 1/theta_k to the harmonic Ritz values of H): `degree` steps from a pseudo-random start
// vector, classical Gram-Schmidt twice, all on the device -- the host receives the (degree+1) x degree
// Hessenberg matrix only (row-major complex128).  which = 0: the level operator A_l; which = 1: the
// even-odd Schur complement S of the level (stencil level: half vectors through k_schur_step; block
// levels: eo_op[0] on the even sites' rows).
int sw_setup_arnoldi(sw_engine* h, int hid, int level, int which, int degree, uint64_t seed, double* Hout) {
  SWCHK(check_hier(h, hid, level, false));
  if (degree < 1 || degree > SW_MAXM || !Hout || (which != 0 && which != 1))
    return sw_fail(h, "sw_setup_arnoldi: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  Level& lv = H.lv[level];
  if (lv.n <= 0 || (!lv.stencil && !lv.A.set)) return sw_fail(h, "level %d has no operator yet", level);
  const bool schur = which == 1;
  if (schur && !lv.stencil && !(lv.eo_op[0].set && lv.eo_op[0].bsr_tmap))
    return sw_fail(h, "level %d has no even-odd Schur operator", level);
  if (schur && lv.stencil && (lv.n % 2)) return sw_fail(h, "odd lattice level");
  const int nbp = 64;
  const int n = (schur && lv.stencil) ? lv.n / 2 : lv.n;     // rows of the vectors the operator acts on
  const size_t vec = (size_t)n * nbp;
  DevBuf<cplx> V(h);      // degree + 1 basis vectors
  DevBuf<cplx> d(h);      // [2][degree + 1][nbp] dots of the two passes, + [nbp] norm
  SWCHK(dev_realloc(h, &V.p, vec * (degree + 1)));
  SWCHK(dev_realloc(h, &d.p, (size_t)(2 * (degree + 1) + 1) * nbp));
  cplx* d1 = d;
  cplx* d2 = d + (size_t)(degree + 1) * nbp;
  cplx* nr = d + (size_t)2 * (degree + 1) * nbp;
  auto normalise = [&](cplx* w) -> int {
    return launch(h, T_AXPY, swk::k_colscale,
                  dim3(std::min(4096, (n + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK), 1), dim3(SW_BLOCK), w,
                  (const cplx*)nr, n, nbp);
  };
  auto apply = [&](const cplx* x, cplx* y) -> int {
    if (!schur) return apply_op(h, lv, 0, x, nullptr, y, nbp);
    if (lv.stencil) return schur_apply(h, lv, 0, x, nullptr, y, nbp);
    SWCHK(zero_vec(h, y, n, nbp));
    return launch_bsr(h, lv.eo_op[0], 0, x, nullptr, y, nbp, T_MVM, cplx{0.0, 0.0});
  };
  // start vector: one pseudo-random column (the other 63 stay zero), on the rows the operator acts on
  {
    cplx* tmp = (schur && !lv.stencil) ? V + vec : V;
    SWCHK(launch(h, T_OTHER, swk::k_fill_random, dim3((n + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK),
                 dim3(SW_BLOCK), tmp, n, nbp, 1, (unsigned long long)(seed ? seed : 2024)));
    if (schur && !lv.stencil) {
      SWCHK(zero_vec(h, V, n, nbp));
      const int items = lv.eo_op[0].bsr_RT * 16;
      SWCHK(launch(h, T_OTHER, swk::k_copy_tiles, dim3((items + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK),
                   dim3(SW_BLOCK), (const cplx*)tmp, (const int*)lv.eo_op[0].bsr_tmap, lv.eo_op[0].bsr_RT, nbp, V));
    }
    SWCHK(dot_into(h, V, V, n, nbp, nr));
    SWCHK(normalise(V));
  }
  std::vector<std::complex<double>> Hm((size_t)(degree + 1) * degree, std::complex<double>(0.0, 0.0));
  std::vector<std::complex<double>> hd((size_t)(2 * (degree + 1) + 1) * nbp);
  for (int j = 0; j < degree; ++j) {
    cplx* w = V + vec * (j + 1);
    SWCHK(apply(V + vec * j, w));
    PtrList pv;
    for (int k = 0; k <= j; ++k) pv.p[k] = V + vec * k;
    SWCHK(multidot(h, pv, j + 1, (const cplx*)w, n, nbp, d1));
    SWCHK(multiaxpy(h, pv, j + 1, d1, -1.0, (const cplx*)w, w, n, nbp, nullptr));
    SWCHK(multidot(h, pv, j + 1, (const cplx*)w, n, nbp, d2));
    SWCHK(multiaxpy(h, pv, j + 1, d2, -1.0, (const cplx*)w, w, n, nbp, nr));
    SWCHK(stream_sync(h));
    HIPCHK(hipMemcpy(hd.data(), d, hd.size() * sizeof(cplx), hipMemcpyDeviceToHost));
    for (int k = 0; k <= j; ++k)
      Hm[(size_t)k * degree + j] = hd[(size_t)k * nbp] + hd[(size_t)(degree + 1 + k) * nbp];
    const double hn = std::sqrt(std::max(0.0, hd[(size_t)2 * (degree + 1) * nbp].real()));
    Hm[(size_t)(j + 1) * degree + j] = hn;
    if (!(hn > 0.0)) break;      // invariant subspace: the remaining columns stay zero
    SWCHK(normalise(w));
  }
  SWCHK(stream_sync(h));
  std::memcpy(Hout, Hm.data(), Hm.size() * sizeof(std::complex<double>));
  return 0;
}

int sw_get_level_dense(sw_engine* h, int hid, int level, double* dense) {
  SWCHK(check_hier(h, hid, level, false));
  if (!dense) return sw_fail(h, "null output");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[hid].lv[level];
  const EllOp& A = lv.A;
  if (!A.set || A.bsr_KS <= 0) return sw_fail(h, "level %d has no block-row operator", level);
  const int n = lv.n, RT = n / 16, KS = A.bsr_KS;
  std::vector<std::complex<double>> vals((size_t)RT * KS * 64);
  std::vector<int> kcol((size_t)RT * KS);
  SWCHK(stream_sync(h));
  HIPCHK(hipMemcpy(vals.data(), A.bsr_vals, vals.size() * sizeof(cplx), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(kcol.data(), A.bsr_kcol, kcol.size() * sizeof(int), hipMemcpyDeviceToHost));
  std::complex<double>* D = (std::complex<double>*)dense;
  std::fill(D, D + (size_t)n * n, std::complex<double>(0, 0));
  for (int rt = 0; rt < RT; ++rt)
    for (int ks = 0; ks < KS; ++ks)
      for (int lane = 0; lane < 64; ++lane) {
        const int row = rt * 16 + (lane & 15), col = kcol[(size_t)rt * KS + ks] + (lane >> 4);
        D[(size_t)row * n + col] += vals[((size_t)rt * KS + ks) * 64 + lane];
      }
  return 0;
}

int sw_set_gmres_smoother(sw_engine* h, int hid, int level, int m, int cycles) {
  SWCHK(check_hier(h, hid, level, false));
  if (m < 0 || m > SW_MAXM || (m > 0 && cycles < 1) || cycles > 16)
    return sw_fail(h, "sw_set_gmres_smoother: need 0 <= m <= %d and 1 <= cycles <= 16", SW_MAXM);
  Level& lv = h->hier[hid].lv[level];
  lv.gm_m = m;
  lv.gm_cycles = m > 0 ? cycles : 0;
  return 0;
}

int sw_set_eo_operator(sw_engine* h, int hid, int level, int which, int RT, int KS, const int32_t* tmap,
                       const int32_t* kcol, const double* vals) {
  SWCHK(check_hier(h, hid, level, false));
  if (which < 0 || which > 4) return sw_fail(h, "even-odd operator index %d out of [0,4]", which);
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[hid].lv[level];
  h->hier[hid].f32_valid = h->hier[hid].even_valid = false;
  if (lv.stencil || lv.n <= 0 || lv.n % 16) return sw_fail(h, "level %d is not a block level", level);
  if (RT <= 0 || KS <= 0 || (KS & 3) || !tmap || !kcol || !vals) return sw_fail(h, "bad arguments");
  const int tiles = lv.n / 16;
  for (int i = 0; i < RT; ++i)
    if (tmap[i] < 0 || tmap[i] >= tiles) return sw_fail(h, "tile map entry out of range");
  for (size_t i = 0; i < (size_t)RT * KS; ++i)
    if (kcol[i] < 0 || kcol[i] + 4 > lv.n) return sw_fail(h, "k-step column out of range");
  EllOp& op = lv.eo_op[which];
  SWCHK(free_op(h, op));
  if (which < 4) SWCHK(free_op(h, lv.eo_op[4]));     // an inverse of the previous S is stale
  op.nrows = op.ncols = lv.n;
  op.bsr_RT = RT;
  op.bsr_KS = KS;
  SWCHK(upload(h, &op.bsr_tmap, (const int*)tmap, (size_t)RT));
  SWCHK(upload(h, &op.bsr_kcol, (const int*)kcol, (size_t)RT * KS));
  SWCHK(upload(h, (std::complex<double>**)&op.bsr_vals, (const std::complex<double>*)vals,
               (size_t)RT * KS * 64));
  op.set = true;
  check_diag_last(op, kcol, tmap);
  if (which == 4) {
    // a dense inverse: every row tile lists the same columns in the same order?
    bool uni = true;
    for (int r = 1; r < RT && uni; ++r) uni = std::memcmp(kcol, kcol + (size_t)r * KS, sizeof(int32_t) * KS) == 0;
    op.dense_uniform = uni;
  }
  return 0;
}

// The four even-odd operators of a block level built ON THE DEVICE from its operator in block-row form
// (5-point stencil of 16 x 16 blocks, own site last -- what sw_setup_galerkin produces):
//   G = D_oo^-1 (k_block_inverse),  F = A_eo G,  Hb = G A_oe,  S = D_ee - F A_oe (k_block_products);
// the index structure is derived here from the operator's own k-step columns.
int sw_setup_eo_operators(sw_engine* h, int hid, int level, int Lc) {
  SWCHK(check_hier(h, hid, level, false));
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  H.f32_valid = H.even_valid = false;
  Level& lv = H.lv[level];
  const int ns = Lc * Lc;
  if (lv.stencil || Lc < 8 || (Lc & 1) || lv.n != ns * 16)
    return sw_fail(h, "level %d is not a block level of %d x %d sites (extent even, >= 8)", level, Lc, Lc);
  const EllOp& A = lv.A;
  if (!A.set || A.bsr_KS != 20 || !A.bsr_vals || !A.bsr_kcol || A.bsr_tmap)
    return sw_fail(h, "level %d has no 5-point block-row operator (20 k-steps per site)", level);
  std::vector<int> kc((size_t)ns * 20);
  HIPCHK(hipMemcpy(kc.data(), A.bsr_kcol, kc.size() * sizeof(int), hipMemcpyDeviceToHost));
  // nbr[s][j]: the site block j of row site s acts on; the own site must be block 4
  std::vector<int> nbr((size_t)ns * 5);
  auto parity = [&](int s) { return ((s % Lc) + (s / Lc)) & 1; };
  for (int s = 0; s < ns; ++s)
    for (int j = 0; j < 5; ++j) {
      const int t = kc[(size_t)s * 20 + 4 * j] / 16;
      for (int g = 0; g < 4; ++g)
        if (kc[(size_t)s * 20 + 4 * j + g] != 16 * t + 4 * g)
          return sw_fail(h, "level %d: k-step columns are not whole site blocks", level);
      if (t < 0 || t >= ns || (j == 4 ? t != s : parity(t) == parity(s)))
        return sw_fail(h, "level %d: not a nearest-neighbour operator with the own site last", level);
      nbr[(size_t)s * 5 + j] = t;
    }
  // The row tiles of the four operators are listed -- i.e. WALKED by the block-row kernel, XCD band by XCD band --
  // in lattice tiles of 16 x 16 sites (SW_EO_WALK_TILE) on lattices of 32 x 32 sites and more: a row of S reads the x tiles of nine
  // sites, and in plain lattice order the neighbours in y are a whole lattice row of x tiles apart (128 sites x
  // 32 KiB = 4 MB at 128 probes: the size of an XCD's L2), so they came from the fabric every time -- 2.73 GB
  // fetched per launch of the 262144-row level's Schur step against 0.84 GB algorithmic
  // (profiles/kernel_pmc_1024.json).  An 8 x 8 tile with its halo is 3.2 MB of x.  (Output tiles go through tmap,
  // columns through kcol: the order of the list is free.)
  std::vector<int> walk(ns);
  for (int s = 0; s < ns; ++s) walk[s] = s;
  if (Lc >= 32 && Lc % 16 == 0) {
    const char* te_ = std::getenv("SW_EO_WALK_TILE");
    // (1024^2, 128 probes, strict: lattice order 508.7 probe-samples/s, tiles of 4 / 8 / 16 sites 512.7 / 515.1 / 521.3;
    // the Schur step of the 262144-row level 395 -> 342 us and 2.73 -> 1.90 GB fetched with 8: r04r / r04s)
    const int T = (te_ && std::atoi(te_) > 0 && Lc % std::atoi(te_) == 0) ? std::atoi(te_) : 16, tpr = Lc / T;
    std::stable_sort(walk.begin(), walk.end(), [&](int a, int b) {
      const int ta = ((a / Lc) / T) * tpr + (a % Lc) / T, tb = ((b / Lc) / T) * tpr + (b % Lc) / T;
      return ta < tb;
    });
  }
  std::vector<int> E, O, rank(ns);
  for (int s : walk) {
    std::vector<int>& v = parity(s) ? O : E;
    rank[s] = (int)v.size();
    v.push_back(s);
  }
  const int ne = (int)E.size(), no = (int)O.size();
  // the nine even targets of S, own site LAST (k_bsr_mfma's register shortcut)
  static const int disp[9][2] = {{2, 0}, {-2, 0}, {0, 2}, {0, -2}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}, {0, 0}};
  auto site_at = [&](int s, int dx, int dy) {
    const int x = ((s % Lc) + dx + Lc) % Lc, y = ((s / Lc) + dy + Lc) % Lc;
    return y * Lc + x;
  };
  auto slot_of = [&](int e, int t) {
    for (int q = 0; q < 9; ++q)
      if (site_at(e, disp[q][0], disp[q][1]) == t) return q;
    return -1;
  };
  struct Built {
    std::vector<int> tmap, kcol;
    int KS;
  };
  auto shape = [&](const std::vector<int>& rows, int nblk, auto&& target) {
    Built b;
    b.KS = 4 * nblk;
    b.tmap = rows;
    b.kcol.resize(rows.size() * (size_t)b.KS);
    for (size_t r = 0; r < rows.size(); ++r)
      for (int q = 0; q < nblk; ++q)
        for (int g = 0; g < 4; ++g) b.kcol[r * b.KS + 4 * q + g] = 16 * target((int)r, q) + 4 * g;
    return b;
  };
  Built bS = shape(E, 9, [&](int r, int q) { return site_at(E[r], disp[q][0], disp[q][1]); });
  Built bF = shape(E, 4, [&](int r, int q) { return nbr[(size_t)E[r] * 5 + q]; });
  Built bG = shape(O, 1, [&](int r, int) { return O[r]; });
  Built bH = shape(O, 4, [&](int r, int q) { return nbr[(size_t)O[r] * 5 + q]; });
  Built* built[4] = {&bS, &bF, &bG, &bH};
  SWCHK(free_op(h, lv.eo_op[4]));                      // an inverse of the previous S is stale
  for (int w = 0; w < 4; ++w) {
    EllOp& op = lv.eo_op[w];
    SWCHK(free_op(h, op));
    op.nrows = op.ncols = lv.n;
    op.bsr_RT = (int)built[w]->tmap.size();
    op.bsr_KS = built[w]->KS;
    SWCHK(upload(h, &op.bsr_tmap, built[w]->tmap.data(), built[w]->tmap.size()));
    SWCHK(upload(h, &op.bsr_kcol, built[w]->kcol.data(), built[w]->kcol.size()));
    SWCHK(dev_realloc(h, &op.bsr_vals, (size_t)op.bsr_RT * op.bsr_KS * 64));
    op.set = true;
    check_diag_last(op, built[w]->kcol.data(), built[w]->tmap.data());
  }
  const cplx* Av = A.bsr_vals;
  auto ablk = [](int s, int j) { return ((long long)s * 20 + 4 * j) * 64; };          // block j of row site s in A
  auto oblk = [](int r, int nblk, int q) { return ((long long)r * nblk + q) * 256; };   // block q of row r
  DevBuf<int> info(h);
  SWCHK(dev_realloc(h, &info.p, (size_t)1));
  HIPCHK(hipMemsetAsync(info, 0, sizeof(int), h->stream));
  // G
  {
    std::vector<long long> so(no), dof(no);
    for (int r = 0; r < no; ++r) {
      so[r] = ablk(O[r], 4);
      dof[r] = oblk(r, 1, 0);
    }
    DevBuf<long long> dso(h), ddo(h);
    SWCHK(upload(h, &dso.p, so.data(), so.size()));
    SWCHK(upload(h, &ddo.p, dof.data(), dof.size()));
    SWCHK(launch(h, T_OTHER, swk::k_block_inverse, dim3(no), dim3(256), Av, (const long long*)dso,
                 lv.eo_op[2].bsr_vals, (const long long*)ddo, info));
    SWCHK(stream_sync(h));
  }
  auto products = [&](const std::vector<int>& ptr, const std::vector<long long>& ao,
                      const std::vector<long long>& bo, const cplx* Ab, const cplx* Bb,
                      const std::vector<long long>& io, double sign, cplx* out,
                      const std::vector<long long>& oo) -> int {
    DevBuf<int> dptr(h);
    DevBuf<long long> dao(h), dbo(h), dio(h), doo(h);
    SWCHK(upload(h, &dptr.p, ptr.data(), ptr.size()));
    SWCHK(upload(h, &dao.p, ao.data(), ao.size()));
    SWCHK(upload(h, &dbo.p, bo.data(), bo.size()));
    SWCHK(upload(h, &dio.p, io.data(), io.size()));
    SWCHK(upload(h, &doo.p, oo.data(), oo.size()));
    SWCHK(launch(h, T_OTHER, swk::k_block_products, dim3((unsigned)oo.size()), dim3(256), (const int*)dptr,
                 (const long long*)dao, (const long long*)dbo, Ab, Bb, (const long long*)dio, Av, sign, out,
                 (const long long*)doo));
    return stream_sync(h);
  };
  const cplx* Gv = lv.eo_op[2].bsr_vals;
  // F(e, j) = A(e, j) G(o_j);  Hb(o, j) = G(o) A(o, j)
  {
    std::vector<int> ptr;
    std::vector<long long> ao, bo, io, oo;
    for (int r = 0; r < ne; ++r)
      for (int j = 0; j < 4; ++j) {
        ptr.push_back((int)ao.size());
        ao.push_back(ablk(E[r], j));
        bo.push_back(oblk(rank[nbr[(size_t)E[r] * 5 + j]], 1, 0));
        io.push_back(-1);
        oo.push_back(oblk(r, 4, j));
      }
    ptr.push_back((int)ao.size());
    SWCHK(products(ptr, ao, bo, Av, Gv, io, 1.0, lv.eo_op[1].bsr_vals, oo));
  }
  {
    std::vector<int> ptr;
    std::vector<long long> ao, bo, io, oo;
    for (int r = 0; r < no; ++r)
      for (int j = 0; j < 4; ++j) {
        ptr.push_back((int)ao.size());
        ao.push_back(oblk(r, 1, 0));
        bo.push_back(ablk(O[r], j));
        io.push_back(-1);
        oo.push_back(oblk(r, 4, j));
      }
    ptr.push_back((int)ao.size());
    SWCHK(products(ptr, ao, bo, Gv, Av, io, 1.0, lv.eo_op[3].bsr_vals, oo));
  }
  // S(e, slot) = [slot == own] D(e) - sum over (j, j') with target(o_j, j') in that slot of F(e, j) A(o_j, j')
  {
    std::vector<int> ptr;
    std::vector<long long> ao, bo, io, oo;
    for (int r = 0; r < ne; ++r) {
      std::vector<std::pair<long long, long long>> lists[9];
      for (int j = 0; j < 4; ++j) {
        const int o = nbr[(size_t)E[r] * 5 + j];
        for (int jp = 0; jp < 4; ++jp) {
          const int q = slot_of(E[r], nbr[(size_t)o * 5 + jp]);
          if (q < 0) return sw_fail(h, "level %d: a two-hop target is outside the nine-point pattern", level);
          lists[q].push_back({oblk(r, 4, j), ablk(o, jp)});
        }
      }
      for (int q = 0; q < 9; ++q) {
        ptr.push_back((int)ao.size());
        for (auto& pr : lists[q]) {
          ao.push_back(pr.first);
          bo.push_back(pr.second);
        }
        io.push_back(q == 8 ? ablk(E[r], 4) : -1);
        oo.push_back(oblk(r, 9, q));
      }
    }
    ptr.push_back((int)ao.size());
    SWCHK(products(ptr, ao, bo, lv.eo_op[1].bsr_vals, Av, io, -1.0, lv.eo_op[0].bsr_vals, oo));
  }
  int hinfo = 0;
  HIPCHK(hipMemcpy(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost));
  if (hinfo != 0) return sw_fail(h, "level %d: a diagonal block of an odd site is singular", level);
  return 0;
}

// Y = op X for one of a block level's even-odd operators (which: 0 S, 1 F, 2 G, 3 Hb) on full-length
// level vectors in the reference layout; rows the operator does not write come back zero
int sw_apply_eo_operator(sw_engine* h, int hid, int level, int which, int nb, const double* X, double* Y) {
  SWCHK(check_hier(h, hid, level, false));
  if (which < 0 || which > 4 || nb <= 0 || !X || !Y) return sw_fail(h, "sw_apply_eo_operator: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[hid].lv[level];
  if (lv.stencil || !lv.eo_op[which].set) return sw_fail(h, "level %d has no even-odd operator %d", level, which);
  const int nbp = pad64(nb);
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(pack_host(h, lv, nb, X, a, nbp));
  SWCHK(zero_vec(h, b, lv.n, nbp));
  SWCHK(launch_bsr(h, lv.eo_op[which], 0, a, nullptr, b, nbp, T_MVM, cplx{0.0, 0.0}));
  return unpack_host(h, lv, nb, b, Y, nbp);
}

int sw_get_level_bsr(sw_engine* h, int hid, int level, int* KS, int32_t* kcol, double* vals) {
  SWCHK(check_hier(h, hid, level, false));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[hid].lv[level];
  const EllOp& A = lv.A;
  if (!A.set || A.bsr_KS <= 0) return sw_fail(h, "level %d has no block-row operator", level);
  if (KS) *KS = A.bsr_KS;
  if (!kcol || !vals) return 0;     // size query
  SWCHK(stream_sync(h));
  const size_t items = (size_t)(lv.n / 16) * A.bsr_KS;
  HIPCHK(hipMemcpy(kcol, A.bsr_kcol, items * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(vals, A.bsr_vals, items * 64 * sizeof(cplx), hipMemcpyDeviceToHost));
  return 0;
}

int sw_set_eo_smoother(sw_engine* h, int hid, int level, int n_post, const double* w_post) {
  SWCHK(check_hier(h, hid, level, false));
  if (n_post < 0 || n_post > 64 || (n_post > 0 && !w_post)) return sw_fail(h, "sw_set_eo_smoother: bad arguments");
  Level& lv = h->hier[hid].lv[level];
  if (n_post > 0 && !lv.stencil && !(lv.eo_op[0].set && lv.eo_op[1].set && lv.eo_op[2].set && lv.eo_op[3].set))
    return sw_fail(h, "level %d: the even-odd operators are not set (sw_set_eo_operator)", level);
  lv.w_eo.clear();
  for (int i = 0; i < n_post; ++i) lv.w_eo.emplace_back(w_post[2 * i], w_post[2 * i + 1]);
  if (!swp::product_form(lv.w_eo, lv.q_w, lv.q_beta)) lv.q_w.clear();
  if (n_post > 0) lv.rich = true;     // the cycle with fixed weights (vcycle_rich)
  h->hier[hid].even_valid = false;
  return 0;
}

int sw_hier_end(sw_engine* h, int hid) {
  SWCHK(check_hier(h, hid, 0, false));
  Hier& H = h->hier[hid];
  H.f32_valid = H.even_valid = false;
  for (int l = 0; l < H.nlevels; ++l) {
    Level& lv = H.lv[l];
    if (lv.n <= 0) return sw_fail(h, "level %d has no size", l);
    if (l < H.nlevels - 1) {
      if (!lv.stencil && !lv.A.set) return sw_fail(h, "level %d has no operator", l);
      if (!lv.P.set) return sw_fail(h, "level %d has no prolongator", l);
    }
  }
  if (H.nlevels > 1 && !H.cinv.set) return sw_fail(h, "coarsest inverse missing");
  if (H.nlevels == 1 && !H.lv[0].stencil && !H.lv[0].A.set)
    return sw_fail(h, "single-level hierarchy has no operator");
  // the coarsest level may also carry its operator (optional)
  H.ready = true;
  return 0;
}

int sw_set_solver(sw_engine* h, int restart, int solver_hid) {
  if (!h) return 1;
  if (restart < 1 || restart > SW_MAXM) return sw_fail(h, "restart %d out of [1,%d]", restart, SW_MAXM);
  if (solver_hid < 0 || solver_hid >= SW_MAX_HIER) return sw_fail(h, "bad solver hierarchy id");
  h->restart = restart;
  h->solver_hid = solver_hid;
  return 0;
}

int sw_set_option(sw_engine* h, const char* name, double value) {
  if (!h || !name) return 1;
  for (const EngineOption& o : kOptions)
    if (o.set && std::strcmp(name, o.name) == 0) {
      if (o.ok && !o.ok(value)) return sw_fail(h, "%s", o.msg);
      o.set(h, value);
      return 0;
    }
  return sw_fail(h, "unknown option %s", name);
}

// ---- device eigensolver: block subspace iteration with the engine's own batched solves as the
// shift-invert (the counterpart of eigs(A_l, k, sigma=0) at multigrid.py:174 and of
// eigsh(gamma_3 A, k, sigma=0) at utils.py:140).  The engine supplies the O(n) work on blocks of 64
// vectors -- W = Op^-1 V, the 64 x 64 Gram matrices V^H W, W^H W, block rotations V <- W Y -- the caller
// the 64 x 64 dense algebra in between (Rayleigh-Ritz, Cholesky-QR).
static int solve_dev(sw_engine* h, int hid, int level0, const cplx* B, cplx* X, double tol, int maxiter,
                     int nbp, int* total);
static int diff_levels(sw_engine* h, int level, int skip, int* fine_hid, int* lcoarse);
static int diff_apply(sw_engine* h, int fine_hid, int level, int lcoarse, const cplx* x, int nbp, cplx* z, cplx* ca,
                      cplx* cb, double tol, int maxiter, int count_nb, const cplx** y, int* total_f);
static int eig_check(sw_engine* h, int a) {
  if (h->eig_n <= 0 || !h->eig_buf[0]) return sw_fail(h, "sw_eig_begin has not been called");
  if (a < 0 || a > 2) return sw_fail(h, "block buffer index %d out of 0..2", a);
  return 0;
}

int sw_eig_begin(sw_engine* h, int hid, int level, uint64_t seed) {
  return sw_eig_begin_wide(h, hid, level, seed, 64);
}

// Blocks of `width` vectors (a multiple of 64, at most 512): width/64 groups, each an [n][64] array like
// the buffers of width 64; the other sw_eig_* calls then act on all groups.
int sw_eig_begin_wide(sw_engine* h, int hid, int level, uint64_t seed, int width) {
  SWCHK(check_hier(h, hid, level, true));
  if (width < 64 || width > 512 || (width & 63)) return sw_fail(h, "block width %d: a multiple of 64 in 64..512", width);
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[hid].lv[level];
  if (lv.n <= 0 || (lv.n & 3)) return sw_fail(h, "level %d has n = %d (a multiple of 4 is needed)", level, lv.n);
  const size_t cnt = (size_t)lv.n * width;
  for (int q = 0; q < 3; ++q) SWCHK(dev_realloc(h, &h->eig_buf[q], cnt));
  SWCHK(dev_realloc(h, &h->eig_small, (size_t)width * width));
  h->eig_w = width;
  for (int q = 0; q < 2; ++q) {     // sized for the level below this one on first use of sw_eig_apply_diff
    if (h->eig_cs[q]) SWCHK(dev_free(h, h->eig_cs[q]));
    h->eig_cs[q] = nullptr;
  }
  // gamma_3 = +1 on the first half of the REFERENCE order, -1 on the second (multigrid.py:130-133)
  std::vector<signed char> sg(lv.n);
  for (int i = 0; i < lv.n; ++i) {
    const int r = lv.h_rowmap.empty() ? i : lv.h_rowmap[i];
    sg[r] = (i < lv.n / 2) ? 1 : -1;
  }
  SWCHK(upload(h, &h->eig_sign, (const signed char*)sg.data(), (size_t)lv.n));
  h->eig_hid = hid;
  h->eig_level = level;
  h->eig_n = lv.n;
  for (int g = 0; g < width / 64; ++g) {
    SWCHK(launch(h, T_OTHER, swk::k_fill_random, dim3((lv.n + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK),
                 dim3(SW_BLOCK), h->eig_buf[0] + (size_t)g * lv.n * 64, lv.n, 64, 64,
                 (unsigned long long)(seed ? seed : 11) + 0x632be59bd9b4e019ull * (unsigned long long)g));
  }
  return stream_sync(h);
}

int sw_eig_end(sw_engine* h) {
  if (!h) return 1;
  for (int q = 0; q < 3; ++q) {
    if (h->eig_buf[q]) SWCHK(dev_free(h, h->eig_buf[q]));
    h->eig_buf[q] = nullptr;
  }
  if (h->eig_sign) SWCHK(dev_free(h, h->eig_sign));
  h->eig_sign = nullptr;
  if (h->eig_small) SWCHK(dev_free(h, h->eig_small));
  h->eig_small = nullptr;
  for (int q = 0; q < 2; ++q) {
    if (h->eig_cs[q]) SWCHK(dev_free(h, h->eig_cs[q]));
    h->eig_cs[q] = nullptr;
  }
  h->eig_n = 0;
  h->eig_w = 64;
  h->eig_hid = h->eig_level = -1;
  return 0;
}

// Overwrite the first ncols columns of block buffer `dst` with host vectors (reference order, ncols
// contiguous vectors of length n), e.g. converged vectors of the level above as a start.
int sw_eig_load(sw_engine* h, int dst, int ncols, const double* X) {
  SWCHK(eig_check(h, dst));
  if (ncols < 1 || ncols > h->eig_w || !X) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[h->eig_hid].lv[h->eig_level];
  const int spare = dst == 2 ? 1 : 2;
  const size_t gs = (size_t)lv.n * 64;
  // per group: pack into a spare buffer (all 64 columns written, zero beyond ncols), then copy the columns over
  for (int g = 0; g * 64 < ncols; ++g) {
    const int nc = std::min(64, ncols - g * 64);
    SWCHK(pack_host(h, lv, nc, X + (size_t)g * 64 * lv.n * 2, h->eig_buf[spare], 64));
    HIPCHK(hipMemcpy2DAsync(h->eig_buf[dst] + g * gs, 64 * sizeof(cplx), h->eig_buf[spare], 64 * sizeof(cplx),
                            (size_t)nc * sizeof(cplx), (size_t)lv.n, hipMemcpyDeviceToDevice, h->stream));
  }
  return stream_sync(h);
}

// dst = Op^-1 src on all columns (one batched solve of 64 per group): mode 0 Op = A_level (multigrid.py:174), mode 1 Op = gamma_3 A_level
// (utils.py:137-140; Q^-1 = A^-1 gamma_3).  Batched solve of the (hierarchy, level) to `tol`.
int sw_eig_solve(sw_engine* h, int src, int dst, int mode, double tol, int maxiter, int32_t* iters_max) {
  SWCHK(eig_check(h, src));
  SWCHK(eig_check(h, dst));
  if (src == dst) return sw_fail(h, "source and destination buffers must differ");
  if (mode != 0 && mode != 1) return sw_fail(h, "mode must be 0 (A) or 1 (gamma_3 A)");
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[h->eig_hid];
  Level& lv = H.lv[h->eig_level];
  const size_t gs = (size_t)lv.n * 64;
  int worst = 0;
  for (int g = 0; g < h->eig_w / 64; ++g) {
    const cplx* rhs = h->eig_buf[src] + g * gs;
    if (mode == 1) {
      cplx* tmp = h->eig_buf[3 - src - dst] + g * gs;
      SWCHK(launch(h, T_OTHER, swk::k_row_sign, dim3((lv.n + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK, 1),
                   dim3(SW_BLOCK), rhs, (const signed char*)h->eig_sign, tmp, lv.n, 64));
      rhs = tmp;
    }
    int total = 0;
    SWCHK(solve_dev(h, h->eig_hid, h->eig_level, rhs, h->eig_buf[dst] + g * gs, tol, maxiter, 64, &total));
    SWCHK(stream_sync(h));
    worst = std::max(worst, total);
  }
  if (iters_max) *iters_max = worst;
  return 0;
}

// dst = (A_l^-1 - P A_c^-1 R) Gamma src on all columns (64 per pass), l = the level of sw_eig_begin on hierarchy 0:
// the MLMC difference operator of utils.py:141-143 / multigrid.py:461-549 through diff_apply, the helper the probe
// body of sw_hutch_run applies too.  Gamma = gamma_3 (g3 = 1) or the identity (g3 = 0); skip = 1: A_0^-1 - P_0 P_1
// A_2^-1 R_1 R_0.  The third eigen buffer and two coarse blocks of the eigen state are the scratch; the probe
// workspace is not touched.
int sw_eig_apply_diff(sw_engine* h, int src, int dst, int skip, int g3, double tol, int maxiter,
                      int32_t* iters_max) {
  SWCHK(eig_check(h, src));
  SWCHK(eig_check(h, dst));
  if (src == dst) return sw_fail(h, "source and destination buffers must differ");
  if (g3 != 0 && g3 != 1) return sw_fail(h, "g3 must be 0 (identity) or 1 (gamma_3)");
  if (skip != 0 && skip != 1) return sw_fail(h, "skip must be 0 or 1");
  if (maxiter < 1) return sw_fail(h, "maxiter must be >= 1");
  if (h->eig_hid != 0) return sw_fail(h, "the difference operator needs the eigen buffers on hierarchy 0");
  HIPCHK(hipSetDevice(h->device));
  Hier& H0 = h->hier[0];
  const int level = h->eig_level;
  if (skip && (level != 0 || H0.nlevels < 3))
    return sw_fail(h, "level skipping is defined for level 0 of a hierarchy with at least three levels");
  int fine_hid, lcoarse;
  SWCHK(diff_levels(h, level, skip, &fine_hid, &lcoarse));
  Level& lv = H0.lv[level];
  const int n = lv.n;
  // two coarse blocks of the level below (with skip the level two below is smaller and fits in them)
  for (int q = 0; q < 2; ++q)
    if (!h->eig_cs[q]) SWCHK(dev_realloc(h, &h->eig_cs[q], (size_t)H0.lv[level + 1].n * 64));
  int worst = 0;
  for (int g = 0; g < h->eig_w / 64; ++g) {
    const size_t go = (size_t)g * n * 64;   // this group of 64 columns
    cplx* t = h->eig_buf[3 - src - dst] + go;
    cplx* d = h->eig_buf[dst] + go;
    // x = Gamma src (in dst: it is overwritten last)
    const cplx* x = h->eig_buf[src] + go;
    if (g3) {
      SWCHK(launch(h, T_OTHER, swk::k_row_sign, dim3((n + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK, 1),
                   dim3(SW_BLOCK), x, (const signed char*)h->eig_sign, d, n, 64));
      x = d;
    }
    // t = A_l^-1 x, y = the coarse solution on the level below, dst = t - P y
    const cplx* y;
    int total_f = 0;
    SWCHK(diff_apply(h, fine_hid, level, lcoarse, x, 64, t, h->eig_cs[0], h->eig_cs[1], tol, maxiter, 0, &y,
                     &total_f));
    SWCHK(launch_ell(h, lv.P, 1, y, t, d, 64, T_P));
    SWCHK(stream_sync(h));
    worst = std::max(worst, total_f);
  }
  if (iters_max) *iters_max = worst;
  return 0;
}

// out[w*w] (row-major complex128) = buf_a^H buf_b, w = the block width (64: k_block_gram)
int sw_eig_gram(sw_engine* h, int a, int b, double* out) {
  SWCHK(eig_check(h, a));
  SWCHK(eig_check(h, b));
  if (!out) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  const int n = h->eig_n;
  const int w = h->eig_w;
  if (w > 64) {
    // ~1024 workgroups over (row slice, group pair), 8..256 slices of at least 64 rows
    const int ng = w / 64;
    const int pw = std::max(8, std::min(256, 1024 / (ng * ng)));
    const int rpbw = std::max(64, (n + pw - 1) / pw);
    const int Pw = (n + rpbw - 1) / rpbw;
    SWCHK(ensure_partial(h, (size_t)Pw * w * w * sizeof(cplx)));
    SWCHK(launch(h, T_DOTS, swk::k_block_gram_wide, dim3(Pw, ng, ng), dim3(SW_BLOCK), (const cplx*)h->eig_buf[a],
                 (const cplx*)h->eig_buf[b], n, rpbw, w, h->partial));
    SWCHK(launch(h, T_DOTS, swk::k_reduce_partials, dim3(w, ng), dim3(SW_BLOCK), (const cplx*)h->partial, Pw, w,
                 w, h->eig_small, (const cplx*)nullptr, (cplx*)nullptr));
    HIPCHK(hipMemcpyAsync(out, h->eig_small, (size_t)w * w * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
    return stream_sync(h);
  }
  int rpb = std::max(64, ((n + 255) / 256 + 3) & ~3);     // ~256 row blocks, multiples of 4 rows
  const int P = (n + rpb - 1) / rpb;
  SWCHK(ensure_partial(h, (size_t)P * 4096 * sizeof(cplx)));
  SWCHK(launch(h, T_DOTS, swk::k_block_gram, dim3(P, 4), dim3(SW_BLOCK), (const cplx*)h->eig_buf[a],
               (const cplx*)h->eig_buf[b], n, rpb, h->partial));
  SWCHK(launch(h, T_DOTS, swk::k_block_gram_reduce, dim3(64), dim3(64), (const cplx*)h->partial, P,
               h->eig_small));
  HIPCHK(hipMemcpyAsync(out, h->eig_small, 4096 * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
  return stream_sync(h);
}

// buf_dst = buf_src Y (sub < 0) or buf_dst = buf_sub - buf_src Y, Y[w*w] row-major complex128 (dst != src)
int sw_eig_rotate(sw_engine* h, int src, const double* Y, int dst, int sub) {
  SWCHK(eig_check(h, src));
  SWCHK(eig_check(h, dst));
  if (sub >= 0) SWCHK(eig_check(h, sub));
  if (src == dst || !Y) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  const int w = h->eig_w;
  if (w > 64) {
    HIPCHK(hipMemcpyAsync(h->eig_small, Y, (size_t)w * w * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
    SWCHK(launch(h, T_AXPY, swk::k_block_rotate_wide, dim3((h->eig_n + 63) / 64, w / 64), dim3(SW_BLOCK),
                 (const cplx*)h->eig_buf[src], (const cplx*)h->eig_small,
                 (const cplx*)(sub >= 0 ? h->eig_buf[sub] : nullptr), h->eig_buf[dst], h->eig_n, w));
    return stream_sync(h);
  }
  HIPCHK(hipMemcpyAsync(h->eig_small, Y, 4096 * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
  SWCHK(launch(h, T_AXPY, swk::k_block_rotate, dim3(std::min(2048, h->eig_n / SW_WAVES_PER_BLOCK)),
               dim3(SW_BLOCK), (const cplx*)h->eig_buf[src], (const cplx*)h->eig_small,
               (const cplx*)(sub >= 0 ? h->eig_buf[sub] : nullptr), h->eig_buf[dst], h->eig_n));
  return stream_sync(h);
}

// The first k columns of buf_src as k host vectors of length n in the reference order.
int sw_eig_fetch(sw_engine* h, int src, int k, double* out) {
  SWCHK(eig_check(h, src));
  if (k < 1 || k > h->eig_w || !out) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[h->eig_hid].lv[h->eig_level];
  for (int g = 0; g * 64 < k; ++g)
    SWCHK(unpack_host(h, lv, std::min(64, k - g * 64), h->eig_buf[src] + (size_t)g * lv.n * 64,
                      out + (size_t)g * 64 * lv.n * 2, 64));
  return 0;
}

// Current value of an engine option (what a caller saves before an A/B run and restores afterwards), or of
// one of the read-only statistics of kOptions.
int sw_get_option(sw_engine* h, const char* name, double* value) {
  if (!h || !name || !value) return 1;
  for (const EngineOption& o : kOptions)
    if (std::strcmp(name, o.name) == 0) {
      *value = o.get(h);
      return 0;
    }
  return sw_fail(h, "unknown option %s", name);
}

int sw_set_deflation(sw_engine* h, int k, const double* U) {
  SWCHK(check_hier(h, 0, 0, false));
  if (k < 0 || k > SW_MAX_DEFL) return sw_fail(h, "deflation rank %d out of [0,%d]", k, SW_MAX_DEFL);
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  h->kd = 0;
  h->lm_k = 0;   // the low-mode inverse belongs to the vectors it was formed with
  if (k == 0) return 0;
  if (!U) return sw_fail(h, "null deflation vectors");
  if (lv.n <= 0) return sw_fail(h, "level 0 undefined");
  const std::complex<double>* Uh = (const std::complex<double>*)U;
  const int ld = defl_ld(k);
  std::vector<std::complex<double>> Ui((size_t)lv.n * ld);
  for (int i = 0; i < lv.n; ++i) {
    const int r = lv.h_rowmap.empty() ? i : lv.h_rowmap[i];
    for (int q = 0; q < k; ++q) Ui[(size_t)r * ld + q] = Uh[(size_t)i * k + q];
  }
  SWCHK(upload(h, (std::complex<double>**)&h->U, Ui.data(), Ui.size()));
  h->kd = k;
  return 0;
}

int sw_set_level_deflation(sw_engine* h, int level, int k, const double* V) {
  SWCHK(check_hier(h, 0, level, false));
  if (k < 0 || k > SW_MAX_DEFL) return sw_fail(h, "deflation rank %d out of [0,%d]", k, SW_MAX_DEFL);
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[level];
  h->lkd[level] = 0;
  if (k == 0) return 0;
  if (!V) return sw_fail(h, "null deflation vectors");
  if (lv.n <= 0) return sw_fail(h, "level %d undefined", level);
  const std::complex<double>* Vh = (const std::complex<double>*)V;
  const int ld = defl_ld(k);
  std::vector<std::complex<double>> Vi((size_t)lv.n * ld);
  for (int i = 0; i < lv.n; ++i) {
    const int r = lv.h_rowmap.empty() ? i : lv.h_rowmap[i];
    for (int q = 0; q < k; ++q) Vi[(size_t)r * ld + q] = Vh[(size_t)i * k + q];
  }
  SWCHK(upload(h, (std::complex<double>**)&h->lV[level], Vi.data(), Vi.size()));
  h->lkd[level] = k;
  return 0;
}

int sw_set_perm(sw_engine* h, int level, int64_t shift) {
  SWCHK(check_hier(h, 0, level, false));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[level];
  if (shift < 0) {
    SWCHK(dev_free(h, h->perm_src[level]));
    h->perm_src[level] = nullptr;
    return 0;
  }
  if (lv.n <= 0) return sw_fail(h, "level %d undefined", level);
  if (shift >= lv.n) return sw_fail(h, "shift %lld >= n", (long long)shift);
  // (Pperm^T v)[i] = v[(i - shift) mod n]   (multigrid.py:151-153)
  std::vector<int> src(lv.n);
  for (int i = 0; i < lv.n; ++i) {
    const int s = (int)(((int64_t)i - shift + lv.n) % lv.n);
    const int ri = lv.h_rowmap.empty() ? i : lv.h_rowmap[i];
    const int rs = lv.h_rowmap.empty() ? s : lv.h_rowmap[s];
    src[ri] = rs;
  }
  SWCHK(upload(h, &h->perm_src[level], src.data(), src.size()));
  return 0;
}

int sw_set_rhsmap(sw_engine* h, int level, int n, const int64_t* indptr, const int32_t* indices,
                  const double* data) {
  SWCHK(check_hier(h, 0, level, false));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[level];
  if (lv.n != n) return sw_fail(h, "rhs map size %d != level size %d", n, lv.n);
  SWCHK(free_op(h, h->rhsmap[level]));
  std::vector<int> rows_int;
  if (!lv.h_rowmap.empty()) {
    rows_int.resize(n);
    for (int i = 0; i < n; ++i) rows_int[lv.h_rowmap[i]] = i;
  }
  return build_ell(h, h->rhsmap[level], n, n, indptr, indices, (const std::complex<double>*)data,
                   rows_int, lv.h_rowmap, 1);
}

// ---- building blocks ---------------------------------------------------------------------
static int simple_op(sw_engine* h, int hid, int level, int nb, const double* X, double* Y, int what) {
  SWCHK(check_hier(h, hid, level, true));
  if (nb <= 0 || !X || !Y) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  const int nbp = pad64(nb);
  Level& lv = H.lv[level];
  cplx *a, *b;
  if (what == 0) {  // dirac
    if (level == H.nlevels - 1 && !lv.stencil && !lv.A.set)
      return sw_fail(h, "coarsest level operator was not supplied");
    SWCHK(io_vectors(h, lv, nbp, &a, &b));
    SWCHK(pack_host(h, lv, nb, X, a, nbp));
    SWCHK(apply_op(h, lv, 0, a, nullptr, b, nbp));
    return unpack_host(h, lv, nb, b, Y, nbp);
  }
  if (what == 3) {  // coarsest inverse
    Level& ll = H.lv[H.nlevels - 1];
    SWCHK(io_vectors(h, ll, nbp, &a, &b));
    SWCHK(pack_host(h, ll, nb, X, a, nbp));
    SWCHK(apply_coarsest(h, H, a, b, nbp));
    return unpack_host(h, ll, nb, b, Y, nbp);
  }
  if (level + 1 >= H.nlevels) return sw_fail(h, "no transfer at the coarsest level");
  Level& lc = H.lv[level + 1];
  cplx *c, *d;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(io_vectors(h, lc, nbp, &c, &d));
  if (what == 1) {  // restrict
    SWCHK(pack_host(h, lv, nb, X, a, nbp));
    SWCHK(launch_ell(h, lv.R, 0, a, nullptr, c, nbp, T_R));
    return unpack_host(h, lc, nb, c, Y, nbp);
  }
  SWCHK(pack_host(h, lc, nb, X, c, nbp));
  SWCHK(launch_ell(h, lv.P, 0, c, nullptr, a, nbp, T_P));
  return unpack_host(h, lv, nb, a, Y, nbp);
}

int sw_apply_dirac(sw_engine* h, int hid, int level, int nb, const double* X, double* Y) {
  return simple_op(h, hid, level, nb, X, Y, 0);
}
int sw_restrict(sw_engine* h, int hid, int level, int nb, const double* X, double* Y) {
  return simple_op(h, hid, level, nb, X, Y, 1);
}
int sw_prolong(sw_engine* h, int hid, int level, int nb, const double* X, double* Y) {
  return simple_op(h, hid, level, nb, X, Y, 2);
}
int sw_coarsest(sw_engine* h, int hid, int nb, const double* X, double* Y) {
  return simple_op(h, hid, 0, nb, X, Y, 3);
}

int sw_vcycle(sw_engine* h, int hid, int level0, int nb, const double* B, double* X) {
  SWCHK(check_hier(h, hid, level0, true));
  if (nb <= 0 || !B || !X) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  const int nbp = pad64(nb);
  Level& lv = H.lv[level0];
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(pack_host(h, lv, nb, B, a, nbp));
  if (h->precond_f32 && f32_capable(H, level0)) SWCHK(vcycle_f32_boundary(h, H, level0, a, b, nbp));
  else SWCHK(vcycle(h, H, level0, a, b, nbp));
  return unpack_host(h, lv, nb, b, X, nbp);
}

// What sw_apply_op32 and sw_apply_op64 share: the argument checks, the operator behind a `which` code with the
// kernel category the cycles launch it under, and `info`.  f32: the complex64 entry point (its mirrors are made
// here; it has the lattice level's even-odd kernels and no lattice operator, the fp64 one the reverse).
struct OpSel {
  const EllOp* op = nullptr;
  int cat = T_MVM;
  bool inplace = false, square = false, smoother = false, transfer = false, up = false;
};
static int select_op(sw_engine* h, const char* fn, bool f32, int hid, int level, int which, int mode, int nb,
                     const double* X, const double* B, const double* Y, int flags, int32_t* info, OpSel* s) {
  SWCHK(check_hier(h, hid, level, true));
  const bool inplace = s->inplace = (flags & SW_OP32_INPLACE) != 0;
  const bool square = s->square = which == SW_OP32_A || (which >= SW_OP32_EO0 && which <= SW_OP32_EO0 + 4);
  const bool smoother = s->smoother = which == SW_OP32_EO_SMOOTH || which == SW_OP32_EO_SMOOTH_REDUCED;
  if (which < 0 || which > SW_OP32_EO_SMOOTH_REDUCED || nb <= 0 || !X || !Y || (flags & ~SW_OP32_INPLACE))
    return sw_fail(h, "%s: bad arguments", fn);
  if (!f32 && (which == SW_OP32_SCHUR || smoother))
    return sw_fail(h, "%s: operation %d (the lattice level's even-odd kernels) is not available here", fn, which);
  if (!(mode == 0 || (square && (mode == 1 || mode == 3))))
    return sw_fail(h, "%s: operation %d has no mode %d", fn, which, mode);
  if (inplace && !(square && mode == 1))
    return sw_fail(h, "%s: the in-place form is Y = X - op X (mode 1) of a square operator", fn);
  if (!B && ((mode != 0 && !inplace) || smoother)) return sw_fail(h, "%s: operation %d needs B", fn, which);
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  const int last = H.nlevels - 1;
  const bool transfer = s->transfer = which >= SW_OP32_R && which <= SW_OP32_RE;
  if (transfer && level >= last) return sw_fail(h, "no transfer at the coarsest level");
  if (which == SW_OP32_COARSEST && level != last)
    return sw_fail(h, "%s: the coarsest inverse acts on level %d", fn, last);
  Level& lv = H.lv[level];
  const bool on_stencil = which == SW_OP32_RE || which == SW_OP32_SCHUR || smoother;
  if (on_stencil && !(lv.stencil && lv.U1 && !lv.w_eo.empty()))
    return sw_fail(h, "level %d is not a lattice level with the even-odd smoother", level);
  const EllOp* op = nullptr;
  int cat = T_MVM;
  if (which == SW_OP32_A) op = &lv.A;
  if (which == SW_OP32_R) { op = &lv.R; cat = T_R; }
  if (which == SW_OP32_P || which == SW_OP32_P_EVEN) { op = &lv.P; cat = T_P; }
  if (which == SW_OP32_COARSEST) { op = &H.cinv; cat = T_COARSEST; }
  if (square && which != SW_OP32_A) {
    op = &lv.eo_op[which - SW_OP32_EO0];
    if (which == SW_OP32_EO0 + 4) cat = T_COARSEST;
  }
  if (which == SW_OP32_A && lv.stencil) {
    if (f32) return sw_fail(h, "level %d is the lattice level: no complex64 operator", level);
    if (!lv.U1) return sw_fail(h, "level %d: the lattice level has no gauge links", level);
    if (inplace) return sw_fail(h, "%s: the stencil reads its neighbours' rows: no in-place form", fn);
    op = nullptr;
  }
  if (op && !op->set) return sw_fail(h, "level %d: operation %d has no operator", level, which);
  if (f32) SWCHK(ensure_f32(h, H));
  if (which == SW_OP32_RE || which == SW_OP32_P_EVEN) {
    SWCHK(ensure_even_orders(h, H));
    if (which == SW_OP32_RE) {
      if (!lv.Re.set) return sw_fail(h, "level %d has no even-column restrictor", level);
      if (f32) SWCHK(mirror_op32(h, lv.Re));
      op = &lv.Re;
      cat = T_R;
    } else if (!(lv.P.order_even && h->p_even)) {
      return sw_fail(h, "level %d has no even-sites-only prolongation", level);
    }
  }
  if (info) {
    info[0] = op ? (op->bsr_RT > 0 ? op->bsr_RT : (op->bsr_KS > 0 ? op->nrows / 16 : 0)) : 0;
    info[1] = op ? op->bsr_KS : 0;
    info[2] = (op && op->cols) ? op->G : 0;
    info[3] = (op && op->cols) ? op->K : 0;
  }
  s->op = op;
  s->cat = cat;
  s->up = which == SW_OP32_P || which == SW_OP32_P_EVEN;
  return 0;
}

// One operation of the complex64 cycle alone on host vectors (the per-kernel parity tests): fp64 in, cast to
// complex64 (k_cast), ONE launch through the launcher vcycle32 / vcycle32_even use -- with the kernel category
// they pass, so the options pick the variant exactly as in the cycle --, cast back (exact), fp64 out.  Rows the
// operation does not write come back zero (in place: as they went in).
int sw_apply_op32(sw_engine* h, int hid, int level, int which, int mode, int nb, const double* X, const double* B,
                  double w_re, double w_im, int flags, double* Y, int32_t* info) {
  OpSel sel;
  SWCHK(select_op(h, "sw_apply_op32", true, hid, level, which, mode, nb, X, B, Y, flags, info, &sel));
  const bool inplace = sel.inplace, smoother = sel.smoother, up = sel.up;
  const EllOp* op = sel.op;
  const int cat = sel.cat;
  Hier& H = h->hier[hid];
  Level& lv = H.lv[level];
  Level& lc = H.lv[sel.transfer ? level + 1 : level];
  const int nbp = pad64(nb);
  // input on `lin`, output on `lout` (they differ for the transfers only)
  Level& lin = up ? lc : lv;
  Level& lout = up ? lv : lc;
  SWCHK(ensure_level_ws32(h, lin, nbp));
  SWCHK(ensure_level_ws32(h, lout, nbp));
  cplx *a, *b, *c, *d;
  SWCHK(io_vectors(h, lin, nbp, &a, &b));
  SWCHK(io_vectors(h, lout, nbp, &c, &d));
  (void)b;
  const size_t cin = (size_t)lin.n * nbp, cout = (size_t)lout.n * nbp;
  const cplxf w{(float)w_re, (float)w_im};
  cplxf* x32 = lin.x32;
  cplxf* y32 = inplace ? x32 : lout.t32;
  if (smoother) {
    // as vcycle32 / vcycle32_even: the iterate starts in the buffer from which the last step lands in Xout
    const bool odd_steps = (lv.w_eo.size() & 1) != 0;
    y32 = lv.x32;
    x32 = odd_steps ? lv.t32 : lv.x32;
  }
  SWCHK(pack_host(h, lin, nb, X, a, nbp));
  SWCHK(cast_vec(h, (const cplx*)a, x32, cin));
  const cplxf* b32 = inplace ? x32 : nullptr;
  if (B && !inplace && (mode != 0 || smoother)) {
    SWCHK(pack_host(h, lout, nb, B, c, nbp));
    SWCHK(cast_vec(h, (const cplx*)c, lout.b32, cout));
    b32 = lout.b32;
  }
  if (!inplace && !smoother) HIPCHK(hipMemsetAsync(y32, 0, cout * sizeof(cplxf), h->stream));
  if (which == SW_OP32_SCHUR) {
    SWCHK(schur_apply32(h, lv, x32, y32, nbp));
  } else if (smoother) {
    cplxf* other = (x32 == lv.x32) ? lv.t32 : lv.x32;
    SWCHK(eo_smooth32(h, lv, b32, x32, other, y32, nbp, which == SW_OP32_EO_SMOOTH_REDUCED));
  } else {
    SWCHK(launch_ell32(h, *op, mode, x32, b32, y32, nbp, cat, w, which == SW_OP32_P_EVEN));
  }
  SWCHK(cast_vec(h, (const cplxf*)y32, d, cout));
  if (which == SW_OP32_EO_SMOOTH_REDUCED)      // half vectors: the odd sites' rows were never the smoother's
    HIPCHK(hipMemsetAsync(d + cout / 2, 0, (cout / 2) * sizeof(cplx), h->stream));
  return unpack_host(h, lout, nb, d, Y, nbp);
}

// The fp64 twin: ONE launch through the launcher the fp64 cycle uses for the operation (launch_ell with the
// cycle's kernel category, launch_stencil on the lattice level), no casts, so use_mfma, mfma_ops, mfma_3m, the
// tile, stage, map and stencil options and the batch width pick the kernel variant exactly as in the cycle.  The
// coarsest inverse is the dense operator itself (H.cinv), not the even-odd direct path of apply_coarsest.
int sw_apply_op64(sw_engine* h, int hid, int level, int which, int mode, int nb, const double* X, const double* B,
                  double w_re, double w_im, int flags, double* Y, int32_t* info) {
  OpSel sel;
  SWCHK(select_op(h, "sw_apply_op64", false, hid, level, which, mode, nb, X, B, Y, flags, info, &sel));
  Hier& H = h->hier[hid];
  Level& lv = H.lv[level];
  Level& lc = H.lv[sel.transfer ? level + 1 : level];
  Level& lin = sel.up ? lc : lv;
  Level& lout = sel.up ? lv : lc;
  const int nbp = pad64(nb);
  SWCHK(ensure_level_ws(h, lin, nbp));
  SWCHK(ensure_level_ws(h, lout, nbp));
  // three distinct buffers also where input and output live on the same level
  cplx* x = lin.b;
  cplx* y = sel.inplace ? x : lout.x;
  const cplx* b = sel.inplace ? x : nullptr;
  SWCHK(pack_host(h, lin, nb, X, x, nbp));
  if (mode != 0 && !sel.inplace) {
    SWCHK(pack_host(h, lout, nb, B, lout.r, nbp));
    b = lout.r;
  }
  if (!sel.inplace) HIPCHK(hipMemsetAsync(y, 0, (size_t)lout.n * nbp * sizeof(cplx), h->stream));
  const cplx w{w_re, w_im};
  if (!sel.op) SWCHK(launch_stencil<cplx, cplx>(h, lv, mode == 3 ? 2 : mode, x, b, y, nbp, w));
  else SWCHK(launch_ell(h, *sel.op, mode, x, b, y, nbp, sel.cat, w, which == SW_OP32_P_EVEN));
  return unpack_host(h, lout, nb, y, Y, nbp);
}

// ---------------------------------------------------------------------------------------------
// One operation of the Krylov solver alone on host data (test-only, no hierarchy needed): each entry runs the
// production host helper -- multidot, multigram + multiaxpy as gram_cycle_update, multiaxpy, launch_tail,
// launch_fg_solve --, so row_blocking, fused_ok, red_args, the KT / NV instantiation and the options fused_reduce
// and dot_blocks choose the launch exactly as in a solve.  Vectors in the (nb, n) host layout, per-probe arrays
// [rows][nb]; on the device the pad columns up to nbp are zero.  Output buffers start as NaN patterns: an entry
// a kernel does not write shows.
// ---------------------------------------------------------------------------------------------
static_assert(SW_KRYLOV_BEGIN == SW_TAIL_BEGIN && SW_KRYLOV_HESS == SW_TAIL_HESS &&
                  SW_KRYLOV_VERIFY == SW_TAIL_VERIFY && SW_KRYLOV_SOLVE > SW_TAIL_GRAM,
              "the operation codes of sw_krylov_scalars are the tail kinds");
int sw_krylov_multidot(sw_engine* h, int n, int nb, int K, int storage, const double* V, const double* W,
                       const double* svec, double* out, double* coef, int32_t* info) {
  if (!h) return 1;
  if (K < 1 || K > SW_MAXK) return sw_fail(h, "sw_krylov_multidot: K=%d out of [1,%d]", K, SW_MAXK);
  if (n <= 0 || nb <= 0 || !V || !W || !out || (svec && !coef))
    return sw_fail(h, "sw_krylov_multidot: bad arguments");
  if (storage != SW_KRYLOV_C128 && storage != SW_KRYLOV_C64)
    return sw_fail(h, "sw_krylov_multidot: unsupported storage %d", storage);
  HIPCHK(hipSetDevice(h->device));
  const int nbp = pad64(nb);
  DevBuf<cplx> d(h);       // out [K][nbp], coef [K][nbp], svec [K][nbp]
  const size_t cnt = (size_t)K * nbp;
  SWCHK(dev_realloc(h, &d.p, 3 * cnt));
  HIPCHK(hipMemsetAsync(d.p, 0xFF, 2 * cnt * sizeof(cplx), h->stream));
  if (svec) SWCHK(put_cols(h, d.p + 2 * cnt, svec, K, nb, nbp, false));
  const cplx* sv = svec ? d.p + 2 * cnt : nullptr;
  cplx* cf = svec ? d.p + cnt : nullptr;
  blocking_info(h, n, nbp, true, info);
  if (storage == SW_KRYLOV_C64) SWCHK(krylov_multidot<cplxf>(h, n, nb, nbp, K, V, W, sv, d.p, cf));
  else SWCHK(krylov_multidot<cplx>(h, n, nb, nbp, K, V, W, sv, d.p, cf));
  // (out comes back at the padded width: its pad columns are part of what is checked)
  SWCHK(get_cols(h, d.p, out, K, nbp, nbp));
  if (svec) SWCHK(get_cols(h, d.p + cnt, coef, K, nb, nbp));
  return 0;
}

int sw_krylov_gram_cycle(sw_engine* h, int n, int nb, int NV, int flags, const double* U, const double* Z,
                         double* X, double* normb, int32_t* iters, double tol, double tol_stop, int iter_base,
                         double* gram, double* ys, double* relres, double* g, int32_t* notconv, int32_t* info) {
  if (!h) return 1;
  if (NV < 2 || NV > SW_GRAM_MAXL + 1)
    return sw_fail(h, "sw_krylov_gram_cycle: %d vectors out of [2,%d]", NV, SW_GRAM_MAXL + 1);
  const bool with_tail = !(flags & SW_KRYLOV_NOTAIL);
  if (n <= 0 || nb <= 0 || !U || !gram || (flags & ~(SW_KRYLOV_INIT | SW_KRYLOV_NOTAIL)) ||
      (with_tail && (!Z || !X || !normb || !iters || !ys || !relres || !g || !notconv)))
    return sw_fail(h, "sw_krylov_gram_cycle: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  const int nbp = pad64(nb), L = NV - 1, K = NV * (NV + 1) / 2;
  const size_t vec = (size_t)n * nbp;
  blocking_info(h, n, nbp, true, info);
  KrylovScope ks(h);
  KrylovWS& ws = ks.ws;
  SWCHK(ensure_krylov(h, ws, L, n, nbp, false));
  DevBuf<cplx> rx(h);      // r0, X
  SWCHK(dev_realloc(h, &rx.p, 2 * vec));
  cplx* r0 = rx.p;
  cplx* x = rx.p + vec;
  SWCHK(pack_vectors(h, n, nb, nbp, 1, U, r0));
  SWCHK(pack_vectors(h, n, nb, nbp, L, U + (size_t)nb * n * 2, ws.V));
  PtrList pu, pz;
  pu.p[0] = r0;
  for (int j = 0; j < L; ++j) {
    pu.p[j + 1] = ws.V + vec * j;
    pz.p[j] = ws.Z + vec * j;
  }
  HIPCHK(hipMemsetAsync(ws.gram, 0xFF, (size_t)K * nbp * sizeof(cplx), h->stream));
  if (!with_tail) {
    SWCHK(multigram(h, pu, NV, n, nbp, ws.gram, nullptr));
    return get_cols(h, ws.gram, gram, K, nb, nbp);
  }
  SWCHK(pack_vectors(h, n, nb, nbp, L, Z, ws.Z));
  SWCHK(pack_vectors(h, n, nb, nbp, 1, X, x));
  SWCHK(put_cols(h, ws.sc.normb, normb, 1, nb, nbp, false));
  SWCHK(put_ints(h, ws.sc.iters, iters, nb, nbp));
  HIPCHK(hipMemsetAsync(ws.sc.ys, 0xFF, (size_t)L * nbp * sizeof(cplx), h->stream));
  HIPCHK(hipMemsetAsync(ws.sc.relres, 0xFF, (size_t)nbp * sizeof(cplx), h->stream));
  HIPCHK(hipMemsetAsync(ws.sc.g, 0xFF, (size_t)nbp * sizeof(cplx), h->stream));
  SWCHK(reset_slots(h));
  swk::FgTail tg{};
  tg.tol = tol;
  tg.tol_stop = tol_stop;
  tg.iter_base = iter_base;
  tg.first_cycle = (flags & SW_KRYLOV_INIT) ? 1 : 0;
  SWCHK(take_slot(h, &tg.notconv));
  SWCHK(gram_cycle_update(h, pu, pz, L, n, nbp, x, ws, tg));
  int left = 0;
  SWCHK(read_slot(h, tg.notconv, &left));
  *notconv = left;
  SWCHK(get_cols(h, ws.gram, gram, K, nb, nbp));
  SWCHK(get_cols(h, ws.sc.ys, ys, L, nb, nbp));
  SWCHK(get_cols(h, ws.sc.relres, relres, 1, nb, nbp, false));
  SWCHK(get_cols(h, ws.sc.g, g, 1, nb, nbp, false));
  SWCHK(get_cols(h, ws.sc.normb, normb, 1, nb, nbp, false));
  SWCHK(get_ints(h, ws.sc.iters, iters, nb));
  return unpack_rows(h, n, nullptr, nb, x, X, nbp);
}

int sw_krylov_multiaxpy(sw_engine* h, int n, int nb, int K, int storage_v, int storage_w, int flags,
                        const double* V, const double* coef, double sign, double* W, double* nrm, double* W32,
                        int32_t* info) {
  if (!h) return 1;
  if (K < 1 || K > SW_MAXK) return sw_fail(h, "sw_krylov_multiaxpy: K=%d out of [1,%d]", K, SW_MAXK);
  const bool norm = (flags & SW_KRYLOV_NORM) != 0, w32 = (flags & SW_KRYLOV_W32) != 0;
  if (n <= 0 || nb <= 0 || !V || !coef || !W || (flags & ~(SW_KRYLOV_NORM | SW_KRYLOV_W32)) || (norm && !nrm) ||
      (w32 && !W32))
    return sw_fail(h, "sw_krylov_multiaxpy: bad arguments");
  // the storage pairs fgmres_loop instantiates: the fp64 basis and the iterate (V, W fp64), the complex64 basis
  // of f32_krylov (both complex64), complex64 directions into the fp64 iterate
  const bool v32 = storage_v == SW_KRYLOV_C64, wc32 = storage_w == SW_KRYLOV_C64;
  if ((storage_v != SW_KRYLOV_C128 && !v32) || (storage_w != SW_KRYLOV_C128 && !wc32) || (!v32 && wc32))
    return sw_fail(h, "sw_krylov_multiaxpy: unsupported storage pair V %d, W %d", storage_v, storage_w);
  if (w32 && wc32) return sw_fail(h, "sw_krylov_multiaxpy: the complex64 copy goes with an fp64 W");
  HIPCHK(hipSetDevice(h->device));
  const int nbp = pad64(nb);
  DevBuf<cplx> d(h);       // coef [K][nbp], nrm [nbp]
  const size_t cnt = (size_t)K * nbp;
  SWCHK(dev_realloc(h, &d.p, cnt + nbp));
  SWCHK(put_cols(h, d.p, coef, K, nb, nbp));
  HIPCHK(hipMemsetAsync(d.p + cnt, 0xFF, (size_t)nbp * sizeof(cplx), h->stream));
  cplx* nr = norm ? d.p + cnt : nullptr;
  blocking_info(h, n, nbp, norm, info);
  double* c32 = w32 ? W32 : nullptr;
  if (v32 && wc32) SWCHK(krylov_multiaxpy<cplxf, cplxf>(h, n, nb, nbp, K, V, d.p, sign, W, nr, c32));
  else if (v32) SWCHK(krylov_multiaxpy<cplxf, cplx>(h, n, nb, nbp, K, V, d.p, sign, W, nr, c32));
  else SWCHK(krylov_multiaxpy<cplx, cplx>(h, n, nb, nbp, K, V, d.p, sign, W, nr, c32));
  if (norm) SWCHK(get_cols(h, nr, nrm, 1, nb, nbp, false));
  return 0;
}

int sw_krylov_scalars(sw_engine* h, int m, int nb, int op, int j, int flag, double tol, double tol_stop,
                      int iter_base, const double* h1, const double* h2, const double* nrm, double* state,
                      int32_t* iters, int32_t* notconv) {
  if (!h) return 1;
  if (m < 1 || m > SW_MAXM) return sw_fail(h, "sw_krylov_scalars: restart %d out of [1,%d]", m, SW_MAXM);
  if (nb <= 0 || !state || !iters || !notconv) return sw_fail(h, "sw_krylov_scalars: bad arguments");
  const bool hess = op == SW_TAIL_HESS, solve = op == SW_KRYLOV_SOLVE;
  if (!(op == SW_TAIL_BEGIN || hess || op == SW_TAIL_VERIFY || solve))
    return sw_fail(h, "sw_krylov_scalars: unknown operation %d", op);
  if ((hess && (j < 0 || j >= m || !h1)) || (solve && (j < 0 || j > m)))
    return sw_fail(h, "sw_krylov_scalars: column %d out of range", j);
  if (!solve && !nrm && !(hess && flag)) return sw_fail(h, "sw_krylov_scalars: operation %d needs nrm", op);
  HIPCHK(hipSetDevice(h->device));
  const int nbp = pad64(nb);
  KrylovScope ks(h);
  KrylovWS& ws = ks.ws;
  SWCHK(ensure_krylov(h, ws, m, 0, nbp, false));
  // the packed state: H, cs, sn, g, y, normb, relres, svec, ys, each [rows][nb] complex
  struct Part { cplx* p; int rows; };
  const Part parts[] = {{ws.sc.H, (m + 1) * m}, {ws.sc.cs, m}, {ws.sc.sn, m}, {ws.sc.g, m + 1}, {ws.sc.y, m},
                        {ws.sc.normb, 1},       {ws.sc.relres, 1}, {ws.sc.svec, m + 1}, {ws.sc.ys, m}};
  size_t off = 0;
  for (const Part& q : parts) {
    SWCHK(put_cols(h, q.p, state + off, q.rows, nb, nbp));
    off += (size_t)q.rows * nb * 2;
  }
  SWCHK(put_ints(h, ws.sc.iters, iters, nb, nbp));
  if (h1) SWCHK(put_cols(h, ws.h1, h1, m + 2, nb, nbp));
  if (h2) SWCHK(put_cols(h, ws.h2, h2, m + 2, nb, nbp));
  if (nrm) SWCHK(put_cols(h, ws.nrm, nrm, 1, nb, nbp, false));
  SWCHK(reset_slots(h));
  int* slot = nullptr;
  SWCHK(take_slot(h, &slot));
  if (solve) SWCHK(launch_fg_solve(h, ws.sc, j));
  else if (op == SW_TAIL_BEGIN) SWCHK(launch_tail(h, tail_begin(ws, flag ? 1 : 0)));
  else if (hess) SWCHK(launch_tail(h, tail_hess(ws, j, h2 != nullptr, flag != 0, tol, tol_stop, iter_base, slot)));
  else SWCHK(launch_tail(h, tail_verify(ws, tol, tol_stop, slot)));
  int left = 0;
  SWCHK(read_slot(h, slot, &left));
  *notconv = left;
  off = 0;
  for (const Part& q : parts) {
    SWCHK(get_cols(h, q.p, state + off, q.rows, nb, nbp));
    off += (size_t)q.rows * nb * 2;
  }
  return get_ints(h, ws.sc.iters, iters, nb);
}

// ---------------------------------------------------------------------------------------------
// Outer solve of an even-odd smoothed stencil level on the EVEN-ODD REDUCED system.
//   A x = b  <=>  S x_e = b'_e,  b'_e = b_e - A_eo A_oo^-1 b_o,  x_o = A_oo^-1 (b_o - A_oe x_e),
//   S = A_ee - A_eo A_oo^-1 A_oe  (here A_oo = D, the Schur complement k_schur_step applies).
// The cycle's even-odd smoother leaves the odd residual exactly zero, so in the full-system FGMRES the
// odd halves of all Krylov vectors carry no information; here they do not exist: every vector of the
// Krylov solver (basis, directions, iterate, residual) is a HALF vector -- the first n / 2 rows of
// the parity-sorted level --, the operator is one k_schur_step<0> (two half passes instead of the
// stencil's four), and the preconditioner is the even block of the same multigrid cycle,
// M_S r_e = [M (r_e; 0)]_e ~ (A^-1)_ee = S^-1: restriction from the even columns only (Level::Re), no
// hop before the Schur steps (b_o = 0 makes b' = r_e) and none after them (the odd half is not
// needed).  The residual of the reduced system IS the residual of the full one (its odd half vanishes
// identically once x_o is set from x_e), and it is measured against ||b|| of the full system, so the
// stopping criterion is the reference's (multigrid.py:347-366).  Per iteration on the lattice level:
// about 47 half-vector passes instead of 64.
// ---------------------------------------------------------------------------------------------

// Y_e = S X_e (mode 0) or Bp_e - S X_e (mode 1); all three are half vectors
static int schur_apply(sw_engine* h, Level& lv, int mode, const cplx* X, const cplx* Bp, cplx* Y, int nbp) {
  swk::StencilArgs a = stencil_args<cplx>(h, lv, nbp, true);
  if (mode == 0) return launch_schur_step<0>(h, T_SCHUR_OP, a, X, Bp, Y, nbp);
  return launch_schur_step<1>(h, T_SCHUR_OP, a, X, Bp, Y, nbp);
}

static bool eo_solve_eligible(sw_engine* h, Hier& H, int level) {
  if (!h->eo_solve || level != 0 || H.nlevels < 2) return false;
  Level& lv = H.lv[0];
  if (!(lv.stencil && lv.rich && lv.gm_m == 0 && !lv.w_eo.empty() && lv.w_pre.empty() && lv.P.set &&
        lv.R.set && !h->cgs2 && h->p_even && (lv.n % 2 == 0)))
    return false;
  // single-precision preconditioner: only its default form (complex64 cycle AND complex64 Krylov basis)
  if (h->precond_f32 && !(h->f32_krylov && f32_capable(H, 0))) return false;
  if (ensure_even_orders(h, H) != 0) return false;
  return lv.Re.set && lv.P.order_even != nullptr;
}

// Xout_e = [M (Bin_e; 0)]_e : the even block of the level-0 cycle (see above); half vectors in and out
static int vcycle_even(sw_engine* h, Hier& H, const cplx* Bin, cplx* Xout, int nbp) {
  Level& lv = H.lv[0];
  Level& lc = H.lv[1];
  SWCHK(ensure_level_ws(h, lv, nbp));
  SWCHK(ensure_level_ws(h, lc, nbp));
  SWCHK(ensure_even_orders(h, H));
  if (!lv.Re.set) return sw_fail(h, "internal: even-column restrictor missing");
  SWCHK(launch_ell(h, lv.Re, 0, Bin, nullptr, lc.b, nbp, T_R));
  SWCHK(coarse_correction(h, H, 0, nbp));
  // (Xout is a HALF-length array: the prolongation must write the even sites only)
  if (!(lv.P.order_even && h->p_even))
    return sw_fail(h, "internal: even-odd reduced solve needs the even-sites-only prolongation (p_even)");
  if (h->eo_product && !lv.q_w.empty() && lv.q_w.size() + 1 == lv.w_eo.size()) {
    // product form: the coarse correction lands in Xout and is smoothed there; the two halves of lv.t are scratch
    SWCHK(launch_ell(h, lv.P, 0, lc.x, nullptr, Xout, nbp, T_P, cplx{0.0, 0.0}, true));
    return schur_product_steps(h, lv, Xout, lv.t, lv.t + (size_t)(lv.n / 2) * nbp, Bin, nbp);
  }
  // ping-pong between lv.t and Xout (only their even halves are touched) so that the last step lands in Xout
  const bool odd_steps = (lv.w_eo.size() & 1) != 0;
  cplx* cur = odd_steps ? lv.t : Xout;
  cplx* nxt = odd_steps ? Xout : lv.t;
  SWCHK(launch_ell(h, lv.P, 0, lc.x, nullptr, cur, nbp, T_P, cplx{0.0, 0.0}, true));
  cplx* res = nullptr;
  SWCHK(schur_steps(h, lv, cur, nxt, Bin, nbp, &res));
  if (res != Xout) return sw_fail(h, "internal: even-odd smoother ended in the wrong buffer");
  return 0;
}

// the same in complex64 (option precond_f32): half vectors of complex64 in and out
static int vcycle32_even(sw_engine* h, Hier& H, const cplxf* Bin, cplxf* Xout, int nbp) {
  Level& lv = H.lv[0];
  Level& lc = H.lv[1];
  const int last = H.nlevels - 1;
  SWCHK(ensure_level_ws32(h, lv, nbp));
  SWCHK(ensure_level_ws32(h, lc, nbp));
  SWCHK(ensure_even_orders(h, H));
  if (!lv.Re.set) return sw_fail(h, "internal: even-column restrictor missing");
  SWCHK(mirror_op32(h, lv.Re));
  SWCHK(launch_ell32(h, lv.Re, 0, Bin, nullptr, lc.b32, nbp, T_R));
  if (lv.kcycle > 0 && 1 < last) {
    // (as vcycle32: the few-step inner FGMRES of a K-cycle stays fp64, preconditioned in complex64)
    const size_t cc = (size_t)lc.n * nbp;
    SWCHK(ensure_level_ws(h, lc, nbp));
    SWCHK(cast_vec(h, (const cplxf*)lc.b32, lc.b, cc, T_AXPY));
    SWCHK(ensure_krylov(h, lc.kws, lv.kcycle, lc.n, nbp, false));
    SWCHK(fgmres(h, H, 1, lc.b, lc.x, 0.0, lv.kcycle, lv.kcycle, false, lc.kws, nbp, nullptr, true));
    SWCHK(cast_vec(h, (const cplx*)lc.x, lc.x32, cc, T_AXPY));
  } else {
    SWCHK(vcycle32(h, H, 1, lc.b32, lc.x32, nbp));
  }
  if (!(lv.P.order_even && h->p_even))
    return sw_fail(h, "internal: even-odd reduced solve needs the even-sites-only prolongation (p_even)");
  const bool odd_steps = (lv.w_eo.size() & 1) != 0;
  cplxf* start = odd_steps ? lv.t32 : Xout;
  cplxf* other = odd_steps ? Xout : lv.t32;
  SWCHK(launch_ell32(h, lv.P, 0, lc.x32, nullptr, start, nbp, T_P, cplxf{0.f, 0.f}, true));
  return eo_smooth32(h, lv, Bin, start, other, Xout, nbp, true);
}

// The even-odd reduced system S x_e = b'_e of the stencil level (half vectors), preconditioned by the even
// block of the level-0 cycle.  With the single-precision preconditioner (precond_f32 + f32_krylov) the
// restart cycle is complex64 as in the full system: basis, directions and w = S z in complex64 (S applied in
// single precision), inner products accumulated in fp64; residual b' - S x, iterate and convergence check
// fp64, once per restart.  ||b|| of the FULL system fixes normb (reduced_rhs).
static KrylovSys reduced_system(sw_engine* h, Hier& H, int nbp) {
  Level& lv = H.lv[0];
  KrylovSys s;
  s.n = lv.n / 2;
  s.normb_set = true;
  s.apply = [h, &lv, nbp](int mode, const cplx* x, const cplx* b, cplx* y) {
    return schur_apply(h, lv, mode, x, b, y, nbp);
  };
  s.precond = [h, &H, nbp](const cplx* v, cplx* z) { return vcycle_even(h, H, v, z, nbp); };
  if (h->precond_f32 && h->f32_krylov && f32_capable(H, 0)) {
    s.precond32 = [h, &H, nbp](const cplxf* v, cplxf* z) { return vcycle32_even(h, H, v, z, nbp); };
    s.op32 = [h, &lv, nbp](const cplxf* z, cplxf* w) { return schur_apply32(h, lv, z, w, nbp); };
  }
  return s;
}

// ||b|| of the FULL system fixes normb (the reference's stopping criterion); b'_e = b_e + H_eo b_o / D
// into ws.xacc
static int reduced_rhs(sw_engine* h, Level& lv, const cplx* B, KrylovWS& ws, int nbp) {
  PtrList pl;
  pl.p[0] = B;
  const swk::FgTail tbeg = tail_begin(ws, 1);
  SWCHK(multidot(h, pl, 1, B, lv.n, nbp, ws.nrm, nullptr, nullptr, &tbeg));
  return eo_hop<0>(h, lv, B, B, ws.xacc, nbp);
}

// batched flexible GMRES(m) on the even-odd reduced system: the full system's restart loop on S, then
// x_o = (b_o + H_oe x_e) / D
static int fgmres_eo(sw_engine* h, Hier& H, const cplx* B, cplx* X, double tol, int maxiter, int m,
                     KrylovWS& ws, int nbp, int* iters_total) {
  Level& lv = H.lv[0];
  SWCHK(ensure_level_ws(h, lv, nbp));
  SWCHK(reduced_rhs(h, lv, B, ws, nbp));
  // the iterate lives in the even half of X
  SWCHK(fgmres_loop(h, H, 0, reduced_system(h, H, nbp), ws.xacc, X, tol, maxiter, m, true, ws, nbp,
                    iters_total));
  return eo_hop<1>(h, lv, B, X, X, nbp);
}

// The same solve with restart cycles in GRAM-MATRIX form (option gram_cycle, default).  A cycle of L <= m
// steps builds z_0 = M r, w_0 = S z_0, z_1 = M w_0, w_1 = S z_1, ... with NO inner products or
// orthogonalisation in between -- the same Krylov space FGMRES(m) spans --, then one pass over [r, w_0 ..
// w_{L-1}] yields all their inner products and the minimal-residual combination follows per probe from a
// Cholesky-factorised L x L system (fg_gram_col, which also gives the residual norm of every nested
// sub-cycle: per-probe iteration counts as before).  Per cycle of three: 12 half-vector passes of BLAS-1 and
// residual instead of 29, 4 launches instead of 9.  Every cycle ends with the TRUE residual b' - S x, so the
// convergence test always sees true residuals; the read-backs are per cycle, not per iteration: cycles run
// unobserved until the previous batch's iteration count is within one cycle, then the residuals of all
// probes come back (a few KB) and the last cycle is cut to the length they call for.
static int fgmres_eo_gram(sw_engine* h, Hier& H, const cplx* B, cplx* X, double tol, int maxiter, int m,
                          KrylovWS& ws, int nbp, int* iters_total) {
  Level& lv = H.lv[0];
  const int hid_idx = (int)(&H - &h->hier[0]);
  const int hint = h->lazy_sync ? h->sync_hint[hid_idx][0] : 0;
  const KrylovSys sys = reduced_system(h, H, nbp);
  const double tol_stop = tol * h->stop_factor;
  SWCHK(ensure_level_ws(h, lv, nbp));
  SWCHK(reset_slots(h));
  SWCHK(reduced_rhs(h, lv, B, ws, nbp));
  const cplx* bp = ws.xacc;
  SWCHK(zero_vec(h, X, sys.n, nbp));
  std::vector<std::complex<double>> hrr(nbp), hrr0(nbp);
  int done = 0;
  bool converged = false;
  const cplx* Rcur = bp;
  int L = std::min(m, maxiter);
  while (done < maxiter && !converged) {
    L = std::max(1, std::min(L, std::min(m, maxiter - done)));
    int* slot = nullptr;
    SWCHK(take_slot(h, &slot));
    swk::FgTail tg{};
    tg.tol = tol;
    tg.tol_stop = tol_stop;
    tg.iter_base = done;
    tg.notconv = slot;
    SWCHK(gram_cycle(h, sys, Rcur, X, L, ws, nbp, tg));
    done += L;
    // the true residual: input of the next cycle and of the final check
    SWCHK(sys.apply(1, X, bp, ws.rres));
    Rcur = ws.rres;
    // Observe?  Not while the previous batch's count says more than one further cycle is due.
    const bool observe = tol_stop > 0.0 && (hint <= 0 || done + m >= hint || done >= maxiter);
    int Lnext = m;
    if (observe) {
      int left = 0;
      SWCHK(read_slot(h, slot, &left));
      if (left == 0) {
        converged = true;
      } else {
        // how many more steps do the slowest probes need at the rate this cycle achieved?
        HIPCHK(hipMemcpy(hrr.data(), ws.sc.relres, sizeof(cplx) * nbp, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hrr0.data(), ws.sc.g, sizeof(cplx) * nbp, hipMemcpyDeviceToHost));
        double need = 1.0;
        for (int c = 0; c < nbp; ++c) {
          const double r1 = hrr[c].real(), r0 = hrr0[c].real();
          if (!(r1 >= tol_stop) || !(r0 > 0.0)) continue;
          const double rate = std::pow(std::min(0.9, std::max(1e-6, r1 / r0)), 1.0 / L);   // per step
          need = std::max(need, std::ceil(std::log(0.9 * tol_stop / r1) / std::log(rate)));
        }
        Lnext = (int)std::min<double>(m, need);
      }
    }
    if (converged && h->verify) {
      // (the decision above used the cycle's own estimate of |r_L|; the residual just formed is the true one)
      PtrList pr;
      pr.p[0] = ws.rres;
      int* vslot = nullptr;
      SWCHK(take_slot(h, &vslot));
      const swk::FgTail tv = tail_verify(ws, tol, tol_stop, vslot);
      SWCHK(multidot(h, pr, 1, ws.rres, sys.n, nbp, ws.nrm, nullptr, nullptr, &tv));
      int left = 0;
      SWCHK(read_slot(h, vslot, &left));
      if (left != 0) {
        converged = false;
        Lnext = 1;
      }
    }
    L = Lnext;
  }
  SWCHK(eo_hop<1>(h, lv, B, X, X, nbp));
  if (iters_total) *iters_total = done;
  h->sync_hint[hid_idx][0] = converged ? done : 0;
  return 0;
}

static bool level_is_direct(sw_engine* h, Hier& H, int level) {
  return h->direct_small && level < H.nlevels - 1 && !H.lv[level].stencil && H.lv[level].dinv.set &&
         h->use_mfma;
}

// device-resident solve used by sw_solve and the probe drivers
static int solve_dev(sw_engine* h, int hid, int level0, const cplx* B, cplx* X, double tol,
                     int maxiter, int nbp, int* total) {
  Hier& H = h->hier[hid];
  Level& lv = H.lv[level0];
  if (level0 == H.nlevels - 1 && H.nlevels > 1) {
    // coarsest level: the dense inverse is the solve (multigrid.py:413-416)
    SWCHK(apply_coarsest(h, H, B, X, nbp));
    if (total) *total = 1;
    return 0;
  }
  if (level_is_direct(h, H, level0)) {
    // x = A^-1 b ; x += A^-1 (b - A x): dense inverse on the matrix cores, one refinement step
    SWCHK(ensure_level_ws(h, lv, nbp));
    SWCHK(launch_bsr(h, lv.dinv, 0, B, nullptr, X, nbp, T_COARSEST, cplx{0.0, 0.0}));
    SWCHK(apply_op(h, lv, 1, X, B, lv.r, nbp));
    SWCHK(launch_bsr(h, lv.dinv, 0, lv.r, nullptr, lv.t, nbp, T_COARSEST, cplx{0.0, 0.0}));
    SWCHK(vec_add(h, X, lv.t, X, lv.n, nbp));
    if (total) *total = 1;
    // The refinement step takes the inverse's own residual (eps * cond) below the solver tolerance on the
    // operators this was built for; that is MEASURED here, not assumed: ||b - A x|| / ||b|| per right-hand
    // side, further refinement steps while any of them is above stop_factor * tol, and the multigrid-
    // preconditioned FGMRES of the general path if three more steps do not get there.
    SWCHK(ensure_small(h, nbp));
    h->direct_relres.assign(nbp, 0.0);
    for (int pass = 0;; ++pass) {
      SWCHK(apply_op(h, lv, 1, X, B, lv.r, nbp));
      SWCHK(dot_into(h, lv.r, lv.r, lv.n, nbp, h->small));
      SWCHK(dot_into(h, B, B, lv.n, nbp, h->small + nbp));
      SWCHK(stream_sync(h));
      std::vector<std::complex<double>> nn(2 * (size_t)nbp);
      HIPCHK(hipMemcpy(nn.data(), h->small, sizeof(cplx) * 2 * nbp, hipMemcpyDeviceToHost));
      double worst = 0.0;
      for (int j = 0; j < nbp; ++j) {
        const double b2 = nn[nbp + j].real(), r2 = nn[j].real();
        const double rr = b2 > 0.0 ? std::sqrt(r2 / b2) : 0.0;
        h->direct_relres[j] = rr;
        worst = std::max(worst, rr);
      }
      if (!(worst > tol * h->stop_factor)) return 0;
      if (pass == 3) break;
      SWCHK(launch_bsr(h, lv.dinv, 0, lv.r, nullptr, lv.t, nbp, T_COARSEST, cplx{0.0, 0.0}));
      SWCHK(vec_add(h, X, lv.t, X, lv.n, nbp));
    }
    h->direct_relres.clear();      // the iterative path reports its own residuals
    h->direct_fallbacks++;
    const int mfb = std::min(h->restart, std::max(1, maxiter));
    SWCHK(ensure_krylov(h, lv.sws, mfb, lv.n, nbp, true));
    return fgmres(h, H, level0, B, X, tol, maxiter, mfb, true, lv.sws, nbp, total);
  }
  const int m = std::min(h->restart, std::max(1, maxiter));
  SWCHK(ensure_krylov(h, lv.sws, m, lv.n, nbp, true));
  if (eo_solve_eligible(h, H, level0)) {
    const bool k32 = h->precond_f32 && h->f32_krylov && f32_capable(H, 0);
    int P = 0, rpb = 0;
    row_blocking(lv.n / 2, nbp, true, &P, &rpb);
    if (h->gram_cycle && !k32 && m <= SW_GRAM_MAXL && fused_ok(h, P, nbp))
      return fgmres_eo_gram(h, H, B, X, tol, maxiter, m, lv.sws, nbp, total);
    return fgmres_eo(h, H, B, X, tol, maxiter, m, lv.sws, nbp, total);
  }
  return fgmres(h, H, level0, B, X, tol, maxiter, m, true, lv.sws, nbp, total);
}

static int fetch_iters(sw_engine* h, KrylovWS& ws, int nb, int32_t* iters, double* relres,
                       int fallback_iters) {
  std::vector<int> it(ws.nbp);
  std::vector<std::complex<double>> rr(ws.nbp);
  HIPCHK(hipMemcpy(it.data(), ws.sc.iters, sizeof(int) * ws.nbp, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rr.data(), ws.sc.relres, sizeof(cplx) * ws.nbp, hipMemcpyDeviceToHost));
  for (int j = 0; j < nb; ++j) {
    if (iters) iters[j] = it[j] >= 0 ? it[j] : fallback_iters;
    if (relres) relres[j] = rr[j].real();
  }
  return 0;
}

int sw_solve(sw_engine* h, int hid, int level0, int nb, const double* B, double* X, double tol,
             int maxiter, int32_t* iters, double* relres) {
  SWCHK(check_hier(h, hid, level0, true));
  if (nb <= 0 || !B || !X || maxiter < 1) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Hier& H = h->hier[hid];
  const int nbp = pad64(nb);
  Level& lv = H.lv[level0];
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(pack_host(h, lv, nb, B, a, nbp));
  int total = 0;
  SWCHK(solve_dev(h, hid, level0, a, b, tol, maxiter, nbp, &total));
  SWCHK(unpack_host(h, lv, nb, b, X, nbp));
  if (level0 == H.nlevels - 1 && H.nlevels > 1) {
    for (int j = 0; j < nb; ++j) {
      if (iters) iters[j] = 1;
      if (relres) relres[j] = 0.0;
    }
    return 0;
  }
  if (level_is_direct(h, H, level0) && (int)h->direct_relres.size() >= nb) {
    // directly solved level: iteration count 1 as for the coarsest level, the MEASURED residual
    for (int j = 0; j < nb; ++j) {
      if (iters) iters[j] = 1;
      if (relres) relres[j] = h->direct_relres[j];
    }
    return 0;
  }
  return fetch_iters(h, lv.sws, nb, iters, relres, total);
}

// ---- probe batches ---------------------------------------------------------------------
static int ensure_probe_ws(sw_engine* h, int nbp) {
  if (h->pb_ws_nbp == nbp && h->pb_x0) return 0;
  Hier& H0 = h->hier[0];
  int nmax = 0;
  for (int l = 0; l < H0.nlevels; ++l) nmax = std::max(nmax, H0.lv[l].n);
  const size_t cnt = (size_t)nmax * nbp;
  SWCHK(dev_realloc(h, &h->pb_x0, cnt));
  SWCHK(dev_realloc(h, &h->pb_rhs, cnt));
  SWCHK(dev_realloc(h, &h->pb_z, cnt));
  SWCHK(dev_realloc(h, &h->pb_xc, cnt));
  SWCHK(dev_realloc(h, &h->pb_xc2, cnt));
  SWCHK(dev_realloc(h, &h->pb_y, cnt));
  SWCHK(dev_realloc(h, &h->pb_w, cnt));
  SWCHK(dev_realloc(h, &h->pb_w2, cnt));
  SWCHK(dev_realloc(h, &h->pb_xd, cnt));
  SWCHK(dev_realloc(h, &h->pb_est, (size_t)4 * nbp));
  SWCHK(dev_realloc(h, &h->pb_iters, (size_t)2 * nbp));
  // the probes' int8 codes of the shifted dots and the slice reductions; a new batch width drops the shifted result
  SWCHK(dev_realloc(h, &h->pb_codes, cnt));
  h->r_shifts.drop();
  h->pb_ws_nbp = nbp;
  return 0;
}

// sw_hutch_fetch_*: the result `r` of the last completed batch of its mode, out[rows][nb]; `none` = the mode's
// message when there is none
static int fetch_result(sw_engine* h, ResultBuf sw_engine::* r, const char* none, double* out) {
  if (!h) return 1;
  if (!out) return sw_fail(h, "null output");
  const ResultBuf& res = h->*r;
  if (res.nb <= 0 || !res.p) return sw_fail(h, "%s", none);
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  return result_fetch(h, res, res.nb, out);
}

int sw_probes_upload_slot(sw_engine* h, int slot, int level, int nb, const int8_t* probes) {
  SWCHK(check_hier(h, 0, level, true));
  if (nb <= 0 || !probes) return sw_fail(h, "bad arguments");
  if (slot < 0 || slot >= 4096) return sw_fail(h, "probe slot %d out of range", slot);
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[level];
  const size_t bytes = (size_t)nb * lv.n;
  if ((int)h->slots.size() <= slot) h->slots.resize(slot + 1);
  sw_engine::ProbeSlot& sl = h->slots[slot];
  if (sl.pending) {
    HIPCHK(hipStreamSynchronize(h->gen_stream));
    sl.pending = false;
  }
  if (sl.bytes < bytes) {
    SWCHK(dev_free(h, sl.p));
    sl.p = nullptr;
    void* q;
    SWCHK(dev_alloc(h, &q, bytes));
    sl.p = (int8_t*)q;
    sl.bytes = bytes;
  }
  HIPCHK(hipMemcpyAsync(sl.p, probes, bytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  sl.level = level;
  sl.nb = nb;
  return 0;
}

int sw_probes_select(sw_engine* h, int slot) {
  if (!h) return 1;
  if (slot < 0 || slot >= (int)h->slots.size() || !h->slots[slot].p)
    return sw_fail(h, "probe slot %d is empty", slot);
  h->pb_slot = slot;
  h->pb_probes = h->slots[slot].p;
  h->pb_level = h->slots[slot].level;
  h->pb_nb = h->slots[slot].nb;
  h->pb_nbp = pad64(h->pb_nb);
  return 0;
}

int sw_probes_upload(sw_engine* h, int level, int nb, const int8_t* probes) {
  SWCHK(sw_probes_upload_slot(h, 0, level, nb, probes));
  return sw_probes_select(h, 0);
}

// ---- device-side probe generation --------------------------------------------------------
int sw_probes_stream_set(sw_engine* h, const uint32_t* window) {
  if (!h) return 1;
  if (!window) return sw_fail(h, "null MT19937 window");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->gen_stream));      // a queued generation may still read the old window
  if (!h->mt_win0) SWCHK(dev_realloc(h, &h->mt_win0, (size_t)SW_MT_N));
  if (!h->mt_win) SWCHK(dev_realloc(h, &h->mt_win, (size_t)2 * SW_MT_N));
  if (!h->mt_poly) SWCHK(dev_realloc(h, &h->mt_poly, (size_t)SW_MT_N));
  HIPCHK(hipMemcpyAsync(h->mt_win0, window, SW_MT_N * sizeof(uint32_t), hipMemcpyHostToDevice,
                        h->stream));
  HIPCHK(hipMemcpyAsync(h->mt_win, window, SW_MT_N * sizeof(uint32_t), hipMemcpyHostToDevice,
                        h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->mt_cur = 0;
  h->mt_pos = 0;
  h->mt_dist = 0;
  h->mt_set = true;
  return 0;
}

// probes per generator segment: segments of ~64K draws (105 state blocks), whole probes
static inline int mt_probes_per_segment(int n) { return std::max(1, 65536 / n); }

int sw_probes_generate(sw_engine* h, int slot, int level, int nb, int kind, uint64_t pos) {
  SWCHK(check_hier(h, 0, level, true));
  if (!h->mt_set) return sw_fail(h, "no probe stream set (sw_probes_stream_set)");
  if (nb <= 0) return sw_fail(h, "bad arguments");
  if (kind != SW_PROBES_Z2 && kind != SW_PROBES_Z4) return sw_fail(h, "unknown probe kind %d", kind);
  if (slot < 0 || slot >= 4096) return sw_fail(h, "probe slot %d out of range", slot);
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[level];
  const int n = lv.n;
  if (n % 4) return sw_fail(h, "device probe generation needs n %% 4 == 0 (n = %d)", n);
  const uint64_t total = (uint64_t)nb * (uint64_t)n;
  // Asynchronous, on the generation stream: the call returns once the work is queued, the slot's `ready`
  // event orders it ahead of the sw_hutch_run that consumes the slot.  (While profiling, generation
  // stays on the solve stream so that the per-launch event pairs bracket it.)
  // (SW_SINGLE_STREAM=1 keeps it on the solve stream as well: for tools that want one queue per process)
  static const bool single_stream = [] {
    const char* e = getenv("SW_SINGLE_STREAM");
    return e && e[0] == '1';
  }();
  hipStream_t gs = (h->profiling || single_stream) ? h->stream : h->gen_stream;
  // 1. move the resident window to `pos`
  if (pos < h->mt_pos) {
    HIPCHK(hipMemcpyAsync(h->mt_win + (size_t)SW_MT_N * h->mt_cur, h->mt_win0,
                          SW_MT_N * sizeof(uint32_t), hipMemcpyDeviceToDevice, gs));
    h->mt_pos = 0;
  }
  if (pos > h->mt_pos) {
    const uint64_t dist = pos - h->mt_pos;
    if (dist != h->mt_dist) {
      uint32_t poly[SW_MT_N];
      if (sw_mt_jump_poly(dist, poly) != 0) return sw_fail(h, "jump polynomial construction failed");
      // the previous polynomial may still be in use by a queued k_mt_jump: stream order protects it
      HIPCHK(hipMemcpyAsync(h->mt_poly, poly, sizeof poly, hipMemcpyHostToDevice, gs));
      HIPCHK(hipStreamSynchronize(gs));   // `poly` is a stack buffer
      h->mt_dist = dist;
    }
    LaunchScope ls(h, T_OTHER);
    hipLaunchKernelGGL(swk::k_mt_jump, dim3(1), dim3(SW_MT_BLOCK), 0, gs,
                       (const uint32_t*)(h->mt_win + (size_t)SW_MT_N * h->mt_cur),
                       (const uint32_t*)h->mt_poly, h->mt_win + (size_t)SW_MT_N * (1 - h->mt_cur));
    KLAUNCH_CHECK();
    h->mt_cur = 1 - h->mt_cur;
    h->mt_pos = pos;
  }
  // 2. the polynomial family of the segment starts
  const int pps = mt_probes_per_segment(n);
  const uint64_t segdraws = (uint64_t)pps * (uint64_t)n;
  const int S = (nb + pps - 1) / pps;
  if (S > 1 && (h->mt_fam_seg != segdraws || h->mt_fam_count < S - 1)) {
    std::vector<uint32_t> fam((size_t)(S - 1) * SW_MT_N);
    for (int s = 1; s < S; ++s)
      if (sw_mt_jump_poly((uint64_t)s * segdraws, &fam[(size_t)(s - 1) * SW_MT_N]) != 0)
        return sw_fail(h, "jump polynomial construction failed");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->gen_stream));
    SWCHK(upload(h, &h->mt_family, fam.data(), fam.size()));
    h->mt_fam_seg = segdraws;
    h->mt_fam_count = S - 1;
  }
  // 3. generate into the slot
  if ((int)h->slots.size() <= slot) h->slots.resize(slot + 1);
  sw_engine::ProbeSlot& sl = h->slots[slot];
  if (sl.bytes < total) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->gen_stream));
    SWCHK(dev_free(h, sl.p));
    sl.p = nullptr;
    void* q;
    SWCHK(dev_alloc(h, &q, total));
    sl.p = (int8_t*)q;
    sl.bytes = total;
  }
  {
    LaunchScope ls(h, T_OTHER);
    hipLaunchKernelGGL(swk::k_mt_generate, dim3(S), dim3(SW_MT_BLOCK), 0, gs,
                       (const uint32_t*)(h->mt_win + (size_t)SW_MT_N * h->mt_cur),
                       (const uint32_t*)h->mt_family, (unsigned long long)segdraws,
                       (unsigned long long)total, kind, sl.p);
    KLAUNCH_CHECK();
  }
  sl.level = level;
  sl.nb = nb;
  if (!sl.ready) HIPCHK(hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming));
  HIPCHK(hipEventRecord(sl.ready, gs));
  sl.pending = true;
  return 0;
}

int sw_probes_fetch(sw_engine* h, int slot, int8_t* out) {
  if (!h) return 1;
  if (!out) return sw_fail(h, "null output");
  if (slot < 0 || slot >= (int)h->slots.size() || !h->slots[slot].p)
    return sw_fail(h, "probe slot %d is empty", slot);
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  HIPCHK(hipStreamSynchronize(h->gen_stream));
  const sw_engine::ProbeSlot& sl = h->slots[slot];
  const size_t bytes = (size_t)sl.nb * h->hier[0].lv[sl.level].n;
  HIPCHK(hipMemcpy(out, sl.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}

static int dot_into(sw_engine* h, const cplx* A, const cplx* Bv, int n, int nbp, cplx* out) {
  PtrList pl;
  pl.p[0] = A;
  return multidot(h, pl, 1, Bv, n, nbp, out);
}

static int record_iters(sw_engine* h, KrylovWS* ws, int total_or_const, std::vector<int32_t>& dst,
                        int nb) {
  dst.assign(nb, total_or_const);
  if (ws) {
    std::vector<int> it(ws->nbp);
    HIPCHK(hipMemcpy(it.data(), ws->sc.iters, sizeof(int) * ws->nbp, hipMemcpyDeviceToHost));
    for (int j = 0; j < nb; ++j) dst[j] = it[j] >= 0 ? it[j] : total_or_const;
  }
  return 0;
}

// The first half of deflate(), cbuf[ld][nbp] = U^H X (the scalar kernels write the rows below kd only): returns in *gemm which
// kernel pair the rank and the option select.
static int defl_coeffs(sw_engine* h, const cplx* U, int kd, const cplx* X, int n, int nbp, cplx* cbuf, bool* gemm) {
  const int ld = defl_ld(kd);
  *gemm = h->defl_gemm || kd > 64;
  if (*gemm) {
    // ~2048 workgroups of 16 probes, at least 64 rows per slice
    const int nchunks = nbp / 16;
    const int pmax = std::max(1, (n + 63) / 64);
    int P = std::max(1, std::min(pmax, 2048 / nchunks));
    const int rpb = (n + P - 1) / P;
    P = (n + rpb - 1) / rpb;
    SWCHK(ensure_partial(h, (size_t)P * ld * nbp * sizeof(cplx)));
    // 64-column groups of U per workgroup: 1, 2 or 4
    SWCHK(pick_ge<64, 128, 256>(ld, [&](auto LD) {
      return launch(h, T_DEFL, swk::k_defl_gemm_dots<LD / 64>, dim3(P, nchunks), dim3(SW_BLOCK), U, ld, X, n, nbp,
                    rpb, h->partial);
    }));
    return launch(h, T_DEFL, swk::k_reduce_partials, dim3(ld, nbp / 64), dim3(SW_BLOCK), h->partial, P, ld, nbp,
                  cbuf, (const cplx*)nullptr, (cplx*)nullptr);
  }
  int P, rpb;
  row_blocking(n, nbp, true, &P, &rpb);
  for (int k0 = 0; k0 < kd; k0 += 32) {
    const int kc = std::min(32, kd - k0);
    SWCHK(ensure_partial(h, (size_t)P * kc * nbp * sizeof(cplx)));
    SWCHK(pick_ge<8, 16, 32>(kc, [&](auto KC) {
      return launch(h, T_DEFL, swk::k_defl_dots<KC>, dim3(P, nbp / 64), dim3(SW_BLOCK), (const cplx*)(U + k0), ld,
                    kc, X, n, nbp, rpb, h->partial);
    }));
    SWCHK(launch(h, T_DEFL, swk::k_reduce_partials, dim3(kc, nbp / 64), dim3(SW_BLOCK), h->partial, P, kc, nbp,
                 cbuf + (size_t)k0 * nbp, (const cplx*)nullptr, (cplx*)nullptr));
  }
  return 0;
}

// out[r] = X[s] - sum_k U[s][k] (U^H X)[k],  s = srcrow[r] (NULL: identity)   (utils.py:221-225)
// U is [n][defl_ld(kd)].  Up to kd = 64 (and defl_gemm = 0): k_defl_dots in chunks of 32 vectors, then
// k_defl_apply; above, or with defl_gemm = 1: the matrix-core pair k_defl_gemm_dots / k_defl_gemm_apply,
// which read the probe block once for all kd vectors.
static int deflate(sw_engine* h, const cplx* U, int kd, const int* srcrow, const cplx* X, cplx* out,
                   int n, int nbp) {
  const int ld = defl_ld(kd);
  cplx* cbuf = h->small + 8 * nbp;  // [ld][nbp], ld <= SW_MAX_DEFL
  bool gemm;
  SWCHK(defl_coeffs(h, U, kd, X, n, nbp, cbuf, &gemm));
  if (gemm)
    return launch(h, T_DEFL, swk::k_defl_gemm_apply<true>, dim3((n + 63) / 64, nbp / 64), dim3(SW_BLOCK), U, ld,
                  (const cplx*)cbuf, srcrow, X, out, n, nbp);
  dim3 grid((n + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK, nbp / 64);
  return launch(h, T_DEFL, swk::k_defl_apply, grid, dim3(SW_BLOCK), U, ld, kd, cbuf, srcrow, X, out, n, nbp);
}

// out = U G' U^H X on ncols columns (a multiple of 64) with the registered vectors U and low-mode inverse G:
// c = U^H X by deflate()'s first half, c' = s G c (k_low_mode_coef; nq > 0: s = +1 / -1 on the column groups of
// nq columns of even / odd index, the g_a of a two-point source; nq = 0: s = 1), out = U c' by the apply kernel
// without its subtraction.  X is not read after the first half, so out may be X itself.
static int low_mode_apply(sw_engine* h, const cplx* X, int n, int ncols, int nq, cplx* out) {
  const int kd = h->kd, ld = defl_ld(kd);
  const size_t per = (size_t)ld * ncols;
  if (h->lm_coef_cap < 2 * per) {
    SWCHK(dev_realloc(h, &h->lm_coef, 2 * per));
    h->lm_coef_cap = 2 * per;
  }
  cplx *c = h->lm_coef, *c2 = h->lm_coef + per;
  bool gemm;
  SWCHK(defl_coeffs(h, h->U, kd, X, n, ncols, c, &gemm));
  SWCHK(launch(h, T_DEFL, swk::k_low_mode_coef, dim3((ld + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK, ncols / 64),
               dim3(SW_BLOCK), (const cplx*)h->lm_G, kd, ld, (const cplx*)c, ncols, nq, c2));
  return launch(h, T_DEFL, swk::k_defl_gemm_apply<false>, dim3((n + 63) / 64, ncols / 64), dim3(SW_BLOCK),
                (const cplx*)h->U, ld, (const cplx*)c2, (const int*)nullptr, (const cplx*)nullptr, out, n, ncols);
}

static int low_mode_ready(sw_engine* h) {
  if (h->kd <= 0 || !h->U) return sw_fail(h, "no deflation vectors registered (sw_set_deflation)");
  if (h->lm_k != h->kd || !h->lm_G)
    return sw_fail(h, "no low-mode inverse registered for the %d deflation vectors (sw_set_low_mode_inverse)", h->kd);
  return 0;
}

int sw_set_low_mode_inverse(sw_engine* h, int k, const double* G) {
  SWCHK(check_hier(h, 0, 0, false));
  h->lm_k = 0;
  if (k == 0) return 0;
  if (h->kd <= 0) return sw_fail(h, "no deflation vectors registered (sw_set_deflation)");
  if (k != h->kd) return sw_fail(h, "low-mode inverse of rank %d, %d deflation vectors are registered", k, h->kd);
  if (!G) return sw_fail(h, "null low-mode inverse");
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  SWCHK(upload(h, &h->lm_G, (const cplx*)G, (size_t)k * k));
  h->lm_k = k;
  return 0;
}

// Y = U G U^H X on host vectors (reference order): the low-mode chain of SW_MODE_TWO_POINT_LMA without the sign.
int sw_apply_low_mode(sw_engine* h, int nb, const double* X, double* Y) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nb <= 0 || !X || !Y) return sw_fail(h, "bad arguments");
  SWCHK(low_mode_ready(h));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int nbp = pad64(nb);
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(pack_host(h, lv, nb, X, a, nbp));
  SWCHK(low_mode_apply(h, a, lv.n, nbp, 0, b));
  return unpack_host(h, lv, nb, b, Y, nbp);
}

// Y = the registered deflation projection of the host vectors X (reference order, nb contiguous vectors):
// which = 0: Pperm^T (I - U U^H) X at level 0 (Hutchinson, sw_set_deflation / sw_set_perm), which = 1:
// (I - V_l V_l^H) X at `level` (sw_set_level_deflation).  The kernels and the launch sequence of
// sw_hutch_run's deflation step.
int sw_apply_deflation(sw_engine* h, int which, int level, int nb, const double* X, double* Y) {
  SWCHK(check_hier(h, 0, level, false));
  if (which != 0 && which != 1) return sw_fail(h, "which must be 0 (Hutchinson) or 1 (MLMC level)");
  if (which == 0 && level != 0) return sw_fail(h, "the Hutchinson deflation acts at level 0");
  if (nb <= 0 || !X || !Y) return sw_fail(h, "bad arguments");
  const int kd = which == 0 ? h->kd : h->lkd[level];
  const cplx* U = which == 0 ? h->U : h->lV[level];
  if (kd <= 0 || !U) return sw_fail(h, "no deflation vectors registered at level %d", level);
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[level];
  const int nbp = pad64(nb);
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(ensure_small(h, nbp));
  SWCHK(pack_host(h, lv, nb, X, a, nbp));
  SWCHK(deflate(h, U, kd, which == 0 ? (const int*)h->perm_src[0] : nullptr, a, b, lv.n, nbp));
  return unpack_host(h, lv, nb, b, Y, nbp);
}

// ---- shifted probe dots: Tr(A^-1 D_s) at many flat shifts s = 2 L d from one solve per probe ----------
int sw_set_shifts(sw_engine* h, int nshifts, const int64_t* shifts) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nshifts < 0 || nshifts > SW_MAX_SHIFTS)
    return sw_fail(h, "%d shifts: at most %d per registration", nshifts, SW_MAX_SHIFTS);
  h->r_shifts.drop();
  if (nshifts == 0) {
    h->shifts.clear();
    return 0;
  }
  if (!shifts) return sw_fail(h, "null shift list");
  Level& lv = h->hier[0].lv[0];
  if (!lv.stencil || lv.h_rowmap.empty())
    return sw_fail(h, "shifted traces need a lattice level 0 (sw_set_lattice)");
  const int L = lv.L, n = lv.n;
  if (L > SW_SHIFT_MAX_L) return sw_fail(h, "shifted traces: L=%d above %d", L, SW_SHIFT_MAX_L);
  std::vector<int> disp;
  for (int j = 0; j < nshifts; ++j) {
    const int64_t sft = shifts[j];
    if (sft < 0 || sft >= n) return sw_fail(h, "shift %lld outside [0,%d)", (long long)sft, n);
    if (sft % (2 * L)) return sw_fail(h, "shift %lld is not a multiple of 2L = %d", (long long)sft, 2 * L);
    for (int i = 0; i < j; ++i)
      if (shifts[i] == sft) return sw_fail(h, "shift %lld listed twice", (long long)sft);
    disp.push_back((int)(sft / (2 * L)));
  }
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  disp.resize((size_t)((nshifts + 15) / 16) * 16, disp[0]);
  SWCHK(upload(h, &h->shift_disp, disp.data(), disp.size()));
  // reference index i = q * 2L + r: ring r in [0, 2L), position q in [0, L)
  std::vector<int> rr((size_t)n);
  for (int r = 0; r < 2 * L; ++r)
    for (int q = 0; q < L; ++q) rr[(size_t)r * L + q] = lv.h_rowmap[(size_t)q * 2 * L + r];
  SWCHK(upload(h, &h->ringrow, rr.data(), rr.size()));
  h->shifts.assign(shifts, shifts + nshifts);
  return 0;
}

// r_shifts[j][col] = sum_i conj(x_col[(i + s_j) mod n]) z_col[i] for the registered shifts: the probes' codes
// from their int8 form (reference order), then k_shift_dots over the rings and the sum over its ring blocks
static int shift_dots(sw_engine* h, Level& lv, const int8_t* probes, int nb, const cplx* Z, int nbp) {
  const int S = (int)h->shifts.size();
  const int L = lv.L, n = lv.n, nrings = 2 * L;
  SWCHK(ensure_probe_ws(h, nbp));
  SWCHK(result_begin(h, h->r_shifts, S, nbp));
  SWCHK(launch(h, T_OTHER, swk::k_probe_codes, dim3((n + 63) / 64, nbp / 64), dim3(SW_BLOCK), probes, nb, n,
               (const int*)lv.rowmap, h->pb_codes, nbp));
  // shifts per pass over z: the smallest group that holds them all, 16 beyond that (S = 5..8 would otherwise
  // pay for 16 accumulators, most of them on padded copies of the first shift)
  return pick_ge<1, 4, 8, 16>(S, [&](auto SGc) {
    constexpr int SG = decltype(SGc)::value;
    const int Sp = (S + SG - 1) / SG * SG;           // <= the padded length of shift_disp
    const int other = (nbp / 64) * (Sp / SG);
    // ~2048 workgroups
    int rpb = std::max(1, std::min(nrings, (nrings * other + 2047) / 2048));
    const int P = (nrings + rpb - 1) / rpb;
    SWCHK(ensure_partial(h, (size_t)P * Sp * nbp * sizeof(cplx)));
    const dim3 grid(P, nbp / 64, Sp / SG);
    SWCHK(pick_ge<SW_SHIFT_SMALL_L, SW_SHIFT_MID_L, SW_SHIFT_MAX_L>(L, [&](auto LC) {
      return launch(h, T_DOTS, swk::k_shift_dots<SG, decltype(LC)::value>, grid, dim3(SW_BLOCK),
                    (const int8_t*)h->pb_codes, Z, (const int*)h->ringrow, (const int*)h->shift_disp, L, nrings,
                    rpb, nbp, Sp, h->partial);
    }));
    // the first S of the Sp sums
    return launch(h, T_DOTS, swk::k_reduce_partials, dim3(S, nbp / 64), dim3(SW_BLOCK), h->partial, P, Sp, nbp,
                  h->r_shifts.p, (const cplx*)nullptr, (cplx*)nullptr);
  });
}

// The kernel alone on host inputs (reference ordering): out[j][k] = vdot(roll(x_k, -s_j), Z_k).
int sw_apply_shift_dots(sw_engine* h, int nb, const int8_t* probes, const double* Z, double* out) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nb <= 0 || !probes || !Z || !out) return sw_fail(h, "bad arguments");
  if (h->shifts.empty()) return sw_fail(h, "no shifts registered (sw_set_shifts)");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int nbp = pad64(nb);
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(pack_host(h, lv, nb, Z, a, nbp));
  DevBuf<int8_t> pr(h);
  SWCHK(upload(h, &pr.p, probes, (size_t)nb * lv.n));
  SWCHK(shift_dots(h, lv, pr, nb, a, nbp));
  SWCHK(stream_sync(h));
  return result_fetch(h, h->r_shifts, nb, out);
}

int sw_hutch_fetch_shifts(sw_engine* h, double* ests) {
  return fetch_result(h, &sw_engine::r_shifts, "no shifted batch to fetch", ests);
}

// ---- timeslice loops: spin- and momentum-resolved traces per timeslice from one solve per probe --------
// The checks and device tables of a momentum registration (`what` names the mode in the messages): every p in
// [0, L), no duplicates, at most SW_MAX_MOMENTA; mom = the momenta padded to SW_MAX_MOMENTA with the first,
// phase = omega^j = e^{-2 pi i j / L}, j in [0, L), slicerow = the (timeslice, x, spin) -> internal row table.
static int check_momenta(sw_engine* h, const char* what, int nmom, const int32_t* p) {
  if (!p) return sw_fail(h, "null momentum list");
  Level& lv = h->hier[0].lv[0];
  if (!lv.stencil || lv.h_rowmap.empty())
    return sw_fail(h, "%s need a lattice level 0 (sw_set_lattice)", what);
  const int L = lv.L;
  if (L > SW_SHIFT_MAX_L) return sw_fail(h, "%s: L=%d above %d", what, L, SW_SHIFT_MAX_L);
  for (int j = 0; j < nmom; ++j) {
    if (p[j] < 0 || p[j] >= L) return sw_fail(h, "momentum %d outside [0,%d)", (int)p[j], L);
    for (int i = 0; i < j; ++i)
      if (p[i] == p[j]) return sw_fail(h, "momentum %d listed twice", (int)p[j]);
  }
  return 0;
}
static int upload_slicerow(sw_engine* h, int** d_slicerow);
static int upload_slice_tables(sw_engine* h, int nmom, const int32_t* p, int** d_mom, cplx** d_phase,
                               int** d_slicerow) {
  const int L = h->hier[0].lv[0].L;
  std::vector<int> mom(p, p + nmom);
  mom.resize(SW_MAX_MOMENTA, mom[0]);
  SWCHK(upload(h, d_mom, mom.data(), mom.size()));
  std::vector<cplx> ph((size_t)L);
  for (int j = 0; j < L; ++j) {
    // exact at the multiples of a quarter turn, so p = 0 and the real/imaginary axes carry no rounding
    const int q = (4 * j) / L;
    if ((4 * j) % L == 0) {
      ph[j] = cplx{q == 0 ? 1.0 : q == 2 ? -1.0 : 0.0, q == 1 ? -1.0 : q == 3 ? 1.0 : 0.0};
    } else {
      const double a = -2.0 * M_PI * (double)j / (double)L;
      ph[j] = cplx{std::cos(a), std::sin(a)};
    }
  }
  SWCHK(upload(h, d_phase, ph.data(), ph.size()));
  return upload_slicerow(h, d_slicerow);
}
static int upload_slicerow(sw_engine* h, int** d_slicerow) {
  Level& lv = h->hier[0].lv[0];
  const int L = lv.L, n = lv.n;
  // reference index idx(a,x,t) = a L^2 + t L + x
  std::vector<int> sr((size_t)n);
  for (int t = 0; t < L; ++t)
    for (int x = 0; x < L; ++x)
      for (int a = 0; a < 2; ++a)
        sr[((size_t)t * L + x) * 2 + a] = lv.h_rowmap[(size_t)a * L * L + (size_t)t * L + x];
  return upload(h, d_slicerow, sr.data(), sr.size());
}

int sw_set_loop_momenta(sw_engine* h, int nmom, const int32_t* p) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nmom < 0 || nmom > SW_MAX_MOMENTA)
    return sw_fail(h, "%d momenta: at most %d per registration", nmom, SW_MAX_MOMENTA);
  for (ResultBuf* r : {&h->r_loops, &h->r_mloops, &h->r_links}) r->drop();
  if (nmom == 0) {
    h->momenta.clear();
    return 0;
  }
  SWCHK(check_momenta(h, "timeslice loops", nmom, p));
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  SWCHK(upload_slice_tables(h, nmom, p, &h->loop_mom, &h->loop_phase, &h->slicerow));
  h->momenta.assign(p, p + nmom);
  return 0;
}

// Meson fields of the registered deflation vectors for the momentum p into a device buffer of the caller's scope:
// phi[c][d][t][m][m'], [2][2][L][kd][kd], k_meson_field on the engine's U; tables of its own (no momentum registration
// is touched).  The caller has checked the vectors and p.
static int meson_fields_dev(sw_engine* h, int p, DevBuf<cplx>& phi) {
  const int32_t p32 = p;
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  SWCHK(upload_slice_tables(h, 1, &p32, &h->lm_mom, &h->lm_phase, &h->lm_slicerow));
  Level& lv = h->hier[0].lv[0];
  const int L = lv.L, kd = h->kd, ld = defl_ld(kd);
  SWCHK(dev_realloc(h, &phi.p, (size_t)4 * L * kd * kd));
  if (h->profiling) h->twork[T_MESON_FIELD] += 32.0 * (double)L * (double)L * (double)ld * (double)ld;
  const dim3 grid(L, 4, (ld / 16 + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK);
  if (p == 0)
    return launch(h, T_MESON_FIELD, swk::k_meson_field<false>, grid, dim3(SW_BLOCK), (const cplx*)h->U, ld, kd,
                  (const int*)h->lm_slicerow, (const cplx*)h->lm_phase, p, L, phi.p);
  return launch(h, T_MESON_FIELD, swk::k_meson_field<true>, grid, dim3(SW_BLOCK), (const cplx*)h->U, ld, kd,
                (const int*)h->lm_slicerow, (const cplx*)h->lm_phase, p, L, phi.p);
}

// out[c][d][t][m][m'], complex128 [2][2][L][kd][kd]: the meson fields of meson_fields_dev on the host.
int sw_meson_fields(sw_engine* h, int p, double* out) {
  SWCHK(check_hier(h, 0, 0, false));
  if (!out) return sw_fail(h, "null output");
  if (h->kd <= 0 || !h->U) return sw_fail(h, "no deflation vectors registered (sw_set_deflation)");
  const int32_t p32 = p;
  SWCHK(check_momenta(h, "meson fields", 1, &p32));
  DevBuf<cplx> phi(h);
  SWCHK(meson_fields_dev(h, p, phi));
  SWCHK(stream_sync(h));
  const size_t cnt = (size_t)4 * h->hier[0].lv[0].L * h->kd * h->kd;
  HIPCHK(hipMemcpy(out, phi.p, cnt * sizeof(cplx), hipMemcpyDeviceToHost));
  return 0;
}

// One launch of an instantiation of k_cgemm_nt: nz batches (kchunk = 0) or K splits of kchunk elements.
typedef void (*cgemm_nt_kernel)(const cplx*, int, size_t, const cplx*, int, size_t, cplx*, int, size_t, int, int, int,
                                int);
static int cgemm_nt(sw_engine* h, cgemm_nt_kernel kern, const cplx* A, int lda, size_t sA, const cplx* B, int ldb, size_t sB, cplx* C,
                    int ldc, size_t sC, int M, int N, int K, int nz, int kchunk) {
  return launch(h, T_LM_CONTRACT, kern, dim3((N + 63) / 64, (M + 63) / 64, nz),
                dim3(SW_BLOCK), A, lda, sA, B, ldb, sB, C, ldc, sC, M, N, K, kchunk);
}

// The low-mode two-point functions of the momentum p for every source timeslice, contracted on the device:
// out[a][b][c][d][t][t0] = g_a g_b sum_{m,m'} Phi[c][d][t][m][m'] conj(Psi[a][b][t0][m][m']), Psi = G Phi G^H, complex128
// [2][2][2][2][L][L].  Phi by meson_fields_dev; W^T[s] = conj(G) Phi[s]^T and Psi[s] = G (W^T[s])^T as two products
// batched over the 4 L slices s; the (4 L x kd^2)(kd^2 x 4 L) contraction with split K into partial sums, added in a
// fixed order by k_lm_two_point_reduce.  The number of splits follows from L and kd alone: about 1024 workgroups, at
// most 64 splits, whole steps of 16 per split.  All buffers live for this call only.
int sw_low_mode_two_point(sw_engine* h, int p, double* out) {
  SWCHK(check_hier(h, 0, 0, false));
  if (!out) return sw_fail(h, "null output");
  SWCHK(low_mode_ready(h));
  const int32_t p32 = p;
  SWCHK(check_momenta(h, "low-mode two-point functions", 1, &p32));
  DevBuf<cplx> phi(h), wt(h), psi(h), part(h), res(h);
  SWCHK(meson_fields_dev(h, p, phi));
  const int L = h->hier[0].lv[0].L, kd = h->kd, ld = defl_ld(kd), R = 4 * L, K = kd * kd;
  const size_t per = (size_t)kd * kd, total = (size_t)R * R;
  const int tiles = ((R + 63) / 64) * ((R + 63) / 64), steps = (K + 15) / 16;
  const int want = std::min(steps, std::min(64, std::max(1, 1024 / tiles)));
  const int kchunk = 16 * ((steps + want - 1) / want), nsplit = (K + kchunk - 1) / kchunk;
  SWCHK(dev_realloc(h, &wt.p, R * per));
  SWCHK(dev_realloc(h, &psi.p, R * per));
  SWCHK(dev_realloc(h, &part.p, nsplit * total));
  SWCHK(dev_realloc(h, &res.p, total));
  if (h->profiling)
    h->twork[T_LM_CONTRACT] += 8.0 * (2.0 * R * (double)ld * ld * ld + (double)R * R * (double)kd * kd);
  const cplx* G = h->lm_G;
  SWCHK(cgemm_nt(h, swk::k_cgemm_nt<true, false>, G, kd, 0, phi.p, kd, per, wt.p, kd, per, kd, kd, kd, R, 0));
  SWCHK(cgemm_nt(h, swk::k_cgemm_nt<false, false>, G, kd, 0, wt.p, kd, per, psi.p, kd, per, kd, kd, kd, R, 0));
  SWCHK(cgemm_nt(h, swk::k_cgemm_nt<false, true>, phi.p, K, 0, psi.p, K, 0, part.p, R, total, R, R, K, nsplit, kchunk));
  SWCHK(launch(h, T_LM_CONTRACT, swk::k_lm_two_point_reduce, dim3((unsigned)((total + SW_BLOCK - 1) / SW_BLOCK)),
               dim3(SW_BLOCK), (const cplx*)part.p, nsplit, L, res.p));
  SWCHK(stream_sync(h));
  HIPCHK(hipMemcpy(out, res.p, total * sizeof(cplx), hipMemcpyDeviceToHost));
  return 0;
}

// rows of the loop buffers [p][a][b][t]
static size_t loop_rows(sw_engine* h) { return h->momenta.size() * 4 * (size_t)h->hier[0].lv[0].L; }

// res[p][a][b][t][col] = sum_x e^{-2 pi i p x / L} conj(x_col[idx(a,x,t)]) z_col[idx(b,x,t)] for the registered
// momenta, res = mode 5's loops or the MLMC level loops: the probes' codes from their int8 form (reference order),
// then k_slice_dots, one workgroup per (timeslice, 64 probes); total (optional) = the scalar total of the first
// momentum's block per probe
static int slice_dots(sw_engine* h, Level& lv, const int8_t* probes, int nb, const cplx* Z, int nbp,
                      cplx* total, ResultBuf& res) {
  const int M = (int)h->momenta.size();
  const int L = lv.L, n = lv.n;
  SWCHK(ensure_probe_ws(h, nbp));
  SWCHK(result_begin(h, res, loop_rows(h), nbp));
  cplx* out = res.p;
  SWCHK(launch(h, T_OTHER, swk::k_probe_codes, dim3((n + 63) / 64, nbp / 64), dim3(SW_BLOCK), probes, nb, n,
               (const int*)lv.rowmap, h->pb_codes, nbp));
  SWCHK(pick_momenta(h, [&](auto NP, auto PH) {
    return launch(h, T_DOTS, swk::k_slice_dots<decltype(NP)::value, decltype(PH)::value>, dim3(L, nbp / 64),
                  dim3(SW_BLOCK), (const int8_t*)h->pb_codes, Z, (const int*)h->slicerow, (const cplx*)h->loop_phase,
                  (const int*)h->loop_mom, L, nbp, M, out);
  }));
  if (!total) return 0;
  return launch(h, T_DOTS, swk::k_slice_total, dim3(nbp / 64), dim3(SW_BLOCK), (const cplx*)out, L, nbp, total);
}

// out[p][a][b][t][col] = sum_x e^{-2 pi i p x / L} conj(U_col[idx(a,x,t)]) V_col[idx(b,x,t)] for the registered
// momenta, U and V two blocks [n_0][nbp] of the lattice level (k_slice_cdots: same grid, same choice of momenta
// per pass as slice_dots)
static int slice_cdots_into(sw_engine* h, Level& lv0, const cplx* U, const cplx* V, int nbp, cplx* out) {
  const int M = (int)h->momenta.size(), L = lv0.L;
  return pick_momenta(h, [&](auto NP, auto PH) {
    return launch(h, T_SLICE_CDOTS, swk::k_slice_cdots<decltype(NP)::value, decltype(PH)::value>, dim3(L, nbp / 64),
                  dim3(SW_BLOCK), U, V, (const int*)h->slicerow, (const cplx*)h->loop_phase, (const int*)h->loop_mom, L,
                  nbp, M, out);
  });
}

// the same into the MLMC loop buffer; total (optional) = the scalar total of the first momentum's block
static int slice_cdots(sw_engine* h, Level& lv0, const cplx* U, const cplx* V, int nbp, cplx* total) {
  SWCHK(result_begin(h, h->r_mloops, loop_rows(h), nbp));
  cplx* out = h->r_mloops.p;
  SWCHK(slice_cdots_into(h, lv0, U, V, nbp, out));
  if (!total) return 0;
  return launch(h, T_DOTS, swk::k_slice_total, dim3(nbp / 64), dim3(SW_BLOCK), (const cplx*)out, lv0.L, nbp, total);
}

// The kernel alone on host inputs (reference ordering): out[p][a][b][t][k] as above with z_k = Z_k.
int sw_apply_slice_dots(sw_engine* h, int nb, const int8_t* probes, const double* Z, double* out) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nb <= 0 || !probes || !Z || !out) return sw_fail(h, "bad arguments");
  if (h->momenta.empty()) return sw_fail(h, "no momenta registered (sw_set_loop_momenta)");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int nbp = pad64(nb);
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(pack_host(h, lv, nb, Z, a, nbp));
  DevBuf<int8_t> pr(h);
  SWCHK(upload(h, &pr.p, probes, (size_t)nb * lv.n));
  SWCHK(slice_dots(h, lv, pr, nb, a, nbp, nullptr, h->r_loops));
  SWCHK(stream_sync(h));
  return result_fetch(h, h->r_loops, nb, out);
}

// k_slice_cdots alone on host inputs (reference ordering): out[p][a][b][t][k] with the complex left operand U_k.
int sw_apply_slice_cdots(sw_engine* h, int nb, const double* U, const double* V, double* out) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nb <= 0 || !U || !V || !out) return sw_fail(h, "bad arguments");
  if (h->momenta.empty()) return sw_fail(h, "no momenta registered (sw_set_loop_momenta)");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int nbp = pad64(nb);
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(pack_host(h, lv, nb, U, a, nbp));
  SWCHK(pack_host(h, lv, nb, V, b, nbp));
  SWCHK(slice_cdots(h, lv, a, b, nbp, nullptr));
  SWCHK(stream_sync(h));
  return result_fetch(h, h->r_mloops, nb, out);
}

int sw_hutch_fetch_loops(sw_engine* h, double* out) {
  return fetch_result(h, &sw_engine::r_loops, "no loop batch to fetch", out);
}

int sw_hutch_fetch_mlmc_loops(sw_engine* h, double* out) {
  return fetch_result(h, &sw_engine::r_mloops, "no MLMC loop batch to fetch", out);
}

// ---- point-split link loops: a probe entry at n paired with the solution at n +- mu through the link --------
// what SW_MODE_HUTCHINSON_LINK_LOOPS and sw_apply_slice_link_dots need beyond a momentum registration: links
static int link_loops_ready(sw_engine* h) {
  if (h->momenta.empty()) return sw_fail(h, "no momenta registered (sw_set_loop_momenta)");
  Level& lv = h->hier[0].lv[0];
  if (!lv.stencil || !lv.U1 || !lv.U2) return sw_fail(h, "link loops need a lattice level 0 with links (sw_set_lattice)");
  return 0;
}

// link[d][p][a][b][t][col], d = (F_x, B_x, F_t, B_t), for the registered momenta from the codes k_probe_codes left
// in pb_codes (slice_dots of the same probes ran before, or probes != NULL: written here) and Z [n_0][nbp]:
// k_slice_link_dots, one workgroup per (timeslice, 64 probes, branch), the momenta per pass chosen as slice_dots
// does.  The buffer is the mode's own; only a completed batch marks it fetchable.
static int slice_link_dots(sw_engine* h, Level& lv, const int8_t* probes, int nb, const cplx* Z, int nbp) {
  const int M = (int)h->momenta.size();
  const int L = lv.L, n = lv.n;
  SWCHK(ensure_probe_ws(h, nbp));
  SWCHK(result_begin(h, h->r_links, 4 * loop_rows(h), nbp));
  if (probes)
    SWCHK(launch(h, T_OTHER, swk::k_probe_codes, dim3((n + 63) / 64, nbp / 64), dim3(SW_BLOCK), probes, nb, n,
                 (const int*)lv.rowmap, h->pb_codes, nbp));
  return pick_momenta(h, [&](auto NP, auto PH) {
    return launch(h, T_LINK_DOTS, swk::k_slice_link_dots<decltype(NP)::value, decltype(PH)::value>,
                  dim3(L, nbp / 64, 4), dim3(SW_BLOCK), (const int8_t*)h->pb_codes, Z, (const int*)h->slicerow,
                  (const cplx*)h->loop_phase, (const int*)h->loop_mom, (const cplx*)lv.U1, (const cplx*)lv.U2, L, nbp,
                  M, 0, h->r_links.p);
  });
}

// The kernel alone on host inputs (reference ordering): out[d][p][a][b][t][k] with z_k = Z_k.
int sw_apply_slice_link_dots(sw_engine* h, int nb, const int8_t* probes, const double* Z, double* out) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nb <= 0 || !probes || !Z || !out) return sw_fail(h, "bad arguments");
  SWCHK(link_loops_ready(h));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int nbp = pad64(nb);
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(pack_host(h, lv, nb, Z, a, nbp));
  DevBuf<int8_t> pr(h);
  SWCHK(upload(h, &pr.p, probes, (size_t)nb * lv.n));
  SWCHK(slice_link_dots(h, lv, pr, nb, a, nbp));
  SWCHK(stream_sync(h));
  return result_fetch(h, h->r_links, nb, out);
}

int sw_hutch_fetch_link_loops(sw_engine* h, double* out) {
  return fetch_result(h, &sw_engine::r_links, "no link-loop batch to fetch", out);
}

// X (level `level` of hierarchy 0, [n_level][nbp]) prolonged to the lattice level through P_{level-1} ... P_0,
// alternating between the scratch blocks s0 and s1 (each [n_0][nbp] at least); *res = where the result is
// (X itself at level 0)
static int prolong_to_lattice(sw_engine* h, int level, const cplx* X, cplx* s0, cplx* s1, int nbp, const cplx** res) {
  Hier& H0 = h->hier[0];
  const cplx* cur = X;
  for (int l = level - 1; l >= 0; --l) {
    cplx* dst = cur == s0 ? s1 : s0;
    SWCHK(launch_ell(h, H0.lv[l].P, 0, cur, nullptr, dst, nbp, T_P));
    cur = dst;
  }
  *res = cur;
  return 0;
}

// Iteration counts of an outer solve on (H, level) for the first nb columns, once the stream has drained: 1 on the
// coarsest and on a directly solved level, the solver's own counts elsewhere
static int record_level_iters(sw_engine* h, Hier& H, int level, int total, std::vector<int32_t>& dst, int nb) {
  SWCHK(stream_sync(h));
  if ((level == H.nlevels - 1 && H.nlevels > 1) || level_is_direct(h, H, level)) {
    dst.assign(nb, 1);
    return 0;
  }
  return record_iters(h, &H.lv[level].sws, total, dst, nb);
}

// The hierarchy that solves level `level` of hierarchy 0: the solver hierarchy at level 0 when it is ready, else
// hierarchy 0 itself
static int solve_hier(sw_engine* h, int level, int* hid) {
  *hid = (level == 0 && h->hier[h->solver_hid].ready) ? h->solver_hid : 0;
  if (*hid != 0 && h->hier[*hid].lv[0].n != h->hier[0].lv[level].n)
    return sw_fail(h, "solver hierarchy level-0 size mismatch");
  return 0;
}

// The two solves of the MLMC difference operator d = A_l^-1 x - P A_c^-1 R x of level `level` of hierarchy 0 (skip:
// A_0^-1 x - P_0 P_1 A_2^-1 R_1 R_0 x; utils.py:288-341): the fine one on the solver hierarchy at level 0 when it is
// ready, the coarse one on hierarchy 0 at lcoarse = level + 1 (skip: + 2).  Refused before anything is allocated or
// launched; every user of the operator goes through this pair of functions.
static int diff_levels(sw_engine* h, int level, int skip, int* fine_hid, int* lcoarse) {
  *lcoarse = level + (skip ? 2 : 1);
  if (*lcoarse >= h->hier[0].nlevels) return sw_fail(h, "no coarse level %d", *lcoarse);
  return solve_hier(h, level, fine_hid);
}

// The operator on the block x [n_level][nbp] up to its last step: z = A_l^-1 x and *y = A_c^-1 R x on level + 1
// (skip: P_1 A_2^-1 R_1 R_0 x).  The caller finishes d = z - P_l y: launch_ell(P_l, 1, y, z, d) in one launch, or
// w = P_l y and two dots (modes 1 / 2).  ca, cb: two coarse blocks [n_{level+1}][nbp] (with skip the level two below
// is smaller and fits in them), *y is one of them.  count_nb > 0: the stream is drained after each solve and the
// iteration counts of the first count_nb columns go to last_iters_f / last_iters_c; without it nothing here waits for
// the device.  total_f (optional) = the fine solve's iteration total.
static int diff_apply(sw_engine* h, int fine_hid, int level, int lcoarse, const cplx* x, int nbp, cplx* z, cplx* ca,
                      cplx* cb, double tol, int maxiter, int count_nb, const cplx** y, int* total_f) {
  Hier& H0 = h->hier[0];
  const bool skip = lcoarse == level + 2;
  // xc = R x (skip: R_1 R_0 x)             utils.py:298-304
  SWCHK(launch_ell(h, H0.lv[level].R, 0, x, nullptr, ca, nbp, T_R));
  const cplx* xc = ca;
  cplx* yc = cb;
  if (skip) {
    SWCHK(launch_ell(h, H0.lv[1].R, 0, ca, nullptr, cb, nbp, T_R));
    xc = cb;
    yc = ca;
  }
  int tf = 0, tc = 0;
  SWCHK(solve_dev(h, fine_hid, level, x, z, tol, maxiter, nbp, &tf));
  if (count_nb) SWCHK(record_level_iters(h, h->hier[fine_hid], level, tf, h->last_iters_f, count_nb));
  // y = A_c^-1 xc                           utils.py:306-329
  SWCHK(solve_dev(h, 0, lcoarse, xc, yc, tol, maxiter, nbp, &tc));
  if (count_nb) SWCHK(record_level_iters(h, H0, lcoarse, tc, h->last_iters_c, count_nb));
  if (skip) {
    SWCHK(launch_ell(h, H0.lv[1].P, 0, yc, nullptr, cb, nbp, T_P));
    yc = cb;
  }
  *y = yc;
  if (total_f) *total_f = tf;
  return 0;
}

// The frame of the column-blocked sums sum_j S_q(Pi u_j, Pi v_j) of sw_coarsest_loops and sw_level_deflation_loops:
// 64 columns per pass, prolonged to the lattice level and reduced with k_slice_cdots; the passes are added in
// ascending order on the device and the 64 columns of the sum by one host loop in ascending order, so two calls agree
// bit for bit.  The probe workspace and the loop buffers of the modes are not touched.
struct BlockSums {
  size_t rows;
  DevBuf<cplx> s[4], acc, part;
  explicit BlockSums(sw_engine* h)
      : rows(loop_rows(h)), s{DevBuf<cplx>(h), DevBuf<cplx>(h), DevBuf<cplx>(h), DevBuf<cplx>(h)}, acc(h), part(h) {}
};
// scratch for blocks of `level` and the zeroed sum
static int sums_begin(sw_engine* h, BlockSums& S, int level) {
  int nmax = 0;
  for (int l = 0; l < h->hier[0].nlevels; ++l) nmax = std::max(nmax, h->hier[0].lv[l].n);
  if (level > 0)
    for (auto& b : S.s) SWCHK(dev_realloc(h, &b.p, (size_t)nmax * 64));
  SWCHK(dev_realloc(h, &S.acc.p, S.rows * 64));
  SWCHK(dev_realloc(h, &S.part.p, S.rows * 64));
  return zero_vec(h, S.acc, (int)S.rows, 64);
}
// acc += S_q(Pi U, Pi V) of the blocks U, V [n_level][64]
static int sums_add(sw_engine* h, BlockSums& S, int level, const cplx* U, const cplx* V) {
  const cplx *u, *v;
  SWCHK(prolong_to_lattice(h, level, U, S.s[0], S.s[1], 64, &u));
  SWCHK(prolong_to_lattice(h, level, V, S.s[2], S.s[3], 64, &v));
  SWCHK(slice_cdots_into(h, h->hier[0].lv[0], u, v, 64, S.part));
  return vec_add(h, S.acc, S.part, S.acc, (int)S.rows, 64);
}
// out[p][a][b][t] = the sum over the 64 columns
static int sums_finish(sw_engine* h, BlockSums& S, double* out) {
  SWCHK(stream_sync(h));
  std::vector<std::complex<double>> ha(S.rows * 64);
  HIPCHK(hipMemcpy(ha.data(), S.acc.p, ha.size() * sizeof(cplx), hipMemcpyDeviceToHost));
  for (size_t r = 0; r < S.rows; ++r) {
    std::complex<double> sum(0.0, 0.0);
    for (int c = 0; c < 64; ++c) sum += ha[r * 64 + c];
    out[2 * r] = sum.real();
    out[2 * r + 1] = sum.imag();
  }
  return 0;
}

// The exact coarsest term of the MLMC loops: out[p][a][b][t] = sum_j S_q(Pi e_j, Pi A_c^-1 e_j), Pi = P_0 ... P_{M-2},
// on 64-column blocks of the identity and of the coarsest inverse (BlockSums).
int sw_coarsest_loops(sw_engine* h, double* out) {
  SWCHK(check_hier(h, 0, 0, true));
  if (!out) return sw_fail(h, "null output");
  if (h->momenta.empty()) return sw_fail(h, "no momenta registered (sw_set_loop_momenta)");
  Hier& H0 = h->hier[0];
  if (H0.nlevels < 2) return sw_fail(h, "the coarsest loops need at least two levels");
  HIPCHK(hipSetDevice(h->device));
  const int last = H0.nlevels - 1;
  const int nc = H0.lv[last].n, nbp = 64;
  DevBuf<cplx> E(h), Y(h);
  BlockSums S(h);
  SWCHK(dev_realloc(h, &E.p, (size_t)nc * nbp));
  SWCHK(dev_realloc(h, &Y.p, (size_t)nc * nbp));
  SWCHK(sums_begin(h, S, last));
  std::vector<std::complex<double>> he((size_t)nc * nbp);
  for (int j0 = 0; j0 < nc; j0 += 64) {
    std::fill(he.begin(), he.end(), std::complex<double>(0.0, 0.0));
    for (int c = 0; c < 64 && j0 + c < nc; ++c) he[(size_t)(j0 + c) * nbp + c] = 1.0;   // any order of the unit vectors gives the sum
    SWCHK(stream_sync(h));                 // the previous block's reads of E are done
    HIPCHK(hipMemcpy(E.p, he.data(), he.size() * sizeof(cplx), hipMemcpyHostToDevice));
    SWCHK(apply_coarsest(h, H0, E, Y, nbp));
    SWCHK(sums_add(h, S, last, E, Y));
  }
  return sums_finish(h, S, out);
}

// The deflated part of a level's term of the MLMC loops: out[p][a][b][t] = sum_j S_q(Pi V_j, Pi D V_j) over the
// vectors V_j registered at `level` (sw_set_level_deflation), D the level's difference operator through diff_apply,
// Pi = P_0 ... P_{level-1}; 64 columns of V per pass (BlockSums).
int sw_level_deflation_loops(sw_engine* h, int level, int skip, double tol, int maxiter, double* out) {
  SWCHK(check_hier(h, 0, level, true));
  if (!out) return sw_fail(h, "null output");
  if (skip != 0 && skip != 1) return sw_fail(h, "skip must be 0 or 1");
  if (maxiter < 1) return sw_fail(h, "maxiter must be >= 1");
  if (h->momenta.empty()) return sw_fail(h, "no momenta registered (sw_set_loop_momenta)");
  Hier& H0 = h->hier[0];
  if (skip && level != 0) return sw_fail(h, "level skipping is defined for level 0 only");
  int fine_hid, lcoarse;
  SWCHK(diff_levels(h, level, skip, &fine_hid, &lcoarse));
  const int k = h->lkd[level];
  if (k <= 0 || !h->lV[level]) return sw_fail(h, "no deflation vectors registered at level %d", level);
  HIPCHK(hipSetDevice(h->device));
  Level& lv = H0.lv[level];
  const int n = lv.n, n1 = H0.lv[level + 1].n, nbp = 64, ld = defl_ld(k);
  DevBuf<cplx> X(h), Z(h), Dv(h), ca(h), cb(h);
  BlockSums S(h);
  SWCHK(dev_realloc(h, &X.p, (size_t)n * nbp));
  SWCHK(dev_realloc(h, &Z.p, (size_t)n * nbp));
  SWCHK(dev_realloc(h, &Dv.p, (size_t)n * nbp));
  // two coarse blocks of the level below (with skip the level two below is smaller and fits in them)
  SWCHK(dev_realloc(h, &ca.p, (size_t)n1 * nbp));
  SWCHK(dev_realloc(h, &cb.p, (size_t)n1 * nbp));
  SWCHK(sums_begin(h, S, level));
  for (int j0 = 0; j0 < k; j0 += 64) {
    // x = the columns [j0, j0 + 64) of V, zero beyond the last vector (a zero column adds exact zeros)
    const int nc = std::min(64, k - j0);
    SWCHK(zero_vec(h, X, n, nbp));
    HIPCHK(hipMemcpy2DAsync(X.p, (size_t)nbp * sizeof(cplx), h->lV[level] + j0, (size_t)ld * sizeof(cplx),
                            (size_t)nc * sizeof(cplx), (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    // d = z - P y
    const cplx* y;
    SWCHK(diff_apply(h, fine_hid, level, lcoarse, X, nbp, Z, ca, cb, tol, maxiter, 0, &y, nullptr));
    SWCHK(launch_ell(h, lv.P, 1, y, Z, Dv, nbp, T_P));
    SWCHK(sums_add(h, S, level, X, Dv));
  }
  return sums_finish(h, S, out);
}

// ---- one-end-trick two-point functions from timeslice sources ------------------------------------------
int sw_set_two_point(sw_engine* h, int t0, int nmom, const int32_t* p) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nmom < 0 || nmom > SW_MAX_MOMENTA)
    return sw_fail(h, "%d momenta: at most %d per registration", nmom, SW_MAX_MOMENTA);
  h->r_tp.drop();
  h->r_lma.drop();
  h->r_tps.drop();
  if (nmom == 0) {
    h->tp_momenta.clear();
    return 0;
  }
  SWCHK(check_momenta(h, "two-point functions", nmom, p));
  const int L = h->hier[0].lv[0].L;
  if (t0 < 0 || t0 >= L) return sw_fail(h, "source timeslice %d outside [0,%d)", t0, L);
  int j0 = -1;
  for (int j = 0; j < nmom; ++j)
    if (p[j] == 0) j0 = j;
  if (j0 < 0) return sw_fail(h, "the two-point momenta have to contain 0 (its solutions are the conjugated factor)");
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  SWCHK(upload_slice_tables(h, nmom, p, &h->tp_mom, &h->tp_phase, &h->tp_slicerow));
  h->tp_momenta.assign(p, p + nmom);
  h->tp_t0 = t0;
  h->tp_j0 = j0;
  return 0;
}

// the sources and solutions of a two-point batch: two blocks [n][ncols], ncols = 2 M nq
static int ensure_two_point_ws(sw_engine* h, size_t cnt) {
  if (h->tp_ws_cap >= cnt && h->tp_rhs) return 0;
  SWCHK(dev_realloc(h, &h->tp_rhs, cnt));
  SWCHK(dev_realloc(h, &h->tp_z, cnt));
  h->tp_ws_cap = cnt;
  return 0;
}

// rhs[row][(2 j + a) nq + k] = the source eta_k^(j,a) of every registered momentum j, spin a and noise k < nb
static int slice_sources(sw_engine* h, Level& lv, const int8_t* probes, int nb, int nq, cplx* rhs) {
  const int ncols = 2 * (int)h->tp_momenta.size() * nq;
  return launch(h, T_TP_SOURCES, swk::k_slice_sources, dim3((lv.n + 15) / 16, ncols / 64), dim3(SW_BLOCK), probes, nb,
                lv.n, (const int*)lv.rowmap, (const cplx*)h->tp_phase, (const int*)h->tp_mom, lv.L, h->tp_t0, nq,
                ncols, rhs);
}

// res[j][a][b][c][d][t][k] from the solutions Z [n][2 M nq]: the p = 0 instantiation for the registered
// momentum 0, the phased one over the others; total (optional) = sum_t sum_ac T[j0][a][a][c][c][t][k]
// (pair_dots_into: the same launches into `out`, M 16 L rows of a buffer the caller has begun)
static int pair_dots_into(sw_engine* h, Level& lv, const cplx* Z, int nq, cplx* out, cplx* total) {
  const int M = (int)h->tp_momenta.size(), L = lv.L;
  const int ncols = 2 * M * nq;
  SWCHK(launch(h, T_TP_DOTS, swk::k_slice_pair_dots<false>, dim3(L, nq / 64, 1), dim3(SW_BLOCK), Z,
               (const int*)h->tp_slicerow, (const cplx*)h->tp_phase, (const int*)h->tp_mom, h->tp_j0, L, nq, ncols,
               out));
  if (M > 1)
    SWCHK(launch(h, T_TP_DOTS, swk::k_slice_pair_dots<true>, dim3(L, nq / 64, M - 1), dim3(SW_BLOCK), Z,
                 (const int*)h->tp_slicerow, (const cplx*)h->tp_phase, (const int*)h->tp_mom, h->tp_j0, L, nq,
                 ncols, out));
  if (!total) return 0;
  return launch(h, T_TP_DOTS, swk::k_pair_total, dim3(nq / 64), dim3(SW_BLOCK), (const cplx*)out, h->tp_j0, L, nq,
                total);
}
static int pair_dots(sw_engine* h, Level& lv, const cplx* Z, int nq, ResultBuf& res, cplx* total) {
  SWCHK(result_begin(h, res, h->tp_momenta.size() * 16 * lv.L, nq));
  return pair_dots_into(h, lv, Z, nq, res.p, total);
}

static int two_point_args(sw_engine* h, int nb, const void* in, const void* out) {
  SWCHK(check_hier(h, 0, 0, false));
  if (h->tp_momenta.empty()) return sw_fail(h, "no two-point registration (sw_set_two_point)");
  if (nb <= 0 || !in || !out) return sw_fail(h, "bad arguments");
  return 0;
}

// The source kernel alone: out[g][k][n] (reference ordering), g = 2 j + a, from the int8 probes [nb][n].
int sw_apply_slice_sources(sw_engine* h, int nb, const int8_t* probes, double* out) {
  SWCHK(two_point_args(h, nb, probes, out));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int nq = pad64(nb), G = 2 * (int)h->tp_momenta.size();
  SWCHK(ensure_two_point_ws(h, (size_t)lv.n * G * nq));
  DevBuf<int8_t> pr(h);
  SWCHK(upload(h, &pr.p, probes, (size_t)nb * lv.n));
  SWCHK(slice_sources(h, lv, pr, nb, nq, h->tp_rhs));
  const size_t per = (size_t)nb * lv.n;
  SWCHK(ensure_stage(h, per * G * sizeof(cplx)));
  for (int g = 0; g < G; ++g)
    SWCHK(launch(h, T_OTHER, swk::k_unpack_c, dim3((lv.n + 63) / 64, nq / 64), dim3(SW_BLOCK),
                 (const cplx*)(h->tp_rhs + (size_t)g * nq), G * nq, lv.n, (const int*)lv.rowmap,
                 (cplx*)h->stage + (size_t)g * per, nb));
  HIPCHK(hipMemcpyAsync(out, h->stage, per * G * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
  return stream_sync(h);
}

// The pair-dot kernels alone on host solutions Z[g][k][n] (reference ordering): out[j][a][b][c][d][t][k].
int sw_apply_pair_dots(sw_engine* h, int nb, const double* Z, double* out) {
  SWCHK(two_point_args(h, nb, Z, out));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int nq = pad64(nb), G = 2 * (int)h->tp_momenta.size();
  SWCHK(ensure_two_point_ws(h, (size_t)lv.n * G * nq));
  const size_t per = (size_t)nb * lv.n;
  SWCHK(ensure_stage(h, per * G * sizeof(cplx)));
  HIPCHK(hipMemcpyAsync(h->stage, Z, per * G * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
  for (int g = 0; g < G; ++g)
    SWCHK(launch(h, T_OTHER, swk::k_pack_c, dim3((lv.n + 63) / 64, nq / 64), dim3(SW_BLOCK),
                 (const cplx*)h->stage + (size_t)g * per, nb, lv.n, (const int*)lv.rowmap,
                 h->tp_z + (size_t)g * nq, G * nq));
  SWCHK(pair_dots(h, lv, h->tp_z, nq, h->r_tp, nullptr));
  SWCHK(stream_sync(h));
  return result_fetch(h, h->r_tp, nb, out);
}

int sw_hutch_fetch_two_point(sw_engine* h, double* out) {
  return fetch_result(h, &sw_engine::r_tp, "no two-point batch to fetch", out);
}

int sw_hutch_fetch_two_point_lma(sw_engine* h, double* out) {
  return fetch_result(h, &sw_engine::r_lma, "no low-mode averaged two-point batch to fetch", out);
}

// ---- smeared sources and sinks: gauge-covariant Jacobi smearing of the two-point functions' quark fields -----
int sw_set_smearing(sw_engine* h, double kappa, int source_steps, int nsink, const int32_t* sink_steps) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nsink < 0 || nsink > SW_MAX_SINK_LEVELS)
    return sw_fail(h, "%d sink smearing levels: at most %d per registration", nsink, SW_MAX_SINK_LEVELS);
  h->r_tps.drop();
  if (nsink == 0) {
    h->sm_sink.clear();
    return 0;
  }
  Level& lv = h->hier[0].lv[0];
  if (!lv.stencil || !lv.U1 || !lv.U2 || lv.h_rowmap.empty())
    return sw_fail(h, "smearing needs a lattice level 0 with links (sw_set_lattice)");
  if (!sink_steps) return sw_fail(h, "null sink step list");
  if (!(kappa > 0.0) || !std::isfinite(kappa))
    return sw_fail(h, "smearing kappa %g has to be positive and finite", kappa);
  if (source_steps < 0 || source_steps > SW_MAX_SMEARING_STEPS)
    return sw_fail(h, "%d source smearing steps outside [0,%d]", source_steps, SW_MAX_SMEARING_STEPS);
  for (int i = 0; i < nsink; ++i) {
    if (sink_steps[i] < 0 || sink_steps[i] > SW_MAX_SMEARING_STEPS)
      return sw_fail(h, "%d sink smearing steps outside [0,%d]", (int)sink_steps[i], SW_MAX_SMEARING_STEPS);
    if (i > 0 && sink_steps[i] <= sink_steps[i - 1])
      return sw_fail(h, "sink smearing steps have to ascend strictly (%d after %d)", (int)sink_steps[i],
                     (int)sink_steps[i - 1]);
  }
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  SWCHK(upload_slicerow(h, &h->sm_slicerow));
  h->sm_kappa = kappa;
  // the two coefficients of a step (smear_site): each two roundings away from its exact value
  h->sm_c0 = 1.0 / (1.0 + 2.0 * kappa);
  h->sm_c1 = kappa / (1.0 + 2.0 * kappa);
  h->sm_source = source_steps;
  h->sm_sink.assign(sink_steps, sink_steps + nsink);
  return 0;
}

static int smearing_ready(sw_engine* h) {
  if (h->sm_sink.empty()) return sw_fail(h, "no smearing registration (sw_set_smearing)");
  return 0;
}
static bool smear_has_fused(int L) { return L == 16 || L == 128; }

// X [n][ncols] <- S^steps X on the nt timeslices from t_first on (both spins), in place: the fused kernel where L has
// an instantiation and `fused`, else `steps` launches of k_smear_step alternating with `tmp` (as large as X; only
// the rows of those lines are written) and, after an odd count, the copy back.  steps = 0: nothing is launched.
static int smear(sw_engine* h, Level& lv, cplx* X, cplx* tmp, int ncols, int t_first, int nt, int steps, bool fused) {
  if (steps == 0) return 0;
  const dim3 grid(2 * nt, ncols / 64);
  const int* sr = h->sm_slicerow;
  const cplx* U = lv.U1;
  if (fused && lv.L == 16)
    return launch(h, T_SMEAR, swk::k_smear_fused<4>, grid, dim3(SW_BLOCK), X, sr, U, t_first, ncols, h->sm_c0,
                  h->sm_c1, steps);
  if (fused && lv.L == 128)
    return launch(h, T_SMEAR, swk::k_smear_fused<32>, grid, dim3(SW_BLOCK), X, sr, U, t_first, ncols, h->sm_c0,
                  h->sm_c1, steps);
  cplx *a = X, *b = tmp;
  for (int k = 0; k < steps; ++k, std::swap(a, b))
    SWCHK(launch(h, T_SMEAR, swk::k_smear_step<false>, grid, dim3(SW_BLOCK), (const cplx*)a, b, sr, U, lv.L, t_first,
                 ncols, h->sm_c0, h->sm_c1));
  if (a == X) return 0;
  return launch(h, T_SMEAR, swk::k_smear_step<true>, grid, dim3(SW_BLOCK), (const cplx*)tmp, X, sr, U, lv.L, t_first,
                ncols, h->sm_c0, h->sm_c1);
}

// Y = S^steps X on nb host vectors (reference ordering), every timeslice: the smearing kernels alone.
int sw_apply_smearing(sw_engine* h, int nb, int steps, int fused, const double* X, double* Y) {
  SWCHK(check_hier(h, 0, 0, false));
  SWCHK(smearing_ready(h));
  if (nb <= 0 || !X || !Y) return sw_fail(h, "bad arguments");
  if (steps < 0 || steps > SW_MAX_SMEARING_STEPS)
    return sw_fail(h, "%d smearing steps outside [0,%d]", steps, SW_MAX_SMEARING_STEPS);
  Level& lv = h->hier[0].lv[0];
  if (fused && !smear_has_fused(lv.L))
    return sw_fail(h, "no fused smearing kernel for L=%d (16 and 128 have one)", lv.L);
  HIPCHK(hipSetDevice(h->device));
  const int nbp = pad64(nb);
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  SWCHK(pack_host(h, lv, nb, X, a, nbp));
  SWCHK(smear(h, lv, a, b, nbp, 0, lv.L, steps, fused != 0));
  return unpack_host(h, lv, nb, a, Y, nbp);
}

int sw_hutch_fetch_two_point_smeared(sw_engine* h, double* out) {
  return fetch_result(h, &sw_engine::r_tps, "no smeared two-point batch to fetch", out);
}

// ---- distillation: perambulators between the Laplacian eigenvectors of the timeslices -----------------------
// the elementals belong to the eigenvectors they were made from
static int drop_laph_momenta(sw_engine* h) {
  h->lh_momenta.clear();
  SWCHK(dev_free(h, h->lh_M));
  h->lh_M = nullptr;
  return 0;
}

int sw_set_distillation(sw_engine* h, int nev, const double* V) {
  SWCHK(check_hier(h, 0, 0, false));
  SWCHK(drop_laph_momenta(h));
  if (nev == 0) {
    h->lh_nev = 0;
    return 0;
  }
  Level& lv = h->hier[0].lv[0];
  if (!lv.stencil || lv.h_rowmap.empty())
    return sw_fail(h, "distillation needs a lattice level 0 (sw_set_lattice)");
  const int L = lv.L;
  if (nev < 1 || nev > std::min(L, SW_MAX_LAPH))
    return sw_fail(h, "%d distillation vectors outside [1,%d]", nev, std::min(L, SW_MAX_LAPH));
  if (!V) return sw_fail(h, "null eigenvectors");
  swp::LaphHost p;
  swp::laph_pack(p, L, nev, (const std::complex<double>*)V);
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  h->lh_nev = 0;
  SWCHK(upload_slicerow(h, &h->lh_slicerow));
  SWCHK(upload(h, (std::complex<double>**)&h->lh_V, p.v.data(), p.v.size()));
  h->lh_Lp = p.Lp;
  h->lh_ld = p.ld;
  h->lh_nev = nev;
  return 0;
}

static int distillation_ready(sw_engine* h) {
  if (h->lh_nev <= 0 || !h->lh_V) return sw_fail(h, "no distillation registration (sw_set_distillation)");
  return 0;
}
// distinct source timeslices inside [0, L), in any order
static int check_source_timeslices(sw_engine* h, int nsrc, const int32_t* t0) {
  const int L = h->hier[0].lv[0].L;
  if (nsrc < 1 || nsrc > L) return sw_fail(h, "%d source timeslices outside [1,%d]", nsrc, L);
  if (!t0) return sw_fail(h, "null source timeslice list");
  std::vector<char> seen(L, 0);
  for (int s = 0; s < nsrc; ++s) {
    if (t0[s] < 0 || t0[s] >= L) return sw_fail(h, "source timeslice %d outside [0,%d)", (int)t0[s], L);
    if (seen[t0[s]]) return sw_fail(h, "source timeslice %d listed twice", (int)t0[s]);
    seen[t0[s]] = 1;
  }
  return 0;
}

// rhs [n][ncols] = the eigenvector sources of the global columns [col_first, col_first + nvalid), pad columns zero
static int laph_sources(sw_engine* h, Level& lv, const int* d_t0, int col_first, int nvalid, int ncols, cplx* rhs) {
  return launch(h, T_LAPH_SRC, swk::k_laph_sources, dim3((lv.n + 15) / 16, ncols / 64), dim3(SW_BLOCK),
                (const cplx*)h->lh_V, h->lh_ld, h->lh_Lp, h->lh_nev, d_t0, col_first, nvalid, lv.n,
                (const int*)lv.rowmap, lv.L, ncols, rhs);
}
// out [L][2][nev][ncols] = the projection of the block Z [n][ncols] onto every timeslice's eigenvectors
static int laph_project(sw_engine* h, Level& lv, const cplx* Z, int ncols, cplx* out) {
  const int L = lv.L, ld = h->lh_ld;
  if (h->profiling) h->twork[T_LAPH] += 8.0 * 2.0 * (double)L * (double)L * (double)ld * (double)ncols;
  return pick<1, 2, 3, 4, 5, 6, 7, 8>(ld / 16, [&](auto NT) {
    return launch(h, T_LAPH, swk::k_laph_project<decltype(NT)::value>, dim3(L, 2, ncols / 64), dim3(SW_BLOCK),
                  (const cplx*)h->lh_V, ld, h->lh_Lp, h->lh_nev, Z, (const int*)h->lh_slicerow, L, ncols, out);
  });
}

// One solve block of the perambulators: the global columns [c0, c0 + nvalid) of the sources d_t0, padded to ncols --
// k_laph_sources -> solve_dev on hierarchy hid -> k_laph_project into proj [L][2][nev][ncols]; the blocks live in the
// two-point workspace (ensure_two_point_ws by the caller).  iters (or NULL): the nvalid iteration counts.
static int laph_block(sw_engine* h, int hid, Level& lv, const int* d_t0, int c0, int nvalid, int ncols, double tol,
                      int maxiter, cplx* proj, int32_t* iters) {
  SWCHK(laph_sources(h, lv, d_t0, c0, nvalid, ncols, h->tp_rhs));
  int tot = 0;
  SWCHK(solve_dev(h, hid, 0, h->tp_rhs, h->tp_z, tol, maxiter, ncols, &tot));
  std::vector<int32_t> it;
  SWCHK(record_level_iters(h, h->hier[hid], 0, tot, it, nvalid));
  if (iters) std::copy(it.begin(), it.end(), iters);
  return laph_project(h, lv, h->tp_z, ncols, proj);
}
// The global columns [c0, c0 + nvalid) between the block proj [L][2][nev][ncols] (its columns 0 ..) and the host
// perambulators tau [nsrc][L][2][nev][nev][2]: the columns of one source timeslice are contiguous in tau, one strided
// copy per timeslice the block touches.  to_host: proj -> tau, else tau -> proj.  The stream has drained.
static int laph_copy_tau(sw_engine* h, cplx* tau, int c0, int nvalid, int ncols, cplx* proj, bool to_host) {
  const int per = 2 * h->lh_nev;
  const size_t rows = (size_t)h->hier[0].lv[0].L * per;
  for (int c = c0; c < c0 + nvalid;) {
    const int s = c / per, e = std::min(c0 + nvalid, (s + 1) * per);
    cplx* host = tau + (size_t)s * rows * per + (c - s * per);
    cplx* dev = proj + (c - c0);
    if (to_host)
      HIPCHK(hipMemcpy2D(host, sizeof(cplx) * per, dev, sizeof(cplx) * ncols, sizeof(cplx) * (e - c), rows,
                         hipMemcpyDeviceToHost));
    else
      HIPCHK(hipMemcpy2D(dev, sizeof(cplx) * ncols, host, sizeof(cplx) * per, sizeof(cplx) * (e - c), rows,
                         hipMemcpyHostToDevice));
    c = e;
  }
  return 0;
}

// tau[s][t][c][m][n][a] = sum_x conj(v_m(x,t)) z^(s,n,a)[idx(c,x,t)], z = A^-1 eta for the eigenvector sources of the
// nsrc source timeslices: the 2 nev nsrc columns in blocks of at most 256 (padded to 64 with zero columns), each block
// k_laph_sources -> solve_dev on the hierarchy of solve_hier (no deflation, no permutation) -> k_laph_project -> the
// copy to `out`.  Stateless: no mode buffer and no probe slot is touched; the blocks live in the two-point workspace,
// everything else for this call only.
int sw_perambulators(sw_engine* h, int nsrc, const int32_t* t0, double tol, int maxiter, double* out,
                     int32_t* iters) {
  SWCHK(check_hier(h, 0, 0, true));
  SWCHK(distillation_ready(h));
  SWCHK(check_source_timeslices(h, nsrc, t0));
  if (maxiter < 1) return sw_fail(h, "maxiter must be >= 1");
  if (!out) return sw_fail(h, "null output");
  int hid;
  SWCHK(solve_hier(h, 0, &hid));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int n = lv.n, L = lv.L, nev = h->lh_nev, per = 2 * nev, total = per * nsrc;
  const int bmax = std::min(256, pad64(total));
  const size_t rows = (size_t)L * 2 * nev;
  DevBuf<int> d_t0(h);
  DevBuf<cplx> proj(h);
  SWCHK(upload(h, &d_t0.p, (const int*)t0, (size_t)nsrc));
  SWCHK(ensure_two_point_ws(h, (size_t)n * bmax));
  SWCHK(dev_realloc(h, &proj.p, rows * bmax));
  for (int c0 = 0; c0 < total; c0 += 256) {
    const int nvalid = std::min(256, total - c0), ncols = pad64(nvalid);
    SWCHK(laph_block(h, hid, lv, d_t0, c0, nvalid, ncols, tol, maxiter, proj, iters ? iters + c0 : nullptr));
    SWCHK(stream_sync(h));
    SWCHK(laph_copy_tau(h, (cplx*)out, c0, nvalid, ncols, proj, true));
  }
  return 0;
}

// k_laph_sources alone: out complex128 [nsrc nev 2][n], the sources in the reference ordering, column (s, n, a).
int sw_apply_laph_sources(sw_engine* h, int nsrc, const int32_t* t0, double* out) {
  SWCHK(check_hier(h, 0, 0, false));
  SWCHK(distillation_ready(h));
  SWCHK(check_source_timeslices(h, nsrc, t0));
  if (!out) return sw_fail(h, "null output");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int total = 2 * h->lh_nev * nsrc;
  DevBuf<int> d_t0(h);
  DevBuf<cplx> rhs(h);
  SWCHK(upload(h, &d_t0.p, (const int*)t0, (size_t)nsrc));
  SWCHK(dev_realloc(h, &rhs.p, (size_t)lv.n * 256));
  for (int c0 = 0; c0 < total; c0 += 256) {
    const int nvalid = std::min(256, total - c0), ncols = pad64(nvalid);
    SWCHK(laph_sources(h, lv, d_t0, c0, nvalid, ncols, rhs));
    SWCHK(unpack_host(h, lv, nvalid, rhs, out + (size_t)2 * c0 * lv.n, ncols));
  }
  return 0;
}

// k_laph_project alone on nb host vectors Z [nb][n] (reference ordering): out complex128 [L][2][nev][nb].
int sw_apply_laph_project(sw_engine* h, int nb, const double* Z, double* out) {
  SWCHK(check_hier(h, 0, 0, false));
  SWCHK(distillation_ready(h));
  if (nb <= 0 || !Z || !out) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int nbp = pad64(nb);
  const size_t rows = (size_t)lv.L * 2 * h->lh_nev;
  DevBuf<cplx> z(h), proj(h);
  SWCHK(dev_realloc(h, &z.p, (size_t)lv.n * nbp));
  SWCHK(dev_realloc(h, &proj.p, rows * nbp));
  SWCHK(pack_host(h, lv, nb, Z, z, nbp));
  SWCHK(laph_project(h, lv, z, nbp, proj));
  SWCHK(stream_sync(h));
  HIPCHK(hipMemcpy2D(out, sizeof(cplx) * nb, proj.p, sizeof(cplx) * nbp, sizeof(cplx) * nb, rows,
                     hipMemcpyDeviceToHost));
  return 0;
}

// ---- distillation: the two-point functions contracted on the device ----------------------------------------
// The momenta of sw_distilled_two_point with their elementals, computed here once and kept on the device:
// Mt[j][t][ld][ld], transposed and padded (k_laph_elementals), nmom L ld^2 16 bytes.  Any sw_set_distillation and a
// new definition of hierarchy 0 drop them.
int sw_set_distillation_momenta(sw_engine* h, int nmom, const int32_t* p) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nmom < 0 || nmom > SW_MAX_MOMENTA)
    return sw_fail(h, "%d momenta: at most %d per registration", nmom, SW_MAX_MOMENTA);
  if (nmom == 0) return drop_laph_momenta(h);
  SWCHK(distillation_ready(h));
  SWCHK(check_momenta(h, "distilled two-point functions", nmom, p));
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  SWCHK(drop_laph_momenta(h));
  SWCHK(upload_slice_tables(h, nmom, p, &h->lh_mom, &h->lh_phase, &h->lh_slicerow));
  Level& lv = h->hier[0].lv[0];
  const int L = lv.L, ld = h->lh_ld, Lp = h->lh_Lp;
  const size_t per = (size_t)L * ld * ld;
  SWCHK(dev_realloc(h, &h->lh_M, (size_t)nmom * per));
  const dim3 grid(L, (ld / 16 + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK);
  for (int j = 0; j < nmom; ++j) {
    if (h->profiling) h->twork[T_LAPH_CONTRACT] += 8.0 * (double)L * (double)Lp * (double)ld * (double)ld;
    if (p[j] == 0)
      SWCHK(launch(h, T_LAPH_CONTRACT, swk::k_laph_elementals<false>, grid, dim3(SW_BLOCK), (const cplx*)h->lh_V, ld,
                   Lp, h->lh_nev, (const cplx*)h->lh_phase, 0, L, h->lh_M + j * per));
    else
      SWCHK(launch(h, T_LAPH_CONTRACT, swk::k_laph_elementals<true>, grid, dim3(SW_BLOCK), (const cplx*)h->lh_V, ld,
                   Lp, h->lh_nev, (const cplx*)h->lh_phase, (int)p[j], L, h->lh_M + j * per));
  }
  SWCHK(stream_sync(h));
  h->lh_momenta.assign(p, p + nmom);
  return 0;
}

static int laph_momenta_ready(sw_engine* h) {
  if (h->lh_momenta.empty() || !h->lh_M)
    return sw_fail(h, "no distillation momenta registered (sw_set_distillation_momenta)");
  return 0;
}

// out complex128 [nmom][L][nev][nev]: the registered elementals M[j][t][m][m'], untransposed and dense.
int sw_apply_laph_elementals(sw_engine* h, double* out) {
  SWCHK(check_hier(h, 0, 0, false));
  SWCHK(distillation_ready(h));
  SWCHK(laph_momenta_ready(h));
  if (!out) return sw_fail(h, "null output");
  HIPCHK(hipSetDevice(h->device));
  const int nev = h->lh_nev, nz = (int)h->lh_momenta.size() * h->hier[0].lv[0].L;
  const size_t cnt = (size_t)nz * nev * nev;
  DevBuf<cplx> dense(h);
  SWCHK(dev_realloc(h, &dense.p, cnt));
  SWCHK(launch(h, T_LAPH_CONTRACT, swk::k_laph_elementals_unpack, dim3((nev * nev + SW_BLOCK - 1) / SW_BLOCK, nz),
               dim3(SW_BLOCK), (const cplx*)h->lh_M, h->lh_ld, nev, dense.p));
  SWCHK(stream_sync(h));
  HIPCHK(hipMemcpy(out, dense.p, cnt * sizeof(cplx), hipMemcpyDeviceToHost));
  return 0;
}

// The blocks of sw_distilled_two_point and sw_apply_laph_contract: whole sources, max(1, 256 / (2 nev)) per block
static inline int laph_sources_per_block(int nev) { return std::max(1, 256 / (2 * nev)); }

// The workspace of the contraction of one block: Y [2 L][ncols][ld], X [2 L][ns][2][nev][ld], T [ns][nmom][16][L],
// loops [ns][nmom][4], sized for the largest block of the call and reused by every momentum and block.
struct LaphContractWS {
  DevBuf<cplx> Y, X, T, loops;
  explicit LaphContractWS(sw_engine* h) : Y(h), X(h), T(h), loops(h) {}
};
static int laph_contract_ws(sw_engine* h, LaphContractWS& ws, int ns, int ncols) {
  const int L = h->hier[0].lv[0].L, nev = h->lh_nev, ld = h->lh_ld, nmom = (int)h->lh_momenta.size();
  SWCHK(dev_realloc(h, &ws.Y.p, (size_t)2 * L * ncols * ld));
  SWCHK(dev_realloc(h, &ws.X.p, (size_t)2 * L * ns * 2 * nev * ld));
  SWCHK(dev_realloc(h, &ws.T.p, (size_t)ns * nmom * 16 * L));
  return dev_realloc(h, &ws.loops.p, (size_t)ns * nmom * 4);
}
// T [ns][nmom][2][2][2][2][L] and loops [ns][nmom][2][2] of the ns sources d_t0 whose columns are the first 2 nev ns of
// the projection block proj [L][2][nev][ncols], into the host arrays: per registered momentum k_laph_left ->
// k_laph_right -> k_laph_reduce (three launches of class SW_KCLASS_LAPH_CONTRACT), then two small copies.
static int laph_contract(sw_engine* h, const cplx* proj, const int* d_t0, int ns, int ncols, LaphContractWS& ws,
                         cplx* T, cplx* loops) {
  const int L = h->hier[0].lv[0].L, nev = h->lh_nev, ld = h->lh_ld, nmom = (int)h->lh_momenta.size();
  const int NTv = ld / 16, K4 = (nev + 3) / 4 * 4;
  const size_t per = (size_t)L * ld * ld;
  for (int j = 0; j < nmom; ++j) {
    const cplx* Mt = h->lh_M + j * per;
    if (h->profiling)
      h->twork[T_LAPH_CONTRACT] += 8.0 * (2.0 * L * (double)ncols * ld * K4 + 4.0 * L * (double)ns * ld * ld * K4 +
                                          16.0 * L * (double)ns * nev * nev + 4.0 * (double)ns * nev * nev);
    SWCHK(pick<1, 2, 3, 4, 5, 6, 7, 8>(NTv, [&](auto NT) {
      SWCHK(launch(h, T_LAPH_CONTRACT, swk::k_laph_left<decltype(NT)::value>, dim3(L, 2, ncols / 64), dim3(SW_BLOCK),
                   proj, nev, ncols, Mt, ld, ws.Y.p));
      return launch(h, T_LAPH_CONTRACT, swk::k_laph_right<decltype(NT)::value>,
                    dim3(2 * L, 2 * ns, (NTv + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK), dim3(SW_BLOCK),
                    (const cplx*)ws.Y.p, nev, ncols, Mt, ld, d_t0, ns, L, ws.X.p);
    }));
    SWCHK(launch(h, T_LAPH_CONTRACT, swk::k_laph_reduce, dim3(L, ns), dim3(SW_BLOCK), proj, nev, ncols,
                 (const cplx*)ws.X.p, Mt, ld, d_t0, ns, L, j, nmom, ws.T.p, ws.loops.p));
  }
  SWCHK(stream_sync(h));
  HIPCHK(hipMemcpy(T, ws.T.p, sizeof(cplx) * ns * nmom * 16 * L, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(loops, ws.loops.p, sizeof(cplx) * ns * nmom * 4, hipMemcpyDeviceToHost));
  return 0;
}

// The distilled two-point functions of nsrc source timeslices, solved, projected and contracted on the device: per
// block of whole sources laph_block (as sw_perambulators on that chunk) and laph_contract.  Stateless: no mode buffer,
// no probe slot and no registration is touched; everything but the two-point workspace lives for this call only.
int sw_distilled_two_point(sw_engine* h, int nsrc, const int32_t* t0, double tol, int maxiter, double* T,
                           double* loops, double* tau, int32_t* iters) {
  SWCHK(check_hier(h, 0, 0, true));
  SWCHK(distillation_ready(h));
  SWCHK(laph_momenta_ready(h));
  SWCHK(check_source_timeslices(h, nsrc, t0));
  if (maxiter < 1) return sw_fail(h, "maxiter must be >= 1");
  if (!T || !loops) return sw_fail(h, "null output");
  int hid;
  SWCHK(solve_hier(h, 0, &hid));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int L = lv.L, nev = h->lh_nev, per = 2 * nev, nmom = (int)h->lh_momenta.size();
  const int spb = laph_sources_per_block(nev), nsmax = std::min(spb, nsrc), bmax = pad64(nsmax * per);
  DevBuf<int> d_t0(h);
  DevBuf<cplx> proj(h);
  LaphContractWS ws(h);
  SWCHK(upload(h, &d_t0.p, (const int*)t0, (size_t)nsrc));
  SWCHK(ensure_two_point_ws(h, (size_t)lv.n * bmax));
  SWCHK(dev_realloc(h, &proj.p, (size_t)L * per * bmax));
  SWCHK(laph_contract_ws(h, ws, nsmax, bmax));
  for (int s0 = 0; s0 < nsrc; s0 += spb) {
    const int ns = std::min(spb, nsrc - s0), nvalid = ns * per, ncols = pad64(nvalid);
    SWCHK(laph_block(h, hid, lv, d_t0.p + s0, 0, nvalid, ncols, tol, maxiter, proj,
                     iters ? iters + (size_t)s0 * per : nullptr));
    SWCHK(laph_contract(h, proj, d_t0.p + s0, ns, ncols, ws, (cplx*)T + (size_t)s0 * nmom * 16 * L,
                        (cplx*)loops + (size_t)s0 * nmom * 4));
    if (tau) SWCHK(laph_copy_tau(h, (cplx*)tau + (size_t)s0 * L * per * per, 0, nvalid, ncols, proj, true));
  }
  return 0;
}

// The contraction alone on host perambulators tau [nsrc][L][2][nev][nev][2] (the layout of sw_perambulators), in the
// blocks of sw_distilled_two_point; the pad columns of a block are zeros.
int sw_apply_laph_contract(sw_engine* h, int nsrc, const int32_t* t0, const double* tau, double* T, double* loops) {
  SWCHK(check_hier(h, 0, 0, false));
  SWCHK(distillation_ready(h));
  SWCHK(laph_momenta_ready(h));
  SWCHK(check_source_timeslices(h, nsrc, t0));
  if (!tau || !T || !loops) return sw_fail(h, "null argument");
  HIPCHK(hipSetDevice(h->device));
  const int L = h->hier[0].lv[0].L, nev = h->lh_nev, per = 2 * nev, nmom = (int)h->lh_momenta.size();
  const int spb = laph_sources_per_block(nev), nsmax = std::min(spb, nsrc), bmax = pad64(nsmax * per);
  DevBuf<int> d_t0(h);
  DevBuf<cplx> proj(h);
  LaphContractWS ws(h);
  SWCHK(upload(h, &d_t0.p, (const int*)t0, (size_t)nsrc));
  SWCHK(dev_realloc(h, &proj.p, (size_t)L * per * bmax));
  SWCHK(laph_contract_ws(h, ws, nsmax, bmax));
  for (int s0 = 0; s0 < nsrc; s0 += spb) {
    const int ns = std::min(spb, nsrc - s0), nvalid = ns * per, ncols = pad64(nvalid);
    SWCHK(stream_sync(h));
    HIPCHK(hipMemset(proj.p, 0, sizeof(cplx) * L * per * ncols));
    SWCHK(laph_copy_tau(h, (cplx*)tau + (size_t)s0 * L * per * per, 0, nvalid, ncols, proj, false));
    SWCHK(laph_contract(h, proj, d_t0.p + s0, ns, ncols, ws, (cplx*)T + (size_t)s0 * nmom * 16 * L,
                        (cplx*)loops + (size_t)s0 * nmom * 4));
  }
  return 0;
}

// ---- distillation: two-meson correlators from the perambulators ---------------------------
// The operators of one side of a two-meson call: the folded spin matrices and momentum indices as the kernels take
// them, and the number of non-zero spin entries (the work counted).
struct LaphMesonSide {
  swk::LaphMesonOps ops;
  int n = 0, nnz[SW_MAX_MESON_OPS] = {0, 0, 0, 0};
};
static int laph_meson_side(sw_engine* h, const char* what, int n, const double* spin, const int32_t* mom,
                           LaphMesonSide& side) {
  if (n < 1 || n > SW_MAX_MESON_OPS) return sw_fail(h, "%d %s operators outside [1,%d]", n, what, SW_MAX_MESON_OPS);
  if (!spin || !mom) return sw_fail(h, "null %s operators", what);
  const int nmom = (int)h->lh_momenta.size();
  std::memset(&side.ops, 0, sizeof(side.ops));
  side.n = n;
  for (int k = 0; k < n; ++k) {
    if (mom[k] < 0 || mom[k] >= nmom)
      return sw_fail(h, "%s operator %d: momentum index %d outside the %d registered", what, k, (int)mom[k], nmom);
    side.ops.mom[k] = mom[k];
    side.nnz[k] = 0;
    for (int e = 0; e < 4; ++e) {
      side.ops.w[k][2 * e] = spin[8 * k + 2 * e];
      side.ops.w[k][2 * e + 1] = spin[8 * k + 2 * e + 1];
      if (spin[8 * k + 2 * e] != 0.0 || spin[8 * k + 2 * e + 1] != 0.0) side.nnz[k]++;
    }
  }
  return 0;
}

// The tiling of the sandwich: RT = ceil(2 nev / 16) row tiles, the column tiles in `halves` passes of NT
static inline void laph_sandwich_tiles(int nev, int* RT, int* halves, int* NT) {
  *RT = (2 * nev + 15) / 16;
  *halves = (*RT + 7) / 8;
  *NT = (*RT + *halves - 1) / *halves;
}

// The workspace of one block: W [L][2][nev][ncols], Qt [nk][ns][L][P][P], R [nk][nkp][ns][L][P][P] (P = 2 ld), the
// results C1 [ns][nk][nkp][L] and C2 [ns][nk][nk][nkp][nkp][L] and, when the sandwich is asked for, Q dense
// [ns][nk][L][2 nev][2 nev]; sized for the largest block of the call.
struct LaphTwoMesonWS {
  DevBuf<cplx> W, Qt, R, C1, C2, Q;
  explicit LaphTwoMesonWS(sw_engine* h) : W(h), Qt(h), R(h), C1(h), C2(h), Q(h) {}
};
static int laph_two_meson_ws(sw_engine* h, LaphTwoMesonWS& ws, int ns, int ncols, int nk, int nkp, bool want_Q) {
  const int L = h->hier[0].lv[0].L, nev = h->lh_nev, P = 2 * h->lh_ld;
  const size_t mat = (size_t)ns * L * P * P;
  SWCHK(dev_realloc(h, &ws.W.p, (size_t)L * 2 * nev * ncols));
  SWCHK(dev_realloc(h, &ws.Qt.p, (size_t)nk * mat));
  SWCHK(dev_realloc(h, &ws.R.p, (size_t)nk * nkp * mat));
  SWCHK(dev_realloc(h, &ws.C1.p, (size_t)ns * nk * nkp * L));
  SWCHK(dev_realloc(h, &ws.C2.p, (size_t)ns * nk * nk * nkp * nkp * L));
  if (want_Q) SWCHK(dev_realloc(h, &ws.Q.p, (size_t)ns * nk * L * 4 * nev * nev));
  return 0;
}
// C1 [ns][nk][nkp][L] and C2 [ns][nk][nk][nkp][nkp][L] (and Q, or NULL) of the ns sources d_t0 whose columns are the
// first 2 nev ns of the projection block proj [L][2][nev][ncols], into the host arrays: per sink operator k_laph_sink
// -> k_laph_sandwich, then k_laph_source, k_laph_trace1 and k_laph_trace2 once each (2 nk + 3 launches of class
// SW_KCLASS_LAPH_TWO_MESON, one more for Q), then the small copies.
static int laph_two_meson(sw_engine* h, const cplx* proj, const int* d_t0, int ns, int ncols, const LaphMesonSide& snk,
                          const LaphMesonSide& src, LaphTwoMesonWS& ws, cplx* C1, cplx* C2, cplx* Q) {
  const int L = h->hier[0].lv[0].L, nev = h->lh_nev, ld = h->lh_ld, P = 2 * ld, per = 2 * nev;
  const int nk = snk.n, nkp = src.n, K4 = (nev + 3) / 4 * 4, K4p = (per + 3) / 4 * 4;
  int RT, halves, NTq;
  laph_sandwich_tiles(nev, &RT, &halves, &NTq);
  const int groups = (RT + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK;
  const int mgroups = (ld / 16 + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK;
  const size_t mat = (size_t)ns * L * P * P;
  const cplx* Mt = h->lh_M;
  if (h->profiling) {
    double w = 0.0;
    for (int k = 0; k < nk; ++k)
      w += (double)snk.nnz[k] * L * ld * ncols * K4 + (double)L * ns * (16.0 * RT) * (16.0 * NTq * halves) * K4p;
    for (int kp = 0; kp < nkp; ++kp) w += (double)nk * src.nnz[kp] * L * ns * (16.0 * RT) * ld * K4;
    w += (double)nk * nkp * L * ns * 5.0 * nev * nev + (double)nk * nk * nkp * nkp * L * ns * (double)per * per;
    h->twork[T_LAPH_2M] += 8.0 * w;
  }
  for (int k = 0; k < nk; ++k) {
    SWCHK(launch(h, T_LAPH_2M, swk::k_laph_sink<4>, dim3(L, 2, mgroups * (ncols / 64)), dim3(SW_BLOCK), proj, nev,
                 ncols, Mt, ld, snk.ops, k, ws.W.p));
    SWCHK(pick<1, 2, 3, 4, 5, 6, 7, 8>(NTq, [&](auto NT) {
      return launch(h, T_LAPH_2M, swk::k_laph_sandwich<decltype(NT)::value>, dim3(L, ns, groups * halves),
                    dim3(SW_BLOCK), (const cplx*)ws.W.p, proj, nev, ncols, halves, P, ws.Qt.p + k * mat);
    }));
  }
  SWCHK(pick<1, 2, 3, 4, 5, 6, 7, 8>(ld / 16, [&](auto NT) {
    return launch(h, T_LAPH_2M, swk::k_laph_source<decltype(NT)::value>, dim3(L, 2 * ns, nk * nkp * groups),
                  dim3(SW_BLOCK), (const cplx*)ws.Qt.p, nev, P, Mt, ld, d_t0, ns, nkp, src.ops, groups, ws.R.p);
  }));
  SWCHK(launch(h, T_LAPH_2M, swk::k_laph_trace1, dim3(nk * nkp, L, ns), dim3(SW_BLOCK), (const cplx*)ws.Qt.p, nev, P,
               Mt, ld, d_t0, nkp, src.ops, ws.C1.p));
  SWCHK(launch(h, T_LAPH_2M, swk::k_laph_trace2, dim3(nk * nk * nkp * nkp, L, ns), dim3(SW_BLOCK),
               (const cplx*)ws.R.p, nev, P, nk, nkp, ws.C2.p));
  if (Q)
    SWCHK(launch(h, T_LAPH_2M, swk::k_laph_sandwich_unpack, dim3((per * per + SW_BLOCK - 1) / SW_BLOCK, L, nk * ns),
                 dim3(SW_BLOCK), (const cplx*)ws.Qt.p, nev, P, nk, ws.Q.p));
  SWCHK(stream_sync(h));
  HIPCHK(hipMemcpy(C1, ws.C1.p, sizeof(cplx) * ns * nk * nkp * L, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(C2, ws.C2.p, sizeof(cplx) * ns * nk * nk * nkp * nkp * L, hipMemcpyDeviceToHost));
  if (Q) HIPCHK(hipMemcpy(Q, ws.Q.p, sizeof(cplx) * ns * nk * L * per * per, hipMemcpyDeviceToHost));
  return 0;
}

// The two-meson building blocks of nsrc source timeslices, solved, projected and contracted on the device: per block
// of whole sources laph_block (as sw_perambulators on that chunk) and laph_two_meson.  Stateless: no mode buffer, no
// probe slot and no registration is touched; everything but the two-point workspace lives for this call only.
int sw_distilled_two_meson(sw_engine* h, int nsrc, const int32_t* t0, int nk, const double* sink_spin,
                           const int32_t* sink_mom, int nkp, const double* source_spin, const int32_t* source_mom,
                           double tol, int maxiter, double* C1, double* C2, int32_t* iters) {
  SWCHK(check_hier(h, 0, 0, true));
  SWCHK(distillation_ready(h));
  SWCHK(laph_momenta_ready(h));
  SWCHK(check_source_timeslices(h, nsrc, t0));
  LaphMesonSide snk, src;
  SWCHK(laph_meson_side(h, "sink", nk, sink_spin, sink_mom, snk));
  SWCHK(laph_meson_side(h, "source", nkp, source_spin, source_mom, src));
  if (maxiter < 1) return sw_fail(h, "maxiter must be >= 1");
  if (!C1 || !C2) return sw_fail(h, "null output");
  int hid;
  SWCHK(solve_hier(h, 0, &hid));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int L = lv.L, nev = h->lh_nev, per = 2 * nev;
  const int spb = laph_sources_per_block(nev), nsmax = std::min(spb, nsrc), bmax = pad64(nsmax * per);
  const size_t c1 = (size_t)nk * nkp * L, c2 = (size_t)nk * nk * nkp * nkp * L;
  DevBuf<int> d_t0(h);
  DevBuf<cplx> proj(h);
  LaphTwoMesonWS ws(h);
  SWCHK(upload(h, &d_t0.p, (const int*)t0, (size_t)nsrc));
  SWCHK(ensure_two_point_ws(h, (size_t)lv.n * bmax));
  SWCHK(dev_realloc(h, &proj.p, (size_t)L * per * bmax));
  SWCHK(laph_two_meson_ws(h, ws, nsmax, bmax, nk, nkp, false));
  for (int s0 = 0; s0 < nsrc; s0 += spb) {
    const int ns = std::min(spb, nsrc - s0), nvalid = ns * per, ncols = pad64(nvalid);
    SWCHK(laph_block(h, hid, lv, d_t0.p + s0, 0, nvalid, ncols, tol, maxiter, proj,
                     iters ? iters + (size_t)s0 * per : nullptr));
    SWCHK(laph_two_meson(h, proj, d_t0.p + s0, ns, ncols, snk, src, ws, (cplx*)C1 + s0 * c1, (cplx*)C2 + s0 * c2,
                         nullptr));
  }
  return 0;
}

// The contraction alone on host perambulators tau [nsrc][L][2][nev][nev][2] (the layout of sw_perambulators), in the
// blocks of sw_distilled_two_meson; the pad columns of a block are zeros.  Q (or NULL): the sandwich, dense.
int sw_apply_laph_two_meson(sw_engine* h, int nsrc, const int32_t* t0, const double* tau, int nk,
                            const double* sink_spin, const int32_t* sink_mom, int nkp, const double* source_spin,
                            const int32_t* source_mom, double* C1, double* C2, double* Q) {
  SWCHK(check_hier(h, 0, 0, false));
  SWCHK(distillation_ready(h));
  SWCHK(laph_momenta_ready(h));
  SWCHK(check_source_timeslices(h, nsrc, t0));
  LaphMesonSide snk, src;
  SWCHK(laph_meson_side(h, "sink", nk, sink_spin, sink_mom, snk));
  SWCHK(laph_meson_side(h, "source", nkp, source_spin, source_mom, src));
  if (!tau || !C1 || !C2) return sw_fail(h, "null argument");
  HIPCHK(hipSetDevice(h->device));
  const int L = h->hier[0].lv[0].L, nev = h->lh_nev, per = 2 * nev;
  const int spb = laph_sources_per_block(nev), nsmax = std::min(spb, nsrc), bmax = pad64(nsmax * per);
  const size_t c1 = (size_t)nk * nkp * L, c2 = (size_t)nk * nk * nkp * nkp * L, q = (size_t)nk * L * per * per;
  DevBuf<int> d_t0(h);
  DevBuf<cplx> proj(h);
  LaphTwoMesonWS ws(h);
  SWCHK(upload(h, &d_t0.p, (const int*)t0, (size_t)nsrc));
  SWCHK(dev_realloc(h, &proj.p, (size_t)L * per * bmax));
  SWCHK(laph_two_meson_ws(h, ws, nsmax, bmax, nk, nkp, Q != nullptr));
  for (int s0 = 0; s0 < nsrc; s0 += spb) {
    const int ns = std::min(spb, nsrc - s0), nvalid = ns * per, ncols = pad64(nvalid);
    SWCHK(stream_sync(h));
    HIPCHK(hipMemset(proj.p, 0, sizeof(cplx) * L * per * ncols));
    SWCHK(laph_copy_tau(h, (cplx*)tau + (size_t)s0 * L * per * per, 0, nvalid, ncols, proj, false));
    SWCHK(laph_two_meson(h, proj, d_t0.p + s0, ns, ncols, snk, src, ws, (cplx*)C1 + s0 * c1, (cplx*)C2 + s0 * c2,
                         Q ? (cplx*)Q + s0 * q : nullptr));
  }
  return 0;
}

// ---- distillation: generalized perambulators, the distilled three-point functions ---------
// What a k_laph_generalized call needs besides the fields: the insertion timeslices and momenta with their tables on
// the device, for this call only.
struct LaphGenTables {
  DevBuf<int> tins, mom, sr;
  DevBuf<cplx> phase;
  int nt = 0, nmom = 0, jz = -1;
  explicit LaphGenTables(sw_engine* h) : tins(h), mom(h), sr(h), phase(h) {}
};
// the argument checks both entry points share; nothing is allocated or launched here
static int laph_generalized_args(sw_engine* h, int nt, const int32_t* tins, int nmom, const int32_t* q) {
  Level& lv = h->hier[0].lv[0];
  if (nmom < 1 || nmom > SW_MAX_MOMENTA)
    return sw_fail(h, "%d momenta: between 1 and %d per call", nmom, SW_MAX_MOMENTA);
  SWCHK(check_momenta(h, "generalized perambulators", nmom, q));
  if (!lv.U1 || !lv.U2)
    return sw_fail(h, "generalized perambulators need a lattice level 0 with links (sw_set_lattice)");
  const int L = lv.L;
  if (nt < 1 || nt > L) return sw_fail(h, "%d insertion timeslices outside [1,%d]", nt, L);
  if (!tins) return sw_fail(h, "null insertion timeslice list");
  std::vector<char> seen(L, 0);
  for (int i = 0; i < nt; ++i) {
    if (tins[i] < 0 || tins[i] >= L) return sw_fail(h, "insertion timeslice %d outside [0,%d)", (int)tins[i], L);
    if (seen[tins[i]]) return sw_fail(h, "insertion timeslice %d listed twice", (int)tins[i]);
    seen[tins[i]] = 1;
  }
  return 0;
}
static int laph_generalized_tables(sw_engine* h, LaphGenTables& tb, int nt, const int32_t* tins, int nmom,
                                   const int32_t* q) {
  SWCHK(upload(h, &tb.tins.p, (const int*)tins, (size_t)nt));
  SWCHK(upload_slice_tables(h, nmom, q, &tb.mom.p, &tb.phase.p, &tb.sr.p));
  tb.nt = nt;
  tb.nmom = nmom;
  tb.jz = -1;
  for (int j = 0; j < nmom; ++j)
    if (q[j] == 0) tb.jz = j;
  return 0;
}
// column tiles of 16 per wave and column groups of a launch over nb0 source columns: at most 8 tiles per wave
static inline void laph_generalized_tiles(int nb0, int* NT, int* ncg) {
  const int ct = (nb0 + 15) / 16;
  *ncg = (ct + 7) / 8;
  *NT = (ct + *ncg - 1) / *ncg;
}
// bytes of G per insertion timeslice, and the timeslices of one chunk of the scoped device buffer (at most 256 MB)
static inline size_t laph_generalized_chunk(int nt, int nmom, int nbf, int nb0) {
  const size_t per_t = (size_t)nmom * 6 * nbf * nb0 * sizeof(cplx);
  return std::min<size_t>((size_t)nt, std::max<size_t>(1, ((size_t)256 << 20) / per_t));
}
// G [nt][nmom][6][nbf][nb0] on the host from the columns [cf, cf + nbf) of Zf [n][ldf] and [c0, c0 + nb0) of Z0
// [n][ld0]: per chunk of timeslices k_laph_generalized (the table-free instantiation for a momentum 0, the phased one
// over the others) into the buffer `g`, then one copy.
static int laph_generalized(sw_engine* h, Level& lv, const LaphGenTables& tb, const cplx* Zf, int ldf, int cf, int nbf,
                            const cplx* Z0, int ld0, int c0, int nb0, DevBuf<cplx>& g, cplx* out) {
  const int L = lv.L, M = tb.nmom, jz = tb.jz, nz = M - (jz >= 0 ? 1 : 0);
  int NTv, ncg;
  laph_generalized_tiles(nb0, &NTv, &ncg);
  const int rgs = (nbf + 63) / 64, Lp = (L + 3) / 4 * 4;
  const size_t per_t = (size_t)M * 6 * nbf * nb0, chunk = laph_generalized_chunk(tb.nt, M, nbf, nb0);
  SWCHK(dev_realloc(h, &g.p, per_t * chunk));
  for (size_t t0 = 0; t0 < (size_t)tb.nt; t0 += chunk) {
    const int ntc = (int)std::min(chunk, (size_t)tb.nt - t0);
    // eight complex products per timeslice and momentum, over the tiles the launch issues
    if (h->profiling)
      h->twork[T_LAPH_GEN] += 8.0 * 8.0 * (double)ntc * M * Lp * (16.0 * ((nbf + 15) / 16)) * (16.0 * NTv * ncg);
    SWCHK(pick<1, 2, 3, 4, 5, 6, 7, 8>(NTv, [&](auto NT) {
      if (jz >= 0)
        SWCHK(launch(h, T_LAPH_GEN, swk::k_laph_generalized<false, decltype(NT)::value>,
                     dim3(6 * ntc, 1, rgs * ncg), dim3(SW_BLOCK), Zf, ldf, cf, nbf, Z0, ld0, c0, nb0,
                     (const int*)tb.sr.p, (const cplx*)tb.phase.p, (const int*)tb.mom.p,
                     (const int*)tb.tins.p + t0, (const cplx*)lv.U1, (const cplx*)lv.U2, jz, M, L, ncg, g.p));
      if (nz > 0)
        SWCHK(launch(h, T_LAPH_GEN, swk::k_laph_generalized<true, decltype(NT)::value>,
                     dim3(6 * ntc, nz, rgs * ncg), dim3(SW_BLOCK), Zf, ldf, cf, nbf, Z0, ld0, c0, nb0,
                     (const int*)tb.sr.p, (const cplx*)tb.phase.p, (const int*)tb.mom.p,
                     (const int*)tb.tins.p + t0, (const cplx*)lv.U1, (const cplx*)lv.U2, jz, M, L, ncg, g.p));
      return 0;
    }));
    SWCHK(stream_sync(h));
    HIPCHK(hipMemcpy(out + t0 * per_t, g.p, sizeof(cplx) * per_t * ntc, hipMemcpyDeviceToHost));
  }
  return 0;
}

// k_laph_generalized alone on host fields Zf [nbf][n], Z0 [nb0][n] (reference ordering): out complex128
// [nt][nmom][6][nbf][nb0].  Needs a lattice level 0 with links (the condition of sw_set_three_point), no distillation.
int sw_apply_laph_generalized(sw_engine* h, int nbf, const double* Zf, int nb0, const double* Z0, int nt,
                              const int32_t* tins, int nmom, const int32_t* q, double* out) {
  SWCHK(check_hier(h, 0, 0, false));
  SWCHK(laph_generalized_args(h, nt, tins, nmom, q));
  if (nbf < 1 || nbf > 256 || nb0 < 1 || nb0 > 256)
    return sw_fail(h, "%d x %d columns outside [1,256]", nbf, nb0);
  if (!Zf || !Z0 || !out) return sw_fail(h, "null argument");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int ldf = pad64(nbf), ld0 = pad64(nb0);
  LaphGenTables tb(h);
  DevBuf<cplx> zf(h), z0(h), g(h);
  SWCHK(laph_generalized_tables(h, tb, nt, tins, nmom, q));
  SWCHK(dev_realloc(h, &zf.p, (size_t)lv.n * ldf));
  SWCHK(dev_realloc(h, &z0.p, (size_t)lv.n * ld0));
  SWCHK(pack_host(h, lv, nbf, Zf, zf, ldf));
  SWCHK(stream_sync(h));   // the stage is free for the second block
  SWCHK(pack_host(h, lv, nb0, Z0, z0, ld0));
  return laph_generalized(h, lv, tb, zf, ldf, 0, nbf, z0, ld0, 0, nb0, g, (cplx*)out);
}

// The generalized perambulators between the source timeslice t0 and the sink timeslice tf:
//   G [nt][nmom][6][2 nev][2 nev], row (m, e) = the solution of eigenvector m, spin e on tf, column (n, b) on t0,
// from the solve blocks sw_perambulators(h, 2, {t0, tf}) makes (tau [2][L][2][nev][nev][2] and iters [2][nev][2],
// either may be NULL, are what it returns, bit for bit).  One block (4 nev <= 256): the kernel reads both column
// ranges from the solution block in the two-point workspace.  Two blocks: the columns of the first are copied into
// scoped buffers before the second solve.  Stateless: no mode buffer, no probe slot and no registration is touched.
int sw_generalized_perambulators(sw_engine* h, int t0, int tf, int nt, const int32_t* tins, int nmom, const int32_t* q,
                                 double tol, int maxiter, double* G, double* tau, int32_t* iters) {
  SWCHK(check_hier(h, 0, 0, true));
  SWCHK(distillation_ready(h));
  SWCHK(laph_generalized_args(h, nt, tins, nmom, q));
  const int32_t ends[2] = {t0, tf};
  SWCHK(check_source_timeslices(h, 2, ends));
  if (maxiter < 1) return sw_fail(h, "maxiter must be >= 1");
  if (!G) return sw_fail(h, "null output");
  int hid;
  SWCHK(solve_hier(h, 0, &hid));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int n = lv.n, L = lv.L, nev = h->lh_nev, per = 2 * nev, total = 2 * per;
  const int bmax = std::min(256, pad64(total)), ldz = pad64(per);
  const size_t rows = (size_t)L * 2 * nev;
  LaphGenTables tb(h);
  DevBuf<int> d_t0(h);
  DevBuf<cplx> proj(h), z0(h), zf(h), g(h);
  SWCHK(upload(h, &d_t0.p, (const int*)ends, (size_t)2));
  SWCHK(laph_generalized_tables(h, tb, nt, tins, nmom, q));
  SWCHK(ensure_two_point_ws(h, (size_t)n * bmax));
  SWCHK(dev_realloc(h, &proj.p, rows * bmax));
  const bool split = total > 256;
  if (split) {
    SWCHK(dev_realloc(h, &z0.p, (size_t)n * ldz));
    SWCHK(dev_realloc(h, &zf.p, (size_t)n * ldz));   // the pad columns beyond 2 nev are never read
  }
  for (int c0 = 0; c0 < total; c0 += 256) {
    const int nvalid = std::min(256, total - c0), ncols = pad64(nvalid);
    SWCHK(laph_block(h, hid, lv, d_t0, c0, nvalid, ncols, tol, maxiter, proj, iters ? iters + c0 : nullptr));
    if (split) {
      // global columns [c0, c0 + nvalid): those below `per` belong to t0, the others to tf
      const int n0 = std::max(0, std::min(c0 + nvalid, per) - c0), nf = nvalid - n0;
      if (n0 > 0)
        HIPCHK(hipMemcpy2DAsync(z0.p + c0, sizeof(cplx) * ldz, h->tp_z, sizeof(cplx) * ncols, sizeof(cplx) * n0, n,
                                hipMemcpyDeviceToDevice, h->stream));
      if (nf > 0)
        HIPCHK(hipMemcpy2DAsync(zf.p + (c0 + n0 - per), sizeof(cplx) * ldz, h->tp_z + n0, sizeof(cplx) * ncols,
                                sizeof(cplx) * nf, n, hipMemcpyDeviceToDevice, h->stream));
    }
    SWCHK(stream_sync(h));
    if (tau) SWCHK(laph_copy_tau(h, (cplx*)tau, c0, nvalid, ncols, proj, true));
  }
  if (split) return laph_generalized(h, lv, tb, zf, ldz, 0, per, z0, ldz, 0, per, g, (cplx*)G);
  return laph_generalized(h, lv, tb, h->tp_z, bmax, per, per, h->tp_z, bmax, 0, per, g, (cplx*)G);
}

// ---- three-point functions: sequential one-end-trick solves and a local or point-split insertion ---------
// (g3 Gf g3)^H for Gf = 1, g3, s1, s2 as k_seq_sources takes it: bit 0 = the rows select the other spin, bits 1-2 /
// 3-4 = the entry of row 0 / row 1 as a power of i:  1, diag(1,-1), -s1, -s2 = [[0, i], [-i, 0]]
static const int kSeqGammaCode[4] = {0, 2 << 3, 1 | (2 << 1) | (2 << 3), 1 | (1 << 1) | (3 << 3)};

int sw_set_three_point(sw_engine* h, int t0, int tf, int sink_gamma, int pf, int nmom, const int32_t* q) {
  SWCHK(check_hier(h, 0, 0, false));
  if (nmom < 0 || nmom > SW_MAX_MOMENTA)
    return sw_fail(h, "%d momenta: at most %d per registration", nmom, SW_MAX_MOMENTA);
  h->r_t3.drop();
  if (nmom == 0) {
    h->t3_momenta.clear();
    return 0;
  }
  SWCHK(check_momenta(h, "three-point functions", nmom, q));
  Level& lv = h->hier[0].lv[0];
  const int L = lv.L;
  if (!lv.U1 || !lv.U2) return sw_fail(h, "three-point functions need a lattice level 0 with links (sw_set_lattice)");
  if (t0 < 0 || t0 >= L) return sw_fail(h, "source timeslice %d outside [0,%d)", t0, L);
  if (tf < 0 || tf >= L) return sw_fail(h, "sink timeslice %d outside [0,%d)", tf, L);
  if (tf == t0) return sw_fail(h, "sink timeslice %d equals the source timeslice", tf);
  if (pf < 0 || pf >= L) return sw_fail(h, "sink momentum %d outside [0,%d)", pf, L);
  if (sink_gamma < 0 || sink_gamma > 3) return sw_fail(h, "unknown sink spin matrix code %d (0..3 = 1, g3, s1, s2)", sink_gamma);
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  SWCHK(upload_slice_tables(h, nmom, q, &h->t3_mom, &h->t3_phase, &h->t3_slicerow));
  const std::vector<int> zero(SW_MAX_MOMENTA, 0);
  SWCHK(upload(h, &h->t3_mom0, zero.data(), zero.size()));
  h->t3_momenta.assign(q, q + nmom);
  h->t3_t0 = t0;
  h->t3_tf = tf;
  h->t3_gamma = sink_gamma;
  h->t3_pf = pf;
  h->t3_jz = -1;
  for (int j = 0; j < nmom; ++j)
    if (q[j] == 0) h->t3_jz = j;
  return 0;
}

// what SW_MODE_THREE_POINT and its stateless entries need: a registration on a lattice level 0 with links
static int three_point_ready(sw_engine* h) {
  if (h->t3_momenta.empty()) return sw_fail(h, "no three-point registration (sw_set_three_point)");
  Level& lv = h->hier[0].lv[0];
  if (!lv.stencil || !lv.U1 || !lv.U2)
    return sw_fail(h, "three-point functions need a lattice level 0 with links (sw_set_lattice)");
  return 0;
}

// the three blocks [n][2 nq] of a three-point batch: sources (either stage), z, zeta
static int ensure_three_point_ws(sw_engine* h, size_t cnt) {
  if (h->t3_ws_cap >= cnt && h->t3_rhs) return 0;
  SWCHK(dev_realloc(h, &h->t3_rhs, cnt));
  SWCHK(dev_realloc(h, &h->t3_z, cnt));
  SWCHK(dev_realloc(h, &h->t3_zeta, cnt));
  h->t3_ws_cap = cnt;
  return 0;
}

// S = the sequential sources of Z [n][2 nq] through the registered sink; total (optional) = c_k of Z
static int seq_sources(sw_engine* h, Level& lv, const cplx* Z, int nb, int nq, cplx* S, cplx* total) {
  SWCHK(launch(h, T_3PT_SOURCES, swk::k_seq_sources, dim3((lv.n + 15) / 16, 2 * nq / 64), dim3(SW_BLOCK), Z, nb, lv.n,
               (const int*)lv.rowmap, (const int*)h->t3_slicerow, (const cplx*)h->t3_phase, lv.L, h->t3_tf, h->t3_pf,
               kSeqGammaCode[h->t3_gamma], nq, S));
  if (!total) return 0;
  return launch(h, T_3PT_SOURCES, swk::k_pair_slice_total, dim3(nq / 64), dim3(SW_BLOCK), Z,
                (const int*)h->t3_slicerow, lv.L, h->t3_tf, nq, total);
}

// r_t3[d][j][a][b][f][c][t][k] from Zeta and Z [n][2 nq]: the table-free instantiation for a registered momentum
// 0, the phased one over the others
static int seq_dots(sw_engine* h, Level& lv, const cplx* Zeta, const cplx* Z, int nq) {
  const int M = (int)h->t3_momenta.size(), L = lv.L, jz = h->t3_jz;
  SWCHK(result_begin(h, h->r_t3, (size_t)5 * M * 16 * L, nq));
  cplx* est = h->r_t3.p;
  if (jz >= 0)
    SWCHK(launch(h, T_3PT_DOTS, swk::k_slice_seq_dots<false>, dim3(L, nq / 64, 5), dim3(SW_BLOCK), Zeta, Z,
                 (const int*)h->t3_slicerow, (const cplx*)h->t3_phase, (const int*)h->t3_mom, (const cplx*)lv.U1,
                 (const cplx*)lv.U2, jz, 1, M, L, nq, est));
  const int nz = M - (jz >= 0 ? 1 : 0);
  if (nz > 0)
    SWCHK(launch(h, T_3PT_DOTS, swk::k_slice_seq_dots<true>, dim3(L, nq / 64, 5 * nz), dim3(SW_BLOCK), Zeta, Z,
                 (const int*)h->t3_slicerow, (const cplx*)h->t3_phase, (const int*)h->t3_mom, (const cplx*)lv.U1,
                 (const cplx*)lv.U2, jz, nz, M, L, nq, est));
  return 0;
}

// host vectors [2][nb][n] (reference ordering) <-> a block [n][2 nq]
static int pack_pair(sw_engine* h, Level& lv, int nb, int nq, const double* X, cplx* dst) {
  const size_t per = (size_t)nb * lv.n;
  SWCHK(ensure_stage(h, per * 2 * sizeof(cplx)));
  HIPCHK(hipMemcpyAsync(h->stage, X, per * 2 * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
  for (int g = 0; g < 2; ++g)
    SWCHK(launch(h, T_OTHER, swk::k_pack_c, dim3((lv.n + 63) / 64, nq / 64), dim3(SW_BLOCK),
                 (const cplx*)h->stage + (size_t)g * per, nb, lv.n, (const int*)lv.rowmap, dst + (size_t)g * nq,
                 2 * nq));
  return stream_sync(h);   // the stage is free for the next block
}

static int three_point_args(sw_engine* h, int nb, const void* a, const void* b, const void* out) {
  SWCHK(check_hier(h, 0, 0, false));
  SWCHK(three_point_ready(h));
  if (nb <= 0 || !a || !b || !out) return sw_fail(h, "bad arguments");
  return 0;
}

// k_seq_sources alone on host solutions Z[a][k][n] (reference ordering): out[a][k][n] = s_k^a.
int sw_apply_seq_sources(sw_engine* h, int nb, const double* Z, double* out) {
  SWCHK(three_point_args(h, nb, Z, Z, out));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int nq = pad64(nb);
  SWCHK(ensure_three_point_ws(h, (size_t)lv.n * 2 * nq));
  SWCHK(pack_pair(h, lv, nb, nq, Z, h->t3_z));
  SWCHK(seq_sources(h, lv, h->t3_z, nb, nq, h->t3_rhs, nullptr));
  const size_t per = (size_t)nb * lv.n;
  for (int g = 0; g < 2; ++g)
    SWCHK(launch(h, T_OTHER, swk::k_unpack_c, dim3((lv.n + 63) / 64, nq / 64), dim3(SW_BLOCK),
                 (const cplx*)(h->t3_rhs + (size_t)g * nq), 2 * nq, lv.n, (const int*)lv.rowmap,
                 (cplx*)h->stage + (size_t)g * per, nb));
  HIPCHK(hipMemcpyAsync(out, h->stage, per * 2 * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
  return stream_sync(h);
}

// k_slice_seq_dots alone on host fields Zeta, Z [a][k][n] (reference ordering): out[d][j][a][b][f][c][t][k].
int sw_apply_seq_dots(sw_engine* h, int nb, const double* Zeta, const double* Z, double* out) {
  SWCHK(three_point_args(h, nb, Zeta, Z, out));
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[0].lv[0];
  const int nq = pad64(nb);
  SWCHK(ensure_three_point_ws(h, (size_t)lv.n * 2 * nq));
  SWCHK(pack_pair(h, lv, nb, nq, Zeta, h->t3_zeta));
  SWCHK(pack_pair(h, lv, nb, nq, Z, h->t3_z));
  SWCHK(seq_dots(h, lv, h->t3_zeta, h->t3_z, nq));
  SWCHK(stream_sync(h));
  return result_fetch(h, h->r_t3, nb, out);
}

int sw_hutch_fetch_three_point(sw_engine* h, double* out) {
  return fetch_result(h, &sw_engine::r_t3, "no three-point batch to fetch", out);
}

// ---- probe batches: one skeleton (sw_hutch_run), one body per mode -------------------
// What sw_hutch_run has settled before a body runs: the probes of `level` are selected (nb of them, padded to nbp
// columns), the probe workspace is sized, and hid is the hierarchy that solves `level` (solve_hier; lcoarse: the
// coarse level of a difference mode).
struct Batch {
  int mode, level, hid, lcoarse, nb, nbp;
  double tol;
  int maxiter;
};

// x0 <- the int8 probes, engine row order
static int pack_probes(sw_engine* h, const Batch& b) {
  Level& lv = h->hier[0].lv[b.level];
  return launch(h, T_OTHER, swk::k_pack_i8, dim3((lv.n + 63) / 64, b.nbp / 64), dim3(SW_BLOCK), h->pb_probes, b.nb,
                lv.n, (const int*)lv.rowmap, h->pb_x0, b.nbp);
}

// The fine solve of a level-0 probe block: pb_z = A^-1 rhs with rhs = x0 - U U^H x0 for the registered U (none:
// x0 itself, not copied); gather: the rows of rhs through perm_src[0], Pperm^T (utils.py:221-233).  *total = the
// solve's iteration total.
static int fine_solve(sw_engine* h, const Batch& b, bool gather, int* total) {
  const int n = h->hier[0].lv[0].n, nbp = b.nbp;
  const int* src = gather ? (const int*)h->perm_src[0] : nullptr;
  const cplx* rhs = h->pb_x0;
  if (h->kd > 0) {
    SWCHK(deflate(h, h->U, h->kd, src, h->pb_x0, h->pb_rhs, n, nbp));
    rhs = h->pb_rhs;
  } else if (gather) {
    dim3 grid((n + SW_WAVES_PER_BLOCK - 1) / SW_WAVES_PER_BLOCK, nbp / 64);
    SWCHK(launch(h, T_DEFL, swk::k_gather_rows, grid, dim3(SW_BLOCK), src, h->pb_x0, h->pb_rhs, n, nbp));
    rhs = h->pb_rhs;
  }
  return solve_dev(h, b.hid, 0, rhs, h->pb_z, b.tol, b.maxiter, nbp, total);
}

// sum[k] += the largest iteration count among the G columns of probe k (column g nbp + k) of the level-0 solve that
// just drained
static int fold_iters(sw_engine* h, const Batch& b, int total, int G, std::vector<int32_t>& sum) {
  std::vector<int32_t> all;
  SWCHK(record_iters(h, &h->hier[b.hid].lv[0].sws, total, all, G * b.nbp));
  for (int k = 0; k < b.nb; ++k) {
    int32_t most = 0;
    for (int g = 0; g < G; ++g) most = std::max(most, all[(size_t)g * b.nbp + k]);
    sum[k] += most;
  }
  return 0;
}

// The end of a level-0 batch: drain the stream, mark the mode's results fetchable, iteration counts of the last
// solve (G columns per probe) on top of `sum` (the earlier stages; empty: none), no coarse solves.
static int batch_tail(sw_engine* h, const Batch& b, int total, int G, std::initializer_list<ResultBuf*> results,
                      std::vector<int32_t> sum = {}) {
  SWCHK(stream_sync(h));
  for (ResultBuf* r : results) r->done(b.nb);
  sum.resize(b.nb, 0);
  SWCHK(fold_iters(h, b, total, G, sum));
  h->last_iters_f = sum;
  h->last_iters_c.assign(b.nb, 0);
  return 0;
}

// e = x^H A^-1 Pperm^T (x - U U^H x)       utils.py:221-249
static int body_hutchinson(sw_engine* h, const Batch& b) {
  int total = 0;
  SWCHK(pack_probes(h, b));
  SWCHK(fine_solve(h, b, true, &total));
  SWCHK(dot_into(h, h->pb_x0, h->pb_z, h->hier[0].lv[0].n, b.nbp, h->pb_est));
  return batch_tail(h, b, total, 1, {});
}

// z = A^-1 (x - U U^H x) once, then e_j = (D_{s_j}^T x)^H z for every registered shift; U as registered (the
// caller's W = gamma_3 V sgn(lambda) without Pperm), no perm_src gather; pb_est = the first shift's estimates
static int body_shifts(sw_engine* h, const Batch& b) {
  int total = 0;
  SWCHK(pack_probes(h, b));
  SWCHK(fine_solve(h, b, false, &total));
  SWCHK(shift_dots(h, h->hier[0].lv[0], h->pb_probes, b.nb, h->pb_z, b.nbp));
  HIPCHK(hipMemcpyAsync(h->pb_est, h->r_shifts.p, sizeof(cplx) * b.nbp, hipMemcpyDeviceToDevice, h->stream));
  return batch_tail(h, b, total, 1, {&h->r_shifts});
}

// z exactly as SW_MODE_HUTCHINSON_SHIFTS, then the reduction that stops at the timeslice and keeps the spin
// components apart; pb_est = the scalar total of the first momentum.  SW_MODE_HUTCHINSON_LINK_LOOPS: the same (its
// local loops land in mode 5's buffer, bit for bit), then the four link branches of the same z and the same codes
// into the buffer of its own
static int body_loops(sw_engine* h, const Batch& b) {
  Level& lv = h->hier[0].lv[0];
  int total = 0;
  SWCHK(pack_probes(h, b));
  SWCHK(fine_solve(h, b, false, &total));
  SWCHK(slice_dots(h, lv, h->pb_probes, b.nb, h->pb_z, b.nbp, h->pb_est, h->r_loops));
  if (b.mode != SW_MODE_HUTCHINSON_LINK_LOOPS) return batch_tail(h, b, total, 1, {&h->r_loops});
  SWCHK(slice_link_dots(h, lv, nullptr, b.nb, h->pb_z, b.nbp));
  return batch_tail(h, b, total, 1, {&h->r_loops, &h->r_links});
}

// The 2 M sources of every noise straight from the int8 probes, one solve over all 2 M nq columns (no deflation),
// then the reduction that is bilinear in two solution columns; pb_est = the pion total at p = 0.
// SW_MODE_TWO_POINT_LMA: R = T(z, z) - T(z_L, z_L), z_L = A_L^-1 eta = g_a U G (U^H eta) written over the sources, in
// a buffer of the mode's own (mode 6's last batch stays fetchable); pb_est = the pion total of R.  Iterations of a
// noise = the largest count among its 2 M columns.
static int body_two_point(sw_engine* h, const Batch& b) {
  Level& lv = h->hier[0].lv[0];
  const int n = lv.n, nb = b.nb, nbp = b.nbp;
  const int G = 2 * (int)h->tp_momenta.size(), ncols = G * nbp;
  SWCHK(ensure_two_point_ws(h, (size_t)n * ncols));
  SWCHK(slice_sources(h, lv, h->pb_probes, nb, nbp, h->tp_rhs));
  int total = 0;
  SWCHK(solve_dev(h, b.hid, 0, h->tp_rhs, h->tp_z, b.tol, b.maxiter, ncols, &total));
  if (b.mode == SW_MODE_TWO_POINT) {
    SWCHK(pair_dots(h, lv, h->tp_z, nbp, h->r_tp, h->pb_est));
    return batch_tail(h, b, total, G, {&h->r_tp});
  }
  SWCHK(pair_dots(h, lv, h->tp_z, nbp, h->r_lma, nullptr));
  SWCHK(low_mode_apply(h, h->tp_rhs, n, ncols, nbp, h->tp_rhs));
  SWCHK(pair_dots(h, lv, h->tp_rhs, nbp, h->lma_tmp, nullptr));
  const size_t cnt = h->r_lma.rows * nbp;
  SWCHK(launch(h, T_TP_DOTS, swk::k_sub_inplace, dim3((unsigned)std::min<size_t>(2048, (cnt + 255) / 256)), dim3(256),
               h->r_lma.p, (const cplx*)h->lma_tmp.p, cnt));
  SWCHK(launch(h, T_TP_DOTS, swk::k_pair_total, dim3(nbp / 64), dim3(SW_BLOCK), (const cplx*)h->r_lma.p, h->tp_j0,
               lv.L, nbp, h->pb_est));
  return batch_tail(h, b, total, G, {&h->r_lma});
}

// SW_MODE_TWO_POINT_SMEARED: mode 6 with the sources smeared on their timeslice after the phase, and the solution
// block smeared in place, on every timeslice, from one registered sink level to the next (the increments add up:
// S_a S_b = S_{a+b}); the pair sums of level i land in slab i of the mode's buffer.  pb_est = the pion total of
// slab 0, real and positive at any level.  The fused kernel where L has one, else the one-step chain with the
// source block as its second buffer (the solve is over: the sources are no longer needed).
static int body_two_point_smeared(sw_engine* h, const Batch& b) {
  Level& lv = h->hier[0].lv[0];
  const int n = lv.n, nb = b.nb, nbp = b.nbp, L = lv.L;
  const int M = (int)h->tp_momenta.size(), G = 2 * M, ncols = G * nbp, nsink = (int)h->sm_sink.size();
  const bool fused = smear_has_fused(L);
  SWCHK(ensure_two_point_ws(h, (size_t)n * ncols));
  SWCHK(slice_sources(h, lv, h->pb_probes, nb, nbp, h->tp_rhs));
  SWCHK(smear(h, lv, h->tp_rhs, h->tp_z, ncols, h->tp_t0, 1, h->sm_source, fused));
  int total = 0;
  SWCHK(solve_dev(h, b.hid, 0, h->tp_rhs, h->tp_z, b.tol, b.maxiter, ncols, &total));
  const size_t slab = (size_t)M * 16 * L;
  SWCHK(result_begin(h, h->r_tps, nsink * slab, nbp));
  int done = 0;
  for (int i = 0; i < nsink; ++i) {
    SWCHK(smear(h, lv, h->tp_z, h->tp_rhs, ncols, 0, L, h->sm_sink[i] - done, fused));
    done = h->sm_sink[i];
    SWCHK(pair_dots_into(h, lv, h->tp_z, nbp, h->r_tps.p + i * slab * nbp, nullptr));
  }
  SWCHK(launch(h, T_TP_DOTS, swk::k_pair_total, dim3(nbp / 64), dim3(SW_BLOCK), (const cplx*)h->r_tps.p, h->tp_j0, L,
               nbp, h->pb_est));
  return batch_tail(h, b, total, G, {&h->r_tps});
}

// Stage 1: the two spin sources of every noise at momentum 0 and their solutions z (no deflation); stage 2: the
// sequential sources through the sink, written over the stage-1 sources, and their solutions zeta to the same tol;
// then the field x field sums of zeta and z.  pb_est = c_k, the pion two-point value at the sink slice.  Iterations
// of a noise = the largest count among its two columns, stage 1 plus stage 2.
static int body_three_point(sw_engine* h, const Batch& b) {
  Level& lv = h->hier[0].lv[0];
  const int n = lv.n, nb = b.nb, nbp = b.nbp, ncols = 2 * nbp;
  SWCHK(ensure_three_point_ws(h, (size_t)n * ncols));
  h->r_t3.drop();
  SWCHK(launch(h, T_3PT_SOURCES, swk::k_slice_sources, dim3((n + 15) / 16, ncols / 64), dim3(SW_BLOCK),
               (const int8_t*)h->pb_probes, nb, n, (const int*)lv.rowmap, (const cplx*)h->t3_phase,
               (const int*)h->t3_mom0, lv.L, h->t3_t0, nbp, ncols, h->t3_rhs));
  int total = 0;
  std::vector<int32_t> stage1(nb, 0);
  SWCHK(solve_dev(h, b.hid, 0, h->t3_rhs, h->t3_z, b.tol, b.maxiter, ncols, &total));
  SWCHK(seq_sources(h, lv, h->t3_z, nb, nbp, h->t3_rhs, h->pb_est));
  SWCHK(stream_sync(h));
  SWCHK(fold_iters(h, b, total, 2, stage1));
  total = 0;
  SWCHK(solve_dev(h, b.hid, 0, h->t3_rhs, h->t3_zeta, b.tol, b.maxiter, ncols, &total));
  SWCHK(seq_dots(h, lv, h->t3_zeta, h->t3_z, nbp));
  return batch_tail(h, b, total, 2, {&h->r_t3}, stage1);
}

// e = x0^H A_l^-1 (Bblock_perm_l Pperm_l^T) x0: the plain Hutchinson estimator of one level's trace term
// (stochastic form of the coarsest-level term, stoch_trace.py:428-437)
static int body_level(sw_engine* h, const Batch& b) {
  const int level = b.level, nbp = b.nbp;
  SWCHK(pack_probes(h, b));
  const cplx* xdef = h->pb_x0;
  if (h->rhsmap[level].set) {
    SWCHK(launch_ell(h, h->rhsmap[level], 0, xdef, nullptr, h->pb_rhs, nbp, T_OTHER));
    xdef = h->pb_rhs;
  }
  int total = 0;
  SWCHK(solve_dev(h, b.hid, level, xdef, h->pb_z, b.tol, b.maxiter, nbp, &total));
  SWCHK(dot_into(h, h->pb_x0, h->pb_z, h->hier[0].lv[level].n, nbp, h->pb_est));
  SWCHK(record_level_iters(h, h->hier[b.hid], level, total, h->last_iters_f, b.nb));
  h->last_iters_c.assign(b.nb, 0);
  return 0;
}

// The MLMC difference of level `level` through diff_apply: e = x0^H (z - P y) (modes 1 / 2, utils.py:336-355), or the
// level loops S_q(Pi x, Pi (z - P y)) into the MLMC loop buffer (modes 7 - 10; 9 / 10 with the level's registered
// projection on the right-hand side, which modes 1 / 2 apply whenever it is registered)
static int body_mlmc(sw_engine* h, const Batch& b) {
  Hier& H0 = h->hier[0];
  const int level = b.level, nb = b.nb, nbp = b.nbp;
  Level& lv = H0.lv[level];
  const int n = lv.n;
  const bool mloops = b.mode != SW_MODE_MLMC && b.mode != SW_MODE_MLMC_SKIP;
  SWCHK(pack_probes(h, b));
  // x_def = Bblock_perm * Pperm^T * x0      utils.py:288-290
  const cplx* xdef = h->pb_x0;
  if (h->lkd[level] > 0) {
    // x_def = x0 - V V^H x0                 utils.py:260-266 (defl_type exact / inexact_01); the deflated level
    // loops solve and restrict x_def too, and keep the plain x0 (level 0: the int8 codes) as the left operand
    SWCHK(deflate(h, h->lV[level], h->lkd[level], nullptr, h->pb_x0, h->pb_xd, n, nbp));
    xdef = h->pb_xd;
  }
  if (h->rhsmap[level].set && !mloops) {   // the loops take the plain probe, as mode 5 ignores sw_set_perm
    SWCHK(launch_ell(h, h->rhsmap[level], 0, xdef, nullptr, h->pb_rhs, nbp, T_OTHER));
    xdef = h->pb_rhs;
  }
  // z = A_l^-1 x_def, y = the coarse solution on level + 1 (iteration counts recorded after each solve)
  const cplx* y;
  SWCHK(diff_apply(h, b.hid, level, b.lcoarse, xdef, nbp, h->pb_z, h->pb_xc, h->pb_y, b.tol, b.maxiter, nb, &y,
                   nullptr));
  if (mloops) {
    // d = z - P y on level `level`, one launch with the prolongation
    SWCHK(launch_ell(h, lv.P, 1, y, h->pb_z, h->pb_w, nbp, T_P));
    Level& lv0 = H0.lv[0];
    if (level == 0) {
      // the probe is the int8 codes themselves: mode 5's reduction on d, one pass
      SWCHK(slice_dots(h, lv0, h->pb_probes, nb, h->pb_w, nbp, h->pb_est, h->r_mloops));
    } else {
      // u = P_0 ... P_{level-1} x, v = P_0 ... P_{level-1} d on the lattice, then the reduction with a complex
      // left operand
      const cplx *u, *v;
      SWCHK(prolong_to_lattice(h, level, h->pb_x0, h->pb_xc, h->pb_xc2, nbp, &u));
      SWCHK(prolong_to_lattice(h, level, h->pb_w, h->pb_y, h->pb_w2, nbp, &v));
      SWCHK(slice_cdots(h, lv0, u, v, nbp, h->pb_est));
    }
    SWCHK(stream_sync(h));
    h->r_mloops.done(nb);
    return 0;
  }
  // w = P y, e = x0^H z - x0^H w            utils.py:336-355
  SWCHK(launch_ell(h, lv.P, 0, y, nullptr, h->pb_w, nbp, T_P));
  SWCHK(dot_into(h, h->pb_x0, h->pb_z, n, nbp, h->pb_est + nbp));
  SWCHK(dot_into(h, h->pb_x0, h->pb_w, n, nbp, h->pb_est + 2 * nbp));
  SWCHK(launch(h, T_OTHER, swk::k_est_combine, dim3((nbp + 255) / 256), dim3(256), (const cplx*)(h->pb_est + nbp),
               (const cplx*)(h->pb_est + 2 * nbp), nbp, h->pb_est));
  return stream_sync(h);
}

// The modes of sw_hutch_run, one row each.  level0: the mode runs at level 0 only, under this name in its refusal;
// diff: 1 = a difference mode (its coarse level has to exist), 2 = its level-skipping form (level 0 only); ready:
// what has to be registered (nullptr: nothing).  sw_hutch_run makes every refusal from this row before anything is
// allocated or launched.  A new mode: a row here, a body, and a ResultBuf if it leaves a resolved result.
struct ProbeMode {
  int mode;
  const char* level0;
  int diff;
  int (*ready)(sw_engine*, int level);
  int (*body)(sw_engine*, const Batch&);
};
static int momenta_ready(sw_engine* h, int) {
  if (h->momenta.empty()) return sw_fail(h, "no momenta registered (sw_set_loop_momenta)");
  return 0;
}
static int mlmc_loops_ready(sw_engine* h, int level) {
  SWCHK(momenta_ready(h, level));
  if (h->lkd[level] > 0)
    return sw_fail(h, "MLMC loops do not combine with MLMC-level deflation (level %d holds %d vectors)", level,
                   h->lkd[level]);
  return 0;
}
static int two_point_ready(sw_engine* h, int) {
  if (h->tp_momenta.empty()) return sw_fail(h, "no two-point registration (sw_set_two_point)");
  return 0;
}
static int two_point_lma_ready(sw_engine* h, int level) {
  SWCHK(two_point_ready(h, level));
  return low_mode_ready(h);
}
static int two_point_smeared_ready(sw_engine* h, int level) {
  SWCHK(two_point_ready(h, level));
  return smearing_ready(h);
}
static const ProbeMode kModes[] = {
    {SW_MODE_HUTCHINSON, "Hutchinson", 0, nullptr, body_hutchinson},
    {SW_MODE_MLMC, nullptr, 1, nullptr, body_mlmc},
    {SW_MODE_MLMC_SKIP, nullptr, 2, nullptr, body_mlmc},
    {SW_MODE_LEVEL, nullptr, 0, nullptr, body_level},
    {SW_MODE_HUTCHINSON_SHIFTS, "shifted Hutchinson", 0,
     [](sw_engine* h, int) { return h->shifts.empty() ? sw_fail(h, "no shifts registered (sw_set_shifts)") : 0; },
     body_shifts},
    {SW_MODE_HUTCHINSON_LOOPS, "timeslice-loop Hutchinson", 0, momenta_ready, body_loops},
    {SW_MODE_TWO_POINT, "two-point", 0, two_point_ready, body_two_point},
    {SW_MODE_MLMC_LOOPS, nullptr, 1, mlmc_loops_ready, body_mlmc},
    {SW_MODE_MLMC_LOOPS_SKIP, nullptr, 2, mlmc_loops_ready, body_mlmc},
    {SW_MODE_MLMC_DEFL_LOOPS, nullptr, 1, momenta_ready, body_mlmc},
    {SW_MODE_MLMC_DEFL_LOOPS_SKIP, nullptr, 2, momenta_ready, body_mlmc},
    {SW_MODE_TWO_POINT_LMA, "two-point", 0, two_point_lma_ready, body_two_point},
    {SW_MODE_HUTCHINSON_LINK_LOOPS, "link-loop Hutchinson", 0, [](sw_engine* h, int) { return link_loops_ready(h); },
     body_loops},
    {SW_MODE_THREE_POINT, "three-point", 0, [](sw_engine* h, int) { return three_point_ready(h); },
     body_three_point},
    {SW_MODE_TWO_POINT_SMEARED, "smeared two-point", 0, two_point_smeared_ready, body_two_point_smeared},
};

int sw_hutch_run(sw_engine* h, int mode, int level, double tol, int maxiter) {
  SWCHK(check_hier(h, 0, level, true));
  if (h->pb_level != level || h->pb_nb <= 0) return sw_fail(h, "no probes uploaded for level %d", level);
  if (maxiter < 1) return sw_fail(h, "maxiter must be >= 1");
  const ProbeMode* m =
      std::find_if(std::begin(kModes), std::end(kModes), [&](const ProbeMode& q) { return q.mode == mode; });
  if (m == std::end(kModes)) return sw_fail(h, "unknown mode %d", mode);
  if (m->level0 && level != 0) return sw_fail(h, "%s mode runs at level 0", m->level0);
  if (m->ready) SWCHK(m->ready(h, level));
  Batch b{mode, level, 0, level, h->pb_nb, h->pb_nbp, tol, maxiter};
  SWCHK(solve_hier(h, level, &b.hid));
  if (m->diff == 2 && level != 0) return sw_fail(h, "level skipping is defined for level 0 only");
  if (m->diff) SWCHK(diff_levels(h, level, m->diff == 2, &b.hid, &b.lcoarse));
  HIPCHK(hipSetDevice(h->device));
  SWCHK(ensure_probe_ws(h, b.nbp));
  SWCHK(ensure_small(h, b.nbp));
  if (h->pb_slot >= 0 && h->pb_slot < (int)h->slots.size() && h->slots[h->pb_slot].pending) {
    // the slot was (or is being) generated on the generation stream
    HIPCHK(hipStreamWaitEvent(h->stream, h->slots[h->pb_slot].ready, 0));
    h->slots[h->pb_slot].pending = false;
  }
  return m->body(h, b);
}


// ---- the one collective of the path: trace-sum / variance statistics over the ranks (RCCL over xGMI)
namespace {
struct RcclUid {
  char internal[128];
};
struct Rccl {
  void* lib = nullptr;
  int (*get_uid)(RcclUid*) = nullptr;
  int (*init_rank)(void**, int, RcclUid, int) = nullptr;
  int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*destroy)(void*) = nullptr;
  bool tried = false, ok = false;
};
Rccl g_rccl;
bool load_rccl() {
  if (g_rccl.tried) return g_rccl.ok;
  g_rccl.tried = true;
  // A process that runs torch.distributed with backend nccl already has RCCL mapped (PyTorch's bundled
  // copy); a second copy of a ROCm library in one process is what broke rocBLAS handle creation earlier
  // (two HIP runtimes' worth of static state), so: the mapped one first (RTLD_NOLOAD), by the names it
  // goes by, and only then a fresh load.
  for (const char* nm : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
    g_rccl.lib = dlopen(nm, RTLD_NOW | RTLD_NOLOAD);
    if (g_rccl.lib) break;
  }
  if (!g_rccl.lib && dlsym(RTLD_DEFAULT, "ncclCommInitRank")) g_rccl.lib = dlopen(nullptr, RTLD_NOW);
  if (!g_rccl.lib) g_rccl.lib = dlopen("librccl.so", RTLD_NOW);
  if (!g_rccl.lib) g_rccl.lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW);
  if (!g_rccl.lib) return false;
  g_rccl.get_uid = (int (*)(RcclUid*))dlsym(g_rccl.lib, "ncclGetUniqueId");
  g_rccl.init_rank = (int (*)(void**, int, RcclUid, int))dlsym(g_rccl.lib, "ncclCommInitRank");
  g_rccl.all_reduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(
      g_rccl.lib, "ncclAllReduce");
  g_rccl.destroy = (int (*)(void*))dlsym(g_rccl.lib, "ncclCommDestroy");
  g_rccl.ok = g_rccl.get_uid && g_rccl.init_rank && g_rccl.all_reduce && g_rccl.destroy;
  if (g_rccl.ok) g_rccl_destroy = g_rccl.destroy;
  return g_rccl.ok;
}
}  // namespace

int sw_comm_unique_id(char id[128]) {
  if (!id || !load_rccl()) return 1;
  RcclUid u;
  if (g_rccl.get_uid(&u) != 0) return 1;
  std::memcpy(id, u.internal, 128);
  return 0;
}

int sw_comm_init(sw_engine* h, int nranks, int rank, const char id[128]) {
  if (!h) return 1;
  if (!id || nranks < 1 || rank < 0 || rank >= nranks) return sw_fail(h, "bad arguments");
  if (!load_rccl()) return sw_fail(h, "RCCL could not be loaded (%s)", dlerror());
  HIPCHK(hipSetDevice(h->device));
  if (h->comm) {
    g_rccl.destroy(h->comm);
    h->comm = nullptr;
  }
  RcclUid u;
  std::memcpy(u.internal, id, 128);
  void* c = nullptr;
  const int rc = g_rccl.init_rank(&c, nranks, u, rank);
  if (rc != 0 || !c) return sw_fail(h, "ncclCommInitRank failed (status %d)", rc);
  h->comm = c;
  if (!h->d_stats) SWCHK(dev_realloc(h, &h->d_stats, (size_t)4));
  return 0;
}

int sw_allreduce_stats(sw_engine* h, double stats[4]) {
  if (!h) return 1;
  if (!stats) return sw_fail(h, "null statistics");
  if (!h->comm) return sw_fail(h, "no communicator (sw_comm_init)");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(h->d_stats, stats, 4 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const int rc = g_rccl.all_reduce(h->d_stats, h->d_stats, 4, /*ncclFloat64*/ 8, /*ncclSum*/ 0,
                                   h->comm, h->stream);
  if (rc != 0) return sw_fail(h, "ncclAllReduce failed (status %d)", rc);
  HIPCHK(hipMemcpyAsync(stats, h->d_stats, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int sw_comm_destroy(sw_engine* h) {
  if (!h) return 1;
  if (h->comm && g_rccl.ok) g_rccl.destroy(h->comm);
  h->comm = nullptr;
  return 0;
}

int sw_sync(sw_engine* h) {
  if (!h) return 1;
  HIPCHK(hipSetDevice(h->device));
  if (h->gen_stream) HIPCHK(hipStreamSynchronize(h->gen_stream));
  return stream_sync(h);
}

int sw_hutch_fetch(sw_engine* h, double* ests, int32_t* iters) {
  if (!h) return 1;
  if (h->pb_nb <= 0 || !h->pb_est) return sw_fail(h, "nothing to fetch");
  HIPCHK(hipSetDevice(h->device));
  SWCHK(stream_sync(h));
  const int nb = h->pb_nb;
  if (ests) HIPCHK(hipMemcpy(ests, h->pb_est, sizeof(cplx) * nb, hipMemcpyDeviceToHost));
  if (iters) {
    for (int j = 0; j < nb; ++j) {
      iters[j] = j < (int)h->last_iters_f.size() ? h->last_iters_f[j] : 0;
      iters[nb + j] = j < (int)h->last_iters_c.size() ? h->last_iters_c[j] : 0;
    }
  }
  return 0;
}

int sw_hutch_batch(sw_engine* h, int mode, int level, int nb, const int8_t* probes, double tol,
                   int maxiter, double* ests, int32_t* iters) {
  SWCHK(sw_probes_upload(h, level, nb, probes));
  SWCHK(sw_hutch_run(h, mode, level, tol, maxiter));
  return sw_hutch_fetch(h, ests, iters);
}

// ---- measurement -----------------------------------------------------------------------
int sw_bench_dirac(sw_engine* h, int hid, int level, int nb, int reps, double* ms_per_apply) {
  SWCHK(check_hier(h, hid, level, true));
  if (nb <= 0 || reps <= 0 || !ms_per_apply) return sw_fail(h, "bad arguments");
  HIPCHK(hipSetDevice(h->device));
  Level& lv = h->hier[hid].lv[level];
  const int nbp = pad64(nb);
  cplx *a, *b;
  SWCHK(io_vectors(h, lv, nbp, &a, &b));
  // deterministic non-trivial input: +-1 pattern
  {
    std::vector<std::complex<double>> hx((size_t)lv.n * nbp);
    uint32_t s = 12345u;
    for (auto& v : hx) {
      s = s * 1664525u + 1013904223u;
      const double re = ((s >> 16) & 0xffff) / 65536.0 - 0.5;
      s = s * 1664525u + 1013904223u;
      const double im = ((s >> 16) & 0xffff) / 65536.0 - 0.5;
      v = std::complex<double>(re, im);
    }
    HIPCHK(hipMemcpy(a, hx.data(), hx.size() * sizeof(cplx), hipMemcpyHostToDevice));
  }
  const bool prof = h->profiling;
  h->profiling = false;
  const int bm = h->bench_mode;
  const int what = h->bench_what;
  Hier& H = h->hier[hid];
  if ((what == 1 || what == 2) && level + 1 >= H.nlevels) return sw_fail(h, "no transfer at this level");
  if (what == 1 || what == 2) SWCHK(ensure_level_ws(h, H.lv[level + 1], nbp));
  if (what == 3) SWCHK(ensure_level_ws(h, H.lv[H.nlevels - 1], nbp));
  cplx* c = lv.r;   // third buffer: the right-hand side of modes 1 / 2
  if (bm != 0) HIPCHK(hipMemcpy(c, a, (size_t)lv.n * nbp * sizeof(cplx), hipMemcpyDeviceToDevice));
  const cplx wgt = cplx{0.31, 0.07};
  auto one = [&](int i) -> int {
    if (what == 1) return launch_ell(h, lv.R, 0, a, nullptr, H.lv[level + 1].b, nbp, T_R);
    if (what == 2) return launch_ell(h, lv.P, 0, H.lv[level + 1].b, nullptr, b, nbp, T_P);
    if (what == 3) {
      Level& ll = H.lv[H.nlevels - 1];
      return apply_coarsest(h, H, (i & 1) ? ll.x : ll.b, (i & 1) ? ll.b : ll.x, nbp);
    }
    return apply_op(h, lv, bm, (i & 1) ? b : a, bm ? c : nullptr, (i & 1) ? a : b, nbp, wgt);
  };
  for (int i = 0; i < 3; ++i) SWCHK(one(i));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipEventRecord(e0, h->stream));
  for (int i = 0; i < reps; ++i) SWCHK(one(i));
  HIPCHK(hipEventRecord(e1, h->stream));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  h->profiling = prof;
  *ms_per_apply = (double)ms / reps;
  return 0;
}

int sw_set_profiling(sw_engine* h, int on) {
  if (!h) return 1;
  if (h->gen_stream) HIPCHK(hipStreamSynchronize(h->gen_stream));
  SWCHK(stream_sync(h));
  h->profiling = on != 0;
  return 0;
}
int sw_timers(sw_engine* h, double t[8]) {
  if (!h || !t) return 1;
  SWCHK(stream_sync(h));
  for (int i = 0; i < 8; ++i) t[i] = h->tacc[i];
  t[T_MVM] += h->tacc[T_STENCIL] + h->tacc[T_STENCIL_RES] + h->tacc[T_STENCIL_SM] + h->tacc[T_MFMA_OP] +
              h->tacc[T_MFMA_OP2] + h->tacc[T_SCHUR] + h->tacc[T_SCHUR_OP];
  t[T_COARSEST] += h->tacc[T_MFMA_DENSE];
  t[T_OTHER] += h->tacc[T_TP_SOURCES] + h->tacc[T_3PT_SOURCES] + h->tacc[T_SMEAR] + h->tacc[T_LAPH_SRC];
  t[T_DOTS] += h->tacc[T_TP_DOTS] + h->tacc[T_SLICE_CDOTS] + h->tacc[T_MESON_FIELD] + h->tacc[T_LM_CONTRACT] +
               h->tacc[T_LINK_DOTS] + h->tacc[T_3PT_DOTS] + h->tacc[T_LAPH] + h->tacc[T_LAPH_CONTRACT] +
               h->tacc[T_LAPH_GEN] + h->tacc[T_LAPH_2M];
  return 0;
}
int sw_timers_reset(sw_engine* h) {
  if (!h) return 1;
  SWCHK(stream_sync(h));
  for (int i = 0; i < T_NCAT; ++i) {
    h->tacc[i] = 0.0;
    h->tcount[i] = 0;
    h->twork[i] = 0.0;
  }
  h->launches = 0;
  return 0;
}
int sw_kernel_stats(sw_engine* h, int which, double* total_ms, int64_t* launches) {
  if (!h || !total_ms || !launches) return 1;
  if (which < 0 || which >= T_NCAT || which == T_LAPH_SRC) return sw_fail(h, "kernel class %d out of range", which);
  SWCHK(stream_sync(h));
  *total_ms = h->tacc[which];
  *launches = h->tcount[which];
  if (which == T_LAPH) {
    *total_ms += h->tacc[T_LAPH_SRC];
    *launches += h->tcount[T_LAPH_SRC];
  }
  return 0;
}
int sw_kernel_work(sw_engine* h, int which, double* work) {
  if (!h || !work) return 1;
  if (which < 0 || which >= T_NCAT || which == T_LAPH_SRC) return sw_fail(h, "kernel class %d out of range", which);
  *work = h->twork[which];
  return 0;
}
int sw_launch_count(sw_engine* h, int64_t* n) {
  if (!h || !n) return 1;
  *n = h->launches;
  return 0;
}

}  // extern "C"
