/*
 * schwinger_hip.h -- C ABI of the MI355X (gfx950) deflated-MLMC Hutchinson trace engine.
 *
 * This is the drop-in boundary for the hot path of Gustavroot/DeflatedMLMC_Schwinger
 * (SURVEY.md section 8).  The reference has no native code: every arithmetic call on the
 * path goes through SciPy/NumPy/pyamg wheels.  Each entry point below names the
 * reference call site(s) (file:line under the reference repo) whose work it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; sw_last_error() gives text;
 *     no C++ exception crosses the boundary;
 *   - complex numbers are interleaved (re, im) doubles ("complex128"); `double*` arguments
 *     that hold complex data say so;
 *   - host vectors use the REFERENCE ordering and shape: `nb` right-hand sides, each a
 *     contiguous flat vector of length n (level 0: idx(s,x,y) = s*L*L + y*L + x);
 *   - all buffers are caller-owned host memory unless the name ends in _dev;
 *   - one host thread per handle; device streams are internal;
 *   - a handle holds up to SW_MAX_HIER multigrid hierarchies (`hid`): hid 0 is the
 *     reference hierarchy (the MLMC level operators of multigrid.py:100-345), hid 1 an
 *     optional solver-only hierarchy for level 0 (parity is on converged solves).
 */
#ifndef SCHWINGER_HIP_H
#define SCHWINGER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SW_MAX_HIER 2
#define SW_MAX_LEVELS 8
#define SW_MAX_KRYLOV 32
#define SW_MAX_DEFL 256
#define SW_MAX_SHIFTS 128
#define SW_MAX_MOMENTA 8
#define SW_MAX_SINK_LEVELS 4
#define SW_MAX_SMEARING_STEPS 1024
#define SW_MAX_LAPH 128
#define SW_MAX_MESON_OPS 4 /* sink operators, and source operators, of one sw_distilled_two_meson call */

typedef struct sw_engine sw_engine;

/* ---- lifetime ------------------------------------------------------------------------ */
/* Replaces MG.__init__ (multigrid.py:58-89).  Fails (non-zero) when no HIP device exists. */
int sw_create(sw_engine** out, int device_id);
int sw_destroy(sw_engine* h);
const char* sw_last_error(sw_engine* h);          /* h may be NULL: last create() error */
int sw_device_count(void);                         /* 0 when no GPU is visible            */
/* Device blocks of 32 MB and more that an engine frees (setup scratch, workspaces, everything at sw_destroy)
 * are parked in a process-wide pool and handed out again instead of going back to the driver (cap SW_POOL_GB,
 * default 128 GB; 0 disables; an allocation that fails with blocks parked releases them and retries):
 * sw_pool_trim() releases what is parked. */
int sw_pool_trim(void);
const char* sw_version(void);

/* ---- operands (products of MG.setup, multigrid.py:100-345, and matrix.py:14-31) ------ */
/* Start (or reset) hierarchy `hid` with `nlevels` levels. */
int sw_hier_begin(sw_engine* h, int hid, int nlevels);
/* Level-0 operator as the matrix-free U(1) Wilson stencil A = S + mass*I of SURVEY F2
 * (replaces the CSR built by matrix.py:21-29).  U1,U2: complex128[L*L], site index y*L+x.
 * Sets n_0 = 2*L*L and the even-odd internal layout. */
int sw_set_lattice(sw_engine* h, int hid, int L, double mass, const double* U1, const double* U2);
/* Level operator as CSR, complex128 data (multigrid.py:276-280 A_{l+1} = R A P; also
 * accepted for level 0 when no lattice is set). */
int sw_set_csr(sw_engine* h, int hid, int level, int n, const int64_t* indptr,
               const int32_t* indices, const double* data);
/* Prolongator P_l (n_f x n_c CSR, multigrid.py:262-264); R_l = P_l^H (multigrid.py:267-274). */
int sw_set_transfer(sw_engine* h, int hid, int level, int n_f, int n_c, const int64_t* indptr,
                    const int32_t* indices, const double* data);
/* Dense inverse of the coarsest operator, row-major complex128[n*n] (multigrid.py:342-344). */
int sw_set_coarsest_inv(sw_engine* h, int hid, int n, const double* dense);
/* Cycle shape at `level`: MR smoothing steps before/after the coarse correction and the
 * number of flexible-GMRES steps wrapped around the next-level cycle (0 = plain V-cycle).
 * Stands in for lgmres(maxiter=smooth_iters) at multigrid.py:393-394,438-439 (parity is on
 * converged solves). */
int sw_set_cycle(sw_engine* h, int hid, int level, int nu_pre, int nu_post, int kcycle);
/* Replace the adaptive MR steps at `level` by a fixed polynomial smoother: n_pre / n_post
 * Richardson steps x <- x + w_k (b - A x) with complex128 weights w_k (the inverse roots of a
 * GMRES residual polynomial computed at setup).  One fused kernel per step, no inner products.
 * n_pre = n_post = 0 returns to MR(nu) of sw_set_cycle. */
int sw_set_smoother(sw_engine* h, int hid, int level, int n_pre, const double* w_pre, int n_post,
                    const double* w_post);
/* Even-odd (Schur-complement) post-smoother for the stencil level: n_post Richardson steps
 * x_e <- x_e + w_k (b'_e - S x_e) on the even sites, S = D - H_eo H_oe / D, then the odd sites
 * exactly (x_o = (b_o + H_oe x_e) / D).  Half-vector traffic per step, operator four times better
 * conditioned; takes the place of the post-smoothing steps of sw_set_smoother on that level (no
 * pre-smoothing).  n_post = 0 switches back.  Same role as sw_set_smoother
 * (multigrid.py:438-439). */
int sw_set_eo_smoother(sw_engine* h, int hid, int level, int n_post, const double* w_post);
/* The same construction on a coarse (block) level, whose operator is a 5-point stencil of 16x16
 * blocks over the coarse sites: four operators that act on the even or odd sites only, in MFMA
 * block-row form -- which = 0: S = D_ee - A_eo D_oo^-1 A_oe (9-point), 1: F = A_eo D_oo^-1,
 * 2: G = D_oo^-1, 3: Hb = D_oo^-1 A_oe.  RT row tiles, KS k-steps per tile (multiple of 4),
 * tmap[RT] = tile (site) of the level vector each row tile writes, kcol[RT*KS] = first level row of
 * each 4-column group, vals[RT*KS*64] complex128 lane-packed as for the level operators.  With all
 * four set, sw_set_eo_smoother accepts the level.  Optional which = 4: the DENSE inverse of S over the even
 * sites' rows (every row tile lists all even sites' columns); with it the level is solved exactly --
 * x_e = S^-1 (b_e - F b_o), x_o = G b_o - Hb x_e -- instead of smoothed and the levels below it are not
 * visited (option "eo_direct"); it is dropped whenever one of the four operators is set again.
 * sw_get_level_bsr reads a (device-built) level operator back in that form (kcol = vals = NULL: only *KS). */
int sw_set_eo_operator(sw_engine* h, int hid, int level, int which, int RT, int KS, const int32_t* tmap,
                       const int32_t* kcol, const double* vals);
int sw_get_level_bsr(sw_engine* h, int hid, int level, int* KS, int32_t* kcol, double* vals);
/* The same four operators built ON THE DEVICE from the level's own block-row operator (as
 * sw_setup_galerkin leaves it: five site blocks per row, own site last; Lc x Lc sites, Lc even and >= 8):
 * batched 16x16 inverses of the odd sites' diagonal blocks and block products, no host algebra.
 * sw_apply_eo_operator applies one of them (which as above) to nb full-length level vectors in the
 * reference layout (rows it does not write come back zero) -- used to fit the smoother polynomial to S
 * and by the parity tests.  Build-only extension of the even-odd smoother above. */
int sw_setup_eo_operators(sw_engine* h, int hid, int level, int Lc);
int sw_apply_eo_operator(sw_engine* h, int hid, int level, int which, int nb, const double* X, double* Y);
/* Reference-faithful cycle at `level` ("function_iters / total_complexity in both
 * modes"): MG.one_mg_step exactly as multigrid.py:369-447 lays it out -- smooth, residual,
 * restrict, recurse, prolong, residual, smooth -- with `cycles` restart cycles of unpreconditioned
 * GMRES(m) from a zero guess as the smoother, the counterpart of
 * lgmres(A_l, r, tol=1e-20, maxiter=smooth_iters=2) with SciPy's inner_m = 30 (SURVEY F5;
 * LGMRES's single augmentation vector in the second cycle is not reproduced).  m = 0 switches back. */
int sw_set_gmres_smoother(sw_engine* h, int hid, int level, int m, int cycles);
/* ---- GPU-side setup of a hierarchy (device counterpart of multigrid.py:157-280) ----
 * The test vectors of a level stay in HBM.  Coarse levels built this way carry 16 dofs per coarse
 * site (8 test vectors x 2 chirality halves), i.e. one MFMA row tile per site.
 * sw_setup_testvectors: `sweeps` rounds of V <- A_level^-1 V by batched flexible GMRES to `tol`
 *   (precond = 0: unpreconditioned, for a hierarchy still under construction; 1: with the finished
 *   hierarchy's own cycle from `level` down).  seed != 0 starts from pseudo-random vectors, seed = 0
 *   from the vectors the level already holds (the restricted ones of the level above).
 *   iters_out[sweeps] receives the iteration counts.  Replaces eigs(A_l, k, sigma=0), multigrid.py:174.
 * sw_setup_transfer: per-(aggregate, half) orthonormalisation of the level's test vectors on the
 *   device (multigrid.py:232-259), P_level and R_level = P^H from it (multigrid.py:262-274), and
 *   the restricted test vectors as level+1's start.  blk_rows[nblocks*rpb]: level rows (engine row
 *   order) of each block; P's grouped-ELL structure comes from the caller's geometry: group size
 *   G, K columns per group pcols[ngroups*K], and pmap[ngroups*K*G] = index (block*rpb + member)*8 + k
 *   of the value, or -1; porder[ngroups] (may be NULL): order in which the kernel visits the row
 *   groups (groups that share coarse columns adjacent).
 * sw_setup_galerkin: A_{level+1} = R A P (multigrid.py:276-280) by 16-colour probing with the
 *   engine's own operator kernels, written straight into MFMA block-row form.  nbr[ncs*5]: the five
 *   sites of each coarse site's 5-point neighbourhood, pairwise distinct (the site itself last lets
 *   the smoother kernel keep its own X rows in registers).
 * sw_get_level_dense: a device-built level operator as a dense row-major complex128[n*n] (for the
 *   host inverse of the coarsest level, multigrid.py:342-344). */
int sw_setup_testvectors(sw_engine* h, int hid, int level, int nvec, uint64_t seed, int sweeps,
                         double tol, int maxiter, int precond, int32_t* iters_out);
int sw_setup_transfer(sw_engine* h, int hid, int level, int nblocks, int rpb, const int32_t* blk_rows,
                      int G, int K, const int32_t* pcols, const int64_t* pmap, const int32_t* porder);
int sw_setup_galerkin(sw_engine* h, int hid, int level, int Lc, const int32_t* nbr);
int sw_get_level_dense(sw_engine* h, int hid, int level, double* dense);
/* Dense inverse of a device-built coarsest operator without leaving the GPU: in-place Gauss-Jordan
 * with partial pivoting by the engine's own kernels (k_gj_*; n <= 8192), then packed into MFMA block-row
 * form as sw_set_coarsest_inv would (multigrid.py:342-344: np.linalg.inv).  Fails on a singular operator. */
int sw_setup_invert_coarsest(sw_engine* h, int hid);
/* The dense coarsest inverse the engine holds (handed over by sw_set_coarsest_inv or formed on the device by
 * sw_setup_invert_coarsest -- which also accepts a coarsest operator given as CSR, sw_set_csr) as a row-major
 * complex128[n*n] host array: the reference's mg_solver.coarsest_inv (multigrid.py:342-344) for callers that
 * read it (stoch_trace.py:428-435 traces it directly). */
int sw_get_coarsest_inv(sw_engine* h, int hid, double* dense);
/* The same one level up: the DENSE inverse of a block level's even-odd Schur complement (operator 0 of
 * sw_setup_eo_operators / sw_set_eo_operator; at most 8192 rows) formed on the device and installed as
 * that level's even-odd operator 4, with which the cycle solves the level exactly (option "eo_direct")
 * instead of smoothing it and visiting the levels below (multigrid.py:342-344,413-416 one level up). */
int sw_setup_direct_level(sw_engine* h, int hid, int level);
/* Dense inverse of a small level's OPERATOR (n <= 8192, multiple of 16), formed on the device and kept as the
 * level's direct solver (option "direct_small", default on): solves that START at this level -- the MLMC
 * coarse solves A_c^-1 R x of utils.py:306-329 on the reference hierarchy's small levels, the fine solves of
 * its coarse difference levels (utils.py:292) -- become x = A^-1 b, x += A^-1 (b - A x) on the matrix cores
 * instead of a multigrid-preconditioned FGMRES (multigrid.py:347-366); same solution to the solver tolerance,
 * iteration count reported as 1. */
int sw_setup_level_inverse(sw_engine* h, int hid, int level);
/* Arnoldi relation for the smoother polynomial, on the device: `degree` steps (classical Gram-Schmidt
 * twice) of the level operator (which = 0) or of its even-odd Schur complement (which = 1) from a
 * pseudo-random start vector; Hout receives the (degree+1) x degree Hessenberg matrix, row-major
 * complex128.  The host turns its harmonic Ritz values into the weights of sw_set_smoother /
 * sw_set_eo_smoother (the tuned stand-in for lgmres(maxiter=2), multigrid.py:393-394). */
int sw_setup_arnoldi(sw_engine* h, int hid, int level, int which, int degree, uint64_t seed, double* Hout);
/* ---- device eigensolver (SURVEY 8f-2 completed: the host ARPACK + SuperLU calls of the setup) -------------
 * Block subspace iteration with the engine's own batched solve as the shift-invert operator: replaces
 * eigs(A_l, k, sigma=0) (multigrid.py:174: test vectors) and eigsh(gamma_3 A, k, sigma=0) (utils.py:140:
 * deflation vectors).  The engine does the O(n) work on blocks of 64 vectors held in three device buffers
 * (index 0..2) on one finished (hid, level); the caller does the 64 x 64 dense algebra in between
 * (Rayleigh-Ritz on V^H Op^-1 V, Cholesky-QR), see setup_gpu.device_eigenpairs.
 *   sw_eig_begin   buffers on (hid, level), buffer 0 <- pseudo-random block
 *   sw_eig_begin_wide  the same with blocks of `width` vectors (a multiple of 64, at most 512): width/64
 *                  groups of 64 columns; load / fetch then take up to `width` columns, gram returns and
 *                  rotate takes width x width, solve and apply_diff act on every group (64 at a time)
 *   sw_eig_load    first ncols columns of buffer dst <- host vectors (reference order)
 *   sw_eig_solve   buf_dst = Op^-1 buf_src, 64 right-hand sides to `tol`; mode 0: Op = A_level, mode 1:
 *                  Op = gamma_3 A_level (gamma_3 = +1 / -1 on the first / second half of the reference order)
 *   sw_eig_apply_diff  buf_dst = (A_l^-1 - P A_c^-1 R) Gamma buf_src on all 64 columns, l = the level of
 *                  sw_eig_begin, which must be on hierarchy 0: the MLMC difference operator of the probe body
 *                  (SW_MODE_MLMC; skip = 1: A_0^-1 - P_0 P_1 A_2^-1 R_1 R_0 as SW_MODE_MLMC_SKIP, level 0 of
 *                  at least three levels only).  Gamma = gamma_3 (g3 = 1) or the identity (g3 = 0).  Both
 *                  solves run to `tol` with `maxiter`; *iters_max = the fine solve's iteration count.  Uses
 *                  the third buffer and two coarse blocks of the eigen state as scratch (not the probe state)
 *   sw_eig_gram    out[64*64] = buf_a^H buf_b (fp64 MFMA, deterministic two-stage sum)
 *   sw_eig_rotate  buf_dst = buf_src Y (sub < 0) or buf_sub - buf_src Y (the block residual W - V T), Y[64*64]
 *                  row-major, dst != src
 *   sw_eig_fetch   first k columns of buf_src as k host vectors in the reference order
 *   sw_eig_end     release the buffers */
int sw_eig_begin(sw_engine* h, int hid, int level, uint64_t seed);
int sw_eig_begin_wide(sw_engine* h, int hid, int level, uint64_t seed, int width);
int sw_eig_load(sw_engine* h, int dst, int ncols, const double* X);
int sw_eig_solve(sw_engine* h, int src, int dst, int mode, double tol, int maxiter, int32_t* iters_max);
int sw_eig_apply_diff(sw_engine* h, int src, int dst, int skip, int g3, double tol, int maxiter,
                      int32_t* iters_max);
int sw_eig_gram(sw_engine* h, int a, int b, double* out);
int sw_eig_rotate(sw_engine* h, int src, const double* Y, int dst, int sub);
int sw_eig_fetch(sw_engine* h, int src, int k, double* out);
int sw_eig_end(sw_engine* h);
/* Mark the hierarchy complete (allocates level workspaces lazily). */
int sw_hier_end(sw_engine* h, int hid);

/* Deflation vectors U (utils.py:145-155), row-major complex128[n0*k], reference ordering, k <= SW_MAX_DEFL. */
int sw_set_deflation(sw_engine* h, int k, const double* U);
/* Low-mode inverse G of the registered deflation vectors (build-only: low-mode averaged two-point functions), row-major
 * complex128[k*k]: the low-mode part of the propagator is A_L^-1 = U G U^H gamma_3, G meant to be (U^H gamma_3 A U)^-1
 * made Hermitian (any G keeps SW_MODE_TWO_POINT_LMA unbiased).  k must equal the registered deflation rank; k = 0
 * clears; every sw_set_deflation drops it. */
int sw_set_low_mode_inverse(sw_engine* h, int k, const double* G);
/* MLMC-level deflation vectors V_l of the difference operator at `level` of hid 0
 * (utils.py:141-157,260-266), row-major complex128[n_l*k]; k = 0 clears. */
int sw_set_level_deflation(sw_engine* h, int level, int k, const double* V);
/* Index shift of Pperm at `level` of hid 0 (multigrid.py:142-155,320-326). shift<0 clears. */
int sw_set_perm(sw_engine* h, int level, int64_t shift);
/* MLMC right-hand-side map C_i = Bblock_perm_i * Pperm_i^T as CSR (multigrid.py:328-331,
 * utils.py:288-290); n x n at `level` of hid 0. */
int sw_set_rhsmap(sw_engine* h, int level, int n, const int64_t* indptr, const int32_t* indices,
                  const double* data);
/* Flat-index shifts s_j of SW_MODE_HUTCHINSON_SHIFTS (build-only: displaced traces Tr(A^-1 D_s), (D_s v)[i] =
 * v[(i - s) mod n], at many displacements from one solve per probe).  Lattice level 0 only (sw_set_lattice);
 * every shift a multiple of 2L in [0, n), no duplicates, at most SW_MAX_SHIFTS; nshifts = 0 clears. */
int sw_set_shifts(sw_engine* h, int nshifts, const int64_t* shifts);
/* Spatial momenta p_j of SW_MODE_HUTCHINSON_LOOPS (build-only: timeslice loops, the phase of site x is
 * e^{-2 pi i p x / L}).  Lattice level 0 only (sw_set_lattice); every p in [0, L), no duplicates, at most
 * SW_MAX_MOMENTA; nmom = 0 clears. */
int sw_set_loop_momenta(sw_engine* h, int nmom, const int32_t* p);
/* Source timeslice t0 and spatial momenta p_j of SW_MODE_TWO_POINT (build-only: one-end-trick meson two-point
 * functions).  A registration of its own, independent of sw_set_loop_momenta; the same checks, plus 0 <= t0 < L
 * and 0 among the momenta (its solutions are the conjugated factor of every momentum); nmom = 0 clears. */
int sw_set_two_point(sw_engine* h, int t0, int nmom, const int32_t* p);
/* Gauge-covariant Jacobi (Wuppertal) smearing of SW_MODE_TWO_POINT_SMEARED (build-only): on every line (spin,
 * timeslice t), (H psi)(x) = U1(x,t) psi(x+1) + conj(U1(x-1,t)) psi(x-1) (x +- 1 mod L) and S_n =
 * [(1 + kappa H) / (1 + 2 kappa)]^n.  source_steps smear the sources on their timeslice (after the momentum phase);
 * sink_steps[nsink] are the sink levels, each applied to every timeslice of every solution (0 = a local sink).  A
 * registration of its own on a lattice level 0 with links (the condition of SW_MODE_HUTCHINSON_LINK_LOOPS): kappa > 0
 * and finite, 0 <= steps <= SW_MAX_SMEARING_STEPS, 1 <= nsink <= SW_MAX_SINK_LEVELS, the sink steps strictly
 * ascending; nsink = 0 clears. */
int sw_set_smearing(sw_engine* h, double kappa, int source_steps, int nsink, const int32_t* sink_steps);
/* Distillation (build-only): the nev eigenvectors of every timeslice's gauge-covariant spatial Laplacian 2 - H_t (H_t as
 * in sw_set_smearing) onto which sw_perambulators projects the quark fields, V complex128[L][nev][L] = v_m(x,t) at
 * [t][m][x].  A registration of its own on a lattice level 0 of hid 0 (the condition of sw_meson_fields);
 * 1 <= nev <= min(L, SW_MAX_LAPH); nev = 0 clears.  V is packed on the host into the kernels' layout (conjugated,
 * [t][x][m], padded with zeros to 4 sites and 16 vectors).  Orthonormality is NOT checked: V defines the operator. */
int sw_set_distillation(sw_engine* h, int nev, const double* V);
/* Source timeslice t0, sink timeslice tf, sink spin matrix (0..3 = 1, gamma_3, sigma_1, sigma_2), sink momentum pf
 * and insertion momenta q_j of SW_MODE_THREE_POINT (build-only: three-point functions from sequential one-end-trick
 * solves).  A registration of its own beside sw_set_two_point; the momentum checks of sw_set_loop_momenta (the list
 * need not contain 0), plus 0 <= t0, tf < L, tf != t0, 0 <= pf < L, a known matrix code and a lattice level 0 with
 * links (the condition of SW_MODE_HUTCHINSON_LINK_LOOPS); nmom = 0 clears. */
int sw_set_three_point(sw_engine* h, int t0, int tf, int sink_gamma, int pf, int nmom, const int32_t* q);
/* Outer flexible-GMRES restart length (<= SW_MAX_KRYLOV) and the hierarchy used to
 * precondition level-0 solves (0 or 1). */
int sw_set_solver(sw_engine* h, int restart, int solver_hid);

/* Engine switches (defaults are the measured-best settings; everything else exists for A/B runs,
 * profiles/ holds the measurements).  Unknown names and out-of-range values fail with a message.
 *   solver:        "eo_direct" (1) block levels that were given the dense inverse of their even-odd Schur
 *                  complement (sw_set_eo_operator, which = 4) are solved with it instead of smoothed;
 *                  "eo_solve" (1) outer solves of an even-odd smoothed lattice level on the even-odd
 *                  reduced system (half-length Krylov vectors; same stopping criterion, same results);
 *                  "precond_f32" (0) multigrid cycle in complex64 inside the fp64 FGMRES; "f32_krylov" (1)
 *                  with it, complex64 Krylov basis per restart cycle; "cgs2" (0) / "inner_cgs2" (0) second
 *                  Gram-Schmidt pass; "pyth_last" (1) last Arnoldi step of a restart cycle without its
 *                  orthogonalisation pass; "verify" (1) true-residual check of every outer solve;
 *                  "stop_factor" (1) outer solves iterate until every residual is below stop_factor * tol
 *                  (iteration counts are still reported at tol; 0.1 pins per-probe estimates to 1e-10
 *                  relative even where they cancel to small numbers); "fused_reduce" (1) inner products
 *                  completed inside the launch that forms their partial sums, FGMRES scalar updates
 *                  riding along; "gram_cycle" (1) restart cycles of the even-odd reduced outer solve and the
 *                  K-cycle's inner iteration in Gram-matrix form (directions without orthogonalisation, one
 *                  pass for all inner products, per-probe Cholesky solve); "lgmres_aug" (1) LGMRES
 *                  augmentation vector in the reference-faithful smoother's second cycle;
 *                  "lazy_sync" (1) convergence read-back only near the expected iteration count;
 *                  "dot_blocks" row blocks of the reducing BLAS-1 launches
 *   stencil level: "stencil_spw", "stencil_tile", "stencil_nt" (sites per wave, lattice tile width,
 *                  non-temporal stores); "p_even" (1) prolongation onto the even sites only ahead of an
 *                  even-odd smoother; "eo_skew" (-1) time-skewed strip order of the even-odd smoother's steps
 *                  on lattices beyond the Infinity Cache (-1 automatic, 0 off, > 0 strip height in rows; batches
 *                  too wide for admissible strips are walked 64-probe chunk by chunk, "eo_skew_chunk" (0)
 *                  forces that);
 *                  "eo_tile" (0) the fp64 even-odd launches of the lattice level that carry no b' operand (reduced
                  operator, product-form factors) from LDS-staged halo tiles in rotated coordinates, double-buffered
                  by LDS-DMA, one persistent workgroup of 4 or 8 waves per CU (k_schur_tile); bit-identical results;
                  "eo_product" (1) the even-odd smoother of the reduced-system cycle in product form,
 *                  x + beta prod_j (1 - u_j S)(b' - S x): the same polynomial as the steps
 *                  x <- x + w_k (b' - S x), 2 nu + 2 half-vector passes instead of 3 nu
 *   block levels:  "use_mfma" (1) fp64-MFMA block-row kernels vs grouped ELL; "mfma_3m" (1) three real
 *                  matrix products per complex one (k_bsr_mfma3) instead of four; "mfma3_tiles" (0: by size)
 *                  tiles of 16 probes per wave in that kernel; "mfma_ops", "mfma_tiles",
 *                  "mfma_small_tiles", "bsr_stages" / "dense_stages" (register pipeline depth), "bsr_nt",
 *                  "bsr_xreg", "bsr_sub", "dense_map", "ell_order"; complex64 twins "f32_tiles",
 *                  "f32_stages", "f32_dense_stages", "f32_splitk", "f32_pairs"
 *                  "dense_lds" (4) dense operators (coarsest inverse, dense Schur inverse of a directly solved
 *                  level, direct inverse of a small level) through k_dense_mfma3_lds: operands shared through LDS
 *                  (register-staged, double-buffered), 2 or 4 row tiles x 2 probe tiles per workgroup (0: k_bsr_mfma3)
 *   setup:         "gj_block" (32) panel width of the blocked Gauss-Jordan inverse (0: unblocked)
 *   deflation:     "defl_gemm" (0) 0: k_defl_dots / k_defl_apply up to 64 vectors, the fp64-MFMA pair
 *                  k_defl_gemm_dots / k_defl_gemm_apply above; 1: the MFMA pair at every rank
 *   sw_bench_dirac: "bench_mode" (0 Y=AX, 1 residual, 2 smoother step), "bench_what" (operator / R / P /
 *                  coarsest) */
int sw_set_option(sw_engine* h, const char* name, double value);
/* Current value of a switch (save / restore around A/B runs); also the read-only counter
 * "direct_fallbacks": solves on a directly solved level (sw_setup_level_inverse) whose measured residual stayed
 * above the tolerance after four refinement steps and that were handed to the iterative path instead. */
int sw_get_option(sw_engine* h, const char* name, double* value);

/* ---- building blocks (host buffers, reference ordering) -------------------------------- */
/* Y = A_level X.  Replaces MG.matvec (multigrid.py:552-557) and the residual SpMVs at
 * multigrid.py:388,402,433.  X,Y: complex128[nb*n]. */
int sw_apply_dirac(sw_engine* h, int hid, int level, int nb, const double* X, double* Y);
/* Y = R_level X (multigrid.py:406; utils.py:301-303) / Y = P_level X (multigrid.py:429;
 * utils.py:339-341). */
int sw_restrict(sw_engine* h, int hid, int level, int nb, const double* X, double* Y);
int sw_prolong(sw_engine* h, int hid, int level, int nb, const double* X, double* Y);
/* Y = coarsest_inv X (multigrid.py:413-416; utils.py:309-310,321-322). */
int sw_coarsest(sw_engine* h, int hid, int nb, const double* X, double* Y);
/* Y = the registered deflation projection of X with the kernels of sw_hutch_run.  which = 0: the
 * Hutchinson form Pperm_0^T (I - U U^H) X at level 0 (sw_set_deflation, sw_set_perm); which = 1: the MLMC
 * form (I - V_l V_l^H) X at `level` (sw_set_level_deflation).  X,Y: complex128[nb*n_level]. */
int sw_apply_deflation(sw_engine* h, int which, int level, int nb, const double* X, double* Y);
/* The shifted-dot kernel of SW_MODE_HUTCHINSON_SHIFTS alone: out[j*nb + k] = sum_i conj(x_k[(i + s_j) mod n])
 * Z_k[i] for the registered shifts; probes int8[nb*n] (codes +-1, +-2 = +-i), Z complex128[nb*n], out
 * complex128[nshifts*nb]. */
int sw_apply_shift_dots(sw_engine* h, int nb, const int8_t* probes, const double* Z, double* out);
/* The slice-dot kernel of SW_MODE_HUTCHINSON_LOOPS alone: out[p][a][b][t][k] = sum_x e^{-2 pi i p x / L}
 * conj(x_k[idx(a,x,t)]) Z_k[idx(b,x,t)] for the registered momenta, idx(s,x,y) = s L^2 + y L + x; probes
 * int8[nb*n] (codes +-1, +-2 = +-i), Z complex128[nb*n], out complex128[nmom*2*2*L*nb]. */
int sw_apply_slice_dots(sw_engine* h, int nb, const int8_t* probes, const double* Z, double* out);
/* The link-dot kernel of SW_MODE_HUTCHINSON_LINK_LOOPS alone: out[d][p][a][b][t][k], the four branches of that mode
 * with z_k = Z_k, for the registered momenta; probes int8[nb*n], Z complex128[nb*n], out complex128[4*nmom*2*2*L*nb].
 * The refusals of the mode. */
int sw_apply_slice_link_dots(sw_engine* h, int nb, const int8_t* probes, const double* Z, double* out);
/* The slice-dot kernel with a complex left operand (SW_MODE_MLMC_LOOPS on coarse levels, sw_coarsest_loops) alone:
 * out[p][a][b][t][k] = sum_x e^{-2 pi i p x / L} conj(U_k[idx(a,x,t)]) V_k[idx(b,x,t)] for the registered momenta;
 * U, V complex128[nb*n] of the lattice level, out complex128[nmom*2*2*L*nb]. */
int sw_apply_slice_cdots(sw_engine* h, int nb, const double* U, const double* V, double* out);
/* The exact coarsest term of the MLMC loops (build-only): out[p][a][b][t] = sum_j S_q(Pi e_j, Pi A_c^-1 e_j) over the
 * unit vectors e_j of the coarsest level of hid 0, Pi = P_0 ... P_{M-2}, S_q(u, v) = sum_x e^{-2 pi i p x / L}
 * conj(u[idx(a,x,t)]) v[idx(b,x,t)], for the registered momenta (sw_set_loop_momenta): 64-column blocks of the
 * identity and of the coarsest inverse prolonged to the lattice and reduced on the device, summed in a fixed
 * order (two calls agree bit for bit).  out complex128[nmom*2*2*L]. */
int sw_coarsest_loops(sw_engine* h, double* out);
/* The deflated part of a level's term of the MLMC loops (build-only): out[p][a][b][t] = sum_j S_q(Pi_l V_j, Pi_l D_l V_j)
 * over the vectors V_j registered at `level` of hid 0 (sw_set_level_deflation), D_l = A_l^-1 - P_l A_{l+1}^-1 R_l
 * (skip = 1, level 0 only: A_0^-1 - P_0 P_1 A_2^-1 R_1 R_0) applied on the device with solves to `tol`, for the
 * registered momenta (sw_set_loop_momenta).  With the SW_MODE_MLMC_DEFL_LOOPS expectation it adds up to the level's
 * term Tr(Pi_l^H Gamma_q Pi_l D_l) for any V, orthonormal or not.  64 columns per pass, summed in a fixed order (two
 * calls agree bit for bit).  Fails without momenta, without vectors at `level`, with skip at a level other than 0
 * and without a coarser level.  out complex128[nmom*2*2*L]. */
int sw_level_deflation_loops(sw_engine* h, int level, int skip, double tol, int maxiter, double* out);
/* The source kernel of SW_MODE_TWO_POINT alone: out[2 j + a][k][i] = the source eta_k^(j,a) of the registration
 * (sw_set_two_point) in the reference ordering, delta_{a,a'} delta_{t,t0} e^{+2 pi i p_j y / L} xi_k(y) at
 * i = idx(a',y,t), xi_k(y) = the code of probe k at idx(0,y,t0); probes int8[nb*n], out complex128[2*nmom*nb*n]. */
int sw_apply_slice_sources(sw_engine* h, int nb, const int8_t* probes, double* out);
/* The pair-dot kernels of SW_MODE_TWO_POINT alone on host solutions: Z complex128[2*nmom][nb][n] in the layout of
 * sw_apply_slice_sources' output, out complex128[nmom][2][2][2][2][L][nb], out[j][a][b][c][d][t][k] =
 * sum_x e^{-2 pi i p_j x / L} conj(Z[2 j0 + a][k][idx(c,x,t)]) Z[2 j + b][k][idx(d,x,t)], j0 = the registered
 * momentum 0. */
int sw_apply_pair_dots(sw_engine* h, int nb, const double* Z, double* out);
/* The smearing kernels alone on nb host vectors in the reference layout: Y = S_steps X with the registered kappa
 * (sw_set_smearing), on every timeslice.  fused = 0: `steps` launches of the one-step kernel k_smear_step (any L);
 * fused = 1: one launch of k_smear_fused, refused when L has no instantiation (16 and 128 have one).  The two agree
 * bit for bit. */
int sw_apply_smearing(sw_engine* h, int nb, int steps, int fused, const double* X, double* Y);
/* Perambulators of the registration of sw_set_distillation (build-only, stateless in the style of
 * sw_level_deflation_loops): for the nsrc source timeslices t0[s] (distinct, each in [0, L), any order) and the
 * sources eta^(s,n,a)[idx(a',y,t)] = delta_aa' delta_{t,t0[s]} v_n(y, t0[s]), z = A^-1 eta solved to `tol` on the
 * hierarchy that solves level 0 (no deflation, no permutation),
 *   out[s][t][c][m][n][a] = sum_x conj(v_m(x,t)) z^(s,n,a)[idx(c,x,t)],   complex128[nsrc][L][2][nev][nev][2],
 * the 2 nev nsrc columns in blocks of at most 256 (padded to 64 with zero columns): k_laph_sources, the solve,
 * k_laph_project (fp64 matrix cores, every output summed by one wave in the order x = 0, 4, 8, ...), the copy out.
 * iters int32[nsrc][nev][2] (may be NULL): the iteration count of every column.  Refused before anything is allocated
 * or launched without a registration, without a finalised hierarchy, on a bad timeslice list, maxiter < 1 or a null
 * out.  No mode buffer and no probe slot is touched; two calls agree bit for bit. */
int sw_perambulators(sw_engine* h, int nsrc, const int32_t* t0, double tol, int maxiter, double* out,
                     int32_t* iters);
/* k_laph_sources alone: out complex128[nsrc*nev*2][n], the sources of sw_perambulators in the reference ordering,
 * column (s, n, a). */
int sw_apply_laph_sources(sw_engine* h, int nsrc, const int32_t* t0, double* out);
/* k_laph_project alone on nb host vectors Z complex128[nb][n] (reference ordering): out complex128[L][2][nev][nb],
 * out[t][c][m][k] = sum_x conj(v_m(x,t)) Z[k][idx(c,x,t)]. */
int sw_apply_laph_project(sw_engine* h, int nb, const double* Z, double* out);
/* The momenta of sw_distilled_two_point: 1 <= nmom <= SW_MAX_MOMENTA distinct p[j] in [0, L); nmom = 0 clears.  Needs
 * the registration of sw_set_distillation.  The elementals
 *   M[j][t][m][m'] = sum_x e^{-2 pi i p_j x / L} conj(v_m(x,t)) v_m'(x,t)
 * are computed here on the fp64 matrix cores (k_laph_elementals: K = x, summed by one wave in the order x = 0, 4, 8,
 * ...) from the packed eigenvectors and the engine's phase table and stay on the device, transposed and padded to
 * ld = nev rounded up to 16 with exact zeros: nmom L ld^2 16 bytes.  Any call of sw_set_distillation and a new
 * definition of hierarchy 0 drop them. */
int sw_set_distillation_momenta(sw_engine* h, int nmom, const int32_t* p);
/* out complex128[nmom][L][nev][nev]: the registered elementals M[j][t][m][m'] (one launch of class
 * SW_KCLASS_LAPH_CONTRACT that counts no work, one copy). */
int sw_apply_laph_elementals(sw_engine* h, double* out);
/* The distilled two-point functions of the source timeslices t0[s] (as sw_perambulators), contracted on the device
 * (build-only, stateless).  The sources go in blocks of max(1, 256 / (2 nev)) WHOLE timeslices, padded to 64 columns;
 * per block k_laph_sources, the solve and k_laph_project exactly as sw_perambulators runs them on that chunk, then per
 * registered momentum j three launches on the block tau = proj[(t,c,m)][(s,n,a)]:
 *   k_laph_left    Y[(t,d)][col][m1]      = sum_m2 M[j][t][m1][m2] tau[(t,d)][m2][col]
 *   k_laph_right   X[(t,d)][s][b][m1][n1] = sum_n2 Y[(t,d)][(s,n2,b)][m1] conj(M[j][t0[s]][n1][n2])
 *   k_laph_reduce  T[s][j][a][b][c][d][t] = sum_{m1,n1} conj(tau[(t,c)][m1][(s,n1,a)]) X[(t,d)][s][b][m1][n1]
 *                  loops[s][j][a][b]      = sum_{m,n} M[j][t0[s]][n][m] tau[(t0[s],b)][m][(s,n,a)]
 * (the two products on v_mfma_f64_16x16x4_f64, the reduction on the VALU; every complex product in four real ones,
 * every sum in an order fixed by L, nev and the source's own columns: no atomics, two calls agree bit for bit, and a
 * source's values do not depend on the other sources of the call), and two small copies.
 *   T      complex128[nsrc][nmom][2][2][2][2][L]
 *   loops  complex128[nsrc][nmom][2][2]
 *   tau    complex128[nsrc][L][2][nev][nev][2], the perambulators of sw_perambulators, or NULL: nothing of that size
 *          leaves the device
 *   iters  int32[nsrc][nev][2], or NULL
 * Refused before anything is allocated or launched without a distillation registration, without momenta, without a
 * finalised hierarchy, on a bad timeslice list, maxiter < 1 or a null T or loops.  No mode buffer, no probe slot and
 * no registration is touched; the work buffers are released on return. */
int sw_distilled_two_point(sw_engine* h, int nsrc, const int32_t* t0, double tol, int maxiter, double* T,
                           double* loops, double* tau, int32_t* iters);
/* The contraction of sw_distilled_two_point alone on host perambulators tau complex128[nsrc][L][2][nev][nev][2], in the
 * same blocks (pad columns zero): T and loops as above. */
int sw_apply_laph_contract(sw_engine* h, int nsrc, const int32_t* t0, const double* tau, double* T, double* loops);
/* The two-meson building blocks of the source timeslices t0[s] (build-only, stateless): the sink
 * operators k = (G_k, sink_mom[k]), 1 <= nk <= SW_MAX_MESON_OPS, and the source operators kp = (H_kp, source_mom[kp]),
 * 1 <= nkp <= SW_MAX_MESON_OPS -- G = gamma_3 Gamma and H = Gamma' gamma_3 folded by the caller, complex128[n][2][2],
 * the momenta as indices into the list of sw_set_distillation_momenta.  With rho = 2 n + a the column of a source,
 *   Q[s][k][t][rho1][rho2] = sum conj(tau[s][t][c][m1][n1][a]) G_k[c][d] M[j_k][t][m1][m2] tau[s][t][d][m2][n2][b]
 *   S[s][kp][rho2][rho1]   = H_kp[b][a] conj(M[j_kp][t0[s]][n1][n2])
 *   C1[s][k][kp][t]        = tr[Q[s][k][t] S[s][kp]]
 *   C2[s][k][l][kp][lp][t] = tr[Q[s][k][t] S[s][kp] Q[s][l][t] S[s][lp]]
 * in the blocks of sw_distilled_two_point (k_laph_sources, the solve and k_laph_project exactly as sw_perambulators
 * runs them on that chunk), then per block 2 nk + 3 launches:
 *   k_laph_sink      W[(t,c)][m1][col]  = sum_d G[c][d] sum_m2 M[t][m1][m2] tau[(t,d)][m2][col]            per k
 *   k_laph_sandwich  Q^T[rho2][rho1]    = sum_(c,m1) W[(t,c)][m1][(s,rho2)] conj(tau[(t,c)][m1][(s,rho1)])  per k
 *   k_laph_source    R[rho][(n1,a)]     = sum_b H[b][a] sum_n2 Q[rho][(n2,b)] conj(M[t0][n1][n2])          all (k, kp)
 *   k_laph_trace1    C1 from Q and S;   k_laph_trace2    C2 = sum R_{k,kp}[rho][sigma] R_{l,lp}[sigma][rho]
 * (the products on v_mfma_f64_16x16x4_f64, the traces on the VALU; every complex product in four real ones, every sum
 * in an order fixed by nev: no atomics, two calls agree bit for bit, and a source's values do not depend on the other
 * sources of the call), and two small copies.
 *   C1     complex128[nsrc][nk][nkp][L]
 *   C2     complex128[nsrc][nk][nk][nkp][nkp][L]
 *   iters  int32[nsrc][nev][2] as sw_perambulators, or NULL
 * Refused before anything is allocated or launched without a distillation registration, without momenta, without a
 * finalised hierarchy, on a bad timeslice list, nk or nkp outside [1, SW_MAX_MESON_OPS], a momentum index outside the
 * registered list, maxiter < 1 or a null output.  No mode buffer, no probe slot and no registration is touched; the
 * work buffers, (nk + nk nkp + 1) ns L (2 ld)^2 16 bytes for a block of ns sources, are released on return. */
int sw_distilled_two_meson(sw_engine* h, int nsrc, const int32_t* t0, int nk, const double* sink_spin,
                           const int32_t* sink_mom, int nkp, const double* source_spin, const int32_t* source_mom,
                           double tol, int maxiter, double* C1, double* C2, int32_t* iters);
/* The contraction of sw_distilled_two_meson alone on host perambulators tau complex128[nsrc][L][2][nev][nev][2], in
 * the same blocks (pad columns zero): C1 and C2 as above; Q (or NULL) the sandwich, complex128[nsrc][nk][L][2 nev]
 * [2 nev], dense (one more launch per block). */
int sw_apply_laph_two_meson(sw_engine* h, int nsrc, const int32_t* t0, const double* tau, int nk,
                            const double* sink_spin, const int32_t* sink_mom, int nkp, const double* source_spin,
                            const int32_t* source_mom, double* C1, double* C2, double* Q);
/* The generalized perambulators of the distilled three-point functions (build-only, stateless in the style of
 * sw_perambulators): z_0^(n,b) and z_f^(m,e) the solutions of the eigenvector sources on the timeslices
 * t0 and tf (different, in [0, L)), in exactly the solve blocks of sw_perambulators(h, 2, {t0, tf}, ...).  For the nt
 * insertion timeslices tins[i] (distinct, in [0, L)) and the nmom momenta q[j] (1 <= nmom <= SW_MAX_MOMENTA, distinct,
 * in [0, L)), with row (m, e) -> 2 m + e and column (n, b) -> 2 n + b,
 *   G[i][j][2 f + c][row][col] = sum_x e^{-2 pi i q x / L} conj(z_f[idx(f,x,t)]) z_0[idx(c,x,t)]
 *   G[i][j][4 + mu][row][col]  = the sums of sw_apply_seq_dots over the link mu = 0 (x), 1 (t) contracted as the
 *                                conserved current, the noise index replaced by the pair of columns
 * by k_laph_generalized on v_mfma_f64_16x16x4_f64: every entry summed by one wave in the order x = 0, 4, 8, ..., two
 * calls agree bit for bit, an entry depends on its own two columns, timeslice and momentum alone.
 *   G      complex128[nt][nmom][6][2 nev][2 nev], through a device buffer of at most 256 MB, chunk by chunk
 *   tau    complex128[2][L][2][nev][nev][2] and iters int32[2][nev][2]: what sw_perambulators returns for {t0, tf},
 *          bit for bit; either may be NULL
 * Refused before anything is allocated or launched without a registration of sw_set_distillation, without a finalised
 * hierarchy or links on level 0, on bad end timeslices (tf == t0 included), a bad insertion list or momenta,
 * maxiter < 1 or a null G.  No mode buffer, no probe slot and no registration is touched. */
int sw_generalized_perambulators(sw_engine* h, int t0, int tf, int nt, const int32_t* tins, int nmom, const int32_t* q,
                                 double tol, int maxiter, double* G, double* tau, int32_t* iters);
/* k_laph_generalized alone on host fields Zf complex128[nbf][n] and Z0 complex128[nb0][n] (reference ordering,
 * 1 <= nbf, nb0 <= 256) in place of the solutions: out complex128[nt][nmom][6][nbf][nb0].  Needs a lattice level 0
 * with links (the condition of sw_set_three_point) and no distillation. */
int sw_apply_laph_generalized(sw_engine* h, int nbf, const double* Zf, int nb0, const double* Z0, int nt,
                              const int32_t* tins, int nmom, const int32_t* q, double* out);
/* The sequential-source kernel of SW_MODE_THREE_POINT alone on host solutions: Z complex128[2][nb][n] (spin group a,
 * noise k, reference ordering), out complex128[2][nb][n], out[a][k][idx(e,x,t)] = delta_{t,tf} e^{+2 pi i pf x / L}
 * sum_c ((g3 Gf g3)^H)[e][c] Z[a][k][idx(c,x,tf)] for the registration of sw_set_three_point.  The refusals of the
 * mode. */
int sw_apply_seq_sources(sw_engine* h, int nb, const double* Z, double* out);
/* The field x field reduction of SW_MODE_THREE_POINT alone on host fields: Zeta, Z complex128[2][nb][n] as above,
 * out complex128[5][nmom][2][2][2][2][L][nb] = S[d][j][a][b][f][c][t][k] of that mode with zeta = Zeta, z = Z.  The
 * refusals of the mode. */
int sw_apply_seq_dots(sw_engine* h, int nb, const double* Zeta, const double* Z, double* out);
/* Meson fields of the registered deflation vectors U (sw_set_deflation; k of them) for ONE spatial momentum p in [0, L)
 * (build-only): out[c][d][t][m][m'] = sum_x e^{-2 pi i p x / L} conj(U[idx(c,x,t)][m]) U[idx(d,x,t)][m'], complex128
 * [2][2][L][k][k] (at most 537 MB at k = 256, L = 128: one momentum per call).  Level 0 of hid 0, lattice set
 * (sw_set_lattice); fp64 MFMA, every entry summed in a fixed order (two calls agree bit for bit).  Fails without
 * vectors and with p out of range. */
int sw_meson_fields(sw_engine* h, int p, double* out);
/* The low-mode two-point functions of ONE momentum p for every source timeslice, contracted on the device from the
 * meson fields Phi of sw_meson_fields (same kernel, never copied to the host) and the registered low-mode inverse G:
 * out[a][b][c][d][t][t0] = g_a g_b sum_{m,m'} Phi[c][d][t][m][m'] conj(Psi[a][b][t0][m][m']), Psi = G Phi G^H,
 * g = (+1, -1), complex128 [2][2][2][2][L][L] -- utils.low_mode_two_point of one momentum.  fp64 MFMA, split-K partial
 * sums added in a fixed order, no atomics (two calls agree bit for bit).  About 3 * 64 * L * k^2 bytes of device
 * scratch for the call (1.6 GB at k = 256, L = 128), released on return; no registration, mode buffer or fetch is
 * touched.  Fails as sw_meson_fields does, and without a low-mode inverse (sw_set_low_mode_inverse). */
int sw_low_mode_two_point(sw_engine* h, int p, double* out);
/* Y = U G U^H X with the registered vectors and low-mode inverse (sw_set_low_mode_inverse) on nb host vectors in the
 * reference layout: the low-mode chain of SW_MODE_TWO_POINT_LMA alone (projection dots, G, expansion), without the
 * gamma_3 sign of its sources. */
int sw_apply_low_mode(sw_engine* h, int nb, const double* X, double* Y);
/* X = one multigrid cycle applied to B starting at level0 (MG.one_mg_step, multigrid.py:369-447). */
int sw_vcycle(sw_engine* h, int hid, int level0, int nb, const double* B, double* X);
/* ONE operation of the complex64 cycle (option "precond_f32") alone on host vectors, for the per-kernel parity
 * tests: X (and B) are cast to complex64 on the device, the operation is launched through the launcher the
 * complex64 cycle uses, with the kernel category the cycle passes -- so "f32_tiles", "f32_stages",
 * "f32_dense_stages", "f32_splitk", "f32_pairs" and the batch width pick the kernel variant exactly as they do
 * there --, and the result is widened (exact) into Y.  The complex64 mirrors are made whatever "precond_f32" is.
 * `which` at `level`:
 *   SW_OP32_A           the level operator of a block level (block-row kernel, or grouped ELL where the level has
 *                       no block rows); modes 0, 1, 3
 *   SW_OP32_R           Y = R_level X        X: level vectors, Y: vectors of level + 1
 *   SW_OP32_P           Y = P_level X        X: vectors of level + 1, Y: level vectors
 *   SW_OP32_P_EVEN      the same onto the even sites' rows only (option "p_even", an even-odd smoothed level)
 *   SW_OP32_RE          Y = R_level X from the even sites' columns only (lattice level smoothed even-odd; the
 *                       odd sites' entries of X are not read)
 *   SW_OP32_COARSEST    Y = coarsest_inv X   (level = the coarsest level)
 *   SW_OP32_EO0 + q     even-odd operator q = 0..4 of a block level (sw_set_eo_operator); modes 0, 1, 3; q = 4
 *                       is launched as a dense operator, like the coarsest inverse
 *   SW_OP32_SCHUR       Y_e = S X_e on the lattice level (k_schur_step, half vectors: the odd sites' entries of X
 *                       are not read)
 *   SW_OP32_EO_SMOOTH   the lattice level's even-odd smoother as the cycle runs it: b'_e = b_e + H_eo b_o / D,
 *                       the registered steps x_e <- x_e + w_k (b'_e - S x_e) from x_e = the even sites' entries
 *                       of X, then x_o = (b_o + H_oe x_e) / D; B = b, Y = x
 *   SW_OP32_EO_SMOOTH_REDUCED  the steps alone, as the even-odd reduced cycle runs them: B holds b'_e
 * mode (operations that list modes; 0 otherwise): 0: Y = op X, 1: Y = B - op X, 3: Y = X + w (B - op X) with
 * w = w_re + i w_im rounded to complex64.  flags = SW_OP32_INPLACE (mode 1 only): B and Y are X itself on the
 * device, Y = X - op X written over X, as the cycle calls even-odd operator 3.  B may be NULL where it is not
 * read.  Rows an operation does not write come back zero (in place: as they went in).  info (may be NULL)
 * receives {row tiles, k-steps per tile} of the operator's block-row form (0, 0 without one) and {group size G,
 * entries per row K} of its grouped-ELL form (0, 0 without one; lattice-level kernels: all four 0). */
#define SW_OP32_A 0
#define SW_OP32_R 1
#define SW_OP32_P 2
#define SW_OP32_P_EVEN 3
#define SW_OP32_RE 4
#define SW_OP32_COARSEST 5
#define SW_OP32_EO0 6
#define SW_OP32_SCHUR 11
#define SW_OP32_EO_SMOOTH 12
#define SW_OP32_EO_SMOOTH_REDUCED 13
#define SW_OP32_INPLACE 1
int sw_apply_op32(sw_engine* h, int hid, int level, int which, int mode, int nb, const double* X, const double* B,
                  double w_re, double w_im, int flags, double* Y, int32_t* info);
/* The fp64 twin of sw_apply_op32 (test-only): ONE operation of the fp64 cycle on host vectors, with no casts,
 * through the launcher and kernel category that cycle uses, so use_mfma, mfma_ops, mfma_3m, the tile, stage, block
 * map, dense_lds, ell_order, p_even and stencil options and the batch width select the kernel variant as they do
 * there.  Same `which` codes, modes, flags, zeroed output and info.  SW_OP32_A also acts on the lattice level
 * (the Wilson stencil; mode 3 is its fused step Y = X + w (B - A X), no in-place form); w is taken in full double
 * precision.  SW_OP32_COARSEST is the dense inverse itself, not the even-odd direct path a directly solved
 * coarsest level takes in the cycle.  SW_OP32_SCHUR and the two SW_OP32_EO_SMOOTH codes are refused. */
int sw_apply_op64(sw_engine* h, int hid, int level, int which, int mode, int nb, const double* X, const double* B,
                  double w_re, double w_im, int flags, double* Y, int32_t* info);
/* ---- one operation of the Krylov solver alone (test-only) -----------------------------------
 * The batched BLAS-1 kernels and the per-probe FGMRES scalar updates, one operation per call on host data, each
 * through the host helper the solves use, so the row blocking, the in-launch or two-stage reduction (options
 * fused_reduce, dot_blocks), and the KT / NV kernel instantiation are chosen exactly as in a solve.  No hierarchy
 * is needed.  Vectors: n rows, nb columns, (nb, n) host layout as everywhere else, complex128; per-probe arrays
 * [rows][nb], complex128 unless said to be real.  storage: SW_KRYLOV_C128, or SW_KRYLOV_C64 -- the operands are
 * rounded to complex64 on the device and the complex64 instantiation runs.  info (may be NULL) receives {row
 * blocks P, rows per block, 1 when the reduction was completed inside the launch, groups of 32 row blocks}. */
#define SW_KRYLOV_C128 0
#define SW_KRYLOV_C64 1
/* out[K][nbp] = V_k^H W (k_multidot; nbp = nb rounded up to 64: the pad columns come back too and must be zero),
 * V = K vectors one after the other; with svec[K][nb] (real) also coef[K][nb] = svec^2 out.  1 <= K <= 34. */
int sw_krylov_multidot(sw_engine* h, int n, int nb, int K, int storage, const double* V, const double* W,
                       const double* svec, double* out, double* coef, int32_t* info);
/* The BLAS-1 half of a restart cycle in Gram-matrix form: U = the NV = L + 1 vectors [r0, w_0 .. w_{L-1}], Z the L
 * directions; k_gram with the Gram tail (Cholesky solve per probe), then X += sum_j ys_j z_j (k_multiaxpy).
 * In/out: X, normb[nb] (real), iters[nb]; out: gram[NV (NV + 1) / 2][nb] (entry (a, b), a <= b, at
 * a NV - a (a - 1) / 2 + (b - a)), ys[L][nb], relres[nb], g[nb] (real: |r_L| / |b| and |r_0| / |b|), notconv = the
 * probes left above tol_stop.  flags: SW_KRYLOV_INIT (r0 is the right-hand side: sets normb and iters),
 * SW_KRYLOV_NOTAIL (the inner products alone: only U and gram are used).  2 <= NV <= 5; refused when the
 * in-launch reduction is not available (fused_reduce off, or too many row blocks). */
#define SW_KRYLOV_INIT 1
#define SW_KRYLOV_NOTAIL 2
int sw_krylov_gram_cycle(sw_engine* h, int n, int nb, int NV, int flags, const double* U, const double* Z,
                         double* X, double* normb, int32_t* iters, double tol, double tol_stop, int iter_base,
                         double* gram, double* ys, double* relres, double* g, int32_t* notconv, int32_t* info);
/* W <- W + sign sum_k coef[k] V_k in place (k_multiaxpy).  flags: SW_KRYLOV_NORM (nrm[nb] (real) = |W|^2 of the
 * values before they are narrowed to the storage of W), SW_KRYLOV_W32 (W32 = the complex64 copy of the new W,
 * widened; fp64 W only).  Storage pairs (V, W): (C128, C128), (C64, C64), (C64, C128); others are refused. */
#define SW_KRYLOV_NORM 1
#define SW_KRYLOV_W32 2
int sw_krylov_multiaxpy(sw_engine* h, int n, int nb, int K, int storage_v, int storage_w, int flags,
                        const double* V, const double* coef, double sign, double* W, double* nrm, double* W32,
                        int32_t* info);
/* One per-probe scalar update of FGMRES(m) on an uploaded state (k_fg_tail, k_fg_solve).  state, in and out: H
 * [(m + 1) m], cs [m], sn [m], g [m + 1], y [m], normb [1], relres [1], svec [m + 1], ys [m] rows of nb complex
 * entries, one block after the other (H row-major: entry (i, j) in row i m + j); iters[nb] in and out.
 *   SW_KRYLOV_BEGIN   start of a cycle from nrm[nb] (real) = |r|^2; flag: first cycle (fixes normb, iters, relres)
 *   SW_KRYLOV_HESS    column j from the raw inner products h1[(m + 2)][nb], h2 (second Gram-Schmidt pass, or NULL)
 *                     and nrm = |vtilde_{j+1}|^2; flag: the last-step form, |A ztilde_j|^2 in row j + 1 of h1, nrm unused
 *   SW_KRYLOV_VERIFY  true-residual check from nrm = |b - A x|^2
 *   SW_KRYLOV_SOLVE   y = H(0:j, 0:j)^-1 g(0:j), ys = svec y
 * notconv = the probes HESS / VERIFY left above tol_stop. */
#define SW_KRYLOV_BEGIN 1
#define SW_KRYLOV_HESS 2
#define SW_KRYLOV_VERIFY 3
#define SW_KRYLOV_SOLVE 5
int sw_krylov_scalars(sw_engine* h, int m, int nb, int op, int j, int flag, double tol, double tol_stop,
                      int iter_base, const double* h1, const double* h2, const double* nrm, double* state,
                      int32_t* iters, int32_t* notconv);
/* Solve A_level0 X = B to ||r|| < tol*||b|| per right-hand side (MG.solve -> pyamg fgmres,
 * multigrid.py:347-366).  iters[nb], relres[nb] may be NULL.  Non-convergence within
 * maxiter is NOT an error (the reference discards exitCode); it is visible in relres. */
int sw_solve(sw_engine* h, int hid, int level0, int nb, const double* B, double* X, double tol,
             int maxiter, int32_t* iters, double* relres);

/* ---- the probe loop body ----------------------------------------------------------------- */
#define SW_MODE_HUTCHINSON 0   /* utils.py:210-250 */
#define SW_MODE_MLMC 1         /* utils.py:252-361 */
#define SW_MODE_MLMC_SKIP 2    /* utils.py:252-361 with mg_solver.skip_level and i == 0 */
#define SW_MODE_LEVEL 3        /* e_k = x^H A_l^-1 C_l x: one level's own trace term, estimated
                                  stochastically (build-only; the reference computes the coarsest
                                  term directly and raises for the stochastic form,
                                  stoch_trace.py:428-437) */
#define SW_MODE_HUTCHINSON_SHIFTS 4 /* e_jk = (D_{s_j}^T x_k)^H A^-1 (x_k - U U^H x_k) for the shifts of
                                  sw_set_shifts, level 0: one projection and one solve per probe serve all
                                  shifts (build-only; U as registered, sw_set_perm ignored; its expectation
                                  is Tr(D_s A^-1 (I - U U^H)), per-probe values are not those of HUTCHINSON) */
#define SW_MODE_HUTCHINSON_LOOPS 5 /* l_k[p][a][b][t] = sum_x e^{-2 pi i p x / L} conj(x_k[idx(a,x,t)])
                                  z_k[idx(b,x,t)], z_k = A^-1 (x_k - U U^H x_k), for the momenta of
                                  sw_set_loop_momenta, level 0: projection and solve exactly as
                                  HUTCHINSON_SHIFTS (build-only; U as registered, sw_set_perm ignored).
                                  sw_hutch_fetch returns sum_t (l[0][0][t] + l[1][1][t]) of the FIRST
                                  registered momentum, which is x^H z -- the shift-0 value of
                                  HUTCHINSON_SHIFTS -- only when that momentum is 0 */
#define SW_MODE_TWO_POINT 6     /* T_k[j][a][b][c][d][t] = sum_x e^{-2 pi i p_j x / L} conj(z_k^(j0,a)[idx(c,x,t)])
                                  z_k^(j,b)[idx(d,x,t)], z_k^(j,a) = A^-1 eta_k^(j,a), for the source timeslice
                                  and momenta of sw_set_two_point, level 0 (build-only; no deflation, no
                                  permutation).  The probes are the noises: probe k's code at idx(0,y,t0) is
                                  xi_k(y); one solve runs over all 2 nmom pad64(nb) columns.  sw_hutch_fetch
                                  returns sum_t sum_ac T[j0][a][a][c][c][t] = sum_a ||z^(j0,a)||^2 and, as the
                                  fine iteration count of a noise, the largest count among its 2 nmom columns. */
#define SW_MODE_MLMC_LOOPS 7    /* l_k[p][a][b][t] = S_q(Pi_l x_k, Pi_l d_k), S_q(u, v) = sum_x e^{-2 pi i p x / L}
                                  conj(u[idx(a,x,t)]) v[idx(b,x,t)], d_k = A_l^-1 x_k - P_l A_{l+1}^-1 R_l x_k the
                                  MLMC difference of the plain probe at `level` of hid 0, Pi_l = P_0 ... P_{l-1}
                                  (Pi_0 = I), for the momenta of sw_set_loop_momenta: the level term of the
                                  timeslice loops (build-only).  Solves and iteration counts as SW_MODE_MLMC;
                                  sw_set_perm / sw_set_rhsmap are ignored (as HUTCHINSON_LOOPS ignores sw_set_perm)
                                  and a level with MLMC-level deflation vectors is refused.  sw_hutch_fetch returns
                                  sum_t (l[0][0][t] + l[1][1][t]) of the FIRST registered momentum, which is
                                  x^H d -- the SW_MODE_MLMC value of the probe -- when that momentum is 0 */
#define SW_MODE_MLMC_LOOPS_SKIP 8 /* the same with d_k = A_0^-1 x_k - P_0 P_1 A_2^-1 R_1 R_0 x_k, level 0 only
                                  (as SW_MODE_MLMC_SKIP) */
#define SW_MODE_MLMC_DEFL_LOOPS 9 /* SW_MODE_MLMC_LOOPS with the MLMC-level deflation of `level` (sw_set_level_deflation):
                                  l_k[p][a][b][t] = S_q(Pi_l x_k, Pi_l d_k) with d_k the MLMC difference of the
                                  projected probe x_k - V_l V_l^H x_k (the fine solve and the restriction take it),
                                  the left operand stays the plain probe (build-only).  Its expectation is
                                  Tr(Pi_l^H Gamma_q Pi_l D_l (I - V_l V_l^H)); sw_level_deflation_loops gives the rest.
                                  With no vectors at `level` the batch equals the SW_MODE_MLMC_LOOPS batch bit for
                                  bit.  Buffer and fetch of SW_MODE_MLMC_LOOPS (sw_hutch_fetch_mlmc_loops);
                                  sw_hutch_fetch returns x^H d -- the SW_MODE_MLMC value of the probe with the same
                                  vectors and no perm / rhsmap -- when the first registered momentum is 0 */
#define SW_MODE_MLMC_DEFL_LOOPS_SKIP 10 /* the same on SW_MODE_MLMC_LOOPS_SKIP's difference, level 0 only */
#define SW_MODE_TWO_POINT_LMA 11 /* SW_MODE_TWO_POINT's stochastic remainder under low-mode averaging, level 0 (build-only):
                                  R_k = T(z_k, z_k) - T(z_L, z_L) with the sources, the one solve z = A^-1 eta and the
                                  pair sum T of SW_MODE_TWO_POINT and z_L^(j,a) = A_L^-1 eta^(j,a) = g_a U G (U^H eta^(j,a)),
                                  g = (+1, -1), for the registered vectors and low-mode inverse.  E[R_k] = E[T_k] - E_L
                                  with E_L the pair sum of A_L^-1 in place of A^-1, exactly, for any U and G.  Needs
                                  sw_set_two_point, sw_set_deflation and sw_set_low_mode_inverse.  A buffer of its own
                                  (sw_hutch_fetch_two_point_lma; sw_hutch_fetch_two_point keeps returning the last
                                  SW_MODE_TWO_POINT batch); sw_hutch_fetch returns sum_t sum_ac R[j0][a][a][c][c][t] and
                                  the iteration counts of SW_MODE_TWO_POINT.  With G = 0 the batch equals the
                                  SW_MODE_TWO_POINT batch bit for bit. */
#define SW_MODE_HUTCHINSON_LINK_LOOPS 12 /* SW_MODE_HUTCHINSON_LOOPS plus the point-split link loops, level 0 (build-only):
                                  projection, solve and local loops exactly as mode 5 -- sw_hutch_fetch and
                                  sw_hutch_fetch_loops return what a mode-5 batch on the same probes returns, bit for
                                  bit -- and, from the same z_k and codes, the four link branches d = (F_x, B_x, F_t, B_t)
                                  F_mu,k[p][a][b][t] = sum_x e^{-2 pi i p x / L} U_mu(n) conj(x_k[idx(a,n)]) z_k[idx(b,n+mu)],
                                  B_mu,k[p][a][b][t] = sum_x e^{-2 pi i p x / L} conj(U_mu(n)) conj(x_k[idx(a,n+mu)]) z_k[idx(b,n)],
                                  n = (x,t) the site that owns the link, n+x^ = ((x+1) mod L, t), n+t^ = (x, (t+1) mod L),
                                  U_x = U1, U_t = U2 of sw_set_lattice, for the momenta of sw_set_loop_momenta.  A
                                  buffer of its own (sw_hutch_fetch_link_loops).  Refused at a level other than 0,
                                  without momenta and when level 0 is no lattice level with links. */
#define SW_MODE_THREE_POINT 13  /* three-point functions source -> insertion at t -> sink at tf, level 0 (build-only), for
                                  the registration of sw_set_three_point.  Per noise k, xi_k(y) = the code of probe k
                                  at idx(0,y,t0) as in SW_MODE_TWO_POINT:
                                  eta_k^a[idx(a',y,t)] = delta_aa' delta_{t,t0} xi_k(y),  z_k^a = A^-1 eta_k^a  (stage 1),
                                  s_k^a[idx(e,x,t)] = delta_{t,tf} e^{+2 pi i pf x / L} sum_c ((g3 Gf g3)^H)[e][c] z_k^a[idx(c,x,tf)],
                                  zeta_k^a = A^-1 s_k^a  (stage 2, the same tol; no deflation in either stage), and for
                                  the branches d = (local, F_x, B_x, F_t, B_t), n = (x,t), n+mu as in mode 12:
                                  S_k[0][j][a][b][f][c][t] = sum_x e^{-2 pi i q_j x / L} conj(zeta^a[idx(f,n)]) z^b[idx(c,n)],
                                  S_k[F_mu] = sum_x e^{-2 pi i q_j x / L} U_mu(n) conj(zeta^a[idx(f,n)]) z^b[idx(c,n+mu)],
                                  S_k[B_mu] = sum_x e^{-2 pi i q_j x / L} conj(U_mu(n)) conj(zeta^a[idx(f,n+mu)]) z^b[idx(c,n)].
                                  Buffers of its own (sw_hutch_fetch_three_point; the last batches of the modes 4, 5,
                                  6, 11 and 12 stay fetchable, and the reverse).  sw_hutch_fetch returns c_k =
                                  sum_{a,c,x} |z_k^a[idx(c,x,tf)]|^2, the pion two-point value at the sink slice, and
                                  per noise the largest stage-1 column count plus the largest stage-2 column count.
                                  Refused before any launch at a level other than 0, without a registration and when
                                  level 0 is no lattice level with links. */
#define SW_MODE_TWO_POINT_SMEARED 14 /* SW_MODE_TWO_POINT with smeared sources and sinks, level 0 (build-only), for the
                                  registrations of sw_set_two_point and sw_set_smearing:
                                  eta_k^(j,a) = S_n (e^{+2 pi i p_j y / L} xi_k) on the timeslice t0, z = A^-1 eta, and
                                  for every registered sink level s_i the pair sums T^(i)_k of S_{s_i} z_k, the
                                  solutions being smeared in place from one level to the next.  A buffer of its own
                                  (sw_hutch_fetch_two_point_smeared); sw_hutch_fetch returns the pion total of sink
                                  level 0 and the iteration counts of SW_MODE_TWO_POINT.  With source_steps = 0 and
                                  the sink levels [0] the batch equals the SW_MODE_TWO_POINT batch bit for bit.
                                  Refused before any launch at a level other than 0 and without either
                                  registration. */
/* One batch of probes x_k in {-1,+1}^n (int8, nb*n, reference ordering) at `level`
 * (build-only extension: entries +-2 encode +-i, i.e. Z4 probes {1,i,-1,-i}):
 *   HUTCHINSON: e_k = x^H A^-1 Pperm^T (x - U U^H x)
 *   MLMC:       e_k = x^H A_f^-1 C x - x^H P A_c^-1 R C x   (SKIP: P0 P1, R1 R0)
 * ests: complex128[nb]; iters: int32[2*nb] = fine-solve and coarse-solve iteration counts. */
int sw_hutch_batch(sw_engine* h, int mode, int level, int nb, const int8_t* probes, double tol,
                   int maxiter, double* ests, int32_t* iters);
/* Split form used when the probes are to be resident in HBM before timing starts:
 * upload -> run (asynchronous on the engine stream) -> sync -> fetch. */
int sw_probes_upload(sw_engine* h, int level, int nb, const int8_t* probes);   /* slot 0 + select */
/* Several batches resident at once (bench: all inputs in HBM before the timed region). */
int sw_probes_upload_slot(sw_engine* h, int slot, int level, int nb, const int8_t* probes);
int sw_probes_select(sw_engine* h, int slot);
/* Device-side probe generation (replaces np.random.randint(2, size=n) at utils.py:213-216,
 * 255-258 for probes that never need to exist on the host).  The engine holds a window of the
 * reference's MT19937 stream: sw_probes_stream_set() hands over the 624 raw state words at the
 * stream position that becomes position 0 (sw_mt_window() below makes them from a seed or from a
 * NumPy state); sw_probes_generate() fills `slot` with the nb probes whose first entry is draw
 * number `pos` of that stream (one 32-bit draw per entry, bit-exact with NumPy), jumping there
 * with GF(2) jump polynomials -- cost independent of `pos`.  Asynchronous on a generation stream of the
 * engine's own: the call returns when the work is queued, the sw_hutch_run that consumes the slot waits
 * for it on the device -- so the probes of batch k + 1 (another slot) are drawn while batch k is solved. */
#define SW_PROBES_Z2 1   /* entry = 2*(draw & 1) - 1              (the reference's probes)          */
#define SW_PROBES_Z4 2   /* draw & 3 -> 1, i, -1, -i as 1,2,-1,-2  (build-only, BASELINE config 1)  */
int sw_probes_stream_set(sw_engine* h, const uint32_t* window);
int sw_probes_generate(sw_engine* h, int slot, int level, int nb, int kind, uint64_t pos);
/* Copy the int8 codes held in `slot` (uploaded or generated) to the host: nb*n bytes. */
int sw_probes_fetch(sw_engine* h, int slot, int8_t* out);
int sw_hutch_run(sw_engine* h, int mode, int level, double tol, int maxiter);
int sw_sync(sw_engine* h);
int sw_hutch_fetch(sw_engine* h, double* ests, int32_t* iters);
/* After a SW_MODE_HUTCHINSON_SHIFTS batch: ests complex128[nshifts][nb], row j = the estimates at shift j of
 * the registration (sw_hutch_fetch returns row 0 and the iteration counts). */
int sw_hutch_fetch_shifts(sw_engine* h, double* ests);
/* After a SW_MODE_HUTCHINSON_LOOPS batch: out complex128[nmom][2][2][L][nb], the loops l_k[p][a][b][t] of every
 * probe k of the batch (sw_hutch_fetch returns the scalar total of the first momentum and the iteration
 * counts). */
int sw_hutch_fetch_loops(sw_engine* h, double* out);
/* After a SW_MODE_MLMC_LOOPS / _SKIP batch: out complex128[nmom][2][2][L][nb], the level loops of every probe of the
 * batch (a buffer of its own: sw_hutch_fetch_loops keeps returning the last SW_MODE_HUTCHINSON_LOOPS batch). */
int sw_hutch_fetch_mlmc_loops(sw_engine* h, double* out);
/* After a SW_MODE_HUTCHINSON_LINK_LOOPS batch: out complex128[4][nmom][2][2][L][nb], the link branches
 * F/B_k[d][p][a][b][t] of every probe of the batch (a buffer of its own: batches of other modes leave it intact, and
 * sw_hutch_fetch_loops returns the local loops of the same batch). */
int sw_hutch_fetch_link_loops(sw_engine* h, double* out);
/* After a SW_MODE_TWO_POINT batch: out complex128[nmom][2][2][2][2][L][nb], the pair sums T_k[j][a][b][c][d][t] of
 * every noise k of the batch.  The results of the modes 4, 5 and 6 live in buffers of their own: each fetch
 * returns its own mode's last batch whatever ran since. */
int sw_hutch_fetch_two_point(sw_engine* h, double* out);
/* After a SW_MODE_TWO_POINT_LMA batch: out complex128[nmom][2][2][2][2][L][nb], the remainders R_k[j][a][b][c][d][t]. */
int sw_hutch_fetch_two_point_lma(sw_engine* h, double* out);
/* After a SW_MODE_THREE_POINT batch: out complex128[5][nmom][2][2][2][2][L][nb], the sums S_k[d][j][a][b][f][c][t] of
 * every noise k of the batch ("no three-point batch to fetch" otherwise). */
int sw_hutch_fetch_three_point(sw_engine* h, double* out);
/* After a SW_MODE_TWO_POINT_SMEARED batch: out complex128[nsink][nmom][2][2][2][2][L][nb], the pair sums
 * T^(i)_k[j][a][b][c][d][t] of every sink level i and noise k ("no smeared two-point batch to fetch" otherwise, and
 * again after sw_set_smearing or sw_set_two_point). */
int sw_hutch_fetch_two_point_smeared(sw_engine* h, double* out);

/* ---- multi-GPU: the one collective of the path ------------------------------------ */
/* One process per GPU, one engine per process; the probe loop shards by probe and needs a single
 * small reduction per round: {sum Re e, sum Im e, sum |e|^2, n} (population variance as
 * stoch_trace.py:143-145).  RCCL (ncclAllReduce over xGMI) behind the C ABI, loaded on first use:
 * rank 0 calls sw_comm_unique_id and hands the 128 bytes to the other ranks by any means; every
 * rank calls sw_comm_init; sw_allreduce_stats sums the four doubles in place over all ranks. */
int sw_comm_unique_id(char id[128]);
int sw_comm_init(sw_engine* h, int nranks, int rank, const char id[128]);
int sw_allreduce_stats(sw_engine* h, double stats[4]);
int sw_comm_destroy(sw_engine* h);

/* ---- measurement ----------------------------------------------------------------------- */
/* Timed stencil loop for the roofline figure: `reps` applications of the level-0 operator of
 * hierarchy hid on nb resident right-hand sides, HIP events on the engine stream.
 * ms_per_apply is the average launch duration. */
int sw_bench_dirac(sw_engine* h, int hid, int level, int nb, int reps, double* ms_per_apply);
/* Bucketed device time (ms) since the last reset, measured with HIP events when profiling
 * is enabled (CustomTimer buckets of utils.py:366-445 plus the Krylov BLAS-1 the reference
 * leaves untimed):  [0]=mvm [1]=defl [2]=P [3]=R [4]=axpy [5]=dots [6]=coarsest [7]=other. */
int sw_set_profiling(sw_engine* h, int on);
int sw_timers(sw_engine* h, double t[8]);
int sw_timers_reset(sw_engine* h);
/* Accumulated HIP-event time and launch count of one kernel class since the last reset
 * (profiling on): classes 0..7 as sw_timers (without the kernels listed next), and */
#define SW_KCLASS_STENCIL 8         /* k_stencil<0>  Y = A X                       */
#define SW_KCLASS_STENCIL_RES 9     /* k_stencil<1>  Y = B - A X                   */
#define SW_KCLASS_STENCIL_SM 10     /* k_stencil<2>  Y = X + w (B - A X)           */
#define SW_KCLASS_MFMA_DENSE 11     /* k_bsr_mfma, dense coarsest inverse          */
#define SW_KCLASS_MFMA_OP 12        /* k_bsr_mfma, block-structured level operator */
/* (class 13: unused; it was a fused two-step stencil, removed after it measured no faster) */
#define SW_KCLASS_MFMA_OP2 14       /* k_bsr_mfma, level operators below level 1   */
#define SW_KCLASS_SCHUR 15          /* k_schur_step / k_eo_hop, even-odd smoother  */
#define SW_KCLASS_TP_SOURCES 17     /* k_slice_sources (SW_MODE_TWO_POINT); in sw_timers: other */
#define SW_KCLASS_TP_DOTS 18        /* k_slice_pair_dots, k_pair_total (SW_MODE_TWO_POINT); in sw_timers: dots */
#define SW_KCLASS_SLICE_CDOTS 19    /* k_slice_cdots (SW_MODE_MLMC_LOOPS, sw_coarsest_loops); in sw_timers: dots */
#define SW_KCLASS_MESON_FIELD 20    /* k_meson_field (sw_meson_fields); in sw_timers: dots; sw_kernel_work counts
                                       8 * 4 * L^2 * ld^2 flops per launch, ld = the rank rounded up to 16 */
#define SW_KCLASS_LM_CONTRACT 21    /* k_cgemm_nt, k_lm_two_point_reduce (sw_low_mode_two_point); in sw_timers: dots;
                                       sw_kernel_work counts 8 * (2 * 4L * ld^3 + (4L)^2 * k^2) flops per call */
#define SW_KCLASS_LINK_DOTS 22      /* k_slice_link_dots (SW_MODE_HUTCHINSON_LINK_LOOPS); in sw_timers: dots */
#define SW_KCLASS_3PT_SOURCES 23    /* k_seq_sources, k_pair_slice_total and the stage-1 k_slice_sources
                                       (SW_MODE_THREE_POINT); in sw_timers: other */
#define SW_KCLASS_3PT_DOTS 24       /* k_slice_seq_dots (SW_MODE_THREE_POINT); in sw_timers: dots */
#define SW_KCLASS_SMEAR 25          /* k_smear_step, k_smear_fused (SW_MODE_TWO_POINT_SMEARED, sw_apply_smearing); in
                                       sw_timers: other */
#define SW_KCLASS_LAPH 26           /* k_laph_sources, k_laph_project (sw_perambulators, sw_apply_laph_*); in sw_timers
                                       the sources count as other, the projection as dots; sw_kernel_work counts
                                       8 * 2 L^2 * ld * ncols flops per projection launch, ld = nev rounded up to 16 */
#define SW_KCLASS_LAPH_CONTRACT 27  /* k_laph_elementals, k_laph_left, k_laph_right, k_laph_reduce (and the unpack of
                                       sw_apply_laph_elementals); in sw_timers: dots.  sw_kernel_work counts, with
                                       K4 = nev rounded up to 4 and Lp = L rounded up to 4, 8 * L * Lp * ld^2 flops
                                       per momentum of sw_set_distillation_momenta and, per momentum and block of
                                       ns sources in ncols columns, 8 * (2L * ncols * ld * K4 + 4L * ns * ld^2 * K4
                                       + 16 L * ns * nev^2 + 4 ns * nev^2) */
#define SW_KCLASS_LAPH_GENERALIZED 28  /* k_laph_generalized (sw_generalized_perambulators,
                                       sw_apply_laph_generalized); in sw_timers: dots.  sw_kernel_work counts, per
                                       insertion timeslice and momentum, the eight complex products of the tiles
                                       issued: 8 * 8 * Lp * (16 RT) * (16 NT ncg), Lp = L rounded up to 4, RT =
                                       ceil(rows / 16), ncg = ceil(ceil(columns / 16) / 8) column groups of NT =
                                       ceil(ceil(columns / 16) / ncg) tiles */
#define SW_KCLASS_LAPH_TWO_MESON 30  /* (29 is the engine's internal bucket of k_laph_sources, reported with class
                                       26, and stays out of range)  k_laph_sink, k_laph_sandwich, k_laph_source, k_laph_trace1, k_laph_trace2 (and
                                       the unpack of Q); in sw_timers: dots.  sw_kernel_work counts, per block of ns
                                       sources in ncols columns, with K4 = nev and K4' = 2 nev rounded up to 4, RT =
                                       ceil(2 nev / 16) row tiles whose columns go in h = ceil(RT / 8) passes of NT =
                                       ceil(RT / h) tiles, z(.) the non-zero entries of a folded spin matrix:
                                       8 * (sum_k [z(G_k) L ld ncols K4 + L ns (16 RT) (16 NT h) K4']
                                       + sum_kp nk z(H_kp) L ns (16 RT) ld K4 + nk nkp L ns 5 nev^2
                                       + nk^2 nkp^2 L ns (2 nev)^2) */
int sw_kernel_stats(sw_engine* h, int which, double* total_ms, int64_t* launches);
/* Floating-point operations issued by the launches of an MFMA kernel class since the last reset
 * (profiling on): 8 flops per complex multiply-add over every (row tile, k-step, probe). */
int sw_kernel_work(sw_engine* h, int which, double* work);
/* Kernel launches issued since the last reset (for launch-bound analysis). */
int sw_launch_count(sw_engine* h, int64_t* n);

/* ---- host-only helpers (no GPU needed) ---------------------------------------------------- */
/* The probe stream of utils.py:213-216: MT19937 seeded as np.random.seed(seed); entry =
 * 2*(next_uint32 & 1) - 1; the stream continues across calls. */
typedef struct sw_mt19937 sw_mt19937;
sw_mt19937* sw_mt_create(uint32_t seed);
void sw_mt_destroy(sw_mt19937* g);
void sw_mt_skip(sw_mt19937* g, uint64_t ndraws);
void sw_mt_raw(sw_mt19937* g, uint64_t n, uint32_t* out);
void sw_mt_rademacher(sw_mt19937* g, uint64_t n, int8_t* out);
void sw_mt_z4(sw_mt19937* g, uint64_t n, int8_t* out);   /* codes 1,2,-1,-2 from draw & 3 */
/* NumPy interchange: key[624] + pos exactly as np.random.get_state()[1:3]. */
sw_mt19937* sw_mt_from_state(const uint32_t* key, int pos);
void sw_mt_get_state(const sw_mt19937* g, uint32_t* key, int* pos);
/* The 624 raw words starting at the current stream position (input of sw_probes_stream_set). */
void sw_mt_window(sw_mt19937* g, uint32_t* out);
/* Jump ahead by ndraws in O(1) state refills: g_J(x) = x^J mod phi(x) over GF(2) applied to the
 * window (sw_mt_skip is the sequential checker).  sw_mt_jump_poly returns the 19937 coefficient
 * bits of g_J in 624 words (bit i of the array = coefficient of x^i); non-zero = failure. */
int sw_mt_jump(sw_mt19937* g, uint64_t ndraws);
int sw_mt_jump_poly(uint64_t ndraws, uint32_t* poly);
int sw_mt_window_jump(const uint32_t* window, uint64_t ndraws, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* SCHWINGER_HIP_H */
