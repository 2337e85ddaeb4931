"""GPU: every fp64 operator kernel variant alone, against a double-double evaluation of the same operation.

Engine.apply_op64 (sw_apply_op64) runs ONE operation through the launcher the fp64 cycle uses, with the kernel
category the cycle passes and no casts, so the engine options and the batch width pick the kernel variant exactly
as in production.  The reference is the same expression on the same float64 operands in double-double arithmetic
(oracle/f64_bounds.py; unit roundoff about 2^-104), computed once per (operator, mode) and shared by all variants;
the limits are those of the complex64 tests with u = 2^-53 (tests/test_f64_bounds_host.py shows on the CPU that
they pass the emulations and reject a dropped or doubled k-step, a dropped tail tile, own-X rows from the wrong
tile, a flipped w.y sign and an unwritten (row tile, chunk)):

  hard limit    every real and imaginary part within (4 K + 16) u S_i (any order of the sum, also the
                three-product form; K = stored complex entries per row, padding included: 4 KS for block rows, the
                reported K for grouped ELL, 9 for the Wilson stencil)
  tight limit   max_i err / (u S_i) <= 4 c_ref + 4, c_ref the same figure of the NumPy float64 emulation of the
                kernel's arithmetic form: four separate real sums (k_bsr_mfma), three products with rounded operand
                sums (k_bsr_mfma3, k_dense_mfma3_lds), row-sequential (k_ell, the stencil)

Rows an operation does not write must come back zero, an in-place call leaves them as they went in.

The two problems of the complex64 file (host-built solver hierarchy, coarsening [(4, 8), (2, 8)], both fine levels
smoothed even-odd):

  schwinger16       levels 512 / 256 / 64.  Level 1: RT = 16, KS = 20, RB = 4: (RB & 7) != 0 selects block map 0
                    whatever bsr_map says; KS = 20 is the tail of the 8-stage pipelines.  Even-odd operators with
                    KS = 28 / 16 / 4 / 16 (KS = 4: fewer k-steps than an 8-stage prologue loads).  Coarsest inverse
                    64^2 (KS = 16: below the 32 k-steps k_dense_mfma3_lds needs, it stays on k_bsr_mfma3).  The
                    lattice tiles wrap the torus.
  synthetic 32^2    levels 2048 / 1024 / 256, direct_levels = [1].  Level 1: RT = 64, RB = 16, RB / 8 = 2: bsr_map 1,
                    2 and 3 take their own paths, bsr_sub 1 and 2 reach the sub-band order of map 2, bsr_sub 8 falls
                    back to map 1.  Even-odd operators: RT = 32, RB = 8, RB / 8 = 1, KS = 36 / 16 / 4 / 16.  Dense
                    Schur inverse 512^2 (RT = 32, KS = 128), coarsest inverse 256^2 (RT = 16, KS = 64, RB = 4).

Batch widths nb = 3 (nbp = 64: one 64-probe chunk), 70 (nbp = 128) and, for the block maps, 130 (nbp = 192: an
odd number of chunks).

Instantiations reached:
  k_bsr_mfma<MODE, NT, NTIO, STG>    all 36: MODE 0, 1, 3 x NT 2, 4 (mfma_small_tiles 2, 4, and 0 with mfma_tiles 2, 4)
                                     x NTIO (bsr_nt) x STG 2, 4, 8 on A and the even-odd operators (STG 8 only
                                     where KS % 8 == 0: KS = 16; KS = 20, 28, 36, 4 fall back to 4 stages in the
                                     launcher); xreg 0, 1 in MODE 3 at 4 stages; the dense operators with
                                     dense_stages 2, 4, 8 (NTIO = 0); maps 0..3 x bsr_sub 1, 2, 8; dense_map 0..3
  k_bsr_mfma3<MODE, NT, NTIO, STG>   STG = 4: MODE 0, 1, 3 x NT 1, 2, 4 (mfma3_tiles; 0 picks 1) x NTIO 0, 1;
                                     STG = 8: MODE 0, NTIO 0, NT 1, 2, 4 on KS = 20, 36, 28, 4, 16 (the in-kernel
                                     tail) and on the dense operators; STG = 16: the dense operators (NT 1);
                                     xreg 0, 1 in MODE 3; the in-place MODE 1 call of even-odd operator 3; maps as above
  k_dense_mfma3_lds<RTW, 4>          RTW 2, 4 on the Schur inverse 512^2 and the coarsest inverse 256^2
  k_ell<G, MODE, cplx>               use_mfma = 0 and mfma_ops = 0: G = 16 in MODE 0, 1, 3 (level 1, K = 80 on
                                     both problems), G = 16 MODE 0 (the coarsest inverse, K = 64 / 256, with
                                     use_mfma = 0), the transfers in MODE 0 with the (G, K) the packer chose -- the
                                     test records them in its report.  NOT reached: MODE 2 (Y = B + op X, the
                                     prolongation onto an existing iterate: no `which` code has it; the cycle of a
                                     hierarchy with pre-smoothing runs it), G = 1 and 2 (no operator of these two
                                     hierarchies packs to them), and MODE 1, 3 at any G other than the level
                                     operator's
  k_stencil<MODE, SPW, cplx, cplx>   all 12: MODE 0, 1, 2 (ABI mode 3) x SPW 1, 2, 4, 8 x stencil_tile 0, 4, 8
                                     (16^2; a tile of 4 caps the window at 4) / 0, 8, 16 (32^2) x stencil_nt 0, 1.  The
                                     complex64-input instantiations (CI = cplxf) belong to the complex64 file.

Figures measured on an MI355X are in DESIGN.md, "Per-kernel parity of the fp64 operator kernels"; every assertion
message carries its own.
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import engine as EN  # noqa: E402
from deflatedmlmc_schwinger_amd import gateway, hierarchy, matrix  # noqa: E402
from deflatedmlmc_schwinger_amd.multigrid import MG, SOLVER_HID  # noqa: E402
from oracle import f64_bounds as fb  # noqa: E402

OPTIONS = ("use_mfma", "mfma_ops", "mfma_3m", "mfma_tiles", "mfma_small_tiles", "mfma3_tiles", "bsr_stages",
           "dense_stages", "bsr_nt", "bsr_xreg", "bsr_map", "dense_map", "bsr_sub", "dense_lds", "stencil_spw",
           "stencil_tile", "stencil_nt", "ell_order", "p_even")
NU0, NU1 = 4, 3
W = 0.37 - 0.21j
NBMAX = 130
STENCIL_K = 9       # a row of the Wilson operator: its own entry and four neighbours x two spins
EO_OPS = ("eo0", "eo1", "eo2", "eo3")


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


class Problem:
    """One lattice with its host-built three-level solver hierarchy on the GPU and, on the host, the float64
    values of every operator the fp64 cycle applies, with their double-double products (computed once)."""

    def __init__(self, A, direct):
        cfg = dict(hierarchy.DEFAULT_SOLVER_CFG, coarsening=[(4, 8), (2, 8)], cycle=[(0, NU0, 0), (0, NU1, 0)],
                   eo_levels=[0, 1])
        if direct:
            cfg["direct_levels"] = [1]
        self.mg = MG(A)
        self.mg.setup_solver_only(cfg)
        self.eng = eng = self.mg.engine
        sh = self.mg.solver_hier
        self.L, mass, U1, U2 = self.mg.lattice
        self.n = [a.shape[0] for a in sh["A"]]
        self.defaults = {k: eng.get_option(k) for k in OPTIONS}
        kcol, vals = eng.level_bsr(SOLVER_HID, 1)
        self.block = {"A": (np.arange(kcol.shape[0], dtype=np.int32), kcol, vals)}
        w1, ops = hierarchy.upload_coarse_eo([eng], SOLVER_HID, 1, sh["A"][1], self.L // 4, NU1)
        if "packed" in ops:
            packed = ops["packed"]
        else:       # fewer than 8 x 8 coarse sites: the general construction (as upload_coarse_eo packs it)
            packed = [hierarchy.block_rows_from_matrix(ops[k], ops[s], self.n[1])
                      for k, s in (("S", "E_sites"), ("F", "E_sites"), ("G", "O_sites"), ("Hb", "O_sites"))]
        for q, pk in enumerate(packed):
            self.block["eo%d" % q] = pk
        self.dense = {"cinv": fb.pack_dense(np.asarray(sh["coarsest_inv"]))}
        if direct:
            pk = hierarchy.dense_schur_inverse_blocks(ops)
            eng.set_eo_operator(SOLVER_HID, 1, 4, *pk)
            self.dense["eo4"] = pk
        self.E1 = ops["E_rows"]
        self.P = [sp.csr_matrix(p).astype(np.complex128) for p in sh["P"]]
        # the lattice level: the Wilson operator from the links the engine holds (entries: links and 4 + mass, exact)
        Aw = hierarchy.wilson_from_links(U1, U2, self.L)
        _, self.E0, self.O0, _ = hierarchy.schur_complement(Aw, self.L)
        self.A0 = sp.csr_matrix(sh["A"][0]).astype(np.complex128)
        self._products, self._cache = {}, {}

    def restore(self):
        for k, v in self.defaults.items():
            self.eng.set_option(k, v)

    def set(self, **options):
        for k, v in options.items():
            self.eng.set_option(k, v)

    def operator(self, name):
        return self.block[name] if name in self.block else self.dense[name]

    def product(self, name):
        """(X, B, op X in double-double, |op| |X|, rows, M) on NBMAX columns (70 for the dense operators): narrower
        batches use the first columns"""
        if name not in self._products:
            nbmax = 70 if name in self.dense else NBMAX
            if name == "A0":
                n, M = self.n[0], self.A0
                seed = 4000
                X, B = _rand((n, 70), seed), _rand((n, 70), seed + 1)
                AX, rows = fb.dd_rows(M, X), np.arange(n)
            else:
                tmap, kcol, vals = self.operator(name)
                n = self.n[2] if name == "cinv" else self.n[1]
                seed = 1000 + sum(map(ord, name))
                X, B = _rand((n, nbmax), seed), _rand((n, nbmax), seed + 1)
                M = fb.packed_matrix(tmap, kcol, vals, n)
                AX, rows = fb.dd_block_rows(tmap, kcol, vals, X)
            self._products[name] = (X, B, AX, fb.abs1_matrix(M) @ fb.abs1(X), rows, M)
        return self._products[name]

    def reference(self, name, nb, mode, form, in_place=False):
        """(X, B, y_ref, its low part, S, rows, c_ref, K) of an operator on nb columns in a mode; form: "4m" / "3m"
        block rows, "rows": row-sequential; in_place: B = X"""
        key = (name, nb, mode, form, in_place)
        if key not in self._cache:
            X, B, AX, S_ax, rows, M = self.product(name)
            X, B, AX, S_ax = X[:, :nb], B[:, :nb], AX[:, :nb], S_ax[:, :nb]
            if in_place:
                B = X
            ref, low, S = fb.mode_reference(AX, S_ax, X, B, mode, W)
            if form == "rows":
                emu = fb.emulate_rows(M, X, B, mode, W)
                K = STENCIL_K if name == "A0" else None
            else:
                tmap, kcol, vals = self.operator(name)
                emu = fb.emulate_block_rows(tmap, kcol, vals, X, B, mode, W, form=form)
                K = 4 * kcol.shape[1]
            self._cache[key] = (X, B, ref, low, S, rows, fb.error_ratio(emu, ref, S, rows, low), K)
        return self._cache[key]


@pytest.fixture(scope="module")
def p16():
    params = gateway.set_params('schwinger16')
    return Problem(matrix.loadMatrix(params['matrix'], params['matrix_params']), direct=False)


@pytest.fixture(scope="module")
def p32():
    return Problem(matrix.synthetic_matrix(32, 0.05, sigma=0.3, seed=132), direct=True)


WHICH = {"A": EN.OP32_A, "A0": EN.OP32_A, "cinv": EN.OP32_COARSEST}
WHICH.update({"eo%d" % q: EN.OP32_EO0 + q for q in range(5)})
LEVEL = {"A0": 0, "cinv": 2}


class Report:
    def __init__(self):
        self.lines, self.ok = [], []

    def add(self, label, c_ref, r, K, good=True):
        self.lines.append("%s: c_ref %.2f kernel %.2f (tight limit %.1f, hard limit %d)"
                          % (label, c_ref, r, fb.tight_limit(c_ref), fb.hard_limit(K)))
        print(self.lines[-1])
        self.ok.append(bool(good and r <= fb.tight_limit(c_ref) and r <= fb.hard_limit(K)))

    def finish(self):
        bad = [line for line, good in zip(self.lines, self.ok) if not good]
        assert self.lines and not bad, "\n".join(["over the limit:"] + bad + ["all figures:"] + self.lines)


def _check(p, name, nb, mode, form, label, report, in_place=False, ell=False):
    """one launch of an operator against its reference: both limits, unwritten rows; the figures go into `report`.
    ell: the launch must have gone through the grouped-ELL form, whose K it reports"""
    X, B, ref, low, S, rows, c_ref, K = p.reference(name, nb, mode, form, in_place)
    Y, info = p.eng.apply_op64(SOLVER_HID, LEVEL.get(name, 1), WHICH[name], X.T.copy(),
                               None if (mode == 0 or in_place) else B.T.copy(), mode=mode, w=W, in_place=in_place)
    Y = Y.T
    if ell:
        assert info[2] > 0 and info[3] > 0, (label, info)
        K = info[3]
        label += " (G %d, K %d)" % (info[2], K)
    elif name != "A0":
        assert info[1] * 4 == K, (label, info)
    other = np.ones(Y.shape[0], dtype=bool)
    other[rows] = False
    unwritten = np.array_equal(Y[other], X[other]) if in_place else not Y[other].any()
    report.add(label, c_ref, fb.error_ratio(Y, ref, S, rows, low), K, unwritten)


def _tile_settings():
    """(label, options) reaching NT = 2 and NT = 4 of k_bsr_mfma both ways: through mfma_tiles (the small-operator
    override off) and through mfma_small_tiles (which applies at these sizes)"""
    return [("tiles %d small 0" % t, dict(mfma_small_tiles=0, mfma_tiles=t)) for t in (2, 4)] + \
           [("small %d" % t, dict(mfma_small_tiles=t, mfma_tiles=6 - t)) for t in (2, 4)]


@pytest.mark.parametrize("prob", ["p16", "p32"])
def test_four_product_kernel_every_variant(prob, request):
    """k_bsr_mfma<MODE, NT, NTIO, STG> (mfma_3m = 0) on the level operator and the even-odd operators: modes 0, 1, 3 x
    NT 2, 4 (both ways) x bsr_nt 0, 1 x bsr_stages 2, 4, 8 x nb 3, 70; bsr_xreg 0, 1 in mode 3 at 4 stages; the
    in-place mode-1 call of even-odd operator 3"""
    p = request.getfixturevalue(prob)
    rep = Report()
    try:
        p.set(mfma_3m=0)
        for tl, topt in _tile_settings():
            p.set(**topt)
            for nt in (0, 1):
                for stages in (2, 4, 8):
                    p.set(bsr_nt=nt, bsr_stages=stages, bsr_xreg=1)
                    for nb in (3, 70):
                        for name in ("A",) + EO_OPS:
                            for mode in (0, 1, 3):
                                label = "%s %s mode %d %s nt %d stages %d nb %d" % (prob, name, mode, tl, nt, stages, nb)
                                _check(p, name, nb, mode, "4m", label, rep)
                        _check(p, "eo3", nb, 1, "4m", "%s eo3 in place %s nt %d stages %d nb %d"
                               % (prob, tl, nt, stages, nb), rep, in_place=True)
                p.set(bsr_nt=nt, bsr_stages=4, bsr_xreg=0)
                for nb in (3, 70):
                    for name in ("A",) + EO_OPS:
                        _check(p, name, nb, 3, "4m", "%s %s mode 3 %s nt %d stages 4 xreg 0 nb %d"
                               % (prob, name, tl, nt, nb), rep)
    finally:
        p.restore()
    rep.finish()


@pytest.mark.parametrize("prob", ["p16", "p32"])
def test_three_product_kernel_every_variant(prob, request):
    """k_bsr_mfma3<MODE, NT, NTIO, STG>: modes 0, 1, 3 x mfma3_tiles 0, 1, 2, 4 x bsr_nt 0, 1 at 4 stages, bsr_xreg 0, 1 in
    mode 3, the in-place mode-1 call of even-odd operator 3; mode 0 with bsr_nt = 0 and bsr_stages = 8: the 8-stage
    instantiation with its in-kernel tail on KS = 20, 36 / 28, 4 (and 16, no tail)"""
    p = request.getfixturevalue(prob)
    rep = Report()
    try:
        p.set(mfma_3m=1, dense_lds=0)
        for tiles in (0, 1, 2, 4):
            for nt in (0, 1):
                p.set(mfma3_tiles=tiles, bsr_nt=nt, bsr_stages=4)
                for nb in (3, 70):
                    for name in ("A",) + EO_OPS:
                        for mode in (0, 1, 3):
                            for xreg in ((0, 1) if mode == 3 else (1,)):
                                p.set(bsr_xreg=xreg)
                                label = ("%s %s mode %d tiles3 %d nt %d xreg %d nb %d"
                                         % (prob, name, mode, tiles, nt, xreg, nb))
                                _check(p, name, nb, mode, "3m", label, rep)
                    _check(p, "eo3", nb, 1, "3m", "%s eo3 in place tiles3 %d nt %d nb %d" % (prob, tiles, nt, nb), rep,
                           in_place=True)
            p.set(bsr_nt=0, bsr_stages=8)
            for nb in (3, 70):
                for name in ("A",) + EO_OPS:
                    KS = p.block[name][1].shape[1]
                    _check(p, name, nb, 0, "3m", "%s %s (KS %d) mode 0 tiles3 %d 8 stages nb %d"
                           % (prob, name, KS, tiles, nb), rep)
    finally:
        p.restore()
    rep.finish()


@pytest.mark.parametrize("prob", ["p16", "p32"])
def test_dense_operators(prob, request):
    """the coarsest inverse and the dense Schur inverse (mode 0): k_bsr_mfma with dense_stages 2, 4, 8 and NT 2, 4;
    k_bsr_mfma3 (dense_lds = 0) with dense_stages 4, 8, 16 and mfma3_tiles 0, 1, 2, 4; k_dense_mfma3_lds with
    dense_lds 2, 4; dense_map 0..3 in the first two"""
    p = request.getfixturevalue(prob)
    rep = Report()
    try:
        for nb in (3, 70):
            for name in sorted(p.dense):
                p.set(mfma_3m=0)
                for tl, topt in _tile_settings():
                    p.set(**topt)
                    for stages in (2, 4, 8):
                        p.set(dense_stages=stages, dense_map=0)
                        _check(p, name, nb, 0, "4m", "%s %s four products %s dense stages %d nb %d"
                               % (prob, name, tl, stages, nb), rep)
                for dmap in (1, 2, 3):
                    for sub in (1, 2, 8):
                        p.set(dense_map=dmap, bsr_sub=sub, dense_stages=8)
                        _check(p, name, nb, 0, "4m", "%s %s four products dense map %d sub %d nb %d"
                               % (prob, name, dmap, sub, nb), rep)
                p.set(mfma_3m=1, dense_lds=0, bsr_sub=p.defaults["bsr_sub"])
                for tiles in (0, 1, 2, 4):
                    for stages in (4, 8, 16):
                        p.set(mfma3_tiles=tiles, dense_stages=stages, dense_map=0)
                        _check(p, name, nb, 0, "3m", "%s %s three products tiles3 %d dense stages %d nb %d"
                               % (prob, name, tiles, stages, nb), rep)
                p.set(mfma3_tiles=0)
                for dmap in (1, 2, 3):
                    for sub in (1, 2, 8):
                        for stages in (4, 16):
                            p.set(dense_map=dmap, bsr_sub=sub, dense_stages=stages)
                            _check(p, name, nb, 0, "3m", "%s %s three products dense map %d sub %d stages %d nb %d"
                                   % (prob, name, dmap, sub, stages, nb), rep)
                p.set(dense_map=0, bsr_sub=p.defaults["bsr_sub"], dense_stages=8)
                for lds in (2, 4):
                    p.set(dense_lds=lds)
                    _check(p, name, nb, 0, "3m", "%s %s dense_lds %d nb %d" % (prob, name, lds, nb), rep)
    finally:
        p.restore()
    rep.finish()


def test_block_maps(p32):
    """bsr_map 0..3 x bsr_sub 1, 2, 8 in both MFMA kernels on level 1 (RB / 8 = 2: the sub-band order of map 2 with
    bsr_sub 1 and 2, its fall-back to map 1 with 8) and on the even-odd operators (RB / 8 = 1) of the 32^2 problem,
    nb = 70 (two or eight chunks) and 130 (an odd count): a wrong map computes one (row block, chunk) twice and
    leaves another zero"""
    p = p32
    rep = Report()
    try:
        for m3, form in ((0, "4m"), (1, "3m")):
            p.set(mfma_3m=m3, dense_lds=0)
            for bmap in (0, 1, 2, 3):
                for sub in (1, 2, 8):
                    p.set(bsr_map=bmap, bsr_sub=sub)
                    for nb in (70, 130):
                        for name in ("A",) + EO_OPS:
                            for mode in (0, 1, 3):
                                label = "p32 %s mode %d %s map %d sub %d nb %d" % (name, mode, form, bmap, sub, nb)
                                _check(p, name, nb, mode, form, label, rep)
    finally:
        p.restore()
    rep.finish()


@pytest.mark.parametrize("prob", ["p16", "p32"])
def test_grouped_ell_kernel(prob, request):
    """k_ell<G, MODE, cplx>: with use_mfma = 0 and again with mfma_ops = 0 the level-1 operator in modes 0, 1, 3 and
    the coarsest inverse (use_mfma = 0; mfma_ops = 0 leaves it on the matrix cores); R, P, P onto the even sites
    on both fine levels and Re (the restriction from the even sites' columns, which only the lattice level has) with
    ell_order 0, 1; p_even = 0 refuses P_EVEN"""
    p = request.getfixturevalue(prob)
    rep = Report()
    seen = set()
    evens = {0: p.E0, 1: p.E1}
    try:
        for off in ("use_mfma", "mfma_ops"):
            p.restore()
            p.set(**{off: 0})
            for nb in (3, 70):
                for mode in (0, 1, 3):
                    _check(p, "A", nb, mode, "rows", "%s A mode %d %s 0 nb %d" % (prob, mode, off, nb), rep, ell=True)
                form, ell = ("rows", True) if off == "use_mfma" else ("3m", False)
                p.set(dense_lds=0)
                _check(p, "cinv", nb, 0, form, "%s cinv %s 0 nb %d" % (prob, off, nb), rep, ell=ell)
            for order in (0, 1):
                p.set(ell_order=order)
                for level in (0, 1):
                    P = p.P[level]
                    R = sp.csr_matrix(P.conj().T)
                    for nb in (3, 70):
                        Xf, Xc = _rand((p.n[level], nb), 50 + level + nb), _rand((p.n[level + 1], nb), 60 + level + nb)
                        Xe = np.zeros_like(Xf)
                        Xe[evens[level]] = Xf[evens[level]]
                        cases = [("R", EN.OP32_R, R, Xf, Xf, None), ("P", EN.OP32_P, P, Xc, Xc, None),
                                 ("P even", EN.OP32_P_EVEN, P, Xc, Xc, evens[level])]
                        if level == 0:
                            cases.append(("Re", EN.OP32_RE, R, Xf, Xe, None))     # the odd entries of Xf must not be read
                        for label, which, M, Xin, Xref, rows in cases:
                            key = (label, level, nb)
                            if key not in p._cache:
                                dd = fb.dd_rows(M, Xref)
                                S = fb.abs1_matrix(M) @ fb.abs1(Xref)
                                c = fb.error_ratio(fb.emulate_rows(M, Xref), dd.rounded(), S, rows, dd.low())
                                p._cache[key] = (dd.rounded(), dd.low(), S, c)
                            ref, low, S, c_ref = p._cache[key]
                            Y, info = p.eng.apply_op64(SOLVER_HID, level, which, Xin.T.copy())
                            Y = Y.T
                            G, K = info[2], info[3]
                            seen.add((label, level, G, K))
                            good = K > 0
                            if rows is not None:
                                other = np.ones(Y.shape[0], dtype=bool)
                                other[rows] = False
                                good = good and not Y[other].any()
                            rep.add("%s %s level %d nb %d %s 0 ell_order %d (G %d, K %d)"
                                    % (prob, label, level, nb, off, order, G, K), c_ref,
                                    fb.error_ratio(Y, ref, S, rows, low), max(K, 1), good)
        p.set(p_even=0)
        with pytest.raises(EN.EngineError, match="no even-sites-only prolongation"):
            p.eng.apply_op64(SOLVER_HID, 0, EN.OP32_P_EVEN, _rand((2, p.n[1]), 3))
    finally:
        p.restore()
    print("group sizes:", sorted(seen))
    rep.finish()


@pytest.mark.parametrize("prob", ["p16", "p32"])
def test_stencil_every_variant(prob, request):
    """k_stencil<MODE, SPW>: modes 0, 1, 3 (the stencil's mode 2) x stencil_spw 1, 2, 4, 8 x stencil_tile 0, L / 4, L / 2
    (4, 8 on 16^2: a tile of 4 caps the window at 4; 8, 16 on 32^2) x stencil_nt 0, 1 x nb 3, 70, against the Wilson
    operator of the problem in double-double: the window's left neighbour, link and wrap at x = 0 and x = L - 1 sit
    inside a tile walk"""
    p = request.getfixturevalue(prob)
    rep = Report()
    try:
        for spw in (1, 2, 4, 8):
            for tile in (0, p.L // 4, p.L // 2):
                for nt in (0, 1):
                    p.set(stencil_spw=spw, stencil_tile=tile, stencil_nt=nt)
                    for nb in (3, 70):
                        for mode in (0, 1, 3):
                            label = "%s stencil mode %d spw %d tile %d nt %d nb %d" % (prob, mode, spw, tile, nt, nb)
                            _check(p, "A0", nb, mode, "rows", label, rep)
    finally:
        p.restore()
    rep.finish()


def test_apply_op64_argument_errors(p16):
    eng = p16.eng
    X = _rand((2, p16.n[1]), 1)
    for kwargs in (dict(which=99), dict(which=EN.OP32_A, mode=2), dict(which=EN.OP32_R, mode=1),
                   dict(which=EN.OP32_A, mode=1), dict(which=EN.OP32_A, mode=3, in_place=True, B=X),
                   dict(which=EN.OP32_A, mode=0, in_place=True), dict(which=EN.OP32_EO0 + 4),
                   dict(which=EN.OP32_COARSEST)):
        with pytest.raises(EN.EngineError):
            eng.apply_op64(SOLVER_HID, 1, kwargs.pop("which"), X, **kwargs)
    X0 = _rand((2, p16.n[0]), 2)
    for which in (EN.OP32_SCHUR, EN.OP32_EO_SMOOTH, EN.OP32_EO_SMOOTH_REDUCED):
        with pytest.raises(EN.EngineError, match="not available"):
            eng.apply_op64(SOLVER_HID, 0, which, X0, B=X0)
    with pytest.raises(EN.EngineError):          # the stencil reads its neighbours' rows: no in-place form
        eng.apply_op64(SOLVER_HID, 0, EN.OP32_A, X0, mode=1, in_place=True)
    with pytest.raises(EN.EngineError):
        eng.apply_op64(SOLVER_HID, 0, EN.OP32_A, X0, mode=3)          # mode 3 needs B
    with pytest.raises(EN.EngineError):
        eng.apply_op64(SOLVER_HID, 2, EN.OP32_R, _rand((2, p16.n[2]), 3))     # no transfer at the coarsest level
