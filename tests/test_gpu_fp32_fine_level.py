"""The FP32 fine level kernel by kernel against long double (fp32_reference.py: reference, bound and the counted constants).

Three kernel families in their float instances: the one-term matrix-free kernel (vmult, residual, both smoother epilogues, the
epilogue written over its own x_prev, the tail slab, every tile of test_mf_vmult_independent_of_tile), the multi-term sweep (two
and three terms, 2 / 3 / 4 rows per wavefront, D^-1 derived or stored, reference and mode-space arithmetic) and the one-pass
residual restriction on float vectors.  Inputs are float32 values, the reference is long double from them, the check is per
entry, |got - ref| <= k u mag with u = 2^-24; outputs are NaN before every launch.

Counted k (fp32_reference.py) and the worst |got - ref| / (u mag) observed on an MI355X over all cases of this module
(test_worst_ratios_observed prints them):
  one-term kernel   k = 16 (one coefficient per cell), 32 (eight; the 2-D kernel); smoother epilogues + 12     observed 3.5
  sweep             k = 16 + 12 per term, propagated through the recurrence                                   observed 3.3
  restriction       all arithmetic FP64 after the load: the bits of the FP64 entry; gamma_256 in 2^-53        observed 69

The 69 of the restriction is above a quarter of its k and belongs to one case, (20, 20, 20) with the entries of x and b spread
over 16 decades (4.6 at most on every other mesh, 1.8 there with plain normal inputs): a row is then dominated by one entry of x
times one table entry (R A)_im, and the table is made by the FP64 operator kernel, whose error is relative to B |v| (see
fp32_reference.py), not to the |A| |v| this magnitude is built from -- B has max|K_e| where the cell matrix of a cube has entries
a quarter of that and zeros.  It is the same figure for the FP64 entry (the two give the same bits), not a property of the float path.

Shapes are cells; DoFs are one more per direction.  With three halo lanes a full chunk column owns 58 node columns, and the
FP64 operator gives the rest to a narrow last column where it is 1 .. 29 wide.  The float operator does not (mf_laplace.hip:
its sweep was slower with it) -- it spreads the columns evenly, so the shapes named after their narrow column are here the
shapes at which the two instances cut the rows differently: 65 node columns are 33 + 32 in float, 117 are three chunks of 39."""
import functools

import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
import mfmg_oracle as O
import fp32_reference as F

pytestmark = pytest.mark.gpu

HALO = 3
LD = np.longdouble
AL = [0.0, 0.23, 0.31]
BE = [0.61, 0.87, 0.79]
ALF = [float(np.float32(v)) for v in AL]      # what the float entry points receive
BEF = [float(np.float32(v)) for v in BE]

MESHES = [(6, 5, 7), (20, 17, 9), (64, 18, 6), (64, 19, 6), (86, 19, 11), (115, 20, 8), (116, 20, 8)]
SWEEP_CASES = [(n, 0) for n in MESHES] + [((32, 24, 22), 4), ((32, 24, 22), 5)]          # (cells, z-tile: 0 = the sweep's choice)
DEGENERATE = [(1, 1, 1), (2, 1, 3), (1, 5, 1), (62, 1, 1), (63, 1, 1), (64, 2, 1), (125, 2, 1), (126, 1, 2)]
TAIL_SLAB = [(65, 70, 5), (128, 65, 4)]
ONE_TERM_TILES = [(1, 2, 1), (1, 5, 3), (2, 3, 8), (4, 4, 16), (8, 1, 2), (3, 2, 5), (4, 12, 2), (8, 5, 64), (0, 1, 1)]   # (nw, ty, tz)
SWEEP_TILES = [None, (8, 3, 5), (4, 3, 8), (2, 4, 7), (8, 2, 64), (1, 4, 3), (4, 4, 0)]

WORST = {"one-term": 0.0, "sweep": 0.0, "restriction": 0.0}


def _narrow_column(nx):
    full = 64 - 2 * HALO
    ncols = (nx + full - 1) // full
    rest = nx - (ncols - 1) * full
    return ncols >= 2 and 1 <= rest <= 32 - HALO


def _own_rows(nw, ty, n_terms):
    return nw * ty - 2 * n_terms + 1


def test_shapes_reach_the_edges_they_name():
    nx = {n: n[0] + 1 for n in MESHES}
    assert [_narrow_column(nx[n]) for n in MESHES] == [False, False, True, True, True, False, True]
    assert nx[(64, 18, 6)] == 58 + 7 and nx[(86, 19, 11)] == 58 + 29 and nx[(115, 20, 8)] == 2 * 58 and nx[(116, 20, 8)] == 2 * 58 + 1
    assert not _narrow_column(58 + 30)                                   # (29 is the widest narrow column)
    assert nx[(6, 5, 7)] < 58 and 6 < _own_rows(8, 3, 3) and not _narrow_column(33)
    # 19 node rows: one y-tile of 8 x 3 at three terms, two of 4 x 4 at two terms (13 owned rows); 20 rows: one tile and a row
    assert _own_rows(8, 3, 3) == 19 and _own_rows(4, 4, 2) == 13
    tiles = lambda ny, own: (ny + own - 1) // own
    assert tiles(19, 19) == 1 and tiles(19, 13) == 2 and tiles(20, 19) == 2
    # z-tiles of 4 and 5 layers: fill and drain shorter and longer than three terms, several tiles along z
    assert 4 < 2 * 3 - 1 <= 5 and tiles(23, 4) > 1 and tiles(23, 5) > 1
    # the only tile the sweep tests skip: one wavefront of four rows at three terms
    assert [(t, k) for t in SWEEP_TILES if t for k in (2, 3) if _own_rows(t[0], t[1], k) < 1] == [((1, 4, 3), 3)]


# ---- problems and references (one per mesh and material, shared by the tests) ----
def _problem(n, material):
    if material == "cellwise":         # one coefficient per cell in [0.5, 1.5), as _cellwise_problem of test_gpu_kernels.py
        prob = M.LaplaceProblem(n, "constant", device="cuda")
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        prob.coefficient = (0.5 + torch.rand(prob.n_cells_total, 1, dtype=torch.float64, device="cuda", generator=g)).expand(-1, 2 ** len(n)).contiguous()
        return prob
    return M.LaplaceProblem(n, material, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(n, material):
    prob = _problem(n, material)
    ref = F.Reference(n, prob.coefficient.cpu().numpy())
    rng = np.random.default_rng([len(material), *n])
    x, b, xp = (F.f32(rng.standard_normal(ref.n_dofs)) for _ in range(3))
    return prob, ref, x, b, xp


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


def _operator(ctx, prob, stored=False):
    ctx.set_stored_diagonal(stored)
    try:
        op = M.MatrixFreeLaplaceF32(ctx, prob)
    finally:
        ctx.set_stored_diagonal(False)
    return op


def _check(family, got, ref, unit, k, what):
    got = got.cpu().numpy()
    ratio = F.worst_ratio(got, ref, unit)
    WORST[family] = max(WORST[family], ratio if np.isfinite(ratio) else 0.0)
    print(f"{what}: worst |got - ref| / (u mag) = {ratio:.2f} (k = {k})")
    F.assert_within(got, ref, unit, k, what)


# ---- a. the one-term float kernel ----
def _one_term_outputs(ctx, op, x, b, xp):
    n = x.numel()
    out = [_nan(n) for _ in range(5)]
    op.vmult(out[0], x)
    op.residual(x, b, out[1])
    op.smoother_step(b, x, None, 0.0, BE[0], out[2])
    op.smoother_step(b, x, xp, AL[1], BE[1], out[3])
    out[4] = xp.clone()                                       # the momentum step written over its own x_prev
    op.smoother_step(b, x, out[4], AL[1], BE[1], out[4])
    ctx.synchronize()
    return out


def _one_term_references(ref, x, b, xp):
    ax = ref.vmult(x)
    first = ref.step(x, b, None, 0.0, BEF[0], ax=ax)
    mom = ref.step(x, b, xp, ALF[1], BEF[1], ax=ax)
    refs = [ax, ax - b.astype(LD), first, mom, mom]
    units = [ref.unit_vmult(x), ref.unit_residual(x, b), ref.unit_step(x, b, None, 0.0, BEF[0]), ref.unit_step(x, b, xp, ALF[1], BEF[1])]
    return refs, units + [units[3]], [ref.k_op, ref.k_op + 1, ref.k_step, ref.k_step, ref.k_step]


OPS = ["vmult", "residual", "first-term step", "momentum step", "momentum step over its own x_prev"]


def _one_term_battery(ctx, op, case, what):
    """Every operation against the bound on the default tile; the same bits on every other tile."""
    prob, ref, x, b, xp = case
    xd, bd, xpd = _gpu(x), _gpu(b), _gpu(xp)
    base = _one_term_outputs(ctx, op, xd, bd, xpd)
    refs, units, ks = _one_term_references(ref, x, b, xp)
    for name, got, want, unit, k in zip(OPS, base, refs, units, ks):
        _check("one-term", got, want, unit, k, f"{what} {name}")
    # owner computes, in float as in double: no tile changes a bit
    for nw, ty, tz in ONE_TERM_TILES:
        op.set_tile(ty, tz, nw)
        for name, got, want in zip(OPS, _one_term_outputs(ctx, op, xd, bd, xpd), base):
            assert torch.equal(got, want), f"{what} tile {(nw, ty, tz)}: {name} differs from the default tile in {(got != want).sum().item()} entries"
    # D^-1: two roundings (the coefficients to float, the result) from the oracle's
    dinv = op.diagonal_inverse().cpu().numpy().astype(LD)
    assert not F.beyond(dinv, ref.dinv, 2 * F.U32 * ref.dinv).any(), f"{what}: D^-1 beyond 2 u"
    return base, refs, units, ks


@pytest.mark.parametrize("material", ["constant", "cellwise", "linear"])
@pytest.mark.parametrize("n", MESHES + [(32, 24, 22)] + DEGENERATE + TAIL_SLAB, ids=lambda v: "x".join(map(str, v)))
def test_one_term_kernel_every_epilogue_and_tile(ctx, n, material):
    case = _case(n, material)
    prob, ref, x, b, xp = case
    op = _operator(ctx, prob)
    cc = material != "linear"
    assert op.cell_constant_layout() == cc and op.diagonal_in_record() == (not cc)
    base, refs, units, ks = _one_term_battery(ctx, op, case, f"{n} {material}")
    if cc:
        # D^-1 kept in the records instead of derived in the kernel: the smoother steps within the same bound
        op_s = _operator(ctx, prob, stored=True)
        assert op_s.diagonal_in_record()
        stored = _one_term_outputs(ctx, op_s, _gpu(x), _gpu(b), _gpu(xp))
        for i in (2, 3, 4):
            _check("one-term", stored[i], refs[i], units[i], ks[i], f"{n} {material} {OPS[i]}, stored D^-1")
    if cc and n in TAIL_SLAB:
        # records with one halo lane (the layout of a context that runs one term per launch): the columns of the nearly empty
        # last chunk run as a rotated slab inside the same launch -- with three halo lanes the columns are spread evenly
        ctx.set_mf_fused_terms(1)
        try:
            op_1 = _operator(ctx, prob)
        finally:
            ctx.set_mf_fused_terms(3)
        assert not op_1.sweep_available(2)
        _one_term_battery(ctx, op_1, case, f"{n} {material} one halo lane (tail slab)")


@pytest.mark.parametrize("n,material", [((8, 8), "constant"), ((12, 7), "linear"), ((33, 5), "discontinuous"), ((1, 1), "constant")])
def test_one_term_kernel_in_two_dimensions(ctx, n, material):
    """The float constructor accepts a 2-D mesh (the plain kernel of the small reference meshes): every mode against the bound."""
    prob, ref, x, b, xp = _case(n, material)
    op = M.MatrixFreeLaplaceF32(ctx, prob)
    refs, units, ks = _one_term_references(ref, x, b, xp)
    for what, got, want, unit, k in zip(OPS, _one_term_outputs(ctx, op, _gpu(x), _gpu(b), _gpu(xp)), refs, units, ks):
        _check("one-term", got, want, unit, k, f"{n} {material} {what}")
    assert not F.beyond(op.diagonal_inverse().cpu().numpy().astype(LD), ref.dinv, 2 * F.U32 * ref.dinv).any()


# ---- b. the float sweep ----
def _sweep(ctx, op, al, be, b, x, with_prev):
    out, outp = _nan(b.numel()), (_nan(b.numel()) if with_prev else None)
    op.smoother_sweep(al, be, b, x, out, outp)
    ctx.synchronize()
    return out, outp


_DEFAULT_TILE_BITS = {}


@pytest.mark.parametrize("tile", SWEEP_TILES, ids=lambda t: "default" if t is None else "x".join(map(str, t)))
@pytest.mark.parametrize("n_terms", [2, 3])
@pytest.mark.parametrize("material", ["constant", "cellwise"])
@pytest.mark.parametrize("n,tz", SWEEP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"tz{v}")
def test_sweep_reference_bits_and_default_arithmetic_bound(ctx, n, tz, material, n_terms, tile):
    if tile is not None and _own_rows(tile[0], tile[1], n_terms) < 1:
        pytest.skip("tile smaller than its halo rows")
    prob, ref, x, b, _ = _case(n, material)
    xd, bd = _gpu(x), _gpu(b)
    al, be = AL[:n_terms], BE[:n_terms]
    its = ref.sweep(x, b, ALF[:n_terms], BEF[:n_terms])
    units = ref.unit_sweep(its, b, ALF[:n_terms], BEF[:n_terms])
    for stored in (False, True):
        op = _operator(ctx, prob, stored)
        assert op.sweep_available(n_terms) and op.diagonal_in_record() == stored
        # the terms as one launch each (the one-term float kernel, held to the bound above)
        terms = [xd]
        for k in range(n_terms):
            o = _nan(xd.numel())
            op.smoother_step(bd, terms[-1], terms[-2] if k > 0 else None, al[k], be[k], o)
            terms.append(o)
        nw, ty, t_z = tile if tile is not None else op.get_sweep_tile(n_terms)
        if tile is not None or tz:
            op.set_sweep_tile(nw, ty, tz or t_z)
            got_tile = op.get_sweep_tile(n_terms)
            assert got_tile[:2] == (nw, ty) and (not (tz or t_z) or got_tile[2] == (tz or t_z)), got_tile
        for with_prev in (True, False):
            op.set_sweep_reference(True)
            out, outp = _sweep(ctx, op, al, be, bd, xd, with_prev)
            assert torch.equal(out, terms[-1]), f"reference arithmetic: x_{n_terms} differs from the term-by-term sequence in {(out != terms[-1]).sum().item()} entries"
            assert outp is None or torch.equal(outp, terms[-2]), f"reference arithmetic: x_{n_terms - 1} differs from the term-by-term sequence"
            # the arithmetic production launches
            op.set_sweep_reference(False)
            out, outp = _sweep(ctx, op, al, be, bd, xd, with_prev)
            what = f"{n} tz {tz} {material} {n_terms} terms tile {tile} stored D^-1 {stored} out_prev {with_prev}"
            _check("sweep", out, its[-1], units[-1], ref.k_step, what + f": x_{n_terms}")
            if with_prev:
                _check("sweep", outp, its[-2], units[-2], ref.k_step, what + f": x_{n_terms - 1}")
            # ... does not depend on the tile, bit for bit: against the sweep's own choice on the same inputs
            key = (n, material, n_terms, stored)
            if key not in _DEFAULT_TILE_BITS:
                op0 = _operator(ctx, prob, stored)
                _DEFAULT_TILE_BITS[key] = _sweep(ctx, op0, al, be, bd, xd, True)
            assert torch.equal(out, _DEFAULT_TILE_BITS[key][0]), f"{what}: differs from the default tile in {(out != _DEFAULT_TILE_BITS[key][0]).sum().item()} entries"
            assert outp is None or torch.equal(outp, _DEFAULT_TILE_BITS[key][1]), f"{what}: x_{n_terms - 1} differs from the default tile"


def test_sweep_keeps_its_default_tile_when_asked_for_12_x_2_and_needs_a_guess(ctx):
    prob, ref, x, b, _ = _case((20, 17, 9), "cellwise")
    op = _operator(ctx, prob)
    assert op.get_sweep_tile(3)[:2] == (8, 3) and op.get_sweep_tile(2)[:2] == (4, 4)
    op.set_sweep_tile(12, 2, 0)
    assert op.get_sweep_tile(3)[:2] == (8, 3) and op.get_sweep_tile(2)[:2] == (4, 4)
    out, _ = _sweep(ctx, op, AL, BE, _gpu(b), _gpu(x), False)
    its = ref.sweep(x, b, ALF, BEF)
    _check("sweep", out, its[-1], ref.unit_sweep(its, b, ALF, BEF)[-1], ref.k_step, "(20, 17, 9) after a 12 x 2 request")
    # the sweep from a zero guess (x null) is FP64 only: the float entry refuses a null x
    with pytest.raises(L.MfmgInvalidArgument, match="null"):
        op.smoother_sweep(AL, BE, _gpu(b), None, _nan(b.size))
    for bad in ((9, 3, 4), (8, 5, 4), (12, 3, 4)):
        with pytest.raises(L.MfmgInvalidArgument, match="out of range"):
            op.set_sweep_tile(*bad)
    with pytest.raises(L.MfmgInvalidArgument, match="out of range"):
        op.set_tile(65, 1)
    with pytest.raises(L.MfmgInvalidArgument):
        op.set_tile(2, 2, 9)


# ---- c. the one-pass residual restriction on float vectors ----
RR_MESHES = [(n, "constant") for n in ((4, 4, 4), (66, 8, 6), (130, 6, 4), (12, 70, 6), (8, 6, 40), (20, 20, 20), (138, 8, 8))] \
    + [((4, 4, 4), "discontinuous"), ((20, 20, 20), "discontinuous")]
U64 = 2.0 ** -53
# the table entries (R A)_im: dot products of at most 27 entries of R with sums of cell entries, computed in FP64 by the operator
# kernel (at most 64 roundings behind one of them, see K_OP_GENERAL and twice that for the product with R), then the 125 + 27
# products and their sums and the final difference: 64 + 2 * 152 / 2 + ... < 256
K_RR = 256


def _hierarchy(ctx, n, material):
    params = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": False,
              "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}, "fine level precision": "float"}
    return M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", M.LaplaceProblem(n, material, device="cuda"), params)


def _spmv_long(Acoo, v):
    prod = Acoo.data.astype(LD) * v[Acoo.col]
    out, mag = np.zeros(Acoo.shape[0], dtype=LD), np.zeros(Acoo.shape[0], dtype=LD)
    np.add.at(out, Acoo.row, prod)
    np.add.at(mag, Acoo.row, np.abs(prod))
    return out, mag


@pytest.mark.parametrize("n,material", RR_MESHES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_residual_restriction_on_float_vectors(ctx, monkeypatch, n, material):
    """Both instances of the kernel widen x and b as they load them and do all arithmetic in FP64 in the same order
    (residual_restriction.hip: pair_of<TI> -> pair_of<double>): the float entry gives the bits of the FP64 entry on the widened
    vectors, under either kernel form, and R (A x - b) in long double within gamma_256 of |R| (|A| |x| + |b|) per row."""
    h = _hierarchy(ctx, n, material)
    monkeypatch.setenv("MFMG_RR_KERNEL", "rows")
    h_rows = _hierarchy(ctx, n, material)
    monkeypatch.delenv("MFMG_RR_KERNEL")
    assert h.residual_restriction_classes() > 0 and h_rows.residual_restriction_classes() > 0
    nf, nc = h.level_size(0), h.level_size(1)
    mesh = O.StructuredMesh(n)
    con = mesh.constrained_mask()
    A = O.assemble_csr(mesh, O.coefficient_table(mesh, material)).tolil()
    A.setdiag(np.where(con, 1.0, A.diagonal()))               # matrix-free rule: constrained rows are identities
    A, R = A.tocoo(), h.restrictor().to_scipy().tocoo()
    rng = np.random.default_rng(5)
    for scale in (False, True):
        x, b = rng.standard_normal(nf), rng.standard_normal(nf)
        if scale:                                             # entries over 16 decades
            x, b = x * 10.0 ** rng.uniform(-8, 8, nf), b * 10.0 ** rng.uniform(-8, 8, nf)
        x, b = F.f32(x), F.f32(b)
        xd, bd = _gpu(x), _gpu(b)
        out = [torch.full((nc,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
        h.restrict_residual_f32(xd, bd, out[0])
        h.restrict_residual(xd.double(), bd.double(), out[1])
        h_rows.restrict_residual_f32(xd, bd, out[2])
        ctx.synchronize()
        assert torch.equal(out[0], out[1]), f"{n} {material}: differs from the FP64 entry on the widened vectors in {(out[0] != out[1]).sum().item()} rows"
        assert torch.equal(out[0], out[2]), f"{n} {material}: differs from MFMG_RR_KERNEL=rows in {(out[0] != out[2]).sum().item()} rows"
        ax, amag = _spmv_long(A, x.astype(LD))
        want, _ = _spmv_long(R, ax - b.astype(LD))
        _, mag = _spmv_long(R, amag + np.abs(b).astype(LD))
        got = out[0].cpu().numpy()
        ratio = F.worst_ratio(got, want, U64 * mag)
        WORST["restriction"] = max(WORST["restriction"], ratio)
        print(f"{n} {material} scaled {scale}: worst |got - ref| / (2^-53 mag) = {ratio:.2f} (k = {K_RR})")
        bad = F.beyond(got, want, K_RR * U64 / (1 - K_RR * U64) * mag)
        assert not bad.any(), f"{n} {material}: {int(bad.sum())} rows beyond gamma_{K_RR}, first at {np.flatnonzero(bad)[:5]}"


def test_residual_restriction_on_float_vectors_is_refused_where_the_form_is_not_built(ctx):
    h = _hierarchy(ctx, (9, 7, 5), "constant")
    assert h.residual_restriction_classes() == 0
    nf, nc = h.level_size(0), h.level_size(1)
    x = torch.zeros(nf, dtype=torch.float32, device="cuda")
    with pytest.raises(L.MfmgNotImplementedError):
        h.restrict_residual_f32(x, x.clone(), torch.zeros(nc, dtype=torch.float64, device="cuda"))


def test_worst_ratios_observed():
    """(runs last: what the cases above measured, for the figures of the module docstring)"""
    print("worst |got - ref| / (u mag) per family: " + ", ".join(f"{k} {v:.2f}" for k, v in WORST.items()))
