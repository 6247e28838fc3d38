"""The FP64 fine level kernel by kernel against long double (fp32_reference.py with u = 2^-53: reference, bound and the counted
constants; test_fp64_bound_bites.py shows on the CPU that the bound notices planted errors which 1e-12 of the max-norm lets pass).

Two kernel families in their double instances: the one-term matrix-free kernel (vmult, residual, both smoother epilogues, the
epilogue written over its own x_prev, D^-1 derived or stored, the tail slab, a random numbering, the 2-D kernel, the interior and
shell launches of a distributed rank) and the multi-term sweep (two and three terms; 12 x 2, the default of three terms with a
derived D^-1, 8 x 3, 4 x 4 and other tiles; the body of a narrow last chunk column beside one, two and three y-tiles; from a
vector and from the zero guess; reference and mode-space arithmetic).  Inputs are doubles spread over six decades, signed; the
reference is long double from them; the check is per entry, |got - ref| <= (k + k_ref) u mag with u = 2^-53 and k_ref = 0.047 for
the reference's own roundings at 2^-64; outputs are NaN before every launch.

Counted k (fp32_reference.py) and the worst |got - ref| / (u mag) observed on an MI355X over all cases of this module
(test_worst_ratios_observed prints them; documentation, not thresholds):
  one-term kernel   k = 16 (one coefficient per cell), 32 (eight; the 2-D kernel); smoother epilogues + 12     observed 10.1
  sweep             k = 16 + 12 per term, propagated through the recurrence                                   observed 8.9
  sweep from zero   the same k, the recurrence started at x_0 = 0                                             observed 7.3

Shapes are cells; DoFs are one more per direction.  With three halo lanes a full chunk column owns 58 node columns, and the FP64
operator gives the rest to a narrow last column where it is 1 .. 29 wide: the sweeps of 8 x 3 and 12 x 2 (three terms) and 4 x 4
(two terms) run it with a body of its own, two y-tiles per workgroup (NARROW_TOO) -- in mode space; the 12 x 2 kernel of the
reference arithmetic has no such body.  Every other tile runs that column with ordinary tiles."""
import functools

import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
import mfmg_oracle as O
import fp32_reference as F
from test_gpu_fp32_fine_level import MESHES, DEGENERATE, TAIL_SLAB, ONE_TERM_TILES, SWEEP_TILES, HALO, _narrow_column, _own_rows
from test_gpu_fp32_fine_level import SWEEP_CASES as SWEEP_CASES_F32

pytestmark = pytest.mark.gpu

LD = np.longdouble
AL = [0.0, 0.23, 0.31]
BE = [0.61, 0.87, 0.79]
MATERIALS = ["constant", "cellwise", "cellwise6", "linear", "discontinuous"]
SWEEP_MATERIALS = ["constant", "cellwise", "cellwise6"]
# the shapes of test_gpu_sweep_12x2.py that the float module does not have: 39 and 40 node rows (three y-tiles of 19 owned rows
# beside the narrow column: a full pair and a half-idle one), 79 node columns
SWEEP_CASES = SWEEP_CASES_F32 + [((64, 38, 6), 0), ((78, 39, 8), 0)]
# narrow last chunk column: (node columns in it, y-tiles of the three-term sweep beside it)
NARROW = {(64, 18, 6): (7, 1), (64, 19, 6): (7, 2), (86, 19, 11): (29, 2), (116, 20, 8): (1, 2), (64, 38, 6): (7, 3), (78, 39, 8): (21, 3)}
ONE_TERM_OTHER_TILES = [(2, 3, 8), (3, 2, 5)]                 # (nw, ty, tz) of ONE_TERM_TILES, for bit equality with the default tile
# tiles of the sweep beside the default: what each path offers, and three more of SWEEP_TILES
TILES_3_DERIVED = [None, (8, 3, 0), (12, 2, 0), (4, 3, 8), (2, 4, 7), (8, 2, 64)]
TILES_3_STORED = [None, (8, 3, 5), (4, 3, 8), (2, 4, 7), (8, 2, 64)]
TILES_2 = [None, (4, 4, 0), (8, 3, 5), (2, 4, 7), (8, 2, 64)]

WORST = {"one-term": 0.0, "sweep": 0.0, "sweep from zero": 0.0}


def _y_tiles(ny, own):
    return (ny + own - 1) // own


def _offers_zero_guess(n_terms, tile):
    """fused_zero_guess_available of the operator: three terms in mode space, three rows per wavefront or twelve wavefronts of two."""
    return n_terms == 3 and (tile[1] == 3 or tile[:2] == (12, 2))


def test_shapes_reach_the_edges_they_name():
    assert np.finfo(LD).nmant >= 63
    cases = [n for n, _ in SWEEP_CASES]
    # node columns and rows of test_gpu_sweep_12x2.py, and 87 = 58 + 29 columns, the widest narrow column
    assert {65, 79, 116, 117, 87} <= {n[0] + 1 for n in cases} and {19, 20, 39, 40} <= {n[1] + 1 for n in cases}
    assert {tz for _, tz in SWEEP_CASES} == {0, 4, 5}
    full = 64 - 2 * HALO
    for n in set(cases):
        nx, ny = n[0] + 1, n[1] + 1
        assert _narrow_column(nx) == (n in NARROW), n
        if n in NARROW:
            assert NARROW[n] == (nx - (nx - 1) // full * full, _y_tiles(ny, _own_rows(12, 2, 3))), n
    # the narrow body runs beside one, two and three y-tiles (12 x 2 and 8 x 3 own the same 19 rows; 4 x 4 at two terms 13: 2, 2, 3, 4)
    assert _own_rows(12, 2, 3) == _own_rows(8, 3, 3) == 19 and _own_rows(4, 4, 2) == 13
    assert {t for _, t in NARROW.values()} == {1, 2, 3}
    # what a case cannot run: a tile smaller than its halo rows (none of the lists has one; (1, 4, 3) of SWEEP_TILES at three
    # terms is why that tile is not in them), and 12 x 2 at two terms or with a stored D^-1 (asked for, the sweep keeps its default:
    # asserted on the device)
    assert all(_own_rows(t[0], t[1], k) >= 1 for k, tiles in ((3, TILES_3_DERIVED), (3, TILES_3_STORED), (2, TILES_2)) for t in tiles if t)
    assert _own_rows(1, 4, 3) < 1 and (12, 2, 0) not in TILES_3_STORED and (12, 2, 0) not in TILES_2
    for tiles in (TILES_3_DERIVED, TILES_3_STORED, TILES_2):
        assert len([t for t in tiles if t and any(t[:2] == s[:2] for s in SWEEP_TILES if s)]) >= 3
    assert all(t in ONE_TERM_TILES for t in ONE_TERM_OTHER_TILES)
    # the sweep from a zero guess: offered by 12 x 2 and by the tiles of three rows, three terms only
    assert [t for t in TILES_3_DERIVED if t and _offers_zero_guess(3, t)] == [(8, 3, 0), (12, 2, 0), (4, 3, 8)]
    assert not any(_offers_zero_guess(2, t) for t in TILES_2 if t)


# ---- problems and references (one per mesh and material, shared by the tests) ----
def _problem(n, material, numbering=None):
    kw = {"dof_numbering": numbering} if numbering is not None else {}
    if material in ("cellwise", "cellwise6"):
        prob = M.LaplaceProblem(n, "constant", device="cuda", **kw)
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        r = torch.rand(prob.n_cells_total, 1, dtype=torch.float64, device="cuda", generator=g)
        c = 0.5 + r if material == "cellwise" else 10.0 ** (6.0 * r - 3.0)       # [0.5, 1.5) / 10^U(-3, 3)
        prob.coefficient = c.expand(-1, 2 ** len(n)).contiguous()
        return prob
    return M.LaplaceProblem(n, material, device="cuda", **kw)


def _vectors(rng, n_dofs, count):
    return [rng.standard_normal(n_dofs) * 10.0 ** rng.uniform(-3, 3, n_dofs) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def _case(n, material):
    prob = _problem(n, material)
    ref = F.Reference(n, prob.coefficient.cpu().numpy(), u=F.U64)
    x, b, xp = _vectors(np.random.default_rng([len(material), *n]), ref.n_dofs, 3)
    return prob, ref, x, b, xp


@functools.lru_cache(maxsize=None)
def _sweep_reference_3(n, material, zero):
    prob, ref, x, b, _ = _case(n, material)
    its = ref.sweep(np.zeros_like(x) if zero else x, b, AL, BE)
    return its, ref.unit_sweep(its, b, AL, BE)


def _sweep_reference(n, material, n_terms, zero):
    """(iterates, propagated units) of the recurrence from x (zero: from x_0 = 0), one per mesh and material: two terms are the
    first two of three."""
    its, units = _sweep_reference_3(n, material, zero)
    return its[:n_terms + 1], units[:n_terms]


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _operator(ctx, prob, stored=False):
    ctx.set_stored_diagonal(stored)
    try:
        op = M.MatrixFreeLaplace(ctx, prob)
    finally:
        ctx.set_stored_diagonal(False)
    return op


def _check(family, got, ref, unit, k, what, k_ref=F.K_REF * F.ULD / F.U64, perm=None):
    got = got.cpu().numpy()
    if perm is not None:
        got = got[perm]
    ratio = F.worst_ratio(got, ref, unit)
    WORST[family] = max(WORST[family], ratio if np.isfinite(ratio) else 0.0)
    print(f"{what}: worst |got - ref| / (u mag) = {ratio:.2f} (k = {k})")
    F.assert_within(got, ref, unit, k + k_ref, what)


def _check_dinv(op, ref, what, perm=None):
    dinv = op.diagonal_inverse().cpu().numpy()
    if perm is not None:
        dinv = dinv[perm]
    assert not F.beyond(dinv, ref.dinv, F.K_DINV_F64 * F.U64 * ref.dinv).any(), f"{what}: D^-1 beyond {F.K_DINV_F64} u"


# ---- a. the one-term FP64 kernel ----
OPS = ["vmult", "residual", "first-term step", "momentum step", "momentum step over its own x_prev"]


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


@functools.lru_cache(maxsize=None)
def _one_term_references(n, material):
    prob, ref, x, b, xp = _case(n, material)
    ax = ref.vmult(x)
    first = ref.step(x, b, None, 0.0, BE[0], ax=ax)
    mom = ref.step(x, b, xp, AL[1], BE[1], ax=ax)
    refs = [ax, ax - b.astype(LD), first, mom, mom]
    units = [ref.unit_vmult(x), ref.unit_residual(x, b), ref.unit_step(x, b, None, 0.0, BE[0]), ref.unit_step(x, b, xp, AL[1], BE[1])]
    return refs, units + [units[3]], [ref.k_op, ref.k_op + 1, ref.k_step, ref.k_step, ref.k_step]


def _to_dof(v, perm):
    """Value of node i lives at DoF perm[i]."""
    if perm is None:
        return v
    o = np.empty_like(v)
    o[perm] = v
    return o


def _one_term_battery(ctx, op, n, material, what, tiles=ONE_TERM_OTHER_TILES, perm=None):
    """Every operation against the bound on the default tile; the same bits on two other tiles; D^-1."""
    prob, ref, x, b, xp = _case(n, material)
    xd, bd, xpd = (_gpu(_to_dof(v, perm)) for v in (x, b, xp))
    base = _one_term_outputs(ctx, op, xd, bd, xpd)
    refs, units, ks = _one_term_references(n, material)
    for name, got, want, unit, k in zip(OPS, base, refs, units, ks):
        _check("one-term", got, want, unit, k, f"{what} {name}", perm=perm)
    for nw, ty, tz in tiles:
        op.set_tile(ty, tz, nw)
        for name, got, want in zip(OPS, _one_term_outputs(ctx, op, xd, bd, xpd), base):
            assert torch.equal(got, want), f"{what} tile {(nw, ty, tz)}: {name} differs from the default tile in {(got != want).sum().item()} entries"
    _check_dinv(op, ref, what, perm)
    return base


@pytest.mark.parametrize("material", MATERIALS)
@pytest.mark.parametrize("n", MESHES + [(32, 24, 22)] + DEGENERATE + TAIL_SLAB, ids=lambda v: "x".join(map(str, v)))
def test_one_term_kernel_every_epilogue(ctx, n, material):
    prob, ref, x, b, xp = _case(n, material)
    op = _operator(ctx, prob)
    cc = ref.cell_constant
    assert cc == (material != "linear") or material == "discontinuous"
    assert op.cell_constant_layout() == cc and op.diagonal_in_record() == (not cc)      # (cellwise6: still one coefficient per cell)
    _one_term_battery(ctx, op, n, material, f"{n} {material}")
    refs, units, ks = _one_term_references(n, material)
    if cc:
        # D^-1 kept in the records instead of derived in the kernel: the smoother steps within the same bound
        op_s = _operator(ctx, prob, stored=True)
        assert op_s.diagonal_in_record()
        stored = _one_term_outputs(ctx, op_s, _gpu(x), _gpu(b), _gpu(xp))
        for i in (2, 3, 4):
            _check("one-term", stored[i], refs[i], units[i], ks[i], f"{n} {material} {OPS[i]}, stored D^-1")
        _check_dinv(op_s, ref, f"{n} {material} stored")
    if cc and n in TAIL_SLAB:
        # records with one halo lane (the layout of a context that runs one term per launch): the columns of the nearly empty
        # last chunk run as a rotated slab inside the same launch -- with three halo lanes the columns are spread evenly
        ctx.set_mf_fused_terms(1)
        try:
            op_1 = _operator(ctx, prob)
        finally:
            ctx.set_mf_fused_terms(3)
        assert not op_1.sweep_available(2)
        _one_term_battery(ctx, op_1, n, material, f"{n} {material} one halo lane (tail slab)")


@pytest.mark.parametrize("material", ["linear", "cellwise6"])
def test_one_term_kernel_with_a_random_numbering(ctx, material):
    """Ids read from the records, not computed: vectors and results permuted, the same reference."""
    n = (20, 17, 9)
    _, ref, _, _, _ = _case(n, material)
    perm = np.random.default_rng(3).permutation(ref.n_dofs)
    prob = _problem(n, material, numbering=torch.from_numpy(perm))
    op = _operator(ctx, prob)
    assert not op.ids_computed() and not op.sweep_available(2)
    assert _operator(ctx, _case(n, "linear")[0]).ids_computed()           # (lexicographic, eight coefficients: computed)
    _one_term_battery(ctx, op, n, material, f"{n} {material} random numbering", perm=perm)


@pytest.mark.parametrize("n,material", [((8, 8), "constant"), ((12, 7), "linear"), ((33, 5), "discontinuous"), ((1, 1), "constant")])
def test_one_term_kernel_in_two_dimensions(ctx, n, material):
    prob, ref, x, b, xp = _case(n, material)
    op = M.MatrixFreeLaplace(ctx, prob)
    refs, units, ks = _one_term_references(n, material)
    assert ks[0] == F.K_OP_GENERAL
    for what, got, want, unit, k in zip(OPS, _one_term_outputs(ctx, op, _gpu(x), _gpu(b), _gpu(xp)), refs, units, ks):
        _check("one-term", got, want, unit, k, f"{n} {material} {what}")
    _check_dinv(op, ref, f"{n} {material}")


# ---- b. the FP64 sweep ----
def _sweep(ctx, op, al, be, b, x, with_prev):
    out, outp = _nan(b.numel()), (_nan(b.numel()) if with_prev else None)
    op.smoother_sweep(al, be, b, x, out, outp)
    ctx.synchronize()
    return out, outp


@pytest.mark.parametrize("n_terms", [2, 3])
@pytest.mark.parametrize("material", SWEEP_MATERIALS)
@pytest.mark.parametrize("n,tz", SWEEP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"tz{v}")
def test_sweep_every_tile_both_arithmetics_and_the_zero_guess(ctx, n, tz, material, n_terms):
    prob, ref, x, b, _ = _case(n, material)
    xd, bd, zd = _gpu(x), _gpu(b), torch.zeros(ref.n_dofs, dtype=torch.float64, device="cuda")
    al, be = AL[:n_terms], BE[:n_terms]
    its, units = _sweep_reference(n, material, n_terms, False)
    narrow = _narrow_column(n[0] + 1)
    assert narrow == (n in NARROW)
    for stored in (False, True):
        op = _operator(ctx, prob, stored)
        assert op.cell_constant_layout() and op.sweep_available(n_terms) and op.diagonal_in_record() == stored
        # the default: twelve wavefronts of two rows for three terms with a derived D^-1, 8 x 3 / 4 x 4 otherwise -- also when asked for 12 x 2
        default = (12, 2) if (n_terms == 3 and not stored) else ((8, 3) if n_terms == 3 else (4, 4))
        assert op.get_sweep_tile(n_terms)[:2] == default
        op.set_sweep_tile(12, 2, 0)
        assert op.get_sweep_tile(n_terms)[:2] == default
        op.set_sweep_tile(0, 0, 0)
        if narrow:
            assert _y_tiles(n[1] + 1, _own_rows(*default, n_terms)) == (NARROW[n][1] if n_terms == 3 else _y_tiles(n[1] + 1, 13))
        # the terms as one launch each (the one-term kernel, held to the bound above)
        terms = [xd]
        for k in range(n_terms):
            o = _nan(xd.numel())
            op.smoother_step(bd, terms[-1], terms[-2] if k > 0 else None, al[k], be[k], o)
            terms.append(o)
        default_bits = zero_bits = None
        for tile in (TILES_2 if n_terms == 2 else (TILES_3_STORED if stored else TILES_3_DERIVED)):
            if tile is None:
                nw, ty, t_z = op.get_sweep_tile(n_terms)
                t_z = 0
            else:
                nw, ty, t_z = tile
            op.set_sweep_tile(nw, ty, tz or t_z)
            in_force = op.get_sweep_tile(n_terms)
            assert in_force[:2] == (nw, ty) and (not (tz or t_z) or in_force[2] == (tz or t_z)), (tile, in_force)
            what = f"{n} tz {tz} {material} {n_terms} terms tile {in_force} stored D^-1 {stored}"
            for with_prev in (True, False):
                op.set_sweep_reference(True)
                out, outp = _sweep(ctx, op, al, be, bd, xd, with_prev)
                assert torch.equal(out, terms[-1]), f"{what}, reference arithmetic: x_{n_terms} differs from the term-by-term sequence in {(out != terms[-1]).sum().item()} entries"
                assert outp is None or torch.equal(outp, terms[-2]), f"{what}, reference arithmetic: x_{n_terms - 1} differs from the term-by-term sequence"
                if n_terms == 3:
                    with pytest.raises(L.MfmgNotImplementedError):        # (no zero-guess kernel in the reference arithmetic)
                        op.smoother_sweep(al, be, bd, None, _nan(bd.numel()))
                # the arithmetic production launches
                op.set_sweep_reference(False)
                out, outp = _sweep(ctx, op, al, be, bd, xd, with_prev)
                _check("sweep", out, its[-1], units[-1], ref.k_step, f"{what} out_prev {with_prev}: x_{n_terms}")
                if with_prev:
                    _check("sweep", outp, its[-2], units[-2], ref.k_step, f"{what}: x_{n_terms - 1}")
                    default_bits = default_bits or (out, outp)
                # ... does not depend on the tile, bit for bit (the first tile of the list is the default)
                assert torch.equal(out, default_bits[0]), f"{what}: differs from the default tile in {(out != default_bits[0]).sum().item()} entries"
                assert outp is None or torch.equal(outp, default_bits[1]), f"{what}: x_{n_terms - 1} differs from the default tile"
                # from a zero guess, x_0 not read
                if not _offers_zero_guess(n_terms, in_force):
                    with pytest.raises(L.MfmgNotImplementedError):
                        op.smoother_sweep(al, be, bd, None, _nan(bd.numel()))
                    continue
                zits, zunits = _sweep_reference(n, material, n_terms, True)
                out, outp = _sweep(ctx, op, al, be, bd, None, with_prev)           # (raises unless the operator offers it)
                _check("sweep from zero", out, zits[-1], zunits[-1], ref.k_step, f"{what} out_prev {with_prev} from zero: x_3")
                if with_prev:
                    _check("sweep from zero", outp, zits[-2], zunits[-2], ref.k_step, f"{what} from zero: x_2")
                onz, onzp = _sweep(ctx, op, al, be, bd, zd, with_prev)
                assert torch.equal(out, onz) and (outp is None or torch.equal(outp, onzp)), f"{what}: from zero differs from the sweep on a zeroed vector"
                if with_prev:
                    zero_bits = zero_bits or (out, outp)
                assert torch.equal(out, zero_bits[0]) and (outp is None or torch.equal(outp, zero_bits[1])), f"{what}: from zero differs from the default tile"


# ---- c. the interior and shell launches of a distributed rank, on one rank ----
@pytest.mark.parametrize("material", ["constant", "linear"])
def test_interior_and_shell_launches_within_the_bound(ctx, material):
    """The launches of the corner rank of a 2 x 2 x 2 grid (Context.set_mf_emulate_split, as test_interior_and_shell_launches_change_no_bit):
    the operator and the three-term polynomial of the hierarchy's smoother, one launch pair per term, in every shell mode."""
    n = (70, 30, 20)
    prob, ref, x, b, _ = _case(n, material)
    lmax, lmin = 1.9, 0.095
    params = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": False, "max levels": 2,
              "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0, "fused_terms": 1, "lambda_max": lmax, "lambda_min": lmin},
              "solver": {"type": "pcg", "n_iterations": 4}}
    ctx.set_mf_fused_terms(1)
    try:
        h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, params)
    finally:
        ctx.set_mf_fused_terms(3)
    h.set_operator_tile(2, 2, 4)          # several column, y- and z-tiles
    assert h.smoother_info() == (3, lmin, lmax)
    coefs = O.ChebyshevParams(3, lmax, lmin).step_coefficients()
    al, be = [c[0] for c in coefs], [c[1] for c in coefs]
    its = ref.sweep(x, b, al, be)
    units = ref.unit_sweep(its, b, al, be)
    ax, unit_ax = ref.vmult(x), ref.unit_vmult(x)
    xd, bd = _gpu(x), _gpu(b)

    def run(what):
        y, xs = _nan(ref.n_dofs), xd.clone()
        h.operator_apply(0, xd, y)
        h.smoother_apply(0, bd, xs)
        ctx.synchronize()
        _check("one-term", y, ax, unit_ax, ref.k_op, f"{n} {material} {what}: A x")
        # (the coefficients of the polynomial are computed in double on either side: one more rounding each, within the epilogue's count)
        _check("one-term", xs, its[-1], units[-1], ref.k_step, f"{n} {material} {what}: three terms")
        return y, xs

    whole = run("one launch")
    try:
        ctx.set_mf_emulate_split("xyz")
        for variant in ("beside", "after", "slabs"):
            ctx.set_mf_shell(variant)
            out = run(f"shell {variant}")
            assert torch.equal(out[0], whole[0]) and torch.equal(out[1], whole[1]), variant
    finally:
        ctx.set_mf_emulate_split(None)
        ctx.set_mf_shell("beside")


def test_worst_ratios_observed():
    """(runs last: what the cases above measured, for the figures of the module docstring)"""
    print("worst |got - ref| / (u mag) per family: " + ", ".join(f"{k} {v:.2f}" for k, v in WORST.items()))
