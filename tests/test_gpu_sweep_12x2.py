"""The three-term FP64 sweep in its shape of twelve wavefronts of two cell rows (mf_cheb_fused_wg12_kernel, three wavefronts
per SIMD): the same bits as the term-by-term smoother_step sequence (reference arithmetic) and as the sweep of eight
wavefronts of three rows on the same inputs (both arithmetics), with torch.equal -- the results of the sweep do not depend on
its tiling.  Both shapes own 19 DoF rows per y-tile.

Shapes are (Nx, Ny, Nz) in DoFs; LaplaceProblem takes cells, one fewer per direction.  Each reaches one edge of the tiling:
a tile larger than the mesh, Ny at one y-tile / one plus a row / two plus a row, a narrow last chunk column with three y-tiles
(one full pair and one half-idle pair), meshes of several chunk columns, and z-tiles whose fill and drain are shorter (4) and
longer (5) than the three terms.  By the rule of mf_laplace.hip (a last column of 1 .. 32 - halo node columns beside full
ones of 64 - 2 halo = 58) 117 node columns are 58 + 58 + 1: two full chunk columns AND a narrow one of a single column;
116 node columns are the two full ones alone, so that shape is here too.  The reference-arithmetic kernel of this shape has
no body for a narrow column (the two bodies in one kernel do not fit 168 VGPRs) and runs it with ordinary tiles; the narrow
body of the mode-space kernel is held to the 8 x 3 sweep."""
import pytest
import torch

import mfmg_amd as M

pytestmark = pytest.mark.gpu

COEFS = [(0.0, 0.61), (0.23, 0.87), (0.31, 0.79)]  # (alpha, beta) of three Chebyshev-like terms
AL = [c[0] for c in COEFS]
BE = [c[1] for c in COEFS]
HALO = 3       # halo lanes of the records (Context default: three smoother terms per sweep)
OWN_ROWS = 19  # 12 x 2 - 2 x 3 + 1 = 8 x 3 - 2 x 3 + 1

# (DoFs, z-tile: 0 = the sweep's own choice)
CASES = [((9, 9, 9), 0), ((65, 19, 7), 0), ((65, 20, 7), 0), ((65, 39, 7), 0), ((79, 40, 9), 0), ((117, 21, 9), 0), ((116, 21, 9), 0),
         ((33, 25, 23), 4), ((33, 25, 23), 5)]


def _narrow_column(nx):
    full = 64 - 2 * HALO
    ncols = (nx + full - 1) // full
    rest = nx - (ncols - 1) * full
    return ncols >= 2 and 1 <= rest <= 32 - HALO


def _problem(dofs, material):
    prob = M.LaplaceProblem(tuple(v - 1 for v in dofs), material, device="cuda")
    if material == "discontinuous":  # one coefficient per cell: that of its first corner
        prob.coefficient = prob.coefficient[:, :1].expand(-1, 8).contiguous()
    return prob


def _vectors(n_dofs, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.rand(n_dofs, dtype=torch.float64, device="cuda", generator=g)
    b = torch.rand(n_dofs, dtype=torch.float64, device="cuda", generator=g)
    return x, b


def _sweep(ctx, op, b, x, with_prev):
    out = torch.full_like(b, float("nan"))
    outp = torch.full_like(b, float("nan")) if with_prev else None
    op.smoother_sweep(AL, BE, b, x, out, outp)
    ctx.synchronize()
    return out, outp


def test_sweep_12x2_cases_reach_the_edges_they_name():
    assert not _narrow_column(9) and not _narrow_column(33) and not _narrow_column(116)
    assert _narrow_column(65) and _narrow_column(79) and _narrow_column(117)
    # Ny at one y-tile, one more row, two tiles and a row; three y-tiles beside the narrow column: a full and a half-idle pair
    assert [(ny + OWN_ROWS - 1) // OWN_ROWS for ny in (19, 20, 39, 40)] == [1, 2, 3, 3]


@pytest.mark.parametrize("material", ["constant", "discontinuous"])
@pytest.mark.parametrize("dofs,tz", CASES)
def test_sweep_12x2_equals_term_by_term_and_8x3(ctx, dofs, tz, material):
    prob = _problem(dofs, material)
    assert prob.n_dofs == dofs[0] * dofs[1] * dofs[2]
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.sweep_available(3)
    x, b = _vectors(prob.n_dofs, 5)
    # the terms as one launch each
    its = [x]
    for k in range(3):
        o = torch.full_like(x, float("nan"))
        op.smoother_step(b, its[-1], its[-2] if k > 0 else None, AL[k], BE[k], o)
        its.append(o)
    ctx.synchronize()
    assert torch.isfinite(its[-1]).all()
    for reference in (True, False):
        op.set_sweep_reference(reference)
        op.set_sweep_tile(8, 3, tz)
        assert tuple(op.get_sweep_tile(3))[:2] == (8, 3)
        ref, refp = _sweep(ctx, op, b, x, True)
        op.set_sweep_tile(12, 2, tz)
        tile = tuple(op.get_sweep_tile(3))
        assert tile[:2] == (12, 2) and (tz == 0 or tile[2] == tz), tile
        out, outp = _sweep(ctx, op, b, x, True)
        alone, none = _sweep(ctx, op, b, x, False)  # (out_prev null)
        assert none is None
        if reference:
            assert torch.equal(ref, its[-1]) and torch.equal(refp, its[-2])
            assert torch.equal(out, its[-1]), "12 x 2, reference arithmetic: x_3 differs from the term-by-term sequence"
            assert torch.equal(outp, its[-2]), "12 x 2, reference arithmetic: x_2 differs from the term-by-term sequence"
        assert torch.isfinite(out).all() and torch.isfinite(outp).all()
        assert torch.equal(out, ref), f"12 x 2 differs from 8 x 3 (reference arithmetic: {reference})"
        assert torch.equal(outp, refp), f"12 x 2 differs from 8 x 3 in x_2 (reference arithmetic: {reference})"
        assert torch.equal(alone, ref), f"12 x 2 without out_prev differs (reference arithmetic: {reference})"


@pytest.mark.parametrize("dofs,tz", [((79, 40, 9), 0), ((33, 25, 23), 4)])
def test_sweep_12x2_zero_guess(ctx, dofs, tz):
    """From a zero guess (x_0 not read): the bits of the sweep on a zeroed vector, of the 8 x 3 zero-guess sweep, and of the terms."""
    prob = _problem(dofs, "discontinuous")
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.sweep_available(3)
    _, b = _vectors(prob.n_dofs, 7)
    zero = torch.zeros_like(b)
    op.set_sweep_tile(8, 3, tz)
    ref8, _ = _sweep(ctx, op, b, None, False)
    op.set_sweep_tile(12, 2, tz)
    assert tuple(op.get_sweep_tile(3))[:2] == (12, 2)
    ref, refp = _sweep(ctx, op, b, zero, True)
    out, outp = _sweep(ctx, op, b, None, True)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref) and torch.equal(outp, refp) and torch.equal(out, ref8)
    # reference arithmetic (no zero-guess kernel of its own: the sweep on the zeroed vector) against the terms
    op.set_sweep_reference(True)
    its = [zero]
    for k in range(3):
        o = torch.full_like(b, float("nan"))
        op.smoother_step(b, its[-1], its[-2] if k > 0 else None, AL[k], BE[k], o)
        its.append(o)
    out, outp = _sweep(ctx, op, b, zero, True)
    assert torch.equal(out, its[-1]) and torch.equal(outp, its[-2])
