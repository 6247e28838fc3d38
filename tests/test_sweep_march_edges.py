"""Edges of the march of the multi-term smoother sweep (mf_cheb_fused.hip): the loop runs trips of K super-passes, so
short tiles (TZ = 1 .. 4), thin meshes (Nz = 3 .. 8) and tiles at the bottom and the top of the mesh end a trip early at
every position.  Two and three terms, a narrow last chunk column, the zero guess.  LaplaceProblem takes cell counts: 86 cells
in x are 87 node columns = 58 + 29, and with the default 3 halo lanes a last column of at most 32 - 3 = 29 is swept by the
narrow body (mf_laplace.hip); 20 cells (21 nodes, one chunk column) take the wide body alone."""
import pytest
import torch

import mfmg_amd as M

pytestmark = pytest.mark.gpu

COEFS = [(0.0, 0.61), (0.23, 0.87), (0.31, 0.79)]  # (alpha, beta) of three Chebyshev-like terms
TILE = {2: (4, 4), 3: (8, 3)}                      # (wavefronts, rows per wavefront) the sweeps take by default


def _problem(n, material):
    prob = M.LaplaceProblem(n, "constant", device="cuda")
    if material == "cellwise":
        g = torch.Generator(device="cuda")
        g.manual_seed(11)
        prob.coefficient = (0.5 + torch.rand(prob.n_cells_total, 1, dtype=torch.float64, device="cuda", generator=g)).expand(-1, 8).contiguous()
    return prob


def _vectors(n_dofs, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.rand(n_dofs, dtype=torch.float64, device="cuda", generator=g)
    b = torch.rand(n_dofs, dtype=torch.float64, device="cuda", generator=g)
    return x, b


def _sweep(ctx, op, al, be, b, x, with_prev):
    out = torch.full_like(b, float("nan"))
    outp = torch.full_like(b, float("nan")) if with_prev else None
    op.smoother_sweep(al, be, b, x, out, outp)
    ctx.synchronize()
    return out, outp


MESHES = [((86, 13, 3), "cellwise"), ((86, 11, 4), "constant"), ((20, 9, 5), "cellwise"), ((86, 7, 8), "cellwise")]
HALO = 3  # halo lanes of the records (Context default: three smoother terms per sweep)


def test_sweep_march_edges_meshes_reach_the_narrow_column():
    """The meshes with 86 cells in x end in a narrow chunk column (the rule of mf_laplace.hip), the others do not."""
    full = 64 - 2 * HALO
    for n, _ in MESHES:
        nodes = n[0] + 1
        rest = nodes - (nodes + full - 1) // full * full + full
        narrow = nodes > full and 1 <= rest <= 32 - HALO
        assert narrow == (n[0] == 86), (n, rest)


@pytest.mark.parametrize("n,material", MESHES)
@pytest.mark.parametrize("n_terms", [2, 3])
def test_sweep_march_edges_reference_term_by_term(ctx, n, material, n_terms):
    """The reference-arithmetic sweep == its terms as one launch each, bit for bit, for z-tiles of 1 .. 4 layers."""
    prob = _problem(n, material)
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.sweep_available(n_terms)
    op.set_sweep_reference(True)
    x, b = _vectors(prob.n_dofs, 5)
    al = [c[0] for c in COEFS][:n_terms]
    be = [c[1] for c in COEFS][:n_terms]
    its = [x]
    for k in range(n_terms):
        o = torch.full_like(x, float("nan"))
        op.smoother_step(b, its[-1], its[-2] if k > 0 else None, al[k], be[k], o)
        its.append(o)
    for tz in (1, 2, 3, 4):
        op.set_sweep_tile(*TILE[n_terms], tz)
        out, outp = _sweep(ctx, op, al, be, b, x, True)
        assert torch.equal(out, its[-1]), f"tz={tz}"
        assert torch.equal(outp, its[-2]), f"tz={tz}"


@pytest.mark.parametrize("n,material", MESHES)
@pytest.mark.parametrize("n_terms", [2, 3])
def test_sweep_march_edges_modes_tiling_independent(ctx, n, material, n_terms):
    """The mode-space sweep gives the same bits for every z-tile height, including one z-tile over the whole mesh."""
    prob = _problem(n, material)
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.sweep_available(n_terms)
    x, b = _vectors(prob.n_dofs, 6)
    al = [c[0] for c in COEFS][:n_terms]
    be = [c[1] for c in COEFS][:n_terms]
    op.set_sweep_tile(*TILE[n_terms], n[2])
    ref, refp = _sweep(ctx, op, al, be, b, x, True)
    assert torch.isfinite(ref).all() and torch.isfinite(refp).all()
    for tz in (1, 2, 3, 4):
        op.set_sweep_tile(*TILE[n_terms], tz)
        out, outp = _sweep(ctx, op, al, be, b, x, True)
        assert torch.equal(out, ref), f"tz={tz}"
        assert torch.equal(outp, refp), f"tz={tz}"


@pytest.mark.parametrize("n,material", MESHES)
def test_sweep_march_edges_zero_guess(ctx, n, material):
    """The three-term sweep from a zero guess (x_0 not read) == the sweep run on a zeroed vector, for z-tiles of 1 .. 4 layers."""
    prob = _problem(n, material)
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.sweep_available(3)
    _, b = _vectors(prob.n_dofs, 7)
    al = [c[0] for c in COEFS]
    be = [c[1] for c in COEFS]
    zero = torch.zeros_like(b)
    for tz in (1, 2, 3, 4):
        op.set_sweep_tile(*TILE[3], tz)
        ref, _ = _sweep(ctx, op, al, be, b, zero, False)
        out, _ = _sweep(ctx, op, al, be, b, None, False)
        assert torch.isfinite(out).all() and torch.equal(out, ref), f"tz={tz}"
