"""What the operator does NOT take for a uniform coefficient (MatrixFreeLaplace.uniform_coefficient, decided on the device at
construction): a coefficient that differs in one cell by one bit, the materials "discontinuous" and "linear", a mesh with faces
that are not Dirichlet, and the local problem of a rank with ghost layers.  Each of them keeps the sweep kernels of before
(uniform_sweep_launches stays zero); for the one-bit case the results equal those with MFMG_MF_UNIFORM_SWEEP=0 bit for bit."""
import os

import numpy as np
import pytest
import torch

import mfmg_amd as M

pytestmark = pytest.mark.gpu

AL = [0.0, 0.23, 0.31]
BE = [0.61, 0.87, 0.79]
CELLS = (59, 20, 8)


def _sweep(ctx, op, b, x):
    out = torch.full_like(b, float("nan"))
    outp = torch.full_like(b, float("nan"))
    op.smoother_sweep(AL, BE, b, x, out, outp)
    ctx.synchronize()
    return out, outp


def _vectors(n):
    rng = np.random.default_rng(5)
    return (torch.from_numpy(rng.standard_normal(n)).cuda() for _ in range(2))


def _keeps_the_kernels_of_before(ctx, op):
    assert not op.uniform_coefficient()
    if not op.sweep_available(3):
        return None
    b, x = _vectors(op.n_dofs)
    res = _sweep(ctx, op, b, x) + _sweep(ctx, op, b, None)
    assert op.uniform_sweep_launches() == 0
    return b, x, res


def test_constant_is_uniform(ctx):
    op = M.MatrixFreeLaplace(ctx, M.LaplaceProblem(CELLS, "constant", device="cuda"))
    assert op.uniform_coefficient() and op.uniform_sweep_launches() == 0


@pytest.mark.parametrize("cell", ["first", "middle", "last"])
def test_one_cell_changed_in_the_last_bit(ctx, cell):
    prob = M.LaplaceProblem(CELLS, "constant", device="cuda")
    c = prob.coefficient.clone()
    i = {"first": 0, "middle": prob.n_cells_total // 2 + 7, "last": prob.n_cells_total - 1}[cell]
    c[i, :] = torch.nextafter(c[i, :], torch.full_like(c[i, :], float("inf")))
    assert (c[i] != prob.coefficient[i]).all()
    prob.coefficient = c.contiguous()
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.cell_constant_layout() and op.sweep_available(3) and op.get_sweep_tile(3)[:2] == (12, 2)
    b, x, res = _keeps_the_kernels_of_before(ctx, op)
    os.environ["MFMG_MF_UNIFORM_SWEEP"] = "0"
    try:
        off = _sweep(ctx, op, b, x) + _sweep(ctx, op, b, None)
    finally:
        del os.environ["MFMG_MF_UNIFORM_SWEEP"]
    assert all(torch.equal(g, w) for g, w in zip(res, off))


@pytest.mark.parametrize("material", ["discontinuous", "linear"])
def test_varying_materials(ctx, material):
    prob = M.LaplaceProblem(CELLS, material, device="cuda")
    _keeps_the_kernels_of_before(ctx, M.MatrixFreeLaplace(ctx, prob))


def test_faces_that_are_not_dirichlet(ctx):
    prob = M.LaplaceProblem(CELLS, "constant", device="cuda", dirichlet=False)
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.cell_constant_layout()
    _keeps_the_kernels_of_before(ctx, op)
    # one face alone: the free nodes of the high z face (its edges belong to the other faces)
    prob = M.LaplaceProblem(CELLS, "constant", device="cuda")
    con = prob.constrained.reshape(tuple(reversed(prob.N))).clone()
    con[-1, 1:-1, 1:-1] = 0
    prob.constrained = con.reshape(-1).contiguous()
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.cell_constant_layout()
    _keeps_the_kernels_of_before(ctx, op)


@pytest.mark.parametrize("rank", [0, 7])
def test_local_problem_of_a_rank_with_ghost_layers(mfmg_lib, rank):
    """The local problem of a corner rank of a 2 x 2 x 2 grid on a plain context (no communicator): constant material, ghost
    layers towards its neighbours, Dirichlet faces on the other sides only."""
    ctx = M.Context()
    part = M.BoxPartition((32, 32, 32), rank, (2, 2, 2), low_ghost_cells=4)
    prob = part.local_problem("constant", "cuda")
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.cell_constant_layout()
    _keeps_the_kernels_of_before(ctx, op)
