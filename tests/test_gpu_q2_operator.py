"""The Q2 matrix-free operator on the GPU, entry by entry against long double (q2_reference.py): vmult, the residual, the `first`
and `next` smoother terms, `next` written over its own x_prev, the diagonal and its inverse, on the meshes of q2_cases.py (every
tile edge of the default tile) and five coefficient layouts.  The bound is (K + K_REF) u mag with K counted from the kernel."""
import numpy as np
import pytest
import torch

import mfmg_amd as M
import q2_reference as R
from q2_cases import q2_meshes

pytestmark = pytest.mark.gpu

MATERIALS = ["constant", "linear", "discontinuous", "random cell", "random cell as 27"]
WORST = {}


def _meshes():
    return q2_meshes(M.q2_tile_shapes()[0])


def _problem(n, h, dirichlet, material, seed):
    kind = material if material in ("constant", "linear", "discontinuous") else "constant"
    p = M.LaplaceProblemQ2(n, kind, device="cuda", dirichlet=dirichlet, cell_size=h)
    if material.startswith("random cell"):
        rng = np.random.default_rng(seed)
        c = 10.0 ** rng.uniform(-3, 3, p.n_cells_total)     # one value per cell over six decades
        p.coefficient = torch.from_numpy(np.repeat(c[:, None], 27, axis=1).copy()).cuda()
    return p


def _operator(ctx, p, material):
    ctx.set_cell_constant_layout(material != "random cell as 27")
    try:
        return M.MatrixFreeLaplaceQ2(ctx, p)
    finally:
        ctx.set_cell_constant_layout(True)


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _check(name, got, ref, mag, k):
    ok, worst = R.within_bound(got.cpu().numpy(), ref, mag, k)
    WORST[name] = max(WORST.get(name, 0.0), worst)
    assert ok, f"{name}: worst |got - ref| / bound = {worst}"


@pytest.mark.parametrize("material", MATERIALS)
@pytest.mark.parametrize("case", range(15))
def test_every_entry_within_the_bound(ctx, case, material):
    name, n, h, dirichlet = _meshes()[case]
    p = _problem(n, h, dirichlet, material, seed=case)
    op = _operator(ctx, p, material)
    assert op.cell_constant_layout() == (material in ("constant", "random cell"))
    ref = R.Q2Reference(n, p.h, p.coefficient.cpu().numpy(), p.constrained.cpu().numpy())
    nd = p.n_dofs
    rng = np.random.default_rng(100 + case)
    x, b, xp = (R.six_decades(rng, nd) for _ in range(3))
    xd, bd, xpd = (torch.from_numpy(v).cuda() for v in (x, b, xp))
    con = p.constrained.cpu().numpy().astype(bool)
    alpha, beta = 0.37, 0.81

    diag, dinv = op.diagonal(), op.diagonal_inverse()
    dref, dmag = ref.diagonal()
    _check("diagonal", diag, dref, dmag, R.K_DIAG)
    _check("diagonal inverse", dinv, 1 / dref, 1 / dmag, R.K_DINV)
    assert np.all(diag.cpu().numpy()[con] == 1.0) and np.all(dinv.cpu().numpy()[con] == 1.0)
    dinv_h = dinv.cpu().numpy()

    y = _nan(nd)
    op.vmult(y, xd)
    ctx.synchronize()
    _check("vmult", y, *ref.mode("apply", x), R.K_MODE["apply"])
    assert np.array_equal(y.cpu().numpy()[con], x[con])          # constrained rows return x

    res = _nan(nd)
    op.residual(xd, bd, res)
    ctx.synchronize()
    _check("residual", res, *ref.mode("residual", x, b), R.K_MODE["residual"])

    out = _nan(nd)
    op.smoother_step(bd, xd, None, 0.0, beta, out)
    ctx.synchronize()
    _check("first", out, *ref.mode("first", x, b, beta=beta, dinv=dinv_h), R.K_MODE["first"])

    out2 = _nan(nd)
    op.smoother_step(bd, xd, xpd, alpha, beta, out2)
    ctx.synchronize()
    nref, nmag = ref.mode("next", x, b, xp, alpha, beta, dinv_h)
    _check("next", out2, nref, nmag, R.K_MODE["next"])

    over = xpd.clone()
    op.smoother_step(bd, xd, over, alpha, beta, over)             # out is x_prev
    ctx.synchronize()
    assert torch.equal(over, out2)

    # the same bits on a second run and on every offered tile
    for tile in M.q2_tile_shapes():
        op.set_tile(*tile)
        assert op.get_tile() == tile
        again, again2 = _nan(nd), _nan(nd)
        op.vmult(again, xd)
        op.smoother_step(bd, xd, xpd, alpha, beta, again2)
        ctx.synchronize()
        assert torch.equal(again, y), tile
        assert torch.equal(again2, out2), tile
    op.set_tile(0, 0, 0)
    assert op.get_tile() == M.q2_tile_shapes()[0]


@pytest.mark.parametrize("case", [2, 14])
def test_compact_and_27_value_layouts_agree(ctx, case):
    name, n, h, dirichlet = _meshes()[case]
    p = _problem(n, h, dirichlet, "random cell", seed=case)
    a, b = _operator(ctx, p, "random cell"), _operator(ctx, p, "random cell as 27")
    assert a.cell_constant_layout() and not b.cell_constant_layout()
    ref = R.Q2Reference(n, p.h, p.coefficient.cpu().numpy(), p.constrained.cpu().numpy())
    x = R.six_decades(np.random.default_rng(7), p.n_dofs)
    xd = torch.from_numpy(x).cuda()
    ya, yb = _nan(p.n_dofs), _nan(p.n_dofs)
    a.vmult(ya, xd)
    b.vmult(yb, xd)
    ctx.synchronize()
    _, mag = ref.apply(x)
    diff = np.abs(ya.cpu().numpy().astype(R.LD) - yb.cpu().numpy().astype(R.LD))
    assert np.all(diff <= 2 * (R.K_APPLY + R.K_REF) * R.U * mag)


def test_refusals(ctx):
    p = M.LaplaceProblemQ2((2, 2, 2), device="cuda")
    op = M.MatrixFreeLaplaceQ2(ctx, p)
    x = torch.zeros(p.n_dofs, dtype=torch.float64, device="cuda")
    with pytest.raises(M.lib.MfmgInvalidArgument, match="in place"):
        op.vmult(x, x)
    with pytest.raises(M.lib.MfmgInvalidArgument, match="tile"):
        op.set_tile(3, 3, 3)
    d = p.mesh_desc()
    d.dim = 2
    import ctypes as C
    h = C.c_void_p()
    assert M.lib.load().mfmg_hip_mf_laplace_q2_create(ctx.handle, C.byref(d), C.byref(h)) == M.lib.ERROR_NOT_IMPLEMENTED
    d = p.mesh_desc()
    d.n_dofs = p.n_dofs + 1
    assert M.lib.load().mfmg_hip_mf_laplace_q2_create(ctx.handle, C.byref(d), C.byref(h)) == M.lib.ERROR_INVALID_ARGUMENT
    d = p.mesh_desc()
    d.n_cells[0] = d.n_cells[1] = d.n_cells[2] = 700     # 1401^3 unknowns: beyond 2^31 (refused before anything is read)
    d.n_dofs = 1401 ** 3
    assert M.lib.load().mfmg_hip_mf_laplace_q2_create(ctx.handle, C.byref(d), C.byref(h)) == M.lib.ERROR_INVALID_ARGUMENT
    # a context with a communicator (rank 0 of 2, ghost cells towards the upper neighbour)
    ranks = M.Context()
    M.lib.check(M.lib.load().mfmg_hip_context_set_communicator(ranks.handle, 0, 2, 0, 2))
    with pytest.raises(M.lib.MfmgNotImplementedError, match="communicator"):
        M.MatrixFreeLaplaceQ2(ranks, p)


def test_worst_observed_ratio_is_printed():
    """Documentation, not a threshold: the worst |got - ref| / ((K + K_REF) u mag) the tests above saw, per quantity."""
    for name, worst in sorted(WORST.items()):
        print(f"Q2 operator, worst error / bound, {name}: {worst:.3f}")
