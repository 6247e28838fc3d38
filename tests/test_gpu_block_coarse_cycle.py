"""The coarse cycle on blocks of vectors: HipSolver::apply_block under Hierarchy.coarse_apply_block, apply_block, vmult_block and
solve_cg_block, column by column against the one-vector calls, bit for bit.

Mesh: (52, 52, 52) cells.  At the (24, 24, 24) the cases were first meant for, the first coarse operator has 2 * 12^3 = 3456
rows and runs a CSR kernel: SparseMatrixDevice builds block diagonals from 32768 rows on, and with two eigenvectors per 2 x 2 x 2
agglomerate the smallest cubic mesh that gets there is 52 cells a side (2 * 26^3 = 35152 rows; 148877 fine DoFs).  There A_c of
`linear` and `discontinuous` is the symmetric half of stored planes in the split kernel (asserted), which has the block form.
No prolongator or P~ of the aggregation hierarchy reports kind 4 at any small mesh: row-base storage starts at 200000 rows (a
first coarse level of a 93-cell mesh), so P (LDS-cached CSR here), P^T and the levels below run column by column inside the
block cycle -- the loop of every step that has no block call is part of what is tested.

For k = 1, 3, 4, 7 on ONE hierarchy per parameter set: guard rows on either side of the k rows and tails behind the vector
size carry a NaN payload that must survive; B must come back unchanged.  coarse_block_info() must report block launches for
every k >= 2 -- so nothing here passes by looping over the columns --, the same number per group of 2 or 4 columns whatever k
is, and the one-vector launches of the matrices that have no block form.  Where the solver has to loop (tables left on,
n_cycles 2, lu_dense) the width is 1 and there is no block launch."""
import ctypes as C

import pytest
import torch

import mfmg_amd as M
from mfmg_amd.api import SparseMatrixDevice, block_groups
from mfmg_amd.lib import check

pytestmark = pytest.mark.gpu

N = (52, 52, 52)
KS = [1, 3, 4, 7]
K_MAX = max(KS)
PAYLOAD = 0x7FF8DEAD0000BEEF


def _params(is_preconditioner, pre_smoothing_levels=None, solver=None, **amg):
    amg = {"coarsest_size": 40, **amg}
    if pre_smoothing_levels is not None:
        amg["pre_smoothing_levels"] = pre_smoothing_levels
    return {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": is_preconditioner,
            "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0},
            "solver": solver or {"type": "amg", "amg": amg}}


def _hierarchy(ctx, material, params):
    return M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", M.LaplaceProblem(N, material, device="cuda"), params)


def _amg_matrices(h):
    """[(level, which, form(), block width)] of the matrices of the aggregation hierarchy: which 0 A_l, 1 P_l, 2 P_l^T, 3 P~_l
    (one borrowed view at a time: the library hands out one)."""
    n = C.c_int32()
    check(h._lib.mfmg_hip_hierarchy_coarse_amg_levels(h.handle, C.byref(n)))
    smoothed = [i["smoothed"] for i in h.coarse_amg_setup_info()]
    out = []
    for l in range(n.value):
        for which in (0, 1, 2, 3):
            if (which in (1, 2) and l + 1 == n.value) or (which == 3 and not smoothed[l]):
                continue
            p = C.c_void_p()
            check(h._lib.mfmg_hip_hierarchy_coarse_amg_get(h.handle, l, which, C.byref(p)))
            m = SparseMatrixDevice(h.ctx, _handle=p, _borrowed=True, _keepalive=h)
            out.append((l, which, m.form(), m.block_info()["width"]))
    return out


def _even(n):
    return n + 6 + (n & 1)


def _guarded(cols, ld):
    blk = torch.full((len(cols) + 2, ld), PAYLOAD, dtype=torch.int64, device="cuda").view(torch.float64)
    for c, v in enumerate(cols):
        blk[c + 1, :v.numel()] = v
    return blk


def _untouched(t):
    return bool((t.contiguous().view(torch.int64) == PAYLOAD).all().item())


def _wide_groups(k):
    return len([w for w in block_groups(k) if w > 1])


def _vectors(n, seed, count=K_MAX):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return [torch.randn(n, dtype=torch.float64, device="cuda", generator=g) for _ in range(count)]


def _check_block(ctx, what, k, n, call_block, b, x0, single):
    """call_block(B, X) on guarded blocks of the first k vectors against the one-vector results `single`."""
    ld = _even(n)
    B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
    call_block(B[1:k + 1], X[1:k + 1])
    ctx.synchronize()
    for col in range(k):
        got = X[col + 1, :n]
        assert torch.equal(got, single[col]), f"{what} k {k}: column {col} differs from the one-vector call in {(got != single[col]).sum().item()} entries"
    assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, n:]), f"{what} k {k}: wrote outside its columns"
    assert _untouched(B[0]) and _untouched(B[k + 1]) and _untouched(B[1:k + 1, n:]), f"{what} k {k}: wrote into the block b"
    assert all(torch.equal(B[col + 1, :n], b[col]) for col in range(k)), f"{what} k {k}: b changed"


def _singles(ctx, call, b, x0):
    out = []
    for col in range(len(b)):
        x = x0[col].clone()
        call(b[col], x)
        out.append(x)
    ctx.synchronize()
    assert all(bool(torch.isfinite(v).all().item()) for v in out)
    return out


@pytest.mark.parametrize("is_preconditioner", [True, False], ids=["preconditioner", "solver"])
@pytest.mark.parametrize("pre", [None, 0], ids=["V11", "V01"])
@pytest.mark.parametrize("material", ["linear", "discontinuous"])
def test_the_coarse_cycle_on_blocks_gives_the_bits_of_the_columns(ctx, material, pre, is_preconditioner):
    h = _hierarchy(ctx, material, _params(is_preconditioner, pre))
    what = f"{material} pre_smoothing_levels {pre} preconditioner {is_preconditioner}"
    # the forms the case is here for
    fc = h.coarse_operator().form()
    assert fc["kind"] == 3 and fc["regular"] == 0 and fc["stored_kernel"] == "sym_split", fc
    assert h.coarse_operator().block_info()["width"] == 4
    mats = _amg_matrices(h)
    assert mats[0][:2] == (0, 0) and mats[0][2]["stored_kernel"] == "sym_split" and mats[0][3] == 4, mats[0]
    # (no prolongator or P~ with kind 4 at any small mesh, see the docstring: they take the loop inside the block cycle)
    assert all(width == 1 and f["kind"] != 4 for l, which, f, width in mats[1:]), [(l, w, f["kind"], width) for l, w, f, width in mats]
    assert h.coarse_block_info()["width"] == 4 and h.block_info()["width"] == 4
    nf, nc = h.level_size(0), h.level_size(1)
    assert nc == 2 * 26 ** 3

    # ---- the coarse solver alone
    bc, xc = _vectors(nc, 21), _vectors(nc, 22)
    single = _singles(ctx, h.coarse_apply, bc, xc)
    per_group = set()
    loops = {}
    for k in KS:
        _check_block(ctx, f"{what}: coarse_apply_block", k, nc, h.coarse_apply_block, bc, xc, single)
        info = h.coarse_block_info()
        assert info["width"] == 4, info
        if k >= 2:
            assert info["block_launches"] > 0, (what, k, info)
            assert info["block_launches"] % _wide_groups(k) == 0, (what, k, info)
            per_group.add(info["block_launches"] // _wide_groups(k))
        else:
            assert info["block_launches"] == 0, (what, k, info)
        loops[k] = info["column_launches"]
    assert len(per_group) == 1, (what, per_group)
    # one-vector launches: a whole cycle for the odd last column, and per column of a group the matrices without a block form
    assert loops[1] > 0 and loops[3] > loops[1] and loops[7] - loops[3] == loops[4], (what, loops)

    # ---- the cycle and the operator form of it
    b, x0 = _vectors(nf, 23), _vectors(nf, 24)
    single = _singles(ctx, h.apply, b, x0)
    single_v = _singles(ctx, lambda bb, xx: h.vmult(xx, bb), b, x0)
    assert all(torch.equal(u, v) for u, v in zip(single, single_v))
    for k in KS:
        _check_block(ctx, f"{what}: apply_block", k, nf, h.apply_block, b, x0, single)
        info = h.coarse_block_info()
        assert info["block_launches"] == (next(iter(per_group)) * _wide_groups(k)), (what, k, info)
        _check_block(ctx, f"{what}: vmult_block", k, nf, lambda B, X: h.vmult_block(X, B), b, x0, single)
        assert h.coarse_block_info()["block_launches"] == info["block_launches"], (what, k)

    # ---- block CG through it (a symmetric cycle: V(1,1) only; solve_cg asks for "is preconditioner" true)
    if pre is None and is_preconditioner:
        ref = []
        for col in range(K_MAX):
            x = x0[col].clone()
            it, hist = h.solve_cg(b[col], x, 1e-8, 200)
            ref.append((x, it, hist.copy()))
        ctx.synchronize()
        ld = _even(nf)
        for k in KS:
            B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
            its, hists, _ = h.solve_cg_block(B[1:k + 1], X[1:k + 1], [1e-8] * k, 200)
            ctx.synchronize()
            for col in range(k):
                assert its[col] == ref[col][1], (what, k, col, its, [r[1] for r in ref])
                assert hists[col].tobytes() == ref[col][2].tobytes(), f"{what}: solve_cg_block k {k}: history of column {col} differs"
                assert torch.equal(X[col + 1, :nf], ref[col][0]), f"{what}: solve_cg_block k {k}: x of column {col} differs from solve_cg"
            assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nf:])
            if k >= 2:
                assert h.coarse_block_info()["block_launches"] > 0, (what, k)


@pytest.mark.parametrize("tables", [False, True], ids=["stored", "tables"])
def test_constant_coefficient_with_and_without_its_tables(ctx, tables):
    """`constant`: A_c repeats its rows and runs from tables -- no block form, the solver loops.  With the tables switched off
    (coarse_amg_kernels(regular_rows=False)) the same matrix is stored planes and the block cycle takes it."""
    h = _hierarchy(ctx, "constant", _params(True))
    assert h.coarse_operator().form()["regular"] == 1
    if not tables:
        h.coarse_amg_kernels(regular_rows=False)
        f = h.coarse_operator().form()
        assert f["regular"] == 0 and f["stored_kernel"] == "sym_split", f
    want = 1 if tables else 4
    assert h.coarse_block_info()["width"] == want
    nc = h.level_size(1)
    bc, xc = _vectors(nc, 31, 4), _vectors(nc, 32, 4)
    single = _singles(ctx, h.coarse_apply, bc, xc)
    for k in (3, 4):
        _check_block(ctx, f"constant tables {tables}: coarse_apply_block", k, nc, h.coarse_apply_block, bc, xc, single)
        info = h.coarse_block_info()
        assert info["width"] == want
        assert (info["block_launches"] == 0) if tables else (info["block_launches"] > 0), info
        assert info["column_launches"] > 0


@pytest.mark.parametrize("params", [_params(True, n_cycles=2), _params(True, solver={"type": "lu_dense"})], ids=["n_cycles_2", "lu_dense"])
def test_solvers_that_take_the_loop(ctx, params):
    n = (8, 8, 8)                          # (a dense factorisation of the first coarse level: a small one)
    lu = params["solver"]["type"] == "lu_dense"
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", M.LaplaceProblem(N if not lu else n, "linear", device="cuda"), params)
    if not lu:
        assert h.coarse_operator().block_info()["width"] == 4          # (the matrix would; the solver does not)
    assert h.coarse_block_info()["width"] == 1
    nc = h.level_size(1)
    bc, xc = _vectors(nc, 41, 4), _vectors(nc, 42, 4)
    single = _singles(ctx, h.coarse_apply, bc, xc)
    for k in (3, 4):
        _check_block(ctx, f"{params['solver']}: coarse_apply_block", k, nc, h.coarse_apply_block, bc, xc, single)
        info = h.coarse_block_info()
        assert info["width"] == 1 and info["block_launches"] == 0, info
    nf = h.level_size(0)
    b, x0 = _vectors(nf, 43, 4), _vectors(nf, 44, 4)
    single = _singles(ctx, h.apply, b, x0)
    _check_block(ctx, f"{params['solver']}: apply_block", 4, nf, h.apply_block, b, x0, single)
    assert h.coarse_block_info()["block_launches"] == 0
