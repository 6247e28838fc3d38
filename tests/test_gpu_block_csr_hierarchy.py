"""Hierarchy.set_block_csr: the block forms of the CSR kernels in the coarse cycle, on the fine level of an assembled operator
and in the bottom solve -- column by column against the one-vector calls, bit for bit (the pattern of
test_gpu_block_coarse_cycle.py: guard rows and tails with a NaN payload, B unchanged, k = 1, 3, 4, 7).

(24, 24, 24) cells: the first coarse operator has 2 * 12^3 = 3456 rows, so every matrix of the aggregation hierarchy runs a CSR
kernel and by default the whole coarse cycle loops over the columns (coarse_block_info()["width"] == 1).  With the switch every
such matrix reports the width 4; where the test finds all of them there and the return value says that the two triangular
inverses of the bottom flipped too, a group of four launches no one-vector kernel at all.  (52, 52, 52): A_c is on stored
planes already, the matrices below it gain.  HipMeshEvaluator at (16, 16, 16): the fine operator itself is CSR.  The solver-level
rules stay: n_cycles 2 and lu_dense keep the loop whatever the matrices offer."""
import pytest
import torch

import mfmg_amd as M
from test_gpu_block_coarse_cycle import KS, K_MAX, _amg_matrices, _check_block, _even, _guarded, _params, _singles, _untouched, _vectors, _wide_groups

pytestmark = pytest.mark.gpu

SMALL, LARGE = (24, 24, 24), (52, 52, 52)


def _hierarchy(ctx, cells, material, params, evaluator="HipMatrixFreeMeshEvaluator"):
    return M.Hierarchy(ctx, evaluator, M.LaplaceProblem(cells, material, device="cuda"), params)


def _mats(h):
    """_amg_matrices without the fields of form() that record the last launch."""
    return [(l, which, {k: v for k, v in f.items() if k not in ("pairs", "twin_wide")}, width) for l, which, f, width in _amg_matrices(h)]


def _is_csr(f):
    return f["kind"] in (0, 1) and f["csr_kernel"] in ("lanes", "row_block", "lds")


def _flip_and_check(h, mats_before, extra=0):
    """set_block_csr(True): every matrix on a CSR kernel at width 4, the others as they were; returns whether every matrix of
    the coarse cycle -- the bottom inverses included, which only the return value shows -- is at width 4."""
    n = h.set_block_csr(True)
    mats = _mats(h)
    assert [(l, w, f) for l, w, f, _ in mats] == [(l, w, f) for l, w, f, _ in mats_before]      # (no form changed)
    for (l, which, f, width), (_, _, _, was) in zip(mats, mats_before):
        assert width == (4 if _is_csr(f) else was), (l, which, f, width, was)
    flipped = sum(1 for l, which, f, width in mats if _is_csr(f))
    assert flipped > 0 and n - extra in (flipped, flipped + 2), (n, extra, flipped)
    return all(width == 4 for _, _, _, width in mats) and n - extra == flipped + 2


def _coarse_counters(ctx, h, k, bc, xc, single, what):
    _check_block(ctx, what, k, h.level_size(1), h.coarse_apply_block, bc, xc, single)
    return h.coarse_block_info()


@pytest.mark.parametrize("pre", [None, 0], ids=["V11", "V01"])
def test_the_whole_aggregation_hierarchy_on_csr_block_kernels(ctx, pre):
    h = _hierarchy(ctx, SMALL, "linear", _params(True, pre))
    what = f"linear {SMALL} pre_smoothing_levels {pre}"
    nf, nc = h.level_size(0), h.level_size(1)
    assert nc == 2 * 12 ** 3
    before = _mats(h)
    assert all(_is_csr(f) and width == 1 for _, _, f, width in before), [(l, w, f["kind"], width) for l, w, f, width in before]
    assert h.coarse_block_info()["width"] == 1 and h.coarse_operator().block_info()["width"] == 1
    bc, xc = _vectors(nc, 21), _vectors(nc, 22)
    single = _singles(ctx, h.coarse_apply, bc, xc)
    default = _coarse_counters(ctx, h, 4, bc, xc, single, f"{what}: default")
    assert default["width"] == 1 and default["block_launches"] == 0 and default["column_launches"] > 0, default

    all_wide = _flip_and_check(h, before)
    assert all_wide                                                       # (every level and the bottom: nothing here has tables)
    assert h.coarse_block_info()["width"] == 4 and h.coarse_operator().block_info()["width"] == 4
    per_group = set()
    for k in KS:
        info = _coarse_counters(ctx, h, k, bc, xc, single, f"{what}: coarse_apply_block")
        assert info["width"] == 4
        if k >= 2:
            assert info["block_launches"] > 0 and info["block_launches"] % _wide_groups(k) == 0, (what, k, info)
            per_group.add(info["block_launches"] // _wide_groups(k))
        else:
            assert info["block_launches"] == 0, (what, k, info)
        if k == 4:
            assert info["column_launches"] < default["column_launches"], (what, info, default)
            assert info["column_launches"] == 0, (what, info)             # all_wide: no one-vector kernel for a group of four
    assert len(per_group) == 1, (what, per_group)

    # ---- the cycle and the operator form of it
    b, x0 = _vectors(nf, 23), _vectors(nf, 24)
    single_f = _singles(ctx, h.apply, b, x0)
    for k in KS:
        _check_block(ctx, f"{what}: apply_block", k, nf, h.apply_block, b, x0, single_f)
        info = h.coarse_block_info()
        assert info["block_launches"] == next(iter(per_group)) * _wide_groups(k), (what, k, info)
        _check_block(ctx, f"{what}: vmult_block", k, nf, lambda B, X: h.vmult_block(X, B), b, x0, single_f)

    # ---- the block solves through it: CG needs the symmetric cycle, FGMRES takes V(0,1)
    solve, solve_block = (h.solve_cg, h.solve_cg_block) if pre is None else (h.solve_fgmres, h.solve_fgmres_block)
    ref = []
    for col in range(K_MAX):
        x = x0[col].clone()
        it, hist = solve(b[col], x, 1e-8, 200)
        ref.append((x, it, hist.copy()))
    ctx.synchronize()
    ld = _even(nf)
    for k in KS:
        B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
        its, hists, _ = solve_block(B[1:k + 1], X[1:k + 1], [1e-8] * k, 200)
        ctx.synchronize()
        for col in range(k):
            assert its[col] == ref[col][1], (what, k, col, its, [r[1] for r in ref])
            assert hists[col].tobytes() == ref[col][2].tobytes(), f"{what}: block solve k {k}: history of column {col} differs"
            assert torch.equal(X[col + 1, :nf], ref[col][0]), f"{what}: block solve k {k}: x of column {col} differs"
        assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nf:])
        if k >= 2:
            assert h.coarse_block_info()["block_launches"] > 0, (what, k)

    # ---- off again: the widths and counters of an untouched hierarchy
    assert h.set_block_csr(False) == 0
    assert _mats(h) == before and h.coarse_block_info()["width"] == 1
    again = _coarse_counters(ctx, h, 4, bc, xc, single, f"{what}: switched off")
    assert again == default, (again, default)


def test_stored_planes_on_top_csr_below(ctx):
    h = _hierarchy(ctx, LARGE, "linear", _params(True))
    what = f"linear {LARGE}"
    nf, nc = h.level_size(0), h.level_size(1)
    before = _mats(h)
    assert before[0][2]["stored_kernel"] == "sym_split" and before[0][3] == 4           # A_c has its block form already
    bc, xc = _vectors(nc, 21), _vectors(nc, 22)
    single = _singles(ctx, h.coarse_apply, bc, xc)
    default = _coarse_counters(ctx, h, 4, bc, xc, single, f"{what}: default")
    assert default["width"] == 4 and default["block_launches"] > 0 and default["column_launches"] > 0
    all_wide = _flip_and_check(h, before)
    for k in KS:
        info = _coarse_counters(ctx, h, k, bc, xc, single, f"{what}: coarse_apply_block")
        if k == 4:
            assert info["column_launches"] < default["column_launches"] and info["block_launches"] > default["block_launches"], (info, default)
            assert not all_wide or info["column_launches"] == 0, info
    b, x0 = _vectors(nf, 23, 4), _vectors(nf, 24, 4)
    single_f = _singles(ctx, h.apply, b, x0)
    _check_block(ctx, f"{what}: apply_block", 4, nf, h.apply_block, b, x0, single_f)


def test_an_assembled_fine_operator_in_csr(ctx):
    cells = (16, 16, 16)
    h = _hierarchy(ctx, cells, "linear", _params(True), evaluator="HipMeshEvaluator")
    what = f"HipMeshEvaluator {cells}"
    nf = h.level_size(0)
    fine = h.fine_operator()
    assert _is_csr(fine.form()) and fine.block_info()["width"] == 1 and h.block_info()["width"] == 1
    b, x0 = _vectors(nf, 33), _vectors(nf, 34)
    single = _singles(ctx, h.apply, b, x0)
    ref = []
    for col in range(K_MAX):
        x = x0[col].clone()
        it, hist = h.solve_cg(b[col], x, 1e-8, 200)
        ref.append((x, it, hist.copy()))
    ctx.synchronize()
    before = _mats(h)
    # (the fine operator is one more matrix the walk flips; a restrictor in CSR would be another)
    restrictor_csr = 0 if h.restrictor_form(1)["structured"] else 1
    _flip_and_check(h, before, extra=1 + restrictor_csr)
    assert fine.block_info()["width"] == 4 and h.block_info()["width"] == 4
    for k in KS:
        launches = fine.block_info()["block_launches"]
        _check_block(ctx, f"{what}: apply_block", k, nf, h.apply_block, b, x0, single)
        if k >= 2:
            assert fine.block_info()["block_launches"] > launches, (what, k)
    ld = _even(nf)
    for k in KS:
        launches = fine.block_info()["block_launches"]
        B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
        its, hists, _ = h.solve_cg_block(B[1:k + 1], X[1:k + 1], [1e-8] * k, 200)
        ctx.synchronize()
        for col in range(k):
            assert its[col] == ref[col][1] and hists[col].tobytes() == ref[col][2].tobytes(), (what, k, col)
            assert torch.equal(X[col + 1, :nf], ref[col][0]), f"{what}: solve_cg_block k {k}: x of column {col} differs from solve_cg"
        assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nf:])
        if k >= 2:
            assert fine.block_info()["block_launches"] > launches, (what, k)
    h.set_block_csr(False)
    assert fine.block_info()["width"] == 1 and h.block_info()["width"] == 1


def test_constant_coefficients_tables_stay_csr_flips(ctx):
    h = _hierarchy(ctx, SMALL, "constant", _params(True))
    nc = h.level_size(1)
    before = _mats(h)
    assert any(_is_csr(f) for _, _, f, _ in before)
    _flip_and_check(h, before)                                            # (a matrix on tables or node classes keeps its width 1)
    assert h.coarse_block_info()["width"] == 4
    bc, xc = _vectors(nc, 31, 4), _vectors(nc, 32, 4)
    single = _singles(ctx, h.coarse_apply, bc, xc)
    for k in (3, 4):
        info = _coarse_counters(ctx, h, k, bc, xc, single, "constant: coarse_apply_block")
        assert info["width"] == 4 and info["block_launches"] > 0, info


@pytest.mark.parametrize("params,cells", [(_params(True, n_cycles=2), SMALL), (_params(True, solver={"type": "lu_dense"}), (8, 8, 8))],
                         ids=["n_cycles_2", "lu_dense"])
def test_solvers_that_take_the_loop_with_the_switch_on(ctx, params, cells):
    h = _hierarchy(ctx, cells, "linear", params)
    h.set_block_csr(True)
    assert h.coarse_operator().block_info()["width"] == 4               # (the matrix would; the solver does not)
    assert h.coarse_block_info()["width"] == 1
    nc, nf = h.level_size(1), h.level_size(0)
    bc, xc = _vectors(nc, 41, 4), _vectors(nc, 42, 4)
    single = _singles(ctx, h.coarse_apply, bc, xc)
    for k in (3, 4):
        info = _coarse_counters(ctx, h, k, bc, xc, single, f"{params['solver']}: coarse_apply_block")
        assert info["width"] == 1 and info["block_launches"] == 0, info
    b, x0 = _vectors(nf, 43, 4), _vectors(nf, 44, 4)
    single = _singles(ctx, h.apply, b, x0)
    _check_block(ctx, f"{params['solver']}: apply_block", 4, nf, h.apply_block, b, x0, single)
    assert h.coarse_block_info()["block_launches"] == 0
