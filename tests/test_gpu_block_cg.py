"""Hierarchy.solve_cg_block against k calls of solve_cg on the same hierarchy, bit for bit: x, the iteration count, the final
residual and the whole residual history of every column.

Hierarchies as in test_gpu_block_hierarchy.py: Chebyshev(3), two eigenvectors, 2 x 2 x 2 agglomerates, "is preconditioner" true,
the default (symmetric) coarse cycle.  `linear` and `discontinuous` take the block kernel, `constant` the loop over the columns
under the cycle and the block vector kernels above it; `linear` under deal.II's numbering in caller mode and with "internal
numbering" lexicographic; (64,64,64) has 274,625 DoFs, where the reductions take a second grid-stride trip (k = 3 only).
Column c has a random b and a random initial guess and the tolerance ||b_c|| 10^(-2 - c): the columns retire at different
iterations.  Of the seven columns, column 5 is b = 0, x0 = 0 (zero iterations) and column 6 starts from the result of a one-vector
solve to 1e-12 (zero iterations or one).  k = 1, 3, 4, 7 in that order on ONE hierarchy, then 3 again: the second solve with
fewer columns runs in the working blocks of the first."""
import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L

pytestmark = pytest.mark.gpu

K_MAX = 7
MAX_ITERATIONS = 100
PAYLOAD = 0x7FF8DEAD0000BEEF          # a quiet NaN nobody computes
CASES = [((16, 16, 16), "linear", None, None, [1, 3, 4, 7, 3]), ((20, 12, 10), "discontinuous", None, None, [1, 3, 4, 7, 3]),
         ((16, 16, 16), "constant", None, None, [1, 3, 4, 7, 3]), ((16, 16, 16), "linear", "dealii", "caller", [1, 3, 4, 7, 3]),
         ((16, 16, 16), "linear", "dealii", "lexicographic", [1, 3, 4, 7, 3]), ((64, 64, 64), "linear", None, None, [3])]


def _params(mode, n):
    p = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": True,
         "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}}
    if mode is not None:
        p["internal numbering"] = mode
    if max(n) > 32:
        # 65,536 coarse rows are beyond the dense direct solver of the small cases: the multilevel coarse solver with its
        # default (symmetric) cycle
        p["solver"] = {"type": "amg", "amg": {"coarsest_size": 600}}
    return p


def _guarded(cols, ld):
    blk = torch.full((len(cols) + 2, ld), PAYLOAD, dtype=torch.int64, device="cuda").view(torch.float64)
    for c, v in enumerate(cols):
        blk[c + 1, :v.numel()] = v
    return blk


def _untouched(t):
    return bool((t.contiguous().view(torch.int64) == PAYLOAD).all().item())


def _hierarchy(ctx, n, material, numbering, mode):
    kw = {"dof_numbering": M.dealii_numbering(n)} if numbering == "dealii" else {}
    prob = M.LaplaceProblem(n, material, device="cuda", **kw)
    return M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, _params(mode, n))


def _single(h, b, x0, tol, max_iterations):
    """solve_cg on a copy of x0: (x, iterations, history, converged)"""
    x = x0.clone()
    try:
        it, hist = h.solve_cg(b, x, tol, max_iterations)
        return x, it, hist, True
    except L.MfmgError as e:
        assert "did not reach the tolerance" in str(e)
        return x, None, None, False


@pytest.mark.parametrize("n,material,numbering,mode,ks", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_block_cg_equals_the_one_vector_driver(ctx, n, material, numbering, mode, ks):
    h = _hierarchy(ctx, n, material, numbering, mode)
    nd = h.level_size(0)
    ld = nd + 6 + (nd & 1)
    block = material != "constant"
    assert h.block_info()["width"] == (4 if block else 1)
    k_max = max(ks)

    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    b = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(k_max)]
    x0 = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(k_max)]
    if k_max == K_MAX:
        b[5].zero_()
        x0[5].zero_()
        try:
            h.solve_cg(b[6], x0[6], 1e-12, MAX_ITERATIONS)
        except L.MfmgError:
            pass                                             # (stagnated above 1e-12: x0[6] is what was reached)
    tol = [float(torch.linalg.norm(b[c]).item()) * 10.0 ** (-2 - c) for c in range(k_max)]
    # the one-vector driver, once per column: what every block run below is compared with
    ref = [_single(h, b[c], x0[c], tol[c], MAX_ITERATIONS) for c in range(k_max)]
    assert all(r[3] for r in ref)
    ref_its = [r[1] for r in ref]
    print(f"{n} {material} {numbering} {mode}: iterations of the one-vector driver {ref_its}")
    if k_max == K_MAX:
        # otherwise the retire path is not reached
        assert 0 in ref_its and ref_its[5] == 0 and ref_its[6] <= 1 and len(set(ref_its)) > 2, ref_its
    else:
        assert len(set(ref_its)) > 1, ref_its

    for k in ks:
        B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
        its, hists, work = h.solve_cg_block(B[1:k + 1], X[1:k + 1], tol[:k], MAX_ITERATIONS)
        ctx.synchronize()
        what = f"{n} {material} {numbering} {mode} k {k}"
        assert its == ref_its[:k], (what, its, ref_its[:k])
        for c in range(k):
            assert torch.equal(X[c + 1, :nd], ref[c][0]), f"{what}: x of column {c} differs from solve_cg in {(X[c + 1, :nd] != ref[c][0]).sum().item()} entries"
            assert len(hists[c]) == its[c] + 1 and list(hists[c]) == list(ref[c][2]), (what, c, hists[c], ref[c][2])
            assert torch.equal(B[c + 1, :nd], b[c]), f"{what}: b changed"
        assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nd:]), f"{what}: wrote outside its columns"
        assert _untouched(B[0]) and _untouched(B[k + 1]) and _untouched(B[1:k + 1, nd:]), f"{what}: wrote into b"
        assert work["preconditioner_columns"] == work["operator_columns"] == sum(its), (what, work, its)
        assert 0 <= work["slot_moves"] <= k, (what, work)
        if not block:
            assert work["block_launches"] == 0, (what, work)
        elif k >= 2 and sorted(its)[-2] >= 1:               # at least two columns are active for at least one iteration
            assert work["block_launches"] > 0, (what, work)
        elif k == 1:
            assert work["block_launches"] == 0, (what, work)

    if k_max < 4:
        return
    # ---- no convergence within two iterations: the error class of solve_cg, the outputs filled ----
    k = 4
    B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
    two = [_single(h, b[c], x0[c], tol[c], 2) for c in range(k)]
    assert not all(t[3] for t in two)
    with pytest.raises(L.MfmgError, match="did not reach the tolerance") as info:
        h.solve_cg_block(B[1:k + 1], X[1:k + 1], tol[:k], 2)
    assert type(info.value) is L.MfmgError
    ctx.synchronize()
    its, hists, work = h.last_block_solve
    for c in range(k):
        want = min(ref_its[c], 2)
        assert its[c] == want and list(hists[c]) == list(ref[c][2][:want + 1]), (c, its, hists[c], ref[c][2])
        assert torch.equal(X[c + 1, :nd], two[c][0]), f"column {c} after two iterations"
    assert work["preconditioner_columns"] == work["operator_columns"] == sum(its)
    assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nd:])


@pytest.mark.parametrize("material", ["linear", "constant"])
def test_operator_apply_block_equals_operator_apply(ctx, material):
    h = _hierarchy(ctx, (16, 16, 16), material, None, None)
    nd = h.level_size(0)
    ld = nd + 6 + (nd & 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    x = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
    ref = []
    for c in range(K_MAX):
        y = torch.empty(nd, dtype=torch.float64, device="cuda")
        h.operator_apply(0, x[c], y)
        ref.append(y)
    for k in (1, 3, 4, 7):
        X = _guarded(x[:k], ld)
        Y = torch.full((k + 2, ld), PAYLOAD, dtype=torch.int64, device="cuda").view(torch.float64)
        h.operator_apply_block(0, X[1:k + 1], Y[1:k + 1])
        ctx.synchronize()
        for c in range(k):
            assert torch.equal(Y[c + 1, :nd], ref[c]), f"{material} k {k} column {c}"
            assert torch.equal(X[c + 1, :nd], x[c])
        assert _untouched(Y[0]) and _untouched(Y[k + 1]) and _untouched(Y[1:k + 1, nd:])
        launches = h.block_info()["block_launches"]
        assert launches == (len([w for w in M.api.block_groups(k) if w > 1]) if material == "linear" else 0), (material, k, launches)


def test_refusals(ctx):
    h = _hierarchy(ctx, (16, 16, 16), "linear", None, None)
    nd = h.level_size(0)                                       # 4913: odd
    new = lambda rows, ld: torch.zeros((rows, ld), dtype=torch.float64, device="cuda")
    ld = nd + 7
    with pytest.raises(L.MfmgInvalidArgument, match="even"):
        h.solve_cg_block(new(2, nd + 2), new(2, nd + 2), [1.0, 1.0])
    with pytest.raises(L.MfmgInvalidArgument, match="at least the vector size"):
        h.solve_cg_block(new(2, nd - 1), new(2, nd - 1), [1.0, 1.0])
    with pytest.raises(L.MfmgInvalidArgument):                # (an empty tensor has no address: refused as a null argument)
        h.solve_cg_block(new(2, ld)[1:1], new(2, ld)[1:1], [])
    with pytest.raises(L.MfmgInvalidArgument, match="1 to 64"):   # k = 0 with real blocks, at the C entry point
        import ctypes as C
        B0, X0, tol0 = new(1, ld), new(1, ld), (C.c_double * 1)(1.0)
        L.check(L.load().mfmg_hip_hierarchy_solve_cg_block(h.handle, 0, ld, B0.data_ptr(), X0.data_ptr(), tol0, 10, None, None, None, 0, None))
    with pytest.raises(L.MfmgInvalidArgument, match="1 to 64"):
        h.solve_cg_block(new(65, ld), new(65, ld), [1.0] * 65)
    big = new(4, ld)
    with pytest.raises(L.MfmgInvalidArgument, match="overlap"):
        h.solve_cg_block(big[0:2], big[1:3], [1.0, 1.0])
    with pytest.raises(L.MfmgInvalidArgument, match="stopping criterion"):
        h.solve_cg_block(new(2, ld), new(2, ld), [1.0, -1e-300])
    with pytest.raises(L.MfmgInvalidArgument, match="stopping criterion"):
        h.solve_cg_block(new(2, ld), new(2, ld), [1.0, 1.0], max_iterations=-1)
    # and a good call right after the refused ones
    B, X = new(2, ld), new(2, ld)
    B[:, :nd] = 1.0
    its, hists, work = h.solve_cg_block(B, X, [1e-6, 1e-3])
    assert its[0] > its[1] > 0 and work["operator_columns"] == sum(its)
