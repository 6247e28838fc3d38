"""Hierarchy.solve_fgmres_block against k calls of solve_fgmres on the same hierarchy, bit for bit: x, the iteration count, the
final residual and the whole residual history of every column.

Hierarchies: Chebyshev(3), two eigenvectors, 2 x 2 x 2 agglomerates, "is preconditioner" true.  (16,16,16) `linear` with the
default symmetric cycle; (16,16,16) `constant` and (20,12,10) `discontinuous` with the non-symmetric V(0,1) coarse cycle of
tests/test_gpu_fgmres.py; `linear` under deal.II's numbering in caller mode and with "internal numbering" lexicographic; `linear`
with "fine level precision" float, V(0,1) and the FP32 fine level as preconditioner.  `constant` has no block kernel: the loop
over the columns under the cycle, the block basis kernels above it.  Restart 30 (one cycle) and 3 (several).
Column c has a random b and a random initial guess and the tolerance ||b_c|| 10^(-2 - c): the columns retire at different
iterations, inside a cycle and at a cycle start.  Of the seven columns, column 5 is b = 0, x0 = 0 (zero iterations) and column 6
starts from the result of a one-vector solve to 1e-12 (zero iterations or one).  k = 1, 3, 4, 7 in that order on ONE hierarchy,
then 3 again: the second solve with fewer columns runs in the bases of the first.
Breakdown: b = e_c with c a Dirichlet DoF in column 1 of four (tests/test_gpu_fgmres.py,
test_breakdown_ends_the_cycle_and_the_true_residual_decides): h_{1,0} = 0 in the first step of that column alone.

work["cycle_starts"] is derived from the one-vector histories: a column with `its` iterations in cycles of m starts 1 + its // m
cycles, one fewer when its is a positive multiple of m and the last recorded residual met the tolerance (it converged inside the
cycle, not at the restart that would have followed), one more after a breakdown."""
import ctypes as C

import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L

pytestmark = pytest.mark.gpu

K_MAX = 7
MAX_ITERATIONS = 100
PAYLOAD = 0x7FF8DEAD0000BEEF          # a quiet NaN nobody computes
KS = [1, 3, 4, 7, 3]
CHEB3 = {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}
V01 = {"type": "amg", "amg": {"coarsest_size": 300, "pre_smoothing_levels": 0}}   # the non-symmetric coarse cycle
# name: (nodes, material, numbering, extra parameters, preconditioner)
CASES = {"linear_symmetric": ((16, 16, 16), "linear", None, {}, "double"),
         "constant_v01": ((16, 16, 16), "constant", None, {"solver": V01}, "double"),
         "discontinuous_v01": ((20, 12, 10), "discontinuous", None, {"solver": V01}, "double"),
         "linear_dealii_caller": ((16, 16, 16), "linear", "dealii", {"internal numbering": "caller"}, "double"),
         "linear_dealii_lexicographic": ((16, 16, 16), "linear", "dealii", {"internal numbering": "lexicographic"}, "double"),
         "linear_v01_fp32": ((16, 16, 16), "linear", None, {"solver": V01, "fine level precision": "float"}, "float")}


def _params(extra):
    p = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": True,
         "max levels": 2, "smoother": dict(CHEB3)}
    p.update(extra)
    return p


_built = {}


def _case(ctx, name):
    """the hierarchy of a case, its right-hand sides, initial guesses and tolerances: built once, shared, left unchanged"""
    if name not in _built:
        n, material, numbering, extra, pre = CASES[name]
        kw = {"dof_numbering": M.dealii_numbering(n)} if numbering == "dealii" else {}
        prob = M.LaplaceProblem(n, material, device="cuda", **kw)
        h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, _params(extra))
        nd = h.level_size(0)
        g = torch.Generator(device="cuda")
        g.manual_seed(11)
        b = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
        x0 = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
        b[5].zero_()
        x0[5].zero_()
        try:
            h.solve_fgmres(b[6], x0[6], 1e-12, MAX_ITERATIONS, preconditioner=pre)
        except L.MfmgError:
            pass                                             # (stagnated above 1e-12: x0[6] is what was reached)
        tol = [float(torch.linalg.norm(b[c]).item()) * 10.0 ** (-2 - c) for c in range(K_MAX)]
        _built[name] = dict(h=h, prob=prob, nd=nd, b=b, x0=x0, tol=tol, pre=pre, block=material != "constant")
    return _built[name]


def _single(h, b, x0, tol, max_iterations, restart, pre):
    """solve_fgmres on a copy of x0: (x, iterations, final residual, history, converged)"""
    x = x0.clone()
    it, res = C.c_int32(), C.c_double()
    hist = np.zeros(max_iterations + 1)
    status = h._lib.mfmg_hip_hierarchy_solve_fgmres(h.handle, b.data_ptr(), x.data_ptr(), tol, max_iterations, restart, int(pre == "float"),
                                                    C.byref(it), C.byref(res), hist.ctypes.data_as(C.POINTER(C.c_double)), len(hist))
    assert status in (L.SUCCESS, L.ERROR_RUNTIME), h._lib.mfmg_hip_last_error().decode()
    return x, it.value, res.value, hist[: it.value + 1].copy(), status == L.SUCCESS


def _guarded(cols, ld):
    blk = torch.full((len(cols) + 2, ld), PAYLOAD, dtype=torch.int64, device="cuda").view(torch.float64)
    for c, v in enumerate(cols):
        blk[c + 1, :v.numel()] = v
    return blk


def _untouched(t):
    return bool((t.contiguous().view(torch.int64) == PAYLOAD).all().item())


def _cycle_starts(its, hist, tol, m, broke_down=False):
    starts = 1 + its // m
    if its > 0 and its % m == 0 and hist[its] <= tol:
        starts -= 1
    return starts + int(broke_down)


def _compare(what, case, k, restart, out, ref, B, X, b, tol, breakdown_column=None):
    its, hists, work = out
    nd = case["nd"]
    assert its == [r[1] for r in ref], (what, its, [r[1] for r in ref])
    for c in range(k):
        assert torch.equal(X[c + 1, :nd], ref[c][0]), f"{what}: x of column {c} differs from solve_fgmres in {(X[c + 1, :nd] != ref[c][0]).sum().item()} entries"
        assert len(hists[c]) == its[c] + 1 and hists[c].tobytes() == ref[c][3].tobytes(), (what, c, hists[c], ref[c][3])
        assert np.float64(work["residuals"][c]).tobytes() == np.float64(ref[c][2]).tobytes(), (what, c, work["residuals"][c], ref[c][2])
        assert torch.equal(B[c + 1, :nd], b[c]), f"{what}: b changed"
    assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nd:]), f"{what}: wrote outside its columns"
    assert _untouched(B[0]) and _untouched(B[k + 1]) and _untouched(B[1:k + 1, nd:]), f"{what}: wrote into b"
    assert work["preconditioner_columns"] == work["operator_columns"] == sum(its), (what, work, its)
    m = min(restart, MAX_ITERATIONS)
    want = sum(_cycle_starts(its[c], ref[c][3], tol[c], m, c == breakdown_column) for c in range(k))
    assert work["cycle_starts"] == want, (what, work, want)
    # the block kernel: where the fine level has one and two neighbouring columns are there (the first residuals already are)
    if case["block"] and k >= 2:
        assert work["block_launches"] > 0, (what, work)
    else:
        assert work["block_launches"] == 0, (what, work)


@pytest.mark.parametrize("restart", [30, 3], ids=["restart30", "restart3"])
@pytest.mark.parametrize("name", list(CASES))
def test_block_fgmres_equals_the_one_vector_driver(ctx, name, restart):
    case = _case(ctx, name)
    h, nd, b, x0, tol, pre = case["h"], case["nd"], case["b"], case["x0"], case["tol"], case["pre"]
    ld = nd + 6 + (nd & 1)
    assert h.block_info()["width"] == (4 if case["block"] else 1)
    # the one-vector driver, once per column: what every block run below is compared with
    ref = [_single(h, b[c], x0[c], tol[c], MAX_ITERATIONS, restart, pre) for c in range(K_MAX)]
    assert all(r[4] for r in ref)
    ref_its = [r[1] for r in ref]
    print(f"{name} restart {restart}: iterations of the one-vector driver {ref_its}")
    # otherwise retiring is never reached
    assert 0 in ref_its and ref_its[5] == 0 and ref_its[6] <= 1 and len(set(ref_its)) > 2, ref_its

    for k in KS:
        B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
        out = h.solve_fgmres_block(B[1:k + 1], X[1:k + 1], tol[:k], MAX_ITERATIONS, restart=restart, preconditioner=pre)
        ctx.synchronize()
        _compare(f"{name} restart {restart} k {k}", case, k, restart, out, ref[:k], B, X, b, tol)

    # ---- a breakdown in column 1 of four: b = e_c, c a Dirichlet DoF, from x = 0 to 1e-12 ----
    k = 4
    dirichlet = int(np.flatnonzero(case["prob"].constrained.cpu().numpy() == 1)[7])
    bb, xx, tt = list(b[:k]), list(x0[:k]), list(tol[:k])
    bb[1] = torch.zeros(nd, dtype=torch.float64, device="cuda")
    bb[1][dirichlet] = 1.0
    xx[1] = torch.zeros(nd, dtype=torch.float64, device="cuda")
    tt[1] = 1e-12
    one = _single(h, bb[1], xx[1], tt[1], MAX_ITERATIONS, restart, pre)
    broke_down = one[1] == 1 and one[3][0] == 1.0 and one[3][1] <= 1e-12 and int(torch.count_nonzero(one[0]).item()) == 1
    if pre == "double":
        assert one[4] and broke_down, (name, one[1], one[3])    # the input of test_breakdown_ends_the_cycle_...: one iteration, x = e_c
    ref4 = [ref[0], one, ref[2], ref[3]]
    B, X = _guarded(bb, ld), _guarded(xx, ld)
    out = h.solve_fgmres_block(B[1:k + 1], X[1:k + 1], tt, MAX_ITERATIONS, restart=restart, preconditioner=pre)
    ctx.synchronize()
    _compare(f"{name} restart {restart} breakdown", case, k, restart, out, ref4, B, X, bb, tt, breakdown_column=1 if broke_down else None)

    # ---- no convergence within two iterations: the error class of solve_fgmres, the outputs filled ----
    B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
    two = [_single(h, b[c], x0[c], tol[c], 2, restart, pre) for c in range(k)]
    assert not all(t[4] for t in two)
    with pytest.raises(L.MfmgError, match="did not reach the tolerance") as info:
        h.solve_fgmres_block(B[1:k + 1], X[1:k + 1], tol[:k], 2, restart=restart, preconditioner=pre)
    assert type(info.value) is L.MfmgError
    ctx.synchronize()
    its, hists, work = h.last_block_solve
    for c in range(k):
        assert its[c] == two[c][1] and hists[c].tobytes() == two[c][3].tobytes(), (c, its, hists[c], two[c][3])
        assert np.float64(work["residuals"][c]).tobytes() == np.float64(two[c][2]).tobytes(), c
        assert torch.equal(X[c + 1, :nd], two[c][0]), f"column {c} after two iterations"
    assert work["preconditioner_columns"] == work["operator_columns"] == sum(its)
    assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nd:])


def test_refusals(ctx):
    case = _case(ctx, "linear_symmetric")
    h, nd = case["h"], case["nd"]                              # 4913: odd
    new = lambda rows, ld: torch.zeros((rows, ld), dtype=torch.float64, device="cuda")
    ld = nd + 7
    with pytest.raises(L.MfmgInvalidArgument, match="even"):
        h.solve_fgmres_block(new(2, nd + 2), new(2, nd + 2), [1.0, 1.0])
    with pytest.raises(L.MfmgInvalidArgument, match="1 to 64"):
        h.solve_fgmres_block(new(65, ld), new(65, ld), [1.0] * 65)
    big = new(4, ld)
    with pytest.raises(L.MfmgInvalidArgument, match="overlap"):
        h.solve_fgmres_block(big[0:2], big[1:3], [1.0, 1.0])
    with pytest.raises(L.MfmgInvalidArgument, match="stopping criterion"):
        h.solve_fgmres_block(new(2, ld), new(2, ld), [1.0, -1e-300])
    with pytest.raises(L.MfmgInvalidArgument, match="restart"):
        h.solve_fgmres_block(new(2, ld), new(2, ld), [1.0, 1.0], restart=0)
    with pytest.raises(L.MfmgInvalidArgument, match="fine level precision"):
        h.solve_fgmres_block(new(2, ld), new(2, ld), [1.0, 1.0], preconditioner="float")
    with pytest.raises(L.MfmgInvalidArgument, match="preconditioner"):
        h.solve_fgmres_block(new(2, ld), new(2, ld), [1.0, 1.0], preconditioner="half")
    # and a good call right after the refused ones
    B, X = new(2, ld), new(2, ld)
    B[:, :nd] = 1.0
    its, hists, work = h.solve_fgmres_block(B, X, [1e-6, 1e-3])
    assert its[0] > its[1] > 0 and work["operator_columns"] == sum(its)


def test_bases_that_cannot_be_allocated_leave_no_workspace_behind(ctx):
    """restart = max_iterations = 2^30 on three columns of 4913 DoFs asks for 2^31 + 1 blocks of three vectors, 250 TB: the
    allocation is refused with the device error; the next solve on the same hierarchy allocates afresh and gives the bits of the
    solve before (tests/test_gpu_fgmres.py, test_a_basis_that_cannot_be_allocated_leaves_no_workspace_behind, in block form)."""
    case = _case(ctx, "linear_symmetric")
    h, nd, b, x0, tol = case["h"], case["nd"], case["b"], case["x0"], case["tol"]
    k, ld = 3, nd + 1
    block = lambda cols: torch.stack([torch.cat([v, v.new_zeros(ld - nd)]) for v in cols])
    X_before = block(x0[:k])
    before = h.solve_fgmres_block(block(b[:k]), X_before, tol[:k], MAX_ITERATIONS, restart=5)
    Xz, tols = block(x0[:k]), (C.c_double * k)(*tol[:k])
    status = h._lib.mfmg_hip_hierarchy_solve_fgmres_block(h.handle, k, ld, block(b[:k]).data_ptr(), Xz.data_ptr(), tols, 2 ** 30, 2 ** 30, 0,
                                                          None, None, None, 0, None)
    assert status == L.ERROR_DEVICE
    assert "memory" in h._lib.mfmg_hip_last_error().decode().lower()
    assert torch.equal(Xz, block(x0[:k]))                                 # nothing was launched on x
    for restart in (5, 30):                                               # the same and larger bases than before the failure
        X = block(x0[:k])
        out = h.solve_fgmres_block(block(b[:k]), X, tol[:k], MAX_ITERATIONS, restart=restart)
        ctx.synchronize()
        if restart == 5:
            assert out[0] == before[0] and all(a.tobytes() == c.tobytes() for a, c in zip(out[1], before[1]))
            assert torch.equal(X, X_before)
        for c in range(k):
            ref = _single(h, b[c], x0[c], tol[c], MAX_ITERATIONS, restart, "double")
            assert torch.equal(X[c, :nd], ref[0]) and out[0][c] == ref[1]
