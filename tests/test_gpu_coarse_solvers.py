"""The coarse solvers on the device against long double (cases, references and the acceptance rule: coarse_solver_cases.py; what
the rule notices: test_coarse_solver_case_table.py).

Direct solvers, through SparseMatrixDevice.solve: every case of the table with lu_dense (at 65 rows cholesky and lu_sparse_host
too: the same bits), x prefilled with a NaN payload, b unchanged, a second call with the same bits; the exact cases entry by
entry with array_equal, the others through assert_solution.  Which implementation ran is asserted from the profiler: the explicit
inverses are two launches of csr_spmv_kernel that read two triangles of n (n + 1) / 2 entries, dense_lu_solve_kernel none.
NOT asserted: dense_lu_solve_kernel by name (it is launched outside the profiler: its run shows as zero SpMV launches and a
solution that replaced the payload) and the lanes per row on either side of 512 rows (every SpMV kernel is timed under the one
name csr_spmv_kernel, and the factors of a solve are not reachable for form()); the sizes 511, 512, 513 run and are held to the
bound all the same.

Through a hierarchy: coarse_apply on the Galerkin operators of (20,20,20) cells (2000 rows: inverses) and (22,22,18) cells
(2178 rows: the kernel), accepted by the same rule on the downloaded A_c; prints how many rows the pivoting moves there.

PCG: every size and iteration count against the long-double restatement; zeros for no iteration and for b = 0; D^-1 b bit for
bit on a diagonal of powers of two, where from the second step on only the guards stand between the solution and NaN.

Every test prints its worst measured fraction of the bound (pytest -s)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import coarse_solver_cases as C
import mfmg_amd as M
from mfmg_amd import lib as L

pytestmark = pytest.mark.gpu

PAYLOAD = 0x7FF8000000C0FFEE          # a quiet NaN that no arithmetic produces


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def payload(n):
    return torch.full((n,), PAYLOAD, dtype=torch.int64, device="cuda").view(torch.float64)


def bits(t):
    return t.view(torch.int64).cpu().numpy()


def solve(ctx, Ad, params, b, n):
    x = payload(n)
    Ad.solve({"solver": params}, b, x)
    ctx.synchronize()
    return x


@pytest.mark.parametrize("name", C.direct_names())
def test_direct_case(ctx, name):
    c = C.direct_case(name)
    n = c["n"]
    Ad = M.SparseMatrixDevice(ctx, c["A"])
    b = dev(c["b"])
    solvers = ("lu_dense", "cholesky", "lu_sparse_host") if n == 65 else ("lu_dense",)
    runs = [bits(solve(ctx, Ad, {"type": s}, b, n)) for s in solvers for _ in range(2)]
    for other in runs[1:]:
        assert np.array_equal(runs[0], other)                          # a second call, the other two names: the same bits
    assert np.array_equal(bits(b), c["b"].view(np.int64))
    got = runs[0].view(np.float64)
    assert not (runs[0] == PAYLOAD).any()
    if c["exact"]:
        assert np.array_equal(got, c["x_ref"].astype(np.float64))
        ratio = 0.0
    else:
        ratio = C.assert_solution(got, c)
    print(f"\n[coarse] {name}: n {n}, {c['path']}, rows moved {(c['perm'] != np.arange(n)).sum()}, forward and backward error "
          f"as fractions of the bound {C.measure(got, c)}, worst {ratio:.3g}")


@pytest.mark.parametrize("n", [511, 512, 513, 2048, 2049])
def test_the_path_that_ran(ctx, n):
    c = C.direct_case(f"rotated_{n}")
    Ad = M.SparseMatrixDevice(ctx, c["A"])
    b = dev(c["b"])
    ctx.profile_enable(True, only="csr_spmv_kernel")
    try:
        x = solve(ctx, Ad, {"type": "lu_dense"}, b, n)
        launches, _, nbytes = ctx.profile_query("csr_spmv_kernel")
    finally:
        ctx.profile_enable(False)
    if n <= C.INVERSE_LIMIT:
        triangle = n * (n + 1) // 2                                   # entries of L^-1 P, and of U^-1
        assert launches == 2 and nbytes == 2 * (12.0 * triangle + 4.0 * (n + 1) + 16.0 * n)
    else:
        assert launches == 0 and nbytes == 0                          # dense_lu_solve_kernel, which alone can have written x
    ratio = C.assert_solution(bits(x).view(np.float64), c)
    print(f"\n[coarse] path rotated_{n}: {launches} SpMV launches, worst {ratio:.3g}")


@pytest.mark.parametrize("cells,rows", [((20, 20, 20), 2000), ((22, 22, 18), 2178)])
def test_coarse_apply_of_a_hierarchy(ctx, cells, rows):
    prob = M.LaplaceProblem(cells, "linear", device="cuda")
    params = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": False,
              "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 2, "smoothing_range": 20.0}, "solver": {"type": "lu_dense"}}
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, params)
    A_c = h.coarse_operator().to_scipy()
    assert A_c.shape == (rows, rows)
    c = C.make_case(f"galerkin_{rows}", A_c, np.random.default_rng(rows).standard_normal(rows))
    assert c["path"] == ("inverse" if rows == 2000 else "substitution")
    b, x = dev(c["b"]), payload(rows)
    h.coarse_apply(b, x)
    ctx.synchronize()
    again = payload(rows)
    h.coarse_apply(b, again)
    ctx.synchronize()
    assert np.array_equal(bits(x), bits(again)) and np.array_equal(bits(b), c["b"].view(np.int64))
    got = bits(x).view(np.float64)
    ratio = C.assert_solution(got, c)
    moved = int((c["perm"] != np.arange(rows)).sum())
    print(f"\n[coarse] galerkin {cells}: {rows} rows, {c['path']}, partial pivoting moves {moved} rows, forward and backward error "
          f"as fractions of the bound {C.measure(got, c)}, worst {ratio:.3g}")
    with pytest.raises(L.MfmgError, match="cannot run in place"):
        h.coarse_apply(x, x)
    assert np.array_equal(bits(x), bits(again))


def test_refusals_leave_x_alone(ctx):
    def refused(A, params, match, error=L.MfmgError):
        n = A.shape[0]
        x = payload(n)
        with pytest.raises(error, match=match):
            M.SparseMatrixDevice(ctx, A).solve({"solver": params}, dev(np.ones(n)), x)
        ctx.synchronize()
        assert (bits(x) == PAYLOAD).all()

    zero_row = C.tridiag(8).tolil()
    zero_row[3, :] = 0
    zero_row = zero_row.tocsr()
    zero_row.eliminate_zeros()
    assert zero_row.indptr[4] == zero_row.indptr[3]
    refused(zero_row, {"type": "lu_dense"}, "singular matrix")
    refused(C.tridiag(40), {"type": "lu_dense", "dense_limit": 39}, "too large for the dense direct solver")
    x = solve(ctx, M.SparseMatrixDevice(ctx, C.tridiag(40)), {"type": "lu_dense", "dense_limit": 40}, dev(C.tridiag(40) @ np.ones(40)), 40)
    assert np.abs(x.cpu().numpy() - 1.0).max() < 1e-14                # (the limit itself is allowed)
    refused(sp.csr_matrix(np.ones((5, 6))), {"type": "lu_dense"}, "needs a square matrix", L.MfmgInvalidArgument)
    refused(C.tridiag(8), {"type": "pcg", "n_iterations": -1}, "non-negative")


@pytest.mark.parametrize("n", C.PCG_SIZES)
def test_pcg_against_long_double(ctx, n):
    kind = "scaled_tridiagonal"
    Ad = M.SparseMatrixDevice(ctx, C.pcg_matrix(kind, n))
    b = dev(C.pcg_system(kind, n)[3])
    zero = torch.zeros(n, dtype=torch.float64, device="cuda")
    worst = 0.0
    for n_it in C.PCG_ITERATIONS:
        c = C.pcg_case(kind, n, n_it)
        x = solve(ctx, Ad, {"type": "pcg", "n_iterations": n_it}, b, n)
        got = bits(x).view(np.float64)
        if n_it == 0:
            assert (got == 0).all()                                   # zeros over the payload
        worst = max(worst, C.assert_pcg(got, c))
        if n_it in (1, 5):                                            # b = 0: exact zeros, the guards keep 0 / 0 out
            assert (bits(solve(ctx, Ad, {"type": "pcg", "n_iterations": n_it}, zero, n)).view(np.float64) == 0).all()
    assert np.array_equal(bits(b), C.pcg_system(kind, n)[3].view(np.int64))
    print(f"\n[coarse] pcg {kind} n {n}: worst fraction of the bound over {C.PCG_ITERATIONS} iterations {worst:.3g}")


@pytest.mark.parametrize("n", C.PCG_SIZES)
def test_pcg_converged_early(ctx, n):
    """a diagonal of powers of two: exact after the first step; then r = 0, p = 0, p^T A p = 0 and rz = 0"""
    kind = "diagonal"
    _, d, _, b = C.pcg_system(kind, n)
    Ad = M.SparseMatrixDevice(ctx, C.pcg_matrix(kind, n))
    for n_it in C.PCG_ITERATIONS:
        got = bits(solve(ctx, Ad, {"type": "pcg", "n_iterations": n_it}, dev(b), n)).view(np.float64)
        assert np.array_equal(got, b / d if n_it else np.zeros(n)), n_it
        assert C.assert_pcg(got, C.pcg_case(kind, n, n_it)) == 0.0
