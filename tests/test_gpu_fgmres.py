"""Flexible GMRES (Hierarchy.solve_fgmres) and the fused orthogonalisation kernels under it (krylov_basis.hip).

Kernel bounds, u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3), references in
long double (64-bit significand: its own error is 2^-11 of the bounds below):
  dots     every product enters its sum through one fma, n terms in some fixed order: |h_i - V_i.w| <= gamma_n sum|V_i||w|, whatever
           the order; asserted with gamma_{n+2}
  update   w - sum h_i V_i, one fma per term: j + 1 roundings per entry in a pass.  One pass is launched for this bound, so that
           the h returned is the h applied (after two passes on a general V the applied h_1, h_2 can cancel in their sum, and a
           bound in terms of the sum does not hold); asserted with gamma_{j+3} (|w| + sum|h_i||V_i|) against the long-double
           result formed from the h the kernel returned -- inside the gamma_{2j+6} that covers two passes
  norm     sum of n squares by fma, then a correctly rounded square root: gamma_{n+1} / 2 + u relative; asserted with gamma_{n+2}
  combine  as update with one pass: gamma_{j+3}
  CGS2     on an orthonormal V, "twice is enough" (Giraud, Langou, Rozloznik, van den Eshof 2005): the result is orthogonal to V to
           a small multiple of u; asserted as max|V_i.w| / ||w|| <= 64 u sqrt(n), for n > columns (for n <= columns no w has a part
           outside the span of an orthonormal V)
  summed h after two passes on that V.  With h1 = Q w + e1, w1 = w - Q^T h1 + d1, h2 = Q w1 + e2 and E = Q Q^T - I:
           h1 + h2 = Q w - E h1 + Q d1 + e2 (e1 cancels), then one rounding of the sum.  |e2_i| <= gamma_{n+2} sum|Q_i||w1|,
           |d1| <= gamma_{j+3} (|w| + |Q^T||h1|), so |h_i - (Q w)_i| <= (|E||h1|)_i + |Q_i|.|d1| + gamma_{n+2} |Q_i|.|w1| + u |h_i|,
           every term formed in long double from Q and w (h1, w1 by their exact values, their own errors enter at second order:
           the bound is taken times 1 + 1e-3 for them)
Padding entries of the columns (n odd: ld = n + 1) hold NaN: a kernel that reads one fails every bound.

Driver: compared with a numpy restatement written here (CGS2, Givens rotations, the same stopping rule) that takes A from
Hierarchy.operator_apply and M^-1 from Hierarchy.vmult; tolerances for histories are those of test_outer_cg_driver_matches_oracle
(rtol 1e-7, atol 1e-3 tol), 1e-10 where the same library runs the same problem in two numberings (tests/test_gpu_numbering.py)."""
import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble
SIZES = [1, 2, 63, 64, 65, 4097, 131073]
COLUMNS = [1, 2, 8, 9, 31]


def gamma(k):
    return k * U / (1.0 - k * U)


def dev(a, dtype=np.float64):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()    # (a copy: the shared inputs are read-only)


def signed_decades(rng, shape):
    """signed values whose magnitudes span six decades"""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)


def padded(columns, n):
    """[columns, ld] with ld = n rounded up to even, the padding NaN"""
    ld = (n + 1) // 2 * 2
    out = np.full((columns.shape[0], ld), np.nan)
    out[:, :n] = columns
    return out


_inputs = {}


def kernel_inputs(n, k):
    """V [k, n], w [n] and their long-double copies: computed once, shared and left unchanged"""
    if (n, k) not in _inputs:
        rng = np.random.default_rng(1000 * k + n)
        V, w = signed_decades(rng, (k, n)), signed_decades(rng, n)
        V.setflags(write=False)
        w.setflags(write=False)
        _inputs[(n, k)] = (V, w, V.astype(LD), w.astype(LD))
    return _inputs[(n, k)]


def orthogonalize(ctx, Vp, w, k, passes):
    wd = dev(w)
    h, norm = ctx.krylov_orthogonalize(dev(Vp), wd, k, passes)
    ctx.synchronize()
    return h.cpu().numpy(), wd.cpu().numpy(), float(norm.cpu()[0])


# ---- 1. kernels against long double ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", COLUMNS)
@pytest.mark.parametrize("n", SIZES)
def test_dots_update_and_norm_against_long_double(ctx, n, k):
    V, w, Vl, wl = kernel_inputs(n, k)
    h, w_out, norm = orthogonalize(ctx, padded(V, n), w, k, passes=1)
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(w_out)) and np.isfinite(norm)
    h_ref = (Vl * wl).sum(axis=1)
    h_bound = gamma(n + 2) * (np.abs(Vl) * np.abs(wl)).sum(axis=1)
    assert np.all(np.abs(h.astype(LD) - h_ref) <= h_bound), (np.abs(h - h_ref) / h_bound).max()
    hl = h.astype(LD)
    w_ref = wl - (hl[:, None] * Vl).sum(axis=0)
    w_bound = gamma((k - 1) + 3) * (np.abs(wl) + (np.abs(hl)[:, None] * np.abs(Vl)).sum(axis=0))
    assert np.all(np.abs(w_out.astype(LD) - w_ref) <= w_bound), (np.abs(w_out - w_ref) / w_bound).max()
    norm_ref = np.sqrt((w_out.astype(LD) ** 2).sum())
    assert abs(LD(norm) - norm_ref) <= gamma(n + 2) * norm_ref
    # a repeated launch gives the same bits
    h2, w2, norm2 = orthogonalize(ctx, padded(V, n), w, k, passes=1)
    assert h.tobytes() == h2.tobytes() and w_out.tobytes() == w2.tobytes() and norm == norm2


@pytest.mark.parametrize("n,k", [(n, k) for n in SIZES for k in COLUMNS if n > k])
def test_two_passes_leave_w_orthogonal_to_an_orthonormal_basis(ctx, n, k):
    rng = np.random.default_rng(7 * n + k)
    Q = np.linalg.qr(rng.standard_normal((n, k)))[0].T.copy()
    w = signed_decades(rng, n)
    h, w_out, norm = orthogonalize(ctx, padded(Q, n), w, k, passes=2)
    wl = w_out.astype(LD)
    norm_ref = np.sqrt((wl ** 2).sum())
    assert norm_ref > 0 and abs(LD(norm) - norm_ref) <= gamma(n + 2) * norm_ref
    ratio = float(np.abs((Q.astype(LD) * wl).sum(axis=1)).max() / norm_ref)
    assert ratio <= 64 * U * np.sqrt(n), ratio
    # the summed coefficients of the two passes (bound: head of this file)
    Ql, w0 = Q.astype(LD), w.astype(LD)
    h1 = Ql @ w0
    w1 = w0 - h1 @ Ql
    d1 = gamma((k - 1) + 3) * (np.abs(w0) + np.abs(h1) @ np.abs(Ql))
    E = Ql @ Ql.T - np.eye(k, dtype=LD)
    h_bound = (1 + 1e-3) * (np.abs(E) @ np.abs(h1) + np.abs(Ql) @ d1 + gamma(n + 2) * (np.abs(Ql) @ (np.abs(w1) + d1)) + U * np.abs(h1))
    assert np.all(np.abs(h.astype(LD) - h1) <= h_bound), float((np.abs(h.astype(LD) - h1) / h_bound).max())
    h2, w2, norm2 = orthogonalize(ctx, padded(Q, n), w, k, passes=2)
    assert h.tobytes() == h2.tobytes() and w_out.tobytes() == w2.tobytes() and norm == norm2


@pytest.mark.parametrize("k", COLUMNS)
@pytest.mark.parametrize("n", SIZES)
def test_combine_against_long_double(ctx, n, k):
    Z, x, Zl, xl = kernel_inputs(n, k)
    y = signed_decades(np.random.default_rng(3 * n + k), k)
    out = []
    for _ in range(2):
        xd = dev(x)
        ctx.krylov_combine(dev(padded(Z, n)), dev(y), xd)
        ctx.synchronize()
        out.append(xd.cpu().numpy())
    yl = y.astype(LD)
    ref = xl + (yl[:, None] * Zl).sum(axis=0)
    bound = gamma((k - 1) + 3) * (np.abs(xl) + (np.abs(yl)[:, None] * np.abs(Zl)).sum(axis=0))
    assert np.all(np.abs(out[0].astype(LD) - ref) <= bound)
    assert out[0].tobytes() == out[1].tobytes()


@pytest.mark.parametrize("n,k", [(65, 9), (4097, 31)])
def test_unaligned_columns_take_the_scalar_loads(ctx, n, k):
    """ld = n odd: every second column is 8 bytes off the 16-byte grid, and so is a w that starts at an odd entry"""
    V, w, Vl, wl = kernel_inputs(n, k)
    wd = torch.empty(n + 1, dtype=torch.float64, device="cuda")[1:]
    assert wd.data_ptr() % 16 == 8
    wd.copy_(dev(w))
    h, norm = ctx.krylov_orthogonalize(dev(V), wd, k, 1)
    ctx.synchronize()
    h, w_out = h.cpu().numpy(), wd.cpu().numpy()
    h_ref = (Vl * wl).sum(axis=1)
    assert np.all(np.abs(h.astype(LD) - h_ref) <= gamma(n + 2) * (np.abs(Vl) * np.abs(wl)).sum(axis=1))
    hl = h.astype(LD)
    w_ref = wl - (hl[:, None] * Vl).sum(axis=0)
    assert np.all(np.abs(w_out.astype(LD) - w_ref) <= gamma((k - 1) + 3) * (np.abs(wl) + (np.abs(hl)[:, None] * np.abs(Vl)).sum(axis=0)))
    norm_ref = np.sqrt((w_out.astype(LD) ** 2).sum())
    assert abs(LD(float(norm.cpu()[0])) - norm_ref) <= gamma(n + 2) * norm_ref
    xd = torch.empty(n + 1, dtype=torch.float64, device="cuda")[1:]
    xd.copy_(dev(w))
    y = signed_decades(np.random.default_rng(n), k)
    ctx.krylov_combine(dev(V), dev(y), xd)
    ctx.synchronize()
    yl = y.astype(LD)
    ref = wl + (yl[:, None] * Vl).sum(axis=0)
    assert np.all(np.abs(xd.cpu().numpy().astype(LD) - ref) <= gamma((k - 1) + 3) * (np.abs(wl) + (np.abs(yl)[:, None] * np.abs(Vl)).sum(axis=0)))


# ---- 2. - 7. the driver -------------------------------------------------------------------------------------------------------------
CHEB2 = {"type": "Chebyshev", "degree": 2, "smoothing_range": 20.0}
CHEB3 = {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}
V01 = {"type": "amg", "amg": {"coarsest_size": 300, "pre_smoothing_levels": 0}}   # the non-symmetric coarse cycle


def base_params(smoother, **extra):
    p = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2},
         "is preconditioner": True, "max levels": 2, "smoother": dict(smoother)}
    p.update(extra)
    return p


def problem_data(prob, seed=5):
    rng = np.random.default_rng(seed)
    free = prob.constrained.cpu().numpy() != 1
    return rng.random(prob.n_dofs) * free, rng.random(prob.n_dofs) * free


def operators(ctx, h):
    """A and M^-1 of the restatement: existing entry points of the library on numpy vectors"""
    def A(v):
        y = torch.empty(v.size, dtype=torch.float64, device="cuda")
        h.operator_apply(0, dev(v), y)
        ctx.synchronize()
        return y.cpu().numpy()

    def Minv(v):
        z = torch.zeros(v.size, dtype=torch.float64, device="cuda")
        h.vmult(z, dev(v))
        ctx.synchronize()
        return z.cpu().numpy()
    return A, Minv


def fgmres_restatement(A, Minv, b, x0, tol, max_iterations, restart):
    """Right-preconditioned flexible GMRES(restart): CGS2, Givens rotations, |g_{j+1}| against the absolute tolerance."""
    x = x0.copy()
    r = b - A(x)
    res = np.linalg.norm(r)
    hist, it = [res], 0
    converged = res <= tol
    while not converged and it < max_iterations:
        m = restart
        V, Z = [r / res], []
        R, cs, sn, g = np.zeros((m + 1, m)), np.zeros(m), np.zeros(m), np.zeros(m + 1)
        g[0] = res
        k = 0
        while k < m and it < max_iterations and not converged:
            Z.append(Minv(V[k]))
            w = A(Z[k])
            Vm, hcol = np.array(V), np.zeros(k + 1)
            for _ in range(2):
                c = Vm @ w
                w = w - c @ Vm
                hcol += c
            hn = np.linalg.norm(w)
            V.append(w / hn)
            col = np.append(hcol, hn)
            for i in range(k):
                col[i], col[i + 1] = cs[i] * col[i] + sn[i] * col[i + 1], -sn[i] * col[i] + cs[i] * col[i + 1]
            d = np.hypot(col[k], col[k + 1])
            cs[k], sn[k] = col[k] / d, col[k + 1] / d
            col[k], col[k + 1] = d, 0.0
            R[: k + 2, k] = col
            g[k + 1], g[k] = -sn[k] * g[k], cs[k] * g[k]
            res = abs(g[k + 1])
            k += 1
            it += 1
            hist.append(res)
            converged = res <= tol
        y = np.linalg.solve(np.triu(R[:k, :k]), g[:k])
        x = x + y @ np.array(Z)
        if not converged and it < max_iterations:
            r = b - A(x)
            res = np.linalg.norm(r)
            converged = res <= tol
    return x, np.array(hist), it


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


CASES = {"chebyshev2_linear": ((12, 10, 8), "linear", dict(smoother=CHEB2)),
         "v01_constant": ((16, 16, 16), "constant", dict(smoother=CHEB3, solver=V01))}
_solved = {}


def solved_case(ctx, case, restart):
    """the case solved by the library and by the restatement: once, shared by the tests below"""
    if (case, restart) not in _solved:
        n, material, extra = CASES[case]
        prob = M.LaplaceProblem(n, material, device="cuda")
        h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(**extra))
        b, _ = problem_data(prob)
        x0 = np.zeros(prob.n_dofs)
        tol = 1e-9 * np.linalg.norm(b)
        A, Minv = operators(ctx, h)
        x_ref, hist_ref, it_ref = fgmres_restatement(A, Minv, b, x0, tol, 100, restart)
        x = dev(x0)
        its, hist = h.solve_fgmres(dev(b), x, tol, 100, restart=restart)
        ctx.synchronize()
        _solved[(case, restart)] = dict(h=h, A=A, b=b, tol=tol, x=x.cpu().numpy(), its=its, hist=hist, x_ref=x_ref, hist_ref=hist_ref,
                                        it_ref=it_ref)
    return _solved[(case, restart)]


@pytest.mark.parametrize("restart", [30, 3], ids=["restart30", "restart3"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_driver_matches_the_restatement(ctx, case, restart):
    s = solved_case(ctx, case, restart)
    assert s["its"] == s["it_ref"] and 3 <= s["its"] <= 40, (s["its"], s["it_ref"])
    np.testing.assert_allclose(s["hist"], s["hist_ref"], rtol=1e-7, atol=1e-3 * s["tol"])
    assert relerr(s["x"], s["x_ref"]) < 1e-9
    assert np.linalg.norm(s["b"] - s["A"](s["x"])) <= 1.01 * s["tol"]
    assert np.all(np.diff(s["hist"]) <= 0.0)
    assert len(s["hist"]) == s["its"] + 1 and s["hist"][-1] <= s["tol"] < s["hist"][-2]


def test_restart_3_runs_several_cycles(ctx):
    s = solved_case(ctx, "chebyshev2_linear", 3)
    assert s["its"] > 6, s["its"]


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    s = solved_case(ctx, "chebyshev2_linear", 30)
    h, b, tol = s["h"], s["b"], s["tol"]
    # b = A x0: no iteration, x untouched
    x0 = np.random.default_rng(2).random(b.size)
    b0 = s["A"](x0)
    x = dev(x0)
    its, hist = h.solve_fgmres(dev(b0), x, 1e-9 * np.linalg.norm(b0), 100)
    ctx.synchronize()
    assert its == 0 and len(hist) == 1 and x.cpu().numpy().tobytes() == x0.tobytes()
    # too few iterations: no convergence, the history filled
    n_it, res = L.C.c_int32(), L.C.c_double()
    hist = np.full(8, -1.0)
    xz = torch.zeros(b.size, dtype=torch.float64, device="cuda")
    status = h._lib.mfmg_hip_hierarchy_solve_fgmres(h.handle, dev(b).data_ptr(), xz.data_ptr(), tol, 2, 30, 0, L.C.byref(n_it), L.C.byref(res),
                                                    hist.ctypes.data_as(L.C.POINTER(L.C.c_double)), len(hist))
    ctx.synchronize()
    assert status == L.ERROR_RUNTIME and n_it.value == 2
    np.testing.assert_allclose(hist[:3], s["hist"][:3], rtol=1e-12)
    assert res.value == hist[2] and np.all(hist[3:] == -1.0)
    # ... and x holds the two-iteration iterate: its true residual is the estimate
    assert abs(np.linalg.norm(b - s["A"](xz.cpu().numpy())) - hist[2]) <= 1e-10 * hist[0]
    with pytest.raises(L.MfmgError, match="did not reach"):
        h.solve_fgmres(dev(b), dev(np.zeros(b.size)), tol, 2)
    with pytest.raises(L.MfmgInvalidArgument, match="restart"):
        h.solve_fgmres(dev(b), dev(np.zeros(b.size)), tol, 100, restart=0)
    with pytest.raises(L.MfmgInvalidArgument, match="fine level precision"):
        h.solve_fgmres(dev(b), dev(np.zeros(b.size)), tol, 100, preconditioner="float")


def test_a_basis_that_cannot_be_allocated_leaves_no_workspace_behind(ctx):
    """restart = max_iterations = 2^30 on 1287 DoFs asks for 2^31 + 1 vectors, 22 TB: the allocation is refused (an error status,
    nothing is launched); the next solve on the same hierarchy allocates afresh and gives the bits of the solve before."""
    n, material, extra = CASES["chebyshev2_linear"]
    prob = M.LaplaceProblem(n, material, device="cuda")
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(**extra))
    b, _ = problem_data(prob)
    tol = 1e-9 * np.linalg.norm(b)
    x_before = dev(np.zeros(prob.n_dofs))
    its_before, hist_before = h.solve_fgmres(dev(b), x_before, tol, 100, restart=5)
    xz = dev(np.zeros(prob.n_dofs))
    status = h._lib.mfmg_hip_hierarchy_solve_fgmres(h.handle, dev(b).data_ptr(), xz.data_ptr(), tol, 2 ** 30, 2 ** 30, 0, None, None, None, 0)
    assert status == L.ERROR_DEVICE
    assert "memory" in h._lib.mfmg_hip_last_error().decode().lower()
    for restart in (5, 30):                                               # the same and a larger basis than before the failure
        x = dev(np.zeros(prob.n_dofs))
        its, hist = h.solve_fgmres(dev(b), x, tol, 100, restart=restart)
        ctx.synchronize()
        if restart == 5:
            assert its == its_before and hist.tobytes() == hist_before.tobytes()
            assert x.cpu().numpy().tobytes() == x_before.cpu().numpy().tobytes()
        assert np.linalg.norm(b - operators(ctx, h)[0](x.cpu().numpy())) <= 1.01 * tol


def test_breakdown_ends_the_cycle_and_the_true_residual_decides(ctx):
    """b = e_c, c a Dirichlet DoF: row and column c of A are those of the identity, so e_c is an eigenvector of A and of the cycle,
    A M^-1 e_c = alpha e_c (asserted first, on operator_apply and vmult).  Then w - (v_0, w) v_0 is exactly zero in the first
    step: h_{1,0} = 0, the Krylov space is exhausted.  The driver must end the cycle with the update and report the recomputed
    residual -- here exactly 0: one iteration, a finite x = e_c (row c of A is the identity's: A x = e_c means x_c = 1)."""
    s = solved_case(ctx, "chebyshev2_linear", 30)
    h, A = s["h"], s["A"]
    _, Minv = operators(ctx, h)
    prob = M.LaplaceProblem(*CASES["chebyshev2_linear"][:2], device="cuda")
    c = int(np.flatnonzero(prob.constrained.cpu().numpy() == 1)[7])
    e = np.zeros(prob.n_dofs)
    e[c] = 1.0
    w = A(Minv(e))
    alpha = w[c]
    assert alpha > 0 and np.count_nonzero(w) == 1
    x = dev(np.zeros(prob.n_dofs))
    its, hist = h.solve_fgmres(dev(e), x, 1e-12, 50)
    ctx.synchronize()
    x = x.cpu().numpy()
    assert its == 1 and hist[0] == 1.0 and hist[1] == np.linalg.norm(e - A(x)) <= 1e-12
    assert np.all(np.isfinite(x)) and np.count_nonzero(x) == 1 and abs(x[c] - 1.0) <= 4 * U


# ---- 5. numbering ---------------------------------------------------------------------------------------------------------------
def test_dealii_numbering_in_lexicographic_mode_equals_the_lexicographic_solve(ctx):
    n = (16, 16, 16)
    perm = M.laplace.dealii_numbering(n)
    p = perm.numpy()
    prob = M.LaplaceProblem(n, "constant", device="cuda", dof_numbering=perm)
    prob_lex = M.LaplaceProblem(n, "constant", device="cuda")
    b, _ = problem_data(prob, seed=11)
    tol = 1e-9 * np.linalg.norm(b)
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, solver=V01, **{"internal numbering": "lexicographic"}))
    assert h.internal_numbering() == (1, 1)
    _, lmin, lmax = h.smoother_info()
    # (the same polynomial in both problems: see the head of tests/test_gpu_numbering.py)
    href = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob_lex, base_params(dict(CHEB3, lambda_min=lmin, lambda_max=lmax), solver=V01))
    assert href.smoother_info() == (3, lmin, lmax)
    try:
        counts = []
        for restart in (30, 3):
            x = dev(np.zeros(prob.n_dofs))
            ctx.profile_enable(True, only="dof_permutation")
            its, hist = h.solve_fgmres(dev(b), x, tol, 100, restart=restart)
            counts.append(ctx.profile_query("dof_permutation")[0])
            ctx.profile_enable(False)
            xr = dev(np.zeros(prob.n_dofs))
            its_ref, hist_ref = href.solve_fgmres(dev(b[p]), xr, tol, 100, restart=restart)
            ctx.synchronize()
            assert its == its_ref and 3 <= its <= 40
            np.testing.assert_allclose(hist, hist_ref, rtol=1e-10, atol=1e-12 * hist_ref[0])
            assert np.abs(x.cpu().numpy()[p] - xr.cpu().numpy()).max() <= 1e-10 * np.abs(xr.cpu().numpy()).max()
        assert counts == [2, 2]                                           # whatever the iteration count and the restarts
    finally:
        ctx.profile_enable(False)
    # the solution solves the caller's system
    op = M.MatrixFreeLaplace(ctx, prob)
    r = torch.empty_like(x)
    op.vmult(r, x)
    ctx.synchronize()
    assert np.linalg.norm(r.cpu().numpy() - b) <= 1.01 * tol


# ---- 6. FP32 preconditioner -----------------------------------------------------------------------------------------------------
def test_fp32_preconditioner_under_the_fp64_iteration(ctx):
    n = (16, 16, 16)
    prob = M.LaplaceProblem(n, "constant", device="cuda")
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, **{"fine level precision": "float"}))
    b, _ = problem_data(prob)
    tol = 1e-10 * np.linalg.norm(b)                                       # beyond float accuracy: the outer iteration is FP64
    A, _ = operators(ctx, h)
    x64 = dev(np.zeros(prob.n_dofs))
    its64, _ = h.solve_fgmres(dev(b), x64, tol, 100, preconditioner="double")
    x32 = dev(np.zeros(prob.n_dofs))
    try:
        its32, hist32 = h.solve_fgmres(dev(b), x32, tol, 2 * its64, preconditioner="float")
    except L.MfmgError as e:
        raise AssertionError(f"FP32-preconditioned FGMRES did not converge within 2 x {its64} iterations (the FP64 count): {e}")
    ctx.synchronize()
    assert 3 <= its32 <= 2 * its64, f"FP32 preconditioner: {its32} iterations, FP64 preconditioner: {its64}"
    assert np.linalg.norm(b - A(x32.cpu().numpy())) <= 1.01 * tol
    assert np.linalg.norm(b - A(x64.cpu().numpy())) <= 1.01 * tol


# ---- 7. consistency with CG -----------------------------------------------------------------------------------------------------
def test_fgmres_and_cg_agree_on_the_symmetric_cycle(ctx):
    """Both to 1e-12 ||b||: each solution is then within cond(A) 1e-12 of the exact one, far inside the 1e-8 asked of their difference."""
    s = solved_case(ctx, "chebyshev2_linear", 30)
    h, b = s["h"], s["b"]
    tol = 1e-12 * np.linalg.norm(b)
    x_cg, x_gm = dev(np.zeros(b.size)), dev(np.zeros(b.size))
    its_cg, _ = h.solve_cg(dev(b), x_cg, tol, 100)
    its_gm, _ = h.solve_fgmres(dev(b), x_gm, tol, 100)
    ctx.synchronize()
    assert relerr(x_gm.cpu().numpy(), x_cg.cpu().numpy()) < 1e-8
    assert 3 <= its_gm <= its_cg + 1, (its_gm, its_cg)
