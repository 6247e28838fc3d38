""""internal numbering" lexicographic: a mesh whose DoFs are numbered like deal.II's (cells in Morton order, vertex DoFs at first
touch) or at random runs on the kernels of the lexicographic numbering, and everything visible through the interface stays in the
caller's numbering.

Tolerances are the ones of tests/test_gpu_hierarchy.py: HIST_TOL / HIST_ATOL for residual histories (1e-10 relative), 1e-11 for R,
1e-13 relative (or 1e-12 of the max-norm) for operator and transfer applications, 1e-4 for the FP32 fine level.  Iterates are
compared norm-wise (1e-10 of the max-norm): entries of a converging iterate pass through zero.

The start vector of the Chebyshev eigenvalue estimate is keyed on the DoF id, and in lexicographic mode on the CALLER's id, so that
the estimate is the one of caller mode (asserted to 1e-10).  A lexicographic problem of the same shape hashes other ids and
estimates other bounds (a few per cent apart), hence another polynomial: where a renumbered problem is compared with the
lexicographic PROBLEM, that problem's bounds are pinned (smoother.lambda_min / lambda_max) to the ones the renumbered hierarchy
estimated; the comparison itself -- histories and iterates to HIST_TOL -- is unchanged."""
import os

import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
import mfmg_oracle as O

pytestmark = pytest.mark.gpu
HIST_TOL = 1e-10
HIST_ATOL = 1e-12
N_CYCLES = 8
LEX = "lexicographic"


def dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def make_numbering(kind, n):
    """node -> DoF id (int64 tensor), None for the lexicographic numbering"""
    if kind == LEX:
        return None
    if kind == "dealii":
        return M.laplace.dealii_numbering(n)
    assert kind == "random"
    return torch.from_numpy(np.random.default_rng(7).permutation(int(np.prod([v + 1 for v in n]))))


def base_params(smoother, is_preconditioner=False, mode=None, **extra):
    p = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2},
         "is preconditioner": is_preconditioner, "max levels": 2, "smoother": dict(smoother)}
    if mode is not None:
        p["internal numbering"] = mode
    p.update(extra)
    return p


CHEB3 = {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}
JACOBI = {"type": "Jacobi"}


def history(ctx, h, op, b, x0, is_preconditioner, n_cycles=N_CYCLES):
    """Relative residuals of n_cycles applications: the cycle itself (tests/test_hierarchy.cc:95-123), or -- for a preconditioner,
    which starts from zero -- the defect correction x += M (b - A x)."""
    x, bd = dev(x0), dev(b)
    r, z = torch.empty_like(x), torch.empty_like(x)

    def residual():
        op.vmult(r, x)
        ctx.sadd(r, -1.0, 1.0, bd)
        return ctx.l2_norm(r)
    r0 = residual()
    res = [1.0]
    for _ in range(n_cycles):
        if is_preconditioner:
            h.apply(r, z)
            ctx.sadd(x, 1.0, 1.0, z)
        else:
            h.apply(bd, x)
        res.append(residual() / r0)
    ctx.synchronize()
    return np.array(res), x.cpu().numpy()


def problem_data(prob, seed=11):
    """b and x0 in the numbering of `prob`, zero on its constrained DoFs"""
    rng = np.random.default_rng(seed)
    free = prob.constrained.cpu().numpy() != 1
    return rng.random(prob.n_dofs) * free, rng.random(prob.n_dofs) * free


def assert_same_iterate(x, x_ref):
    assert np.abs(x - x_ref).max() <= HIST_TOL * np.abs(x_ref).max()


def assert_same_vector(y, y_ref):
    np.testing.assert_allclose(y, y_ref, rtol=1e-13, atol=1e-12 * np.abs(y_ref).max())


# ---- 3. the fast paths are reached ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dealii", "random"])
def test_renumbered_mesh_reaches_the_fast_paths(ctx, kind):
    n = (32, 32, 32)
    ref = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", M.LaplaceProblem(n, "constant", device="cuda"), base_params(CHEB3))
    assert max(ref.smoother_sweep_terms()) >= 2                      # the reference problem itself runs a sweep ...
    assert ref.residual_restriction_classes() > 0                    # ... and the one-pass residual restriction
    assert ref.restrictor_form()["structured"]
    prob = M.LaplaceProblem(n, "constant", device="cuda", dof_numbering=make_numbering(kind, n))
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, mode=LEX))
    assert h.internal_numbering() == (1, 1)
    assert h.smoother_sweep_terms() == ref.smoother_sweep_terms()
    assert h.residual_restriction_classes() == ref.residual_restriction_classes()
    assert h.restrictor_form() == ref.restrictor_form()
    # what the caller's numbering costs without the key: no sweep, no one-pass restriction
    hc = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, mode="caller"))
    assert hc.internal_numbering() == (0, 0)
    assert hc.smoother_sweep_terms() == (0, 0) and hc.residual_restriction_classes() == 0


# ---- 4. the same preconditioner ---------------------------------------------------------------------
@pytest.mark.parametrize("is_preconditioner", [False, True])
@pytest.mark.parametrize("smoother", [CHEB3, JACOBI], ids=["chebyshev3", "jacobi"])
@pytest.mark.parametrize("material", ["constant", "linear"])
@pytest.mark.parametrize("kind", ["dealii", "random"])
def test_same_cycle_as_caller_mode_and_as_the_lexicographic_problem(ctx, kind, material, smoother, is_preconditioner):
    n = (16, 16, 16)
    perm = make_numbering(kind, n)
    prob = M.LaplaceProblem(n, material, device="cuda", dof_numbering=perm)
    prob_lex = M.LaplaceProblem(n, material, device="cuda")
    b, x0 = problem_data(prob)
    p = perm.numpy()
    out = {}
    for name, pr, mode in (("lexmode", prob, LEX), ("caller", prob, "caller"), ("lexproblem", prob_lex, None)):
        sm = dict(smoother)
        if name == "lexproblem" and smoother is CHEB3:
            # (the polynomial of the renumbered hierarchy: see the head of this file)
            sm["lambda_min"], sm["lambda_max"] = out["lexmode"][2][1:]
        h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", pr, base_params(sm, is_preconditioner, mode))
        op = M.MatrixFreeLaplace(ctx, pr)
        bb, xx = (b[p], x0[p]) if name == "lexproblem" else (b, x0)      # vector of the lexicographic problem: v_lex[n] = v[dof of n]
        res, x = history(ctx, h, op, bb, xx, is_preconditioner)
        out[name] = (res, x, h.smoother_info())
    assert out["lexmode"][0][-1] < 0.5
    np.testing.assert_allclose(out["lexmode"][0], out["caller"][0], rtol=HIST_TOL, atol=HIST_ATOL)
    np.testing.assert_allclose(out["lexmode"][0], out["lexproblem"][0], rtol=HIST_TOL, atol=HIST_ATOL)
    assert_same_iterate(out["lexmode"][1], out["caller"][1])
    assert_same_iterate(out["lexmode"][1][p], out["lexproblem"][1])
    for other in ("caller", "lexproblem"):
        assert out["lexmode"][2][0] == out[other][2][0]
        assert out["lexmode"][2][1:] == pytest.approx(out[other][2][1:], rel=1e-10)


def test_cycle_against_the_oracle_with_pinned_eigenvalues(ctx):
    """The oracle works in the lexicographic numbering and hashes lexicographic ids for its eigenvalue estimate, so the bounds of
    the polynomial are pinned on both sides; R is the hierarchy's own, downloaded in the caller's numbering."""
    n = (16, 16, 16)
    perm = make_numbering("dealii", n)
    p = perm.numpy()
    lmin, lmax = 0.09, 1.8
    mesh = O.StructuredMesh(n)
    coef = O.coefficient_table(mesh, "linear")
    mf = O.MatrixFreeLaplace(mesh, coef)
    prob = M.LaplaceProblem(n, "linear", device="cuda", dof_numbering=perm)
    smoother = {"type": "Chebyshev", "degree": 3, "lambda_max": lmax, "lambda_min": lmin}
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(smoother, mode=LEX))
    assert h.smoother_info() == (3, lmin, lmax)
    R = h.restrictor().to_scipy().tocsc()[:, p].tocsr()                # column n of the oracle's R: the caller's DoF of node n
    Ro = O.build_restrictor(mesh, coef, mf.diagonal(), n_eig=2, variant="mf", eig_mode="krylov").csr
    assert abs(R - Ro).max() < 1e-11
    Ac = O.galerkin_coarse_matrix(mf.vmult, R)
    cp = O.ChebyshevParams(degree=3, lambda_max=lmax, lambda_min=lmin)
    dinv = mf.diagonal_inverse()
    ho = O.TwoLevelHierarchy(mf.vmult, lambda b, x: O.chebyshev_smoother_apply(mf.vmult, dinv, cp, b, x), R,
                             O.direct_coarse_solver(Ac), 1, False)
    x0_lex = O.random_initial_guess(mesh.n_dofs, mesh.constrained_mask())
    res_o, _, x_o = O.vcycle_history(ho, mf.vmult, np.zeros(mesh.n_dofs), x0_lex, n_cycles=N_CYCLES)
    x0 = np.empty_like(x0_lex)
    x0[p] = x0_lex
    res_g, x_g = history(ctx, h, M.MatrixFreeLaplace(ctx, prob), np.zeros(mesh.n_dofs), x0, False)
    np.testing.assert_allclose(res_g, res_o, rtol=HIST_TOL, atol=HIST_ATOL)
    assert_same_iterate(x_g[p], x_o)


# ---- 5. matrices and level-wise applications in the caller's numbering ------------------------------
@pytest.mark.parametrize("kind", ["dealii", "random"])
def test_restrictor_and_level_operations_in_the_callers_numbering(ctx, kind):
    n = (16, 16, 16)
    prob = M.LaplaceProblem(n, "linear", device="cuda", dof_numbering=make_numbering(kind, n))
    hl = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, mode=LEX, keep_ap=True))
    hc = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, mode="caller", keep_ap=True))
    R = hl.restrictor().to_scipy()
    Rc = hc.restrictor().to_scipy()
    assert R.shape == Rc.shape and abs(R - Rc).max() < 1e-11
    rng = np.random.default_rng(21)
    nf, nc = R.shape[1], R.shape[0]
    xf, bf, xc = rng.random(nf), rng.random(nf), rng.random(nc)

    def both(call, n_out, init=None):
        outs = []
        for h in (hl, hc):
            y = torch.full((n_out,), np.nan, dtype=torch.float64, device="cuda") if init is None else dev(init)
            call(h, y)
            ctx.synchronize()
            outs.append(y.cpu().numpy())
        assert np.isfinite(outs[1]).all()
        assert_same_vector(outs[0], outs[1])
        return outs[0]

    y = both(lambda h, y: h.restrictor_apply(1, dev(xf), y), nc)
    assert_same_vector(y, R @ xf)
    y = both(lambda h, y: h.restrictor_apply(1, dev(xc), y, L.TRANS), nf)
    assert_same_vector(y, R.T @ xc)
    y = both(lambda h, y: h.restrictor_apply(1, dev(xc), y, L.TRANS_SUBTRACT), nf, init=bf)
    assert_same_vector(y, bf - R.T @ xc)
    both(lambda h, y: h.restrict_residual(dev(xf), dev(bf), y), nc)
    both(lambda h, y: h.operator_apply(0, dev(xf), y), nf)
    both(lambda h, y: h.smoother_apply(0, dev(bf), y), nf, init=xf)
    both(lambda h, y: h.ap_apply(1, dev(xc), y), nf)
    # set_restrictor takes the matrix in the caller's numbering and reproduces the cycle
    b, x0 = problem_data(prob)
    op = M.MatrixFreeLaplace(ctx, prob)
    res, x = history(ctx, hl, op, b, x0, False)
    h2 = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, mode=LEX))
    h2.set_restrictor(R)
    assert abs(h2.restrictor().to_scipy() - R).max() == 0.0
    res2, x2 = history(ctx, h2, op, b, x0, False)
    np.testing.assert_allclose(res2, res, rtol=HIST_TOL, atol=HIST_ATOL)
    assert_same_iterate(x2, x)


# ---- 6. the kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["", "brick64", "brick16", "ids"])
@pytest.mark.parametrize("n,kind", [((130, 70, 12), "random"), ((37, 21), "random"), ((16, 16), "dealii"), ((16, 16, 16), "dealii")])
def test_permutation_kernel_against_numpy_indexing(n, kind, variant):
    """Both directions, double and float, every kernel variant (the environment switch is read when the context is created), a
    mesh with tail columns in every direction, 2-D meshes, and vectors that are only 8-byte (4-byte) aligned: exact."""
    saved = os.environ.get("MFMG_DOF_PERMUTATION")
    try:
        if variant:
            os.environ["MFMG_DOF_PERMUTATION"] = variant
        else:
            os.environ.pop("MFMG_DOF_PERMUTATION", None)
        own = M.Context()
    finally:
        if saved is None:
            os.environ.pop("MFMG_DOF_PERMUTATION", None)
        else:
            os.environ["MFMG_DOF_PERMUTATION"] = saved
    perm = make_numbering(kind, n)
    p = perm.numpy()
    prob = M.LaplaceProblem(n, "constant", device="cuda", dof_numbering=perm)
    h = M.Hierarchy(own, "HipMatrixFreeMeshEvaluator", prob,
                    base_params({"type": "Chebyshev", "degree": 2}, mode=LEX, solver={"type": "amg"}))
    assert h.internal_numbering() == (1, 1)
    nd = prob.n_dofs
    rng = np.random.default_rng(3)
    for dtype, tdtype in ((np.float64, torch.float64), (np.float32, torch.float32)):
        v = rng.random(nd).astype(dtype)
        for offset in (0, 1):                                         # 1: the vectors start one element past a 16-byte boundary
            vin = torch.zeros(nd + 4, dtype=tdtype, device="cuda")[offset:offset + nd]
            vin.copy_(torch.from_numpy(v))
            lex = torch.full((nd + 4,), -1.0, dtype=tdtype, device="cuda")[offset:offset + nd]
            back = torch.full((nd + 4,), -1.0, dtype=tdtype, device="cuda")[offset:offset + nd]
            h.permute(vin, lex, to_internal=True)
            h.permute(lex, back, to_internal=False)
            own.synchronize()
            np.testing.assert_array_equal(lex.cpu().numpy(), v[p])     # internal[node] = caller[dof of node]
            np.testing.assert_array_equal(back.cpu().numpy(), v)       # the round trip is the identity
            expect = np.empty_like(v)
            expect[p] = v
            h.permute(vin, back, to_internal=False)                    # and the scatter alone
            own.synchronize()
            np.testing.assert_array_equal(back.cpu().numpy(), expect)
    with pytest.raises(L.MfmgInvalidArgument, match="in place"):
        h.permute(vin, vin)


# ---- 7. launch accounting ---------------------------------------------------------------------------
def test_permutation_launches_per_apply_and_per_solve(ctx):
    n = (16, 16, 16)
    prob = M.LaplaceProblem(n, "constant", device="cuda", dof_numbering=make_numbering("dealii", n))
    b, x0 = problem_data(prob)
    try:
        for is_preconditioner in (False, True):
            h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, is_preconditioner, LEX))
            bd, x = dev(b), dev(x0)
            ctx.profile_enable(True, only="dof_permutation")
            h.apply(bd, x)
            assert ctx.profile_query("dof_permutation")[0] == 2       # one gather (b, or b and x), one scatter
            ctx.profile_enable(True, only="dof_permutation")
            h.vmult(x, bd)
            launches, _, nbytes = ctx.profile_query("dof_permutation")
            assert launches == 2
            assert nbytes == 20.0 * prob.n_dofs * (2 if is_preconditioner else 3)
        iterations = []
        for tol in (1e-3, 1e-10):
            x = dev(np.zeros(prob.n_dofs))
            ctx.profile_enable(True, only="dof_permutation")
            its, _ = h.solve_cg(bd, x, tol * np.linalg.norm(b), 100)
            assert ctx.profile_query("dof_permutation")[0] == 2       # whatever the iteration count
            iterations.append(its)
        assert iterations[1] > iterations[0] >= 1
    finally:
        ctx.profile_enable(False)


@pytest.mark.parametrize("is_preconditioner", [False, True])
def test_lexicographic_numbering_is_never_permuted(ctx, is_preconditioner):
    n = (16, 16, 16)
    prob = M.LaplaceProblem(n, "constant", device="cuda")
    b, x0 = problem_data(prob)
    op = M.MatrixFreeLaplace(ctx, prob)
    out = []
    try:
        for mode in (LEX, "caller"):
            h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, is_preconditioner, mode))
            assert h.internal_numbering() == ((1, 0) if mode == LEX else (0, 0))
            ctx.profile_enable(True, only="dof_permutation")
            out.append(history(ctx, h, op, b, x0, is_preconditioner, n_cycles=3) + (h.smoother_info(),))
            x = dev(np.zeros(prob.n_dofs))
            if is_preconditioner:
                h.solve_cg(dev(b), x, 1e-8 * np.linalg.norm(b), 100)
            assert ctx.profile_query("dof_permutation")[0] == 0
            out[-1] = out[-1] + (x.cpu().numpy(),)
    finally:
        ctx.profile_enable(False)
    np.testing.assert_array_equal(out[0][0], out[1][0])               # bit for bit
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][3], out[1][3])
    assert out[0][2] == out[1][2]


# ---- 8. CG ------------------------------------------------------------------------------------------
def test_cg_on_the_dealii_numbering_equals_the_lexicographic_solve(ctx):
    n = (32, 32, 32)
    perm = make_numbering("dealii", n)
    p = perm.numpy()
    prob = M.LaplaceProblem(n, "constant", device="cuda", dof_numbering=perm)
    prob_lex = M.LaplaceProblem(n, "constant", device="cuda")
    b, _ = problem_data(prob)
    tol = 1e-9 * np.linalg.norm(b)
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, True, LEX))
    assert max(h.smoother_sweep_terms()) >= 2
    x = dev(np.zeros(prob.n_dofs))
    its, hist = h.solve_cg(dev(b), x, tol, 100)
    _, lmin, lmax = h.smoother_info()
    href = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob_lex, base_params(dict(CHEB3, lambda_min=lmin, lambda_max=lmax), True))
    assert href.smoother_info() == (3, lmin, lmax)                    # (the same polynomial: see the head of this file)
    xr = dev(np.zeros(prob.n_dofs))
    its_ref, hist_ref = href.solve_cg(dev(b[p]), xr, tol, 100)
    ctx.synchronize()
    assert its == its_ref and 3 <= its <= 30
    np.testing.assert_allclose(hist, hist_ref, rtol=HIST_TOL, atol=HIST_ATOL * hist_ref[0])
    assert_same_iterate(x.cpu().numpy()[p], xr.cpu().numpy())
    # the solution solves the caller's system
    op = M.MatrixFreeLaplace(ctx, prob)
    r = torch.empty_like(x)
    op.vmult(r, x)
    ctx.synchronize()
    assert np.linalg.norm(r.cpu().numpy() - b) <= 1.0001 * tol
    # a start vector in the caller's numbering is honoured
    x2 = dev(x.cpu().numpy())
    its2, _ = h.solve_cg(dev(b), x2, 2.0 * tol, 100)
    assert its2 == 0


# ---- 9. FP32 fine level -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dealii", "random"])
def test_fp32_fine_level_in_the_internal_numbering(ctx, kind):
    n = (16, 16, 16)
    prob = M.LaplaceProblem(n, "constant", device="cuda", dof_numbering=make_numbering(kind, n))
    params = base_params(CHEB3, mode=LEX)
    params["fine level precision"] = "float"
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, params)
    op = M.MatrixFreeLaplace(ctx, prob)
    _, x0 = problem_data(prob)
    x0 = x0.astype(np.float32).astype(np.float64)
    b = np.zeros(prob.n_dofs)
    res64, _ = history(ctx, h, op, b, x0, False)
    xf = dev(x0, np.float32)
    bf = torch.zeros_like(xf)
    r = torch.empty(prob.n_dofs, dtype=torch.float64, device="cuda")

    def norm():
        op.vmult(r, xf.double())
        return ctx.l2_norm(r)
    r0 = norm()
    res32 = [1.0]
    for _ in range(N_CYCLES):
        h.apply_f32(bf, xf)
        res32.append(norm() / r0)
    np.testing.assert_allclose(res32, res64, rtol=1e-4, atol=2e-6)
    assert res32[-1] < 1e-2


# ---- 10. rejections ---------------------------------------------------------------------------------
def test_rejections(ctx, mfmg_lib):
    n = (8, 8, 8)
    prob = M.LaplaceProblem(n, "constant", device="cuda", dof_numbering=make_numbering("dealii", n))
    with pytest.raises(L.MfmgInvalidArgument, match="internal numbering"):
        M.Hierarchy(ctx, "HipMeshEvaluator", prob, base_params(JACOBI, mode=LEX))
    with pytest.raises(L.MfmgInvalidArgument, match="internal numbering"):
        M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, mode="morton"))
    # a context with a communicator (no transport is needed: the key is refused before anything is exchanged)
    own = M.Context()
    L.check(mfmg_lib.mfmg_hip_context_set_communicator(own.handle, 0, 2, 0, 2))
    with pytest.raises(L.MfmgInvalidArgument, match="internal numbering"):
        M.Hierarchy(own, "HipMatrixFreeMeshEvaluator", prob, base_params(CHEB3, mode=LEX))
    # the caller's mode still takes the assembled evaluator on the renumbered mesh
    M.Hierarchy(ctx, "HipMeshEvaluator", prob, base_params(JACOBI, mode="caller"))
