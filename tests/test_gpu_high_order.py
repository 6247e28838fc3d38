"""The solver for Q2 elements: the Q2 operator preconditioned by a Chebyshev smoother around one cycle of the Q1 hierarchy on the
refined mesh (mfmg_amd.HighOrderSolver).  The composition of the preconditioner against numpy, the eigenvalue estimate of its
smoother against a computed eigenvalue, the CG and FGMRES solves, the refusals, and the bits of an existing solve on the same
context."""
import ctypes as C

import numpy as np
import pytest
import torch

import mfmg_amd as M
import q2_reference as R

pytestmark = pytest.mark.gpu

HIST_TOL = 1e-10          # the library's parity tolerance (tests/test_gpu_hierarchy.py)
MESHES = [(4, 4, 4), (8, 6, 5), (16, 16, 16)]
MATERIALS = ["constant", "linear"]
CONFIGS = [(n, m) for n in MESHES for m in MATERIALS]
# lambda_max of the smoother over the largest eigenvalue of D^-1 A_2: the Lanczos estimate never exceeds the eigenvalue, so the
# ratio cannot exceed the smoother's safety factor 1.2; measured on these meshes 1.138 (4^3), 1.186 .. 1.188 (8 x 6 x 5) and
# 1.170 (16^3) for both materials; the cap is the largest of them plus 5 % for run-to-run spread
ESTIMATE_RATIO_MEASURED = 1.188
ESTIMATE_RATIO_CAP = ESTIMATE_RATIO_MEASURED * 1.05

Q1 = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": True,
      "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}}
V01 = {"type": "amg", "amg": {"coarsest_size": 50, "pre_smoothing_levels": 0}}   # the non-symmetric coarse cycle

_cache = {}


def setup(ctx, n, material):
    key = (n, material)
    if key not in _cache:
        p = M.LaplaceProblemQ2(n, material, device="cuda")
        ref = R.Q2Reference(n, p.h, p.coefficient.cpu().numpy(), p.constrained.cpu().numpy())
        free = p.constrained.cpu().numpy() != 1
        b = np.random.default_rng(11).random(p.n_dofs) * free
        _cache[key] = {"problem": p, "ref": ref, "b": b,
                       "solver": M.HighOrderSolver(ctx, p, dict(Q1, **{"high order": {"smoother": {"degree": 2}}}))}
    return _cache[key]


def A2(ref, v):
    return ref.apply(v)[0].astype(np.float64)


def dev(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


def chebyshev_terms(degree, lmin, lmax):
    """(alpha_k, beta_k) of the library's smoother form: x_{k+1} = x_k + alpha_k (x_k - x_{k-1}) - beta_k D^-1 (A x_k - b)"""
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    terms = [(0.0, 1.0 / theta)]
    rhok, sigma = delta / theta, theta / delta
    for _ in range(degree - 1):
        rhokp = 1.0 / (2.0 * sigma - rhok)
        terms.append((rhokp * rhok, 2.0 * rhokp / delta))
        rhok = rhokp
    return terms


def smooth(ref, dinv, terms, b, x):
    prev = x
    for alpha, beta in terms:
        nxt = x + alpha * (x - prev) - beta * dinv * (A2(ref, x) - b)
        prev, x = x, nxt
    return x


@pytest.mark.parametrize("n,material", CONFIGS)
def test_apply_is_the_four_steps(ctx, n, material):
    s = setup(ctx, n, material)
    solver, ref, b = s["solver"], s["ref"], s["b"]
    degree, lmin, lmax = solver.smoother_info()
    assert degree == 2 and abs(lmax / lmin - 4.0) < 1e-12
    terms = chebyshev_terms(degree, lmin, lmax)
    dinv = (1 / ref.diagonal()[0]).astype(np.float64)
    x = smooth(ref, dinv, terms, b, np.zeros_like(b))
    r = A2(ref, x) - b
    c = torch.zeros(b.size, dtype=torch.float64, device="cuda")
    solver.hierarchy.vmult(c, dev(r))                  # the hierarchy's own cycle on the numpy residual
    ctx.synchronize()
    x = x - c.cpu().numpy()
    x = smooth(ref, dinv, terms, b, x)
    got = torch.full((b.size,), float("nan"), dtype=torch.float64, device="cuda")
    solver.apply(dev(b), got)
    ctx.synchronize()
    err = np.abs(got.cpu().numpy() - x).max() / np.abs(x).max()
    print(f"high-order apply {n} {material}: max difference to the four steps in numpy {err:.2e}")
    assert err <= HIST_TOL


def largest_eigenvalue(ref):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    A = ref.assemble()
    d = A.diagonal()
    s = sp.diags(1 / np.sqrt(d))
    return float(spla.eigsh(s @ A @ s, k=1, which="LA", tol=1e-10, return_eigenvectors=False)[0])


@pytest.mark.parametrize("n,material", CONFIGS)
def test_estimate_against_a_computed_eigenvalue(ctx, n, material):
    s = setup(ctx, n, material)
    _, _, lmax = s["solver"].smoother_info()
    exact = largest_eigenvalue(s["ref"])
    print(f"high-order smoother {n} {material}: lambda_max {lmax:.6f}, largest eigenvalue of D^-1 A_2 {exact:.6f}, ratio {lmax / exact:.4f}")
    if n == (4, 4, 4):
        assert 1.27 < exact < 1.30
    assert lmax >= exact
    assert lmax / exact <= ESTIMATE_RATIO_CAP


@pytest.mark.parametrize("n,material", CONFIGS)
def test_cg_solve(ctx, n, material):
    s = setup(ctx, n, material)
    solver, ref, b = s["solver"], s["ref"], s["b"]
    tol = 1e-8 * np.linalg.norm(b)
    x = torch.zeros(b.size, dtype=torch.float64, device="cuda")
    its, hist = solver.solve_cg(dev(b), x, tolerance=tol, max_iterations=100)     # raises when it does not converge
    ctx.synchronize()
    assert hist[-1] <= tol
    true_res = np.linalg.norm(b - A2(ref, x.cpu().numpy()))
    assert true_res <= 1.01 * tol
    assert np.all(hist[1:] <= 1.01 * hist[:-1]), hist
    plain = M.HighOrderSolver(ctx, s["problem"], dict(Q1, **{"high order": {"smoother": {"degree": 0}}}))
    assert plain.smoother_info()[0] == 0
    x0 = torch.zeros(b.size, dtype=torch.float64, device="cuda")
    its0, _ = plain.solve_cg(dev(b), x0, tolerance=tol, max_iterations=200)
    print(f"high-order CG {n} {material}: {its} iterations with Chebyshev(2), {its0} without smoothing")
    assert its < its0


@pytest.mark.parametrize("n,material", CONFIGS)
def test_fgmres_solve_with_a_nonsymmetric_cycle(ctx, n, material):
    """both solves to 1e-10 ||b||: the solutions then differ by at most cond(A_2) 2e-10 relative, below the 1e-7 asked for"""
    s = setup(ctx, n, material)
    b = s["b"]
    tol = 1e-10 * np.linalg.norm(b)
    x_cg = torch.zeros(b.size, dtype=torch.float64, device="cuda")
    s["solver"].solve_cg(dev(b), x_cg, tolerance=tol, max_iterations=100)
    v01 = M.HighOrderSolver(ctx, s["problem"], dict(Q1, solver=V01, **{"high order": {"smoother": {"degree": 2}}}))
    x = torch.zeros(b.size, dtype=torch.float64, device="cuda")
    its, hist = v01.solve_fgmres(dev(b), x, tolerance=tol, max_iterations=100, restart=30)
    ctx.synchronize()
    assert hist[-1] <= tol
    diff = (x - x_cg).abs().max().item() / x_cg.abs().max().item()
    print(f"high-order FGMRES {n} {material}: {its} iterations, difference to the CG solution {diff:.2e}")
    assert diff <= 1e-7


def test_refusals(ctx):
    lib = M.lib.load()
    s = setup(ctx, (4, 4, 4), "constant")
    # the Q1 hierarchy of another mesh
    other = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", M.LaplaceProblem((6, 8, 8), device="cuda"), Q1)
    h = C.c_void_p()
    status = lib.mfmg_hip_high_order_create(other.handle, s["solver"].operator.handle, b"", C.byref(h))
    assert status == M.lib.ERROR_INVALID_ARGUMENT
    # a context with a communicator
    ranks = M.Context()
    M.lib.check(lib.mfmg_hip_context_set_communicator(ranks.handle, 0, 2, 0, 2))
    with pytest.raises(M.lib.MfmgNotImplementedError, match="communicator"):
        M.HighOrderSolver(ranks, s["problem"], Q1)
    # the block drivers
    n = s["problem"].n_dofs
    ld = n + n % 2
    B = torch.zeros(2 * ld, dtype=torch.float64, device="cuda")
    X = torch.zeros(2 * ld, dtype=torch.float64, device="cuda")
    tol = (C.c_double * 2)(1e-8, 1e-8)
    assert lib.mfmg_hip_high_order_solve_cg_block(s["solver"].handle, 2, ld, B.data_ptr(), X.data_ptr(), tol, 10) == M.lib.ERROR_NOT_IMPLEMENTED
    assert lib.mfmg_hip_high_order_solve_fgmres_block(s["solver"].handle, 2, ld, B.data_ptr(), X.data_ptr(), tol, 10, 5) == M.lib.ERROR_NOT_IMPLEMENTED


def test_existing_solve_keeps_its_bits(ctx):
    p = M.LaplaceProblem((8, 8, 8), "linear", device="cuda")
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", p, Q1)
    free = p.constrained.cpu().numpy() != 1
    b = dev(np.random.default_rng(3).random(p.n_dofs) * free)

    def solve():
        x = torch.zeros(p.n_dofs, dtype=torch.float64, device="cuda")
        its, hist = h.solve_cg(b, x, tolerance=1e-9, max_iterations=100)
        ctx.synchronize()
        return its, hist.copy(), x

    before = solve()
    s = setup(ctx, (4, 4, 4), "linear")
    x2 = torch.zeros(s["b"].size, dtype=torch.float64, device="cuda")
    s["solver"].solve_cg(dev(s["b"]), x2, tolerance=1e-8 * np.linalg.norm(s["b"]), max_iterations=100)
    after = solve()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and torch.equal(before[2], after[2])
