"""The batched Lanczos eigensolver of the restrictor setup ("restrictor.eigensolver" lanczos, amge_lanczos.hip) against the dense
host path: mfmg_amd.api.host_build_restrictor with eigensolver.selection krylov on the CPU copy of the problem.  The dense
eigenvalues for the gaps come from the oracle (tests/amge_lanczos_rule.py: agglomerate_local, cell_matrices, scipy's eigh).

The checker is built once per (case, variant) with 4 eigenvectors: the krylov selection takes the eigenvalue groups in ascending
order until it has n_eig, so the rows of n_eig 1 and 2 are the first rows of every agglomerate of that R."""
import numpy as np
import pytest
import scipy.linalg as sla
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
import mfmg_oracle as O
import amge_lanczos_rule as RL

pytestmark = pytest.mark.gpu
HIST_TOL, HIST_ATOL = 1e-10, 1e-12
EVALUATOR = {"mf": "HipMatrixFreeMeshEvaluator", "device": "HipMeshEvaluator", "host": "HipMeshEvaluator"}
N_EIG = (1, 2, 4)
TOLERANCES = (1e-12, 1e-14)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def params_of(case, n_eig, variant, solver="lanczos", **eigensolver):
    es = {"number of eigenvectors": n_eig, "selection": "krylov"}
    if variant == "host":
        es["variant"] = "host"
    es.update(eigensolver)
    return {"eigensolver": es, "agglomeration": dict(zip(("nx", "ny", "nz"), case[1])), "restrictor": {"eigensolver": solver},
            "is preconditioner": False, "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}}


def build(ctx, case, n_eig, variant, solver="lanczos", **eigensolver):
    prob = M.LaplaceProblem(case[0], case[2], device="cuda")
    return M.Hierarchy(ctx, EVALUATOR[variant], prob, params_of(case, n_eig, variant, solver, **eigensolver)), prob


_CHECKER = {}


def checker(case, variant):
    """Per (case, variant), computed once and left unchanged: the dense host R with 4 eigenvectors, its first row and row count
    per agglomerate, and per agglomerate the dense eigenvalues / vectors and the start vector of the oracle."""
    key = (case, variant)
    if key not in _CHECKER:
        prob = M.LaplaceProblem(case[0], case[2])
        R4 = M.host_build_restrictor(prob, params_of(case, 4, variant, "host"), variant == "mf").tocsr()
        R4.sort_indices()
        dense = []
        for p in RL.agglomerate_problems(case[0], case[1], case[2], variant):
            w, V = sla.eigh(p["M"])
            vals, vecs = O._select_eigenvectors(w, V, min(4, len(w)), "krylov", p["v0"])
            dense.append({"w": w, "V": V, "v0": p["v0"], "vals": vals, "n_vec": vecs.shape[1], "gl": p["gl"],
                          "shift": p["shift"], "na": len(p["v0"])})
        n_vec = np.array([d["n_vec"] for d in dense])
        first = np.concatenate([[0], np.cumsum(n_vec)])
        assert first[-1] == R4.shape[0]
        _CHECKER[key] = {"R4": R4, "dense": dense, "first": first, "n_vec": n_vec}
    return _CHECKER[key]


def checker_rows(ck, n_eig):
    """(R of the checker for n_eig vectors, agglomerate of every row)."""
    rows, agg = [], []
    for a, nv in enumerate(ck["n_vec"]):
        k = min(n_eig, nv)
        rows.extend(range(ck["first"][a], ck["first"][a] + k))
        agg.extend([a] * k)
    return ck["R4"][rows].tocsr(), np.array(agg)


def assert_r_within_bound(R, ck, n_eig, tolerance, what):
    """Check 1: pattern and rows per agglomerate of the checker, every entry within (sqrt 2 tolerance + 64 eps) / g."""
    Rc, agg = checker_rows(ck, n_eig)
    R = R.tocsr()
    R.sort_indices()
    assert R.shape == Rc.shape, (what, R.shape, Rc.shape)
    assert np.array_equal(R.indptr, Rc.indptr) and np.array_equal(R.indices, Rc.indices), what
    g = np.array([RL.selection_gap(d["w"], d["V"], d["v0"], n_eig) for d in ck["dense"]])
    bound_of_row = RL.entry_bound(tolerance, g)[agg]
    err = np.abs(R.data - Rc.data)
    row_of_entry = np.repeat(np.arange(R.shape[0]), np.diff(R.indptr))
    ratio = err / bound_of_row[row_of_entry]
    print(f"{what}: largest |R - R_dense| / bound = {ratio.max():.3g} (largest error {err.max():.3g}, smallest gap {g.min():.3g})")
    assert np.isfinite(R.data).all(), what
    assert (ratio <= 1.0).all(), f"{what}: {int((ratio > 1).sum())} entries beyond the bound, worst {ratio.max():.3g}"


ALL_CASES = [(c, v) for c in RL.CASES for v in ("mf", "device")]


@pytest.mark.parametrize("case,variant", ALL_CASES, ids=[RL.case_id(c) + "-" + v for c, v in ALL_CASES])
def test_restrictor_entry_by_entry_and_bookkeeping(ctx, case, variant):
    """Checks 1 and 3: R of a hierarchy built with the Lanczos solver against the dense host R entry by entry, for 1, 2 and 4
    eigenvectors at tolerances 1e-12 and 1e-14; no agglomerate unconverged, iterations within min(active DoFs, 200), breakdowns
    counted on the (8, 8, 4) case with 4 eigenvectors (the run for them exhausts the Krylov space of the start vector)."""
    ck = checker(case, variant)
    max_active = max(d["na"] for d in ck["dense"])
    for n_eig in N_EIG:
        for tol in TOLERANCES:
            h, _ = build(ctx, case, n_eig, variant, tolerance=tol)
            info = h.restrictor_eigensolver_info()
            what = f"{RL.case_id(case)} {variant} n_eig {n_eig} tolerance {tol:g}"
            print(what, info)
            assert info["solver"] == "lanczos" and info["agglomerates"] == len(ck["dense"])
            assert info["nodes"] == int(np.prod([min(a, n) + 1 for a, n in zip(case[1], case[0])]))
            assert info["unconverged"] == 0, what
            assert 1 <= info["max_iterations"] <= min(max_active, 200), what
            assert 1 <= info["solves"] <= info["agglomerates"]
            if case[0] == (8, 8, 4) and n_eig == 4:      # (one or two vectors converge before the Krylov space is exhausted)
                assert info["breakdowns"] > 0, what
            assert_r_within_bound(h.restrictor().to_scipy(), ck, n_eig, tol, what)


def test_host_variant(ctx):
    case = ((8, 8, 8), (4, 4, 4), "linear")
    ck = checker(case, "host")
    for tol in TOLERANCES:
        h, _ = build(ctx, case, 2, "host", tolerance=tol)
        assert h.restrictor_eigensolver_info()["unconverged"] == 0
        assert_r_within_bound(h.restrictor().to_scipy(), ck, 2, tol, f"host variant, tolerance {tol:g}")


@pytest.mark.parametrize("case,variant", ALL_CASES + [(((8, 8, 8), (4, 4, 4), "linear"), "host")],
                         ids=[RL.case_id(c) + "-" + v for c, v in ALL_CASES] + ["host"])
def test_eigenvalues_and_flags_of_amge_eigen(ctx, case, variant):
    """Check 2: the eigenvalues of amge_eigen within (tolerance + 64 eps) scale of the dense ones; its n_vec, iterations and flags."""
    ck = checker(case, variant)
    prob = M.LaplaceProblem(case[0], case[2], device="cuda")
    for tol in TOLERANCES:
        out = M.amge_eigen(ctx, prob, params_of(case, 4, variant, tolerance=tol), variant == "mf")
        assert out["weights"].shape[0] == len(ck["dense"]) and out["weights"].shape[1] == 4
        assert out["converged"].all()
        worst = 0.0
        for a, d in enumerate(ck["dense"]):
            assert out["n_vec"][a] == d["n_vec"]
            assert 1 <= out["iterations"][a] <= min(d["na"], 200)
            scale = abs(d["w"][-1])
            err = np.abs(out["eigenvalues"][a, :d["n_vec"]] - (d["vals"] - d["shift"]))
            worst = max(worst, (err / ((tol + 64 * RL.EPS) * scale)).max())
        print(f"{RL.case_id(case)} {variant} tolerance {tol:g}: largest eigenvalue error / bound = {worst:.3g}")
        assert worst <= 1.0
        if case[0] == (8, 8, 4):
            assert out["breakdown"].all()


def test_amge_eigen_with_the_dense_device_solver(ctx):
    """The same entry point with restrictor.eigensolver device: the dense kernel's selection, no iterations."""
    case = ((6, 6, 6), (3, 3, 3), "linear")
    ck = checker(case, "mf")
    prob = M.LaplaceProblem(case[0], case[2], device="cuda")
    out = M.amge_eigen(ctx, prob, params_of(case, 4, "mf", "device"), True)
    assert out["weights"].shape == (8, 4, 64) and (out["iterations"] == 0).all() and out["converged"].all()
    for a, d in enumerate(ck["dense"]):
        assert out["n_vec"][a] == d["n_vec"]
        np.testing.assert_allclose(out["eigenvalues"][a, :d["n_vec"]], d["vals"], rtol=0, atol=1e-12 * abs(d["w"][-1]))


def test_identical_agglomerates_share_solves(ctx):
    """Check 3, constant coefficient with at least 64 agglomerates: fewer solves than agglomerates."""
    case = ((16, 16, 16), (4, 4, 4), "constant")
    for variant in ("mf", "device"):
        h, _ = build(ctx, case, 2, variant, tolerance=1e-12)
        info = h.restrictor_eigensolver_info()
        print(info)
        assert info["agglomerates"] == 64 and info["solves"] < info["agglomerates"] and info["unconverged"] == 0
        assert_r_within_bound(h.restrictor().to_scipy(), checker(case, variant), 2, 1e-12, f"shared solves {variant}")


@pytest.mark.parametrize("case", [((16, 16, 16), (4, 4, 4), "constant"), ((10, 9, 7), (4, 4, 4), "linear")], ids=RL.case_id)
def test_determinism(ctx, case, monkeypatch):
    """Check 4: two builds give R bit for bit, and MFMG_AMGE_MEMO=0 (every agglomerate solved by its own workgroup) gives the bits
    of the shared solves."""
    def r_of():
        h, _ = build(ctx, case, 4, "mf", tolerance=1e-12)
        R = h.restrictor().to_scipy().tocsr()
        R.sort_indices()
        return R, h.restrictor_eigensolver_info()
    R1, i1 = r_of()
    R2, _ = r_of()
    monkeypatch.setenv("MFMG_AMGE_MEMO", "0")
    R3, i3 = r_of()
    assert i3["solves"] == i3["agglomerates"]
    if case[2] == "constant":
        assert i1["solves"] < i1["agglomerates"]
    for other in (R2, R3):
        assert np.array_equal(R1.indptr, other.indptr) and np.array_equal(R1.indices, other.indices)
        assert np.array_equal(R1.data.view(np.int64), other.data.view(np.int64))


def test_max_iterations_10(ctx):
    """Check 5: the build succeeds, agglomerates are counted as unconverged, R is finite with the checker's pattern."""
    case = ((8, 8, 8), (4, 4, 4), "linear")
    h, _ = build(ctx, case, 4, "mf", tolerance=1e-12, max_iterations=10)
    info = h.restrictor_eigensolver_info()
    assert info["unconverged"] > 0 and info["max_iterations"] == 10
    R = h.restrictor().to_scipy().tocsr()
    R.sort_indices()
    Rc, _ = checker_rows(checker(case, "mf"), 4)
    assert np.isfinite(R.data).all()
    assert R.shape == Rc.shape and np.array_equal(R.indptr, Rc.indptr) and np.array_equal(R.indices, Rc.indices)


def gpu_history(ctx, h, apply_monitor, b, x0, n_cycles=20):
    x, bd = dev(x0), dev(b)
    r = torch.empty_like(x)
    apply_monitor(r, x)
    ctx.sadd(r, -1.0, 1.0, bd)
    r0 = ctx.l2_norm(r)
    res = [1.0]
    for _ in range(n_cycles):
        h.apply(bd, x)
        apply_monitor(r, x)
        ctx.sadd(r, -1.0, 1.0, bd)
        res.append(ctx.l2_norm(r) / r0)
    ctx.synchronize()
    return np.array(res)


@pytest.mark.parametrize("variant", ["mf", "device"])
def test_cycle_history_against_the_oracle(ctx, variant):
    """Check 6: (16, 16, 16) cells, (4, 4, 4) agglomerates, linear, 4 eigenvectors, Chebyshev(3): the 20-cycle residual history
    equals the oracle's TwoLevelHierarchy run on the downloaded R to 1e-10, and the cycle converges."""
    case = ((16, 16, 16), (4, 4, 4), "linear")
    mesh = O.StructuredMesh(case[0])
    coef = O.coefficient_table(mesh, case[2])
    con = mesh.constrained_mask()
    h, prob = build(ctx, case, 4, variant)
    assert h.restrictor_eigensolver_info()["solver"] == "lanczos"
    deg, lmin, lmax = h.smoother_info()
    R = h.restrictor().to_scipy()
    if variant == "mf":
        mf = O.MatrixFreeLaplace(mesh, coef)
        apply_A, dinv = mf.vmult, mf.diagonal_inverse()
        op = M.MatrixFreeLaplace(ctx, prob)
        monitor = lambda y, x: op.vmult(y, x)
    else:
        A = O.assemble_csr(mesh, coef)
        apply_A, dinv = (lambda v: A @ v), 1.0 / A.diagonal()
        Ad = M.SparseMatrixDevice(ctx, A)
        monitor = lambda y, x: Ad.vmult(y, x)
    Ac = O.galerkin_coarse_matrix(apply_A, R)
    p = O.ChebyshevParams(degree=deg, lambda_max=lmax, lambda_min=lmin)
    smoother = lambda b, x: O.chebyshev_smoother_apply(apply_A, dinv, p, b, x)
    ho = O.TwoLevelHierarchy(apply_A, smoother, R, O.direct_coarse_solver(Ac), 1, False)
    x0 = O.random_initial_guess(mesh.n_dofs, con)
    b = np.zeros(mesh.n_dofs)
    res_o, _, _ = O.vcycle_history(ho, apply_A, b, x0)
    res_g = gpu_history(ctx, h, monitor, b, x0)
    np.testing.assert_allclose(res_g, res_o, rtol=HIST_TOL, atol=HIST_ATOL)
    assert res_g[-1] / res_g[-2] < 1.0


def test_refusals(ctx):
    """Check 7."""
    case = ((8, 8, 8), (4, 4, 4), "linear")
    with pytest.raises(L.MfmgError, match="lapack") as e:
        build(ctx, case, 2, "mf", selection="lapack")
    assert not isinstance(e.value, (L.MfmgNotImplementedError,))
    with pytest.raises(L.MfmgNotImplementedError, match="729"):
        build(ctx, ((9, 9, 9), (9, 9, 9), "linear"), 2, "mf")
    with pytest.raises(L.MfmgError, match="device, host or lanczos"):
        build(ctx, case, 2, "mf", solver="arpack")
    prob = M.LaplaceProblem((9, 9, 9), "linear", device="cuda")
    with pytest.raises(L.MfmgNotImplementedError, match="729"):
        M.amge_eigen(ctx, prob, params_of(((9, 9, 9), (9, 9, 9), "linear"), 2, "mf"), True)


SMALL = [(c, v) for c in RL.CASES_SMALL + [((8, 8), (4, 4), "linear")] for v in ("mf", "device")]


@pytest.mark.parametrize("case,variant", SMALL, ids=[RL.case_id(c) + "-" + v for c, v in SMALL])
def test_small_sizes_against_the_dense_device_kernel(ctx, case, variant):
    """Check 8: on agglomerates of at most 64 nodes the Lanczos R agrees with the R of restrictor.eigensolver device within the
    bound of check 1."""
    ck = checker(case, variant)
    for n_eig in N_EIG:
        hd, _ = build(ctx, case, n_eig, variant, solver="device")
        assert hd.restrictor_eigensolver_info()["solver"] == "device dense"
        Rd = hd.restrictor().to_scipy().tocsr()
        Rd.sort_indices()
        for tol in TOLERANCES:
            h, _ = build(ctx, case, n_eig, variant, tolerance=tol)
            R = h.restrictor().to_scipy().tocsr()
            R.sort_indices()
            assert R.shape == Rd.shape and np.array_equal(R.indptr, Rd.indptr) and np.array_equal(R.indices, Rd.indices)
            _, agg = checker_rows(ck, n_eig)
            g = np.array([RL.selection_gap(d["w"], d["V"], d["v0"], n_eig) for d in ck["dense"]])
            bound = RL.entry_bound(tol, g)[agg][np.repeat(np.arange(R.shape[0]), np.diff(R.indptr))]
            assert (np.abs(R.data - Rd.data) <= bound).all()


def test_host_dense_path_reports_itself(ctx):
    """restrictor.eigensolver device on agglomerates beyond 64 nodes still takes the host cores, silently, and says so here."""
    case = ((8, 8, 4), (4, 4, 2), "constant")
    h, _ = build(ctx, case, 2, "mf", solver="device")
    info = h.restrictor_eigensolver_info()
    assert info["solver"] == "host dense" and info["nodes"] == 75 and info["max_iterations"] == 0
