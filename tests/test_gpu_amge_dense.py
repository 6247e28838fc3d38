"""The dense agglomerate eigensolver of the restrictor setup (mfmg_amd/csrc/amge_device.hip: amge_agglomerate_kernel<27|64>,
amge_key_kernel, amge_spread_kernel) per agglomerate, through mfmg_amd.amge_eigen with restrictor.eigensolver device: the cases and
checks of amge_dense_cases.py (test_amge_dense_case_table.py says which edge each case is there for, that the table is conditioned
and that the checks bite).

Shape cases: every variant x selection x n_eig of the table, every agglomerate: count, zeros, vector (krylov), norm / orthogonality /
residual / completeness (lapack), eigenvalue (of the unshifted problem), and entry by entry against the rows of the CPU path.
Launch cases (krylov, 2 vectors, mf and device): more solves than the grid has wavefronts, so that a wavefront takes a second
agglomerate with its LDS as the first left it -- every member of a class of identical agglomerates has the bits of the class's first,
which passes the checks; the run with the sharing pass has the bits of the run without; the sharing pass at 63 against 64
agglomerates, sharing in patterns and giving up, with the solves that restrictor_eigensolver_info reports.

Worst ratio per check to na eps x magnitude (the bound is K_DENSE = 32 of them), printed when the module's fixture is torn down.
Seen on an MI355X: norm 6.0 (a single active DoF), completeness 3.25, eigenvalue 2.73, orthogonality 2.51, residual 1.47, vector 0.75;
against the CPU path's rows 4e-4 of the 1e-12 max|R| allowed.  This is documentation, not a threshold."""
import numpy as np
import pytest

import amge_dense_cases as D
import mfmg_amd as M

pytestmark = pytest.mark.gpu
EVALUATOR = {"mf": "HipMatrixFreeMeshEvaluator", "device": "HipMeshEvaluator", "host": "HipMeshEvaluator"}
MEMO = "MFMG_AMGE_MEMO"
ARRAYS = ("n_vec", "eigenvalues", "weights")


@pytest.fixture(scope="module")
def worst():
    w = D.Worst()
    yield w
    for name, (ratio, where) in w.items():
        print(f"MI355X, {name}: worst ratio {ratio:.4g} (K_DENSE {D.K_DENSE:g}) at {where}")


def eigen(ctx, case, n_eig, variant, selection):
    prob = M.LaplaceProblem(case[0], case[2], device="cuda")
    out = M.amge_eigen(ctx, prob, D.params_of(case, n_eig, variant, selection), variant == "mf")
    A = D.n_agglomerates(case)
    assert out["weights"].shape == (A, n_eig, D.nmax_of(case)) and out["eigenvalues"].shape == (A, n_eig) and out["n_vec"].shape == (A,)
    assert (out["iterations"] == 0).all() and out["converged"].all() and not out["breakdown"].any()
    return out


def cpu_R(case, variant, selection, n_eig):
    prob = M.LaplaceProblem(case[0], case[2])
    return M.host_build_restrictor(prob, D.params_of(case, n_eig, variant, selection, "host"), variant == "mf")


def same_bits(a, b, what):
    for name in ARRAYS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), f"{what}: {name} differs"
    assert np.array_equal(a["weights"].view(np.int64), b["weights"].view(np.int64)), f"{what}: weights differ in a bit (a sign of zero)"


def check_all(out, probs, agglomerates, selection, n_eig, what, worst, complete=False, rows=None, global_diag=None):
    for a, p in zip(agglomerates, probs):
        w = f"{what} agglomerate {a}"
        D.check_agglomerate(p, selection, n_eig, out["n_vec"][a], out["weights"][a], out["eigenvalues"][a], what=w, worst=worst,
                            complete=complete)
        if rows is not None:
            D.check_against_cpu_rows(p, rows, a, global_diag, n_eig, out["n_vec"][a], out["weights"][a], what=w, worst=worst)


SHAPES = [(c, v) for c in D.SHAPE_CASES for v in D.VARIANTS]


@pytest.mark.parametrize("case,variant", SHAPES, ids=[D.case_id(c) + "-" + v for c, v in SHAPES])
def test_shape_case_per_agglomerate(ctx, worst, case, variant):
    probs = D.problems(case, variant)
    gd = D.global_diagonal(case, variant)
    for selection in D.SELECTIONS:
        rows = D.cpu_rows(cpu_R(case, variant, selection, D.N_EIG_REF), probs, selection, D.N_EIG_REF)
        for n_eig in D.n_eigs_of(case, variant, selection):
            if n_eig == D.N_EIG_ALL:
                rows = D.cpu_rows(cpu_R(case, variant, selection, n_eig), probs, selection, n_eig)
            out = eigen(ctx, case, n_eig, variant, selection)
            check_all(out, probs, range(len(probs)), selection, n_eig, f"{D.case_id(case)} {variant} {selection} n_eig {n_eig}", worst,
                      complete=n_eig == D.N_EIG_ALL, rows=rows, global_diag=gd)


STRIDES = [(c, v) for c in D.STRIDE_CASES for v in D.LAUNCH_VARIANTS]


@pytest.mark.parametrize("case,variant", STRIDES, ids=[D.case_id(c) + "-" + v for c, v in STRIDES])
def test_second_slot_of_a_wavefront(ctx, monkeypatch, worst, case, variant):
    """Constant coefficient, no sharing pass: every agglomerate is solved, those beyond the grid by a wavefront that has solved one
    before.  Equal input, equal bits (what the sharing pass rests on): every member of a class against the class's first, the first
    against the reference.  Then the run with the sharing pass, which solves the firsts only: the same bits."""
    what = f"{D.case_id(case)} {variant}"
    ids, first = D.class_ids(case)
    monkeypatch.setenv(MEMO, "0")
    out = eigen(ctx, case, D.LAUNCH_N_EIG, variant, "krylov")
    for name in ARRAYS:
        odd = np.flatnonzero((out[name] != out[name][first][ids]).reshape(len(ids), -1).any(axis=1))
        assert odd.size == 0, f"{what}: {name} of {odd.size} agglomerates differ from the first of their class, first at {odd[:5]}"
    check_all(out, D.problems_of(case, variant, list(first)), first, "krylov", D.LAUNCH_N_EIG, what, worst)
    monkeypatch.delenv(MEMO)
    same_bits(eigen(ctx, case, D.LAUNCH_N_EIG, variant, "krylov"), out, f"{what}: shared solves against a solve each")


@pytest.mark.parametrize("variant", D.LAUNCH_VARIANTS)
def test_second_slot_with_every_problem_distinct(ctx, monkeypatch, worst, variant):
    """Linear coefficient: the sharing pass gives up, 17576 distinct problems stride.  The reference for a listed subset."""
    case = D.STRIDE_GIVE_UP
    what = f"{D.case_id(case)} {variant}"
    subset = D.give_up_subset(case)
    monkeypatch.delenv(MEMO, raising=False)
    out = eigen(ctx, case, D.LAUNCH_N_EIG, variant, "krylov")
    check_all(out, D.problems_of(case, variant, subset), subset, "krylov", D.LAUNCH_N_EIG, what, worst)
    monkeypatch.setenv(MEMO, "0")
    same_bits(eigen(ctx, case, D.LAUNCH_N_EIG, variant, "krylov"), out, f"{what}: no sharing pass against one that gives up")


SHARING = [(c, e, v) for c, e in D.SHARING_CASES for v in D.LAUNCH_VARIANTS]


@pytest.mark.parametrize("case,expect,variant", SHARING, ids=[D.case_id(c) + "-" + v for c, _, v in SHARING])
def test_sharing_pass_at_its_edges(ctx, monkeypatch, worst, case, expect, variant):
    what = f"{D.case_id(case)} {variant}"
    probs = D.problems(case, variant)
    rows = D.cpu_rows(cpu_R(case, variant, "krylov", D.LAUNCH_N_EIG), probs, "krylov", D.LAUNCH_N_EIG)
    monkeypatch.delenv(MEMO, raising=False)
    shared = eigen(ctx, case, D.LAUNCH_N_EIG, variant, "krylov")
    check_all(shared, probs, range(len(probs)), "krylov", D.LAUNCH_N_EIG, what, worst, rows=rows, global_diag=D.global_diagonal(case, variant))
    monkeypatch.setenv(MEMO, "0")
    same_bits(shared, eigen(ctx, case, D.LAUNCH_N_EIG, variant, "krylov"), f"{what}: shared solves against a solve each")
    monkeypatch.delenv(MEMO)
    prob = M.LaplaceProblem(case[0], case[2], device="cuda")
    info = M.Hierarchy(ctx, EVALUATOR[variant], prob, D.params_of(case, D.LAUNCH_N_EIG, variant, "krylov")).restrictor_eigensolver_info()
    print(what, info)
    assert info["solver"] == "device dense" and info["agglomerates"] == len(probs) and 1 <= info["solves"] <= info["agglomerates"]
    if expect == "less":
        assert info["solves"] < info["agglomerates"]
    elif expect == "equal":
        assert info["solves"] == info["agglomerates"]
