"""The case table of the coarse solvers' tests (tests/coarse_solver_cases.py) without a GPU: the table reaches what it names
(permutations that are neither the identity nor their own inverse, the tie, both sides of the 2048-row switch between the two
implementations and of the 512-row switch between the two SpMV kernels), every reference solves its system to long-double
rounding, and the acceptance function the GPU tests call accepts the restatement and LAPACK while it rejects every planted
defect: the inverse permutation, a dropped row exchange, L^-1 P with its columns left in place, a skipped division, an error of
64 n u in one entry; for the PCG one iteration too few, slots that do not alternate, NaN where the guards give the solution."""
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import coarse_solver_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = C.direct_names()
PIVOTING = [n for n in NAMES if n.split("_")[0] in ("rotated", "gaussian", "saddle")]


def source(name):
    return open(os.path.join(ROOT, "mfmg_amd", "csrc", name)).read()


def rejected(got, case):
    try:
        C.assert_solution(got, case)
    except AssertionError:
        return True
    return False


def test_constants_are_those_of_the_product():
    assert re.search(r"constexpr int kTriangularInverseLimit = (\d+);", source("amge_structured.hpp")).group(1) == str(C.INVERSE_LIMIT)
    hh = source("hip_hierarchy.hip")
    assert "if (n > kTriangularInverseLimit)" in hh
    assert hh.count(f"set_kernel(n >= {C.WIDE_ROWS_FROM} ? 256 : 64, 0);") == 2
    assert "const int cur = it & 1, nxt = cur ^ 1;" in hh
    assert "if (std::abs(A[(size_t)r * n + col]) > best)" in source("amge_structured.cpp")           # strict: the first maximal row
    assert "const double d = 1. / A[(size_t)col * n + col];" in source("amge_structured.cpp")
    assert "constexpr int kReduceBlocks = 1024;" in source("block_krylov.hpp") and "constexpr int block_size = 256;" in source("common.hpp")
    assert max(C.PCG_SIZES) > 1024 * 256                               # a second grid-stride trip in dot_stage1_kernel


def test_the_table_holds_the_cases_it_names():
    sizes = {n: C.direct_case(n, priced=False)["n"] for n in NAMES}
    assert len(set(NAMES)) == len(NAMES)
    assert sorted({s for n, s in sizes.items() if n.startswith("exact")}) == [1, 2, 3, 64, 65, 513]
    assert [sizes[f"rotated_{n}"] for n in C.ROTATED_SIZES] == [65, 511, 512, 513, 2048, 2049]
    assert [sizes[f"gaussian_{n}"] for n in C.GAUSSIAN_SIZES] == [3, 17, 65, 300, 2049]
    assert sizes["saddle"] == 340 and sizes["tie"] == 17 and sizes["control_30"] == 30
    # both sides of either switch
    assert {C.INVERSE_LIMIT, C.INVERSE_LIMIT + 1} <= set(sizes.values())
    assert {C.WIDE_ROWS_FROM - 1, C.WIDE_ROWS_FROM, C.WIDE_ROWS_FROM + 1} <= set(sizes.values())
    assert C.path_of(2048) == "inverse" and C.path_of(2049) == "substitution"
    # every permutation kind at every size that has room for it
    for n in (64, 65, 513):
        assert {f"exact_{k}_{n}" for k in ("identity", "transposition", "shift1", "shift7", "random_fixed_point")} <= set(NAMES)
    saddle = C.direct_case("saddle", priced=False)["A"]
    assert saddle[C.SADDLE_K:, C.SADDLE_K:].nnz == 0 and (saddle.diagonal()[C.SADDLE_K:] == 0).all()      # no stored diagonal there
    assert abs(saddle - saddle.T).max() == 0


@pytest.mark.parametrize("name", NAMES)
def test_reference_and_permutation(name):
    c = C.direct_case(name)
    A, b, n, perm = c["A"], c["b"], c["n"], c["perm"]
    # the reference solves the system to long-double rounding
    mag = C.ld_matvec(abs(A), np.abs(c["x_ref"])) + np.abs(b)
    assert np.abs(c["residual"]).max() <= n * 2.0 ** -60 * mag.max()
    assert sorted(perm) == list(range(n))
    family = name.split("_")[0]
    if name in PIVOTING:
        assert (perm != np.arange(n)).any() and not C.is_involution(perm)
    if family == "rotated":                                            # every row moves
        assert (perm == (np.arange(n) - C.ROTATION) % n).all()
    if family in ("exact", "triangular"):
        # perm undoes the permutation of the rows; the solution is a vector of doubles and solves the system exactly
        q = C.permutations_of(n)["_".join(name.split("_")[1:-1])]
        assert (perm == C.inverse_permutation(q)).all()
        assert (c["residual"] == 0).all() and (c["x_ref"].astype(np.float64).astype(C.LD) == c["x_ref"]).all()
        for path in c["restated_errors"]:
            assert c["restated_errors"][path] == (0.0, 0.0)
            assert np.array_equal(c["restated"]["x_" + path], c["x_ref"].astype(np.float64))
        if "shift" in name or "random" in name and n > 3:
            assert not C.is_involution(perm)                           # tells perm from its inverse
        if "random" in name:
            assert (perm == np.arange(n)).sum() >= 1
        if family == "triangular":
            assert np.count_nonzero(np.tril(c["restated"]["lu"], -1)) > 1000                         # L is not the identity
    if name == "tie":
        col = np.abs(A.toarray()[:, 0])
        assert list(np.flatnonzero(col == col.max())) == [3, 9] and perm[0] == 3                    # the first maximal row
    if name == "control_30":
        assert (perm == np.arange(n)).all()
    values = np.abs(np.concatenate([b, c["x_ref"].astype(np.float64)]))
    if n >= 64 and family != "triangular":
        assert values.max() / values[values > 0].min() > 1e4          # entries over several decades


def mutants(case):
    """(what, solution) produced from the restatement; the first three only where they change anything"""
    r, b, n = case["restated"], case["b"], case["n"]
    lu, perm = r["lu"], r["perm"]
    out = []
    if not C.is_involution(perm):
        out.append(("b[perm^-1] in place of b[perm]", C.substitute(lu, b[C.inverse_permutation(perm)])))
    if r["swaps"]:
        short = np.arange(n)
        for k, piv in r["swaps"][:-1]:
            short[[k, piv]] = short[[piv, k]]
        out.append(("the last row exchange dropped", C.substitute(lu, b[short])))
    if "linv" in r and (perm != np.arange(n)).any():
        out.append(("L^-1 P with its columns left unpermuted", r["uinv"] @ (r["linv"] @ b)))
    out.append(("a division skipped in the backward substitution", C.substitute(lu, b[perm], skip_division=n // 2)))
    bumped = r["x_" + case["path"]].copy()
    bumped[n // 3] += 64 * n * C.U64 * float(np.abs(case["x_ref"]).max())
    out.append(("64 n u max|x_ref| added to one entry", bumped))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_the_bound_bites(name):
    c = C.direct_case(name)
    assert C.assert_solution(c["restated"]["x_" + c["path"]], c) <= 1.0 / C.FACTOR          # the restatement itself passes
    if c["exact"]:
        lapack = sla.lu_solve(sla.lu_factor(c["A"].toarray()), c["b"])
        assert C.assert_solution(lapack, c) == 0.0 and np.array_equal(lapack, c["x_ref"].astype(np.float64))
    planted = mutants(c)
    if name in PIVOTING:                                               # all five (four beyond 2048 rows: no explicit inverses there)
        assert len(planted) == (5 if c["n"] <= C.INVERSE_LIMIT else 4)
    for what, x in planted:
        assert rejected(x, c), f"{name}: not noticed: {what}"
    assert rejected(np.full(c["n"], np.nan), c)


def test_every_mutant_is_planted_somewhere():
    seen = {}
    for name in NAMES:
        for what, _ in mutants(C.direct_case(name)):
            seen.setdefault(what, []).append(name)
    assert len(seen) == 5
    for what, names in seen.items():
        assert len(names) >= 15, what
    assert "rotated_2049" in seen["b[perm^-1] in place of b[perm]"] and "rotated_2048" in seen["L^-1 P with its columns left unpermuted"]


# ---- PCG
def pcg_rejected(got, case):
    try:
        C.assert_pcg(got, case)
    except AssertionError:
        return True
    return False


def test_pcg_table():
    assert C.PCG_SIZES == (1, 63, 64, 65, 1000, 300001) and C.PCG_ITERATIONS == (0, 1, 2, 5, 12)
    assert {i & 1 for i in C.PCG_ITERATIONS if i} == {0, 1}           # odd and even counts: the result's rz sits in either slot
    lo, di, up, b = C.pcg_system("scaled_tridiagonal", 1000)
    assert di.max() / di.min() > 50 and (lo == up).all()              # the Jacobi scaling matters
    A = C.pcg_matrix("scaled_tridiagonal", 1000)
    assert abs(A - A.T).max() == 0 and np.linalg.eigvalsh(A.toarray()).min() > 0
    d = C.pcg_system("diagonal", 65)[1]
    assert (np.frexp(d)[0] == 0.5).all()                               # powers of two


@pytest.mark.parametrize("n", C.PCG_SIZES)
@pytest.mark.parametrize("kind", C.PCG_KINDS)
def test_pcg_bound_bites(kind, n):
    _, di, _, b = C.pcg_system(kind, n)
    for n_it in C.PCG_ITERATIONS:
        c = C.pcg_case(kind, n, n_it)
        assert C.assert_pcg(c["x64"], c) <= 1.0 / C.FACTOR
        if n_it == 0:
            assert (c["x_ref"] == 0).all() and pcg_rejected(np.full(n, 1e-300), c)
            continue
        assert np.isfinite(c["x_ref"].astype(np.float64)).all()
        assert (C.pcg_restated(kind, n, n_it, C.LD, b=np.zeros(n)) == 0).all()                       # b = 0: the guards give zeros
        if kind == "diagonal":
            # converged after the first step: from the second on p^T A p = 0 and only the guards stand between D^-1 b and NaN
            assert np.array_equal(c["x64"], b / di) and np.array_equal(c["x_ref"], (b / di).astype(C.LD))
            unguarded = C.pcg_restated(kind, n, n_it, np.float64, guards=False)
            assert np.isnan(unguarded).all() == (n_it >= 2) and pcg_rejected(unguarded, c) == (n_it >= 2)
        elif n > 1:                                                    # (one unknown: converged after the first step)
            assert pcg_rejected(C.pcg_restated(kind, n, n_it - 1, np.float64), c), "one iteration too few"
            if n_it >= 2:
                assert pcg_rejected(C.pcg_restated(kind, n, n_it, np.float64, alternate=False), c), "slots not alternated"
        assert pcg_rejected(np.where(np.arange(n) == n // 2, np.nan, c["x64"]), c)
