"""The rule of the batched Lanczos eigensolver (tests/amge_lanczos_rule.py: the numpy restatement of amge_lanczos.hip) against the
dense selection of the oracle (scipy's eigh + _select_eigenvectors) on the case table of the GPU tests: it is a second way to the
answer the dense paths give, within the sin-theta bound of its residual."""
import numpy as np
import pytest

import amge_lanczos_rule as RL


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(case, variant):
        key = (case, variant)
        if key not in cache:
            cache[key] = RL.agglomerate_problems(case[0], case[1], case[2], variant)
        return cache[key]
    return get


@pytest.mark.parametrize("variant", ["mf", "device"])
@pytest.mark.parametrize("case", RL.CASES, ids=RL.case_id)
def test_rule_gives_the_dense_krylov_selection(problems, case, variant):
    """Every selected vector and eigenvalue of every agglomerate, n_eig 4, tolerances 1e-12 and 1e-14: vectors within
    (sqrt 2 tolerance + 64 eps) / g entry by entry, eigenvalues within (tolerance + 64 eps) scale; no run unconverged, none
    longer than min(active DoFs, 200)."""
    breakdowns = 0
    for p in problems(case, variant):
        vals, vecs, w, g = RL.dense_selection(p, 4)
        scale = abs(w[-1])
        for tol in (1e-12, 1e-14):
            r = RL.lanczos_select(p["M"], p["v0"], 4, tol)
            assert r["converged"]
            assert r["iterations"] <= min(len(p["v0"]), 200)
            assert r["vectors"].shape == vecs.shape
            assert np.abs(r["vectors"] - vecs).max() <= RL.entry_bound(tol, g)
            assert np.abs(r["values"] - vals).max() <= (tol + 64 * RL.EPS) * scale
            breakdowns += r["breakdown"]
    if case[0] == (8, 8, 4):
        assert breakdowns == 2 * len(problems(case, variant))   # every agglomerate, at both tolerances


def test_host_variant(problems):
    case = ((8, 8, 8), (4, 4, 4), "linear")
    for p in problems(case, "host"):
        vals, vecs, w, g = RL.dense_selection(p, 2)
        r = RL.lanczos_select(p["M"], p["v0"], 2, 1e-12)
        assert r["converged"]
        assert np.abs(r["vectors"] - vecs).max() <= RL.entry_bound(1e-12, g)


def test_without_grouping_the_degenerate_copy_is_selected(problems):
    """(12, 6, 6) cells, one (6, 6, 6) agglomerate per half, constant: the run finds a second copy of the doubly degenerate second
    eigenvalue, grown out of rounding, before the fourth group has converged.  Taking the lowest Ritz pairs as they come selects
    that copy (a vector of noise, far from the dense selection); grouping the Ritz values by the 1e-9 rule of the dense selection
    and projecting the start vector onto each group removes it."""
    case = ((12, 6, 6), (6, 6, 6), "constant")
    for p in problems(case, "mf"):
        vals, vecs, w, g = RL.dense_selection(p, 4)
        grouped = RL.lanczos_select(p["M"], p["v0"], 4, 1e-12, group=True)
        plain = RL.lanczos_select(p["M"], p["v0"], 4, 1e-12, group=False)
        assert np.abs(grouped["vectors"] - vecs).max() <= RL.entry_bound(1e-12, g)
        assert np.abs(plain["vectors"] - vecs).max() > 0.1
        assert abs(plain["values"][2] - plain["values"][1]) <= 1e-9 * abs(w[-1])   # the copy


def test_max_iterations_ends_the_run_unconverged(problems):
    p = problems(((8, 8, 8), (4, 4, 4), "linear"), "mf")[0]
    r = RL.lanczos_select(p["M"], p["v0"], 4, 1e-12, max_iterations=10)
    assert r["iterations"] == 10 and not r["converged"] and not r["breakdown"]
    assert np.isfinite(r["vectors"]).all() and r["vectors"].shape[1] == 4


def test_library_carries_the_solver_and_its_constants(mfmg_lib):
    """The entry points of the Lanczos solver exist, the field count of the binding is the header's, and the breakdown constant of the
    kernel is the one of the restatement above."""
    import os
    import re
    from mfmg_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("mfmg_hip_amge_eigen", "mfmg_hip_hierarchy_restrictor_eigensolver_info"):
        assert hasattr(mfmg_lib, name)
    header = open(os.path.join(root, "include", "mfmg_hip.h")).read()
    assert int(re.search(r"#define\s+MFMG_HIP_EIGENSOLVER_INFO_FIELDS\s+(\d+)", header).group(1)) == L.EIGENSOLVER_INFO_FIELDS
    hpp = open(os.path.join(root, "mfmg_amd", "csrc", "amge_lanczos.hpp")).read()
    assert float(re.search(r"kLanczosBreakdown\s*=\s*([0-9.eE+-]+)", hpp).group(1)) == RL.BREAKDOWN
    assert int(re.search(r"kLanczosMaxNodes\s*=\s*(\d+)", hpp).group(1)) == 9 ** 3
