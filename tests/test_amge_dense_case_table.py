"""The case table of the dense agglomerate eigensolver's tests (tests/amge_dense_cases.py) without a GPU: every edge the table is
there for is reached by some case, the table is conditioned so that the 1e-9 grouping and the krylov selection do not hang on
rounding, the CPU path of the same rule (host_build_restrictor) and its numpy restatement pass every check with K_DENSE, and
planted defects in a reference result each fail the check that is there for them."""
import os
import re

import numpy as np
import pytest

import amge_dense_cases as D
import mfmg_amd as M
import mfmg_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def nloc_of(case):
    return np.prod(D.clipped_shapes(case) + 1, axis=1)


def test_constants_are_those_of_the_kernel_file():
    src = open(os.path.join(ROOT, "mfmg_amd", "csrc", "amge_device.hip")).read()
    assert "std::min<int64_t>((a.n_agg + wpb - 1) / wpb, 256 * 16)" in src and D.GRID_CAP == 4096
    assert "const int wpb = nmax == 27 ? 4 : 1;" in src and D.WAVES_PER_BLOCK == {27: 4, 64: 1}
    assert "nmax = nloc <= 27 ? 27 : 64;" in src
    assert re.search(r"n_all >= (\d+)", src).group(1) == str(D.SHARING_MIN)
    assert "<= 1e-9 * scale" in src and D.GROUP_RTOL == 1e-9
    assert "pn > 1e-12 * v0n" in src and D.PROJECTION_RTOL == 1e-12
    assert "off <= 1e-32 * (dsum + off)" in src


def test_every_edge_is_reached():
    by_shape = {(c[0], c[1]): c for c in D.SHAPE_CASES}
    # ---- the slot stride: only the stride cases give a wavefront a second agglomerate
    assert [D.n_agglomerates(c) for c in D.STRIDE_CASES] == [17576, 4624, 16512]
    assert [D.nmax_of(c) for c in D.STRIDE_CASES] == [27, 64, 27] and [len(c[0]) for c in D.STRIDE_CASES] == [3, 3, 2]
    assert D.n_agglomerates(D.STRIDE_CASES[0]) > D.GRID_CAP * 4 and D.n_agglomerates(D.STRIDE_CASES[1]) > D.GRID_CAP
    for c in D.STRIDE_CASES + [D.STRIDE_GIVE_UP]:
        assert D.slots_per_wave(c) == 2
    for c in D.SHAPE_CASES + [s[0] for s in D.SHARING_CASES]:
        assert D.slots_per_wave(c) == 1
    for c in D.STRIDE_CASES:                        # with the memo on, the classes fit one slot: the stride needs MFMG_AMGE_MEMO=0
        ids, first = D.class_ids(c)
        assert len(first) <= 27 and D.slots_per_wave(c, len(first)) == 1
    subset = D.give_up_subset(D.STRIDE_GIVE_UP)
    assert len(subset) <= 600 and set(range(16380, 16391)) <= set(subset) and subset[0] == 0 and subset[-1] == 17575
    # ---- shapes
    nl = {k: nloc_of(c) for k, c in by_shape.items()}
    assert set(nl[(7, 7, 3), (6, 2, 2)]) >= {63} and D.nmax_of(by_shape[(7, 7, 3), (6, 2, 2)]) == 64
    assert nl[(8, 4, 2), (7, 3, 1)].max() == 64 and nl[(14, 14), (7, 7)].max() == 64 and nl[(6, 6, 6), (3, 3, 3)].max() == 64
    assert nl[(7, 5, 4), (3, 2, 2)].max() == 36 and D.nmax_of(by_shape[(7, 5, 4), (3, 2, 2)]) == 64
    assert nl[(9, 7), (5, 4)].max() == 30 and D.nmax_of(by_shape[(9, 7), (5, 4)]) == 64      # 28 .. 30 nodes take the <64> kernel
    assert nl[(8, 8, 8), (2, 2, 2)].min() == 27 and D.nmax_of(by_shape[(8, 8, 8), (2, 2, 2)]) == 27
    assert set(nl[(3, 3, 3), (2, 2, 2)]) == {27, 18, 12, 8}                                   # clipped, down to one cell
    assert (D.clipped_shapes(by_shape[(4, 4, 4), (1, 1, 1)]) == 1).all() and D.n_agglomerates(by_shape[(4, 4, 4), (1, 1, 1)]) == 64
    assert (D.clipped_shapes(by_shape[(5, 9), (1, 3)])[:, 0] == 1).all()
    for k in [((7, 5, 4), (3, 2, 2)), ((7, 7, 3), (6, 2, 2)), ((8, 4, 2), (7, 3, 1)), ((9, 7), (5, 4)), ((5, 9), (1, 3))]:
        assert len(set(k[1])) > 1 and tuple(D.clipped_shapes(by_shape[k])[0]) == k[1]      # unequal sides, unclipped somewhere
    assert D.n_agglomerates(by_shape[(2, 2, 2), (2, 2, 2)]) == 1
    # ---- every variant x selection pair, every count
    assert set(D.VARIANTS) == {"mf", "device", "host"} and set(D.SELECTIONS) == {"krylov", "lapack"} and D.N_EIGS == (1, 2, 4, 8)
    assert len(D.combos()) == len(D.SHAPE_CASES) * 6
    # ---- active DoFs and counts
    one = D.problems(by_shape[(2, 2, 2), (2, 2, 2)], "mf")
    assert len(one) == 1 and one[0]["na"] == 1 and one[0]["nloc"] == 27
    for sel in D.SELECTIONS:
        assert [D.expected(one[0], sel, n)["n_vec"] for n in D.N_EIGS] == [1, 1, 1, 1]     # n_eig exceeds the active DoFs
    for case, variant, selection in D.COMPLETE:
        full = D.problems(case, variant)
        assert all(p["na"] == 27 and D.expected(p, selection, D.N_EIG_ALL)["n_vec"] == 27 for p in full)
    assert any(np.count_nonzero(np.triu(p["M"], 1)) > 100 for p in D.problems(D.COMPLETE[1][0], "device"))   # not only diagonal matrices
    clipped = D.problems(by_shape[(3, 3, 3), (2, 2, 2)], "mf")
    assert sorted({p["na"] for p in clipped}) == [1, 2, 4, 8]
    for sel in D.SELECTIONS:
        assert len({D.expected(p, sel, 8)["n_vec"] for p in clipped}) > 1                    # n_vec differs between agglomerates
    for case in D.SHAPE_CASES:                      # mf: constrained nodes inside the stride, to be left zero
        assert any(p["na"] < p["nloc"] for p in D.problems(case, "mf"))
    # ---- exactly degenerate groups in every variant of the constant cases, inside the first 8 eigenvalues
    for k in [((6, 6, 6), (3, 3, 3)), ((8, 8, 8), (2, 2, 2))]:
        for variant in D.VARIANTS:
            ties = [np.diff(p["w"][:9]).min() / p["scale"] for p in D.problems(by_shape[k], variant)]
            assert min(ties) <= 1e-14, (k, variant, min(ties))
    # ---- sharing
    assert [D.n_agglomerates(c) for c, _ in D.SHARING_CASES] == [63, 64, 90, 64]
    assert D.SHARING_MIN == 64


@pytest.mark.parametrize("case", [c for c, _ in D.SHARING_CASES if c[2] == "constant"] + [((12, 10), (2, 2), "constant")],
                         ids=D.case_id)
def test_classes_are_those_of_shape_and_constraint_flags(case):
    """class_ids keys per axis; here against the key the kernel hashes: clipped shape and the constraint flag of every node."""
    ids, first = D.class_ids(case)
    con = O.StructuredMesh(case[0]).constrained_mask()
    probs = D.problems(case, "device")
    keys = [(tuple(s), tuple(con[p["gl"]])) for s, p in zip(D.clipped_shapes(case), probs)]
    assert len(set(keys)) == len(first)
    for a, key in enumerate(keys):
        assert key == keys[first[ids[a]]]
        assert np.array_equal(probs[a]["M"], probs[first[ids[a]]]["M"])


def _conditioning(p, what, near_threshold, n_eigs):
    for n_eig in n_eigs:
        ex = D.expected(p, "krylov", n_eig)
        if near_threshold:
            assert ex["gap"] >= 10 * D.GROUP_RTOL, (what, n_eig, ex["gap"])
        else:
            assert ex["gap"] >= 1e-6, (what, n_eig, ex["gap"])
    last = D.expected(p, "krylov", max(n_eigs))["groups"][-1][1]
    steps = np.diff(p["w"][:min(last + 1, p["na"])]) / p["scale"]
    assert not ((steps > 1e-10) & (steps < 1e-8)).any(), (what, steps[(steps > 1e-10) & (steps < 1e-8)])
    return min(D.expected(p, "krylov", n)["gap"] for n in n_eigs)


@pytest.mark.parametrize("case", D.SHAPE_CASES, ids=D.case_id)
def test_conditioning_of_the_shape_cases(case):
    """krylov gaps of at least 1e-6 (near-threshold rows: at least 10 x the grouping threshold, and below 1e-6 somewhere, or the row
    would not be what it is there for); no two neighbouring eigenvalues up to the last selected group between 1e-10 and 1e-8 of
    the scale apart."""
    smallest = np.inf
    for variant in D.VARIANTS:
        for a, p in enumerate(D.problems(case, variant)):
            smallest = min(smallest, _conditioning(p, (D.case_id(case), variant, a), case in D.NEAR_THRESHOLD, D.N_EIGS))
    print(f"{D.case_id(case)}: smallest krylov gap {smallest:.3g}")
    if case in D.NEAR_THRESHOLD:
        assert smallest < 1e-6


def test_conditioning_of_the_launch_cases():
    for case in D.STRIDE_CASES + [c for c, _ in D.SHARING_CASES]:
        for variant in D.LAUNCH_VARIANTS:
            subset = D.class_ids(case)[1] if case[2] == "constant" else range(D.n_agglomerates(case))
            for a, p in zip(subset, D.problems_of(case, variant, list(subset))):
                _conditioning(p, (D.case_id(case), variant, a), False, (D.LAUNCH_N_EIG,))
    subset = D.give_up_subset(D.STRIDE_GIVE_UP)
    for variant in D.LAUNCH_VARIANTS:
        for a, p in zip(subset, D.problems_of(D.STRIDE_GIVE_UP, variant, subset)):
            _conditioning(p, ("give-up", variant, a), False, (D.LAUNCH_N_EIG,))


@pytest.fixture(scope="module")
def worst():
    w = D.Worst()
    yield w
    for name, (ratio, where) in w.items():
        print(f"CPU path, {name}: worst ratio {ratio:.4g} (K_DENSE {D.K_DENSE:g}) at {where}")


def _cpu_R(case, variant, selection, n_eig):
    prob = M.LaplaceProblem(case[0], case[2])
    return M.host_build_restrictor(prob, D.params_of(case, n_eig, variant, selection, "host"), variant == "mf")


@pytest.mark.parametrize("case", D.SHAPE_CASES, ids=D.case_id)
def test_cpu_path_passes_every_check(mfmg_lib, worst, case):
    """host_build_restrictor (the same rule on the CPU) through the checks with the same K_DENSE; it reports no eigenvalues."""
    stride = D.nmax_of(case)
    for variant in D.VARIANTS:
        probs = D.problems(case, variant)
        gd = D.global_diagonal(case, variant)
        for selection in D.SELECTIONS:
            runs = [(D.N_EIG_REF, D.N_EIGS)] + ([(D.N_EIG_ALL, (D.N_EIG_ALL,))] if (case, variant, selection) in D.COMPLETE else [])
            for n_ref, n_eigs in runs:
                rows = D.cpu_rows(_cpu_R(case, variant, selection, n_ref), probs, selection, n_ref)
                for a, p in enumerate(probs):
                    for n_eig in n_eigs:
                        nv, W = D.cpu_weights(p, rows, a, gd, n_eig, stride)
                        D.check_agglomerate(p, selection, n_eig, nv, W, None, worst=worst, complete=n_eig == D.N_EIG_ALL,
                                            what=f"{D.case_id(case)} {variant} {selection} n_eig {n_eig} agglomerate {a}")


SMALL = [c for c in D.SHAPE_CASES if D.nmax_of(c) == 27 and D.n_agglomerates(c) <= 30]


@pytest.mark.parametrize("case", SMALL, ids=D.case_id)
def test_numpy_restatement_passes_every_check(case):
    """jacobi_rule, which K_DENSE was measured with over the whole table, on the cases small enough for a test: the eigenvalue
    check included, which the CPU path cannot be put through."""
    for variant in D.VARIANTS:
        for a, p in enumerate(D.problems(case, variant)):
            for selection in D.SELECTIONS:
                for n_eig in D.n_eigs_of(case, variant, selection):
                    nv, W, ev = D.jacobi_result(p, selection, n_eig, 27)
                    D.check_agglomerate(p, selection, n_eig, nv, W, ev, complete=n_eig == D.N_EIG_ALL,
                                        what=f"{D.case_id(case)} {variant} {selection} n_eig {n_eig} agglomerate {a}")


def test_k_dense_is_the_measured_ratio_times_eight():
    assert D.K_DENSE == 2.0 ** np.ceil(np.log2(8 * D.MEASURED_WORST))


# ---- planted defects: a reference result with one thing wrong fails the check that is there for it ----
DEGENERATE = ((6, 6, 6), (3, 3, 3), "constant")
CLIPPED = ((3, 3, 3), (2, 2, 2), "linear")


def test_planted_perturbed_vector():
    for selection, name in (("krylov", "vector"), ("lapack", "residual")):
        probs = D.problems(CLIPPED, "device")
        p = max((q for q in probs if q["nloc"] == 27), key=lambda q: D.expected(q, "krylov", 2)["gap"])
        nv, W, ev = D.reference_result(p, selection, 2, 27)
        assert nv == 2
        D.check_agglomerate(p, selection, 2, nv, W, ev, what="as it is")
        W[1, 13] += 1e-9 * np.abs(p["diag_loc"]).max()
        with pytest.raises(AssertionError, match=name):
            D.check_agglomerate(p, selection, 2, nv, W, ev, what="perturbed")


def test_planted_swap_of_tied_columns_under_lapack(mfmg_lib):
    """Invisible to every basis-independent check; the CPU path's rows pin the order."""
    probs = D.problems(DEGENERATE, "device")
    gd = D.global_diagonal(DEGENERATE, "device")
    rows = D.cpu_rows(_cpu_R(DEGENERATE, "device", "lapack", 4), probs, "lapack", 4)
    p = probs[0]
    e = next(e for e in range(3) if p["w"][e + 1] - p["w"][e] <= 1e-12 * p["scale"])
    nv, W = D.cpu_weights(p, rows, 0, gd, 4, 64)
    D.check_against_cpu_rows(p, rows, 0, gd, 4, nv, W, what="as it is")
    W[[e, e + 1]] = W[[e + 1, e]]
    D.check_agglomerate(p, "lapack", 4, nv, W, None, what="swapped")
    with pytest.raises(AssertionError, match="same rule"):
        D.check_against_cpu_rows(p, rows, 0, gd, 4, nv, W, what="swapped")


def test_planted_group_split_at_1e_12():
    """A degenerate group pulled 1e-11 .. 1e-10 of the scale apart: one group by the rule, several to a selection that groups at 1e-12."""
    p0 = D.problems(DEGENERATE, "mf")[0]
    i, j = next(g for g in D.selected_groups(p0, 4) if g[1] - g[0] > 1)
    p = D.with_eigh({**p0, "M": p0["M"] + np.diag(np.linspace(-1.0, 1.0, p0["na"])) * 1e-10 * p0["scale"]})
    spread = (p["w"][j - 1] - p["w"][i]) / p["scale"]
    assert 2e-12 < spread < 5e-10 and (i, j) in D.selected_groups(p, 4)
    assert (i, j) not in D.selected_groups(p, 4, rtol=1e-12)
    nv, W, ev = D.reference_result(p, "krylov", 4, 64)
    D.check_agglomerate(p, "krylov", 4, nv, W, ev, what="as it is")
    _, vecs = O._select_eigenvectors(p["w"], p["V"], 4, "krylov", p["v0"], rtol=1e-12)
    W[:, np.flatnonzero(p["act"])] = (p["diag_loc"][p["act"]][:, None] * vecs).T
    with pytest.raises(AssertionError, match="vector"):
        D.check_agglomerate(p, "krylov", 4, nv, W, ev, what="split")


def test_planted_lexicographic_start_vector():
    p = D.problems(DEGENERATE, "mf")[-1]       # (at the near corner the two orders agree on the active DoFs)
    lcon = O.StructuredMesh(DEGENERATE[0]).constrained_mask()[p["gl"]]
    gen = O.MinstdRand0()
    v0 = np.array([0.0 if c else gen.uniform01() for c in lcon])[p["act"]]
    assert not np.array_equal(v0, p["v0"])
    assert any(j - i > 1 for i, j in D.selected_groups(p, 4))      # inside a degenerate group the start vector decides the direction
    nv, W, ev = D.reference_result(D.with_eigh({**p, "v0": v0}), "krylov", 4, 64)
    with pytest.raises(AssertionError, match="vector"):
        D.check_agglomerate(p, "krylov", 4, nv, W, ev, what="lexicographic")


@pytest.mark.parametrize("where", ["slot", "node", "constrained", "eigenvalue slot"])
def test_planted_nonzero_outside_the_result(where):
    p = D.problems(CLIPPED, "mf")[-1]                       # one cell, one active DoF
    assert p["nloc"] == 8 and p["na"] == 1
    nv, W, ev = D.reference_result(p, "krylov", 2, 27)
    D.check_agglomerate(p, "krylov", 2, nv, W, ev, what="as it is")
    if where == "slot":
        W[1, np.flatnonzero(p["act"])[0]] = 1e-300
    elif where == "node":
        W[0, p["nloc"]] = 1e-300
    elif where == "constrained":
        W[0, np.flatnonzero(~p["act"])[0]] = 1e-300
    else:
        ev[1] = 1e-300
    with pytest.raises(AssertionError, match="zeros"):
        D.check_agglomerate(p, "krylov", 2, nv, W, ev, what=where)


@pytest.mark.parametrize("selection", D.SELECTIONS)
def test_planted_eigenvalue_left_shifted(selection):
    p = D.problems(CLIPPED, "host")[0]
    assert p["shift"] > 1e-3 * p["scale"]
    nv, W, ev = D.reference_result(p, selection, 2, 27)
    D.check_agglomerate(p, selection, 2, nv, W, ev, what="as it is")
    with pytest.raises(AssertionError, match="eigenvalue"):
        D.check_agglomerate(p, selection, 2, nv, W, ev + p["shift"] * (ev != 0), what="shifted")
