"""The case table of test_gpu_residual_restriction.py (rr_cases.py) on the CPU: every edge of the tile march that the table is
there for is reached by a case -- and every case is the only one at some edge, so none can leave unnoticed -- and the per-row
bound gamma_256 |R| (|A| |x| + |b|) of the GPU test bites: with the restrictor of the oracle and the long-double reference
rounded to double standing in for a correct kernel it passes; with one defect of a wrong march planted at a time it fails."""
import functools

import numpy as np
import pytest

import mfmg_oracle as O
import rr_cases as C

# edge (named by what it is) -> predicate on plan(case).  Heights above 1 are what no test reached before: P, C and N live together.
EDGES = {
    "shortest run, height 1": lambda p: p["interior"] == 24 and p["runs"] == [24] and p["na"][1] == 2 and p["layers"] == [1] * 7,
    "tiles of 2, 2, 2, 1 layers": lambda p: p["interior"] == 24 and p["layers"] == [2, 2, 2, 1],
    "tiles of 3, 3, 1 layers": lambda p: p["interior"] == 24 and p["layers"] == [3, 3, 1],
    "tiles of 4, 3 layers": lambda p: p["interior"] == 24 and p["layers"] == [4, 3],
    "one tile of 17 node layers, two live wavefronts of eight": lambda p: p["layers"] == [7] and p["live_rows"] == [2],
    "nothing row-wise, height 1": lambda p: p["interior"] == 23 and p["segs"] == 0 and p["main_blocks"] == 0 and p["tile_layers"] == 1
    and p["listed"] == p["n_agg"],
    "nothing row-wise, height 3": lambda p: p["interior"] == 23 and p["segs"] == 0 and p["main_blocks"] == 0 and p["tile_layers"] == 3
    and p["listed"] == p["n_agg"],
    "run of exactly 62, rows 8 + 8 + 1, height 1": lambda p: p["runs"] == [62] and p["tail"] == 1 and p["live_rows"] == [8, 8, 1]
    and p["layers"] == [1, 1, 1],
    "run of exactly 62, tiles of 2, 1 layers": lambda p: p["runs"] == [62] and p["tail"] == 1 and p["layers"] == [2, 1],
    "run of exactly 62, one tile of 3 layers": lambda p: p["runs"] == [62] and p["tail"] == 1 and p["layers"] == [3],
    "tail of one, one full tile of rows, tiles of 2, 2 layers": lambda p: p["interior"] == 63 and p["tail"] == 2 and p["live_rows"] == [8]
    and p["layers"] == [2, 2],
    "tail of one, tiles of 3, 1 layers": lambda p: p["interior"] == 63 and p["tail"] == 2 and p["layers"] == [3, 1],
    "tail of one, one tile of 4 layers": lambda p: p["interior"] == 63 and p["tail"] == 2 and p["layers"] == [4],
    "two runs, the second of 24, height 1": lambda p: p["listed_runs"] == 0 and p["runs"] == [62, 24] and p["live_rows"] == [8, 1]
    and p["tile_layers"] == 1,
    "four workgroups beyond the last tile": lambda p: p["listed_runs"] == 0 and p["runs"] == [62, 24] and p["n_tiles"] == 12
    and p["main_blocks"] == 16 and p["layers"] == [2, 2, 1],
    "two runs, one tile per column": lambda p: p["listed_runs"] == 0 and p["runs"] == [62, 24] and p["layers"] == [5],
    "listed runs beside live rows, a table per row, height 1": lambda p: _listed_beside_live(p) and p["tile_layers"] == 1,
    "listed runs beside live rows, P live and C listed": lambda p: _listed_beside_live(p) and p["layers"] == [2, 2, 1],
    "listed runs beside live rows, one tile per column": lambda p: _listed_beside_live(p) and p["layers"] == [5],
}


def _listed_beside_live(p):
    """Runs in the list whose neighbours in the same tile, and whose own row in other layers, stay in the row-wise part."""
    s = p["listed_run_set"]
    if not s or p["segs"] != 2:
        return False
    k, j, sg = sorted(s)[0]
    tile = range(j // 8 * 8, min(j // 8 * 8 + 8, p["na"][1]))
    return any((k, jj, sg) not in s for jj in tile) and any((kk, j, sg) not in s for kk in range(p["na"][2])) \
        and 4 * p["listed"] <= p["n_agg"]


def _providers(cases):
    plans = {c: C.plan(*c) for c in cases}
    return {edge: [c for c in cases if reached(plans[c])] for edge, reached in EDGES.items()}


def test_case_table_covers_every_edge_of_the_march():
    prov = _providers(C.CASES)
    assert all(prov.values()), [e for e, c in prov.items() if not c]
    # no case can leave unnoticed: each is the only one at some edge
    alone = {c[0] for c in prov.values() if len(c) == 1}
    assert alone == set(C.CASES), set(C.CASES) - alone
    for case in C.CASES:
        rest = _providers([c for c in C.CASES if c != case])
        assert not all(rest.values()), case
    for name, (cells, material, heights) in C.MESHES.items():
        p = C.plan(name, heights[0])
        assert p["n_dofs"] < 100_000
        # what the host asks before it builds the form at all
        assert (p["segs"] > 0 and 4 * p["listed"] <= p["n_agg"]) or p["segs"] == 0
        assert max(heights) > 1 and max(heights) <= p["na"][2]
        if material == "constant":
            assert not p["listed_run_set"]


def test_planning_arithmetic():
    p = C.plan("62+24", 2)
    assert p["na"] == (88, 9, 5) and p["segs"] == 2 and p["main_last"] == 86 and p["tail"] == 1 and p["listed"] == 2 * 45
    assert p["tiles_j"] == 2 and p["n_tiles"] == 12 and p["main_blocks"] == 16
    assert C.plan("62+24", 2, "rows")["main_blocks"] == 24 and C.plan("23", 3, "rows")["main_blocks"] == 0
    p = C.plan("24", 7)
    assert p["na"] == (26, 2, 7) and p["main_last"] == 24 and p["listed"] == 14 * 2 and 2 * p["layers"][0] + 3 == 17
    assert C.plan("23", 1)["segs"] == 0 and C.plan("62", 1)["main_last"] == 62 and C.plan("63", 2)["main_last"] == 62
    # unset: whole rounds of two workgroups per CU -- below 512 tiles one layer per tile, on a 128^3-agglomerate mesh not
    assert all(C.plan(name, 0)["tile_layers"] == 1 for name in C.MESHES if C.plan(name, 0)["segs"])
    assert C.automatic_height(2, 16, 128) > 1
    # the changed cell of "rows": four runs, in the first run of rows 3, 4 of layers 1, 2
    p = C.plan("rows", 1)
    assert p["listed_run_set"] == {(k, j, 0) for k in (1, 2) for j in (3, 4)} and p["listed"] == 2 * 85 + 4 * 62
    coef = C.coefficient("rows")[:, 0].reshape(10, 34, 176)
    rows = coef[::2, ::2, 0]
    assert np.unique(rows).size == rows.size and rows.min() >= 1 and rows.max() < 10
    assert ((coef != coef[:, :, :1]).sum(), coef[4, 8, 62] / coef[4, 8, 61]) == (1, 0.5)


# ---- the bound bites ----
@functools.lru_cache(maxsize=None)
def _mesh(name):
    cells = C.MESHES[name][0]
    mesh, coef = O.StructuredMesh(cells), C.coefficient(name)
    R = O.build_restrictor(mesh, coef, O.MatrixFreeLaplace(mesh, coef).diagonal(), n_eig=2, variant="mf", eig_mode="krylov").csr
    # coarse row 2 ag + e, ag = i + na0 (j + na1 k), lives on the nodes 2 a .. 2 a + 2 of its agglomerate
    na, N = C.agglomerates(cells), mesh.N
    first = R.indices[R.indptr[:-1]]
    ag = np.arange(R.shape[0]) // 2
    assert np.array_equal(first, 2 * (ag % na[0]) + N[0] * (2 * (ag // na[0] % na[1]) + N[1] * 2 * (ag // (na[0] * na[1]))))
    sets = C.data_sets(name, mesh.n_dofs)
    return R, [(x, b) + C.reference(name, R, x, b) for x, b in sets]


MARCHING = [c for c in C.CASES if C.plan(*c)["tile_layers"] > 1]


@pytest.mark.parametrize("name", list(C.MESHES))
def test_reference_rounded_to_double_is_within_the_bound(name):
    R, sets = _mesh(name)
    for x, b, want, mag in sets:
        got, _ = C.planted(name, R, x, b, want, None)
        assert not C.beyond(got, want, mag).any() and C.worst_ratio(got, want, mag) <= 1.0
        got[7] = np.nan                                       # a row nobody wrote
        assert C.beyond(got, want, mag).sum() == 1


@pytest.mark.parametrize("plant", C.PLANTS)
@pytest.mark.parametrize("case", MARCHING, ids=C.case_id)
def test_planted_defect_of_the_march_is_beyond_the_bound(case, plant):
    """(The bound does not depend on the height: the cases of one mesh share its reference; the defect sits in agglomerate layer 1,
    whose layer below touches the face of the box -- on a constant coefficient the only neighbour with another table.)"""
    name = case[0]
    assert {c[0] for c in MARCHING} == set(C.MESHES)
    R, sets = _mesh(name)
    for scaled, (x, b, want, mag) in enumerate(sets):
        got, touched = C.planted(name, R, x, b, want, plant)
        bad = C.beyond(got, want, mag)
        print(f"{C.case_id(case)} {plant} scaled {bool(scaled)}: {int(bad.sum())} of {touched.size} touched rows beyond the bound")
        assert not bad[np.setdiff1d(np.arange(got.size), touched)].any()
        assert bad[touched].any()
        if not scaled:
            assert 4 * bad[touched].sum() > touched.size     # (the second row of an agglomerate has no weight on its middle layer)
