"""The host setup of the aggregation hierarchy (mfmg_amd.host_amg_build, no GPU) against the long-double restatement of
amg_reference.py, for every aggregate block size, and the proof that the per-entry bound bites.

Rule: |got - ref| <= bound per entry, bound = gamma_k mag with k counted from the code (header of amg_reference.py):
  P     k_P = 2 k_B + 2 blk^3 + n_row + 9      on  |t_i| [own] + w |d_i^-1| sum_j |a_ij| |t_j|
  A_c   n_A = n_row + n_col + 1                 on  |P|^T |A| |P|, plus what the bounds of P and of A_l do to it
        (first order, A_l exact: (n_A + 2 k_P) u on (mag P)^T |A| (mag P))
with n_row the longest row of A_l, n_col the longest column of P_l and k_B the inherited error of the near-null vector
(blk^3 + 1 per level).  The chain form is used: level l + 1 of the host setup is compared with the reference's own level
l + 1, the bound of A_l propagated into P_l and A_{l+1}.

Operators: Q1 stiffness matrices of the oracle on the node grid (free boundary: every node a 3^dim stencil), with the
"linear" and the "discontinuous" coefficient, coupled over C components by two different C x C blocks, so that no two
columns carry equal values; the near-null vector varies from node to node and between the components.

PLANTS are computed from the reference on the same inputs; each must fail the comparison.  OLD_RULE_PASSES names the ones
the rule these matrices were held to before -- max |got - ref| < 1e-11 max |ref| (test_transfer_shapes.py) -- lets through.
Worst |got - ref| / (u mag) of the host setup over all cases here (printed by the tests): P 85.6 (blk 2, C 1, fourth level: the
chain form, the error of the levels above included), A_c 11.9; with blocks of 3 and more P stays below 45 and A_c below 1.4."""
import numpy as np
import pytest
import scipy.sparse as sp

import mfmg_amd as M
import mfmg_oracle as O
import amg_reference as R

LD = np.longdouble
COARSEST = 4

# (node grid, components, block).  9 x 7 x 5: no block divides every axis; 8 x 8 x 8: 2, 4 and 8 do; 12 x 7: dims[2] missing;
# 10 x 3 x 2 with blocks of 4: two axes shorter than the block
CASES = [((9, 7, 5), C, blk) for blk in (2, 3, 4, 5, 8) for C in (1, 2, 3)]
CASES += [((8, 8, 8), C, blk) for blk, C in ((2, 2), (3, 1), (4, 3), (5, 2), (8, 2))]
CASES += [((12, 7), C, blk) for blk, C in ((2, 1), (3, 3), (4, 2), (5, 2), (8, 1))]
CASES += [((10, 3, 2), 2, 4)]


def test_long_double_has_a_64_bit_significand():
    assert np.finfo(LD).nmant >= 63
    x = sp.csr_matrix(np.array([[LD(1) + LD(2) ** -60]]))
    assert (x @ x)[0, 0] - 1 == LD(2) ** -59 + LD(2) ** -120 or (x @ x)[0, 0] - 1 == LD(2) ** -59      # (sparse products too)


_OPERATORS = {}


def operator(dims, C):
    """(A, B): a 3^dim-point operator on the node grid `dims` with C components per node, and a near-null vector."""
    if (dims, C) in _OPERATORS:
        return _OPERATORS[(dims, C)]
    mesh = O.StructuredMesh(tuple(d - 1 for d in dims))
    free = np.zeros(mesh.n_dofs, dtype=bool)
    A1 = O.assemble_csr(mesh, O.coefficient_table(mesh, "linear"), constrained=free)
    # (the oracle's discontinuous coefficient switches every 1/100 of the domain: scaled to the cells of these meshes)
    pts = mesh.quadrature_points() * np.array(mesh.n) / 100.0
    A2 = O.assemble_csr(mesh, O.material_property("discontinuous", pts), constrained=free)
    M1 = np.array([[2.0, 0.3, 0.1], [0.3, 1.5, 0.2], [0.1, 0.2, 1.2]])[:C, :C]
    M2 = np.array([[0.011, 0.002, 0.0], [0.002, 0.017, 0.003], [0.0, 0.003, 0.013]])[:C, :C]
    A = (sp.kron(A1, M1) + sp.kron(A2, M2) + sp.kron(sp.diags(0.05 * A1.diagonal()), np.eye(C))).tocsr()
    A.sort_indices()
    i, j, k = R.node_coordinates(dims)
    node = 1.0 + 0.4 * np.sin(0.9 * i + 0.3) * np.cos(0.7 * j) + 0.05 * k
    B = (node[:, None] * (1.0 + 0.25 * np.arange(C))[None, :]).ravel()
    assert B.min() > 0.3
    _OPERATORS[(dims, C)] = (A, B)
    return A, B


def host_levels(A, B, dims, C, blk, coarsest=COARSEST):
    n = A.shape[0]
    gd = list(R.grid3(dims)) if len(dims) == 3 else [dims[0], dims[1], 0]
    return M.host_amg_build(A, B, {"solver": {"amg": {"coarsest_size": coarsest, "aggregate_block": blk}}}, grid_dims=gd,
                            node_of_row=np.arange(n) // C, component_of_row=np.arange(n) % C)


_REFERENCE = {}


def reference(dims, C, blk):
    if (dims, C, blk) not in _REFERENCE:
        A, B = operator(dims, C)
        _REFERENCE[(dims, C, blk)] = R.reference_hierarchy(A, B, dims, C, blk, coarsest_size=COARSEST)
    return _REFERENCE[(dims, C, blk)]


@pytest.mark.parametrize("dims,C,blk", CASES)
def test_host_setup_is_within_the_bound_of_the_restatement(dims, C, blk):
    A, B = operator(dims, C)
    got = host_levels(A, B, dims, C, blk)
    levels, info = reference(dims, C, blk)
    assert len(levels) >= 2 and len(got) == len(levels), (len(got), len(levels))
    d = R.grid3(dims)
    worst_p = worst_a = 0.0
    for l, ((Ag, Pg), (Ar, Pr, Br), I) in enumerate(zip(got, levels, info)):
        assert I["dims"] == d
        assert Ag.shape[0] == int(np.prod(d)) * C
        if l > 0:
            worst_a = max(worst_a, R.compare(Ag, Ar, I["bound_A"], I["mag_A"], f"A_{l}", pattern="equal"))
            assert np.all(Br > 0)
        if Pr is not None:
            worst_p = max(worst_p, R.compare(Pg, Pr, I["bound_P"], I["mag_P"], f"P_{l}", pattern="equal"))
        d = R.coarse_dims(d, blk)
    print(f"{dims} C {C} blk {blk}: {len(levels)} levels, worst |got - ref| / (u mag): P {worst_p:.2f}, A_c {worst_a:.2f}")


def test_coarsening_rule():
    """ceil(dim / blk) per axis with a missing axis counting as 1, and the reach recurrence."""
    assert R.coarse_dims((9, 7, 5), 3) == (3, 3, 2) and R.coarse_dims((12, 7), 5) == (3, 2, 1) and R.coarse_dims((12, 7, 0), 8) == (2, 1, 1)
    assert R.coarse_dims((10, 3, 2), 4) == (3, 1, 1)
    assert [R.reach_recurrence(1, b) for b in (2, 3, 4, 5, 8)] == [2, 1, 1, 1, 1]
    assert [R.reach_recurrence(2, b) for b in (2, 3, 4)] == [3, 2, 2] and R.reach_recurrence(3, 2) == 5
    agg = R.aggregate_of_rows((5, 3), 2, 2)
    assert agg.tolist()[:10] == [0, 1, 0, 1, 2, 3, 2, 3, 4, 5] and agg.max() == 3 * 2 * 2 - 1


# ---- the bound bites ---------------------------------------------------------------------------------------------------------------
PLANTS = ["aliased_probe_of_P", "aliased_probe_of_A_c", "outermost_layer_of_A_c_dropped", "aggregate_boundary_shifted_on_the_clipped_side",
          "two_components_of_a_node_exchanged", "w_off_2^-40", "norm_of_B_over_the_unclipped_cube", "smoothed_prolongator_with_the_next_beta"]
# 1e-11 of the largest entry: an error of relative size 2^-40 = 9e-13 passes it wherever it sits, and the outermost layer of A_c --
# the couplings of aggregates that share no node, through the smoothing of both prolongators -- is small beside the diagonal
OLD_RULE_PASSES = {"w_off_2^-40"}
PLANT_CASES = [((11, 7, 5), 2, 2), ((10, 7, 5), 3, 3)]      # (dims[0] % blk != 0, and more coarse nodes along x than a period)


def _coarse_node_of_column(cols, dims_c, C):
    nd = cols // C
    return nd % dims_c[0], (nd // dims_c[0]) % dims_c[1], nd // (dims_c[0] * dims_c[1])


def _planted(dims, C, blk, plant):
    """[(what, matrix with the planted error, reference, bound)] on level 0 of the case."""
    A, B = operator(dims, C)
    ref = R.reference_level(A, B, dims, C, blk)
    P, Ac = ref["P"], ref["A_c"]
    cd = ref["dims_c"]
    r_c = R.reach_recurrence(1, blk)
    out = []
    if plant in ("aliased_probe_of_P", "aliased_probe_of_A_c"):
        # the column of coarse node (0, 1, 0) and the one a period further along x, summed where the probe is read
        period = (blk - 1 + 2) // blk + 1 if plant == "aliased_probe_of_P" else 2 * r_c + 1
        assert period < cd[0]
        Mx = (P if plant == "aliased_probe_of_P" else Ac).tolil(copy=True)
        j0, j1 = (cd[0] * 1 + 0) * C, (cd[0] * 1 + period) * C
        Mx[:, j0] = Mx[:, j0] + Mx[:, j1]
        out.append(("P" if plant == "aliased_probe_of_P" else "A_c", Mx.tocsr(), *((P, ref["bound_P"]) if plant == "aliased_probe_of_P" else (Ac, ref["bound_A"]))))
    elif plant == "outermost_layer_of_A_c_dropped":
        c = Ac.tocoo()
        ri, rj, rk = _coarse_node_of_column(c.row, cd, C)
        ci, cj, ck = _coarse_node_of_column(c.col, cd, C)
        dist = np.maximum(np.maximum(np.abs(ri - ci), np.abs(rj - cj)), np.abs(rk - ck))
        assert dist.max() == r_c
        keep = dist < r_c
        out.append(("A_c", sp.csr_matrix((c.data[keep], (c.row[keep], c.col[keep])), shape=Ac.shape), Ac, ref["bound_A"]))
    elif plant == "aggregate_boundary_shifted_on_the_clipped_side":
        assert dims[0] % blk != 0
        i, j, k = R.node_coordinates(dims)
        ix = np.where(i == (dims[0] // blk) * blk - 1, i + 1, i) // blk          # the last node of the last whole aggregate moves over
        agg = ((ix + cd[0] * (j // blk + cd[1] * (k // blk)))[:, None] * C + np.arange(C)[None, :]).ravel()
        bad = _level_with(A, B, dims, C, blk, agg=agg)
        out.append(("P", bad[0], P, ref["bound_P"]))
        out.append(("A_c", bad[1], Ac, ref["bound_A"]))
    elif plant == "two_components_of_a_node_exchanged":
        Mx = P.tolil(copy=True)
        r0 = (dims[0] * (dims[1] * 1 + 2) + 3) * C
        Mx[[r0, r0 + 1], :] = Mx[[r0 + 1, r0], :]
        out.append(("P", Mx.tocsr(), P, ref["bound_P"]))
    elif plant == "w_off_2^-40":
        bad = R.reference_level(A, B, dims, C, blk, omega=R.OMEGA * (1 + 2.0 ** -40))
        out.append(("P", bad["P"], P, ref["bound_P"]))
        out.append(("A_c", bad["A_c"], Ac, ref["bound_A"]))
    elif plant == "norm_of_B_over_the_unclipped_cube":
        # the last aggregate along x holds dims[0] % blk nodes per row of the cube: its norm taken as if all blk were there
        assert dims[0] % blk != 0
        Jx = cd[0] - 1
        scale = np.sqrt(LD(dims[0] % blk) / LD(blk))
        Mx = P.tolil(copy=True)
        Mx[:, Jx * C] = Mx[:, Jx * C] * scale
        out.append(("P", Mx.tocsr(), P, ref["bound_P"]))
    elif plant == "smoothed_prolongator_with_the_next_beta":
        nxt = R.reference_level(Ac, ref["B_c"], cd, C, blk)
        cheb = [(1, float(x["rho"]) / 4, float(x["rho"])) for x in (ref, nxt)]
        assert cheb[0] != cheb[1]
        good, mag, k = R.smoothed_prolongator(A, P, cheb[0])
        bad, _, _ = R.smoothed_prolongator(A, P, cheb[1])
        out.append(("P~", bad, good, mag * LD(R.gamma(k))))
    else:
        raise KeyError(plant)
    return out


def _level_with(A, B, dims, C, blk, agg):
    """P and A_c of one level with another aggregate map, stated again (the reference takes no map)."""
    A = sp.csr_matrix(A).astype(LD)
    B = B.astype(LD)
    n_c = int(np.prod(R.coarse_dims(dims, blk))) * C
    norm2 = np.zeros(n_c, dtype=LD)
    np.add.at(norm2, agg, B * B)
    Pt = sp.csr_matrix((B / np.sqrt(norm2)[agg], (np.arange(A.shape[0]), agg)), shape=(A.shape[0], n_c))
    d = A.diagonal()
    w = LD(R.OMEGA) / np.max(np.asarray(abs(A) @ np.ones(A.shape[0], dtype=LD)).ravel() / np.abs(d))
    P = (Pt - sp.diags(w / d) @ (A @ Pt)).tocsr()
    return P, (P.T @ (A @ P)).tocsr()


@pytest.mark.parametrize("dims,C,blk", PLANT_CASES)
def test_reference_rounded_to_double_is_within_the_bound(dims, C, blk):
    A, B = operator(dims, C)
    ref = R.reference_level(A, B, dims, C, blk)
    same = _level_with(A, B, dims, C, blk, agg=R.aggregate_of_rows(dims, C, blk))
    for what, got, want, bound, mag in (("P", same[0], ref["P"], ref["bound_P"], ref["mag_P"]), ("A_c", same[1], ref["A_c"], ref["bound_A"], ref["mag_A"])):
        got = got.astype(np.float64)
        assert R.compare(got, want, bound, mag, what, pattern="equal") <= 1.0       # (one rounding of the result)
        assert R.old_rule_passes(got, want)


@pytest.mark.parametrize("dims,C,blk", PLANT_CASES)
@pytest.mark.parametrize("plant", PLANTS)
def test_planted_error_is_beyond_the_bound(dims, C, blk, plant):
    results = _planted(dims, C, blk, plant)
    assert results
    for what, got, want, bound in results:
        got = sp.csr_matrix(got).astype(np.float64)
        assert not R.within(got, want, bound), f"{plant}: {what} within the bound"
        with pytest.raises(AssertionError):
            R.compare(got, want, bound, what=what)
    passes_old = all(R.old_rule_passes(sp.csr_matrix(got).astype(np.float64), want) for _, got, want, _ in results)
    print(f"{dims} C {C} blk {blk} {plant}: beyond the bound in {[w for w, *_ in results]}; 1e-11 of the largest entry lets it through: {passes_old}")
    assert passes_old == (plant in OLD_RULE_PASSES), plant


def test_an_entry_nobody_wrote_is_a_failure():
    A, B = operator((9, 7, 5), 1)
    ref = R.reference_level(A, B, (9, 7, 5), 1, 3)
    got = ref["P"].astype(np.float64).tocsr()
    got.data[7] = np.nan
    with pytest.raises(AssertionError):
        R.compare(got, ref["P"], ref["bound_P"], what="P")
