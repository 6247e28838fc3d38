"""The setup of the aggregation hierarchy on the device (amg_device_setup.hip, probe_assembly.hip, the replicated tail of
finish_amg_replicated) for every aggregate block size, entry by entry against the long-double restatement of amg_reference.py.

Every case builds its hierarchy twice: "device" -- solver.amg.replicate_rows 1, every level through the probes -- and "tail" --
replicate_rows = the rows of the second level, so that finish_amg_replicated and the host products take over after the first.
Both run V(0,1) with a degree-1 smoother (pre_smoothing_levels 0, smoother_degree 1), so that every level that may carry a
smoothed prolongator P~ does: the probed form on device levels, the column-by-column form on replicated ones.  Then
  (a) full chain: P_l and A_{l+1} within the chain-form bound of the reference hierarchy built from the downloaded A_0 and the
      restated B_0 (row sums of R on component 0, 1 elsewhere); every nonzero of the reference is stored -- unless it lies within
      its own bound of zero: the assembly kernels drop a value that comes out as exactly 0.0, which happens with the constant
      coefficient of the one-cell cases --, every stored entry outside the reference's pattern is within the bound of zero;
  (b) per level: P_l and A_{l+1} against the restatement applied to the setup's own A_l (B_l by the norm recurrence from B_0);
  (c) P~_l within gamma_k (|P| + beta |D^-1| |A| |P|) of (I - beta D^-1 A_l) P_l of the setup's own A_l and P_l, beta = 1 / theta of
      the level's Chebyshev bounds; which levels carry one is asserted (float setups: none);
  (d) the reported reach and probe periods equal the integer rules stated in the test;
  (e) coarse_apply on a random right-hand side against the oracle's cycle on the REFERENCE levels, 1e-10 of the max-norm.
      (Not for "setup value precision" float: its matrices are rounded to 2^-24, the reference's are not.)
The counted k of every bound: header of amg_reference.py.  Worst |got - ref| / (u mag) on an MI355X: CHANGELOG.md."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
import mfmg_oracle as O
import amg_reference as R

GPU = pytest.mark.gpu
LD = np.longdouble
COARSEST = 4


def case(cid, n, agg, n_eig, blk, material="linear", evaluator="HipMatrixFreeMeshEvaluator", precision="double", reach=1):
    return dict(id=f"{cid}_blk{blk}", n=n, agg=agg, n_eig=n_eig, blk=blk, material=material, evaluator=evaluator, precision=precision,
                reach=reach)


CASES = [case("control_18x14x10", (18, 14, 10), (2, 2, 2), 2, 2)]
# reach stays 1; 9 x 7 x 5 -> 3 x 3 x 2, clipped on two axes
CASES += [case("clipped_18x14x10", (18, 14, 10), (2, 2, 2), 2, 3, "discontinuous")]
# blocks larger than an axis of the second level: the periods clamp to the level, coarse dimension 1
CASES += [case("clamped_18x14x10", (18, 14, 10), (2, 2, 2), 2, blk) for blk in (4, 5, 8)]
# a grid the block divides: 18 x 6 x 6 -> 6 x 2 x 2 -> 2 x 1 x 1
CASES += [case("divisible_36x12x12", (36, 12, 12), (2, 2, 2), 1, 3)]
CASES += [case(f"components{C}_12x12x12", (12, 12, 12), (2, 2, 2), C, blk) for C in (1, 3) for blk in (2, 3)]
# operator of reach 2 at the top: agglomerates one cell wide (the one_cell122 / one_cell221 shapes of test_transfer_shapes.py)
CASES += [case("one_cell122_ne1", (12, 8, 8), (1, 2, 2), 1, blk, "constant", reach=2) for blk in (2, 3, 4)]
CASES += [case("one_cell221_ne2", (4, 4, 10), (2, 2, 1), 2, blk, "constant", reach=2) for blk in (2, 3, 4)]
CASES += [case("two_dimensions_24x14", (24, 14), (2, 2), 2, blk) for blk in (2, 3)]
CASES += [case("assembled_12x10x8", (12, 10, 8), (2, 2, 2), 2, 3, evaluator="HipMeshEvaluator")]
CASES += [case("float_12x12x12", (12, 12, 12), (2, 2, 2), 2, blk, precision="float") for blk in (2, 3)]
BY_ID = {c["id"]: c for c in CASES}
MODES = ("device", "tail")
ALL = [(c["id"], mode) for c in CASES for mode in MODES]


def node_grid(c):
    return tuple(v // a for v, a in zip(c["n"], c["agg"]))


def planned_levels(c):
    """[(node grid, rows, reach)] by the coarsening rule: a level is coarsened while it has more than COARSEST rows."""
    dims, reach = R.grid3(node_grid(c)), c["reach"]
    out = [(dims, int(np.prod(dims)) * c["n_eig"], reach)]
    while out[-1][1] > COARSEST:
        dims, reach = R.coarse_dims(dims, c["blk"]), R.reach_recurrence(reach, c["blk"])
        out.append((dims, int(np.prod(dims)) * c["n_eig"], reach))
    return out


def test_case_table_reaches_what_it_names():
    """No GPU: every block size 2, 3, 4, 5, 8; clipped and divisible grids; a coarse dimension of 1 and a period clamped to the
    level; C = 1, 2, 3; the reach recurrences 2 -> 3, 2 -> 2 (blk 3) and 2 -> 2 (blk 4); two dimensions; every case has at least two
    levels and the first level at most about 2000 rows (dense long double)."""
    assert {c["blk"] for c in CASES} == {2, 3, 4, 5, 8} and {c["n_eig"] for c in CASES} == {1, 2, 3}
    plans = {c["id"]: planned_levels(c) for c in CASES}
    assert all(len(p) >= 2 and p[0][1] <= 2000 for p in plans.values())
    assert [d for d, _, _ in plans["clipped_18x14x10_blk3"]][:2] == [(9, 7, 5), (3, 3, 2)]
    assert [d for d, _, _ in plans["divisible_36x12x12_blk3"]] == [(18, 6, 6), (6, 2, 2), (2, 1, 1)]
    for b in (4, 5, 8):       # the block is larger than an axis of a level that is coarsened: that axis becomes 1
        p = plans[f"clamped_18x14x10_blk{b}"]
        assert any(min(d) < b and 1 in dc for (d, _, _), (dc, _, _) in zip(p[:-1], p[1:])), p
    assert [r for _, _, r in plans["one_cell122_ne1_blk2"]][:2] == [2, 3] and R.reach_recurrence(3, 2) == 5
    assert [r for _, _, r in plans["one_cell122_ne1_blk3"]][:2] == [2, 2] and [r for _, _, r in plans["one_cell122_ne1_blk4"]][:2] == [2, 2]
    assert len(plans["control_18x14x10_blk2"]) == 4 and [r for _, _, r in plans["control_18x14x10_blk2"]] == [1, 2, 3, 5]
    assert plans["two_dimensions_24x14_blk2"][0][0] == (12, 7, 1)
    # a period clamped to the level: (blk - 1 + 2 r) / blk + 1 or 2 r_c + 1 beyond the coarse grid of some level
    for c in CASES:
        p = plans[c["id"]]
        assert any(2 * rc + 1 > min(dc) for (_, _, _), (dc, _, rc) in zip(p[:-1], p[1:])), c["id"]


# ---------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def params_of(c, amg):
    return {"eigensolver": {"number of eigenvectors": c["n_eig"]}, "agglomeration": dict(zip(("nx", "ny", "nz"), c["agg"])),
            "is preconditioner": False, "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 2, "smoothing_range": 20.0},
            "setup value precision": c["precision"], "solver": {"type": "amg", "amg": amg}}


def amg_params(c, mode):
    plan = planned_levels(c)
    return {"coarsest_size": COARSEST, "setup": "device", "aggregate_block": c["blk"], "pre_smoothing_levels": 0, "smoother_degree": 1,
            "replicate_rows": 1 if mode == "device" else plan[1][1]}


_BUILT = {}
_CHAIN = {}
WORST = {}


def record(family, ratio, c=None):
    """Worst ratio per family; for a float setup in units of 2^-24, not of u."""
    if c is not None and c["precision"] == "float":
        family, ratio = "float setup, " + family, ratio * 2.0 ** -29
    WORST[family] = max(WORST.get(family, 0.0), ratio)


def built(ctx, cid, mode):
    """The hierarchy of a case and what it stores, downloaded once."""
    if (cid, mode) not in _BUILT:
        c = BY_ID[cid]
        prob = M.LaplaceProblem(c["n"], c["material"], device="cuda")
        h = M.Hierarchy(ctx, c["evaluator"], prob, params_of(c, amg_params(c, mode)))
        _BUILT[(cid, mode)] = dict(h=h, R=h.restrictor().to_scipy(), levels=h.coarse_amg_levels(), info=h.coarse_amg_setup_info(),
                                   smoothed=h.coarse_amg_smoothed_prolongators())
    return _BUILT[(cid, mode)]


def chain(ctx, cid):
    """The reference hierarchy of a case, from the A_0 and R the device mode downloaded (the tail mode must hold the same)."""
    if cid not in _CHAIN:
        c = BY_ID[cid]
        b = built(ctx, cid, "device")
        B0, kB0 = R.near_null_vector(b["R"], c["n_eig"])
        u_store = 2.0 ** -24 if c["precision"] == "float" else 0.0
        levels, info = R.reference_hierarchy(b["levels"][0][0], B0, node_grid(c), c["n_eig"], c["blk"], coarsest_size=COARSEST, kB0=kB0,
                                             u_store=u_store)
        _CHAIN[cid] = dict(levels=levels, info=info, B0=B0, kB0=kB0, u_store=u_store)
    return _CHAIN[cid]


@GPU
@pytest.mark.parametrize("cid,mode", ALL)
def test_levels_and_their_forms(ctx, cid, mode):
    """(d) and the plumbing: the number of levels, their sizes, which are replicated, how every A_c was formed, reach and periods."""
    c = BY_ID[cid]
    b = built(ctx, cid, mode)
    plan = planned_levels(c)
    blk = c["blk"]
    assert len(b["levels"]) == len(plan) >= 2, (len(b["levels"]), plan)
    first_replicated = len(plan) - 1 if mode == "device" else 1
    for l, ((A, P, cheb), I, (dims, rows, reach)) in enumerate(zip(b["levels"], b["info"], plan)):
        last = l + 1 == len(plan)
        assert A.shape == (rows, rows) and (P is None) == last
        assert I["reach"] == reach, (l, I)
        assert I["replicated"] == (l >= first_replicated), (l, I)
        if last:
            assert I["coarse_operator"] is None and I["period_p"] is None and I["period_a"] is None and I["period_t"] is None
            continue
        dc, rc = plan[l + 1][0], plan[l + 1][2]
        assert P.shape == (rows, plan[l + 1][1])
        if l >= first_replicated:
            assert I["coarse_operator"] == "host product" and I["period_p"] is None and I["period_a"] is None and I["period_t"] is None
        else:
            assert I["coarse_operator"] == "probes", (l, I)
            assert I["period_p"] == tuple(max(1, min((blk - 1 + 2 * reach) // blk + 1, d)) for d in dc), (l, I)
            assert I["period_a"] == tuple(max(1, min(2 * rc + 1, d)) for d in dc), (l, I)
            if c["precision"] == "double":
                assert I["period_t"] == tuple(max(1, min((blk - 1 + 4 * reach) // blk + 1, d)) for d in dc), (l, I)
        # the reach is what the pattern shows: no entry of A_l beyond it on any axis, and entries at it on one at least (an
        # agglomerate one cell wide along x reaches 2 along x only) unless the grid is narrower
        co = A.tocoo()
        keep = co.data != 0
        far = [int(np.abs(ri - ci).max()) for ri, ci in zip(node_xyz(co.row[keep], dims, c["n_eig"]), node_xyz(co.col[keep], dims, c["n_eig"]))]
        assert all(f <= min(reach, d - 1) for f, d in zip(far, dims)), (l, far)
        assert any(f == min(reach, d - 1) and d > 1 for f, d in zip(far, dims)), (l, far)
    if mode == "tail":
        A0 = built(ctx, cid, "device")["levels"][0][0]
        assert np.array_equal(A0.indptr, b["levels"][0][0].indptr) and np.array_equal(A0.data, b["levels"][0][0].data)
        assert np.array_equal(built(ctx, cid, "device")["R"].data, b["R"].data)


def node_xyz(rows, dims, C):
    nd = rows // C
    return nd % dims[0], (nd // dims[0]) % dims[1], nd // (dims[0] * dims[1])


@GPU
@pytest.mark.parametrize("cid,mode", ALL)
def test_full_chain_against_the_restatement(ctx, cid, mode):
    """(a)"""
    b = built(ctx, cid, mode)
    ch = chain(ctx, cid)
    assert len(b["levels"]) == len(ch["levels"])
    for l, ((A, P, _), (Ar, Pr, _), I) in enumerate(zip(b["levels"], ch["levels"], ch["info"])):
        if l > 0:
            record(f"{mode} chain A_c", R.compare(A, Ar, I["bound_A"], I["mag_A"], f"{cid} {mode} A_{l}"), BY_ID[cid])
        if Pr is not None:
            record(f"{mode} chain P", R.compare(P, Pr, I["bound_P"], I["mag_P"], f"{cid} {mode} P_{l}"), BY_ID[cid])
    print(f"{cid} {mode}: worst |got - ref| / (u mag) so far: {WORST}")


@GPU
@pytest.mark.parametrize("cid,mode", ALL)
def test_every_level_against_the_restatement_of_its_own_operator(ctx, cid, mode):
    """(b)"""
    c = BY_ID[cid]
    b = built(ctx, cid, mode)
    ch = chain(ctx, cid)
    B, kB, dims = ch["B0"], ch["kB0"], R.grid3(node_grid(c))
    for l, ((A, P, _), (A_next, _, _)) in enumerate(zip(b["levels"][:-1], b["levels"][1:])):
        r = R.reference_level(A, B, dims, c["n_eig"], c["blk"], kB=kB, u_store=ch["u_store"])
        record(f"{mode} level P", R.compare(P, r["P"], r["bound_P"], r["mag_P"], f"{cid} {mode} P_{l} of the setup's A_{l}"), c)
        if ch["u_store"]:
            # (a float setup multiplies the ROUNDED matrices: A_c of the prolongator it stored)
            r = R.reference_level(A, B, dims, c["n_eig"], c["blk"], kB=kB, u_store=ch["u_store"], P_given=P)
        record(f"{mode} level A_c", R.compare(A_next, r["A_c"], r["bound_A"], r["mag_A"], f"{cid} {mode} A_{l + 1} of the setup's A_{l}"), c)
        B, kB, dims = r["B_c"], r["kB_next"], r["dims_c"]
    print(f"{cid} {mode}: worst |got - ref| / (u mag) so far: {WORST}")


@GPU
@pytest.mark.parametrize("cid,mode", ALL)
def test_smoothed_prolongator_of_the_cycle(ctx, cid, mode):
    """(c)"""
    c = BY_ID[cid]
    b = built(ctx, cid, mode)
    n = len(b["levels"])
    carried = [Pt is not None for Pt in b["smoothed"]]
    assert carried == [c["precision"] == "double" and l + 1 < n for l in range(n)], carried
    assert [I["smoothed"] for I in b["info"]] == carried
    with pytest.raises(L.MfmgNotImplementedError, match="not built"):
        h = b["h"]
        L.check(h._lib.mfmg_hip_hierarchy_coarse_amg_get(h.handle, n - 1, 3, ctypes.byref(ctypes.c_void_p())))
    for l, ((A, P, cheb), Pt, I) in enumerate(zip(b["levels"], b["smoothed"], b["info"])):
        if Pt is None:
            continue
        assert cheb[0] == 1
        ref, mag, k = R.smoothed_prolongator(A, P, cheb)
        form = "columns" if I["replicated"] else "probed"
        assert (I["period_t"] is None) == I["replicated"]
        record(f"P~ {form}", R.compare(Pt, ref, mag * LD(R.gamma(k)), mag, f"{cid} {mode} P~_{l} ({form})"))
    if c["precision"] == "double":
        forms = {"columns" if I["replicated"] else "probed" for I in b["info"][:-1]}
        assert forms == ({"probed"} if mode == "device" else ({"probed", "columns"} if n > 2 else {"probed"})), forms
    print(f"{cid} {mode}: worst |got - ref| / (u mag) so far: {WORST}")


@GPU
@pytest.mark.parametrize("cid,mode", [(cid, mode) for cid, mode in ALL if BY_ID[cid]["precision"] == "double"])
def test_cycle_against_the_oracle_on_the_reference_levels(ctx, cid, mode):
    """(e)"""
    b = built(ctx, cid, mode)
    ch = chain(ctx, cid)
    levels = [(sp.csr_matrix(A.astype(np.float64)), None if P is None else sp.csr_matrix(P.astype(np.float64)), got[2])
              for (A, P, _), got in zip(ch["levels"], b["levels"])]
    solve = O.amg_coarse_solver(levels, 1, pre_smoothing_levels=0)
    n = levels[0][0].shape[0]
    rhs = np.random.default_rng(17).standard_normal(n)
    want = solve(rhs)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    b["h"].coarse_apply(dev(rhs), x)
    ctx.synchronize()
    got = x.cpu().numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{cid} {mode}: cycle differs by {err:.2e} of the max-norm")
    assert err < 1e-10


# ---- A_c by the CSR product on the device ------------------------------------------------------------------------------------
# by_product of amg_device_setup.hip: n_col_a = prod_d min(2 r_c + 1, coarse dim d) C >= 1024, n_c <= 8192 and 2 n_col_a >= n_c.
# With blk = 2 the coarse reach is 2, 3, 5 on the first three levels.  C = 3 needs prod >= 342, so 7 x 7 x 7 = 343 probes per
# component: a period of 7 = 2 * 3 + 1 on a coarse grid of at least 7 nodes per axis, which is the THIRD level (r_c = 3) of a first
# level of 25 nodes per axis (25 -> 13 -> 7; 24 -> 12 -> 6 gives 216 * 3 = 648 < 1024).  Then n_c = 1029 <= 8192 and 2 * 1029 >= 1029.
# C = 2 needs 512 = 8^3, a period of 8 <= 2 r_c + 1 with r_c >= 4: the fourth level, at least 57 nodes per axis at the top (57 -> 29 -> 15 -> 8); C = 4 needs
# 7 x 7 x 6, 25 x 25 x 21 nodes with 4 rows each: more rows than 25^3 x 3.  So: 50^3 cells, 2 x 2 x 2 agglomerates, 3 eigenvectors.
PRODUCT = case("product_50x50x50", (50, 50, 50), (2, 2, 2), 3, 2)
PRODUCT_COARSEST = 8


def product_plan():
    dims, reach, C, out = R.grid3(node_grid(PRODUCT)), 1, PRODUCT["n_eig"], []
    while int(np.prod(dims)) * C > PRODUCT_COARSEST:
        dc, rc = R.coarse_dims(dims, 2), R.reach_recurrence(reach, 2)
        n_col_a, n_c = int(np.prod([min(2 * rc + 1, d) for d in dc])) * C, int(np.prod(dc)) * C
        out.append(dict(dims=dims, reach=reach, rows=int(np.prod(dims)) * C, by_product=n_col_a >= 1024 and n_c <= 8192 and 2 * n_col_a >= n_c))
        dims, reach = dc, rc
    out.append(dict(dims=dims, reach=reach, rows=int(np.prod(dims)) * C, by_product=False))
    return out


def test_the_product_case_is_the_smallest_that_reaches_the_branch():
    plan = product_plan()
    assert [p["by_product"] for p in plan] == [False, True, False, False, False, False] and plan[1]["dims"] == (13, 13, 13)
    for n, C in (((48, 48, 48), 3), ((50, 50, 48), 3), ((50, 50, 40), 4), ((112, 112, 112), 2)):
        dims, reach, hit = tuple(v // 2 for v in n), 1, False
        while int(np.prod(dims)) * C > PRODUCT_COARSEST:
            dims, reach = R.coarse_dims(dims, 2), R.reach_recurrence(reach, 2)
            n_col_a, n_c = int(np.prod([min(2 * reach + 1, d) for d in dims])) * C, int(np.prod(dims)) * C
            hit = hit or (n_col_a >= 1024 and n_c <= 8192 and 2 * n_col_a >= n_c)
        assert not hit, (n, C)


_PRODUCT = {}


def product_built(ctx):
    if not _PRODUCT:
        c = PRODUCT
        amg = dict(amg_params(c, "device"), coarsest_size=PRODUCT_COARSEST)
        prob = M.LaplaceProblem(c["n"], c["material"], device="cuda")
        h = M.Hierarchy(ctx, c["evaluator"], prob, params_of(c, amg))
        _PRODUCT.update(h=h, R=h.restrictor().to_scipy(), levels=h.coarse_amg_levels(), info=h.coarse_amg_setup_info())
        forms = []
        for l in range(len(_PRODUCT["levels"])):
            v = ctypes.c_void_p()                              # (one borrowed view at a time)
            L.check(h._lib.mfmg_hip_hierarchy_coarse_amg_get(h.handle, l, 0, ctypes.byref(v)))
            forms.append(M.SparseMatrixDevice(ctx, _handle=v, _borrowed=True, _keepalive=h).form())
        _PRODUCT.update(forms=forms)
    return _PRODUCT


@GPU
def test_product_branch_ran_on_one_level_and_no_other(ctx):
    """(d)"""
    b = product_built(ctx)
    plan = product_plan()
    assert len(b["levels"]) == len(plan)
    for l, (I, p, (A, P, _)) in enumerate(zip(b["info"], plan, b["levels"])):
        assert A.shape[0] == p["rows"] and I["reach"] == p["reach"]
        if P is not None:
            assert I["coarse_operator"] == ("device product" if p["by_product"] else "probes"), (l, I)
            assert (I["period_a"] is None) == p["by_product"] and I["period_p"] is not None
        assert I["replicated"] == (l + 1 == len(plan))
        assert I["smoothed"] == (P is not None and p["rows"] <= 16384), (l, I)


@GPU
def test_product_case_every_level_against_the_restatement_in_float64(ctx):
    """(b) in float64: the reference and the setup are both within the bound of the exact value, so they may differ by twice the
    bound.  Every level is compared before the test fails, so that a failure names all of them.

    Level 0 (46 875 rows) is the only level of this file large enough for the block-diagonal SpMV layout (n >= 32768), and that
    layout keeps a matrix that is symmetric to 1e-13 of its diagonal as its upper half (build_block_diagonals): the operator the
    probes apply has a_ji where the downloaded CSR has a_ij.  R A R^T is symmetric only to the rounding of its own probes, which
    is relative to the large entries of a row, so on an entry seven decades below them the two differ by hundreds of u (first
    seen here: P_0 at (3942, 20), 1.6e-7, off by 6.0e-21 against twice the bound 5.8e-21 without this term).  So on a level that
    reports the symmetric half the applied operator is the downloaded one up to E = |A - A^T| per entry, and E enters the bound as
    the error of A_l does in the chain form -- the larger magnitude, from the layout's own rule, asserted below."""
    c = PRODUCT
    b = product_built(ctx)
    B, kB = R.near_null_vector(b["R"], c["n_eig"])
    B, dims = B.astype(np.float64), R.grid3(node_grid(c))
    failures = []
    assert [bool(f["symmetric_half"]) for f in b["forms"]][:2] == [True, False]      # (the layout is reached, and by level 0 alone)
    for l, ((A, P, _), (A_next, _, _)) in enumerate(zip(b["levels"][:-1], b["levels"][1:])):
        E = None
        if b["forms"][l]["symmetric_half"]:
            E = abs(A - A.T).tocsr()
            assert E.max() <= 1e-13 * abs(A.diagonal()).max()          # (what the layout accepted as symmetric)
        r = R.reference_level(A, B, dims, c["n_eig"], c["blk"], kB=kB, E=E, dtype=np.float64)
        for family, got, want, bound, mag, what in (("float64 level P", P, r["P"], r["bound_P"], r["mag_P"], f"P_{l} of the setup's A_{l}"),
                                                   ("float64 level A_c", A_next, r["A_c"], r["bound_A"], r["mag_A"], f"A_{l + 1} of the setup's A_{l}")):
            try:
                record(family, 0.5 * R.compare(got, want, 2 * bound, mag, what, dtype=np.float64))
            except AssertionError as e:
                failures.append(str(e))
        B, kB, dims = r["B_c"], r["kB_next"], r["dims_c"]
    print(f"product case: half the worst |got - ref| / (u mag) of the levels within the bound: {WORST}")
    assert not failures, "\n".join(failures)


@GPU
def test_product_case_cycle_against_the_oracle_on_the_reference_levels(ctx):
    """(e) in float64."""
    c = PRODUCT
    b = product_built(ctx)
    B, _ = R.near_null_vector(b["R"], c["n_eig"])
    ref, _ = R.reference_hierarchy(b["levels"][0][0], B.astype(np.float64), node_grid(c), c["n_eig"], c["blk"], coarsest_size=PRODUCT_COARSEST,
                                   dtype=np.float64, bounds=False)
    assert len(ref) == len(b["levels"])
    levels = [(A, P, got[2]) for (A, P, _), got in zip(ref, b["levels"])]
    solve = O.amg_coarse_solver(levels, 1, pre_smoothing_levels=0)
    n = levels[0][0].shape[0]
    rhs = np.random.default_rng(17).standard_normal(n)
    want = solve(rhs)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    b["h"].coarse_apply(dev(rhs), x)
    ctx.synchronize()
    err = np.abs(x.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"product case: cycle differs by {err:.2e} of the max-norm")
    assert err < 1e-10


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@GPU
@pytest.mark.parametrize("blk", [1, 9])
def test_block_sizes_outside_2_to_8_are_refused(ctx, blk):
    c = BY_ID["components1_12x12x12_blk2"]
    amg = dict(amg_params(c, "device"), aggregate_block=blk)
    prob = M.LaplaceProblem(c["n"], c["material"], device="cuda")
    with pytest.raises(L.MfmgError, match=r"must be in 2\.\.8"):
        M.Hierarchy(ctx, c["evaluator"], prob, params_of(c, amg))


def test_host_setup_refuses_block_sizes_outside_2_to_8():
    A = sp.identity(8, format="csr")
    for blk in (1, 9):
        with pytest.raises(L.MfmgInvalidArgument, match=r"must be in 2\.\.8"):
            M.host_amg_build(A, np.ones(8), {"solver": {"amg": {"aggregate_block": blk}}}, grid_dims=[2, 2, 2], node_of_row=np.arange(8))


@GPU
def test_device_setup_without_a_smoothed_prolongator_is_refused(ctx):
    c = BY_ID["components1_12x12x12_blk2"]
    amg = dict(amg_params(c, "device"), smooth_prolongator=False)
    prob = M.LaplaceProblem(c["n"], c["material"], device="cuda")
    with pytest.raises(L.MfmgError, match="the device setup of the aggregation hierarchy needs the agglomerate grid of the restrictor, a "
                                          "smoothed prolongator"):
        M.Hierarchy(ctx, c["evaluator"], prob, params_of(c, amg))
