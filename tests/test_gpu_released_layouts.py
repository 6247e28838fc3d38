"""SparseMatrixDevice.release_csr() on every table-driven layout of test_spmv_layouts.py: the launches of a released matrix
have the bits of the launches before the release, and what reads the freed arrays throws.

release_csr() frees val / col / row_ptr (device and host) of a matrix whose kernels read tables -- node classes, or block
diagonals with regular rows and at most 32768 listed rows -- and keeps the listed rows as a packed CSR in the order of the
list; listed_row_wave then reads kept_ptr[w] where it read row_ptr[row].  RELEASABLE / DECLINING below are the case table of
test_spmv_layouts.py cut by that rule, written out by id; a test without a GPU holds the two lists to the rule and to the
forms the released matrices have to reach.

Per releasable matrix (test_released_layout): every mode, both (alpha, beta) pairs, the 8-byte offset for C = 2 and the two
boundary-shell vectors before and after the release, compared with torch.equal -- the kernels, tables, planes, summation
order and lane assignment do not change, the listed rows read the same values from the packed copy --, then against the
long-double reference at the bound of test_spmv_layouts.py, a repeated launch, a second release_csr(), and launch_block with
three rows in the guarded layout of test_gpu_csr_block.py (width 1: the loop over the rows).

What the Python API reaches of the three readers of the freed arrays (a later method that reads them belongs in
test_released_matrix_refuses_what_reads_its_arrays):
  ensure_device_csr <- launch() of a matrix that is not released, release_csr() itself, transpose() [transpose(),
                       apply(.., TRANS) through HipMatrixOperator::get_transposed_matrix], mmult() on both operands
                       [multiply()], inverse_diagonal() [inverse_diagonal(), solve() with pcg], row_ratios() [the smoother
                       setup of solve() with amg], build_block_diagonals() (construction only);
  ensure_host_copy  <- host_row_ptr / host_col / host_val (the setup of a hierarchy), choose_layouts (construction only);
  download          <- to_scipy(), transpose() / mmult() on their host paths, HipSolver::setup_direct [solve() with a
                       direct solver, behind its size limit], the host setup of solve() with amg.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
from test_gpu_csr_block import guarded, guards_intact
from test_spmv_layouts import (ALPHA_BETA, ALPHA_BETA_2, BY_ID, CASES, GENERATORS, assert_within, check_form, launch, make_inputs,
                               modes_of, operands, prolongator_matrix, reference, seed_of, shell_vectors, stencil_matrix)

LIMIT = 32768                       # kListedWaveRows: listed rows up to which each gets a wavefront, and a matrix lets go

RELEASABLE = [
    "inv_r1_c1", "inv_r1_c2", "inv_r1_c3", "inv_r1_c4", "inv_r1_c2_f32", "inv_r1_c2_nonsym", "inv_r2_c1", "inv_r2_c2", "inv_r3_c1",
    "inv_r2_c2_p16_never", "own_r1_c1", "own_r1_c2", "own_r1_c3", "own_r1_c4", "own_r2_c1", "own_r2_c2", "own_r3_c1",
    "shell_perturbed_c1", "layer1_r1", "layer2_r1", "layer2_r2", "layer4_r2", "chain_8255", "chain_8256", "chain_8257",
    "slots_834", "slots_835", "slots_851", "nodecls_tail4_1", "nodecls_tail16_1", "nodecls_tail4_3", "nodecls_tail16_3",
    "nodecls_tail4_4", "nodecls_tail16_4", "nodecls_tail4_5", "nodecls_tail16_5", "nodecls_tail4_16", "nodecls_tail16_16",
    "nodecls_tail4_17", "nodecls_tail16_17", "nodecls_tail16_33", "nodecls_r2_wide_p16", "nodecls_transposed"]

DECLINING = [
    ("inv_r1_c1", "stored"), ("inv_r1_c1", "csr"), ("inv_r1_c2", "stored"), ("inv_r1_c2", "csr"), ("inv_r1_c3", "stored"),
    ("inv_r1_c3", "csr"), ("inv_r1_c4", "stored"), ("inv_r1_c4", "csr"), ("inv_r1_c2_f32", "stored"), ("inv_r1_c2_f32", "csr"),
    ("inv_r1_c2_nonsym", "stored"), ("inv_r1_c2_nonsym", "csr"), ("inv_r2_c1", "stored"), ("inv_r2_c1", "csr"),
    ("inv_r2_c2", "stored"), ("inv_r2_c2", "csr"), ("inv_r3_c1", "stored"), ("inv_r2_c2_p16_never", "stored"),
    ("inv_r2_c2_p16_never", "csr"), ("many_listed_sym", "tables"), ("many_listed_sym_f32", "tables"),
    ("many_listed_nonsym", "tables"), ("planes_sym_c1", "stored"), ("planes_sym_c1_f32", "stored"), ("planes_nonsym_c2", "stored"),
    ("planes_nonsym_c2_f32", "stored"), ("planes_sym_c3_f32", "stored"), ("planes_nonsym_c4", "stored"), ("layer1_r1", "stored"),
    ("layer1_r1", "csr"), ("layer2_r1", "csr"), ("layer2_r2", "csr"), ("layer4_r2", "csr"), ("chain_8255", "stored"),
    ("chain_8256", "stored"), ("chain_8257", "stored"), ("slots_834", "stored"), ("slots_835", "stored"), ("slots_851", "stored"),
    ("nodecls_tail4_1", "csr"), ("nodecls_tail16_1", "csr"), ("nodecls_tail4_3", "csr"), ("nodecls_tail16_3", "csr"),
    ("nodecls_tail4_4", "csr"), ("nodecls_tail16_4", "csr"), ("nodecls_tail4_5", "csr"), ("nodecls_tail16_5", "csr"),
    ("nodecls_tail4_16", "csr"), ("nodecls_tail16_16", "csr"), ("nodecls_tail4_17", "csr"), ("nodecls_tail16_17", "csr"),
    ("nodecls_tail16_33", "csr"), ("nodecls_r2_wide_p16", "csr"), ("row_base", "row_base"), ("row_base_transposed", "transpose"),
    ("thinned_lds", "lds"), ("ragged", "lanes64"), ("long_rows", "row_block")]

# a `stored` / `csr` variant switched back to its tables lets go after all: (case, variant) -> the call that undoes the switch
UNDO = {("inv_r1_c2", "stored"): ("set_regular_rows", True), ("inv_r1_c2", "csr"): ("set_kernel", 0, 3),
        ("nodecls_tail4_5", "csr"): ("set_kernel", 0, 5)}

# three shapes of this file's own: no listed row at all (kept arrays of one element), and the two sides of the limit
NO_LISTED = dict(gen="prolongator", args=dict(dims=(17, 16, 16), perturb=0), shell=((17, 16, 16), 1))
LIMIT_DIMS = (48, 48, 40)           # 92160 rows; the eight corner nodes form no class of 8 members and are listed as well
AT_LIMIT = dict(gen="stencil", args=dict(dims=LIMIT_DIMS, perturb=LIMIT - 8, seed=81), shell=(LIMIT_DIMS, 1))
OVER_LIMIT = dict(gen="stencil", args=dict(dims=LIMIT_DIMS, perturb=LIMIT - 7, seed=82), shell=(LIMIT_DIMS, 1))


def own_case(cid, shape):
    return dict(id=cid, gen=shape["gen"], args=shape["args"], env={}, transpose=False, shell=shape["shell"], variants=[])


# ---- the table, without a GPU ---------------------------------------------------------------------------------------
def releasable_by_rule(c):
    f = c["variants"][0]["form"]
    return f.get("regular") == 1 and f.get("listed_route") != "stored_planes"


def test_the_two_lists_are_the_case_table_cut_by_the_rule():
    releasable = [c["id"] for c in CASES if releasable_by_rule(c)]
    declining = []
    for c in CASES:
        if releasable_by_rule(c):
            declining += [(c["id"], v["label"]) for v in c["variants"] if v["label"] in ("stored", "csr")]
        else:
            declining.append((c["id"], c["variants"][0]["label"]))
    assert RELEASABLE == releasable
    assert DECLINING == declining
    assert all(key in DECLINING for key in UNDO)
    forms = [BY_ID[cid]["variants"][0]["form"] for cid in RELEASABLE]
    reached = lambda k: {f.get(k) for f in forms}
    assert {"class_tail", "split_tail", "own_launch"} <= reached("listed_route")
    assert "stored_planes" not in reached("listed_route")
    assert {2, 3, 5} <= reached("kind")
    assert {1, 2, 3, 4} <= reached("c")
    assert {1, 4, 16} <= reached("class_kernel")
    assert {0, 1, 4, 16} <= reached("regular_kernel")
    assert {0, 1} <= reached("float_planes")
    assert [cid for cid in RELEASABLE if BY_ID[cid]["transpose"]] == ["nodecls_transposed"]
    tails = {f["listed"] for f in forms if isinstance(f.get("listed"), int) and f.get("listed_route") in ("class_tail", "split_tail")}
    assert {1, 3, 4, 5, 16, 17, 33} <= tails
    assert any(BY_ID[cid]["args"].get("empty_lead") for cid in RELEASABLE)
    # the cases the other tests of this file name
    assert {"inv_r1_c1", "shell_perturbed_c1", "layer2_r1", "own_r1_c1", "nodecls_tail16_33", "inv_r1_c2", "nodecls_tail4_5"} <= set(RELEASABLE)
    assert BY_ID["inv_r1_c1"]["variants"][0]["form"]["listed_route"] == "class_tail" and BY_ID["inv_r1_c1"]["variants"][0]["form"]["kind"] == 3
    assert BY_ID["shell_perturbed_c1"]["variants"][0]["form"]["listed_route"] == "own_launch"
    assert BY_ID["layer2_r1"]["variants"][0]["form"]["kind"] == 5 and BY_ID["layer2_r1"]["gen"] == "stencil"      # (square: it has a diagonal)


def test_the_limit_shapes_perturb_interior_nodes_only():
    """(what the expectation listed == perturb + 8 rests on, at a reduced size: every perturbed node and every corner has a
    stencil of its own, every other stencil repeats at least 8 times -- the shortest edge has 8 inner nodes)"""
    A = stencil_matrix(dims=(10, 10, 10), perturb=40, seed=81)
    assert len(listed_rows(A)) == 40 + 8
    assert len(listed_rows(stencil_matrix(dims=(10, 10, 9), perturb=40, seed=81))) == 40 + 8 + 4 * 7


def listed_rows(A):
    """The rows of a one-component matrix of the generators that no class takes: those whose (offsets, values) fewer than 8
    rows share (kMinClass of the class search)."""
    seen = {}
    square = A.shape[0] == A.shape[1]
    for r in range(A.shape[0]):
        s, e = A.indptr[r], A.indptr[r + 1]
        key = ((A.indices[s:e] - (r if square else A.indices[s])).tobytes(), A.data[s:e].tobytes())
        seen.setdefault(key, []).append(r)
    return sorted(r for v in seen.values() if len(v) < 8 for r in v)


# ---- on the GPU -----------------------------------------------------------------------------------------------------
def build(ctx, monkeypatch, c):
    """(base, the matrix under test, its scipy twin): under the environment of the case; transpose() of it where the case
    says so."""
    for k, val in c["env"].items():
        monkeypatch.setenv(k, val)
    A = GENERATORS[c["gen"]](**c["args"])
    base = M.SparseMatrixDevice(ctx, A)
    Ad = base
    if c["transpose"]:
        Ad = base.transpose()
        A = A.T.tocsr()
        A.sort_indices()
    return base, Ad, A


def all_launches(ctx, c, A, Ad, v):
    """{key: out} of every launch of the case: mode x (alpha, beta), at the 8-byte offset as well where C = 2, and the two
    boundary-shell vectors in mode 0."""
    out = {}
    f = Ad.form()
    for mode in modes_of(A):
        for al, be in sorted({ALPHA_BETA[mode], ALPHA_BETA_2.get(mode, ALPHA_BETA[mode])}):
            out[(mode, al, be, 0, None)] = launch(Ad, ctx, mode, v, al, be)
            assert Ad.form()["pairs"] == 1
            if f["c"] == 2:
                out[(mode, al, be, 1, None)] = launch(Ad, ctx, mode, v, al, be, offset=1)
                assert Ad.form()["pairs"] == 0
    if c["shell"] is not None:
        for j, xs in enumerate(shell_vectors(c, A)):
            out[(L.CSR_APPLY, 0.0, 0.0, 0, j)] = launch(Ad, ctx, L.CSR_APPLY, v, 0.0, 0.0, x=xs)
    return out


def same_form(f0, f1, released):
    assert f1["csr_released"] == released
    assert {k: w for k, w in f1.items() if k not in ("csr_released", "pairs")} == {k: w for k, w in f0.items() if k not in ("csr_released", "pairs")}


def block_rows_have_the_bits_of_launch(ctx, where, A, Ad, v):
    """launch_block with 3 rows on a released matrix: width 1, no block launch, the rows of launch(), guards intact."""
    k = 3
    m, n = A.shape
    rng = np.random.default_rng(5)
    scale = lambda a, j: a * (1.0 + 0.5 * j)
    X, B, XP, O0 = (np.stack([scale(v[name], j) for j in range(k)]) for name in ("x", "b", "xp", "out0"))
    X[1:] += rng.standard_normal((k - 1, n))
    dinv = torch.from_numpy(v["dinv"]).cuda()
    ld_x, ld_out = n + 4 + (n & 1), m + 2 + (m & 1)
    assert Ad.block_info()["width"] == 1
    for mode in modes_of(A):
        al, be = ALPHA_BETA[mode]
        need_b, need_d, need_p, reads_out = (o is not None for o in operands(mode, v))
        ref = []
        for c in range(k):
            o = torch.from_numpy(O0[c]).cuda() if reads_out else torch.full((m,), np.nan, dtype=torch.float64, device="cuda")
            Ad.launch(mode, torch.from_numpy(X[c]).cuda(), o, b=torch.from_numpy(B[c]).cuda() if need_b else None,
                      dinv=dinv if need_d else None, x_prev=torch.from_numpy(XP[c]).cuda() if need_p else None, alpha=al, beta=be)
            ref.append(o)
        ctx.synchronize()
        xbuf, xb = guarded(X, ld_x)
        bbuf, bb = guarded(B, ld_out)
        pbuf, pb = guarded(XP, ld_out)
        obuf, ob = guarded(O0 if reads_out else np.full((k, m), np.nan), ld_out)
        x0, b0, p0 = xbuf.clone(), bbuf.clone(), pbuf.clone()
        before = Ad.block_info()
        Ad.launch_block(mode, xb, ob, B=bb if need_b else None, dinv=dinv if need_d else None, X_prev=pb if need_p else None,
                        alpha=al, beta=be)
        ctx.synchronize()
        after = Ad.block_info()
        assert after["width"] == 1 and after["block_launches"] == before["block_launches"], (where, mode, before, after)
        assert after["column_launches"] == before["column_launches"] + k, (where, mode, before, after)
        for c in range(k):
            assert bool(torch.isfinite(ref[c]).all()), f"{where}: launch_block mode {mode}: row {c} of the reference is not finite"
            assert torch.equal(ob[c, :m], ref[c]), f"{where}: launch_block mode {mode}: row {c} differs from launch() on that row"
        assert guards_intact(obuf, k, m), f"{where}: launch_block mode {mode}: a guard row or a tail of out was written"
        for name, buf, was in (("X", xbuf, x0), ("B", bbuf, b0), ("X_prev", pbuf, p0)):
            assert torch.equal(buf.view(torch.int64), was.view(torch.int64)), f"{where}: launch_block mode {mode}: {name} was changed"


def release_and_compare(ctx, c, A, Ad, where):
    """Section (c) from the launches before the release on; returns the outputs kept from before."""
    v = make_inputs(A, seed_of(c))
    before = all_launches(ctx, c, A, Ad, v)
    for key, out in before.items():
        assert bool(torch.isfinite(out).all()), f"{where}: {key}: entries left unwritten or not finite before the release"
    f0 = Ad.form()
    assert Ad.release_csr() is True, f"{where}: release_csr() declined; form {f0}"
    same_form(f0, Ad.form(), 1)
    after = all_launches(ctx, c, A, Ad, v)
    again = all_launches(ctx, c, A, Ad, v)
    assert before.keys() == after.keys()
    for key, out in after.items():
        mode, al, be, offset, shell = key
        assert torch.equal(out, before[key]), (f"{where}: mode {mode}, alpha {al}, beta {be}, offset {offset}, shell {shell}: "
                                               f"{(out != before[key]).sum().item()} entries differ from the launch before the release")
        assert torch.equal(out, again[key]), f"{where}: {key}: a repeated launch on the released matrix changed bits"
        if offset == 0:
            x = v["x"] if shell is None else shell_vectors(c, A)[shell]
            b, d, xp, o0 = operands(mode, v)
            ref, bound = reference(A, mode, x, b, d, xp, al, be, o0)
            assert_within(out.cpu().numpy(), ref, bound, f"{where}, released: mode {mode}, alpha {al}, beta {be}, shell {shell}")
    f1 = Ad.form()
    assert Ad.release_csr() is True
    assert Ad.form() == f1
    key = (L.CSR_RESIDUAL, 0.0, 0.0, 0, None)
    assert torch.equal(launch(Ad, ctx, L.CSR_RESIDUAL, v, 0.0, 0.0), before[key]), f"{where}: a second release_csr() changed the launch"
    block_rows_have_the_bits_of_launch(ctx, where, A, Ad, v)
    return v, before


@pytest.mark.gpu
@pytest.mark.parametrize("cid", RELEASABLE)
def test_released_layout(ctx, monkeypatch, cid):
    c = BY_ID[cid]
    base, Ad, A = build(ctx, monkeypatch, c)
    f = Ad.form()
    print(f"{cid}: {A.shape[0]} x {A.shape[1]}, {A.nnz} entries, form {f}")
    check_form(f, c["variants"][0]["form"], cid)
    assert f["regular"] == 1 and f["listed_route"] != "stored_planes" and f["csr_released"] == 0
    release_and_compare(ctx, c, A, Ad, cid)


@pytest.mark.gpu
def test_released_matrix_without_a_listed_row(ctx, monkeypatch):
    """The kept arrays are one element long and no tail workgroup is launched."""
    c = own_case("no_listed_row", NO_LISTED)
    assert c["args"] == dict(dims=(17, 16, 16), perturb=0)
    A = prolongator_matrix(**c["args"])
    Ad = M.SparseMatrixDevice(ctx, A)
    f = Ad.form()
    check_form(f, dict(kind=5, regular=1, listed=0, listed_route=None), c["id"])
    release_and_compare(ctx, c, A, Ad, c["id"])


@pytest.mark.gpu
def test_the_two_sides_of_the_listed_row_limit(ctx, monkeypatch):
    """32768 listed rows: each a wavefront behind the class launch, and the matrix lets go of its arrays.  32769: rows of the
    stored planes, whose walk reads no CSR array but whose listed rows would have to be kept whole -- release_csr() declines
    and everything still works."""
    c = own_case("listed_32768", AT_LIMIT)
    A = stencil_matrix(**c["args"])
    assert A.shape[0] == 92160
    Ad = M.SparseMatrixDevice(ctx, A)
    f = Ad.form()
    assert f["listed"] == c["args"]["perturb"] + 8 == LIMIT, f
    check_form(f, dict(kind=3, c=1, regular=1, class_kernel=1, listed_route="class_tail", stored_kernel=None), c["id"])
    release_and_compare(ctx, c, A, Ad, c["id"])

    c = own_case("listed_32769", OVER_LIMIT)
    A = stencil_matrix(**c["args"])
    Ad = M.SparseMatrixDevice(ctx, A)
    f = Ad.form()
    assert f["listed"] == c["args"]["perturb"] + 8 == LIMIT + 1, f
    check_form(f, dict(kind=3, c=1, regular=1, class_kernel=1, listed_route="stored_planes", stored_kernel="sym_rows"), c["id"])
    declines(ctx, c, A, Ad, c["id"])


def library_gb():
    return float(M.memory_inventory().strip().splitlines()[-1].split()[0])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["inv_r1_c1", "own_r1_c1", "nodecls_tail16_33", "listed_32768"])
def test_release_frees_the_csr_arrays(ctx, monkeypatch, cid):
    """The ledger of the library's device buffers (the last line of memory_inventory(), GB with three decimals) drops by the CSR
    arrays, 12 B per entry and 4 B per row pointer, less the packed copy of the listed rows, 12 B per kept entry (one at
    least) and 4 B per pointer.  Both readings are rounded to 0.0005 GB: the difference to 0.001 GB, and twice that is
    allowed.  Nothing else the ledger counts changes: the lengths of the listed rows travel through a buffer that is freed
    before release_csr() returns, and the host copy that goes as well is no device buffer."""
    c = own_case(cid, AT_LIMIT) if cid == "listed_32768" else BY_ID[cid]
    base, Ad, A = build(ctx, monkeypatch, c)
    f = Ad.form()
    assert f["c"] == 1
    listed = listed_rows(A)
    assert len(listed) == f["listed"], (len(listed), f)
    kept = int(np.diff(A.indptr)[listed].sum())
    ctx.synchronize()
    before = library_gb()
    assert Ad.release_csr() is True
    after = library_gb()
    freed = 12 * A.nnz + 4 * (A.shape[0] + 1)
    added = 12 * max(kept, 1) + 4 * (len(listed) + 1)
    print(f"{cid}: {A.nnz} entries, {len(listed)} listed rows of {kept} entries: ledger {before:.3f} -> {after:.3f} GB, "
          f"expected drop {(freed - added) * 1e-9:.6f} GB")
    assert abs((before - after) - (freed - added) * 1e-9) <= 0.002


def throws_released(call):
    with pytest.raises(L.MfmgError, match="released"):
        call()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["inv_r1_c1", "shell_perturbed_c1", "layer2_r1"])
def test_released_matrix_refuses_what_reads_its_arrays(ctx, monkeypatch, cid):
    """Kind 3 with classes, kind 3 with a launch of the listed rows, kind 5 (a square one: it has a diagonal).  Every export,
    the setup algebra on either side, the diagonal kernel, a transposed application that was never built and every change of
    kernel that would read the arrays throw; after each call, refused or accepted, the launch has the bits it had.

    solve() with lu_dense throws as well, but not for the release: HipSolver refuses a matrix above solver.dense_limit
    (8192 rows, 16384 at the most) before setup_direct downloads anything, and no table-driven matrix has fewer than 32768
    rows.  The message says "too large"; with pcg the solver asks for the inverse diagonal first and the release is named."""
    c = BY_ID[cid]
    base, Ad, A = build(ctx, monkeypatch, c)
    m = A.shape[0]
    assert m == A.shape[1] and m >= 32768
    v = make_inputs(A, seed_of(c))
    kept = launch(Ad, ctx, L.CSR_RESIDUAL, v, 0.0, 0.0)
    assert Ad.release_csr() is True
    eye = M.SparseMatrixDevice(ctx, sp.identity(m, format="csr"))
    vec = lambda: torch.zeros(m, dtype=torch.float64, device="cuda")

    def still_the_same(what):
        assert torch.equal(launch(Ad, ctx, L.CSR_RESIDUAL, v, 0.0, 0.0), kept), f"{cid}: the launch changed after {what}"
        assert Ad.form()["csr_released"] == 1

    for what, call in (("to_scipy", Ad.to_scipy), ("transpose", Ad.transpose), ("multiply, left", lambda: Ad.multiply(eye)),
                       ("multiply, right", lambda: eye.multiply(Ad)), ("inverse_diagonal", lambda: Ad.inverse_diagonal(vec())),
                       ("apply TRANS", lambda: Ad.apply(vec(), vec(), L.TRANS)),
                       ("solve pcg", lambda: Ad.solve({"solver": {"type": "pcg"}}, vec(), vec()))):
        throws_released(call)
        still_the_same(what)
    with pytest.raises(L.MfmgError, match="too large for the dense direct solver"):
        Ad.solve({"solver": {"type": "lu_dense"}}, vec(), vec())
    still_the_same("solve lu_dense")
    for k in range(6):
        with pytest.raises(L.MfmgError, match="kernel is fixed"):
            Ad.set_kernel(0, k)
        still_the_same(f"set_kernel(0, {k})")
    with pytest.raises(L.MfmgError, match="kernel is fixed"):
        Ad.set_regular_rows(False)
    still_the_same("set_regular_rows(False)")
    f = Ad.form()
    Ad.set_kernel(8, -1)
    still_the_same("set_kernel(8, -1)")
    Ad.set_regular_rows(True)
    still_the_same("set_regular_rows(True)")
    assert {k: w for k, w in Ad.form().items() if k != "pairs"} == {k: w for k, w in f.items() if k != "pairs"}
    # the operands of the products were not released and still export
    assert abs(eye.to_scipy() - sp.identity(m)).max() == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["inv_r1_c2_nonsym", "nodecls_tail4_5"])
def test_a_transpose_built_before_the_release_keeps_working(ctx, monkeypatch, cid):
    """apply(.., TRANS) builds the transposed matrix once and keeps it: an object that applied it before release_csr() applies
    the cached one afterwards, with the bits from before (a non-symmetric square matrix and a rectangular one)."""
    c = BY_ID[cid]
    base, Ad, A = build(ctx, monkeypatch, c)
    m, n = A.shape
    rng = np.random.default_rng(3)
    xt = torch.from_numpy(rng.standard_normal(m)).cuda()
    y0 = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    Ad.apply(xt, y0, L.TRANS)
    ctx.synchronize()
    At = A.T.tocsr()
    At.sort_indices()
    ref, bound = reference(At, L.CSR_APPLY, xt.cpu().numpy(), None, None, None, 0.0, 0.0, None)
    assert_within(y0.cpu().numpy(), ref, bound, f"{cid}: apply(TRANS) before the release")
    assert Ad.release_csr() is True
    y1 = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    Ad.apply(xt, y1, L.TRANS)
    ctx.synchronize()
    assert torch.equal(y0, y1)
    # (transpose() hands out that cached matrix, which owns arrays of its own: it still exports, the released one does not)
    got = Ad.transpose().to_scipy()
    assert np.array_equal(got.indptr, At.indptr) and np.array_equal(got.indices, At.indices) and np.array_equal(got.data, At.data)
    throws_released(Ad.to_scipy)


def declines(ctx, c, A, Ad, where):
    """Section (e): release_csr() is False and leaves the matrix as it was."""
    v = make_inputs(A, seed_of(c))
    f0 = Ad.form()
    assert f0["csr_released"] == 0
    before = {mode: launch(Ad, ctx, mode, v, *ALPHA_BETA[mode]) for mode in modes_of(A)}
    f0 = Ad.form()
    assert Ad.release_csr() is False, f"{where}: release_csr() let go of arrays the kernels read; form {f0}"
    assert Ad.form() == f0
    got = Ad.to_scipy()
    assert got.shape == A.shape and np.array_equal(got.indptr, A.indptr) and np.array_equal(got.indices, A.indices)
    assert np.array_equal(got.data, A.data)
    for mode in modes_of(A):
        assert torch.equal(launch(Ad, ctx, mode, v, *ALPHA_BETA[mode]), before[mode]), f"{where}: mode {mode} changed after the refused release"
    assert Ad.form() == f0


@pytest.mark.gpu
@pytest.mark.parametrize("cid,label", DECLINING, ids=[f"{c}-{l}" for c, l in DECLINING])
def test_declining_layout(ctx, monkeypatch, cid, label):
    c = BY_ID[cid]
    base, Ad, A = build(ctx, monkeypatch, c)
    for var in c["variants"]:               # (the operations of the variants in front of the wanted one apply as well)
        for op in var["ops"]:
            getattr(Ad, op[0])(*op[1:])
        if var["label"] == label:
            break
    assert var["label"] == label
    where = f"{cid}/{label}"
    check_form(Ad.form(), var["form"], where)
    declines(ctx, c, A, Ad, where)
    if (cid, label) in UNDO:
        op = UNDO[(cid, label)]
        getattr(Ad, op[0])(*op[1:])
        check_form(Ad.form(), c["variants"][0]["form"], where + ", switched back")
        release_and_compare(ctx, c, A, Ad, where + ", switched back")
