"""The block forms of the CSR kernels (sparse_matrix_block_csr.hip) behind SparseMatrixDevice.set_block_csr.

The contract is bits: row c of launch_block is torch.equal to launch() on that row's vectors, for every mode the matrix admits
and k = 1, 2, 3, 4, 7 rows -- block_against_columns of test_gpu_csr_block.py, which also holds the NaN-payload guard rows and
tails, the inputs, the counters (block launches == wide groups, column launches == k % 2) and the profiler count under
csr_block_kernel.  The reference is the one-vector launch, which test_spmv_layouts.py holds to long double: no tolerance here.

The switch is off by default: every case first sees the width 1, then set_block_csr(True) must report 4 and the routes -- the
kernel form() names, except that a group of an LDS-cached matrix whose nv windows of x (the most distinct columns of a 128-row
block, 8 bytes each) with the 1040 bytes of the row-pointer table pass 80 KiB takes the lanes kernel --, and set_block_csr(False)
the width 1 and the counters of the loop again.

Cases, from the table of test_spmv_layouts.py: `ragged` on all seven lanes and all seven LDS variants (32 769 rows; rows of 0,
1, 63, 64, 65 entries at the start, middle and end of a 128-row block; a last block of one row: the edges of the batch tail,
the shuffle ladder and the LDS staging), `long_rows` (a workgroup per row; an empty and a one-entry row), `thinned_lds`,
`row_base_transposed` (rectangular, ld_x != ld_out) and `planes_sym_c1` forced to CSR.  A matrix generated here has a window
that fits LDS twice but not four times."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
from mfmg_amd.api import block_csr_info_f32
from test_gpu_csr_block import PAYLOAD, block_against_columns, guarded, guards_intact, wide_groups
from test_gpu_csr_block import KS as BLOCK_KS
from test_spmv_layouts import ALPHA_BETA, BY_ID, GENERATORS, LANES, check_form, modes_of, scaled_normal, seed_of

pytestmark = pytest.mark.gpu

LDS_BUDGET, RP_TABLE = 80 * 1024, 1040
CASES = ([("ragged", f"lanes{l}") for l in LANES] + [("ragged", f"lds{l}") for l in LANES]
         + [("long_rows", "row_block"), ("long_rows", "lanes64"), ("thinned_lds", "lds"), ("thinned_lds", "csr"),
            ("row_base_transposed", "transpose"), ("planes_sym_c1", "csr")])


@functools.lru_cache(maxsize=None)
def host_matrix(cid):
    c = BY_ID[cid]
    A = GENERATORS[c["gen"]](**c["args"])
    if c["transpose"]:
        A = A.T.tocsr()
        A.sort_indices()
    return A


def prepare(ctx, cid, label):
    """(A, device matrix, form, keepalive) of a variant of a case; the operations of the variants in front of it apply too."""
    c = BY_ID[cid]
    assert not c["env"]
    base = M.SparseMatrixDevice(ctx, GENERATORS[c["gen"]](**c["args"]) if c["transpose"] else host_matrix(cid))
    Ad = base.transpose() if c["transpose"] else base
    (var,) = [v for v in c["variants"] if v["label"] == label]
    for v in c["variants"]:
        for op in v["ops"]:
            getattr(Ad, op[0])(*op[1:])
        if v is var:
            break
    f = Ad.form()
    check_form(f, var["form"], f"{cid}/{label}")
    return host_matrix(cid), Ad, f, base


def window_of(A):
    """The most distinct columns a block of 128 rows touches: the entries of one window of x in the LDS form."""
    ptr, col = A.indptr, A.indices
    return max(len(np.unique(col[ptr[r0]:ptr[min(r0 + 128, A.shape[0])]])) for r0 in range(0, A.shape[0], 128))


def routes_of(A, f):
    """(route4, route2) by the rule of the issue: one launch per group, the LDS form where nv windows leave two workgroups per CU."""
    if f["csr_kernel"] != "lds":
        return f["csr_kernel"], f["csr_kernel"]
    w = window_of(A)
    return tuple("lds" if nv * w * 8 + RP_TABLE <= LDS_BUDGET else "lanes" for nv in (4, 2))


def loop_again(ctx, A, Ad):
    """One apply of four rows with the switch off: the bits of launch(), no block launch, four column launches."""
    m, n = A.shape
    rng = np.random.default_rng(5)
    X = np.stack([scaled_normal(rng, n) for _ in range(4)])
    ld_x, ld_out = n + 4 + (n & 1), m + 2 + (m & 1)
    xbuf, xb = guarded(X, ld_x)
    obuf, ob = guarded(np.full((4, m), np.nan), ld_out)
    before = Ad.block_info()
    Ad.launch_block(L.CSR_APPLY, xb, ob)
    ctx.synchronize()
    after = Ad.block_info()
    assert after["width"] == 1 and after["block_launches"] == before["block_launches"] and after["column_launches"] == before["column_launches"] + 4
    for c in range(4):
        o = torch.full((m,), np.nan, dtype=torch.float64, device="cuda")
        Ad.launch(L.CSR_APPLY, torch.from_numpy(X[c]).cuda(), o)
        assert torch.equal(ob[c, :m], o)
    assert guards_intact(obuf, 4, m)


def switch_and_check(ctx, cid, A, Ad, f, want_routes):
    assert f["kind"] in (0, 1) and f["csr_kernel"] in ("lanes", "row_block", "lds")
    assert Ad.block_info()["width"] == 1                                 # off by default
    info = Ad.set_block_csr(True)
    assert info == {"width": 4, "route4": want_routes[0], "route2": want_routes[1]}, (cid, info)
    assert Ad.block_info()["width"] == 4
    blocks, columns = block_against_columns(ctx, cid, A, Ad, 4)
    n_modes = len(modes_of(A))
    assert blocks == n_modes * sum(wide_groups(k) for k in BLOCK_KS) and columns == n_modes * sum(k % 2 for k in BLOCK_KS)
    assert Ad.form() == {**f, "pairs": Ad.form()["pairs"]}               # (the switch changes no field of form())
    info = Ad.set_block_csr(False)
    assert info == {"width": 1, "route4": None, "route2": None}, (cid, info)
    loop_again(ctx, A, Ad)


@pytest.mark.parametrize("cid,label", CASES, ids=[f"{c}-{l}" for c, l in CASES])
def test_csr_block_kernels_give_the_bits_of_the_column_launches(ctx, cid, label):
    A, Ad, f, keep = prepare(ctx, cid, label)
    if cid == "row_base_transposed":
        assert A.shape[0] != A.shape[1] and f["lanes"] == 16
    want = routes_of(A, f)
    if cid == "ragged":
        assert want == ((f["csr_kernel"],) * 2) and f["lanes"] == max(int(label.lstrip("lanesd")), 4 if label.startswith("lds") else 1)
    switch_and_check(ctx, cid, A, Ad, f, want)


def wide_window_matrix(n_rows=256 * 128 + 1, per_row=80, width=2900, seed=3):
    """About 80 entries per row drawn from a window of 2900 columns around the row, the diagonal among them: a 128-row block
    touches at most 2900 + 127 distinct columns and holds about 10100 entries, more than three per column."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n_rows), per_row)
    lo = np.clip(np.arange(n_rows) - width // 2, 0, n_rows - width)
    cols = (lo[:, None] + rng.integers(0, width, (n_rows, per_row)))
    cols[:, 0] = np.arange(n_rows)
    A = sp.coo_matrix((rng.standard_normal(rows.size), (rows, cols.ravel())), shape=(n_rows, n_rows)).tocsr()
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def test_a_window_that_fits_twice_but_not_four_times(ctx):
    A = wide_window_matrix()
    w = window_of(A)
    assert 4 * w * 8 + RP_TABLE > LDS_BUDGET >= 2 * w * 8 + RP_TABLE and A.nnz >= 3 * 257 * w, (w, A.nnz)
    assert 64 * 1024 < 4 * w * 8                                         # (four windows would also pass the default limit)
    Ad = M.SparseMatrixDevice(ctx, A)
    f = Ad.form()
    assert f["csr_kernel"] == "lds" and f["kind"] == 1, f
    assert Ad.block_info()["width"] == 1
    info = Ad.set_block_csr(True)
    assert info == {"width": 4, "route4": "lanes", "route2": "lds"}, info
    BY_ID.setdefault("wide_window", {"id": "wide_window"})                # (seed_of reads the id only)
    try:
        blocks, columns = block_against_columns(ctx, "wide_window", A, Ad, 4)
    finally:
        del BY_ID["wide_window"]
    assert blocks == 7 * sum(wide_groups(k) for k in BLOCK_KS) and columns == 7 * sum(k % 2 for k in BLOCK_KS)


@pytest.mark.parametrize("label", ["lanes8", "lds8"])
def test_columns_are_independent(ctx, label):
    """Column 1 of X carries +Inf, -Inf and a NaN at columns that rows reference: every column, column 1 included, has the
    64-bit patterns of its own launch() -- nothing of one column reaches another, and no product with an entry that is not
    there is added."""
    A, Ad, f, keep = prepare(ctx, "ragged", label)
    m = A.shape[0]
    rng = np.random.default_rng(17)
    X, B, XP = (np.stack([scaled_normal(rng, m) for _ in range(4)]) for _ in range(3))
    marked = A.indices[[0, A.nnz // 3, A.nnz // 2, A.nnz - 1]]
    X[1, marked[0]], X[1, marked[1]], X[1, marked[2]], X[1, marked[3]] = np.inf, -np.inf, np.nan, np.inf
    d = A.diagonal()
    dinv = torch.from_numpy(np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 0.0)).cuda()
    assert Ad.set_block_csr(True)["width"] == 4
    ld = m + 4 + (m & 1)
    for mode in (L.CSR_APPLY, L.CSR_NEXT):
        nxt = mode == L.CSR_NEXT
        al, be = ALPHA_BETA[mode]
        xbuf, xb = guarded(X, ld)
        bbuf, bb = guarded(B, ld)
        pbuf, pb = guarded(XP, ld)
        obuf, ob = guarded(np.full((4, m), np.nan), ld)
        ob[:, :m].view(torch.int64).fill_(int(PAYLOAD))
        before = Ad.block_info()["block_launches"]
        Ad.launch_block(mode, xb, ob, B=bb if nxt else None, dinv=dinv if nxt else None, X_prev=pb if nxt else None, alpha=al, beta=be)
        ctx.synchronize()
        assert Ad.block_info()["block_launches"] == before + 1
        for c in range(4):
            o = torch.full((m,), np.nan, dtype=torch.float64, device="cuda")
            Ad.launch(mode, torch.from_numpy(X[c]).cuda(), o, b=torch.from_numpy(B[c]).cuda() if nxt else None, dinv=dinv if nxt else None,
                      x_prev=torch.from_numpy(XP[c]).cuda() if nxt else None, alpha=al, beta=be)
            ctx.synchronize()
            assert torch.equal(ob[c, :m].view(torch.int64), o.view(torch.int64)), f"ragged/{label}: mode {mode}: column {c}"
            assert bool(torch.isfinite(o).all()) == (c != 1)
        assert guards_intact(obuf, 4, m)


@pytest.mark.parametrize("cid,label,width", [("inv_r1_c2", "tables", 1), ("planes_nonsym_c2", "stored", 4)])
def test_matrices_the_switch_does_not_concern(ctx, cid, label, width):
    A, Ad, f, keep = prepare(ctx, cid, label)
    assert f["kind"] in (2, 3)
    before = Ad.block_info()
    assert before["width"] == width
    info = Ad.set_block_csr(True)
    assert info == {"width": width, "route4": None, "route2": None}, info
    assert Ad.block_info() == before
    Ad.set_block_csr(False)
    assert Ad.block_info() == before


def test_a_float_matrix_keeps_the_width_one(ctx):
    A = GENERATORS["long_rows"](n=120, seed=71)
    assert block_csr_info_f32(ctx, A) == {"width": 1, "route4": None, "route2": None}
    Ad = M.SparseMatrixDevice(ctx, A)                                   # (the same arrays in double do flip)
    assert Ad.set_block_csr(True)["width"] == 4
