"""SparseMatrixDevice.launch_block: the SpMV with its fused epilogues on a block of vectors (sparse_matrix_block.hip).

The contract is bits: row c of launch_block is torch.equal to launch() on that row's vectors, for every mode the matrix
admits and k = 1, 2, 3, 4, 7 rows (one vector; a group of 2; 2 + 1; a group of 4; 4 + 2 + 1).  The reference is the
one-vector launch of the same matrix, which test_spmv_layouts.py holds to long double -- so nothing here needs a tolerance.

Cases: the matrices of test_spmv_layouts.py whose launch is exactly one kernel over stored values that do not repeat --
planes_* (bdia_sym_split_kernel and bdia_spmv_kernel, 1..4 unknowns per node, double and float planes), row_base, and the
`stored` variant of chain_* and slots_* (row counts on either side of a multiple of 256).  There block_info()["width"] is 4,
the groups of 4 and 2 are one launch each of the block kernels (counted by the matrix and by the profiler under
csr_block_kernel) and only the odd last row goes through the one-vector kernel.  A table-driven and a CSR matrix have the
width 1: the same bits from the loop, no block launch.

Blocks are laid out with room to notice a stray store: a guard row in front of and behind the k rows and a tail behind the
m entries of every row, all filled with one NaN payload that must still be there afterwards; the leading dimensions of X and
out differ (the matrix may be rectangular); B and X must come back unchanged."""
import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
from mfmg_amd.api import block_groups
from test_spmv_layouts import ALPHA_BETA, BY_ID, GENERATORS, check_form, modes_of, scaled_normal, seed_of

KS = (1, 2, 3, 4, 7)
K_MAX = max(KS)
PAYLOAD = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.int64)[0]

BLOCK_CASES = ([(f"planes_{n}", "stored") for n in ("sym_c1", "sym_c1_f32", "nonsym_c2", "nonsym_c2_f32", "sym_c3_f32", "nonsym_c4")]
               + [("row_base", "row_base")] + [(f"chain_{n}", "stored") for n in (64 * 129 - 1, 64 * 129, 64 * 129 + 1)]
               + [(f"slots_{n}", "stored") for n in (834, 835, 851)])
LOOP_CASES = [("inv_r1_c2", "tables"), ("planes_sym_c1", "csr")]


def wide_groups(k):
    return sum(1 for w in block_groups(k) if w > 1)


def test_the_groups_of_the_row_counts():
    assert [wide_groups(k) for k in KS] == [0, 1, 1, 1, 2] and [block_groups(k).count(1) for k in KS] == [k % 2 for k in KS]


def payload_block(rows, ld):
    t = torch.empty((rows, ld), dtype=torch.float64, device="cuda")
    t.view(torch.int64).fill_(int(PAYLOAD))
    return t


def guarded(values, ld):
    """(buffer, block): the rows of `values` as the rows 1..k of a payload-filled buffer with the leading dimension ld."""
    k, m = values.shape
    assert ld % 2 == 0 and ld > m
    buf = payload_block(k + 2, ld)
    blk = buf[1:k + 1]
    blk[:, :m].copy_(torch.from_numpy(values))
    assert blk.data_ptr() % 16 == 0 and blk.stride(0) == ld
    return buf, blk


def guards_intact(buf, k, m):
    bits = buf.view(torch.int64)
    return bool((bits[0] == int(PAYLOAD)).all() and (bits[k + 1] == int(PAYLOAD)).all() and (bits[1:k + 1, m:] == int(PAYLOAD)).all())


def matrix_of(cid, label):
    c = BY_ID[cid]
    (var,) = [v for v in c["variants"] if v["label"] == label]
    return c, var, GENERATORS[c["gen"]](**c["args"])


def prepare(ctx, cid, label):
    c, var, A = matrix_of(cid, label)
    assert not c["env"] and not c["transpose"]
    Ad = M.SparseMatrixDevice(ctx, A)
    for v in c["variants"]:               # (the operations of the variants in front of the wanted one apply as well)
        for op in v["ops"]:
            getattr(Ad, op[0])(*op[1:])
        if v is var:
            break
    f = Ad.form()
    check_form(f, var["form"], f"{cid}/{label}")
    return c, A, Ad, f


def block_against_columns(ctx, cid, A, Ad, width):
    """Every mode and k: bits, guards, inputs, counters.  Returns (block launches, column launches) seen in all."""
    m, n = A.shape
    rng = np.random.default_rng(seed_of(BY_ID[cid]) + 1000)
    X, B, XP, O0 = (np.stack([scaled_normal(rng, sz) for _ in range(K_MAX)]) for sz in (n, m, m, m))
    d = A.diagonal() if m == n else None
    dinv = torch.from_numpy(np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 0.0) if m == n else scaled_normal(rng, m)).cuda()
    ld_x, ld_out = n + 4 + (n & 1), m + 2 + (m & 1)
    assert ld_x != ld_out
    total = [0, 0]
    ctx.profile_enable(True, "csr_block_kernel")
    try:
        for mode in modes_of(A):
            al, be = ALPHA_BETA[mode]
            need_b = mode in (L.CSR_RESIDUAL, L.CSR_FIRST, L.CSR_NEXT, L.CSR_PLUS_SCALED)
            need_d = mode in (L.CSR_FIRST, L.CSR_NEXT, L.CSR_PLUS_SCALED)
            need_p = mode == L.CSR_NEXT
            reads_out = mode in (L.CSR_SUBTRACT, L.CSR_ADD)
            # the one-vector launches, once per column
            ref = []
            for c in range(K_MAX):
                o = torch.from_numpy(O0[c]).cuda() if reads_out else torch.full((m,), np.nan, dtype=torch.float64, device="cuda")
                Ad.launch(mode, torch.from_numpy(X[c]).cuda(), o, b=torch.from_numpy(B[c]).cuda() if need_b else None,
                          dinv=dinv if need_d else None, x_prev=torch.from_numpy(XP[c]).cuda() if need_p else None, alpha=al, beta=be)
                ref.append(o)
            ctx.synchronize()
            assert all(bool(torch.isfinite(o).all()) for o in ref)
            for k in KS:
                xbuf, xb = guarded(X[:k], ld_x)
                bbuf, bb = guarded(B[:k], ld_out)
                pbuf, pb = guarded(XP[:k], ld_out)
                obuf, ob = guarded(O0[:k] if reads_out else np.full((k, m), np.nan), ld_out)
                if not reads_out:
                    ob[:, :m].view(torch.int64).fill_(int(PAYLOAD))
                x0, b0, p0 = xbuf.clone(), bbuf.clone(), pbuf.clone()
                before, prof = Ad.block_info(), ctx.profile_query("csr_block_kernel")[0]
                Ad.launch_block(mode, xb, ob, B=bb if need_b else None, dinv=dinv if need_d else None, X_prev=pb if need_p else None,
                                alpha=al, beta=be)
                ctx.synchronize()
                after = Ad.block_info()
                where = f"{cid}: mode {mode}, k {k}"
                for c in range(k):
                    assert torch.equal(ob[c, :m], ref[c]), f"{where}: row {c} differs from launch() on that row"
                assert guards_intact(obuf, k, m), f"{where}: a guard row or a tail of out was written"
                for name, buf, was in (("X", xbuf, x0), ("B", bbuf, b0), ("X_prev", pbuf, p0)):
                    assert torch.equal(buf.view(torch.int64), was.view(torch.int64)), f"{where}: {name} was changed"
                dblock, dcol = after["block_launches"] - before["block_launches"], after["column_launches"] - before["column_launches"]
                assert after["width"] == width
                if width == 4:
                    assert dblock == wide_groups(k) and dcol == k % 2, (where, dblock, dcol)
                else:
                    assert dblock == 0 and dcol == k, (where, dblock, dcol)
                assert ctx.profile_query("csr_block_kernel")[0] - prof == dblock, where
                total[0] += dblock
                total[1] += dcol
    finally:
        ctx.profile_enable(False)
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("cid,label", BLOCK_CASES, ids=[c for c, _ in BLOCK_CASES])
def test_block_kernels_give_the_bits_of_the_column_launches(ctx, cid, label):
    c, A, Ad, f = prepare(ctx, cid, label)
    assert (f["kind"] in (2, 3) and f["regular"] == 0) or f["kind"] == 4
    assert Ad.block_info()["width"] == 4
    if A.shape[0] != A.shape[1]:
        assert cid == "row_base"
    blocks, columns = block_against_columns(ctx, cid, A, Ad, 4)
    n_modes = len(modes_of(A))
    assert blocks == n_modes * sum(wide_groups(k) for k in KS) and columns == n_modes * sum(k % 2 for k in KS)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,label", LOOP_CASES, ids=[f"{c}-{l}" for c, l in LOOP_CASES])
def test_matrices_without_the_block_kernels_loop(ctx, cid, label):
    c, A, Ad, f = prepare(ctx, cid, label)
    assert f["regular"] == 1 or f["kind"] == 0
    assert Ad.block_info()["width"] == 1
    blocks, columns = block_against_columns(ctx, cid, A, Ad, 1)
    assert blocks == 0 and columns == len(modes_of(A)) * sum(KS)


@pytest.mark.gpu
def test_launch_block_refusals(ctx):
    c, A, Ad, f = prepare(ctx, f"chain_{64 * 129}", "stored")         # (the smallest matrix of the table with the block kernels)
    m = A.shape[0]
    assert Ad.block_info()["width"] == 4
    ld = m + 2 + (m & 1)
    pool = torch.ones(66 * ld + 8, dtype=torch.float64, device="cuda")
    other = torch.ones(66 * ld + 8, dtype=torch.float64, device="cuda")
    assert pool.data_ptr() % 16 == 0 and other.data_ptr() % 16 == 0
    blk = lambda buf, k, stride, offset=0: torch.as_strided(buf, (k, m), (stride, 1), offset)
    dinv = torch.ones(m, dtype=torch.float64, device="cuda")
    before = Ad.block_info()
    bad = L.MfmgInvalidArgument
    with pytest.raises(bad):                                            # no vector at all
        Ad.launch_block(L.CSR_APPLY, blk(pool, 0, ld), blk(other, 0, ld))
    with pytest.raises(bad, match="1 to 64"):
        Ad.launch_block(L.CSR_APPLY, blk(pool, 65, ld), blk(other, 65, ld))
    with pytest.raises(bad, match="at least the vector size"):
        Ad.launch_block(L.CSR_APPLY, blk(pool, 2, m - 2 + (m & 1)), blk(other, 2, ld))
    with pytest.raises(bad, match="at least the vector size"):
        Ad.launch_block(L.CSR_APPLY, blk(pool, 2, ld), blk(other, 2, m - 2 + (m & 1)))
    with pytest.raises(bad, match="even"):
        Ad.launch_block(L.CSR_APPLY, blk(pool, 2, ld + 1), blk(other, 2, ld))
    with pytest.raises(bad, match="even"):
        Ad.launch_block(L.CSR_APPLY, blk(pool, 2, ld), blk(other, 2, ld + 1))
    with pytest.raises(bad, match="aligned to 16 bytes"):
        Ad.launch_block(L.CSR_APPLY, blk(pool, 2, ld, 1), blk(other, 2, ld))
    with pytest.raises(bad, match="aligned to 16 bytes"):
        Ad.launch_block(L.CSR_APPLY, blk(pool, 2, ld), blk(other, 2, ld, 1))
    with pytest.raises(bad, match="aligned to 16 bytes"):
        Ad.launch_block(L.CSR_RESIDUAL, blk(pool, 2, ld), blk(other, 2, ld, 4 * ld), B=blk(other, 2, ld, 1))
    with pytest.raises(bad, match="overlap"):                           # out is x, and out begins inside the last row of x
        Ad.launch_block(L.CSR_APPLY, blk(pool, 2, ld), blk(pool, 2, ld))
    with pytest.raises(bad, match="overlap"):
        Ad.launch_block(L.CSR_APPLY, blk(pool, 2, ld), blk(pool, 2, ld, ld + 2))
    with pytest.raises(bad, match="needs b"):
        Ad.launch_block(L.CSR_RESIDUAL, blk(pool, 2, ld), blk(other, 2, ld))
    with pytest.raises(bad, match="inverse diagonal"):
        Ad.launch_block(L.CSR_PLUS_SCALED, blk(pool, 2, ld), blk(other, 2, ld), B=blk(other, 2, ld, 4 * ld))
    with pytest.raises(bad, match="x_prev"):
        Ad.launch_block(L.CSR_NEXT, blk(pool, 2, ld), blk(other, 2, ld), B=blk(other, 2, ld, 4 * ld), dinv=dinv)
    with pytest.raises(bad, match="unknown SpMV mode"):
        Ad.launch_block(7, blk(pool, 2, ld), blk(other, 2, ld))
    with pytest.raises(ValueError):                                     # (the wrapper: B at another distance than out)
        Ad.launch_block(L.CSR_RESIDUAL, blk(pool, 2, ld), blk(other, 2, ld), B=blk(other, 2, ld + 2, 4 * ld))
    assert Ad.block_info() == before                                    # nothing was launched
    Ad.launch_block(L.CSR_APPLY, blk(pool, 2, ld), blk(other, 2, ld))   # (and the accepted call right next to them)
    ctx.synchronize()
    assert Ad.block_info()["block_launches"] == before["block_launches"] + 1
