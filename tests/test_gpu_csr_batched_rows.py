"""The CSR row kernels bit for bit: csr_spmv_kernel, csr_spmv_lds_kernel, csr_spmv_row_block_kernel and listed_row_wave
keep a batch of B entries in flight per lane (lane_row_sum in sparse_matrix_device.hip), which moves requests and must not
move a bit.

The reference for bits is a restatement of the lane order in exact arithmetic, neither an earlier build nor the code
under test: a lane folds fma(val, x, sum) over its entries p0 + lane, p0 + lane + S, .. in order -- the exact fma is
float(Fraction(v) * Fraction(x) + Fraction(s)), correctly rounded --, the S lanes of a row (64 per wavefront) are added by
the xor butterfly 32, 16, .. 1 in float64, and the row-block kernel adds its four wavefronts ((w0 + w1) + w2) + w3.  It
does not know B: the shapes do.  Row lengths sit at the edges of a batched loop (0, 1, S - 1, S, S + 1, B S - 1, B S,
B S + 1, 2 B S + 1: whole batches, a last batch of one entry, a short batch only), the last row of a matrix is a long
one, and the LDS-cached kernel runs blocks whose column lists take 1, 2, 4 and 8 elements per thread to stage, one of them
the short last block.

Modes: apply, residual, subtract and add are one float64 operation on the sum that no compiler can contract: exact
too.  first, next and plus_scaled are held to 2 gamma_k mag against long double, the bound of test_spmv_layouts.py.  out
is pre-filled with NaN where the mode does not read it; a launch with NaN in x at a column that no row references must
leave every output finite (a product formed for an entry that is not there would carry it in); a repeated launch is bit
for bit the same."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
from test_spmv_layouts import ALPHA_BETA, ALPHA_BETA_2, MODES, U, launch, operands, row_sums, scaled_normal, stencil_matrix

B = 4                                      # kRowBatch of sparse_matrix_device.hip: only the shapes depend on it
EXACT_MODES = (L.CSR_APPLY, L.CSR_RESIDUAL, L.CSR_SUBTRACT, L.CSR_ADD)


# ---- the restatement ------------------------------------------------------------------------------------------------
def lane_partials(val, xs, S):
    """The S partial sums of a row: lane l folds fma(val, x, sum) over the entries l, l + S, .. (val, xs: python floats)."""
    parts = []
    for lane in range(S):
        s = Fraction(0)
        f = 0.0
        for p in range(lane, len(val), S):
            f = float(Fraction(val[p]) * Fraction(xs[p]) + s)
            s = Fraction(f)
        parts.append(f)
    return np.array(parts, dtype=np.float64)


def butterfly(part):
    """sum += shfl_xor(sum, off) for off = n / 2 .. 1; lane 0 stores."""
    idx = np.arange(len(part))
    off = len(part) // 2
    while off:
        part = part + part[idx ^ off]
        off //= 2
    return part[0]


def exact_row_sum(A, x, row, S):
    """What the kernel with S lanes per row stores for mode apply (S = 256: four wavefronts, added in their fixed order)."""
    s, e = A.indptr[row], A.indptr[row + 1]
    part = lane_partials(A.data[s:e].tolist(), x[A.indices[s:e]].tolist(), S)
    if S <= 64:
        return butterfly(part)
    w = [butterfly(part[64 * k:64 * k + 64]) for k in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_same_bits(got, want, rows, where):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (f"{where}: {bad.size} of {len(rows)} rows differ, first row {rows[bad[0]]}: got {got[bad[0]]!r}, "
                           f"restatement {want[bad[0]]!r}")


def inputs(A, seed):
    rng = np.random.default_rng(seed)
    m, n = A.shape
    return dict(x=scaled_normal(rng, n), b=scaled_normal(rng, m), xp=scaled_normal(rng, m), out0=scaled_normal(rng, m),
                dinv=scaled_normal(rng, m))


def bounded_reference(A, rows, mode, v, al, be):
    """(ref, 2 gamma_k mag) in long double at `rows` for the modes whose expression a compiler may contract."""
    ld = np.longdouble
    sub = A[rows]
    prod = sub.data.astype(ld) * v["x"].astype(ld)[sub.indices]
    ptr = sub.indptr.astype(np.int64)
    ax, mx = row_sums(ptr, prod), row_sums(ptr, np.abs(prod))
    xl, bl, dl, pl = (v[k][rows].astype(ld) for k in ("x", "b", "dinv", "xp"))
    al, be = ld(al), ld(be)
    if mode == L.CSR_FIRST:
        ref, mag = xl - be * dl * (ax - bl), np.abs(xl) + abs(be) * np.abs(dl) * (mx + np.abs(bl))
    elif mode == L.CSR_NEXT:
        ref = xl + al * (xl - pl) - be * dl * (ax - bl)
        mag = np.abs(xl) + abs(al) * (np.abs(xl) + np.abs(pl)) + abs(be) * np.abs(dl) * (mx + np.abs(bl))
    else:
        assert mode == L.CSR_PLUS_SCALED
        ref, mag = ax + be * dl * bl, mx + abs(be) * np.abs(dl) * np.abs(bl)
    k = (np.diff(ptr) + 6).astype(ld)
    return ref, 2 * (k * ld(U) / (1 - k * ld(U))) * mag


def check_all_modes(Ad, ctx, A, v, rows, sums, where):
    """Every mode at `rows` (sums: the exact restatement of the row sums there), twice."""
    rows = np.asarray(rows)
    for mode in MODES:
        for al, be in sorted({ALPHA_BETA[mode], ALPHA_BETA_2.get(mode, ALPHA_BETA[mode])}):
            out = launch(Ad, ctx, mode, v, al, be)
            got = out.cpu().numpy()
            assert np.all(np.isfinite(got)), f"{where}: mode {mode}: entries left unwritten or not finite"
            if mode in EXACT_MODES:
                want = {L.CSR_APPLY: lambda: sums, L.CSR_RESIDUAL: lambda: sums - v["b"][rows],
                        L.CSR_SUBTRACT: lambda: v["out0"][rows] - sums, L.CSR_ADD: lambda: v["out0"][rows] + sums}[mode]()
                assert_same_bits(got[rows], want, rows, f"{where}: mode {mode}")
            else:
                ref, bound = bounded_reference(A, rows, mode, v, al, be)
                excess = np.abs(got[rows].astype(np.longdouble) - ref) - bound
                i = int(excess.argmax())
                assert excess[i] <= 0, (f"{where}: mode {mode}, alpha {al}, beta {be}: row {rows[i]}: got {got[rows][i]!r}, reference "
                                        f"{float(ref[i])!r}, bound {float(bound[i]):.3e}")
            again = launch(Ad, ctx, mode, v, al, be)
            assert torch.equal(out, again), f"{where}: mode {mode}: a repeated launch changed bits"


def check_apply(Ad, ctx, A, v, rows, S, where):
    rows = np.asarray(rows)
    sums = np.array([exact_row_sum(A, v["x"], r, S) for r in rows])
    out = launch(Ad, ctx, L.CSR_APPLY, v, 0.0, 0.0)
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got)), f"{where}: entries left unwritten or not finite"
    assert_same_bits(got[rows], sums, rows, where)
    again = launch(Ad, ctx, L.CSR_APPLY, v, 0.0, 0.0)
    assert torch.equal(out, again), f"{where}: a repeated launch changed bits"
    return got


def check_nan_column(Ad, ctx, A, v, col, where):
    """NaN in x where no row reads: every output finite, and the bits of the launch without it."""
    assert col not in set(A.indices.tolist())
    clean = launch(Ad, ctx, L.CSR_APPLY, v, 0.0, 0.0)
    x = v["x"].copy()
    x[col] = np.nan
    out = launch(Ad, ctx, L.CSR_APPLY, v, 0.0, 0.0, x=x)
    assert np.all(np.isfinite(out.cpu().numpy())), f"{where}: NaN of an unreferenced column reached an output"
    assert torch.equal(out, clean), where


# ---- the matrices ---------------------------------------------------------------------------------------------------
def rows_matrix(lengths, n_cols, seed, free_col=None, window=None):
    """CSR matrix with the given row lengths, sorted random columns (row r from [lo_r, lo_r + window) where a window is
    given), none at free_col; square where n_cols == len(lengths)."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.empty(ptr[-1], dtype=np.int64)
    for r, ln in enumerate(lengths):
        if window is None:
            c = rng.choice(n_cols - 1, ln, replace=False)
            if free_col is not None:
                c = c + (c >= free_col)                       # (n_cols - 1 values mapped around free_col)
        else:
            w = int(window[r])
            lo = min(max(r - w // 2, 0), n_cols - w)
            c = lo + rng.choice(w, ln, replace=False)
        col[ptr[r]:ptr[r + 1]] = np.sort(c)
    val = scaled_normal(rng, int(ptr[-1]))
    A = sp.csr_matrix((val, col, ptr), shape=(len(lengths), n_cols))
    assert A.has_sorted_indices and np.all(A.data != 0.0)
    return A


def edge_lengths(S):
    return [0, 1, S - 1, S, S + 1, B * S - 1, B * S, B * S + 1, 2 * B * S + 1]


ROW_BLOCK_N = 3000
ROW_BLOCK_FREE = 1500


def row_block_matrix():
    """3000 x 3000 (square: all seven modes), the first 40 rows filled: the edge lengths for S = 256, 2 B S + 128, 2 B S + 1
    (two whole batches, then a last batch of one entry, in lane 0 alone) and random lengths; the other rows are empty."""
    rng = np.random.default_rng(256)
    lens = edge_lengths(256) + [2 * B * 256 + 128, 513, 769] + rng.integers(2, 2500, 28).tolist()
    assert len(lens) == 40
    return rows_matrix(lens + [0] * (ROW_BLOCK_N - 40), ROW_BLOCK_N, 1, free_col=ROW_BLOCK_FREE), 40


def lanes_matrix(S):
    """n_rows is no multiple of the 256 / S rows of a workgroup, the last row of the matrix is the longest."""
    n_rows = 2 * (256 // S) + 11
    edges = edge_lengths(S)
    lens = [edges[r % len(edges)] for r in range(n_rows - 1)] + [2 * B * S + 1]
    return rows_matrix(lens, 700, 10 + S, free_col=350)


LDS_ROWS = 256 * 128 + 57                                    # 32768 rows: the smallest matrix with LDS lists; a last block of 57
LDS_LANES = (4, 16, 64)
LDS_EDGE_BLOCK = {4: 20, 16: 22, 64: 24}                     # the block that holds the edge rows of a lanes-per-row value
LDS_WIDE_BLOCKS = {30: (12, 6000, (1024, 2048)), 32: (30, 20000, (2048, 4096)), 34: (48, 30000, (4096, 6144))}


def lds_matrix():
    """Square, 4 to 12 entries per row from a window of 96 columns around the row (a 128-row block reuses them: the LDS
    lists are built), and: per lanes-per-row value a block with the edge lengths; three blocks of long rows over wide
    windows, whose column lists hold more than 1024, 2048 and 4096 distinct columns (2, 4 and 8 elements per thread of the
    staging); the edge lengths for 4 lanes once more in the short last block."""
    rng = np.random.default_rng(7)
    lens = rng.integers(4, 13, LDS_ROWS)
    window = np.full(LDS_ROWS, 96)
    edge_rows = {}
    for S, blk in LDS_EDGE_BLOCK.items():
        rows = 128 * blk + 5 + 3 * np.arange(len(edge_lengths(S)))
        lens[rows] = edge_lengths(S)
        window[rows] = 2500
        edge_rows[S] = rows
    for blk, (ln, w, _) in LDS_WIDE_BLOCKS.items():
        lens[128 * blk:128 * blk + 128] = ln
        window[128 * blk:128 * blk + 128] = w
    last = 256 * 128 + 2 + 5 * np.arange(len(edge_lengths(4)))
    lens[last] = edge_lengths(4)
    edge_rows[4] = np.concatenate([edge_rows[4], last])
    return rows_matrix(lens.tolist(), LDS_ROWS, 8, window=window), edge_rows


LISTED_DIMS = (26, 26, 25)


def listed_matrix():
    """Reach-3 stencil, two unknowns per node: interior rows of 2 * 7^3 = 686 entries; six interior nodes with a diagonal of
    their own are the listed rows.  Returns the matrix and the rows of those nodes."""
    A = stencil_matrix(LISTED_DIMS, reach=3, comps=2, perturb=6, seed=33)
    d = A.diagonal()[::2]
    nodes = np.flatnonzero(d != np.median(d))
    assert len(nodes) == 6
    rows = np.sort(np.concatenate([2 * nodes, 2 * nodes + 1]))
    assert np.all(np.diff(A.indptr)[rows] == 686)
    return A, rows


# ---- no GPU: the shapes are what the docstring says ------------------------------------------------------------------
def test_shapes_reach_the_edges_of_a_batch():
    A, n = row_block_matrix()
    lens = np.diff(A.indptr)
    assert set(edge_lengths(256)) | {2 * B * 256 + 128} <= set(lens[:n].tolist()) and not lens[n:].any()
    assert A.shape == (ROW_BLOCK_N, ROW_BLOCK_N) and ROW_BLOCK_FREE not in set(A.indices.tolist())
    for S in (1, 4, 64):
        A = lanes_matrix(S)
        lens = np.diff(A.indptr)
        assert A.shape[0] % (256 // S) != 0 and lens[-1] == lens.max() == 2 * B * S + 1 and set(edge_lengths(S)) <= set(lens.tolist())
    A, edge_rows = lds_matrix()
    lens = np.diff(A.indptr)
    assert A.shape[0] % 128 == 57 and A.nnz / A.shape[0] >= 4.0
    for S in LDS_LANES:
        assert set(edge_lengths(S)) <= set(lens[edge_rows[S]].tolist())
    assert edge_rows[4].max() >= 256 * 128
    distinct = [len(np.unique(A.indices[A.indptr[r0]:A.indptr[min(r0 + 128, A.shape[0])]])) for r0 in range(0, A.shape[0], 128)]
    for blk, (_, _, (lo, hi)) in LDS_WIDE_BLOCKS.items():
        assert lo < distinct[blk] <= hi, (blk, distinct[blk])
    # what choose_layouts asks of the lists: no block beyond 6144 columns, a column reused three times on average
    assert max(distinct) <= 6144 and A.nnz >= 3 * sum(distinct)


def test_restatement_orders():
    """The restatement itself on sums small enough to do by hand: the butterfly of 4 lanes is (l0 + l2) + (l1 + l3), a lane
    folds its entries in ascending order with one rounding per entry."""
    assert butterfly(np.array([1.0, 2.0 ** -53, -1.0, 2.0 ** -53])) == 2.0 ** -52
    assert ((1.0 + 2.0 ** -53) + -1.0) + 2.0 ** -53 == 2.0 ** -53              # (another order, another result)
    v = [1.0 + 2.0 ** -52, 1.0, -1.0]
    x = [1.0 + 2.0 ** -52, -1.0, 2.0 ** -110]
    # one lane: fma(v0, x0, 0) = 1 + 2^-51 (the 2^-104 of the square is rounded away), the second entry leaves 2^-51 exactly,
    # the third subtracts 2^-110, less than half an ulp of it
    assert lane_partials(v, x, 1).tolist() == [2.0 ** -51]
    # two lanes: lane 0 has the entries 0 and 2, lane 1 the entry 1
    assert lane_partials(v, x, 2).tolist() == [1.0 + 2.0 ** -51, -1.0]
    # a product that float64 rounds before the addition and an fma does not: 2^-104 survives
    assert lane_partials([1.0, 1.0 + 2.0 ** -52], [-(1.0 + 2.0 ** -51), 1.0 + 2.0 ** -52], 1).tolist() == [2.0 ** -104]


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_row_block_kernel(ctx):
    A, n = row_block_matrix()
    Ad = M.SparseMatrixDevice(ctx, A)
    Ad.set_kernel(256)
    f = Ad.form()
    assert f["csr_kernel"] == "row_block" and f["lanes"] == 256, f
    v = inputs(A, 2)
    rows = np.concatenate([np.arange(n), [n, 1234, ROW_BLOCK_N - 1]])           # (the filled rows and three empty ones)
    sums = np.array([exact_row_sum(A, v["x"], r, 256) for r in rows])
    check_all_modes(Ad, ctx, A, v, rows, sums, "row_block")
    check_nan_column(Ad, ctx, A, v, ROW_BLOCK_FREE, "row_block")


@pytest.mark.gpu
@pytest.mark.parametrize("S", (1, 4, 64))
def test_lanes_kernel(ctx, S):
    A = lanes_matrix(S)
    Ad = M.SparseMatrixDevice(ctx, A)
    Ad.set_kernel(S, 0)
    f = Ad.form()
    assert f["csr_kernel"] == "lanes" and f["lanes"] == S, f
    v = inputs(A, 3)
    check_apply(Ad, ctx, A, v, np.arange(A.shape[0]), S, f"lanes{S}")
    check_nan_column(Ad, ctx, A, v, 350, f"lanes{S}")


@pytest.fixture(scope="module")
def lds_case(ctx):
    A, edge_rows = lds_matrix()
    return A, edge_rows, M.SparseMatrixDevice(ctx, A), inputs(A, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("S", LDS_LANES)
def test_lds_kernel(ctx, lds_case, S):
    A, edge_rows, Ad, v = lds_case
    Ad.set_kernel(S, 1)
    f = Ad.form()
    assert f["csr_kernel"] == "lds" and f["lanes"] == S, f
    wide = np.concatenate([128 * blk + np.array([0, 1, 63, 127]) for blk in LDS_WIDE_BLOCKS])
    sample = np.random.default_rng(100 + S).choice(A.shape[0], 256, replace=False)
    rows = np.unique(np.concatenate([edge_rows[S], wide, sample, [A.shape[0] - 57, A.shape[0] - 1]]))
    check_apply(Ad, ctx, A, v, rows, S, f"lds{S}")


@pytest.mark.gpu
def test_listed_rows(ctx):
    A, rows = listed_matrix()
    Ad = M.SparseMatrixDevice(ctx, A)
    f = Ad.form()
    assert f["kind"] in (2, 3) and f["regular"] == 1 and f["listed"] >= len(rows), f
    assert f["listed_route"] in ("class_tail", "split_tail"), f
    v = inputs(A, 5)
    sums = np.array([exact_row_sum(A, v["x"], r, 64) for r in rows])
    check_all_modes(Ad, ctx, A, v, rows, sums, "listed")
    assert Ad.release_csr()
    assert Ad.form()["csr_released"] == 1
    check_all_modes(Ad, ctx, A, v, rows, sums, "listed, CSR released")
