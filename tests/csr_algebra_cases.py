"""Cases of the device transpose and the device sparse product C = A B (mfmg_amd/csrc/csr_algebra.hip) for
test_csr_algebra_case_table.py (no GPU) and test_gpu_csr_algebra.py: the constants the cases straddle, the rules by which the host
code picks a table and a path restated in plain Python, the generators (all seeded), the references and the comparator.  Nothing
here imports the library; a matrix is the tuple (indptr, indices, data, shape) that SparseMatrixDevice takes as it is.

Product.  csr_multiply_device counts, per row r of A, the candidates ub[r] = sum of the lengths of the rows of B that the row
selects (with multiplicity).  No row above 2048 candidates: every row goes through product_row_kernel, with a hash table in LDS of
64 slots up to 32 candidates, doubling up to 4096 slots at 2048, linear probing from hash_of(column).  Some row above 2048 and B
of at most 8192 columns: EVERY row goes through product_row_direct_kernel, whose table is addressed by the column.  Otherwise the
host algorithm.  The grid is min(a_rows, 2^20) workgroups which stride over the rows.

Transpose.  Histogram of the columns, scan, scatter through per-column cursors (one wavefront per row of A), then every row of
the transpose is sorted: 2 .. 64 entries by a wavefront (one wavefront per row), 65 .. 4096 by a workgroup in LDS, padded to a power
of two of at least 128; a longer row sends the whole transpose to the host.  Both wavefront-per-row grids are capped at 65536
workgroups of four wavefronts and stride beyond.

A product case is built around one NAMED row of A with exactly the candidate count its name gives; every product matrix also
carries the same furniture around it: an empty row of A, a row that selects only empty rows of B (0 candidates), rows of one entry
(1 and 10 candidates) and a row of 40 candidates.

The issue asks, of the probe-chain cases, for 32 (512) distinct columns in a table of 64 (1024) slots that arrive "some of them
twice".  A table of 64 slots serves at most 32 candidates, so 32 distinct columns cannot arrive twice in it.  Three cases per size
cover every reading: `chain-64` (32 distinct columns over three rows of B: the chain fills half the table and wraps),
`chain-64-twice` (24 distinct, 8 of them twice: 32 candidates, still 64 slots) and `chain-64-twice-128` (32 distinct, 8 of them
twice: 40 candidates, 128 slots, where the columns fall on slots 63 and 127 only and the chain from 127 wraps)."""
import functools
from collections import namedtuple

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# ---- the constants the cases straddle, each with the line of csr_algebra.hip it restates ----
K_MAX_SORT_ROW = 4096               # :23   constexpr int kMaxSortRow = 4096
K_MAX_HASH = 4096                   # :24   constexpr int kMaxHash = 4096
K_MAX_DIRECT = 8192                 # :325  constexpr int kMaxDirect = 8192
PRODUCT_GRID_CAP = 1 << 20          # :416  product_grid = min(a_rows, 1 << 20)
TRANSPOSE_WAVE_CAP = (1 << 16) * 4  # :284, :286  n_blocks_for(n * 64, 256, 1 << 16): 65536 workgroups of 256 threads = 262144 wavefronts
HASH_MULTIPLIER = 2654435761        # :142  ((unsigned int)key * 2654435761u) & mask
WAVE_SORT_MAX = 64                  # :56   if (len < 2 || len > 64) continue;  :276  if (cnt[c] > 64) long_rows.push_back
LONG_SORT_MIN_PAD = 128             # :91   int n2 = 128
BLOCK = 256                         # :336  per = (b_cols + 255) / 256

CSR = namedtuple("CSR", "indptr indices data shape")


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * LD(U) / (1 - k * LD(U))


def signed_decades(rng, n):
    """signed values whose magnitudes span six decades (as in test_gpu_fgmres.py)"""
    return rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-3.0, 3.0, size=n)


def small_integers(rng, n):
    """1 .. 8 as doubles: every product and every sum of them is exact whatever the order, and nothing cancels"""
    return rng.integers(1, 9, size=n).astype(np.float64)


# ---- the rules of the host code, restated ----
def hash_of(col, mask):
    return (np.asarray(col, dtype=np.uint64) * np.uint64(HASH_MULTIPLIER) & np.uint64(0xFFFFFFFF)) & np.uint64(mask)


def table_size(candidates):
    """product_row_kernel: size = 64; while (size < 2 * bound && size < kMaxHash) size <<= 1"""
    size = 64
    while size < 2 * candidates and size < K_MAX_HASH:
        size <<= 1
    return size


def last_slot_column(size):
    """The smallest column that hash_of sends to the last slot of a table of `size` slots; every `size`-th column after it follows."""
    c0 = (-pow(HASH_MULTIPLIER % size, -1, size)) % size
    assert int(hash_of(c0, size - 1)) == size - 1
    return c0


def candidate_counts(A, B):
    """ub[r] of product_upper_bound_kernel"""
    b_len = np.diff(B.indptr).astype(np.int64)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return np.bincount(rows, weights=b_len[A.indices], minlength=A.shape[0]).astype(np.int64)


def product_path(A, B):
    """'hash', 'direct' (addressed by the column) or 'fallback', as csr_multiply_device decides for the whole product"""
    ub = candidate_counts(A, B)
    if (2 * ub <= K_MAX_HASH).all():
        return "hash"
    return "direct" if 0 < B.shape[1] <= K_MAX_DIRECT else "fallback"


def transpose_path(A):
    counts = np.bincount(A.indices, minlength=A.shape[1])
    return "device" if counts.max(initial=0) <= K_MAX_SORT_ROW else "fallback"


# ---- references ----
def transpose_reference(A):
    """Values are moved, not computed: a stable sort of the entries by column leaves the rows of each column in order."""
    order = np.argsort(A.indices, kind="stable")
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int32), np.diff(A.indptr))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(A.indices, minlength=A.shape[1]))]).astype(np.int32)
    return CSR(indptr, rows[order], A.data[order], (A.shape[1], A.shape[0]))


def product_reference_bits(A, B):
    """The Gustavson sum as the kernels document it, in float64: the entries of a row of A in storage order, acc[columns of the
    row of B] += a * b, the product rounded, then the sum rounded (numpy has no fma).  A column reached by several terms is one
    entry; a column reached at all is an entry, whatever its sum.  (A Python loop over the entries of A: small matrices only.)"""
    assert A.indices.size <= 20000 and A.shape[1] == B.shape[0]
    acc = np.zeros(B.shape[1])
    indptr, cols_out, vals_out = [0], [], []
    for r in range(A.shape[0]):
        touched = []
        for p in range(A.indptr[r], A.indptr[r + 1]):
            k = A.indices[p]
            cols = B.indices[B.indptr[k]:B.indptr[k + 1]]
            prod = A.data[p] * B.data[B.indptr[k]:B.indptr[k + 1]]
            acc[cols] = acc[cols] + prod                        # (the columns of one row of B are distinct)
            touched.append(cols)
        cols = np.unique(np.concatenate(touched)) if touched else np.zeros(0, dtype=np.int32)
        cols_out.append(cols.astype(np.int32))
        vals_out.append(acc[cols].copy())
        acc[cols] = 0.0
        indptr.append(indptr[-1] + cols.size)
    return CSR(np.asarray(indptr, dtype=np.int32), np.concatenate(cols_out).astype(np.int32), np.concatenate(vals_out),
               (A.shape[0], B.shape[1]))


def _terms(A, B):
    """Every term a_rk b_kc of the product: (row, column, index into A.data, index into B.data), in the order of the Gustavson sum."""
    b_len = np.diff(B.indptr).astype(np.int64)[A.indices]
    total = int(b_len.sum())
    first = np.cumsum(b_len) - b_len
    q = np.repeat(B.indptr[A.indices].astype(np.int64), b_len) + (np.arange(total) - np.repeat(first, b_len))
    p = np.repeat(np.arange(A.indices.size), b_len)
    row = np.repeat(np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr)), b_len)
    return row, B.indices[q].astype(np.int64), p, q


def _reduce_terms(A, B, term_values):
    """Sums of the terms per (row, column): CSR pattern, the segments' starts in the sorted term list and the sorting order."""
    row, col, p, q = _terms(A, B)
    n, b_cols = A.shape[0], B.shape[1]
    if row.size == 0:
        return np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), [v[:0] for v in term_values(p, q)], np.zeros(0, dtype=np.int64)
    key = row * b_cols + col
    order = np.argsort(key, kind="stable")
    key = key[order]
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    sums = [np.add.reduceat(v[order], starts) for v in term_values(p, q)]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(key[starts] // b_cols, minlength=n))]).astype(np.int32)
    m = np.diff(np.concatenate([starts, [key.size]]))
    return indptr, (key[starts] % b_cols).astype(np.int32), sums, m


def product_reference_long(A, B):
    """The same sums in long double, from the list of all terms (not the row loop of product_reference_bits): the pattern as CSR
    without values, and per entry the sum, mag = (|A| |B|) and the number of terms m.  A correct float64 product is within
    gamma_{m+1} mag of the sum: one rounding per product and m - 1 per sum, and one more for the reference's own rounding at 2^-64."""
    def values(p, q):
        t = A.data[p].astype(LD) * B.data[q].astype(LD)
        return t, np.abs(t)
    indptr, indices, (want, mag), m = _reduce_terms(A, B, values)
    return CSR(indptr, indices, None, (A.shape[0], B.shape[1])), want, mag, m


def product_reference_int(A, B):
    """For the matrices of small_integers: the product in int64 -- exact, whatever the order of the sums."""
    assert (A.data == np.rint(A.data)).all() and (B.data == np.rint(B.data)).all() and A.data.min() >= 1 and B.data.min() >= 1
    indptr, indices, (sums,), _ = _reduce_terms(A, B, lambda p, q: (A.data[p].astype(np.int64) * B.data[q].astype(np.int64),))
    assert sums.max() < 2 ** 53
    return CSR(indptr, indices, sums.astype(np.float64), (A.shape[0], B.shape[1]))


def beyond_product_bound(got_data, want, mag, m):
    """Entries outside gamma_{m+1} mag; NaN counts as outside."""
    return ~(np.abs(np.asarray(got_data).astype(LD) - want) <= gamma(m + 1) * mag)


def worst_ratio(got, want, mag):
    ok = mag > 0
    return float((np.abs(np.asarray(got).astype(LD) - want)[ok] / (LD(U) * mag[ok])).max()) if ok.any() else 0.0


def spmv_long(M, x):
    """M x, |M| |x| and the row lengths, in long double."""
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    prod = np.asarray(M.data).astype(LD) * np.asarray(x).astype(LD)[M.indices]
    out, mag = np.zeros(M.shape[0], dtype=LD), np.zeros(M.shape[0], dtype=LD)
    np.add.at(out, rows, prod)
    np.add.at(mag, rows, np.abs(prod))
    return out, mag, np.diff(M.indptr)


def beyond_spmv_bound(got, want, mag, length):
    return ~(np.abs(np.asarray(got).astype(LD) - want) <= gamma(length + 1) * mag)


def assert_same_csr(got, want, what):
    """indptr, indices and the BITS of the data of `got` are those of `want`, and the columns of every row of `got` increase
    strictly.  Reports the first row that differs."""
    gp, gi, gd = (np.asarray(a) for a in (got.indptr, got.indices, got.data))
    wp, wi, wd = (np.asarray(a) for a in (want.indptr, want.indices, want.data))
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    assert gd.dtype == np.float64 and wd.dtype == np.float64
    n = wp.size - 1
    assert gp.size == wp.size and gp[0] == 0, f"{what}: indptr of {gp.size} entries starting at {gp[:1]}"
    if not np.array_equal(gp, wp):
        r = int(np.flatnonzero(np.diff(gp) != np.diff(wp))[0])
        raise AssertionError(f"{what}: row {r} has {gp[r + 1] - gp[r]} entries, expected {wp[r + 1] - wp[r]}")
    assert gi.size == gp[-1] and gd.size == gp[-1], f"{what}: {gi.size} columns and {gd.size} values for indptr[-1] = {gp[-1]}"
    rows = np.repeat(np.arange(n), np.diff(wp))
    within = rows[1:] == rows[:-1]
    unsorted = np.flatnonzero(within & (np.diff(gi.astype(np.int64)) <= 0))
    if unsorted.size:
        r, q = int(rows[unsorted[0]]), int(unsorted[0])
        raise AssertionError(f"{what}: columns of row {r} do not increase strictly: {gi[q]} before {gi[q + 1]}")
    bad = np.flatnonzero(gi != wi)
    if bad.size:
        r = int(rows[bad[0]])
        raise AssertionError(f"{what}: row {r} has columns {gi[gp[r]:gp[r + 1]][:8]}.., expected {wi[wp[r]:wp[r + 1]][:8]}.. "
                             f"({bad.size} entries differ)")
    bad = np.flatnonzero(gd.view(np.uint64) != wd.view(np.uint64))
    if bad.size:
        r, q = int(rows[bad[0]]), int(bad[0])
        raise AssertionError(f"{what}: row {r}, column {gi[q]}: value {gd[q]!r} ({gd[q].hex()}), expected {wd[q]!r} ({wd[q].hex()}); "
                             f"{bad.size} values differ in their bits")


# ---- generators ----
def _subset(rng, pool, k):
    return np.sort(rng.choice(pool, size=k, replace=False))


def _lengths(rng, k, total, hi):
    """k lengths that sum to `total`, none above `hi`, not all alike."""
    out = np.full(k, total // k)
    out[:total % k] += 1
    room = int(min(hi - out.max(), out.min() - 1, out.min() // 4))
    for i in range(0, k - 1, 2):
        d = int(rng.integers(0, room + 1))
        out[i] += d
        out[i + 1] -= d
    assert out.sum() == total and out.max() <= hi and out.min() >= 1
    return out


class _Product:
    """Rows of B (sets of columns) and rows of A (sets of rows of B), collected and turned into two CSR matrices."""

    def __init__(self, rng, b_cols, data):
        self.rng, self.b_cols, self.data = rng, b_cols, data
        self.b_rows, self.a_rows, self.named = [], [], None
        self.empty = [self.b_row([]), self.b_row([])]
        self.single = self.b_row(_subset(rng, b_cols, 1))
        span = min(b_cols, 64)                                   # four rows of ten over a narrow range: they overlap
        self.ten = [self.b_row(_subset(rng, span, 10)) for _ in range(4)]
        self.a_row([])                                           # an empty row of A
        self.a_row(self.empty)                                   # only empty rows of B: 0 candidates
        self.a_row([self.single])                                # 1 candidate
        self.a_row([self.ten[1]])                                # one entry, 10 candidates
        self.forty = self.a_row(self.ten)                        # 40 candidates, some of them twice

    def b_row(self, cols):
        cols = np.asarray(cols, dtype=np.int64)
        assert np.unique(cols).size == cols.size and (cols.size == 0 or (0 <= cols.min() and cols.max() < self.b_cols))
        self.b_rows.append(np.sort(cols))
        return len(self.b_rows) - 1

    def a_row(self, b_rows, named=False):
        assert len(set(b_rows)) == len(b_rows)
        self.a_rows.append(np.sort(np.asarray(b_rows, dtype=np.int64)))
        if named:
            self.named = len(self.a_rows) - 1
        return len(self.a_rows) - 1

    def finish(self):
        self.a_row([self.single, self.empty[0]])                 # after the named row: an empty row of B beside one entry
        self.a_row([])
        self.a_row(self.ten[:2])
        fill = signed_decades if self.data == "float" else small_integers

        def csr(rows, n_cols):
            indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
            indices = np.concatenate(rows).astype(np.int32)
            return CSR(indptr, indices, fill(self.rng, indices.size), (len(rows), n_cols))
        return {"A": csr(self.a_rows, len(self.b_rows)), "B": csr(self.b_rows, self.b_cols), "named": self.named, "data": self.data,
                "forty": self.forty}


def _spread(rng, prod, columns, lengths, twice):
    """Rows of B for a named row: the first rows partition `columns` with the given lengths; each further row is `twice[i]` of the
    same columns again."""
    columns = rng.permutation(columns)
    assert sum(lengths) == columns.size
    rows, at = [], 0
    for n in lengths:
        rows.append(prod.b_row(columns[at:at + n]))
        at += n
    for n in twice:
        rows.append(prod.b_row(_subset(rng, columns, n)))
    return rows


def _hash_case(count, duplicates, b_cols=None, seed=0):
    rng = np.random.default_rng([11, count, int(duplicates), seed])
    prod = _Product(rng, b_cols or 3 * count + 50, "float")
    if count == 0:
        rows = prod.empty + [prod.b_row([])]
    elif count == 1:
        rows = [prod.empty[1], prod.b_row(_subset(rng, prod.b_cols, 1))]
    else:
        distinct = count - count // 2 if duplicates else count
        again = count - distinct
        parts = min(distinct, 3)
        lengths = _lengths(rng, parts, distinct, distinct) if distinct >= 12 else \
            [distinct // parts + (1 if i < distinct % parts else 0) for i in range(parts)]
        twice = [again - again // 2, again // 2] if again >= 2 else [again] if again else []
        rows = _spread(rng, prod, _subset(rng, prod.b_cols, distinct), list(lengths), twice)
    prod.a_row(rows, named=True)
    return prod.finish()


def _chain_case(size, distinct, again):
    """`distinct` columns that all hash to the last slot under mask size - 1, over three rows of B, and `again` of them in a fourth."""
    rng = np.random.default_rng([12, size, distinct, again])
    c0 = last_slot_column(size)
    prod = _Product(rng, c0 + size * distinct + 5, "float")
    columns = c0 + size * np.arange(distinct)
    rows = _spread(rng, prod, columns, list(_lengths(rng, 3, distinct, distinct)), [again] if again else [])
    prod.a_row(rows, named=True)
    out = prod.finish()
    out["chain"] = (size, columns)
    return out


def _direct_case(b_cols, count, k, seed=0):
    """A named row of `count` >= 2049 candidates through k dense-ish rows of B, the first with columns 0 and b_cols - 1; a tenth
    of the inner columns is in none of them, so the compaction of the named row has gaps."""
    rng = np.random.default_rng([13, b_cols, count, k, seed])
    prod = _Product(rng, b_cols, "float")
    pool = np.concatenate([[0], _subset(rng, np.arange(1, b_cols - 1), (b_cols - 2) * 9 // 10), [b_cols - 1]])
    rows = []
    for i, n in enumerate(_lengths(rng, k, count, pool.size)):
        cols = _subset(rng, pool, int(n))
        if i == 0:
            inner = cols[(cols != 0) & (cols != b_cols - 1)]
            cols = np.concatenate([[0, b_cols - 1], inner[:n - 2]])
        rows.append(prod.b_row(cols))
    prod.a_row(rows, named=True)
    return prod.finish()


STRIDE_B_ROWS, STRIDE_PAIRS = 200, 64


def _stride_b(rng, b_cols):
    """Rows of 1 .. 3 entries (even) and of 40 (odd), alternating."""
    rows = [_subset(rng, b_cols, 40 if i % 2 else 1 + (i // 2) % 3) for i in range(STRIDE_B_ROWS)]
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    indices = np.concatenate(rows).astype(np.int32)
    return CSR(indptr, indices, small_integers(rng, indices.size), (STRIDE_B_ROWS, b_cols))


def _stride_a(rng):
    """2^20 + 64 rows of one entry.  Most select a short row of B, one in a hundred a row of 40; the workgroups r < 64 meet two
    rows, r and r + 2^20: a short one and then one of 40 for r < 32, the other way round for 32 <= r < 64."""
    n = PRODUCT_GRID_CAP + STRIDE_PAIRS
    col = 2 * rng.integers(0, STRIDE_B_ROWS // 2, size=n)
    col[rng.random(n) < 0.01] += 1
    first, second = np.arange(STRIDE_PAIRS), np.arange(STRIDE_PAIRS) + PRODUCT_GRID_CAP
    short, long_ = 2 * rng.integers(0, STRIDE_B_ROWS // 2, size=STRIDE_PAIRS), 2 * rng.integers(0, STRIDE_B_ROWS // 2, size=STRIDE_PAIRS) + 1
    low = first < STRIDE_PAIRS // 2
    col[first], col[second] = np.where(low, short, long_), np.where(low, long_, short)
    return CSR(np.arange(n + 1, dtype=np.int32), col.astype(np.int32), small_integers(rng, n), (n, STRIDE_B_ROWS))


STRIDE_DIRECT_ROW = 7


def _stride_case(direct):
    rng = np.random.default_rng(14)                              # (the same A in both cases)
    A = _stride_a(rng)
    if not direct:
        return {"A": A, "B": _stride_b(rng, 500), "named": None, "data": "int"}
    # one more row, of 60 x 40 candidates, at STRIDE_DIRECT_ROW: its workgroup goes on to row STRIDE_DIRECT_ROW + 2^20
    rng = np.random.default_rng(15)
    long_row = np.sort(2 * rng.choice(STRIDE_B_ROWS // 2, size=60, replace=False) + 1).astype(np.int32)
    at = STRIDE_DIRECT_ROW
    indices = np.concatenate([A.indices[:at], long_row, A.indices[at:]])
    data = np.concatenate([A.data[:at], small_integers(rng, 60), A.data[at:]])
    indptr = np.concatenate([A.indptr[:at + 1], A.indptr[at:] + 60]).astype(np.int32)
    return {"A": CSR(indptr, indices, data, (A.shape[0] + 1, STRIDE_B_ROWS)), "B": _stride_b(rng, 100), "named": at, "data": "int"}


HASH_COUNTS = (0, 1, 32, 33, 64, 65, 1024, 1025, 2048)
DIRECT_COLUMNS = (100, 255, 256, 257, 8192)
PRODUCTS = {f"hash-{n}-distinct": functools.partial(_hash_case, n, False) for n in HASH_COUNTS}
PRODUCTS.update({f"hash-{n}-dup": functools.partial(_hash_case, n, True) for n in HASH_COUNTS if n >= 2})
PRODUCTS.update({
    "chain-64": functools.partial(_chain_case, 64, 32, 0),
    "chain-64-twice": functools.partial(_chain_case, 64, 24, 8),
    "chain-64-twice-128": functools.partial(_chain_case, 64, 32, 8),
    "chain-1024": functools.partial(_chain_case, 1024, 512, 0),
    "chain-1024-twice": functools.partial(_chain_case, 1024, 384, 128),
    "chain-1024-twice-2048": functools.partial(_chain_case, 1024, 512, 128),
    "direct-100": functools.partial(_direct_case, 100, 2400, 30),
    "direct-255": functools.partial(_direct_case, 255, 2049, 12),
    "direct-256": functools.partial(_direct_case, 256, 2600, 13),
    "direct-257": functools.partial(_direct_case, 257, 2049, 10),
    "direct-8192": functools.partial(_direct_case, 8192, 18000, 6),
    "fallback-2049-8193": functools.partial(_hash_case, 2049, False, 8193),
    "hash-2048-8193": functools.partial(_hash_case, 2048, False, 8193, 1),
    "stride-hash": functools.partial(_stride_case, False),
    "stride-direct": functools.partial(_stride_case, True),
})

# ---- transposes ----
NAMED_COLUMN_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096)
LENGTHS_SHAPE, LENGTHS_DENSE_ROW = (4100, 300), 17


def named_column(i):
    return 7 + 23 * i


def _from_pairs(rng, rows, cols, shape, fill):
    order = np.lexsort((cols, rows))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=shape[0]))]).astype(np.int32)
    return CSR(indptr, cols[order].astype(np.int32), fill(rng, rows.size), shape)


def _lengths_case():
    """Columns named_column(i) hold exactly NAMED_COLUMN_COUNTS[i] entries; the others 0 .. 8 at random, and row LENGTHS_DENSE_ROW
    has an entry in every second of them (a row of A longer than two wavefronts in the scatter)."""
    rng = np.random.default_rng(16)
    n_rows, n_cols = LENGTHS_SHAPE
    named = {named_column(i): k for i, k in enumerate(NAMED_COLUMN_COUNTS)}
    rows, cols = [], []
    for c in range(n_cols):
        if c in named:
            r = _subset(rng, n_rows, named[c])
        else:
            r = _subset(rng, n_rows, int(rng.integers(0, 9)))
            if c % 2 == 0:
                r = np.union1d(r, [LENGTHS_DENSE_ROW])
        rows.append(r)
        cols.append(np.full(r.size, c))
    return {"A": _from_pairs(rng, np.concatenate(rows), np.concatenate(cols), LENGTHS_SHAPE, signed_decades), "data": "float"}


def _vector_case(shape):
    rng = np.random.default_rng([17, *shape])
    n = max(shape)
    line = np.arange(n)
    rows, cols = (np.zeros(n, dtype=np.int64), line) if shape[0] == 1 else (line, np.zeros(n, dtype=np.int64))
    return {"A": _from_pairs(rng, rows, cols, shape, signed_decades), "data": "float"}


STRIDE_TRANSPOSE_SHAPE = (300000, 270000)


def _stride_transpose_case():
    """Three entries per row, small integers: more rows than the scatter has wavefronts, more columns than the short-row sort has."""
    rng = np.random.default_rng(18)
    n_rows, n_cols = STRIDE_TRANSPOSE_SHAPE
    cols = np.sort(rng.integers(0, n_cols, size=(n_rows, 3)), axis=1)
    while True:
        again = np.flatnonzero((cols[:, 0] == cols[:, 1]) | (cols[:, 1] == cols[:, 2]))
        if again.size == 0:
            break
        cols[again] = np.sort(rng.integers(0, n_cols, size=(again.size, 3)), axis=1)
    indptr = (3 * np.arange(n_rows + 1)).astype(np.int32)
    return {"A": CSR(indptr, cols.reshape(-1).astype(np.int32), small_integers(rng, 3 * n_rows), STRIDE_TRANSPOSE_SHAPE), "data": "int"}


TRANSPOSES = {
    "lengths": _lengths_case,
    "one-row-4096": functools.partial(_vector_case, (1, 4096)),
    "one-column-4096": functools.partial(_vector_case, (4096, 1)),
    "one-column-4097": functools.partial(_vector_case, (4097, 1)),
    "stride": _stride_transpose_case,
}


@functools.lru_cache(maxsize=None)
def product_case(name):
    """The matrices of a product case with its path and its references ("bits": what the device must return bit for bit; "long":
    product_reference_long, float cases only).  Built once, shared, read-only."""
    case = dict(PRODUCTS[name]())
    A, B = case["A"], case["B"]
    case["path"] = product_path(A, B)
    if case["data"] == "float":
        case["bits"] = product_reference_bits(A, B)
        case["long"] = product_reference_long(A, B)
    else:
        case["bits"] = product_reference_int(A, B)
    for M in (A, B, case["bits"]):
        for a in M[:3]:
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def transpose_case(name):
    case = dict(TRANSPOSES[name]())
    case["path"] = transpose_path(case["A"])
    case["bits"] = transpose_reference(case["A"])
    for M in (case["A"], case["bits"]):
        for a in M[:3]:
            a.setflags(write=False)
    return case


def vector_for(name, n):
    """The six-decade vector a result of case `name` is applied to."""
    return signed_decades(np.random.default_rng([19, len(name), n]), n)
