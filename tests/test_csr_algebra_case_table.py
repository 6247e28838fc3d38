"""The case table of test_gpu_csr_algebra.py (csr_algebra_cases.py) on the CPU: every table size, probe chain, compaction width,
fall-back limit, sort length and grid stride that the table is there for is reached by a case, by the rules of the host code
restated in csr_algebra_cases.py -- and the comparator and the references of the GPU test notice what a wrong kernel would
return: each defect planted in a copy of a reference result fails assert_same_csr, or the long-double bound where that applies,
while the references themselves, written twice independently, agree within the bound."""
import numpy as np
import pytest

import csr_algebra_cases as C

SMALL_PRODUCTS = [n for n in C.PRODUCTS if not n.startswith("stride")]
FLOAT_PRODUCTS = [n for n in SMALL_PRODUCTS if C.product_case(n)["data"] == "float"]


def _facts(name):
    """What the host code would compute for a product case."""
    c = C.product_case(name)
    A, B = c["A"], c["B"]
    ub = C.candidate_counts(A, B)
    f = {"name": name, "path": c["path"], "ub": ub, "a_rows": A.shape[0], "b_cols": B.shape[1], "a_len": np.diff(A.indptr),
         "distinct": np.diff(c["bits"].indptr), "named": c["named"], "chain": c.get("chain"), "data": c["data"],
         "m_max": int(c["long"][3].max()) if "long" in c else None}
    if c["named"] is not None:
        r = c["named"]
        f.update(n=int(ub[r]), d=int(f["distinct"][r]), size=C.table_size(int(ub[r])), steps=int(f["a_len"][r]),
                 named_columns=c["bits"].indices[c["bits"].indptr[r]:c["bits"].indptr[r + 1]])
    return f


def _hash_edge(n, duplicates):
    size = {0: 64, 1: 64, 32: 64, 33: 128, 64: 128, 65: 256, 1024: 2048, 1025: 4096, 2048: 4096}[n]
    if duplicates:
        return lambda f: f["path"] == "hash" and f["named"] is not None and f["n"] == n and f["size"] == size and not f["chain"] \
            and 0.4 * n <= f["d"] <= 0.6 * n
    return lambda f: f["path"] == "hash" and f["named"] is not None and f["n"] == n and f["size"] == size and f["d"] == n \
        and f["b_cols"] <= C.K_MAX_DIRECT


def _chain_edge(size, distinct, candidates, table):
    return lambda f: f["path"] == "hash" and f["chain"] is not None and f["chain"][0] == size and f["d"] == distinct \
        and f["n"] == candidates and f["size"] == table and f["steps"] >= 3


def _direct_edge(b_cols):
    return lambda f: f["path"] == "direct" and f["b_cols"] == b_cols and f["data"] == "float" and f["n"] >= 2049 and f["m_max"] >= 4 \
        and {0, 1, 40} <= set(f["ub"].tolist()) and (f["a_len"] == 0).any() and (f["a_len"] == 1).any() \
        and f["named_columns"][0] == 0 and f["named_columns"][-1] == b_cols - 1 and f["d"] < b_cols


PRODUCT_EDGES = {f"hash table for {n} candidates, all distinct": _hash_edge(n, False) for n in C.HASH_COUNTS}
PRODUCT_EDGES.update({f"hash table for {n} candidates, about half of them duplicates": _hash_edge(n, True) for n in C.HASH_COUNTS if n >= 2})
PRODUCT_EDGES.update({
    "32 distinct columns on slot 63 of 64, in three steps": _chain_edge(64, 32, 32, 64),
    "24 columns on slot 63 of 64, 8 of them twice": _chain_edge(64, 24, 32, 64),
    "32 columns of slot 63 of 64, 8 of them twice: 128 slots": _chain_edge(64, 32, 40, 128),
    "512 distinct columns on slot 1023 of 1024, in three steps": _chain_edge(1024, 512, 512, 1024),
    "384 columns on slot 1023 of 1024, 128 of them twice": _chain_edge(1024, 384, 512, 1024),
    "512 columns of slot 1023 of 1024, 128 of them twice: 2048 slots": _chain_edge(1024, 512, 640, 2048),
    "exactly 2049 candidates, addressed by the column": lambda f: f["path"] == "direct" and f["ub"].max() == 2049,
    "2049 candidates and 8193 columns: host": lambda f: f["path"] == "fallback" and f["ub"].max() == 2049 and f["b_cols"] == C.K_MAX_DIRECT + 1,
    "2048 candidates and 8193 columns: hash": lambda f: f["path"] == "hash" and f["ub"].max() == 2048 and f["b_cols"] == C.K_MAX_DIRECT + 1,
    "threads with empty runs in the compaction": lambda f: f["path"] == "direct" and f["b_cols"] < C.BLOCK,
    "two slots per thread, the last thread with one": lambda f: f["path"] == "direct" and f["b_cols"] == 257,
    "hash path, workgroups stride over the rows": lambda f: f["path"] == "hash" and f["a_rows"] == C.PRODUCT_GRID_CAP + 64 and f["data"] == "int",
    "column-addressed path, workgroups stride over the rows": lambda f: f["path"] == "direct" and f["a_rows"] > C.PRODUCT_GRID_CAP
    and f["b_cols"] == 100 and f["data"] == "int",
})
PRODUCT_EDGES.update({f"addressed by the column, B of {b} columns": _direct_edge(b) for b in C.DIRECT_COLUMNS})


def test_product_cases_cover_every_edge():
    facts = {name: _facts(name) for name in C.PRODUCTS}
    providers = {edge: [n for n, f in facts.items() if reached(f)] for edge, reached in PRODUCT_EDGES.items()}
    assert all(providers.values()), [e for e, p in providers.items() if not p]
    assert set().union(*providers.values()) == set(C.PRODUCTS), set(C.PRODUCTS) - set().union(*providers.values())
    # the doubling edges, by the rule itself
    assert [C.table_size(n) for n in (0, 1, 32, 33, 64, 65, 1024, 1025, 2048)] == [64, 64, 64, 128, 128, 256, 2048, 4096, 4096]
    for name in SMALL_PRODUCTS:                                  # the furniture around every named row
        f = facts[name]
        empty_a, only_empty_b = f["a_len"] == 0, (f["a_len"] > 0) & (f["ub"] == 0)
        assert empty_a.any() and only_empty_b.any() and ((f["a_len"] == 1) & (f["ub"] == 1)).any() and (f["ub"] == 40).any(), name
        assert 0 < f["named"] < f["a_rows"] - 1 and f["a_len"][f["named"] + 1] > 0, name
    paths = {p: sorted(n for n, f in facts.items() if f["path"] == p) for p in ("hash", "direct", "fallback")}
    print(paths)
    assert paths["fallback"] == ["fallback-2049-8193"] and len(paths["direct"]) == 6 and len(paths["hash"]) == len(C.PRODUCTS) - 7


@pytest.mark.parametrize("name", [n for n in C.PRODUCTS if n.startswith("chain")])
def test_colliding_columns_hash_to_the_last_slot(name):
    assert C.last_slot_column(64) == 47 and int(C.hash_of(47 + 64 * 5, 63)) == 63
    c, f = C.product_case(name), _facts(name)
    size, columns = c["chain"]
    assert np.array_equal(f["named_columns"], columns) and (C.hash_of(columns, size - 1) == size - 1).all()
    if f["size"] != size:                                        # the larger table: two slots, `size` apart, and the upper one is the last
        assert set(C.hash_of(columns, f["size"] - 1).tolist()) == {size - 1, 2 * size - 1}
    # several steps: no row of B brings all the columns
    A, B = c["A"], c["B"]
    per_step = [B.indptr[k + 1] - B.indptr[k] for k in A.indices[A.indptr[c["named"]]:A.indptr[c["named"] + 1]]]
    assert len(per_step) >= 3 and max(per_step) < columns.size and sum(per_step) == f["n"]
    if f["n"] > f["d"]:
        assert f["m_max"] >= 2


def test_stride_cases_pair_rows_of_different_tables():
    c = C.product_case("stride-hash")
    A, B = c["A"], c["B"]
    ub = C.candidate_counts(A, B)
    cap, pairs = C.PRODUCT_GRID_CAP, C.STRIDE_PAIRS
    assert A.shape[0] == cap + pairs and (np.diff(A.indptr) == 1).all() and c["path"] == "hash"
    b_len = np.diff(B.indptr)
    assert B.shape[0] == 200 and set(b_len[0::2].tolist()) == {1, 2, 3} and (b_len[1::2] == 40).all()
    first = np.array([C.table_size(int(u)) for u in ub[:pairs]])
    second = np.array([C.table_size(int(u)) for u in ub[cap:cap + pairs]])
    assert (first != second).all() and set(first.tolist()) == {64, 128} == set(second.tolist())
    assert (first[:pairs // 2] == 64).all() and (first[pairs // 2:] == 128).all()          # both orders
    assert c["bits"].indices.size < 4_000_000 and np.array_equal(np.diff(c["bits"].indptr), ub)
    d = C.product_case("stride-direct")
    ub = C.candidate_counts(d["A"], d["B"])
    at = C.STRIDE_DIRECT_ROW
    assert d["path"] == "direct" and d["A"].shape[0] == cap + pairs + 1 and d["B"].shape[1] == 100
    assert ub[at] >= 2049 and (np.delete(ub, at) <= 40).all() and 0 < ub[at + cap] <= 40
    assert np.diff(d["bits"].indptr)[at] > 80 and np.diff(d["bits"].indptr)[at + cap] <= 40 and d["bits"].indices.size < 4_000_000
    # the same A, but for the one row
    assert np.array_equal(np.delete(d["A"].indices, np.arange(d["A"].indptr[at], d["A"].indptr[at + 1])), A.indices)


def test_transpose_cases_cover_every_sort_length():
    c = C.transpose_case("lengths")
    A = c["A"]
    counts = np.bincount(A.indices, minlength=A.shape[1])
    named = [C.named_column(i) for i in range(len(C.NAMED_COLUMN_COUNTS))]
    assert tuple(counts[named]) == C.NAMED_COLUMN_COUNTS == (0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096)
    assert A.shape[0] >= 4096 and np.delete(counts, named).max() <= 9 and c["path"] == "device"
    assert np.diff(A.indptr)[C.LENGTHS_DENSE_ROW] > 128                                      # the scatter walks a row in several steps
    # padded lengths of the workgroup sort: 128 for 65 .. 128, 256 for 129, 4096 for 4095 and 4096
    one_row, one_col, beyond = (C.transpose_case(n) for n in ("one-row-4096", "one-column-4096", "one-column-4097"))
    assert one_row["A"].shape == (1, 4096) and (np.diff(one_row["bits"].indptr) == 1).all() and one_row["path"] == "device"
    assert one_col["A"].shape == (4096, 1) and np.diff(one_col["bits"].indptr).tolist() == [C.K_MAX_SORT_ROW] and one_col["path"] == "device"
    assert np.diff(beyond["bits"].indptr).tolist() == [C.K_MAX_SORT_ROW + 1] and beyond["path"] == "fallback"
    s = C.transpose_case("stride")
    lengths = np.diff(s["bits"].indptr)
    assert s["A"].shape[0] > C.TRANSPOSE_WAVE_CAP == 262144 and s["A"].shape[1] > C.TRANSPOSE_WAVE_CAP and s["path"] == "device"
    assert (np.diff(s["A"].indptr) == 3).all() and 2 <= lengths.max() <= C.WAVE_SORT_MAX
    assert (lengths[C.TRANSPOSE_WAVE_CAP:] >= 2).any()                                       # rows the second pass of the sort reaches
    assert (s["A"].data == np.rint(s["A"].data)).all()
    for name in C.TRANSPOSES:                                                                # sorted, distinct columns in every input row
        A = C.transpose_case(name)["A"]
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        assert (np.diff(A.indices.astype(np.int64))[rows[1:] == rows[:-1]] > 0).all(), name


# ---- the comparator and the bound bite ----
def _copy(M):
    return C.CSR(M.indptr.copy(), M.indices.copy(), M.data.copy(), M.shape)


def _fails(got, want):
    with pytest.raises(AssertionError):
        C.assert_same_csr(got, want, "planted")
    return True


def _entry_terms(c, r, col):
    """The terms a b of entry (r, col) in the order of the Gustavson sum, rounded as the kernel rounds them."""
    A, B = c["A"], c["B"]
    out = []
    for p in range(A.indptr[r], A.indptr[r + 1]):
        k = A.indices[p]
        hit = np.flatnonzero(B.indices[B.indptr[k]:B.indptr[k + 1]] == col)
        if hit.size:
            out.append(A.data[p] * B.data[B.indptr[k] + hit[0]])
    return out


def test_references_agree_with_themselves():
    for name in FLOAT_PRODUCTS:
        c = C.product_case(name)
        bits, (pattern, want, mag, m) = c["bits"], c["long"]
        assert np.array_equal(bits.indptr, pattern.indptr) and np.array_equal(bits.indices, pattern.indices), name
        C.assert_same_csr(bits, bits, name)
        bad = C.beyond_product_bound(bits.data, want, mag, m)
        print(f"{name}: reference in double against long double, worst ratio {C.worst_ratio(bits.data, want, mag):.2f}, m <= {m.max()}")
        assert not bad.any(), name
        # the row loop against the list of terms, on integers: the same exact product from two formulations
        rng = np.random.default_rng(3)
        Ai, Bi = c["A"]._replace(data=C.small_integers(rng, c["A"].data.size)), c["B"]._replace(data=C.small_integers(rng, c["B"].data.size))
        C.assert_same_csr(C.product_reference_bits(Ai, Bi), C.product_reference_int(Ai, Bi), name)
    for name in C.TRANSPOSES:
        c = C.transpose_case(name)
        C.assert_same_csr(C.transpose_reference(c["bits"]), c["A"], name)
    # an entry of the reference is the sum of its terms in storage order
    c = C.product_case("direct-100")
    r = c["named"]
    q = c["bits"].indptr[r] + 3
    terms = _entry_terms(c, r, c["bits"].indices[q])
    acc = 0.0
    for t in terms:
        acc = acc + t
    assert len(terms) == c["long"][3][q] and acc == c["bits"].data[q]


def test_planted_defects_of_the_product_are_noticed():
    c = C.product_case("direct-100")
    want, (_, ref, mag, m) = c["bits"], c["long"]
    r = c["named"]
    lo, hi = want.indptr[r], want.indptr[r + 1]
    within = lambda got: not C.beyond_product_bound(got.data, ref, mag, m).any()
    assert within(want)
    # one entry summed in reverse term order: other bits, and still a correctly rounded sum
    planted = None
    for q in range(lo, hi):
        terms = _entry_terms(c, r, want.indices[q])
        back = 0.0
        for t in reversed(terms):
            back = back + t
        if back != want.data[q]:
            planted = _copy(want)
            planted.data[q] = back
            break
    assert planted is not None and _fails(planted, want) and within(planted)
    # a duplicate column left as two entries
    q = lo + int(np.flatnonzero(m[lo:hi] >= 2)[0])
    terms = _entry_terms(c, r, want.indices[q])
    two = C.CSR(np.concatenate([want.indptr[:r + 1], want.indptr[r + 1:] + 1]).astype(np.int32), np.insert(want.indices, q, want.indices[q]),
                np.insert(want.data, q, terms[0]), want.shape)
    two.data[q + 1] = want.data[q] - terms[0]
    assert _fails(two, want)
    # ... and the same with the row lengths of the correct result (the entry behind pushed out of the row): the columns do not increase
    two_same_length = C.CSR(want.indptr.copy(), np.delete(two.indices, hi), np.delete(two.data, hi), want.shape)
    assert _fails(two_same_length, want)
    # two neighbouring columns swapped with their values
    swapped = _copy(want)
    swapped.indices[[q, q + 1]], swapped.data[[q, q + 1]] = want.indices[[q + 1, q]], want.data[[q + 1, q]]
    assert _fails(swapped, want)
    # keys sorted, values left in place (here: where a table of 128 slots would have held them)
    moved = _copy(want)
    moved.data[lo:hi] = want.data[lo:hi][np.argsort(C.hash_of(want.indices[lo:hi], 127), kind="stable")]
    assert _fails(moved, want) and not within(moved)
    # a stale table: a value of the row before added to the next row; a column of the row before left in the next row
    stale = _copy(want)
    stale.data[lo] += want.data[want.indptr[r - 1]]
    assert want.indptr[r - 1] < lo and _fails(stale, want) and not within(stale)
    short = c["forty"] + 1 if c["forty"] + 1 != r else c["forty"] - 1
    extra_col = np.setdiff1d(want.indices[want.indptr[c["forty"]]:want.indptr[c["forty"] + 1]],
                             want.indices[want.indptr[short]:want.indptr[short + 1]])[-1]
    at = want.indptr[short] + np.searchsorted(want.indices[want.indptr[short]:want.indptr[short + 1]], extra_col)
    left = C.CSR(np.concatenate([want.indptr[:short + 1], want.indptr[short + 1:] + 1]).astype(np.int32),
                 np.insert(want.indices, at, extra_col), np.insert(want.data, at, 1.0), want.shape)
    assert _fails(left, want)


@pytest.mark.parametrize("name", FLOAT_PRODUCTS)
def test_an_entry_off_by_four_gamma_is_beyond_the_bound(name):
    c = C.product_case(name)
    want, (_, ref, mag, m) = c["bits"], c["long"]
    for q in {0, int(np.argmax(m)), int(np.argmin(mag)), want.data.size - 1}:
        got = want.data.copy()
        got[q] += float(4 * C.gamma(m[q]) * mag[q])
        bad = C.beyond_product_bound(got, ref, mag, m)
        assert bad[q] and bad.sum() == 1, (name, q, int(m[q]))
        got[q] = np.nan                                          # an entry nobody wrote
        assert C.beyond_product_bound(got, ref, mag, m)[q]


def test_planted_defects_of_the_transpose_are_noticed():
    c = C.transpose_case("lengths")
    want = c["bits"]
    r = C.named_column(C.NAMED_COLUMN_COUNTS.index(4096))
    lo, hi = want.indptr[r], want.indptr[r + 1]
    assert hi - lo == 4096
    # the last entry of the 4096-long row dropped
    dropped = C.CSR(np.concatenate([want.indptr[:r + 1], want.indptr[r + 1:] - 1]).astype(np.int32), np.delete(want.indices, hi - 1),
                    np.delete(want.data, hi - 1), want.shape)
    assert _fails(dropped, want)
    # ... or replaced by the padding of the sort
    padded = _copy(want)
    padded.indices[hi - 1], padded.data[hi - 1] = np.iinfo(np.int32).max, 0.0
    assert _fails(padded, want)
    # a row left as the scatter wrote it (any order), a row with keys sorted and values left in place, one exchange of the network missed
    for r in (C.named_column(i) for i, k in enumerate(C.NAMED_COLUMN_COUNTS) if k >= 2):
        lo, hi = want.indptr[r], want.indptr[r + 1]
        order = np.roll(np.arange(hi - lo), 1)
        unsorted, moved, missed = _copy(want), _copy(want), _copy(want)
        unsorted.indices[lo:hi], unsorted.data[lo:hi] = want.indices[lo:hi][order], want.data[lo:hi][order]
        moved.data[lo:hi] = want.data[lo:hi][order]
        missed.indices[[hi - 2, hi - 1]], missed.data[[hi - 2, hi - 1]] = want.indices[[hi - 1, hi - 2]], want.data[[hi - 1, hi - 2]]
        assert _fails(unsorted, want) and _fails(moved, want) and _fails(missed, want)
    # the values are moved bit for bit: a sign of zero or one ulp is a difference
    ulp = _copy(want)
    ulp.data[5] = np.nextafter(ulp.data[5], np.inf)
    assert _fails(ulp, want)


def test_spmv_bound_of_the_usability_check():
    c = C.transpose_case("lengths")
    T = c["bits"]
    x = C.vector_for("lengths", T.shape[1])
    want, mag, length = C.spmv_long(T, x)
    got = np.array([np.dot(T.data[T.indptr[i]:T.indptr[i + 1]], x[T.indices[T.indptr[i]:T.indptr[i + 1]]]) for i in range(T.shape[0])])
    assert not C.beyond_spmv_bound(got, want, mag, length).any() and length.max() == 4096
    assert (got[length == 0] == 0).all()
    r = C.named_column(C.NAMED_COLUMN_COUNTS.index(4096))
    terms = T.data[T.indptr[r]:T.indptr[r + 1]] * x[T.indices[T.indptr[r]:T.indptr[r + 1]]]
    got[r] -= terms[np.argmax(np.abs(terms))]                                                # one entry of the long row left out
    got[3] = np.nan
    assert np.flatnonzero(C.beyond_spmv_bound(got, want, mag, length)).tolist() == [3, r]
