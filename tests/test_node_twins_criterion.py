"""The matrices of tests/test_gpu_node_twins.py and the twin criterion of SparseMatrixDevice::enable_node_twins, restated.

`pt_like` builds a rectangular matrix shaped like a smoothed prolongator: a fine grid of nx x ny x nz nodes with C
unknowns each, a coarse grid of the halves (rounded up), every fine node coupled to the 3 x 3 x 3 coarse nodes around
(floor(i / 2), floor(j / 2), floor(k / 2)), clipped at the box.  The C x 27 x C values of a node are a function of its
KEY -- the parity of (i, j, k) and, per axis, the distance of its coarse node to the two faces (capped at 1, or exact
along the axes named in `exact`) --, drawn per key as standard_normal * 10 ** uniform(-3, 3): nodes of one key repeat one
tuple, which is what build_node_classes sorts into classes.  `perturb` nodes get values of their own (they match no class
and become listed rows).

`twin_counts` restates what the library does with such a matrix (no GPU): a key with at least 8 unperturbed members is a
class (kMinClass), the base of a node is its lowest coarse neighbour, a twin is (n, n + 1) with n even, both nodes classed
and equal bases, and the layout is taken when twins hold at least 90 % of the classed nodes.  The GPU test derives the
range of form()["twin_slots"] from these counts; the tests here show that the shapes it uses produce the cases it names."""
import numpy as np
import pytest
import scipy.sparse as sp

MIN_CLASS = 8          # kMinClass of build_node_classes
TWIN_TILE = 4096       # twins per tile of enable_node_twins (the smallest tile: the most padding)

# (id, dims, C, exact axes, perturbed nodes): the shapes of the GPU test, the smallest that still take node classes
# (n_rows >= 32768)
SHAPES = [
    ("c2_all_twins", (32, 24, 22), 2, (), 0),
    ("c2_odd_nx", (33, 24, 22), 2, (), 0),
    ("c1", (40, 32, 26), 1, (), 0),
    ("c2_padding_only", (80, 16, 16), 2, (1, 2), 0),
    ("c2_listed_1", (32, 24, 22), 2, (), 1),
    ("c2_listed_17", (32, 24, 22), 2, (), 17),
    ("c2_listed_65", (32, 24, 22), 2, (), 65),
]
SHAPE_IDS = [s[0] for s in SHAPES]


def grids(dims):
    nx, ny, nz = dims
    n = np.arange(nx * ny * nz)
    fine = np.stack([n % nx, (n // nx) % ny, n // (nx * ny)], axis=1)
    cdims = np.array([(nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2])
    return fine, cdims


def node_keys(dims, exact=()):
    """One integer per fine node: parity and the (capped or exact) distances of its coarse node to the faces."""
    fine, cdims = grids(dims)
    coarse = fine // 2
    key = np.zeros(len(fine), dtype=np.int64)
    for ax in range(3):
        lo, hi = coarse[:, ax], cdims[ax] - 1 - coarse[:, ax]
        if ax not in exact:
            lo, hi = np.minimum(lo, 1), np.minimum(hi, 1)
        key = ((key * 2 + fine[:, ax] % 2) * (cdims[ax] + 1) + lo) * (cdims[ax] + 1) + hi
    return key


def perturbed_nodes(dims, perturb, seed):
    n_nodes = int(np.prod(dims))
    return np.sort(np.random.default_rng(seed + 1000).choice(n_nodes, size=perturb, replace=False)) if perturb else np.zeros(0, dtype=np.int64)


def pt_like(dims, c, exact=(), perturb=0, seed=0):
    rng = np.random.default_rng(seed)
    fine, cdims = grids(dims)
    n_nodes = len(fine)
    keys = node_keys(dims, exact)
    uniq, cls = np.unique(keys, return_inverse=True)
    table = rng.standard_normal((len(uniq), c, 27, c)) * 10.0 ** rng.uniform(-3, 3, (len(uniq), c, 27, c))
    coarse = fine // 2
    own = perturbed_nodes(dims, perturb, seed)
    scale = np.ones(n_nodes)
    scale[own] = 1.0 + (1 + np.arange(len(own))) / 1024.0   # (exact factors: every perturbed node a tuple of its own)
    rows, cols, vals = [], [], []
    for d in range(27):
        off = np.array([d % 3 - 1, (d // 3) % 3 - 1, d // 9 - 1])
        nb = coarse + off
        ok = np.all((nb >= 0) & (nb < cdims), axis=1)
        cn = nb[:, 0] + cdims[0] * (nb[:, 1] + cdims[1] * nb[:, 2])
        nd = np.nonzero(ok)[0]
        for rc in range(c):
            for cc in range(c):
                rows.append(nd * c + rc)
                cols.append(cn[nd] * c + cc)
                vals.append(table[cls[nd], rc, d, cc] * scale[nd])
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(n_nodes * c, int(np.prod(cdims)) * c)).tocsr()
    A.sort_indices()
    return A


def twin_counts(dims, exact=(), perturb=0, seed=0):
    """What enable_node_twins must find: classed nodes, twins, single nodes, twin classes, taken or not."""
    fine, cdims = grids(dims)
    n_nodes = len(fine)
    keys = node_keys(dims, exact)
    plain = np.ones(n_nodes, dtype=bool)
    plain[perturbed_nodes(dims, perturb, seed)] = False
    uniq, cls, members = np.unique(np.where(plain, keys, -1), return_inverse=True, return_counts=True)
    classed = plain & (members[cls] >= MIN_CLASS)
    lowest = np.maximum(fine // 2 - 1, 0)
    base = lowest[:, 0] + cdims[0] * (lowest[:, 1] + cdims[1] * lowest[:, 2])
    n = np.arange(0, n_nodes - 1, 2)
    twin = classed[n] & classed[n + 1] & (base[n] == base[n + 1])
    n_twins, n_classed = int(twin.sum()), int(classed.sum())
    first = n[twin]
    twin_classes = len(set(zip(cls[first].tolist(), cls[first + 1].tolist())))
    tiles = -(-n_nodes // (2 * TWIN_TILE))
    return {"nodes": n_nodes, "classed": n_classed, "listed_nodes": n_nodes - n_classed, "twins": n_twins,
            "singles": n_classed - 2 * n_twins, "twin_classes": twin_classes,
            "largest_twin_class": int(np.unique(cls[first], return_counts=True)[1].max()) if n_twins else 0,
            "taken": n_twins > 0 and 20 * n_twins >= 9 * n_classed,
            # every run of a twin class inside a tile is padded to a wavefront: at most 63 slots per run
            "twin_slots": (-(-n_twins // 64) * 64, n_twins + 63 * twin_classes * tiles)}


@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_shapes_take_node_classes(sid):
    _, dims, c, exact, perturb = SHAPES[SHAPE_IDS.index(sid)]
    t = twin_counts(dims, exact, perturb)
    assert t["nodes"] * c >= 32768                      # choose_layouts looks for node classes from here
    assert 10 * t["classed"] >= 9 * t["nodes"]          # the format is used when 90 % of the nodes are in classes
    n_classes = int((np.unique(node_keys(dims, exact), return_counts=True)[1] >= MIN_CLASS).sum())
    assert n_classes < 1024 and t["classed"] >= 32 * n_classes   # (few, populated classes: tables that stay in the caches)


def test_even_nx_every_classed_node_is_a_twin():
    t = twin_counts((32, 24, 22))
    assert t["taken"] and t["singles"] == 0 and 2 * t["twins"] == t["classed"]
    # the eight fine nodes of a corner aggregate are eight keys of one member: listed, never classed
    assert t["listed_nodes"] == 64
    t = twin_counts((40, 32, 26))
    assert t["taken"] and t["singles"] == 0


def test_odd_nx_has_twins_and_singles():
    """33 nodes per row: in the rows that start at an odd node an even n is an odd i, whose neighbour belongs to the next
    aggregate (another base), and the last column (i = 32) has no partner."""
    t = twin_counts((33, 24, 22))
    assert t["twins"] > 0 and t["singles"] > 0
    assert abs(2 * t["twins"] - t["singles"]) < 0.1 * t["classed"]   # about half of the rows keep their twins
    assert not t["taken"]                                               # ... so the matrix declines (90 % rule)


def test_padding_only_shape_keeps_every_twin_class_below_a_wavefront():
    t = twin_counts((80, 16, 16), exact=(1, 2))
    assert t["taken"] and 0 < t["largest_twin_class"] < 64
    assert t["twin_slots"][0] < 64 * t["twin_classes"]   # (not every class fills even one wavefront)


@pytest.mark.parametrize("perturb", [1, 17, 65])
def test_perturbed_nodes_are_listed_and_break_their_twin(perturb):
    plain, t = twin_counts((32, 24, 22)), twin_counts((32, 24, 22), perturb=perturb)
    assert t["taken"]
    assert t["listed_nodes"] >= plain["listed_nodes"] + perturb - 64   # (a perturbed corner node was listed before)
    assert t["listed_nodes"] <= plain["listed_nodes"] + perturb
    assert 0 < plain["twins"] - t["twins"] <= perturb
    assert t["singles"] > 0                                            # the partner of a perturbed node stays single


def test_generator_couples_what_it_claims():
    A = pt_like((6, 4, 5), 2)
    fine, cdims = grids((6, 4, 5))
    assert A.shape == (120 * 2, 3 * 2 * 3 * 2)
    per_axis = [np.minimum(fine[:, ax] // 2 + 1, cdims[ax] - 1) - np.maximum(fine[:, ax] // 2 - 1, 0) + 1 for ax in range(3)]
    want = np.repeat(per_axis[0] * per_axis[1] * per_axis[2] * 2, 2)
    assert np.array_equal(np.diff(A.indptr), want)
    # nodes of one key repeat their values; a perturbed node does not
    W = pt_like((16, 12, 10), 2)
    keys = node_keys((16, 12, 10))
    a, b = np.nonzero(keys == keys[6 + 16 * (5 + 12 * 4)])[0][:2]   # an interior key: several aggregates carry it
    assert a != b and np.array_equal(W[2 * a].data, W[2 * b].data) and np.array_equal(W[2 * a + 1].data, W[2 * b + 1].data)
    B = pt_like((6, 4, 5), 2, perturb=3)
    own = perturbed_nodes((6, 4, 5), 3, 0)
    assert all(not np.array_equal(A[2 * n].data, B[2 * n].data) for n in own)
    assert (A != B).nnz == sum(A[2 * n].nnz + A[2 * n + 1].nnz for n in own)
