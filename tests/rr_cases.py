"""Cases of the one-pass residual restriction b_c = R (A x - b) (residual_restriction.hip) for test_rr_case_table.py (no GPU) and
test_gpu_residual_restriction.py: the case table, the host's planning of a launch restated in plain Python, the long-double
reference with its magnitude sum per row, and the results a wrong tile march would write.

A case is (mesh, MFMG_RR_TILE_LAYERS).  Cells are twice the agglomerates per axis; na = agglomerates, N = 2 na + 1 nodes.

Planning (build_residual_restriction, residual_restriction_grid): lanes 1 .. 62 of a wavefront own a run of up to 62 agglomerates
i = 1 .. main_last of one agglomerate row (j, k); a last run shorter than 24 stays in the list with i = 0 and i = na0 - 1; a run
whose agglomerates do not share a class goes to the list too (0xffff in seg_class).  The tile form gives eight agglomerate rows
j to a workgroup, which marches through `ka` agglomerate layers k = 2 ka + 3 node layers."""
import functools

import numpy as np

import mfmg_oracle as O
from test_gpu_fp32_fine_level import K_RR     # gamma_256: derived there

LD = np.longdouble
U64 = 2.0 ** -53
RUN, SHORTEST_RUN, TILE_ROWS = 62, 24, 8
N_CUS = 256                                   # compute units of an MI355X

# ---- the meshes: name -> (cells, material, heights); test_rr_case_table.py names the edges each case is there for ----
# "rows": one coefficient per agglomerate row (j, k), constant along x, drawn from [1, 10) -- every agglomerate row is a class of
# its own (the weights diag_loc / diag_glob of R see the neighbouring rows as well), so the agglomerate layers P, C, N of a
# wavefront and the eight wavefronts of a tile all read different tables -- with ONE cell changed, ROWS_CELL: the left lower
# front cell of agglomerate (31, 4, 2), in the middle of the first run.  It is a corner cell of the 4 x 4 x 4 cells around the
# agglomerates (30 .. 31, 3 .. 4, 1 .. 2) and of no others: the first runs of rows j = 3, 4 in layers k = 1, 2 are not uniform
# and go to the list, the rows j = 0 .. 2 and 5 .. 7 of the same tile stay in the row-wise part, and so do rows 3, 4 in layers 0, 3, 4.
ROWS_CELL = (62, 8, 4)
MESHES = {
    "24": ((52, 4, 14), "constant", (1, 2, 3, 4, 7)),
    "23": ((50, 6, 6), "constant", (1, 3)),
    "62": ((128, 34, 6), "constant", (1, 2, 3)),
    "63": ((130, 16, 8), "constant", (2, 3, 4)),
    "62+24": ((176, 18, 10), "constant", (1, 2, 5)),
    "rows": ((176, 34, 10), "rows", (1, 2, 5)),
}
CASES = [(name, h) for name, (_, _, heights) in MESHES.items() for h in heights]


def case_id(case):
    name, h = case
    return "x".join(map(str, MESHES[name][0])) + f"-{MESHES[name][1]}-height{h}"


def agglomerates(cells):
    assert all(c % 2 == 0 for c in cells)
    return tuple(c // 2 for c in cells)


@functools.lru_cache(maxsize=None)
def coefficient(name):
    """Coefficient table [cell][quadrature point] of a mesh, float64."""
    cells, material, _ = MESHES[name]
    mesh = O.StructuredMesh(cells)
    if material == "constant":
        return O.coefficient_table(mesh, "constant")
    assert material == "rows"
    na = agglomerates(cells)
    per_row = np.random.default_rng(20).uniform(1.0, 10.0, (na[2], na[1]))
    assert np.unique(per_row).size == per_row.size
    c = np.repeat(np.repeat(per_row, 2, axis=0), 2, axis=1)[:, :, None] * np.ones(cells[0])          # [z][y][x]
    cx, cy, cz = ROWS_CELL
    c[cz, cy, cx] *= 0.5
    return np.ascontiguousarray(np.repeat(c.reshape(-1, 1), 8, axis=1))


def nonuniform_runs(cells, coef, segs, main_last):
    """Runs (k, j, run) along which the rows of R A do not repeat: the 4 x 4 x 4 cells around an agglomerate (those that touch both
    its 3^3 nodes and the 5^3 nodes of its rows of R A; -1 outside the box) differ from those around the first of the run."""
    assert (coef == coef[:, :1]).all()
    nx, ny, nz = cells
    p = np.pad(coef[:, 0].reshape(nz, ny, nx), 1, constant_values=-1.0)
    win = np.lib.stride_tricks.sliding_window_view(p, (4, 4, 4))[::2, ::2, ::2]
    na = agglomerates(cells)
    assert win.shape[:3] == na[::-1]
    out = set()
    for sg in range(segs):
        i0, i1 = 1 + sg * RUN, min(main_last, sg * RUN + RUN)
        blocks = win[:, :, i0:i1 + 1].reshape(na[2], na[1], i1 - i0 + 1, 64)
        differ = (blocks != blocks[:, :, :1]).any(axis=(2, 3))
        out |= {(int(k), int(j), sg) for k, j in zip(*np.nonzero(differ))}
    return out


def automatic_height(segs, tiles_j, na2, n_cus=N_CUS):
    """The height residual_restriction_grid chooses: whole rounds of two workgroups per CU, 2 t + 3 node layers per round."""
    ka, best = 0, 0.0
    for nk in range(1, na2 + 1):
        t = -(-na2 // nk)
        if -(-na2 // t) != nk:
            continue
        tiles, slots = segs * tiles_j * nk, 2 * n_cus
        cost = float(-(-tiles // slots)) * (2.0 * t + 3.0)
        if ka == 0 or cost < best:
            ka, best = t, cost
    return max(ka, 1)


def plan(name, height, kernel="tile", n_cus=N_CUS):
    """What Hierarchy.residual_restriction_form() must report for a mesh built with MFMG_RR_TILE_LAYERS=height (0: unset) and
    MFMG_RR_KERNEL=kernel, and what the test table needs to know about the tiles (`layers`: agglomerate layers of the tiles of
    one column; `live_rows`: agglomerate rows of each tile along y)."""
    cells = MESHES[name][0]
    na = agglomerates(cells)
    interior = max(na[0] - 2, 0)
    segs = interior // RUN + (1 if interior % RUN >= SHORTEST_RUN else 0)
    main_last = min(interior, segs * RUN)
    tail = na[0] - 1 - main_last                               # agglomerates i > main_last of a row, the last one included
    runs = [min(main_last, sg * RUN + RUN) - sg * RUN for sg in range(segs)]
    listed_runs = nonuniform_runs(cells, coefficient(name), segs, main_last)
    listed = na[1] * na[2] * (1 + tail) + sum(runs[sg] for _, _, sg in listed_runs)
    waves = segs * na[1] * na[2]
    out = {"cells": cells, "na": na, "interior": interior, "segs": segs, "main_last": main_last, "tail": tail, "runs": runs,
           "listed": listed, "listed_runs": len(listed_runs), "listed_run_set": listed_runs, "kernel": kernel,
           "n_agg": na[0] * na[1] * na[2], "n_dofs": int(np.prod([c + 1 for c in cells]))}
    if kernel == "rows":
        out.update(tile_layers=0, tiles_j=0, n_tiles=0, layers=[], live_rows=[],
                   main_blocks=-(-(-(-waves // 4)) // 8) * 8 if waves else 0)
        return out
    tiles_j = -(-na[1] // TILE_ROWS)
    ka = min(height, na[2]) if height > 0 else automatic_height(segs, tiles_j, na[2], n_cus)
    layers = [min(ka, na[2] - t * ka) for t in range(-(-na[2] // ka))]
    n_tiles = segs * tiles_j * len(layers)
    out.update(tile_layers=ka, tiles_j=tiles_j, n_tiles=n_tiles, layers=layers,
               live_rows=[min(TILE_ROWS, na[1] - t * TILE_ROWS) for t in range(tiles_j)],
               main_blocks=-(-n_tiles // 8) * 8 if waves else 0)
    return out


FORM_KEYS = ("kernel", "tile_layers", "segs", "main_last", "listed", "listed_runs", "tiles_j", "n_tiles", "main_blocks")


def expected_form(name, height, kernel="tile", n_cus=N_CUS):
    p = plan(name, height, kernel, n_cus)
    return {k: p[k] for k in FORM_KEYS}


# ---- the reference ----
def spmv_long(M, v):
    """M v and |M| |v| per row in long double (M in COO)."""
    prod = M.data.astype(LD) * v[M.col]
    out, mag = np.zeros(M.shape[0], dtype=LD), np.zeros(M.shape[0], dtype=LD)
    np.add.at(out, M.row, prod)
    np.add.at(mag, M.row, np.abs(prod))
    return out, mag


@functools.lru_cache(maxsize=None)
def fine_operator(name):
    """A as the matrix-free operator applies it, assembled by the oracle from the mesh's own coefficient table: constrained rows
    are identities (as in test_residual_restriction_on_float_vectors)."""
    mesh = O.StructuredMesh(MESHES[name][0])
    A = O.assemble_csr(mesh, coefficient(name)).tolil()
    A.setdiag(np.where(mesh.constrained_mask(), 1.0, A.diagonal()))
    return A.tocoo()


def reference(name, R, x, b):
    """R (A x - b) in long double and the magnitude sum |R| (|A| |x| + |b|) per row."""
    A, R = fine_operator(name), R.tocoo()
    ax, amag = spmv_long(A, np.asarray(x).astype(LD))
    want, _ = spmv_long(R, ax - np.asarray(b).astype(LD))
    _, mag = spmv_long(R, amag + np.abs(np.asarray(b)).astype(LD))
    return want, mag


def gamma(k=K_RR):
    return k * U64 / (1 - k * U64)


def beyond(got, want, mag):
    """Rows outside gamma_256 mag; NaN (a row nobody wrote) counts as outside."""
    return ~(np.abs(np.asarray(got).astype(LD) - want) <= gamma() * mag)


def worst_ratio(got, want, mag):
    ok = mag > 0
    return float((np.abs(np.asarray(got).astype(LD) - want)[ok] / (U64 * mag[ok])).max()) if ok.any() else 0.0


def data_sets(name, n, single=False):
    """Two (x, b): standard normal, and the same kind with the entries spread over 16 decades (float32 values with `single`)."""
    rng = np.random.default_rng([5, int(single), *MESHES[name][0]])
    out = []
    for scale in (False, True):
        x, b = rng.standard_normal(n), rng.standard_normal(n)
        if scale:
            x, b = x * 10.0 ** rng.uniform(-8, 8, n), b * 10.0 ** rng.uniform(-8, 8, n)
        if single:
            x, b = x.astype(np.float32), b.astype(np.float32)
        out.append((x, b))
    return out


# ---- what a wrong march writes ----
PLANTS = ("node_layer_left_out", "x_sums_of_two_layers_exchanged", "b_of_the_middle_node_layer_dropped", "written_one_layer_too_high",
          "table_of_the_layer_below", "row_shifted_by_one_node_in_x")


def planted(name, R, x, b, want, plant, K=1):
    """The result (float64) of a march with one defect in agglomerate layer K, from the long-double reference `want`: the sums of
    a row of R A and of R are split by node layer / shifted the way the defect would, the difference is added to the reference.
    Returns the result and the coarse rows the defect touches.  plant None: the reference rounded to double."""
    cells = MESHES[name][0]
    na, N = agglomerates(cells), tuple(c + 1 for c in cells)
    assert 1 <= K and K + 1 < na[2]
    A = fine_operator(name)
    RA, Rc = (R.tocsr() @ A.tocsr()).tocoo(), R.tocoo()
    x, b = np.asarray(x).astype(LD), np.asarray(b).astype(LD)
    layer_rows = 2 * na[0] * na[1]                              # coarse rows of an agglomerate layer
    plane = N[0] * N[1]
    rows_of = lambda k: np.arange(k * layer_rows, (k + 1) * layer_rows)

    def sums(M, v, keep=None, shift=0):
        keep = np.ones(M.nnz, dtype=bool) if keep is None else keep
        out = np.zeros(M.shape[0], dtype=LD)
        np.add.at(out, M.row[keep], M.data[keep].astype(LD) * v[M.col[keep] + shift])
        return out

    got, touched = want.copy(), rows_of(K)
    in_K = lambda M: M.row // layer_rows == K
    if plant == "node_layer_left_out":                          # the middle node layer 2 K + 1 of layer K: its x and its b
        mid = lambda M: in_K(M) & (M.col // plane == 2 * K + 1)
        got -= sums(RA, x, mid(RA)) - sums(Rc, b, mid(Rc))
    elif plant == "x_sums_of_two_layers_exchanged":             # Cs and Ns rotated the wrong way round
        xs = sums(RA, x)
        lo, hi = rows_of(K), rows_of(K + 1)
        got[lo] += xs[hi] - xs[lo]
        got[hi] += xs[lo] - xs[hi]
        touched = np.concatenate([lo, hi])
    elif plant == "b_of_the_middle_node_layer_dropped":
        got += sums(Rc, b, in_K(Rc) & (Rc.col // plane == 2 * K + 1))
    elif plant == "written_one_layer_too_high":                 # akP one too large: every layer lands on the next one
        got[layer_rows:] = want[:-layer_rows]
        touched = np.arange(layer_rows, want.size)
    elif plant == "table_of_the_layer_below":                   # the weights of layer K - 1 on the nodes of layer K
        below = lambda M: M.row // layer_rows == K - 1
        wrong = sums(RA, x, below(RA), 2 * plane) - sums(Rc, b, below(Rc), 2 * plane)
        right = sums(RA, x, in_K(RA)) - sums(Rc, b, in_K(Rc))
        got[rows_of(K)] += wrong[rows_of(K - 1)] - right[rows_of(K)]
    elif plant == "row_shifted_by_one_node_in_x":               # the five nodes 2 i .. 2 i + 4 instead of 2 i - 1 .. 2 i + 3
        ai = (RA.row // 2) % na[0]
        keep = in_K(RA) & (ai >= 1) & (ai <= na[0] - 2)
        got += sums(RA, x, keep, 1) - sums(RA, x, keep)
        touched = touched[((touched // 2) % na[0] >= 1) & ((touched // 2) % na[0] <= na[0] - 2)]
    else:
        assert plant is None
    return got.astype(np.float64), touched
