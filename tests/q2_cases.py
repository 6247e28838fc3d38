"""The meshes the Q2 operator kernel is tested on (test_gpu_q2_operator.py), built from the default tile (tx, ty, tz) in cells the
library reports, and the edges they are meant to reach (test_q2_shapes.py checks that they do)."""

MAX_CELLS = (33, 17, 9)


def q2_meshes(tile):
    """[(name, n_cells, cell_size or None, dirichlet)]"""
    tx, ty, tz = tile
    cases = [("one cell", (1, 1, 1), None, True), ("2x1x3", (2, 1, 3), None, True), ("3x2x4", (3, 2, 4), None, True)]
    for k, v in (("tx-1", tx - 1), ("tx", tx), ("tx+1", tx + 1)):
        cases.append((f"x {k}", (v, 2, 2), None, True))
    for k, v in (("ty-1", ty - 1), ("ty", ty), ("ty+1", ty + 1)):
        cases.append((f"y {k}", (2, v, 2), None, True))
    for k, v in (("tz-1", tz - 1), ("tz", tz), ("2tz+1", 2 * tz + 1)):
        cases.append((f"z {k}", (2, 2, v), None, True))
    cases.append(("three cell sizes", (3, 2, 4), (0.1, 0.25, 0.05), True))
    cases.append(("no Dirichlet faces", (3, 3, 2), None, False))
    cases.append(("tiles along every axis", (tx + 1, ty + 1, tz + 1), None, True))
    return cases


def n_tiles(n, tile):
    return tuple((n[d] + tile[d] - 1) // tile[d] for d in range(3))
