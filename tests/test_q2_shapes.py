"""The mesh list of the Q2 operator test (q2_cases.py) reaches the edges it names, computed from the tile shapes the library
reports (mfmg_hip_mf_laplace_q2_tile_shapes; no GPU needed)."""
import mfmg_amd as M
from q2_cases import MAX_CELLS, n_tiles, q2_meshes


def test_tile_shapes_are_reported(mfmg_lib):
    shapes = M.q2_tile_shapes()
    assert len(shapes) >= 1 and len(set(shapes)) == len(shapes)
    for tx, ty, tz in shapes:
        # one lane per cell of the tile and of its low halo: whole wavefronts, at most 256 lanes
        assert tx >= 1 and ty >= 1 and tz >= 1
        assert ((tx + 1) * (ty + 1)) % 64 == 0 and (tx + 1) * (ty + 1) <= 256


def test_mesh_list_reaches_the_edges(mfmg_lib):
    tile = M.q2_tile_shapes()[0]
    meshes = q2_meshes(tile)
    sizes = [n for _, n, _, _ in meshes]
    for n in ((1, 1, 1), (2, 1, 3), (3, 2, 4)):
        assert n in sizes
    for d in range(3):
        along = {n[d] for n in sizes}
        # one fewer than, equal to and one more than the tile: the last tile full, one short, and a second tile of one cell
        assert {tile[d] - 1, tile[d], tile[d] + 1} <= along, (d, along)
    assert 2 * tile[2] + 1 in {n[2] for n in sizes}            # three z-tiles, the last of one layer
    assert max(n_tiles(n, tile)[2] for n in sizes) == 3
    # a mesh with more than one tile along every axis at once (interior halo cells on all three low faces)
    assert any(min(n_tiles(n, tile)) >= 2 for n in sizes)
    # a single workgroup with idle lanes in x and in y, and a mesh narrower than the halo column
    assert (1, 1, 1) in sizes
    assert any(h is not None and len(set(h)) == 3 for _, _, h, _ in meshes)
    assert any(not dirichlet for _, _, _, dirichlet in meshes)
    for n in sizes:
        assert all(n[d] <= MAX_CELLS[d] for d in range(3)), n


def test_every_offered_tile_cuts_some_mesh_differently(mfmg_lib):
    """the equal-bits check across tiles compares different decompositions on at least one mesh"""
    shapes = M.q2_tile_shapes()
    sizes = [n for _, n, _, _ in q2_meshes(shapes[0])]
    for other in shapes[1:]:
        assert any(n_tiles(n, other) != n_tiles(n, shapes[0]) for n in sizes)
