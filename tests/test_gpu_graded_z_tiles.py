"""The graded z-tiling of the matrix-free operator on small meshes, entry by entry against long double.

In production the one-term kernel (mf_laplace.hip, a whole-mesh launch) and the block kernel (mf_laplace_block.hip, every launch)
do not cut z into tiles of tz layers: they read the table of mf_z_tiles (mf_z_tiles.hpp, tests/test_mf_z_tiles.py) through
`ztab`, 8 m tiles whose heights fall off linearly within every eighth of the layers -- some one layer high, some taller than tz.
The other long-double modules stop at 23 node layers (10 for the block kernels), where that table has one tile per eighth; here
the meshes are the smallest that reach m = 2, 3 and 4, a tile taller than tz, one-layer tiles, a second chunk column of a few
nodes and the tail slab that shares the table of its launch:

  id  cells        layers  tile (nw, ty, tz)       m  heights per eighth
  G1  (12,10,32)   33      the default, (2,3,8)    2  3, 1 (last eighth 3, 2): one-layer tiles
  G2  (6,5,56)     57      (2,2,3)                 3  1 .. 4: the smallest mesh with a tile taller than tz
  G3  (20,17,96)   97      (4,2,4)                 4  5, 3, 3, 1 (last 5, 4, 2, 2): taller than tz and one layer in one table
  G4  (6,5,158)    159     (2,3,8)                 3  9, 6, 4 and 9, 7, 4
  G5  (64,18,32)   33      (2,2,4)                 2  3, 1; 65 node columns: a second chunk column of 3 (halo 1) or 7 (halo 3) nodes
  G6  (65,70,31)   32      (2,2,4)                 2  3, 1; one halo lane, 66 node columns, 71 rows: the 4 tail columns run as the
                                                      rotated slab inside the same launch, on the same table

The default tile of the one-term operator on G1 and of the block operator on G3 is (1, 2, 4) on an MI355X (no tile of the lists
gives 256 compute units two rounds on meshes this small, so the last one is taken); tz = 4 grades at 33 and at 97 layers.

Every case first asserts, from get_tile() / get_block_tile() and mf_z_tiles(layers, tz), that its table is graded with 8 m tiles,
differs from the uniform table and has the extremes of the list above; MFMG_MF_GRADED_TILES=0 in the environment fails the module
(it would run the uniform table everywhere).  Then, with outputs NaN (or a NaN payload) before every launch so that a layer no
tile owns fails the bound:
  - the result on the graded tile is within (k + k_ref) u mag of long double per entry -- reference, inputs, k and k_ref are those
    of test_gpu_fp64_fine_level.py, test_gpu_fp32_fine_level.py, test_gpu_block_operator.py and test_gpu_block_operator_f32.py,
    whose helpers run here; the roundings per entry do not depend on the tiling, so no constant is new;
  - the same launch on (nw, ty, 2) and (nw, ty, 1) -- tz = 1 and 2 never grade: asserted -- gives the same bits;
  - a column of a block has the bits of the one-vector entry point on that column, which runs its own tile and table.
A tile that two tables place differently is thus computed from two different marches (fill, carries between layers, drain).

Counted k (fp32_reference.py) and the worst |got - ref| / (u mag) observed on an MI355X (test_worst_ratios_observed prints them;
documentation, not thresholds):
  one-term FP64   k = 16 / 32 (one / eight coefficients per cell), + 1 residual, + 12 epilogues     observed 10.2
  one-term FP32   the same k at u = 2^-24                                                           observed 3.3
  block FP64      k = 32, + 1, + 12                                                                 observed 10.5
  block FP32      the same k at u = 2^-24                                                           observed 2.2"""
import os

import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd.api import mf_z_tiles
import fp32_reference as F
import test_gpu_fp64_fine_level as D
import test_gpu_fp32_fine_level as S
import test_gpu_block_operator as BD
import test_gpu_block_operator_f32 as BS

pytestmark = pytest.mark.gpu

LD = np.longdouble
DEFAULT_TILE = (1, 2, 4)              # what choose_tile / choose_block_tile take on meshes this small (asserted where it is used)
# cells; the tiles of the one-term operator (None: the default); m; the smallest and the largest tile height of the table
CASES = {
    "G1": {"n": (12, 10, 32), "tiles": [None, (2, 3, 8)], "m": 2, "heights": (1, 3)},
    "G2": {"n": (6, 5, 56), "tiles": [(2, 2, 3)], "m": 3, "heights": (1, 4)},
    "G3": {"n": (20, 17, 96), "tiles": [(4, 2, 4)], "m": 4, "heights": (1, 5)},
    "G4": {"n": (6, 5, 158), "tiles": [(2, 3, 8)], "m": 3, "heights": (4, 9)},
    "G5": {"n": (64, 18, 32), "tiles": [(2, 2, 4)], "m": 2, "heights": (1, 3)},
    "G6": {"n": (65, 70, 31), "tiles": [(2, 2, 4)], "m": 2, "heights": (1, 3)},
}
ONE_TERM_F64 = [(c, m) for c in ("G1", "G3") for m in D.MATERIALS] + [(c, m) for c in ("G2", "G4", "G5") for m in ("linear", "cellwise6")] \
    + [("G6", "constant")]
ONE_TERM_F32 = [("G1", m) for m in ("constant", "cellwise", "linear")] + [(c, m) for c in ("G3", "G5") for m in ("cellwise", "linear")]
# tiles of the block operator (ty in 2 .. 4); None: its default
BLOCK_TILES = {"G1": [(2, 3, 8)], "G3": [(4, 2, 4), None], "G5": [(2, 2, 4)]}
BLOCK_KS = [2, 4, 7]                  # the groups 2; 4; 4 + 2 + 1
UNIFORM_TZ = [2, 1]

WORST = {"one-term FP64": 0.0, "one-term FP32": 0.0, "block FP64": 0.0, "block FP32": 0.0}


def _heights(tab):
    return [b - a for a, b in zip(tab, tab[1:])]


def _graded_table(case, tz):
    """The table of `tz` on the layers of the case, after asserting that it is the graded one the case is listed with."""
    assert os.environ.get("MFMG_MF_GRADED_TILES") != "0", "MFMG_MF_GRADED_TILES=0: every launch would read the uniform table"
    layers = CASES[case]["n"][2] + 1
    tab, uniform = mf_z_tiles(layers, tz), mf_z_tiles(layers, tz, graded=False)
    m = (layers // 8 + tz // 2) // tz + 1
    assert m == CASES[case]["m"] and layers // 8 >= 2 * m, (case, tz, m)
    assert len(tab) - 1 == 8 * m and tab != uniform and len(uniform) - 1 == -(-layers // tz), (case, tz, tab)
    h = _heights(tab)
    assert (min(h), max(h)) == CASES[case]["heights"], (case, tz, h)
    assert tab[0] == 0 and tab[-1] == layers and min(h) >= 1
    return tab


def _uniform_table(case, tz):
    layers = CASES[case]["n"][2] + 1
    tab = mf_z_tiles(layers, tz)
    assert tab == mf_z_tiles(layers, tz, graded=False) == list(range(0, layers, tz)) + [layers], (case, tz)
    return tab


def test_the_cases_reach_the_tables_they_name():
    """(no launch: the tables of every case and tile, and what the shapes are chosen for)"""
    assert np.finfo(LD).nmant >= 63
    for case, c in CASES.items():
        for tile in c["tiles"] + BLOCK_TILES.get(case, []):
            _graded_table(case, (tile or DEFAULT_TILE)[2])
        for tz in UNIFORM_TZ:
            _uniform_table(case, tz)
        # several tiles along y, so a z-tile is marched by more than one workgroup
        assert all(c["n"][1] + 1 > nw * ty - 1 for nw, ty, _ in (t or DEFAULT_TILE for t in c["tiles"]))
    h = lambda case, tz: _heights(mf_z_tiles(CASES[case]["n"][2] + 1, tz))
    assert h("G1", 4) == h("G1", 8) == [3, 1] * 7 + [3, 2] and h("G6", 4) == [3, 1] * 8
    assert set(h("G2", 3)) == {1, 2, 3, 4} and max(h("G2", 3)) > 3
    assert h("G3", 4) == [5, 3, 3, 1] * 7 + [5, 4, 2, 2] and h("G4", 8) == [9, 6, 4] + [9, 7, 4] * 7
    # the tallest meshes of the older modules: one tile per eighth, or not graded at all
    assert len(mf_z_tiles(23, 8)) - 1 == 8 and mf_z_tiles(10, 8) == [0, 8, 10] and mf_z_tiles(10, 4) == [0, 4, 8, 10]
    # G5: 65 node columns are 62 + 3 with one halo lane (eight coefficients per cell), 58 + 7 with three
    assert CASES["G5"]["n"][0] + 1 == 62 + 3 == 58 + 7
    # G6: one halo lane, 62 owned columns per chunk: the last chunk owns 4 <= 24 columns and the mesh has >= 64 node rows, which is
    # when the operator runs those columns as a rotated slab (mf_laplace.hip, "nearly empty last chunk")
    nx, ny = CASES["G6"]["n"][0] + 1, CASES["G6"]["n"][1] + 1
    assert nx - 62 * ((nx + 61) // 62 - 1) == 4 and ny >= 64 and CASES["G6"]["n"] not in S.TAIL_SLAB
    assert 140e3 < nx * ny * 32 < 160e3 and all(np.prod([v + 1 for v in CASES[c]["n"]]) <= 41e3 for c in CASES if c != "G6")
    assert [BD.block_groups(k) for k in BLOCK_KS] == [[2], [4], [4, 2, 1]]


def _set_one_term_tile(op, case, tile):
    """Sets the tile (None: asserts the default) and returns it with its graded table asserted."""
    if tile is None:
        tile = op.get_tile()
        assert tile == DEFAULT_TILE, f"{case}: the default tile is {tile}"
    else:
        op.set_tile(tile[1], tile[2], tile[0])
        assert op.get_tile() == tile, (case, tile, op.get_tile())
    _graded_table(case, tile[2])
    return tile


def _bit_equal_on_uniform_tiles(case, tile, op, run, base, names, what, tzs=UNIFORM_TZ):
    for tz in tzs:
        _uniform_table(case, tz)
        op.set_tile(tile[1], tz, tile[0])
        assert op.get_tile() == (tile[0], tile[1], tz)
        for name, got, want in zip(names, run(), base):
            assert torch.equal(got, want), f"{what}: {name} on the uniform tile tz = {tz} differs from the graded tile in {(got != want).sum().item()} entries"


# ---- a. the one-term operator in FP64 ----
def _one_term_f64(ctx, op, case, material, what0, perm=None, only=range(5)):
    n = CASES[case]["n"]
    prob, ref, x, b, xp = D._case(n, material)
    refs, units, ks = D._one_term_references(n, material)
    xd, bd, xpd = (D._gpu(D._to_dof(v, perm)) for v in (x, b, xp))
    run = lambda: D._one_term_outputs(ctx, op, xd, bd, xpd)
    for tile in CASES[case]["tiles"]:
        tile = _set_one_term_tile(op, case, tile)
        what = f"{case} {n} {material} {what0}tile {tile}"
        base = run()
        for i in only:
            got = base[i].cpu().numpy()
            WORST["one-term FP64"] = max(WORST["one-term FP64"], F.worst_ratio(got[perm] if perm is not None else got, refs[i], units[i]))
            D._check("one-term", base[i], refs[i], units[i], ks[i], f"{what} {D.OPS[i]}", perm=perm)
        _bit_equal_on_uniform_tiles(case, tile, op, run, base, D.OPS, what)
        D._check_dinv(op, ref, what, perm)


@pytest.mark.parametrize("case,material", ONE_TERM_F64, ids=lambda v: v)
def test_one_term_fp64_on_graded_tiles(ctx, case, material):
    n = CASES[case]["n"]
    prob, ref, _, _, _ = D._case(n, material)
    cc = ref.cell_constant
    if case == "G6":
        # records with one halo lane, as TAIL_SLAB of test_gpu_fp64_fine_level.py: the tail columns run as the rotated slab
        ctx.set_mf_fused_terms(1)
        try:
            op = D._operator(ctx, prob)
        finally:
            ctx.set_mf_fused_terms(3)
        assert cc and not op.sweep_available(2)
    else:
        op = D._operator(ctx, prob)
    assert op.cell_constant_layout() == cc and op.diagonal_in_record() == (not cc)
    _one_term_f64(ctx, op, case, material, "")
    if cc and case in ("G1", "G3"):
        # D^-1 kept in the records instead of derived in the kernel: the smoother steps within the same bound
        op_s = D._operator(ctx, prob, stored=True)
        assert op_s.diagonal_in_record()
        _one_term_f64(ctx, op_s, case, material, "stored D^-1 ", only=(2, 3, 4))


def test_one_term_fp64_on_graded_tiles_with_a_random_numbering(ctx):
    """Ids read from the records, not computed: vectors and results permuted, the same reference."""
    case, material = "G1", "linear"
    n = CASES[case]["n"]
    _, ref, _, _, _ = D._case(n, material)
    perm = np.random.default_rng(3).permutation(ref.n_dofs)
    op = D._operator(ctx, D._problem(n, material, numbering=torch.from_numpy(perm)))
    assert not op.ids_computed() and D._operator(ctx, D._case(n, material)[0]).ids_computed()
    _one_term_f64(ctx, op, case, material, "random numbering ", perm=perm)


# ---- b. the one-term operator in FP32 ----
@pytest.mark.parametrize("case,material", ONE_TERM_F32, ids=lambda v: v)
def test_one_term_fp32_on_graded_tiles(ctx, case, material):
    n = CASES[case]["n"]
    prob, ref, x, b, xp = S._case(n, material)
    op = S._operator(ctx, prob)
    cc = material != "linear"
    assert op.cell_constant_layout() == cc and op.diagonal_in_record() == (not cc)
    refs, units, ks = S._one_term_references(ref, x, b, xp)
    xd, bd, xpd = S._gpu(x), S._gpu(b), S._gpu(xp)
    run = lambda: S._one_term_outputs(ctx, op, xd, bd, xpd)
    for tile in CASES[case]["tiles"]:
        tile = _set_one_term_tile(op, case, tile)
        what = f"{case} {n} {material} float tile {tile}"
        base = run()
        for name, got, want, unit, k in zip(S.OPS, base, refs, units, ks):
            WORST["one-term FP32"] = max(WORST["one-term FP32"], F.worst_ratio(got.cpu().numpy(), want, unit))
            S._check("one-term", got, want, unit, k, f"{what} {name}")
        _bit_equal_on_uniform_tiles(case, tile, op, run, base, S.OPS, what, tzs=[2])
        dinv = op.diagonal_inverse().cpu().numpy().astype(LD)
        assert not F.beyond(dinv, ref.dinv, 2 * F.U32 * ref.dinv).any(), f"{what}: D^-1 beyond 2 u"


# ---- c. the block operator in FP64 and FP32 ----
@pytest.mark.parametrize("material", ["linear", "discontinuous"])
@pytest.mark.parametrize("case", sorted(BLOCK_TILES))
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_block_launch_on_graded_tiles(ctx, precision, case, material):
    """Every launch of the block operator reads the graded table.  k = 2, 4 and 7 on guarded blocks; every column within the bound,
    with the bits of the one-vector entry point (its own tile, its own table) and of the same block call on (nw, ty, 2)."""
    B, Op, family = (BD, M.MatrixFreeLaplace, "block FP64") if precision == "FP64" else (BS, M.MatrixFreeLaplaceF32, "block FP32")
    block_kernel = "mf_laplace_block_kernel" if precision == "FP64" else BS.BLOCK
    n = CASES[case]["n"]
    prob, ref, perm, cols, ks = B._case(n, material, "lexicographic")
    assert perm is None and len(cols) >= max(BLOCK_KS)
    nd, ld = ref.n_dofs, B._ld(ref.n_dofs)
    op = Op(ctx, prob)
    assert op.block_available() and not op.cell_constant_layout()
    what0 = f"{case} {n} {material} {precision}"
    # the one-vector entry point runs the default tile of the one-term operator on its own graded table
    one_tile = op.get_tile()
    assert one_tile == DEFAULT_TILE
    _graded_table(case, one_tile[2])
    dev = [tuple(B._gpu(v) for v in col[:3]) for col in cols]
    single = [B._one_vector(ctx, op, *d) for d in dev]
    for c, (col, outs) in enumerate(zip(cols, single)):
        for m, (got, want, unit) in enumerate(zip(outs, col[3], col[4])):
            F.assert_within(got.cpu().numpy(), want, unit, ks[m] + B.K_REF, f"{what0} column {c} {B.MODES[m]}, one vector")
    for tile in BLOCK_TILES[case]:
        op.set_block_tile(*(tile or (0, 0, 0)))
        chosen = (op.get_block_tile(2), op.get_block_tile(4))
        assert chosen == ((tile, tile) if tile else (DEFAULT_TILE, DEFAULT_TILE)), (what0, tile, chosen)
        asked, tile = tile or (0, 0, 0), chosen[1]
        assert 2 <= tile[1] <= 4
        _graded_table(case, tile[2])
        _uniform_table(case, 2)
        for k in BLOCK_KS:
            X, Bb, XP = (B._block_of([d[i] for d in dev[:k]], ld) for i in range(3))
            what = f"{what0} k {k} tile {tile}"

            def run(t, ask):
                op.set_block_tile(*ask)
                assert op.get_block_tile(2) == t and op.get_block_tile(4) == t
                ctx.profile_enable(True, f"{block_kernel},mf_laplace_kernel")
                outs = B._block_outputs(ctx, op, X, Bb, XP, k, ld)
                launches, columns = ctx.profile_query(block_kernel)[0], ctx.profile_query("mf_laplace_kernel")[0]
                ctx.profile_enable(False)
                # no fall back to the loop: the block kernel once per group of 4 or 2 and launch, the one-vector kernel for the rest
                assert launches == 5 * B._wide_groups(k) and columns == 5 * (k % 2), (what, t, launches, columns)
                return outs

            graded, uniform = run(tile, asked), run((tile[0], tile[1], 2), (tile[0], tile[1], 2))
            for m, (out, out_u) in enumerate(zip(graded, uniform)):
                for c in range(k):
                    got = out[c + 1, :nd]
                    g = got.cpu().numpy()
                    WORST[family] = max(WORST[family], F.worst_ratio(g, cols[c][3][m], cols[c][4][m]))
                    F.assert_within(g, cols[c][3][m], cols[c][4][m], ks[m] + B.K_REF, f"{what} column {c} {B.MODES[m]}")
                    assert torch.equal(got, single[c][m]), \
                        f"{what} {B.MODES[m]}: column {c} differs from the one-vector entry point in {(got != single[c][m]).sum().item()} entries"
                    assert torch.equal(got, out_u[c + 1, :nd]), \
                        f"{what} {B.MODES[m]}: column {c} differs from the block call on tz = 2 in {(got != out_u[c + 1, :nd]).sum().item()} entries"
                for o in (out, out_u):
                    assert B._untouched(o[0]) and B._untouched(o[k + 1]) and B._untouched(o[1:k + 1, nd:]), f"{what} {B.MODES[m]}: wrote outside its columns"
            for blk in (X, Bb, XP):
                assert B._untouched(blk[0]) and B._untouched(blk[k + 1]) and B._untouched(blk[1:k + 1, nd:]), f"{what}: an input block was written"
    op.set_block_tile(0, 0, 0)


def test_worst_ratios_observed():
    """(runs last: what the cases above measured, for the figures of the module docstring)"""
    print("worst |got - ref| / (u mag) per family: " + ", ".join(f"{k} {v:.2f}" for k, v in WORST.items()))
