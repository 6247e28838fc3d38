"""The FP32 matrix-free operator on a block of float vectors (MatrixFreeLaplaceF32.block_launch, mf_laplace_block_f32_kernel in
mf_laplace_block.hip) against long double and against the one-vector FP32 entry points, column by column: the battery of
test_gpu_block_operator.py in float.

Reference and bound: fp32_reference.Reference with u = 2^-24 on float32 inputs, outputs NaN before every launch, per entry
|got - ref| <= (k + K_REF) u mag with the counted k of the one-term float kernel (eight coefficients per cell: 32 for A x, one more
for the subtraction of b, + 12 for the smoother epilogues).  K_REF is the reference's own error in units of u: at u = 2^-24 the
Reference builds its cell matrices in double, so its 96 roundings are 96 * 2^-53 / 2^-24 = 1.8e-7 of one unit of k.  Beyond the
bound every column equals vmult / residual / smoother_step of MatrixFreeLaplaceF32 on that column bit for bit, for every tile.

Meshes (cells): (1,1,1) and (2,1,3) degenerate; (125,2,1) 126 node columns, which the float operator spreads evenly over three
chunks; (64,18,6) 65 node columns = 33 + 32, several wavefront hand-overs; (20,17,9) and (6,5,7).  k = 1, 2, 3, 4, 5, 7 are the
group combinations 1; 2; 2+1; 4; 4+1; 4+2+1.  The blocks carry one guard column before and after and a leading dimension of
n_dofs + 6, one more where that is odd (an odd leading dimension is refused: columns are aligned to 8 bytes); the guard columns and
the entries [n_dofs, ld) of every column keep their 32-bit NaN payload.

The LDS: mf_block_lds gives (8, 4, tz) at four float vectors 114 KiB, the largest tile the setter accepts (1..8 wavefronts of 2..4
rows) -- no tile it accepts exceeds the 160 KiB of a compute unit in float, so the "too large for the LDS" error of run_block cannot
be reached through this interface; test_the_largest_tile_fits_the_lds_in_float asserts exactly that and runs the tile."""
import functools

import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
from mfmg_amd.api import block_groups
import fp32_reference as F
from test_gpu_fp32_fine_level import AL, BE, ALF, BEF, _gpu
from test_gpu_fp64_fine_level import _problem, _to_dof

pytestmark = pytest.mark.gpu

LD = np.longdouble
MESHES = [(1, 1, 1), (2, 1, 3), (125, 2, 1), (64, 18, 6), (20, 17, 9), (6, 5, 7)]
KS = [1, 2, 3, 4, 5, 7]
K_MAX = max(KS)
TILES = [None, (1, 2, 1), (2, 3, 8), (3, 2, 5), (4, 4, 16)]          # (nw, ty, tz); None: the default
MODES = ["apply", "residual", "first", "next", "next over its own x_prev"]
K_REF = F.K_REF * F.U64 / F.U32
PAYLOAD = 0x7FC0BEEF                  # a quiet float NaN nobody computes
BLOCK, ONE = "mf_laplace_block_f32_kernel", "mf_laplace_kernel"
LDS_LIMIT = 160 * 1024


def mf_block_lds(nv, nw, ty, elem=4):
    """mf_block_lds of mf_laplace_block.hip"""
    return (nw * nv * (2 * ty + 1) + 2 * nw * nv * 2) * 64 * elem + nw * (ty + 1) * 64 * 4


def _ld(n_dofs):
    return n_dofs + 6 + (n_dofs & 1)


def _nan_block(k, ld):
    """(k + 2) x ld entries of one NaN payload: a guard column, k columns, a guard column."""
    return torch.full((k + 2, ld), PAYLOAD, dtype=torch.int32, device="cuda").view(torch.float32)


def _untouched(t):
    return bool((t.contiguous().view(torch.int32) == PAYLOAD).all().item())


def _block_of(cols, ld):
    blk = _nan_block(len(cols), ld)
    for c, v in enumerate(cols):
        blk[c + 1, :v.numel()] = v
    return blk


@functools.lru_cache(maxsize=None)
def _case(n, material, numbering):
    """Problem, long double reference and K_MAX columns of float32 (x, b, x_prev) with their references, units and k per mode."""
    base = _problem(n, material)
    ref = F.Reference(n, base.coefficient.cpu().numpy())
    perm = np.random.default_rng(3).permutation(ref.n_dofs) if numbering == "random" else None
    prob = _problem(n, material, numbering=torch.from_numpy(perm)) if perm is not None else base
    rng = np.random.default_rng([len(material), *n, 11])
    cols = []
    for c in range(K_MAX):
        x, b, xp = (F.f32(rng.standard_normal(ref.n_dofs)) for _ in range(3))
        ax = ref.vmult(x)
        mom = ref.step(x, b, xp, ALF[1], BEF[1], ax=ax)
        refs = [ax, ax - b.astype(LD), ref.step(x, b, None, 0.0, BEF[0], ax=ax), mom, mom]
        um = ref.unit_step(x, b, xp, ALF[1], BEF[1])
        units = [ref.unit_vmult(x), ref.unit_residual(x, b), ref.unit_step(x, b, None, 0.0, BEF[0]), um, um]
        cols.append((x, b, xp, refs, units))
    ks = [ref.k_op, ref.k_op + 1, ref.k_step, ref.k_step, ref.k_step]
    return prob, ref, perm, cols, ks


def _one_vector(ctx, op, x, b, xp):
    n = x.numel()
    out = [torch.full((n,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)]
    op.vmult(out[0], x)
    op.residual(x, b, out[1])
    op.smoother_step(b, x, None, 0.0, BE[0], out[2])
    op.smoother_step(b, x, xp, AL[1], BE[1], out[3])
    out.append(xp.clone())
    op.smoother_step(b, x, out[4], AL[1], BE[1], out[4])
    ctx.synchronize()
    return out


def _block_outputs(ctx, op, X, B, XP, k, ld):
    """The five launches on the columns 1 .. k of the guarded blocks; returns the guarded output blocks."""
    out = [_nan_block(k, ld) for _ in range(4)]
    op.block_launch("apply", X[1:k + 1], out[0][1:k + 1])
    op.block_launch("residual", X[1:k + 1], out[1][1:k + 1], B=B[1:k + 1])
    op.block_launch("first", X[1:k + 1], out[2][1:k + 1], B=B[1:k + 1], beta=BE[0])
    op.block_launch("next", X[1:k + 1], out[3][1:k + 1], B=B[1:k + 1], X_prev=XP[1:k + 1], alpha=AL[1], beta=BE[1])
    out.append(XP.clone())                                      # the momentum term written over its own x_prev
    op.block_launch("next", X[1:k + 1], out[4][1:k + 1], B=B[1:k + 1], X_prev=out[4][1:k + 1], alpha=AL[1], beta=BE[1])
    ctx.synchronize()
    return out


def _wide_groups(k):
    return len([w for w in block_groups(k) if w > 1])


def _battery(ctx, n, material, numbering, tiles=TILES):
    prob, ref, perm, cols, ks = _case(n, material, numbering)
    nd, ld = ref.n_dofs, _ld(ref.n_dofs)
    op = M.MatrixFreeLaplaceF32(ctx, prob)
    what0 = f"{n} {material} {numbering}"
    assert op.block_available() == (not op.cell_constant_layout()), what0
    dev = [tuple(_gpu(_to_dof(v, perm)) for v in col[:3]) for col in cols]
    single = [_one_vector(ctx, op, *d) for d in dev]
    # the one-vector entry point against long double (what the columns of the blocks are then compared with bit for bit)
    for c, (col, outs) in enumerate(zip(cols, single)):
        for m, (got, want, unit) in enumerate(zip(outs, col[3], col[4])):
            g = got.cpu().numpy()
            F.assert_within(g[perm] if perm is not None else g, want, unit, ks[m] + K_REF, f"{what0} column {c} {MODES[m]}, one vector")
    worst = 0.0
    for tile in tiles:
        op.set_block_tile(*(tile or (0, 0, 0)))
        if tile is not None and op.block_available():
            assert op.get_block_tile(4) == tile and op.get_block_tile(2) == tile
        for k in KS:
            X, B, XP = (_block_of([d[i] for d in dev[:k]], ld) for i in range(3))
            ctx.profile_enable(True, f"{BLOCK},{ONE}")
            outs = _block_outputs(ctx, op, X, B, XP, k, ld)
            launches = ctx.profile_query(BLOCK)[0]
            columns = ctx.profile_query(ONE)[0]
            ctx.profile_enable(False)
            what = f"{what0} k {k} tile {tile or op.get_block_tile(4)}"
            # no vacuous pass: the block kernel ran once per group of 4 or 2 and launch, the one-vector kernel for the rest
            if op.block_available():
                assert launches == 5 * _wide_groups(k), (what, launches)
                assert columns == 5 * (k % 2), (what, columns)
            else:
                assert launches == 0 and columns == 5 * k, (what, launches, columns)
            for m, out in enumerate(outs):
                for c in range(k):
                    got = out[c + 1, :nd]
                    assert torch.equal(got, single[c][m]), \
                        f"{what} {MODES[m]}: column {c} differs from the one-vector entry point in {(got != single[c][m]).sum().item()} entries"
                    if tile is None:      # (the other tiles: the same bits, asserted above)
                        g = got.cpu().numpy()
                        g = g[perm] if perm is not None else g
                        worst = max(worst, F.worst_ratio(g, cols[c][3][m], cols[c][4][m]))
                        F.assert_within(g, cols[c][3][m], cols[c][4][m], ks[m] + K_REF, f"{what} column {c} {MODES[m]}")
                # nothing else is written: the guard columns and the entries [n_dofs, ld) of every column
                assert _untouched(out[0]) and _untouched(out[k + 1]) and _untouched(out[1:k + 1, nd:]), f"{what} {MODES[m]}: wrote outside its columns"
            for blk in (X, B, XP):
                assert _untouched(blk[0]) and _untouched(blk[k + 1]) and _untouched(blk[1:k + 1, nd:]), f"{what}: an input block was written"
    op.set_block_tile(0, 0, 0)
    print(f"{what0}: worst |got - ref| / (u mag) over all columns, modes and tiles = {worst:.2f} (k = {ks})")
    return op


def test_shapes_reach_the_edges_they_name():
    # the float operator with one halo lane owns 62 node columns per chunk and spreads the node columns evenly
    chunks = lambda nx: -(-nx // 62)
    assert chunks(126) == 3 and 126 % 3 == 0 and chunks(65) == 2 and chunks(21) == 1
    assert [block_groups(k) for k in KS] == [[1], [2], [2, 1], [4], [4, 1], [4, 2, 1]]
    # (64,18,6): 19 node rows are more than one y-tile of every tile of TILES (a y-tile owns nw * ty - 1 rows), 7 layers more
    # than one z-tile of (3,2,5) and (1,2,1)
    assert all(19 > nw * ty - 1 for nw, ty, tz in TILES[1:]) and 7 > 5


@pytest.mark.parametrize("material", ["linear", "discontinuous"])
@pytest.mark.parametrize("n", MESHES, ids=lambda v: "x".join(map(str, v)))
def test_block_launch_every_mode_every_group_every_tile(ctx, n, material):
    op = _battery(ctx, n, material, "lexicographic")
    if material == "linear":
        assert op.block_available()
        assert op.ids_computed() == (min(n) >= 2)              # (computed ids need three nodes per direction)


@pytest.mark.parametrize("n", [(20, 17, 9), (64, 18, 6)], ids=lambda v: "x".join(map(str, v)))
def test_block_launch_with_ids_read_from_the_records(ctx, n):
    op = _battery(ctx, n, "linear", "random")
    assert op.block_available() and not op.ids_computed()


def test_cell_constant_layout_loops_over_the_columns(ctx):
    """No block kernel for one coefficient per cell: the block call returns the bits of the loop (asserted in the battery, with
    the launch counts of the loop)."""
    op = _battery(ctx, (20, 17, 9), "constant", "lexicographic")
    assert not op.block_available() and op.cell_constant_layout()


def test_the_largest_tile_fits_the_lds_in_float(ctx):
    """(8, 4, 4) at four vectors: 212 KiB in FP64, refused there; 114 KiB in float.  No tile the setter accepts (1..8 wavefronts
    of 2..4 rows, 2 or 4 vectors) exceeds the LDS in float, so the tile runs and gives the bits of the default tile."""
    assert mf_block_lds(4, 8, 4, 8) > LDS_LIMIT >= mf_block_lds(4, 8, 4) == 116736
    assert all(mf_block_lds(nv, nw, ty) <= LDS_LIMIT for nv in (2, 4) for nw in range(1, 9) for ty in (2, 3, 4))
    prob, ref, perm, cols, ks = _case((20, 17, 9), "linear", "lexicographic")
    op = M.MatrixFreeLaplaceF32(ctx, prob)
    nd, ld = ref.n_dofs, _ld(ref.n_dofs)
    X = _block_of([_gpu(c[0]) for c in cols[:4]], ld)
    out, want = _nan_block(4, ld), _nan_block(4, ld)
    with pytest.raises(L.MfmgInvalidArgument, match="block tile"):
        op.set_block_tile(9, 4, 4)                               # (the setter's range is where a larger tile stops)
    with pytest.raises(L.MfmgInvalidArgument, match="block tile"):
        op.set_block_tile(8, 5, 4)
    op.set_block_tile(8, 4, 4)
    ctx.profile_enable(True, BLOCK)
    op.block_launch("apply", X[1:5], out[1:5])
    ctx.synchronize()
    assert ctx.profile_query(BLOCK)[0] == 1
    ctx.profile_enable(False)
    op.set_block_tile(0, 0, 0)
    op.block_launch("apply", X[1:5], want[1:5])
    ctx.synchronize()
    assert torch.equal(out[1:5, :nd], want[1:5, :nd])
    assert _untouched(out[0]) and _untouched(out[5]) and _untouched(out[1:5, nd:])


def test_rejections(ctx, mfmg_lib):
    prob, ref, perm, cols, ks = _case((6, 5, 7), "linear", "lexicographic")
    op = M.MatrixFreeLaplaceF32(ctx, prob)
    nd = ref.n_dofs
    assert nd % 2 == 0
    ld = nd + 6
    big = _nan_block(70, ld)
    src = _nan_block(70, ld)
    src[:, :] = 1.0
    out = big[1:5]
    x = src[1:5]

    def refused(match, *args, **kw):
        with pytest.raises(L.MfmgInvalidArgument, match=match):
            op.block_launch(*args, **kw)
        ctx.synchronize()
        assert _untouched(big), match

    flat_o, flat_x = big.view(-1), src.view(-1)
    odd = lambda flat, k, l, off=0: torch.as_strided(flat, (k, nd), (l, 1), off)
    refused("even", "apply", odd(flat_x, 4, ld + 1), odd(flat_o, 4, ld + 1))                      # odd ld
    refused("at least n_dofs", "apply", torch.as_strided(flat_x, (4, nd - 2), (nd - 2, 1)), torch.as_strided(flat_o, (4, nd - 2), (nd - 2, 1)))
    refused("1 to 64", "apply", src[1:1], big[1:1])                                                # n_vectors 0
    refused("1 to 64", "apply", src[1:66], big[1:66])                                              # n_vectors 65
    refused("aligned to 8 bytes", "apply", odd(flat_x, 4, ld, 1), out)                             # a view starting at an odd element
    refused("aligned to 8 bytes", "apply", x, odd(flat_o, 4, ld, 1))
    refused("right-hand side", "residual", x, out)                                                 # a null operand the mode reads
    refused("right-hand side", "first", x, out, beta=0.5)
    # the out block overlapping the x block (shifted by one column)
    with pytest.raises(L.MfmgInvalidArgument, match="overlaps"):
        op.block_launch("apply", src[1:5], src[2:6])
    ctx.synchronize()
    assert bool((src == 1.0).all().item())
    # float64 blocks never reach the float entry point
    with pytest.raises(ValueError, match="float32"):
        op.block_launch("apply", x.double(), out)
    # a context with a communicator (no transport is needed: the call is refused before anything runs)
    own = M.Context()
    L.check(mfmg_lib.mfmg_hip_context_set_communicator(own.handle, 0, 2, 0, 2))
    op2 = M.MatrixFreeLaplaceF32(own, prob)
    with pytest.raises(L.MfmgInvalidArgument, match="communicator"):
        op2.block_launch("apply", x, out)
    own.synchronize()
    assert _untouched(big)
