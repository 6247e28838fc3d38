"""The stencil sweep of a uniform coefficient on twelve wavefronts with disjoint node rows (mf_cheb_fused.hip:
mf_cheb_fused_uniform_kernel, three node rows per wavefront of its own, 30 owned rows per y-tile) entry by entry against the long
double restatement of test_gpu_uniform_sweep.py, under that file's rule: per case the largest entry-wise error of the mode-space
sweep (MFMG_MF_UNIFORM_SWEEP=0) against the same reference is measured, and the stencil sweep must stay within twice that.  Both
errors are printed.

Sizes are DoFs per direction, chosen for the edges of this tiling (58 owned columns per full chunk column, 30 owned rows per
y-tile): see CASES.  Checked with NaN-filled outputs: that the operator reports a uniform coefficient and every launch counted was a
stencil kernel; x_3 and x_2 against long double; bit for bit against the other tile shapes of the three-term sweep, which run
mf_cheb_fused_uniform_rows_kernel (shared node rows, 8 x 3, 4 x 3, 2 x 4, 8 x 2 -- the kernels this change leaves alone); bit for
bit across two other z-tile heights; x_3 without x_2 requested; the sweep from a zero guess against the sweep on a zeroed vector and
against the zero guess of the 8 x 3 shape, bit for bit; the default height back after set_sweep_tile(0, 0, 0)."""
import numpy as np
import pytest
import torch

import mfmg_amd as M
from test_gpu_uniform_sweep import LD, OTHER_SHAPES, _case, _err, _gpu, _mode_space, _sweep

pytestmark = pytest.mark.gpu

# (DoFs per direction, two z-tile heights beside the default)
CASES = [((5, 5, 5), (2, 5)),        # every free node next to a face; the rows split across wavefronts 1 and 2
         ((20, 30, 7), (2, 7)),      # exactly one full y-tile of 30 rows
         ((59, 31, 9), (2, 4)),      # one wide column and a narrow one of 1 column; a full y-tile and one row more, paired in the narrow body
         ((60, 32, 9), (3, 9)),      # a narrow column of 2; a second y-tile of 2 rows
         ((84, 61, 70), (7, 33)),    # a narrow column of 26 that pairs two full y-tiles and leaves a third (one row) half idle; several z-tiles
         ((257, 5, 5), (2, 5))]      # five chunk columns, the narrow one of 25
IDS = ["x".join(map(str, c[0])) for c in CASES]


@pytest.mark.parametrize("dofs,heights", CASES, ids=IDS)
def test_disjoint_rows_sweep(ctx, dofs, heights):
    assert np.finfo(LD).nmant >= 63
    prob, x, b, its, zits = _case(dofs)
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.cell_constant_layout() and op.sweep_available(3) and op.uniform_coefficient()
    assert op.get_sweep_tile(3)[:2] == (12, 2)
    xd, bd, zd = _gpu(x), _gpu(b), torch.zeros(b.size, dtype=torch.float64, device="cuda")
    n0 = op.uniform_sweep_launches()
    out, outp = _sweep(ctx, op, bd, xd)
    assert op.uniform_sweep_launches() == n0 + 1, "the sweep did not take the stencil kernel"
    # against long double, beside the mode-space sweep on the same operator
    old, oldp = _mode_space(ctx, op, bd, xd)
    for what, got, parent, ref in (("x_3", out, old, its[3]), ("x_2", outp, oldp, its[2])):
        e_new, e_old = _err(got, ref), _err(parent, ref)
        print(f"{dofs} {what}: largest entry-wise error, stencil sweep {e_new:.3e}, mode-space sweep {e_old:.3e}")
        assert np.isfinite(e_new) and e_old > 0.0
        assert e_new <= 2.0 * e_old, f"{dofs} {what}: {e_new:.3e} beyond twice the mode-space sweep's {e_old:.3e}"
    # x_2 not requested: the same x_3
    only, none = _sweep(ctx, op, bd, xd, with_prev=False)
    assert none is None and torch.equal(only, out)
    # from a zero guess: the bits of the sweep on a zeroed vector
    zout, zoutp = _sweep(ctx, op, bd, None)
    for what, got, ref in (("x_3", zout, zits[3]), ("x_2", zoutp, zits[2])):
        assert np.isfinite(_err(got, ref))
    onz, onzp = _sweep(ctx, op, bd, zd)
    assert torch.equal(zout, onz) and torch.equal(zoutp, onzp), "from zero differs from the sweep on a zeroed vector"
    # the other z-tile heights and the kernels of the other shapes (shared node rows, untouched), bit for bit
    tz0 = op.get_sweep_tile(3)[2]
    launches = op.uniform_sweep_launches()
    for tile in [(12, 2, tz) for tz in heights] + OTHER_SHAPES:
        op.set_sweep_tile(*tile)
        assert op.get_sweep_tile(3)[:2] == tile[:2] and (tile[2] == 0 or op.get_sweep_tile(3)[2] == tile[2])
        o, p = _sweep(ctx, op, bd, xd)
        assert torch.equal(o, out) and torch.equal(p, outp), f"{dofs}: tile {tile} differs from the default (z-tiles of {tz0}) in {(o != out).sum().item()} entries"
        launches += 1
        if tile[:2] == (12, 2) or tile == (8, 3, 0):
            o, p = _sweep(ctx, op, bd, None)
            assert torch.equal(o, zout) and torch.equal(p, zoutp), f"{dofs}: tile {tile} differs from the default from a zero guess"
            launches += 1
    assert op.uniform_sweep_launches() == launches, "a counted launch was no stencil kernel"
    op.set_sweep_tile(0, 0, 0)
    assert op.get_sweep_tile(3) == (12, 2, tz0)


def test_cases_reach_the_edges_they_name():
    own_cols, own_rows = 64 - 2 * 3, 12 * 3 - 2 * 3
    assert (own_cols, own_rows) == (58, 30)
    narrow = {d: d[0] - (d[0] - 1) // own_cols * own_cols for d, _ in CASES if d[0] > own_cols}
    y_tiles = {d: -(-d[1] // own_rows) for d, _ in CASES}
    last_rows = {d: d[1] - (y_tiles[d] - 1) * own_rows for d, _ in CASES}
    assert (narrow[(59, 31, 9)], y_tiles[(59, 31, 9)], last_rows[(59, 31, 9)]) == (1, 2, 1)
    assert (narrow[(60, 32, 9)], y_tiles[(60, 32, 9)], last_rows[(60, 32, 9)]) == (2, 2, 2)
    assert (narrow[(84, 61, 70)], y_tiles[(84, 61, 70)], last_rows[(84, 61, 70)]) == (26, 3, 1)
    assert (narrow[(257, 5, 5)], y_tiles[(257, 5, 5)], last_rows[(257, 5, 5)]) == (25, 1, 5)
    assert -(-257 // own_cols) == 5
    assert y_tiles[(20, 30, 7)] == 1 and last_rows[(20, 30, 7)] == own_rows
    assert all(max(h) <= d[2] and len(set(h)) == 2 for d, h in CASES)
