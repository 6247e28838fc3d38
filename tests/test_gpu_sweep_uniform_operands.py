"""The operands the twelve-wavefront sweep (mf_cheb_fused_wg12_kernel) reads once per tile and holds for the march: the polynomial
coefficients alpha_2, alpha_3, beta_1 .. beta_3 and kd, and the base pointers of x, b, the records, out and out_prev.  A held
operand can go wrong where a re-read one could not: taken from the wrong stage, stale from the launch before, or a pointer held
for the wrong array.  So the coefficients here are NOT Chebyshev's: signed and pairwise distinct, a coefficient of another stage
changes the result; the vectors are views at odd 8-byte offsets into one allocation whose gaps are NaN and must come back with
their bits; and two launches follow each other on one operator with other coefficients and the roles of x and out exchanged.

FP64, one coefficient per cell (varying from cell to cell), D^-1 derived, three terms.  87 node columns are 58 + 29: wide tiles and
the tiles of a narrow last chunk column in one launch; 116 are two full chunk columns.  20 node rows are two y-tiles of 19 owned
rows (a full narrow pair), 39 are three (a full pair and one with an idle half).  9 node layers in z-tiles of 4 and 5: a fill and
a drain of the march shorter and longer than the three terms.

The 12 x 2 sweep is held to the 8 x 3 sweep with torch.equal (the results of the sweep do not depend on its tiling), and once to
long double with the bound of fp32_reference.py at u = 2^-53, as test_gpu_fp64_fine_level.py does."""
import functools

import numpy as np
import pytest
import torch

import mfmg_amd as M
import fp32_reference as F

pytestmark = pytest.mark.gpu

AL = [0.0, 0.37, -1.25]
BE = [0.81, -0.43, 1.9]
AL2 = [0.0, -0.59, 0.83]   # the second launch of the pair
BE2 = [-1.3, 0.67, 0.29]
HALO = 3
OWN_ROWS = 19  # 12 x 2 - 2 x 3 + 1 = 8 x 3 - 2 x 3 + 1
# (DoFs, z-tile)
CASES = [((nx, ny, 9), tz) for nx in (87, 116) for ny in (20, 39) for tz in (4, 5)]


def test_cases_reach_the_edges_they_name():
    full = 64 - 2 * HALO
    assert 87 == full + 29 and 29 <= 32 - HALO and 116 == 2 * full
    assert [(ny + OWN_ROWS - 1) // OWN_ROWS for ny in (20, 39)] == [2, 3]
    coefs = AL[1:] + BE + AL2[1:] + BE2
    assert len(set(coefs)) == len(coefs) and min(coefs) < 0 < max(coefs)


@functools.lru_cache(maxsize=None)
def _problem(dofs):
    prob = M.LaplaceProblem(tuple(v - 1 for v in dofs), "constant", device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    c = 0.5 + torch.rand(prob.n_cells_total, 1, dtype=torch.float64, device="cuda", generator=g)
    prob.coefficient = c.expand(-1, 8).contiguous()
    return prob


@functools.lru_cache(maxsize=None)
def _inputs(n_dofs):
    rng = np.random.default_rng(n_dofs)
    return tuple(rng.standard_normal(n_dofs) * 10.0 ** rng.uniform(-2, 2, n_dofs) for _ in range(2))


class Arena:
    """x, b, out, out_prev as views at odd 8-byte offsets into one allocation; everything else in it is NaN."""

    def __init__(self, n, x, b):
        self.n = n
        self.off, end = [], 0
        for gap in (1, 3, 5, 7):  # doubles before x and between the vectors at least; one more where the offset would be even
            o = end + gap
            o += 1 - o % 2
            self.off.append(o)
            end = o + n
        self.big = torch.full((end + 9,), float("nan"), dtype=torch.float64, device="cuda")
        assert all(o % 2 == 1 for o in self.off)
        self.x, self.b, self.out, self.outp = (self.big[o:o + n] for o in self.off)
        assert all(v.data_ptr() % 16 == 8 for v in (self.x, self.b, self.out, self.outp))
        self.x.copy_(torch.from_numpy(x))
        self.b.copy_(torch.from_numpy(b))
        self.gap = torch.ones_like(self.big, dtype=torch.bool)
        for o in self.off:
            self.gap[o:o + n] = False
        self.before = self.big.clone()

    def assert_untouched(self, what, written):
        """The gaps and the vectors that were only read come back with their bits."""
        same = self.big.view(torch.int64) == self.before.view(torch.int64)
        keep = self.gap.clone()
        for name, o in zip(("x", "b", "out", "outp"), self.off):
            if name not in written:
                keep[o:o + self.n] = True
        assert bool(same[keep].all()), f"{what}: {int((~same[keep]).sum())} entries outside the written vectors changed"


def _run(ctx, op, tile, x, b, al, be, with_prev, zero=False):
    """One sweep on the given tile from an arena; returns (x_3, x_2 or None)."""
    op.set_sweep_tile(*tile)
    assert tuple(op.get_sweep_tile(3))[:2] == tile[:2]
    a = Arena(b.size, x, b)
    op.smoother_sweep(al, be, a.b, None if zero else a.x, a.out, a.outp if with_prev else None)
    ctx.synchronize()
    a.assert_untouched(f"tile {tile}", ("out", "outp") if with_prev else ("out",))
    assert torch.isfinite(a.out).all() and (not with_prev or torch.isfinite(a.outp).all())
    return a.out.clone(), (a.outp.clone() if with_prev else None)


@pytest.mark.parametrize("dofs,tz", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"tz{v}")
def test_held_operands_give_the_bits_of_8x3(ctx, dofs, tz):
    prob = _problem(dofs)
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.sweep_available(3) and op.cell_constant_layout() and not op.diagonal_in_record()
    x, b = _inputs(prob.n_dofs)
    for with_prev in (True, False):
        for zero in (False, True):
            ref, refp = _run(ctx, op, (8, 3, tz), x, b, AL, BE, with_prev, zero)
            out, outp = _run(ctx, op, (12, 2, tz), x, b, AL, BE, with_prev, zero)
            what = f"{dofs} tz {tz} out_prev {with_prev} zero guess {zero}"
            assert torch.equal(out, ref), f"{what}: x_3 differs from 8 x 3 in {(out != ref).sum().item()} entries"
            assert outp is None or torch.equal(outp, refp), f"{what}: x_2 differs from 8 x 3 in {(outp != refp).sum().item()} entries"
    # a coefficient of another stage would show: exchanging two of them changes the result
    swapped, _ = _run(ctx, op, (12, 2, tz), x, b, AL, [BE[1], BE[0], BE[2]], False)
    assert not torch.equal(swapped, out)


def _pair(ctx, op, tile, x, b):
    """Two launches in a row, no synchronisation between them: (AL, BE) from x into out, then (AL2, BE2) from out into the
    vector that held x, out_prev into the other free one."""
    op.set_sweep_tile(*tile)
    a = Arena(b.size, x, b)
    op.smoother_sweep(AL, BE, a.b, a.x, a.out, None)
    op.smoother_sweep(AL2, BE2, a.b, a.out, a.x, a.outp)
    ctx.synchronize()
    a.assert_untouched(f"tile {tile}, two launches", ("x", "out", "outp"))
    return a.out.clone(), a.x.clone(), a.outp.clone()


@pytest.mark.parametrize("dofs,tz", [((87, 39, 9), 4), ((116, 20, 9), 5)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"tz{v}")
def test_two_launches_with_other_coefficients_and_exchanged_vectors(ctx, dofs, tz):
    prob = _problem(dofs)
    op = M.MatrixFreeLaplace(ctx, prob)
    x, b = _inputs(prob.n_dofs)
    ref = _pair(ctx, op, (8, 3, tz), x, b)
    got = _pair(ctx, op, (12, 2, tz), x, b)
    for name, g, r in zip(("first x_3", "second x_3", "second x_2"), got, ref):
        assert torch.isfinite(g).all()
        assert torch.equal(g, r), f"{dofs} tz {tz}: {name} differs from 8 x 3 in {(g != r).sum().item()} entries"
    # the second launch used its own coefficients: the first launch's set gives another result
    op.set_sweep_tile(12, 2, tz)
    a = Arena(b.size, got[0].cpu().numpy(), b)
    op.smoother_sweep(AL, BE, a.b, a.x, a.out, None)
    ctx.synchronize()
    assert not torch.equal(a.out, got[1])


def test_held_operands_against_long_double(ctx):
    """x_3 and x_2 of the 12 x 2 sweep per entry within (k + k_ref) u mag, u = 2^-53, k = 16 + 12 per term propagated through the
    recurrence (fp32_reference.py), for the signed coefficients above on a cell-wise varying material, from a vector and from zero."""
    dofs, tz = (87, 39, 9), 4
    prob = _problem(dofs)
    n = tuple(v - 1 for v in dofs)
    ref = F.Reference(n, prob.coefficient.cpu().numpy(), u=F.U64)
    assert ref.cell_constant and not (ref.coef == ref.coef[0, 0]).all()
    op = M.MatrixFreeLaplace(ctx, prob)
    x, b = _inputs(prob.n_dofs)
    for zero in (False, True):
        its = ref.sweep(np.zeros_like(x) if zero else x, b, AL, BE)
        units = ref.unit_sweep(its, b, AL, BE)
        out, outp = _run(ctx, op, (12, 2, tz), x, b, AL, BE, True, zero)
        for name, got, want, unit in (("x_3", out, its[-1], units[-1]), ("x_2", outp, its[-2], units[-2])):
            got = got.cpu().numpy()
            print(f"{dofs} tz {tz} zero guess {zero} {name}: worst |got - ref| / (u mag) = {F.worst_ratio(got, want, unit):.2f} (k = {ref.k_step})")
            F.assert_within(got, want, unit, ref.k_step + ref.k_ref, f"{dofs} tz {tz} zero guess {zero}: {name}")
