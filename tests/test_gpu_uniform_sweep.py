"""The stencil sweep of a uniform coefficient (mf_cheb_fused.hip: mf_cheb_fused_uniform_kernel) entry by entry against a long
double restatement: the three-term recurrence
    x_1 = x_0 - beta_1 D^-1 (A x_0 - b),   x_s = x_{s-1} + alpha_s (x_{s-1} - x_{s-2}) - beta_s D^-1 (A x_{s-1} - b)
with the assembled 27-point operator on the free DoFs (A = c sum_d 2 f_d K_d (x) M (x) M, K = (2, -1), M = (4/3, 1/3),
f_d = |cell| / 8 / h_d^2; Dirichlet values enter as zero) and identity rows with D^-1 = 1 on the Dirichlet DoFs, from seeded random
x_0 and b.

Tolerance: none is fixed here.  Per case the largest entry-wise error |got - ref| of the mode-space sweep (the kernels of before:
the same operator with MFMG_MF_UNIFORM_SWEEP=0) against the same reference is measured, and the stencil sweep must stay within
twice that -- it does fewer operations per entry, the factor is for their different order.  Both errors are printed.

Sizes are DoFs per direction, chosen for the edges of the tiling (58 owned columns per full chunk column, 19 owned rows per
y-tile of twelve wavefronts of two rows): see CASES.  Checked: x_3 and, where requested, x_2; the sweep from a zero guess against
the same sweep on a zeroed vector, bit for bit; independence of the tiling, bit for bit (the default height and two others; the
other tile shapes of the three-term sweep, which run the same stencil as mf_cheb_fused_uniform_rows_kernel; the kernel has no
split narrow launch); that the operator reports a uniform coefficient and that every launch counted here was a stencil kernel
(uniform_sweep_launches) -- a silent fall-back would pass every parity check."""
import functools
import os

import numpy as np
import pytest
import torch

import mfmg_amd as M

pytestmark = pytest.mark.gpu

LD = np.longdouble
AL = [0.0, 0.23, 0.31]
BE = [0.61, 0.87, 0.79]
# (DoFs per direction, two z-tile heights beside the default)
CASES = [((5, 5, 5), (2, 5)),        # every free node next to a face
         ((59, 20, 9), (2, 4)),      # exactly one wide column of 58 owned columns, a narrow one of 1; one full y-tile of 19 rows and one row more
         ((60, 21, 9), (3, 9)),      # a narrow last column of two columns, a second y-tile of two rows
         ((84, 39, 70), (7, 33)),    # a narrow column of 26 that pairs two full y-tiles and leaves a third (one row) half idle; several z-tiles
         ((257, 5, 5), (2, 5))]      # five chunk columns
IDS = ["x".join(map(str, c[0])) for c in CASES]
OTHER_SHAPES = [(8, 3, 0), (4, 3, 8), (2, 4, 7), (8, 2, 64)]      # (wavefronts, cell rows, layers)


def _stencil(a, axis, d0, d1):
    out = d0 * a
    lo = [slice(None)] * 3
    hi = [slice(None)] * 3
    lo[axis], hi[axis] = slice(0, -1), slice(1, None)
    out[tuple(hi)] += d1 * a[tuple(lo)]
    out[tuple(lo)] += d1 * a[tuple(hi)]
    return out


class Restatement:
    def __init__(self, dofs, h, c):
        self.shape = tuple(reversed(dofs))                     # (Nz, Ny, Nx), x fastest
        free = np.zeros(self.shape, bool)
        free[1:-1, 1:-1, 1:-1] = True
        self.free = free
        h = [LD(v) for v in h]
        vol = h[0] * h[1] * h[2]
        self.f = [vol / LD(8) / (v * v) for v in h]
        self.c = LD(c)
        self.dinv = np.where(free, LD(1) / (self.c * LD(64) / LD(9) * (self.f[0] + self.f[1] + self.f[2])), LD(1))

    def vmult(self, x):
        u = np.where(self.free, x, LD(0))
        k, m = (LD(2), LD(-1)), (LD(4) / LD(3), LD(1) / LD(3))
        y = np.zeros(self.shape, LD)
        for d in range(3):                                      # direction d = axis 2 - d
            t = u
            for e in range(3):
                t = _stencil(t, 2 - e, *(k if e == d else m))
            y += LD(2) * self.f[d] * self.c * t
        return np.where(self.free, y, x)                        # identity rows

    def sweep(self, x0, b):
        its = [x0]
        for s in range(3):
            x = its[-1]
            nxt = x - LD(BE[s]) * self.dinv * (self.vmult(x) - b)
            if s > 0:
                nxt = nxt + LD(AL[s]) * (x - its[-2])
            its.append(nxt)
        return its


@functools.lru_cache(maxsize=None)
def _case(dofs):
    cells = tuple(v - 1 for v in dofs)
    prob = M.LaplaceProblem(cells, "constant", device="cuda")
    c = prob.coefficient.cpu().numpy()
    assert (c == c.flat[0]).all()
    ref = Restatement(dofs, prob.h, c.flat[0])
    rng = np.random.default_rng([11, *dofs])
    x = rng.standard_normal(ref.shape)
    b = rng.standard_normal(ref.shape)
    its = ref.sweep(x.astype(LD), b.astype(LD))
    zits = ref.sweep(np.zeros(ref.shape, LD), b.astype(LD))
    return prob, x.ravel(), b.ravel(), [v.ravel() for v in its], [v.ravel() for v in zits]


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _sweep(ctx, op, b, x, with_prev=True):
    out, outp = _nan(b.numel()), (_nan(b.numel()) if with_prev else None)
    op.smoother_sweep(AL, BE, b, x, out, outp)
    ctx.synchronize()
    return out, outp


def _mode_space(ctx, op, b, x):
    """The sweep of before on the same operator (the A/B switch is read at every sweep)."""
    before = op.uniform_sweep_launches()
    os.environ["MFMG_MF_UNIFORM_SWEEP"] = "0"
    try:
        res = _sweep(ctx, op, b, x)
    finally:
        del os.environ["MFMG_MF_UNIFORM_SWEEP"]
    assert op.uniform_sweep_launches() == before
    return res


def _err(got, ref):
    return float(np.abs(got.cpu().numpy().astype(LD) - ref).max())


@pytest.mark.parametrize("dofs,heights", CASES, ids=IDS)
def test_stencil_sweep_against_long_double(ctx, dofs, heights):
    assert np.finfo(LD).nmant >= 63
    prob, x, b, its, zits = _case(dofs)
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.cell_constant_layout() and op.sweep_available(3) and op.uniform_coefficient()
    assert op.get_sweep_tile(3)[:2] == (12, 2)
    xd, bd, zd = _gpu(x), _gpu(b), torch.zeros(b.size, dtype=torch.float64, device="cuda")
    n0 = op.uniform_sweep_launches()
    out, outp = _sweep(ctx, op, bd, xd)
    assert op.uniform_sweep_launches() == n0 + 1, "the sweep did not take the stencil kernel"
    old, oldp = _mode_space(ctx, op, bd, xd)
    for what, got, parent, ref in (("x_3", out, old, its[3]), ("x_2", outp, oldp, its[2])):
        e_new, e_old = _err(got, ref), _err(parent, ref)
        print(f"{dofs} {what}: largest entry-wise error, stencil sweep {e_new:.3e}, mode-space sweep {e_old:.3e}")
        assert np.isfinite(e_new) and e_old > 0.0
        assert e_new <= 2.0 * e_old, f"{dofs} {what}: {e_new:.3e} beyond twice the mode-space sweep's {e_old:.3e}"
    # x_2 not requested: the same x_3
    only, none = _sweep(ctx, op, bd, xd, with_prev=False)
    assert none is None and torch.equal(only, out)
    # from a zero guess: within twice the mode-space sweep's error; the bits of the sweep on a zeroed vector
    zout, zoutp = _sweep(ctx, op, bd, None)
    zold, zoldp = _mode_space(ctx, op, bd, None)
    for what, got, parent, ref in (("x_3", zout, zold, zits[3]), ("x_2", zoutp, zoldp, zits[2])):
        e_new, e_old = _err(got, ref), _err(parent, ref)
        print(f"{dofs} from zero {what}: largest entry-wise error, stencil sweep {e_new:.3e}, mode-space sweep {e_old:.3e}")
        assert np.isfinite(e_new) and e_old > 0.0
        assert e_new <= 2.0 * e_old, f"{dofs} from zero {what}: {e_new:.3e} beyond twice the mode-space sweep's {e_old:.3e}"
    onz, onzp = _sweep(ctx, op, bd, zd)
    assert torch.equal(zout, onz) and torch.equal(zoutp, onzp), "from zero differs from the sweep on a zeroed vector"
    # independence of the z-tiling, bit for bit
    tz0 = op.get_sweep_tile(3)[2]
    launches = op.uniform_sweep_launches()
    for tile in [(12, 2, tz) for tz in heights] + OTHER_SHAPES:
        op.set_sweep_tile(*tile)
        assert op.get_sweep_tile(3)[:2] == tile[:2] and (tile[2] == 0 or op.get_sweep_tile(3)[2] == tile[2])
        o, p = _sweep(ctx, op, bd, xd)
        assert torch.equal(o, out) and torch.equal(p, outp), f"{dofs}: tile {tile} differs from the default (z-tiles of {tz0}) in {(o != out).sum().item()} entries"
        launches += 1
        if tile[1] == 3 or tile[:2] == (12, 2):              # (the shapes that offer the sweep from a zero guess)
            o, p = _sweep(ctx, op, bd, None)
            assert torch.equal(o, zout) and torch.equal(p, zoutp), f"{dofs}: tile {tile} differs from the default from a zero guess"
            launches += 1
    assert op.uniform_sweep_launches() == launches
    op.set_sweep_tile(0, 0, 0)
    assert op.get_sweep_tile(3)[2] == tz0


def test_cases_reach_the_edges_they_name():
    own_cols, own_rows = 64 - 2 * 3, 12 * 2 - 2 * 3 + 1
    assert (own_cols, own_rows) == (58, 19)
    narrow = {d: d[0] - (d[0] - 1) // own_cols * own_cols for d, _ in CASES if d[0] > own_cols}
    y_tiles = {d: -(-d[1] // own_rows) for d, _ in CASES}
    assert narrow[(59, 20, 9)] == 1 and y_tiles[(59, 20, 9)] == 2 and 20 - own_rows == 1
    assert narrow[(60, 21, 9)] == 2 and y_tiles[(60, 21, 9)] == 2 and 21 - own_rows == 2
    assert narrow[(84, 39, 70)] == 26 and y_tiles[(84, 39, 70)] == 3
    assert narrow[(257, 5, 5)] == 25 and -(-257 // own_cols) == 5
    assert all(max(h) <= d[2] and len(set(h)) == 2 for d, h in CASES)


def test_reference_arithmetic_keeps_its_kernels(ctx):
    """The reference arithmetic runs the kernels of before: the bits of the term-by-term sequence."""
    prob, x, b, its, _ = _case((60, 21, 9))
    op = M.MatrixFreeLaplace(ctx, prob)
    xd, bd = _gpu(x), _gpu(b)
    n0 = op.uniform_sweep_launches()
    op.set_sweep_reference(True)
    terms = [xd]
    for k in range(3):
        o = _nan(xd.numel())
        op.smoother_step(bd, terms[-1], terms[-2] if k > 0 else None, AL[k], BE[k], o)
        terms.append(o)
    for tile in ((0, 0, 0), (12, 2, 0), (8, 3, 0)):
        op.set_sweep_tile(*tile)
        o, p = _sweep(ctx, op, bd, xd)
        assert torch.equal(o, terms[3]) and torch.equal(p, terms[2]), tile
    op.set_sweep_reference(False)
    assert op.uniform_sweep_launches() == n0
