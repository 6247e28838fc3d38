"""The three-term FP64 sweep of twelve wavefronts of two rows with D^-1 read from the operator's vector
(mf_cheb_fused_wg12d_kernel, the default where the vector exists) against the same sweep with D^-1 derived from the coefficient
sums (mf_cheb_fused_wg12_kernel): the vector holds the bits the kernels derive, so the two sweeps are equal with torch.equal --
both arithmetics, with and without x_{K-1}, from the zero guess where the sweep offers it, on vectors at a 16-byte boundary and
8 bytes past one, into outputs that are NaN before every launch.

Shapes are those of test_gpu_sweep_12x2.py, (Nx, Ny, Nz) in DoFs with the z-tile (0: the sweep's own): a tile larger than the
mesh, Ny at one y-tile / one plus a row / two plus a row, a narrow last chunk column with three y-tiles, 117 = 58 + 58 + 1 and
116 = 58 + 58 node columns, z-tiles shorter (4) and longer (5) than the fill and drain of three terms.  Materials: constant,
`discontinuous` made one coefficient per cell, and one coefficient per cell drawn from 10^U(-3, 3).

The vector itself, per entry, against the reciprocal of the diagonal in long double (tests/fp32_reference.py, Reference at
2^-53) within K_DINV_F64 u D^-1, the bound that module derives for D^-1 in FP64; the vector's own chain is shorter (kd rounded
on the host, three sums, a product, a division).  At Dirichlet DoFs, whose entries no kernel reads, finiteness alone.

By default these operators report "stored"; under MFMG_MF_SWEEP_DINV=derived, read at construction (checked in a fresh child
process), they report "derived", hold no vector and refuse to be switched."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
import fp32_reference as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AL = [0.0, 0.23, 0.31]
BE = [0.61, 0.87, 0.79]
# (DoFs, z-tile: 0 = the sweep's own choice): test_gpu_sweep_12x2.py
CASES = [((9, 9, 9), 0), ((65, 19, 7), 0), ((65, 20, 7), 0), ((65, 39, 7), 0), ((79, 40, 9), 0), ((117, 21, 9), 0), ((116, 21, 9), 0),
         ((33, 25, 23), 4), ((33, 25, 23), 5)]
MATERIALS = ["constant", "discontinuous", "cellwise6"]


def _problem(dofs, material):
    n = tuple(v - 1 for v in dofs)
    if material == "cellwise6":  # one coefficient per cell, 10^U(-3, 3)
        prob = M.LaplaceProblem(n, "constant", device="cuda")
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        r = torch.rand(prob.n_cells_total, 1, dtype=torch.float64, device="cuda", generator=g)
        prob.coefficient = (10.0 ** (6.0 * r - 3.0)).expand(-1, 8).contiguous()
        return prob
    prob = M.LaplaceProblem(n, material, device="cuda")
    if material == "discontinuous":  # one coefficient per cell: that of its first corner
        prob.coefficient = prob.coefficient[:, :1].expand(-1, 8).contiguous()
    return prob


@functools.lru_cache(maxsize=None)
def _operator(ctx, dofs, material):
    prob = _problem(dofs, material)
    assert prob.n_dofs == dofs[0] * dofs[1] * dofs[2]
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.sweep_available(3) and op.cell_constant_layout() and not op.diagonal_in_record()
    return prob, op


def _vectors(n_dofs, seed, shift):
    """x, b and a NaN-filled (out, out_prev) maker; shift = 1: every vector starts 8 bytes past a 16-byte boundary."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)

    def place(t):
        buf = torch.empty(n_dofs + 2, dtype=torch.float64, device="cuda")
        first = ((-buf.data_ptr() // 8) % 2 + shift) % 2    # (buf[first] lies on a 16-byte boundary for shift = 0)
        v = buf[first:first + n_dofs]
        assert v.data_ptr() % 16 == 8 * shift
        v.copy_(t)
        return v

    x = place(torch.rand(n_dofs, dtype=torch.float64, device="cuda", generator=g))
    b = place(torch.rand(n_dofs, dtype=torch.float64, device="cuda", generator=g))
    nan = lambda: place(torch.full((n_dofs,), float("nan"), dtype=torch.float64, device="cuda"))
    return x, b, nan


def _sweep(ctx, op, source, b, x, nan, with_prev):
    op.set_sweep_diagonal(source)
    assert op.sweep_diagonal() == source
    out, outp = nan(), (nan() if with_prev else None)
    op.smoother_sweep(AL, BE, b, x, out, outp)
    ctx.synchronize()
    return out, outp


@pytest.mark.parametrize("material", MATERIALS)
@pytest.mark.parametrize("dofs,tz", CASES)
def test_stored_diagonal_sweep_equals_derived(ctx, dofs, tz, material):
    prob, op = _operator(ctx, dofs, material)
    assert op.sweep_diagonal() == "stored", "an operator that can take the 12 x 2 sweep reads its D^-1 vector by default"
    try:
        op.set_sweep_tile(12, 2, tz)
        tile = tuple(op.get_sweep_tile(3))
        assert tile[:2] == (12, 2) and (tz == 0 or tile[2] == tz), tile
        for shift in (0, 1):
            x, b, nan = _vectors(prob.n_dofs, 5 + shift, shift)
            for reference in (False, True):
                op.set_sweep_reference(reference)
                starts = [("x_0 read", x)] + ([] if reference else [("zero guess", None)])   # (offered in mode space only)
                for what, x0 in starts:
                    for with_prev in (True, False):
                        tag = f"{dofs} tz {tz} {material}, reference arithmetic {reference}, {what}, out_prev {with_prev}, offset {8 * shift} B"
                        got, gotp = _sweep(ctx, op, "stored", b, x0, nan, with_prev)
                        ref, refp = _sweep(ctx, op, "derived", b, x0, nan, with_prev)
                        assert torch.isfinite(ref).all(), tag
                        assert torch.equal(got, ref), f"{tag}: x_3 with the stored D^-1 differs from the derived one"
                        if with_prev:
                            assert torch.isfinite(refp).all(), tag
                            assert torch.equal(gotp, refp), f"{tag}: x_2 with the stored D^-1 differs from the derived one"
    finally:
        op.set_sweep_reference(False)
        op.set_sweep_tile(0, 0, 0)
        op.set_sweep_diagonal("stored")


@pytest.mark.parametrize("material", MATERIALS)
@pytest.mark.parametrize("dofs", sorted({d for d, _ in CASES}))
def test_sweep_diagonal_inverse_against_long_double(ctx, dofs, material):
    prob, op = _operator(ctx, dofs, material)
    ref = F.Reference(tuple(v - 1 for v in dofs), prob.coefficient.cpu().numpy(), u=F.U64)
    got = op.sweep_diagonal_inverse().cpu().numpy()
    assert got.shape == (prob.n_dofs,)
    free = ~ref.con
    assert free.any() and ref.con.any()
    assert np.isfinite(got).all(), "entries of Dirichlet DoFs are finite too"
    bound = F.K_DINV_F64 * F.U64 * ref.dinv
    bad = F.beyond(got, ref.dinv, bound) & free
    ratio = F.worst_ratio(got[free], ref.dinv[free], (F.U64 * ref.dinv)[free])
    print(f"{dofs} {material}: worst |D^-1 - ref| / (u D^-1) = {ratio:.2f} (bound {F.K_DINV_F64})")
    assert not bad.any(), f"{dofs} {material}: {int(bad.sum())} entries of the D^-1 vector beyond {F.K_DINV_F64} u (worst {ratio:.2f})"


CHILD = """
import sys
sys.path[:0] = [{root!r}, {root!r} + "/oracle"]
import torch
import mfmg_amd as M
from mfmg_amd import lib as L
ctx = M.Context()
prob = M.LaplaceProblem((64, 19, 6), "constant", device="cuda")
op = M.MatrixFreeLaplace(ctx, prob)
assert op.sweep_available(3) and tuple(op.get_sweep_tile(3))[:2] == (12, 2)
print("sweep diagonal:", op.sweep_diagonal())
for call in (lambda: op.set_sweep_diagonal("stored"), op.sweep_diagonal_inverse):
    try:
        call()
        print("accepted")
    except L.MfmgNotImplementedError:
        print("refused")
op.set_sweep_diagonal("derived")
g = torch.Generator(device="cuda")
g.manual_seed(3)
x, b = (torch.rand(prob.n_dofs, dtype=torch.float64, device="cuda", generator=g) for _ in range(2))
out = torch.full_like(b, float("nan"))
op.smoother_sweep([0.0, 0.23, 0.31], [0.61, 0.87, 0.79], b, x, out)
ctx.synchronize()
print("finite:", bool(torch.isfinite(out).all()))
"""


def test_environment_switch_builds_no_vector(mfmg_lib):
    env = dict(os.environ, MFMG_MF_SWEEP_DINV="derived")
    res = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    lines = res.stdout.strip().splitlines()
    assert lines == ["sweep diagonal: derived", "refused", "refused", "finite: True"], res.stdout


def test_operators_without_the_sweep_hold_no_vector(ctx):
    """Eight coefficients per cell (no sweep) and D^-1 kept in the records (the 12 x 2 sweep does not run there): "derived", no vector."""
    varying = M.MatrixFreeLaplace(ctx, M.LaplaceProblem((8, 8, 8), "linear", device="cuda"))
    assert not varying.cell_constant_layout() and varying.sweep_diagonal() == "derived"
    with pytest.raises(L.MfmgNotImplementedError):
        varying.set_sweep_diagonal("stored")
    with pytest.raises(L.MfmgNotImplementedError):
        varying.sweep_diagonal_inverse()
    ctx.set_stored_diagonal(True)
    try:
        in_records = M.MatrixFreeLaplace(ctx, M.LaplaceProblem((8, 8, 8), "constant", device="cuda"))
    finally:
        ctx.set_stored_diagonal(False)
    assert in_records.diagonal_in_record() and in_records.sweep_diagonal() == "derived"
    with pytest.raises(L.MfmgNotImplementedError):
        in_records.set_sweep_diagonal("stored")
