"""A hierarchy built with "release setup matrices" against its twin built without: which matrices let go of their CSR arrays,
the same bits from every entry point of the cycle, and the exports.

Mesh (52, 52, 52) and the parameters of test_gpu_block_coarse_cycle.py (first coarse level 2 * 26^3 = 35152 rows, the
smallest cubic mesh whose A_c gets a layout at all).  Every parameter set is built twice.  From the twin that kept its arrays
the released matrices are predicted -- regular rows, and node classes or block diagonals with at most 32768 listed rows, the
rule of SparseMatrixDevice::release_csr() read off form() -- and form()["csr_released"] of the other twin must say the same
for A_c and for A_l, P_l, P_l^T, P~_l of every level of the aggregation hierarchy.  `constant` repeats its stencils: A_c runs
from tables and is released, and so is at least one node-class matrix (asserted).  `linear` does not: A_c is stored planes and
keeps its arrays; whatever the rule predicts below it is asserted.

Between the twins, on the same inputs, torch.equal / byte equality (the release changes no kernel, table, plane or order of
summation): apply, coarse_apply, apply_block and coarse_apply_block on 3 and 4 guarded rows for V(1,1) and
pre_smoothing_levels 0; solve_cg and solve_cg_block (3 rows) on the symmetric cycle; solve_fgmres with restart 3 on both;
apply_f32 and apply_f32_block (3 rows) with "fine level precision" float."""
import ctypes as C

import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
from mfmg_amd.api import SparseMatrixDevice
from mfmg_amd.lib import check
from test_gpu_block_coarse_cycle import N, _amg_matrices, _guarded, _params, _untouched

pytestmark = pytest.mark.gpu

LIMIT = 32768
PAYLOAD32 = 0x7FC0BEEF                # a quiet float NaN nobody computes


def _twins(ctx, material, pre, **extra):
    """(kept, released): the same hierarchy with "release setup matrices" false and true."""
    prob = M.LaplaceProblem(N, material, device="cuda")
    out = []
    for release in (False, True):
        p = _params(True, pre)
        p.update(extra)
        p["release setup matrices"] = release
        out.append(M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, p))
    return out


def _matrix(h, level, which):
    p = C.c_void_p()
    check(h._lib.mfmg_hip_hierarchy_coarse_amg_get(h.handle, level, which, C.byref(p)))
    return SparseMatrixDevice(h.ctx, _handle=p, _borrowed=True, _keepalive=h)


def _predicted(f):
    return int(f["regular"] == 1 and (f["kind"] == 5 or (f["kind"] in (2, 3) and f["listed"] <= LIMIT)))


def _same_export(a, b):
    return (a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
            and a.data.tobytes() == b.data.tobytes())


def _vectors(n, seed, count, dtype=torch.float64):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return [torch.randn(n, dtype=dtype, device="cuda", generator=g) for _ in range(count)]


def _even(n):
    return n + 6 + (n & 1)


def _check_released_matrices(kept, released, material):
    """csr_released of every matrix as the rule predicts from the twin, and the exports; returns what was released."""
    mats_k, mats_r = _amg_matrices(kept), _amg_matrices(released)
    assert [(l, w) for l, w, f, width in mats_k] == [(l, w) for l, w, f, width in mats_r]
    assert mats_k[0][:2] == (0, 0)
    assert all(f["csr_released"] == 0 for l, w, f, width in mats_k)
    report = []
    for (l, which, fk, wk), (_, _, fr, wr) in zip(mats_k, mats_r):
        want = _predicted(fk)
        report.append((l, which, fk["kind"], fk["regular"], fk["listed"], fr["csr_released"]))
        assert fr["csr_released"] == want, (material, l, which, fk, fr)
        assert {k: v for k, v in fr.items() if k not in ("csr_released", "pairs", "twin_wide")} == \
               {k: v for k, v in fk.items() if k not in ("csr_released", "pairs", "twin_wide")}, (material, l, which)
        assert wr == (1 if want else wk)
        if want:
            with pytest.raises(L.MfmgError, match="released"):
                _matrix(released, l, which).to_scipy()
        else:
            assert _same_export(_matrix(released, l, which).to_scipy(), _matrix(kept, l, which).to_scipy()), (material, l, which)
    print(f"{material}: (level, which, kind, regular, listed, csr_released) {report}")
    # A_c is level 0, which 0 of the aggregation hierarchy
    fc = released.coarse_operator().form()
    assert fc["csr_released"] == report[0][5]
    if report[0][5]:
        with pytest.raises(L.MfmgError, match="released"):
            released.coarse_operator().to_scipy()
    else:
        assert _same_export(released.coarse_operator().to_scipy(), kept.coarse_operator().to_scipy())
    # coarse_amg_levels() exports A_l and P_l of every level: as a whole it fails when one of them is gone
    if any(rel for l, which, kind, reg, listed, rel in report if which in (0, 1)):
        with pytest.raises(L.MfmgError, match="released"):
            released.coarse_amg_levels()
    else:
        for (Ak, Pk, ck), (Ar, Pr, cr) in zip(kept.coarse_amg_levels(), released.coarse_amg_levels()):
            assert _same_export(Ak, Ar) and (Pk is None) == (Pr is None) and (Pk is None or _same_export(Pk, Pr)) and ck == cr
    kept.coarse_amg_levels()
    # what does not read the arrays works on both, with the same answers
    assert released.coarse_amg_setup_info() == kept.coarse_amg_setup_info()
    strip = lambda f: None if f is None else {k: v for k, v in f.items() if k not in ("csr_released", "pairs", "twin_wide")}
    assert [strip(f) for f in released.coarse_amg_smoothed_prolongator_forms()] == [strip(f) for f in kept.coarse_amg_smoothed_prolongator_forms()]
    assert _same_export(released.restrictor().to_scipy(), kept.restrictor().to_scipy())
    return report


def _block(ctx, h, call, b, x0, k, n):
    """call(B, X) on guarded blocks of the first k vectors; the k result rows."""
    ld = _even(n)
    B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
    call(B[1:k + 1], X[1:k + 1])
    ctx.synchronize()
    assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, n:]), "wrote outside its columns"
    assert _untouched(B[0]) and _untouched(B[k + 1]) and _untouched(B[1:k + 1, n:]), "wrote into the block b"
    assert all(torch.equal(B[c + 1, :n], b[c]) for c in range(k)), "b changed"
    return [X[c + 1, :n].clone() for c in range(k)]


def _cycle_outputs(ctx, h, symmetric):
    """Everything the comparison of the twins looks at, computed on one hierarchy from fixed inputs."""
    nf, nc = h.level_size(0), h.level_size(1)
    out = {}
    b, x0 = _vectors(nf, 23, 4), _vectors(nf, 24, 4)
    bc, xc = _vectors(nc, 21, 4), _vectors(nc, 22, 4)
    for name, call, rhs, start, n in (("apply", h.apply, b, x0, nf), ("coarse_apply", h.coarse_apply, bc, xc, nc)):
        x = start[0].clone()
        call(rhs[0], x)
        ctx.synchronize()
        out[name] = [x]
    for k in (3, 4):
        out[f"apply_block {k}"] = _block(ctx, h, h.apply_block, b, x0, k, nf)
        out[f"coarse_apply_block {k}"] = _block(ctx, h, h.coarse_apply_block, bc, xc, k, nc)
    for name in out:
        assert all(bool(torch.isfinite(v).all()) for v in out[name]), name
    # (the block calls give the bits of the one-vector calls on either twin: the first column says so here as well)
    assert torch.equal(out["apply_block 3"][0], out["apply"][0]) and torch.equal(out["coarse_apply_block 4"][0], out["coarse_apply"][0])
    histories = {}
    if symmetric:
        x = x0[0].clone()
        it, hist = h.solve_cg(b[0], x, 1e-8, 200)
        ctx.synchronize()
        out["solve_cg"] = [x]
        histories["solve_cg"] = ([it], [hist.tobytes()])
        ld = _even(nf)
        B, X = _guarded(b[:3], ld), _guarded(x0[:3], ld)
        its, hists, _ = h.solve_cg_block(B[1:4], X[1:4], [1e-8] * 3, 200)
        ctx.synchronize()
        assert _untouched(X[0]) and _untouched(X[4]) and _untouched(X[1:4, nf:])
        out["solve_cg_block"] = [X[c + 1, :nf].clone() for c in range(3)]
        histories["solve_cg_block"] = (list(its), [hh.tobytes() for hh in hists])
        assert its[0] == it and hists[0].tobytes() == hist.tobytes() and torch.equal(out["solve_cg_block"][0], x)
    x = x0[1].clone()
    it, hist = h.solve_fgmres(b[1], x, 1e-8, 200, restart=3)
    ctx.synchronize()
    out["solve_fgmres"] = [x]
    histories["solve_fgmres"] = ([it], [hist.tobytes()])
    assert it > 3                                          # (the restart was taken)
    return out, histories


def _assert_same(material, what, kept, released):
    (out_k, hist_k), (out_r, hist_r) = kept, released
    assert out_k.keys() == out_r.keys() and hist_k.keys() == hist_r.keys()
    for name in out_k:
        for c, (u, v) in enumerate(zip(out_k[name], out_r[name])):
            assert torch.equal(u, v), f"{material} {what}: {name}, column {c}: {(u != v).sum().item()} entries differ between the twins"
    for name in hist_k:
        assert hist_k[name][0] == hist_r[name][0], f"{material} {what}: {name}: iteration counts {hist_k[name][0]} and {hist_r[name][0]}"
        assert hist_k[name][1] == hist_r[name][1], f"{material} {what}: {name}: the residual histories differ"


@pytest.mark.parametrize("pre", [None, 0], ids=["V11", "V01"])
@pytest.mark.parametrize("material", ["constant", "linear"])
def test_released_hierarchy_is_the_same_cycle(ctx, material, pre):
    kept, released = _twins(ctx, material, pre)
    report = _check_released_matrices(kept, released, material)
    n_released = sum(rel for *_, rel in report)
    if material == "constant":
        assert report[0][:2] == (0, 0) and report[0][5] == 1, report                      # A_c
        assert any(kind == 5 and rel for l, which, kind, reg, listed, rel in report), report
    else:
        fc = kept.coarse_operator().form()
        assert fc["regular"] == 0 and fc["stored_kernel"] == "sym_split" and report[0][5] == 0, (fc, report)
    what = f"pre_smoothing_levels {pre}, {n_released} matrices released"
    _assert_same(material, what, _cycle_outputs(ctx, kept, pre is None), _cycle_outputs(ctx, released, pre is None))


def _guarded32(cols, ld):
    blk = torch.full((len(cols) + 2, ld), PAYLOAD32, dtype=torch.int32, device="cuda").view(torch.float32)
    for c, v in enumerate(cols):
        blk[c + 1, :v.numel()] = v
    return blk


def _untouched32(t):
    return bool((t.contiguous().view(torch.int32) == PAYLOAD32).all().item())


@pytest.mark.parametrize("material", ["constant", "linear"])
def test_released_float_hierarchy_is_the_same_cycle(ctx, material):
    """"fine level precision" float: the matrices below the FP32 fine level are rounded to float and released by the same
    rule; apply_f32 and apply_f32_block of the two float twins agree bit for bit."""
    kept, released = _twins(ctx, material, None, **{"fine level precision": "float"})
    report = _check_released_matrices(kept, released, material + ", float")
    if material == "constant":
        assert report[0][5] == 1, report
    nf = kept.level_size(0)
    b, x0 = _vectors(nf, 33, 3, torch.float32), _vectors(nf, 34, 3, torch.float32)
    ld = _even(nf)
    got = []
    for h in (kept, released):
        x = x0[0].clone()
        h.apply_f32(b[0], x)
        B, X = _guarded32(b, ld), _guarded32(x0, ld)
        h.apply_f32_block(B[1:4], X[1:4])
        ctx.synchronize()
        assert _untouched32(X[0]) and _untouched32(X[4]) and _untouched32(X[1:4, nf:])
        assert _untouched32(B[0]) and _untouched32(B[4]) and _untouched32(B[1:4, nf:])
        assert bool(torch.isfinite(x).all()) and torch.equal(X[1, :nf], x)
        got.append([x] + [X[c + 1, :nf].clone() for c in range(3)])
    for c, (u, v) in enumerate(zip(*got)):
        assert torch.equal(u, v), f"{material}: float cycle, output {c}: {(u != v).sum().item()} entries differ between the twins"
