"""The cycle on a block of vectors (Hierarchy.apply_block, vmult_block, smoother_apply_block) against k calls of the one-vector
entry point, bit for bit.

Setup: (16,16,16) and (20,12,10) cells, Chebyshev(3), two eigenvectors, 2 x 2 x 2 agglomerates, the default coarse solver of the
small cases of test_gpu_hierarchy.py.  `linear` and `discontinuous` take the block kernel on the fine level, `constant` the loop
over the columns; `linear` under deal.II's numbering in caller mode (ids read from the records) and with "internal numbering"
lexicographic (columns gathered into and scattered out of the library's block workspace).  Each with "is preconditioner" true and
false and k = 1, 3, 4, 7 in that order on ONE hierarchy: the workspace, one group wide, grows from a group of two to a group of
four.  The leading dimension is n_dofs + 7 (n_dofs is odd for both meshes; a block needs an even one), with a guard column on
either side that keeps its NaN payload."""
import pytest
import torch

import mfmg_amd as M
from mfmg_amd.api import block_groups

pytestmark = pytest.mark.gpu

KS = [1, 3, 4, 7]
K_MAX = max(KS)
DEGREE = 3
PAYLOAD = 0x7FF8DEAD0000BEEF          # a quiet NaN nobody computes
CASES = [((16, 16, 16), "linear", None, None), ((20, 12, 10), "linear", None, None),
         ((16, 16, 16), "discontinuous", None, None), ((20, 12, 10), "discontinuous", None, None),
         ((16, 16, 16), "constant", None, None), ((20, 12, 10), "constant", None, None),
         ((16, 16, 16), "linear", "dealii", "caller"), ((16, 16, 16), "linear", "dealii", "lexicographic")]


def _params(is_preconditioner, mode):
    p = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": is_preconditioner,
         "max levels": 2, "smoother": {"type": "Chebyshev", "degree": DEGREE, "smoothing_range": 20.0}}
    if mode is not None:
        p["internal numbering"] = mode
    return p


def _guarded(cols, ld):
    blk = torch.full((len(cols) + 2, ld), PAYLOAD, dtype=torch.int64, device="cuda").view(torch.float64)
    for c, v in enumerate(cols):
        blk[c + 1, :v.numel()] = v
    return blk


def _untouched(t):
    return bool((t.contiguous().view(torch.int64) == PAYLOAD).all().item())


@pytest.mark.parametrize("is_preconditioner", [True, False], ids=["preconditioner", "solver"])
@pytest.mark.parametrize("n,material,numbering,mode", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_block_entry_points_equal_the_one_vector_ones(ctx, n, material, numbering, mode, is_preconditioner):
    kw = {"dof_numbering": M.dealii_numbering(n)} if numbering == "dealii" else {}
    prob = M.LaplaceProblem(n, material, device="cuda", **kw)
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, _params(is_preconditioner, mode))
    nd = h.level_size(0)
    ld = nd + 6 + (nd & 1)
    assert ld > nd + 1 and ld % 2 == 0
    op = M.MatrixFreeLaplace(ctx, prob)
    block = material != "constant"
    assert op.cell_constant_layout() == (not block)
    width = h.block_info()["width"]
    assert width == (4 if block else 1), (n, material, numbering, mode, width)

    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    b = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
    x0 = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
    entries = {"apply": (lambda bb, xx: h.apply(bb, xx), lambda B, X: h.apply_block(B, X)),
               "vmult": (lambda bb, xx: h.vmult(xx, bb), lambda B, X: h.vmult_block(X, B)),
               "smoother": (lambda bb, xx: h.smoother_apply(0, bb, xx), lambda B, X: h.smoother_apply_block(0, B, X))}
    single = {}
    for name, (one, _) in entries.items():
        single[name] = []
        for c in range(K_MAX):
            x = x0[c].clone()
            one(b[c], x)
            single[name].append(x)
    ctx.synchronize()
    assert all(bool(torch.isfinite(x).all().item()) for xs in single.values() for x in xs)

    per_group = {}
    for k in KS:                                             # (ascending: the workspace regrows from a group of two to a group of four)
        wide = len([w for w in block_groups(k) if w > 1])
        for name, (_, blk) in entries.items():
            B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
            ctx.profile_enable(True, "mf_laplace_block_kernel")
            blk(B[1:k + 1], X[1:k + 1])
            launches = ctx.profile_query("mf_laplace_block_kernel")[0]
            ctx.profile_enable(False)
            ctx.synchronize()
            what = f"{n} {material} {numbering} {mode} preconditioner {is_preconditioner} k {k} {name}"
            for c in range(k):
                got = X[c + 1, :nd]
                assert torch.equal(got, single[name][c]), f"{what}: column {c} differs from the one-vector entry point in {(got != single[name][c]).sum().item()} entries"
            assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nd:]), f"{what}: wrote outside its columns"
            assert _untouched(B[0]) and _untouched(B[k + 1]) and _untouched(B[1:k + 1, nd:]), f"{what}: wrote into b"
            assert all(torch.equal(B[c + 1, :nd], b[c]) for c in range(k)), f"{what}: b changed"
            info = h.block_info()
            assert info["width"] == width and info["block_launches"] == launches, (what, info, launches)
            if not block:
                assert info["block_launches"] == 0 and info["column_launches"] == k, (what, info)
                continue
            # the groups of mfmg_hip_block_groups: every group of 4 or 2 runs the same launches of the block kernel, the single
            # column the one-vector entry point
            assert info["column_launches"] == k % 2, (what, info)
            if wide == 0:
                assert launches == 0, (what, launches)
                continue
            assert launches % wide == 0, (what, launches, wide)
            per_group.setdefault(name, launches // wide)
            assert launches == per_group[name] * wide, (what, launches, per_group)
            if name == "smoother":
                assert per_group[name] == DEGREE, (what, per_group)
            else:   # pre- and post-smoothing, and the residual unless the restrictor forms R (A x - b) in one pass
                assert per_group[name] in (2 * DEGREE, 2 * DEGREE + 1), (what, per_group)
