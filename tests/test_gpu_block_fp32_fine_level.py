"""The FP32 fine level on blocks of float vectors: Hierarchy.apply_f32_block against k calls of apply_f32 on the same hierarchy,
bit for bit, and solve_fgmres_block(preconditioner="float") running that block cycle.

Hierarchies as in test_gpu_block_fgmres.py: Chebyshev(3), two eigenvectors, 2 x 2 x 2 agglomerates, "fine level precision" float.
(16,16,16) `linear` with the symmetric cycle and with the V(0,1) coarse cycle; `linear` under deal.II's numbering with "internal
numbering" lexicographic (the columns are gathered and scattered one by one); (20,12,10) `discontinuous`; (16,16,16) `constant`,
whose float smoother is a multi-term sweep: the loop over the columns.  "is preconditioner" true, and false from a non-zero x.
k = 1, 2, 3, 4, 5, 7 are the groups 1; 2; 2+1; 4; 4+1; 4+2+1.  The blocks carry a guard column before and after and the entries
[n_dofs, ld) of every column; all keep their 32-bit NaN payload.

Launch counts, derived from the schedule: a wide group (4 or 2 columns) runs 2 x "n_smoothing_steps" x degree smoother terms and,
unless the restrictor forms R (A x - b) in one pass on float vectors (restrict_residual_f32 then accepts the call), one residual
as launches of mf_laplace_block_f32_kernel; a group of one goes through apply_f32.  For the solve the groups of every iteration
follow from the one-vector iteration counts: a column is live in iteration t while t <= its iterations, the live slots are cut
into maximal runs and those into the groups of block_groups, a restart packs the live columns into the first slots, and a column
whose count is reached at a restart without the recorded residual meeting its tolerance retires at that cycle start, after the
packing."""
import ctypes as C

import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
from mfmg_amd.api import block_groups

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 4, 5, 7]
K_MAX = max(KS)
MAX_ITERATIONS = 100
PAYLOAD = 0x7FC0BEEF                  # a quiet float NaN nobody computes
PAYLOAD64 = 0x7FF8DEAD0000BEEF
CHEB3 = {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}
V01 = {"type": "amg", "amg": {"coarsest_size": 300, "pre_smoothing_levels": 0}}   # the non-symmetric coarse cycle
FLOAT = {"fine level precision": "float"}
# name: (nodes, material, numbering, extra parameters, the float operator has the block kernel)
CASES = {"linear_symmetric": ((16, 16, 16), "linear", None, dict(FLOAT), True),
         "linear_v01": ((16, 16, 16), "linear", None, dict(FLOAT, solver=V01), True),
         "linear_dealii_lexicographic": ((16, 16, 16), "linear", "dealii", dict(FLOAT, **{"internal numbering": "lexicographic"}), True),
         "discontinuous": ((20, 12, 10), "discontinuous", None, dict(FLOAT), True),
         "constant": ((16, 16, 16), "constant", None, dict(FLOAT), False),
         "linear_from_x": ((16, 16, 16), "linear", None, dict(FLOAT, **{"is preconditioner": False}), True),
         "constant_from_x": ((16, 16, 16), "constant", None, dict(FLOAT, **{"is preconditioner": False}), False)}


def _params(extra):
    p = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": True,
         "max levels": 2, "smoother": dict(CHEB3)}
    p.update(extra)
    return p


_built = {}


def _case(ctx, name):
    """the hierarchy of a case with K_MAX float right-hand sides and start vectors: built once, shared, left unchanged"""
    if name not in _built:
        n, material, numbering, extra, block = CASES[name]
        kw = {"dof_numbering": M.dealii_numbering(n)} if numbering == "dealii" else {}
        prob = M.LaplaceProblem(n, material, device="cuda", **kw)
        h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, _params(extra))
        nd = h.level_size(0)
        g = torch.Generator(device="cuda")
        g.manual_seed(23)
        b = [torch.randn(nd, dtype=torch.float32, device="cuda", generator=g) for _ in range(K_MAX)]
        x0 = [torch.randn(nd, dtype=torch.float32, device="cuda", generator=g) for _ in range(K_MAX)]
        # the reference, once per column: apply_f32 on a copy of x0
        ref = []
        for c in range(K_MAX):
            x = x0[c].clone()
            h.apply_f32(b[c], x)
            ref.append(x)
        ctx.synchronize()
        # launches of the block kernel per wide group, from the schedule
        degree = h.smoother_info()[0]
        try:
            h.restrict_residual_f32(x0[0], b[0], torch.empty(h.level_size(1), dtype=torch.float64, device="cuda"))
            one_pass = True
        except L.MfmgNotImplementedError:
            one_pass = False
        ctx.synchronize()
        per_group = 2 * 1 * degree + (0 if one_pass else 1)
        _built[name] = dict(h=h, prob=prob, nd=nd, b=b, x0=x0, ref=ref, block=block, per_group=per_group, one_pass=one_pass,
                            from_x=not _params(extra)["is preconditioner"])
    return _built[name]


def _guarded(cols, ld, dtype=torch.float32):
    if dtype == torch.float32:
        blk = torch.full((len(cols) + 2, ld), PAYLOAD, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        blk = torch.full((len(cols) + 2, ld), PAYLOAD64, dtype=torch.int64, device="cuda").view(torch.float64)
    for c, v in enumerate(cols):
        blk[c + 1, :v.numel()] = v
    return blk


def _untouched(t):
    if t.dtype == torch.float32:
        return bool((t.contiguous().view(torch.int32) == PAYLOAD).all().item())
    return bool((t.contiguous().view(torch.int64) == PAYLOAD64).all().item())


def _groups(k):
    w = block_groups(k)
    return len([v for v in w if v > 1]), len([v for v in w if v == 1])


@pytest.mark.parametrize("name", list(CASES))
def test_apply_f32_block_equals_apply_f32(ctx, name):
    case = _case(ctx, name)
    h, nd, b, x0, ref = case["h"], case["nd"], case["b"], case["x0"], case["ref"]
    ld = nd + 6 + (nd & 1)
    assert h.sweep_terms_f32() == (0 if case["block"] else 3), name
    if case["from_x"]:
        # (otherwise the start vector is never read and the case shows nothing)
        z = torch.zeros_like(x0[0])
        h.apply_f32(b[0], z)
        ctx.synchronize()
        assert not torch.equal(z, ref[0])
    for k in KS:
        B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
        h.apply_f32_block(B[1:k + 1], X[1:k + 1])
        ctx.synchronize()
        info = h.block_info_f32()
        what = f"{name} k {k}"
        for c in range(k):
            assert torch.equal(X[c + 1, :nd], ref[c]), f"{what}: column {c} differs from apply_f32 in {(X[c + 1, :nd] != ref[c]).sum().item()} entries"
            assert torch.equal(B[c + 1, :nd], b[c]), f"{what}: b changed"
        assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nd:]), f"{what}: wrote outside its columns"
        assert _untouched(B[0]) and _untouched(B[k + 1]) and _untouched(B[1:k + 1, nd:]), f"{what}: wrote into b"
        wide, single = _groups(k)
        if case["block"]:
            assert info == {"width": 4, "block_launches": wide * case["per_group"], "column_launches": single}, (what, info, case["per_group"])
        else:
            assert info == {"width": 1, "block_launches": 0, "column_launches": k}, (what, info)
    print(f"{name}: {case['per_group']} block launches per wide group (one-pass residual restriction: {case['one_pass']})")


def _single(h, b, x0, tol, restart):
    x = x0.clone()
    it, res = C.c_int32(), C.c_double()
    hist = np.zeros(MAX_ITERATIONS + 1)
    status = h._lib.mfmg_hip_hierarchy_solve_fgmres(h.handle, b.data_ptr(), x.data_ptr(), tol, MAX_ITERATIONS, restart, 1,
                                                    C.byref(it), C.byref(res), hist.ctypes.data_as(C.POINTER(C.c_double)), len(hist))
    assert status == L.SUCCESS, h._lib.mfmg_hip_last_error().decode()
    return x, it.value, res.value, hist[: it.value + 1].copy()


def _expected_groups(its, hists, tol, m):
    """(wide groups, single columns) over all preconditioner applications of a block solve, from the one-vector runs"""
    k = len(its)
    slot_col, live = list(range(k)), [its[c] > 0 for c in range(k)]
    wide = single = it = 0
    while any(live):
        for _ in range(m):
            if not any(live):
                break
            s = 0
            while s < k:                                     # the maximal runs of consecutive live slots
                if not live[s]:
                    s += 1
                    continue
                e = s
                while e < k and live[e]:
                    e += 1
                w, o = _groups(e - s)
                wide, single = wide + w, single + o
                s = e
            it += 1
            for s in range(k):
                c = slot_col[s]
                if live[s] and its[c] == it and hists[c][it] <= tol[c]:
                    live[s] = False                          # converged inside the cycle
        packed = [slot_col[s] for s in range(k) if live[s]]
        slot_col[:len(packed)] = packed
        live = [s < len(packed) and its[slot_col[s]] > it for s in range(k)]    # (its == it: retired at the cycle start)
    return wide, single


@pytest.mark.parametrize("restart", [30, 3], ids=["restart30", "restart3"])
def test_block_fgmres_runs_the_float_block_cycle(ctx, restart):
    case = _case(ctx, "linear_v01")
    h, nd = case["h"], case["nd"]
    ld = nd + 6 + (nd & 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    b = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
    x0 = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
    tol = [float(torch.linalg.norm(b[c]).item()) * 10.0 ** (-2 - c) for c in range(K_MAX)]
    ref = [_single(h, b[c], x0[c], tol[c], restart) for c in range(K_MAX)]
    its = [r[1] for r in ref]
    print(f"restart {restart}: iterations of the one-vector driver {its}")
    assert len(set(its)) > 2 and min(its) > 0, its            # the columns retire at different iterations
    for k in (4, 7):
        B, X = _guarded(b[:k], ld, torch.float64), _guarded(x0[:k], ld, torch.float64)
        out_its, hists, work = h.solve_fgmres_block(B[1:k + 1], X[1:k + 1], tol[:k], MAX_ITERATIONS, restart=restart, preconditioner="float")
        ctx.synchronize()
        info = h.block_info_f32()
        what = f"restart {restart} k {k}"
        assert out_its == its[:k], (what, out_its, its[:k])
        for c in range(k):
            assert torch.equal(X[c + 1, :nd], ref[c][0]), f"{what}: x of column {c} differs from solve_fgmres"
            assert hists[c].tobytes() == ref[c][3].tobytes(), (what, c)
            assert np.float64(work["residuals"][c]).tobytes() == np.float64(ref[c][2]).tobytes(), (what, c)
        assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nd:]), f"{what}: wrote outside its columns"
        assert work["preconditioner_columns"] == sum(out_its)
        wide, single = _expected_groups(its[:k], [r[3] for r in ref[:k]], tol[:k], min(restart, MAX_ITERATIONS))
        print(f"{what}: {info}, expected {wide} wide groups and {single} single columns")
        assert info["width"] == 4 and info["block_launches"] > 0, (what, info)
        assert info["block_launches"] == wide * case["per_group"], (what, info, wide)
        assert info["column_launches"] == single < sum(out_its), (what, info, single)


def test_refusals(ctx, mfmg_lib):
    case = _case(ctx, "linear_symmetric")
    h, nd = case["h"], case["nd"]                              # 4913: odd
    assert nd % 2 == 1
    new = lambda rows, ld: torch.full((rows, ld), PAYLOAD, dtype=torch.int32, device="cuda").view(torch.float32)
    ld = nd + 7
    flat_b, flat_x = new(1, 70 * ld).view(-1), new(1, 70 * ld).view(-1)
    flat_b[:] = 1.0
    view = lambda flat, k, l, m=nd: torch.as_strided(flat, (k, m), (l, 1))

    def refused(match, B, X, hh=h, error=L.MfmgInvalidArgument):
        with pytest.raises(error, match=match):
            hh.apply_f32_block(B, X)
        ctx.synchronize()
        assert _untouched(flat_x), match

    refused("even", view(flat_b, 2, nd + 2), view(flat_x, 2, nd + 2))                  # an odd ld
    refused("at least", view(flat_b, 2, nd - 1, nd - 1), view(flat_x, 2, nd - 1, nd - 1))
    refused("1 to 64", view(flat_b, 65, ld)[0:0], view(flat_x, 65, ld)[0:0])
    refused("1 to 64", view(flat_b, 65, ld), view(flat_x, 65, ld))
    refused("overlap", view(flat_x, 3, ld)[0:2], view(flat_x, 3, ld)[1:3])
    with pytest.raises(ValueError, match="float32"):
        h.apply_f32_block(view(flat_b, 2, ld).double(), view(flat_x, 2, ld).double())
    # a hierarchy without the float level
    prob = M.LaplaceProblem((6, 5, 7), "linear", device="cuda")
    h64 = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, _params({}))
    n64 = h64.level_size(0)
    refused("fine level precision", view(flat_b, 2, n64 + (n64 & 1), n64), view(flat_x, 2, n64 + (n64 & 1), n64), hh=h64)
    with pytest.raises(L.MfmgInvalidArgument, match="fine level precision"):
        h64.block_info_f32()
    # a context with a communicator: the call is refused before anything runs (set after the build, taken back before the teardown)
    own = M.Context()
    hc = M.Hierarchy(own, "HipMatrixFreeMeshEvaluator", prob, _params(FLOAT))
    own.synchronize()
    L.check(mfmg_lib.mfmg_hip_context_set_communicator(own.handle, 0, 2, 0, 2))
    try:
        with pytest.raises(L.MfmgInvalidArgument, match="communicator"):
            hc.apply_f32_block(view(flat_b, 2, n64 + (n64 & 1), n64), view(flat_x, 2, n64 + (n64 & 1), n64))
    finally:
        L.check(mfmg_lib.mfmg_hip_context_set_communicator(own.handle, 0, 1, 0, 0))
    own.synchronize()
    assert _untouched(flat_x)
    # and a good call right after the refused ones
    B, X = view(flat_b, 2, ld), view(flat_x, 2, ld)
    h.apply_f32_block(B, X)
    ctx.synchronize()
    one = torch.empty(nd, dtype=torch.float32, device="cuda")
    h.apply_f32(B[0].contiguous(), one)
    ctx.synchronize()
    assert torch.equal(X[0], one) and torch.equal(X[1], one)
