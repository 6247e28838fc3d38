"""Restriction and prolongation on blocks of vectors: Hierarchy.restrictor_apply_block against restrictor_apply column by column,
bit for bit, and the cycle (apply_block, solve_cg_block) through the block transfers.

The shapes come from the case table of test_transfer_shapes.py, each the smallest that reaches its path; the first assertion of
every case checks restrictor_form(), so that no case passes beside its path.  For k = 1, 2, 3, 4, 7 in that order on ONE
hierarchy and the modes NO_TRANS, TRANS, TRANS_SUBTRACT: blocks with ld = size + 6 (+ 1 where that is odd), a guard column on
either side and the tails beyond the vector size carrying a NaN payload.  Every column must equal restrictor_apply on that column
(which test_transfer_shapes.py pins against long double), guards, tails and the input block must be untouched, and
transfer_block_info() must report the widths of the form and the launches of the groups of block_groups(k) wider than one --
cross-checked with the profiler's count of sr_restrict_block_kernel / sr_prolong_block_kernel."""
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
from mfmg_amd.api import block_groups

from test_transfer_shapes import BY_ID, build, check_form

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 4, 7]
K_MAX = max(KS)
PAYLOAD = 0x7FF8DEAD0000BEEF          # a quiet NaN nobody computes
MODES = [("NO_TRANS", L.NO_TRANS), ("TRANS", L.TRANS), ("TRANS_SUBTRACT", L.TRANS_SUBTRACT)]

# case of test_transfer_shapes.py -> (restrict width, prolong width); the path it is here for
TRANSFER_CASES = {
    "linear222_ne2": (4, 4),          # pair<2> / nodes, planes in double
    "linear222_ne2_f32": (4, 4),      # planes in float
    "linear222_ne3": (4, 4),          # rows kernel and the n_eig loop of the node kernel
    "const322_12x8x8": (4, 4),        # pair<0>
    "const322_36x2x2": (4, 4),        # (beyond the issue's table) pair<0> with the reference table
    "random222_ne2": (4, 4),          # node_dof
    "disc222_12x10x6": (4, 4),        # discontinuous coefficient, no reference table (the three sources mixed: see below)
    "disc222_70x66x4": (4, 4),        # 2310 agglomerates: ten workgroups dealt to a grid of 16, a partial last workgroup
    "const222_130x2x2": (4, 1),       # block222 prolongation: the loop; restriction from the table
    "csr_linear222": (1, 1),          # no agglomerate-wise form
}


def _even(n):
    return n + 6 + (n & 1)


def _guarded(cols, ld):
    blk = torch.full((len(cols) + 2, ld), PAYLOAD, dtype=torch.int64, device="cuda").view(torch.float64)
    for c, v in enumerate(cols):
        blk[c + 1, :v.numel()] = v
    return blk


def _untouched(t):
    return bool((t.contiguous().view(torch.int64) == PAYLOAD).all().item())


def _wide_groups(k):
    return len([w for w in block_groups(k) if w > 1])


@pytest.mark.parametrize("cid", list(TRANSFER_CASES))
def test_block_transfers_equal_the_one_vector_ones(ctx, cid):
    c = BY_ID[cid]
    h, _ = build(ctx, c)
    check_form(h, c)
    if cid == "disc222_70x66x4":
        assert h.level_size(1) == 2 * 2310
    _compare_with_the_one_vector_entry_point(ctx, h, cid, *TRANSFER_CASES[cid])


def test_block_transfers_with_table_and_class_table(ctx, monkeypatch):
    """Beyond the table above: the node kernel where the block222 kernels would run (MFMG_SR_PROLONG=nodes), on the case whose
    agglomerates repeat the reference block (table), repeat a block among themselves (class table) or have a block of their own
    (planes) -- the three sources of both block kernels in one launch."""
    c = BY_ID["const222_130x36x12"]
    monkeypatch.setenv("MFMG_SR_PROLONG", "nodes")
    h, _ = build(ctx, c)
    monkeypatch.delenv("MFMG_SR_PROLONG")
    f = h.restrictor_form(1)
    assert f["structured"] and f["restrict"] == "pair222" and f["prolong"] == "nodes", f
    assert 0 < f["table_agglomerates"] < h.level_size(1) // 2 and f["n_classes"] > 0, f
    _compare_with_the_one_vector_entry_point(ctx, h, c["id"] + " nodes", 4, 4)


def _compare_with_the_one_vector_entry_point(ctx, h, cid, want_r, want_p):
    n_f, n_c = h.level_size(0), h.level_size(1)
    ld_f, ld_c = _even(n_f), _even(n_c)
    assert ld_f % 2 == 0 and ld_c % 2 == 0
    g = torch.Generator(device="cuda")
    g.manual_seed(13)
    fine = [torch.randn(n_f, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
    coarse = [torch.randn(n_c, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
    z = [torch.randn(n_f, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
    single = {}
    for name, mode in MODES:
        single[name] = []
        for col in range(K_MAX):
            if mode == L.NO_TRANS:
                out = torch.full((n_c,), float("nan"), dtype=torch.float64, device="cuda")
                h.restrictor_apply(1, fine[col], out, mode)
            else:
                out = z[col].clone() if mode == L.TRANS_SUBTRACT else torch.full((n_f,), float("nan"), dtype=torch.float64, device="cuda")
                h.restrictor_apply(1, coarse[col], out, mode)
            single[name].append(out)
    ctx.synchronize()
    assert all(bool(torch.isfinite(v).all().item()) for vs in single.values() for v in vs)

    for k in KS:
        wide = _wide_groups(k)
        for name, mode in MODES:
            restriction = mode == L.NO_TRANS
            n_in, n_out = (n_f, n_c) if restriction else (n_c, n_f)
            ld_in, ld_out = (ld_f, ld_c) if restriction else (ld_c, ld_f)
            Vin = _guarded((fine if restriction else coarse)[:k], ld_in)
            if mode == L.TRANS_SUBTRACT:
                Vout = _guarded(z[:k], ld_out)
            else:
                Vout = torch.full((k + 2, ld_out), PAYLOAD, dtype=torch.int64, device="cuda").view(torch.float64)
            ctx.profile_enable(True, "sr_restrict_block_kernel,sr_prolong_block_kernel")
            h.restrictor_apply_block(1, Vin[1:k + 1], Vout[1:k + 1], mode)
            launched = (ctx.profile_query("sr_restrict_block_kernel")[0], ctx.profile_query("sr_prolong_block_kernel")[0])
            ctx.profile_enable(False)
            ctx.synchronize()
            what = f"{cid} k {k} {name}"
            for col in range(k):
                got = Vout[col + 1, :n_out]
                assert torch.equal(got, single[name][col]), \
                    f"{what}: column {col} differs from restrictor_apply in {(got != single[name][col]).sum().item()} entries"
            assert _untouched(Vout[0]) and _untouched(Vout[k + 1]) and _untouched(Vout[1:k + 1, n_out:]), f"{what}: wrote outside its columns"
            assert _untouched(Vin[0]) and _untouched(Vin[k + 1]) and _untouched(Vin[1:k + 1, n_in:]), f"{what}: wrote into the input block"
            src = fine if restriction else coarse
            assert all(torch.equal(Vin[col + 1, :n_in], src[col]) for col in range(k)), f"{what}: the input block changed"
            info = h.transfer_block_info(1)
            assert (info["restrict_width"], info["prolong_width"]) == (want_r, want_p), (what, info)
            width = want_r if restriction else want_p
            want_launches = wide if width == 4 else 0
            assert info["restrict_launches"] == (want_launches if restriction else 0), (what, info)
            assert info["prolong_launches"] == (0 if restriction else want_launches), (what, info)
            assert launched == (info["restrict_launches"], info["prolong_launches"]), (what, info, launched)
            assert info["column_launches"] == (k % 2 if width == 4 else k), (what, info)


def test_block_transfers_refuse_what_they_cannot_take(ctx, mfmg_lib):
    c = BY_ID["linear222_ne2"]
    h, prob = build(ctx, c)
    check_form(h, c)
    n_f, n_c = h.level_size(0), h.level_size(1)
    ld_f, ld_c = _even(n_f), _even(n_c)
    flat_f = torch.full((66 * ld_f + 2,), PAYLOAD, dtype=torch.int64, device="cuda").view(torch.float64)
    flat_c = torch.ones(66 * ld_c + 2, dtype=torch.float64, device="cuda")
    view = lambda flat, k, ld, m, off=0: torch.as_strided(flat, (k, m), (ld, 1), off)

    def refused(match, Vin, Vout, level=1, mode=L.TRANS, hh=h):
        with pytest.raises(L.MfmgInvalidArgument, match=match):
            hh.restrictor_apply_block(level, Vin, Vout, mode)
        ctx.synchronize()
        assert _untouched(flat_f), match

    good_in, good_out = view(flat_c, 2, ld_c, n_c), view(flat_f, 2, ld_f, n_f)
    refused("even", view(flat_c, 2, ld_c + 1, n_c), good_out)                         # an odd ld of the input
    refused("even", good_in, view(flat_f, 2, ld_f + 1, n_f))                          # ... of the output
    refused("at least", view(flat_c, 2, n_c - 2, n_c - 2), good_out)                  # ld below the size
    refused("at least", good_in, view(flat_f, 2, n_f - 1 - (n_f & 1), n_f - 1 - (n_f & 1)))
    with pytest.raises(L.MfmgInvalidArgument, match="1 to 64"):      # (an empty tensor has no pointer: the library itself)
        L.check(mfmg_lib.mfmg_hip_hierarchy_restrictor_apply_block(h.handle, 1, 0, ld_c, good_in.data_ptr(), ld_f, good_out.data_ptr(), L.TRANS))
    refused("1 to 64", view(flat_c, 65, ld_c, n_c), view(flat_f, 65, ld_f, n_f))
    refused("aligned", view(flat_c, 2, ld_c, n_c, 1), good_out)                       # a base at an odd element
    refused("aligned", good_in, view(flat_f, 2, ld_f, n_f, 1))
    # overlapping blocks (one buffer for both sides; the sizes differ, the extents decide)
    refused("overlap", view(flat_f, 2, ld_f, n_c), view(flat_f, 3, ld_f, n_f)[1:3])
    refused("levels >= 1", good_in, good_out, level=0)
    refused("unknown operator mode", good_in, good_out, mode=7)
    with pytest.raises(L.MfmgInvalidArgument, match="levels >= 1"):
        h.transfer_block_info(0)
    # a context with a communicator: refused before anything runs (set after the build, taken back before the teardown)
    own = M.Context()
    hc, _ = build(own, c)
    own.synchronize()
    L.check(mfmg_lib.mfmg_hip_context_set_communicator(own.handle, 0, 2, 0, 2))
    try:
        refused("communicator", good_in, good_out, hh=hc)
    finally:
        L.check(mfmg_lib.mfmg_hip_context_set_communicator(own.handle, 0, 1, 0, 0))
    own.synchronize()
    # and a good call right after the refused ones
    h.restrictor_apply_block(1, good_in, good_out, L.TRANS)
    ctx.synchronize()
    one = torch.empty(n_f, dtype=torch.float64, device="cuda")
    h.restrictor_apply(1, good_in[0].contiguous(), one, L.TRANS)
    ctx.synchronize()
    assert torch.equal(good_out[0], one) and torch.equal(good_out[1], one)
    assert h.transfer_block_info(1)["prolong_launches"] == 1


# ---- the cycle takes the block transfers ---------------------------------------------------------------------------------
DEGREE = 3
CYCLE_CASES = [((16, 16, 16), None, None), ((20, 12, 10), None, None), ((16, 16, 16), "dealii", "lexicographic")]


def _cycle_params(is_preconditioner, mode):
    p = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": is_preconditioner,
         "max levels": 2, "smoother": {"type": "Chebyshev", "degree": DEGREE, "smoothing_range": 20.0}}
    if mode is not None:
        p["internal numbering"] = mode
    return p


def _cycle_hierarchy(ctx, n, numbering, mode, is_preconditioner):
    kw = {"dof_numbering": M.dealii_numbering(n)} if numbering == "dealii" else {}
    prob = M.LaplaceProblem(n, "linear", device="cuda", **kw)
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, _cycle_params(is_preconditioner, mode))
    f = h.restrictor_form(1)
    assert f["structured"] and f["restrict"] == "pair222" and f["prolong"] == "nodes", f
    assert h.block_info()["width"] == 4
    info = h.transfer_block_info(1)
    assert (info["restrict_width"], info["prolong_width"]) == (4, 4), info
    return h


@pytest.mark.parametrize("is_preconditioner", [True, False], ids=["preconditioner", "solver"])
@pytest.mark.parametrize("n,numbering,mode", CYCLE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_cycle_takes_the_block_transfers(ctx, n, numbering, mode, is_preconditioner):
    h = _cycle_hierarchy(ctx, n, numbering, mode, is_preconditioner)
    nd = h.level_size(0)
    ld = _even(nd)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    b = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
    x0 = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(K_MAX)]
    single = []
    for col in range(K_MAX):
        x = x0[col].clone()
        h.apply(b[col], x)
        single.append(x)
    ctx.synchronize()
    # k = 4: one group; k = 7: the groups 4, 2, 1
    for k, want in ((4, (1, 1, 0)), (7, (2, 2, 1))):
        B, X = _guarded(b[:k], ld), _guarded(x0[:k], ld)
        ctx.profile_enable(True, "sr_restrict_block_kernel,sr_prolong_block_kernel")
        h.apply_block(B[1:k + 1], X[1:k + 1])
        launched = (ctx.profile_query("sr_restrict_block_kernel")[0], ctx.profile_query("sr_prolong_block_kernel")[0])
        ctx.profile_enable(False)
        ctx.synchronize()
        what = f"{n} {numbering} {mode} preconditioner {is_preconditioner} k {k}"
        info = h.transfer_block_info(1)
        assert (info["restrict_launches"], info["prolong_launches"], info["column_launches"]) == want, (what, info)
        assert launched == want[:2], (what, launched)
        for col in range(k):
            got = X[col + 1, :nd]
            assert torch.equal(got, single[col]), f"{what}: column {col} differs from apply in {(got != single[col]).sum().item()} entries"
        assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nd:]), f"{what}: wrote outside its columns"
        assert all(torch.equal(B[col + 1, :nd], b[col]) for col in range(k)), f"{what}: b changed"


@pytest.mark.parametrize("n,numbering,mode", CYCLE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_block_cg_through_the_block_transfers(ctx, n, numbering, mode):
    h = _cycle_hierarchy(ctx, n, numbering, mode, True)
    nd = h.level_size(0)
    ld = _even(nd)
    k = 4
    tol = [1e-4, 1e-10, 1e-7, 1e-2]
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    b = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(k)]
    x0 = [torch.randn(nd, dtype=torch.float64, device="cuda", generator=g) for _ in range(k)]
    ref = []
    for col in range(k):
        x = x0[col].clone()
        it, hist = h.solve_cg(b[col], x, tol[col], 200)
        ref.append((x, it, hist.copy()))
    ctx.synchronize()
    B, X = _guarded(b, ld), _guarded(x0, ld)
    its, hists, _ = h.solve_cg_block(B[1:k + 1], X[1:k + 1], tol, 200)
    ctx.synchronize()
    assert len({r[1] for r in ref}) > 1, "the tolerances do not separate the columns"
    info = h.transfer_block_info(1)
    assert info["restrict_launches"] >= 1 and info["prolong_launches"] >= 1, info
    for col in range(k):
        assert its[col] == ref[col][1], (col, its, [r[1] for r in ref])
        assert hists[col].tobytes() == ref[col][2].tobytes(), f"history of column {col} differs"
        assert torch.equal(X[col + 1, :nd], ref[col][0]), f"x of column {col} differs from solve_cg"
    assert _untouched(X[0]) and _untouched(X[k + 1]) and _untouched(X[1:k + 1, nd:])
