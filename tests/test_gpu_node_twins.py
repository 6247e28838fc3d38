"""Twin nodes (SparseMatrixDevice::enable_node_twins, bdia_twin_node_kernel) against the one-node-per-lane kernel.

The matrices are the smoothed-prolongator-like ones of tests/test_node_twins_criterion.py (its SHAPES: all twins, odd nx,
one unknown per node, twin classes below a wavefront, 1 / 17 / 65 perturbed nodes that become listed rows and leave their
partners single).  The reference is the same matrix built under MFMG_NODE_TWINS=0 -- bdia_class_node_kernel, which
tests/test_spmv_layouts.py ties to long double --, and the twin launch must equal it with torch.equal in all five modes a
rectangular matrix accepts (out pre-filled with NaN where the mode does not read it), with b, D^-1 and out 32-byte aligned
(the twin epilogue), offset by 16 bytes (two store_node halves) and by 8 bytes (row by row), and after release_csr();
form()["twin_wide"] and ["pairs"] say after every launch which of the three epilogues it took.  x stays aligned: the C
ABI rejects a source vector off the 16-byte grid.  A square matrix with the same couplings takes twins too and runs all
seven modes.  The form is asserted before any number: twin_kernel == 1 and twin_slots within the range the criterion
test derives.

One hierarchy test: the smallest mesh whose first aggregation level takes a smoothed prolongator in node classes on one
rank (128 x 128 x 64 cells: 262 144 rows, the threshold of `pays` in the setup), three cycles bit-equal to the hierarchy
built under MFMG_NODE_TWINS=0."""
import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
from test_node_twins_criterion import SHAPES, SHAPE_IDS, pt_like, twin_counts

pytestmark = pytest.mark.gpu

RECT_MODES = (L.CSR_APPLY, L.CSR_RESIDUAL, L.CSR_SUBTRACT, L.CSR_ADD, L.CSR_PLUS_SCALED)
READS_OUT = (L.CSR_SUBTRACT, L.CSR_ADD)
BETA = {L.CSR_PLUS_SCALED: -0.7, L.CSR_FIRST: 0.6, L.CSR_NEXT: 0.45}
ALPHA = {L.CSR_NEXT: -0.35}
ALL_MODES = (L.CSR_APPLY, L.CSR_RESIDUAL, L.CSR_FIRST, L.CSR_NEXT, L.CSR_SUBTRACT, L.CSR_ADD, L.CSR_PLUS_SCALED)


def scaled_normal(rng, n):
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)


def build_pair(ctx, monkeypatch, A):
    """(the matrix with twins asked for, whether it took them, the same matrix built under MFMG_NODE_TWINS=0)"""
    monkeypatch.setenv("MFMG_NODE_TWINS", "0")
    ref = M.SparseMatrixDevice(ctx, A)
    assert ref.enable_node_twins() is False
    monkeypatch.delenv("MFMG_NODE_TWINS")
    tw = M.SparseMatrixDevice(ctx, A)
    return tw, tw.enable_node_twins(), ref


def vectors(A, seed):
    rng = np.random.default_rng(seed)
    m, n = A.shape
    return {"x": scaled_normal(rng, n), "b": scaled_normal(rng, m), "dinv": scaled_normal(rng, m), "out": scaled_normal(rng, m),
            "xp": scaled_normal(rng, m)}


def launch(Ad, ctx, mode, v, offset=0):
    """One launch with b, D^-1 and out `offset` doubles behind a 32-byte aligned address (x stays aligned: it is gathered)."""
    m = Ad.shape[0]

    def put(a):
        buf = torch.empty(m + 4, dtype=torch.float64, device="cuda")
        assert buf.data_ptr() % 32 == 0
        t = buf[offset:offset + m]
        t.copy_(torch.from_numpy(a))
        assert t.data_ptr() % 32 == 8 * offset
        return t
    out = put(v["out"] if mode in READS_OUT else np.full(m, np.nan))
    needs_b = mode in (L.CSR_RESIDUAL, L.CSR_FIRST, L.CSR_NEXT, L.CSR_PLUS_SCALED)
    needs_d = mode in (L.CSR_FIRST, L.CSR_NEXT, L.CSR_PLUS_SCALED)
    x = torch.from_numpy(v["x"]).cuda()
    assert x.data_ptr() % 32 == 0
    Ad.launch(mode, x, out, b=put(v["b"]) if needs_b else None, dinv=put(v["dinv"]) if needs_d else None,
              x_prev=put(v["xp"]) if mode == L.CSR_NEXT else None, alpha=ALPHA.get(mode, 0.0), beta=BETA.get(mode, 0.0))
    ctx.synchronize()
    return out


def assert_same_launches(ctx, tw, ref, A, where, seed=3, modes=RECT_MODES):
    v = vectors(A, seed)
    for mode in modes:
        want = launch(ref, ctx, mode, v)
        assert bool(torch.isfinite(want).all()), f"{where}: mode {mode}: the reference left entries unwritten"
        for offset in (0, 2, 1):
            got = launch(tw, ctx, mode, v, offset)
            f = tw.form()
            if f["twin_kernel"] == 1:
                # which epilogue the launch took: 32 bytes per operand and lane, the two 16-byte halves, row by row
                assert (f["twin_wide"], f["pairs"]) == {0: (1, 1), 2: (0, 1), 1: (0, 0)}[offset], f"{where}: mode {mode}, offset {offset}: {f}"
            assert torch.equal(got, want), (f"{where}: mode {mode}, operands {8 * offset} bytes off: "
                                            f"{int((got != want).sum())} of {len(want)} rows differ from the one-node kernel")


@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_twin_launch_equals_single_node_launch(ctx, monkeypatch, sid):
    _, dims, c, exact, perturb = SHAPES[SHAPE_IDS.index(sid)]
    A = pt_like(dims, c, exact, perturb)
    t = twin_counts(dims, exact, perturb)
    tw, taken, ref = build_pair(ctx, monkeypatch, A)
    f, f0 = tw.form(), ref.form()
    print(f"{sid}: {A.shape[0]} x {A.shape[1]}, {A.nnz} entries, expected {t}, form {f}")
    assert f0["kind"] == 5 and f0["class_kernel"] == 1 and f0["c"] == c and f0["twin_kernel"] == 0
    assert f0["listed"] == c * t["listed_nodes"]
    assert taken == t["taken"]
    if not taken:
        # declined (the odd-nx shape: twins in every second row only, below 90 %): the matrix is what it was
        assert t["twins"] > 0 and t["singles"] > 0
        assert f == f0
    else:
        assert f["twin_kernel"] == 1 and f["kind"] == 5 and f["class_kernel"] == 1
        assert t["twin_slots"][0] <= f["twin_slots"] <= t["twin_slots"][1] and f["twin_slots"] % 64 == 0
        assert f["twin_classes"] == t["twin_classes"]
        assert f["listed"] == f0["listed"] and f["listed_route"] == f0["listed_route"]
        assert f["single_slots"] == f["class_slots"] and f["single_slots"] % 64 == 0
        assert (f["single_slots"] > 0) == (t["singles"] > 0) and f["single_slots"] >= t["singles"]
    assert_same_launches(ctx, tw, ref, A, sid)
    if taken:
        assert tw.form()["pairs"] == 0                    # (the last launch sat 8 bytes off)
        assert tw.release_csr() is True
        f1 = tw.form()
        assert f1["csr_released"] == 1 and all(f1[k] == f[k] for k in ("twin_kernel", "twin_slots", "twin_classes", "single_slots", "listed"))
        assert_same_launches(ctx, tw, ref, A, sid + " after release_csr", seed=4)


@pytest.mark.parametrize("dims,c", [((32, 24, 22), 2), ((40, 32, 26), 1)])
def test_square_matrix_with_twins_runs_the_smoother_modes(ctx, monkeypatch, dims, c):
    """The same couplings in a square matrix (zero columns behind the coarse ones): its offsets are too many for block
    diagonals, so it runs as node classes, takes twins through the public entry point, and accepts the modes first and
    next, whose epilogue reads x at the rows of the twin."""
    import scipy.sparse as sp
    P = pt_like(dims, c)
    A = sp.hstack([P, sp.csr_matrix((P.shape[0], P.shape[0] - P.shape[1]))]).tocsr()
    A.sort_indices()
    tw, taken, ref = build_pair(ctx, monkeypatch, A)
    f, f0 = tw.form(), ref.form()
    print(f"square {dims} x {c}: form {f}")
    assert f0["kind"] == 5 and f0["class_kernel"] == 1 and f0["c"] == c
    assert taken and f["twin_kernel"] == 1 and f["twin_wide"] == -1
    t = twin_counts(dims)
    assert t["twin_slots"][0] <= f["twin_slots"] <= t["twin_slots"][1]
    assert_same_launches(ctx, tw, ref, A, f"square {dims} x {c}", modes=ALL_MODES)


def test_three_unknowns_per_node_decline(ctx):
    A = pt_like((32, 24, 22), 3)
    Ad = M.SparseMatrixDevice(ctx, A)
    f0 = Ad.form()
    assert f0["kind"] == 5 and f0["c"] == 3 and f0["class_kernel"] == 1
    assert Ad.enable_node_twins() is False
    f = Ad.form()
    assert f["twin_kernel"] == 0 and f == f0


def test_hierarchy_cycle_with_twins_equals_cycle_without(ctx, monkeypatch):
    prob = M.LaplaceProblem((128, 128, 64), "constant", device="cuda")
    params = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2},
              "is preconditioner": False, "max levels": 2,
              "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0},
              "solver": {"type": "amg", "amg": {"smoother_degree": 1, "smoothing_range": 4.0, "n_cycles": 1, "pre_smoothing_levels": 0,
                                                "aggregate_block": 2, "smoothed_prolongation": True}}}
    monkeypatch.setenv("MFMG_NODE_TWINS", "0")
    h0 = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, params)
    monkeypatch.delenv("MFMG_NODE_TWINS")
    h1 = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, params)
    f0, f1 = h0.coarse_amg_smoothed_prolongator_forms()[0], h1.coarse_amg_smoothed_prolongator_forms()[0]
    print("level 0, MFMG_NODE_TWINS=0:", f0, "\nlevel 0:", f1)
    assert f0 is not None and f0["kind"] == 5 and f0["class_kernel"] == 1 and f0["twin_kernel"] == 0
    assert f1["twin_kernel"] == 1 and f1["c"] == 2 and 2 * f1["twin_slots"] >= 64 * 64 * 32 * 9 // 10
    rng = np.random.default_rng(11)
    free = torch.from_numpy((prob.constrained.cpu().numpy() != 1).astype(np.float64)).cuda()
    b = torch.from_numpy(rng.random(prob.n_dofs)).cuda() * free
    xs = []
    for h in (h0, h1):
        x = torch.from_numpy(np.random.default_rng(12).random(prob.n_dofs)).cuda() * free
        for _ in range(3):
            h.apply(b, x)
        ctx.synchronize()
        xs.append(x)
    assert bool(torch.isfinite(xs[0]).all())
    assert torch.equal(xs[0], xs[1])
