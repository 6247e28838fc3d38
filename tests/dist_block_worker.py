"""Worker of tests/test_gpu_block_distributed.py: run with torch.distributed.run, backend gloo, all ranks on cuda:0.

Blocks of right-hand sides on the ranks of a slab or box grid against the ONE-VECTOR calls on the same ranks: the block entry points
promise a column, on the entries a rank owns, the bits the one-vector call gives that vector there (ghost entries of results are no
more specified than those of the one-vector calls).  Every input -- b, x, the x of the operator -- carries 1e30 on its ghost
entries: they must come from the library's exchanges.

Per k in 1, 2, 4, 5, 7 (a loop, one group of 2, one of 4, 4 + 1, 4 + 2 + 1):
  operator_apply_block, smoother_apply_block, apply_block with "is preconditioner" false and true: the owned entries of every
  column bit-equal to operator_apply / smoother_apply / apply of that column
Counts (tr.n_exchanges, the all-reduces of the transport):
  - block_info() shows the AGREED width -- 4 on the linear meshes, with block launches > 0 after a call with k >= 2; 1 on "mixed",
    where rank 0 keeps one coefficient per cell -- and the same on every rank; the exchanges of every call are the same on all ranks
  - agreed width 4: operator_apply_block at k = 4 makes the exchanges of ONE operator_apply, smoother_apply_block at k = 4 those of
    one smoother_apply, at k = 5 of two, at k = 7 of three; a cycle on 4 columns makes fewer exchanges than 4 cycles (printed)
  - the operator and the cycle make no all-reduce; solve_cg_block makes 1 + 3 x (iterations of the slowest column)
solve_cg_block with k = 4 and 5 and tolerances between 1e-4 and 1e-8 ||b_c||, so that the columns retire at different iterations:
  - two ranks (the all-reduce is one addition per element, whatever the length of the message): iteration count, history and owned
    solution of every column bit-equal to solve_cg of that column on the same ranks
  - four ranks (2 x 1 x 2; gloo may add the ranks' values of a 4-long and of a 1-long message in different orders): the counts equal,
    history and solution within HISTORY_BOUND / SOLUTION_BOUND of the one-vector solves
  - ||b_c - A x_c|| of every gathered column, by the single-process operator on the global mesh, <= 1.01 x its tolerance
  - solve_fgmres_block is still refused on ranks

Bounds of the four-rank case: 100 x the largest deviation MEASURED there (below, with the case), never looser than 1e-6 -- as
tests/dist_krylov_worker.py sets its bounds."""
import argparse
import os

import numpy as np
import torch
import torch.distributed as dist

import dist_worker as W  # (puts the repository and the oracle on sys.path)
import mfmg_amd as M
import mixed_material
from mfmg_amd import lib as L
from mfmg_amd.api import block_groups

# name: (cells per rank along z, (cx, cy) cells per rank along x and y, material, amg parameters) -- after dist_worker.MESHES
MESHES = {
    "small": W.MESHES["small"],                                        # 1 x 1 x 2: linear, V(1,1), A_c gathered right away
    "cube_linear": (24, (24, 24), "linear", dict(W.MESHES["deep"][3])),  # 24^3 cells per rank, the symmetric amg parameters of "deep"
    "mixed": W.MESHES["mixed"],                                        # rank 0 cell-wise constant: no block kernel there
}
KS = (1, 2, 4, 5, 7)
# relative: max_k |hist_k - ref_k| / ref_k and max|x - x_ref| / max|x_ref| over the columns, 2 x 1 x 2 "cube_linear", k = 4 and 5
MEASURED_HISTORY, MEASURED_SOLUTION = 2.7e-15, 3.6e-16   # (k = 5, column 3; k = 5, column 4.  Two of the columns agree bit for bit)
HISTORY_BOUND = min(100 * MEASURED_HISTORY, 1e-6)
SOLUTION_BOUND = min(100 * MEASURED_SOLUTION, 1e-6)


class CountingTransport(M.HaloTransport):
    """the host transport with its all-reduces counted"""
    n_allreduces = 0

    def _allreduce(self, user, values, n, op):
        self.n_allreduces += 1
        return super()._allreduce(user, values, n, op)


def main(args):
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    grid = W.parse_grid(args.grid, world)
    per, (cx, cy), material, amg = MESHES[args.mesh]
    cells = (cx * grid[0], cy * grid[1], per * grid[2])
    part = M.BoxPartition(cells, rank, grid, length=tuple(c / float(cells[0]) for c in cells), low_ghost_cells=args.low_ghost)
    mixed = material in mixed_material.PATTERNS
    table = mixed_material.global_table(cells, material, part.h) if mixed else None
    local_problem = lambda: mixed_material.local_problem(part, table, "cuda") if mixed else part.local_problem(material, "cuda")
    params = dict(W.PRM)
    params.update({"smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0},
                   "solver": {"type": "amg", "amg": dict(amg)}, "is preconditioner": False})
    ctx = M.Context()
    tr = CountingTransport(ctx, part, 2)
    assert tr.name() == "host"
    gctx = M.Context()
    gprob = mixed_material.global_problem(cells, table, part.h, "cuda") if mixed else M.LaplaceProblem(cells, material, device="cuda", cell_size=part.h)
    a_global = M.MatrixFreeLaplace(gctx, gprob)
    ng, nl = gprob.n_dofs, part.n_local_dofs
    own_l, own_g, loc_g = part.owned_local_index().numpy(), part.owned_global_index().numpy(), part.local_global_index().numpy()
    ghost_l = np.ones(nl, bool)
    ghost_l[own_l] = False
    assert ghost_l.any()
    own_t = torch.from_numpy(own_l).cuda()
    ld = nl + 2 + (nl & 1)
    k_max = max(KS)
    rng = np.random.default_rng(0)
    bg, xg = rng.random((k_max, ng)), rng.random((k_max, ng))

    def local_block(vg, k):
        """the local parts of the first k global vectors as a block of leading dimension ld, ghost entries 1e30"""
        out = np.zeros((k, ld))
        out[:, :nl] = vg[:k][:, loc_g]
        out[:, :nl][:, ghost_l] = 1e30
        return torch.from_numpy(out).cuda()

    def owned_bits(v):
        return v[..., :nl][..., own_t].contiguous().cpu().numpy().view(np.int64)

    def same_on_all_ranks(values):
        t = torch.zeros(world, len(values), dtype=torch.float64)
        t[rank] = torch.tensor([float(v) for v in values], dtype=torch.float64)
        W._all_reduce_cpu(t)
        return bool((t == t[rank]).all())

    def counted(f):
        a, e = tr.n_allreduces, tr.n_exchanges()
        out = f()
        ctx.synchronize()
        return out, tr.n_allreduces - a, tr.n_exchanges() - e

    def say(text):
        if rank == 0:
            print(text, flush=True)

    def block_calls(h, is_preconditioner, expected_width):
        """operator, smoother (first hierarchy only) and cycle on blocks against the one-vector calls; returns the counts"""
        counts = {}
        # the one-vector calls on the same ranks, once for the k_max columns
        B1, X1 = local_block(bg, k_max), local_block(xg, k_max)
        ref = {}
        Y = torch.zeros(k_max, ld, dtype=torch.float64, device="cuda")
        one = {}
        for c in range(k_max):
            _, ar, ex = counted(lambda: h.operator_apply(0, X1[c, :nl].clone(), Y[c, :nl]))
            one["operator"] = ex
            assert ar == 0
        ref["operator"] = owned_bits(Y)
        if not is_preconditioner:
            Xs = X1.clone()
            for c in range(k_max):
                _, ar, ex = counted(lambda: h.smoother_apply(0, B1[c, :nl].clone(), Xs[c, :nl]))
                one["smoother"] = ex
                assert ar == 0
            ref["smoother"] = owned_bits(Xs)
        Xc = X1.clone()
        for c in range(k_max):
            _, ar, ex = counted(lambda: h.apply(B1[c, :nl].clone(), Xc[c, :nl]))
            one["cycle"] = ex
            assert ar == 0, "the cycle made an all-reduce of its own"
        ref["cycle"] = owned_bits(Xc)
        assert same_on_all_ranks(list(one.values()))
        for k in KS:
            groups = block_groups(k)
            calls = {"operator": lambda B, X, Yk: h.operator_apply_block(0, X, Yk), "cycle": lambda B, X, Yk: h.apply_block(B, X)}
            if not is_preconditioner:
                calls["smoother"] = lambda B, X, Yk: h.smoother_apply_block(0, B, X)
            for what, call in calls.items():
                B, X = local_block(bg, k), local_block(xg, k)
                Yk = torch.zeros(k, ld, dtype=torch.float64, device="cuda")
                _, ar, ex = counted(lambda: call(B, X, Yk))
                got = owned_bits(Yk if what == "operator" else X)
                assert ar == 0, f"{what} on a block made an all-reduce of its own"
                assert np.array_equal(got, ref[what][:k]), (f"{what} k {k} preconditioner {is_preconditioner}: columns "
                                                            f"{sorted(set(np.nonzero(got != ref[what][:k])[0].tolist()))} differ from the one-vector call")
                info = h.block_info()
                assert info["width"] == expected_width, info
                assert same_on_all_ranks([info["width"], ex]), f"{what} k {k}: the ranks made different exchanges"
                if expected_width == 4 and k >= 2:
                    assert info["block_launches"] > 0, (what, k, info)
                if expected_width == 4 and what in ("operator", "smoother"):
                    # a group of 4 or 2 columns exchanges like ONE vector, a single column is one vector
                    assert ex == len(groups) * one[what], (what, k, ex, one[what])
                if expected_width == 1:
                    assert ex == k * one[what], (what, k, ex, one[what])
                counts[(what, k)] = ex
        if expected_width == 4:
            assert counts[("cycle", 4)] < 4 * one["cycle"], (counts[("cycle", 4)], one["cycle"])
        say(f"is preconditioner {is_preconditioner}: width {expected_width}; exchanges of one operator / smoother / cycle "
            f"{one['operator']} / {one.get('smoother', '-')} / {one['cycle']}; of a cycle on 4 columns {counts[('cycle', 4)]} "
            f"(4 cycles: {4 * one['cycle']}), on 7 columns {counts[('cycle', 7)]}")
        return counts

    expected_width = 1 if mixed else 4
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", local_problem(), params)
    assert h.block_info()["width"] == expected_width, h.block_info()
    block_calls(h, False, expected_width)
    del h
    pp = dict(params)
    pp["is preconditioner"] = True
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", local_problem(), pp)
    block_calls(h, True, expected_width)

    # ---- CG on a block of right-hand sides
    def gather(v_local):
        out = torch.zeros(ng, dtype=torch.float64)
        out[torch.from_numpy(own_g)] = torch.from_numpy(np.ascontiguousarray(v_local.cpu().numpy()[own_l]))
        return W._all_reduce_cpu(out).numpy()

    def true_residual(c, x_global):
        r = torch.empty(ng, dtype=torch.float64, device="cuda")
        a_global.vmult(r, torch.from_numpy(np.ascontiguousarray(x_global)).cuda())
        gctx.synchronize()
        return np.linalg.norm(bg[c] - r.cpu().numpy())

    worst_hist = worst_x = 0.0
    relative = (1e-4, 1e-8, 1e-6, 1e-5, 1e-7)
    for k in (4, 5):
        tol = [relative[c] * np.linalg.norm(bg[c]) for c in range(k)]
        # the one-vector solves on the same ranks
        B1, X1 = local_block(bg, k), local_block(xg, k)
        its1, hist1 = [], []
        for c in range(k):
            it, hist = h.solve_cg(B1[c, :nl].clone(), X1[c, :nl], tol[c], 200)
            its1.append(it)
            hist1.append(hist)
        B, X = local_block(bg, k), local_block(xg, k)
        (its, hists, work), n_allreduces, n_exchanges = counted(lambda: h.solve_cg_block(B, X, tol, 200))
        assert same_on_all_ranks(list(its) + [v for hh in hists for v in hh]), "the ranks disagree on the iteration"
        assert list(its) == its1, (its, its1)
        assert len(set(its)) > 1 and min(its) >= 2, its                      # the columns retire at different iterations
        assert n_allreduces == 1 + 3 * max(its), (n_allreduces, its)
        assert work["preconditioner_columns"] == sum(its) and work["operator_columns"] == sum(its), (work, its)
        if expected_width == 4:
            assert work["block_launches"] > 0, work
        for c in range(k):
            d_hist = float((np.abs(hists[c] - hist1[c]) / hist1[c]).max())
            xo, xo1 = X[c, :nl][own_t], X1[c, :nl][own_t]
            d_x = float(((xo - xo1).abs().max() / xo1.abs().max()).item())
            worst_hist, worst_x = max(worst_hist, d_hist), max(worst_x, d_x)
            say(f"solve_cg_block k {k} column {c}: {its[c]} iterations, deviation from solve_cg history {d_hist:.3e} solution {d_x:.3e}")
            if world == 2:
                assert np.array_equal(np.asarray(hists[c]).view(np.int64), np.asarray(hist1[c]).view(np.int64)), (k, c, d_hist)
                assert torch.equal(xo, xo1), (k, c, d_x)
            else:
                assert d_hist <= HISTORY_BOUND, (k, c, d_hist)
                assert d_x <= SOLUTION_BOUND, (k, c, d_x)
            res = true_residual(c, gather(X[c, :nl]))
            assert res <= 1.01 * tol[c], (k, c, res, tol[c])
        say(f"solve_cg_block k {k}: iterations {list(its)}, all-reduces {n_allreduces}, exchanges {n_exchanges}, work {work}")
        Bf, Xf = local_block(bg, k), local_block(xg, k)
        try:
            h.solve_fgmres_block(Bf, Xf, tol, 200)
            raise AssertionError("solve_fgmres_block on ranks must be refused")
        except L.MfmgInvalidArgument as e:
            assert "communicator" in str(e)
    say(f"distributed block checks passed; grid {'x'.join(map(str, grid))} mesh {args.mesh} width {expected_width}; block CG against the "
        f"one-vector solves: worst deviation history {worst_hist:.3e} solution {worst_x:.3e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="small")
    ap.add_argument("--grid", default="")
    ap.add_argument("--low-ghost", type=int, default=2)
    a = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    try:
        main(a)
    finally:
        dist.destroy_process_group()
