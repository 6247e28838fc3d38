"""Worker of tests/test_gpu_block_fgmres_distributed.py: run with torch.distributed.run, backend gloo, all ranks on cuda:0.

solve_fgmres_block and apply_f32_block on the ranks of a slab or box grid against the ONE-VECTOR calls on the same ranks: a column
gets, on the entries a rank owns, the bits the one-vector call gives that vector there.  Every input carries 1e30 (float blocks: NaN)
on its ghost entries: they must come from the library's exchanges.  Hierarchies with "fine level precision" float and "is
preconditioner" true, one with the non-symmetric V(0,1) coarse cycle (solver.amg.pre_smoothing_levels 0) and one with V(1,1).

Per hierarchy:
  apply_f32_block on 4 and 5 columns: the owned entries of every column bit-equal to apply_f32 of that column;
  block_info_f32()["width"] is the AGREED width -- 4 on the linear meshes, 1 on "mixed" (rank 0 keeps one coefficient per cell: no
  block kernel there) -- and the same on every rank; at width 4 the cycle on 4 columns makes fewer exchanges than four apply_f32,
  at width 1 as many
  solve_fgmres_block, preconditioner "double" and "float", k = 4 and 5, restart 5, tolerances between 1e-4 and 1e-8 ||b_c||, random
  initial guesses but for column 0, which starts close to its solution: the columns retire in different iterations, column 0
  inside the first cycle, so that the restart that follows packs the slots
  - every rank gets the same counts and histories
  - two ranks (the all-reduce is one addition per element, whatever the length of the message): iteration count, final residual,
    history and owned solution of every column bit-equal to solve_fgmres of that column on the same ranks
  - four ranks (2 x 1 x 2; gloo may add the ranks' values of a long and of a short message in different orders): the counts equal;
    history and solution within a bound MEASURED in the same run -- 10 x the largest deviation of the one-vector solve_fgmres on
    these ranks from the one-vector solve of the gathered problem on one process, never looser than 1e-6.  A block changes only the
    summation order of the all-reduces, a subset of what another number of ranks changes.
  - all-reduces, counted through the transport: 3 x (iterations of the slowest column) + the cycle starts (the first and one per
    restart with a live column), equal to work["allreduces"] -- the operator and both cycles make none -- and fewer than the k
    one-vector solves make together
  - ||b_c - A x_c|| of every gathered column, by the single-process operator on the global mesh, <= 1.01 x its tolerance

Measured on 2 x 1 x 2 "cube_linear" (relative: max_k |hist_k - ref_k| / ref_k, max|x - x_ref| / max|x_ref| over all columns, both
cycles and k = 4, 5), block against one-vector on the same ranks: preconditioner "double" history 3.6e-13, solution 2.4e-16, under
bounds of 3.8e-11 to 1.3e-10 and 2.4e-15 to 3.6e-15 measured in that run; preconditioner "float" history 4.1e-8 (one column; the
others 2.4e-13 and below, three of five bit-equal), solution 1.0e-13, under bounds of 7.9e-7 to 8.5e-7 and 9.4e-13 to 2.4e-12 -- the
float copy of v rounds a difference in the last bit of a double to a difference in the last bit of a float.  The iteration counts
equal throughout; on the two-rank cases every column bit-equal."""
import argparse
import ctypes as C
import os

import numpy as np
import torch
import torch.distributed as dist

import dist_worker as W  # (puts the repository and the oracle on sys.path)
import mfmg_amd as M
import mixed_material
from mfmg_amd import lib as L
from dist_block_worker import MESHES, CountingTransport

RESTART = 5
RELATIVE = (1e-4, 1e-8, 1e-6, 1e-5, 1e-7)


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
    global_problem = lambda: (mixed_material.global_problem(cells, table, part.h, "cuda") if mixed
                              else M.LaplaceProblem(cells, material, device="cuda", cell_size=part.h))
    ctx = M.Context()
    tr = CountingTransport(ctx, part, 2)
    assert tr.name() == "host"
    ctx.set_block_fgmres_on_ranks()
    gctx = M.Context()
    gprob = global_problem()
    a_global = M.MatrixFreeLaplace(gctx, gprob)
    ng, nl = gprob.n_dofs, part.n_local_dofs
    own_l, own_g, loc_g = part.owned_local_index().numpy(), part.owned_global_index().numpy(), part.local_global_index().numpy()
    ghost_l = np.ones(nl, bool)
    ghost_l[own_l] = False
    assert ghost_l.any()
    own_t = torch.from_numpy(own_l).cuda()
    ld = nl + 2 + (nl & 1)
    k_max = 5
    rng = np.random.default_rng(0)
    bg, xg = rng.random((k_max, ng)), rng.random((k_max, ng))
    # column 0, with the loosest tolerance, starts close to its solution (b_0 = A x*, x_0 = x* perturbed by 3 %), so that it retires
    # inside the first restart cycle on every mesh (the same bits on every rank: one kernel on one card)
    x_star = rng.random(ng)
    b0 = torch.empty(ng, dtype=torch.float64, device="cuda")
    a_global.vmult(b0, torch.from_numpy(x_star).cuda())
    gctx.synchronize()
    bg[0] = b0.cpu().numpy()
    xg[0] = x_star * (1.0 + 0.03 * (rng.random(ng) - 0.5))
    expected_width = 1 if mixed else 4
    lib = L.load()

    def local_block(vg, k, dtype=np.float64, poison=1e30):
        out = np.zeros((k, ld), dtype=dtype)
        out[:, :nl] = vg[:k][:, loc_g]
        out[:, :nl][:, ghost_l] = poison
        return torch.from_numpy(out).cuda()

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

    def gather(v_local):
        out = torch.zeros(ng, dtype=torch.float64)
        out[torch.from_numpy(own_g)] = torch.from_numpy(np.ascontiguousarray(v_local.cpu().numpy()[own_l]))
        return W._all_reduce_cpu(out).numpy()

    def true_residual(c, x_global):
        r = torch.empty(ng, dtype=torch.float64, device="cuda")
        a_global.vmult(r, torch.from_numpy(np.ascontiguousarray(x_global)).cuda())
        gctx.synchronize()
        return np.linalg.norm(bg[c] - r.cpu().numpy())

    def solve_one(hh, b, x, tol, preconditioner):
        """solve_fgmres with the final residual: (iterations, history, residual)"""
        it, res = C.c_int32(), C.c_double()
        hist = np.zeros(201)
        L.check(lib.mfmg_hip_hierarchy_solve_fgmres(hh.handle, b.data_ptr(), x.data_ptr(), float(tol), 200, RESTART,
                                                    1 if preconditioner == "float" else 0, C.byref(it), C.byref(res),
                                                    hist.ctypes.data_as(C.POINTER(C.c_double)), len(hist)))
        return it.value, hist[: it.value + 1].copy(), res.value

    def cycle_start_calls(its, hists, tol):
        """residuals the block driver forms TOGETHER: the first, and one per restart at which a column is still live"""
        calls, r = 1, 1
        while any(i > r * RESTART or (i == r * RESTART and h_[-1] > t) for i, h_, t in zip(its, hists, tol)):
            calls, r = calls + 1, r + 1
        return calls

    def relative_deviation(a, b):
        return float((np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))).max())

    worst_block = [0.0, 0.0]
    for cycle, extra in (("V(0,1)", {"pre_smoothing_levels": 0}), ("V(1,1)", {})):
        params = dict(W.PRM)
        params.update({"smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0},
                       "solver": {"type": "amg", "amg": dict(amg, **extra)}, "is preconditioner": True, "fine level precision": "float"})
        h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", local_problem(), params)
        hg = M.Hierarchy(gctx, "HipMatrixFreeMeshEvaluator", gprob, params) if world > 2 else None

        # ---- the float cycle on blocks
        b32 = bg.astype(np.float32)
        one_exchanges = None
        X1 = torch.zeros(k_max, ld, dtype=torch.float32, device="cuda")
        B1 = local_block(b32, k_max, np.float32, np.nan)
        for c in range(k_max):
            _, ar, one_exchanges = counted(lambda: h.apply_f32(B1[c, :nl].clone(), X1[c, :nl]))
            assert ar == 0, "the float cycle made an all-reduce of its own"
        for k in (4, 5):
            B, X = local_block(b32, k, np.float32, np.nan), torch.zeros(k, ld, dtype=torch.float32, device="cuda")
            _, ar, ex = counted(lambda: h.apply_f32_block(B, X))
            info = h.block_info_f32()
            assert ar == 0
            assert info["width"] == expected_width and same_on_all_ranks([info["width"], ex]), info
            got, ref = X[:, :nl][:, own_t], X1[:k, :nl][:, own_t]
            assert bool(torch.isfinite(ref).all().item())
            assert torch.equal(got, ref), f"{cycle}: apply_f32_block on {k} columns differs from apply_f32 on the owned entries"
            if expected_width == 4:
                assert info["block_launches"] > 0 and ex < k * one_exchanges, (info, ex, one_exchanges)
            else:
                assert info["block_launches"] == 0 and ex == k * one_exchanges, (info, ex, one_exchanges)
            say(f"{cycle}: apply_f32_block k {k}: width {info['width']}, exchanges {ex} ({k} x apply_f32: {k * one_exchanges})")

        # ---- FGMRES on blocks
        y = torch.zeros(nl, dtype=torch.float64, device="cuda")
        _, op_allreduces, _ = counted(lambda: h.operator_apply(0, local_block(bg, 1)[0, :nl].clone(), y))
        _, cycle_allreduces, _ = counted(lambda: h.vmult(torch.zeros(nl, dtype=torch.float64, device="cuda"), local_block(bg, 1)[0, :nl].clone()))
        assert op_allreduces == 0 and cycle_allreduces == 0
        for preconditioner in ("double", "float"):
            for k in (4, 5):
                tol = [RELATIVE[c] * np.linalg.norm(bg[c]) for c in range(k)]
                B1, X1 = local_block(bg, k), local_block(xg, k)
                one, one_allreduces = [], 0
                for c in range(k):
                    out, ar, _ = counted(lambda: solve_one(h, B1[c, :nl].clone(), X1[c, :nl], tol[c], preconditioner))
                    one.append(out)
                    one_allreduces += ar
                B, X = local_block(bg, k), local_block(xg, k)
                (its, hists, work), n_allreduces, n_exchanges = counted(
                    lambda: h.solve_fgmres_block(B, X, tol, 200, restart=RESTART, preconditioner=preconditioner))
                where = f"{cycle} {preconditioner} k {k}"
                assert same_on_all_ranks(list(its) + [v for hh in hists for v in hh] + work["residuals"]), f"{where}: the ranks disagree"
                assert list(its) == [o[0] for o in one], (where, its, [o[0] for o in one])
                # the columns retire in different iterations, and at the last restart one of them had left: the slots were packed
                assert len(set(its)) > 1 and min(its) >= 2, (where, its)
                assert max(its) > RESTART and min(its) <= RESTART * ((max(its) - 1) // RESTART), (where, its)
                calls = cycle_start_calls(its, hists, tol)
                assert n_allreduces == 3 * max(its) + calls, (where, n_allreduces, its, calls)
                assert work["allreduces"] == n_allreduces and n_allreduces < one_allreduces, (where, work, n_allreduces, one_allreduces)
                assert work["preconditioner_columns"] == sum(its) and work["operator_columns"] == sum(its), (where, work, its)
                if preconditioner == "float":
                    assert h.block_info_f32()["width"] == expected_width
                # (four ranks) what another number of ranks does to the one-vector solve of every column
                bound_hist = bound_x = 0.0
                if hg is not None:
                    for c in range(k):
                        xs = torch.from_numpy(xg[c].copy()).cuda()
                        its_g, hist_g, _ = solve_one(hg, torch.from_numpy(bg[c].copy()).cuda(), xs, tol[c], preconditioner)
                        gctx.synchronize()
                        assert its_g == one[c][0], (where, c, its_g, one[c][0])
                        x_ref = xs.cpu().numpy()
                        bound_hist = max(bound_hist, relative_deviation(one[c][1], hist_g))
                        bound_x = max(bound_x, float(np.abs(gather(X1[c, :nl]) - x_ref).max() / np.abs(x_ref).max()))
                    bound_hist, bound_x = min(10 * bound_hist, 1e-6), min(10 * bound_x, 1e-6)
                for c in range(k):
                    it1, hist1, res1 = one[c]
                    xo, xo1 = X[c, :nl][own_t], X1[c, :nl][own_t]
                    d_hist = relative_deviation(hists[c], hist1)
                    d_x = float(((xo - xo1).abs().max() / xo1.abs().max()).item())
                    d_res = abs(work["residuals"][c] - res1) / res1
                    worst_block = [max(worst_block[0], d_hist), max(worst_block[1], d_x)]
                    say(f"{where} column {c}: {its[c]} iterations, deviation from solve_fgmres history {d_hist:.3e} solution {d_x:.3e} "
                        f"residual {d_res:.3e}" + (f" (bounds {bound_hist:.3e} {bound_x:.3e})" if hg is not None else ""))
                    if world == 2:
                        assert np.array_equal(np.asarray(hists[c]).view(np.int64), np.asarray(hist1).view(np.int64)), (where, c, d_hist)
                        assert np.float64(work["residuals"][c]).tobytes() == np.float64(res1).tobytes(), (where, c, d_res)
                        assert torch.equal(xo, xo1), (where, c, d_x)
                    else:
                        assert d_hist <= bound_hist and d_res <= bound_hist, (where, c, d_hist, d_res, bound_hist)
                        assert d_x <= bound_x, (where, c, d_x, bound_x)
                    res = true_residual(c, gather(X[c, :nl]))
                    assert res <= 1.01 * tol[c], (where, c, res, tol[c])
                say(f"{where}: iterations {list(its)}, all-reduces {n_allreduces} (the {k} one-vector solves: {one_allreduces}), "
                    f"cycle starts {calls}, exchanges {n_exchanges}, work {work}")
        del h, hg
    say(f"distributed block fgmres checks passed; grid {'x'.join(map(str, grid))} mesh {args.mesh} width {expected_width}; block against "
        f"the one-vector solves: worst deviation history {worst_block[0]:.3e} solution {worst_block[1]:.3e}")


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
