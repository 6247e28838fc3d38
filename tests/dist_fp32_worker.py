"""Worker of tests/test_gpu_fp32_distributed.py: run with torch.distributed.run, backend gloo, all ranks on cuda:0, the host
transport.  The FP32 fine level ("fine level precision" float) on the ranks of a slab or box grid against one process on the
global mesh.  A failing rank raises, so it exits non-zero; nothing retries.

1. Context.exchange_f32: a float vector that holds a function of the global node index, ghost entries NaN, exchanged 1, 2 and 3
   planes deep.  Every ghost entry the exchange of that width refreshes (HaloTransport.box_messages: the library's own list) is
   bit-equal to the owner's value, every other ghost entry is still NaN, every owned entry is untouched; the exchange counter
   advances by one and the volume by what the FP64 exchange of that width moves (width 1: measured on mfmg_hip_context_exchange in
   the same run; wider: BoxPartition.exchange_doubles, the figure tests/dist_worker.py holds the FP64 exchange to).  A width
   beyond the ghost planes every rank holds below (3 with two ghost cell layers) is refused on every rank, nothing is sent.
2. Hierarchy.operator_f32 -- vmult, residual, a smoother term with momentum -- on ranks (x, b, x_prev with NaN ghost entries)
   against the same call of the single-process hierarchy, owned entries gathered: tests/fp32_reference.py's per-kernel bound
   (assert_within with the reference's k and magnitudes).
3. Hierarchy.apply_f32 for both "is preconditioner" settings (false: a random x with NaN ghost entries; b with NaN ghost entries
   in both) against apply_f32 of one process.  Reference: the FP64 cycle of one process, x64.  With d(x) = ||x - x64||_2 / ||x64||_2,
   d(distributed FP32) <= 2 d(single-process FP32): both are float roundings of the same operator with another summation order at
   tile and rank boundaries; a wrong ghost plane is an O(1) relative error.  Both figures are printed.
   Exchanges of one cycle: those of the FP64 cycle of the same distributed hierarchy, plus one where that cycle restricts the
   residual in one pass (x two planes deep: one exchange; b is shared with the sweep) and the FP32 cycle in two steps (x, then the
   widened residual: two) -- that is, where the hierarchy has residual-restriction classes and the smoother sweeps.  Counted on
   the cases of the test, FP32 / FP64: 1x1x2 16 / 15; 2x1x1 with two ghost agglomerates 14 / 13 (as a preconditioner 13 / 12: the
   first pre-smoothing sweep starts from zero and exchanges no x); 2x1x2 16 / 15; the mixed material (no sweep, two-step
   restriction in both) 17 / 17.  Measured deviations d: one process 4.3e-8 to 6.8e-8, ranks 4.3e-8 to 6.7e-8.
4. solve_fgmres(preconditioner="float"), tolerance 1e-8 ||b||: converges; the same count and history on every rank; the count
   within one of the single-process FP32-preconditioned solve; ||b - A x|| of the gathered solution by the single-process FP64
   operator within the tolerance; three all-reduces per iteration on top of what the operator and the cycle make themselves."""
import argparse
import os

import numpy as np
import torch
import torch.distributed as dist

import dist_worker as W  # (puts the repository and the oracle on sys.path)
import fp32_reference as F
import mfmg_amd as M
import mfmg_oracle as O
import mixed_material
from dist_krylov_worker import CountingTransport
from mfmg_amd import lib as L

# name: (cells per rank along z, (cx, cy) per rank along x and y (slabs: the global counts), material, amg parameters) -- the two
# smallest meshes of tests/dist_worker.py with a sweep ("cube11") and with ranks whose materials differ ("mixed")
MESHES = {"cube11": W.MESHES["cube11"], "mixed": W.MESHES["mixed"]}


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
    params.update({"smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}, "solver": {"type": "amg", "amg": dict(amg)},
                   "fine level precision": "float"})
    ctx, gctx = M.Context(), M.Context()
    tr = CountingTransport(ctx, part, 2)
    assert tr.name() == "host"
    gprob = mixed_material.global_problem(cells, table, part.h, "cuda") if mixed else M.LaplaceProblem(cells, material, device="cuda", cell_size=part.h)
    ng, nl = gprob.n_dofs, part.n_local_dofs
    own_l, own_g, loc_g = part.owned_local_index().numpy(), part.owned_global_index().numpy(), part.local_global_index().numpy()
    ghost_l = np.ones(nl, bool)
    ghost_l[own_l] = False
    assert ghost_l.any()
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    say = lambda *a: print(*a, flush=True) if rank == 0 else None

    def local(vg, poison=np.nan):
        v = vg[loc_g].copy()
        v[ghost_l] = poison           # ghosts must come from the library's exchanges
        return v

    def gather(v_local):
        out = torch.zeros(ng, dtype=torch.float64)
        out[torch.from_numpy(own_g)] = torch.from_numpy(np.ascontiguousarray(v_local.cpu().numpy()[own_l].astype(np.float64)))
        return W._all_reduce_cpu(out).numpy()

    def same_on_all_ranks(values):
        t = torch.zeros(world, len(values), dtype=torch.float64)
        t[rank] = torch.tensor(values, dtype=torch.float64)
        W._all_reduce_cpu(t)
        return bool((t == t[rank]).all())

    def counted(f):
        a, e = tr.n_allreduces, tr.n_exchanges()
        out = f()
        ctx.synchronize()
        return out, tr.n_allreduces - a, tr.n_exchanges() - e

    def hierarchies(is_preconditioner):
        p = dict(params)
        p["is preconditioner"] = is_preconditioner
        return (M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", local_problem(), p), M.Hierarchy(gctx, "HipMatrixFreeMeshEvaluator", gprob, p))

    h, hg = hierarchies(False)
    # ---- the agreed sweep of the FP32 smoother: the same on every rank, and the FP64 smoother's on these meshes
    expect_terms = 0 if mixed else (3 if args.low_ghost == 4 else 2)
    assert h.sweep_terms_f32() == expect_terms == max(h.smoother_sweep_terms()), (h.sweep_terms_f32(), h.smoother_sweep_terms())
    assert same_on_all_ranks([h.sweep_terms_f32()])
    if mixed:
        mine = mixed_material.cell_constant(local_problem().coefficient)
        assert mine == (rank in mixed_material.expected_constant_ranks(material, world))   # ranks that could sweep on their own

    # ---- 1. exchange_f32
    value = lambda gid: ((gid * 2654435761) % (1 << 24)).astype(np.float32)      # exact in float32
    for width in (1, 2, 3):
        filled = value(loc_g.astype(np.int64))
        filled[ghost_l] = np.nan
        v = dev(filled)
        before = v.cpu().numpy().copy()
        n0, v0 = tr.n_exchanges(), tr.exchange_volume()
        if width > args.low_ghost:
            try:
                ctx.exchange_f32(1, v, width)
                raise AssertionError("an exchange deeper than the ghost planes below must be refused")
            except L.MfmgInvalidArgument:
                pass
            assert (tr.n_exchanges(), tr.exchange_volume()) == (n0, v0)
            continue
        ctx.exchange_f32(1, v, width)
        ctx.synchronize()
        d_count, d_volume = tr.n_exchanges() - n0, tr.exchange_volume() - v0
        got = v.cpu().numpy()
        _, counts, _, recv = tr.box_messages(1, width)
        # the ghost nodes within `width` planes of the owned box along every axis (there are ghost planes towards neighbours only)
        nx, ny, _ = part.local_nodes
        node = np.arange(nl)
        pos = (node % nx, (node // nx) % ny, node // (nx * ny))
        refreshed = ghost_l.copy()
        for d in range(3):
            refreshed &= (pos[d] >= part.own0[d] - width) & (pos[d] < part.own0[d] + part.own_n[d] + width)
        assert np.array_equal(np.sort(recv), np.flatnonzero(refreshed)) and refreshed.sum() == counts.sum()
        assert np.array_equal(got[refreshed].view(np.uint32), value(loc_g[refreshed].astype(np.int64)).view(np.uint32)), f"width {width}: ghost values"
        assert np.isnan(got[ghost_l & ~refreshed]).all(), f"width {width}: a ghost entry beyond the width was written"
        assert np.array_equal(got[own_l].view(np.uint32), before[own_l].view(np.uint32)), f"width {width}: an owned entry changed"
        assert d_count == 1 and d_volume == part.exchange_doubles(width) == counts.sum(), (width, d_count, d_volume, part.exchange_doubles(width))
        if width == 1:
            v64 = dev(local(rng.random(ng), 0.0))
            n0, v0 = tr.n_exchanges(), tr.exchange_volume()
            tr.exchange(1, v64)
            ctx.synchronize()
            assert (tr.n_exchanges() - n0, tr.exchange_volume() - v0) == (d_count, d_volume)
        say(f"exchange_f32 width {width}: {int(counts.sum())} entries in {len(counts)} messages")
    for space in (0, 2):
        try:
            ctx.exchange_f32(space, torch.zeros(nl, dtype=torch.float32, device="cuda"), 1)
            raise AssertionError("exchange_f32 takes the fine space only")
        except L.MfmgInvalidArgument:
            pass

    # ---- 2. the FP32 operator on ranks against one process
    ref = F.Reference(cells, gprob.coefficient.cpu().numpy())
    ref.mesh.h = part.h                                             # (cubic cells: the reference's mesh is the unit cube)
    ref.Ke = O.cell_matrices(ref.mesh, ref.coef).astype(F.LD)
    ref.kmax = np.abs(ref.Ke).max(axis=(1, 2))
    ref.dinv = ref.dinv_from(ref.coef)
    x32, b32, p32 = (F.f32(rng.random(ng) - 0.5) for _ in range(3))
    alpha, beta = 0.3, 0.8
    cases = [("vmult", {}, ref.unit_vmult(x32), ref.k_op), ("residual", {"b": b32}, ref.unit_residual(x32, b32), ref.k_op),
             ("step", {"b": b32, "x_prev": p32, "alpha": alpha, "beta": beta}, ref.unit_step(x32, b32, p32, alpha, beta), ref.k_step)]
    for mode, extra, unit, k in cases:
        lo = {n: (dev(local(a, np.float32(np.nan))) if isinstance(a, np.ndarray) else a) for n, a in extra.items()}
        gl = {n: (dev(a) if isinstance(a, np.ndarray) else a) for n, a in extra.items()}
        out_l, out_g = torch.zeros(nl, dtype=torch.float32, device="cuda"), torch.zeros(ng, dtype=torch.float32, device="cuda")
        h.operator_f32(mode, dev(local(x32, np.float32(np.nan))), out_l, **lo)
        hg.operator_f32(mode, dev(x32), out_g, **gl)
        ctx.synchronize()
        gctx.synchronize()
        got, single = gather(out_l), out_g.cpu().numpy().astype(F.LD)
        say(f"operator_f32 {mode}: worst |ranks - one process| / (u mag) = {F.worst_ratio(got, single, unit):.2f} (bound {k})")
        F.assert_within(got, single, unit, k, f"FP32 {mode} on ranks against one process")

    # ---- 3. the cycle, 4. FGMRES
    bg, xg = rng.random(ng), rng.random(ng)
    rel = lambda a, r: float(np.linalg.norm(a - r) / np.linalg.norm(r))
    for is_preconditioner in (False, True):
        if is_preconditioner:
            del h, hg
            h, hg = hierarchies(True)
        start = F.f32(1e6 * rng.random(ng)) if is_preconditioner else F.f32(xg)      # (a preconditioner application zeroes x itself)
        x64 = dev(start.astype(np.float64))
        hg.apply(dev(bg), x64)
        xs = dev(start)
        hg.apply_f32(dev(F.f32(bg)), xs)
        gctx.synchronize()
        xl = dev(local(start, np.float32(np.nan)))
        _, _, n_f32 = counted(lambda: h.apply_f32(dev(local(F.f32(bg), np.float32(np.nan))), xl))
        x_ref = x64.cpu().numpy()
        d_single, d_ranks = rel(xs.cpu().numpy().astype(np.float64), x_ref), rel(gather(xl), x_ref)
        # the FP64 cycle of the same distributed hierarchy (a second application: its first one has yet to learn that the sweep
        # reads b at ghost DoFs, and sends b later in the cycle -- the same count)
        x64l = dev(local(start.astype(np.float64), 0.0))
        h.apply(dev(local(bg, 0.0)), x64l)
        _, _, n_f64 = counted(lambda: h.apply(dev(local(bg, 0.0)), x64l))
        one_pass = h.residual_restriction_classes() > 0
        extra = 1 if (one_pass and h.sweep_terms_f32() > 0) else 0
        say(f"apply_f32 is_preconditioner={is_preconditioner}: deviation from the FP64 cycle, one process {d_single:.3e}, ranks {d_ranks:.3e}; "
            f"exchanges per cycle: FP32 {n_f32}, FP64 {n_f64} (one-pass restriction: {one_pass})")
        assert 0.0 < d_single < 1e-4, d_single
        assert d_ranks <= 2.0 * d_single, (d_ranks, d_single)
        assert n_f32 == n_f64 + extra, (n_f32, n_f64, extra)

    # (h, hg: "is preconditioner" true)
    tol = 1e-8 * np.linalg.norm(bg)
    y = torch.zeros(nl, dtype=torch.float64, device="cuda")
    _, op_allreduces, _ = counted(lambda: h.operator_apply(0, dev(local(bg, 1e30)), y))
    _, cycle_allreduces, _ = counted(lambda: h.apply_f32(dev(local(F.f32(bg), np.float32(np.nan))), torch.zeros(nl, dtype=torch.float32, device="cuda")))
    restart = 30
    xl = dev(local(xg, 1e30))
    (its, hist), n_allreduces, _ = counted(lambda: h.solve_fgmres(dev(local(bg, 1e30)), xl, tol, 200, restart=restart, preconditioner="float"))
    xs = dev(xg)
    its_g, hist_g = hg.solve_fgmres(dev(bg), xs, tol, 200, restart=restart, preconditioner="float")
    gctx.synchronize()
    assert same_on_all_ranks([its] + list(hist)), "the ranks disagree on the iteration"
    assert hist[-1] <= tol and 3 <= its <= 60, (its, hist[-1], tol)
    assert abs(its - its_g) <= 1, (its, its_g)
    r = torch.empty(ng, dtype=torch.float64, device="cuda")
    hg.operator_apply(0, dev(gather(xl)), r)
    gctx.synchronize()
    res = float(np.linalg.norm(bg - r.cpu().numpy()))
    starts = -(-its // restart) + (1 if hist[-1] > tol else 0)
    say(f"fgmres float: iterations {its} (one process {its_g}), true residual / tolerance {res / tol:.4f}, all-reduces {n_allreduces} "
        f"(cycle {cycle_allreduces}, operator {op_allreduces})")
    assert res <= tol, (res, tol)
    assert n_allreduces == its * (3 + op_allreduces + cycle_allreduces) + starts * (1 + op_allreduces), (n_allreduces, its, starts)
    say(f"distributed fp32 checks passed; grid {'x'.join(map(str, grid))} sweep terms {h.sweep_terms_f32()}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="cube11")
    ap.add_argument("--grid", default="")
    ap.add_argument("--low-ghost", type=int, default=2)
    a = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    try:
        main(a)
    finally:
        dist.destroy_process_group()
