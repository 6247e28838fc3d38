"""Worker of tests/test_gpu_sweep_stored_diagonal_distributed.py: run with torch.distributed.run, backend gloo, all ranks on
cuda:0, the host transport.  The FP64 cycle of a distributed hierarchy whose Chebyshev(3) smoother is one sweep of twelve
wavefronts of two rows (mesh cube11 of tests/dist_worker.py, 2 x 1 x 1 ranks, two ghost agglomerates below: x three planes deep),
built twice on the same ranks: with the D^-1 vector of the sweep (the default) and under MFMG_MF_SWEEP_DINV=derived, which is
read when an operator is constructed.  The vector holds the bits the kernels derive, at ghost DoFs as at any other local DoF,
and nothing about the exchanges depends on it: the owned entries of x after two cycles are equal with torch.equal, and both
hierarchies ask the transport for the same number of exchanges per cycle.  A failing rank raises, so it exits non-zero."""
import argparse
import os

import numpy as np
import torch
import torch.distributed as dist

import dist_worker as W  # (puts the repository and the oracle on sys.path)
import mfmg_amd as M


def main(args):
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    grid = W.parse_grid(args.grid, world)
    per, (cx, cy), material, amg = W.MESHES["cube11"]
    cells = (cx * grid[0], cy * grid[1], per * grid[2])
    part = M.BoxPartition(cells, rank, grid, length=tuple(c / float(cells[0]) for c in cells), low_ghost_cells=4)
    params = dict(W.PRM)
    params.update({"smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0},
                   "solver": {"type": "amg", "amg": dict(amg)}, "is preconditioner": False})
    ctx = M.Context()
    tr = M.HaloTransport(ctx, part, 2)
    assert tr.name() == "host"
    ng, nl = int(np.prod([c + 1 for c in cells])), part.n_local_dofs
    own_l, loc_g = part.owned_local_index().numpy(), part.local_global_index().numpy()
    ghost_l = np.ones(nl, bool)
    ghost_l[own_l] = False
    assert ghost_l.any()
    rng = np.random.default_rng(0)
    bg, xg = rng.random(ng), rng.random(ng)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def local(vg):
        v = vg[loc_g].copy()
        v[ghost_l] = 0.0              # ghosts must come from the library's exchanges
        return v

    def cycles(expect):
        # a stand-alone operator on the same context: what an operator of this rank's local mesh reports
        op = M.MatrixFreeLaplace(ctx, part.local_problem(material, "cuda"))
        assert op.sweep_diagonal() == expect, (op.sweep_diagonal(), expect)
        del op
        h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", part.local_problem(material, "cuda"), params)
        assert max(h.smoother_sweep_terms()) == 3 and tuple(h.sweep_tile(3))[:2] == (12, 2), (h.smoother_sweep_terms(), h.sweep_tile(3))
        x = dev(local(xg))
        h.apply(dev(local(bg)), x)    # (the first application learns that the sweep reads b at ghost DoFs)
        n0 = tr.n_exchanges()
        h.apply(dev(local(bg)), x)
        ctx.synchronize()
        n = tr.n_exchanges() - n0
        out = x.clone()
        del h
        return out, n

    assert "MFMG_MF_SWEEP_DINV" not in os.environ
    x_stored, n_stored = cycles("stored")
    os.environ["MFMG_MF_SWEEP_DINV"] = "derived"
    try:
        x_derived, n_derived = cycles("derived")
    finally:
        del os.environ["MFMG_MF_SWEEP_DINV"]
    own = torch.from_numpy(own_l).cuda()
    assert torch.isfinite(x_derived[own]).all()
    assert torch.equal(x_stored[own], x_derived[own]), "the distributed cycle with the stored D^-1 differs from the derived one"
    assert n_stored == n_derived, (n_stored, n_derived)
    if rank == 0:
        print(f"distributed stored-diagonal checks passed; grid {'x'.join(map(str, grid))}, {n_stored} exchanges per cycle", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="2x1x1")
    a = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    try:
        main(a)
    finally:
        dist.destroy_process_group()
