"""Flexible GMRES on blocks of right-hand sides and the FP32 block level on several ranks, against the one-vector calls on the same
ranks.

Processes (tests/dist_block_fgmres_worker.py under torch.distributed.run, gloo, all ranks sharing one card, the host transport):
slabs 1 x 1 x 2 on the mesh "small"; boxes 2 x 1 x 1 with two ghost agglomerates below and 2 x 1 x 2, 24^3 cells per rank, linear;
slabs 1 x 1 x 2 on the "mixed" material, where one rank has no block kernel and all ranks loop over the columns.  The worker's
docstring lists the checks.

Threads (eight ranks of a 2 x 2 x 2 grid in one process, 16^3 cells per rank, linear; seven neighbours per rank in every exchange):
solve_fgmres_block at k = 4 with the non-symmetric V(0,1) cycle and restart 5, bit-equal per column to solve_fgmres on the same
eight ranks, behind the mailboxes of tests/test_gpu_block_distributed.py that add the ranks' slots in rank order, element by
element -- the bit contract of the block solve holds where the transport adds the ranks' values of an element in the same order
whatever the length of the message."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import mfmg_amd as M
from test_gpu_block_distributed import OrderedMailboxes, _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(world, grid, mesh, low_ghost, timeout=600):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "dist_block_fgmres_worker.py"), "--mesh", mesh, "--grid", grid, "--low-ghost", str(low_ghost)]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    if res.returncode != 0:
        # the first traceback of a rank (the tail of stderr is the launcher's summary)
        at = res.stderr.find("Traceback")
        raise AssertionError(res.stdout[-3000:] + (res.stderr[at:at + 3000] if at >= 0 else res.stderr[-3000:]))
    return res.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("world,grid,mesh,low_ghost", [(2, "1x1x2", "small", 2), (2, "2x1x1", "cube_linear", 4), (4, "2x1x2", "cube_linear", 2),
                                                       (2, "1x1x2", "mixed", 2)])
def test_block_fgmres_on_ranks_matches_the_one_vector_solves(mfmg_lib, world, grid, mesh, low_ghost):
    out = _run(world, grid, mesh, low_ghost)
    print(out)
    assert f"distributed block fgmres checks passed; grid {grid} mesh {mesh} width {1 if mesh == 'mixed' else 4}" in out
    # both cycles, both preconditioners, k = 4 and 5
    for cycle in ("V(0,1)", "V(1,1)"):
        for preconditioner in ("double", "float"):
            for k in (4, 5):
                assert f"{cycle} {preconditioner} k {k}: iterations" in out


@pytest.mark.gpu
def test_block_fgmres_on_2x2x2_threads_matches_the_one_vector_solves(mfmg_lib):
    grid, per, k, restart = (2, 2, 2), 16, 4, 5
    cells = tuple(per * g for g in grid)
    length = tuple(c / float(cells[0]) for c in cells)
    params = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2},
              "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0},
              "solver": {"type": "amg", "amg": {"coarsest_size": 300, "pre_smoothing_levels": 0}}, "is preconditioner": True}
    ng = (cells[0] + 1) * (cells[1] + 1) * (cells[2] + 1)
    rng = np.random.default_rng(5)
    bg, xg = rng.random((k, ng)), rng.random((k, ng))
    relative = (1e-4, 1e-8, 1e-6, 1e-5)
    tol = [relative[c] * np.linalg.norm(bg[c]) for c in range(k)]
    n_ranks = 8
    mb = OrderedMailboxes(n_ranks, timeout=120)
    errors, results = [None] * n_ranks, [None] * n_ranks

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            part = M.BoxPartition(cells, rank, grid, length=length)
            ctx = M.Context()
            tr = M.HaloTransport(ctx, part, callbacks=mb.callbacks(rank))
            ctx.set_block_fgmres_on_ranks()
            h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", part.local_problem("linear", "cuda"), params)
            assert h.block_info()["width"] == 4, h.block_info()
            nl = part.n_local_dofs
            own_l, loc_g = part.owned_local_index().numpy(), part.local_global_index().numpy()
            ghost = np.ones(nl, bool)
            ghost[own_l] = False
            own_t = torch.from_numpy(own_l).cuda()
            ld = nl + 2 + (nl & 1)

            def block(vg):
                out = np.zeros((k, ld))
                out[:, :nl] = vg[:, loc_g]
                out[:, :nl][:, ghost] = 1e30
                return torch.from_numpy(out).cuda()
            B1, X1 = block(bg), block(xg)
            its1, hist1 = [], []
            for c in range(k):
                it, hist = h.solve_fgmres(B1[c, :nl].clone(), X1[c, :nl], tol[c], 200, restart=restart)
                its1.append(it)
                hist1.append(hist)
            B, X = block(bg), block(xg)
            its, hists, work = h.solve_fgmres_block(B, X, tol, 200, restart=restart)
            ctx.synchronize()
            results[rank] = dict(its=list(its), its1=its1, work=work,
                                 hist_equal=[np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)) for a, b in zip(hists, hist1)],
                                 x_equal=torch.equal(X[:, :nl][:, own_t], X1[:, :nl][:, own_t]))
            del h
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors[rank] = e
            mb.barrier.abort()
            for p in range(n_ranks):      # wake the neighbours that wait for a message of this rank
                mb.q[(rank, p)].put(np.zeros(0))

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    first = next((e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError)), None) or \
        next((e for e in errors if e is not None), None)
    if first is not None:
        raise first
    assert all(r is not None for r in results)
    r0 = results[0]
    print(f"2 x 2 x 2: FGMRES({restart}) iterations {r0['its']}, work {r0['work']}")
    for rank, r in enumerate(results):
        assert r["its"] == r["its1"] == r0["its"] and len(set(r["its"])) > 1, (rank, r["its"], r["its1"])
        assert all(r["hist_equal"]), f"rank {rank}: the residual history of solve_fgmres_block differs from solve_fgmres"
        assert r["x_equal"], f"rank {rank}: the solution of solve_fgmres_block differs from solve_fgmres on the owned entries"
        assert r["work"]["preconditioner_columns"] == sum(r["its"]) and r["work"]["block_launches"] > 0, (rank, r["work"])
        assert r["work"]["allreduces"] >= 3 * max(r["its"]) + 1, (rank, r["work"])
