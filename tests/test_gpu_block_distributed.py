"""Blocks of right-hand sides on several ranks: the operator, the smoother, the cycle and CG on blocks against the one-vector calls
on the same ranks.

Processes (tests/dist_block_worker.py under torch.distributed.run, gloo, all ranks sharing one card, the host transport): slabs
1 x 1 x 2 on the mesh "small"; boxes 2 x 1 x 1 with two ghost agglomerates below and 2 x 1 x 2, 24^3 cells per rank, linear, the
symmetric amg parameters of "deep"; slabs 1 x 1 x 2 on the "mixed" material, where one rank has no block kernel and all ranks loop
over the columns.  The worker's docstring lists the checks.

Threads (eight ranks of a 2 x 2 x 2 grid in one process, 16^3 cells per rank, linear; seven neighbours per rank in every exchange):
apply_block and solve_cg_block at k = 4, bit-equal per column to apply and solve_cg on the same eight ranks.  The bit contract of the
block solve holds where the transport adds the ranks' values of an element in the same order whatever the length of the message.
The mailboxes of tests/test_box_threads.py sum the slots with numpy.sum, which adds eight 1-long messages pairwise and eight
4-long ones row by row -- other bits; the mailboxes here add the slots in rank order, element by element."""
import os
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
from test_box_threads import Mailboxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, grid, mesh, low_ghost, timeout=600):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "dist_block_worker.py"), "--mesh", mesh, "--grid", grid, "--low-ghost", str(low_ghost)]
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
def test_blocks_on_ranks_match_the_one_vector_calls(mfmg_lib, world, grid, mesh, low_ghost):
    out = _run(world, grid, mesh, low_ghost)
    print(out)
    assert f"distributed block checks passed; grid {grid} mesh {mesh} width {1 if mesh == 'mixed' else 4}" in out
    assert out.count("solve_cg_block k ") >= 2


class OrderedMailboxes(Mailboxes):
    """Mailboxes whose all-reduce adds the ranks' slots in rank order, element by element: the same bits for an element whether it
    travels alone or in a longer message"""

    def callbacks(self, rank):
        exchange, _, allgather = super().callbacks(rank)

        def allreduce(values, op):
            self.slots[rank] = np.array(values, copy=True)
            self.barrier.wait()
            res = np.array(self.slots[0], copy=True)
            for r in range(1, self.n):
                res = np.maximum(res, self.slots[r]) if op == 1 else res + self.slots[r]
            self.barrier.wait()          # nobody overwrites a slot before everybody has read it
            values[:] = res
        return exchange, allreduce, allgather


def test_ordered_mailboxes_sum_an_element_alike_in_short_and_long_messages():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((8, 4)) * 10.0 ** rng.uniform(-3, 3, (8, 4))

    def reduce(columns):
        mb = OrderedMailboxes(8, timeout=30)
        out = [None] * 8

        def worker(r):
            v = np.array(a[r, columns], copy=True)
            mb.callbacks(r)[1](v, 0)
            out[r] = v
        threads = [threading.Thread(target=worker, args=(r,)) for r in range(8)]
        [t.start() for t in threads]
        [t.join(timeout=60) for t in threads]
        assert all(o is not None and o.tobytes() == out[0].tobytes() for o in out)
        return out[0]
    long = reduce([0, 1, 2, 3])
    for c in range(4):
        assert reduce([c]).tobytes() == long[c: c + 1].tobytes()


@pytest.mark.gpu
def test_blocks_on_2x2x2_threads_match_the_one_vector_calls(mfmg_lib):
    grid, per, k = (2, 2, 2), 16, 4
    cells = tuple(per * g for g in grid)
    length = tuple(c / float(cells[0]) for c in cells)
    params = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2},
              "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0},
              "solver": {"type": "amg", "amg": {"coarsest_size": 300}}, "is preconditioner": True}
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
            # the cycle
            B1, X1 = block(bg), block(xg)
            e0 = tr.n_exchanges()
            for c in range(k):
                h.apply(B1[c, :nl].clone(), X1[c, :nl])
            ctx.synchronize()
            e1 = tr.n_exchanges()
            B, X = block(bg), block(xg)
            h.apply_block(B, X)
            ctx.synchronize()
            e2 = tr.n_exchanges()
            info = h.block_info()
            cycle_equal = torch.equal(X[:, :nl][:, own_t], X1[:, :nl][:, own_t])
            # CG
            B1, X1 = block(bg), block(xg)
            its1, hist1 = [], []
            for c in range(k):
                it, hist = h.solve_cg(B1[c, :nl].clone(), X1[c, :nl], tol[c], 200)
                its1.append(it)
                hist1.append(hist)
            B, X = block(bg), block(xg)
            its, hists, work = h.solve_cg_block(B, X, tol, 200)
            ctx.synchronize()
            results[rank] = dict(cycle_equal=cycle_equal, info=info, exchanges=(e1 - e0, e2 - e1), its=list(its), its1=its1,
                                 hist_equal=[np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)) for a, b in zip(hists, hist1)],
                                 x_equal=torch.equal(X[:, :nl][:, own_t], X1[:, :nl][:, own_t]), work=work)
            try:
                h.solve_fgmres_block(B, X, tol, 10)
                raise AssertionError("solve_fgmres_block on ranks must be refused")
            except L.MfmgInvalidArgument as e:
                assert "communicator" in str(e)
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
    print(f"2 x 2 x 2: exchanges of 4 cycles {r0['exchanges'][0]}, of a cycle on 4 columns {r0['exchanges'][1]}; CG iterations {r0['its']}, work {r0['work']}")
    for rank, r in enumerate(results):
        assert r["cycle_equal"], f"rank {rank}: apply_block differs from apply on the owned entries"
        assert r["info"]["width"] == 4 and r["info"]["block_launches"] > 0, (rank, r["info"])
        assert r["exchanges"] == r0["exchanges"] and r["exchanges"][1] < r["exchanges"][0], (rank, r["exchanges"])
        assert r["its"] == r["its1"] == r0["its"] and len(set(r["its"])) > 1, (rank, r["its"], r["its1"])
        assert all(r["hist_equal"]), f"rank {rank}: the residual history of solve_cg_block differs from solve_cg"
        assert r["x_equal"], f"rank {rank}: the solution of solve_cg_block differs from solve_cg on the owned entries"
        assert r["work"]["preconditioner_columns"] == sum(r["its"]) and r["work"]["block_launches"] > 0, (rank, r["work"])
