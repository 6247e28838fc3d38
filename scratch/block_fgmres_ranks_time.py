"""Block FGMRES on a rank of the 2 x 2 x 2 run, measured on one GPU, `material linear`, the V(0,1) cycle.

The harness of scratch/block_ranks_time.py: eight ranks are set up as threads of this process behind in-memory mailboxes (the setup
needs the real neighbours), then ONE rank switches to the reflecting transport -- every message it sends comes back on the device as
the message it would have received, an all-reduce is the identity -- and runs alone, with a wire that costs nothing or `delay`
microseconds of stream time per grouped send/recv and collective.  No wire COST (bytes per second) can be measured this way, and no
second GPU is involved.

Per delay (default 0 and 20 us) and preconditioner ("double"; "float" where FLOAT=1), after warm-up, seven repetitions that alternate
the two variants, microseconds per column:
  fgmres  solve_fgmres on each of 4 columns | solve_fgmres_block on the 4 columns, `iters` iterations each in one restart cycle
          (tolerance 0: behind the reflecting transport the numbers are not a solution of anything, so the count is fixed by
          max_iterations)
One JSON line per comparison: every repetition, the medians, the ratio of the medians and the range (max - min) / median, the
exchanges of either variant and the all-reduces (the block's as the library counts them, the loop's 4 x (3 iters + 1)).

usage: block_fgmres_ranks_time.py [cells_per_rank=128] [rank=0] [iters=10]      env DELAY_US=0,20  LOW_GHOST=2|4 (default 4)  FLOAT=0|1"""
import gc, json, os, sys, threading, time
os.environ.setdefault("OMP_NUM_THREADS", "2")    # eight ranks as threads: the default OpenMP team per rank starves the launching threads
import numpy as np
import torch
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mfmg_amd as M
from mfmg_amd import lib as L
from test_box_threads import Mailboxes

per = int(sys.argv[1]) if len(sys.argv) > 1 else 128
timed_rank = int(sys.argv[2]) if len(sys.argv) > 2 else 0
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
delays = [float(v) for v in os.environ.get("DELAY_US", "0,20").split(",") if v]
with_float = os.environ.get("FLOAT", "0") == "1"
grid, K, TRIPS = (2, 2, 2), 4, 7
n_ranks = 8
cells = tuple(per * g for g in grid)
length = tuple(float(g) for g in grid)
params = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"partitioner": "block", "nx": 2, "ny": 2, "nz": 2},
          "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0, "n_smoothing_steps": 1},
          "solver": {"type": "amg", "amg": {"smoother_degree": 1, "smoothing_range": 4.0, "n_cycles": 1, "aggregate_block": 2,
                                            "pre_smoothing_levels": 0}},
          "is preconditioner": True, "max levels": 2}
if with_float:
    params["fine level precision"] = "float"


mb = Mailboxes(n_ranks)
errors = [None] * n_ranks
ready = threading.Barrier(n_ranks, timeout=3600)


def wall(ctx, fn):
    """microseconds of wall clock of fn, the stream drained before and after"""
    ctx.synchronize(); torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    ctx.synchronize(); torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6


def compare(ctx, what, extra, variants):
    for fn in variants.values():
        fn(); fn()
    runs = {name: [] for name in variants}
    gc.collect(); gc.disable()
    try:
        for _ in range(TRIPS):
            for name, fn in variants.items():                 # the variants alternate
                runs[name].append(wall(ctx, fn) / K)
    finally:
        gc.enable()
    med = {name: sorted(r)[len(r) // 2] for name, r in runs.items()}
    out = {"comparison": what, "columns": K, "repetitions": TRIPS,
           "us_per_column": {k: [round(v, 1) for v in r] for k, r in runs.items()},
           "median_us_per_column": {k: round(v, 1) for k, v in med.items()},
           "ratio_to_loop": {k: round(v / med["loop"], 4) for k, v in med.items()},
           "range": {k: round((max(r) - min(r)) / med[k], 4) for k, r in runs.items()}}
    out.update(extra)
    print(json.dumps(out), flush=True)


def quiet(fn):
    """a solve that stops at max_iterations (tolerance 0) reports no convergence: that is the plan here"""
    try:
        fn()
    except L.MfmgError:
        pass


def worker(rank):
    try:
        torch.cuda.set_device(0)
        part = M.BoxPartition(cells, rank, grid, length=length, low_ghost_cells=int(os.environ.get("LOW_GHOST", "4")))
        ctx = M.Context()
        tr = M.HaloTransport(ctx, part, callbacks=mb.callbacks(rank))
        ctx.set_block_fgmres_on_ranks()
        h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", part.local_problem("linear", "cuda"), params)
        ctx.synchronize()
        ready.wait()
        if rank == timed_rank:
            n = h.level_size(0)
            ld = n + (n & 1)
            gen = torch.Generator(device="cuda").manual_seed(1)
            B = torch.rand(K, ld, dtype=torch.float64, device="cuda", generator=gen)
            X = torch.zeros(K, ld, dtype=torch.float64, device="cuda")
            print(json.dumps({"rank": rank, "cells_per_rank": per, "local_cells": list(part.local_cells), "n_local_dofs": n,
                              "block_info": h.block_info(), "block_info_f32": h.block_info_f32() if with_float else None,
                              "low_ghost_cells": part.low_ghost_cells, "iterations": iters}), flush=True)
            zero = [0.0] * K
            for d_us in delays:
                tr.reflect(d_us)
                for preconditioner in ("double", "float") if with_float else ("double",):
                    def loop():
                        X.zero_()
                        for c in range(K):
                            quiet(lambda: h.solve_fgmres(B[c, :n], X[c, :n], 0.0, iters, restart=iters, preconditioner=preconditioner))

                    def block():
                        X.zero_()
                        quiet(lambda: h.solve_fgmres_block(B, X, zero, iters, restart=iters, preconditioner=preconditioner))
                    e0 = tr.n_exchanges()
                    loop()
                    e1 = tr.n_exchanges()
                    block()
                    e2 = tr.n_exchanges()
                    extra = {"delay_us_per_group": d_us, "preconditioner": preconditioner, "iterations": iters,
                             "exchanges": {"loop": e1 - e0, "block": e2 - e1},
                             "allreduces": {"loop": K * (3 * iters + 1), "block": h.last_block_solve[2]["allreduces"]}}
                    compare(ctx, "FGMRES", extra, {"loop": loop, "block": block})
        ready.wait()
        del h
    except BaseException as e:  # noqa: BLE001
        errors[rank] = e
        mb.barrier.abort(); ready.abort()
        for p in range(n_ranks):
            mb.q[(rank, p)].put(np.zeros(0))


threads = [threading.Thread(target=worker, args=(r,)) for r in range(n_ranks)]
for t in threads:
    t.start()
for t in threads:
    t.join()
first = next((e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError)), None) or \
    next((e for e in errors if e is not None), None)
if first is not None:
    raise first
