# usage: amge_lanczos_time.py [cells=64] [solvers=lanczos,device] [agglomerates=4,3]
# Wall time of "Setup: build restrictor" (timer_report) per restrictor.eigensolver value, DESIGN.md 6: linear material, 2
# eigenvectors, matrix-free evaluator, median of three builds after none (every build is a fresh hierarchy).
#   agglomerate 4: (4,4,4) cells = 125 nodes: `device` means the dense Jacobi method on the host cores there (the path of every
#                  build before the Lanczos solver), `lanczos` the batched kernel of amge_lanczos.hip
#   agglomerate 3: (3,3,3) cells = 64 nodes: `device` is the dense kernel of amge_device.hip, for information
# A solver name the library does not know (a build from before the Lanczos solver asked for `lanczos`) is reported, not fatal.
import json, os, re, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M

cells = int(sys.argv[1]) if len(sys.argv) > 1 else 64
solvers = (sys.argv[2] if len(sys.argv) > 2 else 'lanczos,device').split(',')
aggs = [int(v) for v in (sys.argv[3] if len(sys.argv) > 3 else '4,3').split(',')]


def params(solver, a):
    return {"eigensolver": {"number of eigenvectors": 2, "tolerance": 1e-14},
            "agglomeration": {"partitioner": "block", "nx": a, "ny": a, "nz": a}, "restrictor": {"eigensolver": solver},
            "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0},
            "solver": {"type": "amg", "amg": {"smoother_degree": 1, "smoothing_range": 4.0, "n_cycles": 1, "aggregate_block": 2}},
            "is preconditioner": True, "max levels": 2}


def section_seconds(report, name):
    m = re.search(re.escape(name) + r"\s*\|\s*\d+\s*\|\s*([0-9.]+)s", report)
    return float(m.group(1)) if m else None


ctx = M.Context()
prob = M.LaplaceProblem((cells,) * 3, 'linear', device='cuda')
for a in aggs:
    for solver in solvers:
        rows = []
        try:
            for _ in range(3):
                t0 = time.perf_counter()
                h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params(solver, a))
                ctx.synchronize()
                total = time.perf_counter() - t0
                report = h.timer_report()
                info = h.restrictor_eigensolver_info() if hasattr(h, 'restrictor_eigensolver_info') else {}
                rows.append((section_seconds(report, "Setup: build restrictor"), total, info))
                del h
        except M.lib.MfmgError as e:
            print(json.dumps({"cells": cells, "agglomerate": a, "solver": solver, "error": str(e)[:200]}), flush=True)
            continue
        print(json.dumps({"cells": cells, "agglomerate": a, "solver": solver,
                          "build_restrictor_s": [r[0] for r in rows], "build_restrictor_median_s": statistics.median(r[0] for r in rows),
                          "hierarchy_s": [round(r[1], 3) for r in rows], "info": rows[-1][2]}), flush=True)
if '--report' in sys.argv:
    print(report)
