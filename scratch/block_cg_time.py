# usage: block_cg_time.py [cells=256] [material=linear] [widths=4,8] [reps=7]
# Hierarchy.solve_cg_block against k calls of Hierarchy.solve_cg at (cells + 1)^3 DoFs, one process, after a warm-up solve of each
# kind.  Every column has its own random right-hand side, a zero initial guess and the tolerance 1e-8 ||b||.  The two
# variants alternate and are repeated `reps` times; a solve is timed on the host between two synchronisations (it synchronises
# once per iteration by itself).  solve_cg is the yardstick: this driver and the kernels under it are those of the commit before
# the block driver.  One JSON line per width: milliseconds per column of every repetition, medians, ranges, the ratio of the
# medians, the iteration counts and the work counters; then, from one profiled block solve, the three block kernels' time per
# column and iteration and their rate on the bytes they must move (dots 16 B, direction 24 B, update 48 B per entry; the profiler
# puts the two stages of a reduction under one name).
import json, os, sys, time
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M

cells = int(sys.argv[1]) if len(sys.argv) > 1 else 256
material = sys.argv[2] if len(sys.argv) > 2 else 'linear'
widths = [int(w) for w in (sys.argv[3] if len(sys.argv) > 3 else '4,8').split(',')]
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
ctx = M.Context()
prob = M.LaplaceProblem((cells,) * 3, material, device='cuda')
n = prob.n_dofs
ld = n + (n & 1)
params = {'eigensolver': {'number of eigenvectors': 2}, 'agglomeration': {'partitioner': 'block', 'nx': 2, 'ny': 2, 'nz': 2},
          'smoother': {'type': 'Chebyshev', 'degree': 3, 'smoothing_range': 20.0, 'n_smoothing_steps': 1},
          'solver': {'type': 'amg', 'amg': {'smoother_degree': 1, 'smoothing_range': 4.0, 'n_cycles': 1, 'aggregate_block': 2}},
          'is preconditioner': True, 'max levels': 2, 'release setup matrices': True}
h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params)
print(json.dumps({'n_dofs': n, 'material': material, 'block_info': h.block_info()}), flush=True)
gen = torch.Generator(device='cuda').manual_seed(1)
MAX_IT = 200


def wall(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


med = lambda r: sorted(r)[len(r) // 2]
for k in widths:
    B = torch.zeros(k, ld, dtype=torch.float64, device='cuda')
    B[:, :n] = torch.rand(k, n, dtype=torch.float64, device='cuda', generator=gen)
    X = torch.zeros_like(B)
    tol = [1e-8 * float(torch.linalg.norm(B[c, :n]).item()) for c in range(k)]

    def loop():
        X.zero_()
        return [h.solve_cg(B[c, :n], X[c, :n], tol[c], MAX_IT)[0] for c in range(k)]

    def block():
        X.zero_()
        its, _, work = h.solve_cg_block(B, X, tol, MAX_IT)
        return its, work

    its_loop, (its_block, work) = loop(), block()             # warm-up (workspaces, tile tables)
    assert its_loop == its_block, (its_loop, its_block)
    runs = {'loop': [], 'block': []}
    for _ in range(reps):                                     # the variants alternate
        runs['loop'].append(wall(loop)[0] / k)
        runs['block'].append(wall(block)[0] / k)
    print(json.dumps({'comparison': 'solve_cg_block against k solve_cg', 'vectors': k, 'reps': reps, 'iterations': its_block, 'work': work,
                      'ms_per_column': {v: [round(t, 3) for t in r] for v, r in runs.items()},
                      'median_ms_per_column': {v: round(med(r), 3) for v, r in runs.items()},
                      'range_ms_per_column': {v: [round(min(r), 3), round(max(r), 3)] for v, r in runs.items()},
                      'ratio_block_to_loop': round(med(runs['block']) / med(runs['loop']), 4)}), flush=True)
    # the three block kernels in one profiled solve
    names = {'block_dots': 16.0, 'block_cg_direction': 24.0, 'block_cg_update': 48.0}
    ctx.profile_enable(True, ','.join(names))
    its, work = block()
    out = {}
    for name, per_entry in names.items():
        launches, ms, by = ctx.profile_query(name)
        out[name] = {'launches': launches, 'us_per_column_and_launch': round(1e3 * ms / max(work['operator_columns'], 1) / (2 if name == 'block_dots' else 1), 2),
                     'GB_per_s': round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
    ctx.profile_enable(False)
    print(json.dumps({'kernels': out, 'vectors': k, 'column_iterations': work['operator_columns'],
                      'note': 'block_dots: the initial (r, r) of all columns is among its launches'}), flush=True)
    del B, X
