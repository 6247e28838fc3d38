# usage: block_fgmres_time.py [cells=256] [material=linear] [widths=4,8] [reps=7] [restart=15]
# Hierarchy.solve_fgmres_block against k calls of Hierarchy.solve_fgmres at (cells + 1)^3 DoFs with the non-symmetric V(0,1) coarse
# cycle (solver.amg.pre_smoothing_levels 0), one process, after a warm-up solve of each kind.  Every column has its
# own random right-hand side, a zero initial guess and the tolerance 1e-8 ||b||.  Restart 15 keeps the bases of k = 8 near 33 GB
# at 257^3.  The two variants alternate and are repeated `reps` times; a solve is timed on the host between two synchronisations
# (it synchronises once per iteration by itself).  solve_fgmres is the yardstick: this driver and the kernels under it compute
# what they did before the block driver.  One JSON line per width: milliseconds per column of every repetition, medians, ranges,
# the ratio of the medians, the iteration counts and the work counters; then, from one profiled block solve and one profiled loop,
# the time of the basis kernels per column and iteration in either form.
import json, os, sys, time
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M

cells = int(sys.argv[1]) if len(sys.argv) > 1 else 256
material = sys.argv[2] if len(sys.argv) > 2 else 'linear'
widths = [int(w) for w in (sys.argv[3] if len(sys.argv) > 3 else '4,8').split(',')]
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
restart = int(sys.argv[5]) if len(sys.argv) > 5 else 15
ctx = M.Context()
prob = M.LaplaceProblem((cells,) * 3, material, device='cuda')
n = prob.n_dofs
ld = n + (n & 1)
params = {'eigensolver': {'number of eigenvectors': 2}, 'agglomeration': {'partitioner': 'block', 'nx': 2, 'ny': 2, 'nz': 2},
          'smoother': {'type': 'Chebyshev', 'degree': 3, 'smoothing_range': 20.0, 'n_smoothing_steps': 1},
          'solver': {'type': 'amg', 'amg': {'smoother_degree': 1, 'smoothing_range': 4.0, 'n_cycles': 1, 'aggregate_block': 2,
                                            'pre_smoothing_levels': 0}},
          'is preconditioner': True, 'max levels': 2, 'release setup matrices': True}
h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params)
print(json.dumps({'n_dofs': n, 'material': material, 'restart': restart, 'block_info': h.block_info()}), flush=True)
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
        return [h.solve_fgmres(B[c, :n], X[c, :n], tol[c], MAX_IT, restart=restart)[0] for c in range(k)]

    def block():
        X.zero_()
        its, _, work = h.solve_fgmres_block(B, X, tol, MAX_IT, restart=restart)
        return its, work

    its_loop, (its_block, work) = loop(), block()             # warm-up (workspaces, tile tables)
    assert its_loop == its_block, (its_loop, its_block)
    runs = {'loop': [], 'block': []}
    for _ in range(reps):                                     # the variants alternate
        runs['loop'].append(wall(loop)[0] / k)
        runs['block'].append(wall(block)[0] / k)
    work = {w: v for w, v in work.items() if w != 'residuals'}
    print(json.dumps({'comparison': 'solve_fgmres_block against k solve_fgmres', 'vectors': k, 'reps': reps, 'iterations': its_block,
                      'work': work, 'ms_per_column': {v: [round(t, 3) for t in r] for v, r in runs.items()},
                      'median_ms_per_column': {v: round(med(r), 3) for v, r in runs.items()},
                      'range_ms_per_column': {v: [round(min(r), 3), round(max(r), 3)] for v, r in runs.items()},
                      'ratio_block_to_loop': round(med(runs['block']) / med(runs['loop']), 4)}), flush=True)
    # the basis kernels of either form, one profiled solve each
    column_iterations = max(work['operator_columns'], 1)
    out = {}
    for prefix, fn in (('block_basis_', block), ('basis_', loop)):
        names = [prefix + s for s in ('dots', 'update', 'scale_store', 'combine')]
        ctx.profile_enable(True, ','.join(names))
        fn()
        for name in names:
            launches, ms, by = ctx.profile_query(name)
            out[name] = {'launches': launches, 'us_per_column_iteration': round(1e3 * ms / column_iterations, 2),
                         'GB_per_s': round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
        ctx.profile_enable(False)
    print(json.dumps({'kernels': out, 'vectors': k, 'column_iterations': column_iterations}), flush=True)
    del B, X
