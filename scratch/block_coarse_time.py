# usage: block_coarse_time.py kernels [cells=256] [trips=7] [reps=20] [material=linear]
#        block_coarse_time.py coarse  [cells=256] [trips=7] [reps=10] [material=linear]
#        block_coarse_time.py cycle   [cells=256] [trips=1] [reps=10] [material=linear]
#        block_coarse_time.py against PARENT_LIBRARY [cells=256] [rounds=7] [material=linear]
# The coarse cycle on blocks of right-hand sides, `material linear` at (cells + 1)^3 DoFs.
#   kernels  (a) per column at k = 4 and k = 2: SparseMatrixDevice.launch_block of the first coarse operator A_c in the modes
#            `next` and `residual` against k calls of launch; one process, after warm-up, HIP events around `reps` calls, the
#            two variants alternating, `trips` repetitions
#   coarse   (b) Hierarchy.coarse_apply_block against k calls of coarse_apply, in the same way
#   cycle    apply_block and solve_cg_block (tolerance 1e-8 ||b||) per column at k = 4 with the library in use
#            (MFMG_HIP_LIBRARY names another build): one JSON line per quantity and trip
#   against  (c) `cycle` in child processes, this library and PARENT_LIBRARY (the library of the commit before, built into a
#            second directory) alternating, `rounds` times each: medians, ranges and ratios per quantity.  The reference is the
#            parent, never the code under test.
# One JSON line per comparison: the figures per column of every trip, medians, ranges, ratios of the medians.  Reads nothing
# outside the repository but PARENT_LIBRARY.
import json, os, subprocess, sys, time

part = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
med = lambda r: sorted(r)[len(r) // 2]
MAX_IT = 100

if part == 'against':
    parent = os.path.abspath(sys.argv[2])
    cells = sys.argv[3] if len(sys.argv) > 3 else '256'
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    material = sys.argv[5] if len(sys.argv) > 5 else 'linear'
    runs = {}
    for _ in range(rounds):
        for name, library in (('this commit', None), ('commit before', parent)):   # the libraries alternate
            env = dict(os.environ)
            env.pop('MFMG_HIP_LIBRARY', None)
            if library:
                env['MFMG_HIP_LIBRARY'] = library
            out = subprocess.run([sys.executable, os.path.abspath(__file__), 'cycle', cells, '1', '10', material], env=env, capture_output=True,
                                 text=True, timeout=600)
            if out.returncode != 0:
                sys.exit(f'{name}: the child failed with status {out.returncode}\n{out.stdout[-2000:]}{out.stderr[-2000:]}')
            for line in out.stdout.splitlines():
                rec = json.loads(line)
                if 'quantity' in rec:
                    runs.setdefault(rec['quantity'], {}).setdefault(name, []).extend(rec['per_column'])
                    runs[rec['quantity']].setdefault('unit', rec['unit'])
    for quantity, r in runs.items():
        unit = r.pop('unit')
        m = {name: med(v) for name, v in r.items()}
        print(json.dumps({'comparison': quantity, 'material': material, 'unit': unit, 'rounds': rounds,
                          'per_column': {k: [round(t, 3) for t in v] for k, v in r.items()},
                          'median': {k: round(v, 3) for k, v in m.items()}, 'range': {k: [round(min(v), 3), round(max(v), 3)] for k, v in r.items()},
                          'ratio': round(m['this commit'] / m['commit before'], 4),
                          'ranges_apart': max(r['this commit']) < min(r['commit before']) or max(r['commit before']) < min(r['this commit'])}), flush=True)
    sys.exit(0)

import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M
from mfmg_amd import lib as L

cells = int(sys.argv[2]) if len(sys.argv) > 2 else 256
trips = int(sys.argv[3]) if len(sys.argv) > 3 else (1 if part == 'cycle' else 7)
reps = int(sys.argv[4]) if len(sys.argv) > 4 else (20 if part == 'kernels' else 10)
material = sys.argv[5] if len(sys.argv) > 5 else 'linear'
library = os.environ.get('MFMG_HIP_LIBRARY', 'this commit')
ctx = M.Context()
prob = M.LaplaceProblem((cells,) * 3, material, device='cuda')
n = prob.n_dofs
params = {'eigensolver': {'number of eigenvectors': 2}, 'agglomeration': {'partitioner': 'block', 'nx': 2, 'ny': 2, 'nz': 2},
          'smoother': {'type': 'Chebyshev', 'degree': 3, 'smoothing_range': 20.0, 'n_smoothing_steps': 1},
          'solver': {'type': 'amg', 'amg': {'smoother_degree': 1, 'smoothing_range': 4.0, 'n_cycles': 1, 'aggregate_block': 2}},
          'is preconditioner': True, 'max levels': 2, 'release setup matrices': True}
h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params)
n_c = h.level_size(1)
gen = torch.Generator(device='cuda').manual_seed(1)


def rand(k, m):
    t = torch.zeros(k, m + (m & 1), dtype=torch.float64, device='cuda')
    t[:, :m] = torch.rand(k, m, dtype=torch.float64, device='cuda', generator=gen)
    return t


def timed(fn):
    """microseconds per call of fn, over `reps` calls between two events"""
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / reps


def compare(what, k, variants, info):
    for fn in variants.values():
        fn()
    runs = {name: [] for name in variants}
    for _ in range(trips):
        for name, fn in variants.items():             # the variants alternate
            runs[name].append(timed(fn) / k)
    m = {name: med(r) for name, r in runs.items()}
    print(json.dumps({'comparison': what, 'material': material, 'vectors': k, 'reps': reps, 'trips': trips, 'info': info(),
                      'us_per_column': {v: [round(t, 2) for t in r] for v, r in runs.items()},
                      'median_us_per_column': {v: round(t, 2) for v, t in m.items()},
                      'range': {v: [round(min(r), 2), round(max(r), 2)] for v, r in runs.items()},
                      'ratio_to_loop': round(m['block'] / m['loop'], 4),
                      'ranges_apart': max(runs['block']) < min(runs['loop']) or max(runs['loop']) < min(runs['block'])}), flush=True)


if part == 'kernels':
    A = h.coarse_operator()
    f = A.form()
    print(json.dumps({'n_dofs': n, 'n_coarse': n_c, 'nnz': A.nnz, 'kind': f['kind'], 'regular': f['regular'], 'stored_kernel': f['stored_kernel'],
                      'stored_d': f['stored_d'], 'c': f['c'], 'float_planes': f['float_planes'], 'block_info': A.block_info()}), flush=True)
    dinv = torch.rand(n_c, dtype=torch.float64, device='cuda', generator=gen)
    for k in (4, 2):
        X, B, P, O = rand(k, n_c), rand(k, n_c), rand(k, n_c), rand(k, n_c)
        for name, mode, kw in (('next', L.CSR_NEXT, dict(alpha=0.3, beta=0.5)), ('residual', L.CSR_RESIDUAL, {})):
            nxt = mode == L.CSR_NEXT
            variants = {'loop': lambda: [A.launch(mode, X[c, :n_c], O[c, :n_c], b=B[c, :n_c], dinv=dinv if nxt else None,
                                                  x_prev=P[c, :n_c] if nxt else None, **kw) for c in range(k)],
                        'block': lambda: A.launch_block(mode, X[:, :n_c], O[:, :n_c], B=B[:, :n_c], dinv=dinv if nxt else None,
                                                        X_prev=P[:, :n_c] if nxt else None, **kw)}
            compare(f'A_c mode {name}', k, variants, A.block_info)
elif part == 'coarse':
    print(json.dumps({'n_dofs': n, 'n_coarse': n_c, 'coarse_block_info': h.coarse_block_info()}), flush=True)
    for k in (4, 2):
        B, X = rand(k, n_c), rand(k, n_c)
        variants = {'loop': lambda: [h.coarse_apply(B[c, :n_c], X[c, :n_c]) for c in range(k)],
                    'block': lambda: h.coarse_apply_block(B[:, :n_c], X[:, :n_c])}
        compare('coarse_apply', k, variants, h.coarse_block_info)
else:
    k = 4
    B, X = rand(k, n), rand(k, n)
    h.apply_block(B, X)
    us = [timed(lambda: h.apply_block(B, X)) / k for _ in range(trips)]
    print(json.dumps({'quantity': f'apply_block k = {k}', 'unit': 'us per column', 'library': library, 'per_column': us}), flush=True)
    tol = [1e-8 * float(torch.linalg.norm(B[c, :n]).item()) for c in range(k)]

    def solve():
        X.zero_()
        ctx.synchronize()
        t0 = time.perf_counter()
        its, _, _ = h.solve_cg_block(B, X, tol, MAX_IT)
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k, its

    solve()
    ms, its = zip(*[solve() for _ in range(trips)])
    print(json.dumps({'quantity': f'solve_cg_block k = {k}', 'unit': 'ms per column', 'library': library, 'iterations': [int(i) for i in its[0]],
                      'per_column': list(ms)}), flush=True)
