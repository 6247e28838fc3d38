# usage: block_fp32_time.py [part=kernels|tiles|solve] [cells=256] [material=linear] [widths=2,4,8] [trips=7] [reps=20]
# The FP32 fine level on blocks of float vectors at (cells + 1)^3 DoFs, one process, after warm-up.
#   kernels  per width k: a `next` smoother term, the residual and the FP32 cycle -- k calls of the one-vector entry point against
#            one block call, HIP events around `reps` calls, the two variants alternating, `trips` repetitions
#   tiles    the `next` term on four and on two vectors for a list of block tiles (how the default list of choose_block_tile
#            was chosen), the same timing
#   solve    solve_fgmres_block with the float preconditioner (V(0,1) coarse cycle, restart 15, tolerance 1e-8 ||b||), `trips`
#            solves per width timed on the host between two synchronisations.  Run it once with this library and once with
#            MFMG_HIP_LIBRARY naming the library of the commit before, in the same job: the driver is the same, the preconditioner
#            step is the column loop there and the block cycle here
# One JSON line per comparison: the figures per column of every trip, medians, ranges, ratios of the medians.
import json, os, sys, time
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M

part = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
cells = int(sys.argv[2]) if len(sys.argv) > 2 else 256
material = sys.argv[3] if len(sys.argv) > 3 else 'linear'
widths = [int(w) for w in (sys.argv[4] if len(sys.argv) > 4 else '2,4,8').split(',')]
trips = int(sys.argv[5]) if len(sys.argv) > 5 else 7
reps = int(sys.argv[6]) if len(sys.argv) > 6 else 20
ctx = M.Context()
prob = M.LaplaceProblem((cells,) * 3, material, device='cuda')
n = prob.n_dofs
ld = n + (n & 1)
gen = torch.Generator(device='cuda').manual_seed(1)
library = os.environ.get('MFMG_HIP_LIBRARY', 'this commit')
med = lambda r: sorted(r)[len(r) // 2]


def rand(k, dtype=torch.float32):
    t = torch.zeros(k, ld, dtype=dtype, device='cuda')
    t[:, :n] = torch.rand(k, n, dtype=dtype, device='cuda', generator=gen)
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


def compare(what, k, variants, **more):
    for fn in variants.values():                              # warm-up (tile tables, attributes, workspaces)
        fn()
    runs = {name: [] for name in variants}
    for _ in range(trips):
        for name, fn in variants.items():                     # the variants alternate
            runs[name].append(timed(fn) / k)
    m = {name: med(r) for name, r in runs.items()}
    first = next(iter(variants))
    print(json.dumps(dict({'comparison': what, 'n_dofs': n, 'material': material, 'vectors': k, 'reps': reps, 'trips': trips,
                           'us_per_column': {v: [round(t, 2) for t in r] for v, r in runs.items()},
                           'median_us_per_column': {v: round(t, 2) for v, t in m.items()},
                           'range_us_per_column': {v: [round(min(r), 2), round(max(r), 2)] for v, r in runs.items()},
                           'ratio_to_' + first: {v: round(t / m[first], 4) for v, t in m.items()}}, **more)), flush=True)


params = {'eigensolver': {'number of eigenvectors': 2}, 'agglomeration': {'partitioner': 'block', 'nx': 2, 'ny': 2, 'nz': 2},
          'smoother': {'type': 'Chebyshev', 'degree': 3, 'smoothing_range': 20.0, 'n_smoothing_steps': 1},
          'solver': {'type': 'amg', 'amg': {'smoother_degree': 1, 'smoothing_range': 4.0, 'n_cycles': 1, 'aggregate_block': 2,
                                            'pre_smoothing_levels': 0}},
          'is preconditioner': True, 'max levels': 2, 'release setup matrices': True, 'fine level precision': 'float'}
al, be = 0.23, 0.87

if part == 'tiles':
    op = M.MatrixFreeLaplaceF32(ctx, prob)
    assert op.block_available()
    tiles = [(0, 0, 0), (4, 2, 16), (4, 2, 8), (4, 2, 32), (8, 2, 8), (8, 2, 16), (6, 2, 16), (4, 3, 16), (4, 4, 16), (8, 3, 16), (8, 4, 16), (2, 2, 16)]
    for k in (4, 2):
        X, B, XP, OUT = (rand(k) for _ in range(4))
        variants = {}
        for t in tiles:
            def run(t=t):
                op.set_block_tile(*t)
                op.block_launch('next', X, OUT, B=B, X_prev=XP, alpha=al, beta=be)
            variants['x'.join(map(str, t))] = run
        op.set_block_tile(0, 0, 0)
        compare('next term by block tile', k, variants, default_tile=op.get_block_tile(k))
        op.set_block_tile(0, 0, 0)

if part == 'kernels':
    op = M.MatrixFreeLaplaceF32(ctx, prob)
    print(json.dumps({'block_available': op.block_available(), 'block_tile_4': op.get_block_tile(4), 'block_tile_2': op.get_block_tile(2),
                      'one_vector_tile': op.get_tile(), 'ids_computed': op.ids_computed()}), flush=True)
    for k in widths:
        X, B, XP, OUT = (rand(k) for _ in range(4))
        compare('next term', k, {
            'loop': lambda: [op.smoother_step(B[c, :n], X[c, :n], XP[c, :n], al, be, OUT[c, :n]) for c in range(k)],
            'block': lambda: op.block_launch('next', X, OUT, B=B, X_prev=XP, alpha=al, beta=be)})
        compare('residual', k, {
            'loop': lambda: [op.residual(X[c, :n], B[c, :n], OUT[c, :n]) for c in range(k)],
            'block': lambda: op.block_launch('residual', X, OUT, B=B)})
        del X, B, XP, OUT
    del op
    torch.cuda.empty_cache()
    h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params)
    for k in widths:
        B, X = rand(k), rand(k)
        compare('FP32 cycle', k, {'loop': lambda: [h.apply_f32(B[c, :n], X[c, :n]) for c in range(k)],
                                  'block': lambda: h.apply_f32_block(B, X)}, block_info_f32=h.block_info_f32())
        print(json.dumps({'vectors': k, 'block_info_f32_after': h.block_info_f32()}), flush=True)

if part == 'solve':
    h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params)
    MAX_IT = 200
    for k in widths:
        B = rand(k, torch.float64)
        X = torch.zeros_like(B)
        tol = [1e-8 * float(torch.linalg.norm(B[c, :n]).item()) for c in range(k)]

        def block():
            X.zero_()
            ctx.synchronize()
            t0 = time.perf_counter()
            its, _, work = h.solve_fgmres_block(B, X, tol, MAX_IT, restart=15, preconditioner='float')
            ctx.synchronize()
            return 1e3 * (time.perf_counter() - t0), its, work

        _, its, work = block()                                # warm-up (workspaces, tile tables)
        runs = [block()[0] / k for _ in range(trips)]
        info = h.block_info_f32() if hasattr(h._lib, 'mfmg_hip_hierarchy_block_info_f32') else None
        print(json.dumps({'comparison': 'solve_fgmres_block, float preconditioner', 'library': library, 'n_dofs': n, 'material': material,
                          'vectors': k, 'iterations': its, 'work': {w: v for w, v in work.items() if w != 'residuals'},
                          'block_info_f32': info, 'ms_per_column': [round(t, 3) for t in runs], 'median_ms_per_column': round(med(runs), 3),
                          'range_ms_per_column': [round(min(runs), 3), round(max(runs), 3)]}), flush=True)
        del B, X
        torch.cuda.empty_cache()
