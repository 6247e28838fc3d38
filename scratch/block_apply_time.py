# usage: block_apply_time.py [cells=256] [reps=20] [trips=5] [parts=abc]
# Blocks of right-hand sides against the per-column loop, `material linear` (eight coefficients per cell) at (cells + 1)^3 DoFs,
# one process, after warm-up, HIP events around every variant.  Each comparison alternates its variants and is
# repeated `trips` times, so that the spread of the repeated runs is visible beside the ratios:
#   (a) a `next` smoother term on four vectors: four one-vector launches | one block launch of 4 | two block launches of 2
#   (b) the residual mode, the same three variants
#   (c) Hierarchy.apply four times | apply_block of four (the width block_info reports)
# One JSON line per comparison: microseconds per vector of every trip, the median, the ratio to the loop (median / median) and the
# spread (max - min) / median of every variant over its trips.
import json, os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M

cells = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
trips = int(sys.argv[3]) if len(sys.argv) > 3 else 5
parts = sys.argv[4] if len(sys.argv) > 4 else 'abc'
K = 4
ctx = M.Context()
prob = M.LaplaceProblem((cells,) * 3, 'linear', device='cuda')
n = prob.n_dofs
ld = n + (n & 1)
gen = torch.Generator(device='cuda').manual_seed(1)
rand = lambda: torch.rand(K, ld, dtype=torch.float64, device='cuda', generator=gen)


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


def compare(what, variants):
    for fn in variants.values():                              # warm-up (tile tables, attributes, workspaces)
        fn()
    runs = {name: [] for name in variants}
    for _ in range(trips):
        for name, fn in variants.items():                     # the variants alternate
            runs[name].append(timed(fn) / K)
    med = {name: sorted(r)[len(r) // 2] for name, r in runs.items()}
    loop = med['loop']
    print(json.dumps({'comparison': what, 'n_dofs': n, 'vectors': K, 'reps': reps, 'trips': trips,
                      'us_per_vector': {k: [round(v, 2) for v in r] for k, r in runs.items()},
                      'median_us_per_vector': {k: round(v, 2) for k, v in med.items()},
                      'ratio_to_loop': {k: round(v / loop, 4) for k, v in med.items()},
                      'spread': {k: round((max(r) - min(r)) / med[k], 4) for k, r in runs.items()}}), flush=True)


if 'a' in parts or 'b' in parts:
    op = M.MatrixFreeLaplace(ctx, prob)
    assert op.block_available()
    X, B, XP, OUT = rand(), rand(), rand(), rand()
    print(json.dumps({'block_tile_4': op.get_block_tile(4), 'block_tile_2': op.get_block_tile(2), 'one_vector_tile': op.get_tile(),
                      'ids_computed': op.ids_computed()}), flush=True)
    al, be = 0.23, 0.87
    if 'a' in parts:
        compare('next term', {
            'loop': lambda: [op.smoother_step(B[c, :n], X[c, :n], XP[c, :n], al, be, OUT[c, :n]) for c in range(K)],
            'block4': lambda: op.block_launch('next', X, OUT, B=B, X_prev=XP, alpha=al, beta=be),
            'block2x2': lambda: [op.block_launch('next', X[c:c + 2], OUT[c:c + 2], B=B[c:c + 2], X_prev=XP[c:c + 2], alpha=al, beta=be) for c in (0, 2)]})
    if 'b' in parts:
        compare('residual', {
            'loop': lambda: [op.residual(X[c, :n], B[c, :n], OUT[c, :n]) for c in range(K)],
            'block4': lambda: op.block_launch('residual', X, OUT, B=B),
            'block2x2': lambda: [op.block_launch('residual', X[c:c + 2], OUT[c:c + 2], B=B[c:c + 2]) for c in (0, 2)]})
    del op, X, B, XP, OUT
    torch.cuda.empty_cache()

if 'c' in parts:
    params = {'eigensolver': {'number of eigenvectors': 2}, 'agglomeration': {'partitioner': 'block', 'nx': 2, 'ny': 2, 'nz': 2},
              'smoother': {'type': 'Chebyshev', 'degree': 3, 'smoothing_range': 20.0, 'n_smoothing_steps': 1},
              'solver': {'type': 'amg', 'amg': {'smoother_degree': 1, 'smoothing_range': 4.0, 'n_cycles': 1, 'aggregate_block': 2}},
              'is preconditioner': False, 'max levels': 2, 'release setup matrices': True}
    h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params)
    B, X = rand(), rand()
    print(json.dumps({'block_info': h.block_info()}), flush=True)
    compare('V-cycle', {'loop': lambda: [h.apply(B[c, :n], X[c, :n]) for c in range(K)], 'apply_block': lambda: h.apply_block(B, X)})
    print(json.dumps({'block_info_after': h.block_info()}), flush=True)
