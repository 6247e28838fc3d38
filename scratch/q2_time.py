# usage: q2_time.py [cells=128] [reps=10] [trips=7] [materials=linear,constant] [parts=os]
# The Q2 operator and the solver on the refined Q1 cycle at `cells`^3 Q2 cells ((2 cells + 1)^3 unknowns), one process, after
# warm-up, HIP events around every variant.  Per material, `trips` alternating repetitions, ranges reported:
#   (o) vmult and a `next` smoother term of the Q2 operator on every tile shape on offer, beside the Q1 operator on the same
#       lattice (linear: eight coefficients per cell; constant: the one-coefficient kernel), with the bytes each launch must move
#   (s) HighOrderSolver.apply, solve_cg to 1e-8 ||b|| with its iteration count (Chebyshev(2) and without smoothing)
# One JSON line per comparison: microseconds of every trip, minimum and maximum.
import json, os, sys, time
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M

cells = int(sys.argv[1]) if len(sys.argv) > 1 else 128
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
trips = int(sys.argv[3]) if len(sys.argv) > 3 else 7
materials = (sys.argv[4] if len(sys.argv) > 4 else 'linear,constant').split(',')
parts = sys.argv[5] if len(sys.argv) > 5 else 'os'
ctx = M.Context()
gen = torch.Generator(device='cuda').manual_seed(1)


def timed(fn, count=reps):
    """microseconds per call of fn, over `count` calls between two events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.synchronize()
    start.record()
    for _ in range(count):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / count


def compare(what, variants, extra=None, count=reps):
    for fn in variants.values():
        fn()
    runs = {name: [] for name in variants}
    for _ in range(trips):
        for name, fn in variants.items():                     # the variants alternate
            runs[name].append(timed(fn, count))
    line = {'comparison': what, 'cells': cells, 'reps': count, 'trips': trips,
            'us': {k: [round(v, 1) for v in r] for k, r in runs.items()},
            'range_us': {k: [round(min(r), 1), round(max(r), 1)] for k, r in runs.items()}}
    line.update(extra or {})
    print(json.dumps(line), flush=True)


for material in materials:
    p2 = M.LaplaceProblemQ2((cells,) * 3, material, device='cuda')
    n = p2.n_dofs
    rand = lambda: torch.rand(n, dtype=torch.float64, device='cuda', generator=gen)
    if 'o' in parts:
        q2 = M.MatrixFreeLaplaceQ2(ctx, p2)
        q1 = M.MatrixFreeLaplace(ctx, p2.refined_q1())
        x, b, xp, out = rand(), rand(), rand(), rand()
        per_cell = 1 if q2.cell_constant_layout() else 27
        bytes_q2 = n * (2 * 8 + 1) + p2.n_cells_total * per_cell * 8
        variants_v, variants_n = {}, {}
        for tile in M.q2_tile_shapes():
            def vm(tile=tile):
                q2.set_tile(*tile)
                q2.vmult(out, x)
            def nx(tile=tile):
                q2.set_tile(*tile)
                q2.smoother_step(b, x, xp, 0.23, 0.87, out)
            variants_v['q2 %dx%dx%d' % tile] = vm
            variants_n['q2 %dx%dx%d' % tile] = nx
        variants_v['q1'] = lambda: q1.vmult(out, x)
        variants_n['q1'] = lambda: q1.smoother_step(b, x, xp, 0.23, 0.87, out)
        info = {'material': material, 'n_dofs': n, 'q2_cell_constant': q2.cell_constant_layout(),
                'q1_cell_constant': q1.cell_constant_layout(), 'q2_bytes_vmult': bytes_q2, 'q2_bytes_next': bytes_q2 + 3 * 8 * n}
        compare('vmult', variants_v, info)
        compare('next term', variants_n, info)
        q2.set_tile(0, 0, 0)
        del q2, q1, x, b, xp, out
        torch.cuda.empty_cache()
    if 's' in parts:
        q1_params = {'eigensolver': {'number of eigenvectors': 2}, 'agglomeration': {'partitioner': 'block', 'nx': 2, 'ny': 2, 'nz': 2},
                     'smoother': {'type': 'Chebyshev', 'degree': 3, 'smoothing_range': 20.0},
                     'solver': {'type': 'amg', 'amg': {'smoother_degree': 1, 'smoothing_range': 4.0, 'n_cycles': 1, 'aggregate_block': 2}},
                     'is preconditioner': True, 'max levels': 2, 'release setup matrices': True}
        for degree in (2, 0):
            t0 = time.time()
            s = M.HighOrderSolver(ctx, p2, dict(q1_params, **{'high order': {'smoother': {'degree': degree}}}))
            ctx.synchronize()
            setup_s = time.time() - t0
            b = rand() * (p2.constrained != 1)
            x = torch.zeros(n, dtype=torch.float64, device='cuda')
            tol = 1e-8 * float(b.norm())
            its = []

            def solve():
                x.zero_()
                its.append(s.solve_cg(b, x, tolerance=tol, max_iterations=200)[0])
            info = {'material': material, 'n_dofs': n, 'smoother_degree': degree, 'smoother_info': s.smoother_info(),
                    'setup_seconds': round(setup_s, 2)}
            compare('apply', {'apply': lambda: s.apply(b, x)}, info)
            compare('solve_cg', {'solve_cg': solve}, info, count=1)
            print(json.dumps({'material': material, 'smoother_degree': degree, 'cg_iterations': sorted(set(its))}), flush=True)
            del s, b, x
            torch.cuda.empty_cache()
