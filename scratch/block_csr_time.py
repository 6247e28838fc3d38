# usage: block_csr_time.py kernels   [cells=128] [trips=7] [reps=20]
#        block_csr_time.py hierarchy [cells=256] [trips=7] [reps=10]
# The block forms of the CSR kernels (SparseMatrixDevice.set_block_csr, Hierarchy.set_block_csr), `material linear`, one process,
# after warm-up, HIP events around `reps` calls, the two variants alternating, `trips` repetitions, per column.
#   kernels    the assembled fine operator at (cells + 1)^3 DoFs forced onto the CSR kernels (set_kernel(0, 0); the LDS form
#              where the matrix has its lists): launch_block in the modes apply, residual and next at k = 4 and 2 against k
#              calls of launch, with the figure of the byte model beside the measured one:
#                  (M + D + k V) / (k (M + D + V)),  M = 12 nnz / rows + 4 bytes of matrix per row, V the bytes of the vectors
#                  of one column per row (x and out 16; b 8; x at the row and x_prev 16), D = 8 of the shared D^-1 where read
#   hierarchy  (a) every matrix of the aggregation hierarchy at (cells + 1)^3 DoFs that runs a CSR kernel: mode apply at k = 4,
#              launch_block against four calls of launch -- one line per matrix with its route, rows and entries;
#              (b) coarse_apply_block and apply_block at k = 4, the switch off against on (set_block_csr between the trips);
#              (c) solve_cg_block (tolerance 1e-8 ||b||) at k = 4 and 8, off against on.
# The comparison is always the other variant in the same session.  One JSON line per comparison: the figures per column of
# every trip, medians, ranges, the ratio of the medians and whether the ranges are apart.  Reads nothing outside the repository.
import ctypes as C
import json, os, sys, time

import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M
from mfmg_amd import lib as L
from mfmg_amd.api import SparseMatrixDevice, host_assemble_matrix

part = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
cells = int(sys.argv[2]) if len(sys.argv) > 2 else (128 if part == 'kernels' else 256)
trips = int(sys.argv[3]) if len(sys.argv) > 3 else 7
reps = int(sys.argv[4]) if len(sys.argv) > 4 else (20 if part == 'kernels' else 10)
material = 'linear'
med = lambda r: sorted(r)[len(r) // 2]
MAX_IT = 100
ctx = M.Context()
gen = torch.Generator(device='cuda').manual_seed(1)


def rand(k, m):
    t = torch.zeros(k, m + (m & 1), dtype=torch.float64, device='cuda')
    t[:, :m] = torch.rand(k, m, dtype=torch.float64, device='cuda', generator=gen)
    return t


def timed(fn, unit=1e3):
    """microseconds (unit 1e3) per call of fn, over `reps` calls between two events"""
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return unit * start.elapsed_time(stop) / reps


def compare(what, k, variants, extra=None, measure=timed, unit='us'):
    """variants: {name: (prepare, fn)}, the first the reference; they alternate, `prepare` runs before each timing of its variant"""
    runs = {name: [] for name in variants}
    for prepare, fn in variants.values():
        prepare()
        measure(fn)
    for _ in range(trips):
        for name, (prepare, fn) in variants.items():
            prepare()
            runs[name].append(measure(fn) / k)
    base, new = list(variants)
    m = {name: med(r) for name, r in runs.items()}
    print(json.dumps({'comparison': what, 'material': material, 'vectors': k, 'reps': reps, 'trips': trips, **(extra or {}),
                      f'{unit}_per_column': {v: [round(t, 2) for t in r] for v, r in runs.items()},
                      f'median_{unit}_per_column': {v: round(t, 2) for v, t in m.items()},
                      'range': {v: [round(min(r), 2), round(max(r), 2)] for v, r in runs.items()},
                      f'ratio_{new}_to_{base}': round(m[new] / m[base], 4),
                      'ranges_apart': max(runs[new]) < min(runs[base]) or max(runs[base]) < min(runs[new])}), flush=True)
    return m[new] / m[base], max(runs[base]) < min(runs[new])


nothing = lambda: None


def kernel_modes(A, label, ks=(4, 2), modes=('apply', 'residual', 'next')):
    m, n = A.shape
    per_row = 12.0 * A.nnz / m + 4.0
    dinv = torch.rand(m, dtype=torch.float64, device='cuda', generator=gen)
    table = {'apply': (L.CSR_APPLY, {}, 16.0, 0.0), 'residual': (L.CSR_RESIDUAL, {}, 24.0, 0.0),
             'next': (L.CSR_NEXT, dict(alpha=0.3, beta=0.5), 40.0, 8.0)}
    for k in ks:
        X, B, P, O = rand(k, n), rand(k, m), rand(k, m), rand(k, m)
        for name in modes:
            mode, kw, V, D = table[name]
            if name != 'apply' and m != n:
                continue
            need_b, nxt = name != 'apply', name == 'next'
            loop = lambda: [A.launch(mode, X[c, :n], O[c, :m], b=B[c, :m] if need_b else None, dinv=dinv if nxt else None,
                                     x_prev=P[c, :m] if nxt else None, **kw) for c in range(k)]
            block = lambda: A.launch_block(mode, X[:, :n], O[:, :m], B=B[:, :m] if need_b else None, dinv=dinv if nxt else None,
                                           X_prev=P[:, :m] if nxt else None, **kw)
            model = (per_row + D + k * V) / (k * (per_row + D + V))
            compare(f'{label} mode {name}', k, {'loop': (nothing, loop), 'block': (nothing, block)},
                    extra={'byte_model': round(model, 3), 'matrix_bytes_per_row': round(per_row, 1), 'block_info': A.block_info()})


if part == 'kernels':
    A_host = host_assemble_matrix(M.LaplaceProblem((cells,) * 3, material))
    A = SparseMatrixDevice(ctx, A_host)
    print(json.dumps({'rows': A.shape[0], 'nnz': A.nnz, 'form_as_built': A.form()}), flush=True)
    for use_lds, want in ((0, 'lanes'), (1, 'lds')):
        A.set_kernel(0, use_lds)
        f = A.form()
        if f['csr_kernel'] != want:
            print(json.dumps({'skipped': want, 'reason': 'the matrix has no lists for this form', 'form': f}), flush=True)
            continue
        info = A.set_block_csr(True)
        print(json.dumps({'csr_kernel': f['csr_kernel'], 'lanes': f['lanes'], 'set_block_csr': info}), flush=True)
        kernel_modes(A, f"fine operator, {f['csr_kernel']}{f['lanes']}")
        A.set_block_csr(False)
    sys.exit(0)

prob = M.LaplaceProblem((cells,) * 3, material, device='cuda')
n = prob.n_dofs
params = {'eigensolver': {'number of eigenvectors': 2}, 'agglomeration': {'partitioner': 'block', 'nx': 2, 'ny': 2, 'nz': 2},
          'smoother': {'type': 'Chebyshev', 'degree': 3, 'smoothing_range': 20.0, 'n_smoothing_steps': 1},
          'solver': {'type': 'amg', 'amg': {'smoother_degree': 1, 'smoothing_range': 4.0, 'n_cycles': 1, 'aggregate_block': 2}},
          'is preconditioner': True, 'max levels': 2, 'release setup matrices': True}
h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params)
n_c = h.level_size(1)

# (a) the matrices of the aggregation hierarchy on CSR kernels, one by one
n_levels = C.c_int32()
L.check(h._lib.mfmg_hip_hierarchy_coarse_amg_levels(h.handle, C.byref(n_levels)))
smoothed = [i['smoothed'] for i in h.coarse_amg_setup_info()]
slower = []
for l in range(n_levels.value):
    for which, name in ((0, 'A'), (1, 'P'), (2, 'P^T'), (3, 'P~')):
        if (which in (1, 2) and l + 1 == n_levels.value) or (which == 3 and not smoothed[l]):
            continue
        p = C.c_void_p()
        L.check(h._lib.mfmg_hip_hierarchy_coarse_amg_get(h.handle, l, which, C.byref(p)))
        A = SparseMatrixDevice(ctx, _handle=p, _borrowed=True, _keepalive=h)
        f = A.form()
        line = {'level': l, 'matrix': name, 'rows': A.shape[0], 'cols': A.shape[1], 'kind': f['kind'], 'csr_kernel': f['csr_kernel'],
                'lanes': f['lanes'], 'csr_released': f['csr_released'], 'width': A.block_info()['width']}
        if f['kind'] not in (0, 1):
            print(json.dumps({**line, 'skipped': 'not on a CSR kernel'}), flush=True)
            continue
        line['nnz'] = A.nnz
        info = A.set_block_csr(True)
        print(json.dumps({**line, 'set_block_csr': info}), flush=True)
        if info['width'] == 4:
            m_, n_ = A.shape
            X, O = rand(4, n_), rand(4, m_)
            ratio, worse = compare(f"level {l} {name} ({m_} x {n_}, {f['csr_kernel']}{f['lanes']}, route4 {info['route4']}) mode apply", 4,
                                   {'loop': (nothing, lambda: [A.launch(L.CSR_APPLY, X[c, :n_], O[c, :m_]) for c in range(4)]),
                                    'block': (nothing, lambda: A.launch_block(L.CSR_APPLY, X[:, :n_], O[:, :m_]))})
            if worse:
                slower.append((l, name, info['route4'], f['lanes'], ratio))
        A.set_block_csr(False)
print(json.dumps({'routes_slower_than_the_loop_with_ranges_apart': slower}), flush=True)

# (b) the coarse cycle and the whole cycle, the switch off against on
off, on = (lambda: h.set_block_csr(False)), (lambda: h.set_block_csr(True))
print(json.dumps({'n_dofs': n, 'n_coarse': n_c, 'matrices_flipped': h.set_block_csr(True), 'coarse_block_info': h.coarse_block_info()}), flush=True)
k = 4
Bc, Xc = rand(k, n_c), rand(k, n_c)
for name, prepare in (('off', off), ('on', on)):
    prepare()
    h.coarse_apply_block(Bc[:, :n_c], Xc[:, :n_c])
    print(json.dumps({'coarse_apply_block k = 4, switch': name, 'coarse_block_info': h.coarse_block_info()}), flush=True)
compare('coarse_apply_block', k, {'off': (off, lambda: h.coarse_apply_block(Bc[:, :n_c], Xc[:, :n_c])),
                                  'on': (on, lambda: h.coarse_apply_block(Bc[:, :n_c], Xc[:, :n_c]))})
B, X = rand(k, n), rand(k, n)
compare('apply_block', k, {'off': (off, lambda: h.apply_block(B[:, :n], X[:, :n])), 'on': (on, lambda: h.apply_block(B[:, :n], X[:, :n]))})

# (c) block CG
for k in (4, 8):
    B, X = rand(k, n), rand(k, n)
    tol = [1e-8 * float(torch.linalg.norm(B[c, :n]).item()) for c in range(k)]
    iterations = {}

    def solve(fn_unused=None):
        X.zero_()
        ctx.synchronize()
        t0 = time.perf_counter()
        its, _, _ = h.solve_cg_block(B[:, :n], X[:, :n], tol, MAX_IT)
        ctx.synchronize()
        iterations['last'] = [int(i) for i in its]
        return 1e3 * (time.perf_counter() - t0)

    compare('solve_cg_block', k, {'off': (off, nothing), 'on': (on, nothing)}, measure=solve, unit='ms', extra={'tolerance': '1e-8 ||b||'})
    print(json.dumps({'solve_cg_block iterations': iterations['last'], 'vectors': k}), flush=True)
h.set_block_csr(False)
