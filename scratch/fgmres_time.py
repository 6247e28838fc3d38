# usage: fgmres_time.py [cells=256] [legs=cg,fgmres,fgmres_f32,kernels]
# The Krylov drivers at size, one session on one box: constant material, Chebyshev(3), the bench's coarse solver,
# reduction 1e-8 from x = 0, median of three solves after a warm-up solve.
#   cg          solve_cg preconditioned by the symmetric V(1,1) cycle (bench.py's cg_solve leg)
#   fgmres      solve_fgmres preconditioned by the V(0,1) cycle (solver.amg.pre_smoothing_levels 0)
#   fgmres_f32  ... with the FP32 fine level as preconditioner ("fine level precision" float)
#   kernels     the four basis kernels inside one fgmres solve (HIP events per launch, a solve of its own): time per
#               iteration, their share of the solve, and the byte rate against the budget of krylov_basis.hpp
# For the per-kernel view from outside: rocprofv3 --kernel-trace --stats -- python scratch/fgmres_time.py 256 fgmres
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M

cells = int(sys.argv[1]) if len(sys.argv) > 1 else 256
legs = (sys.argv[2] if len(sys.argv) > 2 else 'cg,fgmres,fgmres_f32,kernels').split(',')
n = (cells,) * 3
COPY_TBS = 6.3   # float4 copy rate DESIGN.md 6 quotes
BASIS = ('basis_dots', 'basis_update', 'basis_scale_store', 'basis_combine')


def params(v01, fp32=False):
    p = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"partitioner": "block", "nx": 2, "ny": 2, "nz": 2},
         "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0, "n_smoothing_steps": 1},
         "solver": {"type": "amg", "amg": {"smoother_degree": 1, "smoothing_range": 4.0, "n_cycles": 1, "aggregate_block": 2}},
         "is preconditioner": True, "max levels": 2}
    if v01:
        p["solver"]["amg"]["pre_smoothing_levels"] = 0
    if fp32:
        p["fine level precision"] = "float"
    return p


def out(**kw):
    print(json.dumps(kw), flush=True)


ctx = M.Context()
prob = M.LaplaceProblem(n, 'constant', device='cuda')
free = (prob.constrained != 1).to(torch.float64)
x_true = torch.rand(prob.n_dofs, dtype=torch.float64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3)) * free


def solve_ms(leg):
    h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params(v01=leg != 'cg', fp32=leg == 'fgmres_f32'))
    b = torch.empty_like(x_true)
    h.operator_apply(0, x_true, b)
    b *= free
    r0 = ctx.l2_norm(b)

    def solve(x):
        if leg == 'cg':
            return h.solve_cg(b, x, tolerance=1e-8 * r0, max_iterations=200)
        return h.solve_fgmres(b, x, tolerance=1e-8 * r0, max_iterations=200, restart=30,
                              preconditioner='float' if leg == 'fgmres_f32' else 'double')
    runs = []
    for attempt in range(4):
        x = torch.zeros_like(b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        its, hist = solve(x)
        torch.cuda.synchronize()
        if attempt > 0:
            runs.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(runs)[len(runs) // 2]
    h.operator_apply(0, x, r := torch.empty_like(b))
    out(leg=leg, iterations=int(its), ms_total=ms, ms_per_iteration=ms / max(int(its), 1), runs=runs,
        true_reduction=float((r - b).norm() / r0), max_rel_error=float((x - x_true).abs().max() / x_true.abs().max()))
    return h, b, r0, ms, int(its)


for leg in ('cg', 'fgmres', 'fgmres_f32'):
    if leg not in legs:
        continue
    h, b, r0, ms, its = solve_ms(leg)
    if leg == 'fgmres' and 'kernels' in legs:
        total = 0.
        for name in BASIS:
            ctx.profile_enable(True, only=name)
            h.solve_fgmres(b, torch.zeros_like(b), tolerance=1e-8 * r0, max_iterations=200, restart=30)
            launches, kms, nbytes = ctx.profile_query(name)
            ctx.profile_enable(False)
            total += kms
            out(leg='kernels', kernel=name, launches=launches, ms_per_solve=kms, us_per_iteration=1e3 * kms / its,
                TB_per_s=(nbytes / (kms * 1e-3) * 1e-12) if kms else None,
                fraction_of_copy=(nbytes / (kms * 1e-3) * 1e-12 / COPY_TBS) if kms else None)
        out(leg='kernels_summary', basis_ms_per_solve=total, basis_us_per_iteration=1e3 * total / its, share_of_solve=total / ms)
    del h
    torch.cuda.empty_cache()
