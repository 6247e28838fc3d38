# usage: numbering_time.py [cells=256] [legs=kernel,cycle,cg]
# "internal numbering" lexicographic on a renumbered mesh, one session on one box:
#   kernel  the DoF permutation alone (Hierarchy.permute, HIP events per launch) for every kernel variant (MFMG_DOF_PERMUTATION is
#           read when a context is created: one context per variant) x {dealii, random} x {double, float} x direction
#   cycle   ms per V-cycle as bench.py measures it (constant material, Chebyshev(3), the bench's coarse solver, steps 20 warmup 5):
#           the lexicographic problem, and deal.II's numbering in caller mode (the behaviour without the key) and in lexicographic
#           mode, with the "dof_permutation" time per cycle from the profiler in a separate pass
#   cg      solve_cg to 1e-8 as bench.py's cg_solve leg: the lexicographic problem against deal.II's numbering in lexicographic mode
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M

cells = int(sys.argv[1]) if len(sys.argv) > 1 else 256
legs = (sys.argv[2] if len(sys.argv) > 2 else 'kernel,cycle,cg').split(',')
n = (cells,) * 3
COPY_TBS = 6.3   # float4 copy rate DESIGN.md 6 quotes


def params(mode=None, preconditioner=False, small=False):
    p = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"partitioner": "block", "nx": 2, "ny": 2, "nz": 2},
         "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0, "n_smoothing_steps": 1},
         "solver": {"type": "amg", "amg": {"smoother_degree": 1, "smoothing_range": 4.0, "n_cycles": 1, "aggregate_block": 2}},
         "is preconditioner": preconditioner, "max levels": 2}
    if not preconditioner:
        p["solver"]["amg"]["pre_smoothing_levels"] = 0
    if mode:
        p["internal numbering"] = mode
    return p


def numbering(kind):
    if kind == 'lexicographic':
        return None
    if kind == 'dealii':
        return M.dealii_numbering(n)
    return torch.from_numpy(np.random.default_rng(7).permutation((cells + 1) ** 3))


def out(**kw):
    print(json.dumps(kw), flush=True)


if 'kernel' in legs:
    for variant in ('brick64', 'brick16', 'ids'):
        os.environ['MFMG_DOF_PERMUTATION'] = variant
        ctx = M.Context()
        for kind in ('dealii', 'random'):
            prob = M.LaplaceProblem(n, 'constant', device='cuda', dof_numbering=numbering(kind))
            h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params('lexicographic'))
            for dtype in (torch.float64, torch.float32):
                a = torch.rand(prob.n_dofs, dtype=dtype, device='cuda')
                b = torch.empty_like(a)
                for to_internal in (True, False):
                    for _ in range(3):
                        h.permute(a, b, to_internal)
                    ctx.profile_enable(True, only='dof_permutation')
                    for _ in range(20):
                        h.permute(a, b, to_internal)
                    launches, ms, nbytes = ctx.profile_query('dof_permutation')
                    ctx.profile_enable(False)
                    tbs = nbytes / (ms * 1e-3) * 1e-12
                    out(leg='kernel', variant=variant, numbering=kind, dtype=str(dtype).split('.')[-1],
                        direction='gather' if to_internal else 'scatter', us_per_launch=1e3 * ms / launches, TB_per_s=tbs,
                        fraction_of_copy=tbs / COPY_TBS)
            del h, prob, a, b
            torch.cuda.empty_cache()
    os.environ.pop('MFMG_DOF_PERMUTATION', None)

ctx = M.Context()


def cycle_ms(kind, mode, steps=20, warmup=5):
    prob = M.LaplaceProblem(n, 'constant', device='cuda', dof_numbering=numbering(kind))
    h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params(mode))
    free = (prob.constrained != 1).to(torch.float64)
    x = torch.rand(prob.n_dofs, dtype=torch.float64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * free
    b = torch.rand(prob.n_dofs, dtype=torch.float64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4)) * free * float(np.prod(prob.h))
    for _ in range(warmup):
        h.apply(b, x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        h.apply(b, x)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    ctx.profile_enable(True, only='dof_permutation')
    for _ in range(steps):
        h.apply(b, x)
    launches, perm_ms, nbytes = ctx.profile_query('dof_permutation')
    ctx.profile_enable(False)
    out(leg='cycle', numbering=kind, mode=mode or 'caller', ms_per_cycle=ms, sweep_terms=h.smoother_sweep_terms(),
        rr_classes=h.residual_restriction_classes(), permutation_launches_per_cycle=launches / steps,
        permutation_ms_per_cycle=perm_ms / steps, permutation_TB_per_s=(nbytes / (perm_ms * 1e-3) * 1e-12) if perm_ms else None)
    return ms


if 'cycle' in legs:
    lex = cycle_ms('lexicographic', None)
    caller = cycle_ms('dealii', 'caller')
    internal = cycle_ms('dealii', 'lexicographic')
    out(leg='cycle_summary', lexicographic_ms=lex, dealii_caller_ms=caller, dealii_lexicographic_ms=internal,
        gain_over_caller=1. - internal / caller, cost_over_lexicographic_ms=internal - lex)


def cg_ms(kind, mode):
    prob = M.LaplaceProblem(n, 'constant', device='cuda', dof_numbering=numbering(kind))
    h = M.Hierarchy(ctx, 'HipMatrixFreeMeshEvaluator', prob, params(mode, preconditioner=True))
    free = (prob.constrained != 1).to(torch.float64)
    x_true = torch.rand(prob.n_dofs, dtype=torch.float64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3)) * free
    b = torch.empty_like(x_true)
    h.operator_apply(0, x_true, b)
    b *= free
    r0 = ctx.l2_norm(b)
    runs = []
    for attempt in range(4):
        x = torch.zeros_like(b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        its, hist = h.solve_cg(b, x, tolerance=1e-8 * r0, max_iterations=200)
        torch.cuda.synchronize()
        if attempt > 0:
            runs.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(runs)[len(runs) // 2]
    out(leg='cg', numbering=kind, mode=mode or 'caller', iterations=int(its), ms_total=ms, runs=runs,
        max_rel_error=float((x - x_true).abs().max() / x_true.abs().max()))
    return ms


if 'cg' in legs:
    a = cg_ms('lexicographic', None)
    c = cg_ms('dealii', 'lexicographic')
    out(leg='cg_summary', lexicographic_ms=a, dealii_lexicographic_ms=c, difference=c / a - 1.)
