#!/usr/bin/env python3
"""The workflow of the reference's driver (/root/reference/tests/hierarchy_driver.cc) on the HIP back-end.

    python examples/hierarchy_driver.py -f hierarchy_input.info -d 3 -m 1 [-t 1e-6]

Same command line (`:216-253`: --filename/-f, --dim/-d, --matrix_free/-m, --tolerance/-t), same parameter handling
(`:255-283`: the INFO file is read, `fast_ap` is forced to true, `eigensolver.type` to anasazi with tolerance 1e-3,
`solver.tolerance` from the command line; matrix-free runs force `smoother.type Chebyshev`, `:400-402`), same two modes:
`"is preconditioner" false` -> 20 V-cycles on rhs = 0 from a random start vector and the convergence rate
res[20] / res[19] (`:74-101`); true -> CG preconditioned by the hierarchy (`:103-116`).  Differences: the mesh is the
hyper-cube of `laplace.n_refinements` global refinements with Q1 elements, or Q2 elements for a matrix-free CG / FGMRES solve in
3-D (`laplace.fe_degree 2`: the Q2 operator preconditioned by a Chebyshev smoother around the cycle of the hierarchy on the
refined Q1 mesh, M.HighOrderSolver; the subtree `"high order"` of the file holds its parameters); other degrees are
refused (where the file names none the reference takes degree 4, `:269`, this script degree 1), and a matrix-based run whose input file asks for an Ifpack relaxation (Gauss-Seidel, the file's default) takes
Jacobi, the CUDA back-end's smoother, with a note.

`--numbering dealii` numbers the DoFs as deal.II's DoFHandler::distribute_dofs does (cells in Morton order, vertex DoFs at first
touch), `random` by a seeded permutation; both set `"internal numbering" lexicographic` (matrix-free runs), so that the hierarchy
runs on the kernels of the lexicographic numbering and permutes vectors at its interface.

`--solver fgmres` (with `"is preconditioner" true`) solves with the flexible GMRES driver in place of CG: the hierarchy may then
be a non-symmetric cycle (`solver.amg.pre_smoothing_levels 0`), and `--preconditioner-precision float` runs its fine level in
FP32 under the FP64 iteration (sets `"fine level precision" float`; matrix-free, two levels).  `--restart` is the basis size.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mfmg_amd as M  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-f", "--filename", default="hierarchy_input.info")
    ap.add_argument("-d", "--dim", type=int, default=2)
    ap.add_argument("-m", "--matrix_free", type=int, default=0)
    ap.add_argument("-t", "--tolerance", type=float, default=1e-6)
    ap.add_argument("--numbering", choices=["lexicographic", "dealii", "random"], default="lexicographic")
    ap.add_argument("--solver", choices=["cg", "fgmres"], default="cg")
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--preconditioner-precision", choices=["double", "float"], default="double")
    args = ap.parse_args(argv)
    if args.dim not in (2, 3):
        raise SystemExit("dim must be 2 or 3")
    if args.preconditioner_precision == "float" and args.solver != "fgmres":
        raise SystemExit("--preconditioner-precision float needs --solver fgmres (CG wants a fixed, symmetric preconditioner)")
    params = M.info_to_params(open(args.filename).read())
    if not args.matrix_free and params.get("use_raw_ml", False):
        raise SystemExit("use_raw_ml: ML is not part of the HIP build")
    fe_degree = int(params.get("laplace", {}).get("fe_degree", 1))
    if fe_degree == 2:
        if not (args.matrix_free and args.dim == 3 and params.get("is preconditioner", True) and args.numbering == "lexicographic"
                and args.preconditioner_precision == "double"):
            raise SystemExit("laplace.fe_degree 2 is a matrix-free solve in 3-D (\"is preconditioner\" true, lexicographic "
                             "numbering, FP64): the Q2 operator preconditioned by the cycle of the refined Q1 mesh")
    elif fe_degree != 1:
        raise SystemExit("laplace.fe_degree must be 1 or 2: higher degrees are outside the scope of the HIP build")
    params["fast_ap"] = True
    params.setdefault("eigensolver", {})["type"] = "anasazi"
    params["eigensolver"]["tolerance"] = 1e-3
    params.setdefault("solver", {})["tolerance"] = args.tolerance
    print(f"input file: {args.filename}, dimension: {args.dim}, matrix-free: {args.matrix_free}, fe_degree: {fe_degree}, "
          f"solver_tolerance: {args.tolerance}")
    if args.matrix_free:
        params.setdefault("smoother", {})["type"] = "Chebyshev"
    elif str(params.get("smoother", {}).get("type", "Jacobi")).lower() not in ("jacobi", "chebyshev"):
        print(f"note: smoother.type \"{params['smoother']['type']}\" is an Ifpack relaxation; taking Jacobi")
        params["smoother"]["type"] = "Jacobi"
    # coarse solver: the reference's default is a direct solve (Amesos / cuSOLVER); large coarse spaces take the multilevel one
    n_ref = int(params.get("laplace", {}).get("n_refinements", 5))
    cells = (2 ** n_ref,) * args.dim
    material = params.get("material_property", {}).get("type", "constant")
    # (degree 2: the hierarchy is built on the refined Q1 mesh, whose cells decide the coarse solver below)
    q1_cells = tuple(2 * c for c in cells) if fe_degree == 2 else cells
    if "type" not in params["solver"]:
        n_coarse = 2
        for c in q1_cells:
            n_coarse *= max(c // int(params.get("agglomeration", {}).get("nx", 2)), 1)
        params["solver"]["type"] = "lu_dense" if n_coarse <= 4096 else "amg"
    ctx = M.Context()
    if fe_degree == 2:
        for key in ("laplace", "material_property"):       # (read above; not parameters of the hierarchy)
            params.pop(key, None)
        prob2 = M.LaplaceProblemQ2(cells, material, device="cuda")
        solver = M.HighOrderSolver(ctx, prob2, params)
        b = torch.rand(prob2.n_dofs, dtype=torch.float64, device="cuda",
                       generator=torch.Generator(device="cuda").manual_seed(2)) * (prob2.constrained == 0)
        x = torch.zeros_like(b)
        if args.solver == "fgmres":
            its, _ = solver.solve_fgmres(b, x, tolerance=args.tolerance, max_iterations=prob2.n_dofs, restart=args.restart)
        else:
            its, _ = solver.solve_cg(b, x, tolerance=args.tolerance, max_iterations=prob2.n_dofs)
        print(f"Converging after {its} iterations.")
        print(solver.hierarchy.timer_report())
        return its
    numbering = None
    if args.numbering == "dealii":
        numbering = M.dealii_numbering(cells)
    elif args.numbering == "random":
        numbering = torch.randperm(math.prod(c + 1 for c in cells), generator=torch.Generator().manual_seed(7))
    if numbering is not None and args.matrix_free:
        params["internal numbering"] = "lexicographic"
    if args.preconditioner_precision == "float":
        params["fine level precision"] = "float"
    prob = M.LaplaceProblem(cells, material, device="cuda", dof_numbering=numbering)
    evaluator = "HipMatrixFreeMeshEvaluator" if args.matrix_free else "HipMeshEvaluator"
    h = M.Hierarchy(ctx, evaluator, prob, params)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(prob.n_dofs, dtype=torch.float64, device="cuda", generator=g) * (prob.constrained == 0)
    b = torch.zeros_like(x)
    r = torch.empty_like(x)
    if not params.get("is preconditioner", True):
        def resnorm():
            h.operator_apply(0, x, r)
            ctx.sadd(r, -1.0, 1.0, b)
            return ctx.l2_norm(r)
        res = [resnorm()]
        for _ in range(20):
            h.vmult(x, b)
            res.append(resnorm())
        print(f"Convergence rate: {res[20] / res[19]:.2f}")
        rate = res[20] / res[19]
    else:
        g2 = torch.Generator(device="cuda").manual_seed(2)
        b = torch.rand(prob.n_dofs, dtype=torch.float64, device="cuda", generator=g2) * (prob.constrained == 0)
        x.zero_()
        if args.solver == "fgmres":
            its, hist = h.solve_fgmres(b, x, tolerance=args.tolerance, max_iterations=prob.n_dofs, restart=args.restart,
                                       preconditioner=args.preconditioner_precision)
        else:
            its, hist = h.solve_cg(b, x, tolerance=args.tolerance, max_iterations=prob.n_dofs)
        print(f"Converging after {its} iterations.")
        rate = its
    print(h.timer_report())
    return rate


if __name__ == "__main__":
    main()
