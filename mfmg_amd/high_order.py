"""Q2 elements: the mesh arrays of the Q2 Laplace problem, the matrix-free Q2 operator and the solver that preconditions it with
a Chebyshev smoother around one cycle of a Q1 hierarchy on the refined mesh (include/mfmg_hip.h, the section on Q2 elements).

For degree 2 the Lagrange nodes are equidistant, so the Q2 unknowns on n cells are the Q1 unknowns on 2 n cells, in the same
lexicographic lattice of (2 n + 1)^3 nodes."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as _lib
from .api import Context, Hierarchy, _dev_ptr, params_to_info
from .laplace import LaplaceProblem, material_property
from .lib import check

# QGauss<1>(3) on [0, 1]
_G3 = (0.5 - 0.5 * math.sqrt(0.6), 0.5, 0.5 + 0.5 * math.sqrt(0.6))


class LaplaceProblemQ2:
    """Mesh arrays of the Q2 Laplace problem on [0, length]^3 with n cells per direction (FE_Q(2), QGauss(3)): the coefficient
    at the 27 quadrature points of every cell (q = qa + 3 qb + 9 qc, cells x-fastest) and the constrained mask on the lattice of
    (2 n + 1)^3 unknowns, lexicographic with x fastest -- the arrays of ``mfmg_hip_q2_mesh_desc``."""

    def __init__(self, n_cells: Sequence[int], material: str = "constant", length: float = 1.0,
                 device: str | torch.device = "cpu", dirichlet: bool = True, cell_size: Optional[Sequence[float]] = None):
        self.n = tuple(int(v) for v in n_cells)
        self.dim = len(self.n)
        if self.dim != 3:
            raise _lib.MfmgNotImplementedError("the Q2 problem exists in 3-D only")
        self.N = tuple(2 * v + 1 for v in self.n)
        self.h = tuple(float(v) for v in cell_size) if cell_size is not None else tuple(length / v for v in self.n)
        self.length = length
        self.device = torch.device(device)
        self.dirichlet = dirichlet
        self.material = material
        self.n_dofs = math.prod(self.N)
        self.n_cells_total = math.prod(self.n)
        dev = self.device
        idx = [torch.arange(v, device=dev, dtype=torch.int64) for v in self.n]
        k, j, i = torch.meshgrid(idx[2], idx[1], idx[0], indexing="ij")
        org = [i.reshape(-1), j.reshape(-1), k.reshape(-1)]
        pts = torch.empty((self.n_cells_total, 27, 3), dtype=torch.float64, device=dev)
        for q in range(27):
            for d in range(3):
                pts[:, q, d] = (org[d].to(torch.float64) + _G3[(q // 3 ** d) % 3]) * self.h[d]
        self.coefficient = material_property(material, pts).to(torch.float64).contiguous()
        con = torch.zeros(self.N[::-1], dtype=torch.bool, device=dev)
        if dirichlet:
            for ax in range(3):
                sl = [slice(None)] * 3
                sl[ax] = 0
                con[tuple(sl)] = True
                sl[ax] = -1
                con[tuple(sl)] = True
        self.constrained = con.reshape(-1).to(torch.uint8).contiguous()

    def mesh_desc(self) -> _lib.Q2MeshDesc:
        d = _lib.Q2MeshDesc()
        d.dim = 3
        for k in range(3):
            d.n_cells[k] = self.n[k]
            d.cell_size[k] = self.h[k]
        d.n_dofs = self.n_dofs
        d.coefficient = self.coefficient.data_ptr()
        d.constrained = self.constrained.data_ptr()
        d.arrays_on_device = 1 if self.device.type == "cuda" else 0
        return d

    def refined_q1(self) -> LaplaceProblem:
        """The Q1 problem on the same lattice of unknowns: 2 n cells of size h / 2, the same material evaluated at the refined
        cells' own Gauss points."""
        return LaplaceProblem(tuple(2 * v for v in self.n), self.material, device=self.device, dirichlet=self.dirichlet,
                              cell_size=tuple(0.5 * v for v in self.h))


def q2_tile_shapes():
    """The tiles (tx, ty, tz) in cells the Q2 operator kernel offers, the default first.  Needs no GPU."""
    lib = _lib.load()
    n = C.c_int32()
    check(lib.mfmg_hip_mf_laplace_q2_tile_shapes(C.byref(n), None, 0))
    buf = (C.c_int32 * (3 * n.value))()
    check(lib.mfmg_hip_mf_laplace_q2_tile_shapes(C.byref(n), buf, 3 * n.value))
    return [tuple(buf[3 * s: 3 * s + 3]) for s in range(n.value)]


class MatrixFreeLaplaceQ2:
    """LaplaceMatrixFree<3, 2, double> of the reference on the GPU (mfmg_hip_mf_laplace_q2_*)."""

    def __init__(self, ctx: Context, problem: LaplaceProblemQ2):
        self._lib = _lib.load()
        self.ctx = ctx
        self.problem = problem  # keeps the mesh arrays alive during construction
        desc = problem.mesh_desc()
        h = C.c_void_p()
        check(self._lib.mfmg_hip_mf_laplace_q2_create(ctx.handle, C.byref(desc), C.byref(h)))
        self.handle = h
        self.n_dofs = problem.n_dofs

    def vmult(self, dst: torch.Tensor, src: torch.Tensor):
        check(self._lib.mfmg_hip_mf_laplace_q2_vmult(self.handle, _dev_ptr(src, self.n_dofs), _dev_ptr(dst, self.n_dofs)))

    def residual(self, x, b, res):
        n = self.n_dofs
        check(self._lib.mfmg_hip_mf_laplace_q2_residual(self.handle, _dev_ptr(x, n), _dev_ptr(b, n), _dev_ptr(res, n)))

    def smoother_step(self, b, x, x_prev, alpha, beta, out):
        n = self.n_dofs
        check(self._lib.mfmg_hip_mf_laplace_q2_smoother_step(self.handle, _dev_ptr(b, n), _dev_ptr(x, n),
                                                             _dev_ptr(x_prev, n) if x_prev is not None else None,
                                                             alpha, beta, _dev_ptr(out, n)))

    def diagonal(self) -> torch.Tensor:
        d = torch.empty(self.n_dofs, dtype=torch.float64, device="cuda")
        check(self._lib.mfmg_hip_mf_laplace_q2_diagonal(self.handle, _dev_ptr(d, self.n_dofs)))
        self.ctx.synchronize()
        return d

    def diagonal_inverse(self) -> torch.Tensor:
        d = torch.empty(self.n_dofs, dtype=torch.float64, device="cuda")
        check(self._lib.mfmg_hip_mf_laplace_q2_diagonal_inverse(self.handle, _dev_ptr(d, self.n_dofs)))
        self.ctx.synchronize()
        return d

    def cell_constant_layout(self) -> bool:
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_q2_cell_constant_layout(self.handle, C.byref(v)))
        return bool(v.value)

    def get_tile(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_q2_get_tile(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_tile(self, tx: int, ty: int, tz: int):
        check(self._lib.mfmg_hip_mf_laplace_q2_set_tile(self.handle, int(tx), int(ty), int(tz)))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.mfmg_hip_mf_laplace_q2_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


# the Q1 hierarchy of HighOrderSolver unless the caller's `params` say otherwise (keys outside "high order")
_Q1_DEFAULTS = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2},
                "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}, "is preconditioner": True}


class HighOrderSolver:
    """The Q2 operator of `problem_q2` with its preconditioner: a Chebyshev smoother on it around one cycle of the Q1 hierarchy
    built here on ``problem_q2.refined_q1()`` (matrix-free evaluator).  `params`: the parameters of that hierarchy, plus the
    subtree "high order" (smoother.degree 2, smoother.smoothing_range 4, ...) of the preconditioner."""

    def __init__(self, ctx: Context, problem_q2: LaplaceProblemQ2, params: Optional[dict] = None):
        self._lib = _lib.load()
        self.ctx = ctx
        params = dict(params or {})
        high = params.pop("high order", {})
        q1_params = params if params else dict(_Q1_DEFAULTS)
        self.problem = problem_q2
        self.n_dofs = problem_q2.n_dofs
        self.operator = MatrixFreeLaplaceQ2(ctx, problem_q2)
        self.q1_problem = problem_q2.refined_q1()
        self.hierarchy = Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", self.q1_problem, q1_params)
        h = C.c_void_p()
        check(self._lib.mfmg_hip_high_order_create(self.hierarchy.handle, self.operator.handle,
                                                   params_to_info({"high order": high}).encode(), C.byref(h)))
        self.handle = h

    def apply(self, b: torch.Tensor, x: torch.Tensor):
        """x = the preconditioner applied to b, from zero."""
        n = self.n_dofs
        check(self._lib.mfmg_hip_high_order_apply(self.handle, _dev_ptr(b, n), _dev_ptr(x, n)))

    def smoother_info(self):
        d, lo, hi = C.c_int32(), C.c_double(), C.c_double()
        check(self._lib.mfmg_hip_high_order_smoother_info(self.handle, C.byref(d), C.byref(lo), C.byref(hi)))
        return d.value, lo.value, hi.value

    def solve_cg(self, b, x, tolerance: float = 1e-6, max_iterations: int = 1000):
        """CG on the Q2 operator with `apply` as preconditioner (needs a symmetric Q1 cycle).  Returns (iterations, history)."""
        n = self.n_dofs
        it, res = C.c_int32(), C.c_double()
        hist = np.zeros(max(max_iterations, 0) + 1)
        check(self._lib.mfmg_hip_high_order_solve_cg(self.handle, _dev_ptr(b, n), _dev_ptr(x, n), tolerance, max_iterations,
                                                     C.byref(it), C.byref(res), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                                     len(hist)))
        return it.value, hist[: it.value + 1]

    def solve_fgmres(self, b, x, tolerance: float = 1e-6, max_iterations: int = 1000, restart: int = 30):
        """Flexible GMRES(restart) on the Q2 operator with `apply` as right preconditioner.  Returns (iterations, history)."""
        n = self.n_dofs
        it, res = C.c_int32(), C.c_double()
        hist = np.zeros(max(max_iterations, 0) + 1)
        check(self._lib.mfmg_hip_high_order_solve_fgmres(self.handle, _dev_ptr(b, n), _dev_ptr(x, n), tolerance, max_iterations,
                                                         restart, C.byref(it), C.byref(res),
                                                         hist.ctypes.data_as(C.POINTER(C.c_double)), len(hist)))
        return it.value, hist[: it.value + 1]

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.mfmg_hip_high_order_destroy(self.handle)
                self.handle = None
        except Exception:
            pass
