"""Long-double reference and per-entry error bounds for the FP32 fine level (test_gpu_fp32_fine_level.py runs the kernels
against it, test_fp32_bound_bites.py shows on the CPU that the bound notices planted errors).  numpy and the oracle only.

Reference: the inputs are float32 values; the operation is evaluated in np.longdouble from them and from the FP64
coefficient table, with the oracle's cell matrices, constraint rule (constrained DoFs read as zero, their rows identities)
and diagonal.

Bound, per entry, with u = 2^-24:  |got - ref| <= k u mag.
  operator      mag_i = (B |x|)_i,  B assembled from max|K_e| ones(8, 8) per cell (K_e carries the cell's coefficient; one
                coefficient per cell: c_e max|K_ref|).  NOT |A| |x|: the kernels form differences (one-term kernel) or sums and
                differences (mode space) of corner values before they scale them, so the error of a cell scales with its
                largest entry times the sum of its corner magnitudes.  Constrained rows: mag_i = |x_i|.
  residual      mag_i + |b_i|
  smoother step |x_i| + |alpha| (|x_i| + |xp_i|) + |beta| dinv_i (mag_i + |b_i|)
  sweep         e_{k+1} = local_k + (1 + |alpha_k|) e_k + |alpha_k| e_{k-1} + |beta_k| dinv (B e_k), local_k the step bound

The constants k: the longest chain of float roundings behind one output, each rounding at most u times a magnitude that the
sums above majorise (the weights of the interpolations are positive and sum to one per direction, sum_modes lambda = max|K|).
"""
import numpy as np

import mfmg_oracle as O

U32 = 2.0 ** -24
LD = np.longdouble

# One coefficient per cell, arithmetic of the one-term kernel (cell_apply_cc): corner difference 1; mass matrix over p: the
# difference `dlt` and the rounded constant 2/3 act on |i0| + |i1| where the result weighs them 2/3 : 1/3, so they count twice:
# 4, its fma 1; mass matrix over r with the direction factor: product 1, fma 1, rounded factor 1; sum of the three directions 2;
# times the coefficient 1, the coefficient rounded to float 1: 13.  The eight cells of a node are summed in a tree of depth 3
# (lane shift, row carry, layer carry): 3.  Together 16.
# Mode space (cell_row_modes): x, y, z butterflies 3; times lambda 1, lambda rounded 1; times the coefficient 1, the coefficient
# rounded 1; x back 2, y back 1; row sum 1, z back and layer carry 2: 13 <= 16.
K_OP_CC = 16
# Eight coefficients per cell (cell_apply): corner difference 1; two interpolations to the Gauss points (difference, fma,
# rounded weight: 3 each) 6; coefficient pair: two rounded coefficients 1, their sum 1, rounded direction factor 1, product 1;
# flux 1; two interpolations back 6; sum of the three directions 2: 20.  The differences inside the eight interpolations act on
# A (|i0| + |i1|) where the two outputs together weigh |i0| + |i1| once (2 A = 1.58): + 5.  A coefficient that varies inside
# the cell: the flux scales with the largest coefficient pair, max|K_e| with the weighted mean (at least 1 / 1.15 of it): + 4.
# Node tree 3.  Together 32.  (The 2-D kernel, a plain dot product per node: coefficient and constant rounded 2, product 1,
# four terms 4, times u 1, sixteen terms 16: 24 <= 32.)
K_OP_GENERAL = 32
# On top in a smoother step, relative to the beta term: r = A x - b 1, beta rounded 1, D^-1 derived in the kernel (coefficient
# rounded 1, three sums 3, kd rounded 1, product 1, division 1) 7, beta D^-1 1, fma 1, the final rounding of the result 1: 12.
# The x term sees the final rounding alone, the alpha term alpha rounded, the difference, the fma and the final rounding (4).
K_EPILOGUE = 12


class Reference:
    """Operator, diagonal and bounds of one mesh and coefficient table (`coef`: float64 [cells][2^dim])."""

    def __init__(self, n, coef, constrained=None):
        self.mesh = O.StructuredMesh(n)
        self.coef = np.asarray(coef, dtype=np.float64)
        self.cd = self.mesh.cell_dofs().astype(np.int64)
        self.con = self.mesh.constrained_mask() if constrained is None else np.asarray(constrained, dtype=bool)
        self.n_dofs = self.mesh.n_dofs
        self.cell_constant = bool((self.coef == self.coef[:, :1]).all())
        self.Ke = O.cell_matrices(self.mesh, self.coef).astype(LD)                      # [c][i][j]
        if self.mesh.dim == 3:
            self.kmax = np.abs(self.Ke).max(axis=(1, 2))
        else:
            # (2-D kernel: sum_q c_q K_q[m][n] term by term, the terms of one entry may differ in sign)
            G, f = O.reference_gradients(2), O.geometry_factors(self.mesh)
            Kq = np.abs(np.einsum("d,qdi,qdj->qij", f, G, G))
            self.kmax = np.einsum("cq,qij->cij", self.coef, Kq).max(axis=(1, 2)).astype(LD)
        self.k_op = K_OP_CC if (self.cell_constant and self.mesh.dim == 3) else K_OP_GENERAL
        self.k_step = self.k_op + K_EPILOGUE
        self.dinv = self.dinv_from(self.coef)

    def dinv_from(self, coef, cells=None):
        """1 / diagonal (constrained: 1) in long double; `cells`: a mask of the cells that take part."""
        G, f = O.reference_gradients(self.mesh.dim), O.geometry_factors(self.mesh)
        K = np.einsum("d,qdi,qdi->qi", f, G, G)
        dloc = np.einsum("cq,qi->ci", np.asarray(coef, dtype=np.float64), K).astype(LD)
        if cells is not None:
            dloc = dloc * cells[:, None]
        d = np.zeros(self.n_dofs, dtype=LD)
        np.add.at(d, self.cd.ravel(), dloc.ravel())
        d[self.con] = 1
        return 1 / d

    # ---- the operation in long double ----
    def cell_values(self, x, Ke=None):
        xr = np.where(self.con, LD(0), np.asarray(x).astype(LD))
        return np.einsum("cij,cj->ci", self.Ke if Ke is None else Ke, xr[self.cd])

    def scatter(self, v, x):
        y = np.zeros(self.n_dofs, dtype=LD)
        np.add.at(y, self.cd.ravel(), v.ravel())
        y[self.con] = np.asarray(x).astype(LD)[self.con]
        return y

    def vmult(self, x):
        return self.scatter(self.cell_values(x), x)

    def step(self, x, b, xp, alpha, beta, ax=None, dinv=None):
        x, b = np.asarray(x).astype(LD), np.asarray(b).astype(LD)
        ax = self.vmult(x) if ax is None else ax
        mom = LD(alpha) * (x - np.asarray(xp).astype(LD)) if xp is not None else 0
        return x + mom - LD(beta) * (self.dinv if dinv is None else dinv) * (ax - b)

    def sweep(self, x, b, alphas, betas):
        """[x_0, x_1, ..., x_K] of the recurrence."""
        its = [np.asarray(x).astype(LD)]
        for k, (al, be) in enumerate(zip(alphas, betas)):
            its.append(self.step(its[-1], b, its[-2] if k > 0 else None, al, be))
        return its

    # ---- magnitudes ----
    def mag(self, x):
        """(B |x|)_i; constrained rows |x_i|."""
        ax = np.abs(np.asarray(x).astype(LD))
        xr = np.where(self.con, LD(0), ax)
        per_cell = self.kmax.astype(LD) * xr[self.cd].sum(axis=1)
        m = np.zeros(self.n_dofs, dtype=LD)
        np.add.at(m, self.cd.ravel(), np.repeat(per_cell, self.cd.shape[1]))
        m[self.con] = ax[self.con]
        return m

    def unit_vmult(self, x):
        return U32 * self.mag(x)

    def unit_residual(self, x, b):
        return U32 * (self.mag(x) + np.abs(np.asarray(b).astype(LD)))

    def unit_step(self, x, b, xp, alpha, beta):
        ax, axp = np.abs(np.asarray(x).astype(LD)), (np.abs(np.asarray(xp).astype(LD)) if xp is not None else 0)
        return U32 * (ax + abs(alpha) * (ax + axp) + abs(beta) * self.dinv * (self.mag(x) + np.abs(np.asarray(b).astype(LD))))

    def unit_sweep(self, its, b, alphas, betas):
        """Propagated bounds of x_1 .. x_K in units of k_step (multiply by self.k_step)."""
        zero = np.zeros(self.n_dofs, dtype=LD)
        e = [zero]
        for k, (al, be) in enumerate(zip(alphas, betas)):
            local = self.unit_step(its[k], b, its[k - 1] if k > 0 else None, al, be)
            prev = e[-2] if k > 0 else zero
            e.append(local + (1 + abs(al)) * e[-1] + abs(al) * prev + abs(be) * self.dinv * self.mag(e[-1]))
        return e[1:]


def f32(a):
    return np.asarray(a).astype(np.float32)


def beyond(got, ref, bound):
    """Entries outside the bound; NaN (an entry no thread wrote) counts as outside."""
    return ~(np.abs(np.asarray(got).astype(LD) - ref) <= bound)


def worst_ratio(got, ref, unit):
    """max |got - ref| / (u mag) over the entries with a magnitude."""
    err = np.abs(np.asarray(got).astype(LD) - ref)
    ok = unit > 0
    return float((err[ok] / unit[ok]).max()) if ok.any() else 0.0


def assert_within(got, ref, unit, k, what):
    bad = beyond(got, ref, k * unit)
    assert not bad.any(), f"{what}: {int(bad.sum())} entries beyond {k} u mag (worst ratio {worst_ratio(got, ref, unit):.2f}), first at " \
                          f"{np.flatnonzero(bad)[:5]}: got {np.asarray(got)[bad][:3]}, ref {ref[bad][:3].astype(float)}, bound {(k * unit)[bad][:3].astype(float)}"


def old_rule_passes(got, ref):
    """The rule of test_mf_fp32_instance: the largest difference against 1e-4 of the largest entry."""
    ref = np.asarray(ref).astype(float)
    return bool(np.abs(np.asarray(got).astype(float) - ref).max() / max(np.abs(ref).max(), 1e-300) < 1e-4)
