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

Either precision: the unit roundoff is a property of the Reference (u = 2^-24 by default, 2^-53 for the FP64 kernels:
test_gpu_fp64_fine_level.py, test_fp64_bound_bites.py).  At 2^-53 the cell matrices and the diagonal are formed in long double
as well (exact Gauss points, the factors from the double cell sizes), and the reference's own roundings are part of the bound:
k u mag + K_REF 2^-64 mag = (k + k_ref) u mag with k_ref = K_REF 2^-11 (Reference.k_ref; zero at 2^-24, where nothing changes).
"""
import numpy as np

import mfmg_oracle as O

U32 = 2.0 ** -24
U64 = 2.0 ** -53
LD = np.longdouble
ULD = 2.0 ** -64     # unit roundoff of a 64-bit significand (x86 extended precision); checked where a Reference is built at 2^-53

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
# FP64 instances: the same templates, the same constants.  What is "rounded to float" above (the coefficient, beta, alpha) is
# exact in double, which takes one off every chain; the constants 2/3, the Gauss weights and the mass-matrix entries are rounded
# as before.  What does not carry over unchanged is the set-up on the host, done in double for either precision: in float its
# result is rounded once more (the "rounded factor", "lambda rounded" and "kd rounded" above) and its own roundings are 2^-29 of
# that; in double they are roundings like any other.  Written out (mf_cell_factors): f_d = h0 h1 h2 / 8 / h_d^2 4 roundings where
# float has 1 (one-term kernel, one coefficient per cell: 16 - 1 + 3 = 18; mode space, lambda_6 = (f0 + f1 + f2) / 18 7 where float
# has 1: 13 - 1 + 6 = 18); kd = 2 m00 m00 (f0 + f1 + f2) with m00 = A^2 + B^2 from the rounded Gauss weights.  These worst cases lie
# above the constants kept here; the FP64 tests hold the kernels to the float counts all the same (a tighter rule, never a wider
# one), and what they observe on an MI355X is written next to k in test_gpu_fp64_fine_level.py.
#
# The reference's own error at 2^-53, in roundings of 2^-64 behind one entry (every one at most 2^-64 times a magnitude the sums
# of the bound majorise): a cell-matrix entry -- gradients from the rounded Gauss points 3, the factor 4, three directions 5, eight
# Gauss points with their coefficients 16 -- 28; einsum over the 8 corners 15; np.add.at over the 8 cells 8; the epilogue
# (difference with b, D^-1 with its own 28 + 8 + 1, two products, momentum 3, two sums) 45 per term, and the recurrence of the
# sweep propagates them as the bound propagates the kernel's.  96 per term: 96 2^-11 = 0.047 of one unit of k.
K_REF = 96
# diagonal_inverse() in FP64 (mf_diagonal_kernel: a table K[q][m] = sum_d f_d g_d^2 made on the host in double, then
# sum += c_q K[q][m] over 8 cells x 8 Gauss points and 1 / sum, all terms positive): f_d 4; g_d a product of two rounded Gauss
# weights (1 - xi rounded again) 5, squared 11; two products 2; three directions 3: 20 per table entry; 64 accumulations; the
# division 1: 85.  (The float instance does the same in double and rounds once: the 2 u of test_gpu_fp32_fine_level.py.)
K_DINV_F64 = 85


def _cell_tables_long(mesh):
    """(G[q][d][i], f[d]) in long double: the gradients at the exact Gauss points, the factors from the double cell sizes."""
    g = 1 / np.sqrt(LD(3))
    pts = [(1 - g) / 2, (1 + g) / 2]
    assert abs(float(pts[0]) - O.GAUSS_PTS[0]) < 1e-15 and abs(float(pts[1]) - O.GAUSS_PTS[1]) < 1e-15
    dim, nq = mesh.dim, 2 ** mesh.dim
    G = np.zeros((nq, dim, nq), dtype=LD)
    for q in range(nq):
        xi = [pts[(q >> d) & 1] for d in range(dim)]
        for i in range(nq):
            for d in range(dim):
                v = LD(1)
                for e in range(dim):
                    bit = (i >> e) & 1
                    v = v * ((LD(1) if bit else LD(-1)) if e == d else (xi[e] if bit else 1 - xi[e]))
                G[q, d, i] = v
    h = [LD(v) for v in mesh.h]
    vol = LD(1)
    for v in h:
        vol = vol * v
    f = np.array([vol / nq / (v * v) for v in h], dtype=LD)
    return G, f


class Reference:
    """Operator, diagonal and bounds of one mesh and coefficient table (`coef`: float64 [cells][2^dim])."""

    def __init__(self, n, coef, constrained=None, u=U32):
        assert u in (U32, U64)
        self.u = u
        self.long_tables = u == U64
        if self.long_tables:
            # 63 fraction bits: 2^-11 of the FP64 unit roundoff.  Anything less and this reference cannot judge a double.
            assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit significand here: no reference for the FP64 kernels"
        self.k_ref = K_REF * ULD / u if self.long_tables else 0.0
        self.mesh = O.StructuredMesh(n)
        self.coef = np.asarray(coef, dtype=np.float64)
        self.cd = self.mesh.cell_dofs().astype(np.int64)
        self.con = self.mesh.constrained_mask() if constrained is None else np.asarray(constrained, dtype=bool)
        self.n_dofs = self.mesh.n_dofs
        self.cell_constant = bool((self.coef == self.coef[:, :1]).all())
        if self.long_tables:
            self.G, self.f = _cell_tables_long(self.mesh)
            self.Ke = np.einsum("cq,qij->cij", self.coef.astype(LD), np.einsum("d,qdi,qdj->qij", self.f, self.G, self.G))
        else:
            self.G, self.f = O.reference_gradients(self.mesh.dim), O.geometry_factors(self.mesh)
            self.Ke = O.cell_matrices(self.mesh, self.coef).astype(LD)                  # [c][i][j]
        if self.mesh.dim == 3:
            self.kmax = np.abs(self.Ke).max(axis=(1, 2))
        else:
            # (2-D kernel: sum_q c_q K_q[m][n] term by term, the terms of one entry may differ in sign)
            G, f = self.G, self.f
            Kq = np.abs(np.einsum("d,qdi,qdj->qij", f, G, G))
            self.kmax = np.einsum("cq,qij->cij", self.coef, Kq).max(axis=(1, 2)).astype(LD)
        self.k_op = K_OP_CC if (self.cell_constant and self.mesh.dim == 3) else K_OP_GENERAL
        self.k_step = self.k_op + K_EPILOGUE
        self.dinv = self.dinv_from(self.coef)

    def dinv_from(self, coef, cells=None):
        """1 / diagonal (constrained: 1) in long double; `cells`: a mask of the cells that take part."""
        K = np.einsum("d,qdi,qdi->qi", self.f, self.G, self.G)
        dloc = np.einsum("cq,qi->ci", np.asarray(coef, dtype=np.float64).astype(K.dtype), K).astype(LD)
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
        return self.u * self.mag(x)

    def unit_residual(self, x, b):
        return self.u * (self.mag(x) + np.abs(np.asarray(b).astype(LD)))

    def unit_step(self, x, b, xp, alpha, beta):
        ax, axp = np.abs(np.asarray(x).astype(LD)), (np.abs(np.asarray(xp).astype(LD)) if xp is not None else 0)
        return self.u * (ax + abs(alpha) * (ax + axp) + abs(beta) * self.dinv * (self.mag(x) + np.abs(np.asarray(b).astype(LD))))

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


def f64(a):
    return np.asarray(a).astype(np.float64)


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
