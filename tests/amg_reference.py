"""An independent restatement of the smoothed-aggregation setup of the multilevel coarse solver, in long double.

Per level (amg_setup.cpp: build_aggregation_hierarchy with a grid hint; the header of amg_device_setup.hip):
  aggregates   cubes of `blk` nodes aligned at the global origin, one aggregate per component; the coarse grid has
               ceil(dim / blk) nodes per axis (a missing axis counts as 1); rows are node-major, component-minor;
  tentative    t_i = B_i / |B|_aggregate,  B_c = |B|_aggregate;
  damping      rho = max_i sum_j |a_ij| / |a_ii|,  w = omega / rho;
  prolongator  P = (I - w D^-1 A) P_tent;
  operator     A_c = P^T A P;
  a level is coarsened while it has more than `coarsest_size` rows and `max_levels` is not reached.
Nothing here probes, and nothing is imported from the product: the matrices are formed as the formulas read, with
scipy's generic CSR arithmetic instantiated for np.longdouble (64-bit significand: 2^-11 of the FP64 unit roundoff).
`dtype=np.float64` runs the same statements in doubles for one level of a hierarchy too large for this (the per-level
form of the tests).

Beside each value the magnitude sum its error bound is relative to:
  mag P    = |t_i| [own aggregate] + w |d_i^-1| sum_j |a_ij| |t_j|
  mag A_c  = (mag P)^T |A| (mag P)     -- NOT |P|^T |A| |P|: the setup multiplies with ITS P, which is rounded relative to mag P,
                                          so the larger magnitude is the one a correct setup is bounded by (|P| <= mag P)
and the absolute bound itself (`bound_P`, `bound_A`), per entry, with k counted from the code:

  k_B(l)   relative error of the near-null vector of level l in units of u.  Level 0: the row sum of R over n terms in any
           order, n u sum |R_ij| / |sum R_ij| (`near_null_vector`); every level adds the sum of blk^3 squares and a square
           root: k_B(l + 1) = k_B(l) + blk^3 + 1.
  k_t      = 2 k_B + blk^3 + 2: B_i and |B| (both inherited), the sum of blk^3 squares, the square root, the division.
  k_w      = n_row + 2: sum_j |a_ij| over the longest row, s / |d|, omega / rho.
  k_P      = k_t + k_w + blk^3 + 4 + 1: the row applied to the probe has at most blk^3 nonzero terms (one aggregate of one
           component), then 1 / d, w d^-1, times (A y), the subtraction; 1 for the long double itself.
  n_A      = n_row + n_col + 1: the terms of P^T (A (P e)) along the longest chain -- the longest row of A and the longest
           column of P (P e is exact) -- and 1 for the long double.
  bound_P  = gamma_{k_P} mag P  +  what an error E of A_l does to P (chain form)
  bound_A  = gamma_{n_A} Pm^T Am Pm + Pm^T E Pm + bound_P^T Am Pm + Pm^T Am bound_P,   Pm = |P| + bound_P, Am = |A| + E.
           To first order and with E = 0 (the per-level form) that is (n_A + 2 k_P) u on mag A_c.
  E        the bound of A_l of the level above (chain form: |P|^T dA |P| and the rest, propagated); 0 for the per-level form, where
           A_l is the setup's own.  E changes d^-1 by E_ii / |a_ii| and w by max_i E_ii / |a_ii| + max_i (E 1)_i / (|A| 1)_i.
  u_store  2^-24 where the setup rounds every assembled value to float ("setup value precision" float): added per entry on
           the assembled value, (1 + 2^-24) bound + 2^-24 |value|, + one u for the mean of an entry and its transposed partner.
The level operators of this project are applied from CSR rows or from stencil tables that hold the same values, so |A| |v| is the
magnitude of an application on every level here (R A, whose table is NOT the entries, is not part of this setup)."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53
OMEGA = 4.0 / 3.0          # AmgOptions::omega (amg_setup.hpp)


def gamma(k, u=U):
    k = np.asarray(k, dtype=np.float64)
    return k * u / (1.0 - k * u)


def grid3(dims):
    d = [max(int(v), 1) for v in dims] + [1, 1]
    return tuple(d[:3])


def coarse_dims(dims, blk):
    return tuple((d + blk - 1) // blk for d in grid3(dims))


def reach_recurrence(reach, blk):
    return (blk - 1 + 3 * reach) // blk


def node_coordinates(dims):
    nx, ny, nz = grid3(dims)
    nd = np.arange(nx * ny * nz)
    return nd % nx, (nd // nx) % ny, nd // (nx * ny)


def aggregate_of_rows(dims, C, blk):
    """Coarse row of every fine row: node-major, component-minor on both grids."""
    i, j, k = node_coordinates(dims)
    cd = coarse_dims(dims, blk)
    agg = i // blk + cd[0] * (j // blk + cd[1] * (k // blk))
    return (agg[:, None] * C + np.arange(C)[None, :]).ravel()


def near_null_vector(R, C):
    """B_0 of the first aggregation level (build_coarse_solver): the row sum of the restrictor on rows of component 0, 1 on
    the rows of every other component; and k_B(0), the worst n u sum |R_ij| / |sum R_ij| of a row in units of u."""
    R = sp.csr_matrix(R)
    Rl = R.astype(LD)
    ones = np.ones(R.shape[1], dtype=LD)
    s = np.asarray(Rl @ ones).ravel()
    a = np.asarray(abs(Rl) @ ones).ravel()
    comp = np.arange(R.shape[0]) % C
    B = np.where(comp == 0, s, LD(1))
    n = np.diff(R.indptr)
    kB = float(np.max(np.where(comp == 0, n * a / np.abs(np.where(s == 0, 1, s)), 0)))
    return B, kB


def _ones(n, dtype):
    return np.ones(n, dtype=dtype)


def reference_level(A, B, dims, C, blk, omega=OMEGA, kB=0.0, E=None, u_store=0.0, dtype=LD, P_given=None, bounds=True):
    """One level.  Returns a dict: P, A_c, B_c, w, rho, mag_P, mag_A, bound_P, bound_A (all sparse in `dtype`), the counts k_P and
    n_A, and k_B of the next level.  `P_given`: the prolongator the setup stored (float setups: A_c is the product of the
    ROUNDED matrices) -- then P, mag_P are that matrix and bound_P is 0."""
    A = sp.csr_matrix(A).astype(dtype)
    A.sum_duplicates()
    n = A.shape[0]
    B = np.asarray(B).astype(dtype)
    agg = aggregate_of_rows(dims, C, blk)
    assert agg.shape[0] == n == B.shape[0], (agg.shape, n, B.shape)
    n_c = int(np.prod(coarse_dims(dims, blk))) * C
    m = blk ** 3
    norm2 = np.zeros(n_c, dtype=dtype)
    np.add.at(norm2, agg, B * B)
    assert np.all(norm2 > 0)
    B_c = np.sqrt(norm2)
    t = B / B_c[agg]
    P_tent = sp.csr_matrix((t, (np.arange(n), agg)), shape=(n, n_c))
    absA = abs(A)
    d = A.diagonal()
    s = np.asarray(absA @ _ones(n, dtype)).ravel()
    rho = np.max(s / np.abs(d))
    w = dtype(omega) / rho
    Dinv = sp.diags(w / d).tocsr()
    absDinv = abs(Dinv)
    n_row = int(np.diff(A.indptr).max())
    k_t = 2 * kB + m + 2
    k_w = n_row + 2
    k_P = k_t + k_w + m + 4 + 1
    if P_given is None:
        P = (P_tent - Dinv @ (A @ P_tent)).tocsr()
        smooth_mag = (absDinv @ (absA @ abs(P_tent))).tocsr()
        mag_P = (abs(P_tent) + smooth_mag).tocsr()
        bound_P = mag_P * dtype(gamma(k_P))
        if E is not None and E.nnz:
            E = sp.csr_matrix(E).astype(dtype)
            eps_d = E.diagonal() / np.abs(d)
            eps_w = np.max(eps_d) + np.max(np.asarray(E @ _ones(n, dtype)).ravel() / s)
            bound_P = bound_P + absDinv @ (E @ abs(P_tent)) + sp.diags(eps_d + eps_w) @ smooth_mag
        if u_store:
            bound_P = bound_P * dtype(1 + u_store) + abs(P) * dtype(u_store)
        bound_P = bound_P.tocsr()
    else:
        P = sp.csr_matrix(P_given).astype(dtype)
        mag_P = abs(P)
        bound_P = sp.csr_matrix(P.shape, dtype=dtype)
    A_c = (P.T @ (A @ P)).tocsr()
    if not bounds:       # (values only: the levels a cycle is run on)
        return dict(A=A, P=P, A_c=A_c, B=B, B_c=B_c, w=w, rho=rho, kB_next=kB + m + 1, dims_c=coarse_dims(dims, blk), bound_A=None,
                    bound_P=None, mag_P=None, mag_A=None, k_P=k_P, k_A=None, n_A=None)
    mag_A = (mag_P.T @ (absA @ mag_P)).tocsr()
    n_col = int(np.diff(P.tocsc().indptr).max())
    n_A = n_row + n_col + 1
    Pm = (abs(P) + bound_P).tocsr()
    Am = absA if E is None else (absA + sp.csr_matrix(E).astype(dtype)).tocsr()
    AmPm = (Am @ Pm).tocsr()
    bound_A = (Pm.T @ AmPm) * dtype(gamma(n_A))
    if bound_P.nnz:
        cross = (bound_P.T @ AmPm).tocsr()
        bound_A = bound_A + cross + cross.T
    if E is not None and sp.csr_matrix(E).nnz:
        bound_A = bound_A + Pm.T @ (sp.csr_matrix(E).astype(dtype) @ Pm)
    if u_store:
        bound_A = bound_A * dtype(1 + u_store + U) + abs(A_c) * dtype(u_store + U)
    return dict(A=A, P=P, A_c=A_c, B=B, B_c=B_c, w=w, rho=rho, t=t, agg=agg, mag_P=mag_P, mag_A=mag_A, bound_P=bound_P,
                bound_A=bound_A.tocsr(), k_P=k_P, n_A=n_A, k_A=n_A + 2 * k_P, kB_next=kB + m + 1, dims_c=coarse_dims(dims, blk))


def reference_hierarchy(A0, B0, dims, C, blk, omega=OMEGA, coarsest_size=1100, max_levels=10, kB0=0.0, u_store=0.0, dtype=LD, bounds=True):
    """[(A_l, P_l or None, B_l)] and, beside it, one dict per level with the magnitudes and the chain-form bounds: `bound_A_l` of
    the level's own operator (0 on level 0, which is handed in), `bound_P`, `mag_P`, and `mag_A_l`."""
    A = sp.csr_matrix(A0).astype(dtype)
    B = np.asarray(B0).astype(dtype)
    dims = grid3(dims)
    E = None
    kB = kB0
    levels, info = [], []
    mag_A = None
    while len(levels) + 1 < max_levels and A.shape[0] > coarsest_size:
        r = reference_level(A, B, dims, C, blk, omega, kB=kB, E=E, u_store=u_store, dtype=dtype, bounds=bounds)
        levels.append((A, r["P"], B))
        info.append(dict(dims=dims, bound_A=E, mag_A=mag_A, bound_P=r["bound_P"], mag_P=r["mag_P"], k_P=r["k_P"], k_A=r["k_A"],
                         n_A=r["n_A"], w=r["w"], rho=r["rho"]))
        A, B, E, mag_A, kB, dims = r["A_c"], r["B_c"], r["bound_A"], r["mag_A"], r["kB_next"], r["dims_c"]
    levels.append((A, None, B))
    info.append(dict(dims=dims, bound_A=E, mag_A=mag_A, bound_P=None, mag_P=None))
    return levels, info


def chebyshev_beta(cheb):
    """The step of the degree-1 Chebyshev smoother, 1 / theta with theta = (lambda_max + lambda_min) / 2 in doubles, from
    the level's (degree, lambda_min, lambda_max)."""
    degree, lmin, lmax = cheb
    assert degree == 1
    return 1.0 / (0.5 * (lmax + lmin))


def smoothed_prolongator(A, P, cheb, dtype=LD):
    """P~ = (I - beta D^-1 A) P of a V(0,1) level with a damped-Jacobi post-smoother, its magnitude |P| + beta |D^-1| |A| |P|, and
    k: the longest row of A, then 1 / d, beta d^-1, times (A p), the subtraction; 2 for beta (a sum and a division in doubles); 1
    for the long double."""
    A = sp.csr_matrix(A).astype(dtype)
    P = sp.csr_matrix(P).astype(dtype)
    beta = dtype(chebyshev_beta(cheb))
    Dinv = sp.diags(beta / A.diagonal()).tocsr()
    Pt = (P - Dinv @ (A @ P)).tocsr()
    mag = (abs(P) + abs(Dinv) @ (abs(A) @ abs(P))).tocsr()
    k = int(np.diff(A.indptr).max()) + 4 + 2 + 1
    return Pt, mag, k


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def _csr(M, dtype):
    M = sp.csr_matrix(M).astype(dtype)
    M.sum_duplicates()
    return M


def _beyond(got, ref, bound, dtype):
    """(|got - ref|, the entries of it beyond the bound as a sparse matrix): sparse throughout; an entry nobody stores is 0."""
    err = abs(_csr(got, dtype) - _csr(ref, dtype)).tocsr()
    over = (err - _csr(bound, dtype)).tocsr()
    over.data = np.where(over.data > 0, over.data, 0)
    over.eliminate_zeros()
    return err, over


def compare(got, ref, bound, mag=None, what="", pattern="subset", dtype=LD):
    """The per-entry rule.  `got`: the setup's matrix (float64 CSR); `ref`, `bound`, `mag`: the reference's.
    Every entry, stored or not, must lie within its bound: an entry of the reference the setup does not store is compared as 0,
    and a stored entry outside the reference's pattern must be within the bound of zero there (an exact structural zero is).
    pattern "subset": every nonzero of the reference beyond its bound from zero is stored; "equal": and no nonzero is stored
    outside the pattern of the reference.
    Returns the worst |got - ref| / (u mag) over the entries with mag > 0 (0 where no `mag` is given); raises AssertionError."""
    g = sp.csr_matrix(got)
    assert g.shape == ref.shape, f"{what}: shape {g.shape} instead of {ref.shape}"
    assert np.isfinite(g.data).all(), f"{what}: {int((~np.isfinite(g.data)).sum())} entries that are not finite"
    err, over = _beyond(g, ref, bound, dtype)
    if over.nnz:
        c = over.tocoo()
        i, j = int(c.row[0]), int(c.col[0])
        raise AssertionError(f"{what}: {over.nnz} entries beyond the bound, first ({i}, {j}): got {float(g[i, j])!r}, reference "
                             f"{float(ref[i, j])!r}, |difference| {float(err[i, j]):.3e}, bound {float(sp.csr_matrix(bound)[i, j]):.3e}")
    # the patterns, by value.  The assembly kernels drop a value that comes out as exactly 0.0, so a nonzero of the reference
    # that lies within its own bound of zero may be absent (it was compared as 0 above); every other one must be stored
    stored, wanted = (g != 0).tocsr(), ((abs(_csr(ref, dtype)) - _csr(bound, dtype)) > 0).tocsr()
    missing = wanted.nnz - wanted.multiply(stored).nnz
    assert missing == 0, f"{what}: {missing} nonzeros of the reference are not stored"
    if pattern == "equal":
        outside = stored.nnz - stored.multiply((_csr(ref, dtype) != 0).tocsr()).nnz
        assert outside == 0, f"{what}: {outside} stored nonzeros outside the pattern of the reference"
    if mag is None:
        return 0.0
    inv = _csr(mag, dtype)
    inv.eliminate_zeros()
    inv.data = 1 / (dtype(U) * inv.data)
    ratio = err.multiply(inv).tocsr()
    return float(ratio.data.max()) if ratio.nnz else 0.0


def within(got, ref, bound, dtype=LD):
    """compare() as a predicate (pattern not checked)."""
    g = sp.csr_matrix(got)
    return bool(np.isfinite(g.data.astype(np.float64)).all()) and _beyond(g, ref, bound, dtype)[1].nnz == 0


def old_rule_passes(got, ref, tol=1e-11):
    """The rule the suite held these matrices to before: max |got - ref| < 1e-11 max |ref| (test_transfer_shapes.py)."""
    d = abs(_csr(got, np.float64) - _csr(ref, np.float64))
    return bool((d.max() if d.nnz else 0.0) < tol * abs(_csr(ref, np.float64)).max())
