"""The rule of the batched Lanczos eigensolver of the restrictor setup (mfmg_amd/csrc/amge_lanczos.hip), restated in numpy, the case
table of its tests and the bound they share.

The rule, for one agglomerate with matrix M on its active DoFs and start vector v0 (the `krylov` selection of the oracle):
  q_1 = v0 / |v0|;  step j: w = M q_j - beta_{j-1} q_{j-1}, alpha_j = q_j . w, w -= alpha_j q_j, w orthogonalised against
  q_1 .. q_j (classical Gram-Schmidt, two passes), beta_j = |w|; all q are kept.
  The run ends after min(active DoFs, max_iterations) steps or at a breakdown, beta_j <= 1e-14 max |theta(T_j)|.
  T_j is examined at j = 1, whenever 100 (j - j_prev) > percent_overshoot j_prev, at the last step and at a breakdown:
  Ritz pairs ascending, grouped as the dense selection does (|theta_i - theta_first| <= 1e-9 scale); the vector of a group is
  the normalised projection of v0 onto the span of the group's Ritz vectors; a group whose projection is below 1e-12 |v0| is
  skipped; converged when n_eig groups are selected and every Ritz pair of every group up to the last selected one has
  beta_j |s_i[j]| <= tolerance scale.  At the last step or a breakdown what is selected is taken as it is."""
import numpy as np
import scipy.linalg as sla

import mfmg_oracle as O

BREAKDOWN = 1e-14
EPS = 2.0 ** -52

# (cells, agglomerate, material)
CASES_3D_LARGE = [
    ((8, 8, 4), (4, 4, 2), "constant"),          # 75 nodes, every agglomerate ends by breakdown
    ((8, 8, 8), (4, 4, 4), "constant"),
    ((8, 8, 8), (4, 4, 4), "linear"),
    ((8, 8, 8), (4, 4, 4), "discontinuous"),
    ((10, 9, 7), (4, 4, 4), "linear"),           # clipped agglomerates of several shapes in one launch
    ((12, 6, 6), (6, 6, 6), "constant"),         # the degenerate-copy case
    ((12, 12, 12), (6, 6, 6), "linear"),         # 343 nodes
    ((16, 8, 8), (8, 8, 8), "linear"),           # 729 nodes, the most iterations
]
CASES_SMALL = [                                  # the sizes the dense device kernel also serves
    ((4, 4, 4), (2, 2, 2), "linear"),
    ((6, 6, 6), (3, 3, 3), "linear"),
]
CASES_2D = [
    ((16, 16), (8, 8), "linear"),
    ((8, 8), (4, 4), "linear"),
]
CASES = CASES_3D_LARGE + CASES_SMALL + CASES_2D


def case_id(c):
    return "x".join(map(str, c[0])) + "-" + "x".join(map(str, c[1])) + "-" + c[2]


def agglomerate_problems(n, agg, material, variant, subset=None):
    """Per agglomerate (x fastest) of the oracle's mesh: dict with the global DoFs `gl`, the matrix `M` of `variant` on the active
    DoFs, their mask `act`, the start vector `v0` on them, `diag_loc` on all local DoFs and the `shift` of variant host --
    the pieces of oracle.build_restrictor, which this restates line by line up to the eigen-solve.
    subset: the indices of the agglomerates to build, in the order given (the others are not walked); None for all."""
    mesh = O.StructuredMesh(n)
    coef = O.coefficient_table(mesh, material)
    con = mesh.constrained_mask()
    Ae = O.cell_matrices(mesh, coef)
    aggs, _ = O.block_agglomerates(mesh, agg[:mesh.dim])
    out = []
    for lo, hi in (aggs if subset is None else [aggs[a] for a in subset]):
        gl, lcd, cid, lN = O.agglomerate_local(mesh, lo, hi)
        nloc = len(gl)
        A = np.zeros((nloc, nloc))
        for c in range(lcd.shape[0]):
            A[np.ix_(lcd[c], lcd[c])] += Ae[cid[c]]
        lcon = con[gl]
        full_diag = A.diagonal().copy()
        A[lcon, :] = 0.0
        A[:, lcon] = 0.0
        A[lcon, lcon] = 1.0 if variant == "mf" else full_diag[lcon]
        diag_loc = A.diagonal().copy()
        Mx = A.copy()
        shift = 0.0
        if variant == "host":
            shift = diag_loc.sum() / nloc
            Mx[np.diag_indices(nloc)] += shift
            Mx[lcon, lcon] = 200.0
        gen = O.MinstdRand0()
        inv = np.argsort(O.first_touch_numbering(lcd, nloc))
        v0 = np.zeros(nloc)
        for t in range(nloc):
            v0[inv[t]] = 0.0 if lcon[inv[t]] else gen.uniform01()
        act = ~lcon if variant == "mf" else np.ones(nloc, dtype=bool)
        out.append({"gl": gl, "M": Mx[np.ix_(act, act)], "act": act, "v0": v0[act], "diag_loc": diag_loc, "shift": shift})
    return out


def dense_selection(p, n_eig):
    """scipy's eigh and the oracle's `krylov` selection of problem p: (eigenvalues of the selected groups, their vectors on the
    active DoFs, all eigenvalues, relative gap g of the selection)."""
    w, V = sla.eigh(p["M"])
    vals, vecs = O._select_eigenvectors(w, V, min(n_eig, len(w)), "krylov", p["v0"])
    return vals, vecs, w, selection_gap(w, V, p["v0"], n_eig)


def selection_gap(w, V, v0, n_eig):
    """The smallest distance, relative to the largest eigenvalue, from a selected eigenvalue group to an eigenvalue outside it."""
    scale = max(abs(w[-1]), 1e-300)
    n, i, n_sel, g = len(w), 0, 0, np.inf
    while i < n and n_sel < n_eig:
        j = i + 1
        while j < n and abs(w[j] - w[i]) <= 1e-9 * scale:
            j += 1
        P = V[:, i:j]
        if np.linalg.norm(P @ (P.T @ v0)) > 1e-12 * np.linalg.norm(v0):
            n_sel += 1
            if i > 0:
                g = min(g, (w[i] - w[i - 1]) / scale)
            if j < n:
                g = min(g, (w[j] - w[j - 1]) / scale)
        i = j
    return g


def entry_bound(tolerance, g):
    """sin(theta) of a Ritz vector with residual tolerance * scale, plus the rounding of the dense checker, over the gap."""
    return (np.sqrt(2.0) * tolerance + 64 * EPS) / g


def lanczos_select(Mx, v0, n_eig, tolerance=1e-14, max_iterations=200, percent_overshoot=5, group=True):
    """The rule above.  Returns dict: values, vectors (columns, on the active DoFs), iterations, converged, breakdown.
    group=False: the lowest n_eig Ritz pairs as they come (what the rule must NOT do: see the (12, 6, 6) case)."""
    na = len(v0)
    v0n = np.linalg.norm(v0)
    if na == 0 or v0n == 0.0:
        return {"values": np.zeros(0), "vectors": np.zeros((na, 0)), "iterations": 0, "converged": True, "breakdown": False}
    ksteps = min(na, max_iterations)
    Q = np.zeros((na, ksteps))
    Q[:, 0] = v0 / v0n
    alpha, beta = [], []
    k_prev = 0
    for j in range(ksteps):
        w = Mx @ Q[:, j] - (beta[j - 1] * Q[:, j - 1] if j > 0 else 0.0)
        a = Q[:, j] @ w
        w = w - a * Q[:, j]
        for _ in range(2):
            w = w - Q[:, :j + 1] @ (Q[:, :j + 1].T @ w)
        b = np.linalg.norm(w)
        alpha.append(a)
        beta.append(b)
        k = j + 1
        theta, S = sla.eigh_tridiagonal(np.array(alpha), np.array(beta[:k - 1])) if k > 1 else (np.array(alpha), np.ones((1, 1)))
        scale = max(np.abs(theta).max(), 1e-300)
        broke = b <= BREAKDOWN * scale
        last = k == ksteps or broke
        if last or k == 1 or 100 * (k - k_prev) > percent_overshoot * k_prev:
            k_prev = k
            vals, coefs, ok = [], [], True
            i = 0
            while i < k and len(vals) < n_eig:
                e = i + 1
                while group and e < k and abs(theta[e] - theta[i]) <= 1e-9 * scale:
                    e += 1
                if np.any(b * np.abs(S[k - 1, i:e]) > tolerance * scale):
                    ok = False
                c = S[:, i:e] @ S[0, i:e]            # v0 / |v0| = q_1: its projection onto the Ritz vectors Q s_i
                if np.linalg.norm(c) > 1e-12:
                    vals.append(theta[i + np.argmax(np.abs(S[0, i:e]))])
                    coefs.append(c)
                i = e
            if (ok and len(vals) == n_eig) or last:
                vecs = np.zeros((na, len(vals)))
                for t, c in enumerate(coefs):
                    v = Q[:, :k] @ c
                    vecs[:, t] = v / np.linalg.norm(v)
                converged = (ok and len(vals) == n_eig) or broke or k == na
                return {"values": np.array(vals), "vectors": vecs, "iterations": k, "converged": converged, "breakdown": bool(broke)}
        Q[:, k] = w / b
    raise AssertionError("unreachable: the last step returns")
