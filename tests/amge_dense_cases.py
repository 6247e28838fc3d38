"""Cases of the dense agglomerate eigensolver of the restrictor setup (mfmg_amd/csrc/amge_device.hip) for
test_amge_dense_case_table.py (no GPU) and test_gpu_amge_dense.py: the case table, the constants of the launch that the cases
straddle, the references and the checks per agglomerate.  The problems (M, v0, act, diag_loc, shift) are those of
amge_lanczos_rule.agglomerate_problems and the gap is its selection_gap; nothing of them is restated here.

A result, whoever computed it, is per agglomerate: n_vec, weights [n_eig, stride] (diag_loc * vector on the local nodes, x fastest,
stride 27 or 64) and, where the implementation reports them, eigenvalues [n_eig].  The references are scipy's eigh of the reference M
with the oracle's _select_eigenvectors, and the CPU path of the same rule (host_build_restrictor), whose rows are weights divided by
the global diagonal.

Checks per agglomerate (`check_agglomerate`), na the number of active DoFs, eps = 2^-52, scale = the largest |eigenvalue| of M:
  count         n_vec is the reference's: the groups selected (krylov), min(n_eig, na) (lapack).
  zeros         every weight outside (slot < n_vec, local node < nloc, active node) is exactly 0.0, every eigenvalue slot >= n_vec too.
  vector        krylov: |weights - diag_loc v_ref| <= K_DENSE na eps max|diag_loc| / g entry by entry, g the selection_gap (taken
                as 1 where nothing lies outside the selection: a gap relative to the largest eigenvalue is at most 1).
  norm, orthogonality, residual, completeness
                lapack, y_e = weights_e / diag_loc on the active DoFs: | |y_e| - 1 |, |y_e . y_f|, |M y_e - lambda_e y_e|_2 and,
                with all vectors requested, max |sum_e y_e y_e^T - I|, each <= K_DENSE na eps scale.
  eigenvalue    each reported value within K_DENSE na eps scale of a member of its group of the UNSHIFTED problem (krylov: any
                member of the e-th selected group; lapack: the e-th eigenvalue).
  same rule     (`check_against_cpu_rows`) weights / global diagonal against the rows of the CPU path's R for the agglomerate, entry
                by entry within 1e-12 max|R|, same number of rows, columns the sorted DoFs of the agglomerate.

K_DENSE covers the rounding of a converged cyclic Jacobi and that of eigh.  It is measured, on the CPU, with `jacobi_rule` below (the
numpy restatement of symmetric_eigen in amge_structured.cpp) run through these checks over the whole shape table
(`python tests/amge_dense_cases.py`, with tests/ and oracle/ on the path; three minutes): worst ratio met times 8 (a sweep more or less; the wavefront's summation order in the stopping
test), rounded up to a power of two."""
import functools

import numpy as np
import scipy.linalg as sla

import amge_lanczos_rule as RL
import mfmg_oracle as O

EPS = RL.EPS
# measured with jacobi_rule over SHAPE_CASES x VARIANTS x SELECTIONS x N_EIGS (and the 27-vector case): worst ratio
# MEASURED_WORST (see measure_k_dense), times 8, rounded up to a power of two
MEASURED_WORST = 3.041             # completeness, (8, 8, 8) / (2, 2, 2) constant device lapack n_eig 27 agglomerate 42;
                                    # eigenvalue 2.73, norm 2.61, orthogonality 2.03, residual 1.51, vector 0.49
K_DENSE = 32.0
CPU_ROW_TOL = 1e-12                 # of max|R|, as test_restrictor_eigenproblems_on_device uses

# ---- the constants of the launch, each with the line of amge_device.hip it restates ----
GRID_CAP = 256 * 16                 # :501  blocks = min((n_agg + wpb - 1) / wpb, 256 * 16)
WAVES_PER_BLOCK = {27: 4, 64: 1}    # :499  wpb = nmax == 27 ? 4 : 1
SHARING_MIN = 64                    # :427  ... && n_all >= 64
GROUP_RTOL = 1e-9                   # :271  fabs(w[i1] - w[i0]) <= 1e-9 * scale
PROJECTION_RTOL = 1e-12             # :289  pn > 1e-12 * v0n

VARIANTS = ("mf", "device", "host")
SELECTIONS = ("krylov", "lapack")
N_EIGS = (1, 2, 4, 8)
N_EIG_REF = 8                       # one reference of 8 vectors serves 1, 2, 4 and 8: both selections take them in ascending order
N_EIG_ALL = 27                      # all vectors of a full 2x2x2 agglomerate: (case, variant, selection) that also run with it
COMPLETE = [(((2, 2, 2), (2, 2, 2), "linear"), "device", "lapack"),      # 26 of 27 nodes constrained: M is diagonal, V = I
            (((8, 8, 8), (2, 2, 2), "constant"), "device", "lapack")]    # interior agglomerates: the full Neumann matrix

# (cells, agglomerate, material)
SHAPE_CASES = [
    ((2, 2, 2), (2, 2, 2), "linear"),            # one agglomerate; mf: a single active DoF, n_eig exceeds it
    ((3, 3, 3), (2, 2, 2), "linear"),            # clipped 1-cell agglomerates; n_vec differs between agglomerates
    ((4, 4, 4), (1, 1, 1), "linear"),            # sides of 1; exactly 64 agglomerates
    ((7, 5, 4), (3, 2, 2), "discontinuous"),     # 36 nodes in the <64> kernel; unequal sides
    ((7, 7, 3), (6, 2, 2), "linear"),            # 63 nodes
    ((8, 4, 2), (7, 3, 1), "linear"),            # 64 nodes from a non-cube
    ((6, 6, 6), (3, 3, 3), "constant"),          # 64 nodes; exactly degenerate groups in every variant
    ((8, 8, 8), (2, 2, 2), "constant"),          # degenerate groups; NMAX 27 full
    ((7, 7, 7), (3, 3, 3), "linear_x"),          # the near-threshold gap
    ((14, 14), (7, 7), "linear"),                # 2-D, 64 nodes
    ((9, 7), (5, 4), "discontinuous"),           # 2-D, 30 nodes in the <64> kernel
    ((12, 10), (2, 2), "constant"),              # 2-D small
    ((5, 9), (1, 3), "linear"),                  # 2-D unequal with a side of 1
]
NEAR_THRESHOLD = [((7, 7, 7), (3, 3, 3), "linear_x")]      # krylov gaps below 1e-6 on purpose (still 30 x the grouping threshold)

# launch cases: krylov, n_eig 2, variants mf and device
STRIDE_CASES = [                                 # constant, MFMG_AMGE_MEMO=0: every agglomerate solved; reference by class
    ((52, 52, 52), (2, 2, 2), "constant"),       # 17576 solves > 16384: a second slot per wavefront in the <27> kernel
    ((51, 51, 48), (3, 3, 3), "constant"),       # 4624 solves > 4096: the <64> kernel
    ((258, 256), (2, 2), "constant"),            # 16512 solves: the 2-D stride
]
STRIDE_GIVE_UP = ((52, 52, 52), (2, 2, 2), "linear")      # memo default: the sharing pass gives up, 17576 distinct problems stride
SHARING_CASES = [                                # (case, what restrictor_eigensolver_info()["solves"] is against agglomerates)
    (((6, 6, 14), (2, 2, 2), "constant"), "equal"),        # 63 agglomerates: below the threshold, no pass
    (((8, 8, 8), (2, 2, 2), "constant"), "less"),          # 64: shared
    (((12, 10, 6), (2, 2, 2), "discontinuous"), None),     # shares in patterns, whatever the classes allow
    (((8, 8, 8), (2, 2, 2), "linear"), "equal"),           # gives up (more than half of the keys distinct: the early break)
]
LAUNCH_VARIANTS = ("mf", "device")
LAUNCH_N_EIG = 2

case_id = RL.case_id


def n_eigs_of(case, variant, selection):
    return N_EIGS + ((N_EIG_ALL,) if (case, variant, selection) in COMPLETE else ())


def params_of(case, n_eig, variant, selection, where="device"):
    return {"eigensolver": {"number of eigenvectors": n_eig, "variant": variant, "selection": selection},
            "agglomeration": dict(zip(("nx", "ny", "nz"), case[1])), "restrictor": {"eigensolver": where},
            "is preconditioner": False, "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}}


# ---- what the host code decides from the shapes, restated ----
def counts(case):
    return [-(-n // a) for n, a in zip(case[0], case[1])]


def n_agglomerates(case):
    return int(np.prod(counts(case)))


def nmax_of(case):
    """:478  nmax = nloc <= 27 ? 27 : 64, nloc from the unclipped agglomerate"""
    nloc = int(np.prod([a + 1 for a in case[1]]))
    assert nloc <= 64
    return 27 if nloc <= 27 else 64


def slots_per_wave(case, solves=None):
    """The most agglomerates one wavefront of the eigen kernel takes in the launch."""
    solves = n_agglomerates(case) if solves is None else solves
    wpb = WAVES_PER_BLOCK[nmax_of(case)]
    blocks = min(-(-solves // wpb), GRID_CAP)
    return -(-solves // (blocks * wpb))


def clipped_shapes(case):
    """ln (cells per axis) of every agglomerate, x fastest: int array [A, dim]"""
    per_axis = [np.minimum(a, n - a * np.arange(c)) for n, a, c in zip(case[0], case[1], counts(case))]
    grids = np.meshgrid(*per_axis, indexing="ij")
    dim = len(per_axis)
    return np.stack([np.transpose(g, tuple(reversed(range(dim)))).ravel() for g in grids], axis=1)


def class_ids(case):
    """For a coefficient that is the same in every cell: the class of every agglomerate, keyed per axis by (clipped side, touches
    the near boundary, touches the far boundary) -- which fixes the clipped shape and the constraint flags of the nodes, so the
    whole eigenproblem.  Returns (class id [A], first agglomerate of every class)."""
    assert case[2] == "constant"
    key = np.zeros(n_agglomerates(case), dtype=np.int64)
    per_axis = []
    for n, a, c in zip(case[0], case[1], counts(case)):
        lo = a * np.arange(c)
        ln = np.minimum(a, n - lo)
        per_axis.append(ln * 4 + (lo == 0) * 2 + (lo + ln == n))
    grids = np.meshgrid(*per_axis, indexing="ij")
    dim = len(per_axis)
    for g in grids:
        key = key * 1024 + np.transpose(g, tuple(reversed(range(dim)))).ravel()
    _, first, ids = np.unique(key, return_index=True, return_inverse=True)
    return ids, first


def give_up_subset(case):
    """The listed subset of the linear stride case: first and last 64, the slots around the grid's first wrap, every 97th."""
    A = n_agglomerates(case)
    wrap = GRID_CAP * WAVES_PER_BLOCK[nmax_of(case)]
    picks = set(range(64)) | set(range(A - 64, A)) | set(range(wrap - 4, wrap + 7)) | set(range(0, A, 97))
    return sorted(picks)


# ---- references ----
@functools.lru_cache(maxsize=None)
def problems(case, variant):
    """Every agglomerate of a case with its dense eigen-decomposition (computed once, left unchanged)."""
    return tuple(with_eigh(p) for p in RL.agglomerate_problems(case[0], case[1], case[2], variant))


def problems_of(case, variant, subset):
    return [with_eigh(p) for p in RL.agglomerate_problems(case[0], case[1], case[2], variant, subset=subset)]


def with_eigh(p):
    p = dict(p)
    p["w"], p["V"] = sla.eigh(p["M"])
    p["na"], p["nloc"] = len(p["v0"]), len(p["gl"])
    p["scale"] = max(np.abs(p["w"]).max(), 1e-300)
    return p


def selected_groups(p, n_eig, rtol=GROUP_RTOL):
    """[(first, end)] in the ascending eigenvalues of the groups the krylov rule selects."""
    w, V, v0 = p["w"], p["V"], p["v0"]
    scale = max(abs(w[-1]), 1e-300)
    out, i = [], 0
    while i < len(w) and len(out) < n_eig:
        j = i + 1
        while j < len(w) and abs(w[j] - w[i]) <= rtol * scale:
            j += 1
        P = V[:, i:j]
        if np.linalg.norm(P @ (P.T @ v0)) > PROJECTION_RTOL * np.linalg.norm(v0):
            out.append((i, j))
        i = j
    return out


def expected(p, selection, n_eig):
    """The reference for one agglomerate: n_vec; krylov: vectors [na, n_vec] on the active DoFs, groups, gap."""
    ne = min(n_eig, p["na"])
    if selection == "lapack":
        return {"n_vec": ne}
    _, vecs = O._select_eigenvectors(p["w"], p["V"], ne, "krylov", p["v0"])
    groups = selected_groups(p, ne)
    assert len(groups) == vecs.shape[1]
    return {"n_vec": vecs.shape[1], "vecs": vecs, "groups": groups, "gap": min(RL.selection_gap(p["w"], p["V"], p["v0"], ne), 1.0)}


def reference_result(p, selection, n_eig, stride):
    """A result in the layout of amge_eigen computed from eigh: (n_vec, weights [n_eig, stride], eigenvalues [n_eig]).  Under lapack
    the vectors are eigh's columns, one basis of many inside a degenerate group."""
    ex = expected(p, selection, n_eig)
    W, ev = np.zeros((n_eig, stride)), np.zeros(n_eig)
    act = np.flatnonzero(p["act"])
    for e in range(ex["n_vec"]):
        if selection == "lapack":
            W[e, act], ev[e] = p["diag_loc"][act] * p["V"][:, e], p["w"][e] - p["shift"]
        else:
            W[e, act], ev[e] = p["diag_loc"][act] * ex["vecs"][:, e], p["w"][ex["groups"][e][0]] - p["shift"]
    return ex["n_vec"], W, ev


def jacobi_rule(M):
    """symmetric_eigen of amge_structured.cpp in numpy: cyclic Jacobi, rotations in (p, q) row order applied to the columns, then
    the rows, then the vectors; stops when the off-diagonal mass is 1e-32 of the total; ascending, ties in index order.
    Returns (w, V) with the vectors as columns."""
    A = np.array(M, dtype=np.float64)
    n = A.shape[0]
    V = np.eye(n)
    for _ in range(64):
        d = np.diag(A)
        off = (np.triu(A, 1) ** 2).sum()
        if off <= 1e-32 * ((d * d).sum() + off) or off == 0.0:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if abs(apq) < 1e-300:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                ap, aq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * ap - s * aq, s * ap + c * aq
                ap, aq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * ap - s * aq, s * ap + c * aq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
    order = np.argsort(np.diag(A), kind="stable")
    return np.diag(A)[order].copy(), V[:, order].copy()


def jacobi_result(p, selection, n_eig, stride):
    """The rule of the device kernel and the CPU path in numpy, in the layout of amge_eigen (eigenvalues of the unshifted problem)."""
    if "jw" not in p:
        p["jw"], p["jV"] = jacobi_rule(p["M"])
    w, V, v0, na = p["jw"], p["jV"], p["v0"], p["na"]
    W, ev = np.zeros((n_eig, stride)), np.zeros(n_eig)
    act = np.flatnonzero(p["act"])
    dl = p["diag_loc"][act]
    n_sel = 0
    if selection == "lapack":
        n_sel = min(n_eig, na)
        for e in range(n_sel):
            W[e, act], ev[e] = dl * V[:, e], w[e] - p["shift"]
        return n_sel, W, ev
    scale = max(abs(w[-1]), 1e-300)
    i = 0
    while i < na and n_sel < n_eig:
        j = i + 1
        while j < na and abs(w[j] - w[i]) <= GROUP_RTOL * scale:
            j += 1
        proj = V[:, i:j] @ (V[:, i:j].T @ v0)
        pn = np.linalg.norm(proj)
        if pn > PROJECTION_RTOL * np.linalg.norm(v0):
            W[n_sel, act], ev[n_sel] = dl * (proj / pn), w[i] - p["shift"]
            n_sel += 1
        i = j
    return n_sel, W, ev


# ---- the checks ----
class Worst(dict):
    """check name -> (largest ratio to na eps <magnitude>, where)"""

    def record(self, name, ratio, where):
        if ratio >= self.get(name, (-1.0, None))[0]:
            self[name] = (float(ratio), where)

    def largest(self):
        return max((r for r, _ in self.values()), default=0.0)

    def merge(self, other):
        for name, (ratio, where) in other.items():
            self.record(name, ratio, where)


def check_agglomerate(p, selection, n_eig, n_vec, weights, eigenvalues=None, k=None, what="", worst=None, complete=False):
    """All the checks of one agglomerate that need no second implementation; AssertionError names the check that failed.
    weights [>= n_eig, stride], eigenvalues [>= n_eig] or None where the implementation reports none."""
    k = K_DENSE if k is None else k
    worst = Worst() if worst is None else worst
    ex = expected(p, selection, n_eig)
    na, nloc, act = p["na"], p["nloc"], np.flatnonzero(p["act"])
    unit = na * EPS
    W = np.asarray(weights)[:n_eig]
    assert int(n_vec) == ex["n_vec"], f"{what}: count: n_vec {int(n_vec)}, reference {ex['n_vec']}"
    nv = ex["n_vec"]
    allowed = np.zeros(W.shape, dtype=bool)
    allowed[:nv, act] = True
    assert np.isfinite(W).all(), f"{what}: zeros: a weight is not finite"
    assert (W[~allowed] == 0.0).all(), \
        f"{what}: zeros: {int((W[~allowed] != 0.0).sum())} nonzero weights outside (slot < {nv}, node < {nloc}, active)"
    if eigenvalues is not None:
        ev = np.asarray(eigenvalues)[:n_eig]
        assert (ev[nv:] == 0.0).all(), f"{what}: zeros: an eigenvalue beyond slot {nv} is not 0"

    def within(name, err, magnitude):
        ratio = err / (unit * magnitude)
        worst.record(name, ratio, what)
        assert ratio <= k, f"{what}: {name}: {err:.3g} is {ratio:.3g} na eps x magnitude, beyond K_DENSE = {k:g}"

    dl = p["diag_loc"][act]
    if selection == "krylov":
        for e in range(nv):
            within("vector", np.abs(W[e, act] - dl * ex["vecs"][:, e]).max(), np.abs(p["diag_loc"]).max() / ex["gap"])
    else:
        Y = (W[:nv, act] / dl).T                                         # columns y_e
        G = Y.T @ Y
        for e in range(nv):
            within("norm", abs(np.sqrt(G[e, e]) - 1.0), p["scale"])
            within("residual", np.linalg.norm(p["M"] @ Y[:, e] - p["w"][e] * Y[:, e]), p["scale"])
        if nv > 1:
            within("orthogonality", np.abs(G - np.diag(np.diag(G))).max(), p["scale"])
        if complete and nv == na:
            within("completeness", np.abs(Y @ Y.T - np.eye(na)).max(), p["scale"])
    if eigenvalues is not None:
        for e in range(nv):
            members = p["w"][slice(*ex["groups"][e])] if selection == "krylov" else p["w"][e:e + 1]
            within("eigenvalue", np.abs(ev[e] - (members - p["shift"])).min(), p["scale"])
    return worst


def global_diagonal(case, variant):
    mesh = O.StructuredMesh(case[0])
    coef = O.coefficient_table(mesh, case[2])
    return O.MatrixFreeLaplace(mesh, coef).diagonal() if variant == "mf" else O.assemble_csr(mesh, coef).diagonal()


def cpu_rows(R, probs, selection, n_eig_of_R):
    """The CPU path's R (n_eig_of_R vectors asked) cut per agglomerate: (first row [A + 1], R as sorted CSR, max|R|)."""
    R = R.tocsr()
    R.sort_indices()
    n_vec = np.array([expected(p, selection, n_eig_of_R)["n_vec"] for p in probs])
    first = np.concatenate([[0], np.cumsum(n_vec)])
    assert first[-1] == R.shape[0], f"the CPU path gives {R.shape[0]} rows, the reference counts {first[-1]}"
    return first, R, np.abs(R.data).max()


def cpu_weights(p, rows, a, global_diag, n_eig, stride):
    """(n_vec, weights [n_eig, stride]) of agglomerate a as the CPU path's R holds them: rows times the global diagonal."""
    first, R, _ = rows
    nv = min(n_eig, first[a + 1] - first[a])
    W = np.zeros((n_eig, stride))
    for e in range(nv):
        r = first[a] + e
        assert np.array_equal(R.indices[R.indptr[r]:R.indptr[r + 1]], np.sort(p["gl"])), f"agglomerate {a}: pattern of row {r}"
        W[e, :p["nloc"]] = R[r, p["gl"]].toarray().ravel() * global_diag[p["gl"]]
    return nv, W


def check_against_cpu_rows(p, rows, a, global_diag, n_eig, n_vec, weights, what="", worst=None):
    """same rule: the weights over the global diagonal against the rows of the CPU path's R for agglomerate a."""
    first, R, rmax = rows
    nv = min(n_eig, first[a + 1] - first[a])
    assert int(n_vec) == nv, f"{what}: same rule: n_vec {int(n_vec)}, the CPU path has {nv} rows"
    order = np.argsort(p["gl"], kind="stable")
    for e in range(nv):
        r = first[a] + e
        lo, hi = R.indptr[r], R.indptr[r + 1]
        assert np.array_equal(R.indices[lo:hi], p["gl"][order]), f"{what}: same rule: pattern of row {e}"
        err = np.abs(np.asarray(weights)[e, :p["nloc"]][order] / global_diag[p["gl"][order]] - R.data[lo:hi]).max()
        if worst is not None:
            worst.record("same rule", err / (CPU_ROW_TOL * rmax), what)
        assert err <= CPU_ROW_TOL * rmax, f"{what}: same rule: row {e} differs by {err:.3g}, beyond 1e-12 max|R| = {CPU_ROW_TOL * rmax:.3g}"


def combos():
    """Every (case, variant, selection) of the shape table."""
    return [(c, v, s) for c in SHAPE_CASES for v in VARIANTS for s in SELECTIONS]


def measure_k_dense():
    """jacobi_rule through the checks over the whole table; prints the worst ratio per check."""
    worst = Worst()
    for case in SHAPE_CASES:
        stride = nmax_of(case)
        for variant in VARIANTS:
            for a, p in enumerate(problems(case, variant)):
                for selection in SELECTIONS:
                    for n_eig in n_eigs_of(case, variant, selection):
                        nv, W, ev = jacobi_result(p, selection, n_eig, stride)
                        check_agglomerate(p, selection, n_eig, nv, W, ev, k=np.inf, worst=worst, complete=n_eig == N_EIG_ALL,
                                          what=f"{case_id(case)} {variant} {selection} n_eig {n_eig} agglomerate {a}")
        print(case_id(case), {n: f"{r:.3g}" for n, (r, _) in worst.items()}, flush=True)
    for name, (ratio, where) in worst.items():
        print(f"{name}: worst ratio {ratio:.4g} at {where}")
    print(f"worst {worst.largest():.4g}; times 8 = {8 * worst.largest():.4g}; K_DENSE = {2.0 ** np.ceil(np.log2(8 * worst.largest())):g}")


if __name__ == "__main__":
    measure_k_dense()
