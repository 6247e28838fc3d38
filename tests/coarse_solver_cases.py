"""Cases, references and the acceptance rule for the coarse solvers (HipSolver): the dense direct solve in its two forms -- the
explicit triangular inverses applied as two SpMV launches (up to 2048 rows) and dense_lu_solve_kernel (beyond) -- and the
Jacobi-preconditioned CG with its scalars on the device.  numpy and scipy only: test_coarse_solver_case_table.py shows without a
GPU that the table reaches what it names and that the bound notices planted errors; test_gpu_coarse_solvers.py runs the product.

Reference (direct cases): A x = b factored once with scipy.linalg.lu_factor, x refined with the residual b - A x formed in
np.longdouble until that residual no longer falls.  x_ref is the expected value of every comparison.

Restatement: the product's algorithm in float64 numpy -- dense_lu_factor's pivot rule (strict >: the first maximal row wins),
multipliers a * (1 / pivot), then either the substitution in the order of dense_lu_solve_kernel (column sweeps) or the explicit
L^-1 and U^-1 of dense_triangular_inverses applied as U^-1 (L^-1 (P b)).  It is never the expected value: it prices what this
algorithm costs in FP64 on the matrix at hand.  (Explicit inverses are not LAPACK's getrs: on the cases of
this table they cost three times its forward error on the saddle-point matrix and, with b over six decades, 10^4 times its
componentwise backward error on the rotated tridiagonal matrices -- a product with an inverse is not backward stable row by row.)  Where the product sums
sequentially the restatement uses numpy's matrix products -- the same terms in another order: the elimination in panels of NB
columns with one matrix product per panel, the rows of the inverses one matrix-vector product each.

Acceptance, assert_solution(got, case), in long double:
  (a) max|got - x_ref| / max|x_ref|
  (b) max_i |b - A got|_i / (|A| |got| + |b|)_i                               (componentwise backward error)
each at most FACTOR = 4 times max(the restatement's own value on the path the case takes, n 2^-53).  The factor covers the order
in which a row is summed: the device sums a row of a triangular inverse over the lanes of a wavefront (tree) in four parts, numpy
pairwise; nothing else in the arithmetic differs.

PCG: exactly n_iterations steps from zero with the recurrences, the slots and the zero-denominator guards of HipSolver::apply,
restated once in long double (the expected value) and once in float64 (the price); the same factor and floor.
"""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

LD = np.longdouble
U64 = 2.0 ** -53
FACTOR = 4
INVERSE_LIMIT = 2048          # kTriangularInverseLimit: up to here the explicit inverses, beyond dense_lu_solve_kernel
WIDE_ROWS_FROM = 512          # setup_direct: 64 lanes per row below, 256 lanes from here on
NB = 48                       # panel width of the restated elimination


def six_decades(rng, n):
    """seeded normal doubles spread over six signed decades (as fp32_reference / halo_reference.decade_input)"""
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)


# ---------------------------------------------------------------------------------------------------------------------------
# long double helpers
def ld_matvec(A, x):
    """A x in long double, A scipy CSR without empty rows (sequential sums per row)"""
    A = A.tocsr()
    assert (np.diff(A.indptr) > 0).all()
    return np.add.reduceat(A.data.astype(LD) * np.asarray(x, dtype=LD)[A.indices], A.indptr[:-1])


def reference_solution(A, b):
    """(x_ref, residual): lu_factor once, refinement with the long-double residual until it no longer falls"""
    lu = sla.lu_factor(A.toarray())
    bl = np.asarray(b, dtype=LD)
    x = sla.lu_solve(lu, b).astype(LD)
    best, best_norm = x, np.abs(bl - ld_matvec(A, x)).max()
    for _ in range(20):
        r = bl - ld_matvec(A, x)
        x = x + sla.lu_solve(lu, r.astype(np.float64)).astype(LD)
        norm = np.abs(bl - ld_matvec(A, x)).max()
        if not norm < best_norm:
            break
        best, best_norm = x, norm
    return best, bl - ld_matvec(A, best)


def errors(got, A, b, x_ref):
    """(a) and (b) of the module text, as floats (NaN in `got` gives NaN)"""
    g = np.asarray(got).astype(LD)
    forward = np.abs(g - x_ref).max() / np.abs(x_ref).max()
    mag = ld_matvec(abs(A), np.abs(g)) + np.abs(np.asarray(b, dtype=LD))
    backward = (np.abs(np.asarray(b, dtype=LD) - ld_matvec(A, g)) / mag).max()
    return float(forward), float(backward)


# ---------------------------------------------------------------------------------------------------------------------------
# the product's algorithm in float64
def restated_factor(A):
    """dense_lu_factor: (packed L\\U, perm, the row exchanges in order); perm[i] is the row of A that ended in position i"""
    a = np.array(A.toarray() if sp.issparse(A) else A, dtype=np.float64, order="C")
    n = a.shape[0]
    perm = np.arange(n)
    swaps = []
    for k0 in range(0, n, NB):
        k1 = min(k0 + NB, n)
        for k in range(k0, k1):
            piv = k + int(np.argmax(np.abs(a[k:, k])))              # argmax: the first maximal row
            if a[piv, k] == 0.0:
                raise ZeroDivisionError("singular matrix")
            if piv != k:
                a[[k, piv]] = a[[piv, k]]
                perm[[k, piv]] = perm[[piv, k]]
                swaps.append((k, piv))
            a[k + 1:, k] *= 1.0 / a[k, k]
            a[k + 1:, k + 1:k1] -= np.outer(a[k + 1:, k], a[k, k + 1:k1])
        for k in range(k0, k1):                                      # the panel's rows of U to the right of it
            a[k + 1:k1, k1:] -= np.outer(a[k + 1:k1, k], a[k, k1:])
        a[k1:, k1:] -= a[k1:, k0:k1] @ a[k0:k1, k1:]
    return a, perm, swaps


def substitute(lu, y, skip_division=None):
    """dense_lu_solve_kernel after y = b[perm]: column sweeps forward (unit L) and backward"""
    y = np.array(y, dtype=np.float64)
    n = len(y)
    for j in range(n - 1):
        y[j + 1:] -= lu[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):
        if j != skip_division:
            y[j] /= lu[j, j]
        y[:j] -= lu[:j, j] * y[j]
    return y


def restated_inverses(lu):
    """dense_triangular_inverses: L^-1 (unit diagonal) and U^-1, every column an independent substitution whose row i is
    -(L[i, j:i] . x[j:i]) resp. (delta_ij - U[i, i+1:j+1] . x[i+1:j+1]) / U[i, i]; here all columns of one row at once"""
    n = lu.shape[0]
    linv, uinv = np.eye(n), np.zeros((n, n))
    for i in range(1, n):
        linv[i, :i] = -(lu[i, :i] @ linv[:i, :i])
    for i in range(n - 1, -1, -1):
        uinv[i, i] = 1.0 / lu[i, i]
        if i + 1 < n:
            uinv[i, i + 1:] = -(lu[i, i + 1:] @ uinv[i + 1:, i + 1:]) / lu[i, i]
    return linv, uinv


def inverse_permutation(perm):
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return inv


def is_involution(perm):
    return bool((perm[perm] == np.arange(len(perm))).all())


def restatement(A, b):
    """lu, perm, swaps and the two applications x_substitution, x_inverse (the latter with its factors up to INVERSE_LIMIT
    rows only: beyond, the product has no such path)"""
    lu, perm, swaps = restated_factor(A)
    out = {"lu": lu, "perm": perm, "swaps": swaps, "x_substitution": substitute(lu, b[perm])}
    if len(b) <= INVERSE_LIMIT:
        linv, uinv = restated_inverses(lu)
        out.update(linv=linv, uinv=uinv, x_inverse=uinv @ (linv @ b[perm]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# acceptance
def path_of(n):
    return "inverse" if n <= INVERSE_LIMIT else "substitution"


def make_case(name, A, b, exact=False):
    """everything a test needs of one system: A (CSR), b, x_ref with its residual, the restatement's perm and its own errors on
    either path, the path the product takes, and the two bounds"""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    b = np.ascontiguousarray(b, dtype=np.float64)
    x_ref, residual = reference_solution(A, b)
    r = restatement(A, b)
    case = {"name": name, "A": A, "b": b, "n": n, "x_ref": x_ref, "residual": residual, "exact": exact, "path": path_of(n),
            "perm": r["perm"], "swaps": r["swaps"], "restated": r, "restated_errors": {}}
    for path in ("substitution", "inverse"):
        if "x_" + path in r:
            case["restated_errors"][path] = errors(r["x_" + path], A, b, x_ref)
    own = case["restated_errors"][case["path"]]
    case["bounds"] = tuple(FACTOR * max(v, n * U64) for v in own)
    return case


def measure(got, case):
    """the two errors of `got` as fractions of their bounds"""
    e = errors(got, case["A"], case["b"], case["x_ref"])
    return tuple(v / bound for v, bound in zip(e, case["bounds"]))


def assert_solution(got, case):
    """the one acceptance rule of the direct solvers; returns the larger of the two fractions of the bound"""
    forward, backward = measure(got, case)
    assert forward <= 1.0, f"{case['name']}: max|x - x_ref| / max|x_ref| is {forward:.3g} of its bound {case['bounds'][0]:.3g}"
    assert backward <= 1.0, f"{case['name']}: the componentwise backward error is {backward:.3g} of its bound {case['bounds'][1]:.3g}"
    return max(forward, backward)


# ---------------------------------------------------------------------------------------------------------------------------
# the direct cases
def tridiag(n):
    return sp.diags([-np.ones(n - 1), 4 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()


def permutations_of(n):
    """name -> q, where row i of the case matrix is row q[i] of the unpermuted one (the pivoting then finds perm = q^-1)"""
    rng = np.random.default_rng([11, n])
    out = {"identity": np.arange(n)}
    if n >= 2:
        t = np.arange(n)
        t[[0, n - 1]] = t[[n - 1, 0]]
        out["transposition"] = t
    if n >= 3:
        out["shift1"] = (np.arange(n) + 1) % n
        r = np.array([0, 2, 1])                                      # n = 3: with a fixed point there is nothing but a transposition
        while n > 3 and (len(r) != n or (r[r] == np.arange(n)).all()):
            r = np.concatenate([[0], 1 + rng.permutation(n - 1)])
        out["random_fixed_point"] = r
    if n > 8:
        out["shift7"] = (np.arange(n) + 7) % n
    return out


def signed_powers_of_two(rng, n, lo=-8, hi=8):
    return rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(lo, hi + 1, n)


EXACT_SIZES = (1, 2, 3, 64, 65, 513)
ROTATED_SIZES = (65, 511, 512, 513, 2048, 2049)
GAUSSIAN_SIZES = (3, 17, 65, 300, 2049)
ROTATION = 7
SADDLE_K, SADDLE_B = 300, 40
TRIANGULAR_N = 65


def exact_names():
    return [f"exact_{kind}_{n}" for n in EXACT_SIZES for kind in permutations_of(n)]


def direct_names():
    return (exact_names() + [f"triangular_{kind}_{TRIANGULAR_N}" for kind in ("shift7", "random_fixed_point")] +
            [f"rotated_{n}" for n in ROTATED_SIZES] + [f"gaussian_{n}" for n in GAUSSIAN_SIZES] + ["saddle", "tie", "control_30"])


def _build(name):
    """(A, b, exact)"""
    parts = name.split("_")
    family = parts[0]
    if family == "exact":                                            # A = P D
        n, kind = int(parts[-1]), "_".join(parts[1:-1])
        rng = np.random.default_rng([1, n, sorted(permutations_of(n)).index(kind)])
        q = permutations_of(n)[kind]
        A = sp.diags(signed_powers_of_two(rng, n)).tocsr()[q]
        return A, six_decades(rng, n), True
    if family == "triangular":
        # A = P L0 D with L0 = [[I, 0], [C, I]], C dense with entries +-2^-k (k = 1 .. 4), D signed powers of two; column k of
        # L0 D is largest, strictly, in row k, and eliminating it leaves the rest of L0 D as it is (U = D): L = L0, every
        # multiplier and both inverses (L0^-1 = [[I, 0], [-C, I]]) exact.  b = A x with integer x below 2^10: every partial sum
        # of either path is a multiple of 2^-12 below 2^30, so the solve is exact in any order
        n, kind = int(parts[-1]), "_".join(parts[1:-1])
        rng = np.random.default_rng([2, n, len(kind)])
        h = n // 2 + 1
        L0 = np.eye(n)
        L0[h:, :h] = rng.choice([-1.0, 1.0], (n - h, h)) * 2.0 ** -rng.integers(1, 5, (n - h, h))
        d = signed_powers_of_two(rng, n)
        q = permutations_of(n)[kind]
        A = sp.csr_matrix((L0 * d[None, :])[q])
        x = rng.integers(-1000, 1001, n).astype(np.float64)
        x[x == 0] = 1.0
        return A, A @ x, True
    rng = np.random.default_rng([3, len(name), sum(name.encode())])
    if family == "rotated":                                          # the rows of tridiag(-1, 4, -1) rotated: every row moves
        n = int(parts[1])
        A = tridiag(n)[(np.arange(n) + ROTATION) % n]
    elif family == "gaussian":
        n = int(parts[1])
        D = rng.standard_normal((n, n))
        while n == 3 and is_involution(restated_factor(D)[1]):       # (drawn again until the pivoting is no mere exchange)
            D = rng.standard_normal((n, n))
        A = sp.csr_matrix(D)
    elif family == "saddle":                                         # [[K, B^T], [B, 0]], the zero block not stored
        B = sp.csr_matrix(rng.standard_normal((SADDLE_B, SADDLE_K)))
        A = sp.bmat([[tridiag(SADDLE_K), B.T], [B, None]], format="csr")
        n = A.shape[0]
    elif family == "tie":                                            # rows 3 and 9 share the largest |a| of the first column
        n = 17
        D = rng.standard_normal((n, n))
        D[3, 0], D[9, 0] = -4.5, 4.5
        A = sp.csr_matrix(D)
    elif family == "control":                                        # test_direct_solvers_on_the_reference_tridiagonal_system
        n = 30
        A = tridiag(n)
    else:
        raise KeyError(name)
    return A, A @ six_decades(rng, n), False


@functools.lru_cache(maxsize=None)
def _inputs(name):
    A, b, exact = _build(name)
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A, np.ascontiguousarray(b, dtype=np.float64), exact


@functools.lru_cache(maxsize=None)
def _priced(name):
    A, b, exact = _inputs(name)
    return make_case(name, A, b, exact)


def direct_case(name, priced=True):
    """the case of that name, computed once and shared (treat it as read-only); priced=False: A and b alone"""
    if priced:
        return _priced(name)
    A, b, exact = _inputs(name)
    return {"name": name, "A": A, "b": b, "n": A.shape[0], "exact": exact, "path": path_of(A.shape[0])}


# ---------------------------------------------------------------------------------------------------------------------------
# Jacobi-preconditioned CG
PCG_SIZES = (1, 63, 64, 65, 1000, 300001)
PCG_ITERATIONS = (0, 1, 2, 5, 12)
PCG_KINDS = ("scaled_tridiagonal", "diagonal")


@functools.lru_cache(maxsize=None)
def pcg_system(kind, n):
    """(lower, diagonal, upper, b) in float64.  scaled_tridiagonal: D^1/2 tridiag(-1, 4, -1) D^1/2 with a positive diagonal D
    over two decades (the Jacobi scaling matters); diagonal: positive powers of two (D^-1 b and every product with
    it exact).  b over six signed decades."""
    rng = np.random.default_rng([4, PCG_KINDS.index(kind), n])
    if kind == "diagonal":
        d = 2.0 ** rng.integers(-8, 9, n)
        off = np.zeros(max(n - 1, 0))
        return off, d, off.copy(), six_decades(rng, n)
    s = np.sqrt(10.0 ** rng.uniform(-1, 1, n))
    off = -(s[:-1] * s[1:])
    return off, 4.0 * s * s, off.copy(), six_decades(rng, n)


def pcg_matrix(kind, n):
    lo, di, up, _ = pcg_system(kind, n)
    if kind == "diagonal":
        return sp.diags(di).tocsr()
    return sp.diags([lo, di, up], [-1, 0, 1]).tocsr()


def pcg_restated(kind, n, n_iterations, dtype, b=None, alternate=True, guards=True):
    """HipSolver::apply, solver.type pcg: x = 0, r = b, z = D^-1 r, p = z, rz in slot 0; per step Ap, pAp in slot 2,
    alpha = rz[cur] / pAp (0 where pAp == 0), x += alpha p, r -= alpha Ap, z = D^-1 r, rz in slot nxt, beta = rz[nxt] / rz[cur]
    (0 where rz[cur] == 0), p = z + beta p; cur = it & 1.  alternate=False, guards=False: the mutants of the bite test."""
    lo, di, up, b0 = (np.asarray(v, dtype=dtype) for v in pcg_system(kind, n))
    b = b0 if b is None else np.asarray(b, dtype=dtype)
    one, zero = dtype(1), dtype(0)

    def matvec(v):
        y = di * v
        y[1:] += lo * v[:-1]
        y[:-1] += up * v[1:]
        return y

    def ratio(num, den):
        if guards:
            return num / den if den != 0 else zero
        with np.errstate(all="ignore"):
            return np.divide(num, den)

    dinv = np.where(di != 0, one / di, zero)
    x = np.zeros(n, dtype=dtype)
    r = b.copy()
    z = dinv * r
    p = z.copy()
    scal = [zero] * 3
    scal[0] = np.dot(r, z)
    for it in range(n_iterations):
        cur = (it & 1) if alternate else 0
        nxt = cur ^ 1
        ap = matvec(p)
        scal[2] = np.dot(p, ap)
        alpha = ratio(scal[cur], scal[2])
        x = x + alpha * p
        r = r - alpha * ap
        z = dinv * r
        scal[nxt] = np.dot(r, z)
        beta = ratio(scal[nxt], scal[cur])
        p = z + beta * p
    return x


@functools.lru_cache(maxsize=None)
def pcg_case(kind, n, n_iterations):
    """x_ref: the long-double restatement; bound: FACTOR max(the float64 restatement's distance from it, n 2^-53), relative
    to max|x_ref|"""
    x_ref = pcg_restated(kind, n, n_iterations, LD)
    x64 = pcg_restated(kind, n, n_iterations, np.float64)
    scale = np.abs(x_ref).max()
    own = float(np.abs(x64.astype(LD) - x_ref).max() / scale) if scale > 0 else 0.0
    return {"name": f"pcg_{kind}_{n}_{n_iterations}", "kind": kind, "n": n, "n_iterations": n_iterations, "b": pcg_system(kind, n)[3],
            "x_ref": x_ref, "x64": x64, "restated_error": own, "bound": FACTOR * max(own, n * U64)}


def assert_pcg(got, case):
    """the acceptance rule of the PCG cases; returns the error as a fraction of the bound.  A zero x_ref (no iteration) admits
    zeros only."""
    g = np.asarray(got).astype(LD)
    scale = np.abs(case["x_ref"]).max()
    if scale == 0:
        assert (g == 0).all(), f"{case['name']}: the expected solution is zero"
        return 0.0
    ratio = float(np.abs(g - case["x_ref"]).max() / scale) / case["bound"]
    assert ratio <= 1.0, f"{case['name']}: max|x - x_ref| / max|x_ref| is {ratio:.3g} of its bound {case['bound']:.3g}"
    return ratio
