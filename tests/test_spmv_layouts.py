"""Every SpMV layout of SparseMatrixDevice, every fused epilogue and the edge shapes of the lists, against long double.

CASES is one table.  A case names a generated matrix and a list of variants of it (kernel switches); every variant says
which form SparseMatrixDevice.form() must report -- the record the launch itself branches on --, and the GPU test
asserts that form before it looks at a number, so that a later change of a threshold cannot turn a case into a test of
plain CSR.  Then, per variant and for all seven modes of mfmg_hip_csr_launch (rectangular matrices: the five modes
that do not read x by row; modes 2 and 3 are rejected for them, which is asserted):

  * inputs: standard_normal scaled per entry by 10 ** uniform(-3, 3), alpha and beta of both signs, dinv from the true
    diagonal; out pre-filled with NaN in the modes that do not read it, and every entry must come back finite;
  * reference: per entry in np.longdouble from the CSR arrays (np.add.reduceat over the entry products) with the
    matching magnitude sum;
  * bound, derived and not measured: u = 2^-53, k = entries of the row + 6, gamma_k = k u / (1 - k u),
    |got - ref| <= gamma_k * mag with mag = |A||x| (mode 0), + |b| (1), |x| + |beta||d|(|A||x| + |b|) (2),
    |x| + |alpha|(|x| + |x_prev|) + |beta||d|(|A||x| + |b|) (3), |out_0| + |A||x| (4, 5), |A||x| + |beta||d||b| (6).
    It holds for any summation order, with or without fma contraction; float planes hold their values exactly;
  * class kernels, mode 0 only: x = 1 on the boundary shell of the grid and 0 inside, and the reverse (contributions
    read at clamped positions); for a rectangular matrix the shell is that of its column grid;
  * bit for bit: a repeated launch; for C = 2 node kernels the launch with b, dinv, x_prev, out at an 8-byte but not
    16-byte aligned address (form()["pairs"] == 0, the row-by-row half of store_node) against the aligned one.  x stays
    16-byte aligned: the node kernels gather it as double2 whatever the alignment;
  * every variant against the first one of its case within 2 gamma_k mag.

Three tests need no GPU: the table covers REQUIRED_FORMS; scipy's float64 product lies within the bound of the
long-double reference for every generator and mode; the generators produce what they claim."""
import zlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import mfmg_amd as M
from mfmg_amd import lib as L

U = 2.0 ** -53
MODES = (L.CSR_APPLY, L.CSR_RESIDUAL, L.CSR_FIRST, L.CSR_NEXT, L.CSR_SUBTRACT, L.CSR_ADD, L.CSR_PLUS_SCALED)
SQUARE_ONLY = (L.CSR_FIRST, L.CSR_NEXT)
ALPHA_BETA = {L.CSR_APPLY: (0.0, 0.0), L.CSR_RESIDUAL: (0.0, 0.0), L.CSR_FIRST: (0.0, 0.6), L.CSR_NEXT: (-0.35, 0.45),
              L.CSR_SUBTRACT: (0.0, 0.0), L.CSR_ADD: (0.0, 0.0), L.CSR_PLUS_SCALED: (0.0, -0.7)}
ALPHA_BETA_2 = {L.CSR_FIRST: (0.0, -0.6), L.CSR_NEXT: (0.25, -0.45), L.CSR_PLUS_SCALED: (0.0, 0.7)}   # the other signs


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t, ctx):
    ctx.synchronize()
    return t.cpu().numpy()


# ---- generators -----------------------------------------------------------------------------------------------------
_BLK = np.array([[3.0, 0.5, 0.25, 0.125], [0.5, 2.0, 0.5, 0.25], [0.25, 0.5, 2.5, 0.5], [0.125, 0.25, 0.5, 1.5]])


def _t1(n, reach, a, b, symmetric):
    """(2 reach + 1)-point 1-D stencil on n nodes; offsets that do not fit the extent drop out."""
    w = {1: b, 2: 0.25 * b, 3: 0.125 * b}
    m = sp.diags([np.full(n, a)], [0])
    for k in range(1, reach + 1):
        if k < n:
            m = m + sp.diags([np.full(n - k, w[k])], [k]) + sp.diags([np.full(n - k, w[k] * (1.0 if symmetric else 0.5))], [-k])
    return m.tocsr()


def node_coords(dims):
    nx, ny, nz = dims
    i = np.arange(nx * ny * nz)
    return i % nx, (i // nx) % ny, i // (nx * ny)


def shell_mask(dims, reach):
    """Nodes closer than `reach` to a face of the box, along the axes that have an interior at all."""
    m = np.zeros(int(np.prod(dims)), dtype=bool)
    for q, n in zip(node_coords(dims), dims):
        if n > 2 * reach:
            m |= (q < reach) | (q >= n - reach)
    return m


def stencil_pattern(dims, reach, dyadic, symmetric=True):
    """Translation-invariant stencil on an nx x ny x nz node grid (x fastest), Kronecker product of 1-D stencils."""
    b = (-0.25, -0.5, -0.125) if dyadic else (-0.2, -0.25, -0.3)
    a = (1.0, 1.5, 2.0)
    return sp.kron(_t1(dims[2], reach, a[2], b[2], symmetric),
                   sp.kron(_t1(dims[1], reach, a[1], b[1], symmetric), _t1(dims[0], reach, a[0], b[0], symmetric))).tocsr()


def distinct_bumps(rng, count):
    """`count` distinct positive numbers k / 1024 (exact in float next to the diagonals used here)."""
    return (1.0 + rng.permutation(1 << 18)[:count]) / 1024.0


def stencil_matrix(dims, reach=1, comps=1, invariant=True, symmetric=True, dyadic=False, perturb=0, perturb_shell=False,
                   empty_lead=0, seed=0):
    """Square stencil matrix with `comps` unknowns per node.  invariant: one stencil for all interior nodes (regular
    rows and boundary classes), else random values (stored planes).  perturb: that many interior nodes get a diagonal of
    their own (listed rows); perturb_shell: every boundary node does (no class survives).  empty_lead: the first rows
    become identity rows (the rows of another rank), which also makes the matrix non-symmetric."""
    rng = np.random.default_rng(seed)
    pat = stencil_pattern(dims, reach, dyadic, symmetric or not invariant)
    blk = _BLK[:comps, :comps].copy()
    if not symmetric:
        blk = np.triu(blk) + 0.5 * np.tril(blk, -1)
    if not dyadic:
        blk = blk * 1.1
    A = sp.kron(pat, blk).tocsr()
    if not invariant:
        if dyadic:
            A.data = rng.integers(1, 1024, A.nnz) * rng.choice([-1.0, 1.0], A.nnz) / 1024.0
        else:
            A.data = rng.standard_normal(A.nnz)
        if symmetric:
            A = (0.5 * (A + A.T)).tocsr()          # (k / 2048: still exact in float)
        A = (A + sp.diags(np.full(A.shape[0], 30.0))).tocsr()
    n_nodes = int(np.prod(dims))
    bump = np.zeros(A.shape[0])
    shell = shell_mask(dims, reach)
    if perturb:
        inner = np.flatnonzero(~shell)
        nodes = rng.choice(inner, perturb, replace=False)
        bump[nodes * comps] = distinct_bumps(rng, perturb)
    if perturb_shell:
        nodes = np.flatnonzero(shell)
        bump[nodes * comps] = distinct_bumps(rng, len(nodes))
    if perturb or perturb_shell:
        A = (A + sp.diags(bump)).tocsr()
    if empty_lead:
        keep = np.ones(A.shape[0])
        keep[:empty_lead] = 0.0
        A = (sp.diags(keep) @ A + sp.diags(1.0 - keep)).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    assert A.shape[0] == n_nodes * comps
    return A


def prolongator_matrix(dims, reach=1, copies=8, wide=False, invariant=True, perturb=0, thin=0.0, dyadic=False, seed=0):
    """Rectangular stencil-like matrix: `copies` stencil matrices stacked (every value tuple repeats `copies` times, so
    with 8 copies even the corner nodes form classes), `wide`: two column blocks [S, S / 2] (twice the offsets).
    invariant False: random values (row-base storage); thin: that share of the entries removed at random (too
    ragged for row-base storage: LDS-cached CSR).  perturb: that many rows get a first entry of their own."""
    rng = np.random.default_rng(seed)
    pat = stencil_pattern(dims, reach, dyadic)
    row = sp.hstack([pat, 0.5 * pat]).tocsr() if wide else pat
    P = sp.vstack([row] * copies).tocsr()
    P.sort_indices()
    if not invariant:
        P.data = rng.standard_normal(P.nnz)
    if perturb:
        # (interior nodes only: a corner stencil repeats just `copies` times and must not lose a member)
        inner = np.flatnonzero(np.tile(~shell_mask(dims, reach), copies))
        rows = rng.choice(inner, perturb, replace=False)
        P.data[P.indptr[rows]] = 7.5 + distinct_bumps(rng, perturb)
    if thin:
        keep = rng.random(P.nnz) > thin
        ptr = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(np.int64), P.indptr[:-1]))])
        P = sp.csr_matrix((P.data[keep], P.indices[keep], ptr), shape=P.shape)
    return P


RAGGED_LENGTHS = (0, 1, 63, 64, 65)


def ragged_matrix(n_rows=256 * 128 + 1, width=96, seed=0):
    """Unstructured square matrix for the CSR kernels: columns from a window around the row (so that a 128-row block
    reuses them: the LDS lists are built), 4 to 12 entries per row, and rows of exactly 0, 1, 63, 64 and 65 entries at
    the start, in the middle and at the end of 128-row blocks; 256 * 128 + 1 rows: the last block has one row."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(4, 13, n_rows)
    special = {}
    for j, ln in enumerate(RAGGED_LENGTHS):
        for r in (128 * (3 + 2 * j), 128 * (40 + 2 * j) + 77, 128 * (100 + 2 * j) + 127):
            special[r] = ln
    special[n_rows - 1] = 65                      # the lone row of the last block
    for r, ln in special.items():
        lens[r] = ln
    ptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.empty(ptr[-1], dtype=np.int64)
    for r in range(n_rows):                       # (the diagonal is among the entries of every row that has any: dinv)
        lo = min(max(r - width // 2, 0), n_rows - width)
        others = np.setdiff1d(np.arange(lo, lo + width), [r])
        col[ptr[r]:ptr[r + 1]] = np.sort(np.append(rng.choice(others, max(lens[r] - 1, 0), replace=False), r))[:lens[r]] if lens[r] else []
    A = sp.csr_matrix((rng.standard_normal(ptr[-1]), col, ptr), shape=(n_rows, n_rows))
    A.eliminate_zeros()
    A.sort_indices()
    return A


def long_rows_matrix(n=600, seed=0):
    """A few hundred rows of a few hundred entries: a workgroup per row."""
    A = sp.random(n, n, density=0.6, random_state=np.random.default_rng(seed), format="csr") + sp.diags(np.full(n, 50.0))
    A = A.tolil()
    A[13, :] = 0.0
    A[14, :] = 0.0
    A[14, 3] = 2.0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


GENERATORS = {"stencil": stencil_matrix, "prolongator": prolongator_matrix, "ragged": ragged_matrix, "long_rows": long_rows_matrix}


# ---- reference and bound --------------------------------------------------------------------------------------------
def row_sums(ptr, terms):
    """Per-row sums of `terms` (one per entry) for a CSR row pointer, empty rows included."""
    out = np.zeros(len(ptr) - 1, dtype=terms.dtype)
    nonempty = np.diff(ptr) > 0
    if nonempty.any():
        out[nonempty] = np.add.reduceat(terms, ptr[:-1][nonempty])
    return out


def reference(A, mode, x, b, dinv, xp, alpha, beta, out0):
    """(ref, bound) per output entry in long double; A: scipy CSR with sorted rows."""
    ld = np.longdouble
    ptr, col = A.indptr.astype(np.int64), A.indices
    xl = x.astype(ld)
    prod = A.data.astype(ld) * xl[col]
    ax, mx = row_sums(ptr, prod), row_sums(ptr, np.abs(prod))
    bl, dl, pl, ol = (None if v is None else v.astype(ld) for v in (b, dinv, xp, out0))
    al, be = ld(alpha), ld(beta)
    if mode == L.CSR_APPLY:
        ref, mag = ax, mx
    elif mode == L.CSR_RESIDUAL:
        ref, mag = ax - bl, mx + np.abs(bl)
    elif mode == L.CSR_FIRST:
        ref, mag = xl - be * dl * (ax - bl), np.abs(xl) + abs(be) * np.abs(dl) * (mx + np.abs(bl))
    elif mode == L.CSR_NEXT:
        ref = xl + al * (xl - pl) - be * dl * (ax - bl)
        mag = np.abs(xl) + abs(al) * (np.abs(xl) + np.abs(pl)) + abs(be) * np.abs(dl) * (mx + np.abs(bl))
    elif mode == L.CSR_SUBTRACT:
        ref, mag = ol - ax, np.abs(ol) + mx
    elif mode == L.CSR_ADD:
        ref, mag = ol + ax, np.abs(ol) + mx
    else:
        ref, mag = ax + be * dl * bl, mx + abs(be) * np.abs(dl) * np.abs(bl)
    k = (np.diff(ptr) + 6).astype(ld)
    gamma = k * ld(U) / (1 - k * ld(U))
    return ref, gamma * mag


def scaled_normal(rng, n):
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 3.0, n)


def make_inputs(A, seed):
    rng = np.random.default_rng(seed)
    m, n = A.shape
    v = dict(x=scaled_normal(rng, n), b=scaled_normal(rng, m), xp=scaled_normal(rng, m), out0=scaled_normal(rng, m))
    if m == n:
        d = A.diagonal()
        v["dinv"] = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 0.0)
    else:
        v["dinv"] = scaled_normal(rng, m)           # (a rectangular matrix has no diagonal: any scaling vector)
    return v


def operands(mode, v):
    """(b, dinv, x_prev, out0) as the mode reads them, None otherwise."""
    need_b = mode in (L.CSR_RESIDUAL, L.CSR_FIRST, L.CSR_NEXT, L.CSR_PLUS_SCALED)
    need_d = mode in (L.CSR_FIRST, L.CSR_NEXT, L.CSR_PLUS_SCALED)
    return (v["b"] if need_b else None, v["dinv"] if need_d else None, v["xp"] if mode == L.CSR_NEXT else None,
            v["out0"] if mode in (L.CSR_SUBTRACT, L.CSR_ADD) else None)


def modes_of(A):
    return [m for m in MODES if A.shape[0] == A.shape[1] or m not in SQUARE_ONLY]


# ---- the case table -------------------------------------------------------------------------------------------------
def variant(label, ops=(), **form):
    """ops: calls on the device matrix before the launch, e.g. ("set_kernel", 8, 1); form: fields form() must report -- a
    value, or a (low, high) range for counts."""
    return dict(label=label, ops=tuple(ops), form=form)


def case(cid, gen, args, variants, small=None, env=None, transpose=False, tags=(), shell=None):
    """small: generator arguments overriding `args` for the CPU tests; env: environment of the construction;
    transpose: the variants describe (and the launches go to) transpose() of the matrix; shell: (dims, reach) of the
    grid for the boundary-shell runs of the class kernels; tags: what the shape is in the table for."""
    return dict(id=cid, gen=gen, args=args, small={**args, **(small or {})}, variants=variants, env=env or {},
                transpose=transpose, tags=tuple(tags), shell=shell)


NO_REGULAR_CLASS = {"MFMG_REGULAR_AS_CLASS_NODES": "0"}
CUBE1, CUBE2, CUBE3 = (37, 33, 29), (35, 33, 31), (36, 33, 31)
SMALL = dict(dims=(9, 8, 7))


def node_variants(c, sym, class_kernel, regular_kernel, listed_route, float_planes=0, listed=None, stored=None):
    """Table kernels on, then off (stored planes), then plain CSR, for an invariant stencil matrix."""
    on = dict(kind=3 if sym else 2, c=c, regular=1, class_kernel=class_kernel, regular_kernel=regular_kernel,
              all_in_classes=int(regular_kernel == 0), listed_route=listed_route, float_planes=float_planes,
              stored_kernel=stored)
    if listed is not None:
        on["listed"] = listed
    return [variant("tables", **on),
            variant("stored", [("set_regular_rows", False)], kind=3 if sym else 2, c=c, regular=0, float_planes=float_planes,
                    stored_kernel="sym_split" if sym else "rows", class_kernel=0, regular_kernel=0),
            variant("csr", [("set_regular_rows", True), ("set_kernel", 0, 0)], kind=0, csr_kernel="lanes")]


def square_class_variants(c, class_kernel):
    """A square matrix that runs as node classes."""
    return [variant("classes", kind=5, regular=1, c=c, class_kernel=class_kernel,
                    listed_route="class_tail" if class_kernel == 1 else "split_tail"),
            variant("csr", [("set_kernel", 0, 0)], kind=0, csr_kernel="lanes")]


def tail_cases():
    """Node classes of a rectangular matrix whose only listed rows are the perturbed ones: exact tail lengths (33: three
    tail workgroups of 16 wavefronts, the last one with a single row)."""
    out = []
    dims = (17, 16, 16)
    for n in (1, 3, 4, 5, 16, 17, 33):
        if n != 33:
            out.append(case(f"nodecls_tail4_{n}", "prolongator", dict(dims=dims, perturb=n, seed=n), small=SMALL,
                            variants=[variant("classes", kind=5, regular=1, c=1, class_kernel=1, listed=n, listed_route="class_tail"),
                                      variant("csr", [("set_kernel", 0, 0)], kind=0, csr_kernel="lanes")],
                            shell=(dims, 1)))
        out.append(case(f"nodecls_tail16_{n}", "prolongator", dict(dims=dims, wide=True, perturb=n, seed=20 + n), small=SMALL,
                        variants=[variant("classes", kind=5, regular=1, c=1, class_kernel=4, listed=n, listed_route="split_tail"),
                                  variant("csr", [("set_kernel", 0, 0)], kind=0, csr_kernel="lanes")],
                        shell=(dims, 1)))
    return out


LANES = (1, 2, 4, 8, 16, 32, 64)

CASES = [
    # ---- translation-invariant square matrices: regular rows + boundary classes, all in the class lists (small levels)
    *[case(f"inv_r1_c{c}", "stencil", dict(dims=CUBE1, comps=c, perturb=20, seed=c), small=SMALL,
           variants=node_variants(c, True, 1, 0, "class_tail", listed=(20 * c, 20 * c + 8 * c)), shell=(CUBE1, 1)) for c in (1, 2, 3, 4)],
    case("inv_r1_c2_f32", "stencil", dict(dims=CUBE1, comps=2, perturb=20, dyadic=True, seed=5), small=SMALL,
         variants=node_variants(2, True, 1, 0, "class_tail", float_planes=1), shell=(CUBE1, 1)),
    case("inv_r1_c2_nonsym", "stencil", dict(dims=CUBE1, comps=2, perturb=20, symmetric=False, empty_lead=400, seed=6),
         small=dict(dims=(9, 8, 7), empty_lead=40), variants=node_variants(2, False, 1, 0, "class_tail"), shell=(CUBE1, 1)),
    case("inv_r2_c1", "stencil", dict(dims=CUBE2, reach=2, perturb=20, seed=7), small=dict(dims=(9, 8, 7)),
         variants=node_variants(1, True, 4, 0, "split_tail"), shell=(CUBE2, 2)),
    case("inv_r2_c2", "stencil", dict(dims=CUBE2, reach=2, comps=2, perturb=20, seed=8), small=dict(dims=(9, 8, 7)),
         variants=node_variants(2, True, 4, 0, "split_tail"), shell=(CUBE2, 2)),
    case("inv_r3_c1", "stencil", dict(dims=CUBE3, reach=3, perturb=20, seed=9), small=dict(dims=(11, 10, 9)),
         variants=node_variants(1, True, 16, 0, "split_tail")[:2], shell=(CUBE3, 3)),
    case("inv_r2_c2_p16_never", "stencil", dict(dims=(34, 33, 31), reach=2, comps=2, perturb=17, symmetric=False, seed=10),
         small=dict(dims=(9, 8, 7)), variants=node_variants(2, False, 4, 0, "split_tail"), shell=((34, 33, 31), 2)),
    # ---- the same with a launch of the regular nodes of their own (what levels above 5 M nodes run)
    *[case(f"own_r1_c{c}", "stencil", dict(dims=CUBE1, comps=c, perturb=5, seed=10 + c), small=SMALL, env=NO_REGULAR_CLASS,
           variants=node_variants(c, True, 1, 1, "class_tail")[:1], shell=(CUBE1, 1)) for c in (1, 2, 3, 4)],
    case("own_r2_c1", "stencil", dict(dims=CUBE2, reach=2, perturb=16, seed=15), small=dict(dims=(9, 8, 7)), env=NO_REGULAR_CLASS,
         variants=node_variants(1, True, 4, 4, "split_tail")[:1], shell=(CUBE2, 2)),
    case("own_r2_c2", "stencil", dict(dims=CUBE2, reach=2, comps=2, perturb=3, seed=16), small=dict(dims=(9, 8, 7)),
         env=NO_REGULAR_CLASS, variants=node_variants(2, True, 4, 4, "split_tail")[:1], shell=(CUBE2, 2)),
    case("own_r3_c1", "stencil", dict(dims=CUBE3, reach=3, perturb=1, seed=17), small=dict(dims=(11, 10, 9)), env=NO_REGULAR_CLASS,
         variants=node_variants(1, True, 16, 16, "split_tail")[:1], shell=(CUBE3, 3)),
    # ---- listed rows: a launch of their own (no class survives), and the stored planes (more than 32768 of them)
    case("shell_perturbed_c1", "stencil", dict(dims=CUBE1, perturb_shell=True, seed=18), small=SMALL,
         variants=[variant("tables", kind=3, c=1, regular=1, classes=0, class_kernel=0, regular_kernel=1, listed_route="own_launch",
                           listed=(5000, 32768))]),
    case("many_listed_sym", "stencil", dict(dims=(48, 48, 40), perturb=33000, seed=19), small=dict(dims=(9, 8, 7), perturb=40),
         variants=[variant("tables", kind=3, c=1, regular=1, class_kernel=1, listed=(33000, 34000), listed_route="stored_planes",
                           stored_kernel="sym_rows", float_planes=0)]),
    case("many_listed_sym_f32", "stencil", dict(dims=(48, 48, 40), perturb=33000, dyadic=True, seed=20),
         small=dict(dims=(9, 8, 7), perturb=40),
         variants=[variant("tables", kind=3, c=1, regular=1, class_kernel=1, listed=(33000, 34000), listed_route="stored_planes",
                           stored_kernel="sym_rows", float_planes=1)]),
    case("many_listed_nonsym", "stencil", dict(dims=(48, 48, 40), perturb=33000, symmetric=False, seed=21),
         small=dict(dims=(9, 8, 7), perturb=40),
         variants=[variant("tables", kind=2, c=1, regular=1, class_kernel=1, listed=(33000, 34000), listed_route="stored_planes",
                           stored_kernel="rows", float_planes=0)]),
    # ---- stored planes of matrices without repeating values, double and float
    *[case(f"planes_{'sym' if s else 'nonsym'}_c{c}{'_f32' if f else ''}", "stencil",
           dict(dims=CUBE1 if c < 4 else (23, 21, 19), comps=c, invariant=False, symmetric=s, dyadic=f, seed=30 + 4 * c + 2 * s + f),
           small=SMALL,
           variants=[variant("stored", kind=3 if s else 2, c=c, regular=0, float_planes=int(f),
                             stored_kernel="sym_split" if s else "rows"),
                     variant("csr", [("set_kernel", 0, 0)], kind=0, csr_kernel="lanes")])
      for c, s, f in ((1, True, False), (1, True, True), (2, False, False), (2, False, True), (3, True, True), (4, False, False))],
    # ---- thin grids and extents at the reach
    case("layer1_r1", "stencil", dict(dims=(182, 181, 1), perturb=4, seed=40), small=dict(dims=(12, 11, 1)),
         variants=node_variants(1, True, 1, 0, "class_tail"), shell=((182, 181, 1), 1)),
    # (two and four layers: with most offsets outside the grid the block diagonals are too empty to be stored, and the
    # square matrix runs as node classes -- base and clamp act on every node)
    case("layer2_r1", "stencil", dict(dims=(130, 127, 2), comps=2, perturb=4, seed=41), small=dict(dims=(12, 11, 2)),
         variants=square_class_variants(2, 1), shell=((130, 127, 2), 1)),
    case("layer2_r2", "stencil", dict(dims=(129, 128, 2), reach=2, perturb=4, seed=42), small=dict(dims=(12, 11, 2)),
         variants=square_class_variants(1, 4), shell=((129, 128, 2), 2)),
    case("layer4_r2", "stencil", dict(dims=(91, 91, 4), reach=2, perturb=4, seed=43), small=dict(dims=(12, 11, 4)),
         variants=square_class_variants(1, 4), shell=((91, 91, 4), 2)),
    # ---- node counts around the 64-slot granularity of the lists: a chain of 4-component nodes (no class: the two end
    # nodes are listed and have a launch of their own)
    *[case(f"chain_{n}", "stencil", dict(dims=(n, 1, 1), comps=4, seed=50 + j), small=dict(dims=(n // 64, 1, 1)),
           variants=[variant("tables", kind=3, c=4, regular=1, classes=0, regular_kernel=1, class_kernel=0, listed=8,
                             listed_route="own_launch"),
                     variant("stored", [("set_regular_rows", False)], kind=3, regular=0, stored_kernel="sym_split")],
           )
      for j, n in enumerate((64 * 129 - 1, 64 * 129, 64 * 129 + 1))],
    # ---- slots of the class lists around the 256 nodes of a workgroup: a sheet of 4-component nodes, 10 nodes across; the
    # classes are the two long edges, the two short ones (8 nodes in 64 slots each) and the regular nodes, every class
    # padded to whole wavefronts: 2 pad(nx - 2) + 128 + pad(8 (nx - 2)) slots
    *[case(f"slots_{nx}", "stencil", dict(dims=(nx, 10, 1), comps=4, seed=55 + j), small=dict(dims=(12, 10, 1)),
           variants=[variant("tables", kind=3, c=4, regular=1, all_in_classes=1, classes=5, class_slots=slots, class_kernel=1,
                             regular_kernel=0, listed=16, listed_route="class_tail"),
                     variant("stored", [("set_regular_rows", False)], kind=3, regular=0, stored_kernel="sym_split")],
           shell=((nx, 10, 1), 1))
      for j, (nx, slots) in enumerate(((834, 33 * 256), (835, 34 * 256 - 64), (851, 34 * 256 + 64)))],
    # ---- rectangular matrices: node classes (tails of exact lengths), row base, LDS-cached CSR, and their transposes
    *tail_cases(),
    case("nodecls_r2_wide_p16", "prolongator", dict(dims=(17, 16, 16), reach=2, wide=True, perturb=17, seed=60), small=SMALL,
         variants=[variant("classes", kind=5, regular=1, c=1, class_kernel=16, listed=17, listed_route="split_tail"),
                   variant("csr", [("set_kernel", 0, 0)], kind=0, csr_kernel="lanes")], shell=((17, 16, 16), 2)),
    # (two copies of the cube: the transpose has more than 32768 rows and node classes of its own, 54 offsets)
    case("nodecls_transposed", "prolongator", dict(dims=CUBE1, copies=2, perturb=3, seed=61), small=SMALL, transpose=True,
         variants=[variant("transpose", kind=5, regular=1, c=1, class_kernel=4)], tags=["transpose:classed"]),
    case("row_base", "prolongator", dict(dims=(224, 150, 1), copies=6, invariant=False, seed=62), small=dict(dims=(12, 11, 1)),
         variants=[variant("row_base", kind=4, row_base_slots=9), variant("csr", [("set_kernel", 0, 0)], kind=0, csr_kernel="lanes")]),
    case("row_base_transposed", "prolongator", dict(dims=(224, 150, 1), copies=6, invariant=False, seed=62),
         small=dict(dims=(12, 11, 1)), transpose=True, variants=[variant("transpose", kind=0, csr_kernel="lanes", lanes=16)], tags=["transpose:row_base"]),
    case("thinned_lds", "prolongator", dict(dims=CUBE1, copies=6, invariant=False, thin=0.45, seed=63), small=SMALL,
         variants=[variant("lds", kind=1, csr_kernel="lds"), variant("csr", [("set_kernel", 0, 0)], kind=0, csr_kernel="lanes")]),
    # ---- CSR kernels: every lanes-per-row value, plain and LDS-cached; rows of 0, 1, 63, 64, 65 entries; a last block of 1 row
    case("ragged", "ragged", dict(seed=70), small=dict(n_rows=110 * 128 + 1),
         variants=[variant("lanes64", [("set_kernel", 64, 0)], kind=0, csr_kernel="lanes", lanes=64)]
         + [variant(f"lanes{l}", [("set_kernel", l, 0)], kind=0, csr_kernel="lanes", lanes=l) for l in LANES[:-1]]
         + [variant(f"lds{l}", [("set_kernel", l, 1)], kind=1, csr_kernel="lds", lanes=max(l, 4)) for l in LANES],
         tags=["rows:0,1,63,64,65", "last_block_of_1_row"]),
    case("long_rows", "long_rows", dict(seed=71), small=dict(n=120),
         variants=[variant("row_block", kind=0, csr_kernel="row_block", lanes=256),
                   variant("lanes64", [("set_kernel", 64, -1)], kind=0, csr_kernel="lanes", lanes=64)]),
]
BY_ID = {c["id"]: c for c in CASES}


def variant_paths(c, v):
    """The kernel paths a variant reaches, from the form it must report."""
    f = v["form"]
    paths = set()
    planes = "float" if f.get("float_planes") else "double"
    if f.get("csr_kernel") == "lanes" and "lanes" in f:
        paths.add(f"csr_lanes:{f['lanes']}")
    if f.get("csr_kernel") == "lds" and "lanes" in f:
        paths.add(f"csr_lds:{f['lanes']}")
    if f.get("csr_kernel") == "row_block":
        paths.add("csr_row_block")
    if f.get("stored_kernel"):
        paths.add(f"stored_{f['stored_kernel']}:{planes}")
    if f.get("kind") == 4:
        paths.add("row_base")
    if f.get("kind") in (2, 3) and f.get("regular"):
        rk, ck = f.get("regular_kernel"), f.get("class_kernel")
        if rk == 1:
            paths.add(f"regular_node:C{f['c']}")
        elif rk:
            paths.add(f"regular_split{rk}:C{f['c']}")
        if ck == 1:
            paths.add(f"class_node:C{f['c']}")
        elif ck:
            paths.add(f"class_split{ck}:C{f['c']}")
        if f.get("c") == 2:
            paths.add("store_node_row_by_row:C2")
    if f.get("kind") == 5:
        ck = f.get("class_kernel")
        paths.add("nodecls_node" if ck == 1 else f"nodecls_split{ck}")
        if f.get("c") == 2:
            paths.add("store_node_row_by_row:nodecls_C2")
    if f.get("listed_route"):
        paths.add(f"listed:{f['listed_route']}")
    return paths


def shape_paths(c):
    """What the shape of a case is in the table for, from its generator arguments and the forms it must report."""
    a, paths = c["args"], set()
    forms = [v["form"] for v in c["variants"]]
    if c["gen"] == "stencil":
        dims, reach = a["dims"], a.get("reach", 1)
        n_nodes = int(np.prod(dims))
        if min(dims) > 2 * reach and 32768 <= n_nodes * a.get("comps", 1) and n_nodes < 40000:
            paths.add("grid:cube")
        if any(f.get("regular") for f in forms):                      # (the node kernels: where the clamp acts)
            paths |= {f"grid:{n}_layer{'s' if n > 1 else ''}" for n in (1, 2) if min(dims) == n}
            if reach in dims:
                paths.add("grid:extent_reach")
            if 2 * reach in dims:
                paths.add("grid:extent_2reach")
        if any(f.get("regular_kernel") == 1 for f in forms) and n_nodes % 64 in (63, 0, 1) and n_nodes < 64 * 1024:
            paths.add("nodes:64k" + {63: "-1", 0: "", 1: "+1"}[n_nodes % 64])
        if a.get("empty_lead"):
            paths.add("emptied_leading_rows")
    for f in forms:
        if isinstance(f.get("class_slots"), int) and f.get("class_kernel") == 1:
            paths.add("class_slots:256k" + {0: "", 64: "+64", 192: "-64"}.get(f["class_slots"] % 256, "?"))
        if isinstance(f.get("listed"), int) and f.get("listed_route") in ("class_tail", "split_tail"):
            paths.add(f"{f['listed_route']}_length:{f['listed']}")
    return paths


def case_paths(c):
    paths = set(c["tags"]) | shape_paths(c)
    for v in c["variants"]:
        paths |= variant_paths(c, v)
    return paths


# the list a reviewer reads to see coverage
REQUIRED_FORMS = [
    *[f"csr_lanes:{l}" for l in LANES], *[f"csr_lds:{l}" for l in (4, 8, 16, 32, 64)], "csr_row_block",
    "stored_rows:double", "stored_rows:float", "stored_sym_rows:double", "stored_sym_rows:float",
    "stored_sym_split:double", "stored_sym_split:float", "row_base",
    "regular_node:C1", "regular_node:C2", "regular_node:C3", "regular_node:C4",
    "regular_split4:C1", "regular_split4:C2", "regular_split16:C1",
    "class_node:C1", "class_node:C2", "class_node:C3", "class_node:C4",
    "class_split4:C1", "class_split4:C2", "class_split16:C1",
    "nodecls_node", "nodecls_split4", "nodecls_split16", "store_node_row_by_row:C2", "store_node_row_by_row:nodecls_C2",
    "listed:class_tail", "listed:split_tail", "listed:own_launch", "listed:stored_planes",
    *[f"class_tail_length:{n}" for n in (1, 3, 4, 5, 16, 17)], *[f"split_tail_length:{n}" for n in (1, 3, 4, 5, 16, 17, 33)],
    "class_slots:256k", "class_slots:256k-64", "class_slots:256k+64",
    "grid:cube", "grid:2_layers", "grid:1_layer", "grid:extent_reach", "grid:extent_2reach",
    "nodes:64k-1", "nodes:64k", "nodes:64k+1", "emptied_leading_rows",
    "rows:0,1,63,64,65", "last_block_of_1_row", "transpose:classed", "transpose:row_base",
]


# ---- tests that need no GPU -----------------------------------------------------------------------------------------
def test_case_table_covers_every_required_form():
    covered = set()
    for c in CASES:
        covered |= case_paths(c)
    assert sorted(set(REQUIRED_FORMS) - covered) == []
    assert len(BY_ID) == len(CASES)


def seed_of(c):
    return zlib.crc32(c["id"].encode())


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_reference_bounds_scipy_float64(cid):
    """The reference stays inside its own cap: scipy's float64 product, with the epilogue in float64, lies within the bound
    of the long-double reference for every generator and mode (reduced grids)."""
    c = BY_ID[cid]
    A = GENERATORS[c["gen"]](**c["small"])
    if c["transpose"]:
        A = A.T.tocsr()
        A.sort_indices()
    v = make_inputs(A, seed_of(c))
    ax = A @ v["x"]
    for mode in modes_of(A):
        for al, be in {ALPHA_BETA[mode], ALPHA_BETA_2.get(mode, ALPHA_BETA[mode])}:
            b, d, xp, o0 = operands(mode, v)
            ref, bound = reference(A, mode, v["x"], b, d, xp, al, be, o0)
            x = v["x"]
            got = {L.CSR_APPLY: lambda: ax, L.CSR_RESIDUAL: lambda: ax - b, L.CSR_FIRST: lambda: x - be * d * (ax - b),
                   L.CSR_NEXT: lambda: x + al * (x - xp) - be * d * (ax - b), L.CSR_SUBTRACT: lambda: o0 - ax,
                   L.CSR_ADD: lambda: o0 + ax, L.CSR_PLUS_SCALED: lambda: ax + be * d * b}[mode]()
            excess = np.abs(got.astype(np.longdouble) - ref) - bound
            assert excess.max() <= 0, (mode, int(excess.argmax()))


def test_generators_produce_what_they_claim():
    for c in CASES:
        a = c["small"]
        A = GENERATORS[c["gen"]](**a)
        assert A.has_sorted_indices and np.all(A.data != 0.0), c["id"]
        if c["gen"] == "stencil":
            sym = a.get("symmetric", True) and not a.get("empty_lead")
            assert (abs(A - A.T).max() == 0.0) == sym, c["id"]
            assert np.all(A.diagonal() != 0.0)
            if a.get("dyadic"):
                assert np.array_equal(A.data.astype(np.float32).astype(np.float64), A.data), c["id"]
            else:
                assert not np.array_equal(A.data.astype(np.float32).astype(np.float64), A.data), c["id"]
        if c["gen"] == "stencil" and a.get("invariant", True) and not a.get("empty_lead"):
            # distinct node stencils: offsets and values of the block rows of a node
            comps, dims, reach = a.get("comps", 1), a["dims"], a.get("reach", 1)
            seen = {}
            for nd in range(A.shape[0] // comps):
                key = []
                for r in range(nd * comps, (nd + 1) * comps):
                    s, e = A.indptr[r], A.indptr[r + 1]
                    key.append((tuple(A.indices[s:e] - nd * comps), tuple(A.data[s:e])))
                seen.setdefault(tuple(key), []).append(nd)
            counts = sorted(len(v) for v in seen.values())
            shell = shell_mask(dims, reach)
            n_perturbed = a.get("perturb", 0) + (int(shell.sum()) if a.get("perturb_shell") else 0)
            assert sum(1 for k in counts if k == 1) >= n_perturbed, c["id"]      # every perturbed node is alone
            # one stencil per combination of distances to the faces: (2 reach + 1) per axis with an interior
            want = int(np.prod([2 * reach + 1 if n > 2 * reach else n for n in dims]))
            assert len(seen) - n_perturbed == (1 if a.get("perturb_shell") else want), c["id"]
        if c["gen"] == "prolongator" and a.get("invariant", True):
            P = A
            rows = {}
            for r in range(P.shape[0]):
                s, e = P.indptr[r], P.indptr[r + 1]
                rows.setdefault((tuple(P.indices[s:e] - P.indices[s]), tuple(P.data[s:e])), []).append(r)
            assert sum(1 for v in rows.values() if len(v) == 1) == a.get("perturb", 0), c["id"]
            assert min(len(v) for v in rows.values() if len(v) > 1) >= a.get("copies", 8), c["id"]
    R = ragged_matrix()
    lens = np.diff(R.indptr)
    assert R.shape[0] % 128 == 1 and lens[-1] == 65
    for ln in RAGGED_LENGTHS:
        at = np.flatnonzero(lens == ln)
        assert {0, 77, 127} <= set(at % 128), ln
    Lr = long_rows_matrix()
    assert Lr.shape[0] <= 4096 and Lr.nnz / Lr.shape[0] >= 256 and np.diff(Lr.indptr).min() == 0


# ---- GPU tests ------------------------------------------------------------------------------------------------------
def check_form(f, want, where):
    for k, w in want.items():
        if isinstance(w, tuple):
            assert w[0] <= f[k] <= w[1], f"{where}: form()[{k!r}] = {f[k]}, expected within {w}; form: {f}"
        else:
            assert f[k] == w, f"{where}: form()[{k!r}] = {f[k]!r}, expected {w!r}; form: {f}"


def launch(Ad, ctx, mode, v, al, be, offset=0, x=None):
    """One launch; offset 1: b, dinv, x_prev and out sit at 8-byte but not 16-byte aligned addresses (x never does)."""
    m = Ad.shape[0]
    b, d, xp, o0 = operands(mode, v)

    def put(a):
        if a is None:
            return None
        buf = torch.empty(m + 2, dtype=torch.float64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        t = buf[offset:offset + m]
        t.copy_(torch.from_numpy(a))
        assert t.data_ptr() % 16 == 8 * offset
        return t
    out = put(o0 if o0 is not None else np.full(m, np.nan))
    xd = dev(v["x"] if x is None else x)
    assert xd.data_ptr() % 16 == 0
    Ad.launch(mode, xd, out, b=put(b), dinv=put(d), x_prev=put(xp), alpha=al, beta=be)
    ctx.synchronize()
    return out


def assert_within(got, ref, bound, where, factor=1):
    excess = np.abs(got.astype(np.longdouble) - ref) - factor * bound
    i = int(excess.argmax())
    assert excess[i] <= 0, (f"{where}: row {i}: got {got[i]!r}, reference {float(ref[i])!r}, "
                            f"difference {float(abs(got[i] - ref[i])):.3e} > bound {float(factor * bound[i]):.3e}")


def shell_vectors(c, A):
    """x = 1 on the boundary shell of the column grid and 0 inside, and the reverse: the unknowns of a node are
    consecutive in a stencil matrix, the column blocks of a prolongator follow each other."""
    dims, reach = c["shell"]
    per_node = A.shape[1] // int(np.prod(dims))
    assert per_node * int(np.prod(dims)) == A.shape[1]
    mask = shell_mask(dims, reach)
    shell = np.repeat(mask, per_node) if c["gen"] == "stencil" else np.tile(mask, per_node)
    assert 0 < shell.sum() < len(shell)
    return shell.astype(np.float64), (~shell).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_spmv_layout(ctx, monkeypatch, cid):
    c = BY_ID[cid]
    for k, val in c["env"].items():
        monkeypatch.setenv(k, val)
    A = GENERATORS[c["gen"]](**c["args"])
    base = M.SparseMatrixDevice(ctx, A)
    Ad = base
    if c["transpose"]:
        Ad = base.transpose()
        A = A.T.tocsr()
        A.sort_indices()
        # (transpose() wraps the matrix the operator builds once for its transposed application: apply(.., TRANS) launches
        # on the object whose form is asserted below)
        xt = scaled_normal(np.random.default_rng(1), A.shape[1])
        yt = torch.full((A.shape[0],), np.nan, dtype=torch.float64, device="cuda")
        base.apply(dev(xt), yt, L.TRANS)
        ref, bound = reference(A, L.CSR_APPLY, xt, None, None, None, 0.0, 0.0, None)
        assert_within(host(yt, ctx), ref, bound, f"{cid}: apply(TRANS)")
    v = make_inputs(A, seed_of(c))
    modes = modes_of(A)
    first = {}
    for var in c["variants"]:
        for op in var["ops"]:
            getattr(Ad, op[0])(*op[1:])
        f = Ad.form()
        where = f"{cid}/{var['label']}"
        print(f"{where}: {A.shape[0]} x {A.shape[1]}, {A.nnz} entries, form {f}")
        check_form(f, var["form"], where)
        paired_check = f["c"] == 2 and f["regular"] == 1
        for mode in modes:
            for al, be in sorted({ALPHA_BETA[mode], ALPHA_BETA_2.get(mode, ALPHA_BETA[mode])}):
                b, d, xp, o0 = operands(mode, v)
                ref, bound = reference(A, mode, v["x"], b, d, xp, al, be, o0)
                out = launch(Ad, ctx, mode, v, al, be)
                assert Ad.form()["pairs"] == 1
                got = out.cpu().numpy()
                assert np.all(np.isfinite(got)), f"{where}: mode {mode}: entries left unwritten or not finite"
                assert_within(got, ref, bound, f"{where}: mode {mode}, alpha {al}, beta {be}")
                key = (mode, al, be)
                if key in first:
                    assert_within(got, first[key].astype(np.longdouble), bound, f"{where} against {c['variants'][0]['label']}: mode {mode}", 2)
                else:
                    first[key] = got
                again = launch(Ad, ctx, mode, v, al, be)
                assert torch.equal(out, again), f"{where}: mode {mode}: a repeated launch changed bits"
                if paired_check:
                    odd = launch(Ad, ctx, mode, v, al, be, offset=1)
                    assert Ad.form()["pairs"] == 0
                    assert torch.equal(out, odd), f"{where}: mode {mode}: row-by-row store_node differs from the paired one"
        if c["shell"] is not None and f["regular"] == 1:
            for xs in shell_vectors(c, A):
                ref, bound = reference(A, L.CSR_APPLY, xs, None, None, None, 0.0, 0.0, None)
                out = launch(Ad, ctx, L.CSR_APPLY, v, 0.0, 0.0, x=xs)
                assert_within(out.cpu().numpy(), ref, bound, f"{where}: boundary-shell x")
    if A.shape[0] != A.shape[1]:
        with pytest.raises(L.MfmgError, match="square"):
            launch(Ad, ctx, L.CSR_NEXT, v, 0.3, 0.4)


@pytest.mark.gpu
def test_launch_rejects_missing_operands(ctx):
    A = long_rows_matrix(120)
    Ad = M.SparseMatrixDevice(ctx, A)
    n = A.shape[0]
    x, out = dev(np.ones(n)), dev(np.zeros(n))
    with pytest.raises(L.MfmgError, match="needs b"):
        Ad.launch(L.CSR_RESIDUAL, x, out)
    with pytest.raises(L.MfmgError, match="inverse diagonal"):
        Ad.launch(L.CSR_PLUS_SCALED, x, out, b=x)
    with pytest.raises(L.MfmgError, match="x_prev"):
        Ad.launch(L.CSR_NEXT, x, out, b=x, dinv=x)
    with pytest.raises(L.MfmgError, match="in place"):
        Ad.launch(L.CSR_ADD, x, x)
    with pytest.raises(L.MfmgInvalidArgument, match="unknown SpMV mode"):
        Ad.launch(7, x, out)
    # the source vector at an 8-byte but not 16-byte aligned address: refused by every SpMV entry point
    buf = torch.ones(n + 2, dtype=torch.float64, device="cuda")
    odd = buf[1:n + 1]
    assert odd.data_ptr() % 16 == 8
    for call in (lambda: Ad.launch(L.CSR_APPLY, odd, out), lambda: Ad.vmult(out, odd), lambda: Ad.apply(odd, out),
                 lambda: Ad.residual(odd, x, out), lambda: Ad.smoother_step(x, x, odd, None, 0.0, 0.5, out)):
        with pytest.raises(L.MfmgInvalidArgument, match="16-byte aligned"):
            call()
    assert Ad.form()["pairs"] == -1                    # (nothing was launched so far)
    Ad.launch(L.CSR_RESIDUAL, x, odd, b=odd)          # (the other vectors may sit there)
    assert Ad.form()["pairs"] == 0
