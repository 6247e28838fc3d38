"""The AMGe transfer R, R^T and the coarse setup beyond 2 x 2 x 2 agglomerates with two eigenvectors.

Every case of CASES names the mesh, material, agglomerate, eigenvectors, DoF numbering and setup precision, and the form
the restrictor must take (which kernels it launches, table / class / listed-block paths); the first assertion of every
GPU test checks that form, so that no case passes without reaching the path it is meant for.  Then:
  (a) R x, R^T y and z - R^T y against a long-double reference, per entry within gamma_k (|R| |x|)_i;
  (b) the row kernel against the pair kernels and the node kernel against the 2 x 2 x 2 block kernel, bit for bit
      (MFMG_SR_RESTRICT=rows, MFMG_SR_PROLONG=nodes);
  (c) R and R A R^T (device probing and host product) against the oracle;
  (d) 8-cycle residual histories against the oracle with the dense and the aggregation (AMG) coarse solve.
Two tests need no GPU: the coverage of the case table, and the coupling reach of R A R^T in the oracle."""
import numpy as np
import pytest
import torch

import mfmg_amd as M
from mfmg_amd import lib as L
import mfmg_oracle as O

HIST_TOL = 1e-10
HIST_ATOL = 1e-12
U = 2.0 ** -53


def case(cid, n, material="constant", agg=(2, 2, 2), n_eig=2, numbering="lexicographic", precision="double",
         structured=True, form=None, setup=True):
    """`form`: what restrictor_form() must report beyond n_eig and the agglomerate -- restrict / prolong kernel,
    float_planes, and table / classes / listed as True (> 0), False (0) or "several" (listed blocks that fill more than
    two workgroups of 256 threads and leave the last one partial).  `setup`: the mesh is small enough for the oracle's
    setup and cycle (parts c and d)."""
    return dict(id=cid, n=n, material=material, agg=agg, n_eig=n_eig, numbering=numbering, precision=precision,
                structured=structured, form=form or {}, setup=setup)


def pair222(**kw):
    return dict(restrict="pair222", **kw)


CASES = [
    # pair<2> + reference table + class table + block222 with listed blocks over many workgroups (the last one partial)
    case("const222_130x36x12", (130, 36, 12), form=pair222(prolong="block222", table=True, classes=True, listed="several"),
         setup=False),
    # one agglomerate along y and z: block222 on a grid of 2 agglomerate positions per direction
    case("const222_130x2x2", (130, 2, 2), form=pair222(prolong="block222", table=True, classes=False, listed=True)),
    # discontinuous coefficient: almost every agglomerate a block of its own (planes), no table
    case("disc222_70x66x4", (70, 66, 4), "discontinuous", form=pair222(prolong="nodes", table=False), setup=False),
    case("disc222_12x10x6", (12, 10, 6), "discontinuous", form=pair222(prolong="nodes", table=False)),
    # planes in double / in float
    case("linear222_ne2", (8, 6, 4), "linear", form=pair222(prolong="nodes", float_planes=False, table=False)),
    case("linear222_ne2_f32", (8, 6, 4), "linear", precision="float", form=pair222(prolong="nodes", float_planes=True)),
    case("linear222_ne4_f32", (8, 6, 4), "linear", n_eig=4, precision="float",
         form=dict(restrict="rows", prolong="nodes", float_planes=True)),
    # pair<0> with the reference table, node kernel
    case("const322_36x2x2", (36, 2, 2), agg=(3, 2, 2), form=dict(restrict="pair", prolong="nodes", table=True)),
    case("const422_48x2x2", (48, 2, 2), agg=(4, 2, 2), form=dict(restrict="pair", prolong="nodes", table=True)),
    case("const322_12x8x8", (12, 8, 8), agg=(3, 2, 2), form=dict(restrict="pair", prolong="nodes", table=False)),
    # the row kernel and the n_eig loop of the node kernel; 3 x 3 x 3: patches of 64 nodes (the largest device eigen kernel)
    case("const222_ne1", (8, 6, 4), n_eig=1, form=dict(restrict="rows", prolong="nodes", table=False)),
    case("linear222_ne3", (8, 6, 4), "linear", n_eig=3, form=dict(restrict="rows", prolong="nodes")),
    case("linear222_ne4", (8, 6, 4), "linear", n_eig=4, form=dict(restrict="rows", prolong="nodes", float_planes=False)),
    case("const333_ne3", (9, 9, 6), agg=(3, 3, 3), n_eig=3, form=dict(restrict="rows", prolong="nodes")),
    # renumbered DoFs (node_dof)
    case("random222_ne2", (6, 8, 10), "linear", numbering="random", form=pair222(prolong="nodes")),
    case("random222_ne3", (6, 6, 6), "linear", n_eig=3, numbering="random", form=dict(restrict="rows", prolong="nodes")),
    # controls without the agglomerate-wise form: switched off, and clipped agglomerates
    case("csr_linear222", (8, 6, 4), "linear", structured=False),
    case("clipped222_7x6x6", (7, 6, 6), structured=None),
    # agglomerates one cell wide: R A R^T couples agglomerates two apart along that axis
    # (ne1 on 12 x 8 x 8 and 8 x 8 x 12: with only two agglomerates across the other axes R A R^T is singular, see CYCLES)
    case("one_cell122_ne1", (12, 8, 8), agg=(1, 2, 2), n_eig=1, form=dict(restrict="rows", prolong="nodes")),
    case("one_cell122_ne2", (12, 4, 4), agg=(1, 2, 2), form=dict(restrict="pair", prolong="nodes")),
    case("one_cell221_ne1", (8, 8, 12), agg=(2, 2, 1), n_eig=1, form=dict(restrict="rows", prolong="nodes")),
    case("one_cell221_ne2", (4, 4, 10), agg=(2, 2, 1), form=dict(restrict="pair", prolong="nodes")),
    # patches of 75 nodes: eigenproblems on the host
    case("host_eig442", (8, 8, 4), agg=(4, 4, 2), form=dict(restrict="pair", prolong="nodes")),
]
BY_ID = {c["id"]: c for c in CASES}


def case_paths(c):
    """The kernel paths a case reaches, from its expected form."""
    if not c["structured"]:
        return {"csr"}
    f = c["form"]
    paths = {"restrict:" + f["restrict"], "prolong:" + f["prolong"]}
    if f.get("table"):
        paths.add("table")
    if f.get("classes"):
        paths.add("classes")
    if f.get("listed"):
        paths.add("listed_blocks")
    if f.get("listed") == "several":
        paths.add("listed_blocks_several_workgroups")
    paths.add("float_planes" if f.get("float_planes") or c["precision"] == "float" else "double_planes")
    if c["n_eig"] != 2:
        paths.add("n_eig_loop")
    if c["numbering"] != "lexicographic":
        paths.add("node_dof")
    if min(c["agg"]) == 1:
        paths.add("one_cell_agglomerates")
    patch = int(np.prod([a + 1 for a in c["agg"]]))
    if 28 <= patch <= 64:
        paths.add("eigen_kernel_64")
    if patch > 64:
        paths.add("host_eigensolves")
    if f["prolong"] == "block222" and "restrict" in f:
        paths.add("same_bits_block222")
    if f["restrict"].startswith("pair"):
        paths.add("same_bits_rows")
    return paths


REQUIRED_PATHS = {"restrict:pair222", "restrict:pair", "restrict:rows", "prolong:block222", "prolong:nodes", "table", "classes",
                  "listed_blocks", "listed_blocks_several_workgroups", "float_planes", "double_planes", "n_eig_loop", "node_dof",
                  "one_cell_agglomerates", "eigen_kernel_64", "host_eigensolves", "csr", "same_bits_block222", "same_bits_rows"}


def test_case_table_covers_every_transfer_path():
    """Every kernel path of structured_restrictor.hip (and the CSR control) is reached by at least one case, and the table
    has n_eig 1 to 4 and agglomerates one cell wide along x and along z."""
    covered = set().union(*(case_paths(c) for c in CASES))
    assert REQUIRED_PATHS <= covered, sorted(REQUIRED_PATHS - covered)
    assert {c["n_eig"] for c in CASES} >= {1, 2, 3, 4}
    assert {c["agg"] for c in CASES if min(c["agg"]) == 1} >= {(1, 2, 2), (2, 2, 1)}
    assert all(np.prod(c["n"]) <= 130 * 70 * 12 for c in CASES)
    for c in CASES:
        if c["structured"]:
            assert all(v % a == 0 for v, a in zip(c["n"], c["agg"])), c["id"]


@pytest.mark.parametrize("a", [1, 2, 3, 4])
def test_galerkin_coupling_reach_of_the_oracle(a):
    """R A R^T of agglomerates of `a` cells along x couples agglomerates up to 1 + floor(1 / a) apart in x, and 1 apart
    along the axes of 2 cells: the reach the device probing product and the device AMG setup use."""
    n = (6 * a if a > 1 else 8, 4, 4)
    agg = (a, 2, 2)
    mesh = O.StructuredMesh(n)
    coef = O.coefficient_table(mesh, "constant")
    mf = O.MatrixFreeLaplace(mesh, coef)
    R = O.build_restrictor(mesh, coef, mf.diagonal(), agg=agg, n_eig=1, variant="mf", eig_mode="krylov").csr
    Ac = O.galerkin_coarse_matrix(mf.vmult, R).tocoo()
    na = [v // g for v, g in zip(n, agg)]
    keep = np.abs(Ac.data) > 1e-13 * np.abs(Ac.data).max()
    r, c = Ac.row[keep], Ac.col[keep]
    pos = lambda i: (i % na[0], (i // na[0]) % na[1], i // (na[0] * na[1]))
    (rx, ry, rz), (cx, cy, cz) = pos(r), pos(c)
    assert np.abs(rx - cx).max() == 1 + 1 // a
    assert np.abs(ry - cy).max() == 1 and np.abs(rz - cz).max() == 1


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def params_of(c, **extra):
    p = {"eigensolver": {"number of eigenvectors": c["n_eig"]}, "agglomeration": dict(zip(("nx", "ny", "nz"), c["agg"])),
         "is preconditioner": False, "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 2, "smoothing_range": 20.0},
         "setup value precision": c["precision"]}
    if c["structured"] is False:
        p["restrictor"] = {"structured": False}
    if not c["setup"]:
        p["solver"] = {"type": "amg"}       # (coarse problems beyond the dense solver's limit)
    p.update(extra)
    return p


def numbering_of(c):
    if c["numbering"] == "lexicographic":
        return None
    nd = int(np.prod([v + 1 for v in c["n"]]))
    return torch.from_numpy(np.random.default_rng(3).permutation(nd))


def build(ctx, c, **extra):
    prob = M.LaplaceProblem(c["n"], c["material"], device="cuda", dof_numbering=numbering_of(c))
    return M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, params_of(c, **extra)), prob


def check_form(h, c):
    f = h.restrictor_form(1)
    if not c["structured"]:
        assert f == {"structured": False}, (c["id"], f)
        return f
    want = c["form"]
    assert f["structured"] and f["n_eig"] == c["n_eig"] and f["a"] == tuple(c["agg"]), (c["id"], f)
    assert f["restrict"] == want["restrict"] and f["prolong"] == want["prolong"], (c["id"], f)
    if "float_planes" in want:
        assert f["float_planes"] == want["float_planes"], (c["id"], f)
    for key, field in (("table", "table_agglomerates"), ("classes", "n_classes"), ("listed", "listed_blocks")):
        if key not in want:
            continue
        if want[key] == "several":
            assert f[field] * 8 > 2 * 256 and (f[field] * 8) % 256 != 0, (c["id"], f)
        else:
            assert (f[field] > 0) == want[key], (c["id"], f)
    return f


def long_reference(R, x, z=None, transpose=False):
    """(R x) or z - R^T x in long double, and the bound gamma_k (|R| |x| + |z|) per entry, k = terms of the entry + 1."""
    Rc = R.tocoo()
    rows, cols = (Rc.col, Rc.row) if transpose else (Rc.row, Rc.col)
    n_out = R.shape[1] if transpose else R.shape[0]
    prod = Rc.data.astype(np.longdouble) * x[cols].astype(np.longdouble)
    ref = np.zeros(n_out, dtype=np.longdouble)
    mag = np.zeros(n_out, dtype=np.longdouble)
    np.add.at(ref, rows, prod)
    np.add.at(mag, rows, np.abs(prod))
    terms = np.bincount(rows, minlength=n_out)
    if z is not None:
        ref = z.astype(np.longdouble) - ref
        mag = mag + np.abs(z).astype(np.longdouble)
        terms = terms + 1
    k = (terms + 1).astype(np.float64)
    gamma = k * U / (1 - k * U)
    return ref.astype(np.float64), gamma * mag.astype(np.float64)


def assert_within(got, ref, bound, what):
    err = np.abs(got - ref)
    bad = ~(err <= bound)            # (NaN: an entry the kernel did not write)
    assert not bad.any(), f"{what}: {bad.sum()} entries beyond gamma_k (|R||x|), first at {np.flatnonzero(bad)[:5]}: " \
                          f"got {got[bad][:3]}, ref {ref[bad][:3]}, bound {bound[bad][:3]}"


def apply_all(ctx, h, n_f, n_c, x, y, z):
    rx = torch.empty(n_c, dtype=torch.float64, device="cuda")
    h.restrictor_apply(1, dev(x), rx)
    rty = torch.full((n_f,), float("nan"), dtype=torch.float64, device="cuda")
    h.restrictor_apply(1, dev(y), rty, L.TRANS)
    zs = dev(z)
    h.restrictor_apply(1, dev(y), zs, L.TRANS_SUBTRACT)
    ctx.synchronize()
    return rx, rty, zs


GPU = pytest.mark.gpu


@GPU
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_transfer_against_long_double(ctx, cid):
    """(a) R x, R^T y (into a NaN-filled output) and z - R^T y against the long-double products of the downloaded R;
    random x and one x whose entries span 1e-8 .. 1e8 with random signs (cancellation across agglomerate faces)."""
    c = BY_ID[cid]
    h, _ = build(ctx, c)
    check_form(h, c)
    R = h.restrictor().to_scipy()
    n_c, n_f = R.shape
    rng = np.random.default_rng(7)
    inputs = [(rng.random(n_f) - 0.5, rng.random(n_c) - 0.5),
              (10.0 ** rng.uniform(-8, 8, n_f) * rng.choice([-1, 1], n_f), 10.0 ** rng.uniform(-8, 8, n_c) * rng.choice([-1, 1], n_c))]
    for x, y in inputs:
        z = rng.random(n_f) - 0.5
        rx, rty, zs = apply_all(ctx, h, n_f, n_c, x, y, z)
        ref, bound = long_reference(R, x)
        assert_within(rx.cpu().numpy(), ref, bound, f"{cid}: R x")
        ref, bound = long_reference(R, y, transpose=True)
        assert_within(rty.cpu().numpy(), ref, bound, f"{cid}: R^T y")
        ref, bound = long_reference(R, y, z=z, transpose=True)
        assert_within(zs.cpu().numpy(), ref, bound, f"{cid}: z - R^T y")


SAME_BITS = [c["id"] for c in CASES if c["structured"] and c["numbering"] == "lexicographic"
             and (c["form"]["restrict"].startswith("pair") or c["form"]["prolong"] == "block222")
             and c["material"] in ("constant", "discontinuous")]


@GPU
@pytest.mark.parametrize("cid", SAME_BITS)
def test_alternative_kernels_give_the_same_bits(ctx, cid, monkeypatch):
    """(b) The row kernel (MFMG_SR_RESTRICT=rows) against pair<2> / pair<0>, and the node kernel (MFMG_SR_PROLONG=nodes)
    against the 2 x 2 x 2 block kernel: the same sums in the same order, so the same bits -- overwrite and subtract."""
    c = BY_ID[cid]
    h, _ = build(ctx, c)
    f = check_form(h, c)
    monkeypatch.setenv("MFMG_SR_RESTRICT", "rows")
    monkeypatch.setenv("MFMG_SR_PROLONG", "nodes")
    h_alt, _ = build(ctx, c)
    monkeypatch.delenv("MFMG_SR_RESTRICT")
    monkeypatch.delenv("MFMG_SR_PROLONG")
    g = h_alt.restrictor_form(1)
    assert g["restrict"] == "rows" and g["prolong"] == "nodes" and g["listed_blocks"] == 0, g
    assert g["table_agglomerates"] == f["table_agglomerates"] and g["n_classes"] == f["n_classes"]
    R = h.restrictor().to_scipy()
    assert abs(h_alt.restrictor().to_scipy() - R).max() == 0.0
    n_c, n_f = R.shape
    rng = np.random.default_rng(11)
    for scale in (False, True):
        x, y, z = rng.random(n_f) - 0.5, rng.random(n_c) - 0.5, rng.random(n_f) - 0.5
        if scale:
            x = x * 10.0 ** rng.uniform(-8, 8, n_f)
            y = y * 10.0 ** rng.uniform(-8, 8, n_c)
        a = apply_all(ctx, h, n_f, n_c, x, y, z)
        b = apply_all(ctx, h_alt, n_f, n_c, x, y, z)
        for what, u, v in zip(("R x", "R^T y", "z - R^T y"), a, b):
            assert torch.equal(u, v), f"{cid}: {what} differs in {(u != v).sum().item()} entries"


SETUP = [c["id"] for c in CASES if c["setup"]]


def oracle_setup(c, R_dev):
    """The oracle's R (lexicographic columns) and the Galerkin product of the product's own R."""
    mesh = O.StructuredMesh(c["n"])
    coef = O.coefficient_table(mesh, c["material"])
    mf = O.MatrixFreeLaplace(mesh, coef)
    perm = numbering_of(c)
    R_lex = R_dev if perm is None else R_dev[:, perm.numpy()]
    Ac = O.galerkin_coarse_matrix(mf.vmult, R_lex)
    return mesh, coef, mf, R_lex, Ac


@GPU
@pytest.mark.parametrize("on_device", [True, False], ids=["probing", "host"])
@pytest.mark.parametrize("cid", SETUP)
def test_setup_against_the_oracle(ctx, cid, on_device):
    """(c) R against the oracle's matrix-free AMGe restrictor (Krylov selection) to 1e-11, and the coarse operator --
    by colour probes on the device, or the host triple product (control) -- against the oracle's Galerkin product of
    the same R to 1e-11 relative, entry by entry and in its sparsity."""
    c = BY_ID[cid]
    try:
        ctx.set_galerkin_on_device(on_device)
        h, _ = build(ctx, c)
    finally:
        ctx.set_galerkin_on_device(True)
    check_form(h, c)
    R = h.restrictor().to_scipy()
    mesh, coef, mf, R_lex, Ac = oracle_setup(c, R)
    if c["numbering"] == "lexicographic":
        Ro = O.build_restrictor(mesh, coef, mf.diagonal(), agg=c["agg"], n_eig=c["n_eig"], variant="mf", eig_mode="krylov").csr
        if c["precision"] == "float":
            # the setup rounds R to float: one rounding of the oracle's value
            assert np.all(np.abs((R - Ro).toarray()) <= 2.0 ** -24 * np.abs(Ro.toarray()) + 1e-11)
        else:
            assert abs(R - Ro).max() < 1e-11
    Ag = h.coarse_operator().to_scipy()
    scale = abs(Ac).max()
    tol = (2.0 ** -23 if c["precision"] == "float" else 1e-11) * scale
    assert abs(Ag - Ac).max() < tol, f"{cid}: coarse operator differs by {abs(Ag - Ac).max() / scale:.3e} relative"
    big = abs(Ac).multiply(abs(Ac) > 1e-13 * scale)
    assert (abs(Ag).multiply(abs(Ag) > 1e-13 * scale) != 0).nnz == (big != 0).nnz


# With two eigenvectors, agglomerates one cell wide make R A R^T singular -- in the oracle as well: 16 eigenvalues below 1e-17
# of 384 on 12 x 8 x 8 cells with (1, 2, 2), 12 of 96 on 12 x 4 x 4 (the agglomerates at the Dirichlet faces have their free
# nodes on one node plane, which the next agglomerate shares); with one eigenvector it is singular too where only two
# agglomerates lie across the other axes (4 x 4 x 10 with (2, 2, 1)).  A dense solve of a singular system is not reproducible
# to rounding, so the two-eigenvector cases run with the aggregation coarse solver only (its coarsest level is regular).
CYCLES = [(cid, solver) for cid in ("one_cell122_ne1", "one_cell221_ne1", "const322_12x8x8", "const222_ne1", "linear222_ne3",
                                    "linear222_ne4", "clipped222_7x6x6") for solver in ("lu_dense", "amg")]
CYCLES += [("one_cell122_ne2", "amg"), ("one_cell221_ne2", "amg")]


@GPU
@pytest.mark.parametrize("cid,solver", CYCLES)
def test_cycles_against_the_oracle(ctx, cid, solver):
    """(d) 8 V-cycles against the oracle run on the product's R with its own Galerkin product: residual history to
    1e-10 and the final iterate.  lu_dense checks the Galerkin product alone; amg (device setup forced down to a few
    rows) checks the reach the aggregation setup starts from: its first operator is the oracle's Galerkin product, every
    coarser one P^T A P of the level above, and the levels equal those of the host setup."""
    c = BY_ID[cid]
    if solver == "amg":
        amg = {"coarsest_size": 8, "replicate_rows": 1, "setup": "device"}
        extra = {"solver": {"type": "amg", "amg": amg}}
    else:
        extra = {"solver": {"type": "lu_dense"}}
    h, prob = build(ctx, c, **extra)
    check_form(h, c)
    R = h.restrictor().to_scipy()
    mesh, coef, mf, R_lex, Ac = oracle_setup(c, R)
    scale = abs(Ac).max()
    assert abs(h.coarse_operator().to_scipy() - Ac).max() < 1e-11 * scale
    if solver == "amg":
        levels = h.coarse_amg_levels()
        assert len(levels) >= 2, "the aggregation hierarchy has no coarse level: the device setup was not exercised"
        assert abs(levels[0][0] - Ac).max() < 1e-11 * scale
        for (A, P, _), (A_next, _, _) in zip(levels[:-1], levels[1:]):
            G = (P.T @ A @ P).tocsr()
            assert abs(A_next - G).max() < 1e-11 * abs(G).max()
        amg["setup"] = "host"
        h_host, _ = build(ctx, c, **extra)
        host = h_host.coarse_amg_levels()
        assert len(host) == len(levels)
        for (A, P, cheb), (Ah, Ph, chebh) in zip(levels, host):
            assert A.shape == Ah.shape and abs(A - Ah).max() < 1e-11 * abs(Ah).max()
            if P is not None:
                assert abs(P - Ph).max() < 1e-11 * abs(Ph).max()
        del h_host
        coarse = O.amg_coarse_solver(levels, 1)
    else:
        coarse = O.direct_coarse_solver(Ac)
    deg, lmin, lmax = h.smoother_info()
    p = O.ChebyshevParams(deg, lmax, lmin)
    dinv = mf.diagonal_inverse()
    ho = O.TwoLevelHierarchy(mf.vmult, lambda b, x: O.chebyshev_smoother_apply(mf.vmult, dinv, p, b, x), R_lex, coarse, 1, False)
    x0 = O.random_initial_guess(mesh.n_dofs, mesh.constrained_mask())
    b = np.zeros(mesh.n_dofs)
    res_o, _, x_o = O.vcycle_history(ho, mf.vmult, b, x0, n_cycles=8)
    op = M.MatrixFreeLaplace(ctx, prob)
    x = dev(x0)
    bd = dev(b)
    r = torch.empty_like(x)
    op.vmult(r, x)
    r0 = ctx.l2_norm(r)
    res = [1.0]
    for _ in range(8):
        h.apply(bd, x)
        op.vmult(r, x)
        ctx.sadd(r, -1.0, 1.0, bd)
        res.append(ctx.l2_norm(r) / r0)
    ctx.synchronize()
    np.testing.assert_allclose(np.array(res), res_o, rtol=HIST_TOL, atol=HIST_ATOL)
    assert np.abs(x.cpu().numpy() - x_o).max() <= 1e-10 * np.abs(x0).max()
    assert res_o[-1] < res_o[1]


@GPU
def test_reference_device_hierarchy_parameters_with_one_eigenvector(ctx):
    """The reference's device hierarchy test (tests/golden/reference_hierarchy_input.info with one eigenvector, Jacobi):
    assembled operator, 2 x 2 x 2 agglomerates, dense coarse solve; the product's R A R^T and its cycle against the
    oracle's on the same R."""
    n = (8, 8, 8)
    mesh = O.StructuredMesh(n)
    coef = O.coefficient_table(mesh, "constant")
    con = mesh.constrained_mask()
    A = O.assemble_csr(mesh, coef)
    prob = M.LaplaceProblem(n, "constant", device="cuda")
    params = {"eigensolver": {"number of eigenvectors": 1, "tolerance": 1e-14}, "smoother": {"type": "Jacobi"},
              "is preconditioner": False, "agglomeration": {"partitioner": "block", "nx": 2, "ny": 2, "nz": 2},
              "max levels": 2, "solver": {"type": "lu_dense"}}
    h = M.Hierarchy(ctx, "HipMeshEvaluator", prob, params)
    assert h.level_size(1) == 64
    R = h.restrictor().to_scipy()
    Ac = (R @ A @ R.T).tocsr()
    assert abs(h.coarse_operator().to_scipy() - Ac).max() < 1e-11 * abs(Ac).max()
    dinv = 1.0 / A.diagonal()
    smoother = lambda b, x: O.smoother_wrapper(lambda v: A @ v, lambda r: dinv * r, b, x)
    ho = O.TwoLevelHierarchy(lambda v: A @ v, smoother, R, O.direct_coarse_solver(Ac), 1, False)
    x0 = np.where(con, 0.0, np.random.default_rng(2).random(mesh.n_dofs))
    b = np.zeros(mesh.n_dofs)
    res_o, _, x_o = O.vcycle_history(ho, lambda v: A @ v, b, x0, n_cycles=8)
    Ad = M.SparseMatrixDevice(ctx, A)
    x = dev(x0)
    r = torch.empty_like(x)
    Ad.vmult(r, x)
    r0 = ctx.l2_norm(r)
    res = [1.0]
    for _ in range(8):
        h.apply(dev(b), x)
        Ad.vmult(r, x)
        res.append(ctx.l2_norm(r) / r0)
    ctx.synchronize()
    np.testing.assert_allclose(np.array(res), res_o, rtol=HIST_TOL, atol=HIST_ATOL)
    assert np.abs(x.cpu().numpy() - x_o).max() <= 1e-10 * np.abs(x0).max()
