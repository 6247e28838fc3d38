"""The per-entry bound of the FP64 fine-level tests (fp32_reference.py with u = 2^-53) must bite: on the CPU, with the long-double
reference rounded to float64 standing in for a correct kernel, the checker passes; with one error planted at a time it fails.
The oracle's own float64 evaluation (its matrix-free operator and the three-term recurrence in numpy doubles) is a second
correct kernel and stays within the bound.  The same results under the rule the FP64 kernels are held to elsewhere, 1e-12 of the
max-norm (TOL of test_gpu_kernels.py): OLD_RULE_NOTICES lists the planted errors that rule notices on these inputs -- the rest
passes it unnoticed.

Inputs are those of test_gpu_fp64_fine_level.py: one coefficient per cell, 10^U(-3, 3); x and b signed and spread over six decades.
Worst |got - ref| / (u mag) of the oracle's float64 evaluation here (printed by the test): vmult 6.6 .. 7.3 against k = 16 and
4.2 .. 4.7 against k = 32 (eight coefficients per cell), x_3 of the sweep at most 0.4 against k = 28 / 44."""
import numpy as np
import pytest

import mfmg_oracle as O
import fp32_reference as F

MESHES = [(20, 17, 9), (64, 18, 6)]     # the general small case; 65 = 58 + 7 node columns: a narrow last chunk column
AL = [0.0, 0.23, 0.31]
BE = [0.61, 0.87, 0.79]
LD = np.longdouble
TOL = 1e-12                              # (test_gpu_kernels.py)

PLANTS = ["cell_missing_at_a_node", "dinv_from_7_of_8_cells", "cell_coefficient_off_2^-40", "beta_2_off_2^-42",
          "momentum_sign_in_one_row", "last_column_copied_from_its_neighbour", "dirichlet_row_treated_as_free"]
# what 1e-12 of the max-norm notices of them (the same on both meshes): with entries over six decades and coefficients over six
# more, the max-norm is set by a few large entries, and an error of the size of an ordinary entry is far below 1e-12 of it only
# where that entry is small.  The two errors of relative size 2^-40 = 9e-13 and 2^-42 pass it wherever they sit.
OLD_RULE_NOTICES = {"cell_missing_at_a_node", "dinv_from_7_of_8_cells", "momentum_sign_in_one_row",
                    "last_column_copied_from_its_neighbour", "dirichlet_row_treated_as_free"}


def test_long_double_has_a_64_bit_significand():
    """2^-11 of the FP64 unit roundoff: what makes np.longdouble a reference for doubles (fails, never skips, where it is not)."""
    assert np.finfo(LD).nmant >= 63
    assert F.K_REF * F.ULD / F.U64 < 0.05


def _inputs(n, eight=False):
    mesh = O.StructuredMesh(n)
    rng = np.random.default_rng(11)
    coef = np.repeat(10.0 ** rng.uniform(-3, 3, (mesh.n_cells, 1)), 8, axis=1)
    if eight:
        coef = coef * O.coefficient_table(mesh, "linear")          # eight different coefficients per cell, cells over six decades
    x = rng.standard_normal(mesh.n_dofs) * 10.0 ** rng.uniform(-3, 3, mesh.n_dofs)
    b = rng.standard_normal(mesh.n_dofs) * 10.0 ** rng.uniform(-3, 3, mesh.n_dofs)
    return mesh, coef, x, b


_SETUP = {}
WHAT = ("vmult", "step", "x_1", "x_2", "x_3")      # (x_1 and x_2 are what a sweep of two terms returns, x_2 and x_3 one of three)


def _setup(n, eight=False):
    if (n, eight) not in _SETUP:
        mesh, coef, x, b = _inputs(n, eight)
        _SETUP[(n, eight)] = (mesh, coef, F.Reference(n, coef, u=F.U64), x, b)
    return _SETUP[(n, eight)]


def _node(mesh, i, j, k):
    return i + mesh.N[0] * (j + mesh.N[1] * k)


def old_rule_passes(got, ref):
    """relerr(...) < TOL of test_gpu_kernels.py."""
    ref = np.asarray(ref).astype(float)
    return bool(np.abs(np.asarray(got).astype(float) - ref).max() / max(np.abs(ref).max(), 1e-300) < TOL)


def _wanted(ref, x, b):
    its = ref.sweep(x, b, AL, BE)
    xp = F.f64(its[1])
    want = {"vmult": ref.vmult(x), "step": ref.step(x, b, xp, AL[1], BE[1]), "x_1": its[1], "x_2": its[2], "x_3": its[3]}
    units = ref.unit_sweep(its, b, AL, BE)
    unit = {"vmult": ref.unit_vmult(x), "step": ref.unit_step(x, b, xp, AL[1], BE[1]), "x_1": units[0], "x_2": units[1], "x_3": units[2]}
    ks = {w: (ref.k_op if w == "vmult" else ref.k_step) + ref.k_ref for w in WHAT}
    return xp, want, unit, ks


_WANTED = {}


def _results(n, plant=None):
    """(what, float64 result, reference, unit of the bound, k) of the operator, a momentum step and the three-term sweep,
    computed in long double -- with one error planted in the computation -- and rounded to float64."""
    mesh, coef, ref, x, b = _setup(n)
    if n not in _WANTED:
        _WANTED[n] = _wanted(ref, x, b)
    xp, want, unit, ks = _WANTED[n]
    al, be = AL, BE

    # the computation a kernel with the planted error would do
    Nx = mesh.N[0]
    cell = 1 + mesh.n[0] * (1 + mesh.n[1] * 1)               # cell (1, 1, 1); its corner 0 is node (1, 1, 1), next to the mesh corner
    node = _node(mesh, 1, 1, 1)
    Ke, dinv, be_used, mom_sign = ref.Ke, ref.dinv, list(be), np.ones(mesh.n_dofs)
    if plant == "cell_coefficient_off_2^-40":
        # (per-entry means relative to the magnitude at a node, to which its eight cells contribute in proportion to their
        # coefficients: the twelfth digit of a cell a thousand times weaker than its neighbour is below any such bound, as it is
        # below the rounding of a correct kernel.  The cell is the one with the largest coefficient among those off the boundary.)
        inner = np.zeros(mesh.n[::-1], dtype=bool)
        inner[1:-1, 1:-1, 1:-1] = True
        big = int(np.argmax(np.where(inner.ravel(), coef[:, 0], 0.0)))
        Ke = ref.Ke.copy()
        Ke[big] *= 1 + LD(2.0) ** -40
    if plant == "dinv_from_7_of_8_cells":
        cells = np.ones(mesh.n_cells)
        cells[cell] = 0
        d7 = ref.dinv_from(coef, cells)
        dinv = ref.dinv.copy()
        dinv[node] = d7[node]
    if plant == "beta_2_off_2^-42":
        be_used[1] = be[1] * (1 + 2.0 ** -42)
    if plant == "momentum_sign_in_one_row":
        row = np.arange(Nx) + Nx * (5 + mesh.N[1] * 3)       # node row j = 5, k = 3
        mom_sign[row] = -1

    def vmult(v):
        cv = ref.cell_values(v, Ke)
        if plant == "cell_missing_at_a_node":
            cv[cell, 0] = 0
        y = ref.scatter(cv, v)
        if plant == "dirichlet_row_treated_as_free":
            c0 = _node(mesh, 3, 0, 2)                          # a node of the face j = 0: the sum of its cells instead of x
            free = np.zeros(mesh.n_dofs, dtype=LD)
            np.add.at(free, ref.cd.ravel(), cv.ravel())
            y[c0] = free[c0]
        return y

    def step(v, vp, alpha, beta):
        v = np.asarray(v).astype(LD)
        mom = LD(alpha) * mom_sign * (v - np.asarray(vp).astype(LD)) if vp is not None else 0
        return v + mom - LD(beta) * dinv * (vmult(v) - b.astype(LD))

    def narrow(v):
        if plant == "last_column_copied_from_its_neighbour":
            v = v.copy().reshape(mesh.N[::-1])
            v[:, :, -1] = v[:, :, -2]
            v = v.reshape(-1)
        return v

    got_its = [x.astype(LD)]
    for k in range(3):
        got_its.append(step(got_its[-1], got_its[-2] if k > 0 else None, al[k], be_used[k]))
    got = {"vmult": vmult(x), "step": step(x, xp, al[1], be_used[1]), "x_1": got_its[1], "x_2": got_its[2], "x_3": got_its[3]}
    return [(w, F.f64(narrow(got[w])), want[w], unit[w], ks[w]) for w in WHAT]


@pytest.mark.parametrize("n", MESHES)
def test_reference_rounded_to_double_is_within_the_bound(n):
    for what, got, want, unit, k in _results(n):
        F.assert_within(got, want, unit, k, f"{n} {what}")
        assert F.worst_ratio(got, want, unit) <= 1.0          # (one rounding of the result)
        assert old_rule_passes(got, want)


@pytest.mark.parametrize("eight", [False, True], ids=["one coefficient per cell", "eight coefficients per cell"])
@pytest.mark.parametrize("n", MESHES)
def test_the_oracle_in_float64_is_within_the_bound(n, eight):
    """A second correct kernel: the oracle's operator (gradients at the Gauss points, flux, integration: another order of
    operations than any kernel here) and the recurrence in numpy doubles."""
    mesh, coef, ref, x, b = _setup(n, eight)
    assert ref.cell_constant == (not eight) and ref.k_op == (F.K_OP_GENERAL if eight else F.K_OP_CC)
    op = O.MatrixFreeLaplace(mesh, coef)
    dinv = op.diagonal_inverse()
    assert not F.beyond(dinv, ref.dinv, F.K_DINV_F64 * F.U64 * ref.dinv).any()
    its = [x]
    for k in range(3):
        mom = AL[k] * (its[-1] - its[-2]) if k > 0 else 0.0
        its.append(its[-1] + mom - BE[k] * dinv * (op.vmult(its[-1]) - b))
    want = ref.sweep(x, b, AL, BE)
    units = ref.unit_sweep(want, b, AL, BE)
    for what, got, w, unit, k in (("vmult", op.vmult(x), ref.vmult(x), ref.unit_vmult(x), ref.k_op), ("x_1", its[1], want[1], units[0], ref.k_step),
                                  ("x_2", its[2], want[2], units[1], ref.k_step), ("x_3", its[3], want[3], units[2], ref.k_step)):
        print(f"{n} eight coefficients {eight} {what}: worst |got - ref| / (u mag) = {F.worst_ratio(got, w, unit):.2f} (k = {k})")
        F.assert_within(got, w, unit, k + ref.k_ref, f"{n} {what}")


def test_an_entry_nobody_wrote_is_a_failure():
    what, got, want, unit, k = _results(MESHES[0])[0]
    got = got.copy()
    got[77] = np.nan
    assert F.beyond(got, want, k * unit).sum() == 1
    with pytest.raises(AssertionError):
        F.assert_within(got, want, unit, k, "vmult")


@pytest.mark.parametrize("n", MESHES)
@pytest.mark.parametrize("plant", PLANTS)
def test_planted_error_is_beyond_the_bound(n, plant):
    results = _results(n, plant)
    caught = [what for what, got, want, unit, k in results if F.beyond(got, want, k * unit).any()]
    assert caught, f"{n} {plant}: within the bound in every operation"
    # the operation that contains the planted computation directly must notice it, and so must the sweep in one of its outputs
    # (the propagated bounds of x_2 and x_3 are wider than that of x_1, and with neighbouring cells six decades apart the cell
    # with the wrong coefficient may carry little of its nodes: an error in its twelfth digit is caught in x_1, the first
    # iterate that holds A x_0, and may pass the later ones)
    direct = "vmult" if plant in ("cell_missing_at_a_node", "cell_coefficient_off_2^-40", "last_column_copied_from_its_neighbour",
                                  "dirichlet_row_treated_as_free") else "step"
    assert direct in caught and {"x_1", "x_2", "x_3"} & set(caught), (n, plant, caught)
    if plant not in ("beta_2_off_2^-42", "momentum_sign_in_one_row"):    # (these two enter with the second term)
        assert "x_1" in caught, (n, plant, caught)
    noticed_by_old_rule = not all(old_rule_passes(got, want) for _, got, want, _, _ in results)
    print(f"{n} {plant}: beyond the bound in {caught}; 1e-12 of the max-norm notices it: {noticed_by_old_rule}")
    assert noticed_by_old_rule == (plant in OLD_RULE_NOTICES), (n, plant)
