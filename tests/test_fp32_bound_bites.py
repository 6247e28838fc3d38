"""The per-entry bound of the FP32 fine-level tests (fp32_reference.py) must bite: on the CPU, with the long-double reference
rounded to float32 standing in for a correct kernel, the checker passes; with one error planted at a time it fails.  The same
results under the rule that was all the float kernels had before, 1e-4 of the max-norm (test_mf_fp32_instance): OLD_RULE_NOTICES
lists the planted errors that rule notices on these inputs -- the rest passes it unnoticed."""
import numpy as np
import pytest

import mfmg_oracle as O
import fp32_reference as F

MESHES = [(20, 17, 9), (64, 18, 6)]     # the general small case; 65 = 58 + 7 node columns: a narrow last chunk column
AL = [0.0, 0.23, 0.31]
BE = [0.61, 0.87, 0.79]
LD = np.longdouble

PLANTS = ["cell_missing_at_a_node", "dinv_from_7_of_8_cells", "cell_coefficient_off_2^-10", "beta_2_off_2^-12",
          "momentum_sign_in_one_row", "last_column_copied_from_its_neighbour", "dirichlet_row_treated_as_free"]
# what 1e-4 of the max-norm notices of them (the same on both meshes): errors of the size of the entries themselves -- the whole
# contribution of a cell, a boundary value replaced by an interior one -- and beta_2, whose 2.4e-4 relative error acts on the whole
# vector through the dominant term of the step.  A coefficient off in the fourth digit of one cell passes it.
OLD_RULE_NOTICES = {"cell_missing_at_a_node", "dinv_from_7_of_8_cells", "beta_2_off_2^-12", "momentum_sign_in_one_row",
                    "last_column_copied_from_its_neighbour", "dirichlet_row_treated_as_free"}


def _setup(n):
    mesh = O.StructuredMesh(n)
    rng = np.random.default_rng(11)
    coef = np.repeat(0.5 + rng.random((mesh.n_cells, 1)), 8, axis=1)
    ref = F.Reference(n, coef)
    x, b = F.f32(rng.standard_normal(mesh.n_dofs)), F.f32(rng.standard_normal(mesh.n_dofs))
    return mesh, coef, ref, x, b


def _node(mesh, i, j, k):
    return i + mesh.N[0] * (j + mesh.N[1] * k)


def _results(n, plant=None):
    """(what, float32 result, reference, unit of the bound, k) of the operator, a momentum step and the three-term sweep,
    computed in long double -- with one error planted in the computation -- and rounded to float32."""
    mesh, coef, ref, x, b = _setup(n)
    al, be = [float(np.float32(v)) for v in AL], [float(np.float32(v)) for v in BE]
    its = ref.sweep(x, b, al, be)
    want = {"vmult": ref.vmult(x), "step": ref.step(x, b, its[1].astype(np.float32), al[1], be[1]), "x_2": its[2], "x_3": its[3]}
    xp = its[1].astype(np.float32)
    units = ref.unit_sweep(its, b, al, be)
    unit = {"vmult": ref.unit_vmult(x), "step": ref.unit_step(x, b, xp, al[1], be[1]), "x_2": units[1], "x_3": units[2]}
    ks = {"vmult": ref.k_op, "step": ref.k_step, "x_2": ref.k_step, "x_3": ref.k_step}

    # the computation a kernel with the planted error would do
    Nx = mesh.N[0]
    cell = 1 + mesh.n[0] * (1 + mesh.n[1] * 1)               # cell (1, 1, 1); its corner 0 is node (1, 1, 1), next to the mesh corner
    node = _node(mesh, 1, 1, 1)
    Ke, dinv, be_used, mom_sign = ref.Ke, ref.dinv, list(be), np.ones(mesh.n_dofs)
    if plant == "cell_coefficient_off_2^-10":
        Ke = ref.Ke.copy()
        Ke[cell] *= 1 + LD(2.0) ** -10
    if plant == "dinv_from_7_of_8_cells":
        cells = np.ones(mesh.n_cells)
        cells[cell] = 0
        d7 = ref.dinv_from(coef, cells)
        dinv = ref.dinv.copy()
        dinv[node] = d7[node]
    if plant == "beta_2_off_2^-12":
        be_used[1] = be[1] * (1 + 2.0 ** -12)
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
    got = {"vmult": vmult(x), "step": step(x, xp, al[1], be_used[1]), "x_2": got_its[2], "x_3": got_its[3]}
    return [(w, F.f32(narrow(got[w])), want[w], unit[w], ks[w]) for w in ("vmult", "step", "x_2", "x_3")]


@pytest.mark.parametrize("n", MESHES)
def test_reference_rounded_to_float_is_within_the_bound(n):
    for what, got, want, unit, k in _results(n):
        F.assert_within(got, want, unit, k, f"{n} {what}")
        assert F.worst_ratio(got, want, unit) <= 1.0          # (one rounding of the result)
        assert F.old_rule_passes(got, want)


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
    # (the propagated bound of x_3 is wider than that of x_2: an error in the fourth digit of one cell may pass it)
    direct = "vmult" if plant in ("cell_missing_at_a_node", "cell_coefficient_off_2^-10", "last_column_copied_from_its_neighbour",
                                  "dirichlet_row_treated_as_free") else "step"
    assert direct in caught and ("x_2" in caught or "x_3" in caught), (n, plant, caught)
    noticed_by_old_rule = not all(F.old_rule_passes(got, want) for _, got, want, _, _ in results)
    print(f"{n} {plant}: beyond the bound in {caught}; 1e-4 of the max-norm notices it: {noticed_by_old_rule}")
    assert noticed_by_old_rule == (plant in OLD_RULE_NOTICES), (n, plant)
