"""The tile march of the one-pass residual restriction b_c = R (A x - b) (residual_restriction_tile_kernel) at every tile height.

Without MFMG_RR_TILE_LAYERS a mesh of fewer than 512 tiles marches one agglomerate layer per tile: one write, at the fifth node
layer, and the three agglomerate layers in flight per wavefront (P ends, C in its middle, N starts) are never live together.  The
height is read when the tables of a restrictor are built, so the cases of rr_cases.py (the comment of each edge in
test_rr_case_table.py says what it is there for) build one hierarchy per height in one process.  Per case:
  (a) the launch is the one the case names -- Hierarchy.residual_restriction_form() against the planning restated in rr_cases.py;
  (b) the bits of MFMG_RR_KERNEL=rows and of height 1 on the same mesh (so of every other height: the comparison is transitive),
      into NaN-filled vectors;
  (c) per row within gamma_256 |R| (|A| |x| + |b|) of R (A x - b) in long double, A assembled by the oracle from the coefficient
      table of the case, x and b standard normal and spread over 16 decades;
  (d) restrict_residual_f32 on float32 vectors: the bits of the FP64 entry on the widened vectors, the same bound;
  (e) at the largest height of a mesh: x and b as views one element into a larger buffer (FP64 off the 16-byte grid of the
      kernel's requests, FP32 off the 8-byte grid): the bits of the aligned call.

Worst |got - ref| / (2^-53 mag) observed on an MI355X per case (printed when the module's fixture is torn down): see CHANGELOG.md."""
import numpy as np
import pytest
import torch

import mfmg_amd as M
import rr_cases as C

pytestmark = pytest.mark.gpu

def _hierarchy(ctx, name, height=0, kernel=None, precision="double"):
    cells = C.MESHES[name][0]
    prob = M.LaplaceProblem(cells, "constant", device="cuda")
    prob.coefficient = torch.from_numpy(C.coefficient(name)).cuda()
    params = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": False,
              "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0},
              "solver": {"type": "pcg", "n_iterations": 2}}     # (never applied here: no dense factorisation of up to 14960 coarse rows)
    if precision == "float":
        params["fine level precision"] = "float"
    with pytest.MonkeyPatch.context() as mp:                     # (both switches are read when the tables of a restrictor are built)
        mp.delenv("MFMG_RR_TILE_LAYERS", raising=False)
        mp.delenv("MFMG_RR_KERNEL", raising=False)
        if height:
            mp.setenv("MFMG_RR_TILE_LAYERS", str(height))
        if kernel:
            mp.setenv("MFMG_RR_KERNEL", kernel)
        h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, params)
    return h


def _form(h):
    f = h.residual_restriction_form()
    assert f["classes"] == h.residual_restriction_classes()
    return f


def _assert_form(h, name, height, kernel="tile"):
    f, want = _form(h), C.expected_form(name, height, kernel)
    assert f["classes"] > 0, f"{name}: the one-pass form is not built ({f})"
    assert {k: f[k] for k in C.FORM_KEYS} == want, (name, height, kernel, f)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(ctx, h, x, b, single=False):
    out = torch.full((h.level_size(1),), float("nan"), dtype=torch.float64, device="cuda")
    (h.restrict_residual_f32 if single else h.restrict_residual)(x, b, out)
    ctx.synchronize()
    return out


@pytest.fixture(scope="module")
def meshes(ctx):
    """Per mesh, built when its first case runs and freed with the module: the data sets on the device, the outputs of
    MFMG_RR_KERNEL=rows and of height 1, the long-double references; `worst` collects the ratios, printed at the end."""
    cache, worst = {}, {}

    def get(name):
        if name in cache:
            return cache[name]
        h_rows, h_one = _hierarchy(ctx, name, kernel="rows"), _hierarchy(ctx, name, height=1)
        _assert_form(h_rows, name, 0, "rows")
        _assert_form(h_one, name, 1)
        R = h_rows.restrictor().to_scipy()
        assert abs(h_one.restrictor().to_scipy() - R).max() == 0.0
        nf = h_rows.level_size(0)
        sets = []
        for single in (False, True):
            for x, b in C.data_sets(name, nf, single):
                xd, bd = _gpu(x), _gpu(b)
                wide = (xd.double(), bd.double())
                sets.append({"single": single, "x": xd, "b": bd, "wide": wide, "ref": C.reference(name, R, x, b),
                             "rows": _run(ctx, h_rows, *wide), "one": _run(ctx, h_one, *wide)})
        cache[name] = sets
        return sets

    get.worst = worst
    yield get
    for what, ratio in worst.items():
        print(f"{what}: worst |got - ref| / (2^-53 mag) = {ratio:.2f}")
    cache.clear()


def _same(got, other, what):
    assert torch.equal(got, other), f"{what}: {(got != other).sum().item()} rows differ, first at {torch.nonzero(got != other)[:5].flatten().tolist()}"


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_tile_march_at_this_height(ctx, meshes, case):
    name, height = case
    what = C.case_id(case)
    h = _hierarchy(ctx, name, height)
    _assert_form(h, name, height)                                                       # (a), before anything else
    hf = _hierarchy(ctx, name, height, precision="float")
    _assert_form(hf, name, height)
    sets = meshes(name)
    nf = h.level_size(0)
    for n_set, s in enumerate(sets):
        tag = f"{what} {'float32' if s['single'] else 'float64'} data set {n_set % 2}"
        got = _run(ctx, h, *s["wide"])
        _same(got, s["rows"], f"{tag}: against MFMG_RR_KERNEL=rows")                     # (b)
        _same(got, s["one"], f"{tag}: against height 1")
        if s["single"]:
            _same(_run(ctx, hf, s["x"], s["b"], single=True), got, f"{tag}: restrict_residual_f32 against the FP64 entry")   # (d)
            _same(_run(ctx, hf, *s["wide"]), got, f"{tag}: the FP64 entry of the float hierarchy")
        want, mag = s["ref"]
        g = got.cpu().numpy()
        ratio = C.worst_ratio(g, want, mag)
        meshes.worst[what] = max(meshes.worst.get(what, 0.0), ratio)
        print(f"{tag}: worst |got - ref| / (2^-53 mag) = {ratio:.2f} (k = {C.K_RR})")
        bad = C.beyond(g, want, mag)                                                     # (c)
        assert not bad.any(), f"{tag}: {int(bad.sum())} rows beyond gamma_{C.K_RR}, first at {np.flatnonzero(bad)[:5]}"
        if height == max(C.MESHES[name][2]):                                             # (e)
            hh, single = (hf, True) if s["single"] else (h, False)
            bx, bb = (torch.zeros(nf + 2, dtype=s["x"].dtype, device="cuda") for _ in range(2))
            bx[1:nf + 1], bb[1:nf + 1] = s["x"], s["b"]
            assert bx[1:nf + 1].data_ptr() % (2 * bx.element_size()) == bx.element_size()
            _same(_run(ctx, hh, bx[1:nf + 1], bb[1:nf + 1], single), got, f"{tag}: x and b one element off the grid of the requests")


def test_unset_height_is_the_automatic_choice(ctx):
    """MFMG_RR_TILE_LAYERS unset: the height of whole rounds of two workgroups per CU, as before it became a property of the
    restrictor -- and two restrictors of one process keep their own."""
    name = "62+24"
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    h_auto, h_five = _hierarchy(ctx, name), _hierarchy(ctx, name, height=5)
    want = C.expected_form(name, 0, n_cus=n_cus)
    f = _form(h_auto)
    assert want["tile_layers"] == 1 and {k: f[k] for k in C.FORM_KEYS} == want, f
    assert _form(h_five)["tile_layers"] == 5 and _form(h_auto)["tile_layers"] == 1
    # a height above the layers of the mesh is the whole column
    assert _form(_hierarchy(ctx, name, height=99))["tile_layers"] == 5


def test_form_of_a_mesh_without_the_one_pass_form(ctx):
    prob = M.LaplaceProblem((9, 7, 5), "constant", device="cuda")
    params = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2}, "is preconditioner": False,
              "max levels": 2, "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0}}
    h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, params)
    assert h.residual_restriction_form() == dict.fromkeys(("classes", "segs", "main_last", "listed", "listed_runs", "tile_layers", "tiles_j",
                                                           "n_tiles", "main_blocks"), 0) | {"kernel": None}

