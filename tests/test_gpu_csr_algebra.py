"""The device transpose and the device sparse product (mfmg_amd/csrc/csr_algebra.hip) at every table and sort edge: the cases of
csr_algebra_cases.py (test_csr_algebra_case_table.py says which edge each is there for, and shows that the checks below bite).

Per case that the device serves, under MFMG_CSR_ALGEBRA=device_only so that nothing passes through the host algorithm:
  (a) indptr, indices and the bits of the values are those of a reference written in plain numpy -- the Gustavson sum in float64 in
      storage order, multiply then add (float data); the int64 product (integer data, the stride cases); a stable sort by column
      (transposes) -- with the columns of every row strictly increasing;
  (b) float products: per entry within gamma_{m+1} (|A| |B|) of the sum in long double, m the number of terms of the entry;
  (c) a second launch gives the same bits (the slot a column gets depends on which thread wins the CAS; the result must not);
  (d) MFMG_CSR_ALGEBRA=host gives the same bits;
  (e) float cases: the result, applied to a six-decade vector, is within gamma_{len+1} (|M| |x|) per row of the long-double product
      with the reference matrix (a transpose stays on the device, so this is where the layout analysis meets rows of 65 .. 4096
      entries that were sorted there).
Per case beyond the LDS tables: device_only raises, the default mode returns the reference.

Not reached from here: the `float` instances of both algorithms (mfmg_hip_csr_create takes doubles; the C ABI has no entry that
builds a SparseMatrixDevice<float> from values) and the stride of count_columns_kernel (beyond 65536 x 256 = 16.7 M nonzeros).

Worst |got - ref| / (2^-53 mag), printed when the module's fixture is torn down.  Seen on an MI355X: 3.72 over the float products
(direct-100, whose entries are sums of up to 28 terms: the bound there is gamma_29), 2.37 over the applied results
(chain-1024-twice).  The device returned the bits of the numpy reference in every case, so the first figure is that of the
reference itself.  This is documentation, not a threshold."""
import numpy as np
import pytest
import torch

import csr_algebra_cases as C
import mfmg_amd as M

pytestmark = pytest.mark.gpu

FALLBACK_PRODUCTS, FALLBACK_TRANSPOSES = ["fallback-2049-8193"], ["one-column-4097"]
DEVICE_PRODUCTS = [n for n in C.PRODUCTS if n not in FALLBACK_PRODUCTS]
DEVICE_TRANSPOSES = [n for n in C.TRANSPOSES if n not in FALLBACK_TRANSPOSES]
ENV = "MFMG_CSR_ALGEBRA"


@pytest.fixture(scope="module")
def worst():
    ratios = {}
    yield ratios
    for what, (ratio, name) in ratios.items():
        print(f"{what}: worst |got - ref| / (2^-53 mag) = {ratio:.2f} ({name})")


def _device(ctx, matrix):
    return M.SparseMatrixDevice(ctx, tuple(matrix))


def _record(worst, what, ratio, name):
    if ratio >= worst.get(what, (-1.0, None))[0]:
        worst[what] = (ratio, name)


def _assert_product_bound(worst, name, got, case):
    _, want, mag, m = case["long"]
    ratio = C.worst_ratio(got.data, want, mag)
    print(f"{name}: worst |got - ref| / (2^-53 mag) = {ratio:.2f} (m <= {m.max()})")
    _record(worst, "product", ratio, name)
    bad = C.beyond_product_bound(got.data, want, mag, m)
    assert not bad.any(), f"{name}: {int(bad.sum())} entries beyond gamma_(m+1) mag, first at {np.flatnonzero(bad)[:5]}"


def _assert_usable(ctx, worst, name, device_matrix, reference):
    """(e): the matrix as the library holds it, applied."""
    m, n = reference.shape
    assert device_matrix.shape == (m, n)
    x = C.vector_for(name, n)
    y = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
    device_matrix.apply(torch.from_numpy(x).cuda(), y)
    ctx.synchronize()
    want, mag, length = C.spmv_long(reference, x)
    got = y.cpu().numpy()
    _record(worst, "applied", C.worst_ratio(got, want, mag), name)
    bad = C.beyond_spmv_bound(got, want, mag, length)
    assert not bad.any(), f"{name}: applied, {int(bad.sum())} rows beyond gamma_(len+1) |M| |x|, first at {np.flatnonzero(bad)[:5]}"


@pytest.mark.parametrize("name", DEVICE_PRODUCTS)
def test_product_on_the_device(ctx, monkeypatch, worst, name):
    case = C.product_case(name)
    assert case["path"] in ("hash", "direct")
    Ad, Bd = _device(ctx, case["A"]), _device(ctx, case["B"])
    monkeypatch.setenv(ENV, "device_only")
    Cd = Ad.multiply(Bd)
    got = Cd.to_scipy()
    C.assert_same_csr(got, case["bits"], f"{name} ({case['path']}) against the reference")            # (a)
    C.assert_same_csr(Ad.multiply(Bd).to_scipy(), got, f"{name}: second launch against the first")    # (c)
    monkeypatch.setenv(ENV, "host")
    C.assert_same_csr(Ad.multiply(Bd).to_scipy(), got, f"{name}: host algorithm against the device")  # (d)
    if case["data"] == "float":
        _assert_product_bound(worst, name, got, case)                                                  # (b)
        _assert_usable(ctx, worst, name, Cd, case["bits"])                                             # (e)


@pytest.mark.parametrize("name", DEVICE_TRANSPOSES)
def test_transpose_on_the_device(ctx, monkeypatch, worst, name):
    case = C.transpose_case(name)
    assert case["path"] == "device"
    Ad = _device(ctx, case["A"])
    monkeypatch.setenv(ENV, "device_only")
    Td = Ad.transpose()
    got = Td.to_scipy()
    C.assert_same_csr(got, case["bits"], f"{name} against the reference")                              # (a)
    C.assert_same_csr(Ad.transpose().to_scipy(), got, f"{name}: second launch against the first")      # (c)
    monkeypatch.setenv(ENV, "host")
    C.assert_same_csr(Ad.transpose().to_scipy(), got, f"{name}: host algorithm against the device")    # (d)
    if case["data"] == "float":
        _assert_usable(ctx, worst, f"{name} transposed", Td, case["bits"])                             # (e)


@pytest.mark.parametrize("name", FALLBACK_PRODUCTS)
def test_product_beyond_the_tables_falls_back(ctx, monkeypatch, worst, name):
    case = C.product_case(name)
    assert case["path"] == "fallback"
    Ad, Bd = _device(ctx, case["A"]), _device(ctx, case["B"])
    monkeypatch.setenv(ENV, "device_only")
    with pytest.raises(RuntimeError, match="LDS tables"):
        Ad.multiply(Bd)
    monkeypatch.delenv(ENV)
    got = Ad.multiply(Bd).to_scipy()
    C.assert_same_csr(got, case["bits"], f"{name}: default mode against the reference")
    _assert_product_bound(worst, name, got, case)


@pytest.mark.parametrize("name", FALLBACK_TRANSPOSES)
def test_transpose_beyond_the_sort_falls_back(ctx, monkeypatch, name):
    case = C.transpose_case(name)
    assert case["path"] == "fallback"
    Ad = _device(ctx, case["A"])
    monkeypatch.setenv(ENV, "device_only")
    with pytest.raises(RuntimeError, match="LDS tables"):
        Ad.transpose()
    monkeypatch.delenv(ENV)
    C.assert_same_csr(Ad.transpose().to_scipy(), case["bits"], f"{name}: default mode against the reference")
