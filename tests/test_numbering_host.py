"""Driver-side numbering helper and the ABI additions of "internal numbering" (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mfmg_amd as M
import mfmg_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mfmg_hip_hierarchy_internal_numbering", "mfmg_hip_hierarchy_permute")


@pytest.mark.parametrize("n", [(4, 4), (8, 8), (4, 4, 4), (8, 8, 8), (16, 16, 16)])
def test_dealii_numbering_equals_the_oracle(n):
    """Morton cells, vertex DoFs at first touch: the vectorised recipe against the oracle's cell loop."""
    got = M.laplace.dealii_numbering(n)
    assert got.dtype.is_floating_point is False and got.numel() == int(np.prod([v + 1 for v in n]))
    np.testing.assert_array_equal(got.numpy(), O.dealii_global_numbering(O.StructuredMesh(n)))


def test_dealii_numbering_is_a_permutation_at_64_cubed():
    ids = M.laplace.dealii_numbering((64, 64, 64)).numpy()
    assert ids.shape == (65 ** 3,)
    np.testing.assert_array_equal(np.sort(ids), np.arange(65 ** 3))
    assert ids[0] == 0 and not np.array_equal(ids, np.arange(65 ** 3))


def test_dealii_numbering_refuses_other_meshes():
    with pytest.raises(AssertionError):
        M.laplace.dealii_numbering((6, 6, 6))
    with pytest.raises(AssertionError):
        M.laplace.dealii_numbering((8, 4, 4))


def test_header_binding_and_library_carry_the_new_symbols(mfmg_lib):
    text = open(os.path.join(ROOT, "include", "mfmg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mfmg_hip_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(M.lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared
        assert name in mfmg_lib._declared
        assert hasattr(raw, name)
    assert int(re.search(r"#define\s+MFMG_HIP_ABI_VERSION\s+(\d+)", text).group(1)) == 3
