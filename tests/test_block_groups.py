"""How a block of k vectors is cut into launches (mfmg_hip_block_groups; host only, no GPU, no context): groups of 4, then one
of 2, then one single vector."""
import ctypes as C

import pytest

from mfmg_amd import lib as L
from mfmg_amd.api import block_groups


@pytest.mark.parametrize("k", range(1, 65))
def test_groups_of_every_block_size(mfmg_lib, k):
    w = block_groups(k)
    assert sum(w) == k
    assert set(w) <= {4, 2, 1}
    assert w == sorted(w, reverse=True)
    assert w.count(2) <= 1 and w.count(1) <= 1
    assert w == [4] * (k // 4) + [2] * ((k % 4) // 2) + [1] * (k % 2)


@pytest.mark.parametrize("k", [0, 65, -1])
def test_sizes_outside_the_range_are_refused(mfmg_lib, k):
    with pytest.raises(L.MfmgInvalidArgument, match="1 to 64"):
        block_groups(k)


def test_null_arguments_are_refused(mfmg_lib):
    n = C.c_int32()
    assert mfmg_lib.mfmg_hip_block_groups(3, None, C.byref(n)) == L.ERROR_INVALID_ARGUMENT
