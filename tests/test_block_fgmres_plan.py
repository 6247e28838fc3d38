"""The step plan of Hierarchy.solve_fgmres_block (mfmg_hip_block_fgmres_plan, host only) against a restatement in Python: the
maximal runs of consecutive live slots -- what one call of apply_block takes --, each cut into the launches of block_groups, and
the slot -> column map of the next restart cycle, which packs the surviving columns into the first slots in their order.  Every
live pattern of 1 to 8 slots, 200 seeded random patterns at 64, the refusals.  And the header declares the block FGMRES driver."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from mfmg_amd import lib as L
from mfmg_amd.api import block_fgmres_plan, block_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(live, slot_col):
    runs, s, k = [], 0, len(live)
    while s < k:
        if not live[s]:
            s += 1
            continue
        e = s
        while e < k and live[e]:
            e += 1
        runs.append((s, e - s, block_groups(e - s)))
        s = e
    return runs, [slot_col[s] for s in range(k) if live[s]]


def _check(live, slot_col):
    runs, packed = block_fgmres_plan(live, slot_col)
    assert (runs, packed) == _plan(live, slot_col), (live, runs, packed)
    k = len(live)
    # the runs cover exactly the live slots, in order, and are maximal: a dead slot or an end on either side
    covered = [s for start, width, _ in runs for s in range(start, start + width)]
    assert covered == [s for s in range(k) if live[s]], (live, runs)
    for start, width, groups in runs:
        assert width >= 1 and (start == 0 or not live[start - 1]) and (start + width == k or not live[start + width]), (live, runs)
        # the launches of a run: no wider than the block kernel takes, together the run
        assert sum(groups) == width and all(1 <= g <= max(block_groups(64)) for g in groups), (live, runs)
        assert groups == block_groups(width)
    # the packed map keeps the order of the columns' slots (no basis vector moves: the next cycle recomputes v_0 in the new slot)
    assert packed == [slot_col[s] for s in covered]
    assert len(set(packed)) == len(packed)


@pytest.mark.parametrize("k", range(1, 9))
def test_every_live_pattern(mfmg_lib, k):
    rng = np.random.default_rng(k)
    for live in itertools.product([0, 1], repeat=k):
        _check(list(live), [int(c) for c in rng.permutation(64)[:k]])


def test_random_patterns_at_64(mfmg_lib):
    rng = np.random.default_rng(64)
    for i in range(200):
        p = (0.05, 0.5, 0.95)[i % 3]
        _check([int(f) for f in rng.random(64) < p], [int(c) for c in rng.permutation(64)])
    _check([1] * 64, list(range(64)))


def test_no_slot(mfmg_lib):
    assert block_fgmres_plan([], []) == ([], [])
    assert block_fgmres_plan([0, 0, 0], [2, 1, 0]) == ([], [])


def test_refusals(mfmg_lib):
    arr = (C.c_int32 * 65)(*([1] * 65))
    out = [(C.c_int32 * 65)() for _ in range(5)]
    n = [C.c_int32() for _ in range(3)]

    def call(k, args):
        return mfmg_lib.mfmg_hip_block_fgmres_plan(k, args[0], args[1], args[2], args[3], args[4], args[5], args[6], args[7], args[8],
                                                   args[9])

    full = [arr, arr, out[0], out[1], out[2], C.byref(n[0]), out[3], C.byref(n[1]), out[4], C.byref(n[2])]
    assert call(64, full) == L.SUCCESS and n[0].value == 1 and n[2].value == 64
    assert call(65, full) == L.ERROR_INVALID_ARGUMENT                       # more slots than a block holds
    assert call(-1, full) == L.ERROR_INVALID_ARGUMENT
    for missing in range(10):                                               # every argument, when null
        args = list(full)
        args[missing] = None
        assert call(4, args) == L.ERROR_INVALID_ARGUMENT, missing
    with pytest.raises(ValueError):
        block_fgmres_plan([1, 1], [0])


def test_header_declares_the_block_fgmres_driver():
    text = open(os.path.join(ROOT, "include", "mfmg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mfmg_hip_[a-z0-9_]+)\s*\(", text))
    for name in ("mfmg_hip_hierarchy_solve_fgmres_block", "mfmg_hip_block_fgmres_plan", "mfmg_hip_block_krylov_orthogonalize",
                 "mfmg_hip_block_krylov_combine"):
        assert name in declared, name
