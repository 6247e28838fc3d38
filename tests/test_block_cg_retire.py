"""The slot-move plan of Hierarchy.solve_cg_block (mfmg_hip_block_cg_retire, host only) against a restatement in Python: when
slots of the working blocks retire, each retired slot -- in ascending order -- is filled from the last slot that survives behind
it.  Every flag pattern for 1 to 7 active slots, 200 seeded random patterns at 64.  And the header declares the entry points of
the block driver."""
import itertools
import os
import re

import numpy as np
import pytest

from mfmg_amd.api import block_cg_retire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(flags, slot_col):
    cols, alive, moves = list(slot_col), [not f for f in flags], []
    n = len(flags)
    for s in range(n):
        if alive[s] or s >= n:
            continue
        while n > s + 1 and not alive[n - 1]:
            n -= 1                                   # the last slot that survives
        if n - 1 > s:
            moves.append((n - 1, s))
            cols[s], alive[s], alive[n - 1] = cols[n - 1], True, False
    return moves, cols, sum(alive)


def _check(flags, slot_col):
    moves, cols, n_out = block_cg_retire(flags, slot_col)
    want_moves, want_cols, want_out = _plan(flags, slot_col)
    n = len(flags)
    survivors = {slot_col[s] for s in range(n) if not flags[s]}
    assert n_out == want_out == len(survivors), (flags, n_out)
    # the active slots are contiguous: the first n_out slots hold exactly the surviving columns, each once
    assert sorted(cols[:n_out]) == sorted(survivors), (flags, cols)
    assert len(moves) <= sum(map(bool, flags)), (flags, moves)
    for src, dst in moves:
        assert not flags[src] and flags[dst] and dst < n_out <= src, (flags, moves)      # no retired source, into the front
        assert cols[dst] == slot_col[src]
    assert len({m[0] for m in moves}) == len(moves) == len({m[1] for m in moves})
    # a survivor that does not move keeps its slot
    moved = {m[0] for m in moves}
    for s in range(n):
        if not flags[s] and s not in moved:
            assert s < n_out and cols[s] == slot_col[s]
    assert moves == want_moves and cols[:n_out] == want_cols[:n_out], (flags, moves, want_moves)


@pytest.mark.parametrize("n_active", range(1, 8))
def test_every_flag_pattern(mfmg_lib, n_active):
    rng = np.random.default_rng(n_active)
    for flags in itertools.product([0, 1], repeat=n_active):
        _check(list(flags), [int(c) for c in rng.permutation(64)[:n_active]])


def test_random_patterns_at_64(mfmg_lib):
    rng = np.random.default_rng(64)
    for i in range(200):
        p = (0.05, 0.5, 0.95)[i % 3]
        _check([int(f) for f in rng.random(64) < p], [int(c) for c in rng.permutation(64)])


def test_nothing_active(mfmg_lib):
    assert block_cg_retire([], []) == ([], [], 0)


def test_header_declares_the_block_driver():
    text = open(os.path.join(ROOT, "include", "mfmg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mfmg_hip_[a-z0-9_]+)\s*\(", text))
    for name in ("mfmg_hip_hierarchy_solve_cg_block", "mfmg_hip_block_cg_retire", "mfmg_hip_block_dots", "mfmg_hip_block_cg_direction",
                 "mfmg_hip_block_cg_update", "mfmg_hip_hierarchy_operator_apply_block"):
        assert name in declared, name
