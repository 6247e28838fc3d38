"""The z-tiling of the matrix-free operator (mf_z_tiles of mf_z_tiles.hpp through mfmg_hip_mf_z_tiles; host only, no GPU, no
context) against a restatement of its rule in Python, for every n_layers in 1 .. 2100 and tz in 1 .. 64, graded or not.

The table is what the one-term kernel and the block kernel read through `ztab`: z-tile t owns the DoF layers [tab[t], tab[t + 1]).
That the tiles PARTITION the layers can only be seen here.  A layer no tile owns would show on the GPU (the output keeps its
NaN), but a layer two tiles own changes no output bit: the owner computes, both tiles compute the same value from the same
inputs and write it twice -- a wasted layer per overlap and a write race with equal values, invisible to every comparison of
results.  So the partition check is first shown to reject planted tables (a skipped layer, a repeated start, an overlap, a last
entry of n_layers - 1), then held over the whole range.

The rule (restated below, not imported): q = n // 8, m = (q + tz // 2) // tz + 1 z-tiles per eighth, graded iff q >= 2 m; the
eighth s owns [s n // 8, (s + 1) n // 8), cut where the cumulative weights m - k + 0.5 fall, every cut rounded half away from
zero and clamped so that every tile keeps at least one layer.  Arguments without a table: n_layers < 1 and tz < 1 are refused;
m < 1 (only the experiment knob MFMG_MF_GRADE_M at 0 or below gives one; the C ABI takes the default knobs, so the stand-alone
program mf_z_tiles_check.cpp is built and asked for those tables) falls back to the uniform table -- it was a table of zero
tiles, a launch that ran nothing and left `out` as it was."""
import ctypes as C
import functools
import math
import os
import shutil
import subprocess

import pytest

from mfmg_amd import lib as L
from mfmg_amd.api import mf_z_tiles

N_MAX, TZ_MAX = 2100, 64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")


# ---- the rule, restated ----
def _round_half_away(v):
    assert v >= 0.0
    r = math.floor(v)
    return r + 1 if v - r >= 0.5 else r


def _m(n, tz, m_extra=1):
    return (n // 8 + tz // 2) // tz + m_extra


def _grades(n, tz, m_extra=1):
    m = _m(n, tz, m_extra)
    return m >= 1 and n // 8 >= 2 * m


def _uniform(n, tz):
    return list(range(0, n, tz)) + [n]


@functools.lru_cache(maxsize=None)
def _eighth(length, m, w_off):
    """Starts of the m tiles of an eighth of `length` layers, from its first layer (an eighth is cut the same wherever it lies)."""
    total = sum(m - k + w_off for k in range(m))
    starts, cum, prev = [], 0.0, 0
    for k in range(m):
        starts.append(prev)
        cum += m - k + w_off
        nxt = length if k + 1 == m else _round_half_away(length * cum / total)
        prev = min(max(nxt, prev + 1), length - (m - 1 - k))
    return tuple(starts)


def _rule(n, tz, graded, m_extra=1, w_off=0.5):
    if not (graded and _grades(n, tz, m_extra)):
        return _uniform(n, tz)
    m = _m(n, tz, m_extra)
    tab = []
    for s in range(8):
        l0, l1 = s * n // 8, (s + 1) * n // 8
        tab += [l0 + o for o in _eighth(l1 - l0, m, w_off)]
    return tab + [n]


def _heights(tab):
    return [b - a for a, b in zip(tab, tab[1:])]


def _partition_defect(tab, n):
    """None if the tiles [tab[t], tab[t + 1]) own every layer of [0, n) exactly once and none is empty, else what is wrong."""
    if len(tab) < 2:
        return "no tile"
    if tab[0] != 0:
        return f"the first tile starts at {tab[0]}"
    if tab[-1] != n:
        return f"the last tile ends at {tab[-1]}, not at {n}"
    for t, (a, b) in enumerate(zip(tab, tab[1:])):
        if b <= a:
            return f"tile {t} is empty or runs backwards: [{a}, {b})"
    owners = [0] * n                      # (the same statement once more, layer by layer, from the tiles as the kernel reads them)
    for a, b in zip(tab, tab[1:]):
        for l in range(a, b):
            owners[l] += 1
    if owners != [1] * n:
        return f"layers not owned exactly once: {[l for l in range(n) if owners[l] != 1][:5]}"
    return None


# ---- the check bites ----
def test_the_partition_check_rejects_planted_tables():
    good = [0, 3, 4, 7, 8, 11, 12, 15, 16, 19, 20, 23, 24, 27, 28, 31, 33]
    assert good == _rule(33, 4, True) and _partition_defect(good, 33) is None
    planted = {
        "a skipped layer": [1] + good[1:],                         # layer 0 belongs to nobody
        "a repeated start": good[:5] + [good[4]] + good[5:],       # an empty tile
        "an overlap": good[:3] + [3] + good[3:],                   # ... 3, 4, 3, 4, 7: the layers [3, 4) twice, a tile backwards
        "a last entry of n_layers - 1": good[:-1] + [32],          # the last layer belongs to nobody
        "a last entry of n_layers + 1": good[:-1] + [34],          # a layer that does not exist
        "no tile": [33],                                           # the table of m = 0
        "descending": list(reversed(good)),
    }
    for what, tab in planted.items():
        assert _partition_defect(tab, 33) is not None, what
    # an overlap as the kernel would run it from (start, height) pairs: tiles [0, 4) and [3, 7) -- the layer count sees it
    assert _partition_defect([0, 4, 3, 7], 7) is not None
    # and the restated rule is not the uniform rule: the comparison below can fail
    assert _rule(257, 8, True) != _uniform(257, 8) and _rule(257, 8, False) == _uniform(257, 8)


# ---- the whole range ----
@pytest.fixture(scope="module")
def tables(mfmg_lib):
    """Every table of the range, read once through the raw entry point (one buffer for all calls)."""
    cap = N_MAX + 1
    buf, cnt = (C.c_int32 * cap)(), C.c_int32()
    fn = mfmg_lib.mfmg_hip_mf_z_tiles
    out = {}
    for graded in (0, 1):
        for n in range(1, N_MAX + 1):
            for tz in range(1, TZ_MAX + 1):
                assert fn(n, tz, graded, buf, cap, C.byref(cnt)) == L.SUCCESS, (n, tz, graded)
                out[n, tz, graded] = buf[:cnt.value + 1]
    return out


def test_every_table_is_a_partition(tables):
    for (n, tz, graded), tab in tables.items():
        assert tab[0] == 0 and tab[-1] == n and all(b > a for a, b in zip(tab, tab[1:])), (n, tz, graded, tab)
    # layer by layer on a part of the range (the cheap form above says the same)
    for n in list(range(1, 300)) + [511, 512, 513, 1025, 2047, 2100]:
        for tz in (1, 2, 3, 4, 5, 7, 8, 16, 33, 64):
            for graded in (0, 1):
                assert _partition_defect(tables[n, tz, graded], n) is None, (n, tz, graded)


def test_every_table_is_the_restated_rule(tables):
    n_graded, tallest = 0, 0.0
    for (n, tz, graded), tab in tables.items():
        assert tab == _rule(n, tz, bool(graded)), (n, tz, graded)
        if not graded:
            assert tab == _uniform(n, tz) and len(tab) - 1 == -(-n // tz), (n, tz)
            continue
        m = _m(n, tz)
        if _grades(n, tz):
            n_graded += 1
            assert len(tab) - 1 == 8 * m, (n, tz)
            assert tz >= 3, (n, tz)                                                 # tz = 1 and 2 never grade
            # no tile taller than 2 tz (the march of a tile runs its height + 1 layer passes)
            assert max(_heights(tab)) <= 2 * tz, (n, tz, max(_heights(tab)))
            tallest = max(tallest, max(_heights(tab)) / tz)
        else:
            assert tab == _uniform(n, tz) and len(tab) - 1 == -(-n // tz), (n, tz)
    assert n_graded > 50000 and tallest == 2.0          # (2 tz is reached on this range: the bound is the maximum, not a guess)
    # the smallest meshes that grade (16 layers: one tile of two layers per eighth, for tz >= 5; two tiles per eighth need 32
    # layers), and the first tile taller than tz, per tile height
    first_graded = lambda tz, m_min: next(n for n in range(1, N_MAX + 1) if _grades(n, tz) and _m(n, tz) >= m_min)
    first_taller = lambda tz: next(n for n in range(1, N_MAX + 1) if _grades(n, tz) and max(_heights(tables[n, tz, 1])) > tz)
    assert min(first_graded(tz, 1) for tz in range(3, TZ_MAX + 1)) == 16 == first_graded(5, 1) and first_graded(4, 1) == 32
    assert min(first_graded(tz, 2) for tz in range(3, TZ_MAX + 1)) == 32 == first_graded(3, 2) == first_graded(4, 2) == first_graded(8, 2)
    assert (first_taller(3), first_taller(4), first_taller(8)) == (57, 73, 145)


def test_the_tables_the_comments_and_the_gpu_tests_rely_on(mfmg_lib):
    eighths = lambda tab, m: [_heights(tab)[s * m:(s + 1) * m] for s in range(8)]
    # the workload: 257 layers, tz = 8
    assert eighths(mf_z_tiles(257, 8), 5) == [[10, 8, 7, 4, 3]] * 7 + [[10, 9, 6, 5, 3]]
    assert eighths(mf_z_tiles(33, 4), 2) == [[3, 1]] * 7 + [[3, 2]]
    t = mf_z_tiles(57, 3)
    assert len(t) - 1 == 24 and set(_heights(t)) == {1, 2, 3, 4}
    assert eighths(mf_z_tiles(97, 4), 4) == [[5, 3, 3, 1]] * 7 + [[5, 4, 2, 2]]
    assert eighths(mf_z_tiles(159, 8), 3) == [[9, 6, 4]] + [[9, 7, 4]] * 7
    # 32 layers, tz = 4 (the tail slab case of the GPU module): 3, 1 throughout; 33 layers at tz = 8: the table of tz = 4;
    # 23 layers at tz = 8 (the tallest mesh of the older long-double modules): graded, but one tile per eighth
    assert eighths(mf_z_tiles(32, 4), 2) == [[3, 1]] * 8
    assert _m(33, 8) == 2 and mf_z_tiles(33, 8) == mf_z_tiles(33, 4)
    assert _m(23, 8) == 1 and _grades(23, 8) and _heights(mf_z_tiles(23, 8)) == [2, 3, 3, 3, 3, 3, 3, 3]
    # a region launch reads the uniform table; a mesh too short to grade reads it either way
    assert mf_z_tiles(257, 8, graded=False) == list(range(0, 257, 8)) + [257]
    assert mf_z_tiles(23, 4) == mf_z_tiles(23, 4, graded=False) == [0, 4, 8, 12, 16, 20, 23]
    assert mf_z_tiles(1, 1) == [0, 1] and mf_z_tiles(1, 64) == [0, 1]


# ---- refusals ----
def test_refusals(mfmg_lib):
    fn = mfmg_lib.mfmg_hip_mf_z_tiles
    buf, cnt = (C.c_int32 * 64)(), C.c_int32(-7)
    for i in range(64):
        buf[i] = -7
    untouched = lambda: list(buf) == [-7] * 64 and cnt.value == -7
    assert fn(33, 4, 1, None, 64, C.byref(cnt)) == L.ERROR_INVALID_ARGUMENT and untouched()
    assert fn(33, 4, 1, buf, 64, None) == L.ERROR_INVALID_ARGUMENT and untouched()
    for n, tz in ((0, 4), (-1, 4), (33, 0), (33, -4)):
        for graded in (0, 1):
            assert fn(n, tz, graded, buf, 64, C.byref(cnt)) == L.ERROR_INVALID_ARGUMENT and untouched(), (n, tz, graded)
    # 33 layers, tz = 4: 16 tiles graded (17 entries), 9 uniform (10 entries)
    for graded, entries in ((1, 17), (0, 10)):
        for capacity in (entries - 1, 1, 0, -5):
            assert fn(33, 4, graded, buf, capacity, C.byref(cnt)) == L.ERROR_INVALID_ARGUMENT and untouched(), (graded, capacity)
        assert fn(33, 4, graded, buf, entries, C.byref(cnt)) == L.SUCCESS and cnt.value == entries - 1
        assert list(buf[:entries]) == _rule(33, 4, bool(graded)) and list(buf[entries:]) == [-7] * (64 - entries)
        cnt.value = -7
        for i in range(64):
            buf[i] = -7
    for bad in ((0, 4), (33, 0)):
        with pytest.raises(L.MfmgInvalidArgument, match="at least"):
            mf_z_tiles(*bad)


# ---- m < 1: the pure function, through the stand-alone program ----
def test_a_knob_that_leaves_no_tile_per_eighth_gives_the_uniform_table(tmp_path):
    """m_extra = 0 and -1 (MFMG_MF_GRADE_M): wherever m < 1 the table is the uniform one, never a table of zero tiles; wherever
    m >= 1 it is the rule with that m, as before.  The program is built without sanitizers here (with them: make check-z-tiles)."""
    make = shutil.which("make")
    assert make, "make is needed (the library itself is built with it)"
    exe = str(tmp_path / "mf_z_tiles_check")
    res = subprocess.run([make, "-C", CSRC, exe, f"Z_TILES_CHECK={exe}", "Z_TILES_CHECK_FLAGS="], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]

    def table(n, tz, graded, m_extra, w_off=0.5):
        r = subprocess.run([exe, str(n), str(tz), str(int(graded)), str(m_extra), repr(w_off)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(v) for v in r.stdout.split()]

    assert _m(17, 8, 0) == 0 and table(17, 8, True, 0) == [0, 8, 16, 17]         # (was [17]: zero tiles)
    seen = set()
    for m_extra in (0, -1):
        for n, tz in ((17, 8), (1, 1), (7, 64), (31, 8), (33, 64), (100, 64), (257, 8), (97, 4), (2100, 8), (16, 1), (300, 5)):
            m = _m(n, tz, m_extra)
            tab = table(n, tz, True, m_extra)
            assert _partition_defect(tab, n) is None, (n, tz, m_extra, tab)
            assert tab == _rule(n, tz, True, m_extra), (n, tz, m_extra)
            if m < 1:
                assert tab == _uniform(n, tz), (n, tz, m_extra)
            elif _grades(n, tz, m_extra):
                assert len(tab) - 1 == 8 * m, (n, tz, m_extra)
            seen.add((m < 1, _grades(n, tz, m_extra)))
            assert table(n, tz, False, m_extra) == _uniform(n, tz)
    assert seen == {(True, False), (False, False), (False, True)}                   # every branch was taken
    # the default knobs through the program are the library's tables
    assert table(257, 8, True, 1) == mf_z_tiles(257, 8) and table(33, 4, True, 1) == mf_z_tiles(33, 4)
