"""The checks of tests/test_gpu_halo_exchange.py (halo_reference.check_*) must bite: on the CPU, the restatement's own result
stands in for a correct exchange and passes; with one error planted at a time the check reports it.  Two runs, both with three
components per node: a 2 x 2 x 2 grid of boxes (faces, edges, a corner; four ghost layers below, three above) and a 1 x 1 x 3
run of slabs (a middle rank with both neighbours).  The planted errors:
  forward   a ghost region filled from the owner's layers shifted by one; two components swapped inside one message; a write one
            layer deeper than the exchange is wide (with the owner's value, so only its place is wrong)
  reverse   the contribution of an edge neighbour (slabs: of the upper neighbour) added twice; that of the corner neighbour
            (slabs: of the lower neighbour) left out; one ghost entry changed -- each against the exact and the rounded check
  dot       a NaN ghost entry let into the sum; one rank with a sum one ulp off
The rounded check also passes what float64 additions in rank order give (a second correct exchange).
On counts: the doubles the restatement sends are BoxPartition.exchange_doubles(width) * comps on every rank, both directions."""
import numpy as np
import pytest

import halo_reference as H
import mfmg_amd as M

COMPS = 3
RUNS = {"boxes": ((2, 2, 2), (8, 8, 8)), "slabs": (((1, 1, 3)), (4, 6, 12))}
# (run: the rank whose result is spoilt, the split axis looked at, the neighbour whose contribution is doubled / left out)
SPOILT = {"boxes": (0, 0, 3, 7), "slabs": (1, 2, 2, 0)}


def _spaces(run, width=1):
    grid, cells = RUNS[run]
    out = []
    for r in range(grid[0] * grid[1] * grid[2]):
        p = M.BoxPartition(cells, r, grid, low_ghost_cells=4)
        box = {"comps": COMPS, "dims": p.local_nodes, "own0": p.own0, "own_n": p.own_n, "g0": p.offset, "gn": p.global_nodes}
        out.append(H.make_space(box, width, [p.coord[d] > 0 for d in range(3)], [p.coord[d] + 1 < grid[d] for d in range(3)]))
    return out


def _stride(sp, d):
    return sp.comps * (1 if d == 0 else sp.dims[0] if d == 1 else sp.dims[0] * sp.dims[1])


def _ghost_face_below(sp, d, depth):
    """the entries of the ghost layer `depth` below the owned box along axis d, over the owned range of the other axes: what one
    face message fills (depth 1)"""
    co = H.local_coords(sp)
    m = co[d] == sp.own0[d] - depth
    for e in range(3):
        if e != d:
            m &= (co[e] >= sp.own0[e]) & (co[e] < sp.own0[e] + sp.own_n[e])
    return m


def _contribution(spaces, vectors, a, b):
    """(local entries of rank a, values): what rank b's shell holds for entries that rank a owns"""
    owner = H.owner_map(spaces)
    gb = H.global_ids(spaces[b])
    pick = H.shell_mask(spaces[b]) & (owner[gb] == a)
    assert pick.any()
    where = np.full(H.n_global(spaces[a]), -1, dtype=np.int64)
    where[H.global_ids(spaces[a])] = np.arange(H.n_local(spaces[a]))
    return where[gb[pick]], vectors[b][pick]


@pytest.mark.parametrize("run", list(RUNS))
def test_forward_check_reports_every_planted_fault(run):
    spaces = _spaces(run)
    before = [H.forward_input(sp) for sp in spaces]
    good = H.forward(spaces, before)
    assert H.check_forward(spaces, before, good) == []
    for sp, b, g in zip(spaces, before, good):          # the exchange did something, and only inside the dilated box
        sh = H.shell_mask(sp)
        assert sh.any() and np.isfinite(g[sh]).all() and np.isnan(g[~sh & ~H.owned_mask(sp)]).all()
    last = len(spaces) - 1                                # (a lower neighbour along every split axis)
    sp, d = spaces[last], SPOILT[run][1]
    held = H.owner_values(spaces, before)
    gid, face = H.global_ids(sp), _ghost_face_below(sp, d, 1)
    # the region one layer off: the ghost layer holds what lies one layer further from the owned box
    bad = [g.copy() for g in good]
    bad[last][face] = held[gid[np.flatnonzero(face) - _stride(sp, d)]]
    found = H.check_forward(spaces, before, bad)
    assert len(found) == 1 and "do not hold the owner's value" in found[0] and f"rank {last}" in found[0], found
    # two components swapped inside one message
    bad = [g.copy() for g in good]
    co = H.local_coords(sp)
    c0, c1 = np.flatnonzero(face & (co[3] == 0)), np.flatnonzero(face & (co[3] == 1))
    bad[last][c0], bad[last][c1] = good[last][c1], good[last][c0]
    found = H.check_forward(spaces, before, bad)
    assert len(found) == 1 and "do not hold the owner's value" in found[0], found
    # one layer deeper than the exchange is wide: the right value in a place the exchange must not write
    deeper = _ghost_face_below(sp, d, 2)
    bad = [g.copy() for g in good]
    bad[last][deeper] = held[gid[deeper]]
    found = H.check_forward(spaces, before, bad)
    assert len(found) == 1 and "outside the dilated box" in found[0], found
    assert H.check_forward(spaces, before, bad, width=2) != []   # (and no exchange of width 2 either: its edges are missing)
    # an owned entry overwritten
    bad = [g.copy() for g in good]
    bad[0][np.flatnonzero(H.owned_mask(spaces[0]))[-1]] += 1.0
    found = H.check_forward(spaces, before, bad)
    assert len(found) == 1 and "owned entries changed" in found[0], found


def _added_in_rank_order(spaces, before):
    """a reverse exchange in float64: the contributions added to the owner's entry rank after rank"""
    after = [v.copy() for v in before]
    for a in range(len(spaces)):
        for b in range(len(spaces)):
            if a != b and (H.owner_map(spaces)[H.global_ids(spaces[b])[H.shell_mask(spaces[b])]] == a).any():
                at, val = _contribution(spaces, before, a, b)
                np.add.at(after[a], at, val)
    return after


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("run", list(RUNS))
def test_reverse_check_reports_every_planted_fault(run, exact):
    spaces = _spaces(run)
    before = [H.integer_input(sp, r) if exact else H.decade_input(sp, r, 5) for r, sp in enumerate(spaces)]
    ref = H.reverse(spaces, before)
    good = [e.ref.astype(np.float64) for e in ref]
    assert H.check_reverse(spaces, before, good, exact=exact) == []
    ordered = _added_in_rank_order(spaces, before)
    assert H.check_reverse(spaces, before, ordered, exact=exact) == []
    if exact:
        assert all(np.array_equal(o, g) for o, g in zip(ordered, good))
    a, _, twice, omitted = SPOILT[run]
    # the most contributions an entry receives: 7 at the corner node of a box (3 faces, 3 edges, 1 corner), 1 in a plane of a slab
    assert max(int(e.m.max()) for e in ref) == (7 if run == "boxes" else 1)
    for b, sign, what in ((twice, 1.0, "added twice"), (omitted, -1.0, "left out")):
        bad = [g.copy() for g in good]
        at, val = _contribution(spaces, before, a, b)
        bad[a][at] += sign * val
        found = H.check_reverse(spaces, before, bad, exact=exact)
        assert len(found) == 1 and "differ from the sum" in found[0] and f"rank {a}:" in found[0], (what, found)
        n_found = int(found[0].split(":")[2].split(" entries")[0])
        assert n_found == len(at), (what, found)         # every entry of that contribution, no other
    # one ghost entry changed (say, zeroed after it was sent)
    bad = [g.copy() for g in good]
    ghost = np.flatnonzero(~H.owned_mask(spaces[a]))
    bad[a][ghost[len(ghost) // 2]] = 0.0
    found = H.check_reverse(spaces, before, bad, exact=exact)
    assert len(found) == 1 and "changed ghost entries" in found[0], found
    # a contribution that went to the right entries in the wrong order (a permutation inside the region)
    bad = [g.copy() for g in good]
    at, val = _contribution(spaces, before, a, twice)
    bad[a][at] += val[::-1] - val
    assert H.check_reverse(spaces, before, bad, exact=exact) != []


@pytest.mark.parametrize("run", list(RUNS))
def test_dot_check_reports_a_ghost_in_the_sum(run):
    spaces = _spaces(run)
    xs = [H.decade_input(sp, r, 7, ghosts=False) for r, sp in enumerate(spaces)]
    ys = [H.decade_input(sp, r, 8, ghosts=False) for r, sp in enumerate(spaces)]
    ref, mag, most = H.owned_dot(spaces, xs, ys)
    assert np.isfinite(ref) and mag > 0
    n = len(spaces)
    # float64 sums per rank, then over the ranks: a correct reduction
    good = float(np.sum([np.dot(x[H.owned_mask(sp)], y[H.owned_mask(sp)]) for sp, x, y in zip(spaces, xs, ys)]))
    assert H.check_dot(spaces, xs, ys, [good] * n) == []
    # one ghost entry (a NaN) in the sum of one rank: every rank gets the NaN from the all-reduce
    own = H.owned_mask(spaces[0]).copy()
    own[np.flatnonzero(~own)[0]] = True
    leaked = float(np.dot(xs[0][own], ys[0][own])) + good
    found = H.check_dot(spaces, xs, ys, [leaked] * n)
    assert len(found) == n and all("ghost entry" in f for f in found), found
    # a finite ghost entry counted: beyond the bound
    xf, yf = [x.copy() for x in xs], [y.copy() for y in ys]
    g0 = np.flatnonzero(~H.owned_mask(spaces[0]))[0]
    xf[0][g0] = yf[0][g0] = 1.0
    assert H.check_dot(spaces, xf, yf, [good] * n) == []                    # (the reference does not read it)
    found = H.check_dot(spaces, xf, yf, [good + 1.0] * n)
    assert len(found) == n and all("from the long-double sum" in f for f in found), found
    # one rank one ulp off
    found = H.check_dot(spaces, xs, ys, [good] * (n - 1) + [float(np.nextafter(good, np.inf))])
    assert any("different sums" in f for f in found), found


def test_chain_of_the_dot_bound():
    """dot_chain for the sizes of the GPU test: one trip and up to 1024 blocks below 262145 owned entries"""
    assert H.dot_chain(1, 2) == 1 + 1 + 9 + 1 + 9 + 1
    assert H.dot_chain(65536, 8) == 1 + 1 + 9 + 1 + 9 + 7
    assert H.dot_chain(65537, 8) == 1 + 1 + 9 + 2 + 9 + 7
    assert H.dot_chain(262144, 3) == 1 + 1 + 9 + 4 + 9 + 2
    assert H.dot_chain(262145, 3) == 1 + 2 + 9 + 4 + 9 + 2


@pytest.mark.parametrize("run", list(RUNS))
def test_sent_doubles_are_those_of_the_partition(run):
    grid, cells = RUNS[run]
    for width in (1, 2, 3):
        spaces = _spaces(run, width)
        assert all(H.precondition(sp) == [] for sp in spaces)
        want = [M.BoxPartition(cells, r, grid, low_ghost_cells=4).exchange_doubles(width) * COMPS for r in range(len(spaces))]
        assert H.sent_doubles(spaces) == want and H.sent_doubles(spaces, reverse=True) == want and min(want) > 0
    thin = spaces[0]._replace(width=max(spaces[0].own_n) + 1)
    assert any("owned layers" in f for f in H.precondition(thin)) and any("ghost layers above" in f for f in H.precondition(thin))
