"""The kernels and the host logic that move data between ranks, entry by entry: regions_copy_kernel (pack, unpack, the adding mode),
regions_copy_f32_kernel, box_copy_kernel, add_layers_kernel (vector_ops.hip), exchange_box / exchange_on / exchange_reverse_add
(common.hpp) and distributed_dot behind HaloTransport.owned_dot -- against tests/halo_reference.py, which restates the three
operations from the description of a space alone (global ids; no regions, no messages).

Ranks are threads of one process behind the host transport with in-memory mailboxes (tests/test_box_threads.py).  Every rank
builds its context, transport and a small hierarchy -- only so that the spaces are configured the way real runs configure them --
and runs the same sequence of exchanges on every configured space; the main thread compares afterwards.  Per configuration
(CASES: slabs with one and two neighbours, boxes split along x, along y, along two and three axes; one to three components on the
coarse space; exchange widths 1, 2 and 3: the fine space one plane deep, the two-deep fine space of the one-pass residual
restriction, aggregation levels of stencil reach 2 and 3) and space:
  1  along every axis with a neighbour the owned box is `width` thick and `width` ghost layers lie there
  2  forward, exact: owned entries node * 4 + component + 0.25 of the global node, NaN elsewhere; afterwards every entry inside
     the dilated owned box holds its owner's value, every other entry its old bits
  3  reverse, exact: integers below 2^20 on every local entry; owned entries equal the restatement bit for bit, ghost entries keep
     their bits
  4  reverse, rounded: normal doubles over six decades; per owned entry |got - ref| <= m 2^-53 sum |addends|, m the additions into
     that entry (from the restatement, up to 7 at the corner of a box), ref in long double
  5  float forward (space 1): widths 1 .. min(3, low_ghost), the expectations of 2; a wider exchange and another space are refused
  6  n_exchanges grows by one per exchange, exchange_volume by the doubles the restatement sends, in both directions
  7  owned dot: x, y over six decades on owned entries, NaN on every ghost entry; the same bits on every rank and on a second
     call, within k 2^-53 sum |x_i y_i| of the long-double sum
  8  a forward and a reverse exchange back to back on one vector (the staging buffer reused in stream order) give the bits of the
     two with a synchronisation in between, and those of the restatement applied twice

k of 7 (halo_reference.dot_chain) is the longest chain of roundings a term x_i y_i passes through.  A rank reduces its n owned
entries (slabs: the owned planes as they lie; boxes: packed by box_copy_kernel) with dot_stage1_kernel on min(ceil(n / 256), 1024)
blocks of 256 threads: the product is rounded (1), a thread adds the entries of its grid-stride run, ceil(n / (256 blocks)) trips
(1 below 262 145 entries), the wavefront's butterfly adds 6 times, thread 0 adds the sums of the 4 wavefronts (3).
dot_stage2_kernel, one block: a thread adds ceil(blocks / 256) partials (1 up to 65 536 entries, at most 4), then 6 + 3 again.
The all-reduce adds the sums of the R ranks (R - 1).  Here n <= 65 536 on every rank: k = 1 + 1 + 9 + 1 + 9 + (R - 1) = 21 + R - 1
-- 22 on two ranks, 23 on three, 24 on four, 28 on eight (asserted below; the test prints every error)."""
import threading

import numpy as np
import pytest
import torch

import halo_reference as H
import mfmg_amd as M
from test_box_threads import Mailboxes

_REPLICATE = {"coarsest_size": 40, "replicate_rows": 40}
# id: grid, owned cells per rank (x, y, z), material, eigenvectors, coarse solver, low_ghost, what the spaces must show
# Sizes: the smallest the distributed tests set up (tests/dist_worker.py: "small", "deep", "cube11"); the boxes without distributed
# aggregation levels take 8 cells per rank along a split axis, which the setup accepts, and unsplit extents (12 and 6, 14 and 6)
# that leave the three local extents and the three owned extents of every rank different.  No space of these hierarchies has an
# owned range of one layer along a split axis (the thinnest: three layers at width 3 on the last level of the "deep" cases).
CASES = {
    "slabs_2": ((1, 1, 2), (16, 12, 8), "linear", 2, {"coarsest_size": 300}, 2, {"comps": {1, 2}, "widths": {1}}),
    "slabs_3_comps_3": ((1, 1, 3), (16, 12, 8), "linear", 3, {"coarsest_size": 300}, 2, {"comps": {1, 3}, "widths": {1}}),
    "slabs_2_deep": ((1, 1, 2), (16, 16, 24), "constant", 2, _REPLICATE, 4, {"comps": {1, 2}, "widths": {1, 2}, "levels": 2}),
    "boxes_x": ((2, 1, 1), (8, 12, 6), "linear", 2, {"coarsest_size": 300}, 2, {"comps": {1, 2}, "widths": {1}}),
    "boxes_y": ((1, 2, 1), (14, 8, 6), "linear", 2, {"coarsest_size": 300}, 4, {"comps": {1, 2}, "widths": {1}}),
    "boxes_xy_deep": ((2, 2, 1), (24, 24, 24), "constant", 2, {"replicate_rows": 40}, 2, {"comps": {1, 2}, "widths": {1, 2}, "levels": 2}),
    "boxes_xyz_comps_1": ((2, 2, 2), (8, 8, 8), "constant", 1, {"coarsest_size": 300}, 4, {"comps": {1}, "widths": {1}}),
}
# per case: (axes the ranks split, (faces, edges, corners) of the neighbours of the rank with most of them)
REACHES = {"slabs_2": ((2,), (1, 0, 0)), "slabs_3_comps_3": ((2,), (2, 0, 0)), "slabs_2_deep": ((2,), (1, 0, 0)),
           "boxes_x": ((0,), (1, 0, 0)), "boxes_y": ((1,), (1, 0, 0)), "boxes_xy_deep": ((0, 1), (2, 1, 0)),
           "boxes_xyz_comps_1": ((0, 1, 2), (3, 3, 1))}


def _parts(case):
    grid, per, _, _, _, low_ghost, _ = CASES[case]
    cells = tuple(per[d] * grid[d] for d in range(3))
    length = tuple(c / float(cells[0]) for c in cells)           # cubic cells
    return [M.BoxPartition(cells, r, grid, length=length, low_ghost_cells=low_ghost) for r in range(grid[0] * grid[1] * grid[2])]


def _neighbours(part):
    """(faces, edges, corners): the neighbours of a rank by the number of axes they are offset along"""
    n = [0, 0, 0]
    for o in np.ndindex(3, 3, 3):
        o = tuple(v - 1 for v in o)
        if any(o) and all(0 <= part.coord[d] + o[d] < part.grid[d] for d in range(3)):
            n[sum(1 for v in o if v) - 1] += 1
    return tuple(n)


def test_cases_reach_the_edges_they_name():
    assert set(REACHES) == set(CASES)
    for case, (grid, per, _, n_eig, amg, low_ghost, show) in CASES.items():
        parts = _parts(case)
        split, most = REACHES[case]
        assert tuple(d for d in range(3) if grid[d] > 1) == split
        assert max(_neighbours(p) for p in parts) == most and all(sum(_neighbours(p)) > 0 for p in parts), case
        assert all(p.split_xy == (split != (2,)) for p in parts)            # slabs travel as contiguous planes, boxes packed
        for p in parts:
            for d in range(3):
                below, above = p.own0[d], p.local_nodes[d] - p.own0[d] - p.own_n[d]
                # the ghost node planes: low_ghost below (the interface plane belongs to the upper box), three above
                assert below == (low_ghost if p.coord[d] > 0 else 0) and above == (3 if p.coord[d] + 1 < grid[d] else 0)
                assert p.own_n[d] == per[d] + (p.coord[d] + 1 == grid[d])
    # a middle rank with both neighbours; extents that differ per axis where one axis is split, so that a mix-up of axes shows
    mid = _parts("slabs_3_comps_3")[1]
    assert mid.ghost_lo[2] > 0 and mid.ghost_hi[2] > 0
    for case in ("boxes_x", "boxes_y"):
        assert all(len(set(p.local_nodes)) == 3 and len(set(p.own_n)) == 3 for p in _parts(case))
    # one, two and three components on the coarse space; both ghost depths; gathered and distributed coarse levels
    assert {c[3] for c in CASES.values()} == {1, 2, 3} and {c[5] for c in CASES.values()} == {2, 4}
    assert sum("replicate_rows" in c[4] for c in CASES.values()) == 2
    # every owned dot product of the cases is one grid-stride trip and one partial per thread of the second stage: k = 21 + R - 1
    for case in CASES:
        parts = _parts(case)
        n = max(int(np.prod(p.own_n)) for p in parts)
        assert n <= 65536 and H.dot_chain(n, len(parts)) == 21 + len(parts) - 1


def _exchange(ctx, tr, space, arr, mode):
    """one exchange of a copy of `arr` on the device: (result, exchanges counted, doubles counted)"""
    v = torch.from_numpy(arr).cuda()
    torch.cuda.synchronize()
    e0, v0 = tr.n_exchanges(), tr.exchange_volume()
    if mode == "forward":
        tr.exchange(space, v)
    elif mode == "reverse":
        tr.exchange(space, v, reverse=True)
    elif mode in ("chain", "chain_sync"):
        tr.exchange(space, v)
        if mode == "chain_sync":
            ctx.synchronize()
        tr.exchange(space, v, reverse=True)
    else:
        tr.exchange_f32(space, v, mode)
    ctx.synchronize()
    return v.cpu().numpy(), tr.n_exchanges() - e0, tr.exchange_volume() - v0


def _rank_run(ctx, tr, part, rank, low_ghost):
    """what one rank does: per configured space its description and (input, result, counters) of every check"""
    out = {}
    low = [part.coord[d] > 0 for d in range(3)]
    high = [part.coord[d] + 1 < part.grid[d] for d in range(3)]
    n_spaces = tr.space(1)["n_spaces"]
    for s in range(1, n_spaces):
        box = tr.box(s)
        if box["dims"][0] * box["dims"][1] * box["dims"][2] == 0:
            assert s > 2, "the fine space and the first coarse space are configured"
            continue
        sp = H.make_space(box, tr.space(s)["width"], low, high)
        assert tr.space(s)["layer_elems"] * tr.space(s)["n_layers"] == H.n_local(sp)
        assert H.precondition(sp) == [], (s, sp, H.precondition(sp))
        rec = {"space": sp}
        for what, arr, mode in (("forward", H.forward_input(sp), "forward"), ("reverse_exact", H.integer_input(sp, rank), "reverse"),
                                ("reverse_rounded", H.decade_input(sp, rank, 3), "reverse"), ("chain", H.integer_input(sp, rank), "chain"),
                                ("chain_sync", H.integer_input(sp, rank), "chain_sync")):
            rec[what] = (arr,) + _exchange(ctx, tr, s, arr, mode)
        x, y = H.decade_input(sp, rank, 7, ghosts=False), H.decade_input(sp, rank, 8, ghosts=False)
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        torch.cuda.synchronize()
        rec["dot"] = (x, y, tr.owned_dot(xd, yd, s), tr.owned_dot(xd, yd, s))
        if s == 1:
            widths = list(range(1, min(3, low_ghost) + 1))
            for w in widths:
                arr = H.forward_input(sp, np.float32)
                rec[("f32", w)] = (arr,) + _exchange(ctx, tr, s, arr, w)
            rec["f32_widths"] = widths
            v32 = torch.zeros(H.n_local(sp), dtype=torch.float32, device="cuda")
            for bad_space, bad_width in ((1, widths[-1] + 1), (1, 0)):
                with pytest.raises(M.lib.MfmgInvalidArgument):
                    tr.exchange_f32(bad_space, v32, bad_width)
        else:
            v32 = torch.zeros(H.n_local(sp), dtype=torch.float32, device="cuda")
            with pytest.raises(M.lib.MfmgInvalidArgument):
                tr.exchange_f32(s, v32, 1)
        out[s] = rec
    return out


def _compare(case, records):
    """the main thread: every check of every space against the restatement; returns the findings"""
    n_ranks, found = len(records), []
    assert all(set(r) == set(records[0]) for r in records), "the ranks configured different spaces"
    seen = {"comps": set(), "widths": set(), "thin": []}
    for s in sorted(records[0]):
        spaces = [r[s]["space"] for r in records]
        sp0 = spaces[0]
        assert all(sp.width == sp0.width and sp.comps == sp0.comps and sp.gn == sp0.gn for sp in spaces)
        seen["comps"].add(sp0.comps); seen["widths"].add(sp0.width)
        if any(sp.own_n[d] == 1 and (sp.low[d] or sp.high[d]) for sp in spaces for d in range(3)):
            seen["thin"].append(s)
        has_neighbour = [any(sp.low) or any(sp.high) for sp in spaces]
        k = H.dot_chain(max(int(H.owned_mask(sp).sum()) for sp in spaces), n_ranks)
        print(f"{case} space {s}: comps {sp0.comps} width {sp0.width} global nodes {sp0.gn}; per rank dims / own0 / own_n / low / high: "
              + "; ".join(f"{sp.dims} {sp.own0} {sp.own_n} {''.join('xyz'[d] for d in range(3) if sp.low[d]) or '-'} "
                          f"{''.join('xyz'[d] for d in range(3) if sp.high[d]) or '-'}" for sp in spaces) + f"; dot bound k = {k}")
        tag = lambda what, fs: [f"space {s} {what}: {f}" for f in fs]

        def counters(what, sent_once, times=1):
            for r, rec in enumerate(records):
                _, _, n_ex, n_vol = rec[s][what]
                if n_ex != times * has_neighbour[r] or n_vol != sent_once[r]:
                    found.append(f"space {s} {what}: rank {r} counted {n_ex} exchanges and {n_vol} doubles, expected "
                                 f"{times * has_neighbour[r]} and {sent_once[r]}")
        sent_f, sent_r = H.sent_doubles(spaces), H.sent_doubles(spaces, reverse=True)
        assert min(sent_f) > 0 and min(sent_r) > 0
        before, after = [r[s]["forward"][0] for r in records], [r[s]["forward"][1] for r in records]
        found += tag("forward", H.check_forward(spaces, before, after))
        counters("forward", sent_f)
        for what, exact in (("reverse_exact", True), ("reverse_rounded", False)):
            before, after = [r[s][what][0] for r in records], [r[s][what][1] for r in records]
            found += tag(what, H.check_reverse(spaces, before, after, exact=exact))
            counters(what, sent_r)
            if not exact:
                ref = H.reverse(spaces, before)
                worst = max(float(np.max(np.abs(a.astype(np.longdouble) - e.ref)[e.m > 0] / (e.m * H.U * e.mag)[e.m > 0])) for a, e in zip(after, ref))
                print(f"  reverse, rounded: up to {max(int(e.m.max()) for e in ref)} additions into an entry, worst error {worst:.3f} of its bound")
        # forward then reverse on one vector: the same bits with and without a synchronisation in between, and the restatement's
        before = [r[s]["chain"][0] for r in records]
        for what in ("chain", "chain_sync"):
            after = [r[s][what][1] for r in records]
            found += tag(what, H.check_reverse(spaces, H.forward(spaces, before), after, exact=True))
            counters(what, [a + b for a, b in zip(sent_f, sent_r)], times=2)
        for r, rec in enumerate(records):
            if not np.array_equal(rec[s]["chain"][1].view(np.int64), rec[s]["chain_sync"][1].view(np.int64)):
                found.append(f"space {s}: rank {r}: two exchanges back to back differ from the two with a synchronisation in between")
        xs, ys = [r[s]["dot"][0] for r in records], [r[s]["dot"][1] for r in records]
        first, second = [r[s]["dot"][2] for r in records], [r[s]["dot"][3] for r in records]
        found += tag("owned dot", H.check_dot(spaces, xs, ys, first))
        if np.array(first).tobytes() != np.array(second).tobytes():
            found.append(f"space {s} owned dot: a second call gave other bits: {first} / {second}")
        ref, mag, _ = H.owned_dot(spaces, xs, ys)
        print(f"  owned dot: error {float(abs(np.longdouble(first[0]) - ref) / mag):.3e} of sum|xy|, bound {k * H.U:.3e}")
        if s == 1:
            assert all(r[s]["f32_widths"] == records[0][s]["f32_widths"] for r in records)
            for w in records[0][s]["f32_widths"]:
                before, after = [r[s][("f32", w)][0] for r in records], [r[s][("f32", w)][1] for r in records]
                assert all(a.dtype == np.float32 for a in after)
                found += tag(f"float forward, width {w}", H.check_forward(spaces, before, after, width=w))
                counters(("f32", w), H.sent_doubles(spaces, width=w))
    return found, seen


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_exchanges_and_owned_dot_entry_by_entry(mfmg_lib, case):
    grid, per, material, n_eig, amg, low_ghost, show = CASES[case]
    parts = _parts(case)
    n_ranks = len(parts)
    params = {"eigensolver": {"number of eigenvectors": n_eig}, "agglomeration": {"nx": 2, "ny": 2, "nz": 2},
              "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0},
              "solver": {"type": "amg", "amg": dict(amg)}, "is preconditioner": False}
    mb = Mailboxes(n_ranks, timeout=60)
    records, errors = [None] * n_ranks, [None] * n_ranks

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            part = parts[rank]
            ctx = M.Context()
            tr = M.HaloTransport(ctx, part, callbacks=mb.callbacks(rank))
            assert tr.name() == "host"
            h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", part.local_problem(material, "cuda"), params)
            records[rank] = _rank_run(ctx, tr, part, rank, low_ghost)
            ctx.synchronize()
            del h
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors[rank] = e
            mb.barrier.abort()
            for p in range(n_ranks):      # wake the neighbours that wait for a message of this rank
                mb.q[(rank, p)].put(np.zeros(0))

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    first = next((e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError)), None) or \
        next((e for e in errors if e is not None), None)
    if first is not None:
        raise first
    assert all(r is not None for r in records)
    found, seen = _compare(case, records)
    print(f"{case}: comps {sorted(seen['comps'])} widths {sorted(seen['widths'])}, spaces with one owned layer along a split axis: {seen['thin']}")
    assert found == [], "\n".join(found)
    assert seen["comps"] == show["comps"] and seen["widths"] >= show["widths"], (seen, show)
    if "levels" in show:      # local, fine, first coarse + the aggregation levels that stayed distributed (+ the two-deep fine space)
        assert len(records[0]) >= 2 + show["levels"], sorted(records[0])
