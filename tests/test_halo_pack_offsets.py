"""The index arithmetic of the packed halo exchange on the host (halo_box_messages, halo_region_entry of common.hpp through
mfmg_hip_halo_box_messages; no GPU): what the float packing kernel reads and the unpacking kernel writes, against numpy slicing
of the local box, for the grids of tests/test_gpu_fp32_distributed.py and the widths 1 to 3.
  - the entries of every message are the slices exchange_box documents: `width` owned layers next to the neighbour along the axes
    with an offset, the owned range along the others; received into the ghost layers beyond them
  - every entry lies inside the local vector, no ghost entry is written twice, no owned entry is written at all
  - what rank a sends to rank b is, global node by global node, what b receives from a: same count, same order
  - a slab has the two messages of its contiguous form: the lower neighbour first, `width` whole planes each"""
import itertools

import numpy as np
import pytest

import mfmg_amd as M
from mfmg_amd.distributed import box_messages

# (grid, cells, low_ghost_cells): the partitions of the multi-rank tests at their mesh sizes, and 2 x 2 x 2 with its corners
GRIDS = [((1, 1, 2), (16, 16, 48), 2), ((2, 1, 1), (48, 24, 24), 4), ((2, 1, 2), (48, 24, 48), 2), ((2, 2, 2), (8, 8, 8), 4)]


def _messages(part, width):
    box = {"dims": part.local_nodes, "own0": part.own0, "own_n": part.own_n, "comps": 1}
    low = [part.coord[d] > 0 for d in range(3)]
    high = [part.coord[d] + 1 < part.grid[d] for d in range(3)]
    return box_messages(box, low, high, width, part.rank, part.grid)


def _expected(part, width):
    """(peers, send slices, recv slices) in the order of exchange_box: offsets with z slowest, x fastest."""
    nx, ny, nz = part.local_nodes
    ids = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    peers, send, recv = [], [], []
    for oz, oy, ox in itertools.product((-1, 0, 1), repeat=3):
        o = (ox, oy, oz)
        if o == (0, 0, 0) or any((o[d] < 0 and part.coord[d] == 0) or (o[d] > 0 and part.coord[d] + 1 == part.grid[d]) for d in range(3)):
            continue
        s_own, s_ghost = [], []
        for d in range(3):
            o0, o1 = part.own0[d], part.own0[d] + part.own_n[d]
            s_own.append(slice(o0, o0 + width) if o[d] < 0 else slice(o1 - width, o1) if o[d] > 0 else slice(o0, o1))
            s_ghost.append(slice(o0 - width, o0) if o[d] < 0 else slice(o1, o1 + width) if o[d] > 0 else slice(o0, o1))
        peers.append(part.rank + ox + part.grid[0] * (oy + part.grid[1] * oz))
        send.append(ids[s_own[2], s_own[1], s_own[0]].ravel())
        recv.append(ids[s_ghost[2], s_ghost[1], s_ghost[0]].ravel())
    return peers, send, recv


@pytest.mark.parametrize("grid,cells,low_ghost", GRIDS)
def test_packed_entries_are_the_slices_of_the_local_box(mfmg_lib, grid, cells, low_ghost):
    world = grid[0] * grid[1] * grid[2]
    for width in (1, 2, 3):
        if width > low_ghost:
            continue
        sent = {}
        parts = [M.BoxPartition(cells, r, grid, low_ghost_cells=low_ghost) for r in range(world)]
        for part in parts:
            peers, counts, send, recv = _messages(part, width)
            e_peers, e_send, e_recv = _expected(part, width)
            assert list(peers) == e_peers and list(counts) == [len(s) for s in e_send]
            np.testing.assert_array_equal(send, np.concatenate(e_send))
            np.testing.assert_array_equal(recv, np.concatenate(e_recv))
            assert counts.sum() == part.exchange_doubles(width)
            # inside the vector; ghost entries written once; owned entries never written, and only owned entries sent
            owned = np.zeros(part.n_local_dofs, bool)
            owned[part.owned_local_index().numpy()] = True
            assert recv.min() >= 0 and recv.max() < part.n_local_dofs and send.min() >= 0 and send.max() < part.n_local_dofs
            assert len(np.unique(recv)) == len(recv) and not owned[recv].any() and owned[send].all()
            loc_g = part.local_global_index().numpy()
            off = np.concatenate([[0], np.cumsum(counts)])
            for i, p in enumerate(peers):
                sent[(part.rank, int(p))] = loc_g[send[off[i]:off[i + 1]]]
                sent[("recv", part.rank, int(p))] = loc_g[recv[off[i]:off[i + 1]]]
        # the pairing: the global nodes a sends to b, in order, are the global nodes b receives from a
        pairs = [k for k in sent if k[0] != "recv"]
        assert pairs
        for a, b in pairs:
            np.testing.assert_array_equal(sent[(a, b)], sent[("recv", b, a)])


def test_a_slab_packs_the_messages_of_its_contiguous_form(mfmg_lib):
    part = M.BoxPartition((16, 16, 48), 1, (1, 1, 3), low_ghost_cells=2)
    plane = part.local_nodes[0] * part.local_nodes[1]
    for width in (1, 2):
        peers, counts, send, recv = _messages(part, width)
        assert list(peers) == [0, 2] and list(counts) == [width * plane] * 2
        z0, z1 = part.own0[2], part.own0[2] + part.own_n[2]
        np.testing.assert_array_equal(send, np.concatenate([np.arange(z0 * plane, (z0 + width) * plane), np.arange((z1 - width) * plane, z1 * plane)]))
        np.testing.assert_array_equal(recv, np.concatenate([np.arange((z0 - width) * plane, z0 * plane), np.arange(z1 * plane, (z1 + width) * plane)]))


def test_an_exchange_wider_than_the_ghost_layers_is_refused(mfmg_lib):
    part = M.BoxPartition((16, 16, 48), 1, (1, 1, 2), low_ghost_cells=2)
    with pytest.raises(M.lib.MfmgInvalidArgument):
        _messages(part, 3)


def test_the_condition_of_an_exchange_says_what_is_missing(mfmg_lib):
    """halo_check_width, the condition every exchange checks before it packs: the owned box `width` thick, `width` ghost layers on
    every side with a neighbour -- and nothing asked of an axis without neighbours."""
    from mfmg_amd import lib as L
    box = {"dims": (5, 4, 9), "own0": (0, 0, 3), "own_n": (5, 4, 4), "comps": 2}      # three ghost planes below, two above
    none, z = [False] * 3, [False, False, True]
    peers, counts, _, _ = box_messages(box, z, z, 2, 1, (1, 1, 3))
    assert list(peers) == [0, 2] and list(counts) == [2 * 5 * 4 * 2] * 2
    for low, high, width, text in ((z, z, 3, "fewer ghost layers above"), (z, none, 4, "fewer ghost layers below"),
                                   (none, z, 3, "fewer ghost layers above")):
        with pytest.raises(L.MfmgInvalidArgument, match=text):
            box_messages(box, low, high, width, 1, (1, 1, 3))
    assert len(box_messages(box, z, none, 3, 1, (1, 1, 3))[0]) == 1                  # three planes below: enough for width 3
    thin = dict(box, own_n=(5, 4, 1), dims=(5, 4, 9))
    with pytest.raises(L.MfmgInvalidArgument):
        box_messages(thin, z, z, 2, 1, (1, 1, 3))
