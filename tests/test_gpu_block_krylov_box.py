"""The owned-box block reduction of solve_cg_block on several ranks (block_krylov.hip: block_dots_box_stage1_kernel,
block_krylov::dots on a krylov::OwnedBox) on one rank alone, through mfmg_hip_block_dots_box / Context.block_dots_box: on a context
without a communicator the sum over the ranks is the identity (after tests/test_gpu_krylov_box.py).

X and Y are blocks of a rank's local vectors -- the lexicographic box of `local` nodes, `comps` entries per node -- of which the nodes
[own0, own0 + own_n) are owned.  Every GHOST entry, the entries between the columns and a guard column on either side hold NaN: a
kernel that lets one into a sum fails both checks.

  bits    slot s equals, bit for bit, the rank-local sum of HaloTransport.owned_dot formed the one-vector way (distributed_dot): the
          owned entries of the two vectors packed in the order of box_copy_kernel (x fastest, then y, then z; a slab's run as it
          lies) and reduced by the one-vector dot product (Context.dot) over n_owned entries
  bound   |slot - long-double sum| <= k 2^-53 sum |x_i y_i|, k = halo_reference.dot_chain(n_owned, 1) -- the chain of roundings of
          the two-stage reduction (tests/test_gpu_halo_exchange.py derives it)

Shapes: three differing local and owned extents with ghosts on some sides only and rows that start at odd entries; a slab (x and y
owned whole: one contiguous run); an owned range two nodes thick along every axis; two entries per node; x whole or y whole alone;
more than one reduction block; and more owned entries than the fixed grid has threads (1024 blocks x 256), so that a thread adds
more than one product and the grid stride is carried through rows and planes.  Slots: 1, 2, 4, 5, 7."""
import numpy as np
import pytest
import torch

import halo_reference as H

LD = np.longdouble

# name: (local nodes, first owned node, owned nodes, entries per node)
SHAPES = {
    "three_extents": ((13, 11, 9), (3, 2, 0), (9, 7, 6), 1),
    "slab": ((9, 9, 12), (0, 0, 2), (9, 9, 8), 1),
    "two_thick": ((7, 8, 9), (2, 3, 4), (2, 2, 2), 1),
    "two_comps": ((7, 5, 6), (1, 0, 2), (5, 5, 3), 2),
    "y_whole": ((11, 5, 7), (1, 0, 2), (9, 5, 4), 1),
    "x_whole": ((5, 7, 6), (0, 2, 1), (5, 3, 4), 1),
    "blocks": ((43, 43, 43), (3, 3, 3), (40, 40, 40), 1),
    "stride": ((129, 67, 68), (3, 1, 2), (125, 65, 66), 1),
}
SLOTS = (1, 2, 4, 5, 7)


def owned_index(shape):
    local, own0, own_n, comps = shape
    k = np.arange(own0[2], own0[2] + own_n[2]).reshape(-1, 1, 1, 1)
    j = np.arange(own0[1], own0[1] + own_n[1]).reshape(1, -1, 1, 1)
    i = np.arange(own0[0], own0[0] + own_n[0]).reshape(1, 1, -1, 1)
    return ((((k * local[1] + j) * local[0] + i) * comps) + np.arange(comps).reshape(1, 1, 1, -1)).reshape(-1)


def n_local(shape):
    local, _, _, comps = shape
    return comps * local[0] * local[1] * local[2]


_inputs = {}


def inputs(name):
    """owned values of 7 slots, spread over six decades with both signs (computed once, read-only)"""
    if name not in _inputs:
        n = owned_index(SHAPES[name]).size
        rng = np.random.default_rng(n)
        x = rng.choice([-1.0, 1.0], size=(max(SLOTS), n)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(max(SLOTS), n))
        y = rng.choice([-1.0, 1.0], size=(max(SLOTS), n)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(max(SLOTS), n))
        x.setflags(write=False)
        y.setflags(write=False)
        _inputs[name] = (x, y)
    return _inputs[name]


def block(owned_values, shape):
    """(flat device buffer, the block of k rows inside it): guard rows, ghosts and the entries between the rows are NaN"""
    k, nl = owned_values.shape[0], n_local(shape)
    ld = nl + 6 + ((nl + 6) & 1)
    flat = np.full((k + 2, ld), np.nan)
    flat[1: k + 1, owned_index(shape)] = owned_values
    dev = torch.from_numpy(flat).cuda()
    return dev, dev[1: k + 1]


def test_the_shapes_reach_the_edges_they_name():
    assert len({*SHAPES["three_extents"][0]}) == 3 and len({*SHAPES["three_extents"][2]}) == 3
    local, own0, own_n, _ = SHAPES["slab"]
    assert own_n[:2] == local[:2] and own0[:2] == (0, 0) and own_n[2] < local[2]
    assert SHAPES["two_thick"][2] == (2, 2, 2)
    n = {name: owned_index(s).size for name, s in SHAPES.items()}
    assert n["blocks"] > 256 and n["blocks"] <= 1024 * 256 < n["stride"]
    # the chain of roundings: one trip of the grid-stride loop and one partial per thread of the second stage below 65 537 owned
    # entries; three trips and four partials at "stride"
    assert H.dot_chain(n["blocks"], 1) == 21 and H.dot_chain(n["stride"], 1) == 26
    for s in SHAPES.values():
        assert all(s[1][d] + s[2][d] <= s[0][d] for d in range(3)) and owned_index(s).max() < n_local(s)


@pytest.mark.gpu
@pytest.mark.parametrize("k", SLOTS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_slot_has_the_bits_of_the_one_vector_owned_sum(ctx, name, k):
    shape = SHAPES[name]
    x, y = inputs(name)
    x, y = x[:k], y[:k]
    n = x.shape[1]
    keep_x, X = block(x, shape)
    keep_y, Y = block(y, shape)
    out = ctx.block_dots_box(shape, X, Y)
    ctx.synchronize()
    got = out.cpu().numpy()
    again = ctx.block_dots_box(shape, X, Y).cpu().numpy()
    assert got.tobytes() == again.tobytes()
    chain = H.dot_chain(n, 1)
    worst = 0.0
    for s in range(k):
        # the one-vector way: the owned entries packed, then the one-vector dot product
        one = ctx.dot(torch.from_numpy(np.array(x[s])).cuda(), torch.from_numpy(np.array(y[s])).cuda())
        assert np.isfinite(got[s]) and np.float64(got[s]).tobytes() == np.float64(one).tobytes(), (name, k, s, got[s], one)
        p = x[s].astype(LD) * y[s].astype(LD)
        err, mag = abs(LD(got[s]) - p.sum()), np.abs(p).sum()
        assert err <= chain * LD(H.U) * mag, (name, k, s, float(err / mag), chain)
        worst = max(worst, float(err / (chain * LD(H.U) * mag)))
    print(f"{name} k {k}: {n} owned of {n_local(shape)} entries, chain {chain}, worst error {worst:.3f} of its bound")
    # the inputs keep their bits (the kernel writes the partials and the result alone)
    assert torch.isnan(keep_x[0]).all() and torch.isnan(keep_x[k + 1]).all() and torch.isnan(keep_y[0]).all()


@pytest.mark.gpu
def test_arguments_are_checked(ctx, mfmg_lib):
    from mfmg_amd import lib as L
    import mfmg_amd as M
    shape = SHAPES["three_extents"]
    x, y = inputs("three_extents")
    _, X = block(x[:2], shape)
    _, Y = block(y[:2], shape)
    with pytest.raises(L.MfmgInvalidArgument, match="owned box"):
        ctx.block_dots_box((shape[0], (3, 2, 4), shape[2], 1), X, Y)
    with pytest.raises(L.MfmgInvalidArgument, match="bad shape"):
        ctx.block_dots_box(((14, 11, 9), shape[1], shape[2], 1), X[:, : n_local(shape)], Y[:, : n_local(shape)])
    # the kernels of ONE rank: a context with a communicator is refused (no transport is needed: nothing runs)
    own = M.Context()
    L.check(mfmg_lib.mfmg_hip_context_set_communicator(own.handle, 0, 2, 0, 2))
    with pytest.raises(L.MfmgInvalidArgument, match="communicator"):
        own.block_dots_box(shape, X, Y)
