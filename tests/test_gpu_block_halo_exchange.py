"""The block halo exchange (HipHandle::exchange_block, regions_copy_block_kernel; Context.exchange_block / HaloTransport.exchange_block)
entry by entry, against the one-vector exchange of every column and against tests/halo_reference.py.

Ranks are threads of one process behind the host transport with in-memory mailboxes, set up as in tests/test_gpu_halo_exchange.py
(the cases and partitions are imported from there): slabs with one neighbour (slabs_2) and with two (the middle rank of
slabs_3_comps_3) -- which pack here, unlike the one-vector double exchange --, boxes split along x, along y, and the 2 x 2 x 2 grid
with seven neighbours per rank.  Space 1, widths 1 .. min(3, low_ghost), k = 1, 2, 3, 4, 5, 7 columns.

A block lives in a flat buffer of (k + 2) ld doubles, ld = n_local + 6 (+ 1 where that is odd): a guard column on either side of the
k columns.  EVERYTHING but the owned entries of the columns holds one NaN payload (a quiet NaN with a recognisable mantissa); the
owned entries of column c hold node * 4 + 0.25 + c 2^22 of the GLOBAL node: distinct per node and column, exact.  Per width and k:
  1  every column equals, bit for bit, what halo_reference.forward makes of it (inside the dilated box the owner's value, every
     other entry its old bits -- the payload), and at width 1 also what the one-vector HaloTransport.exchange makes of a copy
  2  the guard columns and the entries [n_local, ld) of every column keep the payload
  3  the exchange count grows by one, exchange_volume by k times the doubles the restatement sends for one vector
  4  refused (MfmgInvalidArgument, before anything travels, so on every rank alike): another space, width 0 and a width beyond the
     ghost planes, an odd ld, 0 and 65 columns, a base off 16 bytes, an ld below the local vector's size"""
import threading

import numpy as np
import pytest
import torch

import halo_reference as H
import mfmg_amd as M
from mfmg_amd import lib as L
from test_box_threads import Mailboxes
from test_gpu_halo_exchange import CASES as ALL_CASES, _parts

CASE_IDS = ["slabs_2", "slabs_3_comps_3", "boxes_x", "boxes_y", "boxes_xyz_comps_1"]
KS = (1, 2, 3, 4, 5, 7)
PAYLOAD = np.array([0x7FF8_0000_0BAD_F00D], dtype=np.uint64).view(np.float64)[0]
PAYLOAD_BITS = np.int64(0x7FF8_0000_0BAD_F00D)


def _columns(sp, k):
    """k local vectors: owned entries distinct per node and column, the payload elsewhere"""
    base = H.forward_input(sp)
    own = H.owned_mask(sp)
    cols = []
    for c in range(k):
        v = np.full(H.n_local(sp), PAYLOAD)
        v[own] = base[own] + c * 2.0 ** 22
        cols.append(v)
    return cols


def _rank_run(ctx, tr, part, low_ghost):
    low = [part.coord[d] > 0 for d in range(3)]
    high = [part.coord[d] + 1 < part.grid[d] for d in range(3)]
    sp = H.make_space(tr.box(1), 1, low, high)
    n = H.n_local(sp)
    assert tr.space(1)["layer_elems"] * tr.space(1)["n_layers"] == n
    ld = n + 6 + ((n + 6) & 1)
    widths = list(range(1, min(3, low_ghost) + 1))
    rec = {"space": sp, "widths": widths, "ld": ld, "runs": {}}
    for w in widths:
        assert H.precondition(sp, w) == [], (sp, w)
        for k in KS:
            cols = _columns(sp, k)
            flat = np.full((k + 2) * ld, PAYLOAD)
            for c in range(k):
                flat[(c + 1) * ld: (c + 1) * ld + n] = cols[c]
            dev = torch.from_numpy(flat).cuda()
            block = dev.view(k + 2, ld)[1: k + 1]
            assert block.data_ptr() % 16 == 0 and block.stride(0) == ld
            torch.cuda.synchronize()
            e0, v0 = tr.n_exchanges(), tr.exchange_volume()
            tr.exchange_block(1, block, w)
            ctx.synchronize()
            counted = (tr.n_exchanges() - e0, tr.exchange_volume() - v0)
            single = None
            if w == 1:      # the one-vector exchange of a copy of every column
                single = []
                for c in range(k):
                    v = torch.from_numpy(cols[c]).cuda()
                    tr.exchange(1, v)
                    ctx.synchronize()
                    single.append(v.cpu().numpy())
            rec["runs"][(w, k)] = (cols, dev.cpu().numpy(), counted, single)
    # ---- refusals: every rank raises before anything travels
    buf = torch.zeros(3 * ld + 2, dtype=torch.float64, device="cuda")
    lib = L.load()

    def refused(space, k, ld_, ptr, width, what):
        with pytest.raises(L.MfmgInvalidArgument, match=what):
            L.check(lib.mfmg_hip_context_exchange_block(ctx.handle, space, k, ld_, ptr, width))
    e0 = tr.n_exchanges()
    refused(2, 2, ld, buf.data_ptr(), 1, "fine DoF space")
    refused(0, 2, ld, buf.data_ptr(), 1, "fine DoF space")
    refused(1, 2, ld, buf.data_ptr(), 0, "width")
    refused(1, 2, ld, buf.data_ptr(), widths[-1] + 1, "width")
    refused(1, 2, ld + 1, buf.data_ptr(), 1, "even")
    refused(1, 0, ld, buf.data_ptr(), 1, "1 to 64")
    refused(1, 65, ld, buf.data_ptr(), 1, "1 to 64")
    refused(1, 2, ld, buf.data_ptr() + 8, 1, "16 bytes")
    refused(1, 2, (n - 1) & ~1, buf.data_ptr(), 1, "at least the vector size")
    with pytest.raises(ValueError):
        tr.exchange_block(1, buf[: 2 * ld].view(2, ld).float(), 1)            # a float block never reaches the entry point
    ctx.synchronize()
    assert tr.n_exchanges() == e0 and not bool(buf.any().item())
    return rec


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _compare(case, records):
    found = []
    spaces = [r["space"] for r in records]
    assert all(r["widths"] == records[0]["widths"] for r in records)
    for w in records[0]["widths"]:
        sent = H.sent_doubles(spaces, width=w)
        assert min(sent) > 0
        for k in KS:
            runs = [r["runs"][(w, k)] for r in records]
            for c in range(k):
                before = [run[0][c] for run in runs]
                after = []
                for r, run in enumerate(runs):
                    ld, n = records[r]["ld"], H.n_local(spaces[r])
                    after.append(run[1][(c + 1) * ld: (c + 1) * ld + n])
                found += [f"width {w} k {k} column {c}: {f}" for f in H.check_forward(spaces, before, after, width=w)]
                if w == 1:
                    for r, run in enumerate(runs):
                        if not np.array_equal(_bits(after[r]), _bits(run[3][c])):
                            found.append(f"width 1 k {k} column {c}: rank {r} differs from the one-vector exchange of the column")
            for r, run in enumerate(runs):
                ld, n = records[r]["ld"], H.n_local(spaces[r])
                flat = _bits(run[1]).reshape(k + 2, ld)
                if (flat[0] != PAYLOAD_BITS).any() or (flat[k + 1] != PAYLOAD_BITS).any():
                    found.append(f"width {w} k {k}: rank {r}: a guard column was written")
                if (flat[1: k + 1, n:] != PAYLOAD_BITS).any():
                    found.append(f"width {w} k {k}: rank {r}: entries between the columns were written")
                if run[2] != (1, k * sent[r]):
                    found.append(f"width {w} k {k}: rank {r} counted {run[2][0]} exchanges and {run[2][1]} doubles, expected 1 and {k * sent[r]}")
    return found


def test_the_payload_is_a_nan_that_keeps_its_bits():
    assert np.isnan(PAYLOAD) and _bits(np.full(3, PAYLOAD))[1] == PAYLOAD_BITS
    assert set(CASE_IDS) <= set(ALL_CASES)
    # the cases reach one, two and seven neighbours; slabs and boxes; both ghost depths (widths up to 2 and up to 3)
    assert {ALL_CASES[c][5] for c in CASE_IDS} == {2, 4}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASE_IDS)
def test_block_exchange_entry_by_entry(mfmg_lib, case):
    grid, per, material, n_eig, amg, low_ghost, show = ALL_CASES[case]
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
            # (the hierarchy only so that the fine space is configured the way real runs configure it)
            h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", part.local_problem(material, "cuda"), params)
            records[rank] = _rank_run(ctx, tr, part, low_ghost)
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
    found = _compare(case, records)
    print(f"{case}: {n_ranks} ranks, widths {records[0]['widths']}, k {KS}, local vectors of {[H.n_local(r['space']) for r in records]} entries")
    assert found == [], "\n".join(found[:40])


@pytest.mark.gpu
def test_block_exchange_without_a_communicator_is_a_no_op(mfmg_lib):
    ctx = M.Context()
    v = torch.full((3, 64), 2.5, dtype=torch.float64, device="cuda")
    ctx.exchange_block(1, v, 1)
    ctx.synchronize()
    assert bool((v == 2.5).all().item())
    with pytest.raises(L.MfmgInvalidArgument):
        ctx.exchange_block(2, v, 1)
