"""The float block halo exchange (HipHandle::exchange_block_f32, regions_copy_block_f32_kernel; Context.exchange_block_f32 /
HaloTransport.exchange_block_f32) entry by entry, against the one-vector float exchange of every column.

Ranks are threads of one process behind the host transport with in-memory mailboxes, set up as in
tests/test_gpu_block_halo_exchange.py (cases and partitions from tests/test_gpu_halo_exchange.py): a slab and a box that hold four
ghost planes below (widths 1 to 3), and a box split along x (widths 1 and 2).  Every rank's local vector has an odd number of
entries.  Space 1, k = 1, 2, 4, 5 columns.

A block lives in a flat buffer of (k + 2) ld floats, ld = n_local + 6 (+ 1 where that is odd): a guard column on either side of the
k columns.  EVERYTHING but the owned entries of the columns holds one NaN payload; the owned entries of column c hold
node * 4 + 0.25 + c 2^17 of the GLOBAL node: distinct per node and column, exact in float.  Per width and k:
  1  every column equals, bit for bit, what Context.exchange_f32 makes of a copy of it -- ghost entries and all
  2  the owned entries keep their bits; the guard columns and the entries [n_local, ld) of every column keep the payload
  3  the exchange count grows by one, exchange_volume by k times what the one-vector float exchange of that width adds
  4  refused (MfmgInvalidArgument, before anything travels): another space, width 0 and a width beyond the ghost planes, an odd ld,
     0 and 65 columns, a base off 8 bytes, an ld below the local vector's size; a double block never reaches the entry point"""
import threading

import numpy as np
import pytest
import torch

import halo_reference as H
import mfmg_amd as M
from mfmg_amd import lib as L
from test_box_threads import Mailboxes
from test_gpu_halo_exchange import CASES as ALL_CASES, _parts

CASE_IDS = ["slabs_2_deep", "boxes_y", "boxes_x"]
KS = (1, 2, 4, 5)
PAYLOAD_BITS = np.int32(0x7FC0BEEF)
PAYLOAD = np.array([PAYLOAD_BITS]).view(np.float32)[0]


def _columns(sp, k):
    """k local float vectors: owned entries distinct per node and column, the payload elsewhere"""
    base = H.forward_input(sp)
    own = H.owned_mask(sp)
    cols = []
    for c in range(k):
        v = np.full(H.n_local(sp), PAYLOAD, dtype=np.float32)
        wide = base[own] + c * 2.0 ** 17
        v[own] = wide.astype(np.float32)
        assert np.array_equal(v[own].astype(np.float64), wide)          # exact in float
        cols.append(v)
    return cols


def _rank_run(ctx, tr, part, low_ghost):
    low = [part.coord[d] > 0 for d in range(3)]
    high = [part.coord[d] + 1 < part.grid[d] for d in range(3)]
    sp = H.make_space(tr.box(1), 1, low, high)
    n = H.n_local(sp)
    assert n % 2 == 1
    ld = n + 6 + ((n + 6) & 1)
    widths = list(range(1, min(3, low_ghost) + 1))
    rec = {"space": sp, "widths": widths, "ld": ld, "n": n, "runs": {}}
    for w in widths:
        one_volume = None
        for k in KS:
            cols = _columns(sp, k)
            single = []
            for c in range(k):      # the one-vector float exchange of a copy of every column
                v = torch.from_numpy(cols[c]).cuda()
                v0 = tr.exchange_volume()
                ctx.exchange_f32(1, v, w)
                ctx.synchronize()
                one_volume = tr.exchange_volume() - v0
                single.append(v.cpu().numpy())
            flat = np.full((k + 2) * ld, PAYLOAD, dtype=np.float32)
            for c in range(k):
                flat[(c + 1) * ld: (c + 1) * ld + n] = cols[c]
            dev = torch.from_numpy(flat).cuda()
            block = dev.view(k + 2, ld)[1: k + 1]
            assert block.data_ptr() % 8 == 0 and block.stride(0) == ld
            torch.cuda.synchronize()
            e0, v0 = tr.n_exchanges(), tr.exchange_volume()
            tr.exchange_block_f32(1, block, w)
            ctx.synchronize()
            counted = (tr.n_exchanges() - e0, tr.exchange_volume() - v0)
            rec["runs"][(w, k)] = (cols, dev.cpu().numpy(), counted, single, one_volume)
    # ---- refusals: every rank raises before anything travels
    buf = torch.zeros(3 * ld + 2, dtype=torch.float32, device="cuda")
    lib = L.load()

    def refused(space, k, ld_, ptr, width, what):
        with pytest.raises(L.MfmgInvalidArgument, match=what):
            L.check(lib.mfmg_hip_context_exchange_block_f32(ctx.handle, space, k, ld_, ptr, width))
    e0 = tr.n_exchanges()
    refused(2, 2, ld, buf.data_ptr(), 1, "fine DoF space")
    refused(1, 2, ld, buf.data_ptr(), 0, "width")
    refused(1, 2, ld, buf.data_ptr(), widths[-1] + 1, "width")
    refused(1, 2, ld + 1, buf.data_ptr(), 1, "even")
    refused(1, 0, ld, buf.data_ptr(), 1, "1 to 64")
    refused(1, 65, ld, buf.data_ptr(), 1, "1 to 64")
    refused(1, 2, ld, buf.data_ptr() + 4, 1, "8 bytes")
    refused(1, 2, (n - 1) & ~1, buf.data_ptr(), 1, "at least the vector size")
    with pytest.raises(ValueError):
        tr.exchange_block_f32(1, buf[: 2 * ld].view(2, ld).double(), 1)
    ctx.synchronize()
    assert tr.n_exchanges() == e0 and not bool(buf.any().item())
    return rec


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _compare(records):
    found = []
    for r, rec in enumerate(records):
        sp, ld, n = rec["space"], rec["ld"], rec["n"]
        own = H.owned_mask(sp)
        for (w, k), (cols, after, counted, single, one_volume) in rec["runs"].items():
            flat = _bits(after).reshape(k + 2, ld)
            where = f"rank {r} width {w} k {k}"
            changed = 0
            for c in range(k):
                got = flat[c + 1, :n]
                if not np.array_equal(got, _bits(single[c])):
                    found.append(f"{where} column {c}: differs from the one-vector float exchange of the column")
                if not np.array_equal(got[own], _bits(cols[c])[own]):
                    found.append(f"{where} column {c}: an owned entry was written")
                changed += int((got != _bits(cols[c])).sum())
            if changed == 0:
                found.append(f"{where}: no ghost entry was refreshed")
            if (flat[0] != PAYLOAD_BITS).any() or (flat[k + 1] != PAYLOAD_BITS).any():
                found.append(f"{where}: a guard column was written")
            if (flat[1: k + 1, n:] != PAYLOAD_BITS).any():
                found.append(f"{where}: entries between the columns were written")
            if one_volume <= 0 or counted != (1, k * one_volume):
                found.append(f"{where}: counted {counted[0]} exchanges and {counted[1]} doubles, expected 1 and {k} x {one_volume}")
    return found


def test_the_payload_is_a_nan_that_keeps_its_bits():
    assert np.isnan(PAYLOAD) and _bits(np.full(3, PAYLOAD, dtype=np.float32))[1] == PAYLOAD_BITS
    assert set(CASE_IDS) <= set(ALL_CASES)
    # a slab and a box that reach width 3, a box that stops at 2
    assert [ALL_CASES[c][5] for c in CASE_IDS] == [4, 4, 2]
    assert [_parts(c)[0].split_xy for c in CASE_IDS] == [False, True, True]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASE_IDS)
def test_float_block_exchange_entry_by_entry(mfmg_lib, case):
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
    found = _compare(records)
    print(f"{case}: {n_ranks} ranks, widths {records[0]['widths']}, k {KS}, local vectors of {[r['n'] for r in records]} entries")
    assert found == [], "\n".join(found[:40])


@pytest.mark.gpu
def test_float_block_exchange_without_a_communicator_is_a_no_op(mfmg_lib):
    ctx = M.Context()
    v = torch.full((3, 64), 2.5, dtype=torch.float32, device="cuda")
    ctx.exchange_block_f32(1, v, 1)
    ctx.synchronize()
    assert bool((v == 2.5).all().item())
    with pytest.raises(L.MfmgInvalidArgument):
        ctx.exchange_block_f32(2, v, 1)
