"""The owned-box block Gram-Schmidt kernels of solve_fgmres_block on several ranks (block_krylov_basis.hip, the krylov::OwnedBox
overloads) on one rank, through Context.block_krylov_orthogonalize_box: on a context without a communicator the sum over the ranks
is the identity.

A basis block is a (j + 3, k, ld) tensor: vectors 0 .. j of every slot, w = vector j + 1, and vector j + 2 as a GUARD; ld = the local
size rounded up to even plus 4.  Everything but the owned entries of the live slots' vectors 0 .. j + 1 holds one NaN payload: the
ghost entries, the padding [n_local, ld), the guard vector and the slots that are not live.  The shapes are those of
tests/test_gpu_krylov_box.py (imported), k = 1, 2, 5, 7 slots with live lists that have gaps, j + 1 = 1, 8, 9, 17 basis vectors.

Per case:
  1  h, the norm and the updated w of every live slot are bit-equal to Context.krylov_orthogonalize(..., box=...) on that slot's
     vectors (two passes); v_next is bit-equal to w * (1 / norm) of that result -- the expression of both scale_store kernels, IEEE
     in numpy as on the device (the one-vector entry point returns no v_next)
  2  everything else of the block and of v_next keeps the bits it went in with: ghost entries, padding, guard vector, dead slots
  3  a second call on the same input gives the same bits
One case is checked against long double with the bounds of tests/test_gpu_krylov_box.py (gamma_{n+2}, n the owned entries, on an
orthonormal V: the CGS2 bounds stated there), so that the block kernel and the one-vector kernel cannot be wrong together."""
import numpy as np
import pytest
import torch

from test_gpu_krylov_box import LD, SHAPES, STRIDE_SHAPE, U, dev, gamma, n_local, owned_index, signed_decades

pytestmark = pytest.mark.gpu
PAYLOAD_BITS = np.uint64(0x7FF8_0000_0BAD_F00D)
PAYLOAD = np.array([PAYLOAD_BITS]).view(np.float64)[0]
# slots of the block -> the live ones (ascending; gaps, a dead first slot, a dead last slot)
LIVE = {1: (0,), 2: (1,), 5: (0, 2, 4), 7: (0, 2, 3, 6)}
COLUMNS = [1, 8, 9, 17]


def build_block(shape, k, live, n_columns, seed, orthonormal=False):
    """-> the block (n_columns + 2, k, ld) with the payload everywhere but the owned entries of the live slots, and those entries
    per live slot: V_owned [n_columns, n], w_owned [n]"""
    nl, own = n_local(shape), owned_index(shape)
    ld = (nl + 1) // 2 * 2 + 4
    block = np.full((n_columns + 2, k, ld), PAYLOAD)
    rng = np.random.default_rng(seed)
    owned = {}
    for s in live:
        if orthonormal:
            V = np.linalg.qr(rng.standard_normal((own.size, n_columns)))[0].T.copy()
        else:
            V = signed_decades(rng, (n_columns, own.size))
        w = signed_decades(rng, own.size)
        block[:n_columns, s, own] = V
        block[n_columns, s, own] = w
        owned[s] = (V, w)
    return block, owned


def run_block(ctx, shape, block, n_columns, live):
    k, ld = block.shape[1], block.shape[2]
    Vd = dev(block)
    v_next = dev(np.full((k, ld), PAYLOAD))
    assert Vd.data_ptr() % 16 == 0 and v_next.data_ptr() % 16 == 0
    h, norm = ctx.block_krylov_orthogonalize_box(shape, Vd, n_columns - 1, live, v_next=v_next)
    ctx.synchronize()
    return h.cpu().numpy(), norm.cpu().numpy(), Vd.cpu().numpy(), v_next.cpu().numpy()


def one_vector(ctx, shape, block, n_columns, s):
    """Context.krylov_orthogonalize on the vectors of slot s, aligned to 16 bytes with an even leading dimension (the 16-byte
    kernels the working blocks of a solve take): h, the local w after, the norm"""
    nl = n_local(shape)
    Vd = dev(block[:n_columns, s, : (nl + 1) // 2 * 2])
    wd = dev(block[n_columns, s, :nl])
    assert Vd.data_ptr() % 16 == 0 and wd.data_ptr() % 16 == 0
    h, norm = ctx.krylov_orthogonalize(Vd, wd, n_columns, 2, box=shape)
    ctx.synchronize()
    return h.cpu().numpy(), wd.cpu().numpy(), norm.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_case(ctx, shape, k, n_columns, seed):
    live = LIVE[k]
    nl, own = n_local(shape), owned_index(shape)
    block, _ = build_block(shape, k, live, n_columns, seed)
    h, norm, after, v_next = run_block(ctx, shape, block, n_columns, live)
    touched = np.zeros(block.shape, bool)
    touched_next = np.zeros(v_next.shape, bool)
    for s in live:
        h1, w1, norm1 = one_vector(ctx, shape, block, n_columns, s)
        assert np.all(np.isfinite(h1)) and np.isfinite(norm1[0]) and norm1[0] > 0
        assert h[s].tobytes() == h1.tobytes(), (s, h[s], h1)
        assert norm[s].tobytes() == norm1[0].tobytes(), (s, norm[s], norm1)
        assert after[n_columns, s, :nl].tobytes() == w1.tobytes(), s     # owned entries updated, ghost entries the payload, in both
        expected = w1[own] * (1.0 / norm1[0])
        assert v_next[s, own].tobytes() == expected.tobytes(), s
        touched[n_columns, s, own] = True
        touched_next[s, own] = True
    # ghost entries of w and v_next, padding, the basis itself, the guard vector, dead slots: the bits they went in with
    assert np.array_equal(bits(after)[~touched], bits(block)[~touched])
    assert np.all(bits(v_next)[~touched_next] == PAYLOAD_BITS)
    dead = np.array([s for s in range(k) if s not in live], dtype=int)
    assert np.all(np.isnan(h[dead])) and np.all(np.isnan(norm[dead]))
    # two calls give equal bits
    h2, norm2, after2, v_next2 = run_block(ctx, shape, block, n_columns, live)
    assert h2.tobytes() == h.tobytes() and norm2.tobytes() == norm.tobytes()
    assert after2.tobytes() == after.tobytes() and v_next2.tobytes() == v_next.tobytes()


@pytest.mark.parametrize("n_columns", COLUMNS)
@pytest.mark.parametrize("k", sorted(LIVE))
@pytest.mark.parametrize("name", [n for n in sorted(SHAPES) if n != "blocks"])
def test_every_live_slot_has_the_bits_of_the_one_vector_box_kernels(ctx, name, k, n_columns):
    check_case(ctx, SHAPES[name], k, n_columns, 100 * k + n_columns)


# (more than one reduction block, the last owned entry the last -- odd -- entry of the local vector: fewer combinations, 64000 owned
# entries per vector)
@pytest.mark.parametrize("k,n_columns", [(2, 9), (5, 1), (7, 8)])
def test_more_than_one_reduction_block(ctx, k, n_columns):
    check_case(ctx, SHAPES["blocks"], k, n_columns, 7 * k + n_columns)


def test_the_grid_stride_is_carried_through_rows_and_planes(ctx):
    check_case(ctx, STRIDE_SHAPE, 2, 2, 11)


def test_two_passes_against_long_double(ctx):
    """The bounds at the head of tests/test_gpu_krylov_box.py for CGS2 on a V that is orthonormal over the owned entries, per live
    slot of a block: the norm within gamma_{n+2} relative, max|V_i.w| / ||w|| <= 64 u sqrt(n), the summed h within the bound of
    test_two_passes_leave_w_orthogonal_over_the_owned_entries."""
    shape, k, n_columns = SHAPES["odd_rows"], 7, 9
    live = LIVE[k]
    own = owned_index(shape)
    n = own.size
    block, owned = build_block(shape, k, live, n_columns, 5, orthonormal=True)
    h, norm, after, v_next = run_block(ctx, shape, block, n_columns, live)
    for s in live:
        Q, w = owned[s]
        w_out = after[n_columns, s, own]
        assert np.all(np.isfinite(h[s])) and np.all(np.isfinite(w_out)) and np.isfinite(norm[s])
        wl = w_out.astype(LD)
        norm_ref = np.sqrt((wl ** 2).sum())
        assert norm_ref > 0 and abs(LD(norm[s]) - norm_ref) <= gamma(n + 2) * norm_ref
        ratio = float(np.abs((Q.astype(LD) * wl).sum(axis=1)).max() / norm_ref)
        assert ratio <= 64 * U * np.sqrt(n), ratio
        Ql, w0 = Q.astype(LD), w.astype(LD)
        h1 = Ql @ w0
        w1 = w0 - h1 @ Ql
        d1 = gamma((n_columns - 1) + 3) * (np.abs(w0) + np.abs(h1) @ np.abs(Ql))
        E = Ql @ Ql.T - np.eye(n_columns, dtype=LD)
        h_bound = (1 + 1e-3) * (np.abs(E) @ np.abs(h1) + np.abs(Ql) @ d1 + gamma(n + 2) * (np.abs(Ql) @ (np.abs(w1) + d1)) + U * np.abs(h1))
        assert np.all(np.abs(h[s].astype(LD) - h1) <= h_bound), float((np.abs(h[s].astype(LD) - h1) / h_bound).max())
        # v_next = w (1 / ||w||): one rounding of the reciprocal, one of the product -- (1 + u)^2 - 1 < 3 u
        assert np.all(np.abs(v_next[s, own].astype(LD) - wl / LD(norm[s])) <= 3 * U * np.abs(wl / LD(norm[s])))


def test_arguments_are_checked(ctx):
    from mfmg_amd import lib as L
    shape = SHAPES["odd_rows"]
    block, _ = build_block(shape, 2, (0, 1), 1, 3)
    Vd = dev(block)
    with pytest.raises(L.MfmgInvalidArgument, match="owned box"):
        ctx.block_krylov_orthogonalize_box((shape[0], (3, 2, 4), shape[2], 1), Vd, 0, (0, 1))
    with pytest.raises(L.MfmgInvalidArgument, match="ascending"):
        ctx.block_krylov_orthogonalize_box(shape, Vd, 0, (1, 0))
    with pytest.raises(ValueError):
        ctx.block_krylov_orthogonalize_box(shape, Vd[:, :, :100].contiguous(), 0, (0, 1))
