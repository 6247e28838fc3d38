"""The owned-box Gram-Schmidt kernels of the distributed solve_fgmres (krylov_basis.hip, OwnedBox) on one rank, through
mfmg_hip_krylov_orthogonalize_box: on a context without a communicator the sum over the ranks is the identity.

V and w are local vectors of a rank -- the lexicographic box of `local` nodes, `comps` entries per node -- of which the nodes
[own0, own0 + own_n) are owned.  Every GHOST entry of V and w, and the padding of the columns, holds NaN: a kernel that lets one
into a sum, or reads a pair for its ghost half and multiplies it by zero, fails every bound below.  The ghost entries of w must
come back with the bits they went in with (basis_update leaves them alone).

Bounds: those of tests/test_gpu_fgmres.py for the contiguous kernels, built the same way with n = the number of OWNED entries
(u = 2^-53, gamma_k = k u / (1 - k u), references in long double over the owned entries):
  dots     |h_i - V_i.w| <= gamma_{n+2} sum|V_i||w|
  update   one pass, against the long-double result formed from the h the kernel returned: gamma_{j+3} (|w| + sum|h_i||V_i|)
  norm     gamma_{n+2} relative
  CGS2     two passes on a V that is orthonormal over the owned entries: max|V_i.w| / ||w|| <= 64 u sqrt(n), and the summed h
           within (|E||h1|)_i + |Q_i|.|d1| + gamma_{n+2} |Q_i|.(|w1| + |d1|) + u |h_i| (head of tests/test_gpu_fgmres.py)

Shapes: rows that start at odd entries and are shorter than a wavefront, with ghosts on some sides only; a row longer than one pass
of a wavefront at two doubles per lane; a slab (x and y whole: one contiguous run); more than one reduction block, with the last
owned entry the last (odd) entry of the local vector -- the one pair that must not be loaded whole; two entries per node; x whole
or y whole alone (rows that join, rows that do not); and more slots than the fixed grid has threads, so that the grid stride is
carried through rows and planes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble

# name: (local nodes, first owned node, owned nodes, entries per node)
SHAPES = {
    "odd_rows": ((13, 11, 9), (3, 2, 0), (9, 7, 6), 1),
    "long_row": ((135, 5, 4), (2, 1, 1), (131, 3, 2), 1),
    "slab": ((9, 9, 12), (0, 0, 2), (9, 9, 8), 1),
    "blocks": ((43, 43, 43), (3, 3, 3), (40, 40, 40), 1),
    "two_comps": ((7, 5, 6), (1, 0, 2), (5, 5, 3), 2),
    "y_whole": ((11, 5, 7), (1, 0, 2), (9, 5, 4), 1),
    "x_whole": ((5, 7, 6), (0, 2, 1), (5, 3, 4), 1),
}
# 63 slots per row x 65 x 66 rows = 270270 slots > 1024 blocks x 256 threads: the second trip of the grid-stride loop
STRIDE_SHAPE = ((129, 67, 68), (3, 1, 2), (125, 65, 66), 1)
COLUMNS = [1, 8, 9, 17]


def gamma(k):
    return k * U / (1.0 - k * U)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()


def signed_decades(rng, shape):
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)


def owned_index(shape):
    local, own0, own_n, comps = shape
    k = np.arange(own0[2], own0[2] + own_n[2]).reshape(-1, 1, 1, 1)
    j = np.arange(own0[1], own0[1] + own_n[1]).reshape(1, -1, 1, 1)
    i = np.arange(own0[0], own0[0] + own_n[0]).reshape(1, 1, -1, 1)
    return ((((k * local[1] + j) * local[0] + i) * comps) + np.arange(comps).reshape(1, 1, 1, -1)).reshape(-1)


def n_local(shape):
    local, _, _, comps = shape
    return comps * local[0] * local[1] * local[2]


def poisoned(owned_values, shape):
    """the owned values inside local vectors of NaN: [..., ld], ld = the local size rounded up to even"""
    nl = n_local(shape)
    out = np.full(owned_values.shape[:-1] + ((nl + 1) // 2 * 2,), np.nan)
    out[..., owned_index(shape)] = owned_values
    return out


def orthogonalize(ctx, shape, V_owned, w_owned, passes, misalign_w=False):
    """-> h, the owned entries of w, ||w||, and the local w before and after as raw bits"""
    nl, k = n_local(shape), V_owned.shape[0]
    w_in = poisoned(w_owned, shape)[:nl]
    if misalign_w:
        wd = torch.empty(nl + 1, dtype=torch.float64, device="cuda")[1:]
        assert wd.data_ptr() % 16 == 8
        wd.copy_(dev(w_in))
    else:
        wd = dev(w_in)
    h, norm = ctx.krylov_orthogonalize(dev(poisoned(V_owned, shape)), wd, k, passes, box=shape)
    ctx.synchronize()
    w_out = wd.cpu().numpy()
    return h.cpu().numpy(), w_out[owned_index(shape)], float(norm.cpu()[0]), w_in.view(np.uint64), w_out.view(np.uint64)


def ghosts_untouched(shape, bits_in, bits_out):
    ghost = np.ones(n_local(shape), bool)
    ghost[owned_index(shape)] = False
    return ghost.any() and np.array_equal(bits_in[ghost], bits_out[ghost])


_inputs = {}


def kernel_inputs(name, shape, k):
    if (name, k) not in _inputs:
        n = owned_index(shape).size
        rng = np.random.default_rng(1000 * k + n)
        V, w = signed_decades(rng, (k, n)), signed_decades(rng, n)
        V.setflags(write=False)
        w.setflags(write=False)
        _inputs[(name, k)] = (V, w, V.astype(LD), w.astype(LD))
    return _inputs[(name, k)]


def check_one_pass(ctx, name, shape, k, misalign_w=False):
    V, w, Vl, wl = kernel_inputs(name, shape, k)
    n = w.size
    h, w_out, norm, bits_in, bits_out = orthogonalize(ctx, shape, V, w, 1, misalign_w)
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(w_out)) and np.isfinite(norm)
    h_ref = (Vl * wl).sum(axis=1)
    h_bound = gamma(n + 2) * (np.abs(Vl) * np.abs(wl)).sum(axis=1)
    assert np.all(np.abs(h.astype(LD) - h_ref) <= h_bound), (np.abs(h - h_ref) / h_bound).max()
    hl = h.astype(LD)
    w_ref = wl - (hl[:, None] * Vl).sum(axis=0)
    w_bound = gamma((k - 1) + 3) * (np.abs(wl) + (np.abs(hl)[:, None] * np.abs(Vl)).sum(axis=0))
    assert np.all(np.abs(w_out.astype(LD) - w_ref) <= w_bound), (np.abs(w_out - w_ref) / w_bound).max()
    norm_ref = np.sqrt((w_out.astype(LD) ** 2).sum())
    assert abs(LD(norm) - norm_ref) <= gamma(n + 2) * norm_ref
    assert ghosts_untouched(shape, bits_in, bits_out)
    # a repeated launch gives the same bits
    h2, w2, norm2, _, bits2 = orthogonalize(ctx, shape, V, w, 1, misalign_w)
    assert h.tobytes() == h2.tobytes() and norm == norm2 and np.array_equal(bits_out, bits2)


@pytest.mark.parametrize("k", COLUMNS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_pass_over_the_owned_entries_against_long_double(ctx, name, k):
    check_one_pass(ctx, name, SHAPES[name], k)


@pytest.mark.parametrize("k", COLUMNS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_two_passes_leave_w_orthogonal_over_the_owned_entries(ctx, name, k):
    shape = SHAPES[name]
    n = owned_index(shape).size
    assert n > k
    rng = np.random.default_rng(7 * n + k)
    Q = np.linalg.qr(rng.standard_normal((n, k)))[0].T.copy()
    w = signed_decades(rng, n)
    h, w_out, norm, bits_in, bits_out = orthogonalize(ctx, shape, Q, w, 2)
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(w_out)) and np.isfinite(norm)
    wl = w_out.astype(LD)
    norm_ref = np.sqrt((wl ** 2).sum())
    assert norm_ref > 0 and abs(LD(norm) - norm_ref) <= gamma(n + 2) * norm_ref
    ratio = float(np.abs((Q.astype(LD) * wl).sum(axis=1)).max() / norm_ref)
    assert ratio <= 64 * U * np.sqrt(n), ratio
    Ql, w0 = Q.astype(LD), w.astype(LD)
    h1 = Ql @ w0
    w1 = w0 - h1 @ Ql
    d1 = gamma((k - 1) + 3) * (np.abs(w0) + np.abs(h1) @ np.abs(Ql))
    E = Ql @ Ql.T - np.eye(k, dtype=LD)
    h_bound = (1 + 1e-3) * (np.abs(E) @ np.abs(h1) + np.abs(Ql) @ d1 + gamma(n + 2) * (np.abs(Ql) @ (np.abs(w1) + d1)) + U * np.abs(h1))
    assert np.all(np.abs(h.astype(LD) - h1) <= h_bound), float((np.abs(h.astype(LD) - h1) / h_bound).max())
    assert ghosts_untouched(shape, bits_in, bits_out)
    h2, _, norm2, _, bits2 = orthogonalize(ctx, shape, Q, w, 2)
    assert h.tobytes() == h2.tobytes() and norm == norm2 and np.array_equal(bits_out, bits2)


@pytest.mark.parametrize("name,k", [("odd_rows", 9), ("blocks", 17), ("slab", 8)])
def test_a_w_off_the_16_byte_grid_takes_the_scalar_loads(ctx, name, k):
    check_one_pass(ctx, name, SHAPES[name], k, misalign_w=True)


@pytest.mark.parametrize("k", [1, 9])
def test_the_grid_stride_is_carried_through_rows_and_planes(ctx, k):
    check_one_pass(ctx, "stride", STRIDE_SHAPE, k)


def test_arguments_are_checked(ctx):
    from mfmg_amd import lib as L
    shape = SHAPES["odd_rows"]
    V, w, _, _ = kernel_inputs("odd_rows", shape, 1)
    Vd, wd = dev(poisoned(V, shape)), dev(poisoned(w, shape)[:n_local(shape)])
    with pytest.raises(L.MfmgInvalidArgument, match="owned box"):
        ctx.krylov_orthogonalize(Vd, wd, 1, 1, box=(shape[0], (3, 2, 4), shape[2], 1))
