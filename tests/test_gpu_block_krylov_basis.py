"""The basis kernels of the block FGMRES driver (block_krylov_basis.hip) through their own entry points,
Context.block_krylov_orthogonalize and Context.block_krylov_combine, against the one-vector kernels run per slot on copies
(Context.krylov_orthogonalize, Context.krylov_combine): coefficients, norms, w, v_next and x bit for bit.

Layout: basis vector i of slot s is V[i, s, :n] of a (vectors, k, ld) block, so for one slot the vectors are k ld apart -- the
leading dimension the one-vector call gets on its copy is ld alone, the bits must not care.  Vector lengths: 1 and 2 (the tail
alone, one 16-byte unit), 511 (odd), 131,073 (many blocks and a tail), 524,291 (past 1024 blocks x 256 threads x 2 entries: a
second grid-stride trip).  Basis lengths j = 0, 7, 8, 16: the edges of the groups of eight columns.  k = 1, 3, 5 slots with the
live lists: all, {0, 2}, {k - 1} alone.  Of k > 1 slots the last has a w in the span of its basis, in exact arithmetic (unit
vectors): its norm is exactly zero and the zero-norm branch of scale_store runs.  Dead slots, the padding beyond n, and the rows
around the block hold a NaN payload nobody computes, and hold it afterwards.

Against long double at two shapes, with the bounds of tests/test_gpu_fgmres.py part 1 (u = 2^-53, gamma_k = k u / (1 - k u)).
This entry point runs the two passes of the driver, so the bounds are those part 1 has for two passes on an orthonormal basis --
max |V_i . w| / ||w|| <= 64 u sqrt(n) and the bound of the summed coefficients derived at the head of that file --, the norm
(gamma_{n+2} relative, of the w returned), combine (gamma_{j+3} (|x| + sum |y_i||Z_i|)), and for v_next = w (1 / ||w||), two
roundings and the reference's own, gamma_3 relative."""
import numpy as np
import pytest
import torch

import mfmg_amd as M

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble
PAYLOAD = 0x7FF8DEAD0000BEEF          # a quiet NaN nobody computes
SIZES = [1, 2, 511, 131073, 524291]
BASIS = [0, 7, 8, 16]


def gamma(k):
    return k * U / (1.0 - k * U)


def live_lists(k):
    out = [list(range(k))]
    if k >= 3:
        out.append([0, 2])
    if k > 1:
        out.append([k - 1])
    return out


def payload(shape):
    return torch.full(shape, PAYLOAD, dtype=torch.int64, device="cuda").view(torch.float64)


def untouched(t):
    return bool((t.contiguous().view(torch.int64) == PAYLOAD).all().item())


_inputs = {}


def inputs(n, j, k):
    """V [j + 2, k, n] on the device (vector j + 1 is w), computed once per shape, shared and left unchanged: values over six
    decades.  Of k > 1 slots the last has a w in the span of its basis, chosen so that the arithmetic is exact: its first
    min(n, j + 1) basis vectors are unit vectors spread over the vector (the first and the last entry among them), the others
    zero, w a combination of the unit vectors.  Then h is the combination, w - sum h_i V_i is exactly zero after the first pass,
    and the zero-norm branch of scale_store runs."""
    if (n, j, k) not in _inputs:
        g = torch.Generator(device="cuda")
        g.manual_seed(1000 * j + 10 * k + n % 997)
        V = torch.randn((j + 2, k, n), dtype=torch.float64, device="cuda", generator=g)
        V *= 10.0 ** (6.0 * torch.rand((j + 2, k, n), dtype=torch.float64, device="cuda", generator=g) - 3.0)
        if k > 1:
            s, units = k - 1, min(n, j + 1)
            V[:, s] = 0.0
            where = [(i * (n - 1)) // max(units - 1, 1) for i in range(units)]
            assert len(set(where)) == units
            for i, e in enumerate(where):
                V[i, s, e] = 1.0
                V[j + 1, s, e] = float(torch.randn(1, generator=g, device="cuda", dtype=torch.float64))
        _inputs[(n, j, k)] = V
    return _inputs[(n, j, k)]


_reference = {}


def reference(ctx, n, j, k):
    """per slot: (h, norm, w, v_next, v_next as float) of the one-vector kernels on contiguous copies with ld = n rounded up"""
    if (n, j, k) not in _reference:
        V = inputs(n, j, k)
        ld = n + (n & 1)
        out = []
        for s in range(k):
            Vs = torch.zeros((j + 1, ld), dtype=torch.float64, device="cuda")
            Vs[:, :n] = V[: j + 1, s]
            w = V[j + 1, s].clone()
            h, norm = ctx.krylov_orthogonalize(Vs, w, j + 1, 2)
            ctx.synchronize()
            nrm = float(norm.cpu()[0])
            v = w * (1.0 / nrm) if nrm > 0 else torch.zeros_like(w)       # (IEEE: one division, one product per entry)
            out.append((h.clone(), nrm, w, v, v.to(torch.float32)))
        _reference[(n, j, k)] = out
    return _reference[(n, j, k)]


def basis_block(V, n, ld):
    """the (vectors, k, ld) block of a launch inside guard rows, everything that is not an entry of a vector the payload"""
    nv, k = V.shape[0], V.shape[1]
    blk = payload((nv + 2, k, ld))
    blk[1:nv + 1, :, :n] = V
    return blk


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("j", BASIS)
@pytest.mark.parametrize("n", SIZES)
def test_block_orthogonalize_equals_the_one_vector_kernels(ctx, n, j, k):
    V = inputs(n, j, k)
    ref = reference(ctx, n, j, k)
    ld = n + 4 + (n & 1)
    if k > 1:
        # the slot whose w lies in the span of its basis: an exactly zero norm, zeros stored, nothing divided by zero
        assert ref[k - 1][1] == 0.0 and bool((ref[k - 1][3] == 0.0).all()) and bool(torch.isfinite(ref[k - 1][0]).all())
    for live in live_lists(k):
        blk = basis_block(V, n, ld)
        work = blk[1:j + 3]
        v_next, v_f32 = payload((k, ld)), torch.full((k, ld), -7.0, dtype=torch.float32, device="cuda")
        h, norm = ctx.block_krylov_orthogonalize(n, work, j, live, v_next, v_f32)
        ctx.synchronize()
        what = f"n {n} j {j} k {k} live {live}"
        for s in range(k):
            if s in live:
                hr, nr, wr, vr, vfr = ref[s]
                assert torch.equal(h[s], hr), f"{what}: coefficients of slot {s}"
                assert float(norm[s].cpu()) == nr, f"{what}: norm of slot {s}"
                assert torch.equal(work[j + 1, s, :n], wr), f"{what}: w of slot {s}"
                assert torch.equal(v_next[s, :n], vr), f"{what}: v_next of slot {s}"
                assert torch.equal(v_f32[s, :n], vfr), f"{what}: float copy of slot {s}"
                assert torch.equal(work[: j + 1, s, :n], V[: j + 1, s]), f"{what}: the basis of slot {s} changed"
            else:
                # a dead slot is neither read (its NaN would spread) nor written
                assert bool(torch.isnan(h[s]).all()) and bool(torch.isnan(norm[s])), f"{what}: dead slot {s} got coefficients"
                assert torch.equal(work[:, s, :n], V[:, s]), f"{what}: dead slot {s} changed"
                assert untouched(v_next[s]) and bool((v_f32[s] == -7.0).all()), f"{what}: dead slot {s} got a v_next"
        assert untouched(blk[0]) and untouched(blk[j + 3]) and untouched(work[:, :, n:]), f"{what}: wrote outside the vectors"
        assert untouched(v_next[:, n:]) and bool((v_f32[:, n:] == -7.0).all()), f"{what}: wrote into the padding of v_next"


@pytest.mark.parametrize("n,j", [(511, 7), (131073, 16)])
def test_block_orthogonalize_against_long_double(ctx, n, j):
    k = 3
    V = inputs(n, j, k)
    ld = n + (n & 1)
    blk = basis_block(V, n, ld)
    v_next = payload((k, ld))
    h, norm = ctx.block_krylov_orthogonalize(n, blk[1:j + 3], j, [0, 1, 2], v_next)
    ctx.synchronize()
    # every slot: the norm of the w returned, the normalisation
    for s in range(k):
        wl = blk[j + 2, s, :n].cpu().numpy().astype(LD)
        norm_ref = np.sqrt((wl ** 2).sum())
        nrm = float(norm[s].cpu())
        assert np.isfinite(nrm) and abs(LD(nrm) - norm_ref) <= gamma(n + 2) * norm_ref, s
        v = v_next[s, :n].cpu().numpy().astype(LD)
        if nrm > 0:
            assert np.all(np.abs(v - wl / LD(nrm)) <= gamma(3) * np.abs(wl / LD(nrm))), s
    # slot 0 with an orthonormal basis of its own: "twice is enough", and the summed coefficients
    Q = np.linalg.qr(np.random.default_rng(n + j).standard_normal((n, j + 1)))[0].T.copy()
    Vq = V.clone()
    Vq[: j + 1, 0] = torch.from_numpy(Q).cuda()
    blk = basis_block(Vq, n, ld)
    h, norm = ctx.block_krylov_orthogonalize(n, blk[1:j + 3], j, [0, 2])
    ctx.synchronize()
    wl = blk[j + 2, 0, :n].cpu().numpy().astype(LD)
    norm_ref = np.sqrt((wl ** 2).sum())
    assert norm_ref > 0 and abs(LD(float(norm[0].cpu())) - norm_ref) <= gamma(n + 2) * norm_ref
    Ql, w0 = Q.astype(LD), V[j + 1, 0].cpu().numpy().astype(LD)
    ratio = float(np.abs(Ql @ wl).max() / norm_ref)
    assert ratio <= 64 * U * np.sqrt(n), ratio
    h1 = Ql @ w0
    w1 = w0 - h1 @ Ql
    d1 = gamma(j + 3) * (np.abs(w0) + np.abs(h1) @ np.abs(Ql))
    E = Ql @ Ql.T - np.eye(j + 1, dtype=LD)
    h_bound = (1 + 1e-3) * (np.abs(E) @ np.abs(h1) + np.abs(Ql) @ d1 + gamma(n + 2) * (np.abs(Ql) @ (np.abs(w1) + d1)) + U * np.abs(h1))
    hl = h[0].cpu().numpy().astype(LD)
    assert np.all(np.abs(hl - h1) <= h_bound), float((np.abs(hl - h1) / h_bound).max())


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("j", BASIS)
@pytest.mark.parametrize("n", SIZES)
def test_block_combine_equals_the_one_vector_kernel(ctx, n, j, k):
    Z = inputs(n, j, k)[: j + 1]
    g = torch.Generator(device="cuda")
    g.manual_seed(3 * n + j + k)
    y = torch.randn((k, j + 1), dtype=torch.float64, device="cuda", generator=g)
    x0 = torch.randn((k + 2, n), dtype=torch.float64, device="cuda", generator=g)
    slot_col = [(k + 1) - s for s in range(k)]                          # the columns of x in reverse, columns 0 and 1 partly unused
    ld, ldz = n + (n & 1), n + 4 + (n & 1)
    ref = []
    for s in range(k):
        Zs = torch.zeros((j + 1, ld), dtype=torch.float64, device="cuda")
        Zs[:, :n] = Z[:, s]
        x = x0[slot_col[s]].clone()
        ctx.krylov_combine(Zs, y[s].clone(), x)
        ref.append(x)
    ctx.synchronize()
    # x with an odd leading dimension: every second column is aligned to 8 bytes only; and an even, 16-byte aligned one
    for ldx in (n + 3 - (n & 1), n + 2 + (n & 1)):
        for live in live_lists(k):
            blk = payload((j + 3, k, ldz))
            blk[1:j + 2, :, :n] = Z
            X = payload((k + 2, ldx))
            X[:, :n] = x0
            ctx.block_krylov_combine(n, blk[1:j + 2], y, live, slot_col, X)
            ctx.synchronize()
            what = f"n {n} j {j} k {k} ldx {ldx} live {live}"
            written = {slot_col[s]: s for s in live}
            for c in range(k + 2):
                want = ref[written[c]] if c in written else x0[c]
                assert torch.equal(X[c, :n], want), f"{what}: column {c} of x"
            assert untouched(X[:, n:]), f"{what}: wrote into the padding of x"
            assert torch.equal(blk[1:j + 2, :, :n], Z) and untouched(blk[0]) and untouched(blk[j + 2]) and untouched(blk[:, :, n:]), what


@pytest.mark.parametrize("n,j", [(511, 7), (131073, 16)])
def test_block_combine_against_long_double(ctx, n, j):
    k = 3
    Z = inputs(n, j, k)[: j + 1]
    rng = np.random.default_rng(n + j)
    y = rng.choice([-1.0, 1.0], size=(k, j + 1)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(k, j + 1))
    x0 = rng.standard_normal((k, n))
    ld = n + (n & 1)
    blk = payload((j + 1, k, ld))
    blk[:, :, :n] = Z
    X = payload((k, ld))
    X[:, :n] = torch.from_numpy(x0).cuda()
    ctx.block_krylov_combine(n, blk, torch.from_numpy(y).cuda(), [0, 1, 2], [0, 1, 2], X)
    ctx.synchronize()
    for s in range(k):
        Zl, yl, xl = Z[:, s].cpu().numpy().astype(LD), y[s].astype(LD), x0[s].astype(LD)
        ref = xl + (yl[:, None] * Zl).sum(axis=0)
        bound = gamma(j + 3) * (np.abs(xl) + (np.abs(yl)[:, None] * np.abs(Zl)).sum(axis=0))
        assert np.all(np.abs(X[s, :n].cpu().numpy().astype(LD) - ref) <= bound), s


def test_refusals(ctx):
    from mfmg_amd import lib as L
    V = torch.zeros((3, 2, 10), dtype=torch.float64, device="cuda")
    with pytest.raises(L.MfmgInvalidArgument, match="ascending"):
        ctx.block_krylov_orthogonalize(10, V, 1, [1, 0])
    with pytest.raises(L.MfmgInvalidArgument, match="live"):
        ctx.block_krylov_orthogonalize(10, V, 1, [])
    with pytest.raises(L.MfmgInvalidArgument, match="ascending"):
        ctx.block_krylov_orthogonalize(10, V, 1, [0, 2])                # slot 2 of a block of two
    with pytest.raises(L.MfmgInvalidArgument, match="even"):
        ctx.block_krylov_orthogonalize(9, torch.zeros((3, 2, 9), dtype=torch.float64, device="cuda"), 1, [0])
    X = torch.zeros((2, 10), dtype=torch.float64, device="cuda")
    y = torch.zeros((2, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(L.MfmgInvalidArgument, match="one column"):
        ctx.block_krylov_combine(10, V, y, [0, 1], [1, 1], X)
    with pytest.raises(L.MfmgInvalidArgument, match="outside x"):
        ctx.block_krylov_combine(10, V, y, [0, 1], [0, 2], X)
