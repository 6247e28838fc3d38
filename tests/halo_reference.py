"""A plain restatement of what the halo exchanges and the owned-box reduction of a distributed run compute, from the DESCRIPTION
of a vector space alone (numpy only; no GPU, no call into the library).

A space is what HaloTransport.box(space) says about it on every rank -- comps, dims, own0, own_n, g0, gn, each per axis
(x, y, z) -- plus the width of its exchanges and which neighbours the rank has.  Nothing here enumerates regions or messages (that
arithmetic -- halo_box_messages, halo_region_entry, the packing kernels -- is what the tests check): everything follows from
GLOBAL ids.  Entry ((k ny + j) nx + i) comps + c of a local vector is component c of the global node (i + g0x, j + g0y, k + g0z).

  forward   the dilated owned box is the owned box grown by `width` layers along every axis, clipped to the local box.  A local
            entry inside it that is not owned takes the value its owner holds for the same global id and component; every other
            entry keeps its bits.
  reverse   every rank contributes its entries in the same shell (dilated box minus owned box); each contribution is added to the
            owner's entry of that global id.  Owned entries outside all shells and EVERY ghost entry of every rank keep their
            bits (regions_copy_kernel mode 2 writes through the regions of the owned boundary layers only, and the slab branch of
            exchange_reverse_add adds to owned planes only: neither writes a ghost entry).  The order of the additions is not
            specified: an owned entry that receives m contributions lies within m 2^-53 sum |addends| of the exact sum.
  dot       the long-double sum of x_i y_i over the entries each rank owns; every global entry is counted once.
  sent      doubles a rank sends in one exchange: forward, the pairs (entry of a neighbour's shell that this rank owns, that
            neighbour); reverse, the entries of its own shell (each has one owner).

The check_* functions compare what a run produced with the restatement and return a list of findings (empty: all is well);
tests/test_halo_reference_bites.py shows that they notice planted errors, tests/test_gpu_halo_exchange.py hands them the GPU's
results."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -53

Space = namedtuple("Space", "comps dims own0 own_n g0 gn width low high")


def make_space(box, width, low, high):
    """box: the dict of HaloTransport.box; low / high: per axis, whether a neighbour exists on that side"""
    t = lambda v: tuple(int(x) for x in v)
    return Space(int(box["comps"]), t(box["dims"]), t(box["own0"]), t(box["own_n"]), t(box["g0"]), t(box["gn"]), int(width),
                 tuple(bool(v) for v in low), tuple(bool(v) for v in high))


def n_local(sp):
    return sp.comps * sp.dims[0] * sp.dims[1] * sp.dims[2]


def n_global(sp):
    return sp.comps * sp.gn[0] * sp.gn[1] * sp.gn[2]


def _per_entry(sp, per_axis):
    """per_axis[d]: one value per local node index along axis d; combined over the entries of a local vector (z slowest, x
    fastest, comps innermost) by the caller's rule -- returned as the three broadcastable arrays"""
    return (np.asarray(per_axis[0]).reshape(1, 1, -1, 1), np.asarray(per_axis[1]).reshape(1, -1, 1, 1), np.asarray(per_axis[2]).reshape(-1, 1, 1, 1))


def global_ids(sp):
    """global entry id (global node id * comps + component) of every local entry"""
    gx, gy, gz = _per_entry(sp, [np.arange(sp.dims[d], dtype=np.int64) + sp.g0[d] for d in range(3)])
    c = np.arange(sp.comps, dtype=np.int64).reshape(1, 1, 1, -1)
    return ((((gz * sp.gn[1] + gy) * sp.gn[0] + gx) * sp.comps) + c).reshape(-1)


def _box_mask(sp, lo, hi):
    ax = [(np.arange(sp.dims[d]) >= lo[d]) & (np.arange(sp.dims[d]) < hi[d]) for d in range(3)]
    mx, my, mz = _per_entry(sp, ax)
    return np.broadcast_to(mx & my & mz, (sp.dims[2], sp.dims[1], sp.dims[0], sp.comps)).reshape(-1).copy()


def owned_mask(sp):
    return _box_mask(sp, sp.own0, [sp.own0[d] + sp.own_n[d] for d in range(3)])


def dilated_mask(sp, width=None):
    w = sp.width if width is None else int(width)
    return _box_mask(sp, [max(sp.own0[d] - w, 0) for d in range(3)], [min(sp.own0[d] + sp.own_n[d] + w, sp.dims[d]) for d in range(3)])


def shell_mask(sp, width=None):
    return dilated_mask(sp, width) & ~owned_mask(sp)


def precondition(sp, width=None):
    """findings against: along every axis with a neighbour the owned box is `width` thick and `width` ghost layers lie there"""
    w = sp.width if width is None else int(width)
    out = []
    for d in range(3):
        if (sp.low[d] or sp.high[d]) and sp.own_n[d] < w:
            out.append(f"axis {d}: {sp.own_n[d]} owned layers, exchange {w} wide")
        if sp.low[d] and sp.own0[d] < w:
            out.append(f"axis {d}: {sp.own0[d]} ghost layers below, exchange {w} wide")
        if sp.high[d] and sp.dims[d] - sp.own0[d] - sp.own_n[d] < w:
            out.append(f"axis {d}: {sp.dims[d] - sp.own0[d] - sp.own_n[d]} ghost layers above, exchange {w} wide")
    return out


def owner_map(spaces):
    """rank that owns every global entry; every global entry is owned exactly once"""
    ng = n_global(spaces[0])
    times = np.zeros(ng, dtype=np.int64)
    owner = np.full(ng, -1, dtype=np.int64)
    for r, sp in enumerate(spaces):
        assert n_global(sp) == ng and sp.comps == spaces[0].comps
        g = global_ids(sp)[owned_mask(sp)]
        np.add.at(times, g, 1)
        owner[g] = r
    assert (times == 1).all(), "the owned boxes of the ranks do not tile the global box"
    return owner


def owner_values(spaces, vectors):
    out = np.empty(n_global(spaces[0]), dtype=vectors[0].dtype)
    for sp, v in zip(spaces, vectors):
        m = owned_mask(sp)
        out[global_ids(sp)[m]] = v[m]
    return out


def local_coords(sp):
    """(i, j, k, c) of every local entry: its node along x, y, z and its component"""
    i, j, k = _per_entry(sp, [np.arange(sp.dims[d], dtype=np.int64) for d in range(3)])
    shape = (sp.dims[2], sp.dims[1], sp.dims[0], sp.comps)
    c = np.arange(sp.comps, dtype=np.int64).reshape(1, 1, 1, -1)
    return tuple(np.broadcast_to(a, shape).reshape(-1) for a in (i, j, k, c))


# ---- the inputs of the checks ---------------------------------------------------------------------------------------------------
def forward_input(sp, dtype=np.float64):
    """owned entries: node * 4 + component + 0.25 of the GLOBAL node (distinct, exact in float32 below 2^20 nodes); the rest NaN"""
    assert sp.comps <= 4 and sp.gn[0] * sp.gn[1] * sp.gn[2] < 2 ** 20
    g = global_ids(sp)
    v = np.full(n_local(sp), np.nan, dtype=dtype)
    own = owned_mask(sp)
    v[own] = ((g // sp.comps) * 4 + g % sp.comps + 0.25)[own].astype(dtype)
    return v


def integer_input(sp, rank):
    """every local entry, ghosts included: an integer below 2^20 made of rank and position -- any sum of 27 of them is exact"""
    return (1 + (rank * 104729 + 7 * np.arange(n_local(sp), dtype=np.int64)) % 1000003).astype(np.float64)


def decade_input(sp, rank, seed, ghosts=True):
    """seeded normal doubles spread over six decades; ghosts=False: NaN on every ghost entry"""
    rng = np.random.default_rng([seed, rank])
    v = rng.standard_normal(n_local(sp)) * 10.0 ** rng.uniform(-3, 3, n_local(sp))
    if not ghosts:
        v[~owned_mask(sp)] = np.nan
    return v


def forward(spaces, vectors, width=None):
    """the vectors of all ranks after one forward exchange (any dtype; untouched entries keep their bits)"""
    owner_map(spaces)
    held = owner_values(spaces, vectors)
    out = []
    for sp, v in zip(spaces, vectors):
        assert v.shape == (n_local(sp),)
        e = v.copy()
        sh = shell_mask(sp, width)
        e[sh] = held[global_ids(sp)[sh]]
        out.append(e)
    return out


Reverse = namedtuple("Reverse", "ref m mag")


def reverse(spaces, vectors, width=None):
    """per rank: ref = the vector after one reverse (adding) exchange in long double, m = additions into every entry,
    mag = sum of |addends| of every entry (the owner's own value included)"""
    ng = n_global(spaces[0])
    owner_map(spaces)
    acc, mag, cnt = np.zeros(ng, dtype=np.longdouble), np.zeros(ng, dtype=np.longdouble), np.zeros(ng, dtype=np.int64)
    for sp, v in zip(spaces, vectors):
        assert v.shape == (n_local(sp),)
        sh = shell_mask(sp, width)
        g, a = global_ids(sp)[sh], v[sh].astype(np.longdouble)
        np.add.at(acc, g, a)
        np.add.at(mag, g, np.abs(a))
        np.add.at(cnt, g, 1)
    out = []
    for sp, v in zip(spaces, vectors):
        own, g = owned_mask(sp), global_ids(sp)
        ref, m, mg = v.astype(np.longdouble), np.zeros(len(v), dtype=np.int64), np.abs(v).astype(np.longdouble)
        ref[own] += acc[g[own]]
        mg[own] += mag[g[own]]
        m[own] = cnt[g[own]]
        out.append(Reverse(ref, m, mg))
    return out


def owned_dot(spaces, xs, ys):
    """(long-double sum of x_i y_i over the owned entries of all ranks, sum of |x_i y_i|, owned entries of the largest rank)"""
    owner_map(spaces)
    total, mag, most = np.longdouble(0), np.longdouble(0), 0
    for sp, x, y in zip(spaces, xs, ys):
        own = owned_mask(sp)
        p = x[own].astype(np.longdouble) * y[own].astype(np.longdouble)
        total += p.sum()
        mag += np.abs(p).sum()
        most = max(most, int(own.sum()))
    return total, mag, most


def sent_doubles(spaces, width=None, reverse=False):
    """doubles every rank sends in one exchange"""
    owner = owner_map(spaces)
    sent = np.zeros(len(spaces), dtype=np.int64)
    for r, sp in enumerate(spaces):
        own_of_shell = owner[global_ids(sp)[shell_mask(sp, width)]]
        assert (own_of_shell != r).all() and (own_of_shell >= 0).all()
        if reverse:
            sent[r] += len(own_of_shell)
        else:
            sent += np.bincount(own_of_shell, minlength=len(spaces))
    return [int(v) for v in sent]


# ---- the checks -------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _where(sp, mask, limit=3):
    idx = np.flatnonzero(mask)
    return f"{len(idx)} entries, first {idx[:limit].tolist()} of dims {sp.dims} x {sp.comps}"


def check_forward(spaces, before, after, width=None):
    """exact: inside the dilated box the owner's value, everything else bit for bit what it was"""
    out = []
    for r, (sp, b, a, e) in enumerate(zip(spaces, before, after, forward(spaces, before, width))):
        if a.shape != b.shape or a.dtype != b.dtype:
            out.append(f"rank {r}: the vector changed its shape or type")
            continue
        wrong = _bits(a) != _bits(e)
        own, sh = owned_mask(sp), shell_mask(sp, width)
        if (wrong & own).any():
            out.append(f"rank {r}: owned entries changed: " + _where(sp, wrong & own))
        if (wrong & sh).any():
            out.append(f"rank {r}: ghost entries inside the dilated box do not hold the owner's value: " + _where(sp, wrong & sh))
        if (wrong & ~own & ~sh).any():
            out.append(f"rank {r}: entries outside the dilated box were written: " + _where(sp, wrong & ~own & ~sh))
    return out


def check_reverse(spaces, before, after, width=None, exact=True):
    """ghost entries bit for bit what they were; owned entries the restatement's sums -- exact: bit for bit (data whose sums are
    exact in any order), else within m 2^-53 sum |addends| of the long-double sum"""
    out = []
    for r, (sp, b, a, e) in enumerate(zip(spaces, before, after, reverse(spaces, before, width))):
        if a.shape != b.shape or a.dtype != np.float64:
            out.append(f"rank {r}: the vector changed its shape or type")
            continue
        own = owned_mask(sp)
        ghost_wrong = ~own & (_bits(a) != _bits(b))
        if ghost_wrong.any():
            out.append(f"rank {r}: the reverse exchange changed ghost entries: " + _where(sp, ghost_wrong))
        if exact:
            ref = e.ref.astype(np.float64)
            assert (ref.astype(np.longdouble)[own] == e.ref[own]).all(), "the data of the exact check does not sum exactly"
            bad = own & (_bits(a) != _bits(ref))
        else:
            with np.errstate(invalid="ignore"):
                err = np.abs(a.astype(np.longdouble) - e.ref)
                bad = own & ~(err <= e.m * np.longdouble(U) * e.mag)          # (a NaN fails)
            bad |= own & (e.m == 0) & (_bits(a) != _bits(b))                    # nothing added: not even rounded
        if bad.any():
            out.append(f"rank {r}: owned entries differ from the sum of their contributions: " + _where(sp, bad))
    return out


def dot_chain(n_owned_most, n_ranks):
    """k of the bound k 2^-53 sum |x_i y_i| of the owned dot product (the module docstring of tests/test_gpu_halo_exchange.py
    derives it): the rounding of the product, the trips of a thread's grid-stride run, 6 butterfly steps, 3 sums over the 4
    wavefronts of a block; the partials per thread of the second stage, 6 butterfly steps, 3 sums; ranks - 1 sums of the all-reduce"""
    blocks = min(max((n_owned_most + 255) // 256, 1), 1024)
    trips = (n_owned_most + blocks * 256 - 1) // (blocks * 256)
    return 1 + trips + 6 + 3 + (blocks + 255) // 256 + 6 + 3 + (n_ranks - 1)


def check_dot(spaces, xs, ys, results):
    """results: what every rank got -- the same bits everywhere, finite, within dot_chain() 2^-53 sum |x_i y_i| of the long-double sum"""
    out = []
    ref, mag, most = owned_dot(spaces, xs, ys)
    res = np.asarray(results, dtype=np.float64)
    if (_bits(res) != _bits(res)[0]).any():
        out.append(f"the ranks hold different sums: {res.tolist()}")
    k = dot_chain(most, len(spaces))
    for r, v in enumerate(res):
        if not np.isfinite(v):
            out.append(f"rank {r}: the sum is {v} (a ghost entry in the reduction?)")
        elif not abs(np.longdouble(v) - ref) <= k * np.longdouble(U) * mag:
            out.append(f"rank {r}: {v!r} is {float(abs(np.longdouble(v) - ref) / mag):.3e} sum|xy| from the long-double sum, bound {k} * 2^-53")
    return out
