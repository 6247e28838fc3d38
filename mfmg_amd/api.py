"""Thin Python mirror of the mfmg classes over the C ABI (include/mfmg_hip.h).

Vectors are torch CUDA tensors (float64, contiguous) -- torch only owns the memory;
the arithmetic happens in libmfmg_hip.so on the stream of the Context."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import lib as _lib
from .lib import MeshDesc, check


def params_to_info(params: dict, indent: int = 0) -> str:
    """dict -> boost::property_tree INFO text (tests/data/hierarchy_input.info)."""
    out = []
    pad = " " * indent
    for k, v in params.items():
        key = f'"{k}"' if (" " in str(k) or ":" in str(k)) else str(k)
        if isinstance(v, dict):
            out.append(f"{pad}{key}\n{pad}{{\n{params_to_info(v, indent + 2)}{pad}}}\n")
        else:
            if isinstance(v, bool):
                v = "true" if v else "false"
            elif isinstance(v, float):
                v = repr(v)
            sval = str(v)
            if " " in sval or sval == "":
                sval = f'"{sval}"'
            out.append(f"{pad}{key} {sval}\n")
    return "".join(out)


def info_to_params(text: str) -> dict:
    """boost::property_tree INFO text -> nested dict (the inverse of params_to_info; what
    boost::property_tree::info_parser::read_info does for tests/hierarchy_driver.cc:255-256): `key value`,
    `key { children }` with the brace on the same or the next line, "quoted strings", `;` comments.  Values stay
    strings except true / false, integers and floats."""
    import shlex

    def convert(v: str):
        if v == "true":
            return True
        if v == "false":
            return False
        for cast in (int, float):
            try:
                return cast(v)
            except ValueError:
                pass
        return v

    tokens = []
    for line in text.splitlines():
        lex = shlex.shlex(line, posix=True)
        lex.whitespace_split = True
        lex.commenters = ";"
        lex.quotes = '"'
        toks = list(lex)
        # braces glued to a word do not occur in the files of the reference; split the plain cases anyway
        for t in toks:
            tokens.append(("tok", t))
        tokens.append(("eol", None))

    def parse(pos):
        node = {}
        while pos < len(tokens):
            kind, t = tokens[pos]
            if kind == "eol":
                pos += 1
                continue
            if t == "}":
                return node, pos + 1
            key = t
            pos += 1
            value = None
            if pos < len(tokens) and tokens[pos][0] == "tok" and tokens[pos][1] not in ("{", "}"):
                value = tokens[pos][1]
                pos += 1
            q = pos
            while q < len(tokens) and tokens[q][0] == "eol":
                q += 1
            if q < len(tokens) and tokens[q] == ("tok", "{"):
                child, pos = parse(q + 1)
                node[key] = child
            else:
                node[key] = convert(value) if value is not None else ""
        return node, pos

    return parse(0)[0]


def _dev_ptr(t: torch.Tensor, n: Optional[int] = None, dtype=torch.float64) -> int:
    if not isinstance(t, torch.Tensor):
        raise TypeError("expected a torch tensor")
    if t.device.type != "cuda":
        raise ValueError("vectors must live on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"vectors must be contiguous {dtype} tensors")
    if n is not None and t.numel() != n:
        raise ValueError(f"vector has {t.numel()} entries, expected {n}")
    return t.data_ptr()


def _block_ptr(t: torch.Tensor, dtype=torch.float64):
    """(k, ld, device pointer) of a block of vectors: a 2-D float64 (or, for the FP32 entry points, float32) CUDA tensor of shape
    (k, m) whose rows are the vectors (stride(1) == 1, ld = stride(0)).  What the library asks of k, ld and the alignment it
    checks itself."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("expected a torch tensor")
    if t.device.type != "cuda":
        raise ValueError("vectors must live on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != dtype or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"a block is a 2-D {str(dtype).split('.')[-1]} tensor of shape (k, m) with stride(1) == 1")
    return int(t.shape[0]), int(t.stride(0)), t.data_ptr()


def _same_block(k, ld, t, dtype=torch.float64):
    kk, ll, p = _block_ptr(t, dtype)
    if (kk, ll) != (k, ld):
        raise ValueError("the blocks of one call share the number of vectors and the leading dimension")
    return p


def block_groups(n_vectors: int):
    """Widths of the launches a block of n_vectors (1 .. 64) is cut into: groups of 4, then one of 2, then one vector."""
    lib = _lib.load()
    w = (C.c_int32 * 18)()
    n = C.c_int32()
    check(lib.mfmg_hip_block_groups(int(n_vectors), w, C.byref(n)))
    return [int(w[i]) for i in range(n.value)]


def mf_z_tiles(n_layers: int, tz: int, graded: bool = True):
    """The z-tiling of the matrix-free operator for n_layers DoF layers and the tile height tz: the tile starts followed by
    n_layers, so z-tile t owns the layers [tab[t], tab[t + 1]).  graded: what a whole-mesh launch of the one-term operator and
    every launch of the block operator read (graded where every eighth of the layers holds enough of them, uniform elsewhere);
    otherwise the uniform table of a region launch.  Host only."""
    lib = _lib.load()
    n_layers, tz = int(n_layers), int(tz)
    capacity = max(n_layers, 0) + 1
    starts = (C.c_int32 * capacity)()
    n = C.c_int32()
    check(lib.mfmg_hip_mf_z_tiles(n_layers, tz, int(bool(graded)), starts, capacity, C.byref(n)))
    return list(starts[:n.value + 1])


def block_cg_retire(retire_flags, slot_col):
    """The slot moves of solve_cg_block when the slots flagged in retire_flags (one per active slot) retire: returns
    (moves, slot_col, n_active) -- moves a list of (from, to) pairs, slot_col the updated slot -> column map (its first n_active
    entries are the survivors').  Host only."""
    lib = _lib.load()
    n = len(retire_flags)
    if len(slot_col) != n:
        raise ValueError("one slot_col entry per active slot")
    arr = C.c_int32 * max(n, 1)
    flags, cols, moves = arr(*[int(bool(f)) for f in retire_flags]), arr(*[int(c) for c in slot_col]), (C.c_int32 * (2 * max(n, 1)))()
    n_moves, n_out = C.c_int32(), C.c_int32()
    check(lib.mfmg_hip_block_cg_retire(n, flags, cols, moves, C.byref(n_moves), C.byref(n_out)))
    return [(int(moves[2 * i]), int(moves[2 * i + 1])) for i in range(n_moves.value)], [int(cols[i]) for i in range(n)], n_out.value


def block_fgmres_plan(live, slot_col):
    """The plan of one step of solve_fgmres_block for slots with the flags `live` and the slot -> column map `slot_col`: returns
    (runs, packed) -- runs a list of (start, width, group widths) for every maximal run of consecutive live slots, packed the
    columns of the live slots in slot order (the map of the next restart cycle).  Host only."""
    lib = _lib.load()
    n = len(live)
    if len(slot_col) != n:
        raise ValueError("one slot_col entry per slot")
    arr = C.c_int32 * max(n, 1)
    flags, cols = arr(*[int(bool(f)) for f in live]), arr(*[int(c) for c in slot_col])
    start, width, groups, gw, packed = arr(), arr(), arr(), arr(), arr()
    n_runs, n_groups, n_packed = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.mfmg_hip_block_fgmres_plan(n, flags, cols, start, width, groups, C.byref(n_runs), gw, C.byref(n_groups), packed,
                                         C.byref(n_packed)))
    runs, g0 = [], 0
    for r in range(n_runs.value):
        runs.append((int(start[r]), int(width[r]), [int(gw[g0 + g]) for g in range(groups[r])]))
        g0 += groups[r]
    assert g0 == n_groups.value
    return runs, [int(packed[i]) for i in range(n_packed.value)]


def memory_inventory() -> str:
    """Live bytes of the library's device buffers per (setup section | kind of structure), as text."""
    lib = _lib.load()
    buf = C.create_string_buffer(1 << 16)
    check(lib.mfmg_hip_memory_inventory(buf, len(buf)))
    return buf.value.decode()


class Context:
    """CudaHandle twin: a HIP stream + scratch (source/cuda/cuda_handle.cu:17-56)."""

    def __init__(self, stream: Optional[int] = None, own_stream: bool = False):
        """By default the context runs on torch's current stream, so that tensor operations issued
        through torch and the library's kernels are ordered; `own_stream` asks the library for a
        private non-blocking stream (the caller then synchronises explicitly)."""
        self._lib = _lib.load()
        h = C.c_void_p()
        if own_stream:
            arg = C.c_void_p(-1)
        else:
            if stream is None and torch.cuda.is_available():
                stream = torch.cuda.current_stream().cuda_stream
            arg = C.c_void_p(stream) if stream else None
        check(self._lib.mfmg_hip_context_create(arg, C.byref(h)))
        self.handle = h

    def synchronize(self):
        check(self._lib.mfmg_hip_context_synchronize(self.handle))

    @property
    def stream(self) -> int:
        return self._lib.mfmg_hip_context_stream(self.handle)

    def torch_stream(self) -> "torch.cuda.ExternalStream":
        return torch.cuda.ExternalStream(self.stream)

    def set_cell_constant_layout(self, enable: bool):
        """Operators created afterwards keep one coefficient per cell when a cell's eight are equal (default on)."""
        check(self._lib.mfmg_hip_context_set_cell_constant_layout(self.handle, int(bool(enable))))

    def set_stored_diagonal(self, enable: bool):
        """Cell-constant operators created afterwards keep D^-1 in their chunk records (default: derived in the kernel)."""
        check(self._lib.mfmg_hip_context_set_stored_diagonal(self.handle, int(bool(enable))))

    def set_mf_fused_terms(self, n_terms: int):
        """Matrix-free operators created afterwards can run up to n_terms (1..3) smoother terms per sweep (default 3)."""
        check(self._lib.mfmg_hip_context_set_mf_fused_terms(self.handle, int(n_terms)))

    def set_mf_shell(self, mode):
        """Distributed fine operator: the shell of tiles 'beside' (default) / 'after' the interior tiles, or as 'slabs'."""
        check(self._lib.mfmg_hip_context_set_mf_shell(self.handle, {"beside": 0, "": 0, "after": 1, "slabs": 2}[mode]))

    def set_mf_emulate_split(self, axes):
        """One rank, measurement only: the launches of a rank with neighbours along 'z', 'yz' or 'xyz' ('' / None: off)."""
        check(self._lib.mfmg_hip_context_set_mf_emulate_split(self.handle, {None: 0, "": 0, "z": 1, "yz": 2, "xyz": 3, "1": 3}[axes]))

    def set_galerkin_on_device(self, enable: bool):
        """Hierarchies created afterwards form R A R^T of a matrix-free A by probing on the device (default) or on the host."""
        check(self._lib.mfmg_hip_context_set_galerkin_on_device(self.handle, int(bool(enable))))

    def set_overlap_exchange(self, enable: bool):
        """Distributed runs: overlap the fine-level halo exchange with interior operator tiles (default on)."""
        check(self._lib.mfmg_hip_context_set_overlap_exchange(self.handle, int(bool(enable))))

    def profile_enable(self, enabled: bool = True, only: str = ""):
        """HIP-event timing per kernel name; `only` restricts it to one name (every timed launch costs two
        event records on the stream)."""
        check(self._lib.mfmg_hip_profile_select(self.handle, only.encode() if only else None))
        check(self._lib.mfmg_hip_profile_enable(self.handle, 1 if enabled else 0))

    def profile_query(self, kernel: str):
        """(launches, total milliseconds, summed algorithmic bytes) of one kernel since profile_enable."""
        n, ms, by = C.c_int64(), C.c_double(), C.c_double()
        check(self._lib.mfmg_hip_profile_query(self.handle, kernel.encode(), C.byref(n), C.byref(ms), C.byref(by)))
        return n.value, ms.value, by.value

    def dot(self, x: torch.Tensor, y: torch.Tensor) -> float:
        r = C.c_double()
        check(self._lib.mfmg_hip_vector_dot(self.handle, x.numel(), _dev_ptr(x), _dev_ptr(y), C.byref(r)))
        return r.value

    def l2_norm(self, x: torch.Tensor) -> float:
        r = C.c_double()
        check(self._lib.mfmg_hip_vector_l2_norm(self.handle, x.numel(), _dev_ptr(x), C.byref(r)))
        return r.value

    def set(self, x: torch.Tensor, value: float):
        check(self._lib.mfmg_hip_vector_set(self.handle, x.numel(), value, _dev_ptr(x)))

    def add(self, x: torch.Tensor, a: float, v: torch.Tensor):
        check(self._lib.mfmg_hip_vector_add(self.handle, x.numel(), a, _dev_ptr(v, x.numel()), _dev_ptr(x)))

    def sadd(self, x: torch.Tensor, s: float, a: float, v: torch.Tensor):
        check(self._lib.mfmg_hip_vector_sadd(self.handle, x.numel(), s, a, _dev_ptr(v, x.numel()), _dev_ptr(x)))

    def exchange_f32(self, space: int, v: torch.Tensor, width: int = 1):
        """One forward halo exchange (owner -> ghost) of a float32 vector of the fine DoF space (space 1), `width` planes deep;
        the FP32 fine level does this by itself (for tests).  Nothing happens without a HaloTransport."""
        assert v.dtype == torch.float32 and v.is_contiguous()
        check(self._lib.mfmg_hip_context_exchange_f32(self.handle, int(space), v.data_ptr(), int(width)))

    def exchange_block(self, space: int, V: torch.Tensor, width: int = 1):
        """One forward halo exchange (owner -> ghost) of every row of the block V -- a 2-D float64 tensor of shape (k, m),
        stride(1) == 1, ld = stride(0) even and at least the local vector's size, the base aligned to 16 bytes -- in the fine DoF
        space (space 1), `width` planes deep: one packing launch, one grouped send/recv with one message per neighbour (the
        one-vector messages of the rows one after the other), one unpacking launch; counted as one exchange.  Every row gets the
        bits of HaloTransport.exchange of that row.  Nothing happens without a HaloTransport."""
        k, ld, pv = _block_ptr(V)
        check(self._lib.mfmg_hip_context_exchange_block(self.handle, int(space), k, ld, pv, int(width)))

    def set_block_fgmres_on_ranks(self, enable: bool = True):
        """Lets Hierarchy.solve_fgmres_block run on this context when it has a HaloTransport; without it the call is refused
        there, as it always was.  The solve is collective: every rank enables it on its context before the solve."""
        check(self._lib.mfmg_hip_context_set_block_fgmres_on_ranks(self.handle, 1 if enable else 0))

    def exchange_block_f32(self, space: int, V: torch.Tensor, width: int = 1):
        """exchange_block for the rows of a float32 block (ld = stride(0) even, the base aligned to 8 bytes): one packing launch
        that widens into the staging of the FP64 block exchange, one grouped send/recv, one unpacking launch that narrows; the
        messages and counters of exchange_block.  Every row gets the bits of exchange_f32 of that row.  Nothing happens without
        a HaloTransport."""
        k, ld, pv = _block_ptr(V, torch.float32)
        check(self._lib.mfmg_hip_context_exchange_block_f32(self.handle, int(space), k, ld, pv, int(width)))

    def block_dots_box(self, box, X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        """out[s] = the part of (X[s], Y[s]) over the owned entries of a rank's local vectors, box = (local_nodes, own0, own_n,
        comps) as for krylov_orthogonalize: the reduction of solve_cg_block on several ranks, on a context WITHOUT a communicator.
        Per row the bits of the rank-local sum of HaloTransport.owned_dot; the ghost entries never enter it.  A device tensor."""
        local_nodes, own0, own_n, comps = box
        k, ld, px = _block_ptr(X)
        i3 = C.c_int64 * 3
        out = torch.empty(k, dtype=torch.float64, device=X.device)
        check(self._lib.mfmg_hip_block_dots_box(self.handle, i3(*local_nodes), i3(*own0), i3(*own_n), int(comps), k, ld, px,
                                                _same_block(k, ld, Y), _dev_ptr(out)))
        return out

    def krylov_orthogonalize(self, V: torch.Tensor, w: torch.Tensor, n_columns: int, passes: int = 2, box=None):
        """The fused Gram-Schmidt kernels of solve_fgmres on their own: `passes` times { c = V^T w; w -= V c } in place, against
        the first n_columns columns of V ([columns, ld] contiguous: column-major with leading dimension ld >= len(w)).
        Returns (h, norm): device tensors with the summed coefficients and ||w|| of the result.
        box = (local_nodes, own0, own_n, comps): the vectors are a rank's local ones -- the lexicographic box of local_nodes
        (x, y, z) nodes with comps entries each -- and everything runs over the owned nodes [own0, own0 + own_n) alone (the
        kernels of a distributed solve_fgmres; ghost entries are neither used nor written)."""
        n, ld = w.numel(), V.shape[1]
        assert 1 <= n_columns <= V.shape[0] and ld >= n
        h = torch.empty(n_columns, dtype=torch.float64, device=w.device)
        norm = torch.empty(1, dtype=torch.float64, device=w.device)
        if box is not None:
            local_nodes, own0, own_n, comps = box
            i3 = C.c_int64 * 3
            assert n == comps * local_nodes[0] * local_nodes[1] * local_nodes[2]
            check(self._lib.mfmg_hip_krylov_orthogonalize_box(self.handle, i3(*local_nodes), i3(*own0), i3(*own_n), comps, ld,
                                                              n_columns - 1, _dev_ptr(V), _dev_ptr(w), _dev_ptr(h), _dev_ptr(norm),
                                                              passes))
            return h, norm
        check(self._lib.mfmg_hip_krylov_orthogonalize(self.handle, n, ld, n_columns - 1, _dev_ptr(V), _dev_ptr(w), _dev_ptr(h),
                                                      _dev_ptr(norm), passes))
        return h, norm

    # The vector kernels of Hierarchy.solve_cg_block on their own (tests).  Blocks are 2-D float64 CUDA tensors of shape (k, ld)
    # with stride(1) == 1; n entries of every row are used; scalars are float64 device tensors of k entries.
    def block_dots(self, n: int, X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        """out[s] = (X[s, :n], Y[s, :n]) with the reduction of dot(), bit for bit; a device tensor."""
        k, ld, px = _block_ptr(X)
        out = torch.empty(k, dtype=torch.float64, device=X.device)
        check(self._lib.mfmg_hip_block_dots(self.handle, int(n), k, ld, px, _same_block(k, ld, Y), _dev_ptr(out)))
        return out

    def block_cg_direction(self, n: int, Z: torch.Tensor, P: torch.Tensor, rz_new=None, rz_old=None):
        """P[s] = Z[s] + (rz_new[s] / rz_old[s]) P[s] (a zero divisor: beta = 0); rz_old None: P[s] = Z[s]."""
        k, ld, pz = _block_ptr(Z)
        s = lambda t: None if t is None else _dev_ptr(t, k)
        check(self._lib.mfmg_hip_block_cg_direction(self.handle, int(n), k, ld, pz, _same_block(k, ld, P), s(rz_new), s(rz_old)))

    def block_cg_update(self, n: int, P: torch.Tensor, AP: torch.Tensor, R: torch.Tensor, X: torch.Tensor, slot_col: torch.Tensor,
                        rz: torch.Tensor, pap: torch.Tensor) -> torch.Tensor:
        """alpha = rz[s] / pap[s] (zero divisor: 0); X[slot_col[s]] += alpha P[s]; R[s] -= alpha AP[s]; returns (R[s], R[s]) of the
        new R with the bits of block_dots.  X is a block of its own shape and leading dimension; slot_col an int32 device tensor
        naming every column of X at most once."""
        k, ld, pp = _block_ptr(P)
        kx, ldx, px = _block_ptr(X)
        cols = slot_col.cpu().tolist()
        if len(cols) != k or len(set(cols)) != k or min(cols) < 0 or max(cols) >= kx or ldx < n:
            raise ValueError("slot_col names k different columns of X")
        out = torch.empty(k, dtype=torch.float64, device=P.device)
        check(self._lib.mfmg_hip_block_cg_update(self.handle, int(n), k, ld, pp, _same_block(k, ld, AP), _same_block(k, ld, R), ldx, px,
                                                 _dev_ptr(slot_col, k, torch.int32), _dev_ptr(rz, k), _dev_ptr(pap, k), _dev_ptr(out)))
        return out

    def krylov_combine(self, Z: torch.Tensor, y: torch.Tensor, x: torch.Tensor):
        """x += sum_i y[i] Z[i] in one pass (Z: [columns, ld] contiguous, ld >= len(x); y on the device)."""
        n, ld = x.numel(), Z.shape[1]
        assert 1 <= y.numel() <= Z.shape[0] and ld >= n
        check(self._lib.mfmg_hip_krylov_combine(self.handle, n, ld, y.numel() - 1, _dev_ptr(Z), _dev_ptr(y), _dev_ptr(x)))

    # The basis kernels of Hierarchy.solve_fgmres_block on their own (tests).  A basis block is a contiguous 3-D float64 CUDA tensor
    # of shape (vectors, k, ld): vector i of slot s is V[i, s, :n]; ld even, the base aligned to 16 bytes.  `live` names the slots
    # the launches work on, in ascending order; the others are neither read nor written.
    @staticmethod
    def _basis_block(V: torch.Tensor):
        if not isinstance(V, torch.Tensor) or V.device.type != "cuda" or V.dtype != torch.float64 or V.dim() != 3 or not V.is_contiguous():
            raise ValueError("a basis block is a contiguous 3-D float64 CUDA tensor of shape (vectors, k, ld)")
        return int(V.shape[0]), int(V.shape[1]), int(V.shape[2]), V.data_ptr()

    def block_krylov_orthogonalize(self, n: int, V: torch.Tensor, j: int, live, v_next=None, v_next_f32=None):
        """w_s = V[j + 1, s] is orthogonalised in place against V[0 .. j, s] for every live slot s (classical Gram-Schmidt twice,
        one launch per pass for all of them).  Returns (h, norm): device tensors (k, j + 1) and (k,) with the summed coefficients
        and ||w_s||, NaN where a slot is not live.  v_next (k, ld) float64 receives w_s / ||w_s|| (zeros for a zero norm),
        v_next_f32 (k, ld) float32 its narrowed copy.  Per slot the bits of krylov_orthogonalize."""
        nv, k, ld, pv = self._basis_block(V)
        if not 0 <= j < nv - 1:
            raise ValueError("the block holds no vector j + 1")
        for t, dt in ((v_next, torch.float64), (v_next_f32, torch.float32)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != (k, ld) or not t.is_contiguous() or t.device != V.device):
                raise ValueError("v_next and v_next_f32 are contiguous (k, ld) tensors on the device of V")
        h = torch.full((k, j + 1), float("nan"), dtype=torch.float64, device=V.device)
        norm = torch.full((k,), float("nan"), dtype=torch.float64, device=V.device)
        slots = (C.c_int32 * max(len(live), 1))(*[int(s) for s in live])
        ptr = lambda t: None if t is None else t.data_ptr()
        check(self._lib.mfmg_hip_block_krylov_orthogonalize(self.handle, int(n), k, ld, int(j), len(live), slots, pv, ptr(v_next),
                                                            ptr(v_next_f32), h.data_ptr(), norm.data_ptr()))
        return h, norm

    def block_krylov_orthogonalize_box(self, box, V: torch.Tensor, j: int, live, v_next=None):
        """block_krylov_orthogonalize over the owned entries of a rank's local vectors, box = (local_nodes, own0, own_n, comps) as
        for krylov_orthogonalize: the kernels of solve_fgmres_block on several ranks, on a context WITHOUT a communicator (the sum
        over the ranks is the identity).  Returns (h, norm) as block_krylov_orthogonalize; v_next (k, ld) float64 receives the
        owned entries of w_s / ||w_s||.  Per live slot the bits of krylov_orthogonalize(..., box=box); ghost entries, the padding
        between the rows and the slots that are not live are neither used nor written."""
        nv, k, ld, pv = self._basis_block(V)
        local_nodes, own0, own_n, comps = box
        if not 0 <= j < nv - 1:
            raise ValueError("the block holds no vector j + 1")
        if ld < comps * local_nodes[0] * local_nodes[1] * local_nodes[2]:
            raise ValueError("the leading dimension is smaller than the local vectors of the box")
        if v_next is not None and (v_next.dtype != torch.float64 or tuple(v_next.shape) != (k, ld) or not v_next.is_contiguous()
                                   or v_next.device != V.device):
            raise ValueError("v_next is a contiguous (k, ld) float64 tensor on the device of V")
        h = torch.full((k, j + 1), float("nan"), dtype=torch.float64, device=V.device)
        norm = torch.full((k,), float("nan"), dtype=torch.float64, device=V.device)
        slots = (C.c_int32 * max(len(live), 1))(*[int(s) for s in live])
        i3 = C.c_int64 * 3
        check(self._lib.mfmg_hip_block_krylov_orthogonalize_box(self.handle, i3(*local_nodes), i3(*own0), i3(*own_n), int(comps), k, ld,
                                                                int(j), len(live), slots, pv,
                                                                None if v_next is None else v_next.data_ptr(), h.data_ptr(),
                                                                norm.data_ptr()))
        return h, norm

    def block_krylov_combine(self, n: int, Z: torch.Tensor, y: torch.Tensor, live, slot_col, X: torch.Tensor):
        """X[slot_col[s], :n] += sum_i y[s, i] Z[i, s, :n] for every live slot s in one launch (y: (k, columns) float64 on the
        device; X a block of its own shape and leading dimension, aligned to 8 bytes).  Per slot the bits of krylov_combine."""
        nv, k, ld, pz = self._basis_block(Z)
        kx, ldx, px = _block_ptr(X)
        if y.dim() != 2 or y.shape[0] != k or not 1 <= y.shape[1] <= nv or len(slot_col) != k:
            raise ValueError("y holds one row of at most as many coefficients as Z has vectors per slot, slot_col one entry per slot")
        slots = (C.c_int32 * max(len(live), 1))(*[int(s) for s in live])
        cols = (C.c_int32 * k)(*[int(c) for c in slot_col])
        check(self._lib.mfmg_hip_block_krylov_combine(self.handle, int(n), k, ld, int(y.shape[1]) - 1, len(live), slots, cols, pz,
                                                      _dev_ptr(y, k * int(y.shape[1])), kx, ldx, px))

    def cell_contraction(self, u: torch.Tensor, c: torch.Tensor, v: torch.Tensor, cell_size, variant: str = "mfma"):
        """v[m, cell] = c[cell] * sum_k K_ref[m, k] u[k, cell] (BASELINE.json configs[4]); u, v: [8, n] contiguous CUDA
        tensors, float32 or float64; variant "valu" or "mfma"."""
        n = c.numel()
        dt = u.dtype
        assert dt in (torch.float32, torch.float64) and u.shape == (8, n) and v.shape == (8, n)
        hs = (C.c_double * 3)(*[float(x) for x in cell_size])
        check(self._lib.mfmg_hip_cell_contraction(self.handle, 1 if dt == torch.float32 else 0, 1 if variant == "mfma" else 0, n,
                                                  _dev_ptr(u, 8 * n, dt), _dev_ptr(c, n, dt), _dev_ptr(v, 8 * n, dt), hs))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.mfmg_hip_context_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def _csr_arrays(a):
    """scipy.sparse matrix (or (row_ptr, col, val, shape)) -> int32/int32/float64 numpy arrays."""
    if hasattr(a, "tocsr"):
        a = a.tocsr()
        a.sort_indices()
        return (np.ascontiguousarray(a.indptr, dtype=np.int32), np.ascontiguousarray(a.indices, dtype=np.int32),
                np.ascontiguousarray(a.data, dtype=np.float64), a.shape)
    rp, cl, vl, shape = a
    return (np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(cl, dtype=np.int32),
            np.ascontiguousarray(vl, dtype=np.float64), shape)


def block_csr_info_f32(ctx, matrix) -> dict:
    """What SparseMatrixDevice.set_block_csr(True) reports on the FP32 instance of the matrix class (the values narrowed): the
    block forms of the CSR kernels are FP64 only -- width 1, no route."""
    rp, cl, vl, shape = _csr_arrays(matrix)
    f = (C.c_int32 * 3)()
    check(_lib.load().mfmg_hip_csr_block_csr_info_f32(ctx.handle, shape[0], shape[1], len(vl), rp.ctypes.data, cl.ctypes.data,
                                                       vl.ctypes.data, f))
    return {"width": int(f[0]), "route4": SparseMatrixDevice._CSR_KERNELS[int(f[1])], "route2": SparseMatrixDevice._CSR_KERNELS[int(f[2])]}


class SparseMatrixDevice:
    """SparseMatrixDevice<double> + CudaMatrixOperator (include/mfmg/cuda/sparse_matrix_device.cuh,
    source/cuda/cuda_matrix_operator.cu)."""

    def __init__(self, ctx: Context, matrix=None, _handle=None, _borrowed=False, _keepalive=None):
        self._lib = _lib.load()
        self.ctx = ctx
        self._borrowed = _borrowed
        self._keepalive = _keepalive
        if _handle is not None:
            self.handle = _handle
        else:
            rp, cl, vl, shape = _csr_arrays(matrix)
            h = C.c_void_p()
            check(self._lib.mfmg_hip_csr_create(ctx.handle, shape[0], shape[1], len(vl), rp.ctypes.data,
                                                cl.ctypes.data, vl.ctypes.data, C.byref(h)))
            self.handle = h

    @property
    def shape(self):
        m, n, z = C.c_int64(), C.c_int64(), C.c_int64()
        check(self._lib.mfmg_hip_csr_shape(self.handle, C.byref(m), C.byref(n), C.byref(z)))
        return (m.value, n.value)

    @property
    def nnz(self):
        z = C.c_int64()
        check(self._lib.mfmg_hip_csr_shape(self.handle, None, None, C.byref(z)))
        return z.value

    def set_kernel(self, lanes_per_row: int = 0, use_lds: int = -1):
        check(self._lib.mfmg_hip_csr_set_kernel(self.handle, lanes_per_row, use_lds))

    def regular_rows(self) -> bool:
        v = C.c_int()
        check(self._lib.mfmg_hip_csr_regular_rows(self.handle, C.byref(v)))
        return bool(v.value)

    def stencil_classes(self):
        """(classes of non-regular nodes sharing a stencil, rows left to the stored values)."""
        k, r = C.c_int(), C.c_int64()
        check(self._lib.mfmg_hip_csr_stencil_classes(self.handle, C.byref(k), C.byref(r)))
        return k.value, r.value

    def solve(self, params, b, x):
        """CudaSolver(handle, op, params)->apply(b, x): the coarse solver `solver.type` names, built for this matrix,
        applied once from a zero guess."""
        info = params if isinstance(params, str) else params_to_info(params)
        n = self.shape[0]
        check(self._lib.mfmg_hip_csr_solve(self.handle, info.encode(), _dev_ptr(b, n), _dev_ptr(x, n)))

    def float_storage(self) -> bool:
        """The values the kernels read are kept in float (all representable in it: lossless)."""
        v = C.c_int()
        check(self._lib.mfmg_hip_csr_float_storage(self.handle, C.byref(v)))
        return bool(v.value)

    def set_regular_rows(self, enable: bool):
        check(self._lib.mfmg_hip_csr_set_regular_rows(self.handle, int(bool(enable))))

    def enable_node_twins(self) -> bool:
        """Two row nodes (n, n + 1) per lane for a node-class matrix whose neighbouring nodes share their base (what the
        aggregation setup does to its smoothed prolongators); False where the matrix declined (`MFMG_NODE_TWINS=0`, fewer
        than 90 % twins, not FP64 with 1 or 2 unknowns per node)."""
        v = C.c_int()
        check(self._lib.mfmg_hip_csr_enable_node_twins(self.handle, C.byref(v)))
        return bool(v.value)

    def release_csr(self) -> bool:
        """Free the CSR arrays of a table-driven matrix ("release setup matrices"); False where the kernels read them."""
        v = C.c_int()
        check(self._lib.mfmg_hip_csr_release_csr(self.handle, C.byref(v)))
        return bool(v.value)

    def get_kernel(self):
        a, b = C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_csr_get_kernel(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def vmult(self, dst: torch.Tensor, src: torch.Tensor):
        m, n = self.shape
        check(self._lib.mfmg_hip_csr_vmult(self.handle, _dev_ptr(src, n), _dev_ptr(dst, m)))

    def apply(self, x: torch.Tensor, y: torch.Tensor, mode: int = _lib.NO_TRANS):
        m, n = self.shape
        nx, ny = (n, m) if mode == _lib.NO_TRANS else (m, n)
        check(self._lib.mfmg_hip_csr_apply(self.handle, _dev_ptr(x, nx), _dev_ptr(y, ny), mode))

    def transpose(self) -> "SparseMatrixDevice":
        h = C.c_void_p()
        check(self._lib.mfmg_hip_csr_transpose(self.handle, C.byref(h)))
        return SparseMatrixDevice(self.ctx, _handle=h)

    def multiply(self, b: "SparseMatrixDevice") -> "SparseMatrixDevice":
        h = C.c_void_p()
        check(self._lib.mfmg_hip_csr_multiply(self.handle, b.handle, C.byref(h)))
        return SparseMatrixDevice(self.ctx, _handle=h)

    def inverse_diagonal(self, dinv: torch.Tensor):
        check(self._lib.mfmg_hip_csr_inverse_diagonal(self.handle, _dev_ptr(dinv, self.shape[0])))

    def residual(self, x, b, res):
        m, n = self.shape
        check(self._lib.mfmg_hip_csr_residual(self.handle, _dev_ptr(x, n), _dev_ptr(b, m), _dev_ptr(res, m)))

    def smoother_step(self, dinv, b, x, x_prev, alpha, beta, out):
        n = self.shape[0]
        check(self._lib.mfmg_hip_csr_smoother_step(self.handle, _dev_ptr(dinv, n), _dev_ptr(b, n), _dev_ptr(x, n),
                                                   _dev_ptr(x_prev, n) if x_prev is not None else None,
                                                   alpha, beta, _dev_ptr(out, n)))

    def launch(self, mode: int, x, out, b=None, dinv=None, x_prev=None, alpha: float = 0.0, beta: float = 0.0):
        """One SpMV with the fused epilogue `mode` (lib.CSR_APPLY .. lib.CSR_PLUS_SCALED); operands a mode does not
        read may stay None."""
        m, n = self.shape
        opt = lambda t: _dev_ptr(t, m) if t is not None else None
        check(self._lib.mfmg_hip_csr_launch(self.handle, mode, _dev_ptr(x, n), opt(b), opt(dinv), opt(x_prev), alpha,
                                            beta, _dev_ptr(out, m)))

    def launch_block(self, mode: int, X, out, B=None, dinv=None, X_prev=None, alpha: float = 0.0, beta: float = 0.0):
        """launch() on every row of the blocks X and out (2-D float64 tensors of shape (k, m), stride(1) == 1; each leading
        dimension stride(0) even and at least the size of its vectors, the bases aligned to 16 bytes): row c of out gets the
        bits of launch(mode, X[c], out[c], B[c], dinv, X_prev[c], ...).  B and X_prev share the leading dimension of out; dinv
        is one vector.  Where block_info()["width"] is 4 the stored values are read once per group of 4 or 2 rows."""
        m, n = self.shape
        k, ld_x, px = _block_ptr(X)
        ko, ld_out, po = _block_ptr(out)
        if ko != k:
            raise ValueError("the blocks of one call share the number of vectors")
        opt = lambda t: _same_block(k, ld_out, t) if t is not None else None
        check(self._lib.mfmg_hip_csr_launch_block(self.handle, mode, k, ld_x, px, ld_out, opt(B),
                                                  _dev_ptr(dinv, m) if dinv is not None else None, opt(X_prev), alpha, beta, po))

    def block_info(self) -> dict:
        """width: rows of the widest group launch_block runs as one launch (4: stored values that do not repeat; 1: the loop
        over the rows); block_launches / column_launches: launches of the block kernels, and rows that went through the
        one-vector kernels, of all launch_block calls on this matrix so far."""
        f = (C.c_int64 * 3)()
        check(self._lib.mfmg_hip_csr_block_info(self.handle, f))
        return {"width": int(f[0]), "block_launches": int(f[1]), "column_launches": int(f[2])}

    def set_block_csr(self, on: bool = True) -> dict:
        """Turn the block forms of the CSR kernels on (or off again) for this matrix: where form() names a CSR kernel, the
        matrix is FP64 and its CSR arrays are there, block_info()["width"] becomes 4 and launch_block reads val and col once per
        group of 4 or 2 rows, every row with the bits of launch().  Off by default.  Returns width, and route4 / route2: the
        kernel a group of 4 / of 2 takes (None, "lanes", "row_block", "lds"; an LDS-cached matrix whose windows do not fit
        next to each other takes "lanes")."""
        f = (C.c_int32 * 3)()
        check(self._lib.mfmg_hip_csr_set_block_csr(self.handle, 1 if on else 0, f))
        return {"width": int(f[0]), "route4": self._CSR_KERNELS[int(f[1])], "route2": self._CSR_KERNELS[int(f[2])]}

    _FORM_FIELDS = ("kind", "csr_kernel", "lanes", "c", "stored_d", "full_d", "symmetric_half", "float_planes", "regular",
                    "all_in_classes", "classes", "class_slots", "listed", "listed_route", "regular_kernel", "class_kernel",
                    "stored_kernel", "row_base_slots", "node_class_c", "node_class_d", "pairs", "csr_released",
                    "twin_kernel", "twin_slots", "twin_classes", "single_slots", "twin_wide")
    _CSR_KERNELS = {0: None, 1: "lanes", 2: "row_block", 3: "lds"}
    _LISTED_ROUTES = {0: None, 1: "class_tail", 2: "split_tail", 3: "own_launch", 4: "stored_planes"}
    _STORED_KERNELS = {0: None, 1: "rows", 2: "sym_rows", 3: "sym_split"}

    def form(self) -> dict:
        """Which kernels an application launches as the matrix stands (the record the launch branches on)."""
        f = (C.c_int64 * _lib.CSR_FORM_FIELDS)()
        check(self._lib.mfmg_hip_csr_form(self.handle, f, _lib.CSR_FORM_FIELDS))
        d = {k: int(f[i]) for i, k in enumerate(self._FORM_FIELDS)}
        d["csr_kernel"] = self._CSR_KERNELS[d["csr_kernel"]]
        d["listed_route"] = self._LISTED_ROUTES[d["listed_route"]]
        d["stored_kernel"] = self._STORED_KERNELS[d["stored_kernel"]]
        return d

    def to_scipy(self):
        import scipy.sparse as sp
        m, n = self.shape
        nnz = self.nnz
        rp = np.empty(m + 1, dtype=np.int32)
        cl = np.empty(nnz, dtype=np.int32)
        vl = np.empty(nnz, dtype=np.float64)
        check(self._lib.mfmg_hip_csr_download(self.handle, rp.ctypes.data, cl.ctypes.data, vl.ctypes.data))
        return sp.csr_matrix((vl, cl, rp), shape=(m, n))

    def __del__(self):
        try:
            if getattr(self, "handle", None) and not self._borrowed:
                self._lib.mfmg_hip_csr_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class MatrixFreeLaplace:
    """CudaMatrixFreeOperator + LaplaceOperator (source/cuda/cuda_matrix_free_operator.cu,
    tests/laplace_matrix_free.hpp:121-156) on the GPU."""

    def __init__(self, ctx: Context, problem):
        self._lib = _lib.load()
        self.ctx = ctx
        self.problem = problem  # keeps the mesh arrays alive during construction
        desc = problem.mesh_desc()
        h = C.c_void_p()
        check(self._lib.mfmg_hip_mf_laplace_create(ctx.handle, C.byref(desc), C.byref(h)))
        self.handle = h
        self.n_dofs = problem.n_dofs

    def vmult(self, dst: torch.Tensor, src: torch.Tensor):
        check(self._lib.mfmg_hip_mf_laplace_vmult(self.handle, _dev_ptr(src, self.n_dofs), _dev_ptr(dst, self.n_dofs)))

    def residual(self, x, b, res):
        n = self.n_dofs
        check(self._lib.mfmg_hip_mf_laplace_residual(self.handle, _dev_ptr(x, n), _dev_ptr(b, n), _dev_ptr(res, n)))

    def smoother_step(self, b, x, x_prev, alpha, beta, out):
        n = self.n_dofs
        check(self._lib.mfmg_hip_mf_laplace_smoother_step(self.handle, _dev_ptr(b, n), _dev_ptr(x, n),
                                                          _dev_ptr(x_prev, n) if x_prev is not None else None,
                                                          alpha, beta, _dev_ptr(out, n)))

    def sweep_available(self, n_terms: int) -> bool:
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_sweep_available(self.handle, int(n_terms), C.byref(v)))
        return bool(v.value)

    def smoother_sweep(self, alpha, beta, b, x, out, out_prev=None):
        """len(alpha) smoother terms in one sweep; out = the last iterate, out_prev (optional) the one before.
        x = None: from the zero vector, which is not read (three terms, the default arithmetic; raises where unavailable)."""
        n, k = self.n_dofs, len(alpha)
        a = (C.c_double * k)(*[float(v) for v in alpha])
        be = (C.c_double * k)(*[float(v) for v in beta])
        check(self._lib.mfmg_hip_mf_laplace_smoother_sweep(self.handle, k, a, be, _dev_ptr(b, n), _dev_ptr(x, n) if x is not None else None, _dev_ptr(out, n),
                                                           _dev_ptr(out_prev, n) if out_prev is not None else None))

    def set_sweep_tile(self, waves: int, ty: int, tz: int):
        check(self._lib.mfmg_hip_mf_laplace_set_sweep_tile(self.handle, waves, ty, tz))

    def set_sweep_reference(self, on: bool):
        """The sweep's cell kernel: mode space (default) or the arithmetic of the one-term kernel, bit for bit."""
        check(self._lib.mfmg_hip_mf_laplace_set_sweep_reference(self.handle, int(bool(on))))

    def get_sweep_tile(self, n_terms: int):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_get_sweep_tile(self.handle, int(n_terms), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_sweep_diagonal(self, source: str):
        """D^-1 of the sweep of twelve wavefronts: "stored" (read from the vector built at construction, the default where
        the operator has one) or "derived" (formed from the coefficient sums per DoF and launch); the same bits either way."""
        if source not in ("stored", "derived"):
            raise ValueError("source must be 'stored' or 'derived'")
        check(self._lib.mfmg_hip_mf_laplace_set_sweep_diagonal(self.handle, int(source == "stored")))

    def sweep_diagonal(self) -> str:
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_get_sweep_diagonal(self.handle, C.byref(v)))
        return "stored" if v.value else "derived"

    def sweep_diagonal_inverse(self) -> torch.Tensor:
        """A copy of the D^-1 vector of the sweep (raises where the operator has none)."""
        out = torch.empty(self.n_dofs, dtype=torch.float64, device="cuda")
        check(self._lib.mfmg_hip_mf_laplace_sweep_diagonal_inverse(self.handle, _dev_ptr(out)))
        self.ctx.synchronize()
        return out

    def diagonal_inverse(self) -> torch.Tensor:
        out = torch.empty(self.n_dofs, dtype=torch.float64, device="cuda")
        check(self._lib.mfmg_hip_mf_laplace_diagonal_inverse(self.handle, _dev_ptr(out)))
        self.ctx.synchronize()
        return out

    def diagonal(self) -> torch.Tensor:
        out = torch.empty(self.n_dofs, dtype=torch.float64, device="cuda")
        check(self._lib.mfmg_hip_mf_laplace_diagonal(self.handle, _dev_ptr(out)))
        self.ctx.synchronize()
        return out

    def cell_constant_layout(self) -> bool:
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_cell_constant_layout(self.handle, C.byref(v)))
        return bool(v.value)

    def uniform_coefficient(self) -> bool:
        """One coefficient for the whole mesh, all six faces Dirichlet, one rank: the three-term FP64 sweep applies the
        operator as three 1-D stencils (MFMG_MF_UNIFORM_SWEEP=0 keeps the mode-space kernels)."""
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_uniform_coefficient(self.handle, C.byref(v), None))
        return bool(v.value)

    def uniform_sweep_launches(self) -> int:
        """Sweeps of this operator that took the stencil kernel of a uniform coefficient so far."""
        v, n = C.c_int(), C.c_int64()
        check(self._lib.mfmg_hip_mf_laplace_uniform_coefficient(self.handle, C.byref(v), C.byref(n)))
        return int(n.value)

    def diagonal_in_record(self) -> bool:
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_diagonal_in_record(self.handle, C.byref(v)))
        return bool(v.value)

    def ids_computed(self) -> bool:
        """The kernel computes the DoF ids from the position instead of reading them from its records."""
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_ids_computed(self.handle, C.byref(v)))
        return bool(v.value)

    def get_tile(self):
        """(waves, ty, tz) of the next launch."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_get_tile(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_tile(self, ty: int, tz: int, waves: int = None):
        check(self._lib.mfmg_hip_mf_laplace_set_tile(self.handle, ty, tz))
        if waves is not None:
            check(self._lib.mfmg_hip_mf_laplace_set_tile_waves(self.handle, waves))

    _BLOCK_MODES = {"apply": 0, "residual": 1, "first": 2, "next": 3}

    def block_launch(self, mode: str, X, out, B=None, X_prev=None, alpha: float = 0.0, beta: float = 0.0):
        """One operator launch on every vector of a block: mode "apply" out = A x, "residual" out = A x - b, "first" out = x -
        beta D^-1 (A x - b), "next" out = x + alpha (x - x_prev) - beta D^-1 (A x - b).  The blocks are 2-D float64 tensors of
        shape (k, m), stride(1) == 1, with one leading dimension ld = stride(0) >= n_dofs; out may be X_prev.  Every row gets
        the bits of vmult / residual / smoother_step on that row."""
        k, ld, px = _block_ptr(X)
        check(self._lib.mfmg_hip_mf_laplace_block_launch(
            self.handle, self._BLOCK_MODES[mode], k, ld, px, _same_block(k, ld, B) if B is not None else None,
            _same_block(k, ld, X_prev) if X_prev is not None else None, alpha, beta, _same_block(k, ld, out)))

    def block_available(self) -> bool:
        """Groups of 4 and 2 vectors of a block run the block kernel (eight coefficients per cell, 3-D, no tail slab)."""
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_block_available(self.handle, C.byref(v)))
        return bool(v.value)

    def set_block_tile(self, waves: int, ty: int, tz: int):
        check(self._lib.mfmg_hip_mf_laplace_set_block_tile(self.handle, waves, ty, tz))

    def get_block_tile(self, n_vectors: int):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_get_block_tile(self.handle, int(n_vectors), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.mfmg_hip_mf_laplace_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class MatrixFreeLaplaceF32:
    """FP32 instance of the matrix-free operator (BASELINE.json configs[4]); vectors are float32 tensors."""

    def __init__(self, ctx: Context, problem):
        self._lib = _lib.load()
        self.ctx = ctx
        desc = problem.mesh_desc()
        h = C.c_void_p()
        check(self._lib.mfmg_hip_mf_laplace_f32_create(ctx.handle, C.byref(desc), C.byref(h)))
        self.handle = h
        self.n_dofs = problem.n_dofs

    def _p(self, t):
        return _dev_ptr(t, self.n_dofs, torch.float32)

    def vmult(self, dst, src):
        check(self._lib.mfmg_hip_mf_laplace_f32_vmult(self.handle, self._p(src), self._p(dst)))

    def residual(self, x, b, res):
        check(self._lib.mfmg_hip_mf_laplace_f32_residual(self.handle, self._p(x), self._p(b), self._p(res)))

    def smoother_step(self, b, x, x_prev, alpha, beta, out):
        check(self._lib.mfmg_hip_mf_laplace_f32_smoother_step(self.handle, self._p(b), self._p(x),
                                                              self._p(x_prev) if x_prev is not None else None,
                                                              alpha, beta, self._p(out)))

    def sweep_available(self, n_terms: int) -> bool:
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_f32_sweep_available(self.handle, int(n_terms), C.byref(v)))
        return bool(v.value)

    def smoother_sweep(self, alpha, beta, b, x, out, out_prev=None):
        k = len(alpha)
        a = (C.c_float * k)(*[float(v) for v in alpha])
        be = (C.c_float * k)(*[float(v) for v in beta])
        # (x = None reaches the C entry as a null pointer, which it refuses: the sweep from a zero guess is FP64 only)
        check(self._lib.mfmg_hip_mf_laplace_f32_smoother_sweep(self.handle, k, a, be, self._p(b), self._p(x) if x is not None else None,
                                                               self._p(out), self._p(out_prev) if out_prev is not None else None))

    def set_sweep_reference(self, on: bool):
        check(self._lib.mfmg_hip_mf_laplace_f32_set_sweep_reference(self.handle, int(bool(on))))

    def set_sweep_tile(self, waves: int, ty: int, tz: int):
        check(self._lib.mfmg_hip_mf_laplace_f32_set_sweep_tile(self.handle, waves, ty, tz))

    def get_sweep_tile(self, n_terms: int):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_f32_get_sweep_tile(self.handle, int(n_terms), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def get_tile(self):
        """(waves, ty, tz) of the next launch."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_f32_get_tile(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_tile(self, ty: int, tz: int, waves: int = None):
        check(self._lib.mfmg_hip_mf_laplace_f32_set_tile(self.handle, ty, tz))
        if waves is not None:
            check(self._lib.mfmg_hip_mf_laplace_f32_set_tile_waves(self.handle, waves))

    _BLOCK_MODES = MatrixFreeLaplace._BLOCK_MODES

    def block_launch(self, mode: str, X, out, B=None, X_prev=None, alpha: float = 0.0, beta: float = 0.0):
        """MatrixFreeLaplace.block_launch on float32 blocks: 2-D float32 tensors of shape (k, m), stride(1) == 1, with one even
        leading dimension ld = stride(0) >= n_dofs and bases aligned to 8 bytes; out may be X_prev.  Every row gets the bits of
        vmult / residual / smoother_step of this operator on that row."""
        f32 = torch.float32
        k, ld, px = _block_ptr(X, f32)
        check(self._lib.mfmg_hip_mf_laplace_f32_block_launch(
            self.handle, self._BLOCK_MODES[mode], k, ld, px, _same_block(k, ld, B, f32) if B is not None else None,
            _same_block(k, ld, X_prev, f32) if X_prev is not None else None, alpha, beta, _same_block(k, ld, out, f32)))

    def block_available(self) -> bool:
        """Groups of 4 and 2 vectors of a block run mf_laplace_block_f32_kernel (eight coefficients per cell, 3-D, no tail slab)."""
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_f32_block_available(self.handle, C.byref(v)))
        return bool(v.value)

    def set_block_tile(self, waves: int, ty: int, tz: int):
        check(self._lib.mfmg_hip_mf_laplace_f32_set_block_tile(self.handle, waves, ty, tz))

    def get_block_tile(self, n_vectors: int):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_f32_get_block_tile(self.handle, int(n_vectors), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def diagonal_in_record(self) -> bool:
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_f32_diagonal_in_record(self.handle, C.byref(v)))
        return bool(v.value)

    def cell_constant_layout(self) -> bool:
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_f32_cell_constant_layout(self.handle, C.byref(v)))
        return bool(v.value)

    def ids_computed(self) -> bool:
        v = C.c_int()
        check(self._lib.mfmg_hip_mf_laplace_f32_ids_computed(self.handle, C.byref(v)))
        return bool(v.value)

    def diagonal_inverse(self) -> torch.Tensor:
        out = torch.empty(self.n_dofs, dtype=torch.float32, device="cuda")
        check(self._lib.mfmg_hip_mf_laplace_f32_diagonal_inverse(self.handle, self._p(out)))
        self.ctx.synchronize()
        return out

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.mfmg_hip_mf_laplace_f32_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class Hierarchy:
    """mfmg::Hierarchy<VectorType> (include/mfmg/common/hierarchy.hpp:155-373)."""

    def __init__(self, ctx: Context, evaluator_type: str, problem, params: dict | str):
        self._lib = _lib.load()
        self.ctx = ctx
        info = params if isinstance(params, str) else params_to_info(params)
        desc = problem.mesh_desc()
        h = C.c_void_p()
        check(self._lib.mfmg_hip_hierarchy_create(ctx.handle, evaluator_type.encode(), C.byref(desc),
                                                  info.encode(), C.byref(h)))
        self.handle = h

    @property
    def n_levels(self) -> int:
        n = C.c_int32()
        check(self._lib.mfmg_hip_hierarchy_n_levels(self.handle, C.byref(n)))
        return n.value

    def level_size(self, level: int) -> int:
        n = C.c_int64()
        check(self._lib.mfmg_hip_hierarchy_level_size(self.handle, level, C.byref(n)))
        return n.value

    def internal_numbering(self):
        """(lexicographic, permuted): built with "internal numbering" lexicographic; vectors are permuted at the interface
        (0 where the caller's numbering already was lexicographic)."""
        a, b = C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_hierarchy_internal_numbering(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def permute(self, vin: torch.Tensor, vout: torch.Tensor, to_internal: bool = True):
        """vout = vin in the internal numbering of the hierarchy (to_internal) or back in the caller's; float64 or float32
        fine-level vectors, vin is not vout."""
        n = self.level_size(0)
        assert vin.dtype == vout.dtype and vin.dtype in (torch.float64, torch.float32)
        fp32 = vin.dtype == torch.float32
        check(self._lib.mfmg_hip_hierarchy_permute(self.handle, int(bool(to_internal)), int(fp32), _dev_ptr(vin, n, vin.dtype),
                                                   _dev_ptr(vout, n, vout.dtype)))

    def apply(self, b: torch.Tensor, x: torch.Tensor):
        n = self.level_size(0)
        check(self._lib.mfmg_hip_hierarchy_apply(self.handle, _dev_ptr(b, n), _dev_ptr(x, n)))

    def apply_f32(self, b: torch.Tensor, x: torch.Tensor):
        """The same cycle on float32 vectors with the fine level in FP32 (parameter "fine level precision": "float").  On a
        context with a HaloTransport b and x are the rank's local float vectors (ghost entries are don't-care on entry)."""
        n = self.level_size(0)
        check(self._lib.mfmg_hip_hierarchy_apply_f32(self.handle, _dev_ptr(b, n, torch.float32), _dev_ptr(x, n, torch.float32)))

    def apply_f32_block(self, B: torch.Tensor, X: torch.Tensor):
        """The cycle of apply_f32() on every row of the float32 blocks B and X (shape (k, m), stride(1) == 1, one even leading
        dimension ld = stride(0) >= n_dofs, bases aligned to 8 bytes).  Row c of X gets the bits of apply_f32(B[c], X[c]).  On a
        context with a HaloTransport the rows are the rank's local float vectors and that holds on the entries the rank owns; a
        group of 4 or 2 rows exchanges its ghost planes in one message per neighbour where the ranks agreed on float blocks at
        setup (block_info_f32()["width"] == 4), else every rank loops over the rows."""
        k, ld, pb = _block_ptr(B, torch.float32)
        check(self._lib.mfmg_hip_hierarchy_apply_f32_block(self.handle, k, ld, pb, _same_block(k, ld, X, torch.float32)))

    def block_info_f32(self) -> dict:
        """block_info() of the FP32 fine level: width; block_launches / column_launches of mf_laplace_block_f32_kernel and of the
        one-vector cycle in the last FP32 block call -- apply_f32_block, or the preconditioner applications of the last
        solve_fgmres_block(preconditioner="float")."""
        f = (C.c_int64 * 3)()
        check(self._lib.mfmg_hip_hierarchy_block_info_f32(self.handle, f))
        return {"width": int(f[0]), "block_launches": int(f[1]), "column_launches": int(f[2])}

    def operator_f32(self, mode: str, x: torch.Tensor, out: torch.Tensor, b=None, x_prev=None, alpha: float = 0.0, beta: float = 0.0):
        """The FP32 operator of the fine level on its own (tests): mode "vmult" out = A x, "residual" out = A x - b, "step"
        out = x + alpha (x - x_prev) - beta D^-1 (A x - b).  On ranks the call exchanges the ghost entries of x."""
        n = self.level_size(0)
        p = lambda t: 0 if t is None else _dev_ptr(t, n, torch.float32)
        check(self._lib.mfmg_hip_hierarchy_operator_f32(self.handle, {"vmult": 0, "residual": 1, "step": 2}[mode], p(x), p(b), p(x_prev),
                                                        float(alpha), float(beta), p(out)))

    def sweep_terms_f32(self) -> int:
        """Terms the FP32 smoother runs as one sweep (0: a launch per term); the same on every rank."""
        k = C.c_int()
        check(self._lib.mfmg_hip_hierarchy_sweep_terms_f32(self.handle, C.byref(k)))
        return k.value

    def vmult(self, x: torch.Tensor, b: torch.Tensor):
        n = self.level_size(0)
        check(self._lib.mfmg_hip_hierarchy_vmult(self.handle, _dev_ptr(x, n), _dev_ptr(b, n)))

    def operator_apply(self, level: int, x, y, mode: int = _lib.NO_TRANS):
        n = self.level_size(level)
        check(self._lib.mfmg_hip_hierarchy_operator_apply(self.handle, level, _dev_ptr(x, n), _dev_ptr(y, n), mode))

    def smoother_apply(self, level: int, b, x):
        n = self.level_size(level)
        check(self._lib.mfmg_hip_hierarchy_smoother_apply(self.handle, level, _dev_ptr(b, n), _dev_ptr(x, n)))

    def apply_block(self, B: torch.Tensor, X: torch.Tensor):
        """The cycle of apply() on every row of the blocks B and X: 2-D float64 tensors of shape (k, m), stride(1) == 1, with one
        leading dimension ld = stride(0) >= n_dofs (even; the bases aligned to 16 bytes).  Row c of X gets the bits of
        apply(B[c], X[c]).  On a context with a HaloTransport the rows are the rank's local vectors and that holds on the entries
        the rank owns; a group of 4 or 2 rows then exchanges its ghost planes in one message per neighbour where the ranks agreed
        on blocks at setup (block_info()["width"] == 4), else every rank loops over the rows."""
        k, ld, pb = _block_ptr(B)
        check(self._lib.mfmg_hip_hierarchy_apply_block(self.handle, k, ld, pb, _same_block(k, ld, X)))

    def vmult_block(self, X: torch.Tensor, B: torch.Tensor):
        k, ld, pb = _block_ptr(B)
        check(self._lib.mfmg_hip_hierarchy_vmult_block(self.handle, k, ld, _same_block(k, ld, X), pb))

    def smoother_apply_block(self, level: int, B: torch.Tensor, X: torch.Tensor):
        k, ld, pb = _block_ptr(B)
        check(self._lib.mfmg_hip_hierarchy_smoother_apply_block(self.handle, level, k, ld, pb, _same_block(k, ld, X)))

    def block_info(self) -> dict:
        """width: vectors of the widest group the fine level runs as one launch (1 = the loop over the vectors; on several ranks
        the value all ranks agreed on at setup); block_launches /
        column_launches: launches of the block kernel, and vectors that went through the one-vector entry point, in the last
        block call."""
        f = (C.c_int64 * 3)()
        check(self._lib.mfmg_hip_hierarchy_block_info(self.handle, f))
        return {"width": int(f[0]), "block_launches": int(f[1]), "column_launches": int(f[2])}

    def restrictor_apply(self, level: int, vin, vout, mode: int = _lib.NO_TRANS):
        """vout = R vin (NO_TRANS), vout = R^T vin (TRANS) or vout -= R^T vin (TRANS_SUBTRACT)."""
        nf, nc = self.level_size(level - 1), self.level_size(level)
        ni, no = (nf, nc) if mode == _lib.NO_TRANS else (nc, nf)
        check(self._lib.mfmg_hip_hierarchy_restrictor_apply(self.handle, level, _dev_ptr(vin, ni), _dev_ptr(vout, no), mode))

    def restrictor_apply_block(self, level: int, Vin: torch.Tensor, Vout: torch.Tensor, mode: int = _lib.NO_TRANS):
        """restrictor_apply(level, Vin[c], Vout[c], mode) for every row of the blocks Vin and Vout (2-D float64 tensors of shape
        (k, m), stride(1) == 1; each leading dimension stride(0) even and at least the size of its vectors, the bases aligned
        to 16 bytes), bit for bit.  A restrictor in the agglomerate-wise form reads its stored values once per group of 4 or 2
        rows (transfer_block_info()); one rank only."""
        k, ld_in, pi = _block_ptr(Vin)
        ko, ld_out, po = _block_ptr(Vout)
        if ko != k:
            raise ValueError("the blocks of one call share the number of vectors")
        check(self._lib.mfmg_hip_hierarchy_restrictor_apply_block(self.handle, level, k, ld_in, pi, ld_out, po, mode))

    def transfer_block_info(self, level: int = 1) -> dict:
        """restrict_width / prolong_width: rows of the widest block restriction / prolongation of `level` (1 = the loop over
        the rows); restrict_launches / prolong_launches: launches of the block kernels, and column_launches: rows whose
        restriction or prolongation went through the one-vector kernels, in the last block call on this hierarchy (a cycle, a
        solve or restrictor_apply_block)."""
        f = (C.c_int64 * 5)()
        check(self._lib.mfmg_hip_hierarchy_transfer_block_info(self.handle, level, f))
        return {"restrict_width": int(f[0]), "prolong_width": int(f[1]), "restrict_launches": int(f[2]),
                "prolong_launches": int(f[3]), "column_launches": int(f[4])}

    _RESTRICT_KERNELS = {1: "rows", 2: "pair222", 3: "pair"}
    _PROLONG_KERNELS = {1: "nodes", 2: "block222"}

    def restrictor_form(self, level: int = 1) -> dict:
        """How the restrictor of `level` is evaluated: the agglomerate-wise form or CSR, and which kernels it launches."""
        f = (C.c_int32 * _lib.RESTRICTOR_FORM_FIELDS)()
        check(self._lib.mfmg_hip_hierarchy_restrictor_form(self.handle, level, f, _lib.RESTRICTOR_FORM_FIELDS))
        if not f[0]:
            return {"structured": False}
        return {"structured": True, "n_eig": f[1], "a": (f[2], f[3], f[4]), "float_planes": bool(f[5]),
                "table_agglomerates": f[6], "n_classes": f[7], "listed_blocks": f[8],
                "restrict": self._RESTRICT_KERNELS[f[9]], "prolong": self._PROLONG_KERNELS[f[10]],
                "prolong_march": bool(f[11])}

    _EIGENSOLVERS = {0: "host dense", 1: "device dense", 2: "lanczos"}

    def restrictor_eigensolver_info(self) -> dict:
        """What solved the agglomerate eigenproblems of the restrictor ("restrictor.eigensolver" device | host | lanczos) and its
        bookkeeping: nodes of a full agglomerate, agglomerates, eigenproblems solved (identical agglomerates share one), and for
        the Lanczos solver the largest step count, the agglomerates ended by breakdown and those unconverged at
        eigensolver.max_iterations; kernel_seconds is the wall time of the Lanczos kernel."""
        f = (C.c_int64 * _lib.EIGENSOLVER_INFO_FIELDS)()
        check(self._lib.mfmg_hip_hierarchy_restrictor_eigensolver_info(self.handle, f, _lib.EIGENSOLVER_INFO_FIELDS))
        t = C.c_double()
        check(self._lib.mfmg_hip_hierarchy_restrictor_eigensolver_seconds(self.handle, C.byref(t)))
        return {"solver": self._EIGENSOLVERS[f[0]], "nodes": f[1], "agglomerates": f[2], "solves": f[3], "max_iterations": f[4],
                "breakdowns": f[5], "unconverged": f[6], "kernel_seconds": t.value}

    def ap_apply(self, level: int, vin, vout):
        """vout = (A R^T) vin for the A R^T of `level` (hierarchies built with keep_ap = true)."""
        nf, nc = self.level_size(level - 1), self.level_size(level)
        check(self._lib.mfmg_hip_hierarchy_ap_apply(self.handle, level, _dev_ptr(vin, nc), _dev_ptr(vout, nf)))

    def coarse_apply(self, b, x):
        n = self.level_size(self.n_levels - 1)
        check(self._lib.mfmg_hip_hierarchy_coarse_apply(self.handle, _dev_ptr(b, n), _dev_ptr(x, n)))

    def coarse_apply_block(self, B: torch.Tensor, X: torch.Tensor):
        """coarse_apply() on every row of the blocks B and X (shape (k, m), layout as for apply_block), bit for bit.  With
        solver.type amg the cycle runs on groups of 4 and 2 rows, every matrix with stored values that do not repeat read once
        per group (coarse_block_info())."""
        k, ld, pb = _block_ptr(B)
        check(self._lib.mfmg_hip_hierarchy_coarse_apply_block(self.handle, k, ld, pb, _same_block(k, ld, X)))

    def coarse_block_info(self) -> dict:
        """width: the widest group any matrix of the coarse cycle takes (1: the loop over the rows); block_launches /
        column_launches: launches of the block kernels and one-vector launches of the matrices of the cycle in the last block
        call of the coarse solver (coarse_apply_block, or inside apply_block / vmult_block / a block solve)."""
        f = (C.c_int64 * 3)()
        check(self._lib.mfmg_hip_hierarchy_coarse_block_info(self.handle, f))
        return {"width": int(f[0]), "block_launches": int(f[1]), "column_launches": int(f[2])}

    def set_block_csr(self, on: bool = True) -> int:
        """SparseMatrixDevice.set_block_csr on every FP64 matrix the cycle applies: the assembled fine operator, a restrictor
        given as CSR, the first coarse operator, A, P^T, P and P~ of the aggregation levels and the triangular inverses of the
        bottom (whose solve then runs on the group).  Returns how many of them now report the width 4 through a CSR kernel.
        Off by default; one rank only."""
        n = C.c_int32()
        check(self._lib.mfmg_hip_hierarchy_set_block_csr(self.handle, 1 if on else 0, C.byref(n)))
        return int(n.value)

    def set_restrictor(self, matrix):
        rp, cl, vl, shape = _csr_arrays(matrix)
        check(self._lib.mfmg_hip_hierarchy_set_restrictor(self.handle, shape[0], shape[1], len(vl), rp.ctypes.data,
                                                          cl.ctypes.data, vl.ctypes.data))

    def restrictor(self) -> SparseMatrixDevice:
        h = C.c_void_p()
        check(self._lib.mfmg_hip_hierarchy_get_restrictor(self.handle, C.byref(h)))
        return SparseMatrixDevice(self.ctx, _handle=h, _borrowed=True, _keepalive=self)

    def fine_operator(self) -> SparseMatrixDevice:
        """The assembled operator of level 0 (HipMeshEvaluator hierarchies)."""
        h = C.c_void_p()
        check(self._lib.mfmg_hip_hierarchy_get_fine_operator(self.handle, C.byref(h)))
        return SparseMatrixDevice(self.ctx, _handle=h, _borrowed=True, _keepalive=self)

    def coarse_operator(self) -> SparseMatrixDevice:
        h = C.c_void_p()
        check(self._lib.mfmg_hip_hierarchy_get_coarse_operator(self.handle, C.byref(h)))
        return SparseMatrixDevice(self.ctx, _handle=h, _borrowed=True, _keepalive=self)

    def coarse_amg_levels(self):
        """[(A_l, P_l or None, (degree, lambda_min, lambda_max) or None)] of the multilevel coarse solver."""
        n = C.c_int32()
        check(self._lib.mfmg_hip_hierarchy_coarse_amg_levels(self.handle, C.byref(n)))
        out = []
        for l in range(n.value):
            h = C.c_void_p()
            check(self._lib.mfmg_hip_hierarchy_coarse_amg_get(self.handle, l, 0, C.byref(h)))
            A = SparseMatrixDevice(self.ctx, _handle=h, _borrowed=True, _keepalive=self).to_scipy()
            P = cheb = None
            if l + 1 < n.value:
                check(self._lib.mfmg_hip_hierarchy_coarse_amg_get(self.handle, l, 1, C.byref(h)))
                P = SparseMatrixDevice(self.ctx, _handle=h, _borrowed=True, _keepalive=self).to_scipy()
                d, lo, hi = C.c_int32(), C.c_double(), C.c_double()
                check(self._lib.mfmg_hip_hierarchy_coarse_amg_smoother(self.handle, l, C.byref(d), C.byref(lo), C.byref(hi)))
                cheb = (d.value, lo.value, hi.value)
            out.append((A, P, cheb))
        return out

    def coarse_amg_smoothed_prolongators(self):
        """[P~_l or None] per level of the multilevel coarse solver: the smoothed prolongator of the cycle, (I - beta D^-1 A_l) P_l,
        where the setup built one (levels that apply prolongation and post-smoothing as one operator)."""
        out = []
        for info in self.coarse_amg_setup_info():
            Pt = None
            if info["smoothed"]:
                h = C.c_void_p()
                check(self._lib.mfmg_hip_hierarchy_coarse_amg_get(self.handle, info["level"], 3, C.byref(h)))
                Pt = SparseMatrixDevice(self.ctx, _handle=h, _borrowed=True, _keepalive=self).to_scipy()
            out.append(Pt)
        return out

    def coarse_amg_smoothed_prolongator_forms(self):
        """[form() of P~_l or None] per level of the multilevel coarse solver: which kernels the smoothed prolongator of the
        cycle launches (also after "release setup matrices", when the matrix itself can no longer be exported)."""
        out = []
        for info in self.coarse_amg_setup_info():
            f = None
            if info["smoothed"]:
                h = C.c_void_p()
                check(self._lib.mfmg_hip_hierarchy_coarse_amg_get(self.handle, info["level"], 3, C.byref(h)))
                f = SparseMatrixDevice(self.ctx, _handle=h, _borrowed=True, _keepalive=self).form()
            out.append(f)
        return out

    _AMG_PRODUCTS = ("probes", "device product", "host product")

    def coarse_amg_setup_info(self):
        """What the setup of the aggregation hierarchy did, one dict per level: reach of the level's operator in nodes, probe
        periods per axis of P, A_c and P~ (None: not probed), how the next operator was formed ("probes", "device product",
        "host product"; None on the last level), whether the level is part of the replicated tail and whether it has a
        smoothed prolongator."""
        n = C.c_int32()
        check(self._lib.mfmg_hip_hierarchy_coarse_amg_levels(self.handle, C.byref(n)))
        out = []
        for l in range(n.value):
            v = (C.c_int32 * _lib.AMG_SETUP_INFO_FIELDS)()
            check(self._lib.mfmg_hip_hierarchy_coarse_amg_setup_info(self.handle, l, v, _lib.AMG_SETUP_INFO_FIELDS))
            period = lambda q: tuple(v[q:q + 3]) if any(v[q:q + 3]) else None
            out.append({"level": l, "reach": v[0], "period_p": period(1), "period_a": period(4), "period_t": period(7),
                        "coarse_operator": self._AMG_PRODUCTS[v[10]] if l + 1 < n.value else None,
                        "replicated": bool(v[11]), "smoothed": bool(v[12])})
        return out

    def coarse_amg_kernels(self, regular_rows=None):
        """[(level, which, rows, kernel kind, stencil classes, listed rows)] of the matrices of the multilevel coarse
        solver (which: 0 A_l, 1 P_l, 2 its stored transpose); regular_rows True / False switches the table-driven paths
        of all of them on / off first (tests: both must give the same cycle to rounding)."""
        n = C.c_int32()
        check(self._lib.mfmg_hip_hierarchy_coarse_amg_levels(self.handle, C.byref(n)))
        out = []
        for l in range(n.value):
            for which in (0, 1, 2):
                if which > 0 and l + 1 == n.value:
                    continue
                h = C.c_void_p()                              # (one borrowed view at a time)
                check(self._lib.mfmg_hip_hierarchy_coarse_amg_get(self.handle, l, which, C.byref(h)))
                m = SparseMatrixDevice(self.ctx, _handle=h, _borrowed=True, _keepalive=self)
                if regular_rows is not None:
                    m.set_regular_rows(regular_rows)
                out.append((l, which, m.shape[0], m.get_kernel()[1]) + tuple(m.stencil_classes()))
        return out

    def restrict_residual(self, x: torch.Tensor, b: torch.Tensor, b_coarse: torch.Tensor, level: int = 1):
        """b_coarse = R (A x - b) as the cycle computes it (hierarchy.hpp:281-290): one kernel where the rows of R A
        repeat themselves, the fused residual followed by the restriction otherwise."""
        nf, nc = self.level_size(level - 1), self.level_size(level)
        check(self._lib.mfmg_hip_hierarchy_restrict_residual(self.handle, level, _dev_ptr(x, nf), _dev_ptr(b, nf),
                                                             _dev_ptr(b_coarse, nc)))

    def restrict_residual_f32(self, x: torch.Tensor, b: torch.Tensor, b_coarse: torch.Tensor, level: int = 1):
        """The one-pass form on float32 x and b (b_coarse is float64), as apply_f32 runs it; raises MfmgNotImplementedError where
        that form is not built or the context has a communicator -- there is no two-step form behind it."""
        nf, nc = self.level_size(level - 1), self.level_size(level)
        check(self._lib.mfmg_hip_hierarchy_restrict_residual_f32(self.handle, level, _dev_ptr(x, nf, torch.float32),
                                                                 _dev_ptr(b, nf, torch.float32), _dev_ptr(b_coarse, nc)))

    def residual_restriction_classes(self, level: int = 1) -> int:
        """Agglomerate classes of the one-pass residual restriction; 0 when the two-step form is in use."""
        n = C.c_int32()
        check(self._lib.mfmg_hip_hierarchy_residual_restriction_classes(self.handle, level, C.byref(n)))
        return n.value

    _RR_KERNELS = {0: None, 1: "tile", 2: "rows"}

    def residual_restriction_form(self, level: int = 1) -> dict:
        """What a launch of the one-pass residual restriction consists of: classes, runs per row (`segs`), last agglomerate of a
        row in the row-wise part, agglomerates and runs left to the list, the kernel ("tile" or "rows") and the grid of the next
        launch (`tile_layers`, `tiles_j`, `n_tiles`, `main_blocks`).  All zero and `kernel` None where the form is not built."""
        f = (C.c_int64 * _lib.RESIDUAL_RESTRICTION_FORM_FIELDS)()
        check(self._lib.mfmg_hip_hierarchy_residual_restriction_form(self.handle, level, f, _lib.RESIDUAL_RESTRICTION_FORM_FIELDS))
        return {"classes": f[0], "segs": f[1], "main_last": f[2], "listed": f[3], "listed_runs": f[4],
                "kernel": self._RR_KERNELS[f[5]], "tile_layers": f[6], "tiles_j": f[7], "n_tiles": f[8], "main_blocks": f[9]}

    def coarse_amg_gather_level(self) -> int:
        """Index of the first aggregation level that is gathered and solved redundantly on every rank (-1: one rank)."""
        n = C.c_int32()
        check(self._lib.mfmg_hip_hierarchy_coarse_amg_gather_level(self.handle, C.byref(n)))
        return n.value

    def coarse_amg_gather_rows(self) -> int:
        """Global rows of that level (0 on one rank)."""
        l = self.coarse_amg_gather_level()
        return self.coarse_amg_shapes()[l][0] if l >= 0 else 0

    def coarse_amg_shapes(self):
        """[(rows, nnz(A_l), nnz(P_l) or 0)] of the multilevel coarse solver (no download)."""
        n = C.c_int32()
        check(self._lib.mfmg_hip_hierarchy_coarse_amg_levels(self.handle, C.byref(n)))
        out = []
        for l in range(n.value):
            h = C.c_void_p()
            check(self._lib.mfmg_hip_hierarchy_coarse_amg_get(self.handle, l, 0, C.byref(h)))
            A = SparseMatrixDevice(self.ctx, _handle=h, _borrowed=True, _keepalive=self)
            rows, an, pn = A.shape[0], A.nnz, 0
            if l + 1 < n.value:
                hp = C.c_void_p()
                check(self._lib.mfmg_hip_hierarchy_coarse_amg_get(self.handle, l, 1, C.byref(hp)))
                pn = SparseMatrixDevice(self.ctx, _handle=hp, _borrowed=True, _keepalive=self).nnz
            out.append((rows, an, pn))
        return out

    def smoother_sweep_terms(self):
        """(terms per sweep of the in-place smoother apply, of the out-of-place one); 0 = one launch per term."""
        a, b = C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_hierarchy_smoother_sweep_terms(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def smoother_info(self):
        d, lo, hi = C.c_int32(), C.c_double(), C.c_double()
        check(self._lib.mfmg_hip_hierarchy_smoother_info(self.handle, C.byref(d), C.byref(lo), C.byref(hi)))
        return d.value, lo.value, hi.value

    def solve_cg(self, b, x, tolerance: float = 1e-6, max_iterations: int = 1000):
        """tests/hierarchy_driver.cc:103-116: CG on the fine operator preconditioned by this hierarchy
        (build it with "is preconditioner" true).  Returns (iterations, residual history)."""
        import numpy as np
        n = self.level_size(0)
        it, res = C.c_int32(), C.c_double()
        hist = np.zeros(max_iterations + 1)
        check(self._lib.mfmg_hip_hierarchy_solve_cg(self.handle, _dev_ptr(b, n), _dev_ptr(x, n), tolerance, max_iterations,
                                                    C.byref(it), C.byref(res), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                                    len(hist)))
        return it.value, hist[: it.value + 1]

    def solve_cg_block(self, B: torch.Tensor, X: torch.Tensor, tolerances, max_iterations: int = 1000):
        """solve_cg for every row of the blocks B and X (2-D float64 tensors of shape (k, m), stride(1) == 1, one even leading
        dimension ld = stride(0) >= n_dofs) in one call: row c of X, its iteration count and its history are those of
        solve_cg(B[c], X[c], tolerances[c], max_iterations), bit for bit.  A column that converged costs nothing further.
        Returns (iterations, histories, work): k ints, k arrays, and a dict with the column-applications of the preconditioner
        and of the operator (each the sum of the iterations), the launches of the block kernel and the slot moves.  Raises the
        error of solve_cg when a column is unconverged at max_iterations; X and `last_block_solve` (the same triple) are filled.
        On a context with a HaloTransport B and X hold the rank's local vectors: the three reductions of an iteration run over the
        owned entries of all live rows and cross the ranks in one all-reduce each; every rank gets the same counts and histories,
        and the bits of solve_cg on the same ranks where the transport adds an element in the same order whatever the length of
        the message (any transport on two ranks)."""
        k, ld, pb = _block_ptr(B)
        px = _same_block(k, ld, X)
        tol = np.ascontiguousarray(np.broadcast_to(np.asarray(tolerances, dtype=np.float64), (k,)))
        its = np.zeros(k, dtype=np.int32)
        res = np.zeros(k)
        hist = np.zeros((k, max(max_iterations, 0) + 1))
        work = np.zeros(4, dtype=np.int64)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        status = self._lib.mfmg_hip_hierarchy_solve_cg_block(self.handle, k, ld, pb, px, dp(tol), max_iterations,
                                                             its.ctypes.data_as(C.POINTER(C.c_int32)), dp(res), dp(hist), hist.shape[1],
                                                             work.ctypes.data_as(C.POINTER(C.c_int64)))
        out = ([int(i) for i in its], [hist[c, : its[c] + 1].copy() for c in range(k)],
               {"preconditioner_columns": int(work[0]), "operator_columns": int(work[1]), "block_launches": int(work[2]),
                "slot_moves": int(work[3])})
        self.last_block_solve = out
        check(status)
        return out

    def operator_apply_block(self, level: int, X: torch.Tensor, Y: torch.Tensor):
        """Y[c] = A X[c] on `level` for every row of the blocks, with the bits of operator_apply."""
        k, ld, px = _block_ptr(X)
        check(self._lib.mfmg_hip_hierarchy_operator_apply_block(self.handle, level, k, ld, px, _same_block(k, ld, Y)))

    def solve_fgmres(self, b, x, tolerance: float = 1e-6, max_iterations: int = 1000, restart: int = 30,
                     preconditioner: str = "double"):
        """dealii::SolverFGMRES: right-preconditioned flexible GMRES(restart) on the fine operator with this hierarchy as
        preconditioner -- which may be non-symmetric (solver.amg.pre_smoothing_levels 0) or, with preconditioner="float", the
        FP32 fine level ("fine level precision" float) under the FP64 iteration.  Returns (iterations, residual history).
        On a context with a HaloTransport b and x are the rank's local vectors; every rank gets the same count and history
        (either preconditioner)."""
        if preconditioner not in ("double", "float"):
            raise _lib.MfmgInvalidArgument('preconditioner must be "double" or "float"')
        n = self.level_size(0)
        it, res = C.c_int32(), C.c_double()
        hist = np.zeros(max(max_iterations, 0) + 1)
        check(self._lib.mfmg_hip_hierarchy_solve_fgmres(self.handle, _dev_ptr(b, n), _dev_ptr(x, n), tolerance, max_iterations,
                                                        restart, 1 if preconditioner == "float" else 0, C.byref(it), C.byref(res),
                                                        hist.ctypes.data_as(C.POINTER(C.c_double)), len(hist)))
        return it.value, hist[: it.value + 1]

    def solve_fgmres_block(self, B: torch.Tensor, X: torch.Tensor, tolerances, max_iterations: int = 1000, restart: int = 30,
                           preconditioner: str = "double"):
        """solve_fgmres for every row of the blocks B and X (2-D float64 tensors of shape (k, m), stride(1) == 1, one even leading
        dimension ld = stride(0) >= n_dofs) in one call: row c of X, its iteration count and its history are those of
        solve_fgmres(B[c], X[c], tolerances[c], max_iterations, restart, preconditioner), bit for bit -- with the non-symmetric
        cycles and the FP32 fine level solve_cg_block cannot take.  A column that converged costs nothing further.
        Returns (iterations, histories, work): k ints, k arrays, and a dict with the column-applications of the preconditioner
        and of the operator inside Arnoldi steps (each the sum of the iterations), the launches of the block kernel and the
        cycle-start residuals formed.  Raises the error of solve_fgmres when a column is unconverged at max_iterations; X and
        `last_block_solve` (the same triple, with the final residuals as `residuals` in the dict) are filled.
        On a context with a HaloTransport the call is refused unless every rank called Context.set_block_fgmres_on_ranks(); then
        B and X hold the rank's local vectors: the Gram-Schmidt passes and the norms run over
        the owned entries of all live rows and cross the ranks in one all-reduce each -- three per iteration whatever k, one per
        cycle start, counted in work["allreduces"]; every rank gets the same counts and histories, and the bits of solve_fgmres
        on the same ranks where the transport adds an element in the same order whatever the length of the message (any
        transport on two ranks)."""
        if preconditioner not in ("double", "float"):
            raise _lib.MfmgInvalidArgument('preconditioner must be "double" or "float"')
        k, ld, pb = _block_ptr(B)
        px = _same_block(k, ld, X)
        tol = np.ascontiguousarray(np.broadcast_to(np.asarray(tolerances, dtype=np.float64), (k,)))
        its = np.zeros(k, dtype=np.int32)
        res = np.zeros(k)
        hist = np.zeros((k, max(max_iterations, 0) + 1))
        work = np.zeros(4, dtype=np.int64)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        status = self._lib.mfmg_hip_hierarchy_solve_fgmres_block(self.handle, k, ld, pb, px, dp(tol), max_iterations, restart,
                                                                 1 if preconditioner == "float" else 0,
                                                                 its.ctypes.data_as(C.POINTER(C.c_int32)), dp(res), dp(hist),
                                                                 hist.shape[1], work.ctypes.data_as(C.POINTER(C.c_int64)))
        n_allreduces = C.c_int64()
        count = getattr(self._lib, "mfmg_hip_hierarchy_block_solve_allreduces", None)  # (a comparison library may lack it)
        if count is not None:
            count(self.handle, C.byref(n_allreduces))
        out = ([int(i) for i in its], [hist[c, : its[c] + 1].copy() for c in range(k)],
               {"preconditioner_columns": int(work[0]), "operator_columns": int(work[1]), "block_launches": int(work[2]),
                "cycle_starts": int(work[3]), "allreduces": int(n_allreduces.value), "residuals": [float(r) for r in res]})
        self.last_block_solve = out
        check(status)
        return out

    def operator_tile(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_hierarchy_operator_tile(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def sweep_tile(self, n_terms: int):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.mfmg_hip_hierarchy_sweep_tile(self.handle, int(n_terms), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_sweep_tile(self, waves: int, ty: int, tz: int):
        check(self._lib.mfmg_hip_hierarchy_set_sweep_tile(self.handle, waves, ty, tz))

    def set_operator_tile(self, waves: int, ty: int, tz: int):
        check(self._lib.mfmg_hip_hierarchy_set_operator_tile(self.handle, waves, ty, tz))

    def timer_report(self) -> str:
        buf = C.create_string_buffer(8192)
        check(self._lib.mfmg_hip_hierarchy_timer_report(self.handle, buf, len(buf)))
        return buf.value.decode()

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.mfmg_hip_hierarchy_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def amge_eigen(ctx: Context, problem, params: dict | str, matrix_free: bool) -> dict:
    """The agglomerate eigen-solves of the restrictor setup on their own, with the device solver `params` names
    ("restrictor.eigensolver" device | lanczos).  Arrays per agglomerate (x fastest): n_vec [A], eigenvalues [A, n_eig],
    weights [A, n_eig, nodes] (diag_loc * vector on the local nodes, x fastest), iterations [A], converged [A], breakdown [A].
    The eigenvalues are those of the unshifted problem with either solver: under eigensolver.variant host, where the matrix that is
    solved carries the mean local diagonal as a shift, the shift is taken off.  A krylov group reports one of its members (the dense
    kernel its first).  Slots >= n_vec, nodes beyond the clipped agglomerate up to the stride and nodes that are not part of the
    eigenproblem (constrained ones under variant mf) are exactly 0."""
    lib = _lib.load()
    desc = problem.mesh_desc()
    info = (params if isinstance(params, str) else params_to_info(params)).encode()
    mf = 1 if matrix_free else 0
    na, ne, nn = C.c_int64(), C.c_int32(), C.c_int32()
    check(lib.mfmg_hip_amge_eigen(ctx.handle, C.byref(desc), info, mf, C.byref(na), C.byref(ne), C.byref(nn), None, None, None, None,
                                  None))
    A, E, N = na.value, ne.value, nn.value
    n_vec = np.zeros(A, dtype=np.int32)
    ev = np.zeros((A, E), dtype=np.float64)
    w = np.zeros((A, E, N), dtype=np.float64)
    its = np.zeros(A, dtype=np.int32)
    flags = np.zeros(A, dtype=np.int32)
    check(lib.mfmg_hip_amge_eigen(ctx.handle, C.byref(desc), info, mf, C.byref(na), C.byref(ne), C.byref(nn), n_vec.ctypes.data,
                                  ev.ctypes.data, w.ctypes.data, its.ctypes.data, flags.ctypes.data))
    return {"n_vec": n_vec, "eigenvalues": ev, "weights": w, "iterations": its, "converged": (flags & 1) != 0,
            "breakdown": (flags & 2) != 0}


# ---- host-side setup pieces (no GPU) ------------------------------------------------------
def _host_csr_to_scipy(lib, h):
    import scipy.sparse as sp
    m, n, z = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib.mfmg_hip_host_csr_shape(h, C.byref(m), C.byref(n), C.byref(z)))
    rp = np.empty(m.value + 1, dtype=np.int32)
    cl = np.empty(z.value, dtype=np.int32)
    vl = np.empty(z.value, dtype=np.float64)
    check(lib.mfmg_hip_host_csr_get(h, rp.ctypes.data, cl.ctypes.data, vl.ctypes.data))
    lib.mfmg_hip_host_csr_destroy(h)
    return sp.csr_matrix((vl, cl, rp), shape=(m.value, n.value))


def host_assemble_matrix(problem, semantics: str = "assembled"):
    lib = _lib.load()
    assert problem.device.type == "cpu"
    desc = problem.mesh_desc()
    h = C.c_void_p()
    check(lib.mfmg_hip_host_assemble_matrix(C.byref(desc), 0 if semantics == "assembled" else 1, C.byref(h)))
    return _host_csr_to_scipy(lib, h)


def host_build_restrictor(problem, params: dict | str, matrix_free: bool):
    lib = _lib.load()
    assert problem.device.type == "cpu"
    desc = problem.mesh_desc()
    info = params if isinstance(params, str) else params_to_info(params)
    h = C.c_void_p()
    check(lib.mfmg_hip_host_build_restrictor(C.byref(desc), info.encode(), 1 if matrix_free else 0, C.byref(h)))
    return _host_csr_to_scipy(lib, h)


def host_galerkin(problem, R, semantics: str = "assembled"):
    lib = _lib.load()
    assert problem.device.type == "cpu"
    desc = problem.mesh_desc()
    rp, cl, vl, shape = _csr_arrays(R)
    h = C.c_void_p()
    check(lib.mfmg_hip_host_galerkin(C.byref(desc), 0 if semantics == "assembled" else 1, shape[0], len(vl),
                                     rp.ctypes.data, cl.ctypes.data, vl.ctypes.data, C.byref(h)))
    return _host_csr_to_scipy(lib, h)


def host_amg_build(A, near_null=None, params: dict | str = "", grid_dims=None, node_of_row=None,
                   component_of_row=None):
    """Smoothed-aggregation hierarchy of the multilevel coarse solver on the host: [(A_l, P_l or None)]."""
    lib = _lib.load()
    rp, cl, vl, shape = _csr_arrays(A)
    info = params if isinstance(params, str) else params_to_info(params)
    nn = None if near_null is None else np.ascontiguousarray(near_null, dtype=np.float64)
    gd = None if grid_dims is None else np.ascontiguousarray(grid_dims, dtype=np.int32)
    nr = None if node_of_row is None else np.ascontiguousarray(node_of_row, dtype=np.int32)
    cr = None if component_of_row is None else np.ascontiguousarray(component_of_row, dtype=np.int32)
    h = C.c_void_p()
    check(lib.mfmg_hip_host_amg_build(shape[0], len(vl), rp.ctypes.data, cl.ctypes.data, vl.ctypes.data,
                                      nn.ctypes.data if nn is not None else None,
                                      gd.ctypes.data if gd is not None else None,
                                      nr.ctypes.data if nr is not None else None,
                                      cr.ctypes.data if cr is not None else None, info.encode(), C.byref(h)))
    n = C.c_int32()
    check(lib.mfmg_hip_host_amg_n_levels(h, C.byref(n)))
    out = []
    for l in range(n.value):
        m = C.c_void_p()
        check(lib.mfmg_hip_host_amg_get(h, l, 0, C.byref(m)))
        Al = _host_csr_to_scipy(lib, m)
        Pl = None
        if l + 1 < n.value:
            check(lib.mfmg_hip_host_amg_get(h, l, 1, C.byref(m)))
            Pl = _host_csr_to_scipy(lib, m)
        out.append((Al, Pl))
    lib.mfmg_hip_host_amg_destroy(h)
    return out


def params_get(info: str, path: str) -> str:
    lib = _lib.load()
    buf = C.create_string_buffer(1024)
    check(lib.mfmg_hip_host_params_get(info.encode(), path.encode(), buf, len(buf)))
    return buf.value.decode()
