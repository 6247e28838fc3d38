// Matrix-free Q1 Laplace operator on a logically structured hex mesh, device resident.
//
// Fills the hole of the reference's CUDA back-end: CudaMatrixFreeOperator::vmult
// only forwards to a user evaluator whose base class throws
// (source/cuda/cuda_matrix_free_operator.cu:32-37,
//  include/mfmg/cuda/cuda_matrix_free_mesh_evaluator.cuh:62-69); the arithmetic it
// has to reproduce is LaplaceOperator::local_apply / compute_diagonal of
// tests/laplace_matrix_free.hpp:75-98,129-156 with the constrained-row semantics of
// deal.II's MatrixFreeOperators::Base::vmult.
#pragma once

#include "common.hpp"

#include <algorithm>
#include <memory>

namespace mfmg
{
// Fused epilogues of the operator kernel.
enum class MfMode : int
{
  apply = 0,    // out = A x
  residual = 1, // out = A x - b                       (hierarchy.hpp:284-286)
  first = 2,    // out = x - beta dinv (A x - b)       (Jacobi / first Chebyshev term)
  next = 3      // out = x + alpha (x - x_prev) - beta dinv (A x - b)
};

// A numbering the kernel can compute: id(i, j, k) = base + i s0 + j s1 + k s2 on the node grid (any lexicographic
// numbering; the rotated slab of the tail columns has s0 = row length, s1 = 1), Dirichlet flags on whole faces of the box
// (bit 0 / 1: i = 0 / Nx - 1, bits 2, 3: j, bits 4, 5: k) and ghost flags on whole planes along every axis: the ghost_lo[d] first
// and the ghost_hi[d] last node planes of axis d (the slabs and boxes of a distributed run; a node on a Dirichlet face carries
// the Dirichlet flag only, in a ghost plane too).  Verified slot by slot against the records at construction; the id loads -- a
// request per row whose answer the x requests wait for -- disappear from the kernel.
struct AffineIds
{
  int base, s0, s1, s2;
  int faces;
  int ghost_lo[3], ghost_hi[3];
};

template <typename T>
struct MfArgs; // kernel arguments (mf_laplace.hip)

// The vectors and scalars of one launch: out = the epilogue of the mode on A x (b, x_prev, alpha, beta where the mode reads them).
template <typename T>
struct MfOperands
{
  T const *x, *b, *x_prev;
  T alpha, beta;
  T *out;
};

// The same for a block of n_vectors vectors: the columns of x, b, x_prev and out share the leading dimension ld (column c of x
// starts at x + c * ld elements; ld >= n_dofs, even; the bases aligned to two elements: 16 bytes in FP64, 8 in FP32).  out may be x_prev, column for column.
template <typename T>
struct MfBlockOperands
{
  T const *x, *b, *x_prev;
  T *out;
  int64_t ld;
  int n_vectors;
  T alpha, beta;
};

// How a block of n_vectors (1 .. kMfBlockMaxVectors) is cut into launches: groups of 4, then one of 2, then one single vector.
// Returns the number of groups, their widths in `widths`; InvalidArgumentExc outside the range.  (mf_laplace_block.hip)
constexpr int kMfBlockMaxVectors = 64, kMfBlockMaxGroups = 18;
int mf_block_groups(int n_vectors, int widths[kMfBlockMaxGroups]);

// A smoother term without momentum (no x_prev, or alpha = 0) is a `first` term: it reads no x_prev.
template <typename T>
inline MfMode mf_smoother_mode(T const *x_prev, T alpha)
{
  return (x_prev == nullptr || alpha == T(0)) ? MfMode::first : MfMode::next;
}

// tile of one workgroup: nw wavefronts of ty cell rows each, tz layers
struct MfTile
{
  int nw, ty, tz;
};

// Which tiles of tiling() a launch covers (every DoF is owned by exactly one tile, so regions that cover all tiles once give
// the full result): the box [begin, end) of (column, y, z) tiles, or everything outside it -- the shell around the interior
// tiles of a distributed run, the tail columns included, as ONE launch.  main_part / tail_part (boxes only): the column tiles
// of the box / the columns of a nearly empty last chunk, which are no column tiles (all y, the z-tiles of the box).
// whole_mesh: every tile and the tail; the only region that runs on the graded z-tiling (z_tiling), its box is not read.
struct MfTileRegion
{
  int begin[3] = {0, 0, 0}, end[3] = {0, 0, 0};
  bool whole_mesh = false, outside = false;
  bool main_part = true, tail_part = true;
  hipStream_t stream = nullptr; // nullptr: the context's (the shell of a distributed run goes to the exchange stream)

  static MfTileRegion whole()
  {
    MfTileRegion r;
    r.whole_mesh = true;
    return r;
  }
  static MfTileRegion box(int const begin[3], int const end[3], bool main_part = true, bool tail_part = false)
  {
    MfTileRegion r;
    std::copy(begin, begin + 3, r.begin);
    std::copy(end, end + 3, r.end);
    r.main_part = main_part;
    r.tail_part = tail_part;
    return r;
  }
  static MfTileRegion outside_of(int const begin[3], int const end[3], hipStream_t stream = nullptr)
  {
    MfTileRegion r = box(begin, end, true, true);
    r.outside = true;
    r.stream = stream;
    return r;
  }
};

// The shell of tiles around the box [lo, hi) of an nt[0] x nt[1] x nt[2] tiling as six slabs {c0, c1, y0, y1, z0, z1}: the z
// slabs over all columns and rows (below, above), the y slabs between them, the x slabs between those; lo and hi are clamped
// to the tiling, a slab may be empty (see mf_slab_empty).
inline void mf_shell_slabs(int const lo_in[3], int const hi_in[3], int const nt[3], int slab[6][6])
{
  int lo[3], hi[3];
  for (int d = 0; d < 3; ++d)
  {
    lo[d] = std::min(std::max(lo_in[d], 0), nt[d]);
    hi[d] = std::min(std::max(hi_in[d], lo[d]), nt[d]);
  }
  const int s[6][6] = {{0, nt[0], 0, nt[1], 0, lo[2]},         {0, nt[0], 0, nt[1], hi[2], nt[2]},
                       {0, nt[0], 0, lo[1], lo[2], hi[2]},     {0, nt[0], hi[1], nt[1], lo[2], hi[2]},
                       {0, lo[0], lo[1], hi[1], lo[2], hi[2]}, {hi[0], nt[0], lo[1], hi[1], lo[2], hi[2]}};
  std::copy(&s[0][0], &s[0][0] + 36, &slab[0][0]);
}
inline bool mf_slab_empty(int const slab[6]) { return slab[1] <= slab[0] || slab[3] <= slab[2] || slab[5] <= slab[4]; }

template <typename T>
class MatrixFreeLaplaceDevice
{
public:
  // allow_compact: keep ONE coefficient per cell when the eight quadrature values of every cell are equal
  // (detected on the device); false forces the general eight-value layout
  // sub_mesh (internal, the tail slab): the cells are a sub-box of a larger numbering, n_dofs is the vector length
  MatrixFreeLaplaceDevice(HipHandle &handle, mfmg_hip_mesh_desc const &mesh, bool allow_compact = true,
                          bool sub_mesh = false);
  bool cell_constant_layout() const { return _compact; }
  bool diagonal_in_record() const { return _dinv_in_record; }
  // One coefficient for the whole mesh: the cell-constant layout with a numbering the kernel computes, all six faces Dirichlet,
  // no ghost layers, no D^-1 in the records, and every stored cell coefficient of the same bits (a reduction on the device at
  // construction).  The operator on the free DoFs is then one 27-point stencil and D^-1 one number: the three-term FP64 sweep
  // applies it as three 1-D stencils on every tile shape (mf_cheb_fused.hip: mf_cheb_fused_uniform_kernel for twelve wavefronts of
  // two rows, which then hold three node rows each of their own, mf_cheb_fused_uniform_rows_kernel for the others) unless MFMG_MF_UNIFORM_SWEEP=0 or the reference arithmetic is asked for.
  bool uniform_coefficient() const { return _uniform; }
  // sweeps that took that kernel so far
  int64_t uniform_sweep_launches() const { return _uniform_sweeps; }

  int64_t n_dofs() const { return _n_dofs; }
  int dim() const { return _dim; }
  int dof_grid(int d) const { return _N[d]; }
  int n_cells(int d) const { return _n[d]; }
  double cell_size(int d) const { return _h[d]; }

  void vmult(T const *x, T *y) const { launch(MfMode::apply, {x, nullptr, nullptr, T(0), T(0), y}); }
  void residual(T const *x, T const *b, T *res) const { launch(MfMode::residual, {x, b, nullptr, T(0), T(0), res}); }
  // out = x + alpha (x - x_prev) - beta dinv (A x - b); out must not alias x
  void smoother_step(T const *b, T const *x, T const *x_prev, T alpha, T beta, T *out) const
  {
    launch(mf_smoother_mode(x_prev, alpha), {x, b, x_prev, alpha, beta, out});
  }

  // The same operations on a region of the tiles (a box decomposition overlaps its exchange with the tiles that read no ghost
  // plane along any axis).  tiling: n_tiles / rows per axis -- column tiles of rows[0] DoF columns, y-tiles of rows[1] DoF rows,
  // z-tiles of rows[2] layers; tile t of an axis owns [t rows, (t + 1) rows) and reads one plane below and above.  The columns
  // of a nearly empty last chunk are not part of the column tiles (MfTileRegion: tail_part).  An empty region launches nothing.
  void tiling(int n_tiles[3], int rows[3]) const;
  bool has_tail() const { return _tail != nullptr; }
  void launch_region(MfMode mode, MfOperands<T> const &v, MfTileRegion const &region) const;

  // Several smoother terms in ONE sweep (mf_cheb_fused.hip): x_1 = x - beta[0] dinv (A x - b), then
  // x_s = x_{s-1} + alpha[s-1] (x_{s-1} - x_{s-2}) - beta[s-1] dinv (A x_{s-1} - b) up to s = n_terms (2 or 3); out = x_{n_terms},
  // out_prev (may be null) = x_{n_terms - 1}.  The same bits as n_terms calls of smoother_step.  alpha[0] must be zero; out,
  // out_prev and x must be three different vectors.  Available for the cell-constant layout with a numbering the kernel can
  // compute on one rank (fused_sweep_available); callers fall back to smoother_step otherwise.
  bool fused_sweep_available(int n_terms) const;
  // ... and from x_0 = 0 without reading it (smoother_sweep with x == nullptr: the pre-smoother of a preconditioner application)
  bool fused_zero_guess_available(int n_terms) const;
  // the last chunk column owns at most 32 - 2 halo DoF columns: the sweep kernels of the default tile shapes (three terms 8 x 3
  // rows, two terms 4 x 4) run it two y-tiles per workgroup, one per half of the wavefront
  bool narrow_last_column() const { return _narrow_last; }
  static constexpr bool fused_narrow_capable(int n_terms, int ty, int nw = 8)
  {
    return (n_terms == 3 && ty == 3 && nw <= 8) || (n_terms == 2 && ty == 4 && nw <= 8) || (n_terms == 3 && ty == 2 && nw == 12);
  }
  void smoother_sweep(int n_terms, T const *alpha, T const *beta, T const *b, T const *x, T *out, T *out_prev) const;
  // tile of the sweep: nw wavefronts of ty cell rows, tz owned layers (0, 0, 0: chosen from the mesh)
  void set_fused_tile(int nw, int ty, int tz)
  {
    _fused_tile[0] = nw;
    _fused_tile[1] = ty;
    _fused_tile[2] = tz;
  }
  void get_fused_tile(int n_terms, int &nw, int &ty, int &tz) const { choose_fused_tile(n_terms, nw, ty, tz); }
  int halo_lanes() const { return _halo; }
  // the sweep's cell kernel: mode space (default: ~30 % fewer FP64 operations, its own rounding) or the arithmetic of the
  // one-term kernel (the sweep is then bit-identical to smoother_step after smoother_step)
  void set_fused_reference(bool on) { _fused_reference_arithmetic = on; }
  bool fused_reference() const { return _fused_reference_arithmetic; }
  // bytes one sweep of n_terms must move at least: x_0, b, one coefficient per cell (D^-1 where the records hold it), x_K
  double fused_sweep_bytes(bool with_prev) const { return double(_n_dofs) * sizeof(T) * (4. + (_dinv_in_record ? 1. : 0.) + (with_prev ? 1. : 0.)); }

  T const *diagonal() const { return _diag.data(); }
  T const *diagonal_inverse() const { return _dinv.data(); }

  // D^-1 of the twelve-wavefront sweep as a vector in the operator's numbering: 1 / (kd * sum of the coefficients of the
  // eight cells of a DoF), the bits the sweep and the one-term kernel derive on the fly (mf_laplace.hip: mf_sweep_dinv_kernel;
  // Dirichlet DoFs hold that value too, the kernels take 1 there).  Built once, at construction, for the FP64 operators that
  // can take that sweep (one coefficient per cell, computed ids, three halo lanes, no D^-1 in the records) unless
  // MFMG_MF_SWEEP_DINV=derived; nullptr where it does not exist.  The sweep reads it where it exists and set_sweep_diagonal
  // has not said otherwise: 8 B/DoF more to read, a division and the coefficient sums less to compute per DoF and launch.
  T const *sweep_diagonal_inverse() const { return _sweep_dinv.data(); }
  bool sweep_diagonal_stored() const { return _sweep_dinv_read; }
  void set_sweep_diagonal(bool stored)
  {
    ASSERT_THROW(!stored || _sweep_dinv.size() > 0, "this operator holds no D^-1 vector of the sweep");
    _sweep_dinv_read = stored;
  }

  // tile of one workgroup: n_waves wavefronts of ty cell rows each, tz layers (0 = chosen from the mesh size)
  void set_tile(int ty, int tz)
  {
    _tile_y = ty;
    _tile_z = tz;
  }
  void set_tile_waves(int nw) { _tile_waves = nw; }
  // the tile the next launch uses
  void get_tile(int &nw, int &ty, int &tz) const
  {
    const MfTile t = choose_tile();
    nw = t.nw;
    ty = t.ty;
    tz = t.tz;
  }
  HipHandle &handle() const { return _handle; }

  // The operations of `launch` on a block of vectors (mf_laplace_block.hip): the block is cut by mf_block_groups, groups of
  // 4 and 2 columns run mf_laplace_block_kernel (FP64) or mf_laplace_block_f32_kernel (FP32) -- one read of the chunk records for
  // all columns of the group --, a single column runs the one-vector kernel.  Every column gets the bits of the one-vector launch.  Operators without the block
  // kernel (block_kernel_available: the cell-constant layout, whose sweep has no record bytes worth sharing; dim = 2; a tail
  // slab) run column by column.  InvalidArgumentExc: n_vectors outside 1 .. 64, ld < n_dofs or odd, a base not aligned to 16
  // bytes (FP32: 8), the out block overlapping the x block, a null operand the mode reads, a context with a communicator.
  void launch_block(MfMode mode, MfBlockOperands<T> const &v) const;
  // ... the same launches on this rank's local mesh for a caller that has refreshed the ghost entries of the x block itself
  // (HipMatrixFreeOperator::apply_mode_block on a communicator: one exchange_block, then this).  The checks of launch_block but
  // the refusal of a communicator; no exchange.
  void launch_block_local(MfMode mode, MfBlockOperands<T> const &v) const;
  bool block_kernel_available() const;
  // tile of the block kernel (0, 0, 0: chosen from the mesh and the width of the group); ty = 2, 3 or 4
  void set_block_tile(int nw, int ty, int tz)
  {
    _block_tile[0] = nw;
    _block_tile[1] = ty;
    _block_tile[2] = tz;
  }
  void get_block_tile(int nv, int &nw, int &ty, int &tz) const;
  // launches of the block kernel so far
  int64_t block_launches() const { return _block_launches; }
  // Several ranks: the widest group ALL ranks run as one launch (4, or 1: every rank loops over the columns), agreed once where
  // the fine smoother is built (HipSmoother) from what every rank's operator offers; 0 until then.  A rank that looped over
  // columns while its neighbour sent one block message would leave both waiting, so nothing on ranks asks
  // block_kernel_available() again.
  void set_block_width_agreed(int width) { _block_width_agreed = width; }
  int block_width_agreed() const { return _block_width_agreed; }

  // Bytes of one operator application y = A x.
  // survey: the indexed form of SURVEY.md 8(d) -- x, y, 8 index ints, 8 coefficients (112 B/DoF in FP64; one
  //         coefficient per cell: 56);
  // required: what the chunk-record layout makes the kernel move at least -- x, y, ONE id (each slot stores its own
  //         DoF id, the other seven corners are neighbours' own ids) and the coefficients (84 / 28 B/DoF in FP64);
  //         halo re-reads of the tiling are not in this figure.
  double survey_bytes_apply() const
  {
    return double(_n_dofs) * (2.0 * sizeof(T) + 8 * 4 + (_compact ? 1 : 8) * sizeof(T));
  }
  // (ids: 4 bytes per DoF from the records; none where the kernel computes them, AffineIds)
  double required_bytes_apply() const
  {
    return double(_n_dofs) * (2.0 * sizeof(T) + (ids_computed() ? 0. : 4.) + (_compact ? 1 : 8) * sizeof(T));
  }
  // Used by the eight-coefficient kernels only (measured at 257^3 / 512^3 DoFs, Chebyshev(3) apply: 1.35 -> 1.27 ms and
  // 9.5 -> 9.0 ms; the one-coefficient kernels prefetch their ids a layer ahead and LOSE 3 % to the extra arithmetic).
  // Both parts of a launch (the mesh and the rotated slab of its tail columns) must have such a numbering.
  bool ids_computed() const { return !_compact && _affine_ids && (!_tail || _tail->_affine_ids); }
  // bytes of the epilogue operands of a fused mode on top of that: b, then D^-1 (NOT read in the cell-constant layout:
  // the kernel derives it from the cell coefficients), then x_prev
  double epilogue_bytes(int mode) const
  {
    const double w = sizeof(T) * double(_n_dofs);
    return mode == 0 ? 0. : mode == 1 ? w : (mode == 2 ? 1. : 2.) * w + (_dinv_in_record ? w : 0.);
  }

private:
  void launch(MfMode mode, MfOperands<T> const &v) const { launch_region(mode, v, MfTileRegion::whole()); }
  void run(MfMode mode, MfOperands<T> const &v, MfTile const &tile, MfTileRegion const &region) const;
  // every tile of this part (the mesh, or the slab of its tail columns) over the z-tiles of `ztab`
  void make_args(MfArgs<T> &a, MfMode mode, MfOperands<T> const &v, MfTile const &tile, int const *ztab, int all_z) const;
  // share of the DoFs the region updates (for the profiler's bytes)
  double dof_share(MfTileRegion const &region, int const n_tiles[3], int const rows[3]) const;
  // layers of the z-tiles (device table, built once per tz): graded = shorter tiles at the end of every XCD's run
  int const *z_tiling(int tz, bool graded, int &n_tiles) const;
  struct ZTiling
  {
    int tz = 0, n_tiles = 0;
    DeviceBuffer<int> dev;
  };
  mutable ZTiling _zt_uniform, _zt_graded;
  void check_vectors(MfMode mode, MfOperands<T> const &v) const;
  // dim = 2 (mf_laplace.hip): a plain owner-computes kernel on the caller's arrays
  void init_2d(mfmg_hip_mesh_desc const &mesh);
  void launch_2d(MfMode mode, MfOperands<T> const &v) const;
  int _dim = 3;
  DeviceBuffer<int32_t> _cd2, _node_dof2;
  DeviceBuffer<T> _co2;
  DeviceBuffer<uint8_t> _cn2;
  double _k2[64] = {};
  MfTile choose_tile() const;
  MfTile choose_block_tile(int nv) const;
  void run_block(MfMode mode, MfBlockOperands<T> const &v, int nv) const;
  int _block_tile[3] = {0, 0, 0};
  mutable int64_t _block_launches = 0;
  int _block_width_agreed = 0;
  void choose_fused_tile(int n_terms, int &nw, int &ty, int &tz) const;
  bool fused_wg12_capable(int n_terms) const; // the sweep has the kernel of twelve wavefronts of two rows
  // the sweep of that shape runs mf_cheb_fused_uniform_kernel, whose wavefronts hold three node rows of their own: 30 owned rows
  // per y-tile, not 19 (asked at every call: MFMG_MF_UNIFORM_SWEEP is read anew)
  bool uniform_disjoint_rows(int n_terms, int nw, int ty) const;
  int fused_tile_owned_rows(int n_terms, int nw, int ty) const;
  int _fused_tile[3] = {0, 0, 0};
  bool _fused_reference_arithmetic = false;

  HipHandle &_handle;
  int _N[3]; // DoF grid
  int _n[3]; // cells
  double _h[3];
  int64_t _n_dofs;
  // internal layout (mf_laplace.hip): rows cut into aligned chunks of 64 cell slots (62 owned DoFs + the
  // halo cell); one record per chunk with the b=1 face ids, the coefficients and D^-1, plus the b=0 face ids
  int _ncols = 0;
  bool _narrow_last = false; // (see narrow_last_column)
  int _own = 62, _halo = 1; // chunk c holds the node columns _own c - _halo + lane and owns its lanes [_halo, _halo + _own)
  size_t _n_slots = 0;
  // columns of a nearly empty last chunk, as a slab operator with x and y exchanged (mf_laplace.hip)
  std::unique_ptr<MatrixFreeLaplaceDevice<T>> _tail;
  DeviceBuffer<unsigned char> _rec;
  DeviceBuffer<T> _diag, _dinv;
  DeviceBuffer<T> _sweep_dinv; // (see sweep_diagonal_inverse)
  bool _sweep_dinv_read = false;
  bool _uniform = false; // (see uniform_coefficient)
  double _uniform_coef = 0.;
  mutable int64_t _uniform_sweeps = 0;
  int _tile_y = 0, _tile_z = 0, _tile_waves = 0;
  bool _compact = false;
  bool _dinv_in_record = true; // D^-1 is part of the chunk records (always for eight coefficients per cell)
  size_t _rec_bytes = 0;
  // a numbering the kernel computes instead of reading it from the records (mf_laplace.hip: AffineIds)
  AffineIds _affine = {0, 1, 0, 0, 0, {0, 0, 0}, {0, 0, 0}};
  bool _affine_ids = false;
};
} // namespace mfmg
