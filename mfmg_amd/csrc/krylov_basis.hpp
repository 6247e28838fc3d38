// Orthogonalisation against a growing Krylov basis, fused (flexible GMRES, mfmg_hip_hierarchy_solve_fgmres).
//
// The basis V[ld x (m + 1)] and the preconditioned vectors Z[ld x m] are column-major, `ld` = n rounded up so that every column is
// 16-byte aligned (KrylovBasis::leading_dimension).  Run as BLAS-1 calls, step j of the Arnoldi process costs j dot launches and
// j axpy launches and reads w 2 j times; here
//   dots        h[i] = (V_i, w), i = 0 .. j:  w is read once per 8 columns, every V_i once
//   update      w -= sum h[i] V_i, and the partial sums of ||w||^2 of the updated w: w read once and written once, every V_i once
//   scale_store V_next = w / ||w|| (and its narrowed float copy, the input of an FP32 preconditioner): finishes the norm itself
//   combine     x += sum y[i] Z_i in one pass
// Coefficients and norms stay in device memory.  Reductions are two-stage on a fixed grid, the partials summed in a fixed order:
// no atomics, two runs give the same bits (as vec::dot_async).  All launches go to the handle's stream.
//
// Several ranks: a rank's vectors carry ghost entries, and a dot product runs over the entries the rank OWNS -- a sub-box of its
// local box of nodes (OwnedBox; a slab owns a contiguous run) -- and is then summed over the ranks.  The overloads that take an
// OwnedBox keep every property above over the owned entries alone: what the ghost entries of V, w and Z hold never enters a
// result, the ghost entries of w are not written, the grid is a function of the box alone.  The sum over the ranks lies between
// the launches, with the caller: the coefficients of a pass go to the host, through one all-reduce and back in front of the
// update, and scale_store takes the all-reduced ||w||^2 as a device scalar instead of finishing the partials of this rank.
#pragma once

#include "common.hpp"

namespace mfmg
{
namespace krylov
{
constexpr int kGroup = 8;          // columns whose loads one thread has in flight beside w
constexpr int kMaxBlocks = 1024;   // fixed upper bound of the reduction grid (partials per column)

inline int64_t leading_dimension(int64_t n) { return (n + 1) & ~int64_t(1); }

// The owned entries of a local vector: the nodes [own0, own0 + own_n) per axis (x fastest) of a lexicographic box of `local`
// nodes with `comps` entries per node (HaloSpace).  An axis that is owned whole joins the rows of the next one: a slab is one run.
struct OwnedBox
{
  int64_t local[3] = {0, 0, 0}, own0[3] = {0, 0, 0}, own_n[3] = {0, 0, 0};
  int comps = 1;
  OwnedBox() = default;
  explicit OwnedBox(HaloSpace const &s) : comps(s.comps)
  {
    for (int d = 0; d < 3; ++d)
    {
      local[d] = s.dim(d);
      own0[d] = s.own0(d);
      own_n[d] = s.own_n(d);
    }
  }
  int64_t n_local() const { return comps * local[0] * local[1] * local[2]; }
  int64_t n_owned() const { return comps * own_n[0] * own_n[1] * own_n[2]; }
};

// Scratch of the launches below for up to `max_columns` columns: partials of the dots [column][block], partials of the norm,
// the coefficients of one Gram-Schmidt pass.  Built outside the launch path (it allocates).
struct Scratch
{
  explicit Scratch(int max_columns)
      : capacity(max_columns), dot_partials((size_t)max_columns * kMaxBlocks), norm_partials(kMaxBlocks), pass_coefficients(max_columns),
        norm_squared(1)
  {
  }
  int capacity;
  DeviceBuffer<double> dot_partials, norm_partials, pass_coefficients;
  DeviceBuffer<double> norm_squared; // owned-box launches: ||w||^2, of this rank (basis_norm_finish), then of all ranks (the caller)
};

// blocks of the reduction grid for vectors of n entries (a function of n alone: the order of the partials is fixed)
unsigned int reduction_blocks(int64_t n);

// h_pass[i] = (V_i, w) for the n_columns columns of V; h_total[i] = h_pass[i] (accumulate == false) or += h_pass[i]
void basis_dots(HipHandle &h, Scratch &s, int64_t n, int64_t ld, int n_columns, double const *V, double const *w, double *h_pass,
                double *h_total, bool accumulate);
// w -= sum_i c[i] V_i (c on the device); with_norm: s.norm_partials receives the partial sums of ||w||^2 of the updated w
void basis_update(HipHandle &h, Scratch &s, int64_t n, int64_t ld, int n_columns, double const *V, double const *c, double *w,
                  bool with_norm);
// partial sums of ||w||^2 into s.norm_partials without touching w (the residual that starts a restart cycle)
void basis_norm_partials(HipHandle &h, Scratch &s, int64_t n, double const *w);
// v_next = w / ||w|| with ||w||^2 = the sum of s.norm_partials (v_next == w: in place); v_next_f32 (may be null) receives the
// narrowed copy; norm_out[0] = ||w||.  ||w|| == 0 stores zeros: nothing is divided by zero.  v_next == nullptr: the norm alone.
void basis_scale_store(HipHandle &h, Scratch &s, int64_t n, double const *w, double *v_next, float *v_next_f32, double *norm_out);

// ---- the same over the owned entries of a rank's vectors (V, w, v_next: whole local vectors of box.n_local() entries) ----
unsigned int reduction_blocks(OwnedBox const &box);
// h_pass[i] = the part of (V_i, w) over the owned entries, h_total as above
void basis_dots(HipHandle &h, Scratch &s, OwnedBox const &box, int64_t ld, int n_columns, double const *V, double const *w,
                double *h_pass, double *h_total, bool accumulate);
// the owned entries of w -= sum_i c[i] V_i, the ghost entries of w are left as they are; with_norm: the partial sums over the
// owned entries of the updated w
void basis_update(HipHandle &h, Scratch &s, OwnedBox const &box, int64_t ld, int n_columns, double const *V, double const *c,
                  double *w, bool with_norm);
void basis_norm_partials(HipHandle &h, Scratch &s, OwnedBox const &box, double const *w);
// s.norm_squared = the sum of s.norm_partials in a fixed order: this rank's part of ||w||^2, what the caller sums over the ranks
void basis_norm_finish(HipHandle &h, Scratch &s, OwnedBox const &box);
// the owned entries of v_next = w / sqrt(norm_squared[0]) (device scalar: ||w||^2 over ALL ranks); norm_out (may be null) receives
// the root.  Zero stores zeros; v_next == nullptr: the root alone.
void basis_scale_store(HipHandle &h, OwnedBox const &box, double const *norm_squared, double const *w, double *v_next,
                       double *norm_out);

// x += sum_i y[i] Z_i (y on the device)
void basis_combine(HipHandle &h, int64_t n, int64_t ld, int n_columns, double const *Z, double const *y, double *x);
} // namespace krylov
} // namespace mfmg
