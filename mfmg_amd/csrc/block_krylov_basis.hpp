// Orthogonalisation against the Krylov bases of a block of right-hand sides (mfmg_hip_hierarchy_solve_fgmres_block), FP64.
//
// Every column of a block solve owns a SLOT.  The working blocks are column-major with an even leading dimension ld and a base
// aligned to 16 bytes; basis vector j of slot s lives at V + (j * k + s) * ld (k = the slots of the solve), Z likewise.  For a
// fixed j the slots are ld apart -- a block that Hierarchy::apply_block and Operator::apply_block take --, for a fixed slot the
// basis vectors are ldv = k * ld apart: the leading dimension the bodies of krylov_basis_bodies.hpp see.  One launch runs one pass
// of the one-vector driver over all LIVE slots, the slot as one more grid dimension; a slot gets the bits of the one-vector kernel
// (16-byte accesses, W = 2: the same entries per thread, the same grid of reduction_blocks(n) in x, the same order of every sum):
//   dots           h[s][i] = (V_i of slot s, w_s), i = 0 .. j; partials [slot][column][block], one finish launch for all
//   update         w_s -= sum c[s][i] V_i (one fma per term); with_norm: the partials of ||w_s||^2 per slot [slot][kMaxBlocks]
//   norm_partials  those partials without touching w (the residual that starts a cycle)
//   scale_store    v_next_s = w_s / ||w_s|| (zero norm: zeros), the norm to device memory, an optional float copy
//   combine        x_col(s) += sum y[s][i] Z_i of slot s; x is the caller's block (own leading dimension, 8-byte alignment is
//                  enough: elementwise, the access width does not change a bit)
// The live slots are a by-value list (SlotList): slots that are not in it are neither read nor written.  Coefficients stay in
// device memory, `cstride` doubles per slot.  No atomics: results do not depend on scheduling.  All launches go to the handle's
// stream.
//
// Several ranks: the overloads that take a krylov::OwnedBox run the same passes over the entries the rank OWNS of its local
// vectors (V.n = box.n_local()).  A slot gets the bits of the one-vector owned-box kernel of krylov_basis.hpp -- its bodies, its
// grid in x (krylov::reduction_blocks(box)), its assignment of owned entries to threads, its order of every sum.  What the ghost
// entries of V and w or the padding between the columns hold never enters a result, the ghost entries of w and v_next are not
// written.  The sum over the ranks lies between the launches, with the caller, and takes ALL live slots in one message, so what
// crosses the ranks is PACKED in the order of the list: entry i of the list has its j + 1 coefficients of a pass at
// scratch.pass_coefficients + i * n_columns and its ||w||^2 at scratch.norm_squared + i.  The walk over the rows of the box runs in
// 32-bit integers where the local vector is shorter than 2^31 entries, in 64-bit ones otherwise.
#pragma once

#include "krylov_basis.hpp"

namespace mfmg
{
namespace block_krylov_basis
{
constexpr int kMaxSlots = 64;

// the slots of a launch, in the order of the grid's slot dimension (with `col`: the column of the caller's x of each)
struct SlotList
{
  int32_t count = 0;
  int32_t id[kMaxSlots];
  int32_t col[kMaxSlots];
};

// What the launches write between them, for `slots` slots and bases of up to `columns` vectors: the partials of the dots
// [slot][column][block], of the norms [slot][kMaxBlocks], the coefficients of one pass [slot][columns].  It allocates.
struct Scratch
{
  Scratch(int slots, int columns)
      : slots(slots), columns(columns), dot_partials((size_t)slots * columns * krylov::kMaxBlocks),
        norm_partials((size_t)slots * krylov::kMaxBlocks), pass_coefficients((size_t)slots * columns), norm_squared((size_t)slots)
  {
  }
  int slots, columns;
  DeviceBuffer<double> dot_partials, norm_partials, pass_coefficients;
  DeviceBuffer<double> norm_squared; // owned-box launches: ||w_s||^2 per entry of the list, of this rank (norm_finish), then of all ranks
};

// One block of basis vectors: vector i of slot s at base + i * ldv + s * ld
struct Basis
{
  int64_t n, ld, ldv;
  double *base;
  double *vector(int i, int s = 0) const { return base + (int64_t)i * ldv + (int64_t)s * ld; }
};

// h_pass[s * scratch.columns + i] = (V_i of slot s, w_s) for i < n_columns and every live s, w_s = w + s * ld;
// h_total[s * cstride + i] = that (accumulate == false) or += that
void dots(HipHandle &h, Scratch &s, SlotList const &live, Basis const &V, int n_columns, double const *w, double *h_total, int64_t cstride,
          bool accumulate);
// w_s -= sum_i c[s * scratch.columns + i] V_i of slot s (c = scratch.pass_coefficients); with_norm: the partials of ||w_s||^2
void update(HipHandle &h, Scratch &s, SlotList const &live, Basis const &V, int n_columns, double *w, bool with_norm);
void norm_partials(HipHandle &h, Scratch &s, SlotList const &live, int64_t n, int64_t ld, double const *w);
// v_next_s = w_s / ||w_s|| from the partials of slot s (v_next == w: in place; nullptr: the norm alone); v_next_f32 (may be null):
// the narrowed copy, slot s at v_next_f32 + s * ld; norm_out[s * norm_stride] = ||w_s||
void scale_store(HipHandle &h, Scratch &s, SlotList const &live, int64_t n, int64_t ld, double const *w, double *v_next, float *v_next_f32,
                 double *norm_out, int64_t norm_stride);
// ---- the same over the owned entries of a rank's local vectors (V.n == box.n_local()); i = the position of slot s in the list ----
// scratch.pass_coefficients[i * n_columns + l] = this rank's part of (V_l of slot s, w_s); h_total (may be null):
// h_total[s * cstride + l] = that or += that
void dots(HipHandle &h, Scratch &s, SlotList const &live, krylov::OwnedBox const &box, Basis const &V, int n_columns, double const *w,
          double *h_total, int64_t cstride, bool accumulate);
// the owned entries of w_s -= sum_l scratch.pass_coefficients[i * n_columns + l] V_l of slot s (the coefficients of ALL ranks: the
// caller summed them); with_norm: the partials of ||w_s||^2 over the owned entries
void update(HipHandle &h, Scratch &s, SlotList const &live, krylov::OwnedBox const &box, Basis const &V, int n_columns, double *w,
            bool with_norm);
void norm_partials(HipHandle &h, Scratch &s, SlotList const &live, krylov::OwnedBox const &box, int64_t ld, double const *w);
// scratch.norm_squared[i] = the sum of the partials of slot s in a fixed order: this rank's part of ||w_s||^2, contiguous over the
// list -- one copy and one all-reduce take all live slots
void norm_finish(HipHandle &h, Scratch &s, SlotList const &live, krylov::OwnedBox const &box);
// the owned entries of v_next_s = w_s / sqrt(norm_squared[i]) (device scalars: ||w_s||^2 over ALL ranks); norm_out (may be null):
// norm_out[s * norm_stride] = the root.  Zero stores zeros; v_next == nullptr: the roots alone.
void scale_store(HipHandle &h, SlotList const &live, krylov::OwnedBox const &box, int64_t ld, double const *norm_squared, double const *w,
                 double *v_next, double *norm_out, int64_t norm_stride);

// x_{live.col[i]} += sum_l y[s * ystride + l] Z_l of slot s = live.id[i]; column c of x at x + c * ldx (several ranks: over all
// local entries, as the one-vector driver runs krylov::basis_combine there)
void combine(HipHandle &h, SlotList const &live, Basis const &Z, int n_columns, double const *y, int64_t ystride, double *x, int64_t ldx);

// The plan of one step of the block driver (host only).  Of k slots those with live[s] != 0 work on; slot_col[s] is the column
// of slot s.  Runs: the maximal runs of consecutive live slots in ascending order, run r = the slots [run_start[r],
// run_start[r] + run_width[r]) -- what one call of apply_block takes --, cut into run_groups[r] launches whose widths
// (mf_block_groups of the run's width) follow each other in group_width.  packed_col: the columns of the live slots in the order
// of their slots -- the slot -> column map of the next restart cycle, whose live slots are the first n_packed.  Every output
// holds up to k entries.  Returns the number of runs.
int plan(int k, int32_t const *live, int32_t const *slot_col, int32_t *run_start, int32_t *run_width, int32_t *run_groups,
         int32_t *group_width, int32_t *n_groups, int32_t *packed_col, int32_t *n_packed);
} // namespace block_krylov_basis
} // namespace mfmg
