// Vector kernels of preconditioned CG on a block of right-hand sides (mfmg_hip_hierarchy_solve_cg_block), FP64.
//
// A block is column-major with an even leading dimension ld and a base aligned to 16 bytes; the columns a solve still works on sit
// in the first `k` SLOTS of the working blocks r, z, p, A p.  grid.y is the slot, grid.x the entries: every pass of the one-vector
// driver (vec::dot_async, vec::cg_direction, vec::cg_update) runs ONCE over all active slots.  Every slot gets the bits of the
// one-vector kernels:
//   dots          out[s] = (X_s, Y_s): the two stages of vec::dot_async per slot -- the grid of n_blocks_for(n, 256, 1024) blocks in x,
//                 the same grid-stride assignment of entries to threads, the same wavefront butterfly, the same serial sum over the
//                 wavefronts, the same second stage over the partials (one launch for all slots).  16 B per entry and slot.
//   cg_direction  P_s = Z_s + (rz_new[s] / rz_old[s]) P_s, a zero divisor gives beta = 0 (vec::cg_direction); `first`: P_s = Z_s.
//                 24 B per entry and slot.
//   cg_update     alpha_s = rz[s] / pap[s] (zero divisor: 0); X_col(s) += alpha_s P_s, R_s -= alpha_s AP_s, and IN THE SAME PASS
//                 the stage-1 partials of (R_s, R_s) of the new R.  It runs in the geometry of dots, so a thread accumulates exactly
//                 the entries, in the order, the first stage of a dot over R would give it: rr_out[s] has the bits of the third dot
//                 of the one-vector driver, which is not launched.  X is the caller's block with its own leading dimension ldx,
//                 col(s) the column of slot s there (a small device array): x never moves when slots do.  48 B per entry and slot.
// Scalars are read from and written to device memory; partials are k x kReduceBlocks doubles of the caller.  No atomics: the
// results do not depend on scheduling.  All launches go to the handle's stream.
//
// Several ranks (mfmg_hip_hierarchy_solve_cg_block on a context with a communicator): the blocks hold the ranks' LOCAL vectors, ghost
// entries included.  Direction and update run over all local entries, as p.sadd, x.add and r.add of the one-vector driver do there
// (cg_direction_local: the two roundings of sadd; cg_update_local: the update without the folded reduction, whose grid would not
// be that of the owned entries).  The three reductions run over the entries the rank OWNS (krylov::OwnedBox):
//   dots (box)    out[s] = the part of (X_s, Y_s) over the owned entries, formed in the order distributed_dot forms it: the owned
//                 entries in packed order (x fastest, then y, then z; a slab's contiguous run) on the grid of vec::dot_async for
//                 n_owned entries, the same two stages -- without packing them first.  A slot has the bits of the one-vector
//                 rank-local sum; what the ghost entries hold never enters it.  16 B per owned entry and slot.
// The sum over the ranks lies with the caller: the live slots' values go to the host, through ONE all-reduce of the registered
// transport, and back.  Every rank then holds the same scalars and retires the same columns.  A slot equals the one-vector
// distributed solve bit for bit where the transport sums an element in the same order whatever the length of the message: any
// transport on two ranks (one addition per element), a host transport that adds the ranks' values in rank order.  (numpy.sum over
// eight mailbox slots is not one: it adds eight 1-long messages pairwise and eight 4-long ones row by row.)
#pragma once

#include "common.hpp"
#include "krylov_basis.hpp"

namespace mfmg
{
namespace block_krylov
{
constexpr int kReduceBlocks = 1024; // partials per slot: the reduction grid of vec::dot_async

// blocks in x of the reduction grid for vectors of n entries (a function of n alone)
unsigned int reduction_blocks(int64_t n);

void dots(HipHandle &h, int64_t n, int k, int64_t ld, double const *X, double const *Y, double *partials, double *out);
void cg_direction(HipHandle &h, int64_t n, int k, int64_t ld, double const *Z, double *P, double const *rz_new, double const *rz_old,
                  bool first);
void cg_update(HipHandle &h, int64_t n, int k, int64_t ld, double const *P, double const *AP, double *R, int64_t ldx, double *X,
               int32_t const *slot_col, double const *rz, double const *pap, double *partials, double *rr_out);

// ---- the forms of a rank's local vectors (X, Y, ...: blocks of whole local vectors, ld >= box.n_local()) ----
unsigned int reduction_blocks(krylov::OwnedBox const &box);
void dots(HipHandle &h, krylov::OwnedBox const &box, int k, int64_t ld, double const *X, double const *Y, double *partials, double *out);
// P_s = round(beta_s P_s) + Z_s: the two roundings of p.sadd(beta, 1., z), which is how the one-vector driver forms the direction
// on several ranks (cg_direction above is the one fma of vec::cg_direction, the one-rank driver's)
void cg_direction_local(HipHandle &h, int64_t n, int k, int64_t ld, double const *Z, double *P, double const *rz_new, double const *rz_old,
                        bool first);
void cg_update_local(HipHandle &h, int64_t n, int k, int64_t ld, double const *P, double const *AP, double *R, int64_t ldx, double *X,
                     int32_t const *slot_col, double const *rz, double const *pap);

// Which slots move when some of the n_active slots retire (host only): the active slots stay contiguous.  Retired slots are
// filled in ascending order, each from the last slot that survives behind it: moves[2 i], moves[2 i + 1] = from, to (the caller
// copies r and p; z and A p are recomputed), slot_col[to] = slot_col[from].  At most one move per retired slot.  Returns the
// number of moves; n_active_out slots are left, slot_col beyond them is meaningless.
int plan_retire(int n_active, int32_t const *retire_flags, int32_t *slot_col, int32_t *moves, int *n_active_out);
} // namespace block_krylov
} // namespace mfmg
