// The Krylov drivers of the hierarchy -- preconditioned CG and right-preconditioned flexible GMRES, each for one right-hand side
// and for a block of them, on one rank and on several -- and the working sets they keep between solves.  Plain C++ behind the C
// boundary (c_api.cpp), which checks the caller's arguments, calls in here and maps the result to its out-parameters.  No kernel
// lives here: the drivers launch those of vector_ops, krylov_basis, block_krylov and block_krylov_basis.
#pragma once

#include <functional>
#include <memory>
#include <vector>

#include "block_krylov.hpp"
#include "block_krylov_basis.hpp"
#include "dof_permutation.hpp"
#include "fgmres_column.hpp"
#include "krylov_basis.hpp"
#include "mfmg/hierarchy.hpp"

namespace mfmg
{
// a pinned host allocation of doubles and its owner
struct PinnedFree
{
  void operator()(double *p) const { (void)hipHostFree(p); }
};
using PinnedDoubles = std::unique_ptr<double, PinnedFree>;
inline PinnedDoubles pinned_doubles(size_t bytes)
{
  void *p = nullptr;
  MFMG_HIP_CHECK(hipHostMalloc(&p, bytes));
  return PinnedDoubles(static_cast<double *>(p));
}

// The working sets below are grown on demand by reserve() and never shrunk.  Through reserve_or_empty an allocation that fails
// in there throws with the working set EMPTY (as constructed: no buffer, all sizes zero): the next solve allocates afresh, it never
// runs on a half-built working set.
template <typename Workspace, typename... Args>
void reserve_or_empty(Workspace &ws, Args &&...args)
{
  try
  {
    ws.reserve(std::forward<Args>(args)...);
  }
  catch (...)
  {
    ws = Workspace();
    (void)hipGetLastError(); // (the failed allocation is reported by the exception, not by the next launch check)
    throw;
  }
}

// What solve_fgmres keeps between solves: the basis V[ld x (columns + 1)], the preconditioned vectors Z[ld x columns]
// (krylov_basis.hpp), the float vectors around an FP32 preconditioner, the Hessenberg column / y on the device and their pinned
// host mirror: a solve allocates nothing once its restart length has been seen.
struct KrylovWorkspace
{
  int64_t ld = 0;
  int columns = 0;
  DeviceBuffer<double> V, Z, coefficients; // coefficients: [0, columns]: h_0 .. h_j, ||w||; [columns + 1, 2 columns]: y
  DeviceBuffer<float> v_f32, z_f32;
  std::unique_ptr<krylov::Scratch> scratch;
  PinnedDoubles host; // as `coefficients`
  void reserve(int64_t n, int m, bool fp32) // (the basis is 2 m + 1 fine vectors)
  {
    const int64_t want_ld = krylov::leading_dimension(n);
    if (want_ld != ld || m > columns)
    {
      MemoryKind kind("Krylov basis");
      *this = KrylovWorkspace(); // (before the larger one is allocated)
      V.resize((size_t)want_ld * (m + 1));
      Z.resize((size_t)want_ld * m);
      coefficients.resize((size_t)2 * m + 2);
      scratch.reset(new krylov::Scratch(m + 1));
      host = pinned_doubles(((size_t)2 * m + 2) * sizeof(double));
      ld = want_ld; // only now: everything above stands
      columns = m;
    }
    if (fp32 && (v_f32.size() != (size_t)ld || z_f32.size() != (size_t)ld))
    {
      MemoryKind kind("Krylov basis");
      v_f32.release();
      z_f32.release();
      v_f32.resize((size_t)ld);
      z_f32.resize((size_t)ld);
    }
  }
};

// What solve_cg_block keeps between solves: the working blocks r, z, p, A p [ld x columns], with "internal numbering" lexicographic
// the gathered b and x, the partials of the block reductions [columns x 1024], the per-slot scalars ((r, z) of this / the previous
// iteration, (p, A p), (r, r): four rows of `columns`), the slot -> column map and the pinned host mirror of the (r, r) and the map.
struct BlockCgWorkspace
{
  int64_t ld = 0;
  int columns = 0;
  bool permuted = false;
  DeviceBuffer<double> R, Z, P, AP, B, X, partials, scalars;
  DeviceBuffer<int32_t> slot_col;
  PinnedDoubles host; // `columns` doubles and behind them `columns` slot -> column entries
  int32_t *host_col() const { return reinterpret_cast<int32_t *>(host.get() + columns); }
  void reserve(int64_t want_ld, int k, bool permute, hipStream_t stream)
  {
    if (want_ld == ld && k <= columns && (!permute || permuted))
      return;
    MemoryKind kind("block CG working set");
    const int want = std::max(k, want_ld == ld ? columns : 0);
    *this = BlockCgWorkspace(); // (before the larger one is allocated)
    const size_t block = (size_t)want_ld * want;
    DeviceBuffer<double> *blocks[6] = {&R, &Z, &P, &AP, &B, &X};
    for (int i = 0; i < (permute ? 6 : 4); ++i)
    {
      blocks[i]->resize(block);
      // (zeros: the tails between the columns are never written, and a preconditioner that reads its start vector finds numbers)
      MFMG_HIP_CHECK(hipMemsetAsync(blocks[i]->data(), 0, block * sizeof(double), stream));
    }
    partials.resize((size_t)want * block_krylov::kReduceBlocks);
    scalars.resize((size_t)4 * want);
    slot_col.resize((size_t)want);
    host = pinned_doubles((size_t)want * (sizeof(double) + sizeof(int32_t)));
    ld = want_ld; // only now: everything above stands
    columns = want;
    permuted = permute;
  }
};

// What solve_fgmres_block keeps between solves, for `slots` columns and restart cycles of `columns` vectors: the bases
// V [(columns + 1) x slots x ld] and Z [columns x slots x ld] (block_krylov_basis.hpp), the float vectors around an FP32
// preconditioner [slots x ld] twice, with "internal numbering" lexicographic the gathered b and x, the scratch of the launches,
// per slot the Hessenberg column (columns + 1 doubles) and y (columns doubles) on the device and their pinned host mirror.
struct BlockFgmresWorkspace
{
  int64_t ld = 0;
  int slots = 0, columns = 0;
  bool permuted = false, fp32 = false;
  DeviceBuffer<double> V, Z, B, X, coefficients, y;
  DeviceBuffer<float> v_f32, z_f32;
  std::unique_ptr<block_krylov_basis::Scratch> scratch;
  PinnedDoubles host; // slots x (columns + 1) coefficients, then slots x columns entries of y
  double *host_y() const { return host.get() + (size_t)slots * (columns + 1); }
  void reserve(int64_t want_ld, int k, int m, bool permute, bool with_fp32, hipStream_t stream)
  {
    if (want_ld == ld && k <= slots && m <= columns && (!permute || permuted) && (!with_fp32 || fp32))
      return;
    MemoryKind kind("block FGMRES working set");
    const bool same = want_ld == ld;
    const int want_slots = std::max(k, same ? slots : 0), want_columns = std::max(m, same ? columns : 0);
    permute = permute || (same && permuted);
    with_fp32 = with_fp32 || (same && fp32);
    *this = BlockFgmresWorkspace(); // (before the larger one is allocated)
    const size_t block = (size_t)want_ld * want_slots;
    // (zeros: the tails between the columns are never written, and a cycle that reads its start vector finds numbers)
    auto zeros = [&](DeviceBuffer<double> &b, size_t count) {
      b.resize(count);
      MFMG_HIP_CHECK(hipMemsetAsync(b.data(), 0, count * sizeof(double), stream));
    };
    zeros(V, block * ((size_t)want_columns + 1));
    zeros(Z, block * (size_t)want_columns);
    if (permute)
    {
      zeros(B, block);
      zeros(X, block);
    }
    if (with_fp32)
    {
      v_f32.resize(block);
      z_f32.resize(block);
      MFMG_HIP_CHECK(hipMemsetAsync(v_f32.data(), 0, block * sizeof(float), stream));
      MFMG_HIP_CHECK(hipMemsetAsync(z_f32.data(), 0, block * sizeof(float), stream));
    }
    scratch.reset(new block_krylov_basis::Scratch(want_slots, want_columns + 1));
    coefficients.resize((size_t)want_slots * (want_columns + 1));
    y.resize((size_t)want_slots * want_columns);
    host = pinned_doubles((size_t)want_slots * (2 * (size_t)want_columns + 1) * sizeof(double));
    ld = want_ld; // only now: everything above stands
    slots = want_slots;
    columns = want_columns;
    permuted = permute;
    fp32 = with_fp32;
  }
};

// the working sets of the drivers of one hierarchy
struct KrylovWorkspaces
{
  KrylovWorkspace fgmres;
  BlockCgWorkspace block_cg;
  BlockFgmresWorkspace block_fgmres;
};

// the first `count` columns of a block as vectors (views)
struct BlockViews
{
  std::vector<DVector> store;
  std::vector<DVector *> ptr;
  std::vector<DVector const *> cptr;
  BlockViews(HipHandle &handle, int64_t n, int64_t ld, int count, double *base)
  {
    store.reserve(count);
    for (int c = 0; c < count; ++c)
    {
      store.emplace_back(handle, n, base + (int64_t)c * ld);
      ptr.push_back(&store.back());
      cptr.push_back(&store.back());
    }
  }
};

// the vectors of level `level` hold this many entries; block launches of the fine matrix-free operator so far
int64_t level_size(Hierarchy<DVector> const &hierarchy, int level);
int64_t block_kernel_launches(Hierarchy<DVector> const &hierarchy);

// What a solve runs on.  `perm` is set where the caller's numbering is not the one the hierarchy runs in ("internal numbering"
// lexicographic): b and x are then gathered once into library vectors, the whole iteration -- operator, preconditioner, the
// working vectors, the dot products -- runs in the internal numbering, and x is scattered once at the end, before a solve that did
// not converge is reported: two launches of the permutation per column and solve whatever the iteration count.  The one-vector
// drivers gather into `work`, the block drivers into B and X of their working set.
struct KrylovSetting
{
  HipHandle &handle;
  Hierarchy<DVector> &hierarchy;
  HipFloatFineLevel *fine_f32;  // "fine level precision" float, or null
  DofPermutation *perm;         // or null
  std::shared_ptr<TimerOutput> timer;
  double *work[2];              // with `perm`: two vectors of the fine level
  KrylovWorkspaces &workspaces;
  // An outer operator and its preconditioner z = M^-1 r from zero (mfmg/hip_high_order.hpp: the Q2 operator and the cycle around the
  // hierarchy), both or neither.  The one-vector drivers then iterate on them instead of the hierarchy's fine operator and cycle; the
  // block drivers and the FP32 preconditioner refuse them (NotImplementedExc).  Absent: every driver launches what it always did.
  std::shared_ptr<Operator<DVector> const> outer_operator = nullptr;
  std::function<void(DVector const &r, DVector &z)> outer_preconditioner = nullptr;
};

struct KrylovResult
{
  // per column (one entry from the one-vector drivers)
  std::vector<int32_t> iterations;
  std::vector<double> residuals;
  std::vector<char> converged;
  // block drivers: columns the preconditioner / the operator ran on, block kernel launches, slot moves (CG) / cycle starts (FGMRES:
  // residuals b - A x formed, the first one and one per restart / breakdown; from solve_fgmres too)
  int64_t work[4] = {0, 0, 0, 0};
  int64_t allreduces = 0; // several ranks: the all-reduces of the iteration (FGMRES: 3 per iteration, 1 per cycle start)
  // block FGMRES with the FP32 preconditioner: width, launches and looped columns of its applications
  int64_t block_info_f32[MFMG_HIP_BLOCK_INFO_FIELDS] = {1, 0, 0};
  explicit KrylovResult(int k) : iterations(k, 0), residuals(k, 0.), converged(k, 0) {}
  bool all_converged() const { return std::find(converged.begin(), converged.end(), 0) == converged.end(); }
};

// residual_history (or null) receives ||r|| of iteration it at [it], it < history_len; a block driver writes column c at
// [c history_ld + it].
KrylovResult solve_cg(KrylovSetting const &s, const double *b, double *x, double tolerance, int max_iterations, double *residual_history,
                      int history_len);
KrylovResult solve_cg_block(KrylovSetting const &s, int k, int64_t ld, const double *b, double *x, const double *tolerances,
                            int max_iterations, double *residual_history, int history_ld);
KrylovResult solve_fgmres(KrylovSetting const &s, const double *b, double *x, double tolerance, int max_iterations, int restart, bool fp32,
                          double *residual_history, int history_len);
KrylovResult solve_fgmres_block(KrylovSetting const &s, int k, int64_t ld, const double *b, double *x, const double *tolerances,
                                int max_iterations, int restart, bool fp32, double *residual_history, int history_ld);
} // namespace mfmg
