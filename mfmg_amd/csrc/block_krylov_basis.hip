// The orthogonalisation passes of flexible GMRES on a block of right-hand sides (block_krylov_basis.hpp).  Every kernel here is the
// body of its one-vector kernel (krylov_basis_bodies.hpp, shared with krylov_basis.hip) with the pointers of one slot: grid.x walks
// the entries exactly as there, the last grid dimension indexes the list of live slots.  Streaming kernels, wave64, 256 threads,
// 16-byte accesses; the loads of a group of kGroup = 8 basis vectors are issued before the first is used.
// The owned-box kernels (several ranks) wrap the owned-box bodies the same way: the grid in x and the walk over the rows of the box
// are those of the one-vector owned-box kernels (krylov_basis.hip, head comment), the walk in 32-bit integers where the local vector
// allows it.
#include "block_krylov_basis.hpp"

#include "krylov_basis_bodies.hpp"
#include "mf_laplace.hpp"

namespace mfmg
{
namespace block_krylov_basis
{
namespace
{
using namespace krylov::body;
using krylov::kGroup;
using krylov::kMaxBlocks;

// blockIdx.y: the group of kGroup columns, blockIdx.z: the live slot; partials[slot][column][block]
__global__ __launch_bounds__(block_size) void dots_kernel(SlotList live, int64_t n, int64_t ld, int64_t ldv, int n_columns,
                                                           int partial_columns, double const *__restrict__ V,
                                                           double const *__restrict__ w, double *__restrict__ partials)
{
  __shared__ double wsum[kGroup][kWaves];
  const int64_t s = live.id[blockIdx.z];
  const int c0 = blockIdx.y * kGroup;
  const int nc = min(kGroup, n_columns - c0);
  dots_group<2>(nc, n, ldv, V + s * ld + (int64_t)c0 * ldv, w + s * ld, partials + (s * partial_columns + c0) * gridDim.x, wsum);
}

// blockIdx.x: the column, blockIdx.y: the live slot
__global__ __launch_bounds__(block_size) void dots_finish_kernel(SlotList live, int n_partials, int partial_columns,
                                                                  double const *__restrict__ partials, double *__restrict__ h_pass,
                                                                  double *__restrict__ h_total, int64_t cstride, int accumulate)
{
  __shared__ double wsum[kWaves];
  const int64_t s = live.id[blockIdx.y], column = s * partial_columns + blockIdx.x;
  dots_finish_body(n_partials, partials + column * n_partials, h_pass + column, h_total + s * cstride + blockIdx.x, accumulate, wsum);
}

// the partials of ||w_s||^2: (w, w) of the dots body with w as its only column, as krylov::basis_norm_partials
__global__ __launch_bounds__(block_size) void norm_partials_kernel(SlotList live, int64_t n, int64_t ld, double const *__restrict__ w,
                                                                    double *__restrict__ norm_partials)
{
  __shared__ double wsum[kGroup][kWaves];
  const int64_t s = live.id[blockIdx.y];
  dots_group<2>(1, n, n, w + s * ld, w + s * ld, norm_partials + s * kMaxBlocks, wsum);
}

// W: the width of the accesses (1 where the caller's x is aligned to 8 bytes only); blockIdx.y: the live slot
template <int W, bool kNorm>
__global__ __launch_bounds__(block_size) void axpy_kernel(SlotList live, int64_t n, int64_t ld, int64_t ldv, int n_columns,
                                                           double const *__restrict__ V, double const *__restrict__ c, int64_t cstride,
                                                           double sign, double *__restrict__ out, int64_t ld_out, int out_by_column,
                                                           double *__restrict__ norm_partials)
{
  __shared__ double wsum[kWaves];
  const int64_t s = live.id[blockIdx.y], o = out_by_column ? live.col[blockIdx.y] : s;
  axpy_body<W, kNorm>(n, ldv, n_columns, V + s * ld, c + s * cstride, sign, out + o * ld_out, norm_partials + s * kMaxBlocks, wsum);
}

__global__ __launch_bounds__(block_size) void scale_store_kernel(SlotList live, int64_t n, int64_t ld, int n_partials,
                                                                  double const *__restrict__ partials, double const *w, double *v_next,
                                                                  float *__restrict__ v_next_f32, double *__restrict__ norm_out,
                                                                  int64_t norm_stride)
{
  __shared__ double wsum[kWaves];
  const int64_t s = live.id[blockIdx.y];
  scale_store_body<2>(n, n_partials, partials + s * kMaxBlocks, w + s * ld, v_next ? v_next + s * ld : nullptr,
                      v_next_f32 ? v_next_f32 + s * ld : nullptr, norm_out + s * norm_stride, wsum);
}

// ---- owned-box kernels: the owned-box bodies with the pointers of one slot; Index: the type the walk over the rows runs in ----
// blockIdx.y: the group of kGroup columns, blockIdx.z: the live slot; partials[slot][column][block]
template <typename Index>
__global__ __launch_bounds__(block_size) void box_dots_kernel(SlotList live, RowWalk walk, int64_t ld, int64_t ldv, int n_columns,
                                                               int partial_columns, double const *__restrict__ V,
                                                               double const *__restrict__ w, double *__restrict__ partials)
{
  __shared__ double wsum[kGroup][kWaves];
  const RowWalkT<Index> g(walk);
  const int64_t s = live.id[blockIdx.z];
  const int c0 = blockIdx.y * kGroup;
  const int nc = min(kGroup, n_columns - c0);
  box_dots_group<2>(nc, g, ldv, V + s * ld + (int64_t)c0 * ldv, w + s * ld, partials + (s * partial_columns + c0) * gridDim.x, wsum);
}

// blockIdx.x: the column, blockIdx.y: the live slot; the coefficients of the pass PACKED in the order of the list
__global__ __launch_bounds__(block_size) void box_dots_finish_kernel(SlotList live, int n_partials, int partial_columns, int n_columns,
                                                                      double const *__restrict__ partials, double *h_pass, double *h_total,
                                                                      int64_t cstride, int accumulate)
{
  __shared__ double wsum[kWaves];
  const int64_t s = live.id[blockIdx.y];
  double *const pass = h_pass + (int64_t)blockIdx.y * n_columns + blockIdx.x;
  dots_finish_body(n_partials, partials + (s * partial_columns + blockIdx.x) * n_partials, pass,
                   h_total ? h_total + s * cstride + blockIdx.x : pass, accumulate, wsum);
}

template <typename Index>
__global__ __launch_bounds__(block_size) void box_norm_partials_kernel(SlotList live, RowWalk walk, int64_t ld, double const *__restrict__ w,
                                                                        double *__restrict__ norm_partials)
{
  __shared__ double wsum[kGroup][kWaves];
  const RowWalkT<Index> g(walk);
  const int64_t s = live.id[blockIdx.y];
  box_dots_group<2>(1, g, ld, w + s * ld, w + s * ld, norm_partials + s * kMaxBlocks, wsum);
}

// blockIdx.x: the entry of the list; out[entry] = the partials of its slot in a fixed order
__global__ __launch_bounds__(block_size) void norm_finish_kernel(SlotList live, int n_partials, double const *__restrict__ norm_partials,
                                                                  double *out)
{
  __shared__ double wsum[kWaves];
  const int64_t s = live.id[blockIdx.x];
  dots_finish_body(n_partials, norm_partials + s * kMaxBlocks, out + blockIdx.x, out + blockIdx.x, 0, wsum);
}

// blockIdx.y: the live slot, its coefficients at c + blockIdx.y * n_columns
template <bool kNorm, typename Index>
__global__ __launch_bounds__(block_size) void box_axpy_kernel(SlotList live, RowWalk walk, int64_t ld, int64_t ldv, int n_columns,
                                                               double const *__restrict__ V, double const *__restrict__ c,
                                                               double *__restrict__ out, double *__restrict__ norm_partials)
{
  __shared__ double wsum[1][kWaves];
  const RowWalkT<Index> g(walk);
  const int64_t s = live.id[blockIdx.y];
  box_axpy_body<2, kNorm>(g, ldv, n_columns, V + s * ld, c + (int64_t)blockIdx.y * n_columns, -1., out + s * ld,
                          norm_partials + s * kMaxBlocks, wsum);
}

template <typename Index>
__global__ __launch_bounds__(block_size) void box_scale_store_kernel(SlotList live, RowWalk walk, int64_t ld,
                                                                      double const *__restrict__ norm_squared, double const *w, double *v_next,
                                                                      double *__restrict__ norm_out, int64_t norm_stride)
{
  const RowWalkT<Index> g(walk);
  const int64_t s = live.id[blockIdx.y];
  box_scale_store_body<2>(g, norm_squared + blockIdx.y, w + s * ld, v_next ? v_next + s * ld : nullptr,
                          norm_out ? norm_out + s * norm_stride : nullptr);
}

bool aligned16(void const *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the walk of an owned-box block launch (16-byte accesses) and whether it fits 32-bit integers
bool short_index(krylov::OwnedBox const &box) { return box.n_local() < (int64_t(1) << 31); }

void check_box(krylov::OwnedBox const &b, int64_t n, int64_t ld)
{
  ASSERT_THROW(b.comps >= 1, "block krylov basis: no component");
  for (int d = 0; d < 3; ++d)
    ASSERT_THROW(b.own0[d] >= 0 && b.own_n[d] >= 1 && b.own0[d] + b.own_n[d] <= b.local[d], "block krylov basis: the owned box leaves the local box");
  ASSERT_THROW(n == b.n_local() && ld >= n && ld % 2 == 0, "block krylov basis: the box does not describe the vectors of the block");
}

void check_list(SlotList const &live, int slots)
{
  ASSERT_THROW(live.count >= 1 && live.count <= kMaxSlots, "block krylov basis: a launch takes 1 to 64 live slots");
  for (int i = 0; i < live.count; ++i)
    ASSERT_THROW(live.id[i] >= 0 && live.id[i] < slots, "block krylov basis: a live slot outside the block");
}

void check_basis(Basis const &V, int n_columns)
{
  ASSERT_THROW(V.n >= 1 && n_columns >= 0 && V.ld >= V.n && V.ldv >= V.ld, "block krylov basis: bad shape");
  ASSERT_THROW(V.ld % 2 == 0 && V.ldv % 2 == 0 && aligned16(V.base), "block krylov basis: the working blocks are aligned to 16 bytes");
}
} // namespace

void dots(HipHandle &h, Scratch &s, SlotList const &live, Basis const &V, int n_columns, double const *w, double *h_total, int64_t cstride,
          bool accumulate)
{
  check_list(live, s.slots);
  check_basis(V, n_columns);
  if (n_columns == 0)
    return;
  ASSERT_THROW(n_columns <= s.columns && aligned16(w), "block krylov basis: more columns than the scratch was built for, or w not aligned");
  const unsigned int nb = krylov::reduction_blocks(V.n), n_groups = (unsigned)((n_columns + kGroup - 1) / kGroup);
  hipEvent_t stop = h.profiler.begin("block_basis_dots", 8. * double(V.n) * (n_columns + (int)n_groups) * live.count, h.stream);
  hipLaunchKernelGGL(dots_kernel, dim3(nb, n_groups, live.count), dim3(block_size), 0, h.stream, live, V.n, V.ld, V.ldv, n_columns, s.columns,
                     V.base, w, s.dot_partials.data());
  hipLaunchKernelGGL(dots_finish_kernel, dim3(n_columns, live.count), dim3(block_size), 0, h.stream, live, (int)nb, s.columns,
                     s.dot_partials.data(), s.pass_coefficients.data(), h_total, cstride, accumulate ? 1 : 0);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

void update(HipHandle &h, Scratch &s, SlotList const &live, Basis const &V, int n_columns, double *w, bool with_norm)
{
  check_list(live, s.slots);
  check_basis(V, n_columns);
  ASSERT_THROW(n_columns <= s.columns && aligned16(w), "block krylov basis: more columns than the scratch was built for, or w not aligned");
  const dim3 grid(krylov::reduction_blocks(V.n), live.count);
  hipEvent_t stop = h.profiler.begin("block_basis_update", 8. * double(V.n) * (n_columns + 2) * live.count, h.stream);
  if (with_norm)
    hipLaunchKernelGGL((axpy_kernel<2, true>), grid, dim3(block_size), 0, h.stream, live, V.n, V.ld, V.ldv, n_columns, V.base,
                       s.pass_coefficients.data(), (int64_t)s.columns, -1., w, V.ld, 0, s.norm_partials.data());
  else
    hipLaunchKernelGGL((axpy_kernel<2, false>), grid, dim3(block_size), 0, h.stream, live, V.n, V.ld, V.ldv, n_columns, V.base,
                       s.pass_coefficients.data(), (int64_t)s.columns, -1., w, V.ld, 0, s.norm_partials.data());
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

void norm_partials(HipHandle &h, Scratch &s, SlotList const &live, int64_t n, int64_t ld, double const *w)
{
  check_list(live, s.slots);
  ASSERT_THROW(n >= 1 && ld >= n && ld % 2 == 0 && aligned16(w), "block krylov basis: bad shape");
  hipLaunchKernelGGL(norm_partials_kernel, dim3(krylov::reduction_blocks(n), live.count), dim3(block_size), 0, h.stream, live, n, ld, w,
                     s.norm_partials.data());
  MFMG_HIP_CHECK(hipGetLastError());
}

void scale_store(HipHandle &h, Scratch &s, SlotList const &live, int64_t n, int64_t ld, double const *w, double *v_next, float *v_next_f32,
                 double *norm_out, int64_t norm_stride)
{
  check_list(live, s.slots);
  ASSERT_THROW(n >= 1 && ld >= n && ld % 2 == 0 && aligned16(w) && aligned16(v_next), "block krylov basis: bad shape");
  ASSERT_THROW((reinterpret_cast<uintptr_t>(v_next_f32) & 7u) == 0, "block krylov basis: the float block is aligned to 8 bytes");
  const int nb = (int)krylov::reduction_blocks(n);
  hipEvent_t stop =
      h.profiler.begin("block_basis_scale_store", v_next == nullptr ? 0. : double(n) * (16. + (v_next_f32 ? 4. : 0.)) * live.count, h.stream);
  hipLaunchKernelGGL(scale_store_kernel, dim3(v_next == nullptr ? 1u : (unsigned)nb, live.count), dim3(block_size), 0, h.stream, live, n, ld, nb,
                     s.norm_partials.data(), w, v_next, v_next_f32, norm_out, norm_stride);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

// ---- owned-box launches ---------------------------------------------------------------------------------------------------------
void dots(HipHandle &h, Scratch &s, SlotList const &live, krylov::OwnedBox const &box, Basis const &V, int n_columns, double const *w,
          double *h_total, int64_t cstride, bool accumulate)
{
  check_list(live, s.slots);
  check_basis(V, n_columns);
  check_box(box, V.n, V.ld);
  if (n_columns == 0)
    return;
  ASSERT_THROW(n_columns <= s.columns && aligned16(w), "block krylov basis: more columns than the scratch was built for, or w not aligned");
  const unsigned int nb = krylov::reduction_blocks(box), n_groups = (unsigned)((n_columns + kGroup - 1) / kGroup);
  const RowWalk g = row_walk(box, 2, nb);
  const dim3 grid(nb, n_groups, live.count);
  hipEvent_t stop = h.profiler.begin("block_basis_dots_box", 8. * double(box.n_owned()) * (n_columns + (int)n_groups) * live.count, h.stream);
  if (short_index(box))
    hipLaunchKernelGGL(box_dots_kernel<uint32_t>, grid, dim3(block_size), 0, h.stream, live, g, V.ld, V.ldv, n_columns, s.columns, V.base, w,
                       s.dot_partials.data());
  else
    hipLaunchKernelGGL(box_dots_kernel<int64_t>, grid, dim3(block_size), 0, h.stream, live, g, V.ld, V.ldv, n_columns, s.columns, V.base, w,
                       s.dot_partials.data());
  hipLaunchKernelGGL(box_dots_finish_kernel, dim3(n_columns, live.count), dim3(block_size), 0, h.stream, live, (int)nb, s.columns, n_columns,
                     s.dot_partials.data(), s.pass_coefficients.data(), h_total, cstride, accumulate ? 1 : 0);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

namespace
{
template <bool kNorm>
void launch_box_axpy(HipHandle &h, Scratch &s, SlotList const &live, krylov::OwnedBox const &box, Basis const &V, int n_columns, double *w)
{
  const unsigned int nb = krylov::reduction_blocks(box);
  const RowWalk g = row_walk(box, 2, nb);
  const dim3 grid(nb, live.count);
  if (short_index(box))
    hipLaunchKernelGGL((box_axpy_kernel<kNorm, uint32_t>), grid, dim3(block_size), 0, h.stream, live, g, V.ld, V.ldv, n_columns, V.base,
                       s.pass_coefficients.data(), w, s.norm_partials.data());
  else
    hipLaunchKernelGGL((box_axpy_kernel<kNorm, int64_t>), grid, dim3(block_size), 0, h.stream, live, g, V.ld, V.ldv, n_columns, V.base,
                       s.pass_coefficients.data(), w, s.norm_partials.data());
}
} // namespace

void update(HipHandle &h, Scratch &s, SlotList const &live, krylov::OwnedBox const &box, Basis const &V, int n_columns, double *w,
            bool with_norm)
{
  check_list(live, s.slots);
  check_basis(V, n_columns);
  check_box(box, V.n, V.ld);
  ASSERT_THROW(n_columns <= s.columns && aligned16(w), "block krylov basis: more columns than the scratch was built for, or w not aligned");
  hipEvent_t stop = h.profiler.begin("block_basis_update_box", 8. * double(box.n_owned()) * (n_columns + 2) * live.count, h.stream);
  if (with_norm)
    launch_box_axpy<true>(h, s, live, box, V, n_columns, w);
  else
    launch_box_axpy<false>(h, s, live, box, V, n_columns, w);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

void norm_partials(HipHandle &h, Scratch &s, SlotList const &live, krylov::OwnedBox const &box, int64_t ld, double const *w)
{
  check_list(live, s.slots);
  check_box(box, box.n_local(), ld);
  ASSERT_THROW(aligned16(w), "block krylov basis: bad shape");
  const unsigned int nb = krylov::reduction_blocks(box);
  const RowWalk g = row_walk(box, 2, nb);
  if (short_index(box))
    hipLaunchKernelGGL(box_norm_partials_kernel<uint32_t>, dim3(nb, live.count), dim3(block_size), 0, h.stream, live, g, ld, w,
                       s.norm_partials.data());
  else
    hipLaunchKernelGGL(box_norm_partials_kernel<int64_t>, dim3(nb, live.count), dim3(block_size), 0, h.stream, live, g, ld, w,
                       s.norm_partials.data());
  MFMG_HIP_CHECK(hipGetLastError());
}

void norm_finish(HipHandle &h, Scratch &s, SlotList const &live, krylov::OwnedBox const &box)
{
  check_list(live, s.slots);
  hipLaunchKernelGGL(norm_finish_kernel, dim3(live.count), dim3(block_size), 0, h.stream, live, (int)krylov::reduction_blocks(box),
                     s.norm_partials.data(), s.norm_squared.data());
  MFMG_HIP_CHECK(hipGetLastError());
}

void scale_store(HipHandle &h, SlotList const &live, krylov::OwnedBox const &box, int64_t ld, double const *norm_squared, double const *w,
                 double *v_next, double *norm_out, int64_t norm_stride)
{
  check_list(live, kMaxSlots);
  check_box(box, box.n_local(), ld);
  ASSERT_THROW(norm_squared != nullptr && aligned16(w) && aligned16(v_next), "block krylov basis: bad shape");
  const unsigned int nb = v_next == nullptr ? 1u : krylov::reduction_blocks(box);
  const RowWalk g = row_walk(box, 2, nb);
  hipEvent_t stop = h.profiler.begin("block_basis_scale_store_box", v_next == nullptr ? 0. : 16. * double(box.n_owned()) * live.count, h.stream);
  if (short_index(box))
    hipLaunchKernelGGL(box_scale_store_kernel<uint32_t>, dim3(nb, live.count), dim3(block_size), 0, h.stream, live, g, ld, norm_squared, w,
                       v_next, norm_out, norm_stride);
  else
    hipLaunchKernelGGL(box_scale_store_kernel<int64_t>, dim3(nb, live.count), dim3(block_size), 0, h.stream, live, g, ld, norm_squared, w,
                       v_next, norm_out, norm_stride);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

void combine(HipHandle &h, SlotList const &live, Basis const &Z, int n_columns, double const *y, int64_t ystride, double *x, int64_t ldx)
{
  check_list(live, kMaxSlots);
  check_basis(Z, n_columns);
  ASSERT_THROW(ldx >= Z.n, "block krylov basis: the leading dimension of x is smaller than the vectors");
  for (int i = 0; i < live.count; ++i)
    ASSERT_THROW(live.col[i] >= 0, "block krylov basis: a live slot without a column");
  if (n_columns == 0)
    return;
  const dim3 grid(krylov::reduction_blocks(Z.n), live.count);
  hipEvent_t stop = h.profiler.begin("block_basis_combine", 8. * double(Z.n) * (n_columns + 2) * live.count, h.stream);
  if (aligned16(x) && ldx % 2 == 0)
    hipLaunchKernelGGL((axpy_kernel<2, false>), grid, dim3(block_size), 0, h.stream, live, Z.n, Z.ld, Z.ldv, n_columns, Z.base, y, ystride, 1., x,
                       ldx, 1, nullptr);
  else
    hipLaunchKernelGGL((axpy_kernel<1, false>), grid, dim3(block_size), 0, h.stream, live, Z.n, Z.ld, Z.ldv, n_columns, Z.base, y, ystride, 1., x,
                       ldx, 1, nullptr);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

int plan(int k, int32_t const *live, int32_t const *slot_col, int32_t *run_start, int32_t *run_width, int32_t *run_groups,
         int32_t *group_width, int32_t *n_groups, int32_t *packed_col, int32_t *n_packed)
{
  int n_runs = 0, groups = 0, packed = 0;
  for (int s = 0; s < k;)
  {
    if (!live[s])
    {
      ++s;
      continue;
    }
    int e = s;
    for (; e < k && live[e]; ++e)
      packed_col[packed++] = slot_col[e];
    int widths[kMfBlockMaxGroups];
    const int ng = mf_block_groups(e - s, widths);
    for (int g = 0; g < ng; ++g)
      group_width[groups++] = widths[g];
    run_start[n_runs] = s;
    run_width[n_runs] = e - s;
    run_groups[n_runs] = ng;
    ++n_runs;
    s = e;
  }
  *n_groups = groups;
  *n_packed = packed;
  return n_runs;
}
} // namespace block_krylov_basis
} // namespace mfmg
