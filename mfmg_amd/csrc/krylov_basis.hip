// Fused orthogonalisation kernels of the flexible GMRES driver (krylov_basis.hpp).
//
// Streaming kernels, wave64, 256 threads: a thread owns W = 2 consecutive entries (one 16-byte access per vector; W = 1 where a
// pointer or the leading dimension is not 16-byte aligned) and walks the vector with a grid stride.  The columns are taken in
// groups of kGroup = 8: the loads of a group -- 8 x 16 bytes per thread -- are all issued before the first of them is used, so a
// wavefront keeps 8 KiB of column data in flight beside w (requests in flight, not bytes, bound the streaming kernels here).
// Every product enters its sum through one fma: a term of w - sum h_i V_i is rounded once.
// Reductions: per-thread partial -> __shfl_xor butterfly -> LDS across the 4 waves -> one partial per block and column; a second
// launch sums the partials of a column in a fixed order.  The grid depends on n alone.
//
// Owned-box kernels (OwnedBox): the owned entries are rows of row_len doubles, stride_y / stride_z apart, and a row may start at an
// odd entry.  A thread owns one SLOT of a row: with W = 2 a 16-byte ALIGNED pair of the local vector, of which the head slot of a
// row that starts odd and the tail slot of one that ends odd hold one owned entry each -- no 16-byte access is made at an address
// that is not 16-byte aligned.  The ghost half of such a pair is loaded with it and never used (a select, not a product: it may be
// NaN) and never stored (the two edge slots store 8 bytes).  Every row gets row_len / 2 + 1 slots, the most it can need; a slot
// past the row idles.  The grid stride is carried through (slot, y, z) in mixed radix, its digits computed on the host: no
// division in the loop.  The grid depends on the box alone.
#include "krylov_basis_bodies.hpp"

namespace mfmg
{
namespace krylov
{
namespace
{
using namespace body; // (krylov_basis_bodies.hpp: the bodies of the contiguous and of the owned-box kernels, shared with the block kernels)

// ---- the contiguous kernels: one vector pass each, the bodies of krylov_basis_bodies.hpp -------------------------------------------
// blockIdx.y: the group of kGroup columns; partials[column][block]
template <int W>
__global__ __launch_bounds__(block_size) void dots_kernel(int64_t n, int64_t ld, int n_columns, double const *__restrict__ V,
                                                           double const *__restrict__ w, double *__restrict__ partials)
{
  __shared__ double wsum[kGroup][kWaves];
  const int c0 = blockIdx.y * kGroup;
  const int nc = min(kGroup, n_columns - c0);
  V += (int64_t)c0 * ld;
  partials += (int64_t)c0 * gridDim.x;
  dots_group<W>(nc, n, ld, V, w, partials, wsum);
}

// one block per column: the partials of the column in a fixed order
__global__ __launch_bounds__(block_size) void dots_finish_kernel(int n_partials, double const *__restrict__ partials,
                                                                  double *__restrict__ h_pass, double *__restrict__ h_total, int accumulate)
{
  __shared__ double wsum[kWaves];
  dots_finish_body(n_partials, partials + (int64_t)blockIdx.x * n_partials, h_pass + blockIdx.x, h_total + blockIdx.x, accumulate, wsum);
}

// update / combine: out = out + sign * sum_i c[i] V_i
template <int W, bool kNorm>
__global__ __launch_bounds__(block_size) void axpy_kernel(int64_t n, int64_t ld, int n_columns, double const *__restrict__ V,
                                                           double const *__restrict__ c, double sign, double *__restrict__ out,
                                                           double *__restrict__ norm_partials)
{
  __shared__ double wsum[kWaves];
  axpy_body<W, kNorm>(n, ld, n_columns, V, c, sign, out, norm_partials, wsum);
}

template <int W>
__global__ __launch_bounds__(block_size) void scale_store_kernel(int64_t n, int n_partials, double const *__restrict__ partials,
                                                                  double const *w, double *v_next, float *__restrict__ v_next_f32,
                                                                  double *__restrict__ norm_out)
{
  __shared__ double wsum[kWaves];
  scale_store_body<W>(n, n_partials, partials, w, v_next, v_next_f32, norm_out, wsum);
}

// ---- owned-box kernels: the bodies of krylov_basis_bodies.hpp on one vector ------------------------------------------------------
template <int W>
__global__ __launch_bounds__(block_size) void box_dots_kernel(RowWalk g, int64_t ld, int n_columns, double const *__restrict__ V,
                                                               double const *__restrict__ w, double *__restrict__ partials)
{
  __shared__ double wsum[kGroup][kWaves];
  const int c0 = blockIdx.y * kGroup;
  const int nc = min(kGroup, n_columns - c0);
  V += (int64_t)c0 * ld;
  partials += (int64_t)c0 * gridDim.x;
  box_dots_group<W>(nc, g, ld, V, w, partials, wsum);
}

template <int W, bool kNorm>
__global__ __launch_bounds__(block_size) void box_axpy_kernel(RowWalk g, int64_t ld, int n_columns, double const *__restrict__ V,
                                                               double const *__restrict__ c, double sign, double *__restrict__ out,
                                                               double *__restrict__ norm_partials)
{
  __shared__ double wsum[1][kWaves];
  box_axpy_body<W, kNorm>(g, ld, n_columns, V, c, sign, out, norm_partials, wsum);
}

template <int W>
__global__ __launch_bounds__(block_size) void box_scale_store_kernel(RowWalk g, double const *__restrict__ norm_squared, double const *w,
                                                                      double *v_next, double *__restrict__ norm_out)
{
  box_scale_store_body<W>(g, norm_squared, w, v_next, norm_out);
}

bool aligned16(void const *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

void check_columns(int64_t n, int64_t ld, int n_columns)
{
  ASSERT_THROW(n >= 1 && n_columns >= 0, "krylov basis: empty vector or negative column count");
  ASSERT_THROW(n_columns == 0 || ld >= n, "krylov basis: the leading dimension is smaller than the vectors");
}
} // namespace

unsigned int reduction_blocks(int64_t n) { return n_blocks_for((n + 1) / 2, block_size, kMaxBlocks); }

void basis_dots(HipHandle &h, Scratch &s, int64_t n, int64_t ld, int n_columns, double const *V, double const *w, double *h_pass,
                double *h_total, bool accumulate)
{
  check_columns(n, ld, n_columns);
  if (n_columns == 0)
    return;
  ASSERT_THROW(n_columns <= s.capacity, "krylov basis: more columns than the scratch was built for");
  const unsigned int nb = reduction_blocks(n);
  const dim3 grid(nb, (unsigned)((n_columns + kGroup - 1) / kGroup));
  const int n_groups = (int)grid.y;
  hipEvent_t stop = h.profiler.begin("basis_dots", 8. * double(n) * (n_columns + n_groups), h.stream);
  if (aligned16(V) && aligned16(w) && ld % 2 == 0)
    hipLaunchKernelGGL(dots_kernel<2>, grid, dim3(block_size), 0, h.stream, n, ld, n_columns, V, w, s.dot_partials.data());
  else
    hipLaunchKernelGGL(dots_kernel<1>, grid, dim3(block_size), 0, h.stream, n, ld, n_columns, V, w, s.dot_partials.data());
  hipLaunchKernelGGL(dots_finish_kernel, dim3(n_columns), dim3(block_size), 0, h.stream, (int)nb, s.dot_partials.data(), h_pass, h_total,
                     accumulate ? 1 : 0);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

namespace
{
template <bool kNorm>
void launch_axpy(HipHandle &h, int64_t n, int64_t ld, int n_columns, double const *V, double const *c, double sign, double *out,
                 double *norm_partials)
{
  const dim3 grid(reduction_blocks(n));
  if (aligned16(V) && aligned16(out) && ld % 2 == 0)
    hipLaunchKernelGGL((axpy_kernel<2, kNorm>), grid, dim3(block_size), 0, h.stream, n, ld, n_columns, V, c, sign, out, norm_partials);
  else
    hipLaunchKernelGGL((axpy_kernel<1, kNorm>), grid, dim3(block_size), 0, h.stream, n, ld, n_columns, V, c, sign, out, norm_partials);
}
} // namespace

void basis_update(HipHandle &h, Scratch &s, int64_t n, int64_t ld, int n_columns, double const *V, double const *c, double *w,
                  bool with_norm)
{
  check_columns(n, ld, n_columns);
  hipEvent_t stop = h.profiler.begin("basis_update", 8. * double(n) * (n_columns + 2), h.stream);
  if (with_norm)
    launch_axpy<true>(h, n, ld, n_columns, V, c, -1., w, s.norm_partials.data());
  else
    launch_axpy<false>(h, n, ld, n_columns, V, c, -1., w, nullptr);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

void basis_norm_partials(HipHandle &h, Scratch &s, int64_t n, double const *w)
{
  // (w, w) of the dots kernel with w as its only column: the partials of column 0 are the norm's
  check_columns(n, n, 1);
  const dim3 grid(reduction_blocks(n));
  if (aligned16(w))
    hipLaunchKernelGGL(dots_kernel<2>, grid, dim3(block_size), 0, h.stream, n, n, 1, w, w, s.norm_partials.data());
  else
    hipLaunchKernelGGL(dots_kernel<1>, grid, dim3(block_size), 0, h.stream, n, n, 1, w, w, s.norm_partials.data());
  MFMG_HIP_CHECK(hipGetLastError());
}

void basis_scale_store(HipHandle &h, Scratch &s, int64_t n, double const *w, double *v_next, float *v_next_f32, double *norm_out)
{
  check_columns(n, n, 0);
  const int nb = (int)reduction_blocks(n);
  const dim3 grid(v_next == nullptr ? 1u : (unsigned)nb);
  hipEvent_t stop = h.profiler.begin("basis_scale_store", v_next == nullptr ? 0. : double(n) * (16. + (v_next_f32 ? 4. : 0.)), h.stream);
  if (aligned16(w) && aligned16(v_next) && (reinterpret_cast<uintptr_t>(v_next_f32) & 7u) == 0)
    hipLaunchKernelGGL(scale_store_kernel<2>, grid, dim3(block_size), 0, h.stream, n, nb, s.norm_partials.data(), w, v_next, v_next_f32,
                       norm_out);
  else
    hipLaunchKernelGGL(scale_store_kernel<1>, grid, dim3(block_size), 0, h.stream, n, nb, s.norm_partials.data(), w, v_next, v_next_f32,
                       norm_out);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

// ---- owned-box launches ---------------------------------------------------------------------------------------------------------
namespace
{
void check_box(OwnedBox const &b, int64_t ld, int n_columns)
{
  ASSERT_THROW(b.comps >= 1 && n_columns >= 0, "krylov basis: no component or a negative column count");
  for (int d = 0; d < 3; ++d)
    ASSERT_THROW(b.own0[d] >= 0 && b.own_n[d] >= 1 && b.own0[d] + b.own_n[d] <= b.local[d], "krylov basis: the owned box leaves the local box");
  ASSERT_THROW(n_columns == 0 || ld >= b.n_local(), "krylov basis: the leading dimension is smaller than the vectors");
}

// rows of the box, an axis that is owned whole joined with the next one (x and y whole: one run); slots of a row
void rows_of(OwnedBox const &b, RowWalk &g)
{
  g.stride_y = b.local[0] * b.comps;
  g.stride_z = g.stride_y * b.local[1];
  g.base = b.own0[0] * b.comps + b.own0[1] * g.stride_y + b.own0[2] * g.stride_z;
  g.row_len = b.own_n[0] * b.comps;
  g.n_y = b.own_n[1];
  g.n_z = b.own_n[2];
  g.n_local = b.n_local();
  if (b.own_n[0] == b.local[0])
  {
    g.row_len *= g.n_y;
    g.n_y = 1;
    if (b.own_n[1] == b.local[1])
    {
      g.row_len *= g.n_z;
      g.n_z = 1;
    }
  }
}

} // namespace

namespace body
{
RowWalk row_walk(OwnedBox const &b, int W, unsigned int n_blocks)
{
  RowWalk g;
  rows_of(b, g);
  g.slots = W == 2 ? g.row_len / 2 + 1 : g.row_len;
  const int64_t stride = (int64_t)n_blocks * block_size, rows = stride / g.slots;
  g.d_slot = stride % g.slots;
  g.d_y = rows % g.n_y;
  g.d_z = rows / g.n_y;
  return g;
}
} // namespace body

unsigned int reduction_blocks(OwnedBox const &box)
{
  RowWalk g;
  rows_of(box, g);
  return n_blocks_for((g.row_len / 2 + 1) * g.n_y * g.n_z, block_size, kMaxBlocks); // (the slots of the 16-byte kernels, for both)
}

void basis_dots(HipHandle &h, Scratch &s, OwnedBox const &box, int64_t ld, int n_columns, double const *V, double const *w,
                double *h_pass, double *h_total, bool accumulate)
{
  check_box(box, ld, n_columns);
  if (n_columns == 0)
    return;
  ASSERT_THROW(n_columns <= s.capacity, "krylov basis: more columns than the scratch was built for");
  const unsigned int nb = reduction_blocks(box);
  const dim3 grid(nb, (unsigned)((n_columns + kGroup - 1) / kGroup));
  hipEvent_t stop = h.profiler.begin("basis_dots_box", 8. * double(box.n_owned()) * (n_columns + (int)grid.y), h.stream);
  if (aligned16(V) && aligned16(w) && ld % 2 == 0)
    hipLaunchKernelGGL(box_dots_kernel<2>, grid, dim3(block_size), 0, h.stream, row_walk(box, 2, nb), ld, n_columns, V, w, s.dot_partials.data());
  else
    hipLaunchKernelGGL(box_dots_kernel<1>, grid, dim3(block_size), 0, h.stream, row_walk(box, 1, nb), ld, n_columns, V, w, s.dot_partials.data());
  hipLaunchKernelGGL(dots_finish_kernel, dim3(n_columns), dim3(block_size), 0, h.stream, (int)nb, s.dot_partials.data(), h_pass, h_total,
                     accumulate ? 1 : 0);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

namespace
{
template <bool kNorm>
void launch_box_axpy(HipHandle &h, OwnedBox const &box, int64_t ld, int n_columns, double const *V, double const *c, double *out,
                     double *norm_partials)
{
  const unsigned int nb = reduction_blocks(box);
  if (aligned16(V) && aligned16(out) && ld % 2 == 0)
    hipLaunchKernelGGL((box_axpy_kernel<2, kNorm>), dim3(nb), dim3(block_size), 0, h.stream, row_walk(box, 2, nb), ld, n_columns, V, c, -1., out,
                       norm_partials);
  else
    hipLaunchKernelGGL((box_axpy_kernel<1, kNorm>), dim3(nb), dim3(block_size), 0, h.stream, row_walk(box, 1, nb), ld, n_columns, V, c, -1., out,
                       norm_partials);
}
} // namespace

void basis_update(HipHandle &h, Scratch &s, OwnedBox const &box, int64_t ld, int n_columns, double const *V, double const *c,
                  double *w, bool with_norm)
{
  check_box(box, ld, n_columns);
  hipEvent_t stop = h.profiler.begin("basis_update_box", 8. * double(box.n_owned()) * (n_columns + 2), h.stream);
  if (with_norm)
    launch_box_axpy<true>(h, box, ld, n_columns, V, c, w, s.norm_partials.data());
  else
    launch_box_axpy<false>(h, box, ld, n_columns, V, c, w, nullptr);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

void basis_norm_partials(HipHandle &h, Scratch &s, OwnedBox const &box, double const *w)
{
  // as the contiguous one: (w, w) of the dots kernel with w as its only column
  check_box(box, box.n_local(), 1);
  const unsigned int nb = reduction_blocks(box);
  if (aligned16(w))
    hipLaunchKernelGGL(box_dots_kernel<2>, dim3(nb), dim3(block_size), 0, h.stream, row_walk(box, 2, nb), box.n_local(), 1, w, w,
                       s.norm_partials.data());
  else
    hipLaunchKernelGGL(box_dots_kernel<1>, dim3(nb), dim3(block_size), 0, h.stream, row_walk(box, 1, nb), box.n_local(), 1, w, w,
                       s.norm_partials.data());
  MFMG_HIP_CHECK(hipGetLastError());
}

void basis_norm_finish(HipHandle &h, Scratch &s, OwnedBox const &box)
{
  hipLaunchKernelGGL(dots_finish_kernel, dim3(1), dim3(block_size), 0, h.stream, (int)reduction_blocks(box), s.norm_partials.data(),
                     s.norm_squared.data(), s.norm_squared.data(), 0);
  MFMG_HIP_CHECK(hipGetLastError());
}

void basis_scale_store(HipHandle &h, OwnedBox const &box, double const *norm_squared, double const *w, double *v_next, double *norm_out)
{
  check_box(box, box.n_local(), 0);
  const unsigned int nb = v_next == nullptr ? 1u : reduction_blocks(box);
  hipEvent_t stop = h.profiler.begin("basis_scale_store_box", v_next == nullptr ? 0. : 16. * double(box.n_owned()), h.stream);
  if (aligned16(w) && aligned16(v_next))
    hipLaunchKernelGGL(box_scale_store_kernel<2>, dim3(nb), dim3(block_size), 0, h.stream, row_walk(box, 2, nb), norm_squared, w, v_next, norm_out);
  else
    hipLaunchKernelGGL(box_scale_store_kernel<1>, dim3(nb), dim3(block_size), 0, h.stream, row_walk(box, 1, nb), norm_squared, w, v_next, norm_out);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

void basis_combine(HipHandle &h, int64_t n, int64_t ld, int n_columns, double const *Z, double const *y, double *x)
{
  check_columns(n, ld, n_columns);
  if (n_columns == 0)
    return;
  hipEvent_t stop = h.profiler.begin("basis_combine", 8. * double(n) * (n_columns + 2), h.stream);
  launch_axpy<false>(h, n, ld, n_columns, Z, y, 1., x, nullptr);
  KernelProfiler::end(stop, h.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}
} // namespace krylov
} // namespace mfmg
