// SpMV on a block of vectors for the matrices whose values do not repeat: the stored block diagonals (symmetric half in the
// split kernel, all of them in the row kernel) and the row-base storage.  Block forms, NV = 4 and 2 columns per launch, of
// bdia_sym_split_kernel, bdia_spmv_kernel over all rows and rowbase_spmv_kernel (sparse_matrix_device.hip): a lane keeps its
// row, loads every stored value ONCE and multiplies it into the NV gathered entries of x, at x + c ld_x; it carries NV sums and
// runs the one epilogue() per column.  Per column the operations and their order are those of the one-vector kernel, so
// column c has the bits of launch() on that column.  Column c of b, x_prev and out sits at c ld_out; D^-1 is one vector.
#include "csr_kernel_args.hpp"
#include "mf_laplace.hpp"

#include <algorithm>
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

namespace mfmg
{
namespace
{
// Block diagonals (slots of the row-base storage) whose loads a lane has in flight at once: C stored values and C NV entries of x
// each.  About 40 doubles, so that NV sums, the addresses of NV columns and the batch stay within the 128 VGPRs a 1024-thread
// workgroup allows -- which for the 256-thread kernels is four wavefronts per SIMD to switch to while a batch of gathers is out.
constexpr int block_batch(int C, int NV)
{
  const int u = 40 / (C * (1 + NV));
  return u < 1 ? 1 : u > 4 ? 4 : u;
}

// the epilogues of one row in the NV columns: every operand of every column is requested before the first store (nothing tells
// the compiler that out does not alias them)
template <typename T, int NV>
__device__ __forceinline__ void store_row_block(CsrArgs<T> const &a, int64_t ld_x, int64_t ld_out, int64_t row, T const (&sum)[NV])
{
  const CsrMode mode = static_cast<CsrMode>(a.mode);
  T o[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v)
    o[v] = epilogue(mode, &sum[v], a.x + v * ld_x, a.b + v * ld_out, a.dinv, a.xprev + v * ld_out, a.out + v * ld_out, row, a.alpha,
                    a.beta);
#pragma unroll
  for (int v = 0; v < NV; ++v)
    a.out[v * ld_out + row] = o[v];
}

// bdia_spmv_kernel over all rows
template <typename T, int C, typename V, int NV>
__global__ __launch_bounds__(256) void bdia_spmv_block_kernel(CsrArgs<T> a, int64_t ld_x, int64_t ld_out, V const *val,
                                                              int32_t const *offs, int D)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= a.n_rows)
    return;
  constexpr int kBatch = block_batch(C, NV);
  const int64_t n_nodes = a.n_rows / C;
  const int64_t node = r / C;
  V const *vp = val + r;
  const size_t stride = (size_t)a.n_rows;
  T sum[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v)
    sum[v] = T(0);
#pragma unroll kBatch
  for (int d = 0; d < D; ++d)
  {
    const int64_t nb = node + offs[d];
    if (nb >= 0 && nb < n_nodes)
    {
#pragma unroll
      for (int cc = 0; cc < C; ++cc)
      {
        const T m = T(vp[(size_t)(d * C + cc) * stride]);
        T const *xp = a.x + nb * C + cc;
#pragma unroll
        for (int v = 0; v < NV; ++v)
          sum[v] += m * xp[v * ld_x];
      }
    }
  }
  store_row_block<T, NV>(a, ld_x, ld_out, r, sum);
}

template <typename T, int NV>
__global__ __launch_bounds__(256) void rowbase_spmv_block_kernel(CsrArgs<T> a, int64_t ld_x, int64_t ld_out, T const *val,
                                                                 int32_t const *base, int32_t const *offs, int S, int64_t n_cols)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= a.n_rows)
    return;
  constexpr int kBatch = block_batch(1, NV);
  const int64_t b0 = base[r];
  T const *vp = val + r;
  const size_t stride = (size_t)a.n_rows;
  T sum[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v)
    sum[v] = T(0);
#pragma unroll kBatch
  for (int sidx = 0; sidx < S; ++sidx)
  {
    const int64_t c = b0 + offs[sidx];
    if (c >= 0 && c < n_cols)
    {
      const T m = vp[(size_t)sidx * stride];
      T const *xp = a.x + c;
#pragma unroll
      for (int v = 0; v < NV; ++v)
        sum[v] += m * xp[v * ld_x];
    }
  }
  store_row_block<T, NV>(a, ld_x, ld_out, r, sum);
}

// bdia_sym_split_kernel: the block diagonals dealt to the four quarters of a 1024-thread workgroup, upper part first, then the
// lower part; neighbours outside the matrix read at a clamped position with their entry replaced by 0; the quarters of every
// column added as ((q0 + q1) + q2) + q3 through LDS (3 NV 256 doubles: 24 KiB at NV = 4)
template <typename T, int C, typename V, int NV>
__global__ __launch_bounds__(1024) void bdia_sym_split_block_kernel(CsrArgs<T> a, int64_t ld_x, int64_t ld_out, V const *val,
                                                                    int32_t const *offs, int D)
{
  constexpr int kBatch = block_batch(C, NV);
  __shared__ T part[3][NV][256];
  const int q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)), lane = threadIdx.x & 255;
  const int64_t r = (int64_t)blockIdx.x * 256 + lane;
  const bool active = r < a.n_rows;
  const int64_t rr = active ? r : a.n_rows - 1;
  const int64_t last = a.n_rows / C - 1;
  const int64_t node = rr / C;
  const int c = (int)(rr - node * C);
  const size_t stride = (size_t)a.n_rows;
  V const *vp = val + rr;
  const int d0 = (D * q) / 4, d1 = (D * (q + 1)) / 4;
  T sum[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v)
    sum[v] = T(0);
#pragma unroll kBatch
  for (int d = d0; d < d1; ++d) // offs[0] = 0 < offs[1] < ...; the entry of a neighbour behind the last node is 0
  {
    const int64_t nb = min(node + offs[d], last);
#pragma unroll
    for (int cc = 0; cc < C; ++cc)
    {
      const T m = T(vp[(size_t)(d * C + cc) * stride]);
      T const *xp = a.x + nb * C + cc;
#pragma unroll
      for (int v = 0; v < NV; ++v)
        sum[v] += m * xp[v * ld_x];
    }
  }
#pragma unroll kBatch
  for (int d = max(d0, 1); d < d1; ++d)
  {
    const int64_t nbu = node - offs[d];
    const int64_t nb = max(nbu, (int64_t)0);
    V const *vq = val + (size_t)(d * C + c) * stride + nb * C;
#pragma unroll
    for (int cc = 0; cc < C; ++cc)
    {
      const T m = nbu >= 0 ? T(vq[cc]) : T(0);
      T const *xp = a.x + nb * C + cc;
#pragma unroll
      for (int v = 0; v < NV; ++v)
        sum[v] += m * xp[v * ld_x];
    }
  }
  if (q > 0)
  {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      part[q - 1][v][lane] = sum[v];
  }
  __syncthreads();
  if (q == 0 && active)
  {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      sum[v] = ((sum[v] + part[0][v][lane]) + part[1][v][lane]) + part[2][v][lane];
    store_row_block<T, NV>(a, ld_x, ld_out, r, sum);
  }
}
} // namespace

template <typename T>
int SparseMatrixDevice<T>::block_width() const
{
  if constexpr (!std::is_same_v<T, double>)
    return 1;
  const CsrForm f = form();
  if (((f.kind == 2 || f.kind == 3) && f.regular == 0) || f.kind == 4)
    return 4;
  // (set_block_csr: the CSR kernels, sparse_matrix_block_csr.hip)
  return block_csr_route(4) != CsrForm::csr_none ? 4 : 1;
}

template <typename T>
void SparseMatrixDevice<T>::block_counters(int64_t &block_launches, int64_t &column_launches) const
{
  block_launches = _block_launches.load(std::memory_order_relaxed);
  column_launches = _column_launches.load(std::memory_order_relaxed);
}

template <typename T>
void SparseMatrixDevice<T>::apply_mode_block(CsrMode mode, int n_vectors, T const *x, int64_t ld_x, T const *b, T const *dinv,
                                             T const *x_prev, T alpha, T beta, T *out, int64_t ld_out) const
{
  const int m = static_cast<int>(mode);
  ASSERT_THROW(m >= 0 && m <= 6, "unknown SpMV mode");
  const CsrOperands need = operands_of(mode);
  ASSERT_THROW(x != nullptr && out != nullptr, "null vector");
  ASSERT_THROW(!need.b || b != nullptr, "this SpMV mode needs b");
  ASSERT_THROW(!need.dinv || dinv != nullptr, "this SpMV mode needs the inverse diagonal");
  ASSERT_THROW(!need.xprev || x_prev != nullptr, "this SpMV mode needs x_prev");
  ASSERT_THROW(!need.x || _n_rows == _n_cols, "the smoother needs a square matrix");
  // the block rules ("Blocks of vectors")
  ASSERT_THROW(n_vectors >= 1 && n_vectors <= kMfBlockMaxVectors, "a block holds 1 to 64 vectors");
  ASSERT_THROW(ld_x >= _n_cols && ld_out >= _n_rows, "the leading dimension of a block must be at least the vector size");
  ASSERT_THROW(ld_x % 2 == 0 && ld_out % 2 == 0, "the leading dimension of a block must be even (columns aligned to 16 bytes)");
  auto aligned = [](void const *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  ASSERT_THROW(aligned(x) && aligned(out) && (!need.b || aligned(b)) && (!need.dinv || aligned(dinv)) && (!need.xprev || aligned(x_prev)),
               "the base of a block must be aligned to 16 bytes");
  {
    T const *x_end = x + (size_t)(n_vectors - 1) * ld_x + _n_cols, *out_end = out + (size_t)(n_vectors - 1) * ld_out + _n_rows;
    ASSERT_THROW(x_end <= out || out_end <= x, "SpMV cannot run in place (the block out overlaps the block x)");
  }
  b = need.b ? b : nullptr;
  dinv = need.dinv ? dinv : nullptr;
  x_prev = need.xprev ? x_prev : nullptr;
  alpha = need.xprev ? alpha : T(0);
  beta = need.dinv ? beta : T(0);
  if (_n_rows == 0)
    return;
  const int width = block_width();
  int widths[kMfBlockMaxGroups];
  const int n_groups = mf_block_groups(n_vectors, widths);
  int64_t c0 = 0;
  for (int g = 0; g < n_groups; c0 += widths[g], ++g)
  {
    auto at = [&](T const *p, int64_t ld) { return p != nullptr ? p + c0 * ld : nullptr; };
    if (width > 1 && widths[g] > 1)
    {
      launch_block(mode, widths[g], x + c0 * ld_x, ld_x, at(b, ld_out), dinv, at(x_prev, ld_out), alpha, beta, out + c0 * ld_out, ld_out);
      _block_launches.fetch_add(1, std::memory_order_relaxed);
      continue;
    }
    for (int64_t c = c0; c < c0 + widths[g]; ++c)
      launch(mode, x + c * ld_x, b != nullptr ? b + c * ld_out : nullptr, dinv, x_prev != nullptr ? x_prev + c * ld_out : nullptr, alpha,
             beta, out + c * ld_out);
    _column_launches.fetch_add(widths[g], std::memory_order_relaxed);
  }
}

// one group of 4 or 2 columns of a matrix whose launch is exactly one of the three kernels above, or one of the CSR kernels
// under set_block_csr (block_width() == 4)
template <typename T>
void SparseMatrixDevice<T>::launch_block(CsrMode mode, int nv, T const *x, int64_t ld_x, T const *b, T const *dinv, T const *x_prev,
                                         T alpha, T beta, T *out, int64_t ld_out) const
{
  if constexpr (std::is_same_v<T, double>)
  {
    const CsrForm f = form(); // (every branch below is taken from it, as in launch())
    if (f.kind == 0 || f.kind == 1)
      return launch_block_csr(mode, nv, x, ld_x, b, dinv, x_prev, alpha, beta, out, ld_out);
    ASSERT_THROW((((f.kind == 2 || f.kind == 3) && f.regular == 0) || f.kind == 4) && (nv == 2 || nv == 4),
                 "internal: no block kernel for this matrix or group");
    CsrArgs<T> a;
    a.val = nullptr; // (the block kernels read planes, never the CSR arrays)
    a.col = nullptr;
    a.row_ptr = nullptr;
    a.n_rows = _n_rows;
    a.x = x;
    a.b = b;
    a.dinv = dinv;
    a.xprev = x_prev;
    a.out = out;
    a.alpha = alpha;
    a.beta = beta;
    a.mode = static_cast<int>(mode);
    a.pairs = 1;
    hipStream_t st = _handle.stream;
    // algorithmic bytes: the matrix once, the vectors of launch() nv times
    const CsrOperands need = operands_of(mode);
    const double extra = (need.b || need.out ? 1. : 0.) + (need.x ? 2. : 0.) + (need.xprev ? 1. : 0.);
    const double vectors = sizeof(T) * (double(_n_cols) + double(_n_rows) * (1. + extra));
    const double matrix = algorithmic_bytes_apply() - sizeof(T) * (double(_n_cols) + double(_n_rows));
    hipEvent_t stop = _handle.profiler.begin("csr_block_kernel", matrix + nv * vectors, st);
    const dim3 grid((unsigned int)((_n_rows + 255) / 256));
    auto with_columns = [&](auto &&run) {
      if (nv == 4)
        run(std::integral_constant<int, 4>());
      else
        run(std::integral_constant<int, 2>());
    };
    if (f.kind == 4)
      with_columns([&](auto nvc) {
        hipLaunchKernelGGL((rowbase_spmv_block_kernel<T, decltype(nvc)::value>), grid, dim3(256), 0, st, a, ld_x, ld_out, _rb_val.data(),
                           _rb_base.data(), _rb_offs.data(), _rb_slots, _n_cols);
      });
    else
    {
      auto stored = [&](auto const *planes) {
        using V = std::remove_cv_t<std::remove_pointer_t<decltype(planes)>>;
        with_node_width(_bdia_c, [&](auto cc) {
          constexpr int C = decltype(cc)::value;
          with_columns([&](auto nvc) {
            constexpr int NV = decltype(nvc)::value;
            if (f.stored_kernel == CsrForm::stored_sym_split)
              hipLaunchKernelGGL((bdia_sym_split_block_kernel<T, C, V, NV>), grid, dim3(1024), 0, st, a, ld_x, ld_out, planes,
                                 _bdia_offs.data(), _bdia_d);
            else
              hipLaunchKernelGGL((bdia_spmv_block_kernel<T, C, V, NV>), grid, dim3(256), 0, st, a, ld_x, ld_out, planes, _bdia_offs.data(),
                                 _bdia_d);
          });
        });
      };
      if (f.float_planes)
        stored(_bdia_val_f32.data());
      else
        stored(_bdia_val.data());
    }
    KernelProfiler::end(stop, st);
    MFMG_HIP_CHECK(hipGetLastError());
  }
  else
    ASSERT_THROW(false, "internal: the block kernels are FP64 only");
}

template int SparseMatrixDevice<double>::block_width() const;
template int SparseMatrixDevice<float>::block_width() const;
template void SparseMatrixDevice<double>::block_counters(int64_t &, int64_t &) const;
template void SparseMatrixDevice<float>::block_counters(int64_t &, int64_t &) const;
template void SparseMatrixDevice<double>::apply_mode_block(CsrMode, int, double const *, int64_t, double const *, double const *,
                                                           double const *, double, double, double *, int64_t) const;
template void SparseMatrixDevice<float>::apply_mode_block(CsrMode, int, float const *, int64_t, float const *, float const *, float const *,
                                                          float, float, float *, int64_t) const;
} // namespace mfmg
