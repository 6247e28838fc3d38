// SpMV on a block of vectors for the matrices in CSR: block forms, NV = 4 and 2 columns per launch, of csr_spmv_kernel,
// csr_spmv_row_block_kernel and csr_spmv_lds_kernel (sparse_matrix_device.hip).  The lanes, their entries and the reduction of a
// row are those of the one-vector kernel; a lane loads the index and the value of a batch of its entries ONCE and multiplies
// them into the NV gathered entries of x, at x + c ld_x (the LDS form: into NV windows staged from the NV columns).  Per column
// the multiply-adds, their order and the epilogue are those of the one-vector kernel, so column c has the bits of launch() on
// that column.  Column c of b, x_prev and out sits at c ld_out; D^-1 is one vector.  Opt-in per matrix: set_block_csr.
#include "csr_kernel_args.hpp"

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

namespace mfmg
{
namespace
{
// Entries of a row that a lane keeps in flight: B index and value loads, then B NV reads of x.  At NV = 4 that is 44 registers
// of batch beside 8 of sums and up to 26 of epilogue operands requested ahead (106-118 VGPRs in all, of the 128 a 1024-thread
// workgroup can have); the order of the additions does not depend on it.
constexpr int kBlockRowBatch = 4;

// lane_row_sum on NV columns: the entries p, p + S, .. below e, x of column v taken at x[idx[] + v ld].  The index and the
// value of an entry are loaded once; per column the chain is the one of lane_row_sum -- `sum += val * x` in ascending entry
// order, an entry that is not there skipped, nothing read past e.
template <int S, int B, int NV, typename T, typename I, typename X>
__device__ __forceinline__ void lane_row_sum_block(T const *val, I const *idx, X const *x, int64_t ld, int p, int e, T (&sum)[NV])
{
  I c[B];
  T v[B], xv[B][NV];
#pragma unroll
  for (int w = 0; w < NV; ++w)
    sum[w] = T(0);
  for (; e - p > (B - 1) * S; p += B * S)
  {
#pragma unroll
    for (int k = 0; k < B; ++k)
    {
      c[k] = idx[p + k * S];
      v[k] = val[p + k * S];
    }
#pragma unroll
    for (int k = 0; k < B; ++k)
#pragma unroll
      for (int w = 0; w < NV; ++w)
        xv[k][w] = x[c[k] + w * ld];
#pragma unroll
    for (int w = 0; w < NV; ++w)
#pragma unroll
      for (int k = 0; k < B; ++k)
        sum[w] += v[k] * xv[k][w];
  }
  if (p < e)
  {
    // (B - 1 entries at most; one that is not there reads at the first one's position and is not added, as in lane_row_sum)
#pragma unroll
    for (int k = 0; k < B - 1; ++k)
    {
      const int q = e - p > k * S ? p + k * S : p;
      c[k] = idx[q];
      v[k] = val[q];
    }
#pragma unroll
    for (int k = 0; k < B - 1; ++k)
#pragma unroll
      for (int w = 0; w < NV; ++w)
        xv[k][w] = x[c[k] + w * ld];
#pragma unroll
    for (int w = 0; w < NV; ++w)
#pragma unroll
      for (int k = 0; k < B - 1; ++k)
        if (e - p > k * S)
          sum[w] += v[k] * xv[k][w];
  }
}

// the arguments of column v of a block
template <typename T>
__device__ __forceinline__ CsrArgs<T> column_args(CsrArgs<T> a, int64_t ld_x, int64_t ld_out, int v)
{
  a.x += v * ld_x;
  a.b += v * ld_out;
  a.xprev += v * ld_out;
  a.out += v * ld_out;
  return a;
}

// row_operands for the NV columns, requested ahead of the row loop by the lane that will store
template <typename T, int NV>
__device__ __forceinline__ void row_operands_block(CsrArgs<T> const &a, int64_t ld_x, int64_t ld_out, int64_t row, RowOperands<T> (&ops)[NV])
{
#pragma unroll
  for (int v = 0; v < NV; ++v)
    ops[v] = row_operands(column_args(a, ld_x, ld_out, v), row);
}

// the one epilogue() per column from operands requested before: every result is there before the first store
template <typename T, int NV>
__device__ __forceinline__ void store_row_columns(CsrArgs<T> const &a, int64_t ld_out, int64_t row, T const (&sum)[NV],
                                                  RowOperands<T> const (&ops)[NV])
{
  const CsrMode mode = static_cast<CsrMode>(a.mode);
  T o[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v)
    o[v] = epilogue(mode, &sum[v], &ops[v].x, &ops[v].b, &ops[v].dinv, &ops[v].xprev, &ops[v].out, int64_t(0), a.alpha, a.beta);
#pragma unroll
  for (int v = 0; v < NV; ++v)
    a.out[v * ld_out + row] = o[v];
}

// csr_spmv_kernel: LPR lanes share a row
template <typename T, int LPR, int NV>
__global__ __launch_bounds__(256) void csr_block_lanes_kernel(CsrArgs<T> a, int64_t ld_x, int64_t ld_out)
{
  const int64_t gtid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t row = gtid / LPR;
  const int sub = threadIdx.x % LPR;
  const bool stores = row < a.n_rows && sub == 0;
  RowOperands<T> ops[NV] = {};
  if (stores)
    row_operands_block<T, NV>(a, ld_x, ld_out, row, ops);
  T sum[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v)
    sum[v] = T(0);
  if (row < a.n_rows)
    lane_row_sum_block<LPR, kBlockRowBatch, NV>(a.val, a.col, a.x, ld_x, a.row_ptr[row] + sub, a.row_ptr[row + 1], sum);
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1)
      sum[v] += __shfl_xor(sum[v], off);
  if (stores)
    store_row_columns<T, NV>(a, ld_out, row, sum, ops);
}

// csr_spmv_row_block_kernel: a workgroup of four wavefronts per row, their sums of every column added as ((p0 + p1) + p2) + p3
template <typename T, int NV>
__global__ __launch_bounds__(256) void csr_block_row_kernel(CsrArgs<T> a, int64_t ld_x, int64_t ld_out)
{
  __shared__ T part[4][NV];
  const int64_t row = blockIdx.x;
  // (the row is uniform: requested beside row_ptr by every wavefront, as in the one-vector kernel)
  RowOperands<T> ops[NV];
  row_operands_block<T, NV>(a, ld_x, ld_out, row, ops);
  T sum[NV];
  lane_row_sum_block<256, kBlockRowBatch, NV>(a.val, a.col, a.x, ld_x, a.row_ptr[row] + (int)threadIdx.x, a.row_ptr[row + 1], sum);
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      sum[v] += __shfl_xor(sum[v], off);
  if ((threadIdx.x & 63) == 0)
  {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      part[threadIdx.x >> 6][v] = sum[v];
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      sum[v] = ((part[0][v] + part[1][v]) + part[2][v]) + part[3][v];
    store_row_columns<T, NV>(a, ld_out, row, sum, ops);
  }
}

// csr_spmv_lds_kernel: the window of x listed in l2g staged once per column into NV windows of `window` entries each; the rows
// stream val and the 16-bit lcol once
template <typename T, int LPR, int NV>
__global__ __launch_bounds__(1024) void csr_block_lds_kernel(CsrArgs<T> a, int64_t ld_x, int64_t ld_out, int32_t const *blk_ptr,
                                                             int32_t const *l2g, uint16_t const *lcol, int rows_per_block, int window)
{
  extern __shared__ __align__(16) unsigned char csr_block_smem[];
  T *xs = reinterpret_cast<T *>(csr_block_smem);
  __shared__ int rp[256 + 1];
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t row1 = min(row0 + rows_per_block, a.n_rows);
  const int l0 = blk_ptr[blockIdx.x], l1 = blk_ptr[blockIdx.x + 1];
  // Staging of rp[] and xs[], as in the one-vector kernel: a thread's elements are one batch -- their l2g loads (once for the
  // NV columns), then their x loads, then the LDS writes; an element past the end of the list reads at the thread's first one
  // and is not written.  Batches of 1, 2 or 4 elements (4 NV reads in flight), the rest of a longer list one by one.
  {
    const int n_rp = (int)(row1 - row0) + 1, n_x = l1 - l0, nt = blockDim.x, t = threadIdx.x;
    int r = 0;
    if (t < n_rp)
      r = a.row_ptr[row0 + t];
    auto stage = [&](auto kk) {
      constexpr int K = decltype(kk)::value;
      if (t >= n_x)
        return;
      int g[K];
      T xv[K][NV];
#pragma unroll
      for (int k = 0; k < K; ++k)
        g[k] = l2g[l0 + (n_x - t > k * nt ? t + k * nt : t)];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int v = 0; v < NV; ++v)
          xv[k][v] = a.x[g[k] + v * ld_x];
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (n_x - t > k * nt)
        {
#pragma unroll
          for (int v = 0; v < NV; ++v)
            xs[v * window + t + k * nt] = xv[k][v];
        }
    };
    if (n_x <= nt)
      stage(std::integral_constant<int, 1>());
    else if (n_x <= 2 * nt)
      stage(std::integral_constant<int, 2>());
    else
      stage(std::integral_constant<int, 4>());
    if (t < n_rp)
      rp[t] = r;
#pragma unroll 1
    for (int i = t + 4 * nt; i < n_x; i += nt)
    {
      const int g = l2g[l0 + i];
#pragma unroll
      for (int v = 0; v < NV; ++v)
        xs[v * window + i] = a.x[g + v * ld_x];
    }
#pragma unroll 1
    for (int i = t + nt; i < n_rp; i += nt)
      rp[i] = a.row_ptr[row0 + i];
  }
  __syncthreads();
  const int group = threadIdx.x / LPR, sub = threadIdx.x % LPR, n_groups = blockDim.x / LPR;
  // every lane runs the same number of passes so that the shuffles are wave-uniform
  for (int64_t base = row0; base < row1; base += n_groups)
  {
    const int64_t row = base + group;
    const bool stores = row < row1 && sub == 0;
    RowOperands<T> ops[NV] = {};
    if (stores)
      row_operands_block<T, NV>(a, ld_x, ld_out, row, ops);
    T sum[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v)
      sum[v] = T(0);
    if (row < row1)
      lane_row_sum_block<LPR, kBlockRowBatch, NV>(a.val, lcol, xs, (int64_t)window, rp[row - row0] + sub, rp[row - row0 + 1], sum);
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int off = LPR / 2; off > 0; off >>= 1)
        sum[v] += __shfl_xor(sum[v], off);
    if (stores)
      store_row_columns<T, NV>(a, ld_out, row, sum, ops);
  }
}

// f(std::integral_constant<int, l>()) for l = L, 2 L, .. 64: the instance of `lanes`
template <int L, typename F>
void with_block_lanes(int lanes, F &&f)
{
  if constexpr (L < 64)
  {
    if (lanes == L)
      f(std::integral_constant<int, L>());
    else
      with_block_lanes<2 * L>(lanes, f);
  }
  else
    f(std::integral_constant<int, 64>());
}
} // namespace

// Two 1024-thread workgroups of the LDS form stay resident on a CU: the NV windows and the table of row pointers within half
// of the 160 KiB.
template <typename T>
int SparseMatrixDevice<T>::block_csr_route(int nv) const
{
  if constexpr (!std::is_same_v<T, double>)
    return CsrForm::csr_none;
  if (!_block_csr || _csr_released || (nv != 2 && nv != 4) || (_val.size() == 0 && !_device_csr_deferred))
    return CsrForm::csr_none;
  const CsrForm f = form();
  if ((f.kind != 0 && f.kind != 1) || f.csr_kernel == CsrForm::csr_none)
    return CsrForm::csr_none;
  if (f.csr_kernel != CsrForm::csr_lds)
    return f.csr_kernel;
  // (the table rp[256 + 1] in front of the windows, which are aligned to 16 bytes)
  constexpr size_t kStaticLds = ((256 + 1) * sizeof(int) + 15) / 16 * 16, kLdsPerWorkgroup = 80 * 1024;
  return (size_t)nv * (size_t)_lds_max_cols * sizeof(T) + kStaticLds <= kLdsPerWorkgroup ? CsrForm::csr_lds : CsrForm::csr_lanes;
}

// one group of 4 or 2 columns of a matrix on a CSR kernel, set_block_csr(true): ONE launch, by the route of the group
template <typename T>
void SparseMatrixDevice<T>::launch_block_csr(CsrMode mode, int nv, T const *x, int64_t ld_x, T const *b, T const *dinv, T const *x_prev,
                                             T alpha, T beta, T *out, int64_t ld_out) const
{
  if constexpr (std::is_same_v<T, double>)
  {
    const int route = block_csr_route(nv);
    ASSERT_THROW(route != CsrForm::csr_none, "internal: no CSR block kernel for this matrix or group");
    const CsrForm f = form();
    ensure_device_csr();
    CsrArgs<T> a;
    a.val = _val.data();
    a.col = _col.data();
    a.row_ptr = _row_ptr.data();
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
    auto with_columns = [&](auto &&run) {
      if (nv == 4)
        run(std::integral_constant<int, 4>());
      else
        run(std::integral_constant<int, 2>());
    };
    if (route == CsrForm::csr_lds)
    {
      const size_t lds = (size_t)nv * (size_t)_lds_max_cols * sizeof(T);
      const int64_t nb = (_n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
      with_block_lanes<4>(f.lanes, [&](auto l) {
        with_columns([&](auto nvc) {
          auto kernel = csr_block_lds_kernel<T, decltype(l)::value, decltype(nvc)::value>;
          if (lds > 64 * 1024)
          {
            // (above the default limit of dynamic LDS: raised once per instance)
            static bool raised = false;
            if (!raised)
            {
              MFMG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
              raised = true;
            }
          }
          hipLaunchKernelGGL(kernel, dim3((unsigned int)nb), dim3(1024), lds, st, a, ld_x, ld_out, _blk_ptr.data(), _l2g.data(),
                             _lcol.data(), kRowsPerBlock, _lds_max_cols);
        });
      });
    }
    else if (route == CsrForm::csr_row_block)
      with_columns([&](auto nvc) {
        hipLaunchKernelGGL((csr_block_row_kernel<T, decltype(nvc)::value>), dim3((unsigned int)_n_rows), dim3(256), 0, st, a, ld_x, ld_out);
      });
    else
    {
      // (an LDS-cached matrix whose windows do not fit: the lanes of its LDS instance, through col and the global x)
      const int lanes = f.lanes;
      with_block_lanes<1>(lanes, [&](auto l) {
        constexpr int LPR = decltype(l)::value;
        const int64_t nb = (_n_rows * LPR + 255) / 256;
        with_columns([&](auto nvc) {
          hipLaunchKernelGGL((csr_block_lanes_kernel<T, LPR, decltype(nvc)::value>), dim3((unsigned int)std::max<int64_t>(nb, 1)), dim3(256),
                             0, st, a, ld_x, ld_out);
        });
      });
    }
    KernelProfiler::end(stop, st);
    MFMG_HIP_CHECK(hipGetLastError());
  }
  else
    ASSERT_THROW(false, "internal: the block kernels are FP64 only");
}

template int SparseMatrixDevice<double>::block_csr_route(int) const;
template int SparseMatrixDevice<float>::block_csr_route(int) const;
template void SparseMatrixDevice<double>::launch_block_csr(CsrMode, int, double const *, int64_t, double const *, double const *,
                                                           double const *, double, double, double *, int64_t) const;
template void SparseMatrixDevice<float>::launch_block_csr(CsrMode, int, float const *, int64_t, float const *, float const *, float const *,
                                                          float, float, float *, int64_t) const;
} // namespace mfmg
