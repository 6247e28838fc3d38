// Device bodies of the contiguous orthogonalisation kernels (krylov_basis.hpp), shared by the one-vector kernels of
// krylov_basis.hip and the block kernels of block_krylov_basis.hip: the loops, the reductions and the expressions exist once, so a
// slot of a block launch gets the bits of the one-vector launch.  A body sees one vector pass: its pointers are those of one w (one
// slot), blockIdx.x / gridDim.x walk the entries, and every further grid dimension belongs to the kernel around it.
// Device code only: include from a .hip file.
#pragma once

#include "krylov_basis.hpp"

namespace mfmg
{
namespace krylov
{
namespace body
{
constexpr int kWaves = block_size / 64;

template <int W>
__device__ __forceinline__ void load(double const *p, double (&r)[W])
{
  if constexpr (W == 2)
  {
    const double2 t = *reinterpret_cast<double2 const *>(p);
    r[0] = t.x;
    r[1] = t.y;
  }
  else
    r[0] = *p;
}

template <int W>
__device__ __forceinline__ void store(double *p, double const (&r)[W])
{
  if constexpr (W == 2)
    *reinterpret_cast<double2 *>(p) = make_double2(r[0], r[1]);
  else
    *p = r[0];
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_xor(v, off);
  return v;
}

// the entries past the last whole group of W (n odd, W = 2) belong to the first thread of the grid row
__device__ __forceinline__ bool owns_tail() { return blockIdx.x == 0 && threadIdx.x == 0; }

// the sums of a block: partials[column][block] = sum over the block's threads of acc[column], waves in a fixed order
template <int NC>
__device__ __forceinline__ void block_column_sums(double const (&acc)[NC], double *__restrict__ partials, double (*wsum)[kWaves])
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NC; ++c)
  {
    const double t = wave_sum(acc[c]);
    if (lane == 0)
      wsum[c][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x < NC)
  {
    double t = 0.;
#pragma unroll
    for (int k = 0; k < kWaves; ++k)
      t += wsum[threadIdx.x][k];
    partials[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
  }
}

// ---- dots ----------------------------------------------------------------------------------------------------------------------
template <int W, int NC>
__device__ __forceinline__ void dots_body(int64_t n, int64_t ld, double const *__restrict__ V, double const *__restrict__ w,
                                          double *__restrict__ partials, double (*wsum)[kWaves])
{
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
    acc[c] = 0.;
  const int64_t n_units = n / W, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n_units; u += stride)
  {
    const int64_t e = u * W;
    double v[NC][W], ww[W];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      load<W>(V + c * ld + e, v[c]);
    load<W>(w + e, ww);
#pragma unroll
    for (int c = 0; c < NC; ++c)
    {
#pragma unroll
      for (int k = 0; k < W; ++k)
        acc[c] = fma(v[c][k], ww[k], acc[c]);
    }
  }
  if (owns_tail())
    for (int64_t e = n_units * W; e < n; ++e)
    {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        acc[c] = fma(V[c * ld + e], w[e], acc[c]);
    }
  block_column_sums<NC>(acc, partials, wsum);
}

// one group of nc <= kGroup columns (nc is the same in every thread of the grid row); partials[column][block]
template <int W>
__device__ __forceinline__ void dots_group(int nc, int64_t n, int64_t ld, double const *__restrict__ V, double const *__restrict__ w,
                                           double *__restrict__ partials, double (*wsum)[kWaves])
{
  switch (nc)
  {
  case 1: dots_body<W, 1>(n, ld, V, w, partials, wsum); break;
  case 2: dots_body<W, 2>(n, ld, V, w, partials, wsum); break;
  case 3: dots_body<W, 3>(n, ld, V, w, partials, wsum); break;
  case 4: dots_body<W, 4>(n, ld, V, w, partials, wsum); break;
  case 5: dots_body<W, 5>(n, ld, V, w, partials, wsum); break;
  case 6: dots_body<W, 6>(n, ld, V, w, partials, wsum); break;
  case 7: dots_body<W, 7>(n, ld, V, w, partials, wsum); break;
  default: dots_body<W, 8>(n, ld, V, w, partials, wsum); break;
  }
}

// one block per column: the partials of the column in a fixed order
__device__ __forceinline__ void dots_finish_body(int n_partials, double const *__restrict__ partials, double *__restrict__ h_pass,
                                                 double *__restrict__ h_total, int accumulate, double (&wsum)[kWaves])
{
  double acc = 0.;
  for (int i = threadIdx.x; i < n_partials; i += blockDim.x)
    acc += partials[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0)
    wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    double t = 0.;
    for (int k = 0; k < kWaves; ++k)
      t += wsum[k];
    h_pass[0] = t;
    h_total[0] = accumulate ? h_total[0] + t : t;
  }
}

// ---- update / combine: out = out + sign * sum_i c[i] V_i -------------------------------------------------------------------------
template <int W, int NC>
__device__ __forceinline__ void axpy_group(double (&acc)[W], double const *__restrict__ V, int64_t ld, double const *__restrict__ c,
                                           double sign)
{
  double v[NC][W];
#pragma unroll
  for (int i = 0; i < NC; ++i)
    load<W>(V + i * ld, v[i]);
#pragma unroll
  for (int i = 0; i < NC; ++i)
  {
    const double a = sign * c[i];
#pragma unroll
    for (int k = 0; k < W; ++k)
      acc[k] = fma(a, v[i][k], acc[k]);
  }
}

template <int W>
__device__ __forceinline__ void axpy_columns(double (&acc)[W], double const *__restrict__ V, int64_t ld, int n_columns,
                                             double const *__restrict__ c, double sign)
{
  int g = 0;
  for (; g + kGroup <= n_columns; g += kGroup)
    axpy_group<W, kGroup>(acc, V + (int64_t)g * ld, ld, c + g, sign);
  V += (int64_t)g * ld;
  c += g;
  switch (n_columns - g)
  {
  case 1: axpy_group<W, 1>(acc, V, ld, c, sign); break;
  case 2: axpy_group<W, 2>(acc, V, ld, c, sign); break;
  case 3: axpy_group<W, 3>(acc, V, ld, c, sign); break;
  case 4: axpy_group<W, 4>(acc, V, ld, c, sign); break;
  case 5: axpy_group<W, 5>(acc, V, ld, c, sign); break;
  case 6: axpy_group<W, 6>(acc, V, ld, c, sign); break;
  case 7: axpy_group<W, 7>(acc, V, ld, c, sign); break;
  default: break;
  }
}

// kNorm: norm_partials[block] = the block's part of ||out||^2 of the updated out
template <int W, bool kNorm>
__device__ __forceinline__ void axpy_body(int64_t n, int64_t ld, int n_columns, double const *__restrict__ V, double const *__restrict__ c,
                                          double sign, double *__restrict__ out, double *__restrict__ norm_partials, double (&wsum)[kWaves])
{
  double nrm = 0.;
  const int64_t n_units = n / W, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n_units; u += stride)
  {
    const int64_t e = u * W;
    double acc[W];
    load<W>(out + e, acc);
    axpy_columns<W>(acc, V + e, ld, n_columns, c, sign);
    store<W>(out + e, acc);
    if (kNorm)
    {
#pragma unroll
      for (int k = 0; k < W; ++k)
        nrm = fma(acc[k], acc[k], nrm);
    }
  }
  if (owns_tail())
    for (int64_t e = n_units * W; e < n; ++e)
    {
      double acc[1] = {out[e]};
      axpy_columns<1>(acc, V + e, ld, n_columns, c, sign);
      out[e] = acc[0];
      if (kNorm)
        nrm = fma(acc[0], acc[0], nrm);
    }
  if (kNorm)
  {
    nrm = wave_sum(nrm);
    if ((threadIdx.x & 63) == 0)
      wsum[threadIdx.x >> 6] = nrm;
    __syncthreads();
    if (threadIdx.x == 0)
    {
      double t = 0.;
      for (int k = 0; k < kWaves; ++k)
        t += wsum[k];
      norm_partials[blockIdx.x] = t;
    }
  }
}

// ---- scale_store ---------------------------------------------------------------------------------------------------------------
// Every block sums the norm partials itself, all in the same order: the same norm in every block, no launch in between.
template <int W>
__device__ __forceinline__ void scale_store_body(int64_t n, int n_partials, double const *__restrict__ partials, double const *w,
                                                 double *v_next, float *__restrict__ v_next_f32, double *__restrict__ norm_out,
                                                 double (&wsum)[kWaves])
{
  double acc = 0.;
  for (int i = threadIdx.x; i < n_partials; i += blockDim.x)
    acc += partials[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0)
    wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  double total = 0.;
#pragma unroll
  for (int k = 0; k < kWaves; ++k)
    total += wsum[k];
  const double norm = sqrt(total);
  if (owns_tail())
    norm_out[0] = norm;
  if (v_next == nullptr)
    return;
  const double inv = norm > 0. ? 1. / norm : 0.;
  const int64_t n_units = n / W, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n_units; u += stride)
  {
    const int64_t e = u * W;
    double r[W];
    load<W>(w + e, r);
#pragma unroll
    for (int k = 0; k < W; ++k)
      r[k] *= inv;
    store<W>(v_next + e, r);
    if (v_next_f32 != nullptr)
    {
      if constexpr (W == 2)
        *reinterpret_cast<float2 *>(v_next_f32 + e) = make_float2((float)r[0], (float)r[1]);
      else
        v_next_f32[e] = (float)r[0];
    }
  }
  if (owns_tail())
    for (int64_t e = n_units * W; e < n; ++e)
    {
      const double r = w[e] * inv;
      v_next[e] = r;
      if (v_next_f32 != nullptr)
        v_next_f32[e] = (float)r;
    }
}
} // namespace body
} // namespace krylov
} // namespace mfmg
