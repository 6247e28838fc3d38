// Device bodies of the orthogonalisation kernels (krylov_basis.hpp), the contiguous ones and the owned-box ones, shared by the
// one-vector kernels of krylov_basis.hip and the block kernels of block_krylov_basis.hip: the loops, the reductions and the
// expressions exist once, so a slot of a block launch gets the bits of the one-vector launch.  A body sees one vector pass: its
// pointers are those of one w (one slot), blockIdx.x / gridDim.x walk the entries, and every further grid dimension belongs to the
// kernel around it.
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
// ---- owned-box bodies (krylov_basis.hip, head comment: the slots of a row, the mixed-radix grid stride) ---------------------------
// The rows of an OwnedBox (whole axes joined) and the walk of one launch over their slots.  Index: the type the walk and the
// entry of a slot are computed in -- int64_t, or 32 bits where the local vector is shorter than 2^31 entries (the block kernels);
// the entries a thread visits and the order of every sum do not depend on it.
template <typename Index>
struct RowWalkT
{
  Index base, row_len, stride_y, stride_z, n_y, n_z; // row (y, z) = the entries [s, s + row_len), s = base + y stride_y + z stride_z
  Index n_local;                                     // entries of the local vector: a pair that ends past it is not loaded
  Index slots;                                       // slots per row
  Index d_slot, d_y, d_z;                            // the grid stride in slots = d_slot + slots (d_y + n_y d_z)
  RowWalkT() = default;
  template <typename From>
  __host__ __device__ explicit RowWalkT(RowWalkT<From> const &o)
      : base((Index)o.base), row_len((Index)o.row_len), stride_y((Index)o.stride_y), stride_z((Index)o.stride_z), n_y((Index)o.n_y),
        n_z((Index)o.n_z), n_local((Index)o.n_local), slots((Index)o.slots), d_slot((Index)o.d_slot), d_y((Index)o.d_y), d_z((Index)o.d_z)
  {
  }
};
using RowWalk = RowWalkT<int64_t>;

// the walk of a launch of n_blocks blocks over the box with accesses of W entries (host; krylov_basis.hip)
RowWalk row_walk(OwnedBox const &box, int W, unsigned int n_blocks);

template <int W, typename Index = int64_t>
struct Cursor
{
  Index slot, y, z;
  __device__ __forceinline__ explicit Cursor(RowWalkT<Index> const &g)
  {
    const Index u = (Index)blockIdx.x * (Index)blockDim.x + (Index)threadIdx.x, row = u / g.slots;
    slot = u % g.slots;
    y = row % g.n_y;
    z = row / g.n_y;
  }
  __device__ __forceinline__ bool inside(RowWalkT<Index> const &g) const { return z < g.n_z; }
  __device__ __forceinline__ void advance(RowWalkT<Index> const &g)
  {
    slot += g.d_slot;
    y += g.d_y;
    z += g.d_z;
    if (slot >= g.slots)
    {
      slot -= g.slots;
      ++y;
    }
    if (y >= g.n_y)
    {
      y -= g.n_y;
      ++z;
    }
  }
  // first entry of the slot (W = 2: even) and which of its W entries the row holds
  __device__ __forceinline__ Index entries(RowWalkT<Index> const &g, bool (&in)[W]) const
  {
    const Index s = g.base + y * g.stride_y + z * g.stride_z;
    if constexpr (W == 1)
    {
      in[0] = true; // (slots = row_len)
      return s + slot;
    }
    else
    {
      const Index e = ((s >> 1) + slot) << 1; // (e + 1 >= s)
      in[0] = e >= s && e < s + g.row_len;
      in[1] = e + 1 < s + g.row_len;
      return e;
    }
  }
};

// the products of one slot: WL = the width of the loads (WL < W: the one pair that ends past the vector, its first entry alone)
template <int W, int WL, int NC>
__device__ __forceinline__ void dots_slot(double (&acc)[NC], bool const (&in)[W], double const *__restrict__ V, int64_t ld,
                                          double const *__restrict__ w)
{
  double v[NC][WL], ww[WL];
#pragma unroll
  for (int c = 0; c < NC; ++c)
    load<WL>(V + c * ld, v[c]);
  load<WL>(w, ww);
#pragma unroll
  for (int c = 0; c < NC; ++c)
  {
#pragma unroll
    for (int k = 0; k < WL; ++k)
    {
      const double t = fma(v[c][k], ww[k], acc[c]);
      acc[c] = in[k] ? t : acc[c]; // (not a product with 0: a ghost entry may hold NaN)
    }
  }
}

template <int W, int NC, typename Index>
__device__ __forceinline__ void box_dots_body(RowWalkT<Index> const &g, int64_t ld, double const *__restrict__ V,
                                              double const *__restrict__ w, double *__restrict__ partials, double (*wsum)[kWaves])
{
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
    acc[c] = 0.;
  for (Cursor<W, Index> cur(g); cur.inside(g); cur.advance(g))
  {
    bool in[W];
    const Index e = cur.entries(g, in);
    if (!in[0] && !in[W - 1])
      continue;
    if (W == 1 || e + 1 < g.n_local)
      dots_slot<W, W, NC>(acc, in, V + e, ld, w + e);
    else
      dots_slot<W, 1, NC>(acc, in, V + e, ld, w + e);
  }
  block_column_sums<NC>(acc, partials, wsum);
}

// one group of nc <= kGroup columns (nc is the same in every thread of the grid row); partials[column][block]
template <int W, typename Index>
__device__ __forceinline__ void box_dots_group(int nc, RowWalkT<Index> const &g, int64_t ld, double const *__restrict__ V,
                                               double const *__restrict__ w, double *__restrict__ partials, double (*wsum)[kWaves])
{
  switch (nc)
  {
  case 1: box_dots_body<W, 1>(g, ld, V, w, partials, wsum); break;
  case 2: box_dots_body<W, 2>(g, ld, V, w, partials, wsum); break;
  case 3: box_dots_body<W, 3>(g, ld, V, w, partials, wsum); break;
  case 4: box_dots_body<W, 4>(g, ld, V, w, partials, wsum); break;
  case 5: box_dots_body<W, 5>(g, ld, V, w, partials, wsum); break;
  case 6: box_dots_body<W, 6>(g, ld, V, w, partials, wsum); break;
  case 7: box_dots_body<W, 7>(g, ld, V, w, partials, wsum); break;
  default: box_dots_body<W, 8>(g, ld, V, w, partials, wsum); break;
  }
}

// the owned entries of a slot stored: both halves of a pair in one 16-byte store, an edge slot its one entry
template <int W>
__device__ __forceinline__ void store_owned(double *p, double const (&r)[W], bool const (&in)[W])
{
  if (in[0] && in[W - 1])
    store<W>(p, r);
  else if (in[0])
    p[0] = r[0];
  else if (in[W - 1])
    p[W - 1] = r[W - 1];
}

// the owned entries of out += sign * sum_i c[i] V_i; kNorm: norm_partials[block] = the block's part of ||out||^2 over them
template <int W, bool kNorm, typename Index>
__device__ __forceinline__ void box_axpy_body(RowWalkT<Index> const &g, int64_t ld, int n_columns, double const *__restrict__ V,
                                              double const *__restrict__ c, double sign, double *__restrict__ out,
                                              double *__restrict__ norm_partials, double (*wsum)[kWaves])
{
  double nrm[1] = {0.};
  for (Cursor<W, Index> cur(g); cur.inside(g); cur.advance(g))
  {
    bool in[W];
    const Index e = cur.entries(g, in);
    if (!in[0] && !in[W - 1])
      continue;
    double acc[W];
    if (W == 1 || e + 1 < g.n_local)
    {
      // (a ghost half is computed with its pair -- the entries of a pair do not meet -- and dropped)
      load<W>(out + e, acc);
      axpy_columns<W>(acc, V + e, ld, n_columns, c, sign);
    }
    else
    {
      double first[1] = {out[e]};
      axpy_columns<1>(first, V + e, ld, n_columns, c, sign);
      acc[0] = first[0];
      acc[W - 1] = first[0];
    }
    store_owned<W>(out + e, acc, in);
    if (kNorm)
    {
#pragma unroll
      for (int k = 0; k < W; ++k)
      {
        const double t = fma(acc[k], acc[k], nrm[0]);
        nrm[0] = in[k] ? t : nrm[0];
      }
    }
  }
  if (kNorm)
    block_column_sums<1>(nrm, norm_partials, wsum);
}

// norm_squared: ||w||^2 over all ranks, one device scalar (the partials of a rank are not the norm: the caller summed them)
template <int W, typename Index>
__device__ __forceinline__ void box_scale_store_body(RowWalkT<Index> const &g, double const *__restrict__ norm_squared, double const *w,
                                                     double *v_next, double *__restrict__ norm_out)
{
  const double norm = sqrt(norm_squared[0]);
  if (owns_tail() && norm_out != nullptr)
    norm_out[0] = norm;
  if (v_next == nullptr)
    return;
  const double inv = norm > 0. ? 1. / norm : 0.;
  for (Cursor<W, Index> cur(g); cur.inside(g); cur.advance(g))
  {
    bool in[W];
    const Index e = cur.entries(g, in);
    if (!in[0] && !in[W - 1])
      continue;
    double r[W];
    if (W == 1 || e + 1 < g.n_local)
      load<W>(w + e, r);
    else
      r[0] = r[W - 1] = w[e];
#pragma unroll
    for (int k = 0; k < W; ++k)
      r[k] *= inv;
    store_owned<W>(v_next + e, r, in);
  }
}
} // namespace body
} // namespace krylov
} // namespace mfmg
