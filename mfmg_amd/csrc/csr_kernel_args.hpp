// What the SpMV kernels of SparseMatrixDevice share: their arguments, the fused epilogues, the row body of the CSR kernels
// (lane_row_sum, RowOperands, row_operands, store_row) and the dispatch on the unknowns per node.  Included by the files that
// hold kernels (sparse_matrix_device.hip: one vector; sparse_matrix_block.hip, sparse_matrix_block_csr.hip: blocks of vectors);
// everything has internal linkage, each file compiles its own copy.
#pragma once

#include "sparse_matrix_device.hpp"

#include <type_traits>

namespace mfmg
{
namespace
{
template <typename T>
struct CsrArgs
{
  T const *val;
  int32_t const *col;
  int32_t const *row_ptr;
  int64_t n_rows;
  T const *x;
  T const *b;
  T const *dinv;
  T const *xprev;
  T *out;
  T alpha, beta;
  int mode;
  int pairs; // every vector the mode touches is 16-byte aligned: the two rows of a node are one access per operand (store_node)
  int32_t const *kept_ptr = nullptr; // after release_csr(): val / col hold the listed rows only, row q of the list at [kept_ptr[q], kept_ptr[q + 1])
};

// Which vectors the epilogue of a mode reads at the row it writes (x there -- not the gathered x --, b, D^-1, x_prev, and
// out as an input): what apply_mode checks and what the profiler counts.  On the device epilogue() is the statement of
// it; store_node, which requests the operands ahead of its stores, says it once more in place: through any function, this
// one included, its flags compile to other instruction streams in all 48 node kernels (two gain VGPRs).
struct CsrOperands
{
  bool x, b, dinv, xprev, out;
};
constexpr CsrOperands operands_of(CsrMode m)
{
  const bool smoother = m == CsrMode::first || m == CsrMode::next;
  return {smoother, smoother || m == CsrMode::residual || m == CsrMode::plus_scaled, smoother || m == CsrMode::plus_scaled,
          m == CsrMode::next, m == CsrMode::subtract || m == CsrMode::add};
}

// The fused epilogues (the modes of CsrMode): out at one row from the sum of the row.  The operands come as their vectors
// and the position i in them, the sum by address: each is read inside the case that uses it (the vectors a mode does not
// read are null pointers).  Passed as values they would be read in front of the switch, and the node kernels compile to
// other instruction streams.  No other mode reaches a kernel (apply_mode and the C ABI reject it), so `default` needs no
// code of its own: it stays on the last case, since an unreachable default changes the compare tree of every kernel with
// an epilogue and costs the LDS-cached kernels 4 to 6 VGPRs.
template <typename T>
__device__ __forceinline__ T epilogue(CsrMode mode, T const *sum, T const *x, T const *b, T const *dinv, T const *xprev,
                                      T const *old, int64_t i, T alpha, T beta)
{
  T o;
  switch (mode)
  {
  case CsrMode::apply:
    o = *sum;
    break;
  case CsrMode::residual:
    o = *sum - b[i];
    break;
  case CsrMode::first:
    o = x[i] - beta * dinv[i] * (*sum - b[i]);
    break;
  case CsrMode::next:
    o = x[i] + alpha * (x[i] - xprev[i]) - beta * dinv[i] * (*sum - b[i]);
    break;
  case CsrMode::subtract:
    o = old[i] - *sum;
    break;
  case CsrMode::plus_scaled:
    o = *sum + beta * dinv[i] * b[i];
    break;
  case CsrMode::add:
  default:
    o = old[i] + *sum;
    break;
  }
  return o;
}

// the epilogue of one row
template <typename T>
__device__ __forceinline__ void store_row(CsrArgs<T> const &a, int64_t row, T sum)
{
  a.out[row] = epilogue(static_cast<CsrMode>(a.mode), &sum, a.x, a.b, a.dinv, a.xprev, a.out, row, a.alpha, a.beta);
}

// Entries of a row that a lane keeps in flight (the batch of lane_row_sum and of the staging of csr_spmv_lds_kernel).
constexpr int kRowBatch = 4;

// The partial sum of one lane over a row: the entries p, p + S, p + 2 S, .. below e (S lanes share the row), x taken at
// idx[] -- the global x by column, or the LDS copy of csr_spmv_lds_kernel by local column.  Entry by entry a lane waits for
// (val, idx), then for x, with nothing of the next entry requested: two dependent round trips per entry in kernels bound
// by their latency.  Here B entries are one batch: all of its index and value loads, then all of its x reads, then the
// multiply-adds in ascending entry order, each through the one `sum += val * x` -- the chain of a lane is what it was,
// only the requests are earlier.  In the last, short batch of a row nothing is read past e, and an entry that is not
// there is SKIPPED, never added as a product with zero (the x it reads instead may be Inf or NaN, and a sum of -0 stays
// -0).
template <int S, int B, typename T, typename I, typename X>
__device__ __forceinline__ T lane_row_sum(T const *val, I const *idx, X const *x, int p, int e)
{
  T sum = T(0);
  I c[B];
  T v[B], xv[B];
  // (e - p, not p + (B - 1) S: no overflow at the end of 2^31 entries)
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
      xv[k] = x[c[k]];
#pragma unroll
    for (int k = 0; k < B; ++k)
      sum += v[k] * xv[k];
  }
  if (p < e)
  {
    // B - 1 entries at most, the first of them is there: an entry that is not reads at the first one's position instead
    // (under a branch of its own every load would be waited for with all requests before it: one after the other again)
#pragma unroll
    for (int k = 0; k < B - 1; ++k)
    {
      const int q = e - p > k * S ? p + k * S : p;
      c[k] = idx[q];
      v[k] = val[q];
    }
#pragma unroll
    for (int k = 0; k < B - 1; ++k)
      xv[k] = x[c[k]];
#pragma unroll
    for (int k = 0; k < B - 1; ++k)
      if (e - p > k * S)
        sum += v[k] * xv[k];
  }
  return sum;
}

// The operands of the epilogue at one row, requested ahead of the row loop by the lane that will store (store_row alone
// asks for them after the reduction: one more dependent round trip).  out as an operand (subtract, add) is read before
// the gathers of x, which is the same value only because launch() rejects out == x.
template <typename T>
struct RowOperands
{
  T x, b, dinv, xprev, out;
};
template <typename T>
__device__ __forceinline__ RowOperands<T> row_operands(CsrArgs<T> const &a, int64_t row)
{
  const CsrOperands need = operands_of(static_cast<CsrMode>(a.mode));
  RowOperands<T> o{};
  if (need.x)
    o.x = a.x[row];
  if (need.b)
    o.b = a.b[row];
  if (need.dinv)
    o.dinv = a.dinv[row];
  if (need.xprev)
    o.xprev = a.xprev[row];
  if (need.out)
    o.out = a.out[row];
  return o;
}
// the epilogue of one row from operands requested before (the one epilogue(): same expression, same bits)
template <typename T>
__device__ __forceinline__ void store_row(CsrArgs<T> const &a, int64_t row, T sum, RowOperands<T> const &o)
{
  a.out[row] = epilogue(static_cast<CsrMode>(a.mode), &sum, &o.x, &o.b, &o.dinv, &o.xprev, &o.out, int64_t(0), a.alpha, a.beta);
}

// f(std::integral_constant<int, c>()) for the unknowns per node c = 1 .. 4 of a layout
template <typename F>
void with_node_width(int c, F &&f)
{
  switch (c)
  {
  case 1:
    f(std::integral_constant<int, 1>());
    break;
  case 2:
    f(std::integral_constant<int, 2>());
    break;
  case 3:
    f(std::integral_constant<int, 3>());
    break;
  default:
    f(std::integral_constant<int, 4>());
    break;
  }
}
} // namespace
} // namespace mfmg
