// What the SpMV kernels of SparseMatrixDevice share: their arguments, the fused epilogues and the dispatch on the unknowns per
// node.  Included by the files that hold kernels (sparse_matrix_device.hip: one vector; sparse_matrix_block.hip: blocks of
// vectors); everything has internal linkage, each file compiles its own copy.
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
