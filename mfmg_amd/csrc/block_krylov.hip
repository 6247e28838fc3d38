// The vector passes of CG on a block of right-hand sides (block_krylov.hpp).  The loops, the reduction and the expressions are
// those of vector_ops.hip (dot_stage1_kernel, dot_stage2_kernel, cg_direction_kernel, cg_update_kernel) written the same way and
// compiled with the same flags: the compiler contracts a * b + c here where it does there, which is what makes a slot bit-equal
// to the one-vector kernels.  Grid-stride streaming loops with 8-byte accesses, consecutive lanes on consecutive entries.
#include "block_krylov.hpp"

namespace mfmg
{
namespace block_krylov
{
namespace
{
// (vector_ops.hip: the butterfly over the wavefront, then thread 0 sums the wavefronts in order)
__device__ __forceinline__ double block_reduce_sum(double v)
{
  __shared__ double wsum[16];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_xor(v, off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = (blockDim.x + 63) >> 6;
  if (lane == 0)
    wsum[wave] = v;
  __syncthreads();
  double total = 0.;
  if (threadIdx.x == 0)
    for (int w = 0; w < nw; ++w)
      total += wsum[w];
  return total; // valid in thread 0
}

__global__ void block_dots_stage1_kernel(int64_t n, int64_t ld, double const *X, double const *Y, double *partials)
{
  double const *x = X + (int64_t)blockIdx.y * ld, *y = Y + (int64_t)blockIdx.y * ld;
  double acc = 0.;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    acc += x[i] * y[i];
  const double t = block_reduce_sum(acc);
  if (threadIdx.x == 0)
    partials[(int64_t)blockIdx.y * kReduceBlocks + blockIdx.x] = t;
}

__global__ void block_dots_stage2_kernel(int n_partials, double const *partials, double *result)
{
  double const *mine = partials + (int64_t)blockIdx.y * kReduceBlocks;
  double acc = 0.;
  for (int i = threadIdx.x; i < n_partials; i += blockDim.x)
    acc += mine[i];
  const double t = block_reduce_sum(acc);
  if (threadIdx.x == 0)
    result[blockIdx.y] = t;
}

__global__ void block_cg_direction_kernel(int64_t n, int64_t ld, double const *Z, double *P, double const *rz_new, double const *rz_old,
                                          int first)
{
  double const *z = Z + (int64_t)blockIdx.y * ld;
  double *p = P + (int64_t)blockIdx.y * ld;
  if (first)
  {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
      p[i] = z[i];
    return;
  }
  const double old = rz_old[blockIdx.y];
  const double beta = (old != 0.) ? double(rz_new[blockIdx.y] / old) : double(0);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = z[i] + beta * p[i];
}

__global__ void block_cg_update_kernel(int64_t n, int64_t ld, double const *P, double const *AP, double *R, int64_t ldx, double *X,
                                       int32_t const *slot_col, double const *rz, double const *pap_of, double *partials)
{
  const int s = blockIdx.y;
  double const *p = P + (int64_t)s * ld, *Ap = AP + (int64_t)s * ld;
  double *r = R + (int64_t)s * ld, *x = X + (int64_t)slot_col[s] * ldx;
  const double pap = pap_of[s];
  const double alpha = (pap != 0.) ? double(rz[s] / pap) : double(0);
  double acc = 0.;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
  {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * Ap[i];
    r[i] = ri;
    acc += ri * ri;
  }
  const double t = block_reduce_sum(acc);
  if (threadIdx.x == 0)
    partials[(int64_t)s * kReduceBlocks + blockIdx.x] = t;
}
} // namespace

unsigned int reduction_blocks(int64_t n) { return n_blocks_for(n, block_size, kReduceBlocks); }

void dots(HipHandle &h, int64_t n, int k, int64_t ld, double const *X, double const *Y, double *partials, double *out)
{
  if (k <= 0)
    return;
  const unsigned int nb = reduction_blocks(n);
  hipEvent_t stop = h.profiler.begin("block_dots", 16. * double(n) * k, h.stream);
  hipLaunchKernelGGL(block_dots_stage1_kernel, dim3(nb, k), dim3(block_size), 0, h.stream, n, ld, X, Y, partials);
  hipLaunchKernelGGL(block_dots_stage2_kernel, dim3(1, k), dim3(block_size), 0, h.stream, (int)nb, partials, out);
  MFMG_HIP_CHECK(hipGetLastError());
  KernelProfiler::end(stop, h.stream);
}

void cg_direction(HipHandle &h, int64_t n, int k, int64_t ld, double const *Z, double *P, double const *rz_new, double const *rz_old,
                  bool first)
{
  if (k <= 0)
    return;
  hipEvent_t stop = h.profiler.begin("block_cg_direction", (first ? 16. : 24.) * double(n) * k, h.stream);
  hipLaunchKernelGGL(block_cg_direction_kernel, dim3(n_blocks_for(n, block_size, 256 * 16), k), dim3(block_size), 0, h.stream, n, ld, Z, P,
                     rz_new, rz_old, first ? 1 : 0);
  MFMG_HIP_CHECK(hipGetLastError());
  KernelProfiler::end(stop, h.stream);
}

void cg_update(HipHandle &h, int64_t n, int k, int64_t ld, double const *P, double const *AP, double *R, int64_t ldx, double *X,
               int32_t const *slot_col, double const *rz, double const *pap, double *partials, double *rr_out)
{
  if (k <= 0)
    return;
  const unsigned int nb = reduction_blocks(n);
  hipEvent_t stop = h.profiler.begin("block_cg_update", 48. * double(n) * k, h.stream);
  hipLaunchKernelGGL(block_cg_update_kernel, dim3(nb, k), dim3(block_size), 0, h.stream, n, ld, P, AP, R, ldx, X, slot_col, rz, pap,
                     partials);
  hipLaunchKernelGGL(block_dots_stage2_kernel, dim3(1, k), dim3(block_size), 0, h.stream, (int)nb, partials, rr_out);
  MFMG_HIP_CHECK(hipGetLastError());
  KernelProfiler::end(stop, h.stream);
}

int plan_retire(int n_active, int32_t const *retire_flags, int32_t *slot_col, int32_t *moves, int *n_active_out)
{
  int n_moves = 0, lo = 0, hi = n_active - 1;
  for (;;)
  {
    while (lo <= hi && !retire_flags[lo])
      ++lo; // the first retired slot not yet filled
    while (hi >= lo && retire_flags[hi])
      --hi; // the last survivor behind it
    if (lo > hi)
      break;
    moves[2 * n_moves] = hi;
    moves[2 * n_moves + 1] = lo;
    ++n_moves;
    slot_col[lo] = slot_col[hi];
    ++lo;
    --hi;
  }
  *n_active_out = hi + 1;
  return n_moves;
}
} // namespace block_krylov
} // namespace mfmg
