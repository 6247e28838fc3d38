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
// The owned entries of a local vector in packed order (box_copy_kernel: x fastest over own_n[0] comps entries, then y, then z):
// packed entry i lies at base + x + row (i / rx % ny) + plane (i / (rx ny)).  Where x and y are owned whole the owned entries are one
// run (a slab): base + i.
struct OwnedIndex
{
  int64_t n_owned, base, rx, ny, row, plane;
  int contiguous;
};

// Index: the type the divisions run in (32 bits where the local vector is that short)
template <typename Index>
__global__ void block_dots_box_stage1_kernel(OwnedIndex o, int64_t ld, double const *X, double const *Y, double *partials)
{
  double const *x = X + (int64_t)blockIdx.y * ld, *y = Y + (int64_t)blockIdx.y * ld;
  const Index rx = (Index)o.rx, ny = (Index)o.ny;
  double acc = 0.;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < o.n_owned; i += (int64_t)gridDim.x * blockDim.x)
  {
    int64_t e = o.base + i;
    if (!o.contiguous)
    {
      const Index q = (Index)i / rx;
      e = o.base + (int64_t)((Index)i - q * rx) + (int64_t)(q % ny) * o.row + (int64_t)(q / ny) * o.plane;
    }
    acc += x[e] * y[e];
  }
  const double t = block_reduce_sum(acc);
  if (threadIdx.x == 0)
    partials[(int64_t)blockIdx.y * kReduceBlocks + blockIdx.x] = t;
}

// The direction as the one-vector driver forms it on several ranks, p.sadd(beta, 1., z) (vec::sadd_kernel): beta p is ROUNDED before
// z is added -- the compiler contracts s x + a v there into fma(a, v, s x) -- where block_cg_direction_kernel's z + beta p is one
// fma(beta, p, z).  No contraction in here, so that the two roundings stay two.
__global__ void block_cg_direction_local_kernel(int64_t n, int64_t ld, double const *Z, double *P, double const *rz_new, double const *rz_old,
                                                int first)
{
#pragma clang fp contract(off)
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
  {
    const double scaled = beta * p[i];
    p[i] = scaled + z[i];
  }
}

// block_cg_update_kernel without the partials of (R_s, R_s): on ranks that sum runs over the owned entries, on a grid of its own
__global__ void block_cg_update_local_kernel(int64_t n, int64_t ld, double const *P, double const *AP, double *R, int64_t ldx, double *X,
                                             int32_t const *slot_col, double const *rz, double const *pap_of)
{
  const int s = blockIdx.y;
  double const *p = P + (int64_t)s * ld, *Ap = AP + (int64_t)s * ld;
  double *r = R + (int64_t)s * ld, *x = X + (int64_t)slot_col[s] * ldx;
  const double pap = pap_of[s];
  const double alpha = (pap != 0.) ? double(rz[s] / pap) : double(0);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
  {
    x[i] += alpha * p[i];
    r[i] = r[i] - alpha * Ap[i];
  }
}

OwnedIndex owned_index(krylov::OwnedBox const &box)
{
  for (int d = 0; d < 3; ++d)
    if (box.own0[d] < 0 || box.own_n[d] < 1 || box.own0[d] + box.own_n[d] > box.local[d])
      throw std::runtime_error("internal: the owned box leaves the local box");
  OwnedIndex o;
  o.n_owned = box.n_owned();
  o.rx = box.own_n[0] * box.comps;
  o.ny = box.own_n[1];
  o.row = box.local[0] * box.comps;
  o.plane = o.row * box.local[1];
  o.base = box.own0[2] * o.plane + box.own0[1] * o.row + box.own0[0] * box.comps;
  o.contiguous = (box.own_n[0] == box.local[0] && box.own_n[1] == box.local[1]) ? 1 : 0;
  return o;
}
} // namespace

unsigned int reduction_blocks(int64_t n) { return n_blocks_for(n, block_size, kReduceBlocks); }
unsigned int reduction_blocks(krylov::OwnedBox const &box) { return reduction_blocks(box.n_owned()); }

void dots(HipHandle &h, krylov::OwnedBox const &box, int k, int64_t ld, double const *X, double const *Y, double *partials, double *out)
{
  if (k <= 0)
    return;
  const OwnedIndex o = owned_index(box);
  if (ld < box.n_local())
    throw std::runtime_error("internal: the leading dimension of a block of local vectors is at least their size");
  const unsigned int nb = block_krylov::reduction_blocks(box); // (qualified: krylov::reduction_blocks takes a box as well)
  hipEvent_t stop = h.profiler.begin("block_dots_box", 16. * double(o.n_owned) * k, h.stream);
  if (box.n_local() < (int64_t(1) << 31))
    hipLaunchKernelGGL(block_dots_box_stage1_kernel<uint32_t>, dim3(nb, k), dim3(block_size), 0, h.stream, o, ld, X, Y, partials);
  else
    hipLaunchKernelGGL(block_dots_box_stage1_kernel<int64_t>, dim3(nb, k), dim3(block_size), 0, h.stream, o, ld, X, Y, partials);
  hipLaunchKernelGGL(block_dots_stage2_kernel, dim3(1, k), dim3(block_size), 0, h.stream, (int)nb, partials, out);
  MFMG_HIP_CHECK(hipGetLastError());
  KernelProfiler::end(stop, h.stream);
}

void cg_direction_local(HipHandle &h, int64_t n, int k, int64_t ld, double const *Z, double *P, double const *rz_new, double const *rz_old,
                        bool first)
{
  if (k <= 0)
    return;
  hipEvent_t stop = h.profiler.begin("block_cg_direction_local", (first ? 16. : 24.) * double(n) * k, h.stream);
  hipLaunchKernelGGL(block_cg_direction_local_kernel, dim3(n_blocks_for(n, block_size, 256 * 16), k), dim3(block_size), 0, h.stream, n, ld,
                     Z, P, rz_new, rz_old, first ? 1 : 0);
  MFMG_HIP_CHECK(hipGetLastError());
  KernelProfiler::end(stop, h.stream);
}

void cg_update_local(HipHandle &h, int64_t n, int k, int64_t ld, double const *P, double const *AP, double *R, int64_t ldx, double *X,
                     int32_t const *slot_col, double const *rz, double const *pap)
{
  if (k <= 0)
    return;
  hipEvent_t stop = h.profiler.begin("block_cg_update_local", 48. * double(n) * k, h.stream);
  hipLaunchKernelGGL(block_cg_update_local_kernel, dim3(n_blocks_for(n, block_size, 256 * 16), k), dim3(block_size), 0, h.stream, n, ld, P,
                     AP, R, ldx, X, slot_col, rz, pap);
  MFMG_HIP_CHECK(hipGetLastError());
  KernelProfiler::end(stop, h.stream);
}

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
