// gfx950 kernels of the agglomerate-wise restrictor (structured_restrictor.hpp).
//
// restrict : one thread per coarse row r = a E + e.  Consecutive lanes are consecutive rows, so every
//            plane is read as one contiguous run; the x entries of the patch are shared by the E rows of an
//            agglomerate and by neighbouring agglomerates (L1/L2).
// prolong  : one thread per fine node, owner computes (no atomics, fixed summation order).  A node lies
//            in at most two agglomerates per direction: the one it starts (position m = i mod a) and, on an
//            agglomerate boundary, the previous one (position m = a).  Lanes of even / odd nodes read two
//            planes at the rows of consecutive agglomerates; the two eigenvector passes use both halves of
//            every sector.
#include "structured_restrictor.hpp"

#include "mf_laplace.hpp" // mf_block_groups

#include <omp.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>

namespace mfmg
{
namespace
{
struct SrArgs
{
  double const *planes;
  float const *planes_f; // the same planes kept in float (every value representable in it); then `planes` is null
  int32_t const *node_dof; // nullptr: identity
  int64_t n_coarse;
  int N[3], na[3], a[3];
  int n_eig, patch;
  // agglomerates whose n_eig x patch block repeats a reference block bit for bit (interior agglomerates of a
  // constant-coefficient problem) are evaluated from `table[m * n_eig + e]`; nullptr: none
  uint8_t const *exc;
  uint8_t const *exc_node; // per fine node: 0 = every agglomerate it lies in is regular
  double const *table;
  // the other agglomerates: class of the block they repeat (0xffff: a block of their own, read from the planes)
  uint16_t const *cls;
  double const *class_table; // [class][patch][n_eig]
};

// plane entry / pair of plane entries (the two eigenvectors of an agglomerate) from whichever storage the planes have
__device__ __forceinline__ double sr_plane(SrArgs const &s, size_t idx)
{
  return s.planes_f != nullptr ? (double)s.planes_f[idx] : s.planes[idx];
}
__device__ __forceinline__ double2 sr_plane_pair(SrArgs const &s, size_t pair_idx)
{
  if (s.planes_f != nullptr)
  {
    const float2 v = reinterpret_cast<float2 const *>(s.planes_f)[pair_idx];
    return make_double2((double)v.x, (double)v.y);
  }
  return reinterpret_cast<double2 const *>(s.planes)[pair_idx];
}

__global__ __launch_bounds__(256) void sr_restrict_kernel(SrArgs s, double const *x, double *y)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= s.n_coarse)
    return;
  const int64_t ag = r / s.n_eig;
  const int ai = ag % s.na[0], aj = (ag / s.na[0]) % s.na[1], ak = ag / ((int64_t)s.na[0] * s.na[1]);
  const int64_t base = (int64_t)ai * s.a[0] + (int64_t)s.N[0] * ((int64_t)aj * s.a[1] + (int64_t)s.N[1] * ((int64_t)ak * s.a[2]));
  double sum = 0.;
  int m = 0;
  for (int mz = 0; mz <= s.a[2]; ++mz)
    for (int my = 0; my <= s.a[1]; ++my)
    {
      const int64_t row = base + (int64_t)s.N[0] * (my + (int64_t)s.N[1] * mz);
#pragma unroll 3
      for (int mx = 0; mx <= s.a[0]; ++mx, ++m)
      {
        const int64_t node = row + mx;
        const int64_t id = s.node_dof ? (int64_t)s.node_dof[node] : node;
        sum += sr_plane(s, (size_t)m * s.n_coarse + r) * x[id];
      }
    }
  y[r] = sum;
}

// two eigenvectors per agglomerate: one thread per agglomerate, both rows at once (the x values of the patch are
// fetched once, the two plane entries in one 16-byte request); the sums are formed as in the row kernel
// A = 2: 2 x 2 x 2 agglomerates with the loops unrolled, so that the 27 independent requests of a thread are in
// flight together (with run-time bounds they went out three at a time: latency, not bytes); A = 0: any size
template <int A>
__global__ __launch_bounds__(256) void sr_restrict_pair_kernel(SrArgs s, double const *x, double *y)
{
  const int a0 = A > 0 ? A : s.a[0], a1 = A > 0 ? A : s.a[1], a2 = A > 0 ? A : s.a[2];
  // workgroups are dealt to the 8 XCDs in turn: give every XCD a contiguous run of agglomerates, so that the node
  // planes two layers of agglomerates share stay in one L2 (the grid is a multiple of 8)
  const int64_t bid = (int64_t)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int64_t ag = bid * (int64_t)blockDim.x + threadIdx.x;
  if (2 * ag >= s.n_coarse)
    return;
  const int ai = ag % s.na[0], aj = (ag / s.na[0]) % s.na[1], ak = ag / ((int64_t)s.na[0] * s.na[1]);
  const int64_t base = (int64_t)ai * a0 + (int64_t)s.N[0] * ((int64_t)aj * a1 + (int64_t)s.N[1] * ((int64_t)ak * a2));
  const size_t stride = (size_t)s.n_coarse / 2;
  const bool regular = s.exc != nullptr && s.exc[ag] == 0;
  // a block shared with other agglomerates comes from the class table (cached) instead of the planes (HBM)
  const unsigned int cl = (!regular && s.cls != nullptr) ? s.cls[ag] : 0xffffu;
  double2 const *ct = reinterpret_cast<double2 const *>(s.class_table) + (size_t)(cl == 0xffffu ? 0 : cl) * s.patch;
  double sum0 = 0., sum1 = 0.;
  if constexpr (A == 2)
  {
    // all 27 x requests first (they do not depend on where the weights come from), then one loop per source
    double xv[27];
#pragma unroll
    for (int m = 0; m < 27; ++m)
    {
      const int64_t node = base + (m % 3) + (int64_t)s.N[0] * ((m / 3) % 3 + (int64_t)s.N[1] * (m / 9));
      xv[m] = x[s.node_dof ? (int64_t)s.node_dof[node] : node];
    }
    if (regular)
    {
#pragma unroll
      for (int m = 0; m < 27; ++m)
      {
        sum0 += s.table[2 * m] * xv[m]; // wave-uniform addresses
        sum1 += s.table[2 * m + 1] * xv[m];
      }
    }
    else if (cl != 0xffffu)
    {
#pragma unroll
      for (int m = 0; m < 27; ++m)
      {
        const double2 pv = ct[m];
        sum0 += pv.x * xv[m];
        sum1 += pv.y * xv[m];
      }
    }
    else
    {
#pragma unroll
      for (int m = 0; m < 27; ++m)
      {
        const double2 pv = sr_plane_pair(s, (size_t)m * stride + ag);
        sum0 += pv.x * xv[m];
        sum1 += pv.y * xv[m];
      }
    }
  }
  else
  {
    int m = 0;
    for (int mz = 0; mz <= a2; ++mz)
      for (int my = 0; my <= a1; ++my)
      {
        const int64_t row = base + (int64_t)s.N[0] * (my + (int64_t)s.N[1] * mz);
#pragma unroll 3
        for (int mx = 0; mx <= a0; ++mx, ++m)
        {
          const int64_t node = row + mx;
          const int64_t id = s.node_dof ? (int64_t)s.node_dof[node] : node;
          double2 pv;
          if (regular)
            pv = make_double2(s.table[2 * m], s.table[2 * m + 1]); // wave-uniform address
          else if (cl != 0xffffu)
            pv = ct[m];
          else
            pv = sr_plane_pair(s, (size_t)m * stride + ag);
          const double xv = x[id];
          sum0 += pv.x * xv;
          sum1 += pv.y * xv;
        }
      }
  }
  reinterpret_cast<double2 *>(y)[ag] = make_double2(sum0, sum1);
}

// (sr_prolong_listed222_part below forms the same sum for 2 x 2 x 2 agglomerates with two eigenvectors with its requests in one
// batch: candidate order, m, the plane index p0 / 2 and the choice table / class table / planes must stay in step with this)
// (R^T y) at fine node `node`: a node lies in at most two agglomerates per direction, the one it starts
// (position m = i mod a) and, on an agglomerate boundary, the previous one (position m = a); fixed order
// (z, y, x candidates, then eigenvectors)
__device__ __forceinline__ double sr_node_value(SrArgs const &s, double const *y, int64_t node)
{
  const int i = node % s.N[0], j = (node / s.N[0]) % s.N[1], k = node / ((int64_t)s.N[0] * s.N[1]);
  // candidate agglomerates per direction: c = 0 the one the node starts, c = 1 the previous one
  int ax[2], mx[2], ay[2], my[2], az[2], mz[2];
  auto candidates = [](int idx, int a, int na, int ag[2], int mm[2]) {
    ag[0] = idx / a;
    mm[0] = idx % a;
    if (ag[0] >= na)
      ag[0] = -1;
    ag[1] = (idx % a == 0 && idx / a >= 1) ? idx / a - 1 : -1;
    mm[1] = a;
  };
  candidates(i, s.a[0], s.na[0], ax, mx);
  candidates(j, s.a[1], s.na[1], ay, my);
  candidates(k, s.a[2], s.na[2], az, mz);
  const int px = s.a[0] + 1, py = s.a[1] + 1;
  const bool table = s.exc_node != nullptr && s.exc_node[node] == 0; // all agglomerates around regular (n_eig = 2)
  double sum = 0.;
  for (int cz = 0; cz < 2; ++cz)
  {
    if (az[cz] < 0)
      continue;
    for (int cy = 0; cy < 2; ++cy)
    {
      if (ay[cy] < 0)
        continue;
      for (int cx = 0; cx < 2; ++cx)
      {
        if (ax[cx] < 0)
          continue;
        const int64_t ag = ax[cx] + (int64_t)s.na[0] * (ay[cy] + (int64_t)s.na[1] * az[cz]);
        const int m = mx[cx] + px * (my[cy] + py * mz[cz]);
        const size_t p0 = (size_t)m * s.n_coarse + ag * s.n_eig;
        double const *yy = y + ag * s.n_eig;
        if (s.n_eig == 2)
        {
          // both eigenvectors of the agglomerate in one 16-byte request (rows 2 ag, 2 ag + 1 are adjacent)
          const double2 yv = *reinterpret_cast<double2 const *>(yy);
          double2 pv;
          if (table)
            pv = *reinterpret_cast<double2 const *>(s.table + 2 * m);
          else
          {
            const unsigned int cl = s.cls != nullptr ? s.cls[ag] : 0xffffu;
            pv = cl != 0xffffu ? reinterpret_cast<double2 const *>(s.class_table)[(size_t)cl * s.patch + m]
                               : sr_plane_pair(s, p0 / 2);
          }
          sum += pv.x * yv.x;
          sum += pv.y * yv.y;
        }
        else
          for (int e = 0; e < s.n_eig; ++e)
            sum += sr_plane(s, p0 + e) * yy[e];
      }
    }
  }
  return sum;
}

// one thread per fine node (any agglomerate size, any numbering)
__global__ __launch_bounds__(256) void sr_prolong_kernel(SrArgs s, double const *y, double *out, int subtract)
{
  const int64_t node = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t n_nodes = (int64_t)s.N[0] * s.N[1] * s.N[2];
  if (node >= n_nodes)
    return;
  const double sum = sr_node_value(s, y, node);
  const int64_t id = s.node_dof ? (int64_t)s.node_dof[node] : node;
  out[id] = subtract ? out[id] - sum : sum;
}

// ---- blocks of vectors: K = 2 or 4 columns per launch (column c of x at x + c * ldx) ---------------------------------------
// The planes are the largest stream of the transfers (16 B per agglomerate and patch node against 8 B of fine vector per node
// and column): a block launch fetches every plane pair / table entry / class-table entry ONCE for its K columns.  Column c
// gets the bits of the one-vector launch on that column: every sum is formed over the same terms in the same order with the
// same expression shapes.  Leading dimensions are even and the bases aligned to 16 bytes (the double2 accesses).

// rows form: one thread per coarse row, K sums
template <int K>
__global__ __launch_bounds__(256) void sr_restrict_rows_block_kernel(SrArgs s, double const *x, int64_t ldx, double *y, int64_t ldy)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= s.n_coarse)
    return;
  const int64_t ag = r / s.n_eig;
  const int ai = ag % s.na[0], aj = (ag / s.na[0]) % s.na[1], ak = ag / ((int64_t)s.na[0] * s.na[1]);
  const int64_t base = (int64_t)ai * s.a[0] + (int64_t)s.N[0] * ((int64_t)aj * s.a[1] + (int64_t)s.N[1] * ((int64_t)ak * s.a[2]));
  double sum[K];
#pragma unroll
  for (int c = 0; c < K; ++c)
    sum[c] = 0.;
  int m = 0;
  for (int mz = 0; mz <= s.a[2]; ++mz)
    for (int my = 0; my <= s.a[1]; ++my)
    {
      const int64_t row = base + (int64_t)s.N[0] * (my + (int64_t)s.N[1] * mz);
#pragma unroll 3
      for (int mx = 0; mx <= s.a[0]; ++mx, ++m)
      {
        const int64_t node = row + mx;
        const int64_t id = s.node_dof ? (int64_t)s.node_dof[node] : node;
        const double pv = sr_plane(s, (size_t)m * s.n_coarse + r);
#pragma unroll
        for (int c = 0; c < K; ++c)
          sum[c] += pv * x[id + c * ldx];
      }
    }
#pragma unroll
  for (int c = 0; c < K; ++c)
    y[r + c * ldy] = sum[c];
}

// pair form: one thread per agglomerate, both rows of the K columns.  A = 2: the one-vector kernel keeps its 27 x values and 27
// pairs in flight together; K times the x values do not fit a register file that way, so the requests go out one z-layer of
// the patch at a time: 9 pairs and 9 K values, then the 18 K multiply-adds of the layer in the order m = 0 .. 26.
template <int A, int K>
__global__ __launch_bounds__(256) void sr_restrict_pair_block_kernel(SrArgs s, double const *x, int64_t ldx, double *y, int64_t ldy)
{
  const int a0 = A > 0 ? A : s.a[0], a1 = A > 0 ? A : s.a[1], a2 = A > 0 ? A : s.a[2];
  // (the XCD re-dealing of sr_restrict_pair_kernel: the grid is a multiple of 8)
  const int64_t bid = (int64_t)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int64_t ag = bid * (int64_t)blockDim.x + threadIdx.x;
  if (2 * ag >= s.n_coarse)
    return;
  const int ai = ag % s.na[0], aj = (ag / s.na[0]) % s.na[1], ak = ag / ((int64_t)s.na[0] * s.na[1]);
  const int64_t base = (int64_t)ai * a0 + (int64_t)s.N[0] * ((int64_t)aj * a1 + (int64_t)s.N[1] * ((int64_t)ak * a2));
  const size_t stride = (size_t)s.n_coarse / 2;
  const bool regular = s.exc != nullptr && s.exc[ag] == 0;
  const unsigned int cl = (!regular && s.cls != nullptr) ? s.cls[ag] : 0xffffu;
  // one source of pairs per thread: entry m at src[m * step] -- the reference table, the class table, or the planes in double;
  // planes kept in float are widened as they arrive
  const bool from_float = !regular && cl == 0xffffu && s.planes_f != nullptr;
  double2 const *src = reinterpret_cast<double2 const *>(s.table);
  size_t step = 1;
  if (!regular && cl != 0xffffu)
    src = reinterpret_cast<double2 const *>(s.class_table) + (size_t)cl * s.patch;
  else if (!regular && !from_float)
  {
    src = reinterpret_cast<double2 const *>(s.planes) + ag;
    step = stride;
  }
  float2 const *src_f = reinterpret_cast<float2 const *>(s.planes_f) + ag;
  double sum0[K], sum1[K];
#pragma unroll
  for (int c = 0; c < K; ++c)
    sum0[c] = sum1[c] = 0.;
  if constexpr (A == 2)
  {
    // (not unrolled: unrolled, the requests of all three layers were hoisted to the front -- 334 VGPRs at K = 4)
#pragma unroll 1
    for (int mz = 0; mz < 3; ++mz)
    {
      double xv[9][K];
      double2 pv[9];
#pragma unroll
      for (int q = 0; q < 9; ++q)
      {
        const int64_t node = base + (q % 3) + (int64_t)s.N[0] * (q / 3 + (int64_t)s.N[1] * mz);
        const int64_t id = s.node_dof ? (int64_t)s.node_dof[node] : node;
#pragma unroll
        for (int c = 0; c < K; ++c)
          xv[q][c] = x[id + c * ldx];
      }
      if (from_float)
      {
#pragma unroll
        for (int q = 0; q < 9; ++q)
        {
          const float2 v = src_f[(size_t)(9 * mz + q) * stride];
          pv[q] = make_double2((double)v.x, (double)v.y);
        }
      }
      else
      {
#pragma unroll
        for (int q = 0; q < 9; ++q)
          pv[q] = src[(size_t)(9 * mz + q) * step];
      }
#pragma unroll
      for (int q = 0; q < 9; ++q)
#pragma unroll
        for (int c = 0; c < K; ++c)
        {
          sum0[c] += pv[q].x * xv[q][c];
          sum1[c] += pv[q].y * xv[q][c];
        }
    }
  }
  else
  {
    int m = 0;
    for (int mz = 0; mz <= a2; ++mz)
      for (int my = 0; my <= a1; ++my)
      {
        const int64_t row = base + (int64_t)s.N[0] * (my + (int64_t)s.N[1] * mz);
#pragma unroll 3
        for (int mx = 0; mx <= a0; ++mx, ++m)
        {
          const int64_t node = row + mx;
          const int64_t id = s.node_dof ? (int64_t)s.node_dof[node] : node;
          double2 pv;
          if (from_float)
          {
            const float2 v = src_f[(size_t)m * stride];
            pv = make_double2((double)v.x, (double)v.y);
          }
          else
            pv = src[(size_t)m * step];
#pragma unroll
          for (int c = 0; c < K; ++c)
          {
            const double xv = x[id + c * ldx];
            sum0[c] += pv.x * xv;
            sum1[c] += pv.y * xv;
          }
        }
      }
  }
#pragma unroll
  for (int c = 0; c < K; ++c)
    reinterpret_cast<double2 *>(y + c * ldy)[ag] = make_double2(sum0[c], sum1[c]);
}

// nodes form of R^T y: one thread per fine node, the K sums of sr_node_value (z, y, x candidates, then the eigenvectors) from
// plane pairs read once; SUB (out -= R^T y) as a template parameter, the K entries of out requested first
template <bool SUB, int K>
__global__ __launch_bounds__(256) void sr_prolong_block_kernel(SrArgs s, double const *y, int64_t ldy, double *out, int64_t ldo)
{
  const int64_t node = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t n_nodes = (int64_t)s.N[0] * s.N[1] * s.N[2];
  if (node >= n_nodes)
    return;
  const int64_t id = s.node_dof ? (int64_t)s.node_dof[node] : node;
  double o[K], sum[K];
#pragma unroll
  for (int c = 0; c < K; ++c)
  {
    o[c] = SUB ? out[id + c * ldo] : 0.;
    sum[c] = 0.;
  }
  const int i = node % s.N[0], j = (node / s.N[0]) % s.N[1], k = node / ((int64_t)s.N[0] * s.N[1]);
  int ax[2], mx[2], ay[2], my[2], az[2], mz[2];
  auto candidates = [](int idx, int a, int na, int ag[2], int mm[2]) {
    ag[0] = idx / a;
    mm[0] = idx % a;
    if (ag[0] >= na)
      ag[0] = -1;
    ag[1] = (idx % a == 0 && idx / a >= 1) ? idx / a - 1 : -1;
    mm[1] = a;
  };
  candidates(i, s.a[0], s.na[0], ax, mx);
  candidates(j, s.a[1], s.na[1], ay, my);
  candidates(k, s.a[2], s.na[2], az, mz);
  const int px = s.a[0] + 1, py = s.a[1] + 1;
  const bool table = s.exc_node != nullptr && s.exc_node[node] == 0;
  for (int cz = 0; cz < 2; ++cz)
  {
    if (az[cz] < 0)
      continue;
    for (int cy = 0; cy < 2; ++cy)
    {
      if (ay[cy] < 0)
        continue;
      for (int cx = 0; cx < 2; ++cx)
      {
        if (ax[cx] < 0)
          continue;
        const int64_t ag = ax[cx] + (int64_t)s.na[0] * (ay[cy] + (int64_t)s.na[1] * az[cz]);
        const int m = mx[cx] + px * (my[cy] + py * mz[cz]);
        const size_t p0 = (size_t)m * s.n_coarse + ag * s.n_eig;
        double const *yy = y + ag * s.n_eig;
        if (s.n_eig == 2)
        {
          double2 yv[K];
#pragma unroll
          for (int c = 0; c < K; ++c)
            yv[c] = *reinterpret_cast<double2 const *>(yy + c * ldy);
          double2 pv;
          if (table)
            pv = *reinterpret_cast<double2 const *>(s.table + 2 * m);
          else
          {
            const unsigned int cl = s.cls != nullptr ? s.cls[ag] : 0xffffu;
            pv = cl != 0xffffu ? reinterpret_cast<double2 const *>(s.class_table)[(size_t)cl * s.patch + m]
                               : sr_plane_pair(s, p0 / 2);
          }
#pragma unroll
          for (int c = 0; c < K; ++c)
          {
            sum[c] += pv.x * yv[c].x;
            sum[c] += pv.y * yv[c].y;
          }
        }
        else
          for (int e = 0; e < s.n_eig; ++e)
          {
            const double pv = sr_plane(s, p0 + e);
#pragma unroll
            for (int c = 0; c < K; ++c)
              sum[c] += pv * yy[e + c * ldy];
          }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < K; ++c)
    out[id + c * ldo] = SUB ? o[c] - sum[c] : sum[c];
}

// the nodes of the listed agglomerate positions: a thread per node (the first workgroups of the block kernel)
template <bool SUB>
__device__ __forceinline__ void sr_prolong_listed_part(SrArgs const &s, double const *y, double *out, int32_t const *blocks, int64_t n_blocks)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= 8 * n_blocks)
    return;
  const int64_t v = blocks[t >> 3];
  const int d = (int)(t & 7);
  const int vx = s.na[0] + 1, vy = s.na[1] + 1;
  const int i = 2 * (int)(v % vx) + (d & 1), j = 2 * (int)((v / vx) % vy) + ((d >> 1) & 1),
            k = 2 * (int)(v / ((int64_t)vx * vy)) + (d >> 2);
  if (i >= s.N[0] || j >= s.N[1] || k >= s.N[2])
    return;
  const int64_t node = i + (int64_t)s.N[0] * (j + (int64_t)s.N[1] * k);
  const double sum = sr_node_value(s, y, node);
  out[node] = SUB ? out[node] - sum : sum;
}

// 2 x 2 x 2 agglomerates, two eigenvectors, lexicographic numbering, table-driven blocks: one thread per
// agglomerate position (na + 1 per direction) finishes the 2 x 2 x 2 nodes at the low corner of its agglomerate.
// The y pairs of the (at most) eight agglomerates around are fetched once for the eight nodes, the table
// entries are wave-uniform; every sum is formed in the order of sr_node_value (same bits).
struct __attribute__((aligned(8))) sr_pair
{
  double x, y;
};

// Both parts in ONE launch: the first `listed_blocks` workgroups take the nodes of the listed agglomerate positions (the
// blocks the table-driven part leaves out: a thread per node, latency-bound, so they start first and run beside the
// rest), the others one agglomerate position per thread.  The two nodes 2 i, 2 i + 1 of a row are read / written as one
// 16-byte access: consecutive lanes, consecutive addresses (with 8-byte accesses at a stride of 16 every request used
// half of what it touched).
// SUB (x -= R^T y, the cycle's form) is a template parameter: as a run-time flag every read of `out` sat in a block of its own
// behind a uniform branch with a wait for ALL outstanding loads behind it -- four round trips in a row -- and the 54 table entries
// were fetched by per-lane vector loads with three more waits (the ISA of round 4's kernel; a wavefront lived 11 us for 24 memory
// instructions).  The table is read through the constant address space: scalar loads, whatever the stores of the kernel are.
template <bool SUB>
__global__ __launch_bounds__(256) void sr_prolong_block222_kernel(SrArgs s, double const *y, double *out,
                                                                  uint8_t const *blk_exc, int32_t const *blocks, int64_t n_blocks,
                                                                  unsigned int listed_blocks)
{
  constexpr int subtract = SUB ? 1 : 0;
  typedef __attribute__((address_space(4))) const double ctable_t;
  ctable_t *table = reinterpret_cast<ctable_t *>(reinterpret_cast<uintptr_t>(s.table));
  if (blockIdx.x < listed_blocks)
  {
    sr_prolong_listed_part<SUB>(s, y, out, blocks, n_blocks);
    return;
  }
  const int64_t t = (int64_t)(blockIdx.x - listed_blocks) * blockDim.x + threadIdx.x;
  const int vx = s.na[0] + 1, vy = s.na[1] + 1, vz = s.na[2] + 1;
  if (t >= (int64_t)vx * vy * vz || blk_exc[t] != 0)
    return;
  const int vi = t % vx, vj = (t / vx) % vy, vk = t / ((int64_t)vx * vy);
  // Every request of the thread is issued UNCONDITIONALLY, at a clamped position, and masked afterwards: with a branch around each
  // of them (`has ? y[..] : 0`, `if (live) ...`) every load sat in a basic block of its own with its wait behind it -- twelve
  // dependent round trips per wavefront (the ISA: 127 exec branches, 105 waits; the counters: 1.5 MB in flight, profiles/r04_n).
  double2 yv[8];
  bool has[8];
#pragma unroll
  for (int sidx = 0; sidx < 8; ++sidx)
  {
    const int qi = vi - (sidx & 1), qj = vj - ((sidx >> 1) & 1), qk = vk - (sidx >> 2);
    has[sidx] = qi >= 0 && qi < s.na[0] && qj >= 0 && qj < s.na[1] && qk >= 0 && qk < s.na[2];
    const int ci = min(max(qi, 0), s.na[0] - 1), cj = min(max(qj, 0), s.na[1] - 1), ck = min(max(qk, 0), s.na[2] - 1);
    yv[sidx] = reinterpret_cast<double2 const *>(y)[ci + (int64_t)s.na[0] * (cj + (int64_t)s.na[1] * ck)];
  }
  const bool pair = 2 * vi + 1 < s.N[0];
  // the four rows this thread finishes: all four reads of `out` are requested up front, together with the y pairs above
  // (row by row each read waited behind the store of the row before: out may alias out, four dependent round trips).  The last
  // position of a row (one node, no pair) reads the 16 bytes that END at its node.
  bool live[4];
  double *orow[4];
  sr_pair ov[4];
#pragma unroll
  for (int dyz = 0; dyz < 4; ++dyz)
  {
    const int j = 2 * vj + (dyz & 1), k = 2 * vk + (dyz >> 1);
    live[dyz] = j < s.N[1] && k < s.N[2];
    orow[dyz] = out + 2 * vi + (int64_t)s.N[0] * (min(j, s.N[1] - 1) + (int64_t)s.N[1] * min(k, s.N[2] - 1));
    ov[dyz] = sr_pair{0., 0.};
    if (subtract)
    {
      const sr_pair t = *reinterpret_cast<sr_pair const *>(orow[dyz] - (pair ? 0 : 1));
      ov[dyz].x = pair ? t.x : t.y;
      ov[dyz].y = pair ? t.y : 0.;
    }
  }
#pragma unroll
  for (int sidx = 0; sidx < 8; ++sidx)
    if (!has[sidx])
      yv[sidx] = make_double2(0., 0.); // (an agglomerate outside the mesh contributes exact zeros below)
#pragma unroll
  for (int dyz = 0; dyz < 4; ++dyz)
  {
    const int dy = dyz & 1, dz = dyz >> 1;
    if (!live[dyz])
      continue;
    double sums[2];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
    {
      double sum = 0.; // (formed in the order of sr_node_value: same bits)
#pragma unroll
      for (int sz = 0; sz < 2; ++sz)
#pragma unroll
        for (int sy = 0; sy < 2; ++sy)
#pragma unroll
          for (int sx = 0; sx < 2; ++sx)
          {
            if ((sx && dx) || (sy && dy) || (sz && dz))
              continue; // the previous agglomerate holds the node only on the shared boundary
            const int sidx = sx + 2 * sy + 4 * sz;
            const int m = (sx ? 2 : dx) + 3 * ((sy ? 2 : dy) + 3 * (sz ? 2 : dz));
            sum += table[2 * m] * yv[sidx].x;
            sum += table[2 * m + 1] * yv[sidx].y;
          }
      sums[dx] = sum;
    }
    sr_pair v = ov[dyz];
    v.x = subtract ? v.x - sums[0] : sums[0];
    v.y = subtract ? v.y - sums[1] : sums[1];
    if (pair)
      *reinterpret_cast<sr_pair *>(orow[dyz]) = v;
    else
      orow[dyz][0] = v.x;
  }
}

// The listed positions for the marching kernel: a thread per node and the sums of sr_node_value again (2 x 2 x 2 agglomerates, two
// eigenvectors, lexicographic ids), but every request of a thread leaves before the first answer is used.  sr_node_value asks
// for the class of an agglomerate, then for its block entry, then for the y pair, candidate after candidate behind branches:
// some twenty dependent round trips per wavefront, and on the bench mesh the 9 % of the nodes that lie at the faces of the box
// took as long as all the others.  Here: the position, then y pairs, classes and out for all eight candidates at once
// (agglomerates outside the mesh at a clamped index), then the eight block entries, then the sum -- over the candidates that
// exist, in the same order, so the same bits.
template <bool SUB>
__device__ __forceinline__ void sr_prolong_listed222_part(SrArgs const &s, double const *y, double *out, int32_t const *blocks, int64_t n_blocks,
                                                          unsigned int block)
{
  const int64_t t = block * (int64_t)blockDim.x + threadIdx.x;
  if (t >= 8 * n_blocks)
    return;
  const int64_t v = blocks[t >> 3];
  const int d = (int)(t & 7);
  const int vx = s.na[0] + 1, vy = s.na[1] + 1;
  const int idx[3] = {2 * (int)(v % vx) + (d & 1), 2 * (int)((v / vx) % vy) + ((d >> 1) & 1), 2 * (int)(v / ((int64_t)vx * vy)) + (d >> 2)};
  if (idx[0] >= s.N[0] || idx[1] >= s.N[1] || idx[2] >= s.N[2])
    return;
  const int64_t node = idx[0] + (int64_t)s.N[0] * (idx[1] + (int64_t)s.N[1] * idx[2]);
  // candidate agglomerates per direction, as in sr_node_value: [0] the one the node starts, [1] the previous one
  int ag[3][2], mm[3][2];
#pragma unroll
  for (int q = 0; q < 3; ++q)
  {
    ag[q][0] = idx[q] / 2 < s.na[q] ? idx[q] / 2 : -1;
    mm[q][0] = idx[q] % 2;
    ag[q][1] = (idx[q] % 2 == 0 && idx[q] / 2 >= 1) ? idx[q] / 2 - 1 : -1;
    mm[q][1] = 2;
  }
  const bool table = s.exc_node != nullptr && s.exc_node[node] == 0;
  const double o = SUB ? out[node] : 0.;
  bool valid[8];
  int64_t agc[8];
  int m[8];
  double2 yv[8], pv[8];
  unsigned int cl[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
  {
    const int cz = c >> 2, cy = (c >> 1) & 1, cx = c & 1;
    valid[c] = ag[2][cz] >= 0 && ag[1][cy] >= 0 && ag[0][cx] >= 0;
    agc[c] = valid[c] ? ag[0][cx] + (int64_t)s.na[0] * (ag[1][cy] + (int64_t)s.na[1] * ag[2][cz]) : 0;
    m[c] = mm[0][cx] + 3 * (mm[1][cy] + 3 * mm[2][cz]);
    yv[c] = reinterpret_cast<double2 const *>(y)[agc[c]];
    cl[c] = s.cls != nullptr ? s.cls[agc[c]] : 0xffffu;
  }
  double2 const *table2 = reinterpret_cast<double2 const *>(s.table), *class2 = reinterpret_cast<double2 const *>(s.class_table),
                *planes2 = reinterpret_cast<double2 const *>(s.planes);
  const size_t stride = (size_t)s.n_coarse / 2;
#pragma unroll
  for (int c = 0; c < 8; ++c)
  {
    // one request whatever the source: the reference table, the class table, or the planes (kept in float: below)
    double2 const *src = table2 + m[c];
    if (!table && cl[c] != 0xffffu)
      src = class2 + (size_t)cl[c] * s.patch + m[c];
    else if (!table && planes2 != nullptr)
      src = planes2 + (size_t)m[c] * stride + agc[c];
    pv[c] = *src;
  }
  if (s.planes_f != nullptr)
  {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (valid[c] && !table && cl[c] == 0xffffu)
        pv[c] = sr_plane_pair(s, (size_t)m[c] * stride + agc[c]);
  }
  double sum = 0.;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (valid[c])
    {
      sum += pv[c].x * yv[c].x;
      sum += pv[c].y * yv[c].y;
    }
  out[node] = SUB ? o - sum : sum;
}

// ---- the same as a march -------------------------------------------------------------------------------------------------
// The block kernel asks for the y pair of an agglomerate from eight threads and lives for one round trip.  Here a wavefront
// owns 64 consecutive agglomerate positions of one row (vj) and marches through `len` layers of positions (vk):
//   y    : a lane requests the pairs of its own agglomerate column in the rows vj and vj - 1, once per layer, 16 bytes each;
//          the column before (vi - 1) is the previous lane's (DPP wave shift; lane 0 gets it from a wave-uniform request), the
//          layer before (vk - 1) is carried in registers from the step before.  A pair is requested by two wavefronts of
//          neighbouring rows (the same workgroup) instead of eight threads.
//   out  : the four node rows of layer vk + 1 and that layer's pairs are requested before the sums of layer vk are formed
//          (buffer descriptors: a per-lane offset that never changes and a scalar offset per row), so that two layers of
//          requests are in flight per wavefront and a wait stands only in front of the first use.
//   pairs: node rows start 8 bytes further on from row to row (odd row lengths), so in the rows at an odd distance from the
//          start of the vector a lane takes the nodes (2 vi - 1, 2 vi) instead of (2 vi, 2 vi + 1) -- the last node of the
//          position before and the first of its own, both formed from the very pairs it holds anyway -- and every 16-byte
//          access of a row is aligned: a wavefront reads and writes one contiguous, aligned kilobyte per row; the first node
//          of such a row and the last node of the others are single 8-byte stores (head and tail).
// A node is read and written by the one lane that owns it; a lane at either end of a row reads its pair one node further
// inside and drops the foreign half, and the last step of a march requests its own layer once more and drops all of it.  Every sum is formed in the order of sr_node_value (the same bits as the block kernel).
// Waves share nothing (no LDS, no barrier): the ones of a workgroup are neighbouring rows, for the vector cache.
constexpr int kMarchWaves = 4; // rows vj of a workgroup

struct SrMarch
{
  int lo[3], hi[3]; // box of the agglomerate positions the tables serve (the march covers it; positions in the list are masked)
  int strips, wgs_y, chunks, len;
  unsigned int n_wgs, blocks; // workgroups with work / in the grid (a multiple of 8)
  unsigned int y_bytes, out_bytes;
};

typedef unsigned int sr_v4u __attribute__((ext_vector_type(4)));
typedef unsigned int sr_v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ sr_pair sr_ld_pair(__amdgpu_buffer_rsrc_t r, unsigned int voff, unsigned int soff)
{
  const sr_v4u v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
  sr_pair p;
  p.x = __hiloint2double((int)v.y, (int)v.x);
  p.y = __hiloint2double((int)v.w, (int)v.z);
  return p;
}
__device__ __forceinline__ void sr_st_pair(sr_pair p, __amdgpu_buffer_rsrc_t r, unsigned int voff, unsigned int soff)
{
  sr_v4u v;
  v.x = (unsigned int)__double2loint(p.x), v.y = (unsigned int)__double2hiint(p.x);
  v.z = (unsigned int)__double2loint(p.y), v.w = (unsigned int)__double2hiint(p.y);
  __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, soff, 0);
}
__device__ __forceinline__ void sr_st_one(double d, __amdgpu_buffer_rsrc_t r, unsigned int voff, unsigned int soff)
{
  sr_v2u v;
  v.x = (unsigned int)__double2loint(d), v.y = (unsigned int)__double2hiint(d);
  __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, soff, 0);
}
// value the previous lane of the wavefront holds (DPP wave shift; lane 0 keeps its own)
__device__ __forceinline__ double sr_prev_lane(double v)
{
  const int hi = __double2hiint(v), lo = __double2loint(v);
  return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false),
                          __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false));
}

// y pairs of one layer of agglomerates around a lane: [0] its own column, [1] the column before; [.][sy]: rows vj - sy
struct SrLayer
{
  sr_pair c[2][2];
};

// (R^T y) at the node at offset (DX, DY, DZ) in its agglomerate position: `a0` are the pairs of the agglomerate column the
// position starts, `a1` those of the column before (which holds the node only for DX = 0); [0] the layer vk, [1] vk - 1.
// The terms in the order of sr_node_value / the block kernel.
template <int DX, int DY, int DZ, typename Table>
__device__ __forceinline__ double sr_march_sum(Table table, sr_pair const (&a0)[2][2], sr_pair const (&a1)[2][2])
{
  double sum = 0.;
#pragma unroll
  for (int sz = 0; sz < 2; ++sz)
#pragma unroll
    for (int sy = 0; sy < 2; ++sy)
#pragma unroll
      for (int sx = 0; sx < 2; ++sx)
      {
        if ((sx && DX) || (sy && DY) || (sz && DZ))
          continue;
        const int m = (sx ? 2 : DX) + 3 * ((sy ? 2 : DY) + 3 * (sz ? 2 : DZ));
        const sr_pair yv = sx ? a1[sz][sy] : a0[sz][sy];
        sum += table[2 * m] * yv.x;
        sum += table[2 * m + 1] * yv.y;
      }
  return sum;
}

template <bool SUB>
__global__ __launch_bounds__(64 * kMarchWaves) void sr_prolong_march222_kernel(SrArgs s, SrMarch g, double const *y, double *out,
                                                                               uint8_t const *blk_exc, int32_t const *blocks,
                                                                               int64_t n_blocks)
{
  // the marches first: few workgroups that live long; the listed positions fill the rest of the device beside them
  if (blockIdx.x >= g.blocks)
  {
    sr_prolong_listed222_part<SUB>(s, y, out, blocks, n_blocks, blockIdx.x - g.blocks);
    return;
  }
  typedef __attribute__((address_space(4))) const double ctable_t;
  ctable_t *table = reinterpret_cast<ctable_t *>(reinterpret_cast<uintptr_t>(s.table));
  // a contiguous run of workgroups per XCD: neighbouring rows and neighbouring chunks of layers share y pairs (workgroups are
  // dealt to the 8 XCDs of the MI300 / MI355X in turn, as the restriction kernels above assume; on a part with another count the
  // mapping is still one to one -- `blocks` is a multiple of 8 -- and only the sharing is lost)
  const unsigned int mb = blockIdx.x;
  const unsigned int bid = (mb & 7) * (g.blocks >> 3) + (mb >> 3);
  if (bid >= g.n_wgs)
    return;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int strip = (int)(bid % (unsigned int)g.strips), wy = (int)((bid / (unsigned int)g.strips) % (unsigned int)g.wgs_y),
            ch = (int)(bid / (unsigned int)(g.strips * g.wgs_y));
  const int vj = g.lo[1] + wy * kMarchWaves + w;
  const int vk0 = g.lo[2] + ch * g.len, vk1 = min(vk0 + g.len, g.hi[2] + 1);
  if (vj > g.hi[1] || vk0 >= vk1)
    return; // (waves share nothing: no barrier is left waiting)
  const int na0 = s.na[0], na1 = s.na[1], na2 = s.na[2], N0 = s.N[0], N1 = s.N[1], N2 = s.N[2];
  const int vi0 = g.lo[0] + 64 * strip, vi = vi0 + lane;
  const int vic = min(vi, na0); // (lanes beyond the row: clamped requests, no stores)
  const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(y), 0, g.y_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(out, 0, g.out_bytes, 0x00020000);
  // y: per-lane offset of the own agglomerate column, wave-uniform one of the column before lane 0; agglomerates outside
  // the mesh are requested at a clamped index and contribute exact zeros, as in the block kernel
  const unsigned int yo_own = 16u * (unsigned int)min(vic, na0 - 1);
  unsigned int yo_halo = 16u * (unsigned int)min(max(vi0 - 1, 0), na0 - 1);
  // (kept in a vector register of its own: moved there from a scalar before every request it took the place of a register that
  // an earlier request had yet to fill, with a wait for ALL outstanding requests in front of the move)
  asm volatile("" : "+v"(yo_halo));
  const bool has_own = vi < na0, has_halo = vi0 >= 1;
  const unsigned int y_row[2] = {(unsigned int)min(vj, na1 - 1), (unsigned int)max(vj - 1, 0)};
  const bool has_row[2] = {vj < na1, vj >= 1};
  // out: first node of the lane's pair in the rows at an even / odd distance from the start of the vector, and the same
  // clamped into the row for the request
  const int n_first[2] = {2 * vic, 2 * vic - 1};
  unsigned int oo_ld[2], oo_st[2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
  {
    oo_ld[p] = 8u * (unsigned int)min(max(n_first[p], 0), N0 - 2);
    oo_st[p] = 8u * (unsigned int)max(n_first[p], 0);
  }
  const bool at_head = vic == 0, at_tail = vic == na0; // pair (-1, 0) of an odd row, pair (N0 - 1, N0) of an even one
  const int vx = na0 + 1, vy = na1 + 1;

  struct Raw
  {
    sr_pair own[2], halo[2]; // y pairs of a layer as requested: rows vj, vj - 1
    sr_pair o[4];            // out: node rows (dy, dz) of the layer
    unsigned int exc[2];     // blk_exc of the positions vi, vi - 1
  };
  auto request_y = [&](Raw &r, int vk) {
    const unsigned int kc = (unsigned int)min(max(vk, 0), na2 - 1);
#pragma unroll
    for (int sy = 0; sy < 2; ++sy)
    {
      const unsigned int soff = 16u * (unsigned int)na0 * (y_row[sy] + (unsigned int)na1 * kc);
      r.own[sy] = sr_ld_pair(rs_y, yo_own, soff);
      r.halo[sy] = sr_ld_pair(rs_y, yo_halo, soff);
    }
  };
  auto request_out = [&](Raw &r, int vk) {
    const int64_t pos = (int64_t)vx * (vj + (int64_t)vy * vk);
    r.exc[0] = blk_exc[pos + vic];
    r.exc[1] = blk_exc[pos + max(vic - 1, 0)];
    if constexpr (SUB)
    {
#pragma unroll
      for (int dyz = 0; dyz < 4; ++dyz)
      {
        const int dy = dyz & 1, dz = dyz >> 1;
        const unsigned int row = (unsigned int)min(2 * vj + dy, N1 - 1) + (unsigned int)N1 * (unsigned int)min(2 * vk + dz, N2 - 1);
        r.o[dyz] = sr_ld_pair(rs_o, oo_ld[dy ^ dz], 8u * (unsigned int)N0 * row);
      }
    }
  };
  // the pairs of layer vk around the lane, from what was requested
  auto layer_of = [&](Raw const &r, int vk) {
    const bool has_k = vk >= 0 && vk < na2;
    SrLayer L;
#pragma unroll
    for (int sy = 0; sy < 2; ++sy)
    {
      const bool ho = has_own && has_row[sy] && has_k, hh = has_halo && has_row[sy] && has_k;
      const sr_pair own{ho ? r.own[sy].x : 0., ho ? r.own[sy].y : 0.};
      const sr_pair halo{hh ? r.halo[sy].x : 0., hh ? r.halo[sy].y : 0.};
      const double px = sr_prev_lane(own.x), py = sr_prev_lane(own.y);
      L.c[0][sy] = own;
      L.c[1][sy] = sr_pair{lane == 0 ? halo.x : px, lane == 0 ? halo.y : py};
    }
    return L;
  };
  // the four node rows of layer vk: sums, then out
  auto finish = [&](Raw const &r, SrLayer const &cur, SrLayer const &prev, int vk) {
    sr_pair a_own[2][2], a_prev[2][2]; // [layer vk - sz][row vj - sy]
#pragma unroll
    for (int sy = 0; sy < 2; ++sy)
    {
      a_own[0][sy] = cur.c[0][sy], a_own[1][sy] = prev.c[0][sy];
      a_prev[0][sy] = cur.c[1][sy], a_prev[1][sy] = prev.c[1][sy];
    }
    const bool live_p = vi <= na0 && r.exc[0] == 0, live_m = vi >= 1 && vi <= na0 && r.exc[1] == 0;
#pragma unroll
    for (int dyz = 0; dyz < 4; ++dyz)
    {
      const int dy = dyz & 1, dz = dyz >> 1;
      if (2 * vj + dy >= N1 || 2 * vk + dz >= N2)
        continue; // (wave-uniform)
      const int odd = dy ^ dz;
      double s0, s1;
      bool w0, w1;
      if (odd)
      {
        s0 = dyz == 1 ? sr_march_sum<1, 1, 0>(table, a_prev, a_prev) : sr_march_sum<1, 0, 1>(table, a_prev, a_prev);
        s1 = dyz == 1 ? sr_march_sum<0, 1, 0>(table, a_own, a_prev) : sr_march_sum<0, 0, 1>(table, a_own, a_prev);
        w0 = live_m, w1 = live_p;
      }
      else
      {
        s0 = dyz == 0 ? sr_march_sum<0, 0, 0>(table, a_own, a_prev) : sr_march_sum<0, 1, 1>(table, a_own, a_prev);
        s1 = dyz == 0 ? sr_march_sum<1, 0, 0>(table, a_own, a_own) : sr_march_sum<1, 1, 1>(table, a_own, a_own);
        w0 = live_p, w1 = live_p && vi < na0;
      }
      sr_pair v{s0, s1};
      if constexpr (SUB)
      {
        sr_pair o = r.o[dyz];
        if (odd && at_head)
          o.y = o.x; // requested (0, 1) for (-1, 0)
        if (!odd && at_tail)
          o.x = o.y; // requested (N0 - 2, N0 - 1) for (N0 - 1, N0)
        v.x = o.x - s0, v.y = o.y - s1;
      }
      const unsigned int soff = 8u * (unsigned int)N0 * ((unsigned int)(2 * vj + dy) + (unsigned int)N1 * (unsigned int)(2 * vk + dz));
      if (w0 && w1)
        sr_st_pair(v, rs_o, oo_st[odd], soff);
      else if (w0)
        sr_st_one(v.x, rs_o, oo_st[odd], soff);
      else if (w1)
        sr_st_one(v.y, rs_o, 8u * (unsigned int)(n_first[odd] + 1), soff);
    }
  };

  // one step: the requests of layer vk + 1 leave into `next` before `now` (requested a step ago) is first used; the two sets of
  // registers and the two layers of pairs change roles from step to step (no copies: a copy would wait for the data)
  // (the last step of a march asks for its own layer again: a request under a condition would make the compiler copy the
  // registers it fills where the two paths join, and a copy waits for the data)
  auto step = [&](Raw const &now, Raw &next, SrLayer const &below, SrLayer &here, int vk) {
    const int vn = min(vk + 1, vk1 - 1);
    request_y(next, vn);
    request_out(next, vn);
    here = layer_of(now, vk);
    finish(now, here, below, vk);
  };
  Raw ra, rb;
  SrLayer la, lb;
  request_y(rb, vk0 - 1);
  request_y(ra, vk0);
  request_out(ra, vk0);
  lb = layer_of(rb, vk0 - 1);
  for (int vk = vk0;; vk += 2)
  {
    step(ra, rb, lb, la, vk);
    if (vk + 1 >= vk1)
      break;
    step(rb, ra, la, lb, vk + 1);
    if (vk + 2 >= vk1)
      break;
  }
}
} // namespace

std::shared_ptr<StructuredRestrictorDevice>
StructuredRestrictorDevice::create(HipHandle &handle, StructuredMesh const &mesh, int const agglomerate[3],
                                   int const agg_dims[3], std::vector<int32_t> const &row_agglomerate,
                                   HostCsr const &R)
{
  MemoryKind kind("restrictor: planes, block tables, node lists");
  if (mesh.dim != 3 || R.n_rows == 0 || (int64_t)row_agglomerate.size() != R.n_rows)
    return nullptr;
  int64_t n_agg = 1, n_nodes = 1;
  for (int d = 0; d < 3; ++d)
  {
    if (agglomerate[d] < 1 || mesh.n[d] % agglomerate[d] != 0 || agg_dims[d] != mesh.n[d] / agglomerate[d])
      return nullptr; // clipped agglomerates have smaller patches
    n_agg *= agg_dims[d];
    n_nodes *= mesh.N[d];
  }
  if (R.n_rows % n_agg != 0 || R.n_cols != mesh.n_dofs || n_nodes != mesh.n_dofs)
    return nullptr;
  const int n_eig = (int)(R.n_rows / n_agg);
  for (int64_t r = 0; r < R.n_rows; ++r)
    if (row_agglomerate[r] != r / n_eig)
      return nullptr;
  const int px = agglomerate[0] + 1, py = agglomerate[1] + 1, pz = agglomerate[2] + 1;
  const int patch = px * py * pz;
  if ((int64_t)mesh.node_dof.size() != n_nodes)
    return nullptr;
  // node of every DoF
  std::vector<int32_t> dof_node(mesh.n_dofs, -1);
  bool identity = true;
  for (int64_t nd = 0; nd < n_nodes; ++nd)
  {
    const int32_t g = mesh.node_dof[nd];
    if (g < 0 || g >= mesh.n_dofs)
      return nullptr;
    dof_node[g] = (int32_t)nd;
    identity = identity && (g == nd);
  }
  std::vector<double> planes((size_t)patch * R.n_rows, 0.);
  bool ok = true;
#pragma omp parallel for schedule(static) reduction(&& : ok)
  for (int64_t r = 0; r < R.n_rows; ++r)
  {
    const int64_t ag = r / n_eig;
    const int ai = (int)(ag % agg_dims[0]), aj = (int)((ag / agg_dims[0]) % agg_dims[1]),
              ak = (int)(ag / ((int64_t)agg_dims[0] * agg_dims[1]));
    for (int p = R.row_ptr[r]; p < R.row_ptr[r + 1]; ++p)
    {
      const int32_t nd = dof_node[R.col[p]];
      if (nd < 0)
      {
        ok = false;
        continue;
      }
      const int i = nd % mesh.N[0], j = (nd / mesh.N[0]) % mesh.N[1], k = nd / (mesh.N[0] * mesh.N[1]);
      const int mx = i - ai * agglomerate[0], my = j - aj * agglomerate[1], mz = k - ak * agglomerate[2];
      if (mx < 0 || mx >= px || my < 0 || my >= py || mz < 0 || mz >= pz)
      {
        ok = false;
        continue;
      }
      planes[(size_t)(mx + px * (my + py * mz)) * R.n_rows + r] += R.val[p];
    }
  }
  if (!ok)
    return nullptr;
  std::shared_ptr<StructuredRestrictorDevice> s(new StructuredRestrictorDevice(handle));
  for (int d = 0; d < 3; ++d)
  {
    s->_N[d] = mesh.N[d];
    s->_na[d] = agg_dims[d];
    s->_a[d] = agglomerate[d];
  }
  s->_n_eig = n_eig;
  s->_patch = patch;
  s->_n_coarse = R.n_rows;
  s->_n_fine = mesh.n_dofs;
  s->_nnz = R.row_ptr[R.n_rows];
  s->_identity_numbering = identity;
  // MFMG_SR_RESTRICT=rows: R x by the row kernel; MFMG_SR_PROLONG=nodes: R^T y by the node kernel (no block kernel).  Each gives
  // the same bits as the kernel it replaces (tests/test_transfer_shapes.py); read per restrictor, not cached
  auto env_is = [](char const *name, char const *value) {
    char const *e = std::getenv(name);
    return e != nullptr && std::string(e) == value;
  };
  s->_restrict_rows = env_is("MFMG_SR_RESTRICT", "rows");
  const bool prolong_nodes = env_is("MFMG_SR_PROLONG", "nodes");
  // MFMG_SR_PROLONG=block: the block kernel with a thread per agglomerate position instead of its marching form (the same bits,
  // tests/test_transfer_march_kernels.py; for that comparison and for timing one against the other); MFMG_SR_MARCH_LAYERS: the
  // layers of a march (default: chosen for the grid).  The march addresses both vectors through 32-bit byte offsets
  s->_prolong_march = !env_is("MFMG_SR_PROLONG", "block") && 8 * (int64_t)mesh.n_dofs < (int64_t(1) << 32) && 8 * R.n_rows < (int64_t(1) << 32);
  if (char const *e = std::getenv("MFMG_SR_MARCH_LAYERS"))
    s->_march_layers = std::max(0, std::atoi(e));
  {
    // planes whose values a float holds exactly ("setup value precision" float rounds R) are kept in float
    bool all_float = !planes.empty();
    // (a sample first: FP64 values fail at once, and the full pass over 0.9 GB is spent only on candidates)
    for (int64_t q = 0; q < (int64_t)planes.size() && all_float; q += std::max<int64_t>(1, (int64_t)planes.size() / 4099))
      all_float = (double)(float)planes[q] == planes[q];
    if (all_float)
    {
#pragma omp parallel for schedule(static) reduction(&& : all_float)
      for (int64_t q = 0; q < (int64_t)planes.size(); ++q)
        all_float = all_float && (double)(float)planes[q] == planes[q];
    }
    if (all_float && n_eig % 2 == 0)
    {
      std::vector<float> pf(planes.size());
#pragma omp parallel for schedule(static)
      for (int64_t q = 0; q < (int64_t)planes.size(); ++q)
        pf[q] = (float)planes[q];
      s->_planes_f32.upload(pf.data(), pf.size(), handle.stream);
    }
    else
      s->_planes.upload(planes.data(), planes.size(), handle.stream);
  }
  if (n_eig == 2 && identity && agglomerate[0] == 2 && agglomerate[1] == 2 && agglomerate[2] == 2)
  {
    // class of EVERY agglomerate by the bits of its block (for the residual restriction, residual_restriction.hip);
    // given up beyond 4096 classes (a coefficient that varies from cell to cell: no two blocks alike)
    std::vector<uint64_t> hash(n_agg);
#pragma omp parallel for schedule(static)
    for (int64_t ag = 0; ag < n_agg; ++ag)
    {
      uint64_t h = 1469598103934665603ull;
      for (int m = 0; m < patch; ++m)
        for (int e = 0; e < n_eig; ++e)
        {
          uint64_t bits;
          std::memcpy(&bits, &planes[(size_t)m * R.n_rows + ag * n_eig + e], 8);
          h = (h ^ bits) * 1099511628211ull;
          h ^= h >> 29;
        }
      hash[ag] = h;
    }
    auto same_block = [&](int64_t a1, int64_t a2) {
      for (int m = 0; m < patch; ++m)
        for (int e = 0; e < n_eig; ++e)
          if (planes[(size_t)m * R.n_rows + a1 * n_eig + e] != planes[(size_t)m * R.n_rows + a2 * n_eig + e])
            return false;
      return true;
    };
    std::vector<int64_t> first;
    std::vector<uint16_t> all(n_agg);
    bool fits = true;
    // Classes numbered in the order of their first agglomerate.  In parallel: the first agglomerate of every hash value (per
    // thread over its contiguous share, merged), classes in the order of those, then every agglomerate compared with the
    // representative of its hash; a hash shared by two different blocks sends the whole step to the serial loop below,
    // which compares block by block -- the same classes either way.
    bool parallel_done = false;
    {
      const int nt = std::max(1, omp_get_max_threads());
      std::vector<std::unordered_map<uint64_t, int64_t>> local(nt);
      bool too_many = false;
#pragma omp parallel num_threads(nt)
      {
        const int t = omp_get_thread_num();
        const int64_t lo = n_agg * t / nt, hi = n_agg * (t + 1) / nt;
        auto &m = local[t];
        for (int64_t ag = lo; ag < hi; ++ag)
        {
          m.emplace(hash[ag], ag); // (keeps the first)
          if (m.size() > 4096)
          {
#pragma omp atomic write
            too_many = true;
            break;
          }
        }
      }
      if (too_many)
        fits = false, parallel_done = true; // (more than 4096 different blocks: the serial loop would give up as well)
      else
      {
        std::unordered_map<uint64_t, int64_t> firsts;
        for (auto const &m : local)
          for (auto const &kv : m)
          {
            auto it = firsts.find(kv.first);
            if (it == firsts.end())
              firsts.emplace(kv.first, kv.second);
            else if (kv.second < it->second)
              it->second = kv.second;
          }
        if (firsts.size() > 4096)
          fits = false, parallel_done = true;
        else
        {
          std::vector<std::pair<int64_t, uint64_t>> order;
          for (auto const &kv : firsts)
            order.emplace_back(kv.second, kv.first);
          std::sort(order.begin(), order.end());
          std::unordered_map<uint64_t, int> class_of_hash;
          for (size_t c = 0; c < order.size(); ++c)
          {
            class_of_hash.emplace(order[c].second, (int)c);
            first.push_back(order[c].first);
          }
          bool exact = true;
#pragma omp parallel for schedule(static) reduction(&& : exact)
          for (int64_t ag = 0; ag < n_agg; ++ag)
          {
            const int c = class_of_hash.find(hash[ag])->second;
            all[ag] = (uint16_t)c;
            exact = exact && same_block(first[c], ag);
          }
          parallel_done = exact;
          if (!exact)
            first.clear();
        }
      }
    }
    if (!parallel_done)
    {
    std::unordered_map<uint64_t, std::vector<int>> by_hash; // hash -> classes with that hash
    for (int64_t ag = 0; ag < n_agg && fits; ++ag)
    {
      auto &cands = by_hash[hash[ag]];
      int found = -1;
      for (int c : cands)
        if (same_block(first[c], ag))
        {
          found = c;
          break;
        }
      if (found < 0)
      {
        if (first.size() >= 4096)
        {
          fits = false;
          break;
        }
        found = (int)first.size();
        first.push_back(ag);
        cands.push_back(found);
      }
      all[ag] = (uint16_t)found;
    }
    }
    if (fits)
      s->_cls_host = std::move(all);
  }
  if (n_eig == 2)
  {
    // reference agglomerate: of a few candidates the one a sample of agglomerates repeats most
    auto same = [&](int64_t a1, int64_t a2) {
      for (int m = 0; m < patch; ++m)
        for (int e = 0; e < n_eig; ++e)
          if (planes[(size_t)m * R.n_rows + a1 * n_eig + e] != planes[(size_t)m * R.n_rows + a2 * n_eig + e])
            return false;
      return true;
    };
    int64_t ref = n_agg / 2, best = -1;
    const double frac[] = {0.5, 0.377, 0.613, 0.431, 0.569, 0.289, 0.711, 0.457};
    for (double f : frac)
    {
      const int64_t cand = std::min<int64_t>(n_agg - 1, (int64_t)(f * n_agg) + 12345 % std::max<int64_t>(n_agg / 7, 1));
      int64_t hits = 0;
      for (int64_t t = 0; t < 2048; ++t)
        hits += same((t * 2654435761ll) % n_agg, cand) ? 1 : 0;
      if (hits > best)
      {
        best = hits;
        ref = cand;
      }
    }
    std::vector<uint8_t> exc(n_agg);
    int64_t n_regular = 0;
#pragma omp parallel for schedule(static) reduction(+ : n_regular)
    for (int64_t ag = 0; ag < n_agg; ++ag)
    {
      exc[ag] = same(ag, ref) ? 0 : 1;
      n_regular += exc[ag] ? 0 : 1;
    }
    if (n_regular * 2 >= n_agg)
    {
      s->_n_regular = n_regular;
      // classes among the others (hash of the block, exact comparison with the first agglomerate of the class)
      {
        std::vector<int64_t> others;
        for (int64_t ag = 0; ag < n_agg; ++ag)
          if (exc[ag])
            others.push_back(ag);
        std::vector<uint64_t> hash(others.size());
#pragma omp parallel for schedule(static)
        for (int64_t q = 0; q < (int64_t)others.size(); ++q)
        {
          uint64_t h = 1469598103934665603ull;
          for (int m = 0; m < patch; ++m)
            for (int e = 0; e < n_eig; ++e)
            {
              uint64_t bits;
              std::memcpy(&bits, &planes[(size_t)m * R.n_rows + others[q] * n_eig + e], 8);
              h = (h ^ bits) * 1099511628211ull;
              h ^= h >> 29;
            }
          hash[q] = h;
        }
        std::vector<int64_t> order(others.size());
        std::iota(order.begin(), order.end(), (int64_t)0);
        std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return hash[x] != hash[y] ? hash[x] < hash[y] : x < y; });
        std::vector<uint16_t> cls(n_agg, kNoClass);
        std::vector<double> class_table;
        auto push_block = [&](int64_t ag) {
          for (int m = 0; m < patch; ++m)
            for (int e = 0; e < n_eig; ++e)
              class_table.push_back(planes[(size_t)m * R.n_rows + ag * n_eig + e]);
        };
        push_block(ref); // class 0: the reference block
        for (int64_t ag = 0; ag < n_agg; ++ag)
          if (!exc[ag])
            cls[ag] = 0;
        int n_classes = 1;
        for (size_t g0 = 0; g0 < order.size() && n_classes < 0xfff0;)
        {
          size_t g1 = g0;
          while (g1 < order.size() && hash[order[g1]] == hash[order[g0]])
            ++g1;
          if (g1 - g0 >= 4)
          {
            const int64_t rep = others[order[g0]];
            int64_t members = 0;
            for (size_t q = g0; q < g1; ++q)
              if (same(others[order[q]], rep))
              {
                cls[others[order[q]]] = (uint16_t)n_classes;
                ++members;
              }
            if (members > 0)
            {
              push_block(rep);
              ++n_classes;
            }
          }
          g0 = g1;
        }
        if (n_classes > 1)
        {
          s->_cls.upload(cls.data(), cls.size(), handle.stream);
          s->_class_table.upload(class_table.data(), class_table.size(), handle.stream);
          s->_n_classes = n_classes - 1;
        }
      }
      std::vector<double> table((size_t)patch * n_eig);
      for (int m = 0; m < patch; ++m)
        for (int e = 0; e < n_eig; ++e)
          table[(size_t)m * n_eig + e] = planes[(size_t)m * R.n_rows + ref * n_eig + e];
      // per fine node: is one of the (at most eight) agglomerates it lies in not regular?
      std::vector<uint8_t> exc_node(n_nodes, 0);
#pragma omp parallel for schedule(static)
      for (int64_t nd = 0; nd < n_nodes; ++nd)
      {
        const int ijk[3] = {(int)(nd % mesh.N[0]), (int)((nd / mesh.N[0]) % mesh.N[1]),
                            (int)(nd / ((int64_t)mesh.N[0] * mesh.N[1]))};
        int lo[3], hi[3];
        for (int d = 0; d < 3; ++d)
        {
          const int q = ijk[d] / agglomerate[d];
          hi[d] = std::min(q, agg_dims[d] - 1);
          lo[d] = (ijk[d] % agglomerate[d] == 0 && q >= 1) ? q - 1 : std::min(q, agg_dims[d] - 1);
        }
        uint8_t any = 0;
        for (int c2 = lo[2]; c2 <= hi[2]; ++c2)
          for (int c1 = lo[1]; c1 <= hi[1]; ++c1)
            for (int c0 = lo[0]; c0 <= hi[0]; ++c0)
              any |= exc[c0 + (int64_t)agg_dims[0] * (c1 + (int64_t)agg_dims[1] * c2)];
        exc_node[nd] = any;
      }
      if (identity && agglomerate[0] == 2 && agglomerate[1] == 2 && agglomerate[2] == 2 && !prolong_nodes)
      {
        // agglomerate positions all of whose (existing) agglomerates around are regular -> block kernel
        const int64_t vx = agg_dims[0] + 1, vy = agg_dims[1] + 1, vz = agg_dims[2] + 1;
        std::vector<uint8_t> blk_exc((size_t)(vx * vy * vz), 0);
#pragma omp parallel for schedule(static)
        for (int64_t t = 0; t < vx * vy * vz; ++t)
        {
          const int vi = (int)(t % vx), vj = (int)((t / vx) % vy), vk = (int)(t / (vx * vy));
          uint8_t any = 0;
          for (int sidx = 0; sidx < 8; ++sidx)
          {
            const int qi = vi - (sidx & 1), qj = vj - ((sidx >> 1) & 1), qk = vk - (sidx >> 2);
            if (qi >= 0 && qi < agg_dims[0] && qj >= 0 && qj < agg_dims[1] && qk >= 0 && qk < agg_dims[2])
              any |= exc[qi + (int64_t)agg_dims[0] * (qj + (int64_t)agg_dims[1] * qk)];
          }
          blk_exc[t] = any;
        }
        std::vector<int32_t> exc_blocks;
        int lo[3] = {1 << 30, 1 << 30, 1 << 30}, hi[3] = {-1, -1, -1};
        for (int64_t t = 0; t < vx * vy * vz; ++t)
          if (blk_exc[t])
            exc_blocks.push_back((int32_t)t);
          else
          {
            const int v[3] = {(int)(t % vx), (int)((t / vx) % vy), (int)(t / (vx * vy))};
            for (int d = 0; d < 3; ++d)
            {
              lo[d] = std::min(lo[d], v[d]);
              hi[d] = std::max(hi[d], v[d]);
            }
          }
        for (int d = 0; d < 3; ++d)
        {
          s->_march_lo[d] = lo[d];
          s->_march_hi[d] = hi[d];
        }
        if (hi[0] >= lo[0])
        {
          // grid of the marches.  The lane after the last position of a row takes that position's last node in the odd rows.
          s->_march_strips = (std::min(hi[0] + 1, agg_dims[0]) - lo[0] + 1 + 63) / 64;
          s->_march_wgs_y = (hi[1] - lo[1] + 1 + kMarchWaves - 1) / kMarchWaves;
          const int layers = hi[2] - lo[2] + 1;
          // Layers of a march: as many chunks as give every CU ONE workgroup of marches, in whole rounds -- one per CU streams as
          // fast as four (the marches are bound by bytes: profiles/r07_a), and the rest of the CU is for the listed positions,
          // which are bound by latency and run beside them.  A march passes its layers plus the fill of its pipeline; one
          // shorter than kMarchMin layers re-reads too many y pairs at its start.
          int n_cus = 0, dev = 0;
          if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cus <= 0)
            n_cus = 256;
          constexpr int kMarchMin = 8;
          int len = s->_march_layers > 0 ? std::min(s->_march_layers, layers) : 0;
          if (len == 0)
          {
            double best = 0.;
            for (int nk = 1; nk <= layers; ++nk)
            {
              const int t = (layers + nk - 1) / nk;
              if ((layers + t - 1) / t != nk || (nk > 1 && t < kMarchMin))
                continue;
              const int64_t wgs = (int64_t)s->_march_strips * s->_march_wgs_y * nk;
              const double cost = double((wgs + n_cus - 1) / n_cus) * (t + 2.);
              if (len == 0 || cost < best)
              {
                best = cost;
                len = t;
              }
            }
          }
          s->_march_len = len;
          s->_march_chunks = (layers + len - 1) / len;
        }
        s->_blk_exc.upload(blk_exc.data(), blk_exc.size(), handle.stream);
        s->_exc_blocks.upload(exc_blocks.data(), exc_blocks.size(), handle.stream);
      }
      s->_exc.upload(exc.data(), exc.size(), handle.stream);
      s->_exc_node.upload(exc_node.data(), exc_node.size(), handle.stream);
      s->_table.upload(table.data(), table.size(), handle.stream);
    }
  }
  if (!identity)
    s->_node_dof.upload(mesh.node_dof.data(), mesh.node_dof.size(), handle.stream);
  MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream));
  return s;
}

double StructuredRestrictorDevice::algorithmic_bytes() const
{
  return double(_nnz) * 12. + 4. * double(_n_coarse + 1) + 8. * double(_n_fine) + 8. * double(_n_coarse);
}

namespace
{
SrArgs make_args(double const *planes, float const *planes_f, int32_t const *node_dof, int64_t n_coarse, int const N[3], int const na[3],
                 int const a[3], int n_eig, int patch, uint8_t const *exc, uint8_t const *exc_node, double const *table,
                 uint16_t const *cls, double const *class_table)
{
  SrArgs s;
  s.planes = planes;
  s.planes_f = planes_f;
  s.node_dof = node_dof;
  s.n_coarse = n_coarse;
  for (int d = 0; d < 3; ++d)
  {
    s.N[d] = N[d];
    s.na[d] = na[d];
    s.a[d] = a[d];
  }
  s.n_eig = n_eig;
  s.patch = patch;
  s.exc = exc;
  s.exc_node = exc_node;
  s.table = table;
  s.cls = cls;
  s.class_table = class_table;
  return s;
}
} // namespace

int StructuredRestrictorDevice::restrict_kernel() const
{
  if (_n_eig != 2 || _restrict_rows)
    return kRestrictRows;
  return (_a[0] == 2 && _a[1] == 2 && _a[2] == 2) ? kRestrictPair2 : kRestrictPairAny;
}

void StructuredRestrictorDevice::restrict_to_coarse(double const *x, double *y) const
{
  ASSERT_THROW(x != nullptr && y != nullptr && x != y, "bad vectors");
  SrArgs s = make_args(_planes.data(), _planes_f32.size() ? _planes_f32.data() : nullptr, _identity_numbering ? nullptr : _node_dof.data(), _n_coarse, _N, _na, _a,
                       _n_eig, _patch, _exc.size() ? _exc.data() : nullptr, _exc_node.size() ? _exc_node.data() : nullptr, _table.data(),
                       _cls.size() ? _cls.data() : nullptr, _class_table.data());
  hipEvent_t stop = _handle.profiler.begin("csr_spmv_kernel", algorithmic_bytes(), _handle.stream);
  const int kernel = restrict_kernel();
  if (kernel != kRestrictRows)
  {
    const dim3 grid((unsigned int)(((_n_coarse / 2 + 255) / 256 + 7) / 8 * 8));
    if (kernel == kRestrictPair2)
      hipLaunchKernelGGL(sr_restrict_pair_kernel<2>, grid, dim3(256), 0, _handle.stream, s, x, y);
    else
      hipLaunchKernelGGL(sr_restrict_pair_kernel<0>, grid, dim3(256), 0, _handle.stream, s, x, y);
  }
  else
    hipLaunchKernelGGL(sr_restrict_kernel, dim3((unsigned int)((_n_coarse + 255) / 256)), dim3(256), 0,
                       _handle.stream, s, x, y);
  KernelProfiler::end(stop, _handle.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}

namespace
{
void check_block_operands(int k, int64_t ld_in, int64_t n_in, void const *in, int64_t ld_out, int64_t n_out, void const *out)
{
  ASSERT_THROW(k >= 1 && k <= kMfBlockMaxVectors, "a block holds 1 to 64 vectors");
  ASSERT_THROW(in != nullptr && out != nullptr && in != out, "bad vectors");
  ASSERT_THROW(ld_in >= n_in && ld_out >= n_out, "the leading dimension of a block must be at least the vector size");
  ASSERT_THROW(ld_in % 2 == 0 && ld_out % 2 == 0, "the leading dimension of a block must be even (columns aligned to 16 bytes)");
  ASSERT_THROW(reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0,
               "the base of a block must be aligned to 16 bytes");
}
} // namespace

int StructuredRestrictorDevice::restrict_to_coarse_block(int k, int64_t ldx, double const *x, int64_t ldy, double *y) const
{
  check_block_operands(k, ldx, _n_fine, x, ldy, _n_coarse, y);
  SrArgs s = make_args(_planes.data(), _planes_f32.size() ? _planes_f32.data() : nullptr, _identity_numbering ? nullptr : _node_dof.data(), _n_coarse, _N, _na, _a,
                       _n_eig, _patch, _exc.size() ? _exc.data() : nullptr, _exc_node.size() ? _exc_node.data() : nullptr, _table.data(),
                       _cls.size() ? _cls.data() : nullptr, _class_table.data());
  const int kernel = restrict_kernel();
  int widths[kMfBlockMaxGroups];
  const int n_groups = mf_block_groups(k, widths);
  int looped = 0;
  int64_t c0 = 0;
  for (int g = 0; g < n_groups; c0 += widths[g], ++g)
  {
    const int w = widths[g];
    double const *gx = x + c0 * ldx;
    double *gy = y + c0 * ldy;
    if (w == 1)
    {
      restrict_to_coarse(gx, gy);
      ++looped;
      continue;
    }
    ASSERT_THROW(w == 2 || w == 4, "internal: a group of a block is 4, 2 or 1 columns wide");
    hipEvent_t stop = _handle.profiler.begin("sr_restrict_block_kernel", algorithmic_bytes() + 8. * (w - 1) * double(_n_fine + _n_coarse),
                                             _handle.stream);
    if (kernel != kRestrictRows)
    {
      const dim3 grid((unsigned int)(((_n_coarse / 2 + 255) / 256 + 7) / 8 * 8));
      if (kernel == kRestrictPair2 && w == 4)
        hipLaunchKernelGGL((sr_restrict_pair_block_kernel<2, 4>), grid, dim3(256), 0, _handle.stream, s, gx, ldx, gy, ldy);
      else if (kernel == kRestrictPair2)
        hipLaunchKernelGGL((sr_restrict_pair_block_kernel<2, 2>), grid, dim3(256), 0, _handle.stream, s, gx, ldx, gy, ldy);
      else if (w == 4)
        hipLaunchKernelGGL((sr_restrict_pair_block_kernel<0, 4>), grid, dim3(256), 0, _handle.stream, s, gx, ldx, gy, ldy);
      else
        hipLaunchKernelGGL((sr_restrict_pair_block_kernel<0, 2>), grid, dim3(256), 0, _handle.stream, s, gx, ldx, gy, ldy);
    }
    else
    {
      const dim3 grid((unsigned int)((_n_coarse + 255) / 256));
      if (w == 4)
        hipLaunchKernelGGL(sr_restrict_rows_block_kernel<4>, grid, dim3(256), 0, _handle.stream, s, gx, ldx, gy, ldy);
      else
        hipLaunchKernelGGL(sr_restrict_rows_block_kernel<2>, grid, dim3(256), 0, _handle.stream, s, gx, ldx, gy, ldy);
    }
    KernelProfiler::end(stop, _handle.stream);
    MFMG_HIP_CHECK(hipGetLastError());
    ++_restrict_block_launches;
  }
  return looped;
}

int StructuredRestrictorDevice::prolongate_block(int k, int64_t ldy, double const *y, int64_t ldo, double *out, bool subtract) const
{
  check_block_operands(k, ldy, _n_coarse, y, ldo, _n_fine, out);
  SrArgs s = make_args(_planes.data(), _planes_f32.size() ? _planes_f32.data() : nullptr, _identity_numbering ? nullptr : _node_dof.data(), _n_coarse, _N, _na, _a,
                       _n_eig, _patch, _exc.size() ? _exc.data() : nullptr, _exc_node.size() ? _exc_node.data() : nullptr, _table.data(),
                       _cls.size() ? _cls.data() : nullptr, _class_table.data());
  const bool block = prolong_block_width() > 1;
  int widths[kMfBlockMaxGroups];
  const int n_groups = mf_block_groups(k, widths);
  int looped = 0;
  int64_t c0 = 0;
  for (int g = 0; g < n_groups; c0 += widths[g], ++g)
  {
    const int w = widths[g];
    double const *gy = y + c0 * ldy;
    double *go = out + c0 * ldo;
    if (w == 1 || !block)
    {
      for (int c = 0; c < w; ++c)
        prolongate(gy + c * ldy, go + c * ldo, subtract);
      looped += w;
      continue;
    }
    ASSERT_THROW(w == 2 || w == 4, "internal: a group of a block is 4, 2 or 1 columns wide");
    hipEvent_t stop = _handle.profiler.begin("sr_prolong_block_kernel",
                                             algorithmic_bytes() + 8. * (w - 1) * double(_n_fine + _n_coarse) + (subtract ? 8. * w * double(_n_fine) : 0.),
                                             _handle.stream);
    const dim3 grid((unsigned int)((_n_fine + 255) / 256));
    if (subtract && w == 4)
      hipLaunchKernelGGL((sr_prolong_block_kernel<true, 4>), grid, dim3(256), 0, _handle.stream, s, gy, ldy, go, ldo);
    else if (subtract)
      hipLaunchKernelGGL((sr_prolong_block_kernel<true, 2>), grid, dim3(256), 0, _handle.stream, s, gy, ldy, go, ldo);
    else if (w == 4)
      hipLaunchKernelGGL((sr_prolong_block_kernel<false, 4>), grid, dim3(256), 0, _handle.stream, s, gy, ldy, go, ldo);
    else
      hipLaunchKernelGGL((sr_prolong_block_kernel<false, 2>), grid, dim3(256), 0, _handle.stream, s, gy, ldy, go, ldo);
    KernelProfiler::end(stop, _handle.stream);
    MFMG_HIP_CHECK(hipGetLastError());
    ++_prolong_block_launches;
  }
  return looped;
}

void StructuredRestrictorDevice::prolongate(double const *y, double *out, bool subtract) const
{
  ASSERT_THROW(y != nullptr && out != nullptr && y != out, "bad vectors");
  SrArgs s = make_args(_planes.data(), _planes_f32.size() ? _planes_f32.data() : nullptr, _identity_numbering ? nullptr : _node_dof.data(), _n_coarse, _N, _na, _a,
                       _n_eig, _patch, _exc.size() ? _exc.data() : nullptr, _exc_node.size() ? _exc_node.data() : nullptr, _table.data(),
                       _cls.size() ? _cls.data() : nullptr, _class_table.data());
  hipEvent_t stop = _handle.profiler.begin("csr_spmv_kernel", algorithmic_bytes() + (subtract ? 8. * double(_n_fine) : 0.),
                                           _handle.stream);
  if (prolong_march())
  {
    const int64_t n_listed = (int64_t)_exc_blocks.size();
    unsigned int listed_blocks = (unsigned int)((8 * n_listed + 255) / 256);
    SrMarch g;
    std::memset(&g, 0, sizeof(g));
    for (int d = 0; d < 3; ++d)
    {
      g.lo[d] = _march_lo[d];
      g.hi[d] = _march_hi[d];
    }
    g.strips = _march_strips, g.wgs_y = _march_wgs_y, g.chunks = _march_chunks, g.len = _march_len;
    g.n_wgs = (unsigned int)(g.strips * g.wgs_y * g.chunks);
    g.blocks = (g.n_wgs + 7) / 8 * 8;
    g.y_bytes = (unsigned int)(8 * _n_coarse);
    g.out_bytes = (unsigned int)(8 * _n_fine);
#ifdef MFMG_SR_TIMING_PARTS
    // a measurement build only (-DMFMG_SR_TIMING_PARTS=1 or 2 in CXXFLAGS; wrong results): the launch without its list / without
    // its marches, for the split timings of profiles/r07_a and r07_b
    if (MFMG_SR_TIMING_PARTS == 1)
      listed_blocks = 0;
    else
      g.blocks = 0, g.n_wgs = 0;
#endif
    const dim3 grid(listed_blocks + g.blocks);
    if (grid.x == 0)
      ; // (nothing to launch: only a measurement build gets here, every position is table-driven or in the list)
    else if (subtract)
      hipLaunchKernelGGL(sr_prolong_march222_kernel<true>, grid, dim3(64 * kMarchWaves), 0, _handle.stream, s, g, y, out, _blk_exc.data(),
                         _exc_blocks.data(), n_listed);
    else
      hipLaunchKernelGGL(sr_prolong_march222_kernel<false>, grid, dim3(64 * kMarchWaves), 0, _handle.stream, s, g, y, out, _blk_exc.data(),
                         _exc_blocks.data(), n_listed);
  }
  else if (_blk_exc.size() > 0)
  {
    const int64_t n_pos = (int64_t)_blk_exc.size(), n_listed = (int64_t)_exc_blocks.size();
    const unsigned int listed_blocks = (unsigned int)((8 * n_listed + 255) / 256);
    const dim3 grid(listed_blocks + (unsigned int)((n_pos + 255) / 256));
    if (subtract)
      hipLaunchKernelGGL(sr_prolong_block222_kernel<true>, grid, dim3(256), 0, _handle.stream, s, y, out, _blk_exc.data(), _exc_blocks.data(),
                         n_listed, listed_blocks);
    else
      hipLaunchKernelGGL(sr_prolong_block222_kernel<false>, grid, dim3(256), 0, _handle.stream, s, y, out, _blk_exc.data(), _exc_blocks.data(),
                         n_listed, listed_blocks);
  }
  else
    hipLaunchKernelGGL(sr_prolong_kernel, dim3((unsigned int)((_n_fine + 255) / 256)), dim3(256), 0, _handle.stream,
                       s, y, out, subtract ? 1 : 0);
  KernelProfiler::end(stop, _handle.stream);
  MFMG_HIP_CHECK(hipGetLastError());
}
} // namespace mfmg
