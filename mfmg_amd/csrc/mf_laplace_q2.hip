// Matrix-free Q2 Laplace operator (mf_laplace_q2.hpp): the operator kernel with its four epilogues and the diagonal kernel.
//
// Layout of the operator kernel.  A workgroup of CX x CY lanes takes a tile of cells, one cell per lane, and marches in z.  Lane
// column 0 and lane row 0 are the halo cells of the tile's low x and y faces, recomputed: the workgroup owns the nodes
// [2 bx TX, 2 (bx + 1) TX) x [2 by TY, 2 (by + 1) TY) of the lattice (TX = CX - 1, TY = CY - 1; the last tile of an axis owns the
// last node plane of that axis too) and every node gets all of its up to eight cell contributions inside ONE workgroup: owner
// computes, no atomics, the same bits on every run.  In z the workgroup owns the node planes of tz cell layers and recomputes the
// cell layer below them.
//
// Per cell layer c: the node planes 2c, 2c + 1, 2c + 2 of x are staged in LDS (plane P in slot P % 3: two new planes per layer),
// with constrained entries as zeros; every lane evaluates its cell -- the three directions one after the other, each as three
// 1-D contractions of 27 values in registers, the scaling with coefficient * k_d, three transposed contractions with the tables
// that carry the quadrature weights -- and leaves its 27 values in LDS; then the owned nodes of the planes 2c and 2c + 1 sum
// their cell contributions in ONE fixed order (z, y, x ascending), whatever the tile shape, and run the epilogue of the mode.
// The top plane of a cell layer waits in a double buffer for the layer above it.
//
// The coefficients of a cell are read once per cell evaluation (27 values, or one in the cell-constant layout: a template flag).
#include "mf_laplace_q2.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace mfmg
{
namespace
{
struct Q2Tables
{
  double V[9], D[9];   // [q][a]: value / derivative of the Lagrange polynomial a on {0, 1/2, 1} at the Gauss point q
  double Vw[9], Dw[9]; // ... times the Gauss weight of q (the transposed contractions)
};

struct Q2Args
{
  double const *x, *b, *x_prev, *dinv;
  double *out;
  double const *coef;
  uint8_t const *con;
  int n[3], N[3];
  int tz;
  double alpha, beta;
  double k[3]; // h_x h_y h_z / h_d^2
  Q2Tables t;
};

// new[q] = sum_a M[q][a] v[a] along the lines of stride S of the 3 x 3 x 3 array t (AXIS 0: x, 1: y, 2: z)
template <int AXIS>
__device__ __forceinline__ void q2_contract(double (&t)[27], double const (&M)[9])
{
  constexpr int S = AXIS == 0 ? 1 : AXIS == 1 ? 3 : 9;
#pragma unroll
  for (int l = 0; l < 9; ++l)
  {
    // the nine lines of the axis
    const int o = AXIS == 0 ? 3 * l : AXIS == 1 ? (l % 3) + 9 * (l / 3) : l;
    const double v0 = t[o], v1 = t[o + S], v2 = t[o + 2 * S];
#pragma unroll
    for (int q = 0; q < 3; ++q)
      t[o + q * S] = __builtin_fma(M[3 * q + 2], v2, __builtin_fma(M[3 * q + 1], v1, M[3 * q] * v0));
  }
}
// new[a] = sum_q M[q][a] v[q]
template <int AXIS>
__device__ __forceinline__ void q2_contract_t(double (&t)[27], double const (&M)[9])
{
  constexpr int S = AXIS == 0 ? 1 : AXIS == 1 ? 3 : 9;
#pragma unroll
  for (int l = 0; l < 9; ++l)
  {
    const int o = AXIS == 0 ? 3 * l : AXIS == 1 ? (l % 3) + 9 * (l / 3) : l;
    const double v0 = t[o], v1 = t[o + S], v2 = t[o + 2 * S];
#pragma unroll
    for (int a = 0; a < 3; ++a)
      t[o + a * S] = __builtin_fma(M[6 + a], v2, __builtin_fma(M[3 + a], v1, M[a] * v0));
  }
}

// one direction of the cell operator: t = G_d^T diag(c k_d w) G_d u
template <int DIR, bool COMPACT>
__device__ __forceinline__ void q2_direction(double (&t)[27], double const (&c)[COMPACT ? 1 : 27], double kd, Q2Tables const &tab)
{
  q2_contract<0>(t, DIR == 0 ? tab.D : tab.V);
  q2_contract<1>(t, DIR == 1 ? tab.D : tab.V);
  q2_contract<2>(t, DIR == 2 ? tab.D : tab.V);
  if (COMPACT)
  {
    const double ck = c[0] * kd;
#pragma unroll
    for (int q = 0; q < 27; ++q)
      t[q] *= ck;
  }
  else
  {
#pragma unroll
    for (int q = 0; q < 27; ++q)
      t[q] *= c[q] * kd;
  }
  q2_contract_t<0>(t, DIR == 0 ? tab.Dw : tab.Vw);
  q2_contract_t<1>(t, DIR == 1 ? tab.Dw : tab.Vw);
  q2_contract_t<2>(t, DIR == 2 ? tab.Dw : tab.Vw);
}

template <int CX, int CY, int MODE, bool COMPACT>
__global__ __launch_bounds__(CX *CY) void mf_laplace_q2_kernel(Q2Args a)
{
  constexpr int NC = CX * CY, TX = CX - 1, TY = CY - 1, PX = 2 * CX + 1, PY = 2 * CY + 1, PLANE = PX * PY;
  __shared__ double xs[3][PLANE]; // node plane P of the tile in slot P % 3
  __shared__ double low[18][NC];  // the cell values of the node planes 2c and 2c + 1 of the layer in flight
  __shared__ double top[2][9][NC]; // ... of the node plane 2c + 2, layer c in buffer c & 1
  const int tid = threadIdx.x, lx = tid % CX, ly = tid / CX;
  const int nx = a.n[0], ny = a.n[1], nz = a.n[2], Nx = a.N[0], Ny = a.N[1];
  const int cx0 = (int)blockIdx.x * TX - 1, cy0 = (int)blockIdx.y * TY - 1; // the tile's first (halo) cell
  const int z0 = (int)blockIdx.z * a.tz, z1 = min(z0 + a.tz, nz);
  const int cx = cx0 + lx, cy = cy0 + ly;
  const bool cell_xy = cx >= 0 && cx < nx && cy >= 0 && cy < ny;
  // owned nodes [Ilo, Ihi) x [Jlo, Jhi)
  const int Ilo = 2 * (cx0 + 1), Ihi = (cx0 + 1 + TX >= nx) ? Nx : 2 * (cx0 + 1 + TX);
  const int Jlo = 2 * (cy0 + 1), Jhi = (cy0 + 1 + TY >= ny) ? Ny : 2 * (cy0 + 1 + TY);
  const int nI = Ihi - Ilo, nJ = Jhi - Jlo;
  const int I0 = 2 * cx0, J0 = 2 * cy0; // lattice node of the staged planes' entry (0, 0)
  const int cfirst = z0 > 0 ? z0 - 1 : 0;
  for (int c = cfirst; c < z1; ++c)
  {
    // ---- stage the node planes of x this layer adds
    {
      const int pfirst = c == cfirst ? 2 * c : 2 * c + 1, np = 2 * c + 3 - pfirst;
      for (int i = tid; i < np * PLANE; i += NC)
      {
        const int P = pfirst + i / PLANE, r = i % PLANE;
        const int I = I0 + r % PX, J = J0 + r / PX;
        double v = 0.;
        if (I >= 0 && I < Nx && J >= 0 && J < Ny)
        {
          const int id = I + Nx * (J + Ny * P);
          if (!a.con[id])
            v = a.x[id];
        }
        xs[P % 3][r] = v;
      }
    }
    __syncthreads();
    // ---- the cell of this lane
    if (cell_xy)
    {
      double cq[COMPACT ? 1 : 27];
      const size_t cell = (size_t)cx + (size_t)nx * ((size_t)cy + (size_t)ny * c);
      if (COMPACT)
        cq[0] = a.coef[cell];
      else
      {
#pragma unroll
        for (int q = 0; q < 27; ++q)
          cq[q] = a.coef[27 * cell + q];
      }
      double acc[27], t[27];
#pragma unroll
      for (int d = 0; d < 3; ++d)
      {
#pragma unroll
        for (int m = 0; m < 27; ++m)
          t[m] = xs[(2 * c + m / 9) % 3][(2 * ly + (m / 3) % 3) * PX + 2 * lx + m % 3];
        if (d == 0)
          q2_direction<0, COMPACT>(t, cq, a.k[0], a.t);
        else if (d == 1)
          q2_direction<1, COMPACT>(t, cq, a.k[1], a.t);
        else
          q2_direction<2, COMPACT>(t, cq, a.k[2], a.t);
#pragma unroll
        for (int m = 0; m < 27; ++m)
          acc[m] = d == 0 ? t[m] : acc[m] + t[m];
      }
#pragma unroll
      for (int m = 0; m < 18; ++m)
        low[m][tid] = acc[m];
#pragma unroll
      for (int m = 0; m < 9; ++m)
        top[c & 1][m][tid] = acc[18 + m];
    }
    __syncthreads();
    // ---- the owned nodes of the planes 2c, 2c + 1 (and of the last plane of the mesh after the last layer)
    if (c >= z0)
    {
      const int planes = c == nz - 1 ? 3 : 2;
      for (int i = tid; i < planes * nI * nJ; i += NC)
      {
        const int pp = i / (nI * nJ), r = i % (nI * nJ);
        const int I = Ilo + r % nI, J = Jlo + r / nI;
        const int id = I + Nx * (J + Ny * (2 * c + pp));
        const double xi = a.x[id];
        double ax = xi;
        if (!a.con[id])
        {
          double s = 0.;
          // contributors along each axis: (cell, local node index), low cell first
          const int nzc = (pp == 0 && c > 0) ? 2 : 1;
          const int nyc = (J & 1) ? 1 : 2, nxc = (I & 1) ? 1 : 2;
          for (int zc = 0; zc < nzc; ++zc)
          {
            // pp 0: the layer below (its top plane, kc = 2) then this layer (kc = 0); pp 1: kc = 1; pp 2: kc = 2
            const bool below = pp == 0 && nzc == 2 && zc == 0;
            const int kc = below ? 2 : pp;
            for (int yc = 0; yc < nyc; ++yc)
            {
              const int ccy = (J & 1) ? (J - 1) / 2 : J / 2 - 1 + yc, kb = (J & 1) ? 1 : 2 - 2 * yc;
              if (ccy < 0 || ccy >= ny)
                continue;
              for (int xc = 0; xc < nxc; ++xc)
              {
                const int ccx = (I & 1) ? (I - 1) / 2 : I / 2 - 1 + xc, ka = (I & 1) ? 1 : 2 - 2 * xc;
                if (ccx < 0 || ccx >= nx)
                  continue;
                const int lane = (ccy - cy0) * CX + (ccx - cx0);
                s += kc == 2 ? top[below ? (c - 1) & 1 : c & 1][3 * kb + ka][lane] : low[9 * kc + 3 * kb + ka][lane];
              }
            }
          }
          ax = s;
        }
        double o = ax;
        if (MODE >= 1)
        {
          const double res = ax - a.b[id];
          o = res;
          if (MODE >= 2)
          {
            const double step = a.dinv[id] * res;
            o = __builtin_fma(-a.beta, step, xi);
            if (MODE == 3)
              o = __builtin_fma(a.alpha, xi - a.x_prev[id], o);
          }
        }
        a.out[id] = o;
      }
    }
  }
}

// D and D^-1: per node the sum over its cells (z, y, x ascending) of sum_d k_d sum_q c_q (w G_d[q, i]^2), the squares of the
// tables with their weights from the host (VV, DD); constrained entries 1.  One lane per node.
struct Q2DiagArgs
{
  double const *coef;
  uint8_t const *con;
  double *diag, *dinv;
  int n[3], N[3];
  double k[3];
  double VV[9], DD[9]; // [q][a]: w_q V[q][a]^2, w_q D[q][a]^2
};

template <bool COMPACT>
__global__ __launch_bounds__(256) void mf_laplace_q2_diagonal_kernel(Q2DiagArgs a)
{
  const int64_t n_dofs = (int64_t)a.N[0] * a.N[1] * a.N[2];
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_dofs)
    return;
  if (a.con[id])
  {
    a.diag[id] = 1.;
    a.dinv[id] = 1.;
    return;
  }
  const int I = (int)(id % a.N[0]), J = (int)((id / a.N[0]) % a.N[1]), K = (int)(id / ((int64_t)a.N[0] * a.N[1]));
  const int IJK[3] = {I, J, K};
  double s = 0.;
  int cc[3], kk[3];
  for (int zc = 0; zc < 2; ++zc)
    for (int yc = 0; yc < 2; ++yc)
      for (int xc = 0; xc < 2; ++xc)
      {
        const int sel[3] = {xc, yc, zc};
        bool there = true;
        for (int d = 0; d < 3; ++d)
        {
          const bool odd = IJK[d] & 1;
          if (odd && sel[d] == 1)
            there = false;
          cc[d] = odd ? (IJK[d] - 1) / 2 : IJK[d] / 2 - 1 + sel[d];
          kk[d] = odd ? 1 : 2 - 2 * sel[d];
          if (cc[d] < 0 || cc[d] >= a.n[d])
            there = false;
        }
        if (!there)
          continue;
        const size_t cell = (size_t)cc[0] + (size_t)a.n[0] * ((size_t)cc[1] + (size_t)a.n[1] * cc[2]);
        double sc = 0.;
        for (int d = 0; d < 3; ++d)
        {
          double sd = 0.;
          for (int q = 0; q < 27; ++q)
          {
            const int qa = q % 3, qb = (q / 3) % 3, qc = q / 9;
            const double gx = (d == 0 ? a.DD : a.VV)[3 * qa + kk[0]];
            const double gy = (d == 1 ? a.DD : a.VV)[3 * qb + kk[1]];
            const double gz = (d == 2 ? a.DD : a.VV)[3 * qc + kk[2]];
            const double cq = COMPACT ? a.coef[cell] : a.coef[27 * cell + q];
            sd += (cq * a.k[d]) * ((gx * gy) * gz);
          }
          sc += sd;
        }
        s += sc;
      }
  a.diag[id] = s;
  a.dinv[id] = 1. / s;
}

// flag = 1 where the 27 values of a cell differ in their bits
__global__ void q2_cell_constant_kernel(double const *coef, int64_t n_cells, int *flag)
{
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= n_cells)
    return;
  const unsigned long long first = __double_as_longlong(coef[27 * cell]);
  bool same = true;
  for (int q = 1; q < 27; ++q)
    same = same && (unsigned long long)__double_as_longlong(coef[27 * cell + q]) == first;
  if (!same)
    *flag = 1;
}
__global__ void q2_first_value_kernel(double const *coef, int64_t n_cells, double *out)
{
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell < n_cells)
    out[cell] = coef[27 * cell];
}

// the 1-D tables in long double, rounded once
void q2_tables(long double V[9], long double D[9], long double w[3])
{
  const long double r = std::sqrt((long double)3 / 5) / 2;
  const long double g[3] = {0.5L - r, 0.5L, 0.5L + r};
  w[0] = w[2] = (long double)5 / 18;
  w[1] = (long double)8 / 18;
  for (int q = 0; q < 3; ++q)
  {
    const long double x = g[q];
    V[3 * q + 0] = 2 * (x - 0.5L) * (x - 1);
    V[3 * q + 1] = -4 * x * (x - 1);
    V[3 * q + 2] = 2 * x * (x - 0.5L);
    D[3 * q + 0] = 4 * x - 3;
    D[3 * q + 1] = -8 * x + 4;
    D[3 * q + 2] = 4 * x - 1;
  }
}

template <int CX, int CY, bool COMPACT>
void q2_launch_mode(MfMode mode, Q2Args const &a, dim3 grid, hipStream_t stream)
{
  switch (mode)
  {
  case MfMode::apply:
    hipLaunchKernelGGL((mf_laplace_q2_kernel<CX, CY, 0, COMPACT>), grid, dim3(CX * CY), 0, stream, a);
    break;
  case MfMode::residual:
    hipLaunchKernelGGL((mf_laplace_q2_kernel<CX, CY, 1, COMPACT>), grid, dim3(CX * CY), 0, stream, a);
    break;
  case MfMode::first:
    hipLaunchKernelGGL((mf_laplace_q2_kernel<CX, CY, 2, COMPACT>), grid, dim3(CX * CY), 0, stream, a);
    break;
  case MfMode::next:
    hipLaunchKernelGGL((mf_laplace_q2_kernel<CX, CY, 3, COMPACT>), grid, dim3(CX * CY), 0, stream, a);
    break;
  }
}
} // namespace

MatrixFreeLaplaceQ2Device<double>::MatrixFreeLaplaceQ2Device(HipHandle &handle, Q2MeshDesc const &mesh, bool allow_compact)
  : _handle(handle)
{
  if (mesh.dim != 3)
    ASSERT_THROW_NOT_IMPLEMENTED("the Q2 matrix-free operator exists in 3-D only");
  if (handle.comm.enabled())
    ASSERT_THROW_NOT_IMPLEMENTED("the Q2 matrix-free operator runs on one rank (the context has a communicator)");
  if (mesh.coefficient == nullptr || mesh.constrained == nullptr)
    throw InvalidArgumentExc("null mesh array");
  double dofs = 1.;
  for (int d = 0; d < 3; ++d)
  {
    if (mesh.n_cells[d] < 1 || !(mesh.cell_size[d] > 0.))
      throw InvalidArgumentExc("the Q2 mesh needs at least one cell and a positive cell size per direction");
    _n[d] = mesh.n_cells[d];
    _h[d] = mesh.cell_size[d];
    dofs *= 2. * mesh.n_cells[d] + 1.;
  }
  if (dofs >= 2147483648.)
    throw InvalidArgumentExc("the Q2 matrix-free operator indexes its unknowns with 32 bits: n_dofs must be below 2^31");
  for (int d = 0; d < 3; ++d)
    _N[d] = 2 * _n[d] + 1;
  _n_dofs = (int64_t)_N[0] * _N[1] * _N[2];
  if (mesh.n_dofs != _n_dofs)
    throw InvalidArgumentExc("n_dofs is not the lattice (2 nx + 1)(2 ny + 1)(2 nz + 1) of the Q2 mesh");
  const int64_t cells = (int64_t)_n[0] * _n[1] * _n[2];
  const hipMemcpyKind kind = mesh.arrays_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  MemoryKind memory("Q2 matrix-free operator: coefficients, flags, diagonal");
  _constrained.resize((size_t)_n_dofs);
  MFMG_HIP_CHECK(hipMemcpyAsync(_constrained.data(), mesh.constrained, (size_t)_n_dofs, kind, handle.stream));
  _coef.resize((size_t)cells * 27);
  MFMG_HIP_CHECK(hipMemcpyAsync(_coef.data(), mesh.coefficient, (size_t)cells * 27 * sizeof(double), kind, handle.stream));
  if (allow_compact)
  {
    DeviceBuffer<int> flag(1);
    MFMG_HIP_CHECK(hipMemsetAsync(flag.data(), 0, sizeof(int), handle.stream));
    hipLaunchKernelGGL(q2_cell_constant_kernel, dim3(n_blocks_for(cells)), dim3(block_size), 0, handle.stream, _coef.data(), cells,
                       flag.data());
    MFMG_HIP_CHECK(hipGetLastError());
    _compact = flag.download(handle.stream)[0] == 0;
    if (_compact)
    {
      DeviceBuffer<double> one((size_t)cells);
      hipLaunchKernelGGL(q2_first_value_kernel, dim3(n_blocks_for(cells)), dim3(block_size), 0, handle.stream, _coef.data(), cells,
                         one.data());
      MFMG_HIP_CHECK(hipGetLastError());
      MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream));
      _coef = std::move(one);
    }
  }
  // the diagonal
  _diag.resize((size_t)_n_dofs);
  _dinv.resize((size_t)_n_dofs);
  Q2DiagArgs a;
  a.coef = _coef.data();
  a.con = _constrained.data();
  a.diag = _diag.data();
  a.dinv = _dinv.data();
  long double V[9], D[9], w[3];
  q2_tables(V, D, w);
  for (int d = 0; d < 3; ++d)
  {
    a.n[d] = _n[d];
    a.N[d] = _N[d];
    a.k[d] = _h[0] * _h[1] * _h[2] / (_h[d] * _h[d]);
  }
  for (int q = 0; q < 3; ++q)
    for (int i = 0; i < 3; ++i)
    {
      a.VV[3 * q + i] = (double)(w[q] * V[3 * q + i] * V[3 * q + i]);
      a.DD[3 * q + i] = (double)(w[q] * D[3 * q + i] * D[3 * q + i]);
    }
  const dim3 grid(n_blocks_for(_n_dofs, 256, (int64_t)1 << 30));
  if (_compact)
    hipLaunchKernelGGL(mf_laplace_q2_diagonal_kernel<true>, grid, dim3(256), 0, handle.stream, a);
  else
    hipLaunchKernelGGL(mf_laplace_q2_diagonal_kernel<false>, grid, dim3(256), 0, handle.stream, a);
  MFMG_HIP_CHECK(hipGetLastError());
  MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream));
}

void MatrixFreeLaplaceQ2Device<double>::set_tile(int shape)
{
  if (shape < -1 || shape >= kQ2TileShapes)
    throw InvalidArgumentExc("unknown tile shape of the Q2 operator");
  _shape = shape < 0 ? 0 : shape;
}

void MatrixFreeLaplaceQ2Device<double>::launch(MfMode mode, MfOperands<double> const &v) const
{
  if (v.x == nullptr || v.out == nullptr)
    throw InvalidArgumentExc("null vector");
  if (v.x == v.out)
    throw InvalidArgumentExc("the operator kernel cannot run in place (out aliases x)");
  if (mode != MfMode::apply && v.b == nullptr)
    throw InvalidArgumentExc("null right-hand side");
  if (mode == MfMode::next)
    mode = mf_smoother_mode(v.x_prev, v.alpha);
  Q2Args a;
  a.x = v.x;
  a.b = v.b;
  a.x_prev = v.x_prev;
  a.dinv = _dinv.data();
  a.out = v.out;
  a.coef = _coef.data();
  a.con = _constrained.data();
  a.alpha = v.alpha;
  a.beta = v.beta;
  long double V[9], D[9], w[3];
  q2_tables(V, D, w);
  for (int d = 0; d < 3; ++d)
  {
    a.n[d] = _n[d];
    a.N[d] = _N[d];
    a.k[d] = _h[0] * _h[1] * _h[2] / (_h[d] * _h[d]);
  }
  for (int q = 0; q < 3; ++q)
    for (int i = 0; i < 3; ++i)
    {
      a.t.V[3 * q + i] = (double)V[3 * q + i];
      a.t.D[3 * q + i] = (double)D[3 * q + i];
      a.t.Vw[3 * q + i] = (double)(w[q] * V[3 * q + i]);
      a.t.Dw[3 * q + i] = (double)(w[q] * D[3 * q + i]);
    }
  const Q2Tile tile = kQ2Tiles[_shape];
  a.tz = tile.tz;
  const dim3 grid((_n[0] + tile.tx() - 1) / tile.tx(), (_n[1] + tile.ty() - 1) / tile.ty(), (_n[2] + tile.tz - 1) / tile.tz);
  hipStream_t stream = _handle.stream;
  if (tile.cx == 16 && tile.cy == 8)
    _compact ? q2_launch_mode<16, 8, true>(mode, a, grid, stream) : q2_launch_mode<16, 8, false>(mode, a, grid, stream);
  else
    _compact ? q2_launch_mode<8, 8, true>(mode, a, grid, stream) : q2_launch_mode<8, 8, false>(mode, a, grid, stream);
  MFMG_HIP_CHECK(hipGetLastError());
}
} // namespace mfmg
