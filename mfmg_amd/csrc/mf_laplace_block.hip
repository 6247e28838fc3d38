// gfx950 kernel of the matrix-free Q1 Laplace operator for a BLOCK of NV vectors (NV = 2, 4): one term per launch as
// mf_laplace_kernel (mf_laplace.hip), FP64, 3-D, eight coefficients per cell, all four modes of MfMode.
//
// Why: a `next` smoother term of the one-vector kernel with computed ids moves 104 B per DoF, of which 72 B are the chunk
// record (eight coefficients and D^-1) and 32 B the vectors.  Every vector of a block reads the same record, so NV vectors per
// launch move 72 / NV + 32 B per DoF and vector.
//
// The body is mf_laplace_body with the vector state held NV times.  Once per slot: the ids, the eight coefficients, D^-1, the
// cell factors and every predicate.  Per vector: the x values and their masked copies, the register carries in y, the deferred
// first row, the epilogue operands and the LDS columns (z-carry of the partial sums and of x, the hand-over slots).  Column c
// goes through exactly the operations of the one-vector kernel, in its order, on the same helpers of mf_device.hpp with implicit
// contraction off: every column of the result equals the one-vector result bit for bit, for every tile.
//
// The vectors of a block are columns with a common leading dimension: column c of x starts at x + c * ld elements.  The column
// base is wave-uniform (64 bits, scalar registers); the per-lane part stays the 32-bit byte offset of id_off, so a column stays
// under 2^32 bytes and the block as a whole need not.
#include "mf_laplace.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>

#include "mf_device.hpp"

namespace mfmg
{
namespace
{
// LDS of a workgroup of nw wavefronts of ty cell rows at nv vectors: per wavefront pt[nv][ty] and xz[nv][ty + 1] (columns of
// 64 doubles), the hand-over slots [2][nw][nv][2], per wavefront the id column idz[ty + 1] (held once for all vectors)
constexpr size_t mf_block_lds(int nv, int nw, int ty, size_t elem)
{
  return ((size_t)nw * nv * (2 * ty + 1) + (size_t)2 * nw * nv * 2) * 64 * elem + (size_t)nw * (ty + 1) * 64 * sizeof(int);
}

// The tile body (see mf_laplace_body for the march, the data conventions and the memory pipeline).  TY rows per wavefront at
// compile time, one request batch per cell row: the NV x requests of the row, its coefficients (16 VGPRs, shared), the epilogue
// operands of the row it completes -- all issued before the first cell of the row is computed.  The ids of the next pass are
// prefetched across the barrier.
template <typename T, int NV, int TY, bool AFF>
__device__ __forceinline__ void mf_laplace_block_body(MfArgs<T> const &a, size_t ldim, unsigned int bid)
{
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave-uniform, keep it scalar
  const int NW = blockDim.x >> 6;
  constexpr int kWave = NV * (2 * TY + 1) * 64;
  T *pt = reinterpret_cast<T *>(smem_raw) + (size_t)wv * kWave;         // [NV][TY][64]   z-carry of the partial sums
  T *xz = pt + NV * TY * 64;                                            // [NV][TY+1][64] z-carry of x, one slot per node row
  T *xport = reinterpret_cast<T *>(smem_raw) + (size_t)NW * kWave;      // [2][NW][NV][2][64]
  int *idz = reinterpret_cast<int *>(xport + (size_t)2 * NW * NV * 2 * 64) + (size_t)wv * (TY + 1) * 64;

  // XCD-aware tile order, as the one-vector kernel
  const unsigned int n_tiles = a.ncols_active * a.ntiles_y * a.ntiles_z;
  unsigned int w = bid;
  if (n_tiles >= 64)
  {
    const unsigned int per_xcd = (n_tiles + 7) / 8;
    w = (bid % 8) * per_xcd + bid / 8;
    if (w >= n_tiles)
      return; // the whole workgroup leaves: no barrier is left waiting
  }
  const unsigned int nc = a.ncols_active, ny = a.ntiles_y;
  const int tc = a.col0 + w % nc;
  const int tyi = a.ty0 + (w / nc) % ny;
  const int tzi = a.z_tile0 + w / (nc * ny);
  const int ci = tc * a.own - a.halo + lane;        // cell / DoF column of this lane
  const int Yb = tyi * (NW * TY - 1) - 1 + wv * TY; // first cell row of this wavefront
  const int Z0 = a.ztab[tzi];
  const int TZt = a.ztab[tzi + 1] - Z0; // layers this tile owns
  const bool col_owned = lane >= a.halo && lane < a.halo + a.own && ci < a.Nx;
  const int jj0 = (Yb < 0) ? 1 : 0; // cell row -1 does not exist (its sums are the zero initial carries)
  const size_t rec_row = (size_t)a.ncols * a.rec_bytes;
  const size_t rec_layer = (size_t)a.Ny * rec_row;
  unsigned char const *rec_col = a.rec + (size_t)tc * a.rec_bytes;
  const bool have_rows = (jj0 < TY) && (Yb + jj0 < a.Ny);
  CellFactors<T> fac;
  fac.fx = a.fx;
  fac.fy = a.fy;
  fac.fz = a.fz;
  fac.fax = a.fax;
  fac.fbx = a.fbx;
  fac.fay = a.fay;
  fac.fby = a.fby;
  fac.faz = a.faz;
  fac.fbz = a.fbz;
  // the columns of the block: wave-uniform bases
  const size_t col_bytes = ldim * sizeof(T);
  auto col = [&](T const *base, int c) { return reinterpret_cast<T const *>(reinterpret_cast<char const *>(base) + (size_t)c * col_bytes); };
  auto col_out = [&](int c) { return reinterpret_cast<T *>(reinterpret_cast<char *>(a.out) + (size_t)c * col_bytes); };

  const int id_lane = a.aff.base + ci * a.aff.s0; // (AFF) the part of the id that belongs to the lane
  const bool lane_in = ci >= 0 && ci < a.Nx;
  const bool cell_lane = ci >= 0 && ci < a.Nx - 1; // the slot holds a real cell (the others carry coefficient zero)
  const bool lane_face = ((a.aff.faces & 1) && ci == 0) || ((a.aff.faces & 2) && ci == a.Nx - 1);
  const bool any_ghost = (a.aff.ghost_lo[0] | a.aff.ghost_hi[0] | a.aff.ghost_lo[1] | a.aff.ghost_hi[1] | a.aff.ghost_lo[2] | a.aff.ghost_hi[2]) != 0;
  const bool lane_ghost = any_ghost && (ci < a.aff.ghost_lo[0] || ci >= a.Nx - a.aff.ghost_hi[0]);
  // own id of node row `jrow` (clamped into the mesh) in layer kz
  auto own_id = [&](int kz, int jrow) {
    const int jr = min(max(jrow, 0), a.Ny - 1);
    if constexpr (AFF)
    {
      const int id_row = jr * a.aff.s1 + kz * a.aff.s2;
      const bool row_face = ((a.aff.faces & 4) && jr == 0) || ((a.aff.faces & 8) && jr == a.Ny - 1) ||
                            ((a.aff.faces & 16) && kz == 0) || ((a.aff.faces & 32) && kz == a.Nz - 1);
      const bool row_ghost = any_ghost && (kz < a.aff.ghost_lo[2] || kz >= a.Nz - a.aff.ghost_hi[2] || jr < a.aff.ghost_lo[1] || jr >= a.Ny - a.aff.ghost_hi[1]);
      const bool face = lane_face || row_face;
      const int id = (id_lane + id_row) | (face ? (int)kFlag : 0) | (((lane_ghost || row_ghost) && !face) ? (int)kGhost : 0);
      return lane_in ? id : 0; // (lanes outside the mesh carry id 0 in the records too)
    }
    else
      return reinterpret_cast<int const *>(rec_col + (size_t)kz * rec_layer + (size_t)jr * rec_row)[lane];
  };
  int pf[TY + 1]; // own ids of the node rows Yb .. Yb + TY in the layer after next
#pragma unroll
  for (int r = 0; r < TY + 1; ++r)
    pf[r] = 0;

  for (int kk = 0; kk <= TZt; ++kk)
  {
    const int k = Z0 - 1 + kk;
    if (k >= a.Nz)
      break; // uniform over the workgroup
    const int kc = max(k, 0);            // layer the records of "layer k" are read from
    const int kn = min(k + 1, a.Nz - 1); // ... and those of layer k + 1
    const bool no_cells = k < 0;         // the halo layer below the mesh: coefficient forced to zero
    const bool layer_carry = kk > 0;     // xz / idz hold x and the ids of layer k, written by the pass of layer k - 1
    unsigned char const *rec_k = rec_col + (size_t)kc * rec_layer;
    // per vector: the y carries, the b=0 face carried from the previous cell row (masked x of the four corners, the raw value
    // of the own DoF), the first DoF row of a wavefront w > 0 (finished after the barrier)
    T ry0[NV], ry1[NV], cxm[NV][4], cx0[NV];
    T d00[NV], d01[NV], dx0[NV], dlb[NV], dlx[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c)
    {
      ry0[c] = ry1[c] = cx0[c] = T(0);
      cxm[c][0] = cxm[c][1] = cxm[c][2] = cxm[c][3] = T(0);
      d00[c] = d01[c] = dx0[c] = dlb[c] = dlx[c] = T(0);
    }
    // once: the id of the own DoF of the carried face, id and D^-1 of the deferred row
    int id0 = 0, did0 = 0;
    T dld = T(0);

    // ---- first node row of the pass (the b=0 face of its first cell row)
    if (have_rows)
    {
      const int jf = Yb + jj0;
      int idBf, idAf;
      T xAf[NV], xBf[NV];
      if (layer_carry)
      {
        idAf = idz[jj0 * 64 + lane];
#pragma unroll
        for (int c = 0; c < NV; ++c)
          xAf[c] = xz[(c * (TY + 1) + jj0) * 64 + lane];
        idBf = jj0 ? pf[1] : pf[0]; // (no run-time index into the register array)
      }
      else
      {
        idAf = own_id(kc, jf);
        idBf = own_id(kn, jf);
#pragma unroll
        for (int c = 0; c < NV; ++c)
          xAf[c] = ld_off<T>(col(a.x, c), id_off<T>(idAf));
      }
#pragma unroll
      for (int c = 0; c < NV; ++c)
        xBf[c] = ld_off<T>(col(a.x, c), id_off<T>(idBf));
      if (wv > 0 && kk > 0 && a.mode != 0)
      {
        // epilogue operands of the deferred row (its id has been in LDS since the previous pass)
        const unsigned int g = id_off<T>(idAf);
#pragma unroll
        for (int c = 0; c < NV; ++c)
          dlb[c] = ld_off<T>(col(a.b, c), g);
        if (a.mode >= 2)
          dld = reinterpret_cast<T const *>(rec_k + (size_t)jf * rec_row + Rec<T, false>::kDinvOff)[lane];
        if (a.mode == 3)
        {
#pragma unroll
          for (int c = 0; c < NV; ++c)
            dlx[c] = ld_off<T>(col(a.xprev, c), g);
        }
      }
      idz[jj0 * 64 + lane] = idBf;
      id0 = idAf;
#pragma unroll
      for (int c = 0; c < NV; ++c)
      {
        xz[(c * (TY + 1) + jj0) * 64 + lane] = xBf[c];
        cx0[c] = xAf[c];
        cxm[c][0] = masked<T>(xAf[c], idAf);
        cxm[c][2] = masked<T>(xBf[c], idBf);
        cxm[c][1] = from_next_lane(cxm[c][0]);
        cxm[c][3] = from_next_lane(cxm[c][2]);
      }
    }

#pragma unroll
    for (int jj = 0; jj < TY; ++jj)
    {
      // ---- every request of the row: node row jj + 1 (the b=1 face of cell row jj)
      const int j = Yb + jj;
      const bool ok = jj >= jj0 && j < a.Ny;
      int idA = 0, idB = 0;
      T xA[NV], xB[NV], lb[NV], lxp[NV];
      T ldv = T(0);
      T cf[8];
#pragma unroll
      for (int c = 0; c < NV; ++c)
        xA[c] = xB[c] = lb[c] = lxp[c] = T(0);
      if (ok)
      {
        if (layer_carry)
        {
          idA = idz[(jj + 1) * 64 + lane];
#pragma unroll
          for (int c = 0; c < NV; ++c)
            xA[c] = xz[(c * (TY + 1) + jj + 1) * 64 + lane];
          idB = pf[jj + 1];
        }
        else
        {
          idA = own_id(kc, j + 1);
          idB = own_id(kn, j + 1);
        }
        unsigned char const *recp = rec_k + (size_t)j * rec_row;
#pragma unroll
        for (int c = 0; c < NV; ++c)
          xB[c] = ld_off<T>(col(a.x, c), id_off<T>(idB));
        if (!layer_carry)
        {
#pragma unroll
          for (int c = 0; c < NV; ++c)
            xA[c] = ld_off<T>(col(a.x, c), id_off<T>(idA));
        }
        // slots without a real cell are stored as zeros: do not fetch them (64 bytes per slot; the same bits)
#pragma unroll
        for (int q = 0; q < 8; ++q)
          cf[q] = T(0);
        if (cell_lane && j < a.Ny - 1 && k >= 0 && k < a.Nz - 1)
          load_coef<T, false>(recp, lane, cf);
        if (jj > 0 && kk > 0 && a.mode != 0)
        {
          // the DoF row this cell row completes: node row jj, id = the layer-k id of the previous node row
          const unsigned int gid = id_off<T>(id0);
#pragma unroll
          for (int c = 0; c < NV; ++c)
            lb[c] = ld_off<T>(col(a.b, c), gid);
          if (a.mode >= 2)
            ldv = reinterpret_cast<T const *>(recp + Rec<T, false>::kDinvOff)[lane];
          if (a.mode == 3)
          {
#pragma unroll
            for (int c = 0; c < NV; ++c)
              lxp[c] = ld_off<T>(col(a.xprev, c), gid);
          }
        }
      }
      // ids of the next pass (layer k + 2): the node rows whose current ids this row has just consumed
      if (have_rows)
      {
        if (jj == 0)
          pf[0] = own_id(min(k + 2, a.Nz - 1), Yb);
        pf[jj + 1] = own_id(min(k + 2, a.Nz - 1), Yb + jj + 1);
      }
      if (!ok)
        continue;

      // ---- the row
      idz[(jj + 1) * 64 + lane] = idB;
      if (no_cells)
      {
#pragma unroll
        for (int q = 0; q < 8; ++q)
          cf[q] = T(0);
      }
      const int idr = id0;
      const bool deferred = jj == 0 && wv > 0; // the b=1 sums of the row below arrive from wavefront w-1 after the barrier
      const bool stores = jj > 0 && kk > 0 && col_owned && !((unsigned int)idr & kGhost);
#pragma unroll
      for (int c = 0; c < NV; ++c)
      {
        xz[(c * (TY + 1) + jj + 1) * 64 + lane] = xB[c];
        const T n0m = masked<T>(xA[c], idA), n2m = masked<T>(xB[c], idB);
        const T n1m = from_next_lane(n0m), n3m = from_next_lane(n2m);
        T u[8], v[8];
        u[0] = cxm[c][0];
        u[1] = cxm[c][1];
        u[4] = cxm[c][2];
        u[5] = cxm[c][3];
        u[2] = n0m;
        u[3] = n1m;
        u[6] = n2m;
        u[7] = n3m;
        cell_apply<T>(u, cf, fac, v);
        const T x0 = cx0[c];
        cxm[c][0] = n0m;
        cxm[c][1] = n1m;
        cxm[c][2] = n2m;
        cxm[c][3] = n3m;
        cx0[c] = xA[c];

        // ---- x combine: DoF column ci gets the a=0 corners of its own cell and the a=1 corners of the cell to the left
        const T s00 = v[0] + from_prev_lane(v[1]); // s[b][d]: b=0,d=0
        const T s10 = v[2] + from_prev_lane(v[3]); // b=1,d=0
        const T s01 = v[4] + from_prev_lane(v[5]); // b=0,d=1
        const T s11 = v[6] + from_prev_lane(v[7]); // b=1,d=1
        if (deferred)
        {
          d00[c] = s00;
          d01[c] = s01;
          dx0[c] = x0;
        }
        else
        {
          // ---- y combine (register carry), z combine (LDS column carry)
          const T t0 = s00 + ry0[c];
          const T t1 = s01 + ry1[c];
          T *ptj = pt + (c * TY + jj) * 64 + lane;
          const T yv = t0 + *ptj; // (layer kk = 0 reads what an earlier tile left there: never stored)
          *ptj = t1;
          if (stores)
            st_off<T>(col_out(c), id_off<T>(idr), mf_epilogue<T>(a, idr, x0, yv, lb[c], ldv, lxp[c]));
        }
        ry0[c] = s10;
        ry1[c] = s11;
      }
      if (deferred)
        did0 = idr;
      id0 = idA;
    }
    if (NW > 1)
    {
      // exports are double-buffered by layer parity: a slot written in layer k is read after barrier k
      // and rewritten in layer k+2, i.e. after barrier k+1, which the reader only passes once it has read
      T *xp = xport + ((size_t)((kk & 1) * NW + wv) * NV * 2) * 64 + lane;
#pragma unroll
      for (int c = 0; c < NV; ++c)
      {
        xp[(2 * c) * 64] = ry0[c];
        xp[(2 * c + 1) * 64] = ry1[c];
      }
      __syncthreads();
      if (wv > 0)
      {
        T const *ip = xport + ((size_t)((kk & 1) * NW + wv - 1) * NV * 2) * 64 + lane;
        const bool stores = kk > 0 && have_rows && col_owned && !((unsigned int)did0 & kGhost);
#pragma unroll
        for (int c = 0; c < NV; ++c)
        {
          const T t0 = d00[c] + ip[(2 * c) * 64];
          const T t1 = d01[c] + ip[(2 * c + 1) * 64];
          T *ptj = pt + (c * TY) * 64 + lane;
          const T yv = t0 + *ptj;
          *ptj = t1;
          if (stores)
            st_off<T>(col_out(c), id_off<T>(did0), mf_epilogue<T>(a, did0, dx0[c], yv, dlb[c], dld, dlx[c]));
        }
      }
    }
  }
}

template <int NV, int TY, bool AFF>
__global__ __launch_bounds__(512) void mf_laplace_block_kernel(MfArgs<double> a, size_t ldim)
{
  mf_laplace_block_body<double, NV, TY, AFF>(a, ldim, blockIdx.x);
}

// the float instances: a kernel of their own name (the profiler and the resource tests tell the two apart)
template <int NV, int TY, bool AFF>
__global__ __launch_bounds__(512) void mf_laplace_block_f32_kernel(MfArgs<float> a, size_t ldim)
{
  mf_laplace_block_body<float, NV, TY, AFF>(a, ldim, blockIdx.x);
}

template <int NV>
void block_kernel_launch(MfArgs<double> const &a, size_t ldim, MfGrid const &grid, int ty, bool affine)
{
  auto go = [&](auto kernel) { mf_launch(kernel, grid, a, ldim); };
  with_flag(affine, [&](auto aff) {
    constexpr bool AFF = decltype(aff)::value;
    if (ty == 2)
      go(mf_laplace_block_kernel<NV, 2, AFF>);
    else if (ty == 3)
      go(mf_laplace_block_kernel<NV, 3, AFF>);
    else
      go(mf_laplace_block_kernel<NV, 4, AFF>);
  });
}

template <int NV>
void block_kernel_launch(MfArgs<float> const &a, size_t ldim, MfGrid const &grid, int ty, bool affine)
{
  auto go = [&](auto kernel) { mf_launch(kernel, grid, a, ldim); };
  with_flag(affine, [&](auto aff) {
    constexpr bool AFF = decltype(aff)::value;
    if (ty == 2)
      go(mf_laplace_block_f32_kernel<NV, 2, AFF>);
    else if (ty == 3)
      go(mf_laplace_block_f32_kernel<NV, 3, AFF>);
    else
      go(mf_laplace_block_f32_kernel<NV, 4, AFF>);
  });
}
} // namespace

// ---- how a block of k vectors is cut into launches: groups of 4, then one of 2, then one single vector ----
int mf_block_groups(int n_vectors, int widths[kMfBlockMaxGroups])
{
  if (n_vectors < 1 || n_vectors > kMfBlockMaxVectors)
    throw InvalidArgumentExc("a block holds 1 to 64 vectors");
  int n = 0;
  for (int left = n_vectors; left > 0;)
  {
    const int w = left >= 4 ? 4 : (left >= 2 ? 2 : 1);
    widths[n++] = w;
    left -= w;
  }
  return n;
}

template <typename T>
bool MatrixFreeLaplaceDevice<T>::block_kernel_available() const
{
  return _dim == 3 && !_compact && !_tail && _halo == 1 && _dinv_in_record;
}

// Tiles of the block kernel.  Its wavefronts hold NV times the requests in flight of a one-vector wavefront and NV times its LDS
// columns, so it runs fewer of them: the (8, 2, tz) tile of the one-vector list is at the LDS limit at NV = 4 (150 KiB) and would
// leave a compute unit one workgroup; four wavefronts of two rows (75 KiB at NV = 4, 42 KiB at NV = 2) let two or three workgroups
// share a compute unit.  Two rows at NV = 2 as well: that instance allocates 156 VGPRs (three wavefronts per SIMD), those of three
// and four rows 166 - 173 (two).  As for the one-vector kernel the largest tile that still gives every compute unit two rounds
// is taken.
// FP32: half the LDS (39 KiB at NV = 4 and four wavefronts of two rows, 22 KiB at NV = 2) and fewer VGPRs of vector state; see
// kBlockTilesF32 below for the register counts of the twelve instances and the list chosen by timing.
namespace
{
struct BlockTilePrefs
{
  int tile[5][3];
  int waves_per_simd; // the occupancy the list plans (512 VGPRs / waves per SIMD bound the instance)
};
// FP64 (see above)
constexpr BlockTilePrefs kBlockTilesF64[2] = {{{{4, 2, 16}, {4, 2, 8}, {2, 2, 8}, {2, 2, 4}, {1, 2, 4}}, 3},  // NV = 2
                                              {{{4, 2, 16}, {4, 2, 8}, {2, 2, 8}, {2, 2, 4}, {1, 2, 4}}, 2}}; // NV = 4
// FP32.  VGPRs of the instances <NV, TY> (AFF false / true), from the code object metadata, no spill, no scratch:
//   <2, 2>  98 / 101    <2, 3> 121 / 118    <2, 4> 125 / 120     -- all within 128: four wavefronts per SIMD
//   <4, 2> 141 / 141    <4, 3> 153 / 150    <4, 4> 157 / 152     -- all within 168: three wavefronts per SIMD
// (FP64: 156 - 173 at NV = 2, 220 - 245 at NV = 4.)  The lists plan that occupancy; their order was chosen by timing at 257^3
// DoFs.
constexpr BlockTilePrefs kBlockTilesF32[2] = {{{{4, 2, 16}, {4, 2, 8}, {2, 2, 8}, {2, 2, 4}, {1, 2, 4}}, 4},  // NV = 2
                                              {{{4, 2, 16}, {4, 2, 8}, {2, 2, 8}, {2, 2, 4}, {1, 2, 4}}, 3}}; // NV = 4
} // namespace

template <typename T>
MfTile MatrixFreeLaplaceDevice<T>::choose_block_tile(int nv) const
{
  if (_block_tile[0] > 0 && _block_tile[1] > 0 && _block_tile[2] > 0)
    return {_block_tile[0], _block_tile[1], _block_tile[2]};
  BlockTilePrefs const &p = (std::is_same<T, double>::value ? kBlockTilesF64 : kBlockTilesF32)[nv >= 4 ? 1 : 0];
  const int(*pref)[3] = p.tile;
  constexpr int n_pref = 5;
  const int64_t waves_wanted = (int64_t)2 * 4 * p.waves_per_simd * mf_n_cus(); // two rounds at the planned occupancy
  int pick = n_pref - 1;
  for (int c = 0; c < n_pref; ++c)
  {
    const int64_t wgs = (int64_t)_ncols * ((_N[1] + pref[c][0] * pref[c][1] - 2) / (pref[c][0] * pref[c][1] - 1)) *
                        ((_N[2] + pref[c][2] - 1) / pref[c][2]);
    if (wgs * pref[c][0] >= waves_wanted)
    {
      pick = c;
      break;
    }
  }
  return {pref[pick][0], pref[pick][1], pref[pick][2]};
}

template <typename T>
void MatrixFreeLaplaceDevice<T>::get_block_tile(int nv, int &nw, int &ty, int &tz) const
{
  if (nv != 2 && nv != 4)
    throw InvalidArgumentExc("the block kernel runs 2 or 4 vectors per launch");
  const MfTile t = choose_block_tile(nv);
  nw = t.nw;
  ty = t.ty;
  tz = t.tz;
}

// one launch of the block kernel: nv = 2 or 4 columns
template <typename T>
void MatrixFreeLaplaceDevice<T>::run_block(MfMode mode, MfBlockOperands<T> const &v, int nv) const
{
  {
    const MfTile tile = choose_block_tile(nv);
    const int nw = tile.nw, ty = tile.ty, tz = tile.tz;
    ASSERT_THROW(nw >= 1 && nw <= 8, "1..8 wavefronts per workgroup");
    ASSERT_THROW(ty >= 2 && ty <= 4 && tz >= 1, "the block kernel runs 2, 3 or 4 cell rows per wavefront");
    const size_t lds = mf_block_lds(nv, nw, ty, sizeof(T));
    ASSERT_THROW(lds <= kMfMaxLds, "operator tile too large for the LDS");
    static const bool graded_env = !(std::getenv("MFMG_MF_GRADED_TILES") && std::string(std::getenv("MFMG_MF_GRADED_TILES")) == "0");
    int all_z = 0;
    int const *ztab = z_tiling(tz, graded_env, all_z);
    MfArgs<T> a;
    make_args(a, mode, MfOperands<T>{v.x, v.b, v.x_prev, v.alpha, v.beta, v.out}, tile, ztab, all_z);
    const uint64_t n_tiles = (uint64_t)a.ncols_active * a.ntiles_y * a.ntiles_z;
    ASSERT_THROW(n_tiles < (1ull << 30), "operator tile too small for this mesh (grid size limit)");
    const MfGrid grid{mf_xcd_grid(n_tiles), nw, lds, _handle.stream};
    // bytes the layout requires: the record once, the vectors of the mode nv times
    const double vec = sizeof(T) * double(_n_dofs);
    const double record = required_bytes_apply() - 2. * vec + (mode >= MfMode::first ? vec : 0.);
    const double vectors = 2. * vec + (mode == MfMode::apply ? 0. : vec) + (mode == MfMode::next ? vec : 0.);
    hipEvent_t stop = _handle.profiler.begin(std::is_same<T, double>::value ? "mf_laplace_block_kernel" : "mf_laplace_block_f32_kernel",
                                             record + nv * vectors, _handle.stream);
    if (nv == 4)
      block_kernel_launch<4>(a, (size_t)v.ld, grid, ty, _affine_ids);
    else
      block_kernel_launch<2>(a, (size_t)v.ld, grid, ty, _affine_ids);
    MFMG_HIP_CHECK(hipGetLastError());
    KernelProfiler::end(stop, _handle.stream);
    ++_block_launches;
  }
}

template <typename T>
void MatrixFreeLaplaceDevice<T>::launch_block(MfMode mode, MfBlockOperands<T> const &v) const
{
  auto require = [](bool cond, char const *what) {
    if (!cond)
      throw InvalidArgumentExc(what);
  };
  require(!_handle.comm.enabled(), "blocks of vectors are not implemented for a context with a communicator");
  launch_block_local(mode, v);
}

template <typename T>
void MatrixFreeLaplaceDevice<T>::launch_block_local(MfMode mode, MfBlockOperands<T> const &v) const
{
  auto require = [](bool cond, char const *what) {
    if (!cond)
      throw InvalidArgumentExc(what);
  };
  require(v.n_vectors >= 1 && v.n_vectors <= kMfBlockMaxVectors, "a block holds 1 to 64 vectors");
  require(v.ld >= _n_dofs, "the leading dimension of a block must be at least n_dofs");
  // (a lane reads one element at a time: a column need only be aligned to two elements, 16 bytes in FP64 and 8 in FP32)
  constexpr uintptr_t kAlign = 2 * sizeof(T);
  require(v.ld % 2 == 0, sizeof(T) == 8 ? "the leading dimension of a block must be even (columns aligned to 16 bytes)"
                                        : "the leading dimension of a block must be even (columns aligned to 8 bytes)");
  require(v.x != nullptr && v.out != nullptr, "null vector");
  if (mode == MfMode::next)
    mode = mf_smoother_mode(v.x_prev, v.alpha);
  require(mode == MfMode::apply || v.b != nullptr, "null right-hand side");
  auto aligned = [](void const *p) { return p == nullptr || reinterpret_cast<uintptr_t>(p) % kAlign == 0; };
  require(aligned(v.x) && aligned(v.out) && (mode == MfMode::apply || aligned(v.b)) && (mode != MfMode::next || aligned(v.x_prev)),
          sizeof(T) == 8 ? "the base of a block must be aligned to 16 bytes" : "the base of a block must be aligned to 8 bytes");
  // (the blocks as address ranges: the last column ends n_dofs after its start)
  const int64_t extent = (int64_t)(v.n_vectors - 1) * v.ld + _n_dofs;
  require(v.out + extent <= v.x || v.x + extent <= v.out, "the operator kernel cannot run in place (the out block overlaps the x block)");

  int widths[kMfBlockMaxGroups];
  const int n_groups = mf_block_groups(v.n_vectors, widths);
  const bool kernel = block_kernel_available();
  int c = 0;
  for (int g = 0; g < n_groups; ++g)
  {
    const int wdt = widths[g];
    auto at = [&](T const *p, int col) { return p ? p + (int64_t)col * v.ld : nullptr; };
    if (kernel && wdt > 1)
    {
      MfBlockOperands<T> s = v;
      s.x = at(v.x, c);
      s.b = at(v.b, c);
      s.x_prev = at(v.x_prev, c);
      s.out = v.out + (int64_t)c * v.ld;
      s.n_vectors = wdt;
      run_block(mode, s, wdt);
    }
    else
      for (int q = c; q < c + wdt; ++q)
        launch(mode, {at(v.x, q), at(v.b, q), at(v.x_prev, q), v.alpha, v.beta, v.out + (int64_t)q * v.ld});
    c += wdt;
  }
}

template bool MatrixFreeLaplaceDevice<double>::block_kernel_available() const;
template MfTile MatrixFreeLaplaceDevice<double>::choose_block_tile(int) const;
template void MatrixFreeLaplaceDevice<double>::get_block_tile(int, int &, int &, int &) const;
template void MatrixFreeLaplaceDevice<double>::run_block(MfMode, MfBlockOperands<double> const &, int) const;
template void MatrixFreeLaplaceDevice<double>::launch_block(MfMode, MfBlockOperands<double> const &) const;
template void MatrixFreeLaplaceDevice<double>::launch_block_local(MfMode, MfBlockOperands<double> const &) const;
template bool MatrixFreeLaplaceDevice<float>::block_kernel_available() const;
template MfTile MatrixFreeLaplaceDevice<float>::choose_block_tile(int) const;
template void MatrixFreeLaplaceDevice<float>::get_block_tile(int, int &, int &, int &) const;
template void MatrixFreeLaplaceDevice<float>::run_block(MfMode, MfBlockOperands<float> const &, int) const;
template void MatrixFreeLaplaceDevice<float>::launch_block(MfMode, MfBlockOperands<float> const &) const;
template void MatrixFreeLaplaceDevice<float>::launch_block_local(MfMode, MfBlockOperands<float> const &) const;
} // namespace mfmg
