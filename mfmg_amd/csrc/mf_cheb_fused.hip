// Several terms of the Chebyshev / Jacobi smoother of the matrix-free Q1 Laplace operator in ONE sweep over the mesh
// (temporal blocking).
//
// What it computes, bit for bit, is what K launches of mf_laplace_kernel in its smoother modes compute
// (source/dealii/dealii_matrix_free_smoother.cc:63-76 with the operator of tests/laplace_matrix_free.hpp:129-156):
//   x_1 = x_0 - beta_1 D^-1 (A x_0 - b),      x_s = x_{s-1} + alpha_s (x_{s-1} - x_{s-2}) - beta_s D^-1 (A x_{s-1} - b),  s = 2 .. K
// with x_0, b, the coefficients and the ids read ONCE and only x_K (and x_{K-1} when a further term follows) written.
//
// Decomposition.  A workgroup of NW wavefronts owns (64 - 2 halo) columns x (NW TY - 2K + 1) rows x TZ layers and marches
// over the layers of its tile.  Term ("stage") s runs one cell layer behind term s - 1: in super-pass p stage 1 works on
// the cell layer c, stage 2 on c - 1, stage 3 on c - 2; a stage completes the DoF layer with the number of its cell layer
// (the cells below were the previous super-pass, their sums wait in registers).  A DoF of stage s is right only where its
// whole stencil of stage s - 1 was, so the valid region shrinks by one node per stage on every side of the tile: K halo
// lanes, rows and layers on either side are recomputed by the neighbouring tiles (owner computes, no atomics; results do
// not depend on the tiling, bit for bit, and equal those of the one-term kernel: same cell kernel, same order of the
// corner sums, explicit fma, contraction off).
//
// Where the state lives.  Everything a stage reads from the stage before is private to a LANE: its own node column
// (the neighbour column comes by DPP from the next lane), so the planes x_{s-1} of the two node layers a stage reads sit
// in an LDS ring of two slots per stage that only the lane itself writes and reads -- no barrier protects them.
// b, D^-1, the cell coefficient and the momentum term of a DoF ride in registers from the super-pass that loads /
// forms them to the later stages (a renaming: the march runs in trips of K super-passes).  The only exchange between wavefronts is the one the
// one-term kernel has: the sums of a wavefront's first and last cell row go to the neighbours below and above (one
// barrier per stage pass), and BOTH complete the node row they share, with the same operands in the same order, so
// that each keeps the rows of its own cells to itself.
//
// Memory pipeline.  Only stage 1 reads global memory: the x_0 plane two node layers ahead, b and the coefficients
// one layer ahead are requested at the top of a super-pass and land in the ring / the registers at its end -- a whole
// super-pass of arithmetic hides the round trip, so two wavefronts per SIMD suffice (the per-lane state costs ~200
// VGPRs).  Dirichlet DoFs (identity rows: their recurrence involves no other DoF) are finished by stage 1 on the spot and
// read as zero by every stage.
//
// Preconditions (checked on the host; anything else takes the term-by-term kernels): cell-constant layout, ids the
// kernel can compute (AffineIds: lexicographic numbering, Dirichlet DoFs on whole faces), records with >= K halo lanes,
// one rank.
#include "mf_device.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <utility>

namespace mfmg
{
template <typename T>
struct MfFusedArgs
{
  unsigned char const *rec;
  T const *x;  // x_0
  T const *b;
  T *out;      // x_K
  T *out_prev; // x_{K-1} (nullptr: not wanted)
  int Nx, Ny, Nz;
  unsigned int ncols, ntiles_y, ntiles_z;
  int own, halo;
  int TZ; // DoF layers a z-tile owns
  unsigned int rec_bytes;
  int dinv_in_record;
  T fax, fbx, fay, fby, faz, fbz, kd;
  T lam[7]; // the cell matrix in mode space (MODES): lambda of the modes dss, sds, ssd, dds, dsd, sdd, ddd
  T alpha[3], beta[3];
  AffineIds aff;
  unsigned int vec_bytes, rec_total_bytes; // extents of the vectors / of the record array (descriptors; at most 2^32 - 1)
  // narrow last chunk column (<= 32 - halo owned columns): its tiles come last in the tile list and take TWO y-tiles each, one
  // per half of the wavefront (wide_tiles = tiles of the other columns; ntiles_y2 = ceil(ntiles_y / 2); 0: no such tiles)
  unsigned int wide_tiles, ntiles_y2;
};

namespace
{
template <int V>
struct IntTag
{
  static constexpr int value = V;
};

// a run-time number of smoother terms as the template argument K (with_tile_rows, mf_device.hpp)
template <typename F>
void with_terms(int n_terms, F &&f)
{
  if (n_terms == 1)
    f(std::integral_constant<int, 1>());
  else if (n_terms == 2)
    f(std::integral_constant<int, 2>());
  else
    f(std::integral_constant<int, 3>());
}

// The cell kernel in MODE SPACE (one coefficient per cell).  Per direction a Q1 cell acts on (u0, u1) through s = u0 + u1 and
// d = u1 - u0 alone: the 1-D stiffness matrix is diag(0, 1), the mass matrices diag(1/2, 1/6) and f diag(1, 1/3) on (s, d), and the
// result is (A_s - A_d, A_s + A_d).  So the 8 x 8 cell matrix is DIAGONAL on the eight modes (alpha, beta, gamma) in {s, d}^3
// (lambda_sss = 0), and the transforms are butterflies that neighbouring cells share: the x-sums and differences belong to a NODE
// (two operations per node instead of eight per cell), the y-butterfly to a cell row and node layer.  43 FP64 operations per cell
// and 2 per node instead of 76 -- the sweep is bound by exactly these.  Different rounding from cell_apply_cc (same operator to
// 1e-15 per cell): the sweep keeps both, `MODES = false` is the bit-for-bit twin of the one-term kernel.
template <typename T>
struct ModeFactors
{
  T dss, sds, ssd, dds, dsd, sdd, ddd;
};

// cell row q of a stage pass: P / Q = x-sum / x-difference at the node rows q (0) and q + 1 (1) of the lower (l) and upper (u)
// node layer.  Out: what the row contributes to the node row below it (low: the b = 0 corners) and above it (up), as the
// z-modes s (A) and d (B), already summed over the two cells of the row that share a node column.
template <typename T>
__device__ __forceinline__ void cell_row_modes(T Pl0, T Pl1, T Ql0, T Ql1, T Pu0, T Pu1, T Qu0, T Qu1, T cv, ModeFactors<T> const &m,
                                               T &lowA, T &lowB, T &upA, T &upB)
{
#pragma clang fp contract(off)
  // y butterfly (per node layer)
  const T PPl = Pl0 + Pl1, PDl = Pl1 - Pl0, QPl = Ql0 + Ql1, QDl = Ql1 - Ql0;
  const T PPu = Pu0 + Pu1, PDu = Pu1 - Pu0, QPu = Qu0 + Qu1, QDu = Qu1 - Qu0;
  // z butterfly: the seven modes with a non-zero lambda, scaled by lambda and the cell's coefficient
  const T w_ssd = (m.ssd * (PPu - PPl)) * cv;
  const T w_sds = (m.sds * (PDl + PDu)) * cv;
  const T w_sdd = (m.sdd * (PDu - PDl)) * cv;
  const T w_dss = (m.dss * (QPl + QPu)) * cv;
  const T w_dsd = (m.dsd * (QPu - QPl)) * cv;
  const T w_dds = (m.dds * (QDl + QDu)) * cv;
  const T w_ddd = (m.ddd * (QDu - QDl)) * cv;
  // x back: corner a = 0 gets w_s - w_d, a = 1 gets w_s + w_d; the node column = its own cell's a = 0 + the left cell's a = 1
  const T G_ss = from_prev_lane(w_dss) - w_dss;                 // (w_sss = 0)
  const T G_sd = (w_ssd - w_dsd) + from_prev_lane(w_ssd + w_dsd); // (beta, gamma) = (s, d)
  const T G_ds = (w_sds - w_dds) + from_prev_lane(w_sds + w_dds);
  const T G_dd = (w_sdd - w_ddd) + from_prev_lane(w_sdd + w_ddd);
  // y back: node row q (b = 0) gets G_s - G_d, node row q + 1 gets G_s + G_d
  lowA = G_ss - G_ds;
  upA = G_ss + G_ds;
  lowB = G_sd - G_dd;
  upB = G_sd + G_dd;
}

// ring s holds x_s: three slots where a later stage still reads the own value of the layer two below (the momentum term of
// stage s + 2), two for the last one.  carry: the shape keeps that value in registers instead (twelve wavefronts of two rows:
// three slots per ring would take 192 KiB), and every ring is two slots deep.
__host__ __device__ constexpr int ring_depth(int s, int K, bool carry = false) { return (!carry && s <= K - 2) ? 3 : 2; }
__host__ __device__ constexpr int ring_planes(int K, bool carry = false) { return carry ? 2 * K : (K == 1 ? 2 : (K == 2 ? 5 : 8)); }
__host__ __device__ constexpr int ring_base(int s, int K, bool carry = false)
{
  return carry ? 2 * s : (s == 0 ? 0 : (s == 1 ? ring_depth(0, K) : ring_depth(0, K) + ring_depth(1, K)));
}

// Global memory through buffer descriptors: a request is "descriptor (4 SGPRs, built once per array from the kernel
// arguments) + uniform 32-bit byte offset (an SGPR: row and layer) + per-lane 32-bit byte offset (one VGPR, loop invariant)".
// No 64-bit per-lane addresses: the loop optimiser otherwise keeps a 64-bit pointer per request stream in VGPRs.
template <typename T>
struct BufIO;
template <>
struct BufIO<double>
{
  typedef unsigned int v2u __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ double ld(__amdgpu_buffer_rsrc_t r, unsigned int voff, unsigned int soff)
  {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
  }
  static __device__ __forceinline__ void st(double v, __amdgpu_buffer_rsrc_t r, unsigned int voff, unsigned int soff)
  {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), r, voff, soff, 0);
  }
};
template <>
struct BufIO<float>
{
  static __device__ __forceinline__ float ld(__amdgpu_buffer_rsrc_t r, unsigned int voff, unsigned int soff)
  {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
  }
  static __device__ __forceinline__ void st(float v, __amdgpu_buffer_rsrc_t r, unsigned int voff, unsigned int soff)
  {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v), r, voff, soff, 0);
  }
};

// DBG (timing experiments only, wrong results): 1 = no barrier, 2 = no division, 3 = no global stores
// NARROW: the tile of a narrow last chunk column.  Lanes 0-31 work on y-tile 2 t, lanes 32-63 on y-tile 2 t + 1 of the same
// 32 columns: everything that depends on the y-tile (row numbers, row masks, the row part of an address) is per lane instead of
// per wavefront; the halves exchange nothing (lane 0 of a half is a halo lane; its last lane is at most the last column of the mesh,
// whose cell is a phantom with coefficient zero: what arrives there from the other half is multiplied by it), owner computes as
// everywhere.
// ZERO0: x_0 = 0 (the pre-smoother of a preconditioner application, hierarchy.hpp:253-259): stage 1 is x_1 = beta_1 D^-1 b -- no
// operator application, nothing read of x_0, no exchange between the wavefronts; the same bits as the sweep run on a zeroed vector.
// NWC: the number of wavefronts where the kernel fixes it (0: that of the launch).  Such a kernel also CARRIES the momentum
// operand: x_{S-2} of a DoF is the x_{S-1} that stage S - 1 read of it one super-pass earlier, kept in registers from there
// (xn at the stage that reads it, xq one super-pass later: a renaming like that of bq and dq) instead of in a third slot of
// its ring.  The x_0 layer requested two ahead then lands over the slot of layer c1, which stage 1 has read by the end of the
// super-pass.
// DVEC: D^-1 is read from a vector of its own (dinv_vec: the operator's sweep_diagonal_inverse, by DoF id like b; an argument of
// the kernel beside MfFusedArgs, whose layout the other kernels keep), requested like b one layer ahead, instead of derived from
// the coefficient sums (!DREC) or read from the records (DREC): the bits of the derived form without its divisions, pair sums and
// carried sums.  Dirichlet DoFs take D^-1 = 1 as the derived form does.
template <typename T, int K, int TY, bool DREC, bool MODES, int DBG = 0, bool NARROW = false, bool ZERO0 = false, int NWC = 0, bool DVEC = false>
__device__ __forceinline__ void mf_cheb_fused_body(MfFusedArgs<T> const &a, unsigned int w, T const *dinv_vec = nullptr)
{
#pragma clang fp contract(off)
  static_assert(!(DREC && DVEC), "one source of D^-1");
  static_assert(!DVEC || NWC > 0, "the D^-1 vector is an argument of the twelve-wavefront kernels");
  constexpr int R = TY + 1; // node rows of a wavefront
  constexpr bool DERIVE = !DREC && !DVEC; // D^-1 from the coefficient sums, formed by stage 1
  constexpr bool CARRY = NWC > 0;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int NW = NWC > 0 ? NWC : blockDim.x >> 6;
  // LDS: per wavefront the rings x_0 .. x_{K-1} ([planes][R rows][64 lanes]); then the exports [2][NW][4][64]
  T *ring = reinterpret_cast<T *>(smem_raw) + (size_t)wv * (ring_planes(K, CARRY) * R * 64) + lane;
  // the same planes as the NEXT lane sees them (the last lane: its own, what a DPP shift with the source as old value returns): the
  // x_{s-1} values of the neighbour column are read from the ring, not shifted through the vector ALU, which bounds the sweep
  T const *ring_next = ring + (lane == 63 ? 0 : 1);
  T *xport = reinterpret_cast<T *>(smem_raw) + (size_t)NW * (ring_planes(K, CARRY) * R * 64) + lane;

  // (tile w of the list: the kernel has dealt the list to the XCDs in contiguous runs)
  const int wcols = a.ntiles_y2 > 0 ? (int)a.ncols - 1 : (int)a.ncols; // chunk columns with tiles of their own width
  int tc, tyi, tzi, lx = lane;
  if constexpr (NARROW)
  {
    const unsigned int v = w - a.wide_tiles;
    tc = (int)a.ncols - 1;
    tyi = 2 * (int)(v % a.ntiles_y2) + (lane >> 5); // (per lane)
    tzi = (int)(v / a.ntiles_y2);
    lx = lane & 31;
  }
  else
  {
    tc = (int)(w % (unsigned int)wcols);
    tyi = (int)((w / (unsigned int)wcols) % a.ntiles_y);
    tzi = (int)(w / ((unsigned int)wcols * a.ntiles_y));
  }
  const bool tile_live = !NARROW || tyi < (int)a.ntiles_y; // (an odd number of y-tiles leaves the second half of the last pair idle)

  const int ci = tc * a.own - a.halo + lx; // node / cell column of this lane
  const bool lane_in = ci >= 0 && ci < a.Nx;
  const bool lane_face = ((a.aff.faces & 1) && ci == 0) || ((a.aff.faces & 2) && ci == a.Nx - 1);
  const bool lane_free = lane_in && !lane_face;
  const bool col_owned = tile_live && lx >= a.halo && lx < a.halo + a.own && ci < a.Nx - a.aff.ghost_hi[0] && ci >= a.aff.ghost_lo[0]; // (ghost DoFs: computed, never written)
  const int RY = NW * TY - 2 * K + 1;    // DoF rows a tile owns
  const int Yw = tyi * RY - K + wv * TY; // first node row of this wavefront: node rows Yw .. Yw + TY, cell rows Yw .. Yw + TY - 1
  const int own_y0 = tyi * RY, own_y1 = min(own_y0 + RY, a.Ny);
  const int Z0 = tzi * a.TZ, Z1 = min(Z0 + a.TZ, a.Nz);
  // per-lane part of an address: a 32-bit byte offset from a uniform base (lanes outside the mesh load at a clamped column;
  // what they load is never used)
  const unsigned int off_lane = (unsigned int)(a.aff.base + min(max(ci, 0), a.Nx - 1) * a.aff.s0) * (unsigned int)sizeof(T);
  const unsigned int rec_lane = (unsigned int)lx * (unsigned int)sizeof(T);

  // Arguments that only the epilogues and the requests need (alpha, beta, kd, the vector bases) are re-read from the kernel
  // argument segment where they are used (scalar loads through a pointer the compiler cannot see through): held in scalar
  // registers for the whole pass they pushed ~90 other scalars into VGPR lanes (a v_readlane / v_writelane per use).
  typedef const __attribute__((address_space(4))) char *karg_ptr_t;
  auto karg_T = [&](size_t off) -> T {
    karg_ptr_t p = (karg_ptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *reinterpret_cast<const __attribute__((address_space(4))) T *>(p + off);
  };
  auto karg_ptr = [&](size_t off) -> void * {
    karg_ptr_t p = (karg_ptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *reinterpret_cast<void *const __attribute__((address_space(4))) *>(p + off);
  };
  // CARRY (the twelve-wavefront kernels): read ONCE per tile instead and held as uniform values in vector registers, which
  // these kernels have to spare and the scalar file has not -- a scalar load per use is a round trip to the scalar cache that
  // the wavefront waits for with lgkmcnt(0), its LDS reads drained along with it.  The same operands in the same expressions.
  // How many of the six: all in the wide body of the mode-space kernels (161 VGPRs of 168); beta_1 .. beta_3 in the narrow body, which
  // has room for three pairs (167) -- the others stay scalar there, as all do in the reference arithmetic (163 VGPRs without them)
  // (D^-1 from its vector: ten VGPRs of carried sums are gone, kd is not used, and the narrow body holds the other five as well)
  constexpr int kHoldInVgpr = !MODES ? 0 : ((NARROW && !DVEC) ? 3 : 2 * K);
  T held_alpha[K], held_beta[K], held_kd = T(0);
  if constexpr (CARRY)
  {
    auto hold = [](T v, int rank) {
      if (rank < kHoldInVgpr)
        asm volatile("" : "+v"(v));
      return v;
    };
#pragma unroll
    for (int s = 0; s < K; ++s)
    {
      held_alpha[s] = s > 0 ? hold(a.alpha[s], K + s) : T(0);
      held_beta[s] = hold(a.beta[s], s);
    }
    held_kd = hold(a.kd, K);
  }
  // CARRY: a wave-uniform number as the march sees it anew at a use.  A condition on a tile constant (this wavefront has a
  // neighbour below, the row lies in the mesh, x_{K-1} is wanted) that the compiler can see through is formed before the march and
  // held as a lane mask, two scalar registers each, most of them in spill lanes; formed where it is used it is one comparison.
  auto fresh = [](int v) {
    if constexpr (CARRY)
    {
      v = __builtin_amdgcn_readfirstlane(v);
      asm volatile("" : "+s"(v));
    }
    return v;
  };
  auto k_alpha = [&](int s) {
    if constexpr (CARRY)
      return held_alpha[s];
    else
      return karg_T(offsetof(MfFusedArgs<T>, alpha) + (size_t)s * sizeof(T));
  };
  auto k_beta = [&](int s) {
    if constexpr (CARRY)
      return held_beta[s];
    else
      return karg_T(offsetof(MfFusedArgs<T>, beta) + (size_t)s * sizeof(T));
  };
  auto k_kd = [&]() {
    if constexpr (CARRY)
      return held_kd;
    else
      return karg_T(offsetof(MfFusedArgs<T>, kd));
  };

  CellFactors<T> fac;
  fac.fx = fac.fy = fac.fz = T(0);
  fac.fax = a.fax;
  fac.fbx = a.fbx;
  fac.fay = a.fay;
  fac.fby = a.fby;
  fac.faz = a.faz;
  fac.fbz = a.fbz;
  ModeFactors<T> mf;
  mf.dss = a.lam[0];
  mf.sds = a.lam[1];
  mf.ssd = a.lam[2];
  mf.dds = a.lam[3];
  mf.dsd = a.lam[4];
  mf.sdd = a.lam[5];
  mf.ddd = a.lam[6];

  // wave-uniform description of the node rows, one bit per row
  unsigned int rows_free = 0, rows_own = 0;
#pragma unroll
  for (int r = 0; r < R; ++r)
  {
    const int j = Yw + r;
    const bool real = j >= 0 && j < a.Ny;
    if (real && !(((a.aff.faces & 4) && j == 0) || ((a.aff.faces & 8) && j == a.Ny - 1)))
      rows_free |= 1u << r;
    if (r < TY && j >= own_y0 && j < own_y1 && j >= a.aff.ghost_lo[1] && j < a.Ny - a.aff.ghost_hi[1]) // (the node row two wavefronts share is stored by the upper one)
      rows_own |= 1u << r;
  }
  // the lane x row part of "the DoF is free" / "this lane stores the DoF".  CARRY: formed once per tile, one lane mask per row,
  // instead of recombined from the lane mask and the row bit at every use (each scalar factor is a mask of its own there)
  bool row_free_lane[R], row_own_lane[R];
  if constexpr (CARRY)
  {
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
      row_free_lane[r] = lane_free && ((rows_free >> r) & 1u);
      row_own_lane[r] = col_owned && ((rows_own >> r) & 1u);
    }
  }
  auto free_lane_row = [&](int r) -> bool {
    if constexpr (CARRY)
      return row_free_lane[r];
    else
      return lane_free && ((rows_free >> r) & 1u);
  };
  auto own_lane_row = [&](int r) -> bool {
    if constexpr (CARRY)
      return row_own_lane[r];
    else
      return col_owned && ((rows_own >> r) & 1u);
  };
  // descriptors and uniform byte offsets: node row r / node layer n of a vector (clamped into the mesh), cell row q / layer n
  // of this chunk column's records
  // (CARRY: from the pointers as the kernel received them -- a descriptor is a held pointer plus two constant words, no scalar
  // load per request or store)
  // DVEC: one of the five base addresses (0 .. 4: x, b, out, out_prev, the records) is held in a vector register pair and made
  // uniform where a descriptor is built from it (two v_readfirstlane), like the address of the D^-1 vector below: the scalar
  // file is what these kernels run out of, and with it their sgpr_spill_count stays at or under that of the kernels that derive
  // D^-1.  Which one: the address used least -- x_{K-1}; from a zero guess that of the records, where out_prev left 29 spills
  // against the 25 of the twin (profiles/r11_a_sweep_isa.txt has the counts of the choices tried).  One pair is what the
  // vector registers have room for beside the twin's count.
  constexpr int kHeldBase = !DVEC ? 0 : (ZERO0 ? 16 : 8);
  unsigned long long hp[5] = {0, 0, 0, 0, 0};
  if constexpr (DVEC)
  {
    const unsigned long long base[5] = {(unsigned long long)a.x, (unsigned long long)a.b, (unsigned long long)a.out, (unsigned long long)a.out_prev, (unsigned long long)a.rec};
#pragma unroll
    for (int i = 0; i < 5; ++i)
      if ((kHeldBase >> i) & 1)
      {
        hp[i] = base[i];
        asm volatile("" : "+v"(hp[i]));
      }
  }
  auto hp_get = [&](int i) -> void * {
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)hp[i]), hi = __builtin_amdgcn_readfirstlane((unsigned int)(hp[i] >> 32));
    return reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo);
  };
  auto vec_ptr = [&](size_t off) -> void * {
    if constexpr (CARRY)
    {
      const int i = off == offsetof(MfFusedArgs<T>, x) ? 0 : (off == offsetof(MfFusedArgs<T>, b) ? 1 : (off == offsetof(MfFusedArgs<T>, out) ? 2 : 3));
      if ((kHeldBase >> i) & 1)
        return hp_get(i);
      return const_cast<T *>(off == offsetof(MfFusedArgs<T>, x) ? a.x : (off == offsetof(MfFusedArgs<T>, b) ? a.b : (off == offsetof(MfFusedArgs<T>, out) ? a.out : a.out_prev)));
    }
    else
      return karg_ptr(off);
  };
  auto rec_ptr = [&]() -> void * {
    if constexpr (CARRY)
    {
      if ((kHeldBase >> 4) & 1)
        return hp_get(4);
      return const_cast<unsigned char *>(a.rec);
    }
    else
      return karg_ptr(offsetof(MfFusedArgs<T>, rec));
  };
  auto rs_vec = [&](size_t off) { return __builtin_amdgcn_make_buffer_rsrc(vec_ptr(off), 0, a.vec_bytes, 0x00020000); };
  auto rs_rec_f = [&]() { return __builtin_amdgcn_make_buffer_rsrc(rec_ptr(), 0, a.rec_total_bytes, 0x00020000); };
  // (the address of the D^-1 vector is held in a vector register pair and made uniform where its descriptor is built, once per
  // super-pass: as a sixth pointer in scalar registers it pushed some twenty moves to and from spill lanes into the march of
  // either body)
  unsigned long long dinv_addr = (unsigned long long)dinv_vec;
  if constexpr (DVEC)
    asm volatile("" : "+v"(dinv_addr));
  auto rs_dinv_f = [&]() {
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)dinv_addr), hi = __builtin_amdgcn_readfirstlane((unsigned int)(dinv_addr >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo), 0, a.vec_bytes, 0x00020000);
  };
  const bool want_prev_tile = a.out_prev != nullptr;
  int want_prev_i = 0;
  if constexpr (CARRY)
    want_prev_i = want_prev_tile ? 1 : 0;
  auto want_prev_f = [&]() -> bool {
    if constexpr (CARRY)
      return fresh(want_prev_i) != 0;
    else
      return want_prev_tile;
  };
  const unsigned int row_stride = (unsigned int)a.aff.s1 * (unsigned int)sizeof(T), layer_stride = (unsigned int)a.aff.s2 * (unsigned int)sizeof(T);
  const unsigned int rec_row = a.ncols * a.rec_bytes;
  const unsigned int rec_layer = (unsigned int)a.Ny * rec_row;
  const unsigned int rec_col = (unsigned int)tc * a.rec_bytes;
  // (CARRY: the same sets of layers as two ranges formed once per tile)
  int zfree0 = 0, zfree1 = 0, zown0 = 0, zown1 = 0;
  if constexpr (CARRY)
  {
    zfree0 = (a.aff.faces & 16) ? 1 : 0;
    zfree1 = (a.aff.faces & 32) ? a.Nz - 1 : a.Nz;
    zown0 = max(Z0, a.aff.ghost_lo[2]);
    zown1 = min(Z1, a.Nz - a.aff.ghost_hi[2]);
  }
  auto layer_free = [&](int n) {
    if constexpr (CARRY)
      return n >= zfree0 && n < zfree1;
    else
      return n >= 0 && n < a.Nz && !(((a.aff.faces & 16) && n == 0) || ((a.aff.faces & 32) && n == a.Nz - 1));
  };
  auto layer_own = [&](int n) {
    if constexpr (CARRY)
      return n >= zown0 && n < zown1;
    else
      return n >= Z0 && n < Z1 && n >= a.aff.ghost_lo[2] && n < a.Nz - a.aff.ghost_hi[2];
  };
  // an address = per-lane part + wave-uniform part: the row belongs to the uniform part, except in a NARROW tile, whose halves
  // work on different rows
  struct Off
  {
    unsigned int v, s;
  };
  auto vec_off = [&](int r, int n) -> Off {
    const unsigned int rowb = (unsigned int)min(max(Yw + r, 0), a.Ny - 1) * row_stride, layb = (unsigned int)min(max(n, 0), a.Nz - 1) * layer_stride;
    if constexpr (NARROW)
      return Off{off_lane + rowb, layb};
    else
      return Off{off_lane, rowb + layb};
  };
  auto rec_off = [&](int q, int n, unsigned int field) -> Off {
    const unsigned int rowb = (unsigned int)min(max(Yw + q, 0), a.Ny - 1) * rec_row, layb = rec_col + (unsigned int)min(max(n, 0), a.Nz - 1) * rec_layer + field;
    if constexpr (NARROW)
      return Off{rec_lane + rowb, layb};
    else
      return Off{rec_lane, rowb + layb};
  };
  auto ld_vec = [&](__amdgpu_buffer_rsrc_t rs, int r, int n) -> T {
    const Off o = vec_off(r, n);
    return BufIO<T>::ld(rs, o.v, o.s);
  };
  auto st_vec = [&](T v, __amdgpu_buffer_rsrc_t rs, int r, int n) {
    const Off o = vec_off(r, n);
    BufIO<T>::st(v, rs, o.v, o.s);
  };
  auto ld_coef = [&](__amdgpu_buffer_rsrc_t rs_rec, int q, int n) -> T {
    const Off o = rec_off(q, n, (unsigned int)Rec<T, true>::kCoefOff);
    return BufIO<T>::ld(rs_rec, o.v, o.s);
  };
  auto ld_dinv = [&](__amdgpu_buffer_rsrc_t rs_rec, int r, int n) -> T {
    const Off o = rec_off(r, n, (unsigned int)Rec<T, true>::kDinvOff);
    return BufIO<T>::ld(rs_rec, o.v, o.s);
  };
  // ring slot sl of ring s, node row r: the slot of node layer n is (n - cb) mod the depth of the ring; the march hands a stage
  // pass its slots as constants of the position in its trip (march below)
  auto ring_at = [&](int s, int sl, int r) -> T * { return ring + ((ring_base(s, K, CARRY) + sl) * R + r) * 64; };
  auto ring_next_at = [&](int s, int sl, int r) -> T const * { return ring_next + ((ring_base(s, K, CARRY) + sl) * R + r) * 64; };

  // ---- per-lane state carried from super-pass to super-pass (stage s + 1 uses entry s)
  T bq[K][R];  // b of the DoF (row r, layer of the stage)
  T dq[K][R];  // D^-1 likewise (entry 0 written by stage 1 / loaded from the records or the D^-1 vector)
  T cq[K][TY]; // coefficient of the cell (row q, cell layer of the stage)
  T pt[K][R];  // z-carry of the partial sums
  T pcs[R];    // z-carry of the coefficient sums (D^-1 on the fly)
  T xn[K][R];  // CARRY: x_s of the DoF as stage s + 1 reads it in this super-pass (entry s)
  T xq[K][R];  // CARRY: the same of the super-pass before: the momentum operand of stage s + 2
  T clo = T(0), chi = T(0); // coefficients of the cell rows below / above the wavefront's own, stage-1 layer (D^-1 of the shared rows)
#pragma unroll
  for (int s = 0; s < K; ++s)
  {
#pragma unroll
    for (int r = 0; r < R; ++r)
      bq[s][r] = dq[s][r] = pt[s][r] = xn[s][r] = xq[s][r] = T(0);
#pragma unroll
    for (int q = 0; q < TY; ++q)
      cq[s][q] = T(0);
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    pcs[r] = T(0);

  // stage s works on the cell layers start(s) .. end(s)
  auto stage_start = [&](int s) { return max(Z0 - K + (s - 1), 0); };
  auto stage_end = [&](int s) { return min(Z1 - 1 + (K - s), a.Nz - 1); };
  const int cb = stage_start(1);

  // ---- prologue: the two x_0 layers, b (D^-1) and the coefficients of the first super-pass
  {
    const __amdgpu_buffer_rsrc_t rs_x = rs_vec(offsetof(MfFusedArgs<T>, x)), rs_b = rs_vec(offsetof(MfFusedArgs<T>, b)), rs_rec = rs_rec_f();
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
      if constexpr (!ZERO0)
      {
        *ring_at(0, 0, r) = ld_vec(rs_x, r, cb);
        *ring_at(0, 1, r) = ld_vec(rs_x, r, cb + 1);
      }
      bq[0][r] = ld_vec(rs_b, r, cb);
      if constexpr (DREC)
        dq[0][r] = ld_dinv(rs_rec, r, cb);
      if constexpr (DVEC)
        dq[0][r] = ld_vec(rs_dinv_f(), r, cb);
    }
#pragma unroll
    for (int q = 0; q < TY; ++q)
    {
      const T cv = ld_coef(rs_rec, q, cb);
      cq[0][q] = (Yw + q >= 0) ? cv : T(0);
    }
    if constexpr (DERIVE)
    {
      const T l = ld_coef(rs_rec, -1, cb);
      const T h = ld_coef(rs_rec, TY, cb);
      clo = (Yw - 1 >= 0) ? l : T(0);
      chi = (Yw + TY >= 0) ? h : T(0);
    }
  }

  unsigned int ex = 0; // stage passes so far (parity of the export buffers)

  // ---- one stage pass: stage S (1-based) on the cell layer c; sl(s, d) = the slot of node layer c + d in ring s
  auto stage_pass = [&](auto tag, int c, auto sl) {
    constexpr int S = decltype(tag)::value;
    const bool lo_free = layer_free(c), hi_free = layer_free(c + 1);
    const bool l_own = layer_own(c);
    T xl[R], xu[R], xown[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
      if constexpr (S == 1 && ZERO0)
      {
        xown[r] = xl[r] = xu[r] = T(0);
        continue;
      }
      const T l = *ring_at(S - 1, sl(S - 1, 0), r), u = *ring_at(S - 1, sl(S - 1, 1), r);
      xown[r] = l;
      if constexpr (CARRY && S < K)
        xn[S - 1][r] = l;
      if constexpr (S == 1)
      {
        // x_0 sits in the ring as it was read; Dirichlet and out-of-mesh values enter the cells as zero
        if constexpr (CARRY)
        {
          const bool lrf = free_lane_row(r);
          xl[r] = (lrf && lo_free) ? l : T(0);
          xu[r] = (lrf && hi_free) ? u : T(0);
        }
        else
        {
          const bool rf = (rows_free >> r) & 1u;
          xl[r] = (lane_free && rf && lo_free) ? l : T(0);
          xu[r] = (lane_free && rf && hi_free) ? u : T(0);
        }
      }
      else
      {
        xl[r] = l;
        xu[r] = u;
      }
    }
    T xln[R], xun[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
      if constexpr (S == 1)
      {
        // (x_0 sits in its ring unmasked: the masked values are shifted)
        xln[r] = from_next_lane(xl[r]);
        xun[r] = from_next_lane(xu[r]);
      }
      else
      {
        // x_{S-1} sits in its ring as the cells read it: the neighbour column straight from there (an LDS read instead of two
        // DPP moves and their presets per value; the same numbers)
        xln[r] = *ring_next_at(S - 1, sl(S - 1, 0), r);
        xun[r] = *ring_next_at(S - 1, sl(S - 1, 1), r);
      }
    }
    // per cell row: what it contributes to the node row below (low) and above (up), two values each -- the corner sums of the
    // d = 0 / d = 1 node layer (reference arithmetic) or the z-modes s / d (MODES)
    T lowA[TY], lowB[TY], upA[TY], upB[TY], sx[TY];
    if constexpr (S == 1 && ZERO0)
    {
      // A 0 = 0: no cell arithmetic; the coefficient sums of the diagonal remain
#pragma unroll
      for (int q = 0; q < TY; ++q)
      {
        lowA[q] = lowB[q] = upA[q] = upB[q] = sx[q] = T(0);
        if constexpr (DERIVE)
        {
          const T cv = cq[0][q];
          sx[q] = cv + from_prev_lane(cv);
        }
      }
    }
    else if constexpr (MODES)
    {
      T Pl[R], Ql[R], Pu[R], Qu[R];
#pragma unroll
      for (int r = 0; r < R; ++r)
      {
        Pl[r] = xl[r] + xln[r];
        Ql[r] = xln[r] - xl[r];
        Pu[r] = xu[r] + xun[r];
        Qu[r] = xun[r] - xu[r];
      }
#pragma unroll
      for (int q = 0; q < TY; ++q)
      {
        const T cv = cq[S - 1][q];
        cell_row_modes<T>(Pl[q], Pl[q + 1], Ql[q], Ql[q + 1], Pu[q], Pu[q + 1], Qu[q], Qu[q + 1], cv, mf, lowA[q], lowB[q], upA[q], upB[q]);
        sx[q] = T(0);
        if constexpr (S == 1 && DERIVE)
          sx[q] = cv + from_prev_lane(cv);
      }
    }
    else
    {
#pragma unroll
      for (int q = 0; q < TY; ++q)
      {
        T u[8], v[8];
        u[0] = xl[q];
        u[1] = xln[q];
        u[2] = xl[q + 1];
        u[3] = xln[q + 1];
        u[4] = xu[q];
        u[5] = xun[q];
        u[6] = xu[q + 1];
        u[7] = xun[q + 1];
        const T cv = cq[S - 1][q];
        cell_apply_cc<T>(u, cv, fac, v);
        // x combine: DoF column ci gets the a=0 corners of its own cell and the a=1 corners of the cell of the lane to the left
        lowA[q] = v[0] + from_prev_lane(v[1]);
        upA[q] = v[2] + from_prev_lane(v[3]);
        lowB[q] = v[4] + from_prev_lane(v[5]);
        upB[q] = v[6] + from_prev_lane(v[7]);
        sx[q] = T(0);
        if constexpr (S == 1 && DERIVE)
          sx[q] = cv + from_prev_lane(cv);
      }
    }
    // the sums of the last cell row go up, those of the first go down (double-buffered by the parity of the pass)
    constexpr bool kExchange = !(S == 1 && ZERO0); // (all sums are zero: nothing to hand over, no barrier)
    if constexpr (kExchange)
    {
      T *xp = xport + (size_t)((ex & 1) * NW + wv) * 4 * 64;
      xp[0] = upA[TY - 1];
      xp[64] = upB[TY - 1];
      xp[128] = lowA[0];
      xp[192] = lowB[0];
    }
    // a node row is complete: A, B = its two sums over the cell rows below and above; the value of the DoF layer c and the carry
    // for the layer above (reference: A belongs to layer c, B to c + 1; MODES: the z butterfly back)
    auto z_combine = [&](T A, T B, T &carry) -> T {
      if constexpr (MODES)
      {
        const T yv = (A - B) + carry;
        carry = A + B;
        return yv;
      }
      else
      {
        const T yv = A + carry;
        carry = B;
        return yv;
      }
    };
    // one DoF (row r, layer c) of this stage is complete: yv = (A x_{S-1}) there
    auto finish = [&](auto rtag, T yv, T tcs) {
      constexpr int r = decltype(rtag)::value;
      bool fr, st;
      if constexpr (CARRY)
      {
        fr = free_lane_row(r) && lo_free;
        st = own_lane_row(r) && l_own;
      }
      else
      {
        fr = lane_free && ((rows_free >> r) & 1u) && lo_free;
        st = col_owned && ((rows_own >> r) & 1u) && l_own;
      }
      if constexpr (S == 1)
      {
        T d;
        if constexpr (DERIVE)
        {
          // the eight cells of the DoF: two rows of this layer + the same of the layer below (carried)
          const T sum8 = tcs + pcs[r];
          pcs[r] = tcs;
          d = DBG == 2 ? k_kd() * sum8 : T(1) / (k_kd() * sum8);
          dq[0][r] = d;
        }
        else
          d = dq[0][r];
        const T x0 = xown[r], lb = bq[0][r];
        const T x1 = fmadd<T>(-(k_beta(0) * d), yv - lb, x0);
        if constexpr (K == 1)
        {
          if (st && fr)
            st_vec(x1, rs_vec(offsetof(MfFusedArgs<T>, out)), r, c);
        }
        else
        {
          *ring_at(1, sl(1, 0), r) = fr ? x1 : T(0);
          if constexpr (K == 2)
            if (st && fr && want_prev_f())
              st_vec(x1, rs_vec(offsetof(MfFusedArgs<T>, out_prev)), r, c);
        }
        // Dirichlet DoFs: identity rows with D^-1 = 1 (the stored diagonal says so too) -- the whole recurrence here
        if (st && !fr)
        {
          const T dc = DREC ? d : T(1);
          T xa = x0, xb = fmadd<T>(-(k_beta(0) * dc), x0 - lb, x0); // x_{s-1}, x_s
#pragma unroll
          for (int s = 1; s < K; ++s)
          {
            const T xn = fmadd<T>(-(k_beta(s) * dc), xb - lb, fmadd<T>(k_alpha(s), xb - xa, xb));
            xa = xb;
            xb = xn;
          }
          st_vec(xb, rs_vec(offsetof(MfFusedArgs<T>, out)), r, c);
          if (K > 1 && want_prev_f())
            st_vec(xa, rs_vec(offsetof(MfFusedArgs<T>, out_prev)), r, c);
        }
      }
      else
      {
        // x_{S-1} and x_{S-2} of the DoF (zero where it is not free: the result is dropped there)
        const T xo = xown[r];
        T xoo = T(0);
        if constexpr (CARRY)
          xoo = xq[S - 2][r]; // (zero from a zero guess)
        else if constexpr (!(S == 2 && ZERO0))
          xoo = *ring_at(S - 2, sl(S - 2, 0), r);
        T xoo_m; // (x_0 sits in its ring unmasked)
        if constexpr (CARRY)
          xoo_m = (S == 2) ? ((free_lane_row(r) && lo_free) ? xoo : T(0)) : xoo;
        else
          xoo_m = (S == 2) ? ((lane_free && ((rows_free >> r) & 1u) && lo_free) ? xoo : T(0)) : xoo;
        const T xs = fmadd<T>(-(k_beta(S - 1) * dq[S - 1][r]), yv - bq[S - 1][r], fmadd<T>(k_alpha(S - 1), xo - xoo_m, xo));
        if constexpr (S < K)
        {
          *ring_at(S, sl(S, 0), r) = fr ? xs : T(0);
          if constexpr (S == K - 1)
            if (st && fr && want_prev_f())
              st_vec(xs, rs_vec(offsetof(MfFusedArgs<T>, out_prev)), r, c);
        }
        else
        {
          if (st && fr)
            st_vec(xs, rs_vec(offsetof(MfFusedArgs<T>, out)), r, c);
        }
      }
    };
    // the rows between the wavefront's own cells
    auto inner = [&](auto rtag) {
      constexpr int r = decltype(rtag)::value;
      const T t0 = lowA[r] + upA[r - 1];
      const T t1 = lowB[r] + upB[r - 1];
      const T yv = z_combine(t0, t1, pt[S - 1][r]);
      finish(rtag, yv, sx[r] + sx[r - 1]);
    };
    if constexpr (TY >= 2)
      inner(IntTag<1>{});
    if constexpr (TY >= 3)
      inner(IntTag<2>{});
    if constexpr (TY >= 4)
      inner(IntTag<3>{});
    // (LDS only: the requests of the next super-pass stay in flight across the barrier -- __syncthreads() would drain them.
    // Tried instead: a word per wavefront that its two neighbours poll, no workgroup-wide rendezvous -- 7 % slower.)
    if constexpr (DBG != 1 && kExchange)
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // the rows shared with the neighbours: both wavefronts complete them, with the same operands in the same order
    {
      T lo0 = T(0), lo1 = T(0), hi0 = T(0), hi1 = T(0);
      const int wvu = fresh(wv);
      if (kExchange && wvu > 0)
      {
        T const *ip = xport + (size_t)((ex & 1) * NW + wvu - 1) * 4 * 64;
        lo0 = ip[0];
        lo1 = ip[64];
      }
      if (kExchange && wvu + 1 < NW)
      {
        T const *ip = xport + (size_t)((ex & 1) * NW + wvu + 1) * 4 * 64;
        hi0 = ip[128];
        hi1 = ip[192];
      }
      {
        const T t0 = lowA[0] + lo0;
        const T t1 = lowB[0] + lo1;
        const T yv = z_combine(t0, t1, pt[S - 1][0]);
        T tcs = T(0);
        if constexpr (S == 1 && DERIVE)
          tcs = sx[0] + (clo + from_prev_lane(clo));
        finish(IntTag<0>{}, yv, tcs);
      }
      {
        const T t0 = hi0 + upA[TY - 1];
        const T t1 = hi1 + upB[TY - 1];
        const T yv = z_combine(t0, t1, pt[S - 1][TY]);
        T tcs = T(0);
        if constexpr (S == 1 && DERIVE)
          tcs = (chi + from_prev_lane(chi)) + sx[TY - 1];
        finish(IntTag<TY>{}, yv, tcs);
      }
    }
    if constexpr (kExchange)
      ++ex;
  };

  // ---- the march.  Super-pass c1: stage s on the cell layer c1 - (s - 1), active from first(s) = stage_start(s) + s - 1 to
  // last(s) = stage_end(s) + s - 1 (both grow with s).  sl(s, k) = the slot of node layer c1 + k in ring s.
  auto super_pass = [&](int c1, auto sl) {
    // requests for the next super-pass: x_0 two node layers ahead, b (D^-1) and the coefficients one
    T pfx[R], pfb[R], pfd[R], pfc[TY], pflo = T(0), pfhi = T(0);
    const __amdgpu_buffer_rsrc_t rs_x = rs_vec(offsetof(MfFusedArgs<T>, x)), rs_b = rs_vec(offsetof(MfFusedArgs<T>, b)), rs_rec = rs_rec_f();
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
      pfx[r] = T(0);
      if constexpr (!ZERO0)
        pfx[r] = ld_vec(rs_x, r, c1 + 2);
      pfb[r] = ld_vec(rs_b, r, c1 + 1);
      pfd[r] = T(0);
      if constexpr (DREC)
        pfd[r] = ld_dinv(rs_rec, r, c1 + 1);
      if constexpr (DVEC)
        pfd[r] = ld_vec(rs_dinv_f(), r, c1 + 1);
    }
#pragma unroll
    for (int q = 0; q < TY; ++q)
      pfc[q] = ld_coef(rs_rec, q, c1 + 1);
    if constexpr (DERIVE)
    {
      pflo = ld_coef(rs_rec, -1, c1 + 1);
      pfhi = ld_coef(rs_rec, TY, c1 + 1);
    }

    // CARRY (three terms): the same conditions from Z0 and Nz alone -- c1 <= c_last = min(Z1 + 1, Nz + 1) in the march, which is
    // the upper bound of stage 3 and the Z1 part of the other two
    static_assert(!CARRY || K == 3, "the stage ranges of the twelve-wavefront kernels are those of three terms");
    if (CARRY ? c1 < a.Nz : c1 <= stage_end(1))
      stage_pass(IntTag<1>{}, c1, [&](int s, int d) { return sl(s, d); });
    if constexpr (K >= 2)
      if (CARRY ? (c1 >= max(Z0 - 1, 1) && c1 <= a.Nz) : (c1 - 1 >= stage_start(2) && c1 - 1 <= stage_end(2)))
        stage_pass(IntTag<2>{}, c1 - 1, [&](int s, int d) { return sl(s, d - 1); });
    if constexpr (K >= 3)
      if (CARRY ? c1 >= max(Z0 + 1, 2) : (c1 - 2 >= stage_start(3) && c1 - 2 <= stage_end(3)))
        stage_pass(IntTag<3>{}, c1 - 2, [&](int s, int d) { return sl(s, d - 2); });

    // shift the carried state by one stage (a renaming: the trip of the march is K super-passes), land the requests
#pragma unroll
    for (int s = K - 1; s >= 1; --s)
    {
#pragma unroll
      for (int r = 0; r < R; ++r)
      {
        bq[s][r] = bq[s - 1][r];
        dq[s][r] = dq[s - 1][r];
      }
#pragma unroll
      for (int q = 0; q < TY; ++q)
        cq[s][q] = cq[s - 1][q];
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
      bq[0][r] = pfb[r];
      if constexpr (CARRY)
      {
#pragma unroll
        for (int s = 0; s + 2 <= K; ++s)
          xq[s][r] = xn[s][r];
      }
      if constexpr (DREC || DVEC)
        dq[0][r] = pfd[r];
      if constexpr (!ZERO0)
        *ring_at(0, sl(0, 2), r) = pfx[r];
    }
    int Ywu = Yw; // (a NARROW tile: per lane)
    if constexpr (!NARROW)
      Ywu = fresh(Yw);
    else if constexpr (CARRY)
      asm volatile("" : "+v"(Ywu)); // (one vector register and a comparison per use instead of a held lane mask per cell row)
#pragma unroll
    for (int q = 0; q < TY; ++q)
      cq[0][q] = (Ywu + q >= 0) ? pfc[q] : T(0);
    if constexpr (DERIVE)
    {
      clo = (Ywu - 1 >= 0) ? pflo : T(0);
      chi = (Ywu + TY >= 0) ? pfhi : T(0);
    }
  };

  // The loop's trip is K super-passes (the last trip may end early): the shift of the carried state is a renaming, and
  // with the slot of node layer n taken as (n - cb) mod depth the slot of a layer in a ring of depth K is a constant of the
  // position in the trip; a ring of the other depth takes one uniform base per trip.  (Tried: the march split into fill,
  // steady state without range tests and drain -- five copies of the super-pass; compiled, its wide body took 222 VGPRs and
  // 155 SGPR spills against 190 / 76 here and 198 / 50 before, so it was not run.)
  const int c_last = stage_end(K) + (K - 1);
  int c1 = cb, base2 = 0, base3 = 0;
  auto sl_at = [&](auto jt) {
    constexpr int j = decltype(jt)::value;
    return [&](int s, int k) {
      if (ring_depth(s, K, CARRY) == 3)
        return K % 3 == 0 ? ((j + k) % 3 + 3) % 3 : (base3 + j + k + 3) % 3;
      return K % 2 == 0 ? ((j + k) & 1) : ((base2 + j + k) & 1);
    };
  };
  for (;;)
  {
    super_pass(c1, sl_at(IntTag<0>{}));
    if (++c1 > c_last)
      break;
    if constexpr (K >= 2)
    {
      super_pass(c1, sl_at(IntTag<1>{}));
      if (++c1 > c_last)
        break;
    }
    if constexpr (K >= 3)
    {
      super_pass(c1, sl_at(IntTag<2>{}));
      if (++c1 > c_last)
        break;
    }
    base2 = (base2 + K) & 1;
    base3 = (base3 + K) % 3;
  }
}

// NARROW_TOO: the kernel carries the body for the tiles of a narrow last chunk column as well (twice the code: only the tile
// shapes the sweeps use by default have it; any other shape runs that column with ordinary tiles, most of their lanes idle)
template <typename T, int K, int TY, bool DREC, bool MODES, int DBG = 0, bool NARROW_TOO = false, bool ZERO0 = false>
__global__ __launch_bounds__(512, 2) void mf_cheb_fused_kernel(MfFusedArgs<T> a)
{
  // XCD-aware tile order (as mf_laplace_body): every XCD takes a contiguous run of the tile list (without the narrow body:
  // the tiles of the wide columns, which are all the tiles where there is no narrow column)
  const unsigned int n_tiles = NARROW_TOO ? a.wide_tiles + a.ntiles_y2 * a.ntiles_z : a.wide_tiles;
  unsigned int w = blockIdx.x;
  if (n_tiles >= 64)
  {
    const unsigned int per_xcd = (n_tiles + 7) / 8;
    w = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (w >= n_tiles)
      return; // the whole workgroup leaves
  }
  if constexpr (NARROW_TOO)
  {
    if (w >= a.wide_tiles)
    {
      mf_cheb_fused_body<T, K, TY, DREC, MODES, DBG, true, ZERO0>(a, w);
      return;
    }
  }
  mf_cheb_fused_body<T, K, TY, DREC, MODES, DBG, false, ZERO0>(a, w);
}

// Twelve wavefronts of TY = 2 rows, three per SIMD: the rows of eight of three (the same y-tiling, the same pairing of a narrow
// last column) at three quarters of the per-row state each.  Three terms, FP64, D^-1 from the coefficient sums (the kernels
// below: from the operator's D^-1 vector, which the sweep launches where that vector exists); at most 168
// VGPRs, and the rings two slots deep (mf_cheb_fused_body, NWC) so that 12 x (6 x 3) + 96 planes of 512 B = 156 KiB fit the LDS.
constexpr int kWgWaves12 = 12, kWgRows12 = 2;
constexpr bool kWg12ByDefault = true; // the tile of a sweep that can take it (choose_fused_tile)
template <typename T, bool MODES, bool NARROW_TOO, bool ZERO0>
__global__ __launch_bounds__(64 * kWgWaves12, 3) void mf_cheb_fused_wg12_kernel(MfFusedArgs<T> a)
{
  // (the tile order of mf_cheb_fused_kernel)
  const unsigned int n_tiles = NARROW_TOO ? a.wide_tiles + a.ntiles_y2 * a.ntiles_z : a.wide_tiles;
  unsigned int w = blockIdx.x;
  if (n_tiles >= 64)
  {
    const unsigned int per_xcd = (n_tiles + 7) / 8;
    w = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (w >= n_tiles)
      return;
  }
  if constexpr (NARROW_TOO)
  {
    if (w >= a.wide_tiles)
    {
      mf_cheb_fused_body<T, 3, kWgRows12, false, MODES, 0, true, ZERO0, kWgWaves12>(a, w);
      return;
    }
  }
  mf_cheb_fused_body<T, 3, kWgRows12, false, MODES, 0, false, ZERO0, kWgWaves12>(a, w);
}

// The same kernels with D^-1 read from the operator's vector (mf_cheb_fused_body, DVEC) instead of derived: per wavefront and
// super-pass three divisions, the pair sums of four cell rows with their row and layer sums and two coefficient requests less,
// three requests more (8 B/DoF); ten VGPRs of carried state go.  The sweep is bound by vector-ALU issue, not by memory.
template <typename T, bool MODES, bool NARROW_TOO, bool ZERO0>
__global__ __launch_bounds__(64 * kWgWaves12, 3) void mf_cheb_fused_wg12d_kernel(MfFusedArgs<T> a, T const *dinv)
{
  // (the tile order of mf_cheb_fused_kernel)
  const unsigned int n_tiles = NARROW_TOO ? a.wide_tiles + a.ntiles_y2 * a.ntiles_z : a.wide_tiles;
  unsigned int w = blockIdx.x;
  if (n_tiles >= 64)
  {
    const unsigned int per_xcd = (n_tiles + 7) / 8;
    w = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (w >= n_tiles)
      return;
  }
  if constexpr (NARROW_TOO)
  {
    if (w >= a.wide_tiles)
    {
      mf_cheb_fused_body<T, 3, kWgRows12, false, MODES, 0, true, ZERO0, kWgWaves12, true>(a, w, dinv);
      return;
    }
  }
  mf_cheb_fused_body<T, 3, kWgRows12, false, MODES, 0, false, ZERO0, kWgWaves12, true>(a, w, dinv);
}

// The tiles of a narrow last chunk column alone, launched behind the wide-only kernel on the same stream (MFMG_MF_FUSED_NARROW=split;
// each kernel gets the register budget of its own body).  The default carries both bodies in one launch: at 257^3 all tiles of
// the sweep fit one round of the chip, and a second launch queues its tiles behind the first.
template <typename T, int K, int TY, bool DREC, bool MODES, bool ZERO0 = false>
__global__ __launch_bounds__(512, 2) void mf_cheb_fused_narrow_kernel(MfFusedArgs<T> a)
{
  const unsigned int n_tiles = a.ntiles_y2 * a.ntiles_z;
  unsigned int w = blockIdx.x;
  if (n_tiles >= 64)
  {
    const unsigned int per_xcd = (n_tiles + 7) / 8;
    w = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (w >= n_tiles)
      return;
  }
  mf_cheb_fused_body<T, K, TY, DREC, MODES, 0, true, ZERO0>(a, a.wide_tiles + w);
}

// ---- one coefficient for the whole mesh, all six faces Dirichlet (MatrixFreeLaplaceDevice::uniform_coefficient) ------------
// On the free DoFs the operator is then ONE 27-point stencil and D^-1 one number, and the stencil is separable:
//   A = c (K (x) M (x) M + M (x) K (x) M + M (x) M (x) K),   K = 2 f_d (2, -1), M = (4/3, 1/3) per direction
// (the assembled 1-D stiffness and mass stencils of the cell matrix of cell_row_modes).  Applied direction by direction on the
// node layer n, with the factors 1/3 and 2 f c folded into the constants q[] and z[] (host, in double):
//   x:  s = u[i-1] + u[i+1];            mx = 4 u + s,  kx = 2 u - s                              per node
//   y:  sM = mx[j-1] + mx[j+1], sK likewise;  P = 4 mx + sM,  Q = q0 mx + q1 sM + q2 kx + q3 sK       per node
//   z:  Z1 = z1p P + z1q Q,  Z0 = z0p P + z0q Q;  (A u) of layer n = Z1(n-1) + Z0(n) + Z1(n+1)
// About 20 FP64 operations per node and term against 43 per cell and 2 per node in mode space; no coefficient and no D^-1 is
// loaded or carried.
//
// The structure is that of mf_cheb_fused_body with NWC = 12 (tiles and their order, the march in trips of three, the rings two
// slots deep with the neighbour columns read from them, the carried momentum operand, the descriptors, owner computes, Dirichlet
// DoFs finished by stage 1).  What differs:
//  - A stage pass "on the cell layer c" forms the products of the node layer c + 1 alone and completes the DoF layer c from them
//    and two carries per DoF (cA = Z1(c-1) + Z0(c), cB = Z1(c)).  A stage therefore starts one pass earlier than in the cell form:
//    its first pass primes the carries with layer start + 1, the second completes them, the third is right -- unless the start is
//    the bottom of the mesh, whose layer 0 is Dirichlet and contributes zero.
//  - The exchange: a wavefront exports the x-transformed values (mx, kx) of the node rows next to the two it shares -- with two
//    cell rows that is its middle row, the only row its neighbours do not hold; both neighbours complete the row they share from the
//    same operands in the same order (row below + row above).  Two values per wavefront and stage pass (four with three or four
//    cell rows), one barrier.
//  - Twelve wavefronts (mf_cheb_fused_uniform_kernel) share no row at all.  A node row is completed from the (mx, kx) of the rows
//    below and above it, so the second evaluation of a shared row -- which the cell form needs, its two cell rows both contribute --
//    is repetition here.  Each wavefront holds R = 3 node rows of its own, Yw = tyi RY - K + 3 wv with RY = 12 * 3 - 2 K = 30 owned
//    rows per tile.  It exports (mx, kx) of its rows 0 and R - 1 (four values per stage pass); its row 0 is completed with the lower
//    neighbour's row R - 1 as "below", its row R - 1 with the upper neighbour's row 0 as "above", its middle row from its own; the
//    first and the last wavefront take zeros on the missing side (halo rows).  Still one barrier and the operands in the same
//    order: the bits of the other shapes.
template <typename T>
struct MfUniformArgs
{
  T const *x; // x_0
  T const *b;
  T *out;      // x_3
  T *out_prev; // x_2 (nullptr: not wanted)
  int Nx, Ny, Nz;
  unsigned int ncols, ntiles_y, ntiles_z;
  int own, halo;
  int TZ;
  T q[4], z[4];     // the stencil constants above: z = {z0p, z0q, z1p, z1q}
  T alpha[3], beta[3];
  T bd[3];          // beta_s D^-1 of the free DoFs
  AffineIds aff;
  unsigned int vec_bytes;
  unsigned int wide_tiles, ntiles_y2; // (MfFusedArgs)
};

// TY, NWC: cell rows per wavefront; the number of wavefronts where the kernel fixes it (0: that of the launch).  Every shape
// evaluates a DoF through the same expressions, so the results do not depend on the shape either.
// XV: values a wavefront exports per stage pass -- (mx, kx) of its node row TY - 1 for the neighbour above and of its node row 1
// for the neighbour below; with two cell rows these are one row.  DISJ (NWC = 12): the R node rows of a wavefront are its own, it
// exports its rows R - 1 and 0 (see above).
template <typename T, int TY, bool NARROW, bool ZERO0, int NWC>
__device__ __forceinline__ void mf_cheb_uniform_body(MfUniformArgs<T> const &a, unsigned int w)
{
#pragma clang fp contract(off)
  constexpr bool DISJ = NWC == kWgWaves12;
  static_assert(!DISJ || TY == kWgRows12, "disjoint node rows: three per wavefront");
  constexpr int K = 3, R = TY + 1, XV = (TY == 2 && !DISJ) ? 2 : 4;
  const int NW = NWC > 0 ? NWC : (int)(blockDim.x >> 6);
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // LDS: per wavefront the rings x_0 .. x_2 ([6 planes][R rows][64 lanes]); then the exports [2][NW][XV][64]
  T *ring = reinterpret_cast<T *>(smem_raw) + (size_t)wv * (2 * K * R * 64) + lane;
  // the same planes as the next / the previous lane sees them (the last / first lane: its own, a halo lane)
  T const *ring_next = ring + (lane == 63 ? 0 : 1);
  T const *ring_prev = ring - (lane == 0 ? 0 : 1);
  T *xport = reinterpret_cast<T *>(smem_raw) + (size_t)NW * (2 * K * R * 64) + lane;

  const int wcols = a.ntiles_y2 > 0 ? (int)a.ncols - 1 : (int)a.ncols;
  int tc, tyi, tzi, lx = lane;
  if constexpr (NARROW)
  {
    const unsigned int v = w - a.wide_tiles;
    tc = (int)a.ncols - 1;
    tyi = 2 * (int)(v % a.ntiles_y2) + (lane >> 5); // (per lane)
    tzi = (int)(v / a.ntiles_y2);
    lx = lane & 31;
  }
  else
  {
    tc = (int)(w % (unsigned int)wcols);
    tyi = (int)((w / (unsigned int)wcols) % a.ntiles_y);
    tzi = (int)(w / ((unsigned int)wcols * a.ntiles_y));
  }
  const bool tile_live = !NARROW || tyi < (int)a.ntiles_y;

  // (all six faces are Dirichlet, no ghost layers)
  const int ci = tc * a.own - a.halo + lx;
  const bool lane_free = ci >= 1 && ci < a.Nx - 1;
  const bool col_owned = tile_live && lx >= a.halo && lx < a.halo + a.own && ci < a.Nx;
  const int RY = DISJ ? NW * R - 2 * K : NW * TY - 2 * K + 1;
  const int Yw = tyi * RY - K + wv * (DISJ ? R : TY);
  const int own_y0 = tyi * RY, own_y1 = min(own_y0 + RY, a.Ny);
  const int Z0 = tzi * a.TZ, Z1 = min(Z0 + a.TZ, a.Nz);
  const unsigned int off_lane = (unsigned int)(a.aff.base + min(max(ci, 0), a.Nx - 1) * a.aff.s0) * (unsigned int)sizeof(T);

  // the constants as uniform values in vector registers (mf_cheb_fused_body, CARRY)
  auto hold = [](T v) {
    asm volatile("" : "+v"(v));
    return v;
  };
  const T q0 = hold(a.q[0]), q1 = hold(a.q[1]), q2 = hold(a.q[2]), q3 = hold(a.q[3]);
  const T z0p = hold(a.z[0]), z0q = hold(a.z[1]), z1p = hold(a.z[2]), z1q = hold(a.z[3]);
  T held_alpha[K], held_bd[K];
#pragma unroll
  for (int s = 0; s < K; ++s)
  {
    held_alpha[s] = s > 0 ? hold(a.alpha[s]) : T(0);
    held_bd[s] = hold(a.bd[s]);
  }
  auto fresh = [](int v) {
    v = __builtin_amdgcn_readfirstlane(v);
    asm volatile("" : "+s"(v));
    return v;
  };

  bool row_free_lane[R], row_own_lane[R];
#pragma unroll
  for (int r = 0; r < R; ++r)
  {
    const int j = Yw + r;
    row_free_lane[r] = lane_free && j >= 1 && j < a.Ny - 1;
    if constexpr (DISJ)
      // no row is shared.  The owned rows of a tile are whole wavefronts, 1 .. NW - 2 (K = R), up to the last row of the mesh:
      // one mask for the three rows -- a free DoF lies inside the mesh, a Dirichlet DoF asks for its row where it is stored
      // (row_in_mesh: rarely, and three lane masks less to carry through the march)
      row_own_lane[r] = col_owned && wv >= 1 && wv < NW - 1;
    else
      row_own_lane[r] = col_owned && r < TY && j >= own_y0 && j < own_y1; // (the node row two wavefronts share is stored by the upper one)
  }
  int yw_lane = Yw;
  auto row_in_mesh = [&](int r) -> bool {
    asm volatile("" : "+v"(yw_lane)); // (anew at every use: not a mask per row held across the march)
    return yw_lane + r < a.Ny;
  };
  auto rs_vec = [&](T const *p) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(p), 0, a.vec_bytes, 0x00020000); };
  const int want_prev_i = a.out_prev != nullptr ? 1 : 0;
  auto want_prev_f = [&]() -> bool { return fresh(want_prev_i) != 0; };
  const unsigned int row_stride = (unsigned int)a.aff.s1 * (unsigned int)sizeof(T), layer_stride = (unsigned int)a.aff.s2 * (unsigned int)sizeof(T);
  const int zown0 = Z0, zown1 = Z1;
  auto layer_free = [&](int n) { return n >= 1 && n < a.Nz - 1; };
  auto layer_own = [&](int n) { return n >= zown0 && n < zown1; };
  struct Off
  {
    unsigned int v, s;
  };
  auto vec_off = [&](int r, int n) -> Off {
    const unsigned int rowb = (unsigned int)min(max(Yw + r, 0), a.Ny - 1) * row_stride, layb = (unsigned int)min(max(n, 0), a.Nz - 1) * layer_stride;
    if constexpr (NARROW)
      return Off{off_lane + rowb, layb};
    else
      return Off{off_lane, rowb + layb};
  };
  auto ld_vec = [&](__amdgpu_buffer_rsrc_t rs, int r, int n) -> T {
    const Off o = vec_off(r, n);
    return BufIO<T>::ld(rs, o.v, o.s);
  };
  auto st_vec = [&](T v, __amdgpu_buffer_rsrc_t rs, int r, int n) {
    const Off o = vec_off(r, n);
    BufIO<T>::st(v, rs, o.v, o.s);
  };
  auto ring_at = [&](int s, int sl, int r) -> T * { return ring + ((2 * s + sl) * R + r) * 64; };
  auto ring_next_at = [&](int s, int sl, int r) -> T const * { return ring_next + ((2 * s + sl) * R + r) * 64; };
  auto ring_prev_at = [&](int s, int sl, int r) -> T const * { return ring_prev + ((2 * s + sl) * R + r) * 64; };

  // ---- per-lane state carried from super-pass to super-pass (stage s + 1 uses entry s)
  T bq[K][R];         // b of the DoF (row r, layer of the stage)
  T pa[K][R], pb[K][R]; // the z-carries cA and cB
  T xn[K][R], xq[K][R]; // the momentum operand (mf_cheb_fused_body, CARRY)
#pragma unroll
  for (int s = 0; s < K; ++s)
#pragma unroll
    for (int r = 0; r < R; ++r)
      bq[s][r] = pa[s][r] = pb[s][r] = xn[s][r] = xq[s][r] = T(0);

  // stage s starts on the cell layer max(Z0 - K + (s - 1) - 1, 0): one layer below the start of the cell form (the priming pass)
  const int cb = max(Z0 - K - 1, 0);

  // ---- prologue: the two x_0 layers and b of the first super-pass
  {
    const __amdgpu_buffer_rsrc_t rs_x = rs_vec(a.x), rs_b = rs_vec(a.b);
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
      if constexpr (!ZERO0)
      {
        *ring_at(0, 0, r) = ld_vec(rs_x, r, cb);
        *ring_at(0, 1, r) = ld_vec(rs_x, r, cb + 1);
      }
      bq[0][r] = ld_vec(rs_b, r, cb);
    }
  }

  unsigned int ex = 0; // stage passes so far (parity of the export buffers)

  // ---- one stage pass: stage S (1-based) on the cell layer c; sl(s, d) = the slot of node layer c + d in ring s
  auto stage_pass = [&](auto tag, int c, auto sl) {
    constexpr int S = decltype(tag)::value;
    constexpr bool kApply = !(S == 1 && ZERO0); // (A 0 = 0: no arithmetic, no exchange, no barrier)
    const bool lo_free = layer_free(c), hi_free = layer_free(c + 1);
    const bool l_own = layer_own(c);
    T xown[R], mx[R], kx[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
      xown[r] = mx[r] = kx[r] = T(0);
      if constexpr (kApply)
      {
        const T l = *ring_at(S - 1, sl(S - 1, 0), r), u = *ring_at(S - 1, sl(S - 1, 1), r);
        xown[r] = l;
        if constexpr (S < K)
          xn[S - 1][r] = l;
        T um, sm;
        if constexpr (S == 1)
        {
          // x_0 sits in the ring as it was read; Dirichlet and out-of-mesh values enter the stencil as zero
          um = (row_free_lane[r] && hi_free) ? u : T(0);
          sm = from_prev_lane(um) + from_next_lane(um);
        }
        else
        {
          um = u;
          sm = *ring_prev_at(S - 1, sl(S - 1, 1), r) + *ring_next_at(S - 1, sl(S - 1, 1), r);
        }
        mx[r] = fmadd<T>(T(4), um, sm);
        kx[r] = fmadd<T>(T(2), um, -sm);
      }
    }
    if constexpr (kApply)
    {
      T *xp = xport + (size_t)((ex & 1) * NW + wv) * XV * 64;
      xp[0] = mx[DISJ ? R - 1 : TY - 1];
      xp[64] = kx[DISJ ? R - 1 : TY - 1];
      if constexpr (XV == 4)
      {
        xp[128] = mx[DISJ ? 0 : 1];
        xp[192] = kx[DISJ ? 0 : 1];
      }
    }
    // the y-stencil of a node row from the rows below (b), its own and above (a); then the z-stencil with the carries
    auto apply_yz = [&](T mb, T kb, T m, T k, T ma, T ka, T &cA, T &cB) -> T {
      const T sM = mb + ma, sK = kb + ka;
      const T P = fmadd<T>(T(4), m, sM);
      const T Q = fmadd<T>(q3, sK, fmadd<T>(q2, k, fmadd<T>(q1, sM, q0 * m)));
      const T Zn = fmadd<T>(z1q, Q, z1p * P), Zd = fmadd<T>(z0q, Q, z0p * P);
      const T yv = cA + Zn;
      cA = cB + Zd;
      cB = Zn;
      return yv;
    };
    // one DoF (row r, layer c) of this stage is complete: yv = (A x_{S-1}) there
    auto finish = [&](auto rtag, T yv) {
      constexpr int r = decltype(rtag)::value;
      const bool fr = row_free_lane[r] && lo_free;
      const bool st = row_own_lane[r] && l_own;
      if constexpr (S == 1)
      {
        const T x0 = xown[r], lb = bq[0][r];
        const T x1 = fmadd<T>(-held_bd[0], yv - lb, x0);
        *ring_at(1, sl(1, 0), r) = fr ? x1 : T(0);
        // Dirichlet DoFs: identity rows with D^-1 = 1 -- the whole recurrence here
        if (st && !fr && (!DISJ || row_in_mesh(r)))
        {
          T xa = x0, xb = fmadd<T>(-a.beta[0], x0 - lb, x0); // x_{s-1}, x_s
#pragma unroll
          for (int s = 1; s < K; ++s)
          {
            const T xc = fmadd<T>(-a.beta[s], xb - lb, fmadd<T>(a.alpha[s], xb - xa, xb));
            xa = xb;
            xb = xc;
          }
          st_vec(xb, rs_vec(a.out), r, c);
          if (want_prev_f())
            st_vec(xa, rs_vec(a.out_prev), r, c);
        }
      }
      else
      {
        const T xo = xown[r];
        const T xoo = xq[S - 2][r]; // (zero from a zero guess)
        const T xoo_m = (S == 2) ? (fr ? xoo : T(0)) : xoo; // (x_0 sits in its ring unmasked)
        const T xs = fmadd<T>(-held_bd[S - 1], yv - bq[S - 1][r], fmadd<T>(held_alpha[S - 1], xo - xoo_m, xo));
        if constexpr (S < K)
        {
          *ring_at(S, sl(S, 0), r) = fr ? xs : T(0);
          if constexpr (S == K - 1)
            if (st && fr && want_prev_f())
              st_vec(xs, rs_vec(a.out_prev), r, c);
        }
        else
        {
          if (st && fr)
            st_vec(xs, rs_vec(a.out), r, c);
        }
      }
    };
    // the rows between the wavefront's own cells: their neighbour rows are the wavefront's own
    auto inner = [&](auto rtag) {
      constexpr int r = decltype(rtag)::value;
      T yv = T(0);
      if constexpr (kApply)
        yv = apply_yz(mx[r - 1], kx[r - 1], mx[r], kx[r], mx[r + 1], kx[r + 1], pa[S - 1][r], pb[S - 1][r]);
      finish(rtag, yv);
    };
    inner(IntTag<1>{});
    if constexpr (TY >= 3)
      inner(IntTag<2>{});
    if constexpr (TY >= 4)
      inner(IntTag<3>{});
    // (LDS only: the requests of the next super-pass stay in flight across the barrier)
    if constexpr (kApply)
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // the rows shared with the neighbours: both wavefronts complete them, with the same operands in the same order
    // (DISJ: the wavefront's first and last row, completed by it alone from the neighbour's last / first row)
    {
      T lom = T(0), lok = T(0), him = T(0), hik = T(0);
      const int wvu = fresh(wv);
      if (kApply && wvu > 0)
      {
        T const *ip = xport + (size_t)((ex & 1) * NW + wvu - 1) * XV * 64;
        lom = ip[0];
        lok = ip[64];
      }
      if (kApply && wvu + 1 < NW)
      {
        T const *ip = xport + (size_t)((ex & 1) * NW + wvu + 1) * XV * 64;
        him = ip[XV == 4 ? 128 : 0];
        hik = ip[XV == 4 ? 192 : 64];
      }
      {
        T yv = T(0);
        if constexpr (kApply)
          yv = apply_yz(lom, lok, mx[0], kx[0], mx[1], kx[1], pa[S - 1][0], pb[S - 1][0]);
        finish(IntTag<0>{}, yv);
      }
      {
        T yv = T(0);
        if constexpr (kApply)
          yv = apply_yz(mx[TY - 1], kx[TY - 1], mx[TY], kx[TY], him, hik, pa[S - 1][TY], pb[S - 1][TY]);
        finish(IntTag<TY>{}, yv);
      }
    }
    if constexpr (kApply)
      ++ex;
  };

  // ---- the march (mf_cheb_fused_body; the stages start one super-pass earlier, see above)
  auto super_pass = [&](int c1, auto sl) {
    T pfx[R], pfb[R];
    const __amdgpu_buffer_rsrc_t rs_x = rs_vec(a.x), rs_b = rs_vec(a.b);
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
      pfx[r] = T(0);
      if constexpr (!ZERO0)
        pfx[r] = ld_vec(rs_x, r, c1 + 2);
      pfb[r] = ld_vec(rs_b, r, c1 + 1);
    }
    if (c1 < a.Nz)
      stage_pass(IntTag<1>{}, c1, [&](int s, int d) { return sl(s, d); });
    if (c1 >= max(Z0 - 2, 1) && c1 <= a.Nz)
      stage_pass(IntTag<2>{}, c1 - 1, [&](int s, int d) { return sl(s, d - 1); });
    if (c1 >= max(Z0, 2))
      stage_pass(IntTag<3>{}, c1 - 2, [&](int s, int d) { return sl(s, d - 2); });
#pragma unroll
    for (int s = K - 1; s >= 1; --s)
#pragma unroll
      for (int r = 0; r < R; ++r)
        bq[s][r] = bq[s - 1][r];
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
      bq[0][r] = pfb[r];
#pragma unroll
      for (int s = 0; s + 2 <= K; ++s)
        xq[s][r] = xn[s][r];
      if constexpr (!ZERO0)
        *ring_at(0, sl(0, 2), r) = pfx[r];
    }
  };
  const int c_last = min(Z1 + 1, a.Nz + 1);
  int c1 = cb, base2 = 0;
  auto sl_at = [&](auto jt) {
    constexpr int j = decltype(jt)::value;
    return [&](int, int k) { return (base2 + j + k) & 1; };
  };
  for (;;)
  {
    super_pass(c1, sl_at(IntTag<0>{}));
    if (++c1 > c_last)
      break;
    super_pass(c1, sl_at(IntTag<1>{}));
    if (++c1 > c_last)
      break;
    super_pass(c1, sl_at(IntTag<2>{}));
    if (++c1 > c_last)
      break;
    base2 = (base2 + K) & 1;
  }
}

template <typename T, bool NARROW_TOO, bool ZERO0>
__global__ __launch_bounds__(64 * kWgWaves12, 3) void mf_cheb_fused_uniform_kernel(MfUniformArgs<T> a)
{
  // (the tile order of mf_cheb_fused_kernel)
  const unsigned int n_tiles = NARROW_TOO ? a.wide_tiles + a.ntiles_y2 * a.ntiles_z : a.wide_tiles;
  unsigned int w = blockIdx.x;
  if (n_tiles >= 64)
  {
    const unsigned int per_xcd = (n_tiles + 7) / 8;
    w = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (w >= n_tiles)
      return;
  }
  if constexpr (NARROW_TOO)
  {
    if (w >= a.wide_tiles)
    {
      mf_cheb_uniform_body<T, kWgRows12, true, ZERO0, kWgWaves12>(a, w);
      return;
    }
  }
  mf_cheb_uniform_body<T, kWgRows12, false, ZERO0, kWgWaves12>(a, w);
}

// The same stencil on the other shapes of the three-term sweep (up to eight wavefronts of TY = 2, 3 or 4 rows, two per SIMD; a
// narrow last column as ordinary tiles): a uniform operator gives the same bits on every tile shape.
template <typename T, int TY, bool ZERO0>
__global__ __launch_bounds__(512, 2) void mf_cheb_fused_uniform_rows_kernel(MfUniformArgs<T> a)
{
  // (the tile order of mf_cheb_fused_kernel)
  const unsigned int n_tiles = a.wide_tiles;
  unsigned int w = blockIdx.x;
  if (n_tiles >= 64)
  {
    const unsigned int per_xcd = (n_tiles + 7) / 8;
    w = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (w >= n_tiles)
      return;
  }
  mf_cheb_uniform_body<T, TY, false, ZERO0, 0>(a, w);
}
} // namespace

// ---- host side --------------------------------------------------------------------------------------------------
template <typename T>
bool MatrixFreeLaplaceDevice<T>::fused_sweep_available(int n_terms) const
{
  if (!(_dim == 3 && _compact && _affine_ids && !_tail && n_terms >= 1 && n_terms <= 3 && _halo >= n_terms && (uint64_t)_rec.size() <= 0xffffffffull))
    return false;
  // distributed: the ranks exchange x once per sweep, n_terms planes deep -- all of them or none (what every rank can do)
  if (_handle.comm.enabled() && n_terms > _handle.comm.sweep_terms())
    return false;
  // a side with ghost planes (a neighbouring rank) must hold n_terms of them: the sweep computes them redundantly
  for (int d = 0; d < 3; ++d)
    if ((_affine.ghost_lo[d] > 0 && _affine.ghost_lo[d] < n_terms) || (_affine.ghost_hi[d] > 0 && _affine.ghost_hi[d] < n_terms))
      return false;
  return true;
}

// The sweep from x_0 = 0 (smoother_sweep with x == nullptr): the three-term kernels with three rows per wavefront and the default
// arithmetic carry that variant.
template <typename T>
bool MatrixFreeLaplaceDevice<T>::fused_zero_guess_available(int n_terms) const
{
  if (n_terms != 3 || !fused_sweep_available(n_terms) || _fused_reference_arithmetic)
    return false;
  int nw, ty, tz;
  choose_fused_tile(n_terms, nw, ty, tz);
  return ty == 3 || nw == kWgWaves12;
}

// tile of the sweep: NW wavefronts of TY cell rows, TZ owned layers.  One workgroup of eight wavefronts per CU (two per
// SIMD: the per-lane state takes ~200 VGPRs) or two of four; the height is chosen so that the workgroups fill whole
// rounds of the chip -- a workgroup lives for K TZ + K^2 stage passes, a part-filled round costs a full one.  Three terms in
// FP64 with D^-1 from the coefficient sums also have twelve wavefronts of two rows (three per SIMD, mf_cheb_fused_wg12_kernel):
// asked of a sweep that has no such kernel (two terms, FP32, D^-1 in the records), that shape leaves the sweep on its default.
template <typename T>
bool MatrixFreeLaplaceDevice<T>::fused_wg12_capable(int n_terms) const
{
  return std::is_same<T, double>::value && n_terms == 3 && !_dinv_in_record;
}

// MFMG_MF_FUSED_DBG (timing experiments: the kernels without barrier / without division), read once
static int fused_dbg()
{
  static const int dbg = std::getenv("MFMG_MF_FUSED_DBG") ? std::atoi(std::getenv("MFMG_MF_FUSED_DBG")) : 0;
  return dbg;
}

// The stencil sweep of a uniform coefficient on twelve wavefronts (smoother_sweep: mf_cheb_fused_uniform_kernel): the node rows of
// its wavefronts are disjoint, a y-tile owns 12 * 3 - 2 * 3 = 30 rows.  MFMG_MF_UNIFORM_SWEEP is read at every call, as there.
template <typename T>
bool MatrixFreeLaplaceDevice<T>::uniform_disjoint_rows(int n_terms, int nw, int ty) const
{
  if (!(std::is_same<T, double>::value && _uniform && !_fused_reference_arithmetic && n_terms == 3 && fused_dbg() == 0 && nw == kWgWaves12 && ty == kWgRows12))
    return false;
  char const *uniform_env = std::getenv("MFMG_MF_UNIFORM_SWEEP");
  return !(uniform_env && std::string(uniform_env) == "0");
}

// owned node rows of a y-tile
template <typename T>
int MatrixFreeLaplaceDevice<T>::fused_tile_owned_rows(int n_terms, int nw, int ty) const
{
  return uniform_disjoint_rows(n_terms, nw, ty) ? nw * (ty + 1) - 2 * n_terms : nw * ty - 2 * n_terms + 1;
}

template <typename T>
void MatrixFreeLaplaceDevice<T>::choose_fused_tile(int n_terms, int &nw, int &ty, int &tz) const
{
  // (measured at 257^3 DoFs: three terms 8 x 3 rows -- four rows per wavefront spill --, two terms 4 x 4: two independent
  // workgroups per CU, 0.31 against 0.34 ms; three terms in FP64 12 x 2 rows against 8 x 3: 0.345 against 0.364 ms)
  nw = n_terms == 2 ? 4 : 8;
  ty = n_terms == 2 ? 4 : 3;
  tz = 0;
  if (kWg12ByDefault && fused_wg12_capable(n_terms))
  {
    nw = kWgWaves12;
    ty = kWgRows12;
  }
  static const std::string env = std::getenv("MFMG_MF_FUSED_TILE") ? std::getenv("MFMG_MF_FUSED_TILE") : "";
  if (_fused_tile[0] > 0)
  {
    nw = _fused_tile[0];
    ty = _fused_tile[1];
    tz = _fused_tile[2];
  }
  else if (!env.empty())
  {
    int v[3] = {0, 0, 0};
    if (std::sscanf(env.c_str(), "%d,%d,%d", &v[0], &v[1], &v[2]) == 3)
    {
      nw = v[0];
      ty = v[1];
      tz = v[2];
    }
  }
  if (nw == kWgWaves12 && ty == kWgRows12 && !fused_wg12_capable(n_terms))
  {
    nw = n_terms == 2 ? 4 : 8;
    ty = n_terms == 2 ? 4 : 3;
  }
  ASSERT_THROW(((nw >= 1 && nw <= 8) || (nw == kWgWaves12 && ty == kWgRows12)) && (ty == 2 || ty == 3 || ty == 4),
               "tile of the multi-term sweep: 1..8 wavefronts of 2, 3 or 4 rows, or 12 of 2");
  const int ry = fused_tile_owned_rows(n_terms, nw, ty);
  ASSERT_THROW(ry >= 1, "tile of the multi-term sweep too small for its halo rows");
  if (tz > 0)
    return;
  const int64_t slots = (int64_t)mf_n_cus() * (nw > 8 ? 1 : 8 / nw); // (more than eight wavefronts: one workgroup per CU)
  const int64_t nty = (_N[1] + ry - 1) / ry;
  const int64_t tiles_xy = (narrow_last_column() && fused_narrow_capable(n_terms, ty, nw)) ? (int64_t)(_ncols - 1) * nty + (nty + 1) / 2 : (int64_t)_ncols * nty;
  double best = 0.;
  for (int nz = 1; nz <= _N[2]; ++nz)
  {
    const int t = (_N[2] + nz - 1) / nz;
    if ((_N[2] + t - 1) / t != nz)
      continue;
    const int64_t rounds = (tiles_xy * nz + slots - 1) / slots;
    const double cost = double(rounds) * (double(n_terms) * t + double(n_terms) * n_terms);
    if (tz == 0 || cost < best)
    {
      best = cost;
      tz = t;
    }
  }
}

template <typename T>
void MatrixFreeLaplaceDevice<T>::smoother_sweep(int n_terms, T const *alpha, T const *beta, T const *b, T const *x, T *out, T *out_prev) const
{
  ASSERT_THROW(fused_sweep_available(n_terms), "the multi-term smoother sweep is not available for this operator");
  const bool zero_guess = x == nullptr; // x_0 = 0: nothing is read of it (fused_zero_guess_available)
  ASSERT_THROW(b != nullptr && out != nullptr, "null vector");
  ASSERT_THROW(!zero_guess || fused_zero_guess_available(n_terms), "the sweep from a zero guess is not available for this operator / tile");
  ASSERT_THROW((zero_guess || (x != out && x != out_prev)) && out != out_prev, "the multi-term sweep cannot run in place");
  ASSERT_THROW(alpha[0] == T(0), "the first term of a sweep takes no momentum");
  int nw, ty, tz;
  choose_fused_tile(n_terms, nw, ty, tz);
  MfFusedArgs<T> a{};
  a.rec = _rec.data();
  a.x = zero_guess ? b : x; // (never read from a zero guess; the descriptor wants an address)
  a.b = b;
  a.out = out;
  a.out_prev = out_prev;
  a.Nx = _N[0];
  a.Ny = _N[1];
  a.Nz = _N[2];
  a.ncols = (unsigned int)_ncols;
  // (a uniform coefficient on twelve wavefronts: the tiles of mf_cheb_fused_uniform_kernel, which this call then launches)
  const bool disjoint_rows = uniform_disjoint_rows(n_terms, nw, ty);
  const int ry = fused_tile_owned_rows(n_terms, nw, ty);
  a.ntiles_y = (unsigned int)((_N[1] + ry - 1) / ry);
  a.ntiles_z = (unsigned int)((_N[2] + tz - 1) / tz);
  a.own = _own;
  a.halo = _halo;
  a.TZ = tz;
  a.rec_bytes = (unsigned int)_rec_bytes;
  a.dinv_in_record = _dinv_in_record ? 1 : 0;
  {
    double f[3];
    mf_cell_factors(a, _h, f);
    // the cell matrix on the modes (cell_row_modes): stiffness diag(0, 1), masses diag(1/2, 1/6) and f diag(1, 1/3)
    a.lam[0] = T(f[0] / 2.);
    a.lam[1] = T(f[1] / 2.);
    a.lam[2] = T(f[2] / 2.);
    a.lam[3] = T((f[0] + f[1]) / 6.);
    a.lam[4] = T((f[0] + f[2]) / 6.);
    a.lam[5] = T((f[1] + f[2]) / 6.);
    a.lam[6] = T((f[0] + f[1] + f[2]) / 18.);
  }
  for (int s = 0; s < 3; ++s)
  {
    a.alpha[s] = s < n_terms ? alpha[s] : T(0);
    a.beta[s] = s < n_terms ? beta[s] : T(0);
  }
  a.aff = _affine;
  a.vec_bytes = (unsigned int)std::min<uint64_t>((uint64_t)_n_dofs * sizeof(T), 0xffffffffull);
  ASSERT_THROW((uint64_t)_rec.size() <= 0xffffffffull, "chunk records beyond 4 GiB: the multi-term sweep addresses them with 32-bit offsets");
  a.rec_total_bytes = (unsigned int)_rec.size();
  // a narrow last chunk column (mf_laplace.hip: at most 32 - 2 halo owned columns) is swept two y-tiles per workgroup by the
  // kernels that carry the body for it
  // (twelve wavefronts in the reference arithmetic: both bodies in one kernel do not fit its 168 VGPRs, ordinary tiles there)
  const bool narrow = narrow_last_column() && fused_narrow_capable(n_terms, ty, nw) && !(nw == kWgWaves12 && _fused_reference_arithmetic);
  a.ntiles_y2 = narrow ? (a.ntiles_y + 1) / 2 : 0u;
  a.wide_tiles = (a.ncols - (narrow ? 1u : 0u)) * a.ntiles_y * a.ntiles_z;
  const uint64_t n_tiles = (uint64_t)a.wide_tiles + (uint64_t)a.ntiles_y2 * a.ntiles_z;
  ASSERT_THROW(n_tiles < (1ull << 30), "tile of the multi-term sweep too small for this mesh (grid size limit)");
  const unsigned int n_blocks = mf_xcd_grid(n_tiles);
  const bool wg12 = nw == kWgWaves12; // (choose_fused_tile: three terms of two rows, FP64, D^-1 from the coefficient sums)
  const size_t lds = ((size_t)nw * ring_planes(n_terms, wg12) * (ty + 1) + (size_t)2 * nw * 4) * 64 * sizeof(T);
  ASSERT_THROW(lds <= kMfMaxLds, "tile of the multi-term sweep too large for the LDS");
  hipStream_t st = _handle.stream;
  // Algorithmic bytes of the launch: what its n_terms smoother terms require as launches of their own (x, out, one id, the
  // coefficient, b, x_prev: mf_laplace.hpp) -- the figure the one-term kernel is priced on, so that the two compare.  What the
  // sweep itself must move is fused_sweep_bytes(): x_0, b, the coefficient, x_K (+ x_{K-1}), the ids computed.
  double bytes = 0.;
  for (int k = 0; k < n_terms; ++k)
    bytes += required_bytes_apply() + epilogue_bytes(k == 0 ? 2 : 3);
  hipEvent_t stop = _handle.profiler.begin("mf_cheb_fused_kernel", bytes, st);
  static const bool narrow_split = std::getenv("MFMG_MF_FUSED_NARROW") && std::string(std::getenv("MFMG_MF_FUSED_NARROW")) == "split";
  auto go = [&](auto kernel, unsigned int blocks) { mf_launch(kernel, MfGrid{blocks, nw, lds, st}, a); };
  // a kernel that carries both bodies (joint) or the wide-only kernel followed by the narrow-only one (split)
  auto go_narrow = [&](auto joint, auto wide, auto narrow_only) {
    if (!narrow_split)
      go(joint, n_blocks);
    else
    {
      go(wide, mf_xcd_grid(a.wide_tiles));
      go(narrow_only, mf_xcd_grid((uint64_t)a.ntiles_y2 * a.ntiles_z));
    }
  };
  // the arithmetic of the cell kernel: mode space (default) or the bit-for-bit twin of the one-term kernel (set_fused_reference)
  const bool modes = !_fused_reference_arithmetic;
  const int dbg = fused_dbg();
  // the kernel <K, TY, DREC, MODES> with or without the body of a narrow last column (fused_narrow_capable: two shapes carry it)
  // and, from a zero guess, its ZERO0 form (fused_zero_guess_available: one shape has it)
  auto sweep = [&](auto kt, auto tt, auto dt, auto mt) {
    constexpr int K = decltype(kt)::value, TY = decltype(tt)::value;
    constexpr bool DR = decltype(dt)::value, MO = decltype(mt)::value;
    auto with_guess = [&](auto zt) {
      constexpr bool Z0 = decltype(zt)::value;
      if constexpr (fused_narrow_capable(K, TY))
        if (narrow)
          return go_narrow(mf_cheb_fused_kernel<T, K, TY, DR, MO, 0, true, Z0>, mf_cheb_fused_kernel<T, K, TY, DR, MO, 0, false, Z0>,
                           mf_cheb_fused_narrow_kernel<T, K, TY, DR, MO, Z0>);
      go(mf_cheb_fused_kernel<T, K, TY, DR, MO, 0, false, Z0>, n_blocks);
    };
    if constexpr (K == 3 && TY == 3 && MO)
      if (zero_guess)
        return with_guess(std::true_type());
    with_guess(std::false_type());
  };
  // one coefficient for the whole mesh (uniform_coefficient): the operator as three 1-D stencils.  MFMG_MF_UNIFORM_SWEEP=0 keeps
  // the mode-space kernels (the A/B switch); the reference arithmetic keeps its own.
  // (read at every sweep, not once: a process can measure both)
  // (twelve wavefronts: the tiles above are those of the answer uniform_disjoint_rows gave, the switch is not read a second time)
  char const *uniform_env = std::getenv("MFMG_MF_UNIFORM_SWEEP");
  const bool uniform_off = wg12 ? !disjoint_rows : (uniform_env && std::string(uniform_env) == "0");
  // (every tile shape of the three-term sweep has the stencil: the results of an operator do not depend on the shape asked for)
  bool uniform_taken = false;
  if constexpr (std::is_same<T, double>::value)
    if (_uniform && modes && !uniform_off && n_terms == 3 && dbg == 0)
    {
      MfUniformArgs<T> u{};
      u.x = a.x;
      u.b = a.b;
      u.out = a.out;
      u.out_prev = a.out_prev;
      u.Nx = a.Nx;
      u.Ny = a.Ny;
      u.Nz = a.Nz;
      u.ncols = a.ncols;
      u.ntiles_y = a.ntiles_y;
      u.ntiles_z = a.ntiles_z;
      u.own = a.own;
      u.halo = a.halo;
      u.TZ = a.TZ;
      double f[3];
      MfArgs<T> fa{};
      mf_cell_factors(fa, _h, f); // (kd as the other kernels get it)
      const double c = _uniform_coef;
      u.q[0] = 4. * f[1] * c / 3.;
      u.q[1] = -2. * f[1] * c / 3.;
      u.q[2] = 8. * f[0] * c / 3.;
      u.q[3] = 2. * f[0] * c / 3.;
      u.z[0] = 4. * f[2] * c / 9.;
      u.z[1] = 4. / 3.;
      u.z[2] = -2. * f[2] * c / 9.;
      u.z[3] = 1. / 3.;
      // D^-1 of a free DoF as the other kernels derive it: 1 / (kd * the sum of the eight cell coefficients)
      const double dinv = 1. / (fa.kd * (8. * c));
      for (int s = 0; s < 3; ++s)
      {
        u.alpha[s] = a.alpha[s];
        u.beta[s] = a.beta[s];
        u.bd[s] = a.beta[s] * dinv;
      }
      u.aff = a.aff;
      u.vec_bytes = a.vec_bytes;
      // (the narrow pairing of a last chunk column: the twelve-wavefront kernel alone carries that body)
      u.ntiles_y2 = wg12 ? a.ntiles_y2 : 0u;
      u.wide_tiles = wg12 ? a.wide_tiles : a.ncols * a.ntiles_y * a.ntiles_z;
      const unsigned int n_blocks_u = mf_xcd_grid((uint64_t)u.wide_tiles + (uint64_t)u.ntiles_y2 * a.ntiles_z);
      const size_t lds_u = ((size_t)nw * ring_planes(3, true) * (ty + 1) + (size_t)2 * nw * (ty == 2 && !wg12 ? 2 : 4)) * 64 * sizeof(T);
      ASSERT_THROW(lds_u <= kMfMaxLds, "tile of the multi-term sweep too large for the LDS");
      auto go_u = [&](auto kernel) { mf_launch(kernel, MfGrid{n_blocks_u, nw, lds_u, st}, u); };
      if (wg12)
        with_flag(narrow, [&](auto nt) {
          constexpr bool NT = decltype(nt)::value;
          if (zero_guess)
            go_u(mf_cheb_fused_uniform_kernel<T, NT, true>);
          else
            go_u(mf_cheb_fused_uniform_kernel<T, NT, false>);
        });
      else if (ty == 3 && zero_guess)
        go_u(mf_cheb_fused_uniform_rows_kernel<T, 3, true>); // (fused_zero_guess_available: three rows)
      else
        with_tile_rows<4>(ty, [&](auto tt) { go_u(mf_cheb_fused_uniform_rows_kernel<T, decltype(tt)::value, false>); });
      ++_uniform_sweeps;
      uniform_taken = true;
    }
  // (timing experiments, FP64: the kernels without barrier / without division)
  if (uniform_taken)
    ;
  else if (wg12)
  {
    // (one launch also where the narrow tiles are asked to be split off: the shape has no kernels of one body)
    if constexpr (std::is_same<T, double>::value)
      with_flag(narrow, [&](auto nt) {
        constexpr bool NT = decltype(nt)::value;
        // D^-1 from the operator's vector where it has one (sweep_diagonal_inverse) and set_sweep_diagonal has not said otherwise
        if (_sweep_dinv_read)
        {
          auto go_d = [&](auto kernel) { mf_launch(kernel, MfGrid{n_blocks, nw, lds, st}, a, _sweep_dinv.data()); };
          if (!modes)
            go_d(mf_cheb_fused_wg12d_kernel<T, false, false, false>);
          else if (zero_guess)
            go_d(mf_cheb_fused_wg12d_kernel<T, true, NT, true>);
          else
            go_d(mf_cheb_fused_wg12d_kernel<T, true, NT, false>);
        }
        else if (!modes)
          go(mf_cheb_fused_wg12_kernel<T, false, false, false>, n_blocks);
        else if (zero_guess)
          go(mf_cheb_fused_wg12_kernel<T, true, NT, true>, n_blocks);
        else
          go(mf_cheb_fused_wg12_kernel<T, true, NT, false>, n_blocks);
      });
  }
  else if (dbg > 0 && !zero_guess && n_terms == 3 && ty == 3 && !_dinv_in_record && std::is_same<T, double>::value)
    with_flag(dbg == 1, [&](auto one) { go(mf_cheb_fused_kernel<T, 3, 3, false, true, decltype(one)::value ? 1 : 2>, n_blocks); });
  else
    with_terms(n_terms, [&](auto kt) {
      with_tile_rows<4>(ty, [&](auto tt) {
        with_flag(_dinv_in_record, [&](auto dt) { with_flag(modes, [&](auto mt) { sweep(kt, tt, dt, mt); }); });
      });
    });
  MFMG_HIP_CHECK(hipGetLastError());
  KernelProfiler::end(stop, st);
}

template bool MatrixFreeLaplaceDevice<double>::fused_zero_guess_available(int) const;
template bool MatrixFreeLaplaceDevice<float>::fused_zero_guess_available(int) const;
template bool MatrixFreeLaplaceDevice<double>::fused_sweep_available(int) const;
template bool MatrixFreeLaplaceDevice<float>::fused_sweep_available(int) const;
template bool MatrixFreeLaplaceDevice<double>::fused_wg12_capable(int) const;
template bool MatrixFreeLaplaceDevice<float>::fused_wg12_capable(int) const;
template bool MatrixFreeLaplaceDevice<double>::uniform_disjoint_rows(int, int, int) const;
template bool MatrixFreeLaplaceDevice<float>::uniform_disjoint_rows(int, int, int) const;
template int MatrixFreeLaplaceDevice<double>::fused_tile_owned_rows(int, int, int) const;
template int MatrixFreeLaplaceDevice<float>::fused_tile_owned_rows(int, int, int) const;
template void MatrixFreeLaplaceDevice<double>::choose_fused_tile(int, int &, int &, int &) const;
template void MatrixFreeLaplaceDevice<float>::choose_fused_tile(int, int &, int &, int &) const;
template void MatrixFreeLaplaceDevice<double>::smoother_sweep(int, double const *, double const *, double const *, double const *, double *,
                                                               double *) const;
template void MatrixFreeLaplaceDevice<float>::smoother_sweep(int, float const *, float const *, float const *, float const *, float *, float *) const;
} // namespace mfmg
