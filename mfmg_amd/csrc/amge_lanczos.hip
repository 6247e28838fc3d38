// The agglomerate eigenproblems of the spectral AMGe restrictor by a batched, matrix-free Lanczos method: one workgroup of four
// wavefronts per agglomerate, agglomerates of up to 729 nodes.
//
// Reference: the matrix-free back-end applies the agglomerate operator and runs Lanczos on it
// (include/mfmg/dealii/amge_host.templates.hpp:165-200,310-318, include/mfmg/common/lanczos.templates.hpp:83-503).  What is
// computed here is the `krylov` selection of build_restrictor_structured (amge_structured.cpp): one vector per distinct
// eigenvalue, the normalised projection of the start vector of DealIIMeshEvaluator::set_initial_guess onto the eigenspace --
// which is what a Lanczos run from that start vector converges to.
//
// The rule, per agglomerate (M: the matrix of the variant on the active DoFs, never formed):
//   q_1 = v0 / |v0|;  step j: w = M q_j - beta_{j-1} q_{j-1}, alpha_j = q_j . w, w -= alpha_j q_j, w orthogonalised against
//   q_1 .. q_j (classical Gram-Schmidt, two passes), beta_j = |w|; all q are kept.
//   The run ends after min(active DoFs, max_iterations) steps or at beta_j <= kLanczosBreakdown * max |theta(T_j)|.
//   T_j is examined at j = 1, whenever 100 (j - j_prev) > percent_overshoot * j_prev, at the last step and at a breakdown:
//   Ritz values ascending, grouped like the dense rule (|theta_i - theta_first| <= 1e-9 scale); the vector of a group is the
//   projection of v0 onto the span of its Ritz vectors, a group with a projection below 1e-12 |v0| is skipped; converged when
//   n_eig groups are selected and every Ritz pair of every group up to the last selected one has
//   beta_j |s_i[j]| <= tolerance * scale.
//
// Storage: the vectors of the recurrence, alpha / beta, the tridiagonal work arrays and the reductions live in LDS, indexed by
// LOCAL NODE (inactive nodes hold zeros, so no compaction is needed).  A slab of one scratch allocation per RESIDENT workgroup
// holds the 27 stencil coefficients per local node (expanded once from the cell coefficients and the Kq tables, sums over the
// cells in the order of the dense paths), the Lanczos basis Q and the eigenvectors Z of T_j.
// Tridiagonal method: implicit QL (tql2).  One thread generates the rotations of a QL iteration into LDS, then every thread
// applies them to the row of Z it owns; Z is stored column-major so that the rows of a wavefront are contiguous.  At most 30
// iterations per eigenvalue; an agglomerate that hits the cap is counted as unconverged.  The largest Ritz value of T_j for the
// breakdown test of every step comes from a 64-way multisection of the Gershgorin interval by Sturm counts (one wavefront).
// Every reduction has a fixed order (lane-strided partial sums, butterfly inside a wavefront, the four wavefronts in index
// order), so equal input gives equal bits whatever the workgroup: the sharing of solves between identical agglomerates
// (amge_device.hip) relies on that.  No workgroup waits for another; every loop has a bound known at launch.
#include "amge_lanczos.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>

namespace mfmg
{
namespace
{
constexpr int kThreads = 256;

struct LanczosArgs
{
  double tolerance;
  int max_iterations, percent_overshoot;
  int nmax;   // nodes of a full agglomerate: stride of the output
  int ld;     // leading dimension of the node-indexed slab arrays (>= nmax)
  int kmax;   // most steps of any agglomerate of the launch = columns of Q, order of Z
  double *slab;
  size_t slab_stride; // doubles per workgroup
  double *eigenvalues;
  int32_t *iterations, *flags;
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_xor(v, off);
  return v;
}

// sum over the workgroup, the same bits in every thread; red: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double *red)
{
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
    red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// number of eigenvalues of the tridiagonal (d[0..k), e[0..k-1)) below x
__device__ __forceinline__ int sturm_count(double const *d, double const *e, int k, double x, double tiny)
{
  int count = 0;
  double q = d[0] - x;
  if (q == 0.)
    q = -tiny;
  count += q < 0.;
  for (int i = 1; i < k; ++i)
  {
    q = (d[i] - x) - e[i - 1] * e[i - 1] / q;
    if (q == 0.)
      q = -tiny;
    count += q < 0.;
  }
  return count;
}

__global__ __launch_bounds__(kThreads) void amge_lanczos_kernel(AmgeArgs a, LanczosArgs p)
{
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv_id = tid >> 6;
  const int ld = p.ld, kp = p.kmax + 1;
  double *q_cur = smem;            // [ld]
  double *q_prev = q_cur + ld;     // [ld]
  double *w = q_prev + ld;         // [ld]
  double *dloc = w + ld;           // [ld]
  double *alpha = dloc + ld;       // [kp]
  double *beta = alpha + kp;       // [kp]  beta[j]: couples q_j and q_{j+1} (0-based)
  double *dd = beta + kp;          // [kp]  QL: diagonal -> eigenvalues
  double *ee = dd + kp;            // [kp]
  double *rc = ee + kp;            // [kp]  rotations of one QL iteration
  double *rs = rc + kp;            // [kp]
  double *coef = rs + kp;          // [kp]  Gram-Schmidt / group coefficients
  double *th = coef + kp;          // [kp]  Ritz values ascending
  double *red = th + kp;           // [8]
  int *perm = reinterpret_cast<int *>(red + 8); // [kp]  column of Z of the Ritz value of rank i
  int *ctl = perm + kp;                          // [8]
  unsigned char *act = reinterpret_cast<unsigned char *>(ctl + 8); // [ld]  1: DoF of the eigenproblem
  unsigned char *conf = act + ld;                                   // [ld]  1: constrained

  double *S = p.slab + (size_t)blockIdx.x * p.slab_stride; // [27][ld]
  double *Q = S + (size_t)27 * ld;                         // [kmax][ld]
  double *Z = Q + (size_t)p.kmax * ld;                     // [kmax][kmax], Z[col * zld + row]
  const int zld = p.kmax;
  const int dim = a.dim, nc = a.nc;

  for (int64_t slot = blockIdx.x; slot < a.n_agg; slot += gridDim.x)
  {
    const int64_t agg = a.list ? a.list[slot] : slot;
    int ai[3] = {(int)(agg % a.cnt[0]), (int)((agg / a.cnt[0]) % a.cnt[1]), (int)(agg / ((int64_t)a.cnt[0] * a.cnt[1]))};
    int lo[3] = {0, 0, 0}, ln[3] = {1, 1, 1}, lN[3] = {1, 1, 1};
    for (int d = 0; d < dim; ++d)
    {
      lo[d] = ai[d] * a.ag[d];
      ln[d] = min(a.ag[d], a.n[d] - lo[d]);
      lN[d] = ln[d] + 1;
    }
    if (dim == 2)
    {
      ln[2] = 1;
      lN[2] = 1;
    }
    const int nloc = lN[0] * lN[1] * lN[2]; // <= nmax <= ld
    const int lkz = (dim == 3) ? ln[2] : 1;
    __syncthreads(); // (the previous agglomerate of this workgroup is done with LDS)

    // ---- constraint flags
    for (int r = tid; r < nloc; r += kThreads)
    {
      const int ri = r % lN[0], rj = (r / lN[0]) % lN[1], rk = r / (lN[0] * lN[1]);
      const int64_t node = (lo[0] + ri) + (int64_t)a.N[0] * ((lo[1] + rj) + (int64_t)a.N[1] * ((dim == 3) ? lo[2] + rk : 0));
      const bool con = a.constrained[a.node_dof[node]] == 1;
      conf[r] = con ? 1 : 0;
      act[r] = (a.variant == 2 && con) ? 0 : 1;
    }
    __syncthreads();
    // ---- the 27 stencil coefficients of every local node: entries of the local Neumann matrix, cells in (k, j, i) order
    for (int r = tid; r < nloc; r += kThreads)
    {
      const int ri = r % lN[0], rj = (r / lN[0]) % lN[1], rk = r / (lN[0] * lN[1]);
      for (int o = 0; o < 27; ++o)
      {
        const int ci = ri + (o % 3) - 1, cj = rj + ((o / 3) % 3) - 1, ck = rk + (o / 9) - 1;
        double sum = 0.;
        if (ci >= 0 && ci < lN[0] && cj >= 0 && cj < lN[1] && ck >= 0 && ck < lN[2])
        {
          for (int k = max(max(rk, ck) - 1, 0); k <= min(min(rk, ck), lkz - 1); ++k)
            for (int j = max(max(rj, cj) - 1, 0); j <= min(min(rj, cj), ln[1] - 1); ++j)
              for (int i = max(max(ri, ci) - 1, 0); i <= min(min(ri, ci), ln[0] - 1); ++i)
              {
                const int m = (ri - i) + 2 * (rj - j) + ((dim == 3) ? 4 * (rk - k) : 0);
                const int mp = (ci - i) + 2 * (cj - j) + ((dim == 3) ? 4 * (ck - k) : 0);
                const int64_t cell = (lo[0] + i) + (int64_t)a.n[0] * ((lo[1] + j) + (int64_t)a.n[1] * ((dim == 3) ? lo[2] + k : 0));
                double v = 0.;
                for (int q = 0; q < nc; ++q)
                  v += (a.use_coefficient ? a.coefficient[cell * nc + q] : 1.) * a.Kq[((size_t)q * nc + m) * nc + mp];
                sum += v;
              }
        }
        S[(size_t)o * ld + r] = sum;
      }
      // diag_loc: constrained rows keep 1 ("mf") or the summed local diagonal
      const double full_diag = S[(size_t)13 * ld + r];
      dloc[r] = conf[r] ? ((a.variant == 2) ? 1. : full_diag) : full_diag;
    }
    __syncthreads();
    if (tid == 0)
    {
      // "host": mean of diag_loc, summed in index order like the host loop
      double avg = 0.;
      if (a.variant == 1)
      {
        for (int r = 0; r < nloc; ++r)
          avg += dloc[r];
        avg /= nloc;
      }
      red[4] = avg;
    }
    __syncthreads();
    const double shift = red[4];
    // ---- the matrix of the eigenproblem: constrained rows / columns eliminated
    for (int r = tid; r < nloc; r += kThreads)
    {
      const int ri = r % lN[0], rj = (r / lN[0]) % lN[1], rk = r / (lN[0] * lN[1]);
      for (int o = 0; o < 27; ++o)
      {
        const int ci = ri + (o % 3) - 1, cj = rj + ((o / 3) % 3) - 1, ck = rk + (o / 9) - 1;
        double v = S[(size_t)o * ld + r];
        if (!act[r])
          v = 0.;
        else if (o == 13)
          v = (a.variant == 1) ? (conf[r] ? 200. : dloc[r] + shift) : dloc[r];
        else if (ci >= 0 && ci < lN[0] && cj >= 0 && cj < lN[1] && ck >= 0 && ck < lN[2])
        {
          const int c = ci + lN[0] * (cj + lN[1] * ck);
          if (conf[r] || conf[c])
            v = 0.;
        }
        else
          v = 0.;
        S[(size_t)o * ld + r] = v;
      }
    }
    // ---- start vector: libstdc++ minstd_rand0 + uniform_real_distribution in deal.II's first-touch order of the patch, zero on
    //      constrained DoFs (which consume no random number); w marks the nodes seen
    for (int r = tid; r < ld; r += kThreads)
    {
      w[r] = -1.;
      q_prev[r] = 0.;
    }
    __syncthreads();
    if (tid == 0)
    {
      unsigned long long state = 1ull;
      for (int k = 0; k < lkz; ++k)
        for (int j = 0; j < ln[1]; ++j)
          for (int i = 0; i < ln[0]; ++i)
            for (int m = 0; m < nc; ++m)
            {
              const int l = (i + (m & 1)) + lN[0] * ((j + ((m >> 1) & 1)) + lN[1] * ((dim == 3) ? k + ((m >> 2) & 1) : 0));
              if (w[l] >= 0.)
                continue;
              double val = 0.;
              if (!conf[l])
              {
                const double R = 2147483646.0;
                state = (16807ull * state) % 2147483647ull;
                double s = (double)(state - 1);
                state = (16807ull * state) % 2147483647ull;
                s += (double)(state - 1) * R;
                val = s / (R * R);
                if (val >= 1.0)
                  val = 0.99999999999999988898; // nextafter(1, 0)
              }
              w[l] = val;
            }
    }
    __syncthreads();
    int na = 0;
    double v0n2 = 0.;
    {
      double part = 0.;
      int cnt_act = 0;
      for (int r = tid; r < nloc; r += kThreads)
        if (act[r])
        {
          part += w[r] * w[r];
          ++cnt_act;
        }
      v0n2 = block_sum(part, red);
      na = (int)block_sum((double)cnt_act, red);
    }
    const double v0n = sqrt(v0n2);
    const int ksteps = min(na, min(p.max_iterations, p.kmax));
    double *out = a.weights + (size_t)agg * a.n_eig * p.nmax;
    if (ksteps == 0 || !(v0n > 0.))
    {
      if (tid == 0)
      {
        a.n_vec[agg] = 0;
        p.iterations[agg] = 0;
        p.flags[agg] = kAmgeConverged;
      }
      continue;
    }
    for (int r = tid; r < nloc; r += kThreads)
    {
      const double v = act[r] ? w[r] / v0n : 0.;
      q_cur[r] = v;
      Q[r] = v;
    }
    __syncthreads();

    int k_prev = 0, k_done = 0, n_sel_final = 0;
    bool converged = false, broke = false, ql_failed = false;
    for (int j = 0; j < ksteps; ++j)
    {
      // ---- w = M q_j - beta_{j-1} q_{j-1}
      const double beta_prev = j > 0 ? beta[j - 1] : 0.;
      double part = 0.;
      for (int r = tid; r < nloc; r += kThreads)
      {
        const int ri = r % lN[0], rj = (r / lN[0]) % lN[1], rk = r / (lN[0] * lN[1]);
        double sum = 0.;
        for (int o = 0; o < 27; ++o)
        {
          const int ci = ri + (o % 3) - 1, cj = rj + ((o / 3) % 3) - 1, ck = rk + (o / 9) - 1;
          if (ci >= 0 && ci < lN[0] && cj >= 0 && cj < lN[1] && ck >= 0 && ck < lN[2])
            sum += S[(size_t)o * ld + r] * q_cur[ci + lN[0] * (cj + lN[1] * ck)];
        }
        sum -= beta_prev * q_prev[r];
        w[r] = sum;
        part += q_cur[r] * sum;
      }
      const double al = block_sum(part, red);
      for (int r = tid; r < nloc; r += kThreads)
        w[r] -= al * q_cur[r];
      // ---- classical Gram-Schmidt against q_0 .. q_j, twice
      for (int pass = 0; pass < 2; ++pass)
      {
        __syncthreads();
        for (int i = wv_id; i <= j; i += kThreads / 64)
        {
          double const *qi = Q + (size_t)i * ld;
          double dot = 0.;
          for (int r = lane; r < nloc; r += 64)
            dot += qi[r] * w[r];
          dot = wave_sum(dot);
          if (lane == 0)
            coef[i] = dot;
        }
        __syncthreads();
        for (int r = tid; r < nloc; r += kThreads)
        {
          double v = w[r];
          for (int i = 0; i <= j; ++i)
            v -= coef[i] * Q[(size_t)i * ld + r];
          w[r] = act[r] ? v : 0.;
        }
      }
      part = 0.;
      for (int r = tid; r < nloc; r += kThreads)
        part += w[r] * w[r];
      const double bt = sqrt(block_sum(part, red));
      if (tid == 0)
      {
        alpha[j] = al;
        beta[j] = bt;
      }
      __syncthreads();
      const int k = j + 1; // steps taken: T_k = tridiag(alpha[0..k), beta[0..k-1))
      k_done = k;
      // ---- largest Ritz value of T_k: multisection of the Gershgorin interval (wavefront 0)
      if (wv_id == 0)
      {
        double glo = alpha[0], ghi = alpha[0];
        for (int i = 0; i < k; ++i)
        {
          const double rad = (i > 0 ? fabs(beta[i - 1]) : 0.) + (i + 1 < k ? fabs(beta[i]) : 0.);
          glo = fmin(glo, alpha[i] - rad);
          ghi = fmax(ghi, alpha[i] + rad);
        }
        const double tiny = 1e-300 + 1e-30 * fmax(fabs(glo), fabs(ghi));
        ghi += 1e-12 * fmax(fabs(glo), fabs(ghi)) + 1e-300; // all k eigenvalues are below ghi
        for (int round = 0; round < 9; ++round)
        {
          const double x = glo + (ghi - glo) * ((lane + 1) / 65.);
          const int c = sturm_count(alpha, beta, k, x, tiny);
          const unsigned long long all_below = __ballot(c == k);
          const int first = all_below ? __ffsll((long long)all_below) - 1 : 64;
          const double new_hi = first < 64 ? __shfl(x, first) : ghi;
          const double new_lo = first > 0 ? __shfl(x, first - 1) : glo;
          glo = new_lo;
          ghi = new_hi;
        }
        if (lane == 0)
          red[5] = fmax(fabs(ghi), 1e-300);
      }
      __syncthreads();
      const double scale_k = red[5];
      broke = bt <= kLanczosBreakdown * scale_k;
      const bool last = (k == ksteps) || broke;
      const bool examine = last || k == 1 || 100 * (k - k_prev) > p.percent_overshoot * k_prev;
      if (examine)
      {
        k_prev = k;
        // ---- implicit QL on T_k with the eigenvectors accumulated in Z
        for (int e = tid; e < k * k; e += kThreads)
          Z[(size_t)(e / k) * zld + (e % k)] = (e / k == e % k) ? 1. : 0.;
        if (tid == 0)
        {
          for (int i = 0; i < k; ++i)
          {
            dd[i] = alpha[i];
            ee[i] = i + 1 < k ? beta[i] : 0.;
          }
          ctl[0] = 0; // l
          ctl[1] = 0; // iterations spent on this l
          ctl[4] = 0; // failed
        }
        __syncthreads();
        // at most 30 k iterations plus the k passes that find an eigenvalue converged
        for (int it = 0; it < 31 * k + 1; ++it)
        {
          if (tid == 0)
          {
            int l = ctl[0], iter = ctl[1];
            int m = l, hi_i = 0, lo_i = 0; // rotations rc / rs [lo_i, hi_i) to apply, from hi_i - 1 down
            while (l < k)
            {
              for (m = l; m < k - 1; ++m)
              {
                const double s = fabs(dd[m]) + fabs(dd[m + 1]);
                if (fabs(ee[m]) <= 2.220446049250313e-16 * s)
                  break;
              }
              if (m != l)
                break;
              ++l;
              iter = 0;
            }
            if (l >= k)
              ctl[2] = 2; // done
            else if (iter >= 30)
            {
              ctl[2] = 2;
              ctl[4] = 1;
            }
            else
            {
              ++iter;
              double g = (dd[l + 1] - dd[l]) / (2. * ee[l]);
              double r = hypot(g, 1.);
              g = dd[m] - dd[l] + ee[l] / (g + (g >= 0. ? fabs(r) : -fabs(r)));
              double s = 1., c = 1., pp = 0.;
              int i;
              for (i = m - 1; i >= l; --i)
              {
                double f = s * ee[i];
                const double b = c * ee[i];
                r = hypot(f, g);
                ee[i + 1] = r;
                if (r == 0.)
                {
                  dd[i + 1] -= pp;
                  ee[m] = 0.;
                  break;
                }
                s = f / r;
                c = g / r;
                g = dd[i + 1] - pp;
                r = (dd[i] - g) * s + 2. * c * b;
                pp = s * r;
                dd[i + 1] = g + pp;
                g = c * r - b;
                rc[i] = c;
                rs[i] = s;
              }
              hi_i = m;
              lo_i = i + 1;
              if (!(r == 0. && i >= l))
              {
                dd[l] -= pp;
                ee[l] = g;
                ee[m] = 0.;
              }
              ctl[2] = 1;
            }
            ctl[0] = l;
            ctl[1] = iter;
            ctl[5] = lo_i;
            ctl[6] = hi_i;
          }
          __syncthreads();
          const int what = ctl[2], lo_i = ctl[5], hi_i = ctl[6];
          if (what == 1)
            for (int row = tid; row < k; row += kThreads)
            {
              double hi_v = Z[(size_t)hi_i * zld + row];
              for (int i = hi_i - 1; i >= lo_i; --i)
              {
                const double lo_v = Z[(size_t)i * zld + row];
                Z[(size_t)(i + 1) * zld + row] = rs[i] * lo_v + rc[i] * hi_v;
                hi_v = rc[i] * lo_v - rs[i] * hi_v;
              }
              Z[(size_t)lo_i * zld + row] = hi_v;
            }
          __syncthreads();
          if (what == 2)
            break;
        }
        ql_failed = ctl[4] != 0;
        // ---- ascending Ritz values, ties in index order
        for (int x = tid; x < k; x += kThreads)
        {
          const double wx = dd[x];
          int rank = 0;
          for (int y = 0; y < k; ++y)
          {
            const double wy = dd[y];
            rank += (wy < wx || (wy == wx && y < x)) ? 1 : 0;
          }
          th[rank] = wx;
          perm[rank] = x;
        }
        __syncthreads();
        // ---- groups, projections of the start vector (|v0| s_i[0] on Ritz vector i), residuals beta_k |s_i[k-1]|
        if (tid == 0)
        {
          const double scale = fmax(fmax(fabs(th[0]), fabs(th[k - 1])), 1e-300);
          int n_sel = 0, i0 = 0;
          bool ok = true;
          while (i0 < k && n_sel < a.n_eig)
          {
            int i1 = i0 + 1;
            while (i1 < k && fabs(th[i1] - th[i0]) <= 1e-9 * scale)
              ++i1;
            double wsum = 0.;
            for (int i = i0; i < i1; ++i)
            {
              const double s0 = Z[(size_t)perm[i] * zld], sk = Z[(size_t)perm[i] * zld + (k - 1)];
              wsum += s0 * s0;
              if (!(bt * fabs(sk) <= p.tolerance * scale))
                ok = false;
            }
            if (sqrt(wsum) > 1e-12)
              ++n_sel;
            i0 = i1;
          }
          ctl[3] = (ok && n_sel == a.n_eig && !ql_failed) ? 1 : 0;
        }
        __syncthreads();
        converged = ctl[3] != 0;
        if (converged || last)
          break;
      }
      // ---- q_{j+1} = w / beta_j
      for (int r = tid; r < nloc; r += kThreads)
      {
        const double v = w[r] / bt;
        q_prev[r] = q_cur[r];
        q_cur[r] = v;
        Q[(size_t)k * ld + r] = v;
      }
      __syncthreads();
    }
    // ---- the selected vectors: group by group as at the examination (every thread walks the groups)
    const int k = k_done;
    if (!ql_failed)
    {
      const double scale = fmax(fmax(fabs(th[0]), fabs(th[k - 1])), 1e-300);
      int i0 = 0;
      while (i0 < k && n_sel_final < a.n_eig)
      {
        int i1 = i0 + 1;
        while (i1 < k && fabs(th[i1] - th[i0]) <= 1e-9 * scale)
          ++i1;
        double wsum = 0., best = -1., theta = th[i0];
        for (int i = i0; i < i1; ++i)
        {
          const double s0 = Z[(size_t)perm[i] * zld];
          wsum += s0 * s0;
          if (fabs(s0) > best)
          {
            best = fabs(s0);
            theta = th[i]; // the Ritz value that carries the start vector (a copy grown out of rounding carries none)
          }
        }
        if (sqrt(wsum) > 1e-12)
        {
          __syncthreads();
          for (int t = tid; t < k; t += kThreads)
          {
            double c = 0.;
            for (int i = i0; i < i1; ++i)
              c += Z[(size_t)perm[i] * zld] * Z[(size_t)perm[i] * zld + t];
            coef[t] = c;
          }
          __syncthreads();
          double part = 0.;
          for (int r = tid; r < nloc; r += kThreads)
          {
            double v = 0.;
            for (int t = 0; t < k; ++t)
              v += coef[t] * Q[(size_t)t * ld + r];
            v = act[r] ? v : 0.;
            w[r] = v;
            part += v * v;
          }
          const double vn = sqrt(block_sum(part, red));
          for (int r = tid; r < nloc; r += kThreads)
            out[(size_t)n_sel_final * p.nmax + r] = act[r] ? dloc[r] * (w[r] / vn) : 0.;
          if (tid == 0)
            p.eigenvalues[(size_t)agg * a.n_eig + n_sel_final] = theta - shift;
          ++n_sel_final;
        }
        i0 = i1;
      }
    }
    if (tid == 0)
    {
      a.n_vec[agg] = n_sel_final;
      p.iterations[agg] = k;
      // a run through all active DoFs has the whole space: T is the matrix itself in the basis Q
      const bool complete = !ql_failed && (converged || broke || k == na);
      p.flags[agg] = (complete ? kAmgeConverged : 0) | (broke ? kAmgeBreakdown : 0);
    }
  }
}
} // namespace

bool amge_lanczos_supported(StructuredMesh const &mesh, RestrictorOptions const &opts)
{
  int64_t nloc = 1;
  for (int d = 0; d < mesh.dim; ++d)
    nloc *= (int64_t)std::min(opts.agglomerate[d], mesh.n[d]) + 1;
  return nloc <= kLanczosMaxNodes && (mesh.dim == 2 || mesh.dim == 3);
}

void amge_lanczos_eigen(HipHandle &handle, StructuredMesh const &mesh, RestrictorOptions const &opts, int const cnt[3],
                        std::vector<double> &weights, std::vector<int32_t> &n_vec, int &nmax, std::vector<double> &eigenvalues,
                        std::vector<int32_t> &iterations, std::vector<int32_t> &flags, int64_t *n_solves, double *kernel_seconds)
{
  ASSERT_THROW(opts.selection == "krylov", "the Lanczos eigensolver returns the krylov selection");
  ASSERT_THROW(opts.max_iterations >= 1, "eigensolver.max_iterations must be positive");
  ASSERT_THROW(opts.tolerance >= 0., "eigensolver.tolerance must not be negative");
  ASSERT_THROW(opts.percent_overshoot >= 0, "eigensolver.percent_overshoot must not be negative");
  if (!amge_lanczos_supported(mesh, opts))
    ASSERT_THROW_NOT_IMPLEMENTED("the Lanczos eigensolver takes agglomerates of at most 729 nodes");
  const int dim = mesh.dim;
  int nloc = 1;
  for (int d = 0; d < dim; ++d)
    nloc *= std::min(opts.agglomerate[d], mesh.n[d]) + 1;
  nmax = nloc;
  hipStream_t st = handle.stream;
  AmgeDeviceMesh d_mesh;
  AmgeArgs a = d_mesh.upload(handle, mesh, opts, cnt);
  const int64_t n_all = a.n_agg;
  DeviceBuffer<double> d_w((size_t)n_all * a.n_eig * nmax), d_ev((size_t)n_all * a.n_eig);
  DeviceBuffer<int32_t> d_nv((size_t)n_all), d_it((size_t)n_all), d_fl((size_t)n_all);
  MFMG_HIP_CHECK(hipMemsetAsync(d_w.data(), 0, d_w.size() * sizeof(double), st));
  MFMG_HIP_CHECK(hipMemsetAsync(d_ev.data(), 0, d_ev.size() * sizeof(double), st));
  a.weights = d_w.data();
  a.n_vec = d_nv.data();
  AmgeSharing sharing;
  sharing.find(handle, a);
  if (n_solves)
    *n_solves = a.n_agg;

  LanczosArgs p;
  p.tolerance = opts.tolerance;
  p.max_iterations = opts.max_iterations;
  p.percent_overshoot = opts.percent_overshoot;
  p.nmax = nmax;
  p.ld = (nmax + 7) / 8 * 8;
  p.kmax = std::min(opts.max_iterations, nmax);
  const int kp = p.kmax + 1;
  size_t lds = ((size_t)4 * p.ld + (size_t)8 * kp + 8) * sizeof(double) + ((size_t)kp + 8) * sizeof(int) + (size_t)2 * p.ld;
  lds = (lds + 15) / 16 * 16;
  ASSERT_THROW(lds <= 160 * 1024, "the Lanczos eigensolver does not fit the LDS");
  // the slab is sized by the workgroups that can be resident (LDS-limited, at most 4 per CU), not by the agglomerates
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / lds));
  const unsigned int blocks = (unsigned int)std::min<int64_t>(a.n_agg, (int64_t)256 * per_cu);
  p.slab_stride = ((size_t)27 * p.ld + (size_t)p.kmax * p.ld + (size_t)p.kmax * p.kmax + 1) / 2 * 2;
  DeviceBuffer<double> d_slab;
  {
    MemoryKind kind("Lanczos workspace");
    d_slab.resize(p.slab_stride * blocks);
  }
  p.slab = d_slab.data();
  p.eigenvalues = d_ev.data();
  p.iterations = d_it.data();
  p.flags = d_fl.data();
  MFMG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(amge_lanczos_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     160 * 1024));
  MFMG_HIP_CHECK(hipStreamSynchronize(st));
  const auto t0 = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(amge_lanczos_kernel, dim3(blocks), dim3(kThreads), lds, st, a, p);
  MFMG_HIP_CHECK(hipGetLastError());
  MFMG_HIP_CHECK(hipStreamSynchronize(st));
  if (kernel_seconds)
    *kernel_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  sharing.spread(handle, a.n_eig * nmax, d_w.data(), d_nv.data());
  sharing.spread(handle, a.n_eig, d_ev.data(), d_it.data());
  sharing.spread(handle, a.n_eig, d_ev.data(), d_fl.data());
  weights = d_w.download(st);
  n_vec = d_nv.download(st);
  eigenvalues = d_ev.download(st);
  iterations = d_it.download(st);
  flags = d_fl.download(st);
}
} // namespace mfmg
