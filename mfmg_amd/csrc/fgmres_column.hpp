// The host arithmetic of flexible GMRES for ONE right-hand side, used by the one-vector and the block driver alike
// (krylov_drivers.cpp): the triangular factor of the Hessenberg matrix (column-major with m + 1 rows), the Givens rotations, the
// rotated right-hand side g, the breakdown flag and the back-substitution for y.  Plain C++, nothing of HIP: fgmres_column_check.cpp
// holds it against a restatement in long double on the CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace mfmg
{
struct FgmresColumn
{
  int m;
  std::vector<double> R, cs, sn, g;
  int k = 0; // columns of this cycle
  bool breakdown = false;
  explicit FgmresColumn(int m) : m(m), R((size_t)(m + 1) * m), cs(m), sn(m), g(m + 1) {}
  void begin_cycle(double residual)
  {
    std::fill(g.begin(), g.end(), 0.);
    g[0] = residual;
    k = 0;
    breakdown = false;
  }
  // where the caller puts h_0 .. h_j, ||w|| of step j
  double *column(int j) { return &R[(size_t)j * (m + 1)]; }
  // the column of step k goes through the rotations; returns |g_{k+1}|, the residual norm of the least-squares problem
  double rotate()
  {
    const int j = k;
    double *const c = column(j);
    for (int i = 0; i < j; ++i)
    {
      const double t = cs[i] * c[i] + sn[i] * c[i + 1];
      c[i + 1] = -sn[i] * c[i] + cs[i] * c[i + 1];
      c[i] = t;
    }
    // h_{j+1,j} = 0: the Krylov space is exhausted -- v_{j+1} is zero (basis_scale_store), the cycle ends with the update
    breakdown = c[j + 1] == 0.;
    const double d = std::hypot(c[j], c[j + 1]);
    cs[j] = d > 0. ? c[j] / d : 1.;
    sn[j] = d > 0. ? c[j + 1] / d : 0.;
    c[j] = d;
    c[j + 1] = 0.;
    g[j + 1] = -sn[j] * g[j];
    g[j] = cs[j] * g[j];
    ++k;
    return std::abs(g[j + 1]);
  }
  // R y = g over the k columns of this cycle (a zero pivot -- a singular Hessenberg matrix -- contributes nothing: no division by zero)
  void solve(double *y) const
  {
    for (int i = k - 1; i >= 0; --i)
    {
      double s = g[i];
      for (int l = i + 1; l < k; ++l)
        s -= R[(size_t)l * (m + 1) + i] * y[l];
      const double pivot = R[(size_t)i * (m + 1) + i];
      y[i] = pivot != 0. ? s / pivot : 0.;
    }
  }
};
} // namespace mfmg
