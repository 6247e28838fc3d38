// Stand-alone check of FgmresColumn (fgmres_column.hpp, the host arithmetic of both flexible GMRES drivers): plain C++, no HIP,
// no GPU.
//   make check-fgmres-column    builds it with -fsanitize=address,undefined and runs it
// The recurrence -- the earlier rotations on the new Hessenberg column, the new rotation from hypot, the rotated right-hand side --
// is restated in long double; the restatement and FgmresColumn get the same columns.  Held, with eps = 2^-52 and m the columns of
// the object (the backward error of Givens QR with a generous constant; nothing here is measured):
//   every value of rotate() differs from the long double one by at most 32 m eps |g_0|;
//   after solve(), || g_0 e_1 - H y || recomputed in long double from the UNROTATED columns differs from the last value of
//   rotate() by at most 32 m eps (||H||_F ||y|| + |g_0|).
// Cases: random columns for m = 1, 2, 3, 8; a cycle cut short at k < m; two cycles on one object (begin_cycle resets k, g and
// breakdown: the second cycle has the bits of a fresh object); h_{j+1,j} = 0 exactly with d != 0 and with d = 0 (breakdown is set,
// cs = 1 and sn = 0 where d = 0, no NaN); an exactly zero pivot (y_i = 0 there, every y finite).
// A zero pivot makes the triangular system singular: row i reads 0 y_i + sum_l R_il y_l = g_i and is met only if it happens to
// be.  After an exact breakdown it is (g_i = 0 from there on), and the second bound is held as it stands.  With g_i != 0 the
// least-squares residual is NOT the last value of rotate() -- the drivers know: "a breakdown is not taken at its word", they
// recompute the residual -- and what is held there is the residual the rows left unmet give, || g - R y || of the object's own
// rotated system, to the same bound.
#include "fgmres_column.hpp"

#include <cstdint>
#include <cstdio>

namespace
{
using mfmg::FgmresColumn;
typedef long double real;

int failures = 0;
long checks = 0;

void fail(char const *what, char const *name, int m, int j, double got, double want, double bound)
{
  if (++failures <= 20)
    std::fprintf(stderr, "FAILED %s: case %s m %d column %d: %.17g against %.17g, bound %.3g\n", what, name, m, j, got, want, bound);
}

const double eps = std::ldexp(1., -52);

struct Random
{
  uint64_t state;
  double next() // in (-1, 1)
  {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(state >> 11) + 0.5) / 4503599627370496. - 1.;
  }
};

// the recurrence of FgmresColumn::rotate, restated
struct Restated
{
  int m;
  std::vector<real> R, cs, sn, g;
  int k = 0;
  Restated(int m, double residual) : m(m), R((size_t)(m + 1) * m), cs(m), sn(m), g(m + 1, 0.)
  {
    g[0] = residual;
  }
  real rotate(std::vector<double> const &h)
  {
    const int j = k;
    real *const c = &R[(size_t)j * (m + 1)];
    for (int i = 0; i <= j + 1; ++i)
      c[i] = h[i];
    for (int i = 0; i < j; ++i)
    {
      const real t = cs[i] * c[i] + sn[i] * c[i + 1];
      c[i + 1] = -sn[i] * c[i] + cs[i] * c[i + 1];
      c[i] = t;
    }
    const real d = hypotl(c[j], c[j + 1]);
    cs[j] = d > 0 ? c[j] / d : 1;
    sn[j] = d > 0 ? c[j + 1] / d : 0;
    c[j] = d;
    c[j + 1] = 0;
    g[j + 1] = -sn[j] * g[j];
    g[j] = cs[j] * g[j];
    ++k;
    return fabsl(g[j + 1]);
  }
};

typedef std::vector<std::vector<double>> Columns; // column j: h_0 .. h_{j+1}

Columns random_columns(Random &rng, int k)
{
  Columns H(k);
  for (int j = 0; j < k; ++j)
  {
    H[j].resize(j + 2);
    for (int i = 0; i <= j; ++i)
      H[j][i] = rng.next();
    H[j][j + 1] = 0.5 * (rng.next() + 1.); // a norm: positive
  }
  return H;
}

bool finite(std::vector<double> const &v)
{
  for (double x : v)
    if (!std::isfinite(x))
      return false;
  return true;
}

// One cycle of H.size() columns on `col` from the residual g0: every rotate() against the restatement, then solve() against the
// residual in long double.  `unmet` is for a system with a zero pivot whose right-hand side is not zero there (see the head of
// the file).  Returns the values of rotate() and y behind them.
std::vector<double> run_cycle(char const *name, FgmresColumn &col, double g0, Columns const &H, bool unmet = false)
{
  const int m = col.m, k = (int)H.size();
  Restated ref(m, g0);
  col.begin_cycle(g0);
  std::vector<double> out;
  double last = std::abs(g0);
  for (int j = 0; j < k; ++j)
  {
    std::copy(H[j].begin(), H[j].end(), col.column(j));
    last = col.rotate();
    const real want = ref.rotate(H[j]);
    const double bound = 32. * m * eps * std::abs(g0);
    ++checks;
    if (!(fabsl(last - want) <= bound))
      fail("rotate()", name, m, j, last, (double)want, bound);
    if (col.breakdown != (H[j][j + 1] == 0.))
      fail("breakdown flag", name, m, j, col.breakdown, H[j][j + 1] == 0., 0.);
    out.push_back(last);
  }
  if (col.k != k)
    fail("column count", name, m, k, col.k, k, 0.);
  std::vector<double> y(m, std::nan(""));
  col.solve(y.data());
  y.resize(k);
  if (!finite(y) || !finite(col.R) || !finite(col.cs) || !finite(col.sn) || !finite(col.g))
    fail("a value that is not finite", name, m, k, 0., 0., 0.);
  real norm_h = 0, norm_y = 0, residual = 0;
  for (int i = 0; i <= k; ++i)
  {
    real r = i == 0 ? g0 : 0;
    for (int j = std::max(0, i - 1); j < k; ++j)
      r -= (real)H[j][i] * y[j];
    residual += r * r;
  }
  for (int j = 0; j < k; ++j)
  {
    norm_y += (real)y[j] * y[j];
    for (double h : H[j])
      norm_h += (real)h * h;
  }
  real want = last;
  if (unmet)
  {
    // || g - R y || over the k + 1 rows of the object's rotated system
    want = 0;
    for (int i = 0; i <= k; ++i)
    {
      real r = col.g[i];
      for (int j = i; j < k; ++j)
        r -= (real)col.R[(size_t)j * (m + 1) + i] * y[j];
      want += r * r;
    }
    want = sqrtl(want);
  }
  const double bound = 32. * m * eps * (double)(sqrtl(norm_h) * sqrtl(norm_y) + fabsl(g0));
  ++checks;
  if (!(fabsl(sqrtl(residual) - want) <= bound))
    fail("least-squares residual", name, m, k, (double)sqrtl(residual), (double)want, bound);
  out.insert(out.end(), y.begin(), y.end());
  return out;
}
} // namespace

int main()
{
  Random rng{20240229};
  // random columns, the whole cycle
  for (int m : {1, 2, 3, 8})
    for (int trial = 0; trial < 200; ++trial)
    {
      FgmresColumn col(m);
      const double g0 = (trial % 2 ? 1e-7 : 3.) * (rng.next() + 1.5);
      run_cycle("random", col, g0, random_columns(rng, m));
    }
  // a cycle cut short
  for (int trial = 0; trial < 200; ++trial)
    for (int k = 1; k < 8; ++k)
    {
      FgmresColumn col(8);
      run_cycle("cut short", col, rng.next() + 1.5, random_columns(rng, k));
    }
  // two cycles on one object: the first one full and ended by a breakdown, so that k, every g and the flag are set
  for (int trial = 0; trial < 200; ++trial)
  {
    const int m = 8, k2 = 1 + trial % m;
    Columns first = random_columns(rng, m);
    first[m - 1][m] = 0.;
    const Columns second = random_columns(rng, k2);
    const double g0 = rng.next() + 1.5;
    FgmresColumn used(m), fresh(m);
    run_cycle("first of two cycles", used, 7. * g0, first);
    if (!used.breakdown || used.k != m)
      fail("the first cycle ends by a breakdown", "two cycles", m, m, used.breakdown, 1., 0.);
    used.begin_cycle(g0);
    bool reset = used.k == 0 && !used.breakdown && used.g[0] == g0;
    for (int i = 1; i <= m; ++i)
      reset = reset && used.g[i] == 0.;
    if (!reset)
      fail("begin_cycle resets k, g and breakdown", "two cycles", m, 0, 0., 1., 0.);
    if (run_cycle("second of two cycles", used, g0, second) != run_cycle("fresh object", fresh, g0, second))
      fail("the second cycle has the bits of a fresh object", "two cycles", m, k2, 0., 1., 0.);
  }
  // h_{j+1,j} = 0 exactly, the diagonal entry not zero after the rotations: breakdown, the residual of the cycle is zero
  for (int m : {1, 2, 3, 8})
    for (int j = 0; j < m; ++j)
    {
      Columns H = random_columns(rng, j + 1);
      H[j][j + 1] = 0.;
      FgmresColumn col(m);
      const std::vector<double> out = run_cycle("zero subdiagonal", col, rng.next() + 1.5, H);
      if (!col.breakdown || out[j] != 0. || col.sn[j] != 0. || std::abs(col.cs[j]) != 1.)
        fail("zero subdiagonal: breakdown, sn = 0, |cs| = 1, residual 0", "zero subdiagonal", m, j, out[j], 0., 0.);
    }
  // ... and with d = 0, a whole column of zeros: cs = 1, sn = 0, a zero pivot with g_j != 0 (the first column; `unmet`) ...
  for (int m : {1, 2, 3, 8})
    for (int j = 0; j < m; ++j)
    {
      Columns H = random_columns(rng, m);
      std::fill(H[j].begin(), H[j].end(), 0.);
      FgmresColumn col(m);
      const std::vector<double> out = run_cycle("zero column", col, rng.next() + 1.5, H, true);
      if (col.cs[j] != 1. || col.sn[j] != 0. || col.R[(size_t)j * (m + 1) + j] != 0.)
        fail("zero column: cs = 1, sn = 0, pivot 0", "zero column", m, j, col.cs[j], 1., 0.);
      if (out[m + j] != 0.)
        fail("zero pivot: y = 0 there", "zero column", m, j, out[m + j], 0., 0.);
    }
  // ... and a zero pivot after an exact breakdown: column j - 1 ends the Krylov space (g_j = 0), column j has entries in the rows
  // 0 .. j - 1 alone, which the rotations leave there (sn_{j-1} = 0): R_jj = 0, and the system is met with y_j = 0
  for (int m : {2, 3, 8})
    for (int j = 1; j < m; ++j)
    {
      Columns H = random_columns(rng, m);
      H[j - 1][j] = 0.;
      H[j][j] = H[j][j + 1] = 0.;
      FgmresColumn col(m);
      const std::vector<double> out = run_cycle("zero pivot after a breakdown", col, rng.next() + 1.5, H);
      if (col.R[(size_t)j * (m + 1) + j] != 0. || col.cs[j] != 1. || col.sn[j] != 0.)
        fail("zero pivot after a breakdown: pivot 0, cs = 1, sn = 0", "zero pivot after a breakdown", m, j, col.R[(size_t)j * (m + 1) + j], 0., 0.);
      if (out[m + j] != 0.)
        fail("zero pivot: y = 0 there", "zero pivot after a breakdown", m, j, out[m + j], 0., 0.);
    }
  std::printf("%ld values held against long double; %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
