// Stand-alone check of mf_z_tiles (mf_z_tiles.hpp, the z-tiling of the matrix-free operator): plain C++, no HIP, no GPU.
//   make check-z-tiles          builds it with -fsanitize=address,undefined and runs the sweep
//   mf_z_tiles_check            the sweep: every n_layers in 1 .. 2100, tz in 1 .. 64, graded or not, m_extra in -1 .. 2
//   mf_z_tiles_check n tz graded m_extra w_off     prints that table (tests/test_mf_z_tiles.py reads the tables of m_extra <= 0)
// The sweep holds: the tiles partition [0, n_layers) with no empty tile (so never zero tiles); m < 1 gives the uniform table;
// the default knobs give 8 m tiles where graded and ceil(n / tz) otherwise; n_layers < 1 and tz < 1 throw.
#include "mf_z_tiles.hpp"

#include <cstdio>
#include <cstdlib>

namespace
{
int failures = 0;

void fail(char const *what, int n, int tz, int graded, int m_extra, double w_off)
{
  if (++failures <= 20)
    std::fprintf(stderr, "FAILED %s: n_layers %d tz %d graded %d m_extra %d w_off %g\n", what, n, tz, graded, m_extra, w_off);
}

bool is_partition(std::vector<int> const &tab, int n)
{
  if (tab.size() < 2 || tab.front() != 0 || tab.back() != n)
    return false;
  for (size_t t = 0; t + 1 < tab.size(); ++t)
    if (tab[t + 1] <= tab[t])
      return false;
  return true;
}

template <typename F>
bool throws(F &&f)
{
  try
  {
    f();
  }
  catch (std::invalid_argument const &)
  {
    return true;
  }
  return false;
}
} // namespace

int main(int argc, char **argv)
{
  using mfmg::mf_z_tiles;
  if (argc == 6)
  {
    for (int v : mf_z_tiles(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]) != 0, std::atoi(argv[4]), std::atof(argv[5])))
      std::printf("%d ", v);
    std::printf("\n");
    return 0;
  }
  long tables = 0, graded_tables = 0, fell_back = 0;
  for (int n = 1; n <= 2100; ++n)
    for (int tz = 1; tz <= 64; ++tz)
    {
      const std::vector<int> uniform = mf_z_tiles(n, tz, false);
      if (!is_partition(uniform, n) || (int)uniform.size() - 1 != (n + tz - 1) / tz)
        fail("uniform table", n, tz, 0, 1, 0.5);
      for (int m_extra = -1; m_extra <= 2; ++m_extra)
      {
        // (false with any knob: the uniform table)
        if (mf_z_tiles(n, tz, false, m_extra) != uniform)
          fail("knob changes the uniform table", n, tz, 0, m_extra, 0.5);
        const std::vector<int> tab = mf_z_tiles(n, tz, true, m_extra);
        ++tables;
        if (!is_partition(tab, n))
          fail("no partition", n, tz, 1, m_extra, 0.5);
        const int m = (n / 8 + tz / 2) / tz + m_extra;
        const bool grades = m >= 1 && n / 8 >= 2 * m;
        if (grades ? (int)tab.size() - 1 != 8 * m : tab != uniform)
          fail(grades ? "tile count where graded" : "not uniform where not graded", n, tz, 1, m_extra, 0.5);
        graded_tables += grades;
        fell_back += m < 1;
      }
    }
  // weights far from the default: still partitions (zero, negative and non-finite weights and totals)
  const double offs[] = {-1e300, -7.5, -2., -1.5, -1., -0.5, 0., 0.25, 3., 1e300, HUGE_VAL, -HUGE_VAL, std::nan("")};
  for (double w_off : offs)
    for (int n : {16, 33, 57, 97, 159, 257, 2100})
      for (int tz : {1, 3, 4, 8, 64})
        for (int m_extra = -1; m_extra <= 2; ++m_extra)
          if (!is_partition(mf_z_tiles(n, tz, true, m_extra, w_off), n))
            fail("no partition", n, tz, 1, m_extra, w_off);
  // sizes at the end of the range of int
  for (int n : {2147483647, 2147483640})
    for (int tz : {2147483647, 1073741824, 268435456})
      if (!is_partition(mf_z_tiles(n, tz, true), n) || !is_partition(mf_z_tiles(n, tz, false), n))
        fail("no partition", n, tz, 1, 1, 0.5);
  for (int g = 0; g < 2; ++g)
    if (!throws([&] { mf_z_tiles(0, 4, g != 0); }) || !throws([&] { mf_z_tiles(-3, 4, g != 0); }) || !throws([&] { mf_z_tiles(17, 0, g != 0); }) ||
        !throws([&] { mf_z_tiles(17, -2, g != 0); }))
      fail("no exception", 0, 0, g, 1, 0.5);
  if (mf_z_tiles(17, 8, true, 0) != std::vector<int>{0, 8, 16, 17}) // (was [17] alone: a launch of zero tiles)
    fail("17 layers, tz = 8, m_extra = 0", 17, 8, 1, 0, 0.5);
  std::printf("%ld tables with graded asked for: %ld graded, %ld with m < 1 uniform; %d failures\n", tables, graded_tables, fell_back, failures);
  return failures ? 1 : 0;
}
