// The z-tiling of the matrix-free operator as a pure host function: no HIP header, no state, so a plain C++ program can
// compile it and a test can read every table without a GPU (MatrixFreeLaplaceDevice<T>::z_tiling uploads what it returns).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace mfmg
{
// Tile starts of n_layers DoF layers followed by n_layers: z-tile t owns the layers [tab[t], tab[t + 1]).
//
// Uniform: tile t owns [t tz, (t + 1) tz), ceil(n_layers / tz) tiles.
//
// Graded (asked for with graded = true and taken when every eighth of the layers holds at least 2 m layers,
// m = (n_layers / 8 + tz / 2) / tz + m_extra the z-tiles per eighth): the eighth s owns [s n / 8, (s + 1) n / 8), cut into m
// tiles whose heights fall off linearly -- the weights are m - k + w_off, k = 0 .. m - 1; every cut is the rounded (half away
// from zero) share of the cumulative weight, clamped so that every tile keeps at least one layer.  8 m tiles.  Heights:
//   257 layers, tz = 8: 10, 8, 7, 4, 3 seven times, then 10, 9, 6, 5, 3 (the last eighth has 33 layers)
//    33 layers, tz = 4: 3, 1 seven times, then 3, 2
//
// What the function does with arguments no table exists for:
//   - n_layers < 1 or tz < 1 throws std::invalid_argument (there is no uniform table to fall back to);
//   - m < 1 (m_extra, the experiment knob, at 0 or below on a short mesh) falls back to the uniform table.
// So a table for n_layers >= 1 always has at least one tile, and its tiles always partition [0, n_layers).
inline std::vector<int> mf_z_tiles(int n_layers, int tz, bool graded, int m_extra = 1, double w_off = 0.5)
{
  if (n_layers < 1 || tz < 1)
    throw std::invalid_argument("z-tiling: at least one layer and a tile height of at least 1");
  std::vector<int> tab;
  const int Nz = n_layers;
  const int64_t m64 = (int64_t)(Nz / 8 + tz / 2) / tz + m_extra; // z-tiles per XCD
  if (graded && m64 >= 1 && Nz / 8 >= 2 * m64)
  {
    const int m = (int)m64;
    double total = 0.;
    for (int k = 0; k < m; ++k)
      total += m - k + w_off;
    for (int s = 0; s < 8; ++s)
    {
      const int l0 = (int)((int64_t)s * Nz / 8), l1 = (int)((int64_t)(s + 1) * Nz / 8);
      double cum = 0.;
      int prev = l0;
      for (int k = 0; k < m; ++k)
      {
        tab.push_back(prev);
        cum += m - k + w_off;
        // (a share outside [0, l1 - l0] or not a number -- only a w_off far from its default gives one -- is brought into
        // that range before it is rounded; the clamp below would bring it there anyway)
        const double share = (l1 - l0) * cum / total;
        const double cut = share >= 0. ? std::min(share, (double)(l1 - l0)) : 0.;
        int next = k + 1 == m ? l1 : l0 + (int)std::lround(cut);
        next = std::min(std::max(next, prev + 1), l1 - (m - 1 - k)); // every tile owns at least one layer
        prev = next;
      }
    }
    tab.push_back(Nz);
  }
  else
  {
    for (int64_t l = 0; l < Nz; l += tz)
      tab.push_back((int)l);
    tab.push_back(Nz);
  }
  return tab;
}
} // namespace mfmg
