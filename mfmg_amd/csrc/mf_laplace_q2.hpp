// Matrix-free Q2 Laplace operator on a structured hex mesh, device resident (FP64, 3-D, one rank).
//
// The arithmetic of LaplaceOperator::local_apply / compute_diagonal of the reference (tests/laplace_matrix_free.hpp:75-98,
// 129-156, 158-199) for FE_Q(2) with QGauss(3): per cell the gradients at the 27 quadrature points by sum factorisation with
// the two 3 x 3 one-dimensional tables (value and derivative of the Lagrange polynomials on {0, 1/2, 1} at the Gauss points),
// times coefficient * JxW / h_d^2, then the transposed contraction.  Constrained rows return y_c = x_c and constrained entries
// of x contribute nothing to other rows: the semantics of the Q1 kernel (mf_laplace.hpp).
//
// Unknowns sit on the lattice N[d] = 2 n[d] + 1, numbered lexicographically with x fastest; no other numbering is taken.
// coefficient[cell][27] at the points q = qa + 3 qb + 9 qc of QGauss<1>(3)^3, cells x-fastest.
//
// Refused at construction: dim != 3 (NotImplementedExc), a context with a communicator (NotImplementedExc), n_dofs >= 2^31 or
// n_dofs != prod(2 n[d] + 1) (InvalidArgumentExc).  There is no FP32 instance and no block form (the class is not a template
// of the scalar; the C boundary has no such entry points).
#pragma once

#include "common.hpp"
#include "mf_laplace.hpp"

namespace mfmg
{
// What the C boundary hands over (include/mfmg_hip.h: mfmg_hip_q2_mesh_desc)
struct Q2MeshDesc
{
  int dim;
  int n_cells[3];
  double cell_size[3];
  int64_t n_dofs;
  double const *coefficient;    // [n_cells_total][27]
  uint8_t const *constrained;   // [n_dofs]
  bool arrays_on_device;
};

// Tile of one workgroup in cells, halo cells of the low faces included in the lanes: cx x cy lanes (one cell each) own the nodes
// of (cx - 1) x (cy - 1) cells per layer and march over tz owned cell layers after the halo layer below them.
struct Q2Tile
{
  int cx, cy, tz;
  int tx() const { return cx - 1; }
  int ty() const { return cy - 1; }
};

// the tile shapes the launch path offers (shape 0 is the default); all give the same bits
constexpr int kQ2TileShapes = 3;
constexpr Q2Tile kQ2Tiles[kQ2TileShapes] = {{16, 8, 4}, {8, 8, 8}, {16, 8, 8}};

template <typename T>
class MatrixFreeLaplaceQ2Device;

template <>
class MatrixFreeLaplaceQ2Device<double>
{
public:
  using T = double;
  // allow_compact: keep ONE coefficient per cell when the 27 quadrature values of every cell are equal (detected on the device)
  MatrixFreeLaplaceQ2Device(HipHandle &handle, Q2MeshDesc const &mesh, bool allow_compact = true);

  bool cell_constant_layout() const { return _compact; }
  int64_t n_dofs() const { return _n_dofs; }
  int dof_grid(int d) const { return _N[d]; }
  int n_cells(int d) const { return _n[d]; }
  double cell_size(int d) const { return _h[d]; }
  HipHandle &handle() const { return _handle; }

  void vmult(T const *x, T *y) const { launch(MfMode::apply, {x, nullptr, nullptr, T(0), T(0), y}); }
  void residual(T const *x, T const *b, T *res) const { launch(MfMode::residual, {x, b, nullptr, T(0), T(0), res}); }
  // out = x + alpha (x - x_prev) - beta dinv (A x - b); out must not alias x, out may be x_prev
  void smoother_step(T const *b, T const *x, T const *x_prev, T alpha, T beta, T *out) const
  {
    launch(mf_smoother_mode(x_prev, alpha), {x, b, x_prev, alpha, beta, out});
  }
  void launch(MfMode mode, MfOperands<T> const &v) const;

  T const *diagonal() const { return _diag.data(); }
  T const *diagonal_inverse() const { return _dinv.data(); }

  // shape: index into kQ2Tiles (-1: the default)
  void set_tile(int shape);
  Q2Tile get_tile() const { return kQ2Tiles[_shape]; }

  // bytes one application must move at least: x, y, 27 or 1 coefficients per cell, one flag byte per unknown
  double required_bytes_apply() const
  {
    const double cells = double(_n[0]) * _n[1] * _n[2];
    return double(_n_dofs) * (2. * sizeof(T) + 1.) + cells * (_compact ? 1. : 27.) * sizeof(T);
  }

private:
  HipHandle &_handle;
  int _N[3], _n[3];
  double _h[3];
  int64_t _n_dofs;
  bool _compact = false;
  int _shape = 0;
  DeviceBuffer<T> _coef;            // [cells][27], or [cells] in the cell-constant layout
  DeviceBuffer<uint8_t> _constrained;
  DeviceBuffer<T> _diag, _dinv;
};
} // namespace mfmg
