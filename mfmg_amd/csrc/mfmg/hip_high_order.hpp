// Q2 elements on the refined Q1 cycle (low-order-refined preconditioning).
//
// For degree 2 the Lagrange nodes are equidistant: the Q2 unknowns on n cells are the Q1 unknowns on 2 n cells, in the same
// lexicographic lattice of (2 n + 1)^3 nodes, and the Q1 operator on that refined mesh is spectrally equivalent to the Q2
// operator.  HipQ2Operator puts the device operator of mf_laplace_q2.hpp behind the interface a HipSmoother drives;
// HighOrderPreconditioner wraps a Chebyshev smoother on it around one cycle of a Q1 hierarchy the caller built on the refined
// problem (the same lattice, h / 2, the same material; matrix-free evaluator, one rank, lexicographic numbering).
#pragma once

#include <memory>

#include "../mf_laplace_q2.hpp"
#include "hierarchy.hpp"

namespace mfmg
{
class HipQ2Operator : public HipOperator
{
public:
  explicit HipQ2Operator(std::shared_ptr<MatrixFreeLaplaceQ2Device<double>> op) : _op(std::move(op)) {}

  void apply(DVector const &x, DVector &y, OperatorMode mode = OperatorMode::NO_TRANS) const override;
  std::shared_ptr<Operator<DVector>> transpose() const override
  {
    ASSERT_THROW_NOT_IMPLEMENTED();
    return nullptr;
  }
  std::shared_ptr<Operator<DVector>> multiply(std::shared_ptr<Operator<DVector> const>) const override
  {
    ASSERT_THROW_NOT_IMPLEMENTED();
    return nullptr;
  }
  std::shared_ptr<Operator<DVector>> multiply_transpose(std::shared_ptr<Operator<DVector> const>) const override
  {
    ASSERT_THROW_NOT_IMPLEMENTED();
    return nullptr;
  }
  std::shared_ptr<DVector> build_domain_vector() const override { return std::make_shared<DVector>(_op->handle(), _op->n_dofs()); }
  std::shared_ptr<DVector> build_range_vector() const override { return build_domain_vector(); }
  size_t grid_complexity() const override { return (size_t)_op->n_dofs(); }
  size_t operator_complexity() const override { return 0; }
  void residual(DVector const &x, DVector const &b, DVector &res) const override;
  void smoother_step(DVector const &b, DVector const &x, DVector const *x_prev, double alpha, double beta, DVector &out) const override;
  double const *get_diagonal_inverse() const override { return _op->diagonal_inverse(); }
  HipHandle &get_hip_handle() const override { return _op->handle(); }
  std::shared_ptr<MatrixFreeLaplaceQ2Device<double>> get_device_operator() const { return _op; }

private:
  std::shared_ptr<MatrixFreeLaplaceQ2Device<double>> _op;
};

// apply(b, x), always from zero:  x = S(b, 0);  r = A_2 x - b;  x -= Hierarchy::vmult(r);  x = S(b, x)
// with S the Chebyshev smoother on A_2.  Parameters (the subtree "high order" of the INFO text): smoother.degree (2; 0: no
// smoothing, the pure refined-Q1 preconditioner), smoother.smoothing_range (4), smoother.eig_cg_n_iterations, smoother.lambda_max,
// smoother.lambda_min (as HipSmoother).  InvalidArgumentExc where the hierarchy's fine level is not of the operator's size.
class HighOrderPreconditioner
{
public:
  HighOrderPreconditioner(std::shared_ptr<HipQ2Operator const> a2, Hierarchy<DVector> const &q1_cycle, ptree const &params);
  void apply(DVector const &b, DVector &x) const;
  std::shared_ptr<HipQ2Operator const> get_operator() const { return _a2; }
  HipSmoother const *smoother() const { return _smoother.get(); } // null: smoother.degree 0
  int64_t size() const { return (int64_t)_a2->grid_complexity(); }

private:
  std::shared_ptr<HipQ2Operator const> _a2;
  Hierarchy<DVector> const &_q1_cycle;
  std::unique_ptr<HipSmoother> _smoother;
  mutable std::unique_ptr<DVector> _r, _c;
};
} // namespace mfmg
