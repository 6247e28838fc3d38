// HipQ2Operator and HighOrderPreconditioner (mfmg/hip_high_order.hpp).  No kernel lives here: the operator launches those of
// mf_laplace_q2.hip, the preconditioner the smoother's and the hierarchy's.
#include "mfmg/hip_high_order.hpp"

#include "krylov_drivers.hpp"

namespace mfmg
{
void HipQ2Operator::apply(DVector const &x, DVector &y, OperatorMode mode) const
{
  if (mode != OperatorMode::NO_TRANS)
    ASSERT_THROW_NOT_IMPLEMENTED();
  _op->vmult(x.get_values(), y.get_values());
}

void HipQ2Operator::residual(DVector const &x, DVector const &b, DVector &res) const
{
  _op->residual(x.get_values(), b.get_values(), res.get_values());
}

void HipQ2Operator::smoother_step(DVector const &b, DVector const &x, DVector const *x_prev, double alpha, double beta, DVector &out) const
{
  _op->smoother_step(b.get_values(), x.get_values(), x_prev ? x_prev->get_values() : nullptr, alpha, beta, out.get_values());
}

HighOrderPreconditioner::HighOrderPreconditioner(std::shared_ptr<HipQ2Operator const> a2, Hierarchy<DVector> const &q1_cycle,
                                                 ptree const &params)
  : _a2(std::move(a2)), _q1_cycle(q1_cycle)
{
  if (_a2 == nullptr)
    throw InvalidArgumentExc("null Q2 operator");
  if (level_size(q1_cycle, 0) != size())
    throw InvalidArgumentExc("the fine level of the Q1 hierarchy is not of the size of the Q2 operator (build it on the refined mesh)");
  const int degree = params.get("smoother.degree", 2);
  if (degree < 0)
    throw InvalidArgumentExc("high order: smoother.degree must not be negative");
  if (degree > 0)
  {
    auto sp = std::make_shared<ptree>();
    sp->put("smoother.type", std::string("Chebyshev"));
    sp->put("smoother.degree", degree);
    sp->put("smoother.smoothing_range", params.get("smoother.smoothing_range", 4.));
    if (auto v = params.get_optional<int>("smoother.eig_cg_n_iterations"))
      sp->put("smoother.eig_cg_n_iterations", *v);
    if (auto v = params.get_optional<double>("smoother.lambda_max"))
      sp->put("smoother.lambda_max", *v);
    if (auto v = params.get_optional<double>("smoother.lambda_min"))
      sp->put("smoother.lambda_min", *v);
    _smoother.reset(new HipSmoother(_a2, sp));
  }
}

void HighOrderPreconditioner::apply(DVector const &b, DVector &x) const
{
  HipHandle &handle = _a2->get_hip_handle();
  const int64_t n = size();
  if (b.size() != n || x.size() != n)
    throw InvalidArgumentExc("high order: vector size mismatch");
  if (!_r)
  {
    MemoryKind kind("high order preconditioner: residual and correction");
    _r.reset(new DVector(handle, n));
    _c.reset(new DVector(handle, n));
  }
  if (_smoother)
  {
    _smoother->apply_zero_guess(b, x);
    _a2->residual(x, b, *_r);
  }
  else
  {
    x = 0.;
    *_r = 0.;
    _r->add(-1., b); // r = A_2 0 - b
  }
  if (!_q1_cycle.is_preconditioner())
    *_c = 0.; // (such a cycle reads its start vector)
  _q1_cycle.vmult(*_c, *_r);
  x.add(-1., *_c);
  if (_smoother)
    _smoother->apply(b, x);
}
} // namespace mfmg
