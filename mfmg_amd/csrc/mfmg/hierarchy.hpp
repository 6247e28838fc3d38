// Hierarchy<VectorType>: mirror of include/mfmg/common/hierarchy.hpp:155-373.
// The constructor follows the reference line by line in *structure* (operator ->
// smoother -> restrictor -> A R^T -> R (A R^T) -> coarse solver, hierarchy.hpp:159-236)
// and apply() is the same recursive V-cycle with the negative-residual convention
// (hierarchy.hpp:246-309); what changes is what runs underneath: fused HIP kernels,
// temporaries built once per level, no host round trips.
#pragma once

#include <functional>

#include "hierarchy_helpers.hpp"
#include "hip_hierarchy_helpers.hpp"
#include "level.hpp"
#include "timer.hpp"

namespace mfmg
{
// String switch on the evaluator tag (include/mfmg/common/hierarchy.hpp:49-153).
template <typename VectorType>
std::unique_ptr<HierarchyHelpers<VectorType>> create_hierarchy_helpers(std::shared_ptr<MeshEvaluator> evaluator)
{
  std::unique_ptr<HierarchyHelpers<VectorType>> hierarchy_helpers;
  std::string evaluator_type = evaluator->get_mesh_evaluator_type();
  if (evaluator_type == "HipMeshEvaluator" || evaluator_type == "HipMatrixFreeMeshEvaluator")
  {
    auto hip_evaluator = std::dynamic_pointer_cast<HipMeshEvaluator>(evaluator);
    ASSERT_THROW(hip_evaluator != nullptr, "downcasting failed");
    hierarchy_helpers.reset(new HipHierarchyHelpers<VectorType>(hip_evaluator->get_hip_handle()));
  }
  else
  {
    // "DealIIMeshEvaluator", "DealIIMatrixFreeMeshEvaluator", "CudaMeshEvaluator" belong to
    // back-ends that are not part of this build.
    ASSERT_THROW_NOT_IMPLEMENTED("mesh evaluator type \"" + evaluator_type + "\" is not available in the HIP build");
  }
  return hierarchy_helpers;
}

template <typename VectorType>
class Hierarchy
{
public:
  Hierarchy(Communicator comm, std::shared_ptr<MeshEvaluator> evaluator, std::shared_ptr<ptree> params = nullptr,
            std::shared_ptr<TimerOutput> timer = nullptr)
      : _timer(timer)
  {
    timer_enter_subsection(_timer, "Setup");
    if (!params)
      params = std::make_shared<ptree>();
    _helpers = create_hierarchy_helpers<VectorType>(evaluator);
    auto &hierarchy_helpers = _helpers;

    _is_preconditioner = params->get("is preconditioner", true);
    _n_smoothing_steps = params->get("smoother.n_smoothing_steps", 1);

    int const num_levels = params->get("max levels", 2);
    ASSERT_THROW(num_levels > 0, "number of levels specified by \"max levels\" parameter must be positive");
    _levels.resize(num_levels);

    _levels[0].set_operator(hierarchy_helpers->get_global_operator(evaluator));
    for (int level_index = 0; level_index < num_levels; level_index++)
    {
      auto &level_fine = _levels[level_index];
      auto a = level_fine.get_operator();

      if (level_index == num_levels - 1)
      {
        if (level_index == 0)
          params->put("coarse.params.zero starting solution", _is_preconditioner);

        timer_enter_subsection(_timer, "Setup: build coarse solver");
        auto coarse_solver = hierarchy_helpers->build_coarse_solver(a, params);
        level_fine.set_solver(coarse_solver);
        timer_leave_subsection(_timer);
        break;
      }

      auto &level_coarse = _levels[level_index + 1];

      timer_enter_subsection(_timer, "Setup: build smoother");
      auto smoother = hierarchy_helpers->build_smoother(a, params);
      level_fine.set_smoother(smoother);
      timer_leave_subsection(_timer);

      timer_enter_subsection(_timer, "Setup: build restrictor");
      auto restrictor = hierarchy_helpers->build_restrictor(comm, evaluator, params);
      level_coarse.set_restrictor(restrictor);
      hierarchy_helpers->set_coarse_space_hint(restrictor);
      hierarchy_helpers->prepare_residual_restriction(a, restrictor, params);
      timer_leave_subsection(_timer);

      std::shared_ptr<Operator<VectorType>> ap;
      bool fast_ap = params->get("fast_ap", false);
      if (fast_ap)
      {
        timer_enter_subsection(_timer, "Setup: fast_ap");
        ap = hierarchy_helpers->fast_multiply_transpose();
        timer_leave_subsection(_timer);
      }
      else
      {
        timer_enter_subsection(_timer, "Setup: ap");
        ap = a->multiply_transpose(restrictor);
        timer_leave_subsection(_timer);
      }

      timer_enter_subsection(_timer, "Setup: build coarse matrix");
      auto a_coarse = restrictor->multiply(ap);
      timer_leave_subsection(_timer);
      // Extension ("keep_ap", default false): A R^T of every level stays reachable (ap_operators()), so that a test
      // can compare it with another way of forming it, as tests/test_hierarchy.cc:507-642 does.
      if (params->get("keep_ap", false))
        _ap_operators.push_back(ap);

      level_coarse.set_operator(a_coarse);
    }
    _params = params;
    timer_leave_subsection(_timer);
  }

  void vmult(VectorType &x, VectorType const &b) const
  {
    timer_enter_subsection(_timer, "Apply");
    apply(b, x, 0);
    timer_leave_subsection(_timer);
  }

  // `deliver` (level 0 of a hierarchy that runs in an internal numbering, dof_permutation.hpp): called with the vector that holds
  // the result in place of the copy into x that ends the cycle -- the caller scatters it into its own vector, from wherever the
  // iterate came to rest
  using Deliver = std::function<void(VectorType const &)>;

  void apply(VectorType const &b, VectorType &x, int level_index = 0, Deliver const *deliver = nullptr) const
  {
    auto const num_levels = _levels.size();

    auto &level_fine = _levels[level_index];
    auto a = level_fine.get_operator();

    const bool coarsest = level_index == static_cast<int>(num_levels) - 1;
    const bool from_zero = level_index > 0 || _is_preconditioner;
    // Zero out any garbage in x (hierarchy.hpp:253-259); a solver that does not read x needs no pass over it, and neither does a
    // smoother that can start from zero by itself (Smoother::apply_from_zero, tried below).
    bool zero_pending = from_zero && !(coarsest && level_fine.get_solver()->ignores_initial_guess());
    if (zero_pending && (coarsest || _n_smoothing_steps == 0))
    {
      x = 0.;
      zero_pending = false;
    }

    if (coarsest)
    {
      timer_enter_subsection(_timer, "Apply: coarsest level");
      auto coarse_solver = level_fine.get_solver();
      coarse_solver->apply(b, x);
      if (deliver)
        (*deliver)(x);
      timer_leave_subsection(_timer);
    }
    else
    {
      timer_enter_subsection(_timer, "Apply: fine levels");
      auto &level_coarse = _levels[level_index + 1];
      auto restrictor = level_coarse.get_restrictor();

      // (distributed runs: the ghost entries of b, which only the restriction of the residual reads, travel beside the
      // pre-smoother instead of in front of the restriction)
      restrictor->prefetch_rhs(b);

      // pre-smoother.  A smoother that works out of place (the multi-term sweep: it cannot write the vector it reads) alternates
      // between x and a workspace vector; pre- and post-smoothing together switch an even number of times.
      auto smoother = level_fine.get_smoother();
      VectorType *cur = &x, *other = nullptr;
      unsigned int first_step = 0;
      if (zero_pending)
      {
        // the first pre-smoothing step from x = 0: the smoother writes its result into the workspace vector without reading x
        bool done = false;
        if (smoother->prefers_out_of_place())
        {
          other = level_fine.workspace_vector(3).get();
          done = smoother->apply_from_zero(b, *other);
        }
        if (done)
        {
          std::swap(cur, other);
          first_step = 1;
        }
        else
          x = 0.;
      }
      auto smooth = [&] {
        for (unsigned int i = first_step; i < _n_smoothing_steps; ++i)
        {
          if (smoother->prefers_out_of_place())
          {
            if (other == nullptr)
              other = level_fine.workspace_vector(3).get();
            smoother->apply_to(b, *cur, *other);
            std::swap(cur, other);
          }
          else
            smoother->apply(b, *cur);
        }
      };
      smooth();
      first_step = 0;

      // negative residual -r = A x - b and its restriction: one pass where the restrictor holds the rows of R A,
      // otherwise one fused kernel for the residual and the restriction after it
      auto b_coarse = level_coarse.workspace_vector(1);
      if (!restrictor->restrict_residual(*a, *cur, b, *b_coarse))
      {
        auto res = level_fine.workspace_vector(0);
        a->residual(*cur, b, *res);
        restrictor->apply(*res, *b_coarse);
      }

      // coarse grid correction
      auto x_coarse = level_coarse.workspace_vector(2);
      apply(*b_coarse, *x_coarse, level_index + 1);

      // x -= R^T x_c (prolongation fused with the update)
      restrictor->apply_subtract(*x_coarse, *cur, OperatorMode::TRANS);

      // post-smoother
      smooth();
      if (deliver)
        (*deliver)(*cur);
      else if (cur != &x)
        x = *cur;
      restrictor->release_rhs();
      timer_leave_subsection(_timer);
    }
  }

  // The cycle of apply() on the columns of a block of vectors (several right-hand sides): x[c] gets the bits of apply(b[c], x[c]).
  // Where the fine level offers no block kernel (Smoother / Operator::block_width() == 1) that is what runs.  Otherwise the
  // block is taken in the groups of mf_block_groups (at most four columns) and the whole cycle runs per group: pre-smoothing and
  // residual on the block -- the operator's data read once for the group --, then the restriction of the group's residuals into
  // a coarse block and, after the coarse cycle -- on the group where the coarse solver offers it (Solver::block_width: its matrices
  // read once for the columns), column by column with the kernels of apply() otherwise --, the prolongation of the group in
  // one launch each where the restrictor offers it (Operator::transfer_block_width: its stored values read once for the group;
  // column by column otherwise, and the restriction as in apply() where R (A x - b) is formed in one pass), then post-smoothing
  // on the block.  The workspaces are one group wide whatever the number of columns; they are built at the first block call.
  // The columns of b and of x must share one leading dimension.
  void apply_block(std::vector<VectorType const *> const &b, std::vector<VectorType *> const &x) const
  {
    ASSERT_THROW(b.size() == x.size() && !b.empty(), "a block needs as many right-hand sides as iterates");
    _block_columns_looped = 0;
    auto &level_fine = _levels[0];
    auto a = level_fine.get_operator();
    auto smoother = level_fine.get_smoother();
    const bool block = _levels.size() > 1 && smoother && !smoother->prefers_out_of_place() && smoother->block_width() > 1 && a->block_width() > 1;
    int widths[kMfBlockMaxGroups];
    const int n_groups = mf_block_groups((int)b.size(), widths);
    size_t c0 = 0;
    for (int g = 0; g < n_groups; c0 += widths[g], ++g)
    {
      const size_t w = (size_t)widths[g];
      if (!block || w == 1)
      {
        for (size_t c = c0; c < c0 + w; ++c)
          apply(*b[c], *x[c]);
        _block_columns_looped += (int64_t)w;
        _transfer_columns_looped += (int64_t)w;
        continue;
      }
      timer_enter_subsection(_timer, "Apply: fine levels");
      const std::vector<VectorType const *> bg(b.begin() + c0, b.begin() + c0 + w);
      const std::vector<VectorType *> xg(x.begin() + c0, x.begin() + c0 + w);
      auto &level_coarse = _levels[1];
      auto restrictor = level_coarse.get_restrictor();
      if (_is_preconditioner)
        for (auto *xc : xg)
          *xc = 0.;
      for (unsigned int i = 0; i < _n_smoothing_steps; ++i)
        smoother->apply_block(bg, xg);
      // the coarse vectors of the group: columns of one block where the restrictor has block transfers (right-hand sides, then
      // iterates), the level's two workspace vectors for one column after the other otherwise
      auto b_coarse = level_coarse.workspace_vector(1);
      auto x_coarse = level_coarse.workspace_vector(2);
      const bool wide_restrict = restrictor->transfer_block_width(OperatorMode::NO_TRANS) > 1,
                 wide_prolong = restrictor->transfer_block_width(OperatorMode::TRANS) > 1;
      std::vector<VectorType *> bc(w, b_coarse.get()), xc(w, x_coarse.get());
      // ... and where the coarse solver runs its cycle on a group (Solver::block_width: the matrices of its levels read once for
      // the columns): then the group is solved in one call between the restrictions and the prolongations
      auto coarse_solver = _levels.size() == 2 ? level_coarse.get_solver() : nullptr;
      const bool wide_solve = coarse_solver && coarse_solver->block_width() > 1 && coarse_solver->ignores_initial_guess();
      if (wide_restrict || wide_prolong || wide_solve)
      {
        if (_coarse_block_workspace.size() < 2 * w)
        {
          MemoryKind kind("hierarchy: coarse block workspace (right-hand sides and iterates of one group on the first coarse level)");
          _coarse_block_workspace.clear(); // (before the wider one is built)
          const int64_t n_coarse = b_coarse->size();
          _coarse_block_workspace = level_coarse.get_operator()->build_domain_block(2 * (int)w, n_coarse + (n_coarse & 1));
        }
        for (size_t c = 0; c < w; ++c)
        {
          bc[c] = _coarse_block_workspace[c].get();
          xc[c] = _coarse_block_workspace[w + c].get();
        }
      }
      // the residual of the group in one launch, unless the restrictor forms R (A x - b) in one pass as apply() then does
      const bool one_pass = restrictor->restrict_residual(*a, *xg[0], *bg[0], *bc[0]);
      std::vector<VectorType *> res;
      if (!one_pass)
      {
        const int64_t ld = w > 1 ? (int64_t)(xg[1]->get_values() - xg[0]->get_values()) : xg[0]->size();
        if (_block_workspace.size() < w || _block_workspace_ld != ld)
        {
          MemoryKind kind("hierarchy: block workspace (residual of one group of right-hand sides)");
          _block_workspace.clear(); // (before the wider one is built)
          _block_workspace = a->build_domain_block((int)w, ld);
          _block_workspace_ld = ld;
        }
        for (size_t c = 0; c < w; ++c)
          res.push_back(_block_workspace[c].get());
        a->residual_block(std::vector<VectorType const *>(xg.begin(), xg.end()), bg, res);
      }
      // restriction and prolongation of the group in one launch each where the restrictor reads its stored values once for the
      // columns; the coarse cycle column by column in between
      const bool block_restrict = !one_pass && wide_restrict;
      if (block_restrict)
        restrictor->apply_block(std::vector<VectorType const *>(res.begin(), res.end()), bc);
      for (size_t c = 0; c < w; ++c)
      {
        if (!one_pass && !block_restrict)
          restrictor->apply(*res[c], *bc[c]);
        else if (one_pass && c > 0)
          ASSERT_THROW(restrictor->restrict_residual(*a, *xg[c], *bg[c], *bc[c]), "internal: the one-pass residual restriction was refused");
        if (wide_solve)
          continue;
        apply(*bc[c], *xc[c], 1);
        if (!wide_prolong)
          restrictor->apply_subtract(*xc[c], *xg[c], OperatorMode::TRANS);
      }
      if (wide_solve)
      {
        timer_enter_subsection(_timer, "Apply: coarsest level");
        coarse_solver->apply_block(std::vector<VectorType const *>(bc.begin(), bc.end()), xc);
        timer_leave_subsection(_timer);
        if (!wide_prolong)
          for (size_t c = 0; c < w; ++c)
            restrictor->apply_subtract(*xc[c], *xg[c], OperatorMode::TRANS);
      }
      if (wide_prolong)
        restrictor->apply_subtract_block(std::vector<VectorType const *>(xc.begin(), xc.end()), xg, OperatorMode::TRANS);
      if (!wide_prolong || (!one_pass && !block_restrict))
        _transfer_columns_looped += (int64_t)w;
      for (unsigned int i = 0; i < _n_smoothing_steps; ++i)
        smoother->apply_block(bg, xg);
      timer_leave_subsection(_timer);
    }
  }
  // columns of the last apply_block that went through apply() one by one
  int64_t block_columns_looped() const { return _block_columns_looped; }
  // columns of all apply_block calls so far whose restriction or prolongation on the fine level went through the one-vector
  // kernels (the launches of the block transfers are counted where they happen, by the restrictor)
  int64_t transfer_columns_looped() const { return _transfer_columns_looped; }
  // width of the widest group apply_block runs as one launch on the fine level (1: the loop over the columns)
  int block_width() const
  {
    auto smoother = _levels[0].get_smoother();
    const bool block = _levels.size() > 1 && smoother && !smoother->prefers_out_of_place() && smoother->block_width() > 1 &&
                       _levels[0].get_operator()->block_width() > 1;
    return block ? std::min(smoother->block_width(), _levels[0].get_operator()->block_width()) : 1;
  }

  // Replace R on level 1 and re-derive A_c and the coarse solver (same sequence as
  // the constructor, hierarchy.hpp:209-233,193-196): lets CPU and GPU runs share one R.
  void set_restrictor(std::shared_ptr<Operator<VectorType>> restrictor)
  {
    ASSERT_THROW(_levels.size() == 2, "set_restrictor supports the two-level hierarchy only");
    auto a = _levels[0].get_operator();
    _levels[1].set_restrictor(restrictor);
    _helpers->prepare_residual_restriction(a, restrictor, _params);
    auto ap = a->multiply_transpose(restrictor);
    auto a_coarse = restrictor->multiply(ap);
    _levels[1].set_operator(a_coarse);
    _coarse_block_workspace.clear();
    _helpers->set_coarse_space_hint(restrictor);
    _levels[1].set_solver(_helpers->build_coarse_solver(a_coarse, _params));
  }

  // stubbed to 0 upstream (hierarchy.hpp:311-366)
  double grid_complexity() const { return 0; }
  double operator_complexity() const { return 0; }

  std::vector<Level<VectorType>> const &levels() const { return _levels; }
  bool is_preconditioner() const { return _is_preconditioner; }
  unsigned int n_smoothing_steps() const { return _n_smoothing_steps; }
  std::shared_ptr<TimerOutput> timer() const { return _timer; }
  std::vector<std::shared_ptr<Operator<VectorType>>> const &ap_operators() const { return _ap_operators; }

private:
  std::shared_ptr<TimerOutput> _timer;
  std::unique_ptr<HierarchyHelpers<VectorType>> _helpers;
  std::shared_ptr<ptree> _params;
  std::vector<Level<VectorType>> _levels;
  std::vector<std::shared_ptr<Operator<VectorType>>> _ap_operators; // only with "keep_ap"
  bool _is_preconditioner = true;
  unsigned int _n_smoothing_steps;
  mutable std::vector<std::shared_ptr<VectorType>> _block_workspace; // apply_block: the residuals of one group
  mutable int64_t _block_workspace_ld = 0;
  mutable int64_t _block_columns_looped = 0;
  mutable std::vector<std::shared_ptr<VectorType>> _coarse_block_workspace; // apply_block: b_c and x_c of one group
  mutable int64_t _transfer_columns_looped = 0;
};
} // namespace mfmg
