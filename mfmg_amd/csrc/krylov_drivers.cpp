// The Krylov drivers and their working sets (krylov_drivers.hpp).
#include "krylov_drivers.hpp"

#include <cmath>
#include <functional>

namespace mfmg
{
int64_t level_size(Hierarchy<DVector> const &hierarchy, int level)
{
  auto op = hierarchy.levels()[level].get_operator();
  if (auto m = std::dynamic_pointer_cast<HipMatrixOperator const>(op))
    return m->get_matrix()->m();
  return (int64_t)op->grid_complexity();
}

int64_t block_kernel_launches(Hierarchy<DVector> const &hierarchy)
{
  auto op = std::dynamic_pointer_cast<HipMatrixFreeOperator const>(hierarchy.levels()[0].get_operator());
  return op ? op->get_mesh_evaluator()->get_device_operator()->block_launches() : 0;
}

// ---- what every driver needs ----------------------------------------------------------------
namespace
{
// Several ranks: the box of owned entries in a local vector of the fine level, over which the drivers take their dots and norms.
// Exc is what the entry point reports a context with that is not set up for it.
template <typename Exc>
krylov::OwnedBox fine_owned_box(KrylovSetting const &s, int64_t n)
{
  HaloCommunicator const &comm = s.handle.comm;
  auto hop = std::dynamic_pointer_cast<HipOperator const>(s.hierarchy.levels()[0].get_operator());
  const int space = hop ? hop->domain_space() : 0;
  if (space <= 0 || space >= (int)comm.spaces.size() || !comm.spaces[space].configured() || comm.transport == nullptr)
    throw Exc("the fine operator has no distributed vector space or no transport was registered");
  const krylov::OwnedBox box(comm.spaces[space]);
  if (box.n_local() != n)
    throw Exc("the fine space does not describe the vectors of the fine level");
  return box;
}

// `count` doubles on the device summed over the ranks through the pinned buffer `host`: to the host, ONE all-reduce, and back to
// `to` where the device needs the sums (null: the host alone reads them).  The sums stay in `host`.
struct RankSum
{
  HipHandle &handle;
  double *host;
  int64_t allreduces = 0;
  void operator()(double const *dev, int count, double *to)
  {
    MFMG_HIP_CHECK(hipMemcpyAsync(host, dev, sizeof(double) * count, hipMemcpyDeviceToHost, handle.stream));
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream));
    handle.comm.transport->allreduce(host, count, 0, handle.stream);
    ++allreduces;
    if (to)
      MFMG_HIP_CHECK(hipMemcpyAsync(to, host, sizeof(double) * count, hipMemcpyHostToDevice, handle.stream));
  }
};

// b and x of k columns in the numbering the hierarchy runs in: the caller's vectors, or with a permutation the library's
// (`work_b`, `work_x` with the leading dimension `work_ld`), gathered here and scattered by scatter()
struct RunVectors
{
  DofPermutation *perm;
  int k;
  int64_t caller_ld, ld;
  double *caller_x;
  double const *b;
  double *x;
  RunVectors(DofPermutation *perm, int k, int64_t caller_ld, double const *caller_b, double *caller_x, int64_t work_ld, double *work_b,
             double *work_x)
    : perm(perm), k(k), caller_ld(caller_ld), ld(perm ? work_ld : caller_ld), caller_x(caller_x), b(perm ? work_b : caller_b),
      x(perm ? work_x : caller_x)
  {
    if (perm)
      for (int c = 0; c < k; ++c)
        perm->gather2(caller_b + c * caller_ld, static_cast<double const *>(caller_x + c * caller_ld), work_b + c * ld, work_x + c * ld);
  }
  void scatter() const
  {
    if (perm)
      for (int c = 0; c < k; ++c)
        perm->scatter(static_cast<double const *>(x + c * ld), caller_x + c * caller_ld);
  }
};

// the operator a one-vector driver iterates on and its preconditioner z = M^-1 r: the outer pair of the setting, or the
// hierarchy's fine operator and cycle
std::shared_ptr<Operator<DVector> const> outer_or_fine_operator(KrylovSetting const &s)
{
  if (s.outer_operator)
    return s.outer_operator;
  return s.hierarchy.levels()[0].get_operator();
}
void precondition(KrylovSetting const &s, DVector const &r, DVector &z)
{
  if (s.outer_preconditioner)
    s.outer_preconditioner(r, z);
  else
    s.hierarchy.vmult(z, r);
}
void refuse_outer(KrylovSetting const &s, char const *what)
{
  if (s.outer_operator || s.outer_preconditioner)
    ASSERT_THROW_NOT_IMPLEMENTED(what);
}

// ||r|| of iteration `it` of column c into a history of history_ld entries per column (or none)
void record(double *history, int history_ld, int c, int it, double v)
{
  if (history && it < history_ld)
    history[(int64_t)c * history_ld + it] = v;
}
} // namespace

// ---- CG ------------------------------------------------------------------------------------
// Preconditioned CG as dealii::SolverCG runs it (third-party, restated): r = b - A x, z = M^-1 r, p = z;
// alpha = (r,z)/(p,Ap); x += alpha p; r -= alpha Ap; stop on ||r||_2 <= tolerance; beta = (r,z)_new/(r,z)_old
KrylovResult solve_cg(KrylovSetting const &s, const double *b, double *x, double tolerance, int max_iterations, double *residual_history,
                      int history_len)
{
  HipHandle &handle = s.handle;
  const int64_t n = level_size(s.hierarchy, 0);
  std::shared_ptr<Operator<DVector> const> op = outer_or_fine_operator(s);
  auto hop = std::dynamic_pointer_cast<HipOperator const>(op);
  const int space = hop ? hop->domain_space() : 0;
  const RunVectors run(s.perm, 1, n, b, x, n, s.work[0], s.work[1]);
  DVector bv(handle, n, const_cast<double *>(run.b)), xv(handle, n, run.x);
  DVector r(handle, n), z(handle, n), p(handle, n), ap(handle, n);
  auto dot = [&](DVector const &u, DVector const &v) { return distributed_dot(handle, space, u, v); };
  op->apply(xv, r);
  r.sadd(-1., 1., bv); // r = b - A x
  double res = std::sqrt(dot(r, r));
  int it = 0;
  record(residual_history, history_len, 0, 0, res);
  double rz = 0.;
  bool converged = res <= tolerance;
  if (!handle.comm.enabled())
  {
    // One rank: the scalars of the iteration stay on the device (vec::cg_direction / cg_update read them there) -- ONE host
    // round trip per iteration, for the stopping test, instead of three; x and r are updated in one pass.  The same sums in the
    // same order as below: the same iterates.
    DeviceBuffer<double> scal(4); // [0], [1]: (r, z) of this / the previous iteration, alternating; [2]: (p, A p); [3]: (r, r)
    int cur = 0;
    while (!converged && it < max_iterations)
    {
      precondition(s, r, z);
      vec::dot_async<double>(handle, n, r.get_values(), z.get_values(), scal.data(), cur);
      if (it == 0)
        p = z;
      else
        vec::cg_direction<double>(handle, n, z.get_values(), p.get_values(), scal.data(), cur, 1 - cur); // p = z + beta p
      op->apply(p, ap);
      vec::dot_async<double>(handle, n, p.get_values(), ap.get_values(), scal.data(), 2);
      vec::cg_update<double>(handle, n, p.get_values(), ap.get_values(), nullptr, xv.get_values(), r.get_values(), nullptr, scal.data(), cur, 2);
      vec::dot_async<double>(handle, n, r.get_values(), r.get_values(), scal.data(), 3);
      MFMG_HIP_CHECK(hipMemcpyAsync(handle.host_result, scal.data() + 3, sizeof(double), hipMemcpyDeviceToHost, handle.stream));
      MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream));
      res = std::sqrt(handle.host_result[0]);
      cur = 1 - cur;
      ++it;
      record(residual_history, history_len, 0, it, res);
      converged = res <= tolerance;
    }
  }
  while (!converged && it < max_iterations)
  {
    precondition(s, r, z);
    const double rz_new = dot(r, z);
    if (it == 0)
      p = z;
    else
      p.sadd(rz_new / rz, 1., z); // p = z + beta p
    rz = rz_new;
    op->apply(p, ap);
    const double alpha = rz / dot(p, ap);
    xv.add(alpha, p);
    r.add(-alpha, ap);
    res = std::sqrt(dot(r, r));
    ++it;
    record(residual_history, history_len, 0, it, res);
    converged = res <= tolerance;
  }
  run.scatter();
  KrylovResult result(1);
  result.iterations[0] = it;
  result.residuals[0] = res;
  result.converged[0] = converged;
  return result;
}

// solve_cg on a block of right-hand sides.  All columns iterate in lockstep, so "the first iteration" is the same for every slot;
// a column that converged leaves the working blocks (block_krylov::plan_retire keeps the active slots contiguous) and costs
// nothing further.  Per iteration: the cycle on the active slots (Hierarchy::apply_block), (r, z) of all of them in one reduction,
// the direction, the operator on the block, (p, A p), the update with the partials of (r, r) folded in, ONE device-to-host copy of
// the active slots' (r, r) and ONE synchronisation.  Every kernel gives a slot the bits the one-vector driver gives its vector, so
// x, the iteration count and the history of a column are those of solve_cg.
// Several ranks: the blocks hold the ranks' local vectors.  The operator and the cycle exchange what they read (a group of columns
// one message per neighbour where the ranks agreed on blocks); direction and update run over all local entries; (r, z), (p, A p)
// and (r, r) run over the owned entries of all live slots in one launch (block_krylov::dots on the OwnedBox of the fine space)
// and are summed over the ranks in ONE all-reduce each -- three per iteration whatever k, plus one for the initial residuals.
// Every control decision is taken from all-reduced values, so every rank retires the same columns and leaves the loop in the same
// iteration.  A column has the bits of the one-vector solve on the same ranks where the transport sums an element in the same
// order whatever the length of the message (block_krylov.hpp).
KrylovResult solve_cg_block(KrylovSetting const &s, int k, int64_t ld, const double *b, double *x, const double *tolerances,
                            int max_iterations, double *residual_history, int history_ld)
{
  refuse_outer(s, "block CG is not implemented for an outer operator (the high-order preconditioner)");
  HipHandle &handle = s.handle;
  const int64_t n = level_size(s.hierarchy, 0);
  auto op = s.hierarchy.levels()[0].get_operator();
  // Without a permutation the working blocks take the caller's leading dimension, so that the operator runs from the caller's x
  // into r on one block layout.
  const bool permute = s.perm != nullptr;
  const int64_t wld = permute ? n + (n & 1) : ld;
  BlockCgWorkspace &ws = s.workspaces.block_cg;
  reserve_or_empty(ws, wld, k, permute, handle.stream);
  const RunVectors run(s.perm, k, ld, b, x, wld, ws.B.data(), ws.X.data());
  double *const R = ws.R.data(), *const Z = ws.Z.data(), *const P = ws.P.data(), *const AP = ws.AP.data();
  double *const partials = ws.partials.data();
  double *const host = ws.host.get();
  int32_t *const host_col = ws.host_col();
  double *const rz[2] = {ws.scalars.data(), ws.scalars.data() + ws.columns}; // (r, z) of this / the previous iteration, alternating
  double *const pap = ws.scalars.data() + 2 * ws.columns, *const rr = ws.scalars.data() + 3 * ws.columns;
  const bool z_is_read = !s.hierarchy.is_preconditioner(); // the cycle then starts from what z holds: the one-vector driver's zero / last z
  if (z_is_read)
    MFMG_HIP_CHECK(hipMemsetAsync(Z, 0, sizeof(double) * (size_t)wld * k, handle.stream));
  const int64_t launches_before = block_kernel_launches(s.hierarchy);
  int64_t preconditioner_columns = 0, operator_columns = 0, slot_moves = 0;
  auto fetch = [&](int count) { // (r, r) of the first `count` slots: the one round trip of an iteration
    MFMG_HIP_CHECK(hipMemcpyAsync(host, rr, sizeof(double) * count, hipMemcpyDeviceToHost, handle.stream));
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream));
  };
  // several ranks: the reductions over the owned entries, summed over the ranks
  const bool distributed = handle.comm.enabled();
  const krylov::OwnedBox box = distributed ? fine_owned_box<InvalidArgumentExc>(s, n) : krylov::OwnedBox();
  RankSum sum_over_ranks{handle, host};
  // out[s] = (X_s, Y_s) of the first `count` slots on the device; several ranks: over the owned entries and summed over the ranks
  // (`host` then holds the sums as well)
  auto reduce = [&](int count, double const *X, double const *Y, double *out) {
    if (!distributed)
      return block_krylov::dots(handle, n, count, wld, X, Y, partials, out);
    block_krylov::dots(handle, box, count, wld, X, Y, partials, out);
    sum_over_ranks(out, count, out != rr ? out : nullptr); // ((r, r) is read on the host alone)
    if (out != rr)
      MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream)); // (`host` is written again by the next reduction)
  };
  // r = b - A x, as the one-vector driver forms it: the operator, then r = -r + b per column
  {
    BlockViews xv(handle, n, wld, k, run.x), rv(handle, n, wld, k, R);
    op->apply_block(xv.cptr, rv.ptr);
    for (int c = 0; c < k; ++c)
      vec::sadd<double>(handle, n, -1., 1., run.b + c * wld, R + c * wld);
  }
  reduce(k, R, R, rr);
  if (!distributed)
    fetch(k);
  KrylovResult result(k);
  std::vector<double> &res = result.residuals;
  std::vector<int32_t> &iterations = result.iterations;
  std::vector<int32_t> flags(k), moves(2 * (size_t)k);
  int n_active = k;
  bool any = false;
  for (int c = 0; c < k; ++c)
  {
    res[c] = std::sqrt(host[c]);
    record(residual_history, history_ld, c, 0, res[c]);
    flags[c] = res[c] <= tolerances[c];
    any = any || flags[c];
    host_col[c] = c;
  }
  int it = 0, cur = 0;
  // the slots named by `flags` retire; r, p (and what else the next iteration reads of a slot) of the slots that move follow.
  // (host_col is written only after the synchronisation that follows the upload before: the copy never reads a changing array)
  auto retire = [&](bool upload_always) {
    int n_left = n_active, n_moves = 0;
    if (any)
      n_moves = block_krylov::plan_retire(n_active, flags.data(), host_col, moves.data(), &n_left);
    n_active = n_left;
    if (n_active == 0 || it >= max_iterations || !(any || upload_always))
      return;
    for (int m = 0; m < n_moves; ++m)
    {
      const int64_t from = moves[2 * m], to = moves[2 * m + 1];
      vec::copy<double>(handle, n, R + from * wld, R + to * wld);
      if (it > 0)
      {
        vec::copy<double>(handle, n, P + from * wld, P + to * wld);
        if (z_is_read)
          vec::copy<double>(handle, n, Z + from * wld, Z + to * wld);
        MFMG_HIP_CHECK(hipMemcpyAsync(rz[1 - cur] + to, rz[1 - cur] + from, sizeof(double), hipMemcpyDeviceToDevice, handle.stream));
      }
    }
    slot_moves += n_moves;
    MFMG_HIP_CHECK(hipMemcpyAsync(ws.slot_col.data(), host_col, sizeof(int32_t) * n_active, hipMemcpyHostToDevice, handle.stream));
  };
  retire(true);
  while (n_active > 0 && it < max_iterations)
  {
    {
      BlockViews rv(handle, n, wld, n_active, R), zv(handle, n, wld, n_active, Z);
      TimerSubsection apply(s.timer, "Apply");
      s.hierarchy.apply_block(rv.cptr, zv.ptr);
    }
    preconditioner_columns += n_active;
    reduce(n_active, R, Z, rz[cur]);
    if (distributed) // (p.sadd(beta, 1., z) of the one-vector driver on ranks rounds beta p before it adds z)
      block_krylov::cg_direction_local(handle, n, n_active, wld, Z, P, rz[cur], rz[1 - cur], it == 0);
    else
      block_krylov::cg_direction(handle, n, n_active, wld, Z, P, rz[cur], rz[1 - cur], it == 0); // p = z + beta p
    {
      BlockViews pv(handle, n, wld, n_active, P), apv(handle, n, wld, n_active, AP);
      op->apply_block(pv.cptr, apv.ptr);
    }
    operator_columns += n_active;
    reduce(n_active, P, AP, pap);
    if (distributed)
    {
      block_krylov::cg_update_local(handle, n, n_active, wld, P, AP, R, wld, run.x, ws.slot_col.data(), rz[cur], pap);
      reduce(n_active, R, R, rr);
    }
    else
    {
      block_krylov::cg_update(handle, n, n_active, wld, P, AP, R, wld, run.x, ws.slot_col.data(), rz[cur], pap, partials, rr);
      fetch(n_active);
    }
    cur = 1 - cur; // rz[1 - cur] is now the (r, z) of the iteration that just ended
    ++it;
    any = false;
    for (int sl = 0; sl < n_active; ++sl)
    {
      const int c = host_col[sl];
      res[c] = std::sqrt(host[sl]);
      iterations[c] = it;
      record(residual_history, history_ld, c, it, res[c]);
      flags[sl] = res[c] <= tolerances[c];
      any = any || flags[sl];
    }
    retire(false);
  }
  run.scatter();
  for (int c = 0; c < k; ++c)
    result.converged[c] = res[c] <= tolerances[c]; // (what retired the column; the others are the slots still active)
  result.work[0] = preconditioner_columns;
  result.work[1] = operator_columns;
  result.work[2] = block_kernel_launches(s.hierarchy) - launches_before;
  result.work[3] = slot_moves;
  result.allreduces = sum_over_ranks.allreduces;
  return result;
}

// ---- flexible GMRES ---------------------------------------------------------------------------
// Right-preconditioned flexible GMRES(restart) as dealii::SolverFGMRES runs it (third-party, restated): r = b - A x, v_0 = r / ||r||;
// step j: z_j = M^-1 v_j, w = A z_j, w orthogonalised against v_0 .. v_j (classical Gram-Schmidt twice, krylov_basis.hpp),
// v_{j+1} = w / ||w||; the Hessenberg column goes through the Givens rotations on the host, |g_{j+1}| is the residual norm of the
// least-squares problem and is what SolverControl sees; x += Z y when it is small enough or the basis is full.
// Several ranks: the vectors are the ranks' local ones, b, x and the basis handed to the operator and the cycle as solve_cg hands
// them (ghost entries are exchanged by whoever reads them, and are don't-care here).  Dots and norms run over the owned entries
// (krylov::OwnedBox of the fine space) and are summed over the ranks on the host: per iteration one all-reduce of the j + 1
// coefficients per Gram-Schmidt pass and one of ||w||^2, three in all.  The Hessenberg column is then on the host already.  EVERY
// control decision below -- convergence, breakdown, restart, the end of the iteration -- is taken from all-reduced values alone
// (`res`, the column, the iteration count), so all ranks take the same branch: a rank that left the loop by itself would leave the
// others waiting in the next exchange.
namespace
{
// The iteration of solve_fgmres on vectors in the numbering the hierarchy runs in (`b_run`, `x_run`), with restart cycles of m
// columns, from the iteration count `it_start`: the state at the start of a cycle is x and the count alone, so a solve that is
// taken up at a cycle start (the block driver hands over a column that broke down) goes on with the bits of the solve that was
// never interrupted.  history[it] receives the residual of iteration it (it < history_len), history[it_start] that of the cycle
// start.
KrylovResult fgmres_run(KrylovSetting const &s, const double *b_run, double *x_run, double tolerance, int max_iterations, int m, bool fp32,
                         int it_start, double *residual_history, int history_len)
{
  HipHandle &handle = s.handle;
  const int64_t n = level_size(s.hierarchy, 0);
  KrylovWorkspace &ws = s.workspaces.fgmres;
  reserve_or_empty(ws, n, m, fp32);
  const int64_t ld = ws.ld;
  krylov::Scratch &scratch = *ws.scratch;
  double *const V = ws.V.data(), *const Z = ws.Z.data(), *const hcol = ws.coefficients.data(), *const y_dev = hcol + ws.columns + 1;
  double *const host = ws.host.get(), *const y_host = host + ws.columns + 1;
  float *const v_f32 = fp32 ? ws.v_f32.data() : nullptr;
  std::shared_ptr<Operator<DVector> const> op = outer_or_fine_operator(s);
  if (fp32)
    refuse_outer(s, "the FP32 preconditioner does not exist for an outer operator");
  const bool distributed = handle.comm.enabled();
  const krylov::OwnedBox box = distributed ? fine_owned_box<std::runtime_error>(s, n) : krylov::OwnedBox();
  RankSum sum_over_ranks{handle, host};
  // ||w||^2 over the owned entries of all ranks from this rank's s.norm_partials: on the device (scratch.norm_squared) and returned
  auto norm_squared_of_all = [&] {
    krylov::basis_norm_finish(handle, scratch, box);
    sum_over_ranks(scratch.norm_squared.data(), 1, scratch.norm_squared.data());
    return host[0];
  };
  DVector bv(handle, n, const_cast<double *>(b_run)), xv(handle, n, x_run);
  auto fetch = [&](int count) { // the first `count` device coefficients: the one round trip of an iteration
    MFMG_HIP_CHECK(hipMemcpyAsync(host, hcol, sizeof(double) * count, hipMemcpyDeviceToHost, handle.stream));
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream));
  };
  // v_0 = r / ||r|| with r = b - A x (and its float copy); returns ||r||
  auto start_cycle = [&] {
    DVector r(handle, n, V);
    op->apply(xv, r);
    r.sadd(-1., 1., bv);
    if (distributed)
    {
      krylov::basis_norm_partials(handle, scratch, box, V);
      const double norm = std::sqrt(norm_squared_of_all());
      krylov::basis_scale_store(handle, box, scratch.norm_squared.data(), V, V, nullptr);
      // (the whole local vector: what its ghost entries hold is exchanged over by the FP32 level where it reads them)
      if (fp32)
        vec::narrow(handle, n, V, v_f32);
      return norm;
    }
    krylov::basis_norm_partials(handle, scratch, n, V);
    krylov::basis_scale_store(handle, scratch, n, V, V, v_f32, hcol);
    fetch(1);
    return host[0];
  };
  auto precondition = [&](int j) { // z_j = M^-1 v_j, from a zero start whatever "is preconditioner" says
    const bool zero_first = !s.hierarchy.is_preconditioner();
    if (fp32)
    {
      if (zero_first)
        MFMG_HIP_CHECK(hipMemsetAsync(ws.z_f32.data(), 0, sizeof(float) * n, handle.stream));
      s.fine_f32->apply(v_f32, ws.z_f32.data());
      vec::widen(handle, n, ws.z_f32.data(), Z + j * ld);
      return;
    }
    DVector vj(handle, n, V + j * ld), zj(handle, n, Z + j * ld);
    if (s.outer_preconditioner)
    {
      s.outer_preconditioner(vj, zj);
      return;
    }
    if (zero_first)
      zj = 0.;
    s.hierarchy.vmult(zj, vj);
  };
  KrylovResult out(1);
  int64_t &cycle_starts = out.work[3];
  double res = start_cycle();
  ++cycle_starts;
  int it = it_start;
  record(residual_history, history_len, 0, it, res);
  bool converged = res <= tolerance;
  FgmresColumn col(m);
  while (!converged && it < max_iterations)
  {
    col.begin_cycle(res);
    while (col.k < m && it < max_iterations && !converged && !col.breakdown)
    {
      const int j = col.k;
      precondition(j);
      double *const w = V + (int64_t)(j + 1) * ld;
      {
        DVector zj(handle, n, Z + j * ld), wv(handle, n, w);
        op->apply(zj, wv);
      }
      double *const c = col.column(j);
      if (distributed)
      {
        // the column h_0 .. h_j, ||w|| is summed over the ranks on its way: no fetch
        double *const pc = scratch.pass_coefficients.data();
        for (int pass = 0; pass < 2; ++pass)
        {
          krylov::basis_dots(handle, scratch, box, ld, j + 1, V, w, pc, pc, false);
          sum_over_ranks(pc, j + 1, pc);
          for (int i = 0; i <= j; ++i)
            c[i] = pass == 0 ? host[i] : c[i] + host[i];
          krylov::basis_update(handle, scratch, box, ld, j + 1, V, pc, w, pass == 1);
        }
        c[j + 1] = std::sqrt(norm_squared_of_all());
        krylov::basis_scale_store(handle, box, scratch.norm_squared.data(), w, w, nullptr);
        if (fp32)
          vec::narrow(handle, n, w, v_f32);
      }
      else
      {
        for (int pass = 0; pass < 2; ++pass)
        {
          krylov::basis_dots(handle, scratch, n, ld, j + 1, V, w, scratch.pass_coefficients.data(), hcol, pass == 1);
          krylov::basis_update(handle, scratch, n, ld, j + 1, V, scratch.pass_coefficients.data(), w, pass == 1);
        }
        krylov::basis_scale_store(handle, scratch, n, w, w, v_f32, hcol + j + 1);
        fetch(j + 2);
        std::copy(host, host + j + 2, c);
      }
      res = col.rotate();
      ++it;
      // a breakdown is not taken at its word (a singular Hessenberg matrix also gives |g_{j+1}| = 0): the cycle ends, and the
      // residual recomputed below is what is recorded and tested
      if (!col.breakdown)
        record(residual_history, history_len, 0, it, res);
      converged = !col.breakdown && res <= tolerance;
    }
    col.solve(y_host);
    MFMG_HIP_CHECK(hipMemcpyAsync(y_dev, y_host, sizeof(double) * col.k, hipMemcpyHostToDevice, handle.stream));
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream)); // (y_host is written again by the next cycle / the next solve)
    krylov::basis_combine(handle, n, ld, col.k, Z, y_dev, x_run);
    // after a restart and after a breakdown the residual is the true one, recomputed
    if (!converged && (it < max_iterations || col.breakdown))
    {
      res = start_cycle();
      ++cycle_starts;
      converged = res <= tolerance;
      if (col.breakdown)
        record(residual_history, history_len, 0, it, res);
    }
  }
  out.iterations[0] = it;
  out.residuals[0] = res;
  out.converged[0] = converged;
  out.allreduces = sum_over_ranks.allreduces;
  return out;
}
} // namespace

KrylovResult solve_fgmres(KrylovSetting const &s, const double *b, double *x, double tolerance, int max_iterations, int restart, bool fp32,
                          double *residual_history, int history_len)
{
  const int64_t n = level_size(s.hierarchy, 0);
  const RunVectors run(s.perm, 1, n, b, x, n, s.work[0], s.work[1]);
  const int m = std::max(1, std::min(restart, max_iterations)); // columns a restart cycle can reach
  KrylovResult result = fgmres_run(s, run.b, run.x, tolerance, max_iterations, m, fp32, 0, residual_history, history_len);
  run.scatter();
  return result;
}

// solve_fgmres on a block of right-hand sides.  Every column owns a slot of the bases (block_krylov_basis.hpp); all live columns
// share the iteration count and, inside a restart cycle, the basis length j.  Per iteration: the cycle and the operator on every
// maximal run of consecutive live slots (Hierarchy::apply_block, Operator::apply_block), classical Gram-Schmidt twice and
// scale_store with one launch each for all live slots, ONE device-to-host copy of their j + 2 coefficients and ONE
// synchronisation, then the rotations per column on the host (FgmresColumn).  A column that converges inside a cycle gets its
// x += Z y at once and leaves the live list; no basis vector is ever copied -- the slots left behind stay where they are until
// the cycle ends, and the next cycle packs the surviving columns into the first slots by changing the slot -> column map alone
// (block_krylov_basis::plan).  A column that breaks down ends its cycle by itself and would be out of step: it gets its update,
// and fgmres_run finishes it from (x, it) -- all a cycle start knows.  Every kernel gives a slot the bits the one-vector driver
// gives its vector, so x, the count, the final residual and the history of a column are those of solve_fgmres.
// Several ranks: the blocks hold the ranks' local vectors.  The operator and the cycle exchange what they read (a group of columns
// one message per neighbour where the ranks agreed on blocks); the Gram-Schmidt passes, the norms and scale_store run over the
// owned entries of all live slots in one launch each (the OwnedBox overloads of block_krylov_basis.hpp), the combination over all
// local entries.  The j + 1 coefficients of a pass of ALL live slots cross the ranks in ONE all-reduce, their ||w||^2 in one more:
// three per iteration whatever k, plus one per cycle start.  The Hessenberg columns are on the host once summed: no fetch.  Every
// control decision -- convergence, breakdown, retirement, restart, the end of the loop -- is taken from all-reduced values, so
// every rank retires the same columns, hands the same column to fgmres_run (collective there) and leaves the loop in the same
// iteration.  A column has the bits of the one-vector solve on the same ranks where the transport sums an element in the same
// order whatever the length of the message (block_krylov.hpp).
KrylovResult solve_fgmres_block(KrylovSetting const &s, int k, int64_t ld, const double *b, double *x, const double *tolerances,
                                int max_iterations, int restart, bool fp32, double *residual_history, int history_ld)
{
  refuse_outer(s, "block FGMRES is not implemented for an outer operator (the high-order preconditioner)");
  namespace bkb = block_krylov_basis;
  HipHandle &handle = s.handle;
  const int64_t n = level_size(s.hierarchy, 0);
  const int m = std::max(1, std::min(restart, max_iterations)); // columns a restart cycle can reach
  auto op = s.hierarchy.levels()[0].get_operator();
  // several ranks: the passes over the owned entries, summed over the ranks (the preconditions of fgmres_run)
  const bool distributed = handle.comm.enabled();
  const krylov::OwnedBox box = distributed ? fine_owned_box<InvalidArgumentExc>(s, n) : krylov::OwnedBox();
  // Without a permutation the bases take the caller's leading dimension, so that the operator runs from the caller's x into the
  // basis on one block layout.
  const bool permute = s.perm != nullptr;
  const int64_t wld = permute ? n + (n & 1) : ld;
  BlockFgmresWorkspace &ws = s.workspaces.block_fgmres;
  reserve_or_empty(ws, wld, k, m, permute, fp32, handle.stream);
  const RunVectors run(s.perm, k, ld, b, x, wld, ws.B.data(), ws.X.data());
  bkb::Scratch &scratch = *ws.scratch;
  const bkb::Basis V{n, wld, (int64_t)k * wld, ws.V.data()}, Z{n, wld, (int64_t)k * wld, ws.Z.data()};
  const int64_t cstride = ws.columns + 1, ystride = ws.columns;
  double *const coef = ws.coefficients.data();
  double *const host = ws.host.get();
  float *const v_f32 = fp32 ? ws.v_f32.data() : nullptr;
  const bool zero_first = !s.hierarchy.is_preconditioner(); // the cycle then starts from what z holds: from zero, as in fgmres_run
  const int64_t launches_before = block_kernel_launches(s.hierarchy);
  int64_t preconditioner_columns = 0, operator_columns = 0, cycle_starts = 0;
  const int64_t fp32_launches_before = fp32 ? s.fine_f32->block_launches() : 0;
  int64_t fp32_columns_looped = 0;

  std::vector<int32_t> live(k, 1), slot_col(k), run_start(k), run_width(k), run_groups(k), group_width(k), packed(k);
  for (int sl = 0; sl < k; ++sl)
    slot_col[sl] = sl;
  int n_live = k;
  KrylovResult result(k);
  std::vector<double> &res = result.residuals;
  std::vector<int32_t> &iterations = result.iterations;
  std::vector<char> &converged = result.converged;
  std::vector<FgmresColumn> columns(k, FgmresColumn(m));

  auto live_list = [&] {
    bkb::SlotList l;
    for (int sl = 0; sl < k; ++sl)
      if (live[sl])
      {
        l.id[l.count] = sl;
        l.col[l.count++] = slot_col[sl];
      }
    return l;
  };
  // the first `count` coefficients of every slot in `l`: the one round trip of an iteration.  One copy from the first to the
  // last of the slots; the coefficients of slot sl are then at fetched(l, sl)
  auto fetch = [&](bkb::SlotList const &l, int count) {
    const int first = l.id[0], last = l.id[l.count - 1];
    MFMG_HIP_CHECK(hipMemcpyAsync(host, coef + first * cstride, sizeof(double) * ((last - first) * cstride + count), hipMemcpyDeviceToHost,
                                  handle.stream));
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream));
  };
  auto fetched = [&](bkb::SlotList const &l, int sl) { return host + (sl - l.id[0]) * cstride; };
  // (`host` holds slots x (2 columns + 1) doubles: the live slots' coefficients of a pass fit)
  RankSum sum_over_ranks{handle, host};
  // ||w_s||^2 over the owned entries of all ranks from this rank's norm partials, for the slots of `l` in the order of the list:
  // on the device (scratch.norm_squared) and in `host`
  auto norms_squared_of_all = [&](bkb::SlotList const &l) {
    bkb::norm_finish(handle, scratch, l, box);
    sum_over_ranks(scratch.norm_squared.data(), l.count, scratch.norm_squared.data());
  };
  // the float copies of the vectors v_s at `v` as the one-vector driver makes them on ranks: the whole local vector (what its
  // ghost entries hold is exchanged over by the FP32 level where it reads them)
  auto narrow_live = [&](bkb::SlotList const &l, double const *v) {
    if (fp32)
      for (int i = 0; i < l.count; ++i)
        vec::narrow(handle, n, v + l.id[i] * wld, v_f32 + l.id[i] * wld);
  };
  // `body(start, width)` for every maximal run of consecutive live slots (with `by_column`: whose columns follow each other too)
  auto for_runs = [&](bool by_column, std::function<void(int, int)> const &body) {
    int32_t n_groups = 0, n_packed = 0;
    const int n_runs = bkb::plan(k, live.data(), slot_col.data(), run_start.data(), run_width.data(), run_groups.data(), group_width.data(),
                                 &n_groups, packed.data(), &n_packed);
    for (int r = 0; r < n_runs; ++r)
    {
      int s0 = run_start[r];
      const int end = s0 + run_width[r];
      for (int sl = s0 + 1; sl <= end; ++sl)
        if (sl == end || (by_column && slot_col[sl] != slot_col[sl - 1] + 1))
        {
          body(s0, sl - s0);
          s0 = sl;
        }
    }
  };
  // v_0 = r / ||r|| with r = b - A x for every live slot (and its float copy); res[column] = ||r||
  auto start_cycle = [&] {
    const bkb::SlotList l = live_list();
    for_runs(true, [&](int s0, int width) {
      BlockViews xv(handle, n, wld, width, run.x + slot_col[s0] * wld), rv(handle, n, wld, width, V.vector(0, s0));
      op->apply_block(xv.cptr, rv.ptr);
    });
    for (int i = 0; i < l.count; ++i)
      vec::sadd<double>(handle, n, -1., 1., run.b + l.col[i] * wld, V.vector(0, l.id[i]));
    cycle_starts += l.count;
    if (distributed)
    {
      bkb::norm_partials(handle, scratch, l, box, wld, V.vector(0));
      norms_squared_of_all(l);
      for (int i = 0; i < l.count; ++i)
        res[l.col[i]] = std::sqrt(host[i]);
      bkb::scale_store(handle, l, box, wld, scratch.norm_squared.data(), V.vector(0), V.vector(0), nullptr, 0);
      narrow_live(l, V.vector(0));
      return;
    }
    bkb::norm_partials(handle, scratch, l, n, wld, V.vector(0));
    bkb::scale_store(handle, scratch, l, n, wld, V.vector(0), V.vector(0), v_f32, coef, cstride);
    fetch(l, 1);
    for (int i = 0; i < l.count; ++i)
      res[l.col[i]] = fetched(l, l.id[i])[0];
  };
  // z_j = M^-1 v_j on the live slots, from a zero start whatever "is preconditioner" says
  auto precondition = [&](int j) {
    if (fp32)
    {
      // the FP32 cycle on every run of live slots, on the float copies scale_store left
      for_runs(false, [&](int s0, int width) {
        float *const zf = ws.z_f32.data() + s0 * wld;
        if (zero_first)
          for (int c = 0; c < width; ++c)
            MFMG_HIP_CHECK(hipMemsetAsync(zf + c * wld, 0, sizeof(float) * n, handle.stream));
        s.fine_f32->apply_block(width, wld, v_f32 + s0 * wld, zf);
        fp32_columns_looped += s.fine_f32->block_columns_looped();
        for (int c = 0; c < width; ++c)
          vec::widen(handle, n, zf + c * wld, Z.vector(j, s0 + c));
      });
      return;
    }
    for_runs(false, [&](int s0, int width) {
      if (zero_first)
        MFMG_HIP_CHECK(hipMemsetAsync(Z.vector(j, s0), 0, sizeof(double) * (size_t)wld * width, handle.stream));
      BlockViews vv(handle, n, wld, width, V.vector(j, s0)), zv(handle, n, wld, width, Z.vector(j, s0));
      TimerSubsection apply(s.timer, "Apply");
      s.hierarchy.apply_block(vv.cptr, zv.ptr);
    });
  };
  // x_col += Z y over the j columns of this cycle for the slots of `l`, each with its own y
  auto combine = [&](bkb::SlotList const &l, int j) {
    const int first = l.id[0], last = l.id[l.count - 1];
    double *const y_host = ws.host_y();
    for (int i = 0; i < l.count; ++i)
      columns[l.col[i]].solve(y_host + l.id[i] * ystride);
    MFMG_HIP_CHECK(hipMemcpyAsync(ws.y.data() + first * ystride, y_host + first * ystride, sizeof(double) * ((last - first) * ystride + j),
                                  hipMemcpyHostToDevice, handle.stream));
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream)); // (the host copy of y is written again by the next retirement)
    bkb::combine(handle, l, Z, j, ws.y.data(), ystride, run.x, wld);
  };
  auto retire_converged_at_start = [&] {
    for (int sl = 0; sl < k; ++sl)
      if (live[sl] && res[slot_col[sl]] <= tolerances[slot_col[sl]])
      {
        converged[slot_col[sl]] = 1;
        live[sl] = 0;
        --n_live;
      }
  };

  start_cycle();
  for (int c = 0; c < k; ++c)
    record(residual_history, history_ld, c, 0, res[c]);
  retire_converged_at_start();
  int it = 0;
  while (n_live > 0 && it < max_iterations)
  {
    for (int sl = 0; sl < k; ++sl)
      if (live[sl])
        columns[slot_col[sl]].begin_cycle(res[slot_col[sl]]);
    int j = 0;
    for (; j < m && it < max_iterations && n_live > 0; ++j)
    {
      const bkb::SlotList l = live_list();
      precondition(j);
      preconditioner_columns += l.count;
      for_runs(false, [&](int s0, int width) {
        BlockViews zv(handle, n, wld, width, Z.vector(j, s0)), wv(handle, n, wld, width, V.vector(j + 1, s0));
        op->apply_block(zv.cptr, wv.ptr);
      });
      operator_columns += l.count;
      double *const w = V.vector(j + 1);
      if (distributed)
      {
        // the columns h_0 .. h_j, ||w|| of all live slots are summed over the ranks on their way: no fetch
        for (int pass = 0; pass < 2; ++pass)
        {
          bkb::dots(handle, scratch, l, box, V, j + 1, w, nullptr, 0, false);
          sum_over_ranks(scratch.pass_coefficients.data(), l.count * (j + 1), scratch.pass_coefficients.data());
          for (int i = 0; i < l.count; ++i)
          {
            double *const c = columns[l.col[i]].column(j);
            double const *const sum = host + (size_t)i * (j + 1);
            for (int q = 0; q <= j; ++q)
              c[q] = pass == 0 ? sum[q] : c[q] + sum[q];
          }
          bkb::update(handle, scratch, l, box, V, j + 1, w, pass == 1);
        }
        norms_squared_of_all(l);
        for (int i = 0; i < l.count; ++i)
          columns[l.col[i]].column(j)[j + 1] = std::sqrt(host[i]);
        bkb::scale_store(handle, l, box, wld, scratch.norm_squared.data(), w, w, nullptr, 0);
        narrow_live(l, w);
      }
      else
      {
        for (int pass = 0; pass < 2; ++pass)
        {
          bkb::dots(handle, scratch, l, V, j + 1, w, coef, cstride, pass == 1);
          bkb::update(handle, scratch, l, V, j + 1, w, pass == 1);
        }
        bkb::scale_store(handle, scratch, l, n, wld, w, w, v_f32, coef + j + 1, cstride);
        fetch(l, j + 2);
      }
      ++it;
      bkb::SlotList leaving, broken;
      for (int i = 0; i < l.count; ++i)
      {
        const int sl = l.id[i], c = l.col[i];
        FgmresColumn &col = columns[c];
        if (!distributed)
          std::copy(fetched(l, sl), fetched(l, sl) + j + 2, col.column(j));
        const double r = col.rotate();
        iterations[c] = it;
        // a breakdown is not taken at its word: the column gets its update, and the residual fgmres_run recomputes is what is
        // recorded and tested
        if (!col.breakdown)
        {
          res[c] = r;
          record(residual_history, history_ld, c, it, r);
          converged[c] = r <= tolerances[c];
        }
        if (col.breakdown || converged[c])
        {
          leaving.id[leaving.count] = sl;
          leaving.col[leaving.count++] = c;
          live[sl] = 0;
          --n_live;
        }
        if (col.breakdown)
          broken.col[broken.count++] = c;
      }
      if (leaving.count > 0)
        combine(leaving, j + 1);
      for (int i = 0; i < broken.count; ++i)
      {
        // (the one-vector loop from this column's x and the shared count: the cycle start is the whole state)
        const int c = broken.col[i];
        const KrylovResult out = fgmres_run(s, run.b + c * wld, run.x + c * wld, tolerances[c], max_iterations, m, fp32, it,
                                             residual_history ? residual_history + (int64_t)c * history_ld : nullptr, history_ld);
        iterations[c] = out.iterations[0];
        res[c] = out.residuals[0];
        converged[c] = out.converged[0];
        cycle_starts += out.work[3];
        sum_over_ranks.allreduces += out.allreduces;
        preconditioner_columns += out.iterations[0] - it;
        operator_columns += out.iterations[0] - it;
      }
    }
    if (n_live > 0)
      combine(live_list(), j);
    if (n_live == 0 || it >= max_iterations)
      break;
    // restart: the survivors move to the first slots (the map alone changes), the residual is the true one, recomputed
    {
      int32_t n_groups = 0, n_packed = 0;
      bkb::plan(k, live.data(), slot_col.data(), run_start.data(), run_width.data(), run_groups.data(), group_width.data(), &n_groups,
                packed.data(), &n_packed);
      for (int sl = 0; sl < k; ++sl)
      {
        live[sl] = sl < n_packed;
        if (sl < n_packed)
          slot_col[sl] = packed[sl];
      }
    }
    start_cycle();
    retire_converged_at_start();
  }
  run.scatter();
  result.work[0] = preconditioner_columns;
  result.work[1] = operator_columns;
  result.work[2] = block_kernel_launches(s.hierarchy) - launches_before;
  result.work[3] = cycle_starts;
  result.allreduces = sum_over_ranks.allreduces;
  if (fp32)
  {
    // (the preconditioner applications of this solve)
    result.block_info_f32[0] = s.fine_f32->block_width();
    result.block_info_f32[1] = s.fine_f32->block_launches() - fp32_launches_before;
    result.block_info_f32[2] = fp32_columns_looped;
  }
  return result;
}
} // namespace mfmg
