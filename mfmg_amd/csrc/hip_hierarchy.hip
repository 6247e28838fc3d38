// Implementation of the HIP back-end classes declared in mfmg/hip_hierarchy_helpers.hpp.
#include "mfmg/hierarchy.hpp" // (HipFloatFineLevel runs the coarse part of the cycle)
#include "mfmg/hip_hierarchy_helpers.hpp"
#include "probe_assembly.hpp"

#include <algorithm>
#include <chrono>
#include <cctype>
#include <cmath>

namespace mfmg
{
namespace
{
std::string to_lower(std::string s)
{
  std::transform(s.begin(), s.end(), s.begin(), [](unsigned char c) { return std::tolower(c); });
  return s;
}

// One workgroup, right-hand side resident in LDS: forward substitution with the unit lower factor,
// backward substitution with U, column sweeps (coalesced in the column-major packed LU).
__global__ void dense_lu_solve_kernel(int n, double const *lu, int32_t const *perm, double const *b, double *x)
{
  extern __shared__ double y[];
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < n; i += nt)
    y[i] = b[perm[i]];
  __syncthreads();
  for (int j = 0; j < n - 1; ++j)
  {
    const double yj = y[j];
    double const *col = lu + (size_t)j * n;
    for (int i = j + 1 + tid; i < n; i += nt)
      y[i] -= col[i] * yj;
    __syncthreads();
  }
  for (int j = n - 1; j >= 0; --j)
  {
    double const *col = lu + (size_t)j * n;
    if (tid == 0)
      y[j] /= col[j];
    __syncthreads();
    const double yj = y[j];
    for (int i = tid; i < j; i += nt)
      y[i] -= col[i] * yj;
    __syncthreads();
  }
  for (int i = tid; i < n; i += nt)
    x[i] = y[i];
}

std::shared_ptr<SparseMatrixDevice<double>> upload(HipHandle &handle, HostCsr &&m, bool analyse = true)
{
  return std::make_shared<SparseMatrixDevice<double>>(handle, m.n_rows, m.n_cols, std::move(m.row_ptr),
                                                      std::move(m.col), std::move(m.val), true, analyse);
}
} // namespace

double distributed_dot(HipHandle &handle, int space, DVector const &x, DVector const &y)
{
  if (!handle.comm.enabled() || space <= 0)
    return x * y;
  HaloSpace const &s = handle.comm.spaces[space];
  if (!s.split_xy())
  {
    const int64_t off = s.owned_begin * s.layer_elems, n = s.owned_count * s.layer_elems;
    const double local = vec::dot<double>(handle, n, x.get_values() + off, y.get_values() + off);
    return handle.allreduce_sum(local);
  }
  // boxes: the owned entries are a sub-box of the local array -- packed, then the same dot product (setup and monitoring only)
  const int64_t n = s.n_owned();
  if ((int64_t)handle.dot_scratch.size() < 2 * n)
    handle.dot_scratch.resize((size_t)2 * n);
  double *a = handle.dot_scratch.data(), *b = a + n;
  halo_box_copy(const_cast<double *>(x.get_values()), s, true, a, 0, handle.stream);
  halo_box_copy(const_cast<double *>(y.get_values()), s, true, b, 0, handle.stream);
  return handle.allreduce_sum(vec::dot<double>(handle, n, a, b));
}

namespace
{
// rows this rank does not own become empty: a rank computes only the rows it owns
void empty_rows_outside(HostCsr &m, HaloSpace const &space)
{
  std::vector<int32_t> rp(m.n_rows + 1, 0), cl;
  std::vector<double> vl;
  cl.reserve(m.col.size());
  vl.reserve(m.val.size());
  for (int64_t r = 0; r < m.n_rows; ++r)
  {
    if (space.owned(r))
      for (int p = m.row_ptr[r]; p < m.row_ptr[r + 1]; ++p)
      {
        cl.push_back(m.col[p]);
        vl.push_back(m.val[p]);
      }
    rp[r + 1] = (int32_t)cl.size();
  }
  m.row_ptr.swap(rp);
  m.col.swap(cl);
  m.val.swap(vl);
}
} // namespace

void dense_lu_solve(HipHandle &handle, int n, double const *lu, int32_t const *perm, double const *b, double *x)
{
  if (n <= 0)
    return;
  const int threads = n >= 1024 ? 1024 : (n >= 256 ? 256 : 64);
  static int attr_device = -1; // (the attribute is per device)
  int dev = 0;
  MFMG_HIP_CHECK(hipGetDevice(&dev));
  if (attr_device != dev)
  {
    MFMG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(dense_lu_solve_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    attr_device = dev;
  }
  hipLaunchKernelGGL(dense_lu_solve_kernel, dim3(1), dim3(threads), (size_t)n * sizeof(double), handle.stream, n,
                     lu, perm, b, x);
  MFMG_HIP_CHECK(hipGetLastError());
}

// ---- evaluators ------------------------------------------------------------------
HipMeshEvaluator::HipMeshEvaluator(HipHandle &handle, mfmg_hip_mesh_desc const &mesh)
    : _handle(handle), _desc(mesh), _mesh(StructuredMesh::from_desc(mesh, handle.stream))
{
  // the hierarchy outlives the caller's arrays: setup works from the host copy
  _desc.cell_dofs = _mesh.cell_dofs.data();
  _desc.coefficient = _mesh.coefficient.data();
  _desc.constrained = _mesh.constrained.data();
  _desc.arrays_on_device = 0;
}

std::shared_ptr<SparseMatrixDevice<double>> HipMeshEvaluator::evaluate_global() const
{
  // (formed on the device: the host assembly of the 458 M entries of a 257^3-DoF matrix took 2.9 s; MFMG_ASSEMBLE_ON_HOST=1
  // keeps the host path, which the tests compare with)
  static const bool on_host = std::getenv("MFMG_ASSEMBLE_ON_HOST") != nullptr && std::string(std::getenv("MFMG_ASSEMBLE_ON_HOST")) == "1";
  if (on_host)
    return upload(_handle, assemble_global_matrix(_mesh, ConstraintSemantics::assembled));
  return fine_operator_on_device(_handle, _mesh, false);
}

std::vector<double> HipMeshEvaluator::get_locally_relevant_diag() const
{
  return operator_diagonal(_mesh, ConstraintSemantics::assembled);
}

RestrictorOptions HipMeshEvaluator::agglomerate_options(ptree const &params) const
{
  RestrictorOptions o;
  o.agglomerate[0] = params.get("agglomeration.nx", 2);
  o.agglomerate[1] = params.get("agglomeration.ny", 2);
  o.agglomerate[2] = params.get("agglomeration.nz", 2);
  std::string const partitioner = params.get("agglomeration.partitioner", "block");
  ASSERT_THROW(partitioner == "block", "only the block partitioner is available (zoltan/metis are mesh-library "
                                       "bound and out of scope): \"" +
                                           partitioner + "\"");
  o.n_eigenvectors = params.get("eigensolver.number of eigenvectors", 1);
  // AMGe_device ignores eigensolver.type: dense, unshifted, first columns
  // (include/mfmg/cuda/amge_device.templates.cuh:256-310)
  o.variant = params.get("eigensolver.variant", "device");
  // "lapack" (first columns of the dense solver, what AMGe_device does) is not unique inside degenerate
  // eigenspaces and picks unit vectors of constrained DoFs; the default here is the Krylov rule, which
  // is basis independent and never selects them
  o.selection = params.get("eigensolver.selection", "krylov");
  // the reference device test poses the agglomerate problems without the coefficient
  // (tests/test_hierarchy_device.cu:239-244)
  o.use_coefficient = params.get("eigensolver.use_coefficient", true);
  // "restrictor.eigensolver lanczos": the keys of the reference's input file (amge_host.templates.hpp:165-200), the tolerance as
  // given (the reference clamps it to >= 1e-4 because its Lanczos does not reorthogonalise; this one does)
  if (params.get("restrictor.eigensolver", "device") == std::string("lanczos"))
  {
    o.solver = "lanczos";
    o.tolerance = params.get("eigensolver.tolerance", 1e-14);
    o.max_iterations = params.get("eigensolver.max_iterations", 200);
    o.percent_overshoot = params.get("eigensolver.percent_overshoot", 5);
  }
  return o;
}

HipMatrixFreeMeshEvaluator::HipMatrixFreeMeshEvaluator(HipHandle &handle, mfmg_hip_mesh_desc const &mesh)
    : HipMeshEvaluator(handle, mesh)
{
  // (from the caller's arrays: when they are on the device already, the host copy of the base class need not travel back)
  _op = std::make_shared<MatrixFreeLaplaceDevice<double>>(handle, mesh, handle.allow_cell_constant);
  HaloCommunicator &c = handle.comm;
  if (c.enabled())
  {
    // fine DoF space: the nodes of the local (extended) mesh; per axis the owned planes [z0, z1) (+ the top plane on the
    // last rank of the axis); the planes below / above belong to the neighbours
    ASSERT_THROW(_mesh.dim == 3, "distributed runs need a 3-D mesh");
    HaloSpace &s = c.spaces[1];
    s = HaloSpace();
    s.comps = 1;
    s.layer_elems = (int64_t)_mesh.N[0] * _mesh.N[1];
    s.n_layers = _mesh.N[2];
    s.width = 1; // operator applications read one plane of each neighbour
    for (int d = 0; d < 3; ++d)
    {
      const bool low = c.ghost_lo[d] > 0, high = c.ghost_hi[d] > 0;
      ASSERT_THROW(low == c.has_lower(d) && high == c.has_upper(d), "ghost cell layers do not match the grid of ranks");
      const int64_t own0 = c.ghost_lo[d], own_n = _mesh.N[d] - c.ghost_lo[d] - (high ? c.ghost_hi[d] + 1 : 0);
      // equal boxes: every rank owns the same number of cell layers, so the global position follows from the rank
      const int64_t own_cells = _mesh.n[d] - c.ghost_lo[d] - c.ghost_hi[d];
      const int64_t g0 = (int64_t)c.coord[d] * own_cells - c.ghost_lo[d], gn = (int64_t)c.grid[d] * own_cells + 1;
      ASSERT_THROW(own_n >= 2 && own_n % 2 == (high ? 0 : 1), "the owned box must hold a whole number of agglomerates per axis");
      if (d == 2)
      {
        s.has_low = low;
        s.has_high = high;
        s.owned_begin = own0;
        s.owned_count = own_n;
        s.global_begin = g0;
        s.global_layers = gn;
      }
      else
      {
        s.n_xy[d] = _mesh.N[d];
        s.low_xy[d] = low;
        s.high_xy[d] = high;
        s.own0_xy[d] = own0;
        s.own_n_xy[d] = own_n;
        s.g0_xy[d] = g0;
        s.gn_xy[d] = gn;
      }
    }
    // local numbering must be lexicographic so that planes are contiguous
    for (int64_t nd = 0; nd < (int64_t)_mesh.node_dof.size(); nd += std::max<int64_t>(1, (int64_t)_mesh.node_dof.size() / 4099))
      ASSERT_THROW(_mesh.node_dof[nd] == nd, "distributed runs need lexicographic local DoF numbering");
  }
}

std::shared_ptr<DVector> HipMatrixFreeMeshEvaluator::build_range_vector() const
{
  return std::make_shared<DVector>(_handle, _mesh.n_dofs);
}

void HipMatrixFreeMeshEvaluator::matrix_free_evaluate_global(DVector const &src, DVector &dst) const
{
  _op->vmult(src.get_values(), dst.get_values());
}

double const *HipMatrixFreeMeshEvaluator::matrix_free_get_diagonal_inverse() const
{
  return _op->diagonal_inverse();
}

std::vector<double> HipMatrixFreeMeshEvaluator::get_diagonal() const
{
  std::vector<double> d(_mesh.n_dofs);
  MFMG_HIP_CHECK(hipMemcpyAsync(d.data(), _op->diagonal(), d.size() * sizeof(double), hipMemcpyDeviceToHost,
                                _handle.stream));
  MFMG_HIP_CHECK(hipStreamSynchronize(_handle.stream));
  return d;
}

RestrictorOptions HipMatrixFreeMeshEvaluator::agglomerate_options(ptree const &params) const
{
  RestrictorOptions o = HipMeshEvaluator::agglomerate_options(params);
  // matrix-free agglomerate operator + Krylov eigensolver semantics
  // (include/mfmg/dealii/amge_host.templates.hpp:278-350)
  o.variant = params.get("eigensolver.variant", "mf");
  o.selection = params.get("eigensolver.selection", "krylov");
  return o;
}

// ---- HipMatrixOperator ---------------------------------------------------------
HipMatrixOperator::HipMatrixOperator(std::shared_ptr<SparseMatrixDevice<double>> sparse_matrix)
    : _matrix(std::move(sparse_matrix))
{
  ASSERT_THROW(_matrix != nullptr, "The matrix must exist");
}

std::shared_ptr<SparseMatrixDevice<double>> HipMatrixOperator::get_transposed_matrix() const
{
  if (!_transposed_matrix)
    _transposed_matrix = _matrix->transpose();
  return _transposed_matrix;
}

void HipMatrixOperator::apply(DVector const &x, DVector &y, OperatorMode mode) const
{
  if (mode == OperatorMode::NO_TRANS)
  {
    ASSERT_THROW(x.size() == _matrix->n() && y.size() == _matrix->m(), "vector sizes do not match the operator");
    _matrix->handle().exchange(_domain_space, const_cast<double *>(x.get_values()));
    if (_structured)
      _structured->restrict_to_coarse(x.get_values(), y.get_values());
    else
      _matrix->vmult(y.get_values(), x.get_values());
    if (_reverse_range_space > 0)
      _matrix->handle().exchange_reverse_add(_reverse_range_space, y.get_values());
  }
  else
  {
    ASSERT_THROW(x.size() == _matrix->m() && y.size() == _matrix->n(), "vector sizes do not match the operator");
    _matrix->handle().exchange(_range_space, const_cast<double *>(x.get_values()));
    if (_structured)
      _structured->prolongate(x.get_values(), y.get_values(), false);
    else
      get_transposed_matrix()->vmult(y.get_values(), x.get_values());
  }
}

void HipMatrixOperator::apply_plus_scaled(DVector const &x, double const *dinv, DVector const &b, double beta, DVector &y) const
{
  ASSERT_THROW(x.size() == _matrix->n() && y.size() == _matrix->m() && b.size() == _matrix->m() && dinv != nullptr,
               "vector sizes do not match the operator");
  _matrix->handle().exchange(_domain_space, const_cast<double *>(x.get_values()));
  _matrix->vmult_plus_scaled(y.get_values(), x.get_values(), dinv, b.get_values(), beta);
}

void HipMatrixOperator::residual(DVector const &x, DVector const &b, DVector &res) const
{
  _matrix->handle().exchange(_domain_space, const_cast<double *>(x.get_values()));
  _matrix->residual(x.get_values(), b.get_values(), res.get_values());
}

void HipMatrixOperator::apply_subtract(DVector const &x, DVector &y, OperatorMode mode) const
{
  _matrix->handle().exchange(mode == OperatorMode::NO_TRANS ? _domain_space : _range_space,
                             const_cast<double *>(x.get_values()));
  if (mode == OperatorMode::NO_TRANS)
    _matrix->vmult_subtract(y.get_values(), x.get_values());
  else if (_structured)
    _structured->prolongate(x.get_values(), y.get_values(), true);
  else
    get_transposed_matrix()->vmult_subtract(y.get_values(), x.get_values());
}

bool HipMatrixOperator::prepare_residual_restriction(std::shared_ptr<Operator<DVector> const> a)
{
  _rr_operator.reset();
  HipHandle &hd = _matrix->handle();
  auto ha = std::dynamic_pointer_cast<HipOperator const>(a);
  if (!_structured || !ha)
    return false;
  const bool distributed = hd.comm.enabled();
  if (distributed && !(_domain_space == 1 && _range_space == 2))
    return false;
  const int64_t n = _matrix->n(), nc = _matrix->m();
  auto apply_a = [&](double const *v, double *w) {
    DVector vv(hd, n, const_cast<double *>(v)), ww(hd, n, w);
    ha->apply_local(vv, ww);
  };
  StructuredRestrictorDevice::SlabInfo slab;
  if (distributed)
  {
    HaloSpace const &f = hd.comm.spaces[1], &c = hd.comm.spaces[2];
    slab.valid_begin = (int)f.owned_begin;
    slab.valid_end = (int)(f.owned_begin + f.owned_count);
    slab.has_low = f.has_low;
    slab.has_high = f.has_high;
    slab.owned_begin = (int)c.owned_begin;
    slab.owned_end = (int)(c.owned_begin + c.owned_count);
    for (int d = 0; d < 2; ++d)
    {
      slab.valid_begin_xy[d] = (int)f.own0_xy[d];
      slab.valid_end_xy[d] = (int)(f.own0_xy[d] + f.own_n_xy[d]);
      slab.has_low_xy[d] = f.low_xy[d];
      slab.has_high_xy[d] = f.high_xy[d];
      slab.owned_begin_xy[d] = (int)c.own0_xy[d];
      slab.owned_end_xy[d] = (int)(c.own0_xy[d] + c.own_n_xy[d]);
    }
  }
  double ok = _structured->build_residual_restriction(apply_a, slab) ? 1. : 0.;
  if (distributed)
  {
    // all ranks or none (a slab too thin to hold a representative of its classes says no): the path changes the exchanges
    ok = -hd.allreduce_max(-ok);
    // the 5 node layers around the top agglomerates of the slab reach one layer further than an operator application
    HaloSpace const &f = hd.comm.spaces[1];
    for (int d = 0; d < 3; ++d)
      if (ok > 0. && ((f.low(d) && f.own0(d) < 2) || (f.high(d) && f.dim(d) - f.own0(d) - f.own_n(d) < 2)))
        ok = 0.;
  }
  if (ok == 0.)
  {
    _structured->drop_residual_restriction();
    return false;
  }
  if (distributed && _rr_space == 0)
  {
    HaloSpace two = hd.comm.spaces[1];
    two.width = 2;
    _rr_space = hd.comm.add_space(two);
  }
  // the check: a random pair (x, b), the one-pass result against residual + restriction (owned rows, all ranks)
  std::vector<double> hx(n), hb(n);
  uint64_t state = 0x9e3779b97f4a7c15ull + (uint64_t)hd.comm.rank * 0x632be59bd9b4e019ull;
  auto next = [&state] {
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return double((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0) - 0.5;
  };
  for (int64_t i = 0; i < n; ++i)
  {
    hx[i] = next();
    hb[i] = next();
  }
  DVector x(hd, n), b(hd, n), res(hd, n), two_step(hd, nc), one_pass(hd, nc);
  MFMG_HIP_CHECK(hipMemcpyAsync(x.get_values(), hx.data(), n * sizeof(double), hipMemcpyHostToDevice, hd.stream));
  MFMG_HIP_CHECK(hipMemcpyAsync(b.get_values(), hb.data(), n * sizeof(double), hipMemcpyHostToDevice, hd.stream));
  a->residual(x, b, res);
  apply(res, two_step);
  _rr_operator = a;
  restrict_residual(*a, x, b, one_pass);
  _rr_operator.reset();
  const double scale = std::sqrt(distributed_dot(hd, _range_space, two_step, two_step));
  one_pass.add(-1., two_step);
  const double diff = std::sqrt(distributed_dot(hd, _range_space, one_pass, one_pass));
  if (std::getenv("MFMG_DEBUG_RR"))
    fprintf(stderr, "[rr] rank %d: %d classes, one pass against two steps: difference %.3e of %.3e\n", hd.comm.rank,
            _structured->residual_restriction_classes(), diff, scale);
  if (!(diff <= 1e-12 * scale))
  {
    _structured->drop_residual_restriction(); // the operator does not repeat itself the way the classes assume
    return false;
  }
  _rr_operator = a;
  return true;
}

bool HipMatrixOperator::restrict_residual(Operator<DVector> const &a, DVector const &x, DVector const &b, DVector &b_coarse) const
{
  if (_rr_operator.get() != &a || !_structured || !_structured->has_residual_restriction())
    return false;
  ASSERT_THROW(x.size() == _matrix->n() && b.size() == _matrix->n() && b_coarse.size() == _matrix->m(),
               "vector sizes do not match the operator");
  HipHandle &hd = _matrix->handle();
  ASSERT_THROW(!hd.comm.enabled() || _domain_space == 1, "internal: the one-pass residual restriction reads b in the fine DoF space");
  // distributed runs: two exchanges as in the two-step form (there: x for the residual, the residual for R) -- here x two
  // layers deep and b one layer deep
  hd.exchange(_rr_space, const_cast<double *>(x.get_values()));
  // (the ghost entries of b left at the start of the cycle, prefetch_rhs; the pre-smoother may have waited for them already)
  hd.need_rhs_ghosts(b.get_values());
  _prefetched_rhs = nullptr;
  _structured->restrict_residual(x.get_values(), b.get_values(), b_coarse.get_values());
  return true;
}

// The ghost entries of the right-hand side are read by one kernel of the cycle, the restriction of the residual (the smoother
// reads b at the DoFs a rank owns).  They are refreshed on the exchange stream at the start of the cycle, beside the
// pre-smoother, instead of by a blocking exchange in front of that kernel.
void HipMatrixOperator::prefetch_rhs(DVector const &b) const
{
  _prefetched_rhs = nullptr;
  HipHandle &hd = _matrix->handle();
  hd.rhs_in_flight = hd.rhs_fresh = nullptr;
  hd.rhs_of_cycle = b.get_values();
  const bool restriction_reads_it = _rr_operator && _structured && _structured->has_residual_restriction();
  if (!hd.comm.enabled() || !hd.overlap_exchange || _domain_space <= 0 || b.size() != _matrix->n() ||
      !(restriction_reads_it || hd.rhs_ghosts_wanted))
    return;
  ASSERT_THROW(_domain_space == 1, "internal: the right-hand side is prefetched in the fine DoF space only");
  hd.exchange_async(hd.fine_space(hd.rhs_ghosts_wanted ? hd.rhs_ghost_width : 1), const_cast<double *>(b.get_values()));
  hd.rhs_fresh_width = hd.rhs_ghosts_wanted ? hd.rhs_ghost_width : 1;
  hd.rhs_in_flight = b.get_values();
  if (restriction_reads_it)
    _prefetched_rhs = b.get_values();
}

void HipMatrixOperator::release_rhs() const
{
  HipHandle &hd = _matrix->handle();
  if (hd.rhs_in_flight != nullptr)
    hd.exchange_async_wait(); // (nobody read the ghost entries: the exchange must still be over before the caller touches b)
  hd.rhs_in_flight = hd.rhs_fresh = hd.rhs_of_cycle = nullptr;
}

bool HipMatrixOperator::restrict_residual_f32(Operator<DVector> const &a, float const *x, float const *b, DVector &b_coarse) const
{
  if (_rr_operator.get() != &a || !_structured || !_structured->has_residual_restriction() || _matrix->handle().comm.enabled())
    return false;
  ASSERT_THROW(x != nullptr && b != nullptr && b_coarse.size() == _matrix->m(), "vector sizes do not match the operator");
  _structured->restrict_residual(x, b, b_coarse.get_values());
  return true;
}

std::shared_ptr<Operator<DVector>> HipMatrixOperator::transpose() const
{
  return std::make_shared<HipMatrixOperator>(get_transposed_matrix());
}

std::shared_ptr<Operator<DVector>> HipMatrixOperator::multiply(std::shared_ptr<Operator<DVector> const> b) const
{
  // R->multiply(A R^T) for a matrix-free A: fused triple product
  if (auto half = std::dynamic_pointer_cast<HipGalerkinHalfProduct const>(b))
  {
    ASSERT_THROW(half->get_r()->get_matrix() == _matrix, "the Galerkin product needs the same restrictor on both sides");
    auto evaluator = half->get_a() ? half->get_a()->get_mesh_evaluator() : nullptr; // (an assembled A has none)
    HipHandle &hd = _matrix->handle();
    // Distributed runs: the same probing with the colours taken on GLOBAL agglomerate coordinates; the applications of
    // R^T, A and R refresh their ghost layers by themselves, and a rank keeps the rows of the agglomerates it owns.
    // (A mesh with ghost nodes but no communicator -- one rank's local problem run alone -- keeps the host product.)
    const bool distributed = hd.comm.enabled() && _range_space > 0;
    bool ghosts = false;
    if (!hd.comm.enabled() && evaluator)
      for (uint8_t f : evaluator->get_mesh().constrained)
        if (f == 2)
        {
          ghosts = true;
          break;
        }
    if (_structured && !ghosts && hd.galerkin_on_device)
    {
      // On device, by probing (the reference's fast_ap idea,
      // source/dealii/dealii_matrix_free_hierarchy_helpers.cc:77-288): R A R^T couples an agglomerate only to the ones
      // within a reach r_d per direction, so the columns of all agglomerates with the same index mod 2 r_d + 1 in every
      // direction (and the same eigenvector) can be applied at once -- u = their indicator, y = R (A (R^T u)) with the
      // kernels of the apply path -- and row (a, e) of y is the entry towards the one agglomerate of that class near a:
      // 27 n_eig operator applications (45 n_eig with one axis of r_d = 2) instead of one per coarse column.  An agglomerate
      // of a_d cells along d spans the nodes [i a_d, (i + 1) a_d], and A couples nodes one apart, so r_d = 1 + floor(1 / a_d):
      // 1, and 2 for agglomerates one cell wide.
      const int ne = _structured->n_eigenvectors();
      int reach[3];
      for (int d = 0; d < 3; ++d)
        reach[d] = _structured->agglomerate_cells(d) == 1 ? 2 : 1;
      const int na[3] = {_structured->agglomerates(0), _structured->agglomerates(1), _structured->agglomerates(2)};
      // period and phase on the GLOBAL agglomerate index (local + offset), rows of the owned agglomerates only
      int off[3] = {0, 0, 0};
      int64_t own0[3] = {0, 0, 0}, own1[3] = {na[0], na[1], na[2]}, glob[3] = {na[0], na[1], na[2]};
      if (distributed)
      {
        HaloSpace const &cs = hd.comm.spaces[_range_space];
        cs.check();
        for (int d = 0; d < 3; ++d)
        {
          ASSERT_THROW(cs.dim(d) == na[d], "internal: coarse space does not match the agglomerate grid");
          off[d] = (int)cs.g0(d);
          own0[d] = cs.own0(d);
          own1[d] = cs.own0(d) + cs.own_n(d);
          glob[d] = cs.gn(d);
        }
      }
      const int k[3] = {(int)std::min<int64_t>(2 * reach[0] + 1, glob[0]), (int)std::min<int64_t>(2 * reach[1] + 1, glob[1]),
                        (int)std::min<int64_t>(2 * reach[2] + 1, glob[2])};
      const int64_t n_agg = (int64_t)na[0] * na[1] * na[2], nc = n_agg * ne;
      ASSERT_THROW(nc == _matrix->m(), "agglomerate grid does not match the restrictor");
      const int n_colors = k[0] * k[1] * k[2] * ne;
      // (the probes stay on the device -- 1.8 GB at 257^3 DoFs -- and the rows are assembled there: probe_assembly.hip)
      DeviceBuffer<double> Y((size_t)n_colors * (size_t)nc);
      {
        auto u = this->build_range_vector();
        auto w = half->build_range_vector();
        for (int color = 0; color < n_colors; ++color)
        {
          const int e0 = color % ne, oc = color / ne;
          const int o[3] = {oc % k[0], (oc / k[0]) % k[1], oc / (k[0] * k[1])};
          vec::probing_vector(hd, na, ne, k, o, e0, u->get_values(), off);
          half->apply(*u, *w);
          DVector y(hd, nc, Y.data() + (size_t)color * (size_t)nc);
          this->apply(*w, y);
        }
      }
      auto coarse = std::make_shared<HipMatrixOperator>(galerkin_from_probes(hd, na, ne, k, reach, off, own0, own1, Y.data()));
      coarse->set_spaces(_range_space, _range_space);
      return coarse;
    }
    if (!evaluator)
    {
      // assembled A without the preconditions of the probing: the explicit products (source/cuda/cuda_matrix_operator.cu:132-225)
      auto ap = half->get_a_matrix()->get_matrix()->mmult(*get_transposed_matrix());
      return std::make_shared<HipMatrixOperator>(_matrix->mmult(*ap));
    }
    HostCsr R, Rt;
    R.n_rows = _matrix->m();
    R.n_cols = _matrix->n();
    _matrix->download(R.row_ptr, R.col, R.val);
    Rt.n_rows = R.n_cols;
    Rt.n_cols = R.n_rows;
    csr_transpose_host<double>(R.n_rows, R.n_cols, R.row_ptr, R.col, R.val, Rt.row_ptr, Rt.col, Rt.val);
    HostCsr Ac = galerkin_triple_product(evaluator->get_mesh(), evaluator->constraint_semantics(), R, Rt);
    HipHandle &hh = _matrix->handle();
    if (hh.comm.enabled())
    {
      // rows of agglomerates owned by the neighbours are incomplete on the local mesh: a rank applies
      // only its own rows, the others arrive by halo exchange
      empty_rows_outside(Ac, hh.comm.spaces[2]);
    }
    auto coarse = std::make_shared<HipMatrixOperator>(upload(hh, std::move(Ac)));
    coarse->set_spaces(_range_space, _range_space);
    return coarse;
  }
  auto downcast_b = std::dynamic_pointer_cast<HipMatrixOperator const>(b);
  ASSERT_THROW(downcast_b != nullptr, "HipMatrixOperator::multiply needs a HipMatrixOperator");
  return std::make_shared<HipMatrixOperator>(_matrix->mmult(*downcast_b->get_matrix()));
}

std::shared_ptr<Operator<DVector>>
HipMatrixOperator::multiply_transpose(std::shared_ptr<Operator<DVector> const> b) const
{
  // C = A B^T (source/cuda/cuda_matrix_operator.cu:151-225)
  auto downcast_b = std::dynamic_pointer_cast<HipMatrixOperator const>(b);
  ASSERT_THROW(downcast_b != nullptr, "HipMatrixOperator::multiply_transpose needs a HipMatrixOperator");
  HipHandle &hd = _matrix->handle();
  // B = a restrictor with its agglomerate-wise form, one rank: A R^T stays symbolic and R->multiply forms R A R^T by probing
  // (27 n_eig applications of R^T, A, R) instead of two explicit products through 516 M + 223 M entries
  if (downcast_b->has_structured() && hd.galerkin_on_device && !hd.comm.enabled() && _matrix->m() == _matrix->n() &&
      downcast_b->get_matrix()->n() == _matrix->m())
  {
    auto self = std::make_shared<HipMatrixOperator>(_matrix);
    return std::make_shared<HipGalerkinHalfProduct>(std::shared_ptr<HipMatrixOperator const>(self), downcast_b);
  }
  return std::make_shared<HipMatrixOperator>(_matrix->mmult(*downcast_b->get_transposed_matrix()));
}

std::shared_ptr<DVector> HipMatrixOperator::build_domain_vector() const
{
  return std::make_shared<DVector>(_matrix->handle(), _matrix->n());
}

std::shared_ptr<DVector> HipMatrixOperator::build_range_vector() const
{
  return std::make_shared<DVector>(_matrix->handle(), _matrix->m());
}

size_t HipMatrixOperator::grid_complexity() const { return _matrix->m(); }

size_t HipMatrixOperator::operator_complexity() const { return _matrix->n_nonzero_elements(); }

double const *HipMatrixOperator::get_diagonal_inverse() const
{
  if (_dinv.size() == 0)
  {
    _dinv.resize(_matrix->m());
    _matrix->inverse_diagonal(_dinv.data());
  }
  return _dinv.data();
}

void HipMatrixOperator::smoother_step(DVector const &b, DVector const &x, DVector const *x_prev, double alpha,
                                      double beta, DVector &out) const
{
  _matrix->handle().exchange(_domain_space, const_cast<double *>(x.get_values()));
  _matrix->smoother_step(get_diagonal_inverse(), b.get_values(), x.get_values(),
                         x_prev ? x_prev->get_values() : nullptr, alpha, beta, out.get_values());
}

// ---- HipMatrixFreeOperator -----------------------------------------------------
HipMatrixFreeOperator::HipMatrixFreeOperator(std::shared_ptr<HipMatrixFreeMeshEvaluator> matrix_free_mesh_evaluator)
    : _mesh_evaluator(std::move(matrix_free_mesh_evaluator))
{
  ASSERT_THROW(_mesh_evaluator != nullptr, "downcasting failed");
}

// One operator application of a distributed run: the tiles that do not read a ghost plane run while the
// boundary planes travel on the second stream; the tiles next to the ghost planes follow (slabs: at most four z-tiles;
// boxes: a shell of tiles along all three axes).
// One body for the FP64 operator of the hierarchy and the FP32 operator of HipFloatFineLevel: the same regions, the same exchanges
// on the same streams (a float x travels widened, HipHandle::exchange_on).
namespace
{
template <typename T>
void distributed_apply_mode(HipHandle &handle, MatrixFreeLaplaceDevice<T> const *op, MfMode mode, MfOperands<T> const &v)
{
  auto whole = [&] { op->launch_region(mode, v, MfTileRegion::whole()); };
  // The shell around the interior tiles is ONE launch over a compact list of its tiles (MfTileRegion::outside_of: z slabs, y slabs, x
  // slabs and the tail columns; consecutive workgroups, consecutive tiles, so that the XCDs share it evenly), enqueued on the
  // EXCHANGE stream behind the unpacking: it runs beside the interior tiles and its workgroups fill the slots the interior
  // launch leaves while it drains.  Measured on one GPU with the launches of the corner rank of a 2 x 2 x 2 grid and no exchange
  // (MFMG_MF_EMULATE_SPLIT=1, 257^3 DoFs, us per operator application, start to start): one launch for the whole mesh 192;
  // interior, then the shell slab by slab (five launches, each a fraction of a round of workgroups and as long as one workgroup
  // lives: rounds 1-3) 290; interior, then the shell as one launch ("MFMG_MF_SHELL=after") 236; beside each other 218.
  // Same tiles, same bits (owner computes).  "MFMG_MF_SHELL=slabs" keeps the old launches for that comparison.
  // (HipHandle::mf_shell_mode: a test switches between the variants inside one process through the context)
  const bool shell_slabs = handle.mf_shell_mode == 2, shell_after = handle.mf_shell_mode == 1;
  // concurrent: the shell launch goes to the exchange stream, behind the unpacking, and runs BESIDE the interior tiles (its
  // workgroups fill the slots the interior launch leaves free while it drains); `stream` joins afterwards.  The two launches
  // write disjoint DoFs and read x, b and x_prev only (a term that overwrites its own x_prev reads and writes it DoF by DoF).
  auto shell = [&](int const lo[3], int const hi[3], int const nt[3]) {
    if (!shell_slabs && !shell_after)
    {
      op->launch_region(mode, v, MfTileRegion::outside_of(lo, hi, handle.exchange_stream()));
      handle.join_exchange_stream();
      return;
    }
    handle.exchange_end(1);
    if (shell_after)
    {
      op->launch_region(mode, v, MfTileRegion::outside_of(lo, hi));
      return;
    }
    // the slabs of mf_shell_slabs, low side then high side (z, y, x each), then the tail columns over all z-tiles
    const int zero[3] = {0, 0, 0};
    int slab[6][6];
    mf_shell_slabs(lo, hi, nt, slab);
    for (int side = 0; side < 2; ++side)
      for (int q = side; q < 6; q += 2)
        if (!mf_slab_empty(slab[q]))
        {
          const int b0[3] = {slab[q][0], slab[q][2], slab[q][4]}, b1[3] = {slab[q][1], slab[q][3], slab[q][5]};
          op->launch_region(mode, v, MfTileRegion::box(b0, b1));
        }
    if (op->has_tail())
      op->launch_region(mode, v, MfTileRegion::box(zero, nt, false, true));
  };
  if (!handle.comm.enabled())
  {
    // (measurement only: the launches of the corner rank of a 2 x 2 x 2 grid -- one neighbour on the high side of every
    // axis -- without the exchange)
    // ("1" / "xyz": 2 x 2 x 2; "yz": 1 x 2 x 2; "z": 1 x 1 x 2 -- the grids of the weak-scaling run at 8, 4 and 2 ranks)
    const int emu = handle.mf_emulate_split; // 1 = z, 2 = yz, 3 = xyz
    if (emu > 0 && op->dim() == 3)
    {
      int nt[3], rows[3];
      op->tiling(nt, rows);
      if (nt[0] >= 2 && nt[1] >= 2 && nt[2] >= 2)
      {
        const int lo[3] = {0, 0, 0};
        const int hi[3] = {nt[0] - (emu == 3 ? 1 : 0), nt[1] - (emu == 1 ? 0 : 1), nt[2] - 1};
        handle.fork_exchange_stream(); // (what an exchange_begin does to the two streams, without the exchange)
        op->launch_region(mode, v, MfTileRegion::box(lo, hi));
        shell(lo, hi, nt);
        return;
      }
    }
    whole();
    return;
  }
  HaloSpace const &s = handle.comm.spaces[1];
  // Tile t of an axis owns the planes [t R, (t + 1) R) and reads one more on either side; the planes the exchange writes are
  // own0 - 1 (towards a lower neighbour) and own0 + own_n (towards an upper one): plane g is read by the tiles
  // ceil(g / R) - 1 ... floor((g + 1) / R).  The tiles that read none of them form a box [lo, hi) of tiles and run while the
  // faces, edges and corners travel (slabs: the two planes along z); the shell around them and the columns of the tail follow.
  int nt[3], rows[3], lo[3], hi[3];
  op->tiling(nt, rows);
  bool interior = handle.overlap_exchange;
  for (int d = 0; d < 3; ++d)
  {
    lo[d] = 0;
    hi[d] = nt[d];
    if (s.low(d))
      lo[d] = (int)std::min<int64_t>(nt[d], s.own0(d) / rows[d] + 1);
    if (s.high(d))
      hi[d] = (int)std::max<int64_t>(0, std::min<int64_t>(nt[d], (s.own0(d) + s.own_n(d) + rows[d] - 1) / rows[d] - 1));
    if (lo[d] >= hi[d])
      interior = false;
  }
  if (!interior)
  {
    handle.exchange(1, const_cast<T *>(v.x));
    whole();
    return;
  }
  handle.exchange_begin(1, const_cast<T *>(v.x));
  op->launch_region(mode, v, MfTileRegion::box(lo, hi));
  shell(lo, hi, nt);
}
} // namespace

void HipMatrixFreeOperator::apply_mode(MfMode mode, MfOperands<double> const &v) const
{
  distributed_apply_mode<double>(get_hip_handle(), _mesh_evaluator->get_device_operator().get(), mode, v);
}

void HipMatrixFreeOperator::apply_local(DVector const &x, DVector &y) const
{
  _mesh_evaluator->get_device_operator()->vmult(x.get_values(), y.get_values());
}

void HipMatrixFreeOperator::vmult(DVector &dst, DVector const &src) const
{
  ASSERT_THROW(dst.size() == src.size(), "vector sizes do not match the operator");
  apply_mode(MfMode::apply, {src.get_values(), nullptr, nullptr, 0., 0., dst.get_values()});
}

void HipMatrixFreeOperator::apply(DVector const &x, DVector &y, OperatorMode mode) const
{
  if (mode != OperatorMode::NO_TRANS)
    ASSERT_THROW_NOT_IMPLEMENTED(); // source/cuda/cuda_matrix_free_operator.cu:64-71
  vmult(y, x);
}

std::shared_ptr<Operator<DVector>> HipMatrixFreeOperator::transpose() const
{
  ASSERT_THROW_NOT_IMPLEMENTED();
  return nullptr;
}

std::shared_ptr<Operator<DVector>> HipMatrixFreeOperator::multiply(std::shared_ptr<Operator<DVector> const>) const
{
  ASSERT_THROW_NOT_IMPLEMENTED();
  return nullptr;
}

std::shared_ptr<Operator<DVector>>
HipMatrixFreeOperator::multiply_transpose(std::shared_ptr<Operator<DVector> const> b) const
{
  auto downcast_b = std::dynamic_pointer_cast<HipMatrixOperator const>(b);
  ASSERT_THROW(downcast_b != nullptr, "HipMatrixFreeOperator::multiply_transpose needs a HipMatrixOperator");
  auto self = std::make_shared<HipMatrixFreeOperator>(_mesh_evaluator);
  return std::make_shared<HipGalerkinHalfProduct>(self, downcast_b);
}

std::shared_ptr<DVector> HipMatrixFreeOperator::build_domain_vector() const
{
  return _mesh_evaluator->build_range_vector();
}

std::shared_ptr<DVector> HipMatrixFreeOperator::build_range_vector() const
{
  return _mesh_evaluator->build_range_vector();
}

size_t HipMatrixFreeOperator::grid_complexity() const { return _mesh_evaluator->get_mesh().n_dofs; }

size_t HipMatrixFreeOperator::operator_complexity() const
{
  ASSERT_THROW_NOT_IMPLEMENTED();
  return 0;
}

void HipMatrixFreeOperator::residual(DVector const &x, DVector const &b, DVector &res) const
{
  apply_mode(MfMode::residual, {x.get_values(), b.get_values(), nullptr, 0., 0., res.get_values()});
}

void HipMatrixFreeOperator::smoother_step(DVector const &b, DVector const &x, DVector const *x_prev, double alpha,
                                          double beta, DVector &out) const
{
  double const *xp = x_prev ? x_prev->get_values() : nullptr;
  apply_mode(mf_smoother_mode(xp, alpha), {x.get_values(), b.get_values(), xp, alpha, beta, out.get_values()});
}

// ---- blocks of vectors ----
int64_t block_leading_dimension(std::vector<DVector const *> const &columns)
{
  if (columns.empty())
    return 0;
  const int64_t n = columns[0]->size();
  if (columns.size() == 1)
    return n;
  const int64_t ld = columns[1]->get_values() - columns[0]->get_values();
  if (ld < n)
    return 0;
  for (size_t c = 0; c < columns.size(); ++c)
    if (columns[c]->size() != n || columns[c]->get_values() != columns[0]->get_values() + (int64_t)c * ld)
      return 0;
  return ld;
}

namespace
{
std::vector<DVector const *> as_const(std::vector<DVector *> const &v) { return std::vector<DVector const *>(v.begin(), v.end()); }
// what launch_block asks of a block beyond equal distances: an even leading dimension, a base aligned to 16 bytes
bool block_kernel_layout(std::vector<DVector const *> const &columns, int64_t ld)
{
  return block_leading_dimension(columns) == ld && ld % 2 == 0 && reinterpret_cast<uintptr_t>(columns[0]->get_values()) % 16 == 0;
}
} // namespace

// ---- blocks of vectors through a restrictor ----
int HipMatrixOperator::transfer_block_width(OperatorMode mode) const
{
  if (!_structured || _matrix->handle().comm.enabled() || _reverse_range_space > 0)
    return 1;
  return mode == OperatorMode::NO_TRANS ? _structured->restrict_block_width() : _structured->prolong_block_width();
}

void HipMatrixOperator::transfer_block(std::vector<DVector const *> const &x, std::vector<DVector *> const &y, Transfer what) const
{
  ASSERT_THROW(x.size() == y.size() && !x.empty(), "the blocks of a transfer need the same number of columns");
  const bool restriction = what == Transfer::restrict_to_coarse;
  const int64_t ldx = block_leading_dimension(x), ldy = block_leading_dimension(as_const(y));
  if (transfer_block_width(restriction ? OperatorMode::NO_TRANS : OperatorMode::TRANS) == 1 || x.size() == 1 ||
      x.size() > (size_t)kMfBlockMaxVectors || ldx == 0 || ldy == 0 || !block_kernel_layout(x, ldx) || !block_kernel_layout(as_const(y), ldy))
  {
    for (size_t c = 0; c < x.size(); ++c)
    {
      if (what == Transfer::prolongate_subtract)
        apply_subtract(*x[c], *y[c], OperatorMode::TRANS);
      else
        apply(*x[c], *y[c], restriction ? OperatorMode::NO_TRANS : OperatorMode::TRANS);
    }
    _transfer_columns_looped += (int64_t)x.size();
    return;
  }
  const int64_t n_in = restriction ? _matrix->n() : _matrix->m(), n_out = restriction ? _matrix->m() : _matrix->n();
  ASSERT_THROW(x[0]->size() == n_in && y[0]->size() == n_out, "vector sizes do not match the operator");
  if (restriction)
    _transfer_columns_looped += _structured->restrict_to_coarse_block((int)x.size(), ldx, x[0]->get_values(), ldy, y[0]->get_values());
  else
    _transfer_columns_looped += _structured->prolongate_block((int)x.size(), ldx, x[0]->get_values(), ldy, y[0]->get_values(),
                                                              what == Transfer::prolongate_subtract);
}

void HipMatrixOperator::apply_block(std::vector<DVector const *> const &x, std::vector<DVector *> const &y) const
{
  if (_structured)
    return transfer_block(x, y, Transfer::restrict_to_coarse);
  ASSERT_THROW(x.size() == y.size() && !x.empty(), "a block needs as many results as vectors");
  if (!matrix_block(CsrMode::apply, x, nullptr, nullptr, nullptr, 0., 0., y))
    Operator<DVector>::apply_block(x, y);
}

void HipMatrixOperator::apply_subtract_block(std::vector<DVector const *> const &x, std::vector<DVector *> const &y, OperatorMode mode) const
{
  if (mode == OperatorMode::NO_TRANS)
  {
    if (!matrix_block(CsrMode::subtract, x, nullptr, nullptr, nullptr, 0., 0., y))
      Operator<DVector>::apply_subtract_block(x, y, mode);
    return;
  }
  transfer_block(x, y, Transfer::prolongate_subtract);
}

// ---- blocks of vectors through a plain matrix operator ----
int HipMatrixOperator::block_width() const
{
  if (_structured || _matrix->handle().comm.enabled() || _reverse_range_space > 0)
    return 1;
  return _matrix->block_width();
}

bool HipMatrixOperator::matrix_block(CsrMode mode, std::vector<DVector const *> const &x, std::vector<DVector const *> const *b,
                                     double const *dinv, std::vector<DVector const *> const *x_prev, double alpha, double beta,
                                     std::vector<DVector *> const &out) const
{
  const size_t k = x.size();
  if (block_width() == 1 || k <= 1 || k > (size_t)kMfBlockMaxVectors || out.size() != k || (b && b->size() != k) ||
      (x_prev && x_prev->size() != k))
    return false;
  const int64_t ld_x = block_leading_dimension(x), ld_out = block_leading_dimension(as_const(out));
  if (ld_x == 0 || ld_out == 0 || !block_kernel_layout(x, ld_x) || !block_kernel_layout(as_const(out), ld_out) ||
      (b && !block_kernel_layout(*b, ld_out)) || (x_prev && !block_kernel_layout(*x_prev, ld_out)) ||
      (dinv && reinterpret_cast<uintptr_t>(dinv) % 16 != 0))
    return false;
  if (x[0]->size() != _matrix->n() || out[0]->size() != _matrix->m() || (b && (*b)[0]->size() != _matrix->m()) ||
      (x_prev && (*x_prev)[0]->size() != _matrix->m()))
    return false;
  // (the kernels read x while they write out: blocks that overlap go column by column, where only equal vectors are refused)
  double const *xb = x[0]->get_values(), *ob = out[0]->get_values();
  if (!(xb + (int64_t)(k - 1) * ld_x + _matrix->n() <= ob || ob + (int64_t)(k - 1) * ld_out + _matrix->m() <= xb))
    return false;
  _matrix->apply_mode_block(mode, (int)k, xb, ld_x, b ? (*b)[0]->get_values() : nullptr, dinv, x_prev ? (*x_prev)[0]->get_values() : nullptr,
                            alpha, beta, out[0]->get_values(), ld_out);
  return true;
}

void HipMatrixOperator::residual_block(std::vector<DVector const *> const &x, std::vector<DVector const *> const &b,
                                       std::vector<DVector *> const &res) const
{
  if (!matrix_block(CsrMode::residual, x, &b, nullptr, nullptr, 0., 0., res))
    Operator<DVector>::residual_block(x, b, res);
}

void HipMatrixOperator::smoother_step_block(int w, int64_t ld, double const *b, double const *x, double const *x_prev, double alpha,
                                            double beta, double *out) const
{
  ASSERT_THROW(block_width() > 1, "internal: a smoother term on a block of a matrix without the block kernels");
  // (SparseMatrixDevice::smoother_step: a term without momentum is a `first` term, which reads no x_prev)
  const bool first = x_prev == nullptr || alpha == 0.;
  _matrix->apply_mode_block(first ? CsrMode::first : CsrMode::next, w, x, ld, b, get_diagonal_inverse(), first ? nullptr : x_prev,
                            first ? 0. : alpha, beta, out, ld);
}

void HipMatrixOperator::apply_plus_scaled_block(std::vector<DVector const *> const &x, double const *dinv, std::vector<DVector const *> const &b,
                                                double beta, std::vector<DVector *> const &y) const
{
  if (matrix_block(CsrMode::plus_scaled, x, &b, dinv, nullptr, 0., beta, y))
    return;
  for (size_t c = 0; c < x.size(); ++c)
    apply_plus_scaled(*x[c], dinv, *b[c], beta, *y[c]);
}

std::vector<std::shared_ptr<DVector>> HipMatrixOperator::build_domain_block(int width, int64_t ld) const
{
  const int64_t n = _matrix->n();
  ASSERT_THROW(width >= 1 && ld >= n, "a block needs a leading dimension of at least the vector size");
  HipHandle &handle = _matrix->handle();
  auto storage = std::make_shared<DeviceBuffer<double>>((size_t)width * ld); // (hipMalloc: aligned to 256 bytes)
  vec::set<double>(handle, (int64_t)width * ld, 0., storage->data());
  std::vector<std::shared_ptr<DVector>> columns;
  for (int c = 0; c < width; ++c)
    columns.emplace_back(new DVector(handle, n, storage->data() + (int64_t)c * ld), [storage](DVector *v) { delete v; });
  return columns;
}

void HipMatrixOperator::transfer_block_counters(int64_t counters[3]) const
{
  counters[0] = _structured ? _structured->restrict_block_launches() : 0;
  counters[1] = _structured ? _structured->prolong_block_launches() : 0;
  counters[2] = _transfer_columns_looped;
}

int HipMatrixFreeOperator::block_width() const
{
  auto op = _mesh_evaluator->get_device_operator();
  // several ranks: what the ranks agreed on when the fine smoother was built (1 before that), never this rank's operator alone
  if (get_hip_handle().comm.enabled())
    return std::max(op->block_width_agreed(), 1);
  return op->block_kernel_available() ? 4 : 1;
}

// Several ranks: per group of 4 or 2 columns ONE exchange_block of the group's x, one plane deep, then the block launch on the
// local mesh -- where apply_mode sends the message of one vector per application, a group sends one message per neighbour.  A
// single column takes the one-vector path with its own exchange.  The exchange is not overlapped with the tiles that read no
// ghost plane (the block kernel has no region launch): DESIGN.md section 8.
void HipMatrixFreeOperator::apply_mode_block(MfMode mode, MfBlockOperands<double> const &v) const
{
  auto op = _mesh_evaluator->get_device_operator();
  HipHandle &handle = get_hip_handle();
  if (!handle.comm.enabled())
    return op->launch_block(mode, v);
  ASSERT_THROW(block_width() > 1, "internal: the ranks did not agree on blocks of vectors");
  int widths[kMfBlockMaxGroups];
  const int n_groups = mf_block_groups(v.n_vectors, widths);
  int c = 0;
  for (int g = 0; g < n_groups; c += widths[g], ++g)
  {
    auto at = [&](double const *p) { return p ? p + (int64_t)c * v.ld : nullptr; };
    if (widths[g] == 1)
    {
      apply_mode(mode, {at(v.x), at(v.b), at(v.x_prev), v.alpha, v.beta, v.out + (int64_t)c * v.ld});
      continue;
    }
    MfBlockOperands<double> s = v;
    s.x = at(v.x);
    s.b = at(v.b);
    s.x_prev = at(v.x_prev);
    s.out = v.out + (int64_t)c * v.ld;
    s.n_vectors = widths[g];
    handle.exchange_block(s.n_vectors, s.ld, const_cast<double *>(s.x), 1);
    op->launch_block_local(mode, s);
  }
}

void HipMatrixFreeOperator::residual_block(std::vector<DVector const *> const &x, std::vector<DVector const *> const &b,
                                           std::vector<DVector *> const &res) const
{
  ASSERT_THROW(x.size() == b.size() && x.size() == res.size() && !x.empty(), "the blocks of a residual need the same number of columns");
  const int64_t ld = block_leading_dimension(x);
  if (block_width() == 1 || x.size() == 1 || x.size() > (size_t)kMfBlockMaxVectors || ld == 0 || !block_kernel_layout(x, ld) ||
      !block_kernel_layout(b, ld) || !block_kernel_layout(as_const(res), ld))
    return Operator<DVector>::residual_block(x, b, res);
  apply_mode_block(MfMode::residual, {x[0]->get_values(), b[0]->get_values(), nullptr, res[0]->get_values(), ld, (int)x.size(), 0., 0.});
}

void HipMatrixFreeOperator::apply_block(std::vector<DVector const *> const &x, std::vector<DVector *> const &y) const
{
  ASSERT_THROW(x.size() == y.size() && !x.empty(), "the blocks of an operator application need the same number of columns");
  const int64_t ld = block_leading_dimension(x);
  if (block_width() == 1 || x.size() == 1 || x.size() > (size_t)kMfBlockMaxVectors || ld == 0 || !block_kernel_layout(x, ld) ||
      !block_kernel_layout(as_const(y), ld))
    return Operator<DVector>::apply_block(x, y);
  // (launch_block cuts the columns into the groups of mf_block_groups)
  apply_mode_block(MfMode::apply, {x[0]->get_values(), nullptr, nullptr, y[0]->get_values(), ld, (int)x.size(), 0., 0.});
}

std::vector<std::shared_ptr<DVector>> HipMatrixFreeOperator::build_domain_block(int width, int64_t ld) const
{
  const int64_t n = (int64_t)grid_complexity();
  ASSERT_THROW(width >= 1 && ld >= n, "a block needs a leading dimension of at least the vector size");
  HipHandle &handle = get_hip_handle();
  auto storage = std::make_shared<DeviceBuffer<double>>((size_t)width * ld); // (hipMalloc: aligned to 256 bytes)
  vec::set<double>(handle, (int64_t)width * ld, 0., storage->data());
  std::vector<std::shared_ptr<DVector>> columns;
  for (int c = 0; c < width; ++c)
    columns.emplace_back(new DVector(handle, n, storage->data() + (int64_t)c * ld), [storage](DVector *v) { delete v; });
  return columns;
}

bool HipMatrixFreeOperator::sweep_available(int n_terms) const
{
  return _mesh_evaluator->get_device_operator()->fused_sweep_available(n_terms);
}

bool HipMatrixFreeOperator::sweep_from_zero_available(int n_terms) const
{
  return _mesh_evaluator->get_device_operator()->fused_zero_guess_available(n_terms);
}

bool HipMatrixFreeOperator::smoother_sweep(int n_terms, double const *alpha, double const *beta, DVector const &b, DVector const &x,
                                           DVector &out, DVector *out_prev) const
{
  auto op = _mesh_evaluator->get_device_operator();
  if (!op->fused_sweep_available(n_terms))
    return false;
  HipHandle &handle = get_hip_handle();
  if (handle.comm.enabled())
  {
    // Distributed: term s of the sweep is right where the whole stencil of term s - 1 was, so the rank computes the ghost DoFs
    // next to its box redundantly: x travels n_terms ghost planes deep (ONE exchange for the n_terms terms instead of one each),
    // b n_terms - 1 planes deep -- as much as the local mesh holds (one agglomerate = two cell layers of a lower neighbour: two
    // terms; two agglomerates, BoxPartition(low_ghost_cells=4): three).
    ASSERT_THROW(n_terms <= handle.comm.sweep_terms(), "internal: more terms per sweep than the ranks hold ghost planes for");
    handle.rhs_ghosts_wanted = true;
    handle.rhs_ghost_width = std::max(handle.rhs_ghost_width, n_terms - 1);
    handle.exchange_on(handle.fine_space(n_terms), const_cast<double *>(x.get_values()), handle.stream, handle.stream, false);
    handle.need_rhs_ghosts(b.get_values(), n_terms - 1);
  }
  op->smoother_sweep(n_terms, alpha, beta, b.get_values(), x.get_values(), out.get_values(), out_prev ? out_prev->get_values() : nullptr);
  return true;
}

bool HipMatrixFreeOperator::smoother_sweep_from_zero(int n_terms, double const *alpha, double const *beta, DVector const &b, DVector &out) const
{
  auto op = _mesh_evaluator->get_device_operator();
  if (!op->fused_zero_guess_available(n_terms))
    return false;
  HipHandle &handle = get_hip_handle();
  if (handle.comm.enabled())
  {
    // (x_0 = 0 on every rank: its ghost entries need no exchange; b as in smoother_sweep)
    ASSERT_THROW(n_terms <= handle.comm.sweep_terms(), "internal: more terms per sweep than the ranks hold ghost planes for");
    handle.rhs_ghosts_wanted = true;
    handle.rhs_ghost_width = std::max(handle.rhs_ghost_width, n_terms - 1);
    handle.need_rhs_ghosts(b.get_values(), n_terms - 1);
  }
  op->smoother_sweep(n_terms, alpha, beta, b.get_values(), nullptr, out.get_values(), nullptr);
  return true;
}

double const *HipMatrixFreeOperator::get_diagonal_inverse() const
{
  return _mesh_evaluator->matrix_free_get_diagonal_inverse();
}

void HipGalerkinHalfProduct::apply(DVector const &x, DVector &y, OperatorMode mode) const
{
  if (mode != OperatorMode::NO_TRANS)
    ASSERT_THROW_NOT_IMPLEMENTED();
  auto tmp = _a_op->build_domain_vector();
  _r->apply(x, *tmp, OperatorMode::TRANS);
  _a_op->apply(*tmp, y);
}

// ---- HipSmoother ---------------------------------------------------------------
namespace
{
// the most terms one sweep of an operator may run within smoother.fused_terms (0: none); a sweep of K terms that is available
// is available for fewer
template <typename Available>
int largest_sweep(int fused_terms, Available available)
{
  int k = 0;
  for (int K = 2; K <= fused_terms; ++K)
    if (available(K))
      k = K;
  return k;
}

// The terms of the polynomial that run as one sweep: at most smoother.fused_terms, at most the `offered` sweep (and the sweep
// from x_0 = 0 only where offered), and only from a first term without momentum (alpha_0 = 0: Jacobi and Chebyshev).
SweepSchedule plan_sweeps(std::vector<std::pair<double, double>> const &coefficients, int fused_terms, int offered,
                          bool offered_from_zero)
{
  SweepSchedule s;
  const int d = (int)coefficients.size();
  if (coefficients[0].first != 0.)
    return s;
  auto fits = [&](int K) { return K >= 2 && K <= offered ? K : 0; };
  s.in_place = fits(std::min(d - 1, fused_terms));
  s.out_of_place = fits(std::min(d, fused_terms));
  s.from_zero = d == 3 && s.out_of_place == 3 && offered_from_zero;
  return s;
}

// (alpha_k, beta_k) of the first n terms in the precision of the operator
template <typename S>
void first_terms(std::vector<std::pair<double, double>> const &coefficients, int n, S *alpha, S *beta)
{
  for (int k = 0; k < n; ++k)
  {
    alpha[k] = S(coefficients[k].first);
    beta[k] = S(coefficients[k].second);
  }
}

// The polynomial from x_in into x_out, for the FP64 smoother (V = DVector) and the FP32 fine level (V = float): the first
// `swept` terms in one sweep -- into x_out when they are all of them, else x_K into scratch(0) and x_{K-1} into scratch(1) --,
// then one launch per term.  The terms before the last land in the scratch vectors: a term may overwrite its own x_{k-1},
// never its x_k (in place, x_in == x_out, the last term is a launch of its own).
template <typename S, typename V, typename Scratch, typename Step, typename Sweep>
void run_polynomial(std::vector<std::pair<double, double>> const &coefficients, int swept, V const *x_in, V *x_out, Scratch scratch,
                    Step step, Sweep sweep)
{
  const int d = (int)coefficients.size();
  V const *cur = x_in, *prev = nullptr;
  if (swept > 0)
  {
    S alpha[3], beta[3];
    first_terms(coefficients, swept, alpha, beta);
    V *out = swept == d ? x_out : scratch(0);
    V *out_prev = swept == d ? nullptr : scratch(1);
    sweep(swept, alpha, beta, x_in, out, out_prev);
    cur = out;
    prev = out_prev;
  }
  for (int k = swept; k < d; ++k)
  {
    V *target = x_out;
    if (k + 1 < d)
    {
      target = scratch(0);
      if (target == cur)
        target = scratch(1);
    }
    ASSERT_THROW(target != cur, "internal: a smoother term cannot overwrite the iterate it reads");
    step(cur, prev, S(coefficients[k].first), S(coefficients[k].second), target);
    prev = cur;
    cur = target;
  }
}
} // namespace

HipSmoother::HipSmoother(std::shared_ptr<Operator<DVector> const> op, std::shared_ptr<ptree const> params)
    : Smoother<DVector>(op, params)
{
  _hip_operator = std::dynamic_pointer_cast<HipOperator const>(this->_operator);
  ASSERT_THROW(_hip_operator != nullptr, "HipSmoother must be constructed from a HipMatrixOperator or a "
                                         "HipMatrixFreeOperator");
  const bool matrix_free = std::dynamic_pointer_cast<HipMatrixFreeOperator const>(_hip_operator) != nullptr;
  // defaults: Jacobi on the device matrix path (source/cuda/cuda_smoother.cu:105), Chebyshev on
  // the matrix-free path (source/dealii/dealii_matrix_free_smoother.cc:24)
  std::string prec_type = this->_params->get("smoother.type", matrix_free ? "Chebyshev" : "Jacobi");
  _type = to_lower(prec_type);
  // polynomial terms per sweep over the mesh (matrix-free operator, mf_cheb_fused.hip); 1 = one launch per term
  _fused_terms = this->_params->get("smoother.fused_terms", 3);
  ASSERT_THROW(_fused_terms >= 1 && _fused_terms <= 3, "smoother.fused_terms must be 1, 2 or 3");
  // ... and the cell arithmetic of that sweep: "modes" (default) or "reference" (the one-term kernel's, bit for bit)
  {
    const std::string arith = to_lower(this->_params->get("smoother.sweep_arithmetic", "modes"));
    ASSERT_THROW(arith == "modes" || arith == "reference", "smoother.sweep_arithmetic must be modes or reference");
    _sweep_reference = arith == "reference";
    if (auto mf = std::dynamic_pointer_cast<HipMatrixFreeOperator const>(_hip_operator))
      mf->get_mesh_evaluator()->get_device_operator()->set_fused_reference(_sweep_reference);
  }
  if (_type == "jacobi")
  {
    _lambda_min = _lambda_max = 1.;
    _coefficients = {{0., 1.}}; // x <- x - D^{-1}(A x - b)
  }
  else if (_type == "chebyshev")
  {
    // AdditionalData of dealii::PreconditionChebyshev as filled at
    // source/dealii/dealii_matrix_free_smoother.cc:34-56 (deal.II 9.1 defaults)
    int degree = this->_params->get("smoother.degree", 1);
    double smoothing_range = this->_params->get("smoother.smoothing_range", 0.);
    double max_eigenvalue = this->_params->get("smoother.max_eigenvalue", 1.);
    int eig_cg_n_iterations = this->_params->get("smoother.eig_cg_n_iterations", 8);
    double eig_cg_residual = this->_params->get("smoother.eig_cg_residual", 1e-2);
    ASSERT_THROW(degree >= 1, "smoother.degree must be at least one");
    auto lmax = this->_params->get_optional<double>("smoother.lambda_max");
    auto lmin = this->_params->get_optional<double>("smoother.lambda_min");
    double min_est = 1., max_est = max_eigenvalue;
    if (lmax)
    {
      max_est = *lmax;
      min_est = lmin ? *lmin : *lmax;
    }
    else if (eig_cg_n_iterations > 0)
    {
      // start vector of the CG: deal.II's (i % 11) pattern looks like a single plane wave under a
      // lexicographic numbering whose row length is a multiple of 11 +/- small (e.g. 128, 256) and then
      // under-estimates lambda_max badly (1.08 instead of 1.5: the smoother diverges); the default is a
      // numbering-independent hashed vector, "dealii" restores the reference pattern.
      _eig_start = to_lower(this->_params->get("smoother.eig_start_vector", "hashed"));
      ASSERT_THROW(_eig_start == "hashed" || _eig_start == "dealii", "unknown smoother.eig_start_vector");
      estimate_eigenvalues(eig_cg_n_iterations, eig_cg_residual, min_est, max_est);
      max_est *= 1.2; // safety factor: the CG is not converged
    }
    _lambda_max = max_est;
    if (lmin)
      _lambda_min = *lmin;
    else
      _lambda_min = smoothing_range > 1. ? max_est / smoothing_range : std::min(0.9 * max_est, min_est);
    const double theta = 0.5 * (_lambda_max + _lambda_min);
    const double delta = 0.5 * (_lambda_max - _lambda_min);
    _coefficients.push_back({0., 1. / theta});
    if (degree >= 2 && std::abs(delta) >= 1e-40)
    {
      double rhok = delta / theta;
      const double sigma = theta / delta;
      for (int k = 0; k < degree - 1; ++k)
      {
        const double rhokp = 1. / (2. * sigma - rhok);
        _coefficients.push_back({rhokp * rhok, 2. * rhokp / delta});
        rhok = rhokp;
      }
    }
  }
  else
  {
    // Gauss-Seidel / SSOR / ILU are sequential Ifpack algorithms outside the HIP path
    ASSERT_THROW(false, "Unknown smoother name: \"" + _type + "\" (the HIP back-end implements Jacobi and Chebyshev)");
  }
  if (matrix_free)
  {
    // The multi-term sweep changes the exchanges of a distributed smoother (x once per sweep, K planes deep, b widened; none of x
    // from a zero guess), so all ranks run it or none does.  What a rank's operator offers follows from its local mesh alone --
    // one coefficient per cell, the ghost planes it holds -- and differs between ranks whose materials differ: the ranks agree on
    // the smallest offer, in ONE collective that every rank reaches here.  Encoded as 2 K + z (z: the sweep from x_0 = 0, which
    // needs K = 3): the minimum over the ranks is the smallest K, with z set only where every rank has K = 3 and z.
    const int k = largest_sweep(_fused_terms, [&](int K) { return _hip_operator->sweep_available(K); });
    const bool z = k == 3 && _hip_operator->sweep_from_zero_available(3);
    const double mine = 2. * k + (z ? 1. : 0.);
    HipHandle &h = _hip_operator->get_hip_handle();
    const int agreed = (int)(h.comm.enabled() ? -h.allreduce_max(-mine) : mine);
    ASSERT_THROW(agreed / 2 <= k, "internal: the ranks agreed on a sweep this rank cannot run");
    _schedule = plan_sweeps(_coefficients, _fused_terms, agreed / 2, (agreed & 1) != 0);
    // Blocks of vectors change the exchanges as well -- a group of columns sends ONE message per neighbour, a loop over the columns
    // one per column -- so the ranks run groups as blocks only where every rank's operator has the block kernel (a rank with one
    // coefficient per cell or a tail slab has not): the smallest offer again, in ONE collective that every rank reaches here.
    // The staging of the group's exchange is sized here, outside the launch path.
    if (h.comm.enabled())
    {
      auto mf = std::dynamic_pointer_cast<HipMatrixFreeOperator const>(_hip_operator);
      auto device_op = mf->get_mesh_evaluator()->get_device_operator();
      const double offer = device_op->block_kernel_available() ? 4. : 1.;
      const int width = (int)-h.allreduce_max(-offer);
      ASSERT_THROW(width == 1 || (width == 4 && offer == 4.), "internal: the ranks agreed on a block width this rank cannot run");
      device_op->set_block_width_agreed(width);
      if (width > 1)
        h.reserve_exchange_block(width, 1);
    }
  }
}

void HipSmoother::estimate_eigenvalues(int n_iterations, double residual, double &min_est, double &max_est) const
{
  // PreconditionChebyshev::estimate_eigenvalues (deal.II 9.1): CG on A with D^{-1}, rhs = the
  // mean-free (i % 11) vector, eigenvalues of the Lanczos tridiagonal.
  HipHandle &h = _hip_operator->get_hip_handle();
  auto rhs = _hip_operator->build_range_vector();
  const int64_t n = rhs->size();
  {
    // (distributed spaces: the pattern follows the GLOBAL lexicographic id and the mean is the global one, so that
    // every rank count -- slabs or boxes -- estimates the same eigenvalues)
    const int sp = _hip_operator->domain_space();
    HaloSpace const *hs = (h.comm.enabled() && sp > 0) ? &h.comm.spaces[sp] : nullptr;
    if (hs)
      hs->check();
    const double n_global = hs ? double(hs->n_global()) : double(n);
    // ("internal numbering" lexicographic: entry i belongs to node i, the pattern follows the CALLER's id of that node, so that
    // the estimate is the one of a hierarchy that runs in the caller's numbering)
    int32_t const *caller_ids =
        (!hs && std::dynamic_pointer_cast<HipMatrixFreeOperator const>(_hip_operator) != nullptr) ? h.setup_caller_ids : nullptr;
    std::vector<double> v(n);
    double mean = 0.;
    for (int64_t i = 0; i < n; ++i)
    {
      const int64_t gi = hs ? hs->global_id(i) : (caller_ids ? (int64_t)caller_ids[i] : i);
      if (_eig_start == "dealii")
        v[i] = double(gi % 11);
      else // splitmix64 finaliser of the DoF id, in [0, 1): white in index space whatever the row length (a
           // multiplicative hash of consecutive ids is a low-discrepancy sequence: smooth, and lambda_max came out
           // 6 % low on a 65 x 129 x 129 mesh)
      {
        uint64_t z = uint64_t(gi) + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        v[i] = double(z >> 11) / 9007199254740992.0;
      }
      if (!hs || hs->owned(i))
        mean += v[i];
    }
    if (h.comm.enabled() && sp > 0)
      mean = h.allreduce_sum(mean); // (a replicated level sums over its own entries only)
    mean /= n_global;
    for (auto &e : v)
      e -= mean;
    MFMG_HIP_CHECK(hipMemcpyAsync(rhs->get_values(), v.data(), n * sizeof(double), hipMemcpyHostToDevice, h.stream));
    MFMG_HIP_CHECK(hipStreamSynchronize(h.stream));
  }
  double const *dinv = _hip_operator->get_diagonal_inverse();
  const int space = _hip_operator->domain_space();
  auto ddot = [&](DVector const &a, DVector const &b2) { return distributed_dot(h, space, a, b2); };
  DVector x(h, n), r(*rhs), z(h, n), p(h, n), ap(h, n);
  vec::scale_pointwise<double>(h, n, dinv, r.get_values(), z.get_values());
  p = z;
  double rz = ddot(r, z);
  const double tol = std::max(residual * std::sqrt(ddot(*rhs, *rhs)), 1e-300);
  std::vector<double> alphas, betas;
  for (int it = 0; it < n_iterations; ++it)
  {
    _hip_operator->apply(p, ap);
    const double pap = ddot(p, ap);
    if (pap == 0.)
      break;
    const double alpha = rz / pap;
    x.add(alpha, p);
    r.add(-alpha, ap);
    alphas.push_back(alpha);
    if (std::sqrt(ddot(r, r)) < tol)
      break;
    vec::scale_pointwise<double>(h, n, dinv, r.get_values(), z.get_values());
    const double rz_new = ddot(r, z);
    const double beta = rz_new / rz;
    betas.push_back(beta);
    rz = rz_new;
    p.sadd(beta, 1., z);
  }
  const int m = (int)alphas.size();
  if (m == 0)
  {
    min_est = max_est = 1.;
    return;
  }
  std::vector<double> T((size_t)m * m, 0.), w, V;
  for (int i = 0; i < m; ++i)
  {
    T[(size_t)i * m + i] = 1. / alphas[i] + (i > 0 ? betas[i - 1] / alphas[i - 1] : 0.);
    if (i + 1 < m)
      T[(size_t)i * m + i + 1] = T[(size_t)(i + 1) * m + i] = std::sqrt(betas[i]) / alphas[i];
  }
  symmetric_eigen(m, T, w, V);
  min_est = w.front();
  max_est = w.back();
}

DVector *HipSmoother::scratch(int i) const
{
  auto &s = i == 0 ? _scratch_a : _scratch_b;
  if (!s)
    s = this->_operator->build_domain_vector();
  return s.get();
}

void HipSmoother::run(int swept, DVector const &b, DVector const &x_in, DVector &x_out) const
{
  run_polynomial<double>(
      _coefficients, swept, &x_in, &x_out, [&](int i) { return scratch(i); },
      [&](DVector const *x, DVector const *x_prev, double alpha, double beta, DVector *out) {
        _hip_operator->smoother_step(b, *x, x_prev, alpha, beta, *out);
      },
      [&](int K, double const *alpha, double const *beta, DVector const *x, DVector *out, DVector *out_prev) {
        // (the ranks agreed on this sweep at setup: a refusal here would leave them with different exchanges)
        ASSERT_THROW(_hip_operator->smoother_sweep(K, alpha, beta, b, *x, *out, out_prev), "internal: the agreed smoother sweep was refused");
      });
}

void HipSmoother::apply(DVector const &b, DVector &x) const
{
  // x <- x - B^{-1}(A x - b) with B^{-1} the Jacobi / Chebyshev polynomial.  In place, so the last term must be a launch of
  // its own that lands in x: the terms before it run as one sweep into the scratch vectors where the schedule has one, else
  // one fused kernel per polynomial term.
  if (_coefficients.size() == 1)
  {
    _hip_operator->smoother_step(b, x, nullptr, 0., _coefficients[0].second, *scratch(0));
    x = *scratch(0);
    return;
  }
  run(_schedule.in_place, b, x, x);
}

int HipSmoother::block_width() const
{
  // (a schedule with a multi-term sweep belongs to the cell-constant layout, which has no block kernel)
  auto mf = std::dynamic_pointer_cast<HipMatrixFreeOperator const>(_hip_operator);
  if (mf)
    return _schedule.in_place == 0 ? mf->block_width() : 1;
  // (a matrix operator has no sweep: its polynomial goes term by term in either direction)
  auto mo = std::dynamic_pointer_cast<HipMatrixOperator const>(_hip_operator);
  return (mo && _schedule.in_place == 0 && _schedule.out_of_place == 0) ? mo->block_width() : 1;
}

int64_t HipSmoother::group_layout(std::vector<DVector const *> const &b, std::vector<DVector const *> const &x_in,
                                  std::vector<DVector const *> const &x_out) const
{
  const int64_t ld = block_leading_dimension(x_out);
  if (block_width() == 1 || x_out.size() == 1 || x_out.size() > (size_t)kMfBlockMaxVectors || ld == 0 || !block_kernel_layout(x_out, ld) ||
      !block_kernel_layout(b, ld) || !block_kernel_layout(x_in, ld))
    return 0;
  return ld;
}

void HipSmoother::run_group(int w, int64_t ld, int64_t n, double const *b, double const *x_in, double *x_out) const
{
  auto mf = std::dynamic_pointer_cast<HipMatrixFreeOperator const>(_hip_operator);
  auto mo = std::dynamic_pointer_cast<HipMatrixOperator const>(_hip_operator);
  HipHandle &handle = _hip_operator->get_hip_handle();
  for (auto &s : _block_scratch)
    if (s.size() < (size_t)w * ld)
    {
      MemoryKind kind("smoother: block scratch vectors (one group of right-hand sides)");
      s.resize((size_t)w * ld);
      vec::set<double>(handle, (int64_t)w * ld, 0., s.data());
    }
  struct Block
  {
    double *p;
  };
  Block xi{const_cast<double *>(x_in)}, xo{x_out}, sa{_block_scratch[0].data()}, sb{_block_scratch[1].data()};
  auto step = [&](Block const *cur, Block const *prev, double alpha, double beta, Block *out) {
    double const *xp = prev ? prev->p : nullptr;
    if (mf)
      mf->apply_mode_block(mf_smoother_mode(xp, alpha), {cur->p, b, xp, out->p, ld, w, alpha, beta});
    else
      mo->smoother_step_block(w, ld, b, cur->p, xp, alpha, beta, out->p);
  };
  if (_coefficients.size() == 1 && x_in == x_out)
  {
    step(&xi, nullptr, 0., _coefficients[0].second, &sa);
    for (int c = 0; c < w; ++c)
      vec::copy<double>(handle, n, sa.p + (int64_t)c * ld, xo.p + (int64_t)c * ld);
    return;
  }
  run_polynomial<double>(
      _coefficients, 0, static_cast<Block const *>(&xi), &xo, [&](int i) { return i == 0 ? &sa : &sb; }, step,
      [&](int, double const *, double const *, Block const *, Block *, Block *) { ASSERT_THROW(false, "internal: no sweep on a block"); });
}

void HipSmoother::apply_block(std::vector<DVector const *> const &b, std::vector<DVector *> const &x) const
{
  ASSERT_THROW(b.size() == x.size() && !x.empty(), "a block needs as many right-hand sides as iterates");
  const int64_t ld = group_layout(b, as_const(x), as_const(x));
  if (ld == 0)
    return Smoother<DVector>::apply_block(b, x);
  // groups of the block: every group runs the polynomial of apply(), its terms as launches on the group
  int widths[kMfBlockMaxGroups];
  const int n_groups = mf_block_groups((int)x.size(), widths);
  size_t c0 = 0;
  for (int g = 0; g < n_groups; c0 += widths[g], ++g)
  {
    if (widths[g] == 1)
      apply(*b[c0], *x[c0]);
    else
      run_group(widths[g], ld, x[0]->size(), b[c0]->get_values(), x[c0]->get_values(), x[c0]->get_values());
  }
}

void HipSmoother::apply_to_block(std::vector<DVector const *> const &b, std::vector<DVector const *> const &x_in,
                                 std::vector<DVector *> const &x_out) const
{
  ASSERT_THROW(b.size() == x_out.size() && x_in.size() == x_out.size() && !x_out.empty(), "a block needs as many right-hand sides as iterates");
  const int64_t ld = group_layout(b, x_in, as_const(x_out));
  int widths[kMfBlockMaxGroups];
  const int n_groups = mf_block_groups((int)x_out.size(), widths);
  size_t c0 = 0;
  for (int g = 0; g < n_groups; c0 += widths[g], ++g)
  {
    if (ld == 0 || widths[g] == 1)
      for (size_t c = c0; c < c0 + (size_t)widths[g]; ++c)
        apply_to(*b[c], *x_in[c], *x_out[c]);
    else
    {
      ASSERT_THROW(x_in[c0]->get_values() != x_out[c0]->get_values(), "apply_to needs two vectors");
      run_group(widths[g], ld, x_out[0]->size(), b[c0]->get_values(), x_in[c0]->get_values(), x_out[c0]->get_values());
    }
  }
}

void HipSmoother::apply_zero_guess_block(std::vector<DVector const *> const &b, std::vector<DVector *> const &x) const
{
  ASSERT_THROW(b.size() == x.size() && !x.empty(), "a block needs as many right-hand sides as iterates");
  // (apply_zero_guess: one term needs no operator application, x_1 = beta_0 D^-1 b per column; more terms run apply() from x = 0)
  if (_coefficients.size() == 1)
  {
    for (size_t c = 0; c < x.size(); ++c)
      apply_zero_guess(*b[c], *x[c]);
    return;
  }
  for (auto *xc : x)
    *xc = 0.;
  apply_block(b, x);
}

void HipSmoother::apply_zero_guess(DVector const &b, DVector &x) const
{
  // the same update for x = 0 on entry: the first polynomial term is x_1 = beta_0 D^{-1} b (what the fused
  // kernel returns for A 0 = 0, bit for bit), which needs no operator application
  const int d = (int)_coefficients.size();
  if (d != 1)
  {
    x = 0.;
    apply(b, x);
    return;
  }
  vec::scaled_pointwise<double>(_hip_operator->get_hip_handle(), x.size(), _coefficients[0].second,
                                _hip_operator->get_diagonal_inverse(), b.get_values(), x.get_values());
}

void HipSmoother::apply_to(DVector const &b, DVector const &x_in, DVector &x_out) const
{
  ASSERT_THROW(x_in.get_values() != x_out.get_values(), "apply_to needs two vectors");
  run(_schedule.out_of_place, b, x_in, x_out);
}

bool HipSmoother::apply_from_zero(DVector const &b, DVector &x_out) const
{
  // the whole polynomial as one sweep that does not read x_0 = 0 (three terms: the kernels that carry the variant)
  if (!_schedule.from_zero)
    return false;
  double alpha[3], beta[3];
  first_terms(_coefficients, 3, alpha, beta);
  // (the ranks agreed on the sweep from zero at setup; a sweep tile set on this operator since then may still refuse it here)
  return _hip_operator->smoother_sweep_from_zero(3, alpha, beta, b, x_out);
}

// ---- HipFloatFineLevel -----------------------------------------------------------
HipFloatFineLevel::HipFloatFineLevel(HipHandle &handle, mfmg_hip_mesh_desc const &mesh, Hierarchy<DVector> const &hierarchy)
    : _hierarchy(hierarchy), _smoother(std::dynamic_pointer_cast<HipSmoother const>(hierarchy.levels()[0].get_smoother())),
      _op(handle, mesh, handle.allow_cell_constant)
{
  ASSERT_THROW(_smoother != nullptr, "unexpected smoother type");
  // the sweep as the FP64 smoother runs it, from what this operator offers; the pre-smoother of a preconditioner application
  // starts from a zeroed x
  _op.set_fused_reference(_smoother->sweep_reference());
  const int fused = _smoother->fused_terms();
  int offered = largest_sweep(fused, [&](int K) { return _op.fused_sweep_available(K); });
  // Several ranks: the sweep decides the exchanges (x once per sweep, as many planes deep as it has terms; b one plane less), so
  // the ranks run the sweep that every one of them offers -- this operator's offer, not the FP64 smoother's agreement: the
  // materials of the ranks may differ, and the float sweep has other tiles.  ONE collective that every rank reaches here.
  // (... and on the sweep from x_0 = 0 that spares the first pre-smoothing step of a preconditioner application the exchange of x,
  // encoded as in HipSmoother: 2 K + z.  One rank keeps zeroing x: its cycle is what it was.)
  // Blocks of float vectors change the exchanges as well (a group of columns sends one message per neighbour), so groups run as
  // blocks only where every rank's float operator has the block kernel: the smallest offer of 4 | 1, a second value of the SAME
  // all-reduce.
  bool from_zero = false;
  _block_offer = _op.block_kernel_available() ? 4 : 1;
  if (handle.comm.enabled())
  {
    if (!handle.comm.transport)
      throw std::runtime_error("no halo transport was registered with the context");
    const double mine = 2. * offered + (offered == 3 && _op.fused_zero_guess_available(3) ? 1. : 0.);
    double smallest[2] = {-mine, -double(_block_offer)}; // (the maximum of the negated values)
    handle.comm.transport->allreduce(smallest, 2, 1, handle.stream);
    const int agreed = (int)-smallest[0], width = (int)-smallest[1];
    ASSERT_THROW(agreed / 2 <= offered && agreed / 2 <= handle.comm.sweep_terms(), "internal: the ranks agreed on a sweep this rank cannot run");
    ASSERT_THROW(width == 1 || (width == 4 && _block_offer == 4), "internal: the ranks agreed on a block width this rank cannot run");
    offered = agreed / 2;
    from_zero = (agreed & 1) != 0;
    _block_offer = width;
  }
  _schedule = plan_sweeps(_smoother->coefficients(), fused, offered, from_zero);
  // (several ranks: a polynomial longer than the agreed sweep starts with that sweep -- two terms where the ranks hold one ghost
  // agglomerate below -- and goes on term by term, as the in-place FP64 smoother does there)
  if (handle.comm.enabled() && _schedule.out_of_place == 0 && offered >= 2 && _smoother->coefficients()[0].first == 0. &&
      (int)_smoother->coefficients().size() > offered)
    _schedule.out_of_place = std::min(offered, fused);
  _b_ghost_width = handle.comm.enabled() && _schedule.out_of_place > 0 ? _schedule.out_of_place - 1 : 0;
  // (the staging of a group's exchange is sized here, outside the launch path; the schedule follows from agreed values alone)
  if (handle.comm.enabled() && block_width() > 1)
    handle.reserve_exchange_block(block_width(), 1);
}

// One application of the FP32 operator.  Several ranks: as HipMatrixFreeOperator::apply_mode -- x is exchanged one plane deep, the
// tiles that read no ghost plane run beside the exchange, the shell behind it.
void HipFloatFineLevel::launch(MfMode mode, MfOperands<float> const &v) const
{
  if (_op.handle().comm.enabled())
    distributed_apply_mode<float>(_op.handle(), &_op, mode, v);
  else
    _op.launch_region(mode, v, MfTileRegion::whole());
}

void HipFloatFineLevel::vmult(float const *x, float *y) const { launch(MfMode::apply, {x, nullptr, nullptr, 0.f, 0.f, y}); }

void HipFloatFineLevel::residual(float const *x, float const *b, float *res) const
{
  launch(MfMode::residual, {x, b, nullptr, 0.f, 0.f, res});
}

void HipFloatFineLevel::smoother_step(float const *b, float const *x, float const *x_prev, float alpha, float beta, float *out) const
{
  launch(mf_smoother_mode(x_prev, alpha), {x, b, x_prev, alpha, beta, out});
}

// the ghost entries of b, `width` planes deep, current on the compute stream (the sweep reads b at the ghost DoFs it computes)
void HipFloatFineLevel::need_b_ghosts(float const *b, int width) const
{
  HipHandle &hd = _op.handle();
  if (_b_in_flight == b)
  {
    hd.exchange_async_wait();
    _b_fresh = b;
    _b_in_flight = nullptr;
  }
  if (_b_fresh != b || _b_fresh_width < width)
  {
    hd.exchange_on(hd.fine_space(std::max(width, _b_ghost_width)), const_cast<float *>(b), hd.stream, hd.stream, false);
    _b_fresh_width = std::max(width, _b_ghost_width);
    _b_fresh = _b_of_cycle == b ? b : nullptr; // (fresh only while the cycle that owns this vector is running)
  }
}

// Several smoother terms in one sweep.  Several ranks: as HipMatrixFreeOperator::smoother_sweep -- x travels n_terms planes deep,
// once; b n_terms - 1 planes deep, once per cycle; the ghost DoFs next to the box are computed redundantly.
void HipFloatFineLevel::smoother_sweep(int n_terms, float const *alpha, float const *beta, float const *b, float const *x, float *out,
                                       float *out_prev) const
{
  HipHandle &hd = _op.handle();
  if (hd.comm.enabled())
  {
    ASSERT_THROW(n_terms <= hd.comm.sweep_terms(), "internal: more terms per sweep than the ranks hold ghost planes for");
    hd.exchange_on(hd.fine_space(n_terms), const_cast<float *>(x), hd.stream, hd.stream, false);
    need_b_ghosts(b, n_terms - 1);
  }
  _op.smoother_sweep(n_terms, alpha, beta, b, x, out, out_prev);
}

// x_out <- x_in - B^-1 (A x_in - b) on two different vectors, with the polynomial of the FP64 smoother
void HipFloatFineLevel::smooth_to(float const *b, float const *x_in, float *x_out) const
{
  run_polynomial<float>(
      _smoother->coefficients(), _schedule.out_of_place, x_in, x_out, [&](int i) { return (i == 0 ? _scratch_a : _scratch_b).data(); },
      [&](float const *x, float const *x_prev, float alpha, float beta, float *out) { smoother_step(b, x, x_prev, alpha, beta, out); },
      [&](int K, float const *alpha, float const *beta, float const *x, float *out, float *out_prev) {
        smoother_sweep(K, alpha, beta, b, x, out, out_prev);
      });
}

void HipFloatFineLevel::apply(float const *b, float *x) const
{
  HipHandle &hd = _op.handle();
  auto const &levels = _hierarchy.levels();
  const int64_t n = _op.n_dofs();
  auto const &fine = *levels[0].get_operator();
  auto const &coarse = *levels[1].get_operator();
  const bool distributed = hd.comm.enabled();
  if (_work.size() == 0)
  {
    _scratch_a.resize(n);
    _scratch_b.resize(n);
    _res.resize(n);
    _work.resize(n);
    if (distributed)
      // (ghost entries beyond what an exchange refreshes are read by no kernel's result, but they are read: no NaN there)
      for (DeviceBuffer<float> *buf : {&_scratch_a, &_scratch_b, &_res, &_work})
        MFMG_HIP_CHECK(hipMemsetAsync(buf->data(), 0, sizeof(float) * n, hd.stream));
  }
  if (!_res64) // (a block call may have built them)
  {
    _res64 = fine.build_range_vector();
    _corr64 = fine.build_range_vector();
  }
  // (set_restrictor may have changed the coarse space since the last cycle)
  if (!_b_coarse || _b_coarse->size() != (int64_t)coarse.grid_complexity())
  {
    _b_coarse = coarse.build_range_vector();
    _x_coarse = coarse.build_range_vector();
  }
  // Several ranks: the ghost entries of b the sweeps read travel on the exchange stream from the start of the cycle, as the FP64
  // cycle sends them (HipMatrixOperator::prefetch_rhs); the first sweep waits for them.  Without sweeps nobody reads them.
  _b_of_cycle = b;
  _b_fresh = _b_in_flight = nullptr;
  if (distributed && _b_ghost_width > 0 && hd.overlap_exchange && _hierarchy.n_smoothing_steps() > 0)
  {
    hd.exchange_async(hd.fine_space(_b_ghost_width), const_cast<float *>(b));
    _b_fresh_width = _b_ghost_width;
    _b_in_flight = b;
  }
  // the iterate alternates between x and a work vector, so that no application ends in a copy
  float *it = x, *other = _work.data();
  unsigned int first_step = 0;
  auto smooth = [&] {
    for (unsigned int i = first_step; i < _hierarchy.n_smoothing_steps(); ++i)
    {
      smooth_to(b, it, other);
      std::swap(it, other);
    }
    first_step = 0;
  };
  if (_hierarchy.is_preconditioner())
  {
    if (_schedule.from_zero && _hierarchy.n_smoothing_steps() > 0)
    {
      // (several ranks, agreed at construction) the first pre-smoothing step as one sweep that does not read x_0 = 0: x is zero on
      // every rank, its ghost entries need no exchange; b as in smoother_sweep
      float alpha[3], beta[3];
      first_terms(_smoother->coefficients(), 3, alpha, beta);
      ASSERT_THROW(_op.fused_zero_guess_available(3), "internal: the agreed sweep from zero was refused");
      need_b_ghosts(b, 2);
      _op.smoother_sweep(3, alpha, beta, b, nullptr, other, nullptr);
      std::swap(it, other);
      first_step = 1;
    }
    else
      MFMG_HIP_CHECK(hipMemsetAsync(x, 0, sizeof(float) * n, hd.stream));
  }
  smooth();
  auto restrictor = levels[1].get_restrictor();
  auto hip_restrictor = std::dynamic_pointer_cast<HipMatrixOperator const>(restrictor);
  // b_c = R (A x - b): one pass over the FP32 vectors where the restrictor holds the rows of R A (one rank), otherwise the FP32
  // residual, widened, and the restriction -- which exchanges the ghost entries of the widened residual itself
  if (!(hip_restrictor && hip_restrictor->restrict_residual_f32(fine, it, b, *_b_coarse)))
  {
    residual(it, b, _res.data());
    vec::widen(hd, n, _res.data(), _res64->get_values());
    restrictor->apply(*_res64, *_b_coarse);
  }
  _hierarchy.apply(*_b_coarse, *_x_coarse, 1);
  restrictor->apply(*_x_coarse, *_corr64, OperatorMode::TRANS);
  vec::subtract_narrowed(hd, n, _corr64->get_values(), it);
  smooth();
  if (it != x)
    MFMG_HIP_CHECK(hipMemcpyAsync(x, it, sizeof(float) * n, hipMemcpyDeviceToDevice, hd.stream));
  if (_b_in_flight != nullptr)
    hd.exchange_async_wait(); // (no sweep waited: the exchange must still be over before the caller touches b)
  _b_of_cycle = _b_fresh = _b_in_flight = nullptr;
}

void HipFloatFineLevel::apply_block(int k, int64_t ld, float const *b, float *x) const
{
  HipHandle &hd = _op.handle();
  const int64_t n = _op.n_dofs();
  auto require = [](bool cond, char const *what) {
    if (!cond)
      throw InvalidArgumentExc(what);
  };
  require(k >= 1 && k <= kMfBlockMaxVectors, "a block holds 1 to 64 vectors");
  require(b != nullptr && x != nullptr, "null vector");
  require(ld >= n, "the leading dimension of a block must be at least n_dofs");
  require(ld % 2 == 0, "the leading dimension of a block must be even (columns aligned to 8 bytes)");
  require(reinterpret_cast<uintptr_t>(b) % 8 == 0 && reinterpret_cast<uintptr_t>(x) % 8 == 0, "the base of a block must be aligned to 8 bytes");
  const int64_t extent = (int64_t)(k - 1) * ld + n;
  require(b + extent <= x || x + extent <= b, "the blocks b and x overlap");
  _block_columns_looped = 0;
  auto const &levels = _hierarchy.levels();
  auto const &fine = *levels[0].get_operator();
  const bool block = block_width() > 1; // (several ranks: agreed at construction, so every rank takes the same branches below)
  const bool distributed = hd.comm.enabled();
  // one launch of the block kernel on a group; several ranks: behind ONE exchange of the group's x, one plane deep
  auto launch_group = [&](MfMode mode, MfBlockOperands<float> const &v) {
    if (!distributed)
      return _op.launch_block(mode, v);
    hd.exchange_block_f32(v.n_vectors, v.ld, const_cast<float *>(v.x), 1);
    _op.launch_block_local(mode, v);
  };
  int widths[kMfBlockMaxGroups];
  const int n_groups = mf_block_groups(k, widths);
  int64_t c0 = 0;
  for (int g = 0; g < n_groups; c0 += widths[g], ++g)
  {
    const int w = widths[g];
    float const *gb = b + c0 * ld;
    float *gx = x + c0 * ld;
    if (!block || w == 1)
    {
      for (int c = 0; c < w; ++c)
        apply(gb + c * ld, gx + c * ld);
      _block_columns_looped += w;
      continue;
    }
    static char const *const kinds[4] = {"FP32 fine level: block scratch vectors a (one group of right-hand sides)",
                                         "FP32 fine level: block scratch vectors b (one group of right-hand sides)",
                                         "FP32 fine level: block residual (one group of right-hand sides)",
                                         "FP32 fine level: block work vectors (one group of right-hand sides)"};
    for (int i = 0; i < 4; ++i)
      if (_block_buffers[i].size() < (size_t)w * ld)
      {
        MemoryKind kind(kinds[i]);
        _block_buffers[i].release(); // (before the wider one is built)
        _block_buffers[i].resize((size_t)w * ld);
        MFMG_HIP_CHECK(hipMemsetAsync(_block_buffers[i].data(), 0, sizeof(float) * (size_t)w * ld, hd.stream));
      }
    if (!_res64)
    {
      _res64 = fine.build_range_vector();
      _corr64 = fine.build_range_vector();
    }
    auto const &coarse = *levels[1].get_operator();
    if (!_b_coarse || _b_coarse->size() != (int64_t)coarse.grid_complexity())
    {
      _b_coarse = coarse.build_range_vector();
      _x_coarse = coarse.build_range_vector();
    }
    struct Block
    {
      float *p;
    };
    Block sa{_block_buffers[0].data()}, sb{_block_buffers[1].data()};
    float *const res = _block_buffers[2].data();
    // the iterate of the group alternates between its x columns and the work block, as the iterate of apply() does
    Block it{gx}, other{_block_buffers[3].data()};
    auto smooth = [&] {
      for (unsigned int i = 0; i < _hierarchy.n_smoothing_steps(); ++i)
      {
        run_polynomial<float>(
            _smoother->coefficients(), 0, static_cast<Block const *>(&it), &other, [&](int i) { return i == 0 ? &sa : &sb; },
            [&](Block const *cur, Block const *prev, float alpha, float beta, Block *out) {
              float const *xp = prev ? prev->p : nullptr;
              launch_group(mf_smoother_mode(xp, alpha), {cur->p, gb, xp, out->p, ld, w, alpha, beta});
            },
            [&](int, float const *, float const *, Block const *, Block *, Block *) { ASSERT_THROW(false, "internal: no sweep on a block"); });
        std::swap(it, other);
      }
    };
    if (_hierarchy.is_preconditioner())
      for (int c = 0; c < w; ++c)
        MFMG_HIP_CHECK(hipMemsetAsync(gx + c * ld, 0, sizeof(float) * n, hd.stream));
    smooth();
    auto restrictor = levels[1].get_restrictor();
    auto hip_restrictor = std::dynamic_pointer_cast<HipMatrixOperator const>(restrictor);
    // b_c = R (A x - b) in one pass per column where apply() forms it so; otherwise the residual of the group in one launch
    const bool one_pass = hip_restrictor && hip_restrictor->restrict_residual_f32(fine, it.p, gb, *_b_coarse);
    if (!one_pass)
      launch_group(MfMode::residual, {it.p, gb, nullptr, res, ld, w, 0.f, 0.f});
    for (int c = 0; c < w; ++c)
    {
      if (!one_pass)
      {
        vec::widen(hd, n, res + c * ld, _res64->get_values());
        restrictor->apply(*_res64, *_b_coarse);
      }
      else if (c > 0)
        ASSERT_THROW(hip_restrictor->restrict_residual_f32(fine, it.p + c * ld, gb + c * ld, *_b_coarse),
                     "internal: the one-pass residual restriction was refused");
      _hierarchy.apply(*_b_coarse, *_x_coarse, 1);
      restrictor->apply(*_x_coarse, *_corr64, OperatorMode::TRANS);
      vec::subtract_narrowed(hd, n, _corr64->get_values(), it.p + c * ld);
    }
    smooth();
    if (it.p != gx)
      for (int c = 0; c < w; ++c)
        MFMG_HIP_CHECK(hipMemcpyAsync(gx + c * ld, it.p + c * ld, sizeof(float) * n, hipMemcpyDeviceToDevice, hd.stream));
  }
}

// ---- HipSolver -----------------------------------------------------------------
void HipSolver::setup_direct(std::shared_ptr<SparseMatrixDevice<double>> matrix, DenseLu &f) const
{
  const int64_t n = matrix->m();
  f.n = n;
  std::vector<int32_t> rp, cl;
  std::vector<double> vl;
  matrix->download(rp, cl, vl);
  std::vector<double> dense((size_t)n * n, 0.);
  for (int64_t r = 0; r < n; ++r)
    for (int p = rp[r]; p < rp[r + 1]; ++p)
      dense[(size_t)r * n + cl[p]] += vl[p];
  std::vector<int32_t> perm;
  dense_lu_factor((int)n, dense, perm);
  if (n > kTriangularInverseLimit)
  {
    f.lu.upload(dense.data(), dense.size(), _handle.stream);
    f.perm.upload(perm.data(), perm.size(), _handle.stream);
    return;
  }
  dense_triangular_inverses((int)n, dense); // column-major: L^-1 below the diagonal (unit diagonal), U^-1 above
  // (L^-1 P): entry (i, perm[j]) = L^-1(i, j), j <= i ;  U^-1: entry (i, j), j >= i.  Rows of a dense
  // triangle are long, the SpMV takes 64 lanes per row
  HostCsr L, U;
  L.n_rows = L.n_cols = U.n_rows = U.n_cols = n;
  L.row_ptr.assign(n + 1, 0);
  U.row_ptr.assign(n + 1, 0);
  for (int64_t i = 0; i < n; ++i)
  {
    L.row_ptr[i + 1] = L.row_ptr[i] + (int32_t)(i + 1);
    U.row_ptr[i + 1] = U.row_ptr[i] + (int32_t)(n - i);
  }
  L.col.resize(L.row_ptr[n]);
  L.val.resize(L.row_ptr[n]);
  U.col.resize(U.row_ptr[n]);
  U.val.resize(U.row_ptr[n]);
  for (int64_t i = 0; i < n; ++i)
  {
    // columns sorted within the row (the permutation scatters them)
    std::vector<std::pair<int32_t, double>> row(i + 1);
    for (int64_t j = 0; j <= i; ++j)
      row[j] = {perm[j], j == i ? 1. : dense[(size_t)j * n + i]};
    std::sort(row.begin(), row.end());
    for (int64_t j = 0; j <= i; ++j)
    {
      L.col[L.row_ptr[i] + j] = row[j].first;
      L.val[L.row_ptr[i] + j] = row[j].second;
    }
    for (int64_t j = i; j < n; ++j)
    {
      U.col[U.row_ptr[i] + (j - i)] = (int32_t)j;
      U.val[U.row_ptr[i] + (j - i)] = dense[(size_t)j * n + i];
    }
  }
  f.l_inv_p = std::make_shared<SparseMatrixDevice<double>>(_handle, n, n, std::move(L.row_ptr), std::move(L.col),
                                                          std::move(L.val), false);
  f.u_inv = std::make_shared<SparseMatrixDevice<double>>(_handle, n, n, std::move(U.row_ptr), std::move(U.col),
                                                        std::move(U.val), false);
  // (triangular rows: half of them are long enough for a workgroup each)
  f.l_inv_p->set_kernel(n >= 512 ? 256 : 64, 0);
  f.u_inv->set_kernel(n >= 512 ? 256 : 64, 0);
  f.tmp.resize(n);
}

void HipSolver::solve_direct(DenseLu const &f, double const *b, double *x) const
{
  if (f.n <= 0)
    return;
  if (f.l_inv_p)
  {
    f.l_inv_p->vmult(f.tmp.data(), b);
    f.u_inv->vmult(x, f.tmp.data());
    return;
  }
  dense_lu_solve(_handle, (int)f.n, f.lu.data(), f.perm.data(), b, x);
}

HipSolver::HipSolver(HipHandle &handle, std::shared_ptr<Operator<DVector> const> op,
                     std::shared_ptr<ptree const> params, std::vector<double> const *near_null,
                     AmgGridHint const *grid)
    : Solver<DVector>(op, params), _handle(handle)
{
  _solver = to_lower(this->_params->get("solver.type", "lu_dense"));
  _matrix_operator = std::dynamic_pointer_cast<HipMatrixOperator const>(this->_operator);
  ASSERT_THROW(_matrix_operator != nullptr, "HipSolver needs a HipMatrixOperator");
  auto matrix = _matrix_operator->get_matrix();
  ASSERT_THROW(matrix->m() == matrix->n(), "The coarse matrix is not square");
  const int64_t n = matrix->m();
  const int op_space = _matrix_operator->domain_space();
  const bool distributed = _handle.comm.enabled() && op_space > 0;
  if (distributed && _solver != "amg")
    ASSERT_THROW_NOT_IMPLEMENTED("distributed runs support solver.type amg only (\"" + _solver + "\" requested)");
  if (_solver == "cholesky" || _solver == "lu_dense" || _solver == "lu_sparse_host")
  {
    // the three direct variants of source/cuda/cuda_solver.cu:51-72 share one dense factorisation here
    const int64_t limit = std::min(this->_params->get("solver.dense_limit", 8192), 16384);
    ASSERT_THROW(n <= limit, "The coarse problem (" + std::to_string(n) +
                                 " rows) is too large for the dense direct solver; use solver.type pcg");
    setup_direct(matrix, _dense);
  }
  else if (_solver == "amg")
  {
    // smoothed-aggregation hierarchy on the host (the role of ML / AMGx upstream), V-cycle on the device
    AmgOptions opts;
    opts.max_levels = this->_params->get("solver.amg.max_levels", 10);
    opts.coarsest_size = this->_params->get("solver.amg.coarsest_size", 1100);
    opts.strength = this->_params->get("solver.amg.strength", 0.08);
    opts.smooth_prolongator = this->_params->get("solver.amg.smooth_prolongator", true);
    opts.deep_level = this->_params->get("solver.amg.deep_level", 1 << 30);
    opts.deep_block = this->_params->get("solver.amg.deep_block", 2);
    _amg_cycles = this->_params->get("solver.amg.n_cycles", 1);
    // levels of the aggregation hierarchy (counted from its top) that pre-smooth; the ones below run V(0,1)
    _amg_pre_smoothing_levels = this->_params->get("solver.amg.pre_smoothing_levels", 1 << 20);
    ASSERT_THROW(opts.coarsest_size <= 16384, "solver.amg.coarsest_size is limited by the dense LU (16384)");
    std::vector<double> b0;
    if (near_null && (int64_t)near_null->size() == n)
      b0 = *near_null;
    else
      b0.assign(n, 1.);
    const bool geometric = this->_params->get("solver.amg.geometric_aggregates", true);
    AmgGridHint local_grid;
    if (geometric && grid)
    {
      local_grid = *grid;
      const int blk = this->_params->get("solver.amg.aggregate_block", 2);
      ASSERT_THROW(blk >= 2 && blk <= 8, "solver.amg.aggregate_block must be in 2..8");
      for (int d = 0; d < 3; ++d)
        local_grid.block[d] = blk;
    }
    auto smoother_params = std::make_shared<ptree>();
    smoother_params->put("smoother.type", "Chebyshev");
    smoother_params->put("smoother.degree", this->_params->get("solver.amg.smoother_degree", 1));
    smoother_params->put("smoother.smoothing_range", this->_params->get("solver.amg.smoothing_range", 4.));
    smoother_params->put("smoother.eig_cg_n_iterations", this->_params->get("solver.amg.eig_cg_n_iterations", 10));
    // setup "device": matrices of the hierarchy read off from operator applications on the device (probing), the
    // levels coupled across the ranks of a distributed run; "host": SpGEMM on the host cores (one rank only)
    // (default: the device wherever its preconditions hold -- one code path for one and for many ranks)
    bool device_ok = local_grid.valid(n) && opts.smooth_prolongator && local_grid.block[0] >= 2 &&
                     opts.deep_level >= (1 << 30) && std::all_of(b0.begin(), b0.end(), [](double v) { return v != 0.; });
    if (device_ok)
    {
      // node-major rows with the same number of components on every node (an agglomerate that yields fewer eigenvectors
      // breaks the pattern: such hierarchies keep the host setup)
      const int ncomp = std::max(local_grid.n_components, 1);
      device_ok = n % ncomp == 0;
      for (int64_t r = 0; device_ok && r < n; ++r)
        device_ok = local_grid.node_of_row[r] == r / ncomp &&
                    (local_grid.component_of_row.empty() ? 0 : local_grid.component_of_row[r]) == r % ncomp;
    }
    std::string const setup = to_lower(this->_params->get("solver.amg.setup", (distributed || device_ok) ? "device" : "host"));
    ASSERT_THROW(setup == "device" || setup == "host", "solver.amg.setup must be device or host");
    if (distributed || setup == "device")
    {
      ASSERT_THROW(setup == "device", "distributed runs build the aggregation hierarchy on the device (solver.amg.setup device)");
      ASSERT_THROW(device_ok, "the device setup of the aggregation hierarchy needs the agglomerate grid of the restrictor, a "
                              "smoothed prolongator, cubic aggregates and a near-null-space vector without zeros");
      setup_amg_on_device(matrix, b0, local_grid, opts, smoother_params);
      return;
    }
    HostCsr A0; // (only the host setup reads the matrix: 2.7 GB at 257^3 DoFs)
    A0.n_rows = A0.n_cols = n;
    matrix->download(A0.row_ptr, A0.col, A0.val);
    auto host_levels = build_aggregation_hierarchy(std::move(A0), std::move(b0), opts, local_grid.valid(n) ? &local_grid : nullptr);
    _amg.resize(host_levels.size());
    int reach = local_grid.valid(n) ? local_grid.reach : 0; // (recorded only: 0 without a grid)
    for (size_t l = 0; l < host_levels.size(); ++l)
    {
      _amg[l].reach = reach;
      reach = reach > 0 ? (local_grid.block[0] - 1 + 3 * reach) / local_grid.block[0] : 0;
      _amg[l].coarse_product = AmgLevel::by_host_product;
      if (l == 0)
        _amg[l].a = std::const_pointer_cast<HipMatrixOperator>(_matrix_operator);
      else
        _amg[l].a = std::make_shared<HipMatrixOperator>(upload(_handle, std::move(host_levels[l].A)));
      if (l + 1 < host_levels.size())
      {
        _amg[l].prolongator = std::make_shared<HipMatrixOperator>(upload(_handle, std::move(host_levels[l].P)));
        _amg[l].restrictor = std::dynamic_pointer_cast<HipMatrixOperator>(_amg[l].prolongator->transpose());
        _amg[l].smoother = std::make_shared<HipSmoother>(_amg[l].a, smoother_params);
      }
    }
    auto last = _amg.back().a->get_matrix();
    ASSERT_THROW(last->m() <= 16384, "the coarsest level of the multilevel solver is too large for the dense LU (" +
                                         std::to_string(last->m()) + " rows)");
    setup_direct(last, _amg_bottom);
  }
  else if (_solver == "pcg")
  {
    _n_iterations = this->_params->get("solver.n_iterations", 10);
    ASSERT_THROW(_n_iterations >= 0, "solver.n_iterations must be non-negative");
    _scal.resize(8);
    _dinv.resize(n);
    matrix->inverse_diagonal(_dinv.data());
  }
  else if (_solver == "amgx")
  {
    ASSERT_THROW_NOT_IMPLEMENTED("AMGx is not part of the HIP build (no AmgX shim); use solver.type pcg");
  }
  else
  {
    ASSERT_THROW(false, "Unknown solver name: \"" + _solver + "\"");
  }
}

void HipSolver::apply(DVector const &b, DVector &x) const
{
  auto matrix = _matrix_operator->get_matrix();
  const int64_t n = matrix->m();
  ASSERT_THROW(b.size() == n && x.size() == n, "vector sizes do not match the coarse operator");
  if (_solver == "amg")
  {
    if (_amg_gather_level == 0)
    {
      ASSERT_THROW(_amg_cycles <= 1, "solver.amg.n_cycles > 1 is not available when the first level is gathered");
      amg_cycle_gathered(0, b, x);
    }
    else if (_amg_cycles <= 1)
      amg_cycle(0, b, x);
    else
    {
      // stationary iteration: x += V(b - A x); the first cycle starts from zero
      amg_cycle(0, b, x);
      auto r = _amg[0].a->build_range_vector();
      auto e = _amg[0].a->build_range_vector();
      for (int c = 1; c < _amg_cycles; ++c)
      {
        _amg[0].a->residual(x, b, *r); // A x - b
        amg_cycle(0, *r, *e);
        x.add(-1., *e);
      }
    }
  }
  else if (_solver == "pcg")
  {
    // exactly n_iterations steps of Jacobi-preconditioned CG from a zero guess, all scalars on the
    // device (no host synchronisation inside the cycle)
    if (!_r)
    {
      _r = _matrix_operator->build_range_vector();
      _z = _matrix_operator->build_range_vector();
      _p = _matrix_operator->build_range_vector();
      _ap = _matrix_operator->build_range_vector();
    }
    x = 0.;
    *_r = b;
    vec::scale_pointwise<double>(_handle, n, _dinv.data(), _r->get_values(), _z->get_values());
    *_p = *_z;
    vec::dot_async<double>(_handle, n, _r->get_values(), _z->get_values(), _scal.data(), 0);
    for (int it = 0; it < _n_iterations; ++it)
    {
      const int cur = it & 1, nxt = cur ^ 1;
      matrix->vmult(_ap->get_values(), _p->get_values());
      vec::dot_async<double>(_handle, n, _p->get_values(), _ap->get_values(), _scal.data(), 2);
      vec::cg_update<double>(_handle, n, _p->get_values(), _ap->get_values(), _dinv.data(), x.get_values(),
                             _r->get_values(), _z->get_values(), _scal.data(), cur, 2);
      vec::dot_async<double>(_handle, n, _r->get_values(), _z->get_values(), _scal.data(), nxt);
      vec::cg_direction<double>(_handle, n, _z->get_values(), _p->get_values(), _scal.data(), nxt, cur);
    }
  }
  else
  {
    ASSERT_THROW(b.get_values() != x.get_values(), "the coarse solve cannot run in place");
    solve_direct(_dense, b.get_values(), x.get_values());
  }
}

// One V-cycle of the aggregation hierarchy: the same recursion as Hierarchy::apply
// (include/mfmg/common/hierarchy.hpp:246-309) with restrictor = P^T and a zero initial guess (the
// content of x on entry is ignored).
void HipSolver::amg_cycle(size_t level, DVector const &b, DVector &x) const
{
  AmgLevel const &L = _amg[level];
  if (level + 1 == _amg.size())
  {
    solve_direct(_amg_bottom, b.get_values(), x.get_values());
    return;
  }
  if (!L.res)
  {
    L.res = L.a->build_range_vector();
    // (the coarse vectors have the local layout of the restrictor's rows; a gathered next level has global ones)
    L.b_coarse = L.restrictor->build_range_vector();
    L.x_coarse = L.restrictor->build_range_vector();
    L.x_work = L.a->build_range_vector();
  }
  // the iterate lives in x_work until the post-smoother writes its result into x
  if ((int)level >= _amg_pre_smoothing_levels)
  {
    // V(0,1) on this level ("solver.amg.pre_smoothing_levels"): from x = 0 the residual is -b, so b itself is restricted and
    // the correction ADDED (the two signs cancel exactly: the same bits as restricting -b and subtracting) -- no smoother
    // launch, no operator application before the recursion
    L.restrictor->apply(b, *L.b_coarse);
    if ((int)level + 1 == _amg_gather_level)
      amg_cycle_gathered(level + 1, *L.b_coarse, *L.x_coarse);
    else
      amg_cycle(level + 1, *L.b_coarse, *L.x_coarse);
    if (L.smoothed_prolongator)
    {
      // prolongation and post-smoothing in one operator (AmgLevel::smoothed_prolongator)
      L.smoothed_prolongator->apply_plus_scaled(*L.x_coarse, L.a->get_diagonal_inverse(), b, L.smoothed_beta, x);
      return;
    }
    L.prolongator->apply(*L.x_coarse, *L.x_work, OperatorMode::NO_TRANS);
    L.smoother->apply_to(b, *L.x_work, x);
    return;
  }
  L.smoother->apply_zero_guess(b, *L.x_work); // zero initial guess by construction
  L.a->residual(*L.x_work, b, *L.res);
  L.restrictor->apply(*L.res, *L.b_coarse);
  if ((int)level + 1 == _amg_gather_level)
    amg_cycle_gathered(level + 1, *L.b_coarse, *L.x_coarse);
  else
    amg_cycle(level + 1, *L.b_coarse, *L.x_coarse);
  L.prolongator->apply_subtract(*L.x_coarse, *L.x_work, OperatorMode::NO_TRANS);
  L.smoother->apply_to(b, *L.x_work, x);
}

// ---- the V-cycle on a block of vectors ----
namespace
{
// `width` vectors of n entries as the columns of one zeroed block at the distance ld
std::vector<std::shared_ptr<DVector>> build_block(HipHandle &handle, int64_t n, int width, int64_t ld)
{
  auto storage = std::make_shared<DeviceBuffer<double>>((size_t)width * ld); // (hipMalloc: aligned to 256 bytes)
  vec::set<double>(handle, (int64_t)width * ld, 0., storage->data());
  std::vector<std::shared_ptr<DVector>> columns;
  for (int c = 0; c < width; ++c)
    columns.emplace_back(new DVector(handle, n, storage->data() + (int64_t)c * ld), [storage](DVector *v) { delete v; });
  return columns;
}
template <typename V>
std::vector<V *> first_columns(std::vector<std::shared_ptr<DVector>> const &block, size_t w)
{
  std::vector<V *> columns;
  for (size_t c = 0; c < w; ++c)
    columns.push_back(block[c].get());
  return columns;
}
} // namespace

bool HipSolver::block_cycle_available() const
{
  return _solver == "amg" && _amg_cycles <= 1 && _amg_gather_level < 0 && !_handle.comm.enabled() && !_amg.empty();
}

int HipSolver::block_width() const
{
  if (!block_cycle_available())
    return 1;
  int width = 1;
  for (auto const &L : _amg)
    for (auto const &op : {L.a, L.restrictor, L.prolongator, L.smoothed_prolongator})
      if (op)
        width = std::max(width, op->block_width());
  return width;
}

void HipSolver::matrix_launch_counters(int64_t &block_launches, int64_t &vector_launches) const
{
  block_launches = vector_launches = 0;
  auto count = [&](std::shared_ptr<SparseMatrixDevice<double>> const &m) {
    if (!m)
      return;
    int64_t blocks = 0, columns = 0;
    m->block_counters(blocks, columns);
    block_launches += blocks;
    vector_launches += m->vector_launches();
  };
  for (auto const &L : _amg)
    for (auto const &op : {L.a, L.restrictor, L.prolongator, L.smoothed_prolongator})
      if (op)
        count(op->get_matrix());
  count(_amg_bottom.l_inv_p);
  count(_amg_bottom.u_inv);
}

void HipSolver::apply_block(std::vector<DVector const *> const &b, std::vector<DVector *> const &x) const
{
  ASSERT_THROW(b.size() == x.size() && !b.empty(), "a block needs as many right-hand sides as iterates");
  int64_t blocks0 = 0, vectors0 = 0;
  matrix_launch_counters(blocks0, vectors0);
  const int64_t ld = block_leading_dimension(b);
  const bool block = block_cycle_available() && b.size() > 1 && b.size() <= (size_t)kMfBlockMaxVectors && ld != 0 &&
                     block_kernel_layout(b, ld) && block_kernel_layout(as_const(x), ld);
  if (!block)
    Solver<DVector>::apply_block(b, x);
  else
  {
    const int64_t n = _matrix_operator->get_matrix()->m();
    ASSERT_THROW(b[0]->size() == n && x[0]->size() == n, "vector sizes do not match the coarse operator");
    int widths[kMfBlockMaxGroups];
    const int n_groups = mf_block_groups((int)b.size(), widths);
    size_t c0 = 0;
    for (int g = 0; g < n_groups; c0 += widths[g], ++g)
    {
      if (widths[g] == 1)
        apply(*b[c0], *x[c0]);
      else
        amg_cycle_block(0, ld, std::vector<DVector const *>(b.begin() + c0, b.begin() + c0 + widths[g]),
                        std::vector<DVector *>(x.begin() + c0, x.begin() + c0 + widths[g]));
    }
  }
  int64_t blocks1 = 0, vectors1 = 0;
  matrix_launch_counters(blocks1, vectors1);
  _last_block_launches += blocks1 - blocks0;
  _last_vector_launches += vectors1 - vectors0;
}

// amg_cycle, step by step, on the w columns b and x (each a block at the distance ld)
void HipSolver::amg_cycle_block(size_t level, int64_t ld, std::vector<DVector const *> const &b, std::vector<DVector *> const &x) const
{
  AmgLevel const &L = _amg[level];
  const size_t w = b.size();
  if (level + 1 == _amg.size())
  {
    DenseLu const &f = _amg_bottom;
    if (f.n > 0 && f.l_inv_p && f.l_inv_p->block_width() == 4 && f.u_inv->block_width() == 4)
    {
      // solve_direct on the group: x = U^-1 ((L^-1 P) b), two launches through a group-wide tmp
      constexpr int group = 4;
      const int64_t ld_tmp = f.n + (f.n & 1);
      if (f.tmp_block.size() < (size_t)group * ld_tmp)
      {
        MemoryKind kind("coarse solver: block workspace of the bottom solve (one group of right-hand sides)");
        f.tmp_block.resize((size_t)group * ld_tmp);
        vec::set<double>(_handle, (int64_t)group * ld_tmp, 0., f.tmp_block.data());
      }
      f.l_inv_p->apply_mode_block(CsrMode::apply, (int)w, b[0]->get_values(), ld, nullptr, nullptr, nullptr, 0., 0., f.tmp_block.data(), ld_tmp);
      f.u_inv->apply_mode_block(CsrMode::apply, (int)w, f.tmp_block.data(), ld_tmp, nullptr, nullptr, nullptr, 0., 0., x[0]->get_values(), ld);
      return;
    }
    for (size_t c = 0; c < w; ++c)
      solve_direct(_amg_bottom, b[c]->get_values(), x[c]->get_values());
    return;
  }
  constexpr int group = 4; // (the widest group of mf_block_groups)
  const int64_t n_coarse = L.restrictor->get_matrix()->m(), ld_coarse = n_coarse + (n_coarse & 1);
  if (L.res_block.empty() || L.block_ld != ld)
  {
    MemoryKind kind("coarse solver: block workspaces of the aggregation levels (one group of right-hand sides)");
    L.res_block.clear(); // (before the new ones are built)
    L.x_work_block.clear();
    const int64_t n = L.a->get_matrix()->m();
    L.res_block = build_block(_handle, n, group, ld);
    L.x_work_block = build_block(_handle, n, group, ld);
    if (L.b_coarse_block.empty())
    {
      L.b_coarse_block = build_block(_handle, n_coarse, group, ld_coarse);
      L.x_coarse_block = build_block(_handle, n_coarse, group, ld_coarse);
    }
    L.block_ld = ld;
  }
  const auto res = first_columns<DVector>(L.res_block, w), x_work = first_columns<DVector>(L.x_work_block, w),
             b_coarse = first_columns<DVector>(L.b_coarse_block, w), x_coarse = first_columns<DVector>(L.x_coarse_block, w);
  // (no level below is gathered: block_cycle_available)
  if ((int)level >= _amg_pre_smoothing_levels)
  {
    // V(0,1) on this level, as in amg_cycle: b itself is restricted and the correction added
    L.restrictor->apply_block(b, b_coarse);
    amg_cycle_block(level + 1, ld_coarse, as_const(b_coarse), x_coarse);
    if (L.smoothed_prolongator)
    {
      L.smoothed_prolongator->apply_plus_scaled_block(as_const(x_coarse), L.a->get_diagonal_inverse(), b, L.smoothed_beta, x);
      return;
    }
    L.prolongator->apply_block(as_const(x_coarse), x_work);
    L.smoother->apply_to_block(b, as_const(x_work), x);
    return;
  }
  L.smoother->apply_zero_guess_block(b, x_work);
  L.a->residual_block(as_const(x_work), b, res);
  L.restrictor->apply_block(as_const(res), b_coarse);
  amg_cycle_block(level + 1, ld_coarse, as_const(b_coarse), x_coarse);
  L.prolongator->apply_subtract_block(as_const(x_coarse), x_work, OperatorMode::NO_TRANS);
  L.smoother->apply_to_block(b, as_const(x_work), x);
}

void HipSolver::amg_cycle_gathered(size_t level, DVector const &b_local, DVector &x_local) const
{
  HaloSpace const &s = _handle.comm.spaces[_gather_space];
  const int64_t n_own = s.n_owned();
  ASSERT_THROW(b_local.size() == s.n_local() && x_local.size() == b_local.size(), "vector sizes do not match the gathered level");
  if (!s.split_xy())
  {
    MFMG_HIP_CHECK(hipMemcpyAsync(_gather_in.data(), b_local.get_values() + s.owned_begin * s.layer_elems,
                                  (size_t)n_own * sizeof(double), hipMemcpyDeviceToDevice, _handle.stream));
    _handle.comm.transport->allgather(_gather_in.data(), n_own, _gather_b->get_values(), _handle.stream);
    amg_cycle(level, *_gather_b, *_gather_x);
    // the local layers (ghost layers included) are a contiguous run of the global ones
    MFMG_HIP_CHECK(hipMemcpyAsync(x_local.get_values(), _gather_x->get_values() + s.global_begin * s.layer_elems,
                                  (size_t)x_local.size() * sizeof(double), hipMemcpyDeviceToDevice, _handle.stream));
    return;
  }
  // boxes: the owned sub-box is packed, the gathered blocks (rank order) are permuted into the global lexicographic order, and
  // the local box (ghosts included) is read back through its global ids
  halo_box_copy(const_cast<double *>(b_local.get_values()), s, true, _gather_in.data(), 0, _handle.stream);
  _handle.comm.transport->allgather(_gather_in.data(), n_own, _gather_ranked.data(), _handle.stream);
  gather_indexed(_gather_b->size(), _gather_ranked.data(), _gather_from_ranked.data(), _gather_b->get_values(), _handle.stream);
  amg_cycle(level, *_gather_b, *_gather_x);
  gather_indexed(x_local.size(), _gather_x->get_values(), _gather_local_ids.data(), x_local.get_values(), _handle.stream);
}

// ---- HipHierarchyHelpers ---------------------------------------------------------
template <typename VectorType>
std::shared_ptr<Operator<VectorType>>
HipHierarchyHelpers<VectorType>::get_global_operator(std::shared_ptr<MeshEvaluator> mesh_evaluator)
{
  if (_operator == nullptr)
  {
    if (mesh_evaluator->get_mesh_evaluator_type() == "HipMatrixFreeMeshEvaluator")
    {
      auto mf = std::dynamic_pointer_cast<HipMatrixFreeMeshEvaluator>(mesh_evaluator);
      ASSERT_THROW(mf != nullptr, "downcasting failed");
      _operator = std::make_shared<HipMatrixFreeOperator>(mf);
    }
    else
    {
      auto hip_mesh_evaluator = std::dynamic_pointer_cast<HipMeshEvaluator>(mesh_evaluator);
      ASSERT_THROW(hip_mesh_evaluator != nullptr, "downcasting failed");
      _operator = std::make_shared<HipMatrixOperator>(hip_mesh_evaluator->evaluate_global());
    }
  }
  return _operator;
}

template <typename VectorType>
std::shared_ptr<Operator<VectorType>>
HipHierarchyHelpers<VectorType>::build_restrictor(Communicator, std::shared_ptr<MeshEvaluator> mesh_evaluator,
                                                  std::shared_ptr<ptree const> params)
{
  auto hip_mesh_evaluator = std::dynamic_pointer_cast<HipMeshEvaluator>(mesh_evaluator);
  ASSERT_THROW(hip_mesh_evaluator != nullptr, "downcasting failed");
  RestrictorOptions opts = hip_mesh_evaluator->agglomerate_options(*params);
  auto global_diag = hip_mesh_evaluator->get_locally_relevant_diag();
  _grid_hint = AmgGridHint();
  // agglomerate eigenproblems: batched on the device (default: dense up to 64 nodes per agglomerate, beyond that on the host
  // cores), on the host cores ("restrictor.eigensolver host"), or by the matrix-free Lanczos solver on the device up to 729
  // nodes ("restrictor.eigensolver lanczos", amge_lanczos.hip)
  std::string const where = params->get("restrictor.eigensolver", "device");
  ASSERT_THROW(where == "device" || where == "host" || where == "lanczos", "restrictor.eigensolver must be device, host or lanczos");
  const bool verbose = std::getenv("MFMG_HIP_VERBOSE") != nullptr;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_r0 = now();
  AmgeEigensolverInfo eig_info;
  HostCsr R = build_restrictor_structured(hip_mesh_evaluator->get_mesh(), global_diag, opts, &_grid_hint.node_of_row,
                                          _grid_hint.dims, where != "host" ? &_handle : nullptr, &eig_info);
  {
    int64_t *f = _handle.restrictor_eigensolver_info;
    f[0] = eig_info.solver;
    f[1] = eig_info.nodes_per_agglomerate;
    f[2] = eig_info.agglomerates;
    f[3] = eig_info.solves;
    f[4] = eig_info.max_iterations;
    f[5] = eig_info.breakdowns;
    f[6] = eig_info.unconverged;
    _handle.restrictor_eigensolver_seconds = eig_info.kernel_seconds;
  }
  // "setup value precision" float | double (default): round the matrices of the setup to float-representable values
  // (R here; R A R^T and the aggregation hierarchy where they are assembled: probe_assembly.hip).  The hierarchy is then
  // the exact FP64 cycle of the ROUNDED matrices -- what get_restrictor / get_coarse_operator hand out -- and the stored
  // blocks of a variable-coefficient problem take half the bytes.  It applies to the device setup by probing.
  {
    std::string const prec = to_lower(params->get("setup value precision", "double"));
    ASSERT_THROW(prec == "double" || prec == "float", "\"setup value precision\" must be double or float");
    _handle.setup_values_float = prec == "float";
    if (_handle.setup_values_float)
    {
#pragma omp parallel for schedule(static)
      for (int64_t p = 0; p < (int64_t)R.val.size(); ++p)
        R.val[p] = (double)(float)R.val[p];
    }
  }
  const double t_r1 = now();
  // R A R^T couples agglomerates up to two apart along an axis where they are one cell wide (HipMatrixOperator::multiply)
  _grid_hint.reach = 1;
  for (int d = 0; d < hip_mesh_evaluator->get_mesh().dim; ++d)
    if (opts.agglomerate[d] == 1)
      _grid_hint.reach = 2;
  // component of a coarse row = its position among the eigenvectors of its agglomerate
  _grid_hint.component_of_row.resize(_grid_hint.node_of_row.size());
  _grid_hint.n_components = 1;
  for (size_t r = 0; r < _grid_hint.node_of_row.size(); ++r)
  {
    const int comp = (r > 0 && _grid_hint.node_of_row[r] == _grid_hint.node_of_row[r - 1])
                         ? _grid_hint.component_of_row[r - 1] + 1
                         : 0;
    _grid_hint.component_of_row[r] = comp;
    _grid_hint.n_components = std::max(_grid_hint.n_components, comp + 1);
  }
  HaloCommunicator &comm = _handle.comm;
  if (comm.enabled())
  {
    ASSERT_THROW(comm.spaces_owner == nullptr || comm.spaces_owner == this,
                 "this distributed context already carries a hierarchy: its halo spaces are in use -- destroy that "
                 "hierarchy first (one hierarchy per communicator context at a time)");
    comm.spaces_owner = this;
    // the b-prefetch state of the context follows the smoother of THIS hierarchy (set by its first sweep): none of an earlier one
    _handle.rhs_ghosts_wanted = false;
    _handle.rhs_ghost_width = 1;
    // first coarse level: the agglomerates of the local mesh, `n_components` unknowns each
    HaloSpace &cs = comm.spaces[2];
    cs = HaloSpace();
    const int64_t per_layer = (int64_t)_grid_hint.dims[0] * _grid_hint.dims[1] * _grid_hint.n_components;
    ASSERT_THROW(R.n_rows == per_layer * _grid_hint.dims[2],
                 "distributed runs need the same number of eigenvectors on every agglomerate");
    cs.comps = _grid_hint.n_components;
    cs.layer_elems = per_layer;
    cs.n_layers = _grid_hint.dims[2];
    cs.width = 1;
    for (int d = 0; d < 3; ++d)
    {
      const bool low = comm.ghost_lo[d] > 0, high = comm.ghost_hi[d] > 0;
      ASSERT_THROW((!low && !high) || opts.agglomerate[d] == 2, "distributed runs need agglomerates of 2 cells along a split axis");
      const int64_t own0 = comm.ghost_lo[d] / 2; // (2 ghost cell layers = one agglomerate; two of them with deep low ghosts)
      const int64_t own_n = _grid_hint.dims[d] - own0 - comm.ghost_hi[d] / 2;
      const int64_t g0 = (int64_t)comm.coord[d] * own_n - own0, gn = (int64_t)comm.grid[d] * own_n;
      if (d == 2)
      {
        cs.has_low = low;
        cs.has_high = high;
        cs.owned_begin = own0;
        cs.owned_count = own_n;
        cs.global_begin = g0;
        cs.global_layers = gn;
      }
      else
      {
        cs.n_xy[d] = _grid_hint.dims[d];
        cs.low_xy[d] = low;
        cs.high_xy[d] = high;
        cs.own0_xy[d] = own0;
        cs.own_n_xy[d] = own_n;
        cs.g0_xy[d] = g0;
        cs.gn_xy[d] = gn;
      }
    }
    comm.spaces.resize(3); // the spaces of the aggregation levels belong to the coarse solver built next
    // rows of the neighbours' agglomerates stay: the lower neighbour's top face is my first owned plane
    // (prolongation), and the Galerkin product of my boundary rows couples to both ghost layers
  }
  std::shared_ptr<StructuredRestrictorDevice> structured;
  // (distributed runs: the local mesh -- owned slab plus one agglomerate layer of each neighbour -- is itself a
  // full structured mesh and R keeps the rows of the neighbours' agglomerates, so the same evaluation applies)
  if (params->get("restrictor.structured", true))
    structured = StructuredRestrictorDevice::create(_handle, hip_mesh_evaluator->get_mesh(), opts.agglomerate,
                                                    _grid_hint.dims, _grid_hint.node_of_row, R);
  const double t_r2 = now();
  // (with the agglomerate-wise form in place the CSR copy serves the setup algebra and get_restrictor only: no layouts)
  auto restrictor = std::make_shared<HipMatrixOperator>(upload(_handle, std::move(R), structured == nullptr));
  restrictor->set_structured(structured);
  if (verbose)
    std::fprintf(stderr, "[mfmg_hip] restrictor: eigenproblems and CSR assembly %.2f s, agglomerate-wise layout %.2f s, upload %.2f s\n",
                 t_r1 - t_r0, t_r2 - t_r1, now() - t_r2);
  if (comm.enabled())
    restrictor->set_spaces(1, 2);
  _own_restrictor = restrictor;
  _ap_operator.reset();
  _ap_weak.reset();
  _fast_ap_prepared = params->get("fast_ap", false);
  if (_fast_ap_prepared)
    _ap_operator = get_global_operator(mesh_evaluator)->multiply_transpose(restrictor);
  return restrictor;
}

template <typename VectorType>
std::shared_ptr<Operator<VectorType>> HipHierarchyHelpers<VectorType>::fast_multiply_transpose()
{
  ASSERT_THROW(_fast_ap_prepared, "fast_multiply_transpose needs a restrictor built with fast_ap = true");
  // (the assembled A R^T holds 125 entries per coarse row: handed over, not kept alive here; formed again if a later
  // call finds it gone)
  auto ap = _ap_operator ? _ap_operator : _ap_weak.lock();
  if (!ap)
    ap = _operator->multiply_transpose(_own_restrictor);
  _ap_weak = ap;
  _ap_operator.reset();
  return ap;
}

template <typename VectorType>
std::shared_ptr<Smoother<VectorType>>
HipHierarchyHelpers<VectorType>::build_smoother(std::shared_ptr<Operator<VectorType> const> op,
                                                std::shared_ptr<ptree const> params)
{
  return std::make_shared<HipSmoother>(op, params);
}

template <typename VectorType>
std::shared_ptr<Solver<VectorType>>
HipHierarchyHelpers<VectorType>::build_coarse_solver(std::shared_ptr<Operator<VectorType> const> op,
                                                     std::shared_ptr<ptree const> params)
{
  // near-null-space hint for the multilevel solver: the coarse image R 1 of the constant
  std::vector<double> near_null;
  auto r = std::dynamic_pointer_cast<HipMatrixOperator const>(_restrictor_hint);
  auto a = std::dynamic_pointer_cast<HipMatrixOperator const>(op);
  if (r && a && r->get_matrix()->m() == a->get_matrix()->m())
  {
    // R 1 on the device (the row sums of R; downloading its 113 M entries for that cost 0.4 s)
    DVector ones(_handle, r->get_matrix()->n()), sums(_handle, r->get_matrix()->m());
    ones = 1.;
    r->apply_local(ones.get_values(), sums.get_values());
    near_null.resize((size_t)sums.size());
    MFMG_HIP_CHECK(hipMemcpyAsync(near_null.data(), sums.get_values(), near_null.size() * sizeof(double), hipMemcpyDeviceToHost, _handle.stream));
    MFMG_HIP_CHECK(hipStreamSynchronize(_handle.stream));
  }
  // the agglomerate grid is known only for the restrictor this object built itself
  const bool own = _restrictor_hint && _restrictor_hint == _own_restrictor;
  if (own && !near_null.empty())
  {
    // candidates per component: the image of the constant for the first eigenvector of every
    // agglomerate, the unit coefficient for the others (smooth fields have smooth coefficients)
    for (size_t i = 0; i < near_null.size(); ++i)
      if (_grid_hint.component_of_row[i] > 0)
        near_null[i] = 1.;
  }
  return std::make_shared<HipSolver>(_handle, op, params, near_null.empty() ? nullptr : &near_null,
                                     own ? &_grid_hint : nullptr);
}

template <typename VectorType>
void HipHierarchyHelpers<VectorType>::prepare_residual_restriction(std::shared_ptr<Operator<VectorType> const> a,
                                                                   std::shared_ptr<Operator<VectorType>> restrictor,
                                                                   std::shared_ptr<ptree const> params)
{
  auto r = std::dynamic_pointer_cast<HipMatrixOperator>(restrictor);
  if (!r || !r->has_structured())
    return;
  char const *env = std::getenv("MFMG_FUSED_RESIDUAL");
  if ((env && std::string(env) == "0") || (params && !params->get("restrictor.fused_residual", true)))
    return;
  r->prepare_residual_restriction(a);
}

template class HipHierarchyHelpers<DVector>;
} // namespace mfmg
