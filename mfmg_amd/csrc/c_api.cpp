// extern "C" boundary of libmfmg_hip.so (include/mfmg_hip.h): exceptions of the C++
// mirror are mapped to status codes; messages are kept per thread.
#include <array>
#include <cmath>
#include <cstring>
#include <exception>
#include <string>

#include "amge_lanczos.hpp"
#include "block_krylov.hpp"
#include "block_krylov_basis.hpp"
#include "cell_contraction.hpp"
#include "dof_permutation.hpp"
#include "halo_transport.hpp"
#include "krylov_basis.hpp"
#include "krylov_drivers.hpp"
#include "mf_z_tiles.hpp"
#include "mfmg/hierarchy.hpp"
#include "mfmg/hip_high_order.hpp"

using namespace mfmg;

namespace
{
thread_local std::string g_last_error;

template <typename F>
int guarded(F &&f)
{
  try
  {
    f();
    return MFMG_HIP_SUCCESS;
  }
  catch (NotImplementedExc const &e)
  {
    g_last_error = e.what();
    return MFMG_HIP_ERROR_NOT_IMPLEMENTED;
  }
  catch (InvalidArgumentExc const &e)
  {
    g_last_error = e.what();
    return MFMG_HIP_ERROR_INVALID_ARGUMENT;
  }
  catch (DeviceExc const &e)
  {
    g_last_error = e.what();
    return MFMG_HIP_ERROR_DEVICE;
  }
  catch (std::exception const &e)
  {
    g_last_error = e.what();
    return MFMG_HIP_ERROR_RUNTIME;
  }
  catch (...)
  {
    g_last_error = "unknown exception";
    return MFMG_HIP_ERROR_RUNTIME;
  }
}

void require(bool cond, char const *what)
{
  if (!cond)
    throw InvalidArgumentExc(what);
}
} // namespace

struct mfmg_hip_context_s
{
  std::unique_ptr<HipHandle> handle;
};

struct mfmg_hip_csr_s
{
  std::shared_ptr<HipMatrixOperator> op; // owns the SparseMatrixDevice
  bool borrowed = false;
};

struct mfmg_hip_mf_laplace_s
{
  std::shared_ptr<MatrixFreeLaplaceDevice<double>> op;
};

struct mfmg_hip_mf_laplace_f32_s
{
  std::shared_ptr<MatrixFreeLaplaceDevice<float>> op;
};

struct mfmg_hip_host_csr_s
{
  HostCsr m;
};

struct mfmg_hip_host_amg_s
{
  std::vector<AmgLevelHost> levels;
};

struct mfmg_hip_hierarchy_s
{
  HipHandle *handle = nullptr;
  std::shared_ptr<HipMeshEvaluator> evaluator;
  std::shared_ptr<TimerOutput> timer;
  std::unique_ptr<Hierarchy<DVector>> hierarchy;
  mfmg_hip_csr_s restrictor_view, coarse_view, amg_view, fine_view;
  int64_t eigensolver_info[MFMG_HIP_EIGENSOLVER_INFO_FIELDS] = {0, 0, 0, 0, 0, 0, 0}; // what solved the agglomerate eigenproblems
  double eigensolver_seconds = 0.;
  bool setup_values_float = false; // "setup value precision" of THIS hierarchy: on the handle only while one of its setups runs
  // "fine level precision" float: the matrix-free operator and its smoother in FP32 around the FP64 coarse levels
  std::unique_ptr<HipFloatFineLevel> fine_f32;
  // "internal numbering" lexicographic: the hierarchy above was built from the mesh in the lexicographic numbering of its nodes.
  // `perm` is set where the caller's numbering is another one: vectors are then permuted where they cross this file, into and
  // out of library-owned vectors of the fine level (built at first use)
  bool lexicographic = false;
  std::unique_ptr<DofPermutation> perm;
  DeviceBuffer<double> work[2];
  DeviceBuffer<float> work_f32[2];
  KrylovWorkspaces krylov; // what the drivers of krylov_drivers.hpp keep between solves
  // block entry points: the permuted columns of one group (b, x) and what the last block call did
  DeviceBuffer<double> block_work[2];
  int64_t block_info[MFMG_HIP_BLOCK_INFO_FIELDS] = {1, 0, 0};
  int64_t block_info_f32[MFMG_HIP_BLOCK_INFO_FIELDS] = {1, 0, 0}; // ... and the last FP32 block call
  int64_t block_solve_allreduces = 0; // all-reduces of the last mfmg_hip_hierarchy_solve_fgmres_block (0 on one rank)
  // the transfer counters of every level (transfer_counters below) when the last block call began
  std::vector<std::array<int64_t, 3>> transfer_snapshot;
  DeviceBuffer<float> block_work_f32[2];
  float *block_workspace_f32(int i, size_t n)
  {
    if (block_work_f32[i].size() < n)
    {
      MemoryKind kind("hierarchy: FP32 block workspace (permuted columns)");
      block_work_f32[i].release();
      block_work_f32[i].resize(n);
      MFMG_HIP_CHECK(hipMemsetAsync(block_work_f32[i].data(), 0, n * sizeof(float), handle->stream));
    }
    return block_work_f32[i].data();
  }
  double *block_workspace(int i, size_t n)
  {
    if (block_work[i].size() < n)
    {
      MemoryKind kind("hierarchy: block workspace (permuted columns of one group)");
      block_work[i].resize(n);
      MFMG_HIP_CHECK(hipMemsetAsync(block_work[i].data(), 0, n * sizeof(double), handle->stream));
    }
    return block_work[i].data();
  }
  double *workspace(int i)
  {
    if (work[i].size() == 0)
      work[i].resize((size_t)perm->n_dofs());
    return work[i].data();
  }
  float *workspace_f32(int i)
  {
    if (work_f32[i].size() == 0)
      work_f32[i].resize((size_t)perm->n_dofs());
    return work_f32[i].data();
  }
};

struct mfmg_hip_mf_laplace_q2_s
{
  HipHandle *handle = nullptr;
  std::shared_ptr<HipQ2Operator> op;
  MatrixFreeLaplaceQ2Device<double> &device() const { return *op->get_device_operator(); }
};

struct mfmg_hip_high_order_s
{
  mfmg_hip_hierarchy_t hierarchy = nullptr; // borrowed
  std::unique_ptr<HighOrderPreconditioner> prec;
};

namespace
{
int64_t level_size(mfmg_hip_hierarchy_t h, int level)
{
  require(level >= 0 && level < (int)h->hierarchy->levels().size(), "level out of range");
  return level_size(*h->hierarchy, level);
}

// the blocks b and x of n_vectors columns of level `level`, of doubles or floats: columns are aligned to two scalars
template <typename T>
void check_block_shape(mfmg_hip_hierarchy_t h, int level, int32_t n_vectors, int64_t ld, const T *b, const T *x)
{
  constexpr bool f64 = sizeof(T) == 8;
  require(n_vectors >= 1 && n_vectors <= MFMG_HIP_BLOCK_MAX_VECTORS, "a block holds 1 to 64 vectors");
  require(b && x, "null argument");
  const int64_t n = level_size(h, level);
  require(ld >= n, "the leading dimension of a block must be at least the vector size");
  require(ld % 2 == 0, f64 ? "the leading dimension of a block must be even (columns aligned to 16 bytes)"
                           : "the leading dimension of a block must be even (columns aligned to 8 bytes)");
  require(reinterpret_cast<uintptr_t>(b) % (2 * sizeof(T)) == 0 && reinterpret_cast<uintptr_t>(x) % (2 * sizeof(T)) == 0,
          f64 ? "the base of a block must be aligned to 16 bytes" : "the base of a block must be aligned to 8 bytes");
  const int64_t extent = (int64_t)(n_vectors - 1) * ld + n;
  require(b + extent <= x || x + extent <= b, "the blocks b and x overlap");
}

// What the drivers of krylov_drivers.hpp run on.  A one-vector driver gathers permuted vectors into the library's two.
KrylovSetting krylov_setting(mfmg_hip_hierarchy_t h, bool one_vector)
{
  const bool work = one_vector && h->perm;
  return {*h->handle, *h->hierarchy, h->fine_f32.get(), h->perm.get(), h->timer, {work ? h->workspace(0) : nullptr, work ? h->workspace(1) : nullptr},
          h->krylov};
}

// ... with the Q2 operator and the high-order preconditioner as the outer pair; the working sets are those of the Q1 hierarchy
KrylovSetting high_order_setting(mfmg_hip_high_order_t p)
{
  KrylovSetting s = krylov_setting(p->hierarchy, true);
  s.fine_f32 = nullptr;
  s.outer_operator = p->prec->get_operator();
  HighOrderPreconditioner const *prec = p->prec.get();
  s.outer_preconditioner = [prec](DVector const &r, DVector &z) { prec->apply(r, z); };
  return s;
}

// (per column; one column from the one-vector drivers)
void deliver_result(KrylovResult const &result, int32_t *n_iterations, double *final_residuals, int64_t *work)
{
  if (n_iterations)
    std::copy(result.iterations.begin(), result.iterations.end(), n_iterations);
  if (final_residuals)
    std::copy(result.residuals.begin(), result.residuals.end(), final_residuals);
  if (work)
    std::copy(result.work, result.work + 4, work);
}
} // namespace

extern "C" {

const char *mfmg_hip_last_error(void) { return g_last_error.c_str(); }
const char *mfmg_hip_version(void) { return "mfmg-hip 0.3.0 (gfx950)"; }
int mfmg_hip_abi_version(void) { return MFMG_HIP_ABI_VERSION; }

int mfmg_hip_memory_inventory(char *buffer, size_t buffer_size)
{
  return guarded([&] {
    require(buffer != nullptr && buffer_size > 0, "null argument");
    const std::string text = DeviceMemoryLedger::get().report();
    std::snprintf(buffer, buffer_size, "%s", text.c_str());
  });
}

// ---- context -------------------------------------------------------------------
int mfmg_hip_context_create(void *hip_stream, mfmg_hip_context_t *ctx)
{
  return guarded([&] {
    require(ctx != nullptr, "null output handle");
    int n_dev = 0;
    hipError_t err = hipGetDeviceCount(&n_dev);
    if (err != hipSuccess || n_dev == 0)
      throw DeviceExc("no HIP device available: the mfmg HIP path has no CPU fallback");
    auto c = new mfmg_hip_context_s;
    const bool own = (hip_stream == MFMG_HIP_OWN_STREAM);
    c->handle.reset(new HipHandle(own ? nullptr : static_cast<hipStream_t>(hip_stream), own));
    *ctx = c;
  });
}

int mfmg_hip_context_destroy(mfmg_hip_context_t ctx)
{
  return guarded([&] { delete ctx; });
}

int mfmg_hip_context_synchronize(mfmg_hip_context_t ctx)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    MFMG_HIP_CHECK(hipStreamSynchronize(ctx->handle->stream));
  });
}

void *mfmg_hip_context_stream(mfmg_hip_context_t ctx) { return ctx ? ctx->handle->stream : nullptr; }

// ---- distributed runs -----------------------------------------------------------------
int mfmg_hip_context_set_communicator(mfmg_hip_context_t ctx, int32_t rank, int32_t n_ranks, int32_t ghost_cells_low,
                                      int32_t ghost_cells_high)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "rank out of range");
    require((ghost_cells_low == 0 || ghost_cells_low == 2 || ghost_cells_low == 4) && (ghost_cells_high == 0 || ghost_cells_high == 2),
            "ghost cell layers must be 0 or 2 (one agglomerate layer; 4 = two of them towards the lower neighbour)");
    require((ghost_cells_low > 0) == (rank > 0) && (ghost_cells_high == 2) == (rank + 1 < n_ranks),
            "ghost layers must be present exactly towards existing neighbours");
    HaloCommunicator &c = ctx->handle->comm;
    auto transport = c.transport;
    c = HaloCommunicator();
    c.transport = transport;
    c.rank = rank;
    c.n_ranks = n_ranks;
    c.ghost_cells_low = ghost_cells_low;
    c.ghost_cells_high = ghost_cells_high;
    c.grid[2] = n_ranks;
    c.coord[2] = rank;
    c.ghost_lo[2] = ghost_cells_low;
    c.ghost_hi[2] = ghost_cells_high;
  });
}

int mfmg_hip_context_set_communicator_box(mfmg_hip_context_t ctx, int32_t rank, const int32_t grid[3], const int32_t ghost_low[3],
                                          const int32_t ghost_high[3])
{
  return guarded([&] {
    require(ctx != nullptr && grid && ghost_low && ghost_high, "null argument");
    require(grid[0] >= 1 && grid[1] >= 1 && grid[2] >= 1, "the grid of ranks needs at least one rank per axis");
    const int n_ranks = grid[0] * grid[1] * grid[2];
    require(rank >= 0 && rank < n_ranks, "rank out of range");
    const int coord[3] = {rank % grid[0], (rank / grid[0]) % grid[1], rank / (grid[0] * grid[1])};
    for (int d = 0; d < 3; ++d)
    {
      require((ghost_low[d] == 0 || ghost_low[d] == 2 || ghost_low[d] == 4) && (ghost_high[d] == 0 || ghost_high[d] == 2),
              "ghost cell layers must be 0 or 2 (one agglomerate layer; 4 = two of them towards the lower neighbour)");
      require((ghost_low[d] > 0) == (coord[d] > 0) && (ghost_high[d] == 2) == (coord[d] + 1 < grid[d]),
              "ghost layers must be present exactly towards existing neighbours");
    }
    HaloCommunicator &c = ctx->handle->comm;
    auto transport = c.transport;
    c = HaloCommunicator();
    c.transport = transport;
    c.rank = rank;
    c.n_ranks = n_ranks;
    for (int d = 0; d < 3; ++d)
    {
      c.grid[d] = grid[d];
      c.coord[d] = coord[d];
      c.ghost_lo[d] = ghost_low[d];
      c.ghost_hi[d] = ghost_high[d];
    }
    c.ghost_cells_low = ghost_low[2];
    c.ghost_cells_high = ghost_high[2];
  });
}

int mfmg_hip_context_set_low_ghost_cells(mfmg_hip_context_t ctx, int32_t cells)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(cells == 2 || cells == 4, "ghost cell layers towards a lower neighbour: 2 or 4");
    HaloCommunicator &c = ctx->handle->comm;
    for (int d = 0; d < 3; ++d)
      require(c.ghost_lo[d] == 0 || c.ghost_lo[d] == cells, "the local mesh of this rank holds another number of ghost cell layers below");
    c.low_ghost_cells = cells;
  });
}

int mfmg_hip_context_set_block_fgmres_on_ranks(mfmg_hip_context_t ctx, int enable)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    ctx->handle->block_fgmres_on_ranks = enable != 0;
  });
}

int mfmg_hip_rccl_available(void)
{
  return guarded([&] { rccl_available(); });
}

int mfmg_hip_rccl_unique_id(unsigned char out[128])
{
  return guarded([&] {
    require(out != nullptr, "null output");
    rccl_unique_id(out);
  });
}

int mfmg_hip_context_use_rccl(mfmg_hip_context_t ctx, const unsigned char unique_id[128])
{
  return guarded([&] {
    require(ctx != nullptr && unique_id != nullptr, "null argument");
    HaloCommunicator &c = ctx->handle->comm;
    c.transport = make_rccl_transport(c.rank, c.n_ranks, unique_id);
    // the exchange stream gets its communicator HERE, where every rank is (ncclCommSplit is collective; created lazily it
    // would be created wherever a rank first overlaps an exchange)
    if (ctx->handle->comm_stream != nullptr)
      c.transport->bind_exchange_stream(ctx->handle->comm_stream);
    else
      (void)ctx->handle->exchange_stream();
  });
}

int mfmg_hip_context_use_host_transport(mfmg_hip_context_t ctx, mfmg_hip_host_exchange_fn exchange,
                                        mfmg_hip_host_allreduce_fn allreduce, mfmg_hip_host_allgather_fn allgather, void *user)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(exchange && allreduce && allgather, "null transport callbacks");
    HaloCommunicator &c = ctx->handle->comm;
    c.transport = make_host_transport(c.rank, c.n_ranks, exchange, allreduce, allgather, user);
  });
}

int mfmg_hip_context_use_reflecting_transport(mfmg_hip_context_t ctx)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    HaloCommunicator &c = ctx->handle->comm;
    require(c.enabled(), "no communicator was set");
    c.transport = make_reflecting_transport(c.n_ranks);
  });
}

int mfmg_hip_context_use_reflecting_transport_delay(mfmg_hip_context_t ctx, double microseconds_per_group)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(microseconds_per_group >= 0. && microseconds_per_group <= 1e4, "delay out of range");
    HaloCommunicator &c = ctx->handle->comm;
    require(c.enabled(), "no communicator was set");
    c.transport = make_reflecting_transport(c.n_ranks, microseconds_per_group);
  });
}

// `reps` loop-back groups (send to self + receive from self) of n doubles back to back on the context's stream, bracketed by
// one event pair: microseconds of stream time per group -- what a grouped send/recv costs before any byte crosses a wire
int mfmg_hip_context_transport_loopback_time(mfmg_hip_context_t ctx, int64_t n, int reps, double *microseconds)
{
  return guarded([&] {
    require(ctx != nullptr && microseconds != nullptr && n > 0 && reps > 0, "bad argument");
    HipHandle &h = *ctx->handle;
    require(h.comm.transport != nullptr, "no transport registered");
    DeviceBuffer<double> a((size_t)n), b((size_t)n);
    MFMG_HIP_CHECK(hipMemsetAsync(a.data(), 0, (size_t)n * sizeof(double), h.stream));
    for (int i = 0; i < 3; ++i)
      h.comm.transport->loopback(a.data(), b.data(), n, h.stream);
    hipEvent_t e0, e1;
    MFMG_HIP_CHECK(hipEventCreate(&e0));
    MFMG_HIP_CHECK(hipEventCreate(&e1));
    MFMG_HIP_CHECK(hipEventRecord(e0, h.stream));
    for (int i = 0; i < reps; ++i)
      h.comm.transport->loopback(a.data(), b.data(), n, h.stream);
    MFMG_HIP_CHECK(hipEventRecord(e1, h.stream));
    MFMG_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    MFMG_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *microseconds = 1e3 * ms / reps;
  });
}

int mfmg_hip_context_transport_name(mfmg_hip_context_t ctx, char *buffer, size_t buffer_size)
{
  return guarded([&] {
    require(ctx != nullptr && buffer != nullptr && buffer_size > 0, "null argument");
    std::string name = ctx->handle->comm.transport ? ctx->handle->comm.transport->name() : "";
    std::snprintf(buffer, buffer_size, "%s", name.c_str());
  });
}

int mfmg_hip_context_transport_ranks(mfmg_hip_context_t ctx, int *n_ranks)
{
  return guarded([&] {
    require(ctx != nullptr && n_ranks != nullptr, "null argument");
    *n_ranks = ctx->handle->comm.transport ? ctx->handle->comm.transport->comm_ranks() : 1;
  });
}

int mfmg_hip_context_transport_selftest(mfmg_hip_context_t ctx, int64_t n, double *max_error)
{
  return guarded([&] {
    require(ctx != nullptr && max_error != nullptr && n > 0, "bad argument");
    HipHandle &h = *ctx->handle;
    require(h.comm.transport != nullptr, "no transport registered");
    const int nr = h.comm.n_ranks, rk = h.comm.rank;
    std::vector<double> host((size_t)n);
    for (int64_t i = 0; i < n; ++i)
      host[i] = 1000. * rk + double(i % 977);
    DeviceBuffer<double> a((size_t)n), b((size_t)n), g((size_t)n * nr);
    MFMG_HIP_CHECK(hipMemcpyAsync(a.data(), host.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, h.stream));
    MFMG_HIP_CHECK(hipMemsetAsync(b.data(), 0, (size_t)n * sizeof(double), h.stream));
    double err = 0.;
    h.comm.transport->loopback(a.data(), b.data(), n, h.stream);
    std::vector<double> back = b.download(h.stream);
    for (int64_t i = 0; i < n; ++i)
      err = std::max(err, std::abs(back[i] - host[i]));
    h.comm.transport->allgather(a.data(), n, g.data(), h.stream);
    std::vector<double> all = g.download(h.stream);
    for (int r = 0; r < nr; ++r)
      for (int64_t i = 0; i < n; ++i)
        err = std::max(err, std::abs(all[(size_t)r * n + i] - (1000. * r + double(i % 977))));
    double v[2] = {double(rk + 1), double(rk + 1)};
    h.comm.transport->allreduce(v, 1, 0, h.stream);
    h.comm.transport->allreduce(v + 1, 1, 1, h.stream);
    err = std::max(err, std::abs(v[0] - 0.5 * nr * (nr + 1)));
    err = std::max(err, std::abs(v[1] - double(nr)));
    *max_error = err;
  });
}

int mfmg_hip_context_exchange_count(mfmg_hip_context_t ctx, int64_t *n_exchanges)
{
  return guarded([&] {
    require(ctx != nullptr && n_exchanges != nullptr, "null argument");
    *n_exchanges = ctx->handle->comm.n_exchanges;
  });
}

int mfmg_hip_context_exchange_volume(mfmg_hip_context_t ctx, int64_t *n_doubles_sent, int64_t *n_overlapped)
{
  return guarded([&] {
    require(ctx != nullptr && n_doubles_sent != nullptr, "null argument");
    *n_doubles_sent = ctx->handle->comm.n_doubles_sent;
    if (n_overlapped)
      *n_overlapped = ctx->handle->comm.n_overlapped;
  });
}

int mfmg_hip_context_exchange(mfmg_hip_context_t ctx, int32_t space, double *vector, int reverse)
{
  return guarded([&] {
    require(ctx != nullptr && vector != nullptr, "null argument");
    if (reverse)
      ctx->handle->exchange_reverse_add(space, vector);
    else
      ctx->handle->exchange(space, vector);
  });
}

// host only: the messages of a box exchange and where their entries lie in the local vector (halo_box_messages, halo_region_entry)
int mfmg_hip_halo_box_messages(const int64_t *local_nodes, const int64_t *own0, const int64_t *own_n, const int32_t *has_low,
                               const int32_t *has_high, int32_t comps, int32_t width, int32_t rank, const int32_t *grid,
                               int32_t *n_messages, int32_t *peers, int64_t *counts, int64_t *send_entries, int64_t *recv_entries,
                               int64_t capacity)
{
  return guarded([&] {
    require(local_nodes && own0 && own_n && has_low && has_high && grid && n_messages && peers && counts, "null argument");
    require(comps >= 1 && width >= 1, "bad space");
    HaloSpace s;
    s.comps = comps;
    s.width = width;
    for (int d = 0; d < 3; ++d)
      require(own0[d] >= 0 && own_n[d] >= width && own0[d] + own_n[d] <= local_nodes[d], "the owned box lies outside the local box");
    s.n_xy[0] = local_nodes[0];
    s.n_xy[1] = local_nodes[1];
    s.n_layers = local_nodes[2];
    s.layer_elems = comps * local_nodes[0] * local_nodes[1];
    for (int d = 0; d < 2; ++d)
    {
      s.own0_xy[d] = own0[d];
      s.own_n_xy[d] = own_n[d];
      s.low_xy[d] = has_low[d] != 0;
      s.high_xy[d] = has_high[d] != 0;
    }
    s.owned_begin = own0[2];
    s.owned_count = own_n[2];
    s.has_low = has_low[2] != 0;
    s.has_high = has_high[2] != 0;
    halo_check_width(s); // (the condition of every exchange: exchange_box, exchange_on, exchange_reverse_add)
    HaloRegions own, ghost;
    int p[26];
    int64_t c[26];
    const int stride[3] = {1, grid[0], grid[0] * grid[1]};
    const int64_t total = halo_box_messages(s, rank, stride, own, ghost, p, c);
    *n_messages = own.count;
    std::copy(p, p + own.count, peers);
    std::copy(c, c + own.count, counts);
    if (send_entries == nullptr && recv_entries == nullptr)
      return;
    require(send_entries && recv_entries && capacity >= total, "entry arrays shorter than the messages");
    for (int64_t i = 0; i < total; ++i)
    {
      send_entries[i] = halo_region_entry(own, comps, s.n_xy[0], s.n_xy[1], i);
      recv_entries[i] = halo_region_entry(ghost, comps, s.n_xy[0], s.n_xy[1], i);
    }
  });
}

int mfmg_hip_context_exchange_f32(mfmg_hip_context_t ctx, int32_t space, float *vector, int width)
{
  return guarded([&] {
    require(ctx != nullptr && vector != nullptr, "null argument");
    HipHandle &h = *ctx->handle;
    require(space == 1, "float vectors are exchanged in the fine DoF space (1) only");
    // (the same answer on every rank: every rank holds low_ghost_cells planes below and three above where it has a neighbour)
    require(width >= 1 && width <= 3 && width <= h.comm.low_ghost_cells, "width: 1 to 3 planes, at most the ghost planes every rank holds");
    if (!h.comm.enabled())
      return;
    (void)h.space_checked(space);
    h.exchange_on(h.fine_space(width), vector, h.stream, h.stream, false);
  });
}

int mfmg_hip_context_exchange_block(mfmg_hip_context_t ctx, int32_t space, int32_t n_vectors, int64_t ld, double *V, int width)
{
  return guarded([&] {
    require(ctx != nullptr && V != nullptr, "null argument");
    HipHandle &h = *ctx->handle;
    require(space == 1, "blocks of vectors are exchanged in the fine DoF space (1) only");
    // (the same answer on every rank, as for mfmg_hip_context_exchange_f32)
    require(width >= 1 && width <= 3 && width <= h.comm.low_ghost_cells, "width: 1 to 3 planes, at most the ghost planes every rank holds");
    // (the layout rules of the block entry points)
    require(n_vectors >= 1 && n_vectors <= MFMG_HIP_BLOCK_MAX_VECTORS, "a block holds 1 to 64 vectors");
    require(ld % 2 == 0, "the leading dimension of a block must be even (columns aligned to 16 bytes)");
    require(reinterpret_cast<uintptr_t>(V) % 16 == 0, "the base of a block must be aligned to 16 bytes");
    if (!h.comm.enabled())
      return;
    require(ld >= h.space_checked(space).n_local(), "the leading dimension of a block must be at least the vector size");
    h.reserve_exchange_block(n_vectors, width);
    h.exchange_block(n_vectors, ld, V, width);
  });
}

int mfmg_hip_context_exchange_block_f32(mfmg_hip_context_t ctx, int32_t space, int32_t n_vectors, int64_t ld, float *V, int width)
{
  return guarded([&] {
    require(ctx != nullptr && V != nullptr, "null argument");
    HipHandle &h = *ctx->handle;
    require(space == 1, "blocks of vectors are exchanged in the fine DoF space (1) only");
    // (the same answer on every rank, as for mfmg_hip_context_exchange_f32)
    require(width >= 1 && width <= 3 && width <= h.comm.low_ghost_cells, "width: 1 to 3 planes, at most the ghost planes every rank holds");
    // (the layout rules of the FP32 block entry points)
    require(n_vectors >= 1 && n_vectors <= MFMG_HIP_BLOCK_MAX_VECTORS, "a block holds 1 to 64 vectors");
    require(ld % 2 == 0, "the leading dimension of a block must be even (columns aligned to 8 bytes)");
    require(reinterpret_cast<uintptr_t>(V) % 8 == 0, "the base of a block must be aligned to 8 bytes");
    if (!h.comm.enabled())
      return;
    require(ld >= h.space_checked(space).n_local(), "the leading dimension of a block must be at least the vector size");
    h.reserve_exchange_block(n_vectors, width);
    h.exchange_block_f32(n_vectors, ld, V, width);
  });
}

int mfmg_hip_context_owned_dot(mfmg_hip_context_t ctx, int32_t space, const double *x, const double *y, double *result)
{
  return guarded([&] {
    require(ctx != nullptr && x && y && result, "null argument");
    HipHandle &h = *ctx->handle;
    require(space > 0 && space < (int)h.comm.spaces.size() && h.comm.spaces[space].configured(), "unknown vector space");
    DVector vx(h, h.comm.spaces[space].n_local(), const_cast<double *>(x)), vy(h, h.comm.spaces[space].n_local(), const_cast<double *>(y));
    *result = distributed_dot(h, space, vx, vy);
  });
}

int mfmg_hip_context_set_cell_constant_layout(mfmg_hip_context_t ctx, int enable)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    ctx->handle->allow_cell_constant = enable != 0;
  });
}
int mfmg_hip_context_set_stored_diagonal(mfmg_hip_context_t ctx, int enable)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    ctx->handle->stored_diagonal = enable != 0;
  });
}
int mfmg_hip_context_set_mf_fused_terms(mfmg_hip_context_t ctx, int n_terms)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(n_terms >= 1 && n_terms <= 3, "1, 2 or 3 terms per sweep");
    ctx->handle->mf_fused_terms = n_terms;
  });
}
int mfmg_hip_context_set_mf_shell(mfmg_hip_context_t ctx, int mode)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(mode >= 0 && mode <= 2, "shell mode: 0 beside the interior tiles, 1 after them, 2 slab by slab");
    ctx->handle->mf_shell_mode = mode;
  });
}
int mfmg_hip_context_set_mf_emulate_split(mfmg_hip_context_t ctx, int axes)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(axes >= 0 && axes <= 3, "emulated split: 0 off, 1 = z, 2 = yz, 3 = xyz");
    ctx->handle->mf_emulate_split = axes;
  });
}
int mfmg_hip_mf_laplace_diagonal_in_record(mfmg_hip_mf_laplace_t op, int *in_record)
{
  return guarded([&] {
    require(op && in_record, "null argument");
    *in_record = op->op->diagonal_in_record() ? 1 : 0;
  });
}
int mfmg_hip_mf_laplace_ids_computed(mfmg_hip_mf_laplace_t op, int *computed)
{
  return guarded([&] {
    require(op && computed, "null argument");
    *computed = op->op->ids_computed() ? 1 : 0;
  });
}
int mfmg_hip_context_set_galerkin_on_device(mfmg_hip_context_t ctx, int enable)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    ctx->handle->galerkin_on_device = enable != 0;
  });
}

int mfmg_hip_mf_laplace_cell_constant_layout(mfmg_hip_mf_laplace_t op, int *in_use)
{
  return guarded([&] {
    require(op && in_use, "null argument");
    *in_use = op->op->cell_constant_layout() ? 1 : 0;
  });
}

int mfmg_hip_mf_laplace_uniform_coefficient(mfmg_hip_mf_laplace_t op, int *uniform, int64_t *sweeps)
{
  return guarded([&] {
    require(op && uniform, "null argument");
    *uniform = op->op->uniform_coefficient() ? 1 : 0;
    if (sweeps)
      *sweeps = op->op->uniform_sweep_launches();
  });
}

int mfmg_hip_mf_laplace_f32_cell_constant_layout(mfmg_hip_mf_laplace_f32_t op, int *in_use)
{
  return guarded([&] {
    require(op && in_use, "null argument");
    *in_use = op->op->cell_constant_layout() ? 1 : 0;
  });
}

int mfmg_hip_mf_laplace_f32_ids_computed(mfmg_hip_mf_laplace_f32_t op, int *computed)
{
  return guarded([&] {
    require(op && computed, "null argument");
    *computed = op->op->ids_computed() ? 1 : 0;
  });
}

int mfmg_hip_context_set_overlap_exchange(mfmg_hip_context_t ctx, int enable)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    ctx->handle->overlap_exchange = enable != 0;
  });
}

int mfmg_hip_context_halo_layout(mfmg_hip_context_t ctx, int32_t space, int64_t *layer_elems, int64_t *n_layers,
                                 int64_t *owned_begin, int64_t *owned_count)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    require(space >= 1 && space < (int)ctx->handle->comm.spaces.size(), "unknown vector space");
    HaloSpace const &s = ctx->handle->comm.spaces[space];
    if (layer_elems)
      *layer_elems = s.layer_elems;
    if (n_layers)
      *n_layers = s.n_layers;
    if (owned_begin)
      *owned_begin = s.owned_begin;
    if (owned_count)
      *owned_count = s.owned_count;
  });
}

int mfmg_hip_context_halo_space(mfmg_hip_context_t ctx, int32_t space, int64_t out[8])
{
  return guarded([&] {
    require(ctx != nullptr && out != nullptr, "null argument");
    require(space >= 1 && space < (int)ctx->handle->comm.spaces.size(), "unknown vector space");
    HaloSpace const &s = ctx->handle->comm.spaces[space];
    out[0] = s.layer_elems;
    out[1] = s.n_layers;
    out[2] = s.owned_begin;
    out[3] = s.owned_count;
    out[4] = s.global_begin;
    out[5] = s.global_layers;
    out[6] = s.width;
    out[7] = (int64_t)ctx->handle->comm.spaces.size();
  });
}

int mfmg_hip_context_halo_box(mfmg_hip_context_t ctx, int32_t space, int64_t out[16])
{
  return guarded([&] {
    require(ctx != nullptr && out != nullptr, "null argument");
    require(space >= 1 && space < (int)ctx->handle->comm.spaces.size(), "unknown vector space");
    HaloSpace const &s = ctx->handle->comm.spaces[space];
    out[0] = s.comps;
    for (int d = 0; d < 3; ++d)
    {
      out[1 + d] = s.dim(d);
      out[4 + d] = s.own0(d);
      out[7 + d] = s.own_n(d);
      out[10 + d] = s.g0(d);
      out[13 + d] = s.gn(d);
    }
  });
}

int mfmg_hip_cell_contraction(mfmg_hip_context_t ctx, int fp32, int variant, int64_t n_cells, const void *u, const void *c,
                              void *v, const double cell_size[3])
{
  return guarded([&] {
    require(ctx != nullptr && u && c && v && cell_size, "null argument");
    if (fp32)
      cell_contraction<float>(*ctx->handle, variant, n_cells, static_cast<float const *>(u), static_cast<float const *>(c),
                              static_cast<float *>(v), cell_size);
    else
      cell_contraction<double>(*ctx->handle, variant, n_cells, static_cast<double const *>(u), static_cast<double const *>(c),
                               static_cast<double *>(v), cell_size);
  });
}

// ---- per-kernel HIP-event timing (bench.py roofline leg) ---------------------------
int mfmg_hip_profile_select(mfmg_hip_context_t ctx, const char *kernel_name)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    ctx->handle->profiler.only = kernel_name ? kernel_name : "";
  });
}

int mfmg_hip_profile_enable(mfmg_hip_context_t ctx, int enabled)
{
  return guarded([&] {
    require(ctx != nullptr, "null context");
    ctx->handle->profiler.enabled = enabled != 0;
    ctx->handle->profiler.reset();
  });
}

int mfmg_hip_profile_query(mfmg_hip_context_t ctx, const char *kernel_name, int64_t *n_launches, double *total_ms,
                           double *algorithmic_bytes)
{
  return guarded([&] {
    require(ctx && kernel_name, "null argument");
    int64_t n = 0;
    double ms = 0., bytes = 0.;
    ctx->handle->profiler.query(kernel_name, n, ms, bytes);
    if (n_launches)
      *n_launches = n;
    if (total_ms)
      *total_ms = ms;
    if (algorithmic_bytes)
      *algorithmic_bytes = bytes;
  });
}

// ---- marshalling ---------------------------------------------------------------
int mfmg_hip_malloc(void **dev_ptr, size_t bytes)
{
  return guarded([&] {
    require(dev_ptr != nullptr, "null output pointer");
    MFMG_HIP_CHECK(hipMalloc(dev_ptr, bytes));
  });
}
int mfmg_hip_free(void *dev_ptr)
{
  return guarded([&] { MFMG_HIP_CHECK(hipFree(dev_ptr)); });
}
int mfmg_hip_copy_to_dev(void *dst_dev, const void *src_host, size_t bytes)
{
  return guarded([&] { MFMG_HIP_CHECK(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice)); });
}
int mfmg_hip_copy_to_host(void *dst_host, const void *src_dev, size_t bytes)
{
  return guarded([&] { MFMG_HIP_CHECK(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost)); });
}

// ---- vector kernels ------------------------------------------------------------
int mfmg_hip_vector_set(mfmg_hip_context_t ctx, int64_t n, double value, double *x)
{
  return guarded([&] {
    require(ctx && x, "null argument");
    vec::set<double>(*ctx->handle, n, value, x);
  });
}
int mfmg_hip_vector_add(mfmg_hip_context_t ctx, int64_t n, double a, const double *v, double *x)
{
  return guarded([&] {
    require(ctx && x && v, "null argument");
    vec::add<double>(*ctx->handle, n, a, v, x);
  });
}
int mfmg_hip_vector_sadd(mfmg_hip_context_t ctx, int64_t n, double s, double a, const double *v, double *x)
{
  return guarded([&] {
    require(ctx && x && v, "null argument");
    vec::sadd<double>(*ctx->handle, n, s, a, v, x);
  });
}
int mfmg_hip_vector_dot(mfmg_hip_context_t ctx, int64_t n, const double *x, const double *y, double *result_host)
{
  return guarded([&] {
    require(ctx && x && y && result_host, "null argument");
    *result_host = vec::dot<double>(*ctx->handle, n, x, y);
  });
}
int mfmg_hip_vector_l2_norm(mfmg_hip_context_t ctx, int64_t n, const double *x, double *result_host)
{
  return guarded([&] {
    require(ctx && x && result_host, "null argument");
    *result_host = vec::l2_norm<double>(*ctx->handle, n, x);
  });
}

// ---- CSR -------------------------------------------------------------------------
int mfmg_hip_csr_create(mfmg_hip_context_t ctx, int64_t n_rows, int64_t n_cols, int64_t nnz,
                        const int32_t *row_ptr_host, const int32_t *col_host, const double *val_host,
                        mfmg_hip_csr_t *out)
{
  return guarded([&] {
    require(ctx && out && row_ptr_host, "null argument");
    require(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "negative size");
    require(nnz == 0 || (col_host && val_host), "null column / value array");
    std::vector<int32_t> rp(row_ptr_host, row_ptr_host + n_rows + 1);
    require(rp[n_rows] == nnz, "row_ptr[n_rows] != nnz");
    std::vector<int32_t> cl(col_host, col_host + nnz);
    std::vector<double> vl(val_host, val_host + nnz);
    auto m = std::make_shared<SparseMatrixDevice<double>>(*ctx->handle, n_rows, n_cols, std::move(rp), std::move(cl),
                                                          std::move(vl));
    auto h = new mfmg_hip_csr_s;
    h->op = std::make_shared<HipMatrixOperator>(m);
    *out = h;
  });
}

int mfmg_hip_csr_destroy(mfmg_hip_csr_t a)
{
  return guarded([&] {
    if (a && !a->borrowed)
      delete a;
  });
}

int mfmg_hip_csr_set_kernel(mfmg_hip_csr_t a, int lanes_per_row, int use_lds)
{
  return guarded([&] {
    require(a != nullptr, "null matrix");
    require(lanes_per_row >= 0 && (lanes_per_row <= 64 || lanes_per_row == 256) &&
                (lanes_per_row & (lanes_per_row - 1)) == 0,
            "lanes_per_row must be 0, a power of two up to 64, or 256 (a workgroup per row)");
    a->op->get_matrix()->set_kernel(lanes_per_row, use_lds);
  });
}
int mfmg_hip_csr_regular_rows(mfmg_hip_csr_t a, int *in_use)
{
  return guarded([&] {
    require(a && in_use, "null argument");
    *in_use = a->op->get_matrix()->regular_rows() ? 1 : 0;
  });
}
int mfmg_hip_csr_stencil_classes(mfmg_hip_csr_t a, int *n_classes, int64_t *listed_rows)
{
  return guarded([&] {
    require(a && n_classes && listed_rows, "null argument");
    *n_classes = a->op->get_matrix()->stencil_classes();
    *listed_rows = a->op->get_matrix()->listed_rows();
  });
}
int mfmg_hip_csr_float_storage(mfmg_hip_csr_t a, int *in_float)
{
  return guarded([&] {
    require(a && in_float, "null argument");
    auto op = a->op;
    // block-diagonal planes of the matrix, or -- for a restrictor with its agglomerate-wise form -- its planes
    *in_float = (op->get_matrix()->float_storage() || op->structured_float_planes()) ? 1 : 0;
  });
}
int mfmg_hip_csr_set_regular_rows(mfmg_hip_csr_t a, int enable)
{
  return guarded([&] {
    require(a != nullptr, "null matrix");
    a->op->get_matrix()->set_regular_rows(enable != 0);
  });
}
int mfmg_hip_csr_get_kernel(mfmg_hip_csr_t a, int *lanes_per_row, int *use_lds)
{
  return guarded([&] {
    require(a && lanes_per_row && use_lds, "null argument");
    *lanes_per_row = a->op->get_matrix()->lanes_per_row();
    *use_lds = a->op->get_matrix()->kernel_kind();
  });
}
int mfmg_hip_csr_shape(mfmg_hip_csr_t a, int64_t *n_rows, int64_t *n_cols, int64_t *nnz)
{
  return guarded([&] {
    require(a != nullptr, "null matrix");
    auto m = a->op->get_matrix();
    if (n_rows)
      *n_rows = m->m();
    if (n_cols)
      *n_cols = m->n();
    if (nnz)
      *nnz = m->n_nonzero_elements();
  });
}

// The node kernels gather the source vector two doubles at a time whatever its address (sparse_matrix_device.hip): a source
// at an 8-byte-only address would make those accesses misaligned for their type, so the entry points refuse it.
static void require_aligned_source(const double *x)
{
  require(reinterpret_cast<uintptr_t>(x) % 16 == 0, "the source vector of an SpMV must be 16-byte aligned");
}

int mfmg_hip_csr_vmult(mfmg_hip_csr_t a, const double *x, double *y)
{
  return guarded([&] {
    require(a && x && y, "null argument");
    require_aligned_source(x);
    a->op->get_matrix()->vmult(y, x);
  });
}

int mfmg_hip_csr_apply(mfmg_hip_csr_t a, const double *x, double *y, int mode)
{
  return guarded([&] {
    require(a && x && y, "null argument");
    require(mode == MFMG_HIP_NO_TRANS || mode == MFMG_HIP_TRANS, "unknown operator mode");
    require_aligned_source(x);
    if (mode == MFMG_HIP_NO_TRANS)
      a->op->get_matrix()->vmult(y, x);
    else
      a->op->get_transposed_matrix()->vmult(y, x);
  });
}

int mfmg_hip_csr_transpose(mfmg_hip_csr_t a, mfmg_hip_csr_t *out)
{
  return guarded([&] {
    require(a && out, "null argument");
    std::unique_ptr<mfmg_hip_csr_s> h(new mfmg_hip_csr_s); // (a released matrix throws below)
    h->op = std::dynamic_pointer_cast<HipMatrixOperator>(a->op->transpose());
    *out = h.release();
  });
}

int mfmg_hip_csr_multiply(mfmg_hip_csr_t a, mfmg_hip_csr_t b, mfmg_hip_csr_t *out)
{
  return guarded([&] {
    require(a && b && out, "null argument");
    std::unique_ptr<mfmg_hip_csr_s> h(new mfmg_hip_csr_s);
    h->op = std::dynamic_pointer_cast<HipMatrixOperator>(a->op->multiply(b->op));
    *out = h.release();
  });
}

int mfmg_hip_csr_download(mfmg_hip_csr_t a, int32_t *row_ptr_host, int32_t *col_host, double *val_host)
{
  return guarded([&] {
    require(a && row_ptr_host, "null argument");
    std::vector<int32_t> rp, cl;
    std::vector<double> vl;
    a->op->get_matrix()->download(rp, cl, vl);
    std::memcpy(row_ptr_host, rp.data(), rp.size() * sizeof(int32_t));
    if (!cl.empty())
    {
      require(col_host && val_host, "null column / value array");
      std::memcpy(col_host, cl.data(), cl.size() * sizeof(int32_t));
      std::memcpy(val_host, vl.data(), vl.size() * sizeof(double));
    }
  });
}

int mfmg_hip_csr_solve(mfmg_hip_csr_t a, const char *params_info, const double *b, double *x)
{
  return guarded([&] {
    require(a && b && x, "null argument");
    auto m = a->op->get_matrix();
    require(m->m() == m->n(), "the solver needs a square matrix");
    auto params = std::make_shared<ptree>(ptree::parse_info(params_info ? params_info : ""));
    HipSolver solver(m->handle(), a->op, params);
    DVector bv(m->handle(), m->m(), const_cast<double *>(b)), xv(m->handle(), m->m(), x);
    solver.apply(bv, xv);
    MFMG_HIP_CHECK(hipStreamSynchronize(m->handle().stream)); // (the solver and its factors go out of scope)
  });
}

int mfmg_hip_csr_inverse_diagonal(mfmg_hip_csr_t a, double *dinv)
{
  return guarded([&] {
    require(a && dinv, "null argument");
    a->op->get_matrix()->inverse_diagonal(dinv);
  });
}

int mfmg_hip_csr_smoother_step(mfmg_hip_csr_t a, const double *dinv, const double *b, const double *x,
                               const double *x_prev, double alpha, double beta, double *out)
{
  return guarded([&] {
    require(a && dinv && b && x && out, "null argument");
    auto m = a->op->get_matrix();
    require(m->m() == m->n(), "the smoother needs a square matrix");
    require_aligned_source(x);
    m->smoother_step(dinv, b, x, x_prev, alpha, beta, out);
  });
}

int mfmg_hip_csr_residual(mfmg_hip_csr_t a, const double *x, const double *b, double *res)
{
  return guarded([&] {
    require(a && x && b && res, "null argument");
    require_aligned_source(x);
    a->op->get_matrix()->residual(x, b, res);
  });
}

int mfmg_hip_csr_launch(mfmg_hip_csr_t a, int mode, const double *x, const double *b, const double *dinv, const double *x_prev,
                        double alpha, double beta, double *out)
{
  return guarded([&] {
    require(a && x && out, "null argument");
    require(mode >= MFMG_HIP_CSR_APPLY && mode <= MFMG_HIP_CSR_PLUS_SCALED, "unknown SpMV mode");
    require_aligned_source(x);
    a->op->get_matrix()->apply_mode(static_cast<CsrMode>(mode), x, b, dinv, x_prev, alpha, beta, out);
  });
}

int mfmg_hip_csr_launch_block(mfmg_hip_csr_t a, int mode, int32_t n_vectors, int64_t ld_x, const double *x, int64_t ld_out, const double *b,
                              const double *dinv, const double *x_prev, double alpha, double beta, double *out)
{
  return guarded([&] {
    require(a && x && out, "null argument");
    require(mode >= MFMG_HIP_CSR_APPLY && mode <= MFMG_HIP_CSR_PLUS_SCALED, "unknown SpMV mode");
    auto m = a->op->get_matrix();
    // (the rules of the other block entry points, and the operands apply_mode asks for, refused as invalid arguments)
    require(n_vectors >= 1 && n_vectors <= MFMG_HIP_BLOCK_MAX_VECTORS, "a block holds 1 to 64 vectors");
    require(ld_x >= m->n() && ld_out >= m->m(), "the leading dimension of a block must be at least the vector size");
    require(ld_x % 2 == 0 && ld_out % 2 == 0, "the leading dimension of a block must be even (columns aligned to 16 bytes)");
    const bool smoother = mode == MFMG_HIP_CSR_FIRST || mode == MFMG_HIP_CSR_NEXT;
    const bool need_b = smoother || mode == MFMG_HIP_CSR_RESIDUAL || mode == MFMG_HIP_CSR_PLUS_SCALED,
               need_dinv = smoother || mode == MFMG_HIP_CSR_PLUS_SCALED, need_prev = mode == MFMG_HIP_CSR_NEXT;
    require(!need_b || b, "this SpMV mode needs b");
    require(!need_dinv || dinv, "this SpMV mode needs the inverse diagonal");
    require(!need_prev || x_prev, "this SpMV mode needs x_prev");
    require(!smoother || m->m() == m->n(), "the smoother needs a square matrix");
    auto aligned = [](const double *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    require(aligned(x) && aligned(out) && (!need_b || aligned(b)) && (!need_dinv || aligned(dinv)) && (!need_prev || aligned(x_prev)),
            "the base of a block must be aligned to 16 bytes");
    const double *x_end = x + (size_t)(n_vectors - 1) * ld_x + m->n(), *out_end = out + (size_t)(n_vectors - 1) * ld_out + m->m();
    require(x_end <= out || out_end <= x, "the blocks x and out overlap");
    m->apply_mode_block(static_cast<CsrMode>(mode), n_vectors, x, ld_x, b, dinv, x_prev, alpha, beta, out, ld_out);
  });
}

int mfmg_hip_csr_block_info(mfmg_hip_csr_t a, int64_t fields[3])
{
  return guarded([&] {
    require(a && fields, "null argument");
    auto m = a->op->get_matrix();
    fields[0] = m->block_width();
    m->block_counters(fields[1], fields[2]);
  });
}

int mfmg_hip_csr_set_block_csr(mfmg_hip_csr_t a, int on, int32_t info[3])
{
  return guarded([&] {
    require(a && info, "null argument");
    auto m = a->op->get_matrix();
    m->set_block_csr(on != 0);
    info[0] = m->block_width();
    info[1] = m->block_csr_route(4);
    info[2] = m->block_csr_route(2);
  });
}

int mfmg_hip_csr_block_csr_info_f32(mfmg_hip_context_t ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *row_ptr_host,
                                    const int32_t *col_host, const double *val_host, int32_t info[3])
{
  return guarded([&] {
    require(ctx && row_ptr_host && info, "null argument");
    require(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "negative size");
    require(nnz == 0 || (col_host && val_host), "null column / value array");
    std::vector<int32_t> rp(row_ptr_host, row_ptr_host + n_rows + 1);
    require(rp[n_rows] == nnz, "row_ptr[n_rows] != nnz");
    std::vector<int32_t> cl(col_host, col_host + nnz);
    std::vector<float> vl(val_host, val_host + nnz);
    SparseMatrixDevice<float> m(*ctx->handle, n_rows, n_cols, std::move(rp), std::move(cl), std::move(vl));
    m.set_block_csr(true);
    info[0] = m.block_width();
    info[1] = m.block_csr_route(4);
    info[2] = m.block_csr_route(2);
  });
}

int mfmg_hip_csr_form(mfmg_hip_csr_t a, int64_t *fields, int32_t n)
{
  return guarded([&] {
    require(a && fields, "null argument");
    require(n >= 22, "csr_form needs 22 fields at least (MFMG_HIP_CSR_FORM_FIELDS for all of them)");
    std::fill(fields, fields + n, (int64_t)0);
    const CsrForm f = a->op->get_matrix()->form();
    fields[0] = f.kind;
    fields[1] = f.csr_kernel;
    fields[2] = f.lanes;
    fields[3] = f.c;
    fields[4] = f.stored_d;
    fields[5] = f.full_d;
    fields[6] = f.symmetric_half;
    fields[7] = f.float_planes;
    fields[8] = f.regular;
    fields[9] = f.all_in_classes;
    fields[10] = f.classes;
    fields[11] = f.class_slots;
    fields[12] = f.listed;
    fields[13] = f.listed_route;
    fields[14] = f.regular_kernel;
    fields[15] = f.class_kernel;
    fields[16] = f.stored_kernel;
    fields[17] = f.row_base_slots;
    fields[18] = f.node_class_c;
    fields[19] = f.node_class_d;
    fields[20] = f.pairs;
    fields[21] = f.csr_released;
    if (n >= MFMG_HIP_CSR_FORM_FIELDS)
    {
      fields[22] = f.twin_kernel;
      fields[23] = f.twin_slots;
      fields[24] = f.twin_classes;
      fields[25] = f.single_slots;
      fields[26] = f.twin_wide;
    }
  });
}

int mfmg_hip_csr_enable_node_twins(mfmg_hip_csr_t a, int *taken)
{
  return guarded([&] {
    require(a && taken, "null argument");
    *taken = a->op->get_matrix()->enable_node_twins() ? 1 : 0;
  });
}

int mfmg_hip_csr_release_csr(mfmg_hip_csr_t a, int *released)
{
  return guarded([&] {
    require(a && released, "null argument");
    *released = a->op->get_matrix()->release_csr() ? 1 : 0;
  });
}

// ---- matrix-free Laplace -----------------------------------------------------------
int mfmg_hip_mf_laplace_create(mfmg_hip_context_t ctx, const mfmg_hip_mesh_desc *mesh, mfmg_hip_mf_laplace_t *out)
{
  return guarded([&] {
    require(ctx && mesh && out, "null argument");
    auto h = new mfmg_hip_mf_laplace_s;
    try
    {
      h->op = std::make_shared<MatrixFreeLaplaceDevice<double>>(*ctx->handle, *mesh, ctx->handle->allow_cell_constant);
    }
    catch (...)
    {
      delete h;
      throw;
    }
    *out = h;
  });
}

int mfmg_hip_mf_laplace_destroy(mfmg_hip_mf_laplace_t op)
{
  return guarded([&] { delete op; });
}

int mfmg_hip_mf_laplace_size(mfmg_hip_mf_laplace_t op, int64_t *n_dofs)
{
  return guarded([&] {
    require(op && n_dofs, "null argument");
    *n_dofs = op->op->n_dofs();
  });
}

int mfmg_hip_mf_laplace_vmult(mfmg_hip_mf_laplace_t op, const double *x, double *y)
{
  return guarded([&] {
    require(op && x && y, "null argument");
    op->op->vmult(x, y);
  });
}

int mfmg_hip_mf_laplace_diagonal_inverse(mfmg_hip_mf_laplace_t op, double *dinv)
{
  return guarded([&] {
    require(op && dinv, "null argument");
    vec::copy<double>(op->op->handle(), op->op->n_dofs(), op->op->diagonal_inverse(), dinv);
  });
}

int mfmg_hip_mf_laplace_diagonal(mfmg_hip_mf_laplace_t op, double *diag)
{
  return guarded([&] {
    require(op && diag, "null argument");
    vec::copy<double>(op->op->handle(), op->op->n_dofs(), op->op->diagonal(), diag);
  });
}

int mfmg_hip_mf_laplace_residual(mfmg_hip_mf_laplace_t op, const double *x, const double *b, double *res)
{
  return guarded([&] {
    require(op && x && b && res, "null argument");
    op->op->residual(x, b, res);
  });
}

int mfmg_hip_mf_laplace_smoother_step(mfmg_hip_mf_laplace_t op, const double *b, const double *x,
                                      const double *x_prev, double alpha, double beta, double *out)
{
  return guarded([&] {
    require(op && b && x && out, "null argument");
    op->op->smoother_step(b, x, x_prev, alpha, beta, out);
  });
}

// ---- blocks of vectors ----
int mfmg_hip_block_groups(int32_t n_vectors, int32_t *widths, int32_t *n_groups)
{
  return guarded([&] {
    require(widths && n_groups, "null argument");
    int w[kMfBlockMaxGroups];
    const int n = mf_block_groups(n_vectors, w);
    for (int g = 0; g < n; ++g)
      widths[g] = w[g];
    *n_groups = n;
  });
}

int mfmg_hip_mf_z_tiles(int32_t n_layers, int32_t tz, int graded, int32_t *starts, int32_t capacity, int32_t *n_tiles)
{
  return guarded([&] {
    require(starts && n_tiles, "null argument");
    require(n_layers >= 1 && tz >= 1, "z-tiling: at least one layer and a tile height of at least 1");
    const std::vector<int> tab = mf_z_tiles(n_layers, tz, graded != 0);
    require((int64_t)capacity >= (int64_t)tab.size(), "z-tiling: `starts` holds n_tiles + 1 entries");
    for (size_t t = 0; t < tab.size(); ++t)
      starts[t] = tab[t];
    *n_tiles = (int32_t)tab.size() - 1;
  });
}

int mfmg_hip_mf_laplace_block_launch(mfmg_hip_mf_laplace_t op, int mode, int32_t n_vectors, int64_t ld, const double *x, const double *b,
                                     const double *x_prev, double alpha, double beta, double *out)
{
  return guarded([&] {
    require(op != nullptr, "null argument");
    require(mode >= 0 && mode <= 3, "mode: 0 out = A x, 1 out = A x - b, 2 / 3 a smoother term without / with x_prev");
    op->op->launch_block(static_cast<MfMode>(mode), {x, b, x_prev, out, ld, n_vectors, alpha, beta});
  });
}

int mfmg_hip_mf_laplace_block_available(mfmg_hip_mf_laplace_t op, int *available)
{
  return guarded([&] {
    require(op && available, "null argument");
    *available = op->op->block_kernel_available() ? 1 : 0;
  });
}

int mfmg_hip_mf_laplace_set_block_tile(mfmg_hip_mf_laplace_t op, int n_waves, int tile_y, int tile_z)
{
  return guarded([&] {
    require(op != nullptr, "null argument");
    require((n_waves == 0 && tile_y == 0 && tile_z == 0) || (n_waves >= 1 && n_waves <= 8 && tile_y >= 2 && tile_y <= 4 && tile_z >= 1),
            "block tile: 1..8 wavefronts of 2..4 cell rows, at least one layer (0, 0, 0: chosen from the mesh)");
    op->op->set_block_tile(n_waves, tile_y, tile_z);
  });
}

int mfmg_hip_mf_laplace_get_block_tile(mfmg_hip_mf_laplace_t op, int n_vectors, int *n_waves, int *tile_y, int *tile_z)
{
  return guarded([&] {
    require(op && n_waves && tile_y && tile_z, "null argument");
    op->op->get_block_tile(n_vectors, *n_waves, *tile_y, *tile_z);
  });
}

int mfmg_hip_mf_laplace_sweep_available(mfmg_hip_mf_laplace_t op, int n_terms, int *available)
{
  return guarded([&] {
    require(op && available, "null argument");
    *available = op->op->fused_sweep_available(n_terms) ? 1 : 0;
  });
}
int mfmg_hip_mf_laplace_smoother_sweep(mfmg_hip_mf_laplace_t op, int n_terms, const double *alpha, const double *beta,
                                       const double *b, const double *x, double *out, double *out_prev)
{
  return guarded([&] {
    require(op && alpha && beta && b && out, "null argument");
    if (!op->op->fused_sweep_available(n_terms))
      ASSERT_THROW_NOT_IMPLEMENTED("the multi-term smoother sweep is not available for this operator");
    // x == NULL: the sweep from x_0 = 0, which is then not read (three terms, default arithmetic)
    if (x == nullptr && !op->op->fused_zero_guess_available(n_terms))
      ASSERT_THROW_NOT_IMPLEMENTED("the sweep from a zero guess is not available for this operator / tile / number of terms");
    op->op->smoother_sweep(n_terms, alpha, beta, b, x, out, out_prev);
  });
}
int mfmg_hip_mf_laplace_set_sweep_reference(mfmg_hip_mf_laplace_t op, int on)
{
  return guarded([&] {
    require(op != nullptr, "null operator");
    op->op->set_fused_reference(on != 0);
  });
}
int mfmg_hip_mf_laplace_f32_set_sweep_reference(mfmg_hip_mf_laplace_f32_t op, int on)
{
  return guarded([&] {
    require(op != nullptr, "null operator");
    op->op->set_fused_reference(on != 0);
  });
}
int mfmg_hip_mf_laplace_set_sweep_diagonal(mfmg_hip_mf_laplace_t op, int stored)
{
  return guarded([&] {
    require(op != nullptr, "null operator");
    if (stored != 0 && op->op->sweep_diagonal_inverse() == nullptr)
      ASSERT_THROW_NOT_IMPLEMENTED("this operator holds no D^-1 vector of the sweep");
    op->op->set_sweep_diagonal(stored != 0);
  });
}
int mfmg_hip_mf_laplace_get_sweep_diagonal(mfmg_hip_mf_laplace_t op, int *stored)
{
  return guarded([&] {
    require(op && stored, "null argument");
    *stored = op->op->sweep_diagonal_stored() ? 1 : 0;
  });
}
int mfmg_hip_mf_laplace_sweep_diagonal_inverse(mfmg_hip_mf_laplace_t op, double *dinv)
{
  return guarded([&] {
    require(op && dinv, "null argument");
    if (op->op->sweep_diagonal_inverse() == nullptr)
      ASSERT_THROW_NOT_IMPLEMENTED("this operator holds no D^-1 vector of the sweep");
    vec::copy<double>(op->op->handle(), op->op->n_dofs(), op->op->sweep_diagonal_inverse(), dinv);
  });
}
int mfmg_hip_mf_laplace_set_sweep_tile(mfmg_hip_mf_laplace_t op, int n_waves, int tile_y, int tile_z)
{
  return guarded([&] {
    require(op != nullptr, "null operator");
    require(((n_waves >= 0 && n_waves <= 8) || (n_waves == 12 && tile_y == 2)) && tile_y >= 0 && tile_y <= 4 && tile_z >= 0 && tile_z <= 4096,
            "sweep tile out of range");
    op->op->set_fused_tile(n_waves, tile_y, tile_z);
  });
}
int mfmg_hip_mf_laplace_get_sweep_tile(mfmg_hip_mf_laplace_t op, int n_terms, int *n_waves, int *tile_y, int *tile_z)
{
  return guarded([&] {
    require(op && n_waves && tile_y && tile_z, "null argument");
    op->op->get_fused_tile(n_terms, *n_waves, *tile_y, *tile_z);
  });
}

// ---- FP32 instance ----------------------------------------------------------------------
int mfmg_hip_mf_laplace_f32_create(mfmg_hip_context_t ctx, const mfmg_hip_mesh_desc *mesh, mfmg_hip_mf_laplace_f32_t *out)
{
  return guarded([&] {
    require(ctx && mesh && out, "null argument");
    std::unique_ptr<mfmg_hip_mf_laplace_f32_s> h(new mfmg_hip_mf_laplace_f32_s);
    h->op = std::make_shared<MatrixFreeLaplaceDevice<float>>(*ctx->handle, *mesh, ctx->handle->allow_cell_constant);
    *out = h.release();
  });
}
int mfmg_hip_mf_laplace_f32_destroy(mfmg_hip_mf_laplace_f32_t op)
{
  return guarded([&] { delete op; });
}
int mfmg_hip_mf_laplace_f32_vmult(mfmg_hip_mf_laplace_f32_t op, const float *x, float *y)
{
  return guarded([&] {
    require(op && x && y, "null argument");
    op->op->vmult(x, y);
  });
}
int mfmg_hip_mf_laplace_f32_diagonal_inverse(mfmg_hip_mf_laplace_f32_t op, float *dinv)
{
  return guarded([&] {
    require(op && dinv, "null argument");
    vec::copy<float>(op->op->handle(), op->op->n_dofs(), op->op->diagonal_inverse(), dinv);
  });
}
int mfmg_hip_mf_laplace_f32_residual(mfmg_hip_mf_laplace_f32_t op, const float *x, const float *b, float *res)
{
  return guarded([&] {
    require(op && x && b && res, "null argument");
    op->op->residual(x, b, res);
  });
}
int mfmg_hip_mf_laplace_f32_smoother_step(mfmg_hip_mf_laplace_f32_t op, const float *b, const float *x,
                                          const float *x_prev, float alpha, float beta, float *out)
{
  return guarded([&] {
    require(op && b && x && out, "null argument");
    op->op->smoother_step(b, x, x_prev, alpha, beta, out);
  });
}

int mfmg_hip_mf_laplace_f32_sweep_available(mfmg_hip_mf_laplace_f32_t op, int n_terms, int *available)
{
  return guarded([&] {
    require(op && available, "null argument");
    *available = op->op->fused_sweep_available(n_terms) ? 1 : 0;
  });
}
int mfmg_hip_mf_laplace_f32_smoother_sweep(mfmg_hip_mf_laplace_f32_t op, int n_terms, const float *alpha, const float *beta,
                                           const float *b, const float *x, float *out, float *out_prev)
{
  return guarded([&] {
    require(op && alpha && beta && b && x && out, "null argument");
    if (!op->op->fused_sweep_available(n_terms))
      ASSERT_THROW_NOT_IMPLEMENTED("the multi-term smoother sweep is not available for this operator");
    op->op->smoother_sweep(n_terms, alpha, beta, b, x, out, out_prev);
  });
}

// the tiles of the FP32 instance: the entry points of the FP64 one, same ranges
int mfmg_hip_mf_laplace_f32_get_tile(mfmg_hip_mf_laplace_f32_t op, int *n_waves, int *tile_y, int *tile_z)
{
  return guarded([&] {
    require(op && n_waves && tile_y && tile_z, "null argument");
    op->op->get_tile(*n_waves, *tile_y, *tile_z);
  });
}
int mfmg_hip_mf_laplace_f32_set_tile_waves(mfmg_hip_mf_laplace_f32_t op, int n_waves)
{
  return guarded([&] {
    require(op != nullptr, "null operator");
    require(n_waves >= 0 && n_waves <= 8, "0..8 wavefronts per workgroup");
    op->op->set_tile_waves(n_waves);
  });
}
int mfmg_hip_mf_laplace_f32_set_tile(mfmg_hip_mf_laplace_f32_t op, int tile_y, int tile_z)
{
  return guarded([&] {
    require(op != nullptr, "null argument");
    require(tile_y >= 0 && tile_z >= 0 && tile_y <= 64 && tile_z <= 1024, "tile size out of range");
    op->op->set_tile(tile_y, tile_z);
  });
}
int mfmg_hip_mf_laplace_f32_set_sweep_tile(mfmg_hip_mf_laplace_f32_t op, int n_waves, int tile_y, int tile_z)
{
  return guarded([&] {
    require(op != nullptr, "null operator");
    require(((n_waves >= 0 && n_waves <= 8) || (n_waves == 12 && tile_y == 2)) && tile_y >= 0 && tile_y <= 4 && tile_z >= 0 && tile_z <= 4096,
            "sweep tile out of range");
    op->op->set_fused_tile(n_waves, tile_y, tile_z);
  });
}
int mfmg_hip_mf_laplace_f32_get_sweep_tile(mfmg_hip_mf_laplace_f32_t op, int n_terms, int *n_waves, int *tile_y, int *tile_z)
{
  return guarded([&] {
    require(op && n_waves && tile_y && tile_z, "null argument");
    op->op->get_fused_tile(n_terms, *n_waves, *tile_y, *tile_z);
  });
}
int mfmg_hip_mf_laplace_f32_diagonal_in_record(mfmg_hip_mf_laplace_f32_t op, int *in_record)
{
  return guarded([&] {
    require(op && in_record, "null argument");
    *in_record = op->op->diagonal_in_record() ? 1 : 0;
  });
}

// ---- blocks of float vectors ----
int mfmg_hip_mf_laplace_f32_block_launch(mfmg_hip_mf_laplace_f32_t op, int mode, int32_t n_vectors, int64_t ld, const float *x, const float *b,
                                         const float *x_prev, float alpha, float beta, float *out)
{
  return guarded([&] {
    require(op != nullptr, "null argument");
    require(mode >= 0 && mode <= 3, "mode: 0 out = A x, 1 out = A x - b, 2 / 3 a smoother term without / with x_prev");
    op->op->launch_block(static_cast<MfMode>(mode), {x, b, x_prev, out, ld, n_vectors, alpha, beta});
  });
}

int mfmg_hip_mf_laplace_f32_block_available(mfmg_hip_mf_laplace_f32_t op, int *available)
{
  return guarded([&] {
    require(op && available, "null argument");
    *available = op->op->block_kernel_available() ? 1 : 0;
  });
}

int mfmg_hip_mf_laplace_f32_set_block_tile(mfmg_hip_mf_laplace_f32_t op, int n_waves, int tile_y, int tile_z)
{
  return guarded([&] {
    require(op != nullptr, "null argument");
    require((n_waves == 0 && tile_y == 0 && tile_z == 0) || (n_waves >= 1 && n_waves <= 8 && tile_y >= 2 && tile_y <= 4 && tile_z >= 1),
            "block tile: 1..8 wavefronts of 2..4 cell rows, at least one layer (0, 0, 0: chosen from the mesh)");
    op->op->set_block_tile(n_waves, tile_y, tile_z);
  });
}

int mfmg_hip_mf_laplace_f32_get_block_tile(mfmg_hip_mf_laplace_f32_t op, int n_vectors, int *n_waves, int *tile_y, int *tile_z)
{
  return guarded([&] {
    require(op && n_waves && tile_y && tile_z, "null argument");
    op->op->get_block_tile(n_vectors, *n_waves, *tile_y, *tile_z);
  });
}

int mfmg_hip_mf_laplace_get_tile(mfmg_hip_mf_laplace_t op, int *n_waves, int *tile_y, int *tile_z)
{
  return guarded([&] {
    require(op && n_waves && tile_y && tile_z, "null argument");
    op->op->get_tile(*n_waves, *tile_y, *tile_z);
  });
}
int mfmg_hip_mf_laplace_set_tile_waves(mfmg_hip_mf_laplace_t op, int n_waves)
{
  return guarded([&] {
    require(op != nullptr, "null operator");
    require(n_waves >= 0 && n_waves <= 8, "0..8 wavefronts per workgroup");
    op->op->set_tile_waves(n_waves);
  });
}
int mfmg_hip_mf_laplace_set_tile(mfmg_hip_mf_laplace_t op, int tile_y, int tile_z)
{
  return guarded([&] {
    require(op != nullptr, "null argument");
    require(tile_y >= 0 && tile_z >= 0 && tile_y <= 64 && tile_z <= 1024, "tile size out of range");
    op->op->set_tile(tile_y, tile_z);
  });
}

// ---- hierarchy -----------------------------------------------------------------------
int mfmg_hip_hierarchy_create(mfmg_hip_context_t ctx, const char *evaluator_type, const mfmg_hip_mesh_desc *mesh,
                              const char *params_info, mfmg_hip_hierarchy_t *out)
{
  return guarded([&] {
    require(ctx && evaluator_type && mesh && out, "null argument");
    auto params = std::make_shared<ptree>(ptree::parse_info(params_info ? params_info : ""));
    std::unique_ptr<mfmg_hip_hierarchy_s> h(new mfmg_hip_hierarchy_s);
    h->handle = ctx->handle.get();
    std::string type(evaluator_type);
    // "internal numbering" lexicographic: evaluator, hierarchy and FP32 fine level are built from the mesh in the lexicographic
    // numbering of its nodes (dof_permutation.hpp); a caller's numbering that is lexicographic already changes nothing
    const std::string numbering = params->get("internal numbering", "caller");
    if (numbering == "lexicographic")
    {
      require(type == "HipMatrixFreeMeshEvaluator", "\"internal numbering\" lexicographic needs the matrix-free evaluator");
      require(!ctx->handle->comm.enabled(), "\"internal numbering\" lexicographic is not available in a distributed run (the local "
                                            "numbering of a rank is the library's own)");
      h->lexicographic = true;
      h->perm.reset(new DofPermutation(*ctx->handle, *mesh));
      if (h->perm->identity())
        h->perm.reset();
      else
        mesh = &h->perm->lexicographic_mesh();
    }
    else
      require(numbering == "caller", "\"internal numbering\" must be caller or lexicographic");
    if (type == "HipMatrixFreeMeshEvaluator")
      h->evaluator = std::make_shared<HipMatrixFreeMeshEvaluator>(*ctx->handle, *mesh);
    else if (type == "HipMeshEvaluator")
      h->evaluator = std::make_shared<HipMeshEvaluator>(*ctx->handle, *mesh);
    else
      ASSERT_THROW_NOT_IMPLEMENTED("mesh evaluator type \"" + type + "\" is not available in the HIP build");
    h->timer = std::make_shared<TimerOutput>();
    {
      // "setup value precision" reaches the probing kernels through the handle (HipHierarchyHelpers::build_restrictor sets it):
      // it must not outlive this setup, or the next hierarchy / user-built operator of the context inherits it
      struct Restore
      {
        HipHandle &hd;
        bool &keep;
        ~Restore()
        {
          keep = hd.setup_values_float;
          hd.setup_values_float = false;
          hd.setup_caller_ids = nullptr;
        }
      } restore{*ctx->handle, h->setup_values_float};
      ctx->handle->setup_values_float = false;
      // what the setup keys on a DoF id takes the caller's id of the node (HipSmoother::estimate_eigenvalues)
      ctx->handle->setup_caller_ids = h->perm ? h->perm->node_dof_host().data() : nullptr;
      h->hierarchy.reset(new Hierarchy<DVector>(nullptr, h->evaluator, params, h->timer));
      std::copy(ctx->handle->restrictor_eigensolver_info, ctx->handle->restrictor_eigensolver_info + MFMG_HIP_EIGENSOLVER_INFO_FIELDS,
                h->eigensolver_info);
      h->eigensolver_seconds = ctx->handle->restrictor_eigensolver_seconds;
    }
    // "release setup matrices" true: once the hierarchy stands, the table-driven operators (A_c, the operators of the aggregation
    // levels) free their CSR arrays -- 12 B per entry that only the setup algebra and the exports (get_coarse_operator, the
    // level matrices) read: those calls throw afterwards.  One rank.
    if (params->get("release setup matrices", false))
    {
      require(!ctx->handle->comm.enabled(), "\"release setup matrices\" is not available in a distributed run");
      auto const &lv = h->hierarchy->levels();
      for (size_t l = 1; l < lv.size(); ++l)
        if (auto op = std::dynamic_pointer_cast<HipMatrixOperator const>(lv[l].get_operator()))
          op->get_matrix()->release_csr();
      if (auto solver = std::dynamic_pointer_cast<HipSolver const>(lv.back().get_solver()))
        std::const_pointer_cast<HipSolver>(solver)->release_setup_matrices();
    }
    const std::string precision = params->get("fine level precision", "double");
    if (precision == "float")
    {
      // built here: the mesh arrays of the caller need not outlive this call
      require(type == "HipMatrixFreeMeshEvaluator", "\"fine level precision\" float needs the matrix-free evaluator");
      require(h->hierarchy->levels().size() == 2, "\"fine level precision\" float needs the two-level hierarchy");
      h->fine_f32.reset(new HipFloatFineLevel(*ctx->handle, *mesh, *h->hierarchy));
    }
    else
      require(precision == "double", "\"fine level precision\" must be double or float");
    MFMG_HIP_CHECK(hipStreamSynchronize(ctx->handle->stream));
    if (h->perm)
      h->perm->release_mesh();
    *out = h.release();
  });
}

int mfmg_hip_hierarchy_destroy(mfmg_hip_hierarchy_t h)
{
  return guarded([&] { delete h; });
}

namespace
{
// Hierarchy::apply on vectors in the caller's numbering while the hierarchy runs in the lexicographic one: ONE launch gathers b
// -- and x, unless the cycle starts from zero and never reads it --, and the copy into x that ends the cycle is the scatter
void apply_permuted(mfmg_hip_hierarchy_t h, const double *b, double *x)
{
  const int64_t n = level_size(h, 0);
  double *wb = h->workspace(0), *wx = h->workspace(1);
  if (h->hierarchy->is_preconditioner())
    h->perm->gather(b, wb);
  else
    h->perm->gather2(b, static_cast<double const *>(x), wb, wx);
  DVector bv(*h->handle, n, wb), xv(*h->handle, n, wx);
  const Hierarchy<DVector>::Deliver deliver = [&](DVector const &result) { h->perm->scatter(result.get_values(), x); };
  h->hierarchy->apply(bv, xv, 0, &deliver);
}
} // namespace

int mfmg_hip_hierarchy_apply(mfmg_hip_hierarchy_t h, const double *b, double *x)
{
  return guarded([&] {
    require(h && b && x, "null argument");
    if (h->perm)
      return apply_permuted(h, b, x);
    const int64_t n = level_size(h, 0);
    DVector bv(*h->handle, n, const_cast<double *>(b)), xv(*h->handle, n, x);
    h->hierarchy->apply(bv, xv);
  });
}

namespace
{
// (on_ranks: the entry point runs on a context with a communicator -- the cycle, the smoother, the operator and CG; block FGMRES
// does not)
// Block transfers of the restrictor of `level` so far: launches of the block restriction and of the block prolongation, columns
// whose transfers went through the one-vector kernels (those of the cycles of apply_block count for level 1)
void transfer_counters(mfmg_hip_hierarchy_t h, int level, int64_t counters[3])
{
  counters[0] = counters[1] = counters[2] = 0;
  if (level < 1 || level >= (int)h->hierarchy->levels().size())
    return;
  if (auto r = std::dynamic_pointer_cast<HipMatrixOperator const>(h->hierarchy->levels()[level].get_restrictor()))
    r->transfer_block_counters(counters);
  if (level == 1)
    counters[2] += h->hierarchy->transfer_columns_looped();
}

// a block call begins: mfmg_hip_hierarchy_transfer_block_info reports what happened since
void begin_block_call(mfmg_hip_hierarchy_t h)
{
  h->transfer_snapshot.resize(h->hierarchy->levels().size());
  for (size_t level = 0; level < h->transfer_snapshot.size(); ++level)
    transfer_counters(h, (int)level, h->transfer_snapshot[level].data());
  // ... and mfmg_hip_hierarchy_coarse_block_info what the coarse solver's block calls launched since
  if (auto hs = std::dynamic_pointer_cast<HipSolver const>(h->hierarchy->levels().back().get_solver()))
    hs->reset_block_counters();
}

void check_block(mfmg_hip_hierarchy_t h, int level, int32_t n_vectors, int64_t ld, const double *b, const double *x, bool on_ranks = true)
{
  require(h && b && x, "null argument");
  begin_block_call(h); // (every block entry point passes here first)
  require(on_ranks || !h->handle->comm.enabled(), "blocks of vectors are not implemented for a context with a communicator");
  check_block_shape(h, level, n_vectors, ld, b, x);
}

// The groups of a block, one after the other: `run` gets the columns of the group as views -- of the caller's vectors, or with
// "internal numbering" lexicographic of the library's block workspace, gathered before and scattered after (x only)
using BlockRun = std::function<void(std::vector<DVector const *> const &, std::vector<DVector *> const &)>;
void for_block_groups(mfmg_hip_hierarchy_t h, int level, bool read_x, int32_t n_vectors, int64_t ld, const double *b, double *x, BlockRun const &run)
{
  const int64_t n = level_size(h, level);
  const bool permute = h->perm && level == 0;
  int widths[kMfBlockMaxGroups];
  const int n_groups = mf_block_groups(n_vectors, widths);
  const int64_t wld = permute ? n + (n & 1) : ld;
  int64_t c0 = 0;
  for (int g = 0; g < n_groups; c0 += widths[g], ++g)
  {
    const int w = widths[g];
    double const *gb = b + c0 * ld;
    double *gx = x + c0 * ld;
    if (permute)
    {
      double *wb = h->block_workspace(0, (size_t)w * wld), *wx = h->block_workspace(1, (size_t)w * wld);
      for (int c = 0; c < w; ++c)
      {
        if (read_x)
          h->perm->gather2(b + (c0 + c) * ld, static_cast<double const *>(x + (c0 + c) * ld), wb + c * wld, wx + c * wld);
        else
          h->perm->gather(b + (c0 + c) * ld, wb + c * wld);
      }
      gb = wb;
      gx = wx;
    }
    BlockViews bv(*h->handle, n, wld, w, const_cast<double *>(gb)), xv(*h->handle, n, wld, w, gx);
    run(bv.cptr, xv.ptr);
    if (permute)
      for (int c = 0; c < w; ++c)
        h->perm->scatter(static_cast<double const *>(gx + c * wld), x + (c0 + c) * ld);
  }
}

void apply_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const double *b, double *x)
{
  check_block(h, 0, n_vectors, ld, b, x);
  const int64_t launches = block_kernel_launches(*h->hierarchy);
  int64_t looped = 0;
  for_block_groups(h, 0, !h->hierarchy->is_preconditioner(), n_vectors, ld, b, x, [&](std::vector<DVector const *> const &bp, std::vector<DVector *> const &xp) {
    h->hierarchy->apply_block(bp, xp);
    looped += h->hierarchy->block_columns_looped();
  });
  h->block_info[0] = h->hierarchy->block_width();
  h->block_info[1] = block_kernel_launches(*h->hierarchy) - launches;
  h->block_info[2] = looped;
}
} // namespace

int mfmg_hip_hierarchy_apply_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const double *b, double *x)
{
  return guarded([&] { apply_block(h, n_vectors, ld, b, x); });
}

int mfmg_hip_hierarchy_vmult_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, double *x, const double *b)
{
  return guarded([&] {
    require(h != nullptr, "null argument");
    TimerSubsection apply(h->timer, "Apply");
    apply_block(h, n_vectors, ld, b, x);
  });
}

int mfmg_hip_hierarchy_smoother_apply_block(mfmg_hip_hierarchy_t h, int32_t level, int32_t n_vectors, int64_t ld, const double *b, double *x)
{
  return guarded([&] {
    require(h != nullptr, "null argument");
    require(level >= 0 && level < (int)h->hierarchy->levels().size(), "level out of range");
    check_block(h, level, n_vectors, ld, b, x);
    auto smoother = h->hierarchy->levels()[level].get_smoother();
    require(smoother != nullptr, "this level has no smoother");
    const int64_t launches = block_kernel_launches(*h->hierarchy);
    int64_t looped = 0;
    for_block_groups(h, level, true, n_vectors, ld, b, x, [&](std::vector<DVector const *> const &bp, std::vector<DVector *> const &xp) {
      smoother->apply_block(bp, xp);
      if (smoother->block_width() == 1 || bp.size() == 1)
        looped += (int64_t)bp.size();
    });
    h->block_info[0] = level == 0 ? smoother->block_width() : 1;
    h->block_info[1] = block_kernel_launches(*h->hierarchy) - launches;
    h->block_info[2] = looped;
  });
}

int mfmg_hip_hierarchy_block_info(mfmg_hip_hierarchy_t h, int64_t *fields)
{
  return guarded([&] {
    require(h && fields, "null argument");
    h->block_info[0] = h->hierarchy->block_width();
    for (int i = 0; i < MFMG_HIP_BLOCK_INFO_FIELDS; ++i)
      fields[i] = h->block_info[i];
  });
}

int mfmg_hip_hierarchy_internal_numbering(mfmg_hip_hierarchy_t h, int *lexicographic, int *permuted)
{
  return guarded([&] {
    require(h && lexicographic && permuted, "null argument");
    *lexicographic = h->lexicographic ? 1 : 0;
    *permuted = h->perm ? 1 : 0;
  });
}

int mfmg_hip_hierarchy_permute(mfmg_hip_hierarchy_t h, int to_internal, int fp32, const void *in, void *out)
{
  return guarded([&] {
    require(h && in && out, "null argument");
    require(in != out, "the permutation does not work in place");
    if (!h->perm)
    {
      const size_t bytes = (size_t)level_size(h, 0) * (fp32 ? sizeof(float) : sizeof(double));
      MFMG_HIP_CHECK(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, h->handle->stream));
    }
    else if (fp32)
    {
      if (to_internal)
        h->perm->gather(static_cast<float const *>(in), static_cast<float *>(out));
      else
        h->perm->scatter(static_cast<float const *>(in), static_cast<float *>(out));
    }
    else
    {
      if (to_internal)
        h->perm->gather(static_cast<double const *>(in), static_cast<double *>(out));
      else
        h->perm->scatter(static_cast<double const *>(in), static_cast<double *>(out));
    }
  });
}

// Hierarchy::apply with the fine level in FP32 (HipFloatFineLevel)
int mfmg_hip_hierarchy_apply_f32(mfmg_hip_hierarchy_t h, const float *b, float *x)
{
  return guarded([&] {
    require(h && b && x, "null argument");
    require(h->fine_f32 != nullptr, "the hierarchy was not built with \"fine level precision\" float");
    if (h->perm)
    {
      float *wb = h->workspace_f32(0), *wx = h->workspace_f32(1);
      if (h->hierarchy->is_preconditioner())
        h->perm->gather(b, wb);
      else
        h->perm->gather2(b, static_cast<float const *>(x), wb, wx);
      h->fine_f32->apply(wb, wx);
      h->perm->scatter(static_cast<float const *>(wx), x);
      return;
    }
    h->fine_f32->apply(b, x);
  });
}

// ... on the columns of a float block (HipFloatFineLevel::apply_block).  "internal numbering" lexicographic: the columns are gathered
// into a library block and scattered back one by one, as mfmg_hip_hierarchy_apply_f32 does with its vector.
int mfmg_hip_hierarchy_apply_f32_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const float *b, float *x)
{
  return guarded([&] {
    require(h != nullptr, "null argument");
    require(h->fine_f32 != nullptr, "the hierarchy was not built with \"fine level precision\" float");
    {
      // several ranks: the float level exchanges in the fine DoF space, through the registered transport
      HaloCommunicator const &comm = h->handle->comm;
      require(!comm.enabled() || (comm.spaces[1].configured() && comm.transport != nullptr),
              "a context with a communicator needs its fine DoF space configured and a transport registered");
    }
    check_block_shape(h, 0, n_vectors, ld, b, x);
    const int64_t n = level_size(h, 0);
    const int64_t launches = h->fine_f32->block_launches();
    if (h->perm)
    {
      const int64_t wld = n + (n & 1);
      float *wb = h->block_workspace_f32(0, (size_t)n_vectors * wld), *wx = h->block_workspace_f32(1, (size_t)n_vectors * wld);
      for (int c = 0; c < n_vectors; ++c)
      {
        if (h->hierarchy->is_preconditioner())
          h->perm->gather(b + c * ld, wb + c * wld);
        else
          h->perm->gather2(b + c * ld, static_cast<float const *>(x + c * ld), wb + c * wld, wx + c * wld);
      }
      h->fine_f32->apply_block(n_vectors, wld, wb, wx);
      for (int c = 0; c < n_vectors; ++c)
        h->perm->scatter(static_cast<float const *>(wx + c * wld), x + c * ld);
    }
    else
      h->fine_f32->apply_block(n_vectors, ld, b, x);
    h->block_info_f32[0] = h->fine_f32->block_width();
    h->block_info_f32[1] = h->fine_f32->block_launches() - launches;
    h->block_info_f32[2] = h->fine_f32->block_columns_looped();
  });
}

int mfmg_hip_hierarchy_block_info_f32(mfmg_hip_hierarchy_t h, int64_t *fields)
{
  return guarded([&] {
    require(h && fields, "null argument");
    require(h->fine_f32 != nullptr, "the hierarchy was not built with \"fine level precision\" float");
    h->block_info_f32[0] = h->fine_f32->block_width();
    for (int i = 0; i < MFMG_HIP_BLOCK_INFO_FIELDS; ++i)
      fields[i] = h->block_info_f32[i];
  });
}

int mfmg_hip_hierarchy_sweep_terms_f32(mfmg_hip_hierarchy_t h, int *terms_out_of_place)
{
  return guarded([&] {
    require(h && terms_out_of_place, "null argument");
    require(h->fine_f32 != nullptr, "the hierarchy was not built with \"fine level precision\" float");
    *terms_out_of_place = h->fine_f32->sweep_terms();
  });
}

// the FP32 operator of the fine level on its own (tests)
int mfmg_hip_hierarchy_operator_f32(mfmg_hip_hierarchy_t h, int mode, const float *x, const float *b, const float *x_prev, float alpha,
                                    float beta, float *out)
{
  return guarded([&] {
    require(h && x && out, "null argument");
    require(h->fine_f32 != nullptr, "the hierarchy was not built with \"fine level precision\" float");
    require(mode >= 0 && mode <= 2, "mode: 0 out = A x, 1 out = A x - b, 2 a smoother term");
    require(mode == 0 || b != nullptr, "null argument");
    require(x != out && x_prev != out, "the operator does not work in place");
    require(!h->perm, "the level-wise FP32 operator takes the internal numbering: not with permuted vectors");
    if (mode == 0)
      h->fine_f32->vmult(x, out);
    else if (mode == 1)
      h->fine_f32->residual(x, b, out);
    else
      h->fine_f32->smoother_step(b, x, x_prev, alpha, beta, out);
  });
}

int mfmg_hip_hierarchy_vmult(mfmg_hip_hierarchy_t h, double *x, const double *b)
{
  return guarded([&] {
    require(h && b && x, "null argument");
    if (h->perm)
    {
      TimerSubsection apply(h->timer, "Apply");
      apply_permuted(h, b, x);
      return;
    }
    const int64_t n = level_size(h, 0);
    DVector bv(*h->handle, n, const_cast<double *>(b)), xv(*h->handle, n, x);
    h->hierarchy->vmult(xv, bv);
  });
}

int mfmg_hip_hierarchy_solve_cg(mfmg_hip_hierarchy_t h, const double *b, double *x, double tolerance,
                                int32_t max_iterations, int32_t *n_iterations, double *final_residual,
                                double *residual_history, int32_t history_len)
{
  return guarded([&] {
    require(h && b && x, "null argument");
    require(tolerance >= 0. && max_iterations >= 0, "bad stopping criterion");
    const KrylovResult result = solve_cg(krylov_setting(h, true), b, x, tolerance, max_iterations, residual_history, history_len);
    deliver_result(result, n_iterations, final_residual, nullptr);
    if (!result.all_converged())
      throw std::runtime_error("CG did not reach the tolerance within max_iterations (SolverControl::NoConvergence)");
  });
}

int mfmg_hip_hierarchy_solve_cg_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const double *b, double *x,
                                      const double *tolerances, int32_t max_iterations, int32_t *n_iterations, double *final_residuals,
                                      double *residual_history, int32_t history_ld, int64_t *work)
{
  return guarded([&] {
    check_block(h, 0, n_vectors, ld, b, x);
    require(tolerances != nullptr, "null argument");
    require(max_iterations >= 0, "bad stopping criterion");
    for (int c = 0; c < n_vectors; ++c)
      require(tolerances[c] >= 0., "bad stopping criterion");
    require(residual_history == nullptr || history_ld >= 0, "bad history length");
    const KrylovResult result =
      solve_cg_block(krylov_setting(h, false), n_vectors, ld, b, x, tolerances, max_iterations, residual_history, history_ld);
    deliver_result(result, n_iterations, final_residuals, work);
    if (!result.all_converged())
      throw std::runtime_error("CG did not reach the tolerance within max_iterations on every column of the block (SolverControl::NoConvergence)");
  });
}

int mfmg_hip_block_cg_retire(int32_t n_active, const int32_t *retire_flags, int32_t *slot_col, int32_t *moves, int32_t *n_moves,
                             int32_t *n_active_out)
{
  return guarded([&] {
    require(retire_flags && slot_col && moves && n_moves && n_active_out, "null argument");
    require(n_active >= 0 && n_active <= MFMG_HIP_BLOCK_MAX_VECTORS, "a block holds at most 64 slots");
    int left = 0;
    *n_moves = block_krylov::plan_retire(n_active, retire_flags, slot_col, moves, &left);
    *n_active_out = left;
  });
}

namespace
{
void check_kernel_block(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld)
{
  require(ctx != nullptr, "null argument");
  require(!ctx->handle->comm.enabled(), "blocks of vectors are not implemented for a context with a communicator");
  require(n >= 1 && k >= 1 && k <= MFMG_HIP_BLOCK_MAX_VECTORS && ld >= n, "bad shape");
}
} // namespace

int mfmg_hip_block_dots(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld, const double *X, const double *Y, double *out)
{
  return guarded([&] {
    check_kernel_block(ctx, n, k, ld);
    require(X && Y && out, "null argument");
    HipHandle &handle = *ctx->handle;
    DeviceBuffer<double> partials((size_t)k * block_krylov::kReduceBlocks);
    block_krylov::dots(handle, n, k, ld, X, Y, partials.data(), out);
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream)); // (the partials go away)
  });
}

int mfmg_hip_block_cg_direction(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld, const double *Z, double *P, const double *rz_new,
                                const double *rz_old)
{
  return guarded([&] {
    check_kernel_block(ctx, n, k, ld);
    require(Z && P && (rz_new || !rz_old), "null argument");
    block_krylov::cg_direction(*ctx->handle, n, k, ld, Z, P, rz_new, rz_old, rz_old == nullptr);
  });
}

int mfmg_hip_block_cg_update(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld, const double *P, const double *AP, double *R,
                             int64_t ldx, double *X, const int32_t *slot_col, const double *rz, const double *pap, double *rr_out)
{
  return guarded([&] {
    check_kernel_block(ctx, n, k, ld);
    require(P && AP && R && X && slot_col && rz && pap && rr_out, "null argument");
    require(ldx >= n, "bad shape");
    HipHandle &handle = *ctx->handle;
    // (slot_col lives on the device: that its entries are columns of X, each named once, is the caller's contract)
    DeviceBuffer<double> partials((size_t)k * block_krylov::kReduceBlocks);
    block_krylov::cg_update(handle, n, k, ld, P, AP, R, ldx, X, slot_col, rz, pap, partials.data(), rr_out);
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream)); // (the partials go away)
  });
}

int mfmg_hip_hierarchy_operator_apply_block(mfmg_hip_hierarchy_t h, int32_t level, int32_t n_vectors, int64_t ld, const double *x, double *y)
{
  return guarded([&] {
    require(h != nullptr, "null argument");
    require(level >= 0 && level < (int)h->hierarchy->levels().size(), "level out of range");
    check_block(h, level, n_vectors, ld, x, y);
    auto op = h->hierarchy->levels()[level].get_operator();
    const int64_t launches = block_kernel_launches(*h->hierarchy);
    for_block_groups(h, level, false, n_vectors, ld, x, y, [&](std::vector<DVector const *> const &xp, std::vector<DVector *> const &yp) {
      op->apply_block(xp, yp);
    });
    h->block_info[0] = h->hierarchy->block_width();
    h->block_info[1] = block_kernel_launches(*h->hierarchy) - launches;
    h->block_info[2] = 0;
  });
}

int mfmg_hip_hierarchy_solve_fgmres(mfmg_hip_hierarchy_t h, const double *b, double *x, double tolerance, int32_t max_iterations,
                                    int32_t restart, int32_t preconditioner_fp32, int32_t *n_iterations, double *final_residual,
                                    double *residual_history, int32_t history_len)
{
  return guarded([&] {
    require(h && b && x, "null argument");
    require(tolerance >= 0. && max_iterations >= 0, "bad stopping criterion");
    require(restart >= 1, "the restart length must be at least 1");
    require(preconditioner_fp32 == 0 || preconditioner_fp32 == 1, "preconditioner_fp32 must be 0 or 1");
    const bool fp32 = preconditioner_fp32 != 0;
    require(!fp32 || h->fine_f32 != nullptr, "preconditioner_fp32 needs a hierarchy built with \"fine level precision\" float");
    const KrylovResult result =
      solve_fgmres(krylov_setting(h, true), b, x, tolerance, max_iterations, restart, fp32, residual_history, history_len);
    deliver_result(result, n_iterations, final_residual, nullptr);
    if (!result.all_converged())
      throw std::runtime_error("FGMRES did not reach the tolerance within max_iterations (SolverControl::NoConvergence)");
  });
}

// (a communicator: only where the caller enabled the block solve on the context with
// mfmg_hip_context_set_block_fgmres_on_ranks, on every rank alike; refused otherwise)
int mfmg_hip_hierarchy_solve_fgmres_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const double *b, double *x,
                                          const double *tolerances, int32_t max_iterations, int32_t restart, int32_t preconditioner_fp32,
                                          int32_t *n_iterations, double *final_residuals, double *residual_history, int32_t history_ld,
                                          int64_t *work)
{
  return guarded([&] {
    check_block(h, 0, n_vectors, ld, b, x, h && h->handle->block_fgmres_on_ranks);
    require(tolerances != nullptr, "null argument");
    require(max_iterations >= 0, "bad stopping criterion");
    for (int c = 0; c < n_vectors; ++c)
      require(tolerances[c] >= 0., "bad stopping criterion");
    require(restart >= 1, "the restart length must be at least 1");
    require(preconditioner_fp32 == 0 || preconditioner_fp32 == 1, "preconditioner_fp32 must be 0 or 1");
    require(residual_history == nullptr || history_ld >= 0, "bad history length");
    const bool fp32 = preconditioner_fp32 != 0;
    require(!fp32 || h->fine_f32 != nullptr, "preconditioner_fp32 needs a hierarchy built with \"fine level precision\" float");
    const KrylovResult result = solve_fgmres_block(krylov_setting(h, false), n_vectors, ld, b, x, tolerances, max_iterations, restart, fp32,
                                                   residual_history, history_ld);
    deliver_result(result, n_iterations, final_residuals, work);
    h->block_solve_allreduces = result.allreduces; // (mfmg_hip_hierarchy_block_solve_allreduces)
    if (fp32) // (mfmg_hip_hierarchy_block_info_f32: the preconditioner applications of this solve)
      std::copy(result.block_info_f32, result.block_info_f32 + MFMG_HIP_BLOCK_INFO_FIELDS, h->block_info_f32);
    if (!result.all_converged())
      throw std::runtime_error("FGMRES did not reach the tolerance within max_iterations on every column of the block (SolverControl::NoConvergence)");
  });
}

int mfmg_hip_hierarchy_block_solve_allreduces(mfmg_hip_hierarchy_t h, int64_t *n)
{
  return guarded([&] {
    require(h && n, "null argument");
    *n = h->block_solve_allreduces;
  });
}

int mfmg_hip_block_fgmres_plan(int32_t n_slots, const int32_t *live, const int32_t *slot_col, int32_t *run_start, int32_t *run_width,
                               int32_t *run_groups, int32_t *n_runs, int32_t *group_width, int32_t *n_groups, int32_t *packed_col,
                               int32_t *n_packed)
{
  return guarded([&] {
    require(live && slot_col && run_start && run_width && run_groups && n_runs && group_width && n_groups && packed_col && n_packed,
            "null argument");
    require(n_slots >= 0 && n_slots <= MFMG_HIP_BLOCK_MAX_VECTORS, "a block holds at most 64 slots");
    *n_runs = block_krylov_basis::plan(n_slots, live, slot_col, run_start, run_width, run_groups, group_width, n_groups, packed_col, n_packed);
  });
}

namespace
{
// the list of the test entry points: n_live different slots of a block of k, in ascending order
extern "C++" block_krylov_basis::SlotList checked_slot_list(int32_t k, int32_t n_live, const int32_t *slots, const int32_t *cols, int32_t n_cols)
{
  require(slots != nullptr, "null argument");
  require(k >= 1 && k <= MFMG_HIP_BLOCK_MAX_VECTORS && n_live >= 1 && n_live <= k, "a block holds 1 to 64 slots, of which 1 to all are live");
  block_krylov_basis::SlotList l;
  for (int i = 0; i < n_live; ++i)
  {
    require(slots[i] >= 0 && slots[i] < k && (i == 0 || slots[i] > slots[i - 1]), "the live slots are named once, in ascending order");
    l.id[i] = slots[i];
    l.col[i] = cols ? cols[slots[i]] : slots[i];
    require(l.col[i] >= 0 && l.col[i] < n_cols, "a slot's column lies outside x");
    for (int q = 0; q < i; ++q)
      require(l.col[q] != l.col[i], "two live slots name one column of x");
  }
  l.count = n_live;
  return l;
}
} // namespace

int mfmg_hip_block_krylov_orthogonalize(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld, int32_t j, int32_t n_live,
                                        const int32_t *live_slots, double *V, double *v_next, float *v_next_f32, double *h_out,
                                        double *norm_out)
{
  namespace bkb = block_krylov_basis;
  return guarded([&] {
    require(ctx && V && h_out && norm_out, "null argument");
    require(!ctx->handle->comm.enabled(), "blocks of vectors are not implemented for a context with a communicator");
    require(n >= 1 && ld >= n && j >= 0, "bad shape");
    require(ld % 2 == 0 && reinterpret_cast<uintptr_t>(V) % 16 == 0 && reinterpret_cast<uintptr_t>(v_next) % 16 == 0 &&
                reinterpret_cast<uintptr_t>(v_next_f32) % 8 == 0,
            "the basis block needs an even leading dimension and a base aligned to 16 bytes");
    const bkb::SlotList l = checked_slot_list(k, n_live, live_slots, nullptr, k);
    HipHandle &handle = *ctx->handle;
    bkb::Scratch scratch(k, j + 1);
    const bkb::Basis B{n, ld, (int64_t)k * ld, V};
    double *const w = B.vector(j + 1);
    for (int pass = 0; pass < 2; ++pass)
    {
      bkb::dots(handle, scratch, l, B, j + 1, w, h_out, j + 1, pass == 1);
      bkb::update(handle, scratch, l, B, j + 1, w, pass == 1);
    }
    bkb::scale_store(handle, scratch, l, n, ld, w, v_next, v_next_f32, norm_out, 1);
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream)); // (the scratch goes away)
  });
}

int mfmg_hip_block_krylov_orthogonalize_box(mfmg_hip_context_t ctx, const int64_t *local_nodes, const int64_t *own0, const int64_t *own_n,
                                            int32_t comps, int32_t k, int64_t ld, int32_t j, int32_t n_live, const int32_t *live_slots,
                                            double *V, double *v_next, double *h_out, double *norm_out)
{
  namespace bkb = block_krylov_basis;
  return guarded([&] {
    require(ctx && local_nodes && own0 && own_n && V && h_out && norm_out, "null argument");
    require(comps >= 1 && j >= 0, "bad shape");
    HipHandle &handle = *ctx->handle;
    require(!handle.comm.enabled(), "mfmg_hip_block_krylov_orthogonalize_box runs the kernels of one rank: a context without a communicator");
    krylov::OwnedBox box;
    box.comps = comps;
    for (int d = 0; d < 3; ++d)
    {
      require(own0[d] >= 0 && own_n[d] >= 1 && own0[d] + own_n[d] <= local_nodes[d], "the owned box leaves the local box");
      box.local[d] = local_nodes[d];
      box.own0[d] = own0[d];
      box.own_n[d] = own_n[d];
    }
    require(ld >= box.n_local(), "bad shape");
    require(ld % 2 == 0 && reinterpret_cast<uintptr_t>(V) % 16 == 0 && reinterpret_cast<uintptr_t>(v_next) % 16 == 0,
            "the basis block needs an even leading dimension and a base aligned to 16 bytes");
    const bkb::SlotList l = checked_slot_list(k, n_live, live_slots, nullptr, k);
    bkb::Scratch scratch(k, j + 1);
    const bkb::Basis B{box.n_local(), ld, (int64_t)k * ld, V};
    double *const w = B.vector(j + 1);
    for (int pass = 0; pass < 2; ++pass)
    {
      // (one rank: the sum over the ranks is the identity)
      bkb::dots(handle, scratch, l, box, B, j + 1, w, h_out, j + 1, pass == 1);
      bkb::update(handle, scratch, l, box, B, j + 1, w, pass == 1);
    }
    bkb::norm_finish(handle, scratch, l, box);
    bkb::scale_store(handle, l, box, ld, scratch.norm_squared.data(), w, v_next, norm_out, 1);
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream)); // (the scratch goes away)
  });
}

int mfmg_hip_block_krylov_combine(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld, int32_t j, int32_t n_live,
                                  const int32_t *live_slots, const int32_t *slot_col, const double *Z, const double *y, int32_t n_x_columns,
                                  int64_t ldx, double *x)
{
  namespace bkb = block_krylov_basis;
  return guarded([&] {
    require(ctx && Z && y && x && slot_col, "null argument");
    require(!ctx->handle->comm.enabled(), "blocks of vectors are not implemented for a context with a communicator");
    require(n >= 1 && ld >= n && ldx >= n && j >= 0 && n_x_columns >= 1, "bad shape");
    require(ld % 2 == 0 && reinterpret_cast<uintptr_t>(Z) % 16 == 0, "the basis block needs an even leading dimension and a base aligned to 16 bytes");
    const bkb::SlotList l = checked_slot_list(k, n_live, live_slots, slot_col, n_x_columns);
    bkb::combine(*ctx->handle, l, bkb::Basis{n, ld, (int64_t)k * ld, const_cast<double *>(Z)}, j + 1, y, j + 1, x, ldx);
  });
}

int mfmg_hip_krylov_orthogonalize(mfmg_hip_context_t ctx, int64_t n, int64_t ld, int32_t j, const double *V, double *w, double *h_out,
                                  double *norm_out, int32_t passes)
{
  return guarded([&] {
    require(ctx && V && w && h_out && norm_out, "null argument");
    require(n >= 1 && ld >= n && j >= 0 && passes >= 1, "bad shape");
    HipHandle &handle = *ctx->handle;
    krylov::Scratch scratch(j + 1);
    for (int pass = 0; pass < passes; ++pass)
    {
      krylov::basis_dots(handle, scratch, n, ld, j + 1, V, w, scratch.pass_coefficients.data(), h_out, pass > 0);
      krylov::basis_update(handle, scratch, n, ld, j + 1, V, scratch.pass_coefficients.data(), w, pass + 1 == passes);
    }
    krylov::basis_scale_store(handle, scratch, n, w, nullptr, nullptr, norm_out);
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream)); // (the scratch goes away)
  });
}

int mfmg_hip_krylov_orthogonalize_box(mfmg_hip_context_t ctx, const int64_t *local_nodes, const int64_t *own0, const int64_t *own_n,
                                      int32_t comps, int64_t ld, int32_t j, const double *V, double *w, double *h_out, double *norm_out,
                                      int32_t passes)
{
  return guarded([&] {
    require(ctx && local_nodes && own0 && own_n && V && w && h_out && norm_out, "null argument");
    require(comps >= 1 && j >= 0 && passes >= 1, "bad shape");
    HipHandle &handle = *ctx->handle;
    require(!handle.comm.enabled(), "mfmg_hip_krylov_orthogonalize_box runs the kernels of one rank: a context without a communicator");
    krylov::OwnedBox box;
    box.comps = comps;
    for (int d = 0; d < 3; ++d)
    {
      require(own0[d] >= 0 && own_n[d] >= 1 && own0[d] + own_n[d] <= local_nodes[d], "the owned box leaves the local box");
      box.local[d] = local_nodes[d];
      box.own0[d] = own0[d];
      box.own_n[d] = own_n[d];
    }
    require(ld >= box.n_local(), "bad shape");
    krylov::Scratch scratch(j + 1);
    for (int pass = 0; pass < passes; ++pass)
    {
      krylov::basis_dots(handle, scratch, box, ld, j + 1, V, w, scratch.pass_coefficients.data(), h_out, pass > 0);
      krylov::basis_update(handle, scratch, box, ld, j + 1, V, scratch.pass_coefficients.data(), w, pass + 1 == passes);
    }
    // (one rank: the sum over the ranks is the identity)
    krylov::basis_norm_finish(handle, scratch, box);
    krylov::basis_scale_store(handle, box, scratch.norm_squared.data(), w, nullptr, norm_out);
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream)); // (the scratch goes away)
  });
}

int mfmg_hip_block_dots_box(mfmg_hip_context_t ctx, const int64_t *local_nodes, const int64_t *own0, const int64_t *own_n, int32_t comps,
                            int32_t k, int64_t ld, const double *X, const double *Y, double *out)
{
  return guarded([&] {
    require(ctx && local_nodes && own0 && own_n && X && Y && out, "null argument");
    require(comps >= 1 && k >= 1 && k <= MFMG_HIP_BLOCK_MAX_VECTORS, "bad shape");
    HipHandle &handle = *ctx->handle;
    require(!handle.comm.enabled(), "mfmg_hip_block_dots_box runs the kernels of one rank: a context without a communicator");
    krylov::OwnedBox box;
    box.comps = comps;
    for (int d = 0; d < 3; ++d)
    {
      require(own0[d] >= 0 && own_n[d] >= 1 && own0[d] + own_n[d] <= local_nodes[d], "the owned box leaves the local box");
      box.local[d] = local_nodes[d];
      box.own0[d] = own0[d];
      box.own_n[d] = own_n[d];
    }
    require(ld >= box.n_local(), "bad shape");
    DeviceBuffer<double> partials((size_t)k * block_krylov::kReduceBlocks);
    block_krylov::dots(handle, box, k, ld, X, Y, partials.data(), out);
    MFMG_HIP_CHECK(hipStreamSynchronize(handle.stream)); // (the partials go away)
  });
}

int mfmg_hip_krylov_combine(mfmg_hip_context_t ctx, int64_t n, int64_t ld, int32_t j, const double *Z, const double *y, double *x)
{
  return guarded([&] {
    require(ctx && Z && y && x, "null argument");
    require(n >= 1 && ld >= n && j >= 0, "bad shape");
    krylov::basis_combine(*ctx->handle, n, ld, j + 1, Z, y, x);
  });
}

int mfmg_hip_hierarchy_n_levels(mfmg_hip_hierarchy_t h, int32_t *n_levels)
{
  return guarded([&] {
    require(h && n_levels, "null argument");
    *n_levels = (int32_t)h->hierarchy->levels().size();
  });
}

int mfmg_hip_hierarchy_level_size(mfmg_hip_hierarchy_t h, int32_t level, int64_t *n)
{
  return guarded([&] {
    require(h && n, "null argument");
    *n = level_size(h, level);
  });
}

int mfmg_hip_hierarchy_operator_apply(mfmg_hip_hierarchy_t h, int32_t level, const double *x, double *y, int mode)
{
  return guarded([&] {
    require(h && x && y, "null argument");
    require(mode == MFMG_HIP_NO_TRANS || mode == MFMG_HIP_TRANS, "unknown operator mode");
    const int64_t n = level_size(h, level);
    // (the level-wise entry points permute per call: fine-level vectors in and out of the workspace)
    const bool permute = h->perm && level == 0;
    if (permute)
      h->perm->gather(x, h->workspace(0));
    DVector xv(*h->handle, n, permute ? h->workspace(0) : const_cast<double *>(x)), yv(*h->handle, n, permute ? h->workspace(1) : y);
    h->hierarchy->levels()[level].get_operator()->apply(
        xv, yv, mode == MFMG_HIP_TRANS ? OperatorMode::TRANS : OperatorMode::NO_TRANS);
    if (permute)
      h->perm->scatter(static_cast<double const *>(h->workspace(1)), y);
  });
}

int mfmg_hip_hierarchy_smoother_apply(mfmg_hip_hierarchy_t h, int32_t level, const double *b, double *x)
{
  return guarded([&] {
    require(h && b && x, "null argument");
    const int64_t n = level_size(h, level);
    auto smoother = h->hierarchy->levels()[level].get_smoother();
    require(smoother != nullptr, "this level has no smoother");
    const bool permute = h->perm && level == 0;
    if (permute)
      h->perm->gather2(b, static_cast<double const *>(x), h->workspace(0), h->workspace(1));
    DVector bv(*h->handle, n, permute ? h->workspace(0) : const_cast<double *>(b)), xv(*h->handle, n, permute ? h->workspace(1) : x);
    smoother->apply(bv, xv);
    if (permute)
      h->perm->scatter(static_cast<double const *>(h->workspace(1)), x);
  });
}

int mfmg_hip_hierarchy_restrictor_apply(mfmg_hip_hierarchy_t h, int32_t level, const double *in, double *out,
                                        int mode)
{
  return guarded([&] {
    require(h && in && out, "null argument");
    require(mode == MFMG_HIP_NO_TRANS || mode == MFMG_HIP_TRANS || mode == MFMG_HIP_TRANS_SUBTRACT, "unknown operator mode");
    require(level >= 1 && level < (int)h->hierarchy->levels().size(), "restrictors live on levels >= 1");
    const int64_t n_fine = level_size(h, level - 1), n_coarse = level_size(h, level);
    auto r = h->hierarchy->levels()[level].get_restrictor();
    const bool permute = h->perm && level == 1; // the fine side of the restrictor of level 1
    if (mode == MFMG_HIP_NO_TRANS)
    {
      if (permute)
        h->perm->gather(in, h->workspace(0));
      DVector iv(*h->handle, n_fine, permute ? h->workspace(0) : const_cast<double *>(in)), ov(*h->handle, n_coarse, out);
      r->apply(iv, ov, OperatorMode::NO_TRANS);
    }
    else
    {
      if (permute && mode == MFMG_HIP_TRANS_SUBTRACT)
        h->perm->gather(static_cast<double const *>(out), h->workspace(0));
      DVector iv(*h->handle, n_coarse, const_cast<double *>(in)), ov(*h->handle, n_fine, permute ? h->workspace(0) : out);
      if (mode == MFMG_HIP_TRANS)
        r->apply(iv, ov, OperatorMode::TRANS);
      else
        r->apply_subtract(iv, ov, OperatorMode::TRANS);
      if (permute)
        h->perm->scatter(static_cast<double const *>(h->workspace(0)), out);
    }
  });
}

int mfmg_hip_hierarchy_restrictor_apply_block(mfmg_hip_hierarchy_t h, int32_t level, int32_t n_vectors, int64_t ld_in, const double *in,
                                              int64_t ld_out, double *out, int mode)
{
  return guarded([&] {
    require(h && in && out, "null argument");
    require(mode == MFMG_HIP_NO_TRANS || mode == MFMG_HIP_TRANS || mode == MFMG_HIP_TRANS_SUBTRACT, "unknown operator mode");
    require(level >= 1 && level < (int)h->hierarchy->levels().size(), "restrictors live on levels >= 1");
    require(!h->handle->comm.enabled(), "blocks of vectors are not implemented for a context with a communicator");
    require(n_vectors >= 1 && n_vectors <= MFMG_HIP_BLOCK_MAX_VECTORS, "a block holds 1 to 64 vectors");
    const int64_t n_fine = level_size(h, level - 1), n_coarse = level_size(h, level);
    const bool restriction = mode == MFMG_HIP_NO_TRANS;
    const int64_t n_in = restriction ? n_fine : n_coarse, n_out = restriction ? n_coarse : n_fine;
    require(ld_in >= n_in && ld_out >= n_out, "the leading dimension of a block must be at least the vector size");
    require(ld_in % 2 == 0 && ld_out % 2 == 0, "the leading dimension of a block must be even (columns aligned to 16 bytes)");
    require(reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0, "the base of a block must be aligned to 16 bytes");
    const int64_t extent_in = (int64_t)(n_vectors - 1) * ld_in + n_in, extent_out = (int64_t)(n_vectors - 1) * ld_out + n_out;
    require(in + extent_in <= out || out + extent_out <= in, "the blocks in and out overlap");
    begin_block_call(h);
    auto r = h->hierarchy->levels()[level].get_restrictor();
    auto hr = std::dynamic_pointer_cast<HipMatrixOperator const>(r);
    require(hr != nullptr, "the restrictor of this level is no matrix operator");
    const auto what = restriction ? HipMatrixOperator::Transfer::restrict_to_coarse
                                  : (mode == MFMG_HIP_TRANS ? HipMatrixOperator::Transfer::prolongate : HipMatrixOperator::Transfer::prolongate_subtract);
    // the fine side of the restrictor of level 1 in the internal numbering: gathered into / scattered out of the block workspace,
    // one group at a time (for_block_groups); otherwise the whole block in one call, which cuts it into the same groups
    const bool permute = h->perm && level == 1;
    int widths[kMfBlockMaxGroups] = {n_vectors};
    const int n_groups = permute ? mf_block_groups(n_vectors, widths) : 1;
    const int64_t wld = n_fine + (n_fine & 1);
    int64_t c0 = 0;
    for (int g = 0; g < n_groups; c0 += widths[g], ++g)
    {
      const int w = widths[g];
      double const *gi = in + c0 * ld_in;
      double *go = out + c0 * ld_out;
      int64_t gld_in = ld_in, gld_out = ld_out;
      if (permute && restriction)
      {
        double *wi = h->block_workspace(0, (size_t)w * wld);
        for (int c = 0; c < w; ++c)
          h->perm->gather(gi + c * ld_in, wi + c * wld);
        gi = wi;
        gld_in = wld;
      }
      else if (permute)
      {
        double *wo = h->block_workspace(1, (size_t)w * wld);
        if (mode == MFMG_HIP_TRANS_SUBTRACT)
          for (int c = 0; c < w; ++c)
            h->perm->gather(static_cast<double const *>(go + c * ld_out), wo + c * wld);
        go = wo;
        gld_out = wld;
      }
      std::vector<DVector> iv, ov;
      iv.reserve(w);
      ov.reserve(w);
      std::vector<DVector const *> ip;
      std::vector<DVector *> op;
      for (int c = 0; c < w; ++c)
      {
        iv.emplace_back(*h->handle, n_in, const_cast<double *>(gi) + c * gld_in);
        ov.emplace_back(*h->handle, n_out, go + c * gld_out);
        ip.push_back(&iv.back());
        op.push_back(&ov.back());
      }
      hr->transfer_block(ip, op, what);
      if (permute && !restriction)
        for (int c = 0; c < w; ++c)
          h->perm->scatter(static_cast<double const *>(go + c * wld), out + (c0 + c) * ld_out);
    }
  });
}

int mfmg_hip_hierarchy_transfer_block_info(mfmg_hip_hierarchy_t h, int32_t level, int64_t fields[5])
{
  return guarded([&] {
    require(h && fields, "null argument");
    require(level >= 1 && level < (int)h->hierarchy->levels().size(), "restrictors live on levels >= 1");
    auto r = h->hierarchy->levels()[level].get_restrictor();
    fields[0] = r->transfer_block_width(OperatorMode::NO_TRANS);
    fields[1] = r->transfer_block_width(OperatorMode::TRANS);
    int64_t now[3];
    transfer_counters(h, level, now);
    for (int i = 0; i < 3; ++i)
      fields[2 + i] = (size_t)level < h->transfer_snapshot.size() ? now[i] - h->transfer_snapshot[level][i] : 0;
  });
}

int mfmg_hip_hierarchy_restrictor_form(mfmg_hip_hierarchy_t h, int32_t level, int32_t *fields, int32_t n)
{
  return guarded([&] {
    require(h && fields, "null argument");
    require(n >= MFMG_HIP_RESTRICTOR_FORM_FIELDS, "restrictor_form needs MFMG_HIP_RESTRICTOR_FORM_FIELDS fields");
    require(level >= 1 && level < (int)h->hierarchy->levels().size(), "restrictors live on levels >= 1");
    auto r = std::dynamic_pointer_cast<HipMatrixOperator const>(h->hierarchy->levels()[level].get_restrictor());
    StructuredRestrictorDevice const *s = r ? r->structured() : nullptr;
    std::fill(fields, fields + n, 0);
    if (s == nullptr)
      return;
    fields[0] = 1;
    fields[1] = s->n_eigenvectors();
    for (int d = 0; d < 3; ++d)
      fields[2 + d] = s->agglomerate_cells(d);
    fields[5] = s->float_planes() ? 1 : 0;
    fields[6] = (int32_t)s->regular_agglomerates();
    fields[7] = s->block_classes();
    fields[8] = (int32_t)s->listed_blocks();
    fields[9] = s->restrict_kernel();
    fields[10] = s->prolong_kernel();
    fields[11] = s->prolong_march() ? 1 : 0;
  });
}

int mfmg_hip_hierarchy_restrictor_eigensolver_info(mfmg_hip_hierarchy_t h, int64_t *fields, int32_t n)
{
  return guarded([&] {
    require(h && fields, "null argument");
    require(n >= MFMG_HIP_EIGENSOLVER_INFO_FIELDS, "restrictor_eigensolver_info needs MFMG_HIP_EIGENSOLVER_INFO_FIELDS fields");
    std::fill(fields, fields + n, 0);
    std::copy(h->eigensolver_info, h->eigensolver_info + MFMG_HIP_EIGENSOLVER_INFO_FIELDS, fields);
  });
}

int mfmg_hip_hierarchy_restrictor_eigensolver_seconds(mfmg_hip_hierarchy_t h, double *seconds)
{
  return guarded([&] {
    require(h && seconds, "null argument");
    *seconds = h->eigensolver_seconds;
  });
}

int mfmg_hip_amge_eigen(mfmg_hip_context_t ctx, const mfmg_hip_mesh_desc *mesh, const char *params_info, int matrix_free,
                        int64_t *n_agglomerates, int32_t *n_eigenvectors, int32_t *n_nodes, int32_t *n_vec, double *eigenvalues,
                        double *weights, int32_t *iterations, int32_t *flags)
{
  return guarded([&] {
    require(ctx && mesh && n_agglomerates && n_eigenvectors && n_nodes, "null argument");
    const bool query = !n_vec && !eigenvalues && !weights && !iterations && !flags;
    require(query || (n_vec && eigenvalues && weights && iterations && flags), "pass all output arrays, or none for the size query");
    ptree params = ptree::parse_info(params_info ? params_info : "");
    HipHandle &handle = *ctx->handle;
    StructuredMesh sm = StructuredMesh::from_desc(*mesh, handle.stream);
    // the options as the evaluators read them (HipMeshEvaluator / HipMatrixFreeMeshEvaluator::agglomerate_options)
    RestrictorOptions o;
    o.agglomerate[0] = params.get("agglomeration.nx", 2);
    o.agglomerate[1] = params.get("agglomeration.ny", 2);
    o.agglomerate[2] = params.get("agglomeration.nz", 2);
    o.n_eigenvectors = params.get("eigensolver.number of eigenvectors", 1);
    o.variant = params.get("eigensolver.variant", matrix_free ? "mf" : "device");
    o.selection = params.get("eigensolver.selection", "krylov");
    o.use_coefficient = params.get("eigensolver.use_coefficient", true);
    const std::string where = params.get("restrictor.eigensolver", "device");
    require(where == "device" || where == "lanczos", "mfmg_hip_amge_eigen runs the device solvers: restrictor.eigensolver device or lanczos");
    ASSERT_THROW(o.variant == "device" || o.variant == "host" || o.variant == "mf", "unknown AMGe variant \"" + o.variant + "\"");
    ASSERT_THROW(o.selection == "lapack" || o.selection == "krylov", "unknown eigenvector selection \"" + o.selection + "\"");
    ASSERT_THROW(o.n_eigenvectors >= 1, "number of eigenvectors must be positive");
    int cnt[3] = {1, 1, 1};
    for (int d = 0; d < sm.dim; ++d)
    {
      ASSERT_THROW(o.agglomerate[d] >= 1, "agglomerate dimensions must be positive");
      cnt[d] = (sm.n[d] + o.agglomerate[d] - 1) / o.agglomerate[d];
    }
    const int64_t n_agg = (int64_t)cnt[0] * cnt[1] * cnt[2];
    if (where == "lanczos")
    {
      o.solver = "lanczos";
      o.tolerance = params.get("eigensolver.tolerance", 1e-14);
      o.max_iterations = params.get("eigensolver.max_iterations", 200);
      o.percent_overshoot = params.get("eigensolver.percent_overshoot", 5);
      ASSERT_THROW(o.selection == "krylov", "eigensolver.selection lapack is not available with the Lanczos eigensolver: a Krylov "
                                            "solver returns the krylov selection");
      if (!amge_lanczos_supported(sm, o))
        ASSERT_THROW_NOT_IMPLEMENTED("the Lanczos eigensolver takes agglomerates of at most 729 nodes");
    }
    else if (!amge_device_supported(sm, o))
      ASSERT_THROW_NOT_IMPLEMENTED("the dense device eigensolver takes agglomerates of at most 64 nodes");
    int nodes = 1;
    if (where == "lanczos")
      for (int d = 0; d < sm.dim; ++d)
        nodes *= std::min(o.agglomerate[d], sm.n[d]) + 1;
    else
    {
      for (int d = 0; d < sm.dim; ++d)
        nodes *= o.agglomerate[d] + 1;
      nodes = nodes <= 27 ? 27 : 64;
    }
    *n_agglomerates = n_agg;
    *n_eigenvectors = o.n_eigenvectors;
    *n_nodes = nodes;
    if (query)
      return;
    std::vector<double> w, ev;
    std::vector<int32_t> nv, its, fl;
    int nmax = 0;
    if (where == "lanczos")
      amge_lanczos_eigen(handle, sm, o, cnt, w, nv, nmax, ev, its, fl);
    else
    {
      amge_device_eigen(handle, sm, o, cnt, w, nv, nmax, &ev);
      its.assign((size_t)n_agg, 0);
      fl.assign((size_t)n_agg, kAmgeConverged);
    }
    require(nmax == nodes, "internal: node stride of the eigensolver output");
    std::copy(nv.begin(), nv.end(), n_vec);
    std::copy(ev.begin(), ev.end(), eigenvalues);
    std::copy(w.begin(), w.end(), weights);
    std::copy(its.begin(), its.end(), iterations);
    std::copy(fl.begin(), fl.end(), flags);
  });
}

int mfmg_hip_hierarchy_ap_apply(mfmg_hip_hierarchy_t h, int32_t level, const double *in, double *out)
{
  return guarded([&] {
    require(h && in && out, "null argument");
    auto const &aps = h->hierarchy->ap_operators();
    require(level >= 1 && level <= (int)aps.size(), "no A R^T kept for this level (build the hierarchy with keep_ap = true)");
    const bool permute = h->perm && level == 1;
    DVector iv(*h->handle, level_size(h, level), const_cast<double *>(in)),
        ov(*h->handle, level_size(h, level - 1), permute ? h->workspace(0) : out);
    aps[level - 1]->apply(iv, ov);
    if (permute)
      h->perm->scatter(static_cast<double const *>(h->workspace(0)), out);
  });
}

int mfmg_hip_hierarchy_residual_restriction_classes(mfmg_hip_hierarchy_t h, int32_t level, int32_t *n_classes)
{
  return guarded([&] {
    require(h && n_classes, "null argument");
    require(level >= 1 && level < (int)h->hierarchy->levels().size(), "restrictors live on levels >= 1");
    auto r = std::dynamic_pointer_cast<HipMatrixOperator const>(h->hierarchy->levels()[level].get_restrictor());
    *n_classes = (r && r->has_residual_restriction()) ? (int32_t)r->residual_restriction_classes() : 0;
  });
}

int mfmg_hip_hierarchy_residual_restriction_form(mfmg_hip_hierarchy_t h, int32_t level, int64_t *fields, int32_t n)
{
  return guarded([&] {
    require(h && fields, "null argument");
    require(n >= MFMG_HIP_RESIDUAL_RESTRICTION_FORM_FIELDS, "residual_restriction_form needs MFMG_HIP_RESIDUAL_RESTRICTION_FORM_FIELDS fields");
    require(level >= 1 && level < (int)h->hierarchy->levels().size(), "restrictors live on levels >= 1");
    auto r = std::dynamic_pointer_cast<HipMatrixOperator const>(h->hierarchy->levels()[level].get_restrictor());
    std::fill(fields, fields + n, 0);
    if (!r || !r->has_residual_restriction() || r->structured() == nullptr)
      return;
    const auto f = r->structured()->residual_restriction_form();
    fields[0] = f.classes;
    fields[1] = f.segs;
    fields[2] = f.main_last;
    fields[3] = f.listed;
    fields[4] = f.listed_runs;
    fields[5] = f.kernel;
    fields[6] = f.tile_layers;
    fields[7] = f.tiles_j;
    fields[8] = f.n_tiles;
    fields[9] = (int64_t)f.main_blocks;
  });
}

int mfmg_hip_hierarchy_restrict_residual(mfmg_hip_hierarchy_t h, int32_t level, const double *x, const double *b, double *b_coarse)
{
  return guarded([&] {
    require(h && x && b && b_coarse, "null argument");
    require(level >= 1 && level < (int)h->hierarchy->levels().size(), "restrictors live on levels >= 1");
    const int64_t n_fine = level_size(h, level - 1), n_coarse = level_size(h, level);
    auto r = h->hierarchy->levels()[level].get_restrictor();
    auto a = h->hierarchy->levels()[level - 1].get_operator();
    const bool permute = h->perm && level == 1;
    if (permute)
      h->perm->gather2(x, b, h->workspace(0), h->workspace(1));
    DVector xv(*h->handle, n_fine, permute ? h->workspace(0) : const_cast<double *>(x)),
        bv(*h->handle, n_fine, permute ? h->workspace(1) : const_cast<double *>(b)), bc(*h->handle, n_coarse, b_coarse);
    if (!r->restrict_residual(*a, xv, bv, bc))
    {
      // the two steps of hierarchy.hpp:281-290
      DVector res(*h->handle, n_fine);
      a->residual(xv, bv, res);
      r->apply(res, bc);
    }
  });
}

int mfmg_hip_hierarchy_restrict_residual_f32(mfmg_hip_hierarchy_t h, int32_t level, const float *x, const float *b, double *b_coarse)
{
  return guarded([&] {
    require(h && x && b && b_coarse, "null argument");
    require(level >= 1 && level < (int)h->hierarchy->levels().size(), "restrictors live on levels >= 1");
    auto r = std::dynamic_pointer_cast<HipMatrixOperator const>(h->hierarchy->levels()[level].get_restrictor());
    auto a = h->hierarchy->levels()[level - 1].get_operator();
    // (no two-step form here: it rounds the residual to float, so it is not what this entry names)
    if (!r || !r->has_residual_restriction() || h->handle->comm.enabled())
      ASSERT_THROW_NOT_IMPLEMENTED("the one-pass residual restriction on float vectors is not available for this level");
    const bool permute = h->perm && level == 1;
    if (permute)
      h->perm->gather2(x, b, h->workspace_f32(0), h->workspace_f32(1));
    DVector bc(*h->handle, level_size(h, level), b_coarse);
    if (!r->restrict_residual_f32(*a, permute ? h->workspace_f32(0) : x, permute ? h->workspace_f32(1) : b, bc))
      ASSERT_THROW_NOT_IMPLEMENTED("the one-pass residual restriction on float vectors is not available for this level");
  });
}

int mfmg_hip_hierarchy_coarse_apply(mfmg_hip_hierarchy_t h, const double *b, double *x)
{
  return guarded([&] {
    require(h && b && x, "null argument");
    const int last = (int)h->hierarchy->levels().size() - 1;
    const int64_t n = level_size(h, last);
    DVector bv(*h->handle, n, const_cast<double *>(b)), xv(*h->handle, n, x);
    h->hierarchy->levels()[last].get_solver()->apply(bv, xv);
  });
}

int mfmg_hip_hierarchy_coarse_apply_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const double *b, double *x)
{
  return guarded([&] {
    require(h != nullptr, "null argument");
    const int last = (int)h->hierarchy->levels().size() - 1;
    begin_block_call(h);
    check_block_shape(h, last, n_vectors, ld, b, x);
    const int64_t n = level_size(h, last);
    std::vector<std::unique_ptr<DVector>> views;
    std::vector<DVector const *> bp;
    std::vector<DVector *> xp;
    for (int32_t c = 0; c < n_vectors; ++c)
    {
      views.emplace_back(new DVector(*h->handle, n, const_cast<double *>(b) + (int64_t)c * ld));
      bp.push_back(views.back().get());
      views.emplace_back(new DVector(*h->handle, n, x + (int64_t)c * ld));
      xp.push_back(views.back().get());
    }
    h->hierarchy->levels()[last].get_solver()->apply_block(bp, xp);
  });
}

int mfmg_hip_hierarchy_coarse_block_info(mfmg_hip_hierarchy_t h, int64_t fields[3])
{
  return guarded([&] {
    require(h && fields, "null argument");
    auto solver = h->hierarchy->levels().back().get_solver();
    fields[0] = solver->block_width();
    fields[1] = fields[2] = 0;
    if (auto hs = std::dynamic_pointer_cast<HipSolver const>(solver))
      hs->block_counters(fields[1], fields[2]);
  });
}

int mfmg_hip_hierarchy_set_block_csr(mfmg_hip_hierarchy_t h, int on, int32_t *n_matrices)
{
  return guarded([&] {
    require(h && n_matrices, "null argument");
    require(!h->handle->comm.enabled(), "the block forms of the CSR kernels are not implemented for a context with a communicator");
    // every SparseMatrixDevice<double> the cycle applies, each once: the assembled fine operator, a restrictor given as CSR, the
    // operators of the levels, and what the coarse solver holds (the aggregation hierarchy and the inverses of its bottom)
    std::vector<SparseMatrixDevice<double> *> seen;
    int n = 0;
    auto flip = [&](std::shared_ptr<SparseMatrixDevice<double>> const &m) {
      if (!m || std::find(seen.begin(), seen.end(), m.get()) != seen.end())
        return;
      seen.push_back(m.get());
      m->set_block_csr(on != 0);
      if (m->block_width() == 4 && m->block_csr_route(4) != CsrForm::csr_none)
        ++n;
    };
    auto const &levels = h->hierarchy->levels();
    for (size_t l = 0; l < levels.size(); ++l)
    {
      if (auto a = std::dynamic_pointer_cast<HipMatrixOperator const>(levels[l].get_operator()))
        flip(a->get_matrix());
      if (l == 0)
        continue;
      auto r = std::dynamic_pointer_cast<HipMatrixOperator const>(levels[l].get_restrictor());
      if (r && !r->has_structured())
        flip(r->get_matrix());
    }
    if (auto hs = std::dynamic_pointer_cast<HipSolver const>(levels.back().get_solver()))
      hs->for_each_cycle_matrix(flip);
    *n_matrices = n;
  });
}

namespace
{
// columns c -> new_id[c], every row sorted again
void renumber_columns(std::vector<int32_t> const &rp, std::vector<int32_t> &cl, std::vector<double> &vl, std::vector<int32_t> const &new_id)
{
  const int64_t n_rows = (int64_t)rp.size() - 1;
#pragma omp parallel
  {
    std::vector<std::pair<int32_t, double>> row;
#pragma omp for schedule(static)
    for (int64_t r = 0; r < n_rows; ++r)
    {
      row.clear();
      for (int32_t p = rp[r]; p < rp[r + 1]; ++p)
        row.emplace_back(new_id[cl[p]], vl[p]);
      std::sort(row.begin(), row.end(), [](auto const &a, auto const &b) { return a.first < b.first; });
      for (int32_t p = rp[r]; p < rp[r + 1]; ++p)
      {
        cl[p] = row[p - rp[r]].first;
        vl[p] = row[p - rp[r]].second;
      }
    }
  }
}
} // namespace

int mfmg_hip_hierarchy_set_restrictor(mfmg_hip_hierarchy_t h, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                      const int32_t *row_ptr_host, const int32_t *col_host, const double *val_host)
{
  return guarded([&] {
    require(h && row_ptr_host && col_host && val_host, "null argument");
    require(n_rows >= 1 && n_cols >= 1 && nnz >= 0 && nnz < (int64_t(1) << 31), "matrix shape out of range");
    require(n_cols == level_size(h, 0), "the restrictor must have one column per fine DoF");
    require(!h->handle->comm.enabled(), "set_restrictor is not available in a distributed run (the restrictor carries "
                                        "the halo layout of the coarse space)");
    require(row_ptr_host[0] == 0 && row_ptr_host[n_rows] == nnz, "row_ptr[0] != 0 or row_ptr[n_rows] != nnz");
    std::vector<int32_t> rp(row_ptr_host, row_ptr_host + n_rows + 1);
    std::vector<int32_t> cl(col_host, col_host + nnz);
    std::vector<double> vl(val_host, val_host + nnz);
    if (h->perm)
    {
      // the caller's columns are its DoF ids: the hierarchy takes the nodes
      auto const &node_dof = h->perm->node_dof_host();
      std::vector<int32_t> dof_node(node_dof.size());
      for (size_t nd = 0; nd < node_dof.size(); ++nd)
        dof_node[node_dof[nd]] = (int32_t)nd;
      for (auto c : cl)
        require(c >= 0 && c < n_cols, "column index out of range");
      renumber_columns(rp, cl, vl, dof_node);
    }
    auto m = std::make_shared<SparseMatrixDevice<double>>(*h->handle, n_rows, n_cols, std::move(rp), std::move(cl),
                                                          std::move(vl));
    {
      // the Galerkin product and the coarse solver are set up again, in the value precision this hierarchy was built with
      struct Restore
      {
        HipHandle &hd;
        ~Restore() { hd.setup_values_float = false; }
      } restore{*h->handle};
      h->handle->setup_values_float = h->setup_values_float;
      h->hierarchy->set_restrictor(std::make_shared<HipMatrixOperator>(m));
    }
    MFMG_HIP_CHECK(hipStreamSynchronize(h->handle->stream));
  });
}

int mfmg_hip_hierarchy_get_restrictor(mfmg_hip_hierarchy_t h, mfmg_hip_csr_t *r_borrowed)
{
  return guarded([&] {
    require(h && r_borrowed, "null argument");
    require(h->hierarchy->levels().size() >= 2, "the hierarchy has a single level");
    auto r = std::dynamic_pointer_cast<HipMatrixOperator const>(h->hierarchy->levels()[1].get_restrictor());
    require(r != nullptr, "the restrictor is not a matrix operator");
    if (h->perm)
    {
      // the hierarchy's columns are nodes: the caller gets a copy whose columns are its DoF ids
      std::vector<int32_t> rp, cl;
      std::vector<double> vl;
      r->get_matrix()->download(rp, cl, vl);
      renumber_columns(rp, cl, vl, h->perm->node_dof_host());
      auto m = std::make_shared<SparseMatrixDevice<double>>(*h->handle, r->get_matrix()->m(), r->get_matrix()->n(), std::move(rp),
                                                            std::move(cl), std::move(vl));
      r = std::make_shared<HipMatrixOperator>(m);
    }
    h->restrictor_view.op = std::const_pointer_cast<HipMatrixOperator>(r);
    h->restrictor_view.borrowed = true;
    *r_borrowed = &h->restrictor_view;
  });
}

int mfmg_hip_hierarchy_get_fine_operator(mfmg_hip_hierarchy_t h, mfmg_hip_csr_t *a_borrowed)
{
  return guarded([&] {
    require(h && a_borrowed, "null argument");
    auto a = std::dynamic_pointer_cast<HipMatrixOperator const>(h->hierarchy->levels().front().get_operator());
    require(a != nullptr, "the fine operator is matrix-free");
    h->fine_view.op = std::const_pointer_cast<HipMatrixOperator>(a);
    h->fine_view.borrowed = true;
    *a_borrowed = &h->fine_view;
  });
}

int mfmg_hip_hierarchy_get_coarse_operator(mfmg_hip_hierarchy_t h, mfmg_hip_csr_t *ac_borrowed)
{
  return guarded([&] {
    require(h && ac_borrowed, "null argument");
    require(h->hierarchy->levels().size() >= 2, "the hierarchy has a single level");
    auto a = std::dynamic_pointer_cast<HipMatrixOperator const>(h->hierarchy->levels().back().get_operator());
    require(a != nullptr, "the coarse operator is not a matrix operator");
    h->coarse_view.op = std::const_pointer_cast<HipMatrixOperator>(a);
    h->coarse_view.borrowed = true;
    *ac_borrowed = &h->coarse_view;
  });
}

namespace
{
HipSolver const *coarse_solver_of(mfmg_hip_hierarchy_t h)
{
  require(h != nullptr, "null argument");
  auto s = std::dynamic_pointer_cast<HipSolver const>(h->hierarchy->levels().back().get_solver());
  require(s != nullptr, "the hierarchy has no HIP coarse solver");
  return s.get();
}
} // namespace

int mfmg_hip_hierarchy_coarse_amg_levels(mfmg_hip_hierarchy_t h, int32_t *n_levels)
{
  return guarded([&] {
    require(n_levels != nullptr, "null argument");
    *n_levels = (int32_t)coarse_solver_of(h)->amg_levels().size();
  });
}

int mfmg_hip_hierarchy_coarse_amg_gather_level(mfmg_hip_hierarchy_t h, int32_t *level)
{
  return guarded([&] {
    require(level != nullptr, "null argument");
    *level = (int32_t)coarse_solver_of(h)->amg_gather_level();
  });
}

int mfmg_hip_hierarchy_coarse_amg_get(mfmg_hip_hierarchy_t h, int32_t level, int32_t which, mfmg_hip_csr_t *borrowed)
{
  return guarded([&] {
    require(borrowed != nullptr, "null argument");
    auto const &lv = coarse_solver_of(h)->amg_levels();
    require(level >= 0 && level < (int)lv.size(), "level out of range");
    require(which >= 0 && which <= 3, "which must be 0 (A), 1 (P), 2 (P^T as stored for the restriction) or 3 (the smoothed prolongator of the cycle)");
    auto op = which == 0 ? lv[level].a : which == 1 ? lv[level].prolongator : which == 2 ? lv[level].restrictor : lv[level].smoothed_prolongator;
    if (which == 3 && op == nullptr)
      throw NotImplementedExc("the smoothed prolongator of this level is not built");
    require(op != nullptr, "the last level has no transfer operators");
    h->amg_view.op = op;
    h->amg_view.borrowed = true;
    *borrowed = &h->amg_view;
  });
}

int mfmg_hip_hierarchy_coarse_amg_setup_info(mfmg_hip_hierarchy_t h, int32_t level, int32_t *values, int32_t n_values)
{
  return guarded([&] {
    require(values != nullptr && n_values >= MFMG_HIP_AMG_SETUP_INFO_FIELDS, "the buffer must hold MFMG_HIP_AMG_SETUP_INFO_FIELDS values");
    auto const &lv = coarse_solver_of(h)->amg_levels();
    require(level >= 0 && level < (int)lv.size(), "level out of range");
    auto const &L = lv[level];
    int32_t *v = values;
    *v++ = L.reach;
    for (int d = 0; d < 3; ++d)
      *v++ = L.period_p[d];
    for (int d = 0; d < 3; ++d)
      *v++ = L.period_a[d];
    for (int d = 0; d < 3; ++d)
      *v++ = L.period_t[d];
    *v++ = L.coarse_product;
    *v++ = L.replicated ? 1 : 0;
    *v++ = L.smoothed_prolongator != nullptr ? 1 : 0;
  });
}

int mfmg_hip_hierarchy_coarse_amg_smoother(mfmg_hip_hierarchy_t h, int32_t level, int32_t *degree, double *lambda_min,
                                           double *lambda_max)
{
  return guarded([&] {
    auto const &lv = coarse_solver_of(h)->amg_levels();
    require(level >= 0 && level + 1 < (int)lv.size(), "level out of range (the last level is solved directly)");
    auto const &s = lv[level].smoother;
    if (degree)
      *degree = s->degree();
    if (lambda_min)
      *lambda_min = s->lambda_min();
    if (lambda_max)
      *lambda_max = s->lambda_max();
  });
}

int mfmg_hip_hierarchy_smoother_info(mfmg_hip_hierarchy_t h, int32_t *degree, double *lambda_min, double *lambda_max)
{
  return guarded([&] {
    require(h != nullptr, "null argument");
    auto s = std::dynamic_pointer_cast<HipSmoother const>(h->hierarchy->levels()[0].get_smoother());
    require(s != nullptr, "level 0 has no HIP smoother");
    if (degree)
      *degree = s->degree();
    if (lambda_min)
      *lambda_min = s->lambda_min();
    if (lambda_max)
      *lambda_max = s->lambda_max();
  });
}

int mfmg_hip_hierarchy_smoother_sweep_terms(mfmg_hip_hierarchy_t h, int *terms_in_place, int *terms_out_of_place)
{
  return guarded([&] {
    require(h != nullptr && terms_in_place != nullptr && terms_out_of_place != nullptr, "null argument");
    auto s = std::dynamic_pointer_cast<HipSmoother const>(h->hierarchy->levels()[0].get_smoother());
    require(s != nullptr, "level 0 has no HIP smoother");
    s->sweep_terms(*terms_in_place, *terms_out_of_place);
  });
}

int mfmg_hip_hierarchy_operator_tile(mfmg_hip_hierarchy_t h, int *n_waves, int *tile_y, int *tile_z)
{
  return guarded([&] {
    require(h && n_waves && tile_y && tile_z, "null argument");
    auto op = std::dynamic_pointer_cast<HipMatrixFreeOperator const>(h->hierarchy->levels()[0].get_operator());
    require(op != nullptr, "the fine-level operator is not matrix-free");
    op->get_mesh_evaluator()->get_device_operator()->get_tile(*n_waves, *tile_y, *tile_z);
  });
}

int mfmg_hip_hierarchy_sweep_tile(mfmg_hip_hierarchy_t h, int n_terms, int *n_waves, int *tile_y, int *tile_z)
{
  return guarded([&] {
    require(h && n_waves && tile_y && tile_z, "null argument");
    auto op = std::dynamic_pointer_cast<HipMatrixFreeOperator const>(h->hierarchy->levels()[0].get_operator());
    require(op != nullptr, "the fine-level operator is not matrix-free");
    op->get_mesh_evaluator()->get_device_operator()->get_fused_tile(n_terms, *n_waves, *tile_y, *tile_z);
  });
}

int mfmg_hip_hierarchy_set_sweep_tile(mfmg_hip_hierarchy_t h, int n_waves, int tile_y, int tile_z)
{
  return guarded([&] {
    require(h != nullptr, "null argument");
    require(((n_waves >= 0 && n_waves <= 8) || (n_waves == 12 && tile_y == 2)) && tile_y >= 0 && tile_y <= 4 && tile_z >= 0, "bad tile");
    auto op = std::dynamic_pointer_cast<HipMatrixFreeOperator const>(h->hierarchy->levels()[0].get_operator());
    require(op != nullptr, "the fine-level operator is not matrix-free");
    op->get_mesh_evaluator()->get_device_operator()->set_fused_tile(n_waves, tile_y, tile_z);
  });
}

int mfmg_hip_hierarchy_set_operator_tile(mfmg_hip_hierarchy_t h, int n_waves, int tile_y, int tile_z)
{
  return guarded([&] {
    require(h != nullptr, "null argument");
    require(n_waves >= 0 && n_waves <= 8 && tile_y >= 0 && tile_z >= 0, "bad tile");
    auto op = std::dynamic_pointer_cast<HipMatrixFreeOperator const>(h->hierarchy->levels()[0].get_operator());
    require(op != nullptr, "the fine-level operator is not matrix-free");
    auto dev = op->get_mesh_evaluator()->get_device_operator();
    dev->set_tile(tile_y, tile_z);
    dev->set_tile_waves(n_waves);
  });
}

int mfmg_hip_hierarchy_timer_report(mfmg_hip_hierarchy_t h, char *buf, size_t buf_size)
{
  return guarded([&] {
    require(h && buf && buf_size > 0, "null argument");
    std::string s = h->timer->summary();
    std::strncpy(buf, s.c_str(), buf_size - 1);
    buf[buf_size - 1] = '\0';
  });
}

// ---- Q2 elements: the matrix-free operator and the solver on the refined Q1 cycle ---------------------------
int mfmg_hip_mf_laplace_q2_create(mfmg_hip_context_t ctx, const mfmg_hip_q2_mesh_desc *mesh, mfmg_hip_mf_laplace_q2_t *out)
{
  return guarded([&] {
    require(ctx && mesh && out, "null argument");
    Q2MeshDesc d;
    d.dim = mesh->dim;
    for (int k = 0; k < 3; ++k)
    {
      d.n_cells[k] = mesh->n_cells[k];
      d.cell_size[k] = mesh->cell_size[k];
    }
    d.n_dofs = mesh->n_dofs;
    d.coefficient = mesh->coefficient;
    d.constrained = mesh->constrained;
    d.arrays_on_device = mesh->arrays_on_device != 0;
    std::unique_ptr<mfmg_hip_mf_laplace_q2_s> h(new mfmg_hip_mf_laplace_q2_s);
    h->handle = ctx->handle.get();
    h->op = std::make_shared<HipQ2Operator>(
      std::make_shared<MatrixFreeLaplaceQ2Device<double>>(*ctx->handle, d, ctx->handle->allow_cell_constant));
    *out = h.release();
  });
}

int mfmg_hip_mf_laplace_q2_destroy(mfmg_hip_mf_laplace_q2_t op)
{
  return guarded([&] { delete op; });
}

int mfmg_hip_mf_laplace_q2_size(mfmg_hip_mf_laplace_q2_t op, int64_t *n_dofs)
{
  return guarded([&] {
    require(op && n_dofs, "null argument");
    *n_dofs = op->device().n_dofs();
  });
}

int mfmg_hip_mf_laplace_q2_cell_constant_layout(mfmg_hip_mf_laplace_q2_t op, int *in_use)
{
  return guarded([&] {
    require(op && in_use, "null argument");
    *in_use = op->device().cell_constant_layout() ? 1 : 0;
  });
}

int mfmg_hip_mf_laplace_q2_vmult(mfmg_hip_mf_laplace_q2_t op, const double *x, double *y)
{
  return guarded([&] {
    require(op && x && y, "null argument");
    op->device().vmult(x, y);
  });
}

int mfmg_hip_mf_laplace_q2_residual(mfmg_hip_mf_laplace_q2_t op, const double *x, const double *b, double *res)
{
  return guarded([&] {
    require(op && x && b && res, "null argument");
    op->device().residual(x, b, res);
  });
}

int mfmg_hip_mf_laplace_q2_smoother_step(mfmg_hip_mf_laplace_q2_t op, const double *b, const double *x, const double *x_prev,
                                         double alpha, double beta, double *out)
{
  return guarded([&] {
    require(op && b && x && out, "null argument");
    op->device().smoother_step(b, x, x_prev, alpha, beta, out);
  });
}

int mfmg_hip_mf_laplace_q2_diagonal(mfmg_hip_mf_laplace_q2_t op, double *diag)
{
  return guarded([&] {
    require(op && diag, "null argument");
    vec::copy<double>(*op->handle, op->device().n_dofs(), op->device().diagonal(), diag);
  });
}

int mfmg_hip_mf_laplace_q2_diagonal_inverse(mfmg_hip_mf_laplace_q2_t op, double *dinv)
{
  return guarded([&] {
    require(op && dinv, "null argument");
    vec::copy<double>(*op->handle, op->device().n_dofs(), op->device().diagonal_inverse(), dinv);
  });
}

int mfmg_hip_mf_laplace_q2_tile_shapes(int32_t *n_shapes, int32_t *tiles, int32_t capacity)
{
  return guarded([&] {
    require(n_shapes != nullptr, "null argument");
    *n_shapes = kQ2TileShapes;
    if (tiles)
    {
      require(capacity >= 3 * kQ2TileShapes, "`tiles` holds three ints per shape");
      for (int s = 0; s < kQ2TileShapes; ++s)
      {
        tiles[3 * s] = kQ2Tiles[s].tx();
        tiles[3 * s + 1] = kQ2Tiles[s].ty();
        tiles[3 * s + 2] = kQ2Tiles[s].tz;
      }
    }
  });
}

int mfmg_hip_mf_laplace_q2_get_tile(mfmg_hip_mf_laplace_q2_t op, int *tile_x, int *tile_y, int *tile_z)
{
  return guarded([&] {
    require(op && tile_x && tile_y && tile_z, "null argument");
    const Q2Tile t = op->device().get_tile();
    *tile_x = t.tx();
    *tile_y = t.ty();
    *tile_z = t.tz;
  });
}

int mfmg_hip_mf_laplace_q2_set_tile(mfmg_hip_mf_laplace_q2_t op, int tile_x, int tile_y, int tile_z)
{
  return guarded([&] {
    require(op != nullptr, "null argument");
    int shape = (tile_x == 0 && tile_y == 0 && tile_z == 0) ? -1 : kQ2TileShapes;
    for (int s = 0; s < kQ2TileShapes; ++s)
      if (kQ2Tiles[s].tx() == tile_x && kQ2Tiles[s].ty() == tile_y && kQ2Tiles[s].tz == tile_z)
        shape = s;
    require(shape < kQ2TileShapes, "not a tile shape of the Q2 operator (mfmg_hip_mf_laplace_q2_tile_shapes lists them)");
    op->device().set_tile(shape);
  });
}

int mfmg_hip_high_order_create(mfmg_hip_hierarchy_t hierarchy, mfmg_hip_mf_laplace_q2_t q2_operator, const char *params_info,
                               mfmg_hip_high_order_t *out)
{
  return guarded([&] {
    require(hierarchy && q2_operator && out, "null argument");
    require(hierarchy->handle == q2_operator->handle, "the hierarchy and the Q2 operator were built on different contexts");
    require(hierarchy->perm == nullptr, "the high-order preconditioner needs a Q1 hierarchy that runs in the caller's lexicographic numbering");
    if (hierarchy->handle->comm.enabled())
      ASSERT_THROW_NOT_IMPLEMENTED("the high-order preconditioner runs on one rank (the context has a communicator)");
    const ptree all = ptree::parse_info(params_info ? params_info : "");
    ptree const *sub = all.get_child_optional("high order");
    std::unique_ptr<mfmg_hip_high_order_s> p(new mfmg_hip_high_order_s);
    p->hierarchy = hierarchy;
    p->prec.reset(new HighOrderPreconditioner(q2_operator->op, *hierarchy->hierarchy, sub ? *sub : ptree()));
    *out = p.release();
  });
}

int mfmg_hip_high_order_destroy(mfmg_hip_high_order_t p)
{
  return guarded([&] { delete p; });
}

int mfmg_hip_high_order_apply(mfmg_hip_high_order_t p, const double *b, double *x)
{
  return guarded([&] {
    require(p && b && x, "null argument");
    require(b != x, "b and x must be two vectors");
    HipHandle &handle = *p->hierarchy->handle;
    const int64_t n = p->prec->size();
    DVector bv(handle, n, const_cast<double *>(b)), xv(handle, n, x);
    p->prec->apply(bv, xv);
  });
}

int mfmg_hip_high_order_smoother_info(mfmg_hip_high_order_t p, int32_t *degree, double *lambda_min, double *lambda_max)
{
  return guarded([&] {
    require(p && degree && lambda_min && lambda_max, "null argument");
    HipSmoother const *s = p->prec->smoother();
    *degree = s ? s->degree() : 0;
    *lambda_min = s ? s->lambda_min() : 0.;
    *lambda_max = s ? s->lambda_max() : 0.;
  });
}

int mfmg_hip_high_order_solve_cg(mfmg_hip_high_order_t p, const double *b, double *x, double tolerance, int32_t max_iterations,
                                 int32_t *n_iterations, double *final_residual, double *residual_history, int32_t history_len)
{
  return guarded([&] {
    require(p && b && x, "null argument");
    require(tolerance >= 0. && max_iterations >= 0, "bad stopping criterion");
    const KrylovResult result = solve_cg(high_order_setting(p), b, x, tolerance, max_iterations, residual_history, history_len);
    deliver_result(result, n_iterations, final_residual, nullptr);
    if (!result.all_converged())
      throw std::runtime_error("CG did not reach the tolerance within max_iterations (SolverControl::NoConvergence)");
  });
}

int mfmg_hip_high_order_solve_fgmres(mfmg_hip_high_order_t p, const double *b, double *x, double tolerance, int32_t max_iterations,
                                     int32_t restart, int32_t *n_iterations, double *final_residual, double *residual_history,
                                     int32_t history_len)
{
  return guarded([&] {
    require(p && b && x, "null argument");
    require(tolerance >= 0. && max_iterations >= 0, "bad stopping criterion");
    require(restart >= 1, "the restart length must be at least 1");
    const KrylovResult result =
      solve_fgmres(high_order_setting(p), b, x, tolerance, max_iterations, restart, false, residual_history, history_len);
    deliver_result(result, n_iterations, final_residual, nullptr);
    if (!result.all_converged())
      throw std::runtime_error("FGMRES did not reach the tolerance within max_iterations (SolverControl::NoConvergence)");
  });
}

int mfmg_hip_high_order_solve_cg_block(mfmg_hip_high_order_t p, int32_t n_vectors, int64_t ld, const double *b, double *x,
                                       const double *tolerances, int32_t max_iterations)
{
  return guarded([&] {
    require(p && b && x && tolerances, "null argument");
    (void)solve_cg_block(high_order_setting(p), n_vectors, ld, b, x, tolerances, max_iterations, nullptr, 0);
  });
}

int mfmg_hip_high_order_solve_fgmres_block(mfmg_hip_high_order_t p, int32_t n_vectors, int64_t ld, const double *b, double *x,
                                           const double *tolerances, int32_t max_iterations, int32_t restart)
{
  return guarded([&] {
    require(p && b && x && tolerances, "null argument");
    (void)solve_fgmres_block(high_order_setting(p), n_vectors, ld, b, x, tolerances, max_iterations, restart, false, nullptr, 0);
  });
}

// ---- host-side setup pieces -------------------------------------------------------------
extern "C++"
{
namespace
{
StructuredMesh host_mesh(const mfmg_hip_mesh_desc *mesh)
{
  require(mesh != nullptr, "null mesh");
  require(mesh->arrays_on_device == 0, "the host entry points need host arrays");
  return StructuredMesh::from_desc(*mesh, nullptr);
}
} // namespace
}

int mfmg_hip_host_csr_shape(mfmg_hip_host_csr_t m, int64_t *n_rows, int64_t *n_cols, int64_t *nnz)
{
  return guarded([&] {
    require(m != nullptr, "null matrix");
    if (n_rows)
      *n_rows = m->m.n_rows;
    if (n_cols)
      *n_cols = m->m.n_cols;
    if (nnz)
      *nnz = m->m.nnz();
  });
}

int mfmg_hip_host_csr_get(mfmg_hip_host_csr_t m, int32_t *row_ptr, int32_t *col, double *val)
{
  return guarded([&] {
    require(m && row_ptr, "null argument");
    std::memcpy(row_ptr, m->m.row_ptr.data(), m->m.row_ptr.size() * sizeof(int32_t));
    if (m->m.nnz() > 0)
    {
      require(col && val, "null column / value array");
      std::memcpy(col, m->m.col.data(), m->m.col.size() * sizeof(int32_t));
      std::memcpy(val, m->m.val.data(), m->m.val.size() * sizeof(double));
    }
  });
}

int mfmg_hip_host_csr_destroy(mfmg_hip_host_csr_t m)
{
  return guarded([&] { delete m; });
}

int mfmg_hip_host_assemble_matrix(const mfmg_hip_mesh_desc *mesh, int semantics, mfmg_hip_host_csr_t *out)
{
  return guarded([&] {
    require(out != nullptr, "null output handle");
    require(semantics == 0 || semantics == 1, "unknown constraint semantics");
    auto sm = host_mesh(mesh);
    auto h = new mfmg_hip_host_csr_s;
    h->m = assemble_global_matrix(sm, semantics == 0 ? ConstraintSemantics::assembled
                                                     : ConstraintSemantics::matrix_free);
    *out = h;
  });
}

int mfmg_hip_host_build_restrictor(const mfmg_hip_mesh_desc *mesh, const char *params_info, int matrix_free,
                                   mfmg_hip_host_csr_t *out)
{
  return guarded([&] {
    require(out != nullptr, "null output handle");
    auto sm = host_mesh(mesh);
    ptree params = ptree::parse_info(params_info ? params_info : "");
    RestrictorOptions o;
    o.agglomerate[0] = params.get("agglomeration.nx", 2);
    o.agglomerate[1] = params.get("agglomeration.ny", 2);
    o.agglomerate[2] = params.get("agglomeration.nz", 2);
    o.n_eigenvectors = params.get("eigensolver.number of eigenvectors", 1);
    o.variant = params.get("eigensolver.variant", matrix_free ? "mf" : "device");
    o.selection = params.get("eigensolver.selection", "krylov");
    o.use_coefficient = params.get("eigensolver.use_coefficient", true);
    auto diag = operator_diagonal(sm, matrix_free ? ConstraintSemantics::matrix_free : ConstraintSemantics::assembled);
    auto h = new mfmg_hip_host_csr_s;
    h->m = build_restrictor_structured(sm, diag, o);
    *out = h;
  });
}

int mfmg_hip_host_galerkin(const mfmg_hip_mesh_desc *mesh, int semantics, int64_t n_rows, int64_t nnz,
                           const int32_t *r_row_ptr, const int32_t *r_col, const double *r_val,
                           mfmg_hip_host_csr_t *out)
{
  return guarded([&] {
    require(out && r_row_ptr && r_col && r_val, "null argument");
    require(semantics == 0 || semantics == 1, "unknown constraint semantics");
    auto sm = host_mesh(mesh);
    HostCsr R, Rt;
    R.n_rows = n_rows;
    R.n_cols = sm.n_dofs;
    R.row_ptr.assign(r_row_ptr, r_row_ptr + n_rows + 1);
    require(R.row_ptr[n_rows] == nnz, "row_ptr[n_rows] != nnz");
    R.col.assign(r_col, r_col + nnz);
    R.val.assign(r_val, r_val + nnz);
    Rt.n_rows = R.n_cols;
    Rt.n_cols = R.n_rows;
    csr_transpose_host<double>(R.n_rows, R.n_cols, R.row_ptr, R.col, R.val, Rt.row_ptr, Rt.col, Rt.val);
    auto h = new mfmg_hip_host_csr_s;
    h->m = galerkin_triple_product(
        sm, semantics == 0 ? ConstraintSemantics::assembled : ConstraintSemantics::matrix_free, R, Rt);
    *out = h;
  });
}

int mfmg_hip_host_amg_build(int64_t n_rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col, const double *val,
                            const double *near_null, const int32_t *grid_dims, const int32_t *node_of_row,
                            const int32_t *component_of_row, const char *params_info, mfmg_hip_host_amg_t *out)
{
  return guarded([&] {
    require(row_ptr && col && val && out, "null argument");
    HostCsr A;
    A.n_rows = A.n_cols = n_rows;
    A.row_ptr.assign(row_ptr, row_ptr + n_rows + 1);
    require(A.row_ptr[n_rows] == nnz, "row_ptr[n_rows] != nnz");
    A.col.assign(col, col + nnz);
    A.val.assign(val, val + nnz);
    std::vector<double> b0 = near_null ? std::vector<double>(near_null, near_null + n_rows)
                                       : std::vector<double>(n_rows, 1.);
    ptree params = ptree::parse_info(params_info ? params_info : "");
    AmgOptions opts;
    opts.max_levels = params.get("solver.amg.max_levels", 10);
    opts.coarsest_size = params.get("solver.amg.coarsest_size", 1100);
    opts.strength = params.get("solver.amg.strength", 0.08);
    opts.smooth_prolongator = params.get("solver.amg.smooth_prolongator", true);
    AmgGridHint grid;
    if (grid_dims && node_of_row)
    {
      for (int d = 0; d < 3; ++d)
        grid.dims[d] = grid_dims[d];
      grid.node_of_row.assign(node_of_row, node_of_row + n_rows);
      const int blk = params.get("solver.amg.aggregate_block", 2);
      require(blk >= 2 && blk <= 8, "solver.amg.aggregate_block must be in 2..8");
      for (int d = 0; d < 3; ++d)
        grid.block[d] = blk;
      if (component_of_row)
      {
        grid.component_of_row.assign(component_of_row, component_of_row + n_rows);
        for (auto c : grid.component_of_row)
          grid.n_components = std::max(grid.n_components, c + 1);
      }
    }
    auto h = new mfmg_hip_host_amg_s;
    h->levels = build_aggregation_hierarchy(std::move(A), std::move(b0), opts, grid.valid(n_rows) ? &grid : nullptr);
    *out = h;
  });
}

int mfmg_hip_host_amg_n_levels(mfmg_hip_host_amg_t amg, int32_t *n_levels)
{
  return guarded([&] {
    require(amg && n_levels, "null argument");
    *n_levels = (int32_t)amg->levels.size();
  });
}

int mfmg_hip_host_amg_get(mfmg_hip_host_amg_t amg, int32_t level, int32_t which, mfmg_hip_host_csr_t *out)
{
  return guarded([&] {
    require(amg && out, "null argument");
    require(level >= 0 && level < (int)amg->levels.size(), "level out of range");
    require(which == 0 || which == 1, "which must be 0 (A) or 1 (P)");
    auto h = new mfmg_hip_host_csr_s;
    h->m = which == 0 ? amg->levels[level].A : amg->levels[level].P;
    *out = h;
  });
}

int mfmg_hip_host_amg_destroy(mfmg_hip_host_amg_t amg)
{
  return guarded([&] { delete amg; });
}

int mfmg_hip_host_params_get(const char *params_info, const char *path, char *value_buf, size_t buf_size)
{
  return guarded([&] {
    require(params_info && path && value_buf && buf_size > 0, "null argument");
    ptree params = ptree::parse_info(params_info);
    std::string v = params.get<std::string>(path);
    std::strncpy(value_buf, v.c_str(), buf_size - 1);
    value_buf[buf_size - 1] = '\0';
  });
}

} // extern "C"
