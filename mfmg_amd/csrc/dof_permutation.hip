// DoF permutation between the caller's numbering and the internal lexicographic one (dof_permutation.hpp).
//
// The kernel.  Per DoF and vector one value is read, one written and one id read (20 B in FP64); one side of the copy is
// contiguous, the other is indexed.  For deal.II's numbering (cells in Morton order, vertex DoFs at first touch) a lexicographic
// x-row of 64 nodes touches ~48 different 64-byte pieces of the caller's vector, a 4 x 4 x 4 brick ~30: the lines are shared with
// the rows above and below, so reuse has to come from the shape of what one workgroup covers.  Two iteration orders:
//   lexicographic  a workgroup of 256 threads covers a BRICK of nodes; the internal side is contiguous (16-byte accesses, ids
//                  read as int2 / int4), the caller's side is indexed.  Bricks: 64 x 8 x 4 nodes ("brick64") or 16 x 8 x 16
//                  ("brick16"; FP32, four nodes per thread: 64 x 16 x 4 and 16 x 16 x 16).
//   caller ids     a workgroup covers 2048 (FP32: 4096) CONSECUTIVE caller ids; the caller's side is contiguous, the internal side
//                  is indexed through the inverse map ("ids").
// Every thread owns U = 4 independent groups of 16 bytes (four layers of its brick, resp. four chunks of its block): it issues the
// id loads of all of them, then all indexed accesses, then the stores -- 8 (FP32: 16) indexed requests in flight per thread.
// Rows of the node grid have odd length, so a group is 16 ALIGNED bytes of the linear vector: row r owns the groups whose first
// element lies in it, which partitions the groups exactly; a group that hangs over the end of its row takes the first node of the
// next one with it.  No atomics; lanes differ only at the tails (rows, bricks, the last group of the vector).
// A vector that is not 16-byte aligned on the contiguous side takes the instance with one element per group.
// MFMG_DOF_PERMUTATION = brick64 | brick16 | ids selects (read when the context is created).  Default: ids -- at 257^3 DoFs in
// deal.II's numbering gather + scatter take 106 + 83 us against 98 + 140 (brick64) and 115 + 135 (brick16); a random permutation
// costs 350-450 us per launch in every variant (one line per lane).  Measurements: DESIGN.md 6.
#include <type_traits>

#include "dof_permutation.hpp"

namespace mfmg
{
namespace
{
// ---- setup: node -> DoF from cell_dofs, validated ------------------------------------------------
struct GridDesc
{
  int dim;
  int n[3]; // cells
  int N[3]; // nodes
  int64_t n_dofs, n_cells;
};

// node n reads its id from the cell below-left of it (clamped into the mesh); ids out of range count as bad and leave -1
__global__ void perm_node_dof_kernel(GridDesc g, int32_t const *cell_dofs, int32_t *node_dof, int *n_bad)
{
  const int nc = 1 << g.dim;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < g.n_dofs; t += (int64_t)gridDim.x * blockDim.x)
  {
    const int i = (int)(t % g.N[0]), j = (int)((t / g.N[0]) % g.N[1]), k = (int)(t / ((int64_t)g.N[0] * g.N[1]));
    const int ic = min(i, g.n[0] - 1), jc = min(j, g.n[1] - 1), kc = g.dim == 3 ? min(k, g.n[2] - 1) : 0;
    const int64_t c = ic + (int64_t)g.n[0] * (jc + (int64_t)g.n[1] * kc);
    const int m = (i - ic) + 2 * (j - jc) + 4 * (k - kc);
    const int32_t id = cell_dofs[c * nc + m];
    if (id < 0 || id >= g.n_dofs)
    {
      atomicAdd(n_bad, 1);
      node_dof[t] = -1;
    }
    else
      node_dof[t] = id;
  }
}

// every corner of every cell carries the id of its node
__global__ void perm_check_cells_kernel(GridDesc g, int32_t const *cell_dofs, int32_t const *node_dof, int *n_bad)
{
  const int nc = 1 << g.dim;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < g.n_cells * nc; t += (int64_t)gridDim.x * blockDim.x)
  {
    const int64_t c = t / nc;
    const int m = (int)(t % nc);
    const int i = (int)(c % g.n[0]) + (m & 1), j = (int)((c / g.n[0]) % g.n[1]) + ((m >> 1) & 1),
              k = (int)(c / ((int64_t)g.n[0] * g.n[1])) + ((m >> 2) & 1);
    if (cell_dofs[t] != node_dof[i + (int64_t)g.N[0] * (j + (int64_t)g.N[1] * k)])
      atomicAdd(n_bad, 1);
  }
}

// dof_node[node_dof[n]] = n (all ids are in range here; of two nodes with one id one wins and the check below finds the other)
__global__ void perm_invert_kernel(int64_t n, int32_t const *node_dof, int32_t *dof_node)
{
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
    dof_node[node_dof[t]] = (int32_t)t;
}

// counts[0]: nodes whose id is taken by another node; counts[1]: nodes whose id is not their index
__global__ void perm_check_inverse_kernel(int64_t n, int32_t const *node_dof, int32_t const *dof_node, int *counts)
{
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
  {
    const int32_t id = node_dof[t];
    if (dof_node[id] != (int32_t)t)
      atomicAdd(counts, 1);
    if (id != (int32_t)t)
      atomicAdd(counts + 1, 1);
  }
}

// the mesh in the lexicographic numbering
__global__ void perm_lex_cell_dofs_kernel(GridDesc g, int32_t *cell_dofs)
{
  const int nc = 1 << g.dim;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < g.n_cells * nc; t += (int64_t)gridDim.x * blockDim.x)
  {
    const int64_t c = t / nc;
    const int m = (int)(t % nc);
    const int i = (int)(c % g.n[0]) + (m & 1), j = (int)((c / g.n[0]) % g.n[1]) + ((m >> 1) & 1),
              k = (int)(c / ((int64_t)g.n[0] * g.n[1])) + ((m >> 2) & 1);
    cell_dofs[t] = (int32_t)(i + (int64_t)g.N[0] * (j + (int64_t)g.N[1] * k));
  }
}

__global__ void perm_lex_constrained_kernel(int64_t n, int32_t const *node_dof, uint8_t const *constrained, uint8_t *constrained_lex)
{
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
    constrained_lex[t] = constrained[node_dof[t]];
}

// ---- the permutation ----------------------------------------------------------------------------
constexpr int kUnroll = 4; // groups per thread

struct PermGeom
{
  int64_t n;  // DoFs
  int64_t N0; // row length of the iteration space (the node grid; n for blocks of consecutive ids)
  int N1, N2; // rows per layer, layers
  int bpx_log2, by_log2, bzt; // 256 threads = 2^bpx_log2 groups along the row x 2^by_log2 rows x bzt layers
  int unroll_x; // the kUnroll groups of a thread: consecutive chunks of its row (1) or consecutive layers (0)
};

template <typename T, int V>
struct Group;
template <typename T>
struct Group<T, 1>
{
  using value = T;
  using index = int32_t;
};
template <>
struct Group<double, 2>
{
  using value = double2;
  using index = int2;
};
template <>
struct Group<float, 4>
{
  using value = float4;
  using index = int4;
};

// V elements from `first`; beyond n: index -1, value 0 (the last group of the vector only)
template <int V>
__device__ __forceinline__ void load_ids(int32_t const *__restrict__ map, int64_t first, int64_t n, int32_t (&id)[V])
{
  if (first + V <= n)
  {
    using I = typename Group<typename std::conditional<V == 2, double, float>::type, V>::index;
    const I v = *reinterpret_cast<I const *>(map + first);
    int32_t const *e = reinterpret_cast<int32_t const *>(&v);
#pragma unroll
    for (int q = 0; q < V; ++q)
      id[q] = e[q];
  }
  else
  {
#pragma unroll
    for (int q = 0; q < V; ++q)
      id[q] = first + q < n ? map[first + q] : -1;
  }
}
template <typename T, int V>
__device__ __forceinline__ void load_values(T const *__restrict__ src, int64_t first, int64_t n, T (&v)[V])
{
  if (first + V <= n)
  {
    using G = typename Group<T, V>::value;
    const G g = *reinterpret_cast<G const *>(src + first);
    T const *e = reinterpret_cast<T const *>(&g);
#pragma unroll
    for (int q = 0; q < V; ++q)
      v[q] = e[q];
  }
  else
  {
#pragma unroll
    for (int q = 0; q < V; ++q)
      v[q] = first + q < n ? src[first + q] : T(0);
  }
}
template <typename T, int V>
__device__ __forceinline__ void store_values(T *__restrict__ dst, int64_t first, int64_t n, T const (&v)[V])
{
  if (first + V <= n)
  {
    using G = typename Group<T, V>::value;
    G g;
    T *e = reinterpret_cast<T *>(&g);
#pragma unroll
    for (int q = 0; q < V; ++q)
      e[q] = v[q];
    *reinterpret_cast<G *>(dst + first) = g;
  }
  else
  {
#pragma unroll
    for (int q = 0; q < V; ++q)
      if (first + q < n)
        dst[first + q] = v[q];
  }
}

// WRITE false: dst[i] = src[map[i]]; true: dst[map[i]] = src[i], i over the iteration space; TWO: the same for a second pair of
// vectors with the ids of the first.  `map` is a permutation of [0, n) (checked when it was built).
template <typename T, int V, bool WRITE, bool TWO>
__global__ __launch_bounds__(256) void dof_permutation_kernel(PermGeom g, int32_t const *__restrict__ map, T const *__restrict__ src0,
                                                              T *__restrict__ dst0, T const *__restrict__ src1, T *__restrict__ dst1)
{
  const int t = threadIdx.x;
  const int bpx = 1 << g.bpx_log2, by = 1 << g.by_log2;
  const int lx = t & (bpx - 1), ly = (t >> g.bpx_log2) & (by - 1), lz = t >> (g.bpx_log2 + g.by_log2);
  const int j = blockIdx.y * by + ly;
  int64_t first[kUnroll];
  bool ok[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u)
  {
    const int64_t layer = (int64_t)blockIdx.z * g.bzt + lz;
    const int64_t k = g.unroll_x ? layer : layer * kUnroll + u;
    const int64_t cx = g.unroll_x ? (int64_t)blockIdx.x * kUnroll + u : (int64_t)blockIdx.x;
    const int64_t r = j + (int64_t)g.N1 * k;
    // the groups whose first element lies in row r
    const int64_t begin = (g.N0 * r + V - 1) / V, end = (g.N0 * (r + 1) + V - 1) / V;
    const int64_t p = begin + cx * bpx + lx;
    ok[u] = j < g.N1 && k < g.N2 && p < end;
    first[u] = p * V;
  }
  int32_t id[kUnroll][V];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u)
    if (ok[u])
      load_ids<V>(map, first[u], g.n, id[u]);
  T v0[kUnroll][V], v1[kUnroll][V];
  if (!WRITE)
  {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (ok[u])
      {
#pragma unroll
        for (int q = 0; q < V; ++q)
        {
          v0[u][q] = id[u][q] >= 0 ? src0[id[u][q]] : T(0);
          if (TWO)
            v1[u][q] = id[u][q] >= 0 ? src1[id[u][q]] : T(0);
        }
      }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (ok[u])
      {
        store_values<T, V>(dst0, first[u], g.n, v0[u]);
        if (TWO)
          store_values<T, V>(dst1, first[u], g.n, v1[u]);
      }
  }
  else
  {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (ok[u])
      {
        load_values<T, V>(src0, first[u], g.n, v0[u]);
        if (TWO)
          load_values<T, V>(src1, first[u], g.n, v1[u]);
      }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (ok[u])
      {
#pragma unroll
        for (int q = 0; q < V; ++q)
          if (id[u][q] >= 0)
          {
            dst0[id[u][q]] = v0[u][q];
            if (TWO)
              dst1[id[u][q]] = v1[u][q];
          }
      }
  }
}

int log2_exact(int v)
{
  int l = 0;
  while ((1 << l) < v)
    ++l;
  return l;
}

bool aligned16(void const *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename T, int V>
void launch_instance(hipStream_t st, dim3 grid, bool write, bool two, PermGeom const &g, int32_t const *map, T const *s0, T *d0, T const *s1, T *d1)
{
  if (write)
  {
    if (two)
      hipLaunchKernelGGL((dof_permutation_kernel<T, V, true, true>), grid, dim3(256), 0, st, g, map, s0, d0, s1, d1);
    else
      hipLaunchKernelGGL((dof_permutation_kernel<T, V, true, false>), grid, dim3(256), 0, st, g, map, s0, d0, s1, d1);
  }
  else
  {
    if (two)
      hipLaunchKernelGGL((dof_permutation_kernel<T, V, false, true>), grid, dim3(256), 0, st, g, map, s0, d0, s1, d1);
    else
      hipLaunchKernelGGL((dof_permutation_kernel<T, V, false, false>), grid, dim3(256), 0, st, g, map, s0, d0, s1, d1);
  }
}
} // namespace

DofPermutation::DofPermutation(HipHandle &handle, mfmg_hip_mesh_desc const &mesh) : _handle(handle), _lex(mesh)
{
  ASSERT_THROW(mesh.dim == 2 || mesh.dim == 3, "mesh dimension must be 2 or 3");
  ASSERT_THROW(mesh.cell_dofs && mesh.coefficient && mesh.constrained, "mesh description arrays must not be null");
  GridDesc g;
  g.dim = mesh.dim;
  g.n_dofs = g.n_cells = 1;
  for (int d = 0; d < 3; ++d)
  {
    if (d < mesh.dim)
      ASSERT_THROW(mesh.n_cells[d] >= 1, "n_cells must be positive");
    g.n[d] = d < mesh.dim ? mesh.n_cells[d] : 1;
    g.N[d] = d < mesh.dim ? g.n[d] + 1 : 1;
    g.n_cells *= g.n[d];
    g.n_dofs *= g.N[d];
    _N[d] = g.N[d];
  }
  ASSERT_THROW(g.n_dofs == mesh.n_dofs, "n_dofs does not match the cell grid (Q1: prod(n_cells+1))");
  ASSERT_THROW(g.n_dofs < (int64_t(1) << 31), "DoF ids are 32-bit");
  _n = g.n_dofs;
  hipStream_t st = handle.stream;
  const int nc = 1 << g.dim;
  const size_t n_cd = (size_t)g.n_cells * nc;
  // the caller's cell_dofs and constrained on the device
  DeviceBuffer<int32_t> cd_tmp;
  DeviceBuffer<uint8_t> con_tmp;
  int32_t const *cd = mesh.cell_dofs;
  uint8_t const *con = mesh.constrained;
  if (!mesh.arrays_on_device)
  {
    cd_tmp.upload(mesh.cell_dofs, n_cd, st);
    con_tmp.upload(mesh.constrained, (size_t)_n, st);
    cd = cd_tmp.data();
    con = con_tmp.data();
  }
  DeviceBuffer<int> counts(2);
  MFMG_HIP_CHECK(hipMemsetAsync(counts.data(), 0, 2 * sizeof(int), st));
  _node_dof.resize((size_t)_n);
  const dim3 grid_n(n_blocks_for(_n, 256, 1 << 16)), grid_c(n_blocks_for((int64_t)n_cd, 256, 1 << 16));
  hipLaunchKernelGGL(perm_node_dof_kernel, grid_n, dim3(256), 0, st, g, cd, _node_dof.data(), counts.data());
  hipLaunchKernelGGL(perm_check_cells_kernel, grid_c, dim3(256), 0, st, g, cd, _node_dof.data(), counts.data());
  MFMG_HIP_CHECK(hipGetLastError());
  int bad = counts.download(st)[0];
  if (bad == 0)
  {
    // (only now: every id is in range)
    _dof_node.resize((size_t)_n);
    MFMG_HIP_CHECK(hipMemsetAsync(_dof_node.data(), 0xff, (size_t)_n * sizeof(int32_t), st));
    hipLaunchKernelGGL(perm_invert_kernel, grid_n, dim3(256), 0, st, _n, _node_dof.data(), _dof_node.data());
    hipLaunchKernelGGL(perm_check_inverse_kernel, grid_n, dim3(256), 0, st, _n, _node_dof.data(), _dof_node.data(), counts.data());
    MFMG_HIP_CHECK(hipGetLastError());
    const std::vector<int> c = counts.download(st);
    bad = c[0];
    _identity = c[1] == 0;
  }
  ASSERT_THROW(bad == 0, "cell_dofs is not a logically structured Q1 mesh in lexicographic cell order (" + std::to_string(bad) +
                             " inconsistencies)");
  if (_identity)
  {
    _node_dof.release();
    _dof_node.release();
    return; // the caller's description is the lexicographic one
  }
  _node_dof_host = _node_dof.download(st);
  _lex_cell_dofs.resize(n_cd);
  _lex_constrained.resize((size_t)_n);
  hipLaunchKernelGGL(perm_lex_cell_dofs_kernel, grid_c, dim3(256), 0, st, g, _lex_cell_dofs.data());
  hipLaunchKernelGGL(perm_lex_constrained_kernel, grid_n, dim3(256), 0, st, _n, _node_dof.data(), con, _lex_constrained.data());
  MFMG_HIP_CHECK(hipGetLastError());
  if (mesh.arrays_on_device)
  {
    _lex.cell_dofs = _lex_cell_dofs.data();
    _lex.constrained = _lex_constrained.data();
    MFMG_HIP_CHECK(hipStreamSynchronize(st));
  }
  else
  {
    // the coefficients stay where the caller has them, so the two computed arrays follow them to the host
    _lex_cell_dofs_host = _lex_cell_dofs.download(st);
    _lex_constrained_host = _lex_constrained.download(st);
    _lex_cell_dofs.release();
    _lex_constrained.release();
    _lex.cell_dofs = _lex_cell_dofs_host.data();
    _lex.constrained = _lex_constrained_host.data();
  }
}

void DofPermutation::release_mesh()
{
  _lex_cell_dofs.release();
  _lex_constrained.release();
  std::vector<int32_t>().swap(_lex_cell_dofs_host);
  std::vector<uint8_t>().swap(_lex_constrained_host);
  _lex.cell_dofs = nullptr;
  _lex.constrained = nullptr;
  _lex.coefficient = nullptr;
}

template <typename T>
void DofPermutation::launch(bool to_lex, int n_vectors, T const *in0, T *out0, T const *in1, T *out1) const
{
  ASSERT_THROW(!_identity, "internal: a lexicographic numbering is not permuted");
  ASSERT_THROW(in0 != nullptr && out0 != nullptr && (n_vectors == 1 || (in1 != nullptr && out1 != nullptr)), "null vector");
  ASSERT_THROW(static_cast<void const *>(in0) != static_cast<void const *>(out0), "the permutation does not work in place");
  const int variant = _handle.dof_permutation_kernel;
  const bool by_ids = variant == 2;
  // the iteration runs over lexicographic nodes (map: node -> DoF) or over caller ids (map: DoF -> node); the vector on the
  // other side of the map is the indexed one.  to_lex: out_lex[n] = in[node_dof[n]], i.e. out[dof_node[g]] = in[g]
  const bool write = to_lex ? by_ids : !by_ids;
  int32_t const *map = by_ids ? _dof_node.data() : _node_dof.data();
  // the contiguous side: what is read in a writing launch, written in a reading one
  const bool vectors_aligned = write ? (aligned16(in0) && (n_vectors == 1 || aligned16(in1)))
                                     : (aligned16(out0) && (n_vectors == 1 || aligned16(out1)));
  constexpr int VT = 16 / (int)sizeof(T);
  const int V = vectors_aligned ? VT : 1;
  PermGeom g;
  g.n = _n;
  int bx_nodes, bzt;
  if (by_ids)
  {
    g.N0 = _n;
    g.N1 = g.N2 = 1;
    bx_nodes = 256 * V;
    bzt = 1;
    g.unroll_x = 1;
  }
  else
  {
    g.N0 = _N[0];
    g.N1 = _N[1];
    g.N2 = _N[2];
    bx_nodes = variant == 1 ? 16 : 64;
    bzt = variant == 1 ? 4 : 1;
    g.unroll_x = 0;
    if (g.N2 == 1)
    {
      // 2-D: no layers to spread the groups of a thread over
      bzt = 1;
      g.unroll_x = 1;
    }
  }
  const int bpx = std::min(256, bx_nodes / V);
  const int by = by_ids ? 1 : 256 / (bpx * bzt);
  g.bpx_log2 = log2_exact(bpx);
  g.by_log2 = log2_exact(by);
  g.bzt = bzt;
  const int64_t groups_per_row = (g.N0 + V - 1) / V + 1; // (a row may own one group more than N0 / V)
  const int64_t chunks = (groups_per_row + bpx - 1) / bpx;
  const int64_t gx = g.unroll_x ? (chunks + kUnroll - 1) / kUnroll : chunks;
  const int64_t gy = (g.N1 + by - 1) / by;
  const int64_t layers_per_block = (int64_t)bzt * (g.unroll_x ? 1 : kUnroll);
  const int64_t gz = (g.N2 + layers_per_block - 1) / layers_per_block;
  ASSERT_THROW(gx < (int64_t(1) << 31) && gy < 65536 && gz < 65536, "mesh too large for the DoF permutation kernel");
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)gz);
  hipStream_t st = _handle.stream;
  hipEvent_t stop = _handle.profiler.begin("dof_permutation", double(n_vectors) * (2. * sizeof(T) + 4.) * double(_n), st);
  const bool two = n_vectors == 2;
  if (V == 1)
    launch_instance<T, 1>(st, grid, write, two, g, map, in0, out0, in1, out1);
  else
    launch_instance<T, VT>(st, grid, write, two, g, map, in0, out0, in1, out1);
  MFMG_HIP_CHECK(hipGetLastError());
  KernelProfiler::end(stop, st);
}

template <typename T>
void DofPermutation::gather(T const *in_caller, T *out_lex) const
{
  launch<T>(true, 1, in_caller, out_lex, nullptr, nullptr);
}
template <typename T>
void DofPermutation::gather2(T const *b_caller, T const *x_caller, T *b_lex, T *x_lex) const
{
  launch<T>(true, 2, b_caller, b_lex, x_caller, x_lex);
}
template <typename T>
void DofPermutation::scatter(T const *in_lex, T *out_caller) const
{
  launch<T>(false, 1, in_lex, out_caller, nullptr, nullptr);
}

template void DofPermutation::gather<double>(double const *, double *) const;
template void DofPermutation::gather<float>(float const *, float *) const;
template void DofPermutation::gather2<double>(double const *, double const *, double *, double *) const;
template void DofPermutation::gather2<float>(float const *, float const *, float *, float *) const;
template void DofPermutation::scatter<double>(double const *, double *) const;
template void DofPermutation::scatter<float>(float const *, float *) const;
} // namespace mfmg
