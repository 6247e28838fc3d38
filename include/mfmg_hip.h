/*
 * mfmg_hip.h -- C ABI of libmfmg_hip.so: the MI355X (gfx950) drop-in for the
 * V-cycle apply path of ORNL-CEES/mfmg.
 *
 * The reference exposes this path through C++ abstract classes
 * (include/mfmg/common/{operator,smoother,solver,hierarchy}.hpp), selected by the
 * string switch create_hierarchy_helpers (include/mfmg/common/hierarchy.hpp:49-153).
 * The same classes are mirrored, deal.II-free, under mfmg_amd/csrc/mfmg/ ; this
 * header is the flat boundary underneath them: plain pointers and sizes, device
 * pointers in, status code out, no C++/torch types.  Every entry point cites the
 * reference interface it replaces (path:line relative to the reference tree).
 *
 * Conventions
 *  - all vectors are raw DEVICE pointers to `double` (or `float` for the _f32
 *    entry points) of the length the operator reports; the caller owns them;
 *  - matrices / operators / hierarchies are opaque handles that OWN their
 *    device arrays (as SparseMatrixDevice does,
 *    include/mfmg/cuda/sparse_matrix_device.templates.cuh:244-272);
 *  - every call is asynchronous on the context's HIP stream unless stated;
 *  - return value: MFMG_HIP_SUCCESS or an error code; the message of the last
 *    error on the calling thread is available from mfmg_hip_last_error().
 *    MFMG_HIP_ERROR_RUNTIME      <-> ASSERT_THROW  (std::runtime_error,
 *                                    include/mfmg/common/exceptions.hpp:48-52)
 *    MFMG_HIP_ERROR_NOT_IMPLEMENTED <-> ASSERT_THROW_NOT_IMPLEMENTED (:54-73)
 */
#ifndef MFMG_HIP_H
#define MFMG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header: bumped whenever an entry point changes its signature or disappears; additions leave it.
 *   1  rounds 1-2 up to the host-callback halo exchange (mfmg_hip_context_set_halo_buffers)
 *   2  round 2: mfmg_hip_context_set_communicator(ctx, rank, n_ranks, ghost_low, ghost_high) replaces the old signature,
 *      mfmg_hip_context_set_halo_buffers removed (transports: mfmg_hip_context_use_rccl / _use_host_transport)
 *      (round 3 added mfmg_hip_hierarchy_ap_apply, mfmg_hip_rccl_available, mfmg_hip_abi_version: no change of the version)
 *   3  round 3: box decomposition -- mfmg_hip_host_exchange_fn (any number of partner ranks per call) replaces
 *      mfmg_hip_host_sendrecv_fn (rank -+ 1); added mfmg_hip_context_set_communicator_box, mfmg_hip_context_halo_box,
 *      mfmg_hip_context_exchange_volume
 *      (later in round 3 added mfmg_hip_context_use_reflecting_transport: no change of the version)
 *      (added mfmg_hip_hierarchy_coarse_amg_setup_info and which = 3 of mfmg_hip_hierarchy_coarse_amg_get: additions, no change
 *      of the version)
 * mfmg_hip_abi_version() returns the value the loaded library was built with. */
#define MFMG_HIP_ABI_VERSION 3

#define MFMG_HIP_SUCCESS 0
#define MFMG_HIP_ERROR_RUNTIME 1
#define MFMG_HIP_ERROR_NOT_IMPLEMENTED 2
#define MFMG_HIP_ERROR_INVALID_ARGUMENT 3
#define MFMG_HIP_ERROR_DEVICE 4

/* OperatorMode (include/mfmg/common/operator.hpp:19-23) */
#define MFMG_HIP_NO_TRANS 0
#define MFMG_HIP_TRANS 1
/* restrictor_apply only: out -= R^T in (Operator::apply_subtract, the form the cycle uses) */
#define MFMG_HIP_TRANS_SUBTRACT 2

typedef struct mfmg_hip_context_s *mfmg_hip_context_t;       /* CudaHandle, include/mfmg/cuda/cuda_handle.cuh:25-48 */
typedef struct mfmg_hip_csr_s *mfmg_hip_csr_t;               /* SparseMatrixDevice<double>, include/mfmg/cuda/sparse_matrix_device.cuh:28-104 */
typedef struct mfmg_hip_mf_laplace_s *mfmg_hip_mf_laplace_t; /* CudaMatrixFreeOperator + the user's LaplaceOperator, source/cuda/cuda_matrix_free_operator.cu:32-37, tests/laplace_matrix_free.hpp:121-156 */
typedef struct mfmg_hip_hierarchy_s *mfmg_hip_hierarchy_t;   /* Hierarchy<VectorType>, include/mfmg/common/hierarchy.hpp:155-373 */

const char *mfmg_hip_last_error(void);
const char *mfmg_hip_version(void);
int mfmg_hip_abi_version(void);
/* What the device memory of the library is spent on right now: one line per (setup section of the reference's TimerOutput |
 * kind of structure) with at least 1 MB live -- "Setup: build restrictor | CSR arrays (val, col, row_ptr)", ... -- and the total,
 * as text (GB).  Process-wide (all contexts). */
int mfmg_hip_memory_inventory(char *buffer, size_t buffer_size);

/* ---- context: stream + scratch (CudaHandle, source/cuda/cuda_handle.cu:17-56) ---- */
/* `hip_stream`: a hipStream_t borrowed from the caller; NULL = the legacy default stream (what the
 * reference runs on); MFMG_HIP_OWN_STREAM = the library creates and owns a non-blocking stream. */
#define MFMG_HIP_OWN_STREAM ((void *)(intptr_t)-1)
int mfmg_hip_context_create(void *hip_stream, mfmg_hip_context_t *ctx);
int mfmg_hip_context_destroy(mfmg_hip_context_t ctx);
int mfmg_hip_context_synchronize(mfmg_hip_context_t ctx);
void *mfmg_hip_context_stream(mfmg_hip_context_t ctx);

/* ---- distributed runs: one process per GPU, the mesh cut into slabs along z or into boxes (2 x 1 x 1, 2 x 2 x 1, 2 x 2 x 2 ...) ----
 * Replaces deal.II's distributed::Vector ghost exchange inside MatrixFree::cell_loop and the all-gather of
 * the whole vector in front of every SpMV on the CUDA path (source/cuda/utils.cu:363-482,
 * include/mfmg/cuda/sparse_matrix_device.templates.cuh:104-138).  The local mesh of a rank is its owned
 * cell slab (box) plus `ghost_cells_low/high` (0 or 2 = one agglomerate) cell layers of its neighbours (per split axis); local
 * DoF numbering must be lexicographic; ghost (not owned) DoFs carry the value 2 in mfmg_hip_mesh_desc.constrained.
 * Boxes (the reference's p4est partition, tests/laplace_matrix_free.hpp:222, with rank-local agglomerates,
 * include/mfmg/common/amge.templates.hpp:453-478,604-621): mfmg_hip_context_set_communicator_box places the rank at
 * (cx, cy, cz) = (rank % gx, (rank / gx) % gy, rank / (gx gy)) of a gx x gy x gz grid of equal boxes; interface planes belong
 * to the upper box (the last box of an axis also owns the top plane).  One exchange = one packing kernel, ONE grouped
 * send/recv with all neighbours (faces, edges, corners: 7 on a 2 x 2 x 2 grid, at most 26) and one unpacking kernel: per fine
 * exchange a rank of a 2 x 2 x 2 grid sends 3 faces of (N/2)^2 doubles (+ 3 edges + 1 corner) where a slab of 8 sends 2 planes
 * of N^2.
 * Every level of the V-cycle is coupled across the ranks: before an operator application the library refreshes
 * the ghost layers of its input (owner -> ghost), after a transposed prolongator it returns the partial sums in
 * the ghost layers to their owners (ghost -> owner, added); the levels of the aggregation hierarchy whose global
 * size is small are gathered and solved redundantly on every rank.  The distributed cycle is the same
 * preconditioner as the single-process one (same matrices to rounding).
 * Transport, one of:
 *   mfmg_hip_context_use_rccl            ncclSend / ncclRecv between slab neighbours on the library's HIP stream
 *                                        (RCCL over xGMI); the 128-byte id comes from mfmg_hip_rccl_unique_id on
 *                                        rank 0 and must reach every rank through the caller's own channel;
 *   mfmg_hip_context_use_host_transport  the library stages the layers through pinned host memory and calls the
 *                                        callbacks with HOST pointers (tests: gloo, several ranks on one card).
 * `exchange` sends count[i] doubles from send[i] to rank peers[i] and receives as many from it into recv[i], for i < n, all
 * at once (slabs: rank - 1 and / or rank + 1);
 * `allreduce` combines `n` doubles over all ranks in place (op 0: sum, 1: max); `allgather` collects `n` doubles of
 * every rank into `out` (n * n_ranks, rank order). */
typedef int (*mfmg_hip_host_exchange_fn)(void *user, int32_t n, const int32_t *peers, const double *const *send, double *const *recv,
                                         const int64_t *count);
typedef int (*mfmg_hip_host_allreduce_fn)(void *user, double *values, int n, int op);
typedef int (*mfmg_hip_host_allgather_fn)(void *user, const double *in, int64_t n, double *out);
int mfmg_hip_context_set_communicator(mfmg_hip_context_t ctx, int32_t rank, int32_t n_ranks, int32_t ghost_cells_low,
                                      int32_t ghost_cells_high);
/* grid[3]: ranks along x, y, z (their product = the number of ranks); ghost_low / ghost_high[3]: ghost cell layers of the local
 * mesh per axis (2 towards an existing neighbour -- or 4 below, see mfmg_hip_context_set_low_ghost_cells --, else 0).  set_communicator(rank, n, lo, hi) is the grid 1 x 1 x n. */
int mfmg_hip_context_set_communicator_box(mfmg_hip_context_t ctx, int32_t rank, const int32_t grid[3], const int32_t ghost_low[3],
                                          const int32_t ghost_high[3]);
/* Ghost cell layers EVERY rank of the run holds towards a lower neighbour: 2 (default, one agglomerate) or 4 (two; then
 * ghost_low[d] = 4 above).  The same value on every rank, also on ranks without a lower neighbour, after set_communicator*:
 * the interface plane belongs to the upper box, so a box holds three ghost node planes above it and `cells` below, and a
 * sweep of K smoother terms (one exchange of x, K planes deep, ghost DoFs computed redundantly) needs K on every side with a
 * neighbour -- 4 lets the whole Chebyshev(3) smoother of a rank run as ONE sweep with ONE exchange. */
int mfmg_hip_context_set_low_ghost_cells(mfmg_hip_context_t ctx, int32_t cells);
int mfmg_hip_rccl_unique_id(unsigned char out[128]);
/* MFMG_HIP_SUCCESS when librccl and the entry points the transport uses can be resolved in this process (dlopen / dlsym
 * only, no RCCL call is made).  Callers agree on the transport with a collective over this flag before they choose. */
int mfmg_hip_rccl_available(void);
int mfmg_hip_context_use_rccl(mfmg_hip_context_t ctx, const unsigned char unique_id[128]);
int mfmg_hip_context_use_host_transport(mfmg_hip_context_t ctx, mfmg_hip_host_exchange_fn exchange,
                                        mfmg_hip_host_allreduce_fn allreduce, mfmg_hip_host_allgather_fn allgather, void *user);
/* MEASUREMENT of one rank's share of a distributed cycle on one GPU, for a hierarchy that was set up with a real transport:
 * from this call on every message this rank sends is copied back on the device as the message it would have received, an
 * all-gather repeats its block, an all-reduce is the identity -- all kernels, packings, stream joins and replicated levels of
 * the partition with a wire that costs nothing (scratch/rank_cycle_on_one_gpu.py).  What the rank iterates on afterwards is
 * not a solution of anything. */
int mfmg_hip_context_use_reflecting_transport(mfmg_hip_context_t ctx);
/* ... the same with a price on the wire: every grouped send/recv and every collective holds its stream for
 * `microseconds_per_group` (a one-thread kernel) before the reflected data arrive -- the latency of a real group, e.g. what
 * mfmg_hip_context_transport_loopback_time measured for the RCCL transport */
int mfmg_hip_context_use_reflecting_transport_delay(mfmg_hip_context_t ctx, double microseconds_per_group);
/* stream time of one loop-back group (send to self + receive from self, n doubles) of the registered transport: `reps` groups
 * back to back between two events */
int mfmg_hip_context_transport_loopback_time(mfmg_hip_context_t ctx, int64_t n, int reps, double *microseconds);
/* "rccl", "host", "reflecting" or "" (none) */
int mfmg_hip_context_transport_name(mfmg_hip_context_t ctx, char *buffer, size_t buffer_size);
/* ranks the registered transport's own communicator reports (RCCL: ncclCommCount; 1 without a transport) */
int mfmg_hip_context_transport_ranks(mfmg_hip_context_t ctx, int *n_ranks);
/* exercises the registered transport: `n` doubles sent to this rank itself and back, an all-gather and sum / max
 * all-reduces over all ranks; returns the largest deviation from the known answers (0 when everything arrived) */
int mfmg_hip_context_transport_selftest(mfmg_hip_context_t ctx, int64_t n, double *max_error);
/* point-to-point exchanges issued through the context so far (diagnostics) */
int mfmg_hip_context_exchange_count(mfmg_hip_context_t ctx, int64_t *n_exchanges);
/* ... the doubles this rank has sent in them, and (n_overlapped, may be NULL) how many of the exchanges ran on the second
 * stream beside the operator tiles that read no ghost plane */
int mfmg_hip_context_exchange_volume(mfmg_hip_context_t ctx, int64_t *n_doubles_sent, int64_t *n_overlapped);
/* one halo exchange of a device vector of `space` (1 fine DoFs, 2 first coarse level, 3.. aggregation levels):
 * reverse = 0 owner -> ghost, 1 ghost -> owner (added).  The cycle does this by itself; exposed for tests. */
int mfmg_hip_context_exchange(mfmg_hip_context_t ctx, int32_t space, double *vector, int reverse);
/* The forward exchange (owner -> ghost) of a FLOAT device vector of the fine DoF space, `width` planes deep (1 to 3, at most the
 * ghost planes every rank holds below: 2, or 4 with two ghost agglomerates).  The packing kernel widens the entries into the
 * staging buffers of the double exchange and the unpacking kernel narrows them (exact both ways), so the transports, the
 * callbacks and the messages are those of a double vector of the space: the same peers and counts, 8 bytes per entry on the
 * wire.  A slab packs too.  space must be 1 (MFMG_HIP_ERROR_INVALID_ARGUMENT otherwise).  What the FP32 fine level does by itself;
 * exposed for tests. */
int mfmg_hip_context_exchange_f32(mfmg_hip_context_t ctx, int32_t space, float *vector, int width);
/* Host only (no context, no GPU; tests): the messages of one box exchange `width` layers deep of a local box of local_nodes[3] nodes
 * (x fastest, `comps` entries per node) that owns [own0, own0 + own_n) per axis and has a neighbour below / above along the axes
 * with has_low / has_high set, on rank `rank` of a grid[3] arrangement.  n_messages (<= 26), peers and counts (26 entries
 * each) describe the group; send_entries / recv_entries (both NULL, or `capacity` >= the sum of the counts entries each) receive
 * for every entry of the packed buffer its position in the local vector: where the packing kernel reads it (owned boundary
 * layers) and where the unpacking kernel writes what arrived in its place (ghost layers). */
int mfmg_hip_halo_box_messages(const int64_t *local_nodes, const int64_t *own0, const int64_t *own_n, const int32_t *has_low,
                               const int32_t *has_high, int32_t comps, int32_t width, int32_t rank, const int32_t *grid,
                               int32_t *n_messages, int32_t *peers, int64_t *counts, int64_t *send_entries, int64_t *recv_entries,
                               int64_t capacity);
/* sum over the ranks of the dot product over the owned entries of two vectors of `space` */
int mfmg_hip_context_owned_dot(mfmg_hip_context_t ctx, int32_t space, const double *x, const double *y, double *result);
/* Distributed runs: overlap the exchange of the fine-level ghost planes with the operator tiles that do not read
 * them (second HIP stream; default on).  Off: exchange first, then one launch over all tiles.  Same results. */
int mfmg_hip_context_set_overlap_exchange(mfmg_hip_context_t ctx, int enable);
/* Matrix-free operators created afterwards: when the eight quadrature coefficients of every cell are equal
 * (material_property constant, the reference's default, or any cell-wise constant material) keep ONE value per
 * cell (20 instead of 76 bytes per cell in FP64; default on).  Off forces the general eight-value layout. */
int mfmg_hip_context_set_cell_constant_layout(mfmg_hip_context_t ctx, int enable);
/* With one coefficient per cell the diagonal of a DoF is kd * (sum of the coefficients of its eight cells); by default the
 * operator kernel derives D^-1 from that on the fly and the chunk records hold no D^-1 (8 bytes per DoF and smoother launch
 * less to read, 768 instead of 1280 B per chunk).  enable != 0: operators created afterwards keep D^-1 in the records. */
int mfmg_hip_context_set_stored_diagonal(mfmg_hip_context_t ctx, int enable);
int mfmg_hip_mf_laplace_diagonal_in_record(mfmg_hip_mf_laplace_t op, int *in_record);
/* Polynomial terms of the Chebyshev smoother that ONE sweep of a matrix-free operator may run (1, 2 or 3; default 3: the whole
 * Chebyshev(3) apply of DealIIMatrixFreeSmoother::apply, source/dealii/dealii_matrix_free_smoother.cc:63-76, reads x, b and the
 * coefficients once).  Operators created afterwards cut their rows into chunks with that many halo columns on either side
 * (1 = the layout of the one-term kernels, which a distributed run always takes). */
int mfmg_hip_context_set_mf_fused_terms(mfmg_hip_context_t ctx, int n_terms);
/* Measurement switches of the distributed fine operator (the environment variables MFMG_MF_SHELL / MFMG_MF_EMULATE_SPLIT give the
 * initial values when the context is created; nothing reads the environment per application).  shell mode: 0 = the shell of
 * tiles around the interior as one launch on the exchange stream beside the interior tiles (default), 1 = after them, 2 = slab
 * by slab.  emulate split (one rank): the launches a rank of 1x1x2 (1), 1x2x2 (2), 2x2x2 (3) would make, without an exchange. */
int mfmg_hip_context_set_mf_shell(mfmg_hip_context_t ctx, int mode);
int mfmg_hip_context_set_mf_emulate_split(mfmg_hip_context_t ctx, int axes);
/* 1 when the operator kernel COMPUTES the DoF ids instead of reading them from its records: a numbering that is affine
 * on the node grid (any lexicographic one), Dirichlet DoFs on whole faces of the box, ghost DoFs on whole z-layers,
 * checked slot by slot at construction; used by the eight-coefficient kernels (where it pays).  MFMG_MF_AFFINE_IDS=0
 * keeps the ids of the records. */
int mfmg_hip_mf_laplace_ids_computed(mfmg_hip_mf_laplace_t op, int *computed);
/* Hierarchies created afterwards form the coarse operator R A R^T of a matrix-free A on the device by probing
 * (27 n_eig applications of R^T, A and R over colour classes of agglomerates; the reference's fast_ap idea,
 * source/dealii/dealii_matrix_free_hierarchy_helpers.cc:77-288) -- the default where the restrictor has the block
 * structure, distributed runs included (colours on global coordinates, every rank keeps its own rows); 0: the host
 * triple product.  Same matrix to rounding. */
int mfmg_hip_context_set_galerkin_on_device(mfmg_hip_context_t ctx, int enable);
/* layout of a distributed space after the hierarchy was built: entries per layer, local layers, owned range;
 * mfmg_hip_context_halo_space adds {global index of local layer 0, global layers, exchange width, number of spaces} */
int mfmg_hip_context_halo_layout(mfmg_hip_context_t ctx, int32_t space, int64_t *layer_elems, int64_t *n_layers,
                                 int64_t *owned_begin, int64_t *owned_count);
int mfmg_hip_context_halo_space(mfmg_hip_context_t ctx, int32_t space, int64_t out[8]);
/* the same per axis (x, y, z): out = {entries per node, local nodes[3], first owned[3], owned[3], global index of local node 0 [3],
 * global nodes[3]}: a vector of the space is the lexicographic array of the local nodes, `entries per node` values each */
int mfmg_hip_context_halo_box(mfmg_hip_context_t ctx, int32_t space, int64_t out[16]);

/* BASELINE.json configs[4]: the cell-local evaluation of the Q1 Laplace as a batched dense contraction,
 * v[m][cell] = c[cell] * sum_k K_ref[m][k] u[k][cell] (K_ref: reference matrix of a Cartesian cell of size `cell_size`,
 * what LaplaceOperator::local_apply computes per cell for a cell-wise constant coefficient, tests/laplace_matrix_free.hpp:129-156)
 * on planar device operands u, v: [8][n_cells], c: [n_cells].  fp32 != 0: float operands.  variant 0: vector ALU,
 * 1: MFMA (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64).  Timed under the kernel names "cell_contraction_valu" /
 * "cell_contraction_mfma" (17 values moved per cell). */
int mfmg_hip_cell_contraction(mfmg_hip_context_t ctx, int fp32, int variant, int64_t n_cells, const void *u, const void *c,
                              void *v, const double cell_size[3]);

/* Per-kernel timing with HIP events recorded on the launch stream (the reference only has the
 * wall-clock dealii::TimerOutput sections, include/mfmg/common/hierarchy.hpp:36-47).  Kernel names:
 * "mf_laplace_kernel", "csr_spmv_kernel".  `algorithmic_bytes` sums SURVEY.md 8d's per-launch figures. */
int mfmg_hip_profile_enable(mfmg_hip_context_t ctx, int enabled);
/* restrict the timing to launches of one kernel name (NULL or "" = all); every timed launch costs two event records */
int mfmg_hip_profile_select(mfmg_hip_context_t ctx, const char *kernel_name);
int mfmg_hip_profile_query(mfmg_hip_context_t ctx, const char *kernel_name, int64_t *n_launches, double *total_ms,
                           double *algorithmic_bytes);

/* ---- host<->device marshalling (source/cuda/utils.cu:484-510, include/mfmg/cuda/utils.cuh:66-99) ---- */
int mfmg_hip_malloc(void **dev_ptr, size_t bytes);                      /* cuda_malloc */
int mfmg_hip_free(void *dev_ptr);                                       /* cuda_free */
int mfmg_hip_copy_to_dev(void *dst_dev, const void *src_host, size_t bytes);  /* cuda_mem_copy_to_dev */
int mfmg_hip_copy_to_host(void *dst_host, const void *src_dev, size_t bytes); /* cuda_mem_copy_to_host */

/* ---- vector kernels used inside the cycle (deal.II CUDA vector ops called at
 *      include/mfmg/common/hierarchy.hpp:258,286,302 and source/cuda/cuda_smoother.cu:50-59) ---- */
int mfmg_hip_vector_set(mfmg_hip_context_t ctx, int64_t n, double value, double *x);                 /* x = value        */
int mfmg_hip_vector_add(mfmg_hip_context_t ctx, int64_t n, double a, const double *v, double *x);    /* x.add(a, v)      */
int mfmg_hip_vector_sadd(mfmg_hip_context_t ctx, int64_t n, double s, double a, const double *v, double *x); /* x.sadd(s,a,v) */
int mfmg_hip_vector_dot(mfmg_hip_context_t ctx, int64_t n, const double *x, const double *y, double *result_host); /* synchronous */
int mfmg_hip_vector_l2_norm(mfmg_hip_context_t ctx, int64_t n, const double *x, double *result_host);              /* synchronous, x.l2_norm() */

/* ---- CSR matrix on device: SparseMatrixDevice<double> ---- */
/* convert_matrix (source/cuda/utils.cu:39-168): upload a host CSR (0-based, int32). */
int mfmg_hip_csr_create(mfmg_hip_context_t ctx, int64_t n_rows, int64_t n_cols, int64_t nnz,
                        const int32_t *row_ptr_host, const int32_t *col_host,
                        const double *val_host, mfmg_hip_csr_t *out);
int mfmg_hip_csr_destroy(mfmg_hip_csr_t a);
int mfmg_hip_csr_shape(mfmg_hip_csr_t a, int64_t *n_rows, int64_t *n_cols, int64_t *nnz); /* m(), n(), n_nonzero_elements() */
/* tuning knob of the SpMV kernel: lanes of a wavefront per row (power of two 1..64; 256 = a workgroup per row, the
 * choice for at most 4096 rows of 256 entries or more; 0 = keep) and the storage variant (0 plain CSR, 1 LDS-cached
 * CSR, 2 block-diagonal (get reports 3 when only the upper half of a symmetric matrix is stored), 4 row-base storage
 * of rectangular stencil-like matrices, 5 node classes (rectangular matrices whose rows repeat a few stencils: per-class
 * tables instead of stored values), -1 = keep; a variant is only taken where its data was built at construction);
 * the summation order, hence the last bits of the result, follows both */
int mfmg_hip_csr_set_kernel(mfmg_hip_csr_t a, int lanes_per_row, int use_lds);
int mfmg_hip_csr_get_kernel(mfmg_hip_csr_t a, int *lanes_per_row, int *use_lds);
/* Rows of a symmetric block-diagonal matrix that repeat one stencil bit for bit (interior rows of the coarse operators
 * of a constant-coefficient problem on a uniform mesh) are evaluated from a table of constants instead of stored
 * values.  in_use: whether such rows were found and the path is on; enable = 0 switches it off (same results to
 * rounding). */
int mfmg_hip_csr_regular_rows(mfmg_hip_csr_t a, int *in_use);
int mfmg_hip_csr_set_regular_rows(mfmg_hip_csr_t a, int enable);
/* Of the rows that are not regular: n_classes stencils that groups of nodes share among themselves (the shells
 * next to the boundary; evaluated from per-class tables) and listed_rows rows left to the stored values. */
int mfmg_hip_csr_stencil_classes(mfmg_hip_csr_t a, int *n_classes, int64_t *listed_rows);
/* 1 when the values the kernels read (block-diagonal planes; the agglomerate-wise planes of a restrictor) are kept in
 * float: every one of them is representable in it -- a hierarchy built with "setup value precision" float -- so the
 * storage is lossless; products and sums stay FP64. */
int mfmg_hip_csr_float_storage(mfmg_hip_csr_t a, int *in_float);
/* The source vector x of the SpMV entry points below (vmult, apply, smoother_step, residual, launch) must be 16-byte
 * aligned (any hipMalloc'ed vector is): kernels read it two doubles at a time.  The other vectors need 8 bytes. */
/* SparseMatrixDevice::vmult  (…templates.cuh:351-371): y = A x */
int mfmg_hip_csr_vmult(mfmg_hip_csr_t a, const double *x, double *y);
/* CudaMatrixOperator::apply (source/cuda/cuda_matrix_operator.cu:80-91); TRANS uses the
 * explicit transpose built once by transpose() (:93-130) -- here by device kernels at first use
 * (csr_algebra.hip; rows of the transpose beyond 4096 entries take the host algorithm). */
int mfmg_hip_csr_apply(mfmg_hip_csr_t a, const double *x, double *y, int mode);
/* CudaMatrixOperator::transpose (:93-130) */
int mfmg_hip_csr_transpose(mfmg_hip_csr_t a, mfmg_hip_csr_t *out);
/* SparseMatrixDevice::mmult / CudaMatrixOperator::multiply (…templates.cuh:373-434, cuda_matrix_operator.cu:132-149): C = A B
 * (setup; row-wise hash SpGEMM in LDS, sums in the order of the host product; rows with more than 2048 candidate
 * columns take the host algorithm; MFMG_CSR_ALGEBRA=host|device|device_only selects) */
int mfmg_hip_csr_multiply(mfmg_hip_csr_t a, mfmg_hip_csr_t b, mfmg_hip_csr_t *out);
/* download (copy_from_dev / convert_to_trilinos_matrix, source/cuda/utils.cu:170-204) */
int mfmg_hip_csr_download(mfmg_hip_csr_t a, int32_t *row_ptr_host, int32_t *col_host, double *val_host);
/* CudaSolver(handle, op, params)->apply(b, x) (source/cuda/cuda_solver.cu:204-515, the standalone use of
 * tests/test_direct_solver_device.cu:23-110): builds the coarse solver `solver.type` names for this matrix -- lu_dense |
 * cholesky | lu_sparse_host (dense LU factored here), pcg, amg -- applies it once from a zero guess and drops it. */
int mfmg_hip_csr_solve(mfmg_hip_csr_t a, const char *params_info, const double *b, double *x);
/* extract_inv_diag (source/cuda/cuda_smoother.cu:86-96): dinv[i] = 1/A_ii on device */
int mfmg_hip_csr_inverse_diagonal(mfmg_hip_csr_t a, double *dinv);
/* One fused Jacobi/Chebyshev step on an assembled operator:
 * out = x + alpha (x - x_prev) - beta * dinv .* (A x - b).   x_prev may be NULL when alpha == 0.
 * Replaces the r=Ax-b / tmp=B^-1 r / x-=tmp sequence of source/cuda/cuda_smoother.cu:48-59. `out` must not alias `x`. */
int mfmg_hip_csr_smoother_step(mfmg_hip_csr_t a, const double *dinv, const double *b, const double *x,
                               const double *x_prev, double alpha, double beta, double *out);
/* res = A x - b  (include/mfmg/common/hierarchy.hpp:284-286, negative residual) */
int mfmg_hip_csr_residual(mfmg_hip_csr_t a, const double *x, const double *b, double *res);
/* One SpMV with any of the fused epilogues (what vmult / residual / smoother_step and, inside a cycle, the prolongations
 * call); b, dinv, x_prev, alpha, beta are read only by the modes that name them and may be NULL / 0 otherwise.  `out`
 * must not alias `x`; modes SUBTRACT and ADD read `out`.  FIRST and NEXT need a square matrix. */
#define MFMG_HIP_CSR_APPLY 0       /* out = A x */
#define MFMG_HIP_CSR_RESIDUAL 1    /* out = A x - b */
#define MFMG_HIP_CSR_FIRST 2       /* out = x - beta dinv (A x - b) */
#define MFMG_HIP_CSR_NEXT 3        /* out = x + alpha (x - x_prev) - beta dinv (A x - b) */
#define MFMG_HIP_CSR_SUBTRACT 4    /* out -= A x */
#define MFMG_HIP_CSR_ADD 5         /* out += A x */
#define MFMG_HIP_CSR_PLUS_SCALED 6 /* out = A x + beta dinv b */
int mfmg_hip_csr_launch(mfmg_hip_csr_t a, int mode, const double *x, const double *b, const double *dinv, const double *x_prev,
                        double alpha, double beta, double *out);
/* Which kernels an application of the matrix launches as it stands (tests: which kernel a case reaches).  Filled from the
 * record the launch itself branches on.  fields[0..26]:
 *   0 storage variant as mfmg_hip_csr_get_kernel reports it
 *   1 CSR kernel: 0 none, 1 lanes per row, 2 a workgroup per row, 3 LDS-cached; 2 lanes per row of the instance
 *   3 unknowns per node, 4 stored block diagonals, 5 offsets of the full stencil (tables)
 *   6 1 = symmetric half stored, 7 1 = planes in float
 *   8 1 = node kernels (stencil / class tables) in use, 9 1 = the regular nodes are one of the classes
 *  10 classes, 11 slots of the class lists (padded to wavefronts), 12 listed rows
 *  13 route of the listed rows: 0 none, 1 tail of the class kernel (4 wavefronts per workgroup), 2 tail of the split
 *     kernel (16), 3 a launch of their own, 4 the stored planes
 *  14 launch of the regular nodes: 0 none, 1 one thread per node, 4 / 16 stencil split over that many wavefronts
 *  15 launch of the classes: 0 none, 1 one thread per node, 4 / 16 split
 *  16 stored-plane kernel: 0 none, 1 rows, 2 rows of a symmetric half, 3 symmetric half split over four wavefronts
 *  17 row-base slots, 18 / 19 unknowns per node and offsets of the node classes of a rectangular matrix
 *  20 whether the last launch found every vector 16-byte aligned (-1: no launch yet), 21 1 = CSR arrays released
 *  22 1 = twin nodes (mfmg_hip_csr_enable_node_twins): one launch of bdia_twin_node_kernel, two row nodes per lane
 *  23 slots of the twin lists (padded to wavefronts, two nodes each), 24 twin classes (ordered pairs of node classes)
 *  25 slots left to the classed nodes without a twin (with twins: also what field 11 reports)
 *  26 whether the last twin launch took the 32-byte epilogue: b, dinv, x_prev and out 32-byte aligned, x 16-byte (-1: no twin
 *     launch yet, 0: the halves of the one-node kernel)
 * (22-26 were appended: n >= 22 is accepted and the fields up to n are filled, so a caller built against 22 fields still
 * works and a caller that passes 27 to an older library reads zeros there: no change of the ABI version) */
#define MFMG_HIP_CSR_FORM_FIELDS 27
int mfmg_hip_csr_form(mfmg_hip_csr_t a, int64_t *fields, int32_t n);
/* Twin nodes for a rectangular matrix in node classes (FP64, 1 or 2 unknowns per node, fewer than 48 offsets): the row nodes
 * (n, n + 1), n even, in classes and with one base become one lane.  *taken = 0 and the matrix as it was where fewer than
 * 90 % of the classed nodes are twins, where the layout does not apply, and under MFMG_NODE_TWINS=0 (read by this call).
 * The aggregation setup calls it on the smoothed prolongators it builds. */
int mfmg_hip_csr_enable_node_twins(mfmg_hip_csr_t a, int *taken);
/* Free the CSR arrays of a matrix whose kernels read tables, as "release setup matrices" does inside a hierarchy (the
 * listed rows are kept as a compact CSR of their own).  *released = 0 for a matrix whose kernels read the arrays. */
int mfmg_hip_csr_release_csr(mfmg_hip_csr_t a, int *released);

/* ---- matrix-free Q1 Laplace operator on a logically structured hex mesh ---- */
/* What the deal.II driver hands over (tests/laplace_matrix_free.hpp:243-313):
 * the cell->DoF index array, the coefficient table _coefficient(cell,q)
 * (:65,100-119), the constrained DoFs (AffineConstraints) and the Cartesian cell size. */
typedef struct mfmg_hip_mesh_desc
{
  int32_t dim;             /* 3 or 2 (2-D: the assembled path, and a plain matrix-free kernel for the small meshes of the reference tests) */
  int32_t n_cells[3];      /* cells per direction, lexicographic cell order, x fastest */
  double cell_size[3];     /* h_x, h_y, h_z (J = diag(h)) */
  int64_t n_dofs;          /* (n_cells+1) product */
  const int32_t *cell_dofs;     /* [n_cells_total][2^dim]  cell->get_dof_indices */
  const double *coefficient;    /* [n_cells_total][2^dim]  _coefficient(cell,q) */
  const uint8_t *constrained;   /* [n_dofs] 1 = Dirichlet-constrained DoF */
  int32_t arrays_on_device;     /* 0: host pointers, 1: device pointers */
} mfmg_hip_mesh_desc;

int mfmg_hip_mf_laplace_create(mfmg_hip_context_t ctx, const mfmg_hip_mesh_desc *mesh, mfmg_hip_mf_laplace_t *out);
int mfmg_hip_mf_laplace_destroy(mfmg_hip_mf_laplace_t op);
int mfmg_hip_mf_laplace_size(mfmg_hip_mf_laplace_t op, int64_t *n_dofs);
/* LaplaceOperator::vmult via matrix_free_evaluate_global (tests/test_hierarchy_helpers.hpp:370-375,
 * source/dealii/dealii_matrix_free_operator.cc:31-36): y = A x, constrained rows y_c = x_c */
int mfmg_hip_mf_laplace_vmult(mfmg_hip_mf_laplace_t op, const double *x, double *y);
/* matrix_free_get_diagonal_inverse (tests/test_hierarchy_helpers.hpp:377-382; compute_diagonal
 * tests/laplace_matrix_free.hpp:75-98): copies the inverse diagonal (constrained entries 1) */
int mfmg_hip_mf_laplace_diagonal_inverse(mfmg_hip_mf_laplace_t op, double *dinv);
int mfmg_hip_mf_laplace_diagonal(mfmg_hip_mf_laplace_t op, double *diag);
/* res = A x - b */
int mfmg_hip_mf_laplace_residual(mfmg_hip_mf_laplace_t op, const double *x, const double *b, double *res);
/* fused smoother step, as mfmg_hip_csr_smoother_step (DealIIMatrixFreeSmoother::apply,
 * source/dealii/dealii_matrix_free_smoother.cc:63-76, one polynomial term per call) */
int mfmg_hip_mf_laplace_smoother_step(mfmg_hip_mf_laplace_t op, const double *b, const double *x,
                                      const double *x_prev, double alpha, double beta, double *out);
/* n_terms (2 or 3) smoother terms in one sweep: x_1 = x - beta[0] dinv (A x - b), x_s = x_{s-1} + alpha[s-1] (x_{s-1} - x_{s-2})
 * - beta[s-1] dinv (A x_{s-1} - b); out = x_{n_terms}, out_prev (may be NULL) = x_{n_terms - 1}.  Bit for bit what n_terms calls
 * of mfmg_hip_mf_laplace_smoother_step return.  alpha[0] must be 0; x, out and out_prev must be different vectors.
 * MFMG_HIP_ERROR_NOT_IMPLEMENTED when the operator cannot run it (mfmg_hip_mf_laplace_sweep_available: cell-constant layout,
 * a numbering the kernel can compute, at least n_terms halo columns, one rank).
 * x == NULL: the sweep from x_0 = 0, which is then not read and whose first term needs no operator application (x_1 = beta[0] dinv b:
 * the pre-smoother of a preconditioner application, include/mfmg/common/hierarchy.hpp:253-259) -- three terms, default arithmetic;
 * the result of the sweep run on a zeroed vector.  Hierarchy::apply uses it when "is preconditioner" is true. */
int mfmg_hip_mf_laplace_sweep_available(mfmg_hip_mf_laplace_t op, int n_terms, int *available);
int mfmg_hip_mf_laplace_smoother_sweep(mfmg_hip_mf_laplace_t op, int n_terms, const double *alpha, const double *beta,
                                       const double *b, const double *x, double *out, double *out_prev);
/* The sweep's cell arithmetic.  Default (0): the cell matrix in mode space -- per direction a Q1 cell acts on the sum and the
 * difference of its two nodes alone, the 8 x 8 cell matrix is diagonal on the eight modes and the butterflies are shared between
 * neighbouring cells: ~30 % fewer FP64 operations, the same operator with its own rounding (1e-15 per cell).  on != 0: the
 * arithmetic of the one-term kernel, bit for bit (tests compare the two kernels that way). */
int mfmg_hip_mf_laplace_set_sweep_reference(mfmg_hip_mf_laplace_t op, int on);
/* tile of the sweep: n_waves (1 .. 8) wavefronts of tile_y cell rows (2, 3 or 4), tile_z owned layers; 0, 0, 0 = chosen from the mesh.
 * 12 wavefronts of 2 rows: the shape of the three-term FP64 sweep with D^-1 derived in the kernel (its default; 8, 3 is the shape
 * of before); a sweep that has no such kernel keeps its default tile when asked for it */
/* Where the sweep of twelve wavefronts of two rows takes D^-1 from.  An FP64 operator that can run that sweep (one coefficient
 * per cell, computed ids, three halo lanes, no D^-1 in the records) builds at construction a vector of n_dofs values
 * 1 / (kd * sum of the coefficients of the eight cells of a DoF), bit for bit what the kernels derive on the fly, and the sweep
 * reads it (stored = 1, the default there) instead of deriving it per DoF and launch (stored = 0: same results, bit for bit).
 * The environment variable MFMG_MF_SWEEP_DINV=derived, read at construction, builds no vector: such an operator, and any that
 * cannot run that sweep, reports 0, and asking it for 1 or for the vector is MFMG_HIP_ERROR_NOT_IMPLEMENTED.
 * mfmg_hip_mf_laplace_sweep_diagonal_inverse copies the vector (device pointer, n_dofs doubles, the operator's numbering;
 * entries of Dirichlet DoFs are finite and not read by any kernel).  (additions, no change of the ABI version) */
int mfmg_hip_mf_laplace_set_sweep_diagonal(mfmg_hip_mf_laplace_t op, int stored);
int mfmg_hip_mf_laplace_get_sweep_diagonal(mfmg_hip_mf_laplace_t op, int *stored);
int mfmg_hip_mf_laplace_sweep_diagonal_inverse(mfmg_hip_mf_laplace_t op, double *dinv);
int mfmg_hip_mf_laplace_set_sweep_tile(mfmg_hip_mf_laplace_t op, int n_waves, int tile_y, int tile_z);
int mfmg_hip_mf_laplace_get_sweep_tile(mfmg_hip_mf_laplace_t op, int n_terms, int *n_waves, int *tile_y, int *tile_z);
/* FP32 instance of the same operator (BASELINE.json configs[4]; the coefficient table is converted once,
 * vectors are device `float`).  The cell kernel stays on the vector ALU: at ~11 flop/B it sits below the
 * FP32-MFMA ridge, so a batched-GEMM reformulation would not lift the HBM bound. */
typedef struct mfmg_hip_mf_laplace_f32_s *mfmg_hip_mf_laplace_f32_t;
int mfmg_hip_mf_laplace_f32_create(mfmg_hip_context_t ctx, const mfmg_hip_mesh_desc *mesh, mfmg_hip_mf_laplace_f32_t *out);
int mfmg_hip_mf_laplace_f32_destroy(mfmg_hip_mf_laplace_f32_t op);
int mfmg_hip_mf_laplace_f32_cell_constant_layout(mfmg_hip_mf_laplace_f32_t op, int *in_use);
int mfmg_hip_mf_laplace_f32_ids_computed(mfmg_hip_mf_laplace_f32_t op, int *computed); /* as mfmg_hip_mf_laplace_ids_computed */
int mfmg_hip_mf_laplace_f32_vmult(mfmg_hip_mf_laplace_f32_t op, const float *x, float *y);
int mfmg_hip_mf_laplace_f32_diagonal_inverse(mfmg_hip_mf_laplace_f32_t op, float *dinv);
int mfmg_hip_mf_laplace_f32_residual(mfmg_hip_mf_laplace_f32_t op, const float *x, const float *b, float *res);
int mfmg_hip_mf_laplace_f32_smoother_step(mfmg_hip_mf_laplace_f32_t op, const float *b, const float *x,
                                          const float *x_prev, float alpha, float beta, float *out);
int mfmg_hip_mf_laplace_f32_sweep_available(mfmg_hip_mf_laplace_f32_t op, int n_terms, int *available);
int mfmg_hip_mf_laplace_f32_set_sweep_reference(mfmg_hip_mf_laplace_f32_t op, int on);
int mfmg_hip_mf_laplace_f32_smoother_sweep(mfmg_hip_mf_laplace_f32_t op, int n_terms, const float *alpha, const float *beta,
                                           const float *b, const float *x, float *out, float *out_prev);
/* The tiles of the FP32 instance, as the entry points of the same names without _f32 below and above (same ranges).  The float sweep
 * has no kernel of 12 wavefronts of 2 rows: asked for it, it keeps its default tile (8 x 3 rows at three terms, 4 x 4 at two). */
int mfmg_hip_mf_laplace_f32_set_tile(mfmg_hip_mf_laplace_f32_t op, int tile_y, int tile_z);
int mfmg_hip_mf_laplace_f32_set_tile_waves(mfmg_hip_mf_laplace_f32_t op, int n_waves);
int mfmg_hip_mf_laplace_f32_get_tile(mfmg_hip_mf_laplace_f32_t op, int *n_waves, int *tile_y, int *tile_z);
int mfmg_hip_mf_laplace_f32_set_sweep_tile(mfmg_hip_mf_laplace_f32_t op, int n_waves, int tile_y, int tile_z);
int mfmg_hip_mf_laplace_f32_get_sweep_tile(mfmg_hip_mf_laplace_f32_t op, int n_terms, int *n_waves, int *tile_y, int *tile_z);
int mfmg_hip_mf_laplace_f32_diagonal_in_record(mfmg_hip_mf_laplace_f32_t op, int *in_record);
/* tuning knob: owned DoF rows / planes per workgroup tile (0 = heuristic) */
int mfmg_hip_mf_laplace_set_tile(mfmg_hip_mf_laplace_t op, int tile_y, int tile_z);
/* wavefronts per workgroup (1..8) stacked in y that hand their boundary sums on through LDS (0 = heuristic) */
int mfmg_hip_mf_laplace_set_tile_waves(mfmg_hip_mf_laplace_t op, int n_waves);
/* 1 when the operator keeps one coefficient per cell (see mfmg_hip_context_set_cell_constant_layout) */
int mfmg_hip_mf_laplace_cell_constant_layout(mfmg_hip_mf_laplace_t op, int *in_use);
/* uniform = 1 when the operator holds ONE coefficient for the whole mesh: the cell-constant layout with computed ids, all six
 * faces Dirichlet, one rank, no D^-1 in the records, every stored cell coefficient of the same bits (decided on the device at
 * construction).  The three-term FP64 sweep then applies the operator as three 1-D stencils, on every tile shape
 * (MFMG_MF_UNIFORM_SWEEP=0: the mode-space kernels as before); sweeps = how many sweeps of this operator took that kernel so
 * far (may be NULL).  (addition, no change of the ABI version) */
int mfmg_hip_mf_laplace_uniform_coefficient(mfmg_hip_mf_laplace_t op, int *uniform, int64_t *sweeps);
/* the tile in use */
int mfmg_hip_mf_laplace_get_tile(mfmg_hip_mf_laplace_t op, int *n_waves, int *tile_y, int *tile_z);
/* mfmg_hip_mf_z_tiles (host only: no context, no GPU): the z-tiling the operator launches read for n_layers DoF layers and the
 * tile height tz -- starts[t] is the first layer of z-tile t, starts[n_tiles] = n_layers, so tile t owns the layers [starts[t],
 * starts[t + 1]).  graded = 0: the uniform table, ceil(n_layers / tz) tiles of tz layers (what a launch on a region of tiles
 * reads).  graded != 0: what a whole-mesh launch of the one-term operator and every launch of the block operator read: with
 * m = (n_layers / 8 + tz / 2) / tz + 1 and n_layers / 8 >= 2 m every eighth of the layers is cut into m tiles whose heights
 * fall off linearly (257 layers, tz = 8: 10, 8, 7, 4, 3), 8 m tiles, some taller than tz; the uniform table otherwise.  The
 * experiment knobs MFMG_MF_GRADE_M and MFMG_MF_GRADE_OFF are not read here.  `starts` has room for `capacity` entries;
 * MFMG_HIP_ERROR_INVALID_ARGUMENT for a null pointer, n_layers < 1, tz < 1 or capacity < n_tiles + 1 (n_layers + 1 always
 * suffices).  (addition, no change of the ABI version) */
int mfmg_hip_mf_z_tiles(int32_t n_layers, int32_t tz, int graded, int32_t *starts, int32_t capacity, int32_t *n_tiles);

/* ---- blocks of vectors: several right-hand sides against one operator (additions, no change of the ABI version) ----
 * A block is n_vectors (1 .. 64) columns of doubles with a common leading dimension: column c starts at base + c * ld elements,
 * ld >= n_dofs and even, the base aligned to 16 bytes.  All blocks of one call share ld.  FP64, one rank: a context with a
 * communicator is refused (MFMG_HIP_ERROR_INVALID_ARGUMENT), as are n_vectors outside 1 .. 64, ld < n_dofs, an odd ld, a
 * misaligned base, an out block that overlaps the x block and a null operand the mode reads.
 * mfmg_hip_block_groups (host only): how a block is cut into launches -- groups of 4, then one of 2, then one single vector;
 * `widths` receives up to MFMG_HIP_BLOCK_MAX_GROUPS entries.
 * mfmg_hip_mf_laplace_block_launch: mode 0 out = A x, 1 out = A x - b, 2 out = x - beta dinv (A x - b), 3 out = x + alpha (x -
 * x_prev) - beta dinv (A x - b), on every column; out may be x_prev.  Groups of 4 and 2 columns run mf_laplace_block_kernel (the
 * chunk records are read once per group) where mfmg_hip_mf_laplace_block_available reports 1: eight coefficients per cell, 3-D;
 * elsewhere, and for a single column, the one-vector kernel runs column by column.  Every column gets the bits of the one-vector
 * entry point.  The block tile (n_waves 1 .. 8, tile_y 2 .. 4, tile_z; 0, 0, 0 = chosen from the mesh and the group's width) is a
 * tuning knob; get_block_tile takes the width of the group (2 or 4). */
#define MFMG_HIP_BLOCK_MAX_VECTORS 64
#define MFMG_HIP_BLOCK_MAX_GROUPS 18
int mfmg_hip_block_groups(int32_t n_vectors, int32_t *widths, int32_t *n_groups);
int mfmg_hip_mf_laplace_block_launch(mfmg_hip_mf_laplace_t op, int mode, int32_t n_vectors, int64_t ld, const double *x, const double *b,
                                     const double *x_prev, double alpha, double beta, double *out);
int mfmg_hip_mf_laplace_block_available(mfmg_hip_mf_laplace_t op, int *available);
int mfmg_hip_mf_laplace_set_block_tile(mfmg_hip_mf_laplace_t op, int n_waves, int tile_y, int tile_z);
int mfmg_hip_mf_laplace_get_block_tile(mfmg_hip_mf_laplace_t op, int n_vectors, int *n_waves, int *tile_y, int *tile_z);

/* ---- hierarchy: Hierarchy<VectorType> ---- */
/* Evaluator tag strings accepted by the string switch (create_hierarchy_helpers,
 * include/mfmg/common/hierarchy.hpp:49-107):
 *   "HipMeshEvaluator"            assembled CSR path (twin of "CudaMeshEvaluator")
 *   "HipMatrixFreeMeshEvaluator"  matrix-free path   (the tag "CudaMatrixFreeMeshEvaluator",
 *                                  source/cuda/cuda_matrix_free_mesh_evaluator.cu:21-24, is never dispatched upstream)
 * `params_info` is the text of a boost::property_tree INFO file
 * (tests/data/hierarchy_input.info); keys as consumed at hierarchy.hpp:168-172,215,
 * dealii_matrix_free_smoother.cc:24-51, cuda_smoother.cu:105, cuda_solver.cu:215. */
int mfmg_hip_hierarchy_create(mfmg_hip_context_t ctx, const char *evaluator_type,
                              const mfmg_hip_mesh_desc *mesh, const char *params_info,
                              mfmg_hip_hierarchy_t *out);
int mfmg_hip_hierarchy_destroy(mfmg_hip_hierarchy_t h);
/* Parameter "internal numbering" (top level of `params_info`): caller (default) | lexicographic.
 * The kernels of the fine level compute their DoF ids, run the whole Chebyshev polynomial as one sweep and restrict the residual
 * in one pass only where the DoF numbering is lexicographic on the node grid; a mesh numbered otherwise (deal.II's
 * DoFHandler::distribute_dofs: cells in Morton order, tests/laplace_matrix_free.hpp:269-279; any DoFRenumbering) is correct in
 * `caller` mode but takes one launch per smoother term and an indexed access per DoF in every pass.  `lexicographic`: the
 * hierarchy is built and run in the lexicographic numbering of the nodes -- the node -> DoF map is derived from cell_dofs as it
 * is validated anyway -- and vectors are permuted where they cross this interface: every fine-level vector argument of the
 * mfmg_hip_hierarchy_* calls, the columns of get_restrictor / set_restrictor and what is keyed on a DoF id (the start vector of
 * the Chebyshev eigenvalue estimate) stay in the CALLER's numbering.  mfmg_hip_hierarchy_apply / _vmult / _apply_f32 cost two
 * launches of the kernel "dof_permutation" (dof_permutation.hip: the gather of b -- and of x unless "is preconditioner" --
 * and the scatter of x in place of the copy that ends the cycle), mfmg_hip_hierarchy_solve_cg two per solve whatever the
 * iteration count; the level-wise calls permute per call.  A numbering that already is lexicographic launches nothing and gives
 * the results of `caller` mode bit for bit.  Matrix-free evaluator, one process (MFMG_HIP_ERROR_INVALID_ARGUMENT otherwise).
 * In this mode the handle of mfmg_hip_hierarchy_get_restrictor is a copy with renumbered columns made by that call.
 *   lexicographic: 1 when the hierarchy was built with "internal numbering" lexicographic
 *   permuted:      1 when vectors are permuted, 0 where the caller's numbering already was lexicographic (or in caller mode) */
int mfmg_hip_hierarchy_internal_numbering(mfmg_hip_hierarchy_t h, int *lexicographic, int *permuted);
/* The permutation itself, for tests and for callers that keep Krylov vectors of their own in the internal numbering:
 * to_internal != 0: out[node] = in[caller's id of node], else out[caller's id of node] = in[node]; fp32 != 0: float vectors.
 * `in` and `out` are different device vectors of the fine level's size.  A plain copy where nothing is permuted. */
int mfmg_hip_hierarchy_permute(mfmg_hip_hierarchy_t h, int to_internal, int fp32, const void *in, void *out);
/* Hierarchy::apply(b, x, 0)  (hierarchy.hpp:246-309) */
int mfmg_hip_hierarchy_apply(mfmg_hip_hierarchy_t h, const double *b, double *x);
/* Hierarchy::vmult(x, b)     (hierarchy.hpp:238-244) */
/* The same cycle with the fine level in FP32 (BASELINE.json configs[4]): float device vectors; pre-smoother,
 * residual and post-smoother through the FP32 instance of the matrix-free operator, restriction, coarse solve and
 * prolongation in FP64.  Needs the parameter "fine level precision" float at creation (matrix-free evaluator, two
 * levels).  On a context with a communicator b and x are the rank's local float vectors (ghost entries are don't-care on entry):
 * the FP32 operator exchanges x like the FP64 one -- one plane per application beside the interior tiles, once per sweep as many
 * planes deep as the sweep has terms, b one plane less once per cycle -- widened to double on the wire
 * (mfmg_hip_context_exchange_f32); the ranks agree at creation on the sweep every rank's FP32 operator offers.  b_c = R (A x - b)
 * takes the two-step form there: the FP32 residual, widened, and the FP64 restriction with its own exchange. */
int mfmg_hip_hierarchy_apply_f32(mfmg_hip_hierarchy_t h, const float *b, float *x);
/* The FP32 operator of that level on its own (tests): mode 0 out = A x, 1 out = A x - b, 2 out = x + alpha (x - x_prev) - beta
 * D^-1 (A x - b) (x_prev NULL or alpha 0: no momentum).  Owned entries; on ranks the ghost entries of x are exchanged by the call.
 * Not with permuted vectors ("internal numbering" lexicographic on a renumbered mesh).  *_sweep_terms_f32: the terms the FP32
 * smoother runs as one sweep (0: a launch per term), the same on every rank. */
int mfmg_hip_hierarchy_operator_f32(mfmg_hip_hierarchy_t h, int mode, const float *x, const float *b, const float *x_prev, float alpha,
                                    float beta, float *out);
int mfmg_hip_hierarchy_sweep_terms_f32(mfmg_hip_hierarchy_t h, int *terms_out_of_place);
int mfmg_hip_hierarchy_vmult(mfmg_hip_hierarchy_t h, double *x, const double *b);
/* Outer Krylov driver of tests/hierarchy_driver.cc:103-116: dealii::SolverCG on the fine-level operator with
 * Hierarchy::vmult as preconditioner, SolverControl(max_iterations, tolerance) on the absolute l2 norm of the
 * residual.  x holds the initial guess on entry.  residual_history (may be NULL) receives ||r_0||, ||r_1||, ... as
 * far as history_len reaches.  Returns MFMG_HIP_ERROR when max_iterations is reached without convergence
 * (SolverControl::NoConvergence upstream), with the outputs filled. */
int mfmg_hip_hierarchy_solve_cg(mfmg_hip_hierarchy_t h, const double *b, double *x, double tolerance,
                                int32_t max_iterations, int32_t *n_iterations, double *final_residual,
                                double *residual_history, int32_t history_len);
/* Right-preconditioned flexible GMRES(restart), dealii::SolverFGMRES: the preconditioner may be non-symmetric (the cycle with
 * solver.amg.pre_smoothing_levels 0) and may change from one iteration to the next (a preconditioner rounded to float), neither
 * of which CG admits.  Same stopping rule and outputs as mfmg_hip_hierarchy_solve_cg: the absolute l2 norm of the residual -- here
 * the residual norm |g_{j+1}| of the least-squares problem, which is what residual_history receives per iteration -- against
 * `tolerance`; ||r_0|| <= tolerance returns 0 iterations with x unchanged; MFMG_HIP_ERROR_RUNTIME without convergence, outputs
 * filled, x updated with what was reached.  x += Z y after `restart` (>= 1) vectors, then the true residual is recomputed and
 * tested (it is not a history entry of its own); a breakdown h_{j+1,j} = 0 ends the cycle with the update, and the true residual
 * recomputed after it -- not the estimate, which a singular Hessenberg matrix makes zero too -- is that iteration's history entry
 * and decides convergence.  An allocation of the basis that fails returns an error and leaves no basis behind: retry with a
 * smaller restart.
 *   preconditioner_fp32 0: z = Hierarchy::vmult(v); 1: the FP32 fine level (mfmg_hip_hierarchy_apply_f32) on the narrowed v, its
 *   result widened -- the outer iteration, operator and basis stay FP64 (needs "fine level precision" float, otherwise
 *   MFMG_HIP_ERROR_INVALID_ARGUMENT).  Either preconditioner starts from zero whatever "is preconditioner" says.
 * Orthogonalisation: classical Gram-Schmidt twice with the fused kernels of krylov_basis.hpp; one device-to-host copy per
 * iteration.  The basis (2 restart + 1 vectors, restart capped by max_iterations) is owned by the hierarchy and kept for the next
 * solve.  "internal numbering" lexicographic: two launches of "dof_permutation" per solve.
 * On a context with a communicator b and x are the rank's local vectors (ghost entries are don't-care on entry), the basis is sized
 * by the local vectors, dots and norms run over the owned entries and are summed over the ranks: three all-reduces per iteration
 * through the registered transport (the coefficients of the two Gram-Schmidt passes, ||w||^2), and no other host round trip.  All
 * ranks return the same iteration count and history.  preconditioner_fp32 1 there: v is narrowed and z widened over the whole local
 * vector, the FP32 level exchanges the ghost entries it reads; the basis, the dots and the three all-reduces are unchanged. */
int mfmg_hip_hierarchy_solve_fgmres(mfmg_hip_hierarchy_t h, const double *b, double *x, double tolerance,
                                    int32_t max_iterations, int32_t restart, int32_t preconditioner_fp32,
                                    int32_t *n_iterations, double *final_residual,
                                    double *residual_history, int32_t history_len);
/* The kernels of that orthogonalisation on their own (tests).  V, Z: column-major device arrays with leading dimension ld >= n,
 * columns 0 .. j; h_out (j + 1 doubles), norm_out (1), y (j + 1): device memory.  16-byte loads where V, w (x) are 16-byte aligned
 * and ld is even, scalar ones otherwise.
 *   orthogonalize: `passes` times { c = V^T w; w -= V c }; h_out = the sum of the c, norm_out = ||w|| of the result
 *   combine:       x += sum_i y[i] Z_i */
int mfmg_hip_krylov_orthogonalize(mfmg_hip_context_t ctx, int64_t n, int64_t ld, int32_t j, const double *V, double *w,
                                  double *h_out, double *norm_out, int32_t passes);
int mfmg_hip_krylov_combine(mfmg_hip_context_t ctx, int64_t n, int64_t ld, int32_t j, const double *Z, const double *y, double *x);
/* orthogonalize over the OWNED entries of a rank's local vectors alone: V, w hold the lexicographic box of local_nodes[3] nodes
 * (x fastest) with `comps` entries per node, of which the nodes [own0, own0 + own_n) per axis are owned; ld >= the entries of the
 * local box.  h_out and norm_out are sums over the owned entries; the ghost entries of V and w never enter a result and those of w
 * are not written.  The kernels of one rank of a distributed mfmg_hip_hierarchy_solve_fgmres, launched on a context WITHOUT a
 * communicator (MFMG_HIP_ERROR_INVALID_ARGUMENT otherwise): the sum over the ranks is the identity (tests). */
int mfmg_hip_krylov_orthogonalize_box(mfmg_hip_context_t ctx, const int64_t *local_nodes, const int64_t *own0, const int64_t *own_n,
                                      int32_t comps, int64_t ld, int32_t j, const double *V, double *w, double *h_out,
                                      double *norm_out, int32_t passes);
int mfmg_hip_hierarchy_n_levels(mfmg_hip_hierarchy_t h, int32_t *n_levels);
int mfmg_hip_hierarchy_level_size(mfmg_hip_hierarchy_t h, int32_t level, int64_t *n);
/* Level::get_operator()->apply (level.hpp:30-33) */
int mfmg_hip_hierarchy_operator_apply(mfmg_hip_hierarchy_t h, int32_t level, const double *x, double *y, int mode);
/* Level::get_smoother()->apply(b, x) (level.hpp:40-43) */
int mfmg_hip_hierarchy_smoother_apply(mfmg_hip_hierarchy_t h, int32_t level, const double *b, double *x);
/* levels[level].get_restrictor()->apply(in, out, mode): level >= 1 (level.hpp:35-38) */
int mfmg_hip_hierarchy_restrictor_apply(mfmg_hip_hierarchy_t h, int32_t level, const double *in, double *out, int mode);
/* How the restrictor of `level` is evaluated (tests: which kernel paths a case reaches).  fields[0..10]:
 *   0 1 = agglomerate-wise form (structured_restrictor.hpp), 0 = CSR (all other fields 0)
 *   1 eigenvectors per agglomerate, 2-4 cells per agglomerate along x, y, z
 *   5 1 = planes stored in float
 *   6 agglomerates evaluated from the reference block table, 7 further block classes, 8 agglomerate positions listed
 *     for the thread-per-node part of the 2 x 2 x 2 prolongation kernel
 *   9 restriction kernel: 1 rows, 2 pairs of 2 x 2 x 2 agglomerates, 3 pairs of any agglomerate
 *  10 prolongation kernel: 1 one thread per node, 2 the 2 x 2 x 2 block kernel
 *  11 the block kernel in its marching form (0: a thread per agglomerate position, MFMG_SR_PROLONG=block) */
#define MFMG_HIP_RESTRICTOR_FORM_FIELDS 12
int mfmg_hip_hierarchy_restrictor_form(mfmg_hip_hierarchy_t h, int32_t level, int32_t *fields, int32_t n);
/* What solved the agglomerate eigenproblems of the restrictor, parameter "restrictor.eigensolver" device (default) | host | lanczos:
 *   device   dense cyclic Jacobi, one wavefront per agglomerate (amge_device.hip), for agglomerates of at most 64 nodes; larger
 *            ones are solved by the same method on the host cores
 *   host     dense cyclic Jacobi on the host cores
 *   lanczos  batched matrix-free Lanczos with full reorthogonalisation on the device (amge_lanczos.hip), agglomerates of at most
 *            729 nodes (8 x 8 x 8 cells; MFMG_HIP_ERROR_NOT_IMPLEMENTED beyond: an explicit request is not served by another
 *            solver).  It honours eigensolver.tolerance (default 1e-14, taken as given), eigensolver.max_iterations (200) and
 *            eigensolver.percent_overshoot (5) and returns the `krylov` selection; eigensolver.selection lapack with it is
 *            MFMG_HIP_ERROR_RUNTIME.  An agglomerate that stops at max_iterations unconverged is counted, not an error.
 * fields[0..6]:
 *   0 solver that ran: 0 dense on the host cores, 1 dense on the device, 2 Lanczos
 *   1 nodes of a full agglomerate, 2 agglomerates, 3 eigenproblems solved (identical agglomerates share one solve)
 *   4 largest number of Lanczos steps of an agglomerate, 5 agglomerates whose run ended by breakdown (the Krylov space of the start
 *     vector is invariant: harmless), 6 agglomerates unconverged at max_iterations   (4-6: 0 for the dense solvers)
 * On several ranks every rank reports its own agglomerates: the solver hooks in per rank where the dense kernel does.
 * *_seconds: wall time of the Lanczos kernel of that setup (0 for the dense solvers). */
#define MFMG_HIP_EIGENSOLVER_INFO_FIELDS 7
int mfmg_hip_hierarchy_restrictor_eigensolver_info(mfmg_hip_hierarchy_t h, int64_t *fields, int32_t n);
int mfmg_hip_hierarchy_restrictor_eigensolver_seconds(mfmg_hip_hierarchy_t h, double *seconds);
/* The agglomerate eigen-solves of the restrictor setup on their own, with the device solver that `params_info` names
 * (restrictor.eigensolver device | lanczos; the agglomeration / eigensolver sections as mfmg_hip_hierarchy_create reads them;
 * `matrix_free` picks the evaluator flavour, i.e. the default eigensolver.variant mf instead of device).
 * Size query: with all five output arrays NULL only *n_agglomerates, *n_eigenvectors and *n_nodes (node stride of `weights`) are
 * set.  Otherwise host arrays, agglomerates x fastest:
 *   n_vec[a]                       vectors selected for agglomerate a
 *   eigenvalues[a * n_eig + e]     eigenvalue of vector e (for eigensolver.variant host with the shift taken off)
 *   weights[(a * n_eig + e) * n_nodes + l]   diag_loc[l] * vector e at local node l (x fastest inside the agglomerate), 0 on
 *                                  nodes that are not part of the eigenproblem
 *   iterations[a]                  Lanczos steps (0 for the dense solver)
 *   flags[a]                       bit 0: converged, bit 1: ended by breakdown */
int mfmg_hip_amge_eigen(mfmg_hip_context_t ctx, const mfmg_hip_mesh_desc *mesh, const char *params_info, int matrix_free,
                        int64_t *n_agglomerates, int32_t *n_eigenvectors, int32_t *n_nodes, int32_t *n_vec, double *eigenvalues,
                        double *weights, int32_t *iterations, int32_t *flags);
/* out = (A R^T) in for the A R^T the coarse operator of `level` was formed from -- `fast_multiply_transpose()` when the
 * parameter `fast_ap` is true (include/mfmg/common/hierarchy.hpp:214-221), `a->multiply_transpose(restrictor)` otherwise.
 * Kept only by a hierarchy built with `keep_ap = true` (tests: the comparison of tests/test_hierarchy.cc:507-642). */
int mfmg_hip_hierarchy_ap_apply(mfmg_hip_hierarchy_t h, int32_t level, const double *in, double *out);
/* coarsest Level::get_solver()->apply(b, x) (level.hpp:45-48) */
int mfmg_hip_hierarchy_coarse_apply(mfmg_hip_hierarchy_t h, const double *b, double *x);
/* Replace the restrictor (and re-derive the Galerkin coarse operator + coarse solver)
 * from a host CSR so that CPU and GPU runs can share the identical R. */
int mfmg_hip_hierarchy_set_restrictor(mfmg_hip_hierarchy_t h, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                      const int32_t *row_ptr_host, const int32_t *col_host, const double *val_host);
/* b_coarse = R (A x - b): the residual of hierarchy.hpp:281-286 and its restriction (:288-290) as the cycle computes them.
 * Where the rows of R A repeat themselves from agglomerate to agglomerate (constant coefficient) this is ONE kernel
 * over x and b (residual_restriction.hip; `restrictor.fused_residual false` or MFMG_FUSED_RESIDUAL=0 switch it off);
 * otherwise the fused residual kernel followed by the restriction.  *_classes: number of agglomerate classes of the
 * one-pass form, 0 when the two-step form is in use. */
int mfmg_hip_hierarchy_restrict_residual(mfmg_hip_hierarchy_t h, int32_t level, const double *x, const double *b, double *b_coarse);
int mfmg_hip_hierarchy_residual_restriction_classes(mfmg_hip_hierarchy_t h, int32_t level, int32_t *n_classes);
/* What a launch of the one-pass form consists of (tests: which path a case reaches).  fields[0..9], all 0 where the form is not built:
 *   0 agglomerate classes, 1 runs of 62 agglomerates per row (row-wise part), 2 last agglomerate index i of a row in that part
 *   3 agglomerates in the list (sixteen lanes each), 4 runs of the row-wise part whose agglomerates are in the list instead
 *   5 kernel: 1 the tile form, 2 the row-wise kernel (MFMG_RR_KERNEL=rows)
 *   6 agglomerate layers per tile (MFMG_RR_TILE_LAYERS when the tables were built, else chosen for the grid), 7 tiles along y,
 *   8 tiles (6-8: 0 for the row-wise kernel), 9 workgroups of the row-wise part (a multiple of 8)
 * Computed by the function the launch takes its grid from. */
#define MFMG_HIP_RESIDUAL_RESTRICTION_FORM_FIELDS 10
int mfmg_hip_hierarchy_residual_restriction_form(mfmg_hip_hierarchy_t h, int32_t level, int64_t *fields, int32_t n);
/* The one-pass form on float x and b, as the FP32 fine level (mfmg_hip_hierarchy_apply_f32) runs it: x and b are widened as they
 * are loaded, all arithmetic and b_coarse are FP64.  There is no two-step form behind this entry (that one rounds the residual to
 * float): MFMG_HIP_ERROR_NOT_IMPLEMENTED where the one-pass form is not built (*_classes == 0) or the context has a communicator. */
int mfmg_hip_hierarchy_restrict_residual_f32(mfmg_hip_hierarchy_t h, int32_t level, const float *x, const float *b, double *b_coarse);
/* restrictor / coarse operator download for inspection: query sizes with *_shape first */
int mfmg_hip_hierarchy_get_restrictor(mfmg_hip_hierarchy_t h, mfmg_hip_csr_t *r_borrowed);
int mfmg_hip_hierarchy_get_coarse_operator(mfmg_hip_hierarchy_t h, mfmg_hip_csr_t *ac_borrowed);
/* the operator of level 0 when it is an assembled matrix ("HipMeshEvaluator": evaluate_global,
 * include/mfmg/cuda/cuda_mesh_evaluator.cuh:39-45); borrowed like the two above; an error for a matrix-free hierarchy */
int mfmg_hip_hierarchy_get_fine_operator(mfmg_hip_hierarchy_t h, mfmg_hip_csr_t *a_borrowed);
/* levels of the multilevel coarse solver (0 when the coarse solver is direct / pcg): operator A_l, prolongator P_l,
 * its transpose as stored for the restriction (which = 0 / 1 / 2; a borrowed handle, valid until the next call) and the
 * Chebyshev bounds of its smoother.  which = 3: the smoothed prolongator of the cycle, P~ = (I - beta D^-1 A_l) P_l, of the
 * levels that apply prolongation and post-smoothing as one operator; MFMG_HIP_ERROR_NOT_IMPLEMENTED ("not built") on the others */
int mfmg_hip_hierarchy_coarse_amg_levels(mfmg_hip_hierarchy_t h, int32_t *n_levels);
/* distributed runs: index of the first level of the multilevel coarse solver that is gathered and solved redundantly on
 * every rank (-1: one rank); the levels before it are coupled across the ranks by halo exchanges */
int mfmg_hip_hierarchy_coarse_amg_gather_level(mfmg_hip_hierarchy_t h, int32_t *level);
int mfmg_hip_hierarchy_coarse_amg_get(mfmg_hip_hierarchy_t h, int32_t level, int32_t which, mfmg_hip_csr_t *borrowed);
int mfmg_hip_hierarchy_coarse_amg_smoother(mfmg_hip_hierarchy_t h, int32_t level, int32_t *degree, double *lambda_min,
                                           double *lambda_max);
/* what the setup of the aggregation hierarchy did on `level`, MFMG_HIP_AMG_SETUP_INFO_FIELDS values:
 *   [0]      reach of the level's operator in nodes (0: a hierarchy without a node grid)
 *   [1..3]   probe period per axis of the prolongator P_l            (0: not probed)
 *   [4..6]   probe period per axis of the next operator P^T A P      (0: not probed)
 *   [7..9]   probe period per axis of the smoothed prolongator P~    (0: not probed, or none)
 *   [10]     how the next operator was formed: 0 probes, 1 CSR product on the device, 2 product on the host
 *   [11]     1: the level belongs to the replicated tail (built by the host code of one rank)
 *   [12]     1: the level has a smoothed prolongator (which = 3 of mfmg_hip_hierarchy_coarse_amg_get)
 * (the last level forms nothing: its periods are 0) */
#define MFMG_HIP_AMG_SETUP_INFO_FIELDS 13
int mfmg_hip_hierarchy_coarse_amg_setup_info(mfmg_hip_hierarchy_t h, int32_t level, int32_t *values, int32_t n_values);
/* smoother polynomial actually used (degree, lambda_min, lambda_max) */
int mfmg_hip_hierarchy_smoother_info(mfmg_hip_hierarchy_t h, int32_t *degree, double *lambda_min, double *lambda_max);
/* polynomial terms the fine-level smoother runs as ONE sweep over the mesh (mf_cheb_fused.hip): by Smoother::apply (in place: the last
 * term stays a launch of its own) and by the out-of-place form Hierarchy::apply uses where the whole polynomial fits a sweep;
 * 0 = one launch per term (eight coefficients per cell, a numbering the kernel cannot compute, smoother.fused_terms 1) */
int mfmg_hip_hierarchy_smoother_sweep_terms(mfmg_hip_hierarchy_t h, int *terms_in_place, int *terms_out_of_place);
/* tile of that sweep for n_terms terms: n_waves wavefronts of tile_y cell rows, tile_z owned layers (0, 0, 0 sets the heuristic) */
int mfmg_hip_hierarchy_sweep_tile(mfmg_hip_hierarchy_t h, int n_terms, int *n_waves, int *tile_y, int *tile_z);
int mfmg_hip_hierarchy_set_sweep_tile(mfmg_hip_hierarchy_t h, int n_waves, int tile_y, int tile_z);
/* tile of the matrix-free fine-level operator (n_waves, rows per wavefront, layers), see mfmg_hip_mf_laplace_get_tile */
int mfmg_hip_hierarchy_operator_tile(mfmg_hip_hierarchy_t h, int *n_waves, int *tile_y, int *tile_z);
int mfmg_hip_hierarchy_set_operator_tile(mfmg_hip_hierarchy_t h, int n_waves, int tile_y, int tile_z); /* 0 = automatic */
/* TimerOutput-style accumulated wall times of the sections of hierarchy.hpp:164-271 as a text table */
int mfmg_hip_hierarchy_timer_report(mfmg_hip_hierarchy_t h, char *buf, size_t buf_size);

/* ---- host-side setup pieces (no GPU needed; SURVEY.md 8f rank 1-2, kept on the host cores) ----
 * Opaque host CSR results are returned through a handle and copied out with *_host_csr_get. */
typedef struct mfmg_hip_host_csr_s *mfmg_hip_host_csr_t;
int mfmg_hip_host_csr_shape(mfmg_hip_host_csr_t m, int64_t *n_rows, int64_t *n_cols, int64_t *nnz);
int mfmg_hip_host_csr_get(mfmg_hip_host_csr_t m, int32_t *row_ptr, int32_t *col, double *val);
int mfmg_hip_host_csr_destroy(mfmg_hip_host_csr_t m);
/* Laplace<dim>::assemble_system on the structured mesh (tests/laplace.hpp:154-204); semantics 0: assembled
 * (AffineConstraints elimination), 1: matrix-free (identity rows on constrained DoFs). Host arrays only. */
int mfmg_hip_host_assemble_matrix(const mfmg_hip_mesh_desc *mesh, int semantics, mfmg_hip_host_csr_t *out);
/* AMGe restrictor (include/mfmg/common/amge.templates.hpp:271-325,412-499;
 * include/mfmg/dealii/amge_host.templates.hpp:278-483; include/mfmg/cuda/amge_device.templates.cuh:217-310).
 * `params_info`: INFO text with the eigensolver / agglomeration sections; `matrix_free` picks the evaluator flavour. */
int mfmg_hip_host_build_restrictor(const mfmg_hip_mesh_desc *mesh, const char *params_info, int matrix_free,
                                   mfmg_hip_host_csr_t *out);
/* A_c = R (A R^T) (include/mfmg/common/hierarchy.hpp:214-233) from operator rows generated on the fly */
int mfmg_hip_host_galerkin(const mfmg_hip_mesh_desc *mesh, int semantics, int64_t n_rows, int64_t nnz,
                           const int32_t *r_row_ptr, const int32_t *r_col, const double *r_val,
                           mfmg_hip_host_csr_t *out);
/* Multilevel coarse solver setup ("solver.type amg": smoothed aggregation, the role ML plays at
 * source/dealii/dealii_solver.cc:48-66): level operators A_l and prolongators P_l on the host.
 * which = 0: A_l, 1: P_l (from level l+1 to l; empty on the last level). */
typedef struct mfmg_hip_host_amg_s *mfmg_hip_host_amg_t;
/* grid_dims / node_of_row / component_of_row (optional, may be NULL): rows live on nodes of a structured
 * grid (for the AMGe coarse level: the agglomerates, x fastest), several rows (components) per node;
 * aggregates are 2x2x2 blocks of nodes, one aggregate per component. */
int mfmg_hip_host_amg_build(int64_t n_rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col, const double *val,
                            const double *near_null, const int32_t *grid_dims, const int32_t *node_of_row,
                            const int32_t *component_of_row, const char *params_info, mfmg_hip_host_amg_t *out);
int mfmg_hip_host_amg_n_levels(mfmg_hip_host_amg_t amg, int32_t *n_levels);
int mfmg_hip_host_amg_get(mfmg_hip_host_amg_t amg, int32_t level, int32_t which, mfmg_hip_host_csr_t *out);
int mfmg_hip_host_amg_destroy(mfmg_hip_host_amg_t amg);

/* boost::property_tree INFO round trip of the parameter reader (tests/test_utils.cc:23-60 exercises ptree2plist) */
int mfmg_hip_host_params_get(const char *params_info, const char *path, char *value_buf, size_t buf_size);


/* ---- the cycle on a block of vectors (layout and checks as above) ----
 * mfmg_hip_hierarchy_apply_block: x[c] = the result of mfmg_hip_hierarchy_apply(b[c], x[c]) for every column, bit for bit;
 * _vmult_block the same with the argument order of _vmult; _smoother_apply_block that of _smoother_apply.  Where the fine level
 * has the block kernel the block is taken in the groups of mfmg_hip_block_groups and pre-smoothing, residual and post-smoothing
 * run as launches on the group; the restriction of the group's residuals and the prolongation of its corrections are one launch
 * each where the restrictor has block transfers (below), and the coarse cycle runs on the group where the coarse solver has a
 * block width above 1 (mfmg_hip_hierarchy_coarse_block_info below), column by column otherwise.  Elsewhere the one-vector
 * entry point runs per column.  With "internal numbering" lexicographic the columns are gathered into and scattered out of the
 * library's block workspace (one group wide).
 * mfmg_hip_hierarchy_block_info: fields[0] width of the widest group the fine level runs as one launch (1 = the loop over the
 * columns), fields[1] launches of mf_laplace_block_kernel and fields[2] columns that went through the one-vector entry point in
 * the last block call. */
#define MFMG_HIP_BLOCK_INFO_FIELDS 3
int mfmg_hip_hierarchy_apply_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const double *b, double *x);
int mfmg_hip_hierarchy_vmult_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, double *x, const double *b);
int mfmg_hip_hierarchy_smoother_apply_block(mfmg_hip_hierarchy_t h, int32_t level, int32_t n_vectors, int64_t ld, const double *b, double *x);
int mfmg_hip_hierarchy_block_info(mfmg_hip_hierarchy_t h, int64_t *fields);

/* ---- stored-value SpMV and the coarse cycle on a block of vectors (additions, no change of the ABI version) ----
 * mfmg_hip_csr_launch_block: mfmg_hip_csr_launch on the n_vectors columns of blocks -- column c of x at x + c ld_x, of b, x_prev
 * and out at c ld_out (the matrix may be rectangular); dinv is ONE vector shared by the columns.  Every column gets the bits of
 * mfmg_hip_csr_launch on that column.  The block is cut by mfmg_hip_block_groups; where mfmg_hip_csr_block_info reports the width
 * 4 a group of 4 or 2 columns is one launch that reads the stored values once (profiler name csr_block_kernel): a matrix whose
 * launch is exactly one kernel over values that do not repeat -- mfmg_hip_csr_form kind 2 or 3 with field 8 (regular) 0, or kind
 * 4.  Elsewhere (tables, node classes, twins, listed rows, a released matrix, and the CSR kernels unless
 * mfmg_hip_csr_set_block_csr below turned their block forms on), and for a single column, the one-vector kernels run column by column.  MFMG_HIP_ERROR_INVALID_ARGUMENT: n_vectors outside 1..64, a leading dimension below
 * the vector size or odd, a base not aligned to 16 bytes, out overlapping x, a null operand the mode reads.
 * mfmg_hip_csr_block_info: fields[0] the width (4 or 1), fields[1] launches of the block kernels and fields[2] columns that went
 * through the one-vector kernels, of all mfmg_hip_csr_launch_block calls on the matrix so far.
 * mfmg_hip_hierarchy_coarse_apply_block: mfmg_hip_hierarchy_coarse_apply on every column of the blocks b and x (one leading
 * dimension; layout and checks of the block entry points above), bit for bit.  With solver.type amg the cycle of the aggregation
 * hierarchy runs on groups of 4 and 2 columns, every matrix that has the block kernels read once per group; the loop over the
 * columns with solver.amg.n_cycles > 1, a gathered level, a communicator, and for the other solver types.
 * mfmg_hip_hierarchy_coarse_block_info: fields[0] the widest group any matrix of the coarse cycle takes (1: the loop), and for
 * the last block call of the coarse solver (the one above, or inside mfmg_hip_hierarchy_apply_block / _vmult_block / a block
 * solve) fields[1] launches of the block kernels, fields[2] one-vector launches of the matrices of the cycle. */
int mfmg_hip_csr_launch_block(mfmg_hip_csr_t a, int mode, int32_t n_vectors, int64_t ld_x, const double *x, int64_t ld_out, const double *b,
                              const double *dinv, const double *x_prev, double alpha, double beta, double *out);
int mfmg_hip_csr_block_info(mfmg_hip_csr_t a, int64_t fields[3]);
int mfmg_hip_hierarchy_coarse_apply_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const double *b, double *x);
int mfmg_hip_hierarchy_coarse_block_info(mfmg_hip_hierarchy_t h, int64_t fields[3]);

/* ---- block forms of the CSR kernels (additions, no change of the ABI version) ----
 * Off by default: a matrix on a CSR kernel (mfmg_hip_csr_form kind 0 or 1) reports the width 1 and runs column by column.
 * mfmg_hip_csr_set_block_csr(a, 1, info) turns the block forms of the three CSR kernels on for this matrix: where it is FP64 and
 * its CSR arrays are there, mfmg_hip_csr_block_info then reports 4 and a group of 4 or 2 columns is ONE launch that reads val and
 * col once (profiler name csr_block_kernel), every column with the bits of mfmg_hip_csr_launch.  The route is read per call, so
 * mfmg_hip_csr_set_kernel afterwards keeps working.  Matrices on tables, node classes, twins, with listed rows, in float or
 * released keep the width 1, stored planes and row base keep 4.  info[0] the width after the call, info[1] the kernel of a group
 * of 4 and info[2] of a group of 2: 0 none, 1 lanes, 2 row_block, 3 lds.  A group of an LDS-cached matrix whose windows of x,
 * with the table of row pointers, pass 80 KiB takes the lanes kernel at the same lanes per row.
 * mfmg_hip_hierarchy_set_block_csr: the same switch on every FP64 matrix the cycle applies -- the assembled fine operator, a
 * restrictor given as CSR, the first coarse operator, A, P^T, P and P~ of every aggregation level and the two triangular inverses
 * of the bottom, whose solve then runs on the group too.  *n_matrices: how many of them now report the width 4 through a CSR
 * kernel.  Between block calls at any time; MFMG_HIP_ERROR_INVALID_ARGUMENT on a context with a communicator. */
int mfmg_hip_csr_set_block_csr(mfmg_hip_csr_t a, int on, int32_t info[3]);
int mfmg_hip_hierarchy_set_block_csr(mfmg_hip_hierarchy_t h, int on, int32_t *n_matrices);
/* What mfmg_hip_csr_set_block_csr(.., 1, info) reports on the FP32 instance of the matrix class built from these arrays (the
 * values narrowed): the block forms are FP64 only, so width 1 and no route.  The C boundary hands out no FP32 matrix; this is the
 * one way to ask. */
int mfmg_hip_csr_block_csr_info_f32(mfmg_hip_context_t ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *row_ptr_host,
                                    const int32_t *col_host, const double *val_host, int32_t info[3]);

/* ---- restriction and prolongation on a block of vectors (additions, no change of the ABI version) ----
 * mfmg_hip_hierarchy_restrictor_apply_block: mfmg_hip_hierarchy_restrictor_apply(level, in[c], out[c], mode) for every column,
 * bit for bit (column c of `in` at in + c * ld_in, of `out` at out + c * ld_out).  mode is MFMG_HIP_NO_TRANS, MFMG_HIP_TRANS or
 * MFMG_HIP_TRANS_SUBTRACT.  1 to 64 vectors; each leading dimension at least the size of its vectors and even; the bases aligned to
 * 16 bytes; the blocks must not overlap.  A restrictor in the agglomerate-wise form reads its stored values once per group of 4
 * or 2 columns (the groups of mfmg_hip_block_groups), a single column and every other restrictor go through the one-vector
 * kernels.  A context with a communicator is refused.  With "internal numbering" lexicographic and level 1 the fine side is
 * gathered into and scattered out of the library's block workspace column by column.
 * mfmg_hip_hierarchy_transfer_block_info: fields[0] columns of the widest block restriction of `level` (1 = the loop over the
 * columns), fields[1] the same of its prolongation (1 for the table-driven 2 x 2 x 2 kernels, which read no stored values per
 * agglomerate); of the last block call on this hierarchy (a cycle, a solve or _restrictor_apply_block): fields[2] launches of
 * the block restriction, fields[3] launches of the block prolongation, fields[4] columns whose restriction or prolongation went
 * through the one-vector kernels. */
#define MFMG_HIP_TRANSFER_BLOCK_INFO_FIELDS 5
int mfmg_hip_hierarchy_restrictor_apply_block(mfmg_hip_hierarchy_t h, int32_t level, int32_t n_vectors, int64_t ld_in, const double *in,
                                              int64_t ld_out, double *out, int mode);
int mfmg_hip_hierarchy_transfer_block_info(mfmg_hip_hierarchy_t h, int32_t level, int64_t fields[5]);

/* ---- preconditioned CG on a block of right-hand sides (additions, no change of the ABI version) ----
 * mfmg_hip_hierarchy_solve_cg_block: mfmg_hip_hierarchy_solve_cg for every column of the blocks b and x (layout and checks of
 * the block entry points above: 1 .. 64 vectors, an even ld >= n_dofs, bases aligned to 16 bytes, no overlap, no communicator;
 * MFMG_HIP_ERROR_INVALID_ARGUMENT otherwise, as for a negative tolerance or max_iterations).  Per column the semantics are exactly
 * those of the one-vector driver, and so are the BITS of x, the iteration count, the final residual and the history: x holds the
 * initial guess; ||r_0|| <= tolerances[c] gives 0 iterations with x[c] unchanged; residual_history (may be NULL) receives
 * ||r_0||, ||r_1||, ... of column c at residual_history[c * history_ld + i] as far as history_ld reaches; tolerances,
 * n_iterations, final_residuals (n_vectors entries each) are host arrays, the tolerances absolute l2 norms.  Returns
 * MFMG_HIP_ERROR_RUNTIME when any column is unconverged at max_iterations, with all outputs filled.
 * A column that converged (or started converged) takes no further preconditioner or operator application and no vector pass:
 * the columns still iterating are kept in the first slots of the library-owned working blocks r, z, p, A p -- when a slot retires
 * the last active slot's r and p are copied into it (mfmg_hip_block_cg_retire is that plan) -- so the groups of
 * mfmg_hip_block_groups apply to what is left.  Per iteration: the cycle on the active slots as mfmg_hip_hierarchy_vmult_block runs
 * it, one reduction for all (r, z), the direction, the operator on the block, one reduction for all (p, A p), the update with the
 * partial sums of (r, r) folded into the same pass, ONE device-to-host copy and ONE stream synchronisation.  The working blocks
 * (4 n_vectors fine vectors; 6 with "internal numbering" lexicographic, where b and x are gathered once and x is scattered once:
 * 2 n_vectors launches of "dof_permutation" per solve) are owned by the hierarchy and kept for the next solve; an allocation that
 * fails returns an error and leaves nothing behind.
 *   work (may be NULL): [0] column-applications of the preconditioner, [1] of the operator -- both the sum of n_iterations --,
 *   [2] launches of mf_laplace_block_kernel, [3] slot moves (at most n_vectors).
 * Not in this driver: non-symmetric cycles and the FP32 preconditioner (mfmg_hip_hierarchy_solve_fgmres_block below), ranks.
 * mfmg_hip_block_cg_retire (host only): of n_active (0 .. 64) slots those with retire_flags[s] != 0 retire.  Retired slots are
 * filled in ascending order, each from the last slot that survives behind it: moves[2 i], moves[2 i + 1] = from, to (capacity
 * n_active pairs), slot_col[to] = slot_col[from]; afterwards the first n_active_out slots are the survivors.  n_moves is at most the
 * number retired.
 * mfmg_hip_hierarchy_operator_apply_block: y[c] = A x[c] on `level` for every column, with the bits of
 * mfmg_hip_hierarchy_operator_apply (one launch of the block kernel per group where the level has it).
 * The kernels of the driver on their own (tests; a context without a communicator; X, Y, Z, P, AP, R: device blocks of k slots with
 * leading dimension ld >= n; the scalars -- k doubles each -- and slot_col are device arrays):
 *   block_dots          out[s] = (X_s, Y_s), per slot the reduction of the one-vector dot product, bit for bit
 *   block_cg_direction  P_s = Z_s + (rz_new[s] / rz_old[s]) P_s, a zero divisor gives beta = 0; rz_old NULL: P_s = Z_s
 *   block_cg_update     alpha_s = rz[s] / pap[s] (zero divisor: 0); X_{slot_col[s]} += alpha_s P_s in the block X with leading
 *                       dimension ldx; R_s -= alpha_s AP_s; rr_out[s] = (R_s, R_s) of the new R with the bits of block_dots */
int mfmg_hip_hierarchy_solve_cg_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const double *b, double *x,
                                      const double *tolerances, int32_t max_iterations, int32_t *n_iterations,
                                      double *final_residuals, double *residual_history, int32_t history_ld, int64_t *work);
int mfmg_hip_block_cg_retire(int32_t n_active, const int32_t *retire_flags, int32_t *slot_col, int32_t *moves, int32_t *n_moves,
                             int32_t *n_active_out);
int mfmg_hip_hierarchy_operator_apply_block(mfmg_hip_hierarchy_t h, int32_t level, int32_t n_vectors, int64_t ld, const double *x,
                                            double *y);
int mfmg_hip_block_dots(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld, const double *X, const double *Y, double *out);
int mfmg_hip_block_cg_direction(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld, const double *Z, double *P,
                                const double *rz_new, const double *rz_old);
int mfmg_hip_block_cg_update(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld, const double *P, const double *AP, double *R,
                             int64_t ldx, double *X, const int32_t *slot_col, const double *rz, const double *pap, double *rr_out);

/* ---- blocks of vectors on several ranks (additions, no change of the ABI version) ----
 * On a context with a communicator mfmg_hip_hierarchy_apply_block, _vmult_block, _smoother_apply_block, _operator_apply_block and
 * _solve_cg_block take the ranks' LOCAL vectors as columns (ghost entries are don't-care on entry, unspecified in results): on
 * the entries a rank owns a column gets the bits the one-vector call on the same ranks gives that vector.  Whether groups of 4
 * and 2 columns run as blocks is agreed ONCE, when the hierarchy is created: the minimum over the ranks of what each rank's fine
 * operator offers (one collective; mfmg_hip_hierarchy_block_info reports the agreed width, the same on every rank -- 1 where one
 * rank keeps one coefficient per cell or has a tail slab: every rank then loops over the columns).  Where it is 4, a smoother term
 * or residual on a group exchanges the group's x in ONE block exchange and launches the block kernel on the local mesh (not
 * overlapped with interior tiles); restriction, coarse cycle and prolongation run column by column with their own exchanges.
 * _solve_cg_block forms (r, z), (p, A p) and (r, r) over the owned entries of all live slots in one launch each and sums them over
 * the ranks in one all-reduce each: three per iteration whatever n_vectors, plus one for the initial residuals; every rank gets the
 * same counts and histories.  The bits of mfmg_hip_hierarchy_solve_cg on the same ranks hold where the transport sums an element in
 * the same order whatever the length of the message (any transport on two ranks).
 * STILL refused on a communicator (MFMG_HIP_ERROR_INVALID_ARGUMENT): mfmg_hip_mf_laplace_block_launch / _f32_block_launch (launches
 * on one rank's memory, no exchange) and the stand-alone kernel calls mfmg_hip_block_dots / _cg_direction / _cg_update /
 * _block_krylov_*.  (mfmg_hip_hierarchy_apply_f32_block runs on ranks, mfmg_hip_hierarchy_solve_fgmres_block where the context
 * enabled it: see below.)
 * mfmg_hip_context_exchange_block: the forward exchange (owner -> ghost) of the n_vectors columns V + c ld of the fine DoF space
 * (space must be 1), `width` planes deep (the rule of mfmg_hip_context_exchange_f32): ONE packing launch, ONE grouped send/recv,
 * ONE unpacking launch.  Every existing neighbour gets one message: the one-vector message of column 0, then that of column 1,
 * ... -- n_vectors times the one-vector doubles, counted as one exchange.  Slabs pack too.  Layout rules of the block entry points
 * (1 .. 64 columns, ld even and at least the local vector's size, base aligned to 16 bytes).  Nothing happens without a
 * communicator.
 * mfmg_hip_block_dots_box: out[s] = the part of (X_s, Y_s) over the OWNED entries of k slots of a rank's local vectors (the box of
 * mfmg_hip_krylov_orthogonalize_box; ld >= the entries of the local box), formed in the order the one-vector owned dot product
 * forms its rank-local sum: bit-equal to it, whatever the ghost entries hold.  The reduction of a distributed _solve_cg_block,
 * launched on a context WITHOUT a communicator (tests). */
int mfmg_hip_context_exchange_block(mfmg_hip_context_t ctx, int32_t space, int32_t n_vectors, int64_t ld, double *V, int width);
int mfmg_hip_block_dots_box(mfmg_hip_context_t ctx, const int64_t *local_nodes, const int64_t *own0, const int64_t *own_n, int32_t comps,
                            int32_t k, int64_t ld, const double *X, const double *Y, double *out);

/* ---- flexible GMRES on blocks and the FP32 block level on several ranks (additions, no change of the ABI version) ----
 * mfmg_hip_context_set_block_fgmres_on_ranks(ctx, 1) lets mfmg_hip_hierarchy_solve_fgmres_block through on a context with a
 * communicator; without it the call stays refused there (MFMG_HIP_ERROR_INVALID_ARGUMENT), as it always was, so that a caller
 * that relies on the refusal keeps it.  The solve is collective: enable it on the context of EVERY rank, before the solve.
 * The blocks then hold the ranks' local vectors.  Both
 * Gram-Schmidt passes, the norms and the scaling run over the owned entries of ALL live slots in one launch each; the j + 1
 * coefficients of a pass of all live slots cross the ranks in ONE all-reduce, their ||w||^2 in one more: three all-reduces per
 * iteration whatever n_vectors, plus one per cycle start.  Every control decision is taken from all-reduced values, so every rank
 * retires, hands over (a breakdown) and restarts the same columns in the same iteration.  On the entries a rank owns every column
 * gets x, the iteration count, the final residual and the history of mfmg_hip_hierarchy_solve_fgmres on the same ranks where the
 * transport sums an element in the same order whatever the length of the message (any transport on two ranks).  work[] reports as
 * on one rank.
 * mfmg_hip_hierarchy_block_solve_allreduces: *n = the all-reduces of the last mfmg_hip_hierarchy_solve_fgmres_block on this
 * hierarchy, those of columns handed to the one-vector loop included (0 on one rank).
 * mfmg_hip_hierarchy_apply_f32_block and preconditioner_fp32 = 1 on ranks: per group of 4 or 2 float columns ONE
 * mfmg_hip_context_exchange_block_f32 of the group's x, one plane deep, in front of each block launch (not overlapped);
 * restriction, coarse cycle and prolongation per column with their own exchanges.  Whether groups run as blocks is agreed once, when
 * the hierarchy is built (the smallest offer of 4 | 1 over the ranks: mfmg_hip_hierarchy_block_info_f32 fields[0]); where a rank
 * offers 1 every rank loops over the columns.  On owned entries a column has the bits of mfmg_hip_hierarchy_apply_f32 on the same
 * ranks.
 * mfmg_hip_context_exchange_block_f32: mfmg_hip_context_exchange_block for the columns of a FLOAT block (ld even, base aligned to
 * 8 bytes): the packing launch widens into the staging of the FP64 block exchange, the unpacking launch narrows -- the same
 * messages, peers and counters (one exchange, n_vectors times the one-vector doubles); every ghost entry gets the bits of
 * mfmg_hip_context_exchange_f32 of its column.
 * mfmg_hip_block_krylov_orthogonalize_box: mfmg_hip_block_krylov_orthogonalize over the OWNED entries of a rank's local vectors
 * (the box of mfmg_hip_krylov_orthogonalize_box replaces n; vectors of comps * the local nodes entries), on a context WITHOUT a
 * communicator -- the sum over the ranks is the identity (tests).  Per live slot the bits of mfmg_hip_krylov_orthogonalize_box
 * with passes = 2; ghost entries, padding and slots that are not live are neither used nor written.  No float copy: on ranks the
 * driver narrows the whole local vector. */
int mfmg_hip_context_set_block_fgmres_on_ranks(mfmg_hip_context_t ctx, int enable);
int mfmg_hip_hierarchy_block_solve_allreduces(mfmg_hip_hierarchy_t h, int64_t *n);
int mfmg_hip_context_exchange_block_f32(mfmg_hip_context_t ctx, int32_t space, int32_t n_vectors, int64_t ld, float *V, int width);
int mfmg_hip_block_krylov_orthogonalize_box(mfmg_hip_context_t ctx, const int64_t *local_nodes, const int64_t *own0, const int64_t *own_n,
                                            int32_t comps, int32_t k, int64_t ld, int32_t j, int32_t n_live, const int32_t *live_slots,
                                            double *V, double *v_next, double *h_out, double *norm_out);

/* ---- flexible GMRES on a block of right-hand sides (additions, no change of the ABI version) ----
 * mfmg_hip_hierarchy_solve_fgmres_block: mfmg_hip_hierarchy_solve_fgmres for every column of the blocks b and x (layout and checks
 * of the block entry points above; restart >= 1, tolerances >= 0, preconditioner_fp32 0 or 1 -- 1 needs "fine level precision"
 * float --, MFMG_HIP_ERROR_INVALID_ARGUMENT otherwise).  Column c of x, n_iterations[c], final_residuals[c] and the history
 * residual_history[c * history_ld + i] are those of mfmg_hip_hierarchy_solve_fgmres(b_c, x_c, tolerances[c], max_iterations,
 * restart, preconditioner_fp32), bit for bit, the entry recorded after a breakdown included.  Returns MFMG_HIP_ERROR_RUNTIME when
 * any column is unconverged at max_iterations, with all outputs filled.
 * Every column owns a SLOT of the library-owned bases: basis vector j of slot s at V + (j k + s) ld, Z likewise (k = n_vectors,
 * ld the caller's, or n_dofs rounded up to even with "internal numbering" lexicographic, where b and x are gathered once and x is
 * scattered once).  All live columns share the iteration count and the basis length.  Per iteration: the cycle and the operator
 * on every maximal run of consecutive live slots (as mfmg_hip_hierarchy_vmult_block / _operator_apply_block run a block; with
 * preconditioner_fp32 the FP32 cycle on the float copies of the run, as mfmg_hip_hierarchy_apply_f32_block runs a block), both Gram-Schmidt passes and the normalisation with one launch each
 * for all live slots, ONE device-to-host copy and ONE stream synchronisation.  A column that converges gets x += Z y at once and
 * leaves the live list; nothing is copied to close the gap, and the next restart cycle packs the surviving columns into the
 * first slots by changing the slot -> column map alone (mfmg_hip_block_fgmres_plan is that plan).  A column that breaks down
 * (h_{j+1,j} = 0) gets its update and is finished by the one-vector driver from its x and the shared iteration count.
 * Working set, owned by the hierarchy, kept for the next solve, grown on demand: with m = max(1, min(restart, max_iterations))
 * (2 m + 1) k ld doubles for V and Z; with preconditioner_fp32 2 k ld floats; with a permutation 2 k ld doubles for b and x;
 * k (m + 1) 1024 + k 1024 doubles of partial sums, k (3 m + 2) doubles of coefficients, k (2 m + 1) pinned host doubles.  An
 * allocation that fails returns MFMG_HIP_ERROR_DEVICE and leaves nothing behind.
 *   work (may be NULL): [0] column-applications of the preconditioner, [1] of the operator inside Arnoldi steps -- both the sum
 *   of n_iterations --, [2] launches of mf_laplace_block_kernel, [3] cycle-start residuals b - A x (one per column and cycle
 *   start, the first included).
 * mfmg_hip_block_fgmres_plan (host only): of n_slots (0 .. 64) slots those with live[s] != 0 work on, slot_col[s] is the column of
 * slot s.  run_start / run_width / run_groups [n_runs]: the maximal runs of consecutive live slots in ascending order and the
 * number of launches each is cut into; group_width [n_groups]: the widths of those launches, run after run (mfmg_hip_block_groups
 * of each run's width); packed_col [n_packed]: the columns of the live slots in slot order -- the map of the next cycle, whose live
 * slots are the first n_packed.  Every output array holds n_slots entries.
 * The kernels of the driver on their own (tests; a context without a communicator).  V, Z: device blocks in the layout above with
 * an even ld >= n and a base aligned to 16 bytes; live_slots: n_live slots of 0 .. k - 1 in ascending order (host array); slots
 * that are not named are neither read nor written:
 *   block_krylov_orthogonalize  w_s = vector j + 1 of slot s: twice { c = V_s^T w_s; w_s -= V_s c } against the vectors 0 .. j
 *                       of the slot, in place; h_out[s (j + 1) + i] = the summed coefficients, norm_out[s] = ||w_s|| (device
 *                       arrays of k (j + 1) and k doubles); v_next (may be NULL; a block of k slots, ld apart, aligned to 16
 *                       bytes) receives w_s / ||w_s||, zeros for a zero norm, and v_next_f32 (may be NULL) its float copy.  Per
 *                       slot the bits of mfmg_hip_krylov_orthogonalize with passes = 2.
 *   block_krylov_combine  x_{slot_col[s]} += sum_{i <= j} y[s (j + 1) + i] Z_i of slot s for the live slots; x: a block of
 *                       n_x_columns columns with leading dimension ldx >= n, aligned to 8 bytes; slot_col: k entries (host
 *                       array), the live ones different columns of x.  Per slot the bits of mfmg_hip_krylov_combine. */
int mfmg_hip_hierarchy_solve_fgmres_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const double *b, double *x,
                                          const double *tolerances, int32_t max_iterations, int32_t restart,
                                          int32_t preconditioner_fp32, int32_t *n_iterations, double *final_residuals,
                                          double *residual_history, int32_t history_ld, int64_t *work);
int mfmg_hip_block_fgmres_plan(int32_t n_slots, const int32_t *live, const int32_t *slot_col, int32_t *run_start, int32_t *run_width,
                               int32_t *run_groups, int32_t *n_runs, int32_t *group_width, int32_t *n_groups, int32_t *packed_col,
                               int32_t *n_packed);
int mfmg_hip_block_krylov_orthogonalize(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld, int32_t j, int32_t n_live,
                                        const int32_t *live_slots, double *V, double *v_next, float *v_next_f32, double *h_out,
                                        double *norm_out);
int mfmg_hip_block_krylov_combine(mfmg_hip_context_t ctx, int64_t n, int32_t k, int64_t ld, int32_t j, int32_t n_live,
                                  const int32_t *live_slots, const int32_t *slot_col, const double *Z, const double *y,
                                  int32_t n_x_columns, int64_t ldx, double *x);

/* ---- the FP32 fine level on blocks of float vectors (additions, no change of the ABI version) ----
 * A float block: n_vectors (1 .. 64) columns of floats with a common leading dimension, column c at base + c * ld elements, ld >=
 * n_dofs and even, the base aligned to 8 bytes (a lane reads one element at a time); one rank.  The refusals are those of the FP64
 * block entry points.
 * mfmg_hip_mf_laplace_f32_block_launch / _block_available / _set_block_tile / _get_block_tile: as the entry points without _f32
 * above, on the FP32 operator.  Groups of 4 and 2 columns run mf_laplace_block_f32_kernel (the chunk records are read once per
 * group), a single column the one-vector kernel; every column gets the bits of the one-vector FP32 entry point, for every tile.
 * mfmg_hip_hierarchy_apply_f32_block: x[c] = the result of mfmg_hip_hierarchy_apply_f32(b[c], x[c]) for every column, bit for bit
 * (needs "fine level precision" float).  Per group of mfmg_hip_block_groups: pre-smoothing, residual and post-smoothing as block
 * launches, restriction, coarse cycle and prolongation column by column; a group of one, and every group where the FP32 operator
 * has no block kernel (cell-constant layout: the multi-term sweep), runs the one-vector cycle.  With "internal numbering"
 * lexicographic on a renumbered mesh the columns are gathered into and scattered from a library block one by one.
 * mfmg_hip_hierarchy_block_info_f32: fields[0] width of the widest group the FP32 fine level runs as one launch, fields[1] launches
 * of mf_laplace_block_f32_kernel and fields[2] columns that went through the one-vector cycle in the last FP32 block call: the last
 * mfmg_hip_hierarchy_apply_f32_block, or the preconditioner applications of the last mfmg_hip_hierarchy_solve_fgmres_block with
 * preconditioner_fp32 = 1. */
int mfmg_hip_mf_laplace_f32_block_launch(mfmg_hip_mf_laplace_f32_t op, int mode, int32_t n_vectors, int64_t ld, const float *x,
                                         const float *b, const float *x_prev, float alpha, float beta, float *out);
int mfmg_hip_mf_laplace_f32_block_available(mfmg_hip_mf_laplace_f32_t op, int *available);
int mfmg_hip_mf_laplace_f32_set_block_tile(mfmg_hip_mf_laplace_f32_t op, int n_waves, int tile_y, int tile_z);
int mfmg_hip_mf_laplace_f32_get_block_tile(mfmg_hip_mf_laplace_f32_t op, int n_vectors, int *n_waves, int *tile_y, int *tile_z);
int mfmg_hip_hierarchy_apply_f32_block(mfmg_hip_hierarchy_t h, int32_t n_vectors, int64_t ld, const float *b, float *x);
int mfmg_hip_hierarchy_block_info_f32(mfmg_hip_hierarchy_t h, int64_t *fields);

/* ---- Q2 elements: the matrix-free operator and a solver on the refined Q1 cycle (additions, no change of the ABI version) ----
 * LaplaceMatrixFree<3, 2, double> of the reference (FE_Q(2), QGauss(3); tests/laplace_matrix_free.hpp:75-98,129-199) on a
 * structured hex mesh.  The unknowns sit on the lattice N[d] = 2 n_cells[d] + 1, numbered lexicographically with x fastest: the
 * only numbering taken, so there is no index array.  Constrained rows return y_c = x_c, constrained entries of x contribute
 * nothing to other rows.  FP64, 3-D, one rank: dim != 3 and a context with a communicator are refused with
 * MFMG_HIP_ERROR_NOT_IMPLEMENTED, n_dofs >= 2^31 or n_dofs != N[0] N[1] N[2] with MFMG_HIP_ERROR_INVALID_ARGUMENT; there is no
 * FP32 and no block form. */
typedef struct mfmg_hip_q2_mesh_desc
{
  int32_t dim;                  /* 3 */
  int32_t n_cells[3];           /* Q2 cells per direction, x fastest */
  double cell_size[3];          /* h[d] */
  int64_t n_dofs;               /* (2 n_cells[0] + 1)(2 n_cells[1] + 1)(2 n_cells[2] + 1) */
  const double *coefficient;    /* [n_cells_total][27] at the points q = qa + 3 qb + 9 qc of QGauss<1>(3)^3 */
  const uint8_t *constrained;   /* [n_dofs] 1 = Dirichlet-constrained */
  int32_t arrays_on_device;     /* 0: host pointers, 1: device pointers */
} mfmg_hip_q2_mesh_desc;
typedef struct mfmg_hip_mf_laplace_q2_s *mfmg_hip_mf_laplace_q2_t;
/* The coefficients are kept as ONE value per cell where the 27 of every cell are equal (detected on the device) unless
 * mfmg_hip_context_set_cell_constant_layout(ctx, 0) was called before; _cell_constant_layout reports which. */
int mfmg_hip_mf_laplace_q2_create(mfmg_hip_context_t ctx, const mfmg_hip_q2_mesh_desc *mesh, mfmg_hip_mf_laplace_q2_t *out);
int mfmg_hip_mf_laplace_q2_destroy(mfmg_hip_mf_laplace_q2_t op);
int mfmg_hip_mf_laplace_q2_size(mfmg_hip_mf_laplace_q2_t op, int64_t *n_dofs);
int mfmg_hip_mf_laplace_q2_cell_constant_layout(mfmg_hip_mf_laplace_q2_t op, int *in_use);
/* y = A x; res = A x - b; out = x + alpha (x - x_prev) - beta D^-1 (A x - b) (x_prev may be null when alpha == 0).  Device
 * vectors; the output must not alias x, out may be x_prev.  The meaning of the entry points without _q2. */
int mfmg_hip_mf_laplace_q2_vmult(mfmg_hip_mf_laplace_q2_t op, const double *x, double *y);
int mfmg_hip_mf_laplace_q2_residual(mfmg_hip_mf_laplace_q2_t op, const double *x, const double *b, double *res);
int mfmg_hip_mf_laplace_q2_smoother_step(mfmg_hip_mf_laplace_q2_t op, const double *b, const double *x, const double *x_prev,
                                         double alpha, double beta, double *out);
/* compute_diagonal and its inverse, constrained entries 1 (copies into device vectors) */
int mfmg_hip_mf_laplace_q2_diagonal(mfmg_hip_mf_laplace_q2_t op, double *diag);
int mfmg_hip_mf_laplace_q2_diagonal_inverse(mfmg_hip_mf_laplace_q2_t op, double *dinv);
/* The tile of one workgroup in cells whose nodes it owns: tile_x x tile_y cells per layer (one more lane column and row
 * recompute the halo cells of the low faces), tile_z layers per workgroup.  _tile_shapes lists the shapes on offer, three ints
 * each, the default first (*n_shapes of them; `tiles` may be null; needs no context); _set_tile takes one of them or (0, 0, 0)
 * for the default, MFMG_HIP_ERROR_INVALID_ARGUMENT otherwise.  Every shape gives the same bits. */
int mfmg_hip_mf_laplace_q2_tile_shapes(int32_t *n_shapes, int32_t *tiles, int32_t capacity);
int mfmg_hip_mf_laplace_q2_get_tile(mfmg_hip_mf_laplace_q2_t op, int *tile_x, int *tile_y, int *tile_z);
int mfmg_hip_mf_laplace_q2_set_tile(mfmg_hip_mf_laplace_q2_t op, int tile_x, int tile_y, int tile_z);

/* The preconditioner of the Q2 operator: a Chebyshev smoother on it around ONE cycle of a Q1 hierarchy the caller built on the
 * refined problem (2 n cells of size h / 2, the same lattice of unknowns; matrix-free evaluator, one rank, lexicographic
 * numbering).  apply(b, x), always from zero:  x = S(b, 0);  r = A_2 x - b;  x -= mfmg_hip_hierarchy_vmult(r);  x = S(b, x).
 * `params_info`: INFO text whose subtree "high order" holds smoother.degree (default 2; 0: no smoothing, the first and the last
 * step are skipped), smoother.smoothing_range (4), smoother.eig_cg_n_iterations, smoother.lambda_max, smoother.lambda_min (as the
 * smoother of a hierarchy).  The hierarchy and the operator must outlive the object and belong to the same context.
 * MFMG_HIP_ERROR_INVALID_ARGUMENT: the fine level of the hierarchy is not of the operator's size, the two were built on different
 * contexts, or the hierarchy runs in an internal numbering of its own.
 * _smoother_info: degree (0: none), lambda_min, lambda_max of the Chebyshev polynomial.
 * _solve_cg / _solve_fgmres: the argument lists of mfmg_hip_hierarchy_solve_cg / _solve_fgmres without the FP32 flag; the
 * iteration runs on A_2 with _apply as preconditioner.  CG needs a symmetric Q1 cycle (V(1,1), the default).
 * _solve_cg_block / _solve_fgmres_block: MFMG_HIP_ERROR_NOT_IMPLEMENTED (there is no block form). */
typedef struct mfmg_hip_high_order_s *mfmg_hip_high_order_t;
int mfmg_hip_high_order_create(mfmg_hip_hierarchy_t hierarchy, mfmg_hip_mf_laplace_q2_t q2_operator, const char *params_info,
                               mfmg_hip_high_order_t *out);
int mfmg_hip_high_order_destroy(mfmg_hip_high_order_t p);
int mfmg_hip_high_order_apply(mfmg_hip_high_order_t p, const double *b, double *x);
int mfmg_hip_high_order_smoother_info(mfmg_hip_high_order_t p, int32_t *degree, double *lambda_min, double *lambda_max);
int mfmg_hip_high_order_solve_cg(mfmg_hip_high_order_t p, const double *b, double *x, double tolerance, int32_t max_iterations,
                                 int32_t *n_iterations, double *final_residual, double *residual_history, int32_t history_len);
int mfmg_hip_high_order_solve_fgmres(mfmg_hip_high_order_t p, const double *b, double *x, double tolerance, int32_t max_iterations,
                                     int32_t restart, int32_t *n_iterations, double *final_residual, double *residual_history,
                                     int32_t history_len);
int mfmg_hip_high_order_solve_cg_block(mfmg_hip_high_order_t p, int32_t n_vectors, int64_t ld, const double *b, double *x,
                                       const double *tolerances, int32_t max_iterations);
int mfmg_hip_high_order_solve_fgmres_block(mfmg_hip_high_order_t p, int32_t n_vectors, int64_t ld, const double *b, double *x,
                                           const double *tolerances, int32_t max_iterations, int32_t restart);

#ifdef __cplusplus
}
#endif
#endif /* MFMG_HIP_H */
