// Batched agglomerate eigenproblems of the spectral AMGe restrictor on the device (amge_device.hip).
#pragma once

#include "amge_structured.hpp"

namespace mfmg
{
// What the kernels of the agglomerate eigenproblems (amge_device.hip, amge_lanczos.hip) are launched with
struct AmgeArgs
{
  int dim, nc;
  int n[3], N[3];    // cells, nodes of the mesh
  int ag[3], cnt[3]; // cells per agglomerate, agglomerates per direction
  int variant;       // 0 device, 1 host, 2 mf
  int krylov;        // selection: 0 lapack, 1 krylov
  int n_eig;
  int use_coefficient;
  int32_t const *node_dof;
  uint8_t const *constrained;
  double const *coefficient; // [cells][nc]
  double const *Kq;          // [nc][nc][nc]
  double *weights;           // [agglomerates][n_eig][NMAX]
  int32_t *n_vec;            // [agglomerates]
  int64_t n_agg;
  int64_t const *list; // nullptr: every agglomerate; otherwise the n_agg agglomerates to solve (representatives)
  double *eigenvalues; // nullptr, or [agglomerates][n_eig]: the eigenvalue of every selected vector
};

// the mesh arrays of AmgeArgs on the device, and the arguments filled in from mesh and options (weights, n_vec, list left unset)
struct AmgeDeviceMesh
{
  DeviceBuffer<int32_t> node_dof;
  DeviceBuffer<uint8_t> constrained;
  DeviceBuffer<double> coefficient, Kq;
  AmgeArgs upload(HipHandle &handle, StructuredMesh const &mesh, RestrictorOptions const &opts, int const cnt[3]);
};

// Identical agglomerates (same shape, constraint flags and coefficients: amge_key_kernel) share one solve unless MFMG_AMGE_MEMO=0:
// when at most half of the agglomerates are representatives, `a.list` / `a.n_agg` are set to them and true is returned.
struct AmgeSharing
{
  DeviceBuffer<int64_t> list, rep_of;
  bool shared = false;
  int64_t n_all = 0;
  bool find(HipHandle &handle, AmgeArgs &a);
  // results of the representatives to every member of their class (amge_spread_kernel); per_agg values and one int per agglomerate
  void spread(HipHandle &handle, int per_agg, double *values, int32_t *ints) const;
};

// agglomerates of at most 64 nodes (one lane of a wavefront per node)
bool amge_device_supported(StructuredMesh const &mesh, RestrictorOptions const &opts);
// weights[(a * n_eig + e) * nmax + l] = diag_loc[l] * (eigenvector e of agglomerate a)[l], n_vec[a] vectors selected
// `eigenvalues` (optional): [(a * n_eig + e)]; `n_solves` (optional): eigenproblems solved (representatives)
void amge_device_eigen(HipHandle &handle, StructuredMesh const &mesh, RestrictorOptions const &opts, int const cnt[3],
                       std::vector<double> &weights, std::vector<int32_t> &n_vec, int &nmax,
                       std::vector<double> *eigenvalues = nullptr, int64_t *n_solves = nullptr);
} // namespace mfmg
