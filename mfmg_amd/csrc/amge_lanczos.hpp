// Batched matrix-free Lanczos eigensolver for the agglomerate eigenproblems of the spectral AMGe restrictor
// (amge_lanczos.hip): agglomerates of up to 729 nodes (8 x 8 x 8 cells), one workgroup per agglomerate.
#pragma once

#include "amge_device.hpp"

namespace mfmg
{
constexpr int kLanczosMaxNodes = 729;

// flags of an agglomerate in the output of amge_lanczos_eigen
constexpr int32_t kAmgeConverged = 1; // the convergence test of the last examination passed (or the Krylov space was complete)
constexpr int32_t kAmgeBreakdown = 2; // the run ended at beta_j <= kLanczosBreakdown * max |theta|

// beta_j <= kLanczosBreakdown * (largest Ritz value of T_j) ends a run: the Krylov space of the start vector is invariant
constexpr double kLanczosBreakdown = 1e-14;

// nodes of a full agglomerate <= kLanczosMaxNodes, dimension 2 or 3
bool amge_lanczos_supported(StructuredMesh const &mesh, RestrictorOptions const &opts);

// What amge_device_eigen returns (weights[(a * n_eig + e) * nmax + l], n_vec[a]; nmax = nodes of a full agglomerate), by Lanczos
// runs from the start vector of the `krylov` selection with full reorthogonalisation; per agglomerate also the eigenvalues
// [(a * n_eig + e)], the Lanczos steps taken and the flags above.  Honours opts.tolerance / max_iterations / percent_overshoot.
void amge_lanczos_eigen(HipHandle &handle, StructuredMesh const &mesh, RestrictorOptions const &opts, int const cnt[3],
                        std::vector<double> &weights, std::vector<int32_t> &n_vec, int &nmax, std::vector<double> &eigenvalues,
                        std::vector<int32_t> &iterations, std::vector<int32_t> &flags, int64_t *n_solves = nullptr,
                        double *kernel_seconds = nullptr);
} // namespace mfmg
