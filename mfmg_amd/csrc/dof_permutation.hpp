// "internal numbering" lexicographic: the hierarchy is built and run in the lexicographic numbering of the mesh nodes, whatever
// numbering the caller's cell_dofs carry, and vectors are permuted where they cross the C ABI (c_api.cpp).  This class derives
// the node -> DoF map from the caller's mesh description on the device (the validation of StructuredMesh::build_node_map, as
// kernels), builds the mesh description in the lexicographic numbering, and owns the map, its inverse and the permutation kernel.
#pragma once

#include <vector>

#include "common.hpp"

namespace mfmg
{
class DofPermutation
{
public:
  // throws (runtime error, the message of StructuredMesh::build_node_map) where cell_dofs is not a logically structured Q1 mesh
  // in lexicographic cell order with a one-to-one numbering
  DofPermutation(HipHandle &handle, mfmg_hip_mesh_desc const &mesh);

  // the caller's numbering already is lexicographic: nothing is ever permuted
  bool identity() const { return _identity; }
  int64_t n_dofs() const { return _n; }

  // The mesh in the lexicographic numbering: cell_dofs computed, constrained[n] = caller's constrained[node_dof[n]], the
  // coefficients are the caller's (cells are lexicographic in mfmg_hip_mesh_desc already).  Its arrays live where the caller's
  // do and belong to this object until release_mesh() -- the evaluators copy what they keep.
  mfmg_hip_mesh_desc const &lexicographic_mesh() const { return _lex; }
  void release_mesh();

  // caller's DoF id of lexicographic node n, on the host
  std::vector<int32_t> const &node_dof_host() const { return _node_dof_host; }
  int32_t const *node_dof() const { return _node_dof.data(); }
  int32_t const *dof_node() const { return _dof_node.data(); }

  // out_lex[n] = in_caller[node_dof[n]]; gather2: two vectors in ONE launch, the ids read once; out_caller[node_dof[n]] = in_lex[n].
  // One launch each, timed as "dof_permutation"; in != out.  T = double, float.
  template <typename T>
  void gather(T const *in_caller, T *out_lex) const;
  template <typename T>
  void gather2(T const *b_caller, T const *x_caller, T *b_lex, T *x_lex) const;
  template <typename T>
  void scatter(T const *in_lex, T *out_caller) const;

private:
  template <typename T>
  void launch(bool to_lex, int n_vectors, T const *in0, T *out0, T const *in1, T *out1) const;

  HipHandle &_handle;
  int64_t _n = 0;
  int _N[3] = {1, 1, 1};
  bool _identity = false;
  DeviceBuffer<int32_t> _node_dof, _dof_node;
  std::vector<int32_t> _node_dof_host;
  // the lexicographic mesh description until release_mesh()
  mfmg_hip_mesh_desc _lex;
  DeviceBuffer<int32_t> _lex_cell_dofs;
  DeviceBuffer<uint8_t> _lex_constrained;
  std::vector<int32_t> _lex_cell_dofs_host;
  std::vector<uint8_t> _lex_constrained_host;
};
} // namespace mfmg
