"""Mixed materials for the distributed tests: the "linear" coefficient inside a region of the domain, 1.0 outside it -- so that
some ranks of a box partition hold a cell-wise constant coefficient (the operator keeps one value per cell and its smoother may
sweep several terms at once) and others do not.  The function is continuous: 1 on the edge of the region, varying from
quadrature point to quadrature point inside it (the tests are about the exchanges of the ranks, not about a jump).

The region is measured in fractions of the domain's extent along each axis (the meshes of the tests are not all the unit cube):
  "corner": every fraction above 0.625 -- cells no rank but the last one of a 2-per-axis grid holds, owned or ghost (the two
            ghost cell layers of a lower rank reach 0.5625 of the extent at most);
  "rest":   some fraction above 0.625 -- every rank of a 2-per-axis grid but rank 0 holds a varying cell."""
import math

import numpy as np
import torch

import mfmg_amd as M

EDGE = 0.625
_G = (0.5 - 0.5 / math.sqrt(3.0), 0.5 + 0.5 / math.sqrt(3.0))   # (the Gauss points of LaplaceProblem)
PATTERNS = ("corner", "rest")


def global_table(cells, pattern, cell_size):
    """Coefficient table [cell, quadrature point] of the global mesh (CPU, float64)."""
    assert pattern in PATTERNS
    lin = M.LaplaceProblem(cells, "linear", cell_size=cell_size).coefficient
    idx = [torch.arange(c, dtype=torch.float64) for c in cells]
    k, j, i = torch.meshgrid(idx[2], idx[1], idx[0], indexing="ij")
    org = (i.reshape(-1), j.reshape(-1), k.reshape(-1))
    # weight per quadrature point: 0 outside the region, growing from 0 at its edge
    w = torch.empty_like(lin)
    for q in range(8):
        beyond = [torch.clamp(((org[d] + _G[(q >> d) & 1]) / cells[d] - EDGE) / (1.0 - EDGE), min=0.0) for d in range(3)]
        w[:, q] = beyond[0] * beyond[1] * beyond[2] if pattern == "corner" else torch.maximum(torch.maximum(beyond[0], beyond[1]), beyond[2])
    return torch.where(w > 0, 1.0 + (lin - 1.0) * w, torch.ones_like(lin)).contiguous()


def local_rows(part, table):
    """The rows of the global table that belong to the cells of a rank's local (extended) box."""
    lc, gc = part.local_cells, part.cells
    k, j, i = np.meshgrid(*(np.arange(lc[d]) + part.offset[d] for d in (2, 1, 0)), indexing="ij")
    return table[torch.from_numpy(((k * gc[1] + j) * gc[0] + i).reshape(-1))].contiguous()


def local_problem(part, table, device="cpu"):
    """BoxPartition.local_problem of the "linear" material with the rank's rows of the mixed table."""
    prob = part.local_problem("linear", device)
    prob.coefficient = local_rows(part, table).to(prob.coefficient.device)
    return prob


def global_problem(cells, table, cell_size, device="cpu"):
    prob = M.LaplaceProblem(cells, "linear", device=device, cell_size=cell_size)
    prob.coefficient = table.to(prob.coefficient.device)
    return prob


def cell_constant(coefficient):
    """True where every cell carries one value at its eight quadrature points (what the operator's compact layout needs)."""
    return bool((coefficient == coefficient[:, :1]).all())


def expected_constant_ranks(pattern, n_ranks):
    """Ranks whose local table is cell-wise constant: all but the last one ("corner"), rank 0 only ("rest")."""
    return set(range(n_ranks - 1)) if pattern == "corner" else {0}
