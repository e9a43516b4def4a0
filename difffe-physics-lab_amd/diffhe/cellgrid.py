"""The uniform cell grid that bins the elements of a mesh by their centroids: the search structure of the density filter
(diffhe/filters.py) and of the point sampler (diffhe/sampling.py), walked on the device by csrc/cell_grid.h."""
from __future__ import annotations

import math

import torch


def cell_index(x: torch.Tensor, lo: torch.Tensor, edge: float, nc, clamp_low: bool) -> torch.Tensor:
    """The linear cell index (int64) of the points x (P, dim) in the grid (lo, edge, nc): floor((x - lo) / edge) per axis,
    clamped at the upper faces, cell = (z * ncy + y) * ncx + x.  clamp_low: the points may lie anywhere -- clamped into
    the grid on both sides (in floating point first: a far point must not overflow the integer)."""
    dim = x.shape[1]
    top = torch.tensor(nc[:dim], device=x.device) - 1
    idx = torch.floor((x - lo) / edge)
    if clamp_low:
        idx = idx.clamp_(-1.0, float(max(nc)))
    idx = torch.minimum(idx.to(torch.int64), top)
    if clamp_low:
        idx = idx.clamp_(min=0)
    cell = idx[:, 0]
    if dim > 1:
        cell = cell + nc[0] * idx[:, 1]
    if dim > 2:
        cell = cell + nc[0] * nc[1] * idx[:, 2]
    return cell


def cell_grid(cent_md: torch.Tensor, min_edge: float):
    """The uniform grid that bins the m centroids cent_md (m, dim): edge = max(min_edge, extent / c) with c^dim <= m, so
    the number of cells stays O(m) however small min_edge is; offsets from the minimum, indices clamped at the upper faces.
    Returns (lo (dim,), edge, [ncx, ncy, ncz], cell_of (m) int32, order (m) int32: the ids sorted by cell and ascending
    within a cell, cell_start (cells + 1) int32)."""
    m, dim = cent_md.shape
    dev = cent_md.device
    lo = cent_md.min(0).values
    ext = (cent_md.max(0).values - lo).cpu()
    c = max(1, int(math.floor(m ** (1.0 / dim) + 1e-9)))
    edge = max(min_edge, float(ext.max()) / c)
    nc = [int(min(math.floor(float(e) / edge), c)) + 1 for e in ext] + [1] * (3 - dim)
    cell = cell_index(cent_md, lo, edge, nc, clamp_low=False)
    n_cells = nc[0] * nc[1] * nc[2]
    cell_sorted, order = torch.sort(cell, stable=True)                 # within a cell: ascending element id
    cell_start = torch.searchsorted(cell_sorted, torch.arange(n_cells + 1, device=dev)).to(torch.int32)
    return lo, edge, nc, cell.to(torch.int32), order.to(torch.int32), cell_start
