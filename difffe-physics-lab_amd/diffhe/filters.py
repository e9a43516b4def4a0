"""Design regularisation in front of the solvers: a mesh-independent density filter with a physical radius on the
elements of any P1 mesh -- lines, triangles, tetrahedra, structured or not -- with its exact adjoint, and the usual tanh
(Heaviside) projection.  Ours: the reference has neither (kernels declared in include/diffhe_filter.h).

With the centroid c_e (the mean of the vertices) and the size v_e (length / area / volume) of element e and a radius R in
mesh units

    N(i) = { j : |c_i - c_j| < R },    w_ij = max(0, R - |c_i - c_j|)  ("cone")   or   1 on N(i)  ("constant"),
    x~_i = (sum_{j in N(i)} w_ij v_j x_j) / S_i,       S_i = sum_{j in N(i)} w_ij v_j

(`volume_weighted=False` drops v_j from both sums).  `DensityFilter` builds the neighbour table once, on the device: the
elements are binned into a uniform grid of cells with an edge >= R (torch: centroids, sizes, cell index, stable sort,
searchsorted, cumsum), one kernel counts the neighbours of every element in the 3^dim cells around it, one fills the ids
of every row in ascending order and sums S in that order.  The table is the ids alone (int32, an int64 row pointer); the
weights are recomputed from the centroids in the apply kernel, whose forward and adjoint directions are the same gather
(N is symmetric, |c_i - c_j| bitwise so).  Every result is a function of the mesh and R alone, bit for bit.

The filter is linear; `diffhe::density_filter` and `diffhe::density_filter_adjoint` are each other's autograd, so
gradients of any order flow through it.
"""
from __future__ import annotations

import math
import time
import weakref
from typing import Optional

import torch
import torch.nn as nn

from . import _hip
from .cellgrid import cell_grid
from .plan import _stream

# refuse a table of more neighbour ids than this before it is allocated (and one that the free device memory cannot hold)
MAX_NEIGHBOURS = 1 << 36
_FILTERS: "weakref.WeakValueDictionary[int, DensityFilter]" = weakref.WeakValueDictionary()


def heaviside(x: torch.Tensor, beta: float, eta: float = 0.5) -> torch.Tensor:
    """The tanh projection (tanh(beta eta) + tanh(beta (x - eta))) / (tanh(beta eta) + tanh(beta (1 - eta))): 0 -> 0,
    1 -> 1, monotone, a step at eta as beta grows.  Elementwise differentiable torch."""
    beta, eta = float(beta), float(eta)
    if not (beta > 0.0 and math.isfinite(beta)):
        raise ValueError(f"beta must be positive and finite, got {beta!r}")
    if not (0.0 <= eta <= 1.0):
        raise ValueError(f"eta must lie in [0, 1], got {eta!r}")
    lo, hi = math.tanh(beta * eta), math.tanh(beta * (1.0 - eta))
    return (lo + torch.tanh(beta * (x - eta))) / (lo + hi)


def _element_sizes(P: torch.Tensor) -> torch.Tensor:
    """Length / area / volume of the P1 elements with vertices P (m, dim + 1, dim)."""
    dim = P.shape[2]
    if dim == 1:
        return (P[:, 1, 0] - P[:, 0, 0]).abs()
    a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    if dim == 2:
        return 0.5 * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).abs()
    return (a * torch.linalg.cross(b, P[:, 3] - P[:, 0])).sum(1).abs() / 6.0


def check_field(x, m: int, layout: str) -> torch.Tensor:
    """x as a tensor, after the refusals of a field on m elements: (m,) or (B, m), or (m, B) with layout="node"."""
    if layout not in ("sample", "node"):
        raise ValueError(f"Unknown layout: {layout!r}")
    x = x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=torch.float64)
    if layout == "node":
        if x.dim() != 2 or x.shape[0] != m or x.shape[1] < 1:
            raise ValueError(f"layout='node': x must be (m, B) with m={m}, got {tuple(x.shape)}")
    elif x.dim() not in (1, 2) or x.shape[-1] != m or x.shape[0] < 1:
        raise ValueError(f"x must be (m,) or (B, m) with m={m}, got {tuple(x.shape)}")
    return x


class DensityFilter(nn.Module):
    """x~ = H x on one value per element, differentiable to any order; `adjoint` is H^T (see the module docstring).

    Parameters
    ----------
    mesh : FEMesh -- P1 lines, triangles or tetrahedra, any node positions.
    radius : float > 0, in the units of mesh.nodes.
    weight : "cone" (default) or "constant".  volume_weighted : weigh neighbour j by its size v_j (default).
    device : the device of the table; fields are moved there.

    `n_neighbours` is |N(i)| per element, `info` the table's statistics: neighbours (total), longest_row, cells,
    table_bytes, build_seconds.
    """

    def __init__(self, mesh, radius: float, *, weight: str = "cone", volume_weighted: bool = True, device="cuda"):
        super().__init__()
        if mesh.dim not in (1, 2, 3):
            raise NotImplementedError(f"diffhe: the density filter is implemented for 1D, 2D and 3D meshes, got dim {mesh.dim}")
        if mesh.elements.shape[1] != mesh.dim + 1:
            raise NotImplementedError("diffhe: the density filter is implemented for P1 elements only (this mesh has "
                                      f"{mesh.elements.shape[1]} nodes per element)")
        if mesh.nodes.requires_grad:
            raise NotImplementedError("diffhe: node gradients are not implemented for the density filter (mesh.nodes "
                                      "requires grad): the neighbour table is built once from fixed centroids")
        radius = float(radius)
        if not (math.isfinite(radius) and radius > 0.0):
            raise ValueError(f"radius must be positive and finite, got {radius!r}")
        if weight not in ("cone", "constant"):
            raise ValueError(f"Unknown weight: {weight!r} (\"cone\" or \"constant\")")
        if mesh.n_elements < 1:
            raise ValueError("the mesh has no elements")
        self.mesh, self.radius, self.weight, self.volume_weighted = mesh, radius, weight, bool(volume_weighted)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"the density filter runs on a GPU (there is no CPU fallback), got device {device!r}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._build()

    # -- the table --------------------------------------------------------------------------------------
    def _build(self) -> None:
        L, dev, R = _hip.lib(), self.device, self.radius
        t0 = time.perf_counter()
        mesh, dim, m = self.mesh, self.mesh.dim, self.mesh.n_elements
        X = mesh.nodes.detach().to(dev, torch.float64)
        P = X[mesh.elements.detach().to(dev, torch.int64)]                  # (m, dim + 1, dim)
        cent_md = P.sum(1) / float(dim + 1)
        self._cent = cent_md.t().contiguous()                              # (dim, m)
        self._size = _element_sizes(P).contiguous()
        self._vol = self._size if self.volume_weighted else None
        _, _, nc, cell_of, order, cell_start = cell_grid(cent_md, R)
        n_cells = nc[0] * nc[1] * nc[2]
        grid = (cell_of, order, cell_start, nc[0], nc[1], nc[2], R)
        st = _stream(dev)
        count = torch.empty(m, dtype=torch.int32, device=dev)
        L.diffhe_filter_count(self._cent, dim, m, *grid, count, st)
        self.n_neighbours = count.to(torch.int64)
        self._row_ptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        torch.cumsum(self.n_neighbours, 0, out=self._row_ptr[1:])
        total = int(self._row_ptr[-1])                                     # known before anything of that size exists
        limit = MAX_NEIGHBOURS
        if dev.type == "cuda":
            limit = min(limit, torch.cuda.mem_get_info(dev)[0] // 4)
        if total > limit:
            raise ValueError(f"density filter: radius {R!r} gives {total} neighbours on {m} elements, a table of "
                             f"{4 * total} bytes, more than can be allocated ({4 * limit} bytes): use a smaller radius")
        try:
            self._nbr = torch.empty(total, dtype=torch.int32, device=dev)
        except torch.OutOfMemoryError:
            raise ValueError(f"density filter: radius {R!r} gives {total} neighbours on {m} elements; a table of "
                             f"{4 * total} bytes could not be allocated: use a smaller radius") from None
        self._S = torch.empty(m, dtype=torch.float64, device=dev)
        self._inv_S = torch.empty(m, dtype=torch.float64, device=dev)
        L.diffhe_filter_fill(self._cent, self._vol, dim, m, *grid, int(self.weight == "constant"), self._row_ptr,
                             self._nbr, self._S, self._inv_S, st)
        longest = int(self.n_neighbours.max())
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        self.info = {"neighbours": total, "longest_row": longest, "cells": n_cells,
                     "table_bytes": 4 * total + 8 * (m + 1), "build_seconds": time.perf_counter() - t0}

    @property
    def row_ptr(self) -> torch.Tensor:
        """(m + 1,) int64: row i of `neighbours` is [row_ptr[i], row_ptr[i + 1])."""
        return self._row_ptr

    @property
    def neighbours(self) -> torch.Tensor:
        """int32 ids of N(i), row after row, ascending within a row."""
        return self._nbr

    @property
    def weight_sums(self) -> torch.Tensor:
        """(m,) S_i."""
        return self._S

    @property
    def sizes(self) -> torch.Tensor:
        """(m,) v_e, whether or not the filter weighs with them."""
        return self._size

    # -- the operator -----------------------------------------------------------------------------------
    def _apply(self, x: torch.Tensor, adjoint: bool, node_layout: bool, variant: Optional[str] = None) -> torch.Tensor:
        """H x or H^T x of a checked fp64 field on the filter's device.  Element-major and flat fields are read in place
        through their strides.  A sample-major (B, m) field is correct through its strides too but not coalesced
        (variant "strided"); the default, "transpose", is a transposed copy with torch around the element-major call,
        which is faster ("Density filter") and gives the same bits."""
        m = self.mesh.n_elements
        if x.dim() == 2 and not node_layout and (variant or _SAMPLE_MAJOR) == "transpose":
            return self._apply(x.t().contiguous(), adjoint, True).t().contiguous()
        y = torch.empty(x.shape, dtype=torch.float64, device=x.device)
        if x.dim() == 1:
            B, xs, ys = 1, (x.stride(0), 0), (1, 0)
        elif node_layout:
            B, xs, ys = x.shape[1], x.stride(), y.stride()
        else:
            B, xs, ys = x.shape[0], x.stride()[::-1], y.stride()[::-1]
        _hip.lib().diffhe_filter_apply(self._cent, self._vol, self.mesh.dim, m, self._row_ptr, self._nbr, self._inv_S,
                                       self.radius, int(self.weight == "constant"), int(adjoint), x, xs[0], xs[1], y,
                                       ys[0], ys[1], B, _stream(x.device))
        return y

    def _call(self, op, x, layout: str) -> torch.Tensor:
        x = check_field(x, self.mesh.n_elements, layout)
        _FILTERS[id(self)] = self
        return op(x.to(self.device, torch.float64), id(self), layout == "node").to(x.device)

    def forward(self, x: torch.Tensor, layout: str = "sample") -> torch.Tensor:
        """The filtered field, in the shape and layout of x: (m,), (B, m), or (m, B) with layout="node".  fp64 tensors on
        the filter's device are taken as they are, whatever their strides; anything else is converted first."""
        return self._call(torch.ops.diffhe.density_filter, x, layout)

    def adjoint(self, g: torch.Tensor, layout: str = "sample") -> torch.Tensor:
        """H^T g, in the shape and layout of g."""
        return self._call(torch.ops.diffhe.density_filter_adjoint, g, layout)


# what a sample-major (B, m) field takes: see `DensityFilter._apply` and DESIGN.md section 7, "Density filter"
_SAMPLE_MAJOR = "transpose"


# ---------------------------------------------------------------------------------------------
# torch.library custom ops diffhe::density_filter / diffhe::density_filter_adjoint: the filter travels as an integer
# handle; each op's autograd is the other op (the operator is linear), so derivatives of any order need no more code.
# ---------------------------------------------------------------------------------------------
def _filter_of(handle: int) -> DensityFilter:
    filt = _FILTERS.get(handle)
    if filt is None:
        raise RuntimeError("diffhe: the DensityFilter of this call is gone")
    return filt


@torch.library.custom_op("diffhe::density_filter", mutates_args=())
def density_filter(x: torch.Tensor, handle: int, node_layout: bool) -> torch.Tensor:
    """H x of the `DensityFilter` registered under `handle`."""
    return _filter_of(handle)._apply(x, False, node_layout)


@torch.library.custom_op("diffhe::density_filter_adjoint", mutates_args=())
def density_filter_adjoint(g: torch.Tensor, handle: int, node_layout: bool) -> torch.Tensor:
    """H^T g of the `DensityFilter` registered under `handle`."""
    return _filter_of(handle)._apply(g, True, node_layout)


@density_filter.register_fake
@density_filter_adjoint.register_fake
def _density_filter_fake(x, handle, node_layout):
    return x.new_empty(x.shape, dtype=torch.float64)


def _setup_context(ctx, inputs, output):
    _x, ctx.handle, ctx.node_layout = inputs
    ctx.filt = _FILTERS.get(ctx.handle)             # keeps the filter alive as long as the graph


def _forward_backward(ctx, grad):
    return torch.ops.diffhe.density_filter_adjoint(grad, ctx.handle, ctx.node_layout), None, None


def _adjoint_backward(ctx, grad):
    return torch.ops.diffhe.density_filter(grad, ctx.handle, ctx.node_layout), None, None


torch.library.register_autograd("diffhe::density_filter", _forward_backward, setup_context=_setup_context)
torch.library.register_autograd("diffhe::density_filter_adjoint", _adjoint_backward, setup_context=_setup_context)
