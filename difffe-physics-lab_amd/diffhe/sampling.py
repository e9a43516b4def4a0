"""The observation side of the solvers: nodal P1 fields sampled at arbitrary points of any P1 mesh -- lines, triangles,
tetrahedra, structured or not -- with the piecewise-constant spatial gradient at those points and the exact transposes of
both.  Ours: the reference compares fields at mesh nodes only (kernels declared in include/diffhe_sample.h).

`PointSampler(mesh, points)` locates every point once, on the device.  The elements are binned by centroid into a uniform
grid whose edge is at least the longest element edge of the mesh (`cellgrid.cell_grid`, the grid of the density filter), so
the element that contains a point has its centroid within one cell edge of it and the 3^dim cells around the point's cell
hold every candidate.  Among the candidates the kernel takes the element whose smallest barycentric coordinate is largest,
ties to the lowest element id; the point is inside if that coordinate is >= -tol.  The rule is a function of the mesh, the
points and tol alone, bit for bit.  The weights are the barycentric coordinates as computed, not clamped.

The search costs O(candidates) per point.  On a strongly graded mesh the cell edge is set by the LARGEST element, so a
point among small elements tests many of them: `info["candidates_max"]` reports the most any point tested.

With S the (P, n) matrix of the weights and G_r, r < dim, the matrices of d phi_k / d x_r of the located elements

    sampler(u) = S u,   sampler.gradient(u)[..., r] = G_r u,   sampler.adjoint(g) = S^T g,
    sampler.gradient_adjoint(g) = sum_r G_r^T g[..., r].

The transposes are gathers over a node -> (point, vertex slot) incidence list in CSR form, built here with a stable torch
sort: no atomics, every sum in ascending order of the points, bitwise reproducible.  `diffhe::point_sample` and
`diffhe::point_sample_adjoint` are each other's autograd (the operators are linear), so gradients of any order flow
through them.  Gradients with respect to the point coordinates or the mesh nodes are not implemented and refused.
"""
from __future__ import annotations

import math
import time
import weakref

import torch
import torch.nn as nn

from . import _hip
from .cellgrid import cell_grid, cell_index
from .plan import _stream

# the transposes visit the touched nodes alone once these are at most n / SPARSE_ROWS ("Point sampling")
SPARSE_ROWS = 4
_SAMPLERS: "weakref.WeakValueDictionary[int, PointSampler]" = weakref.WeakValueDictionary()


def _axes(has_r: bool, node_layout: bool, vector: bool, batched: bool) -> list:
    """The axes of a field: N (nodes or points), c (components, vector fields), r (the gradient's direction), b (samples)."""
    core = ["N"] + (["c"] if vector else [])
    if node_layout:
        return core + (["r"] if has_r else []) + ["b"]
    return (["b"] if batched else []) + core + (["r"] if has_r else [])


def field_axes(shape, count: int, dim: int, has_r: bool, node_layout: bool, vector: bool, what: str) -> list:
    """The axes of a field of that shape on `count` nodes or points, after the refusals (`what` names the counts)."""
    shape = tuple(shape)
    batched = not node_layout and len(shape) == len(_axes(has_r, False, vector, True))
    axes = _axes(has_r, node_layout, vector, batched)
    want = {"N": count, "c": dim, "r": dim}
    if len(shape) != len(axes) or any(shape[i] != want[a] if a != "b" else shape[i] < 1 for i, a in enumerate(axes)):
        names = {"N": what.split("=")[0], "c": f"d={dim}", "r": f"dim={dim}", "b": "B"}
        forms = [_axes(has_r, node_layout, vector, False)] + ([] if node_layout else [_axes(has_r, False, vector, True)])
        text = " or ".join("(" + ", ".join(names[a] for a in f) + ("," if len(f) == 1 else "") + ")" for f in forms)
        raise ValueError(f"the field must be {text} with {what}" + (", layout='node'" if node_layout else "") +
                         (", vector=True" if vector else "") + f", got {shape}")
    return axes


class PointSampler(nn.Module):
    """u -> u(x_p) at P fixed points of a P1 mesh, differentiable in u to any order (see the module docstring).

    Parameters
    ----------
    mesh : FEMesh -- P1 lines, triangles or tetrahedra, any node positions.
    points : (P, dim), or (P,) in 1D; finite, P >= 1.  Converted to fp64 on the device.
    outside : "raise" (default) -- a point in no element is a ValueError -- or "zero": such a point keeps element -1 and
        all-zero weights, its values and gradients are exactly 0.
    tol : a point is inside if the smallest barycentric coordinate of its element is >= -tol (dimensionless).
    device : the GPU of the tables; fields are moved there.

    `element` (P,) int32, `weights` (P, dim + 1) fp64 in the vertex order of mesh.elements, `inside` (P,) bool; `info`:
    points, outside, cells, candidates_max, touched_nodes, table_bytes, build_seconds.

    Fields: scalar (n,), (B, n), or (n, B) with layout="node"; with vector=True (n, d), (B, n, d) or (n, d, B), d = dim.
    `forward` replaces n by P.  `gradient` also appends an axis of length dim (sample layout: (B, P, dim), (B, P, d, dim))
    or places it before the batch axis (node layout: (P, dim, B), (P, d, dim, B)).  `adjoint` and `gradient_adjoint` map
    the other way.  fp64 tensors on the sampler's device are read in place through their strides.
    """

    def __init__(self, mesh, points, *, outside: str = "raise", tol: float = 1e-9, device="cuda"):
        super().__init__()
        if mesh.dim not in (1, 2, 3):
            raise NotImplementedError(f"diffhe: point sampling is implemented for 1D, 2D and 3D meshes, got dim {mesh.dim}")
        if mesh.elements.shape[1] != mesh.dim + 1:
            raise NotImplementedError("diffhe: point sampling is implemented for P1 elements only (this mesh has "
                                      f"{mesh.elements.shape[1]} nodes per element)")
        if mesh.nodes.requires_grad:
            raise NotImplementedError("diffhe: node gradients are not implemented for point sampling (mesh.nodes "
                                      "requires grad): the points are located once in fixed geometry")
        points = points if isinstance(points, torch.Tensor) else torch.as_tensor(points, dtype=torch.float64)
        if points.requires_grad:
            raise NotImplementedError("diffhe: gradients with respect to the point coordinates are not implemented "
                                      "(points requires grad): the points are located once")
        if outside not in ("raise", "zero"):
            raise ValueError(f"Unknown outside: {outside!r} (\"raise\" or \"zero\")")
        tol = float(tol)
        if not (math.isfinite(tol) and tol >= 0.0):
            raise ValueError(f"tol must be non-negative and finite, got {tol!r}")
        if mesh.n_elements < 1:
            raise ValueError("the mesh has no elements")
        dim = mesh.dim
        if points.dim() == 1 and dim == 1:
            points = points[:, None]
        if points.dim() != 2 or points.shape[1] != dim or points.shape[0] < 1:
            raise ValueError(f"points must be (P, dim) with dim={dim} and P >= 1" + (" or (P,)" if dim == 1 else "") +
                             f", got {tuple(points.shape)}")
        if not bool(torch.isfinite(points).all()):
            raise ValueError("points must be finite")
        self.mesh, self.outside, self.tol = mesh, outside, tol
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"point sampling runs on a GPU (there is no CPU fallback), got device {device!r}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._build(points)

    # -- the tables -------------------------------------------------------------------------------------
    def _build(self, points: torch.Tensor) -> None:
        dev, mesh = self.device, self.mesh
        t0 = time.perf_counter()
        dim, n, m = mesh.dim, mesh.n_nodes, mesh.n_elements
        X = mesh.nodes.detach().to(dev, torch.float64).contiguous()
        el = mesh.elements.detach().to(dev, torch.int32).contiguous()
        pts = points.detach().to(dev, torch.float64).contiguous()
        P = pts.shape[0]
        V = X[el.to(torch.int64)]                                           # (m, dim + 1, dim)
        longest = max(float((V[:, i] - V[:, j]).norm(dim=1).max()) for i in range(dim + 1) for j in range(i))
        lo, edge, nc, _, order, cell_start = cell_grid(V.sum(1) / float(dim + 1), longest)
        pcell = cell_index(pts, lo, edge, nc, clamp_low=True)               # a point outside: the nearest cell
        porder = torch.sort(pcell, stable=True)[1].to(torch.int32)
        pcell = pcell.to(torch.int32)
        self._X, self._el, self.points = X, el, pts
        self._grid = (order, cell_start, nc[0], nc[1], nc[2], pts, pcell, porder)
        self.element = torch.empty(P, dtype=torch.int32, device=dev)
        self.weights = torch.empty(P, dim + 1, dtype=torch.float64, device=dev)
        self._gtab = torch.empty(P, dim, dim + 1, dtype=torch.float64, device=dev)
        self._tested = torch.empty(P, dtype=torch.int32, device=dev)
        self._locate()
        self.inside = self.element >= 0
        n_out = P - int(self.inside.sum())
        if n_out and self.outside == "raise":
            first = int(torch.nonzero(~self.inside)[0])
            raise ValueError(f"{n_out} of {P} points lie outside the mesh (tol={self.tol!r}), the first is point {first} at "
                             f"{pts[first].tolist()}: pass outside=\"zero\" to keep them with zero weights")
        # the transpose as a gather: node -> entries p (dim + 1) + k of the inside points, ascending within a row
        ids = torch.nonzero(self.inside.repeat_interleave(dim + 1))[:, 0]
        nodes = el[self.element[self.inside].to(torch.int64)].reshape(-1).to(torch.int64)
        nodes_sorted, perm = torch.sort(nodes, stable=True)
        self._entries = ids[perm].to(torch.int32) if ids.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        self._row_ptr = torch.searchsorted(nodes_sorted, torch.arange(n + 1, device=dev)).to(torch.int64)
        rows = torch.nonzero(self._row_ptr[1:] > self._row_ptr[:-1])[:, 0].to(torch.int32)
        touched = rows.numel()
        # few touched nodes: the transposes zero their result and visit those rows alone (the same bits)
        self._rows = rows if touched <= n // SPARSE_ROWS else None
        torch.cuda.synchronize(dev)
        self.info = {"points": P, "outside": n_out, "cells": nc[0] * nc[1] * nc[2], "candidates_max": int(self._tested.max()),
                     "touched_nodes": touched,
                     "table_bytes": 4 * P + 8 * P * (dim + 1) ** 2 + 8 * (n + 1) + 4 * ids.numel(),
                     "build_seconds": time.perf_counter() - t0}

    def _locate(self) -> None:
        """The locate kernel on the stored grid: fills element, weights, the gradient table and the candidate counts."""
        mesh = self.mesh
        _hip.lib().diffhe_sample_locate(self._X, self._el, mesh.dim, mesh.n_nodes, mesh.n_elements, *self._grid,
                                        self.points.shape[0], self.tol, self.element, self.weights, self._gtab,
                                        self._tested, _stream(self.device))

    @property
    def row_ptr(self) -> torch.Tensor:
        """(n + 1,) int64: row i of `entries` is [row_ptr[i], row_ptr[i + 1])."""
        return self._row_ptr

    @property
    def entries(self) -> torch.Tensor:
        """int32 p (dim + 1) + k of every (inside point p, vertex slot k) at node i, row after row, ascending in a row."""
        return self._entries

    @property
    def gradient_table(self) -> torch.Tensor:
        """(P, dim, dim + 1): d phi_k / d x_r of the element of point p at [p, r, k]."""
        return self._gtab

    # -- the operators ----------------------------------------------------------------------------------
    def _apply(self, x: torch.Tensor, adjoint: bool, gradient: bool, node_layout: bool, vector: bool) -> torch.Tensor:
        """S x or G x (adjoint: the transposes) of a checked fp64 field on the sampler's device, in one of two routes with
        the same bits.  The kernels run with lanes over samples.  Sample-minor fields, flat fields and sparse calls -- a
        forward with fewer vertex reads than nodes, a transpose that visits the touched nodes alone -- are read and written
        in place through their strides.  Any other (B, ...) field takes a transposed copy with torch on the way in and on
        the way out, around a coalesced sample-minor call ("Point sampling")."""
        dim, n, P = self.mesh.dim, self.mesh.n_nodes, self.points.shape[0]
        src, dst = (P, n) if adjoint else (n, P)
        axes = field_axes(x.shape, src, dim, gradient and adjoint, node_layout, vector, "")
        B, C, R = (x.shape[axes.index("b")] if "b" in axes else 1), (dim if vector else 1), (dim if gradient else 1)
        rows = self._rows if adjoint else None
        sparse = rows is not None if adjoint else P * (dim + 1) < n
        out_axes = _axes(gradient and not adjoint, node_layout, vector, "b" in axes)
        around = axes[0] == "b" and B > 1 and not sparse
        if around:
            x, axes, out_axes = x.movedim(0, -1).contiguous(), axes[1:] + ["b"], out_axes[1:] + ["b"]
        xs = {a: x.stride(i) for i, a in enumerate(axes)}
        sizes = {"N": dst, "c": C, "r": R, "b": B}
        y = (torch.empty if rows is None else torch.zeros)([sizes[a] for a in out_axes], dtype=torch.float64, device=x.device)
        ys = {a: y.stride(i) for i, a in enumerate(out_axes)}
        W = self._gtab if gradient else self.weights
        st = _stream(x.device)
        if adjoint and (rows is None or rows.numel()):
            _hip.lib().diffhe_sample_adjoint(self._row_ptr, self._entries, rows, 0 if rows is None else rows.numel(), dim, n,
                                             W, R, P, x, xs["N"], xs.get("r", 0), xs.get("c", 0), xs.get("b", 0), y,
                                             ys["N"], ys.get("c", 0), ys.get("b", 0), C, B, st)
        elif not adjoint:
            _hip.lib().diffhe_sample_apply(self._el, dim, n, self.element, W, R, P, x, xs["N"], xs.get("c", 0),
                                           xs.get("b", 0), y, ys["N"], ys.get("r", 0), ys.get("c", 0), ys.get("b", 0), C, B,
                                           st)
        return y.movedim(-1, 0).contiguous() if around else y

    def _call(self, op, x, adjoint: bool, gradient: bool, layout: str, vector: bool) -> torch.Tensor:
        if layout not in ("sample", "node"):
            raise ValueError(f"Unknown layout: {layout!r}")
        x = x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=torch.float64)
        n, P = self.mesh.n_nodes, self.points.shape[0]
        field_axes(x.shape, P if adjoint else n, self.mesh.dim, gradient and adjoint, layout == "node", bool(vector),
                   f"P={P} (n={n})" if adjoint else f"n={n}")
        _SAMPLERS[id(self)] = self
        return op(x.to(self.device, torch.float64), id(self), gradient, layout == "node", bool(vector)).to(x.device)

    def forward(self, u: torch.Tensor, layout: str = "sample", vector: bool = False) -> torch.Tensor:
        """The field at the points: (n,) -> (P,), (B, n) -> (B, P), layout="node": (n, B) -> (P, B); vector=True:
        (n, d) -> (P, d), (B, n, d) -> (B, P, d), (n, d, B) -> (P, d, B)."""
        return self._call(torch.ops.diffhe.point_sample, u, False, False, layout, vector)

    def gradient(self, u: torch.Tensor, layout: str = "sample", vector: bool = False) -> torch.Tensor:
        """The spatial gradient of the field at the points, constant on each element: the shapes of `forward` with an axis
        of length dim appended (sample layout) or placed before the batch axis (node layout)."""
        return self._call(torch.ops.diffhe.point_sample, u, False, True, layout, vector)

    def adjoint(self, g: torch.Tensor, layout: str = "sample", vector: bool = False) -> torch.Tensor:
        """S^T g: point data in a shape `forward` returns -> the nodal field of that layout; exact zeros at nodes that no
        point touches."""
        return self._call(torch.ops.diffhe.point_sample_adjoint, g, True, False, layout, vector)

    def gradient_adjoint(self, g: torch.Tensor, layout: str = "sample", vector: bool = False) -> torch.Tensor:
        """sum_r G_r^T g[..., r]: point data in a shape `gradient` returns -> the nodal field of that layout."""
        return self._call(torch.ops.diffhe.point_sample_adjoint, g, True, True, layout, vector)


# ---------------------------------------------------------------------------------------------
# torch.library custom ops diffhe::point_sample / diffhe::point_sample_adjoint: the sampler travels as an integer handle;
# each op's autograd is the other op (the operators are linear), so derivatives of any order need no more code.
# ---------------------------------------------------------------------------------------------
def _sampler_of(handle: int) -> PointSampler:
    sampler = _SAMPLERS.get(handle)
    if sampler is None:
        raise RuntimeError("diffhe: the PointSampler of this call is gone")
    return sampler


@torch.library.custom_op("diffhe::point_sample", mutates_args=())
def point_sample(u: torch.Tensor, handle: int, gradient: bool, node_layout: bool, vector: bool) -> torch.Tensor:
    """S u (gradient: G u) of the `PointSampler` registered under `handle`."""
    return _sampler_of(handle)._apply(u, False, gradient, node_layout, vector)


@torch.library.custom_op("diffhe::point_sample_adjoint", mutates_args=())
def point_sample_adjoint(g: torch.Tensor, handle: int, gradient: bool, node_layout: bool, vector: bool) -> torch.Tensor:
    """S^T g (gradient: G^T g) of the `PointSampler` registered under `handle`."""
    return _sampler_of(handle)._apply(g, True, gradient, node_layout, vector)


def _fake(x, handle, gradient, node_layout, vector, adjoint):
    s = _sampler_of(handle)
    dim, n, P = s.mesh.dim, s.mesh.n_nodes, s.points.shape[0]
    axes = field_axes(x.shape, P if adjoint else n, dim, gradient and adjoint, node_layout, vector, "")
    out = _axes(gradient and not adjoint, node_layout, vector, "b" in axes)
    sizes = {"N": n if adjoint else P, "c": dim, "r": dim, "b": x.shape[axes.index("b")] if "b" in axes else 1}
    return x.new_empty([sizes[a] for a in out], dtype=torch.float64)


@point_sample.register_fake
def _point_sample_fake(u, handle, gradient, node_layout, vector):
    return _fake(u, handle, gradient, node_layout, vector, False)


@point_sample_adjoint.register_fake
def _point_sample_adjoint_fake(g, handle, gradient, node_layout, vector):
    return _fake(g, handle, gradient, node_layout, vector, True)


def _setup_context(ctx, inputs, output):
    _x, ctx.handle, ctx.gradient, ctx.node_layout, ctx.vector = inputs
    ctx.sampler = _SAMPLERS.get(ctx.handle)         # keeps the sampler alive as long as the graph


def _forward_backward(ctx, grad):
    return (torch.ops.diffhe.point_sample_adjoint(grad, ctx.handle, ctx.gradient, ctx.node_layout, ctx.vector),
            None, None, None, None)


def _adjoint_backward(ctx, grad):
    return (torch.ops.diffhe.point_sample(grad, ctx.handle, ctx.gradient, ctx.node_layout, ctx.vector),
            None, None, None, None)


torch.library.register_autograd("diffhe::point_sample", _forward_backward, setup_context=_setup_context)
torch.library.register_autograd("diffhe::point_sample_adjoint", _adjoint_backward, setup_context=_setup_context)
