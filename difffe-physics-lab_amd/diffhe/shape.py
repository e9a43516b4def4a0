"""Solves differentiable with respect to the mesh node coordinates (ours: shape / mesh optimisation).

`ShapeDifferentiableFESolver` is `DifferentiableFESolver3D` (1D, 2D and 3D P1 meshes; same constructor, options, kappa
layouts and `layout=`) that also returns dL/dX when `mesh.nodes.requires_grad` is set -- a leaf, or a tensor computed
from parameters (a mesh deformation driven by a network, say).  Then `forward` hands the nodes to the custom op
`diffhe::fe_solve` as an input; its backward runs ONE adjoint solve for the kappa / f / load / node gradients together
and contracts the adjoint lambda and u once more per element (`diffhe_p1_shape_grad`, csrc/shape.hip):

    dL/dX = -lambda^T (dK/dX) u + lambda^T (dF/dX) - c lambda^T (dM_L/dX) u

with the load map and lumped mass the solve uses (F_p = A_e / (d+1) * mean f in 2D and 3D, the reference's trapezoid
h/2 f_i in 1D).  Any explicit dependence the caller's graph carries (an f computed from X) adds through autograd as usual.
Without nodes requiring grad `forward` is exactly the base class.

Convention: this is the full P1 shape derivative.  In 1D it equals the reference's autograd to `mesh.nodes`, where
h_e = x_j - x_i is not detached.  In 2D it is NOT the reference's partial derivative through `area` alone (the reference
detaches b and c, solver.py:125-134, as `DifferentiableFESolver` keeps doing by reading detached coordinates).

The batch shares one mesh, so dL/dX sums over the samples.  Not covered: P2 meshes (NotImplementedError), second order
through X (a backward with create_graph=True while the nodes need grad raises NotImplementedError), node gradients
through `diffhe.heat.HeatEquation`.  A moved mesh builds a new solve plan, as any change of `mesh.nodes` does.

Layouts handed to the kernel: the 2D / 3D / general paths keep u and lambda node-major (n, Bp); the 1D chain keeps its
sample-major (B, n) arrays and the kernel takes strides (sn, sb) -- no transposing copy on either path.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _hip
from .plan import _stream
from .solver import _SOLVERS
from .tet3d import DifferentiableFESolver3D

__all__ = ("ShapeDifferentiableFESolver",)


def _check_nodes(mesh, nodes: torch.Tensor, version: int) -> None:
    """The nodes handed to the op must be the mesh's own tensor at the version `forward` saw: the solve plan is built
    from (and keyed on) exactly that tensor."""
    ref = mesh.nodes
    same = nodes is ref or (nodes.device == ref.device and nodes.data_ptr() == ref.data_ptr()
                            and tuple(nodes.shape) == tuple(ref.shape) and nodes.stride() == ref.stride())
    if not same:
        raise ValueError("diffhe: the nodes given to diffhe::fe_solve are not mesh.nodes of the solver")
    if nodes._version != version or ref._version != version:
        raise ValueError(f"diffhe: mesh.nodes was modified in place (version {nodes._version}, expected {version}); "
                         "the solve plan would not match the coordinates")


def _node_grad(state, lam: torch.Tensor) -> torch.Tensor:
    """(n, dim) fp64 dL/dX from the saved solve and its adjoint `lam` (in the path's layout, as `state.adjoint` returns it)."""
    plan = state.plan
    L = _hip.lib()
    n, m, dim, B = plan.n, plan.m, plan.dim, state.call.B
    inc_ptr, inc = plan.shape_incidence()
    u, lam, sn, sb, g = state.shape_fields(lam)
    kdev, kse, ksb = state.call.kappa_s
    fdev, fsn, fsb = state.call.f_s
    work = torch.empty((m, (dim + 1) * dim), dtype=torch.float64, device=plan.device)
    grad = torch.empty((n, dim), dtype=torch.float64, device=plan.device)
    L.diffhe_p1_shape_grad(plan.coords, plan.elems, dim, n, m, B, u, g, lam, sn, sb, kdev, kse, ksb, fdev, fsn, fsb,
                           float(state.call.reaction), inc_ptr, inc, work, grad, _stream(plan.device))
    return grad


class ShapeDifferentiableFESolver(DifferentiableFESolver3D):
    """`DifferentiableFESolver3D` that also differentiates with respect to `mesh.nodes` (see the module docstring)."""

    _dims = (1, 2, 3)

    def _solve_op(self, f64: torch.Tensor, load64: torch.Tensor, g64: Optional[torch.Tensor],
                  node_major: bool) -> torch.Tensor:
        nodes = self.mesh.nodes
        if not (nodes.requires_grad and torch.is_grad_enabled()):
            return super()._solve_op(f64, load64, g64, node_major)
        if g64 is not None:
            raise NotImplementedError("diffhe: dirichlet= together with node gradients is not implemented "
                                      "(mesh.nodes requires grad)")
        if self.mesh.elements.shape[1] != self.mesh.dim + 1:
            raise NotImplementedError("diffhe: node gradients are implemented for P1 elements only "
                                      "(this mesh has P2 elements and mesh.nodes requires grad)")
        _SOLVERS[id(self)] = self
        u, _token = torch.ops.diffhe.fe_solve(self._kappa, f64, load64, id(self), True, node_major, None, nodes,
                                              nodes._version)
        return u
