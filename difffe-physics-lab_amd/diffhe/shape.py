"""Solves differentiable with respect to the mesh node coordinates (ours: shape / mesh optimisation).

`ShapeDifferentiableFESolver` is `DifferentiableFESolver3D` (1D, 2D and 3D P1 meshes; same constructor, options, kappa
layouts and `layout=`) that also returns dL/dX when `mesh.nodes.requires_grad` is set -- a leaf, or a tensor computed
from parameters (a mesh deformation driven by a network, say).  Then `forward` runs the custom op `diffhe::fe_solve_shape`,
which takes the nodes as an input; its backward runs ONE adjoint solve for the kappa / f / load / node gradients together
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

from typing import Tuple

import torch

from . import _hip
from . import solver as _solver
from .plan import _stream
from .solver import _SOLVERS, _STATES, _TOKENS, _kappa_strided, _save_for_adjoint, _state_of
from .tet3d import DifferentiableFESolver3D

__all__ = ("ShapeDifferentiableFESolver",)


def _check_nodes(mesh, nodes: torch.Tensor, version: int) -> None:
    """The nodes handed to the op must be the mesh's own tensor at the version `forward` saw: the solve plan is built
    from (and keyed on) exactly that tensor."""
    ref = mesh.nodes
    same = nodes is ref or (nodes.device == ref.device and nodes.data_ptr() == ref.data_ptr()
                            and tuple(nodes.shape) == tuple(ref.shape) and nodes.stride() == ref.stride())
    if not same:
        raise ValueError("diffhe: the nodes given to fe_solve_shape are not mesh.nodes of the solver")
    if nodes._version != version or ref._version != version:
        raise ValueError(f"diffhe: mesh.nodes was modified in place (version {nodes._version}, expected {version}); "
                         "the solve plan would not match the coordinates")


def _shape_inputs(state, kappa: torch.Tensor, f: torch.Tensor, node_major: bool) -> None:
    """Kappa and f as the node-gradient kernel reads them (device views of the op's inputs, strides instead of copies)."""
    call, plan = state.call, state.plan
    state.shape_kappa = _kappa_strided(kappa, call.mode, call.kappa_em, call.B, plan.m, plan.device)
    fd = f.detach().to(plan.device, torch.float64)
    if fd.dim() == 1:
        state.shape_f = (fd.contiguous(), 1, 0)                      # one forcing for the batch
    else:
        fv = fd.t() if node_major else fd                            # (B, n) view
        state.shape_f = (fv, fv.stride(1), fv.stride(0))


def _node_grad(state, lam: torch.Tensor) -> torch.Tensor:
    """(n, dim) fp64 dL/dX from the saved solve and its adjoint `lam` (as `_solve_backward` returns it)."""
    plan = state.plan
    L = _hip.lib()
    n, m, dim, B = plan.n, plan.m, plan.dim, state.call.B
    inc_ptr, inc = plan.shape_incidence()
    u, lam, sn, sb, g = state.shape_fields(lam)
    kdev, kse, ksb = state.shape_kappa
    fdev, fsn, fsb = state.shape_f
    work = torch.empty((m, (dim + 1) * dim), dtype=torch.float64, device=plan.device)
    grad = torch.empty((n, dim), dtype=torch.float64, device=plan.device)
    _hip.check(L.diffhe_p1_shape_grad(_hip.ptr(plan.coords), _hip.ptr(plan.elems), dim, n, m, B, _hip.ptr(u),
                                      _hip.ptr(g), _hip.ptr(lam), sn, sb, _hip.ptr(kdev), kse, ksb, _hip.ptr(fdev),
                                      fsn, fsb, float(state.call.reaction), _hip.ptr(inc_ptr), _hip.ptr(inc),
                                      _hip.ptr(work), _hip.ptr(grad), _stream(plan.device)), "diffhe_p1_shape_grad")
    return grad


@torch.library.custom_op("diffhe::fe_solve_shape", mutates_args=())
def fe_solve_shape(kappa: torch.Tensor, f: torch.Tensor, load: torch.Tensor, nodes: torch.Tensor, nodes_version: int,
                   handle: int, save: bool, node_major: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """`diffhe::fe_solve` with the node coordinates as an input: (u, token).  `nodes` must be the solver's mesh.nodes at
    version `nodes_version` (the tensor the plan is built from)."""
    solver = _SOLVERS[handle]
    _check_nodes(solver.mesh, nodes, nodes_version)
    u, state = _solver._solve_forward(solver, kappa, f, load, node_major)
    token = next(_TOKENS) if save else 0
    if save:
        _shape_inputs(state, kappa, f, node_major)
        _STATES[token] = state
    return u, torch.tensor(token, dtype=torch.int64)


@fe_solve_shape.register_fake
def _fe_solve_shape_fake(kappa, f, load, nodes, nodes_version, handle, save, node_major=False):
    return _solver._fe_solve_fake(kappa, f, load, handle, save, node_major)


@torch.library.custom_op("diffhe::fe_solve_shape_backward", mutates_args=())
def fe_solve_shape_backward(gbar: torch.Tensor, token: torch.Tensor, need_k: bool, need_f: bool, need_load: bool,
                            need_x: bool, kappa_like: torch.Tensor, f_like: torch.Tensor, load_like: torch.Tensor,
                            nodes_like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dL/dkappa, dL/df, dL/dload, dL/dX) of the forward call named by `token` from ONE adjoint solve; unused gradients
    come back empty."""
    state = _state_of(token)
    gk, gf, gl, lam = _solver._solve_backward(state, gbar, need_k, need_f, need_load)
    gx = _node_grad(state, lam).to(nodes_like.device, nodes_like.dtype) if need_x else nodes_like.new_empty(0)
    return (gk if gk is not None else kappa_like.new_empty(0), gf if gf is not None else f_like.new_empty(0),
            gl.to(load_like.dtype) if gl is not None else load_like.new_empty(0), gx)


@fe_solve_shape_backward.register_fake
def _fe_solve_shape_backward_fake(gbar, token, need_k, need_f, need_load, need_x, kappa_like, f_like, load_like,
                                  nodes_like):
    return (torch.empty_like(kappa_like) if need_k else kappa_like.new_empty(0),
            torch.empty_like(f_like) if need_f else f_like.new_empty(0),
            torch.empty_like(load_like) if need_load else load_like.new_empty(0),
            torch.empty_like(nodes_like) if need_x else nodes_like.new_empty(0))


def _shape_setup_context(ctx, inputs, output):
    kappa, f, load, nodes, _version, handle, _save, node_major = inputs
    _save_for_adjoint(ctx, (kappa, f, load, nodes), output, handle, node_major)


def _shape_backward(ctx, grad_u, _grad_token):
    if torch.is_grad_enabled():
        raise NotImplementedError("diffhe: second-order derivatives through the node coordinates are not implemented "
                                  "(backward with create_graph=True while mesh.nodes requires grad)")
    token, kappa, f, load, nodes = ctx.saved_tensors[:5]
    need_k, need_f, need_load, need_x = ctx.needs_input_grad[:4]
    gk, gf, gl, gx = torch.ops.diffhe.fe_solve_shape_backward(grad_u, token, need_k, need_f, need_load, need_x, kappa,
                                                              f, load, nodes)
    return ((gk if need_k else None), (gf if need_f else None), (gl if need_load else None), (gx if need_x else None),
            None, None, None, None)


torch.library.register_autograd("diffhe::fe_solve_shape", _shape_backward, setup_context=_shape_setup_context)


class ShapeDifferentiableFESolver(DifferentiableFESolver3D):
    """`DifferentiableFESolver3D` that also differentiates with respect to `mesh.nodes` (see the module docstring)."""

    _dims = (1, 2, 3)

    def _solve_bc_op(self, f64: torch.Tensor, load64: torch.Tensor, g64: torch.Tensor, node_major: bool) -> torch.Tensor:
        if self.mesh.nodes.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("diffhe: dirichlet= together with node gradients is not implemented "
                                      "(mesh.nodes requires grad)")
        return super()._solve_bc_op(f64, load64, g64, node_major)

    def _solve_op(self, f64: torch.Tensor, load64: torch.Tensor, node_major: bool) -> torch.Tensor:
        nodes = self.mesh.nodes
        if not (nodes.requires_grad and torch.is_grad_enabled()):
            return super()._solve_op(f64, load64, node_major)
        if self.mesh.elements.shape[1] != self.mesh.dim + 1:
            raise NotImplementedError("diffhe: node gradients are implemented for P1 elements only "
                                      "(this mesh has P2 elements and mesh.nodes requires grad)")
        _SOLVERS[id(self)] = self
        u, _token = torch.ops.diffhe.fe_solve_shape(self._kappa, f64, load64, nodes, nodes._version, id(self), True,
                                                    node_major)
        return u
