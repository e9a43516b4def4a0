"""Elastic solves and stresses differentiable with respect to the mesh node coordinates (ours: shape design of elastic
bodies -- fillets, tapers, r-adaptivity of a stress concentration).

`ShapeElasticFESolver` is `ElasticFESolver` (same constructor, options, E layouts and `layout=`) that also returns dL/dX
when `mesh.nodes.requires_grad` is set -- a leaf, or a tensor computed from parameters.  Without nodes requiring grad, or
with grad disabled, every method takes exactly the base class's path.

Solve.  `forward` hands the nodes (with their `_version`) to the custom op `diffhe::elastic_solve_shape`; its backward runs
the ONE adjoint solve of `_ElasticSolve.adjoint`, unchanged, for dL/dE, dL/df and dL/dload, and contracts the same adjoint
lambda with u once more per element (`diffhe_elast_shape_grad`, csrc/elastic_shape.hip).  With the exact P1 gradients
g_p = grad phi_p of the plan's oriented table, the element size A_e, H_w[a][t] = sum_p w_(p,a) g_p[t] for the full u
(prescribed values included) and for lambda, and S(H) = 2 mu' sym(H) + lambda' tr(H) I, element e adds to its vertex p

    A_e [ sum_b E_eb ( H_u^T S(H_lam) + H_lam^T S(H_u) - (S(H_u) : H_lam) I ) + q_e I ] g_p,
    q_e = sum_b sum_a (sum_p lam_(p,a)) (sum_p f_(p,a)) / (d+1)^2          (0 without f).

Stress.  `stress`, `von_mises` and `stress_and_von_mises` go through `diffhe::elastic_stress_shape`: for a given u the
stress depends on X through grad phi alone, and with T = dL/dH_u -- the symmetric tensor of the stress adjoint's element
pass -- vertex p gets -(sum_b H_u^T T_b) g_p (`diffhe_stress_shape_grad`).  du and dE come from the base class's adjoint,
unchanged.  The explicit dependence on X and the one through u(X) add up by autograd to the total derivative of, say,
`pnorm(solver.von_mises(solver(f, load)))`.

The batch shares one mesh, so dL/dX sums over the samples, in a fixed order (bitwise reproducible).  Not covered
(NotImplementedError while the nodes need grad): `eigenstrain=` on the solve and on the stress methods and
`eigenstrain_load` -- lambda^T F0 adds A_e E_e [ (S0 : H_lam) I - H_lam^T S0 ] g_p, the named follow-up -- and second order
through X (a backward with create_graph=True).  `ElasticEigenSolver` keeps refusing moving nodes.  A moved mesh builds a
new solve plan, dof system and unit-E hierarchy, as any change of `mesh.nodes` does ("Elastic shape
derivative", has its cost).
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _hip
from .elastic import ElasticFESolver, _ElasticSolve, _run_adjoint, _solve_autograd, _solve_call, _solve_fake, _solve_result
from .elastic_stress import (_stress_adjoint, _stress_autograd, _stress_call, _stress_fake, _stress_forward,
                             _stress_outputs, _stress_shapes)
from .plan import _stream
from .shape import _check_nodes
from .solver import _SOLVERS, _fake_grads, _like_grads

__all__ = ("ShapeElasticFESolver",)


def _solve_node_grad(state) -> torch.Tensor:
    """(n, d) fp64 dL/dX on the plan's device from the saved solve and the adjoint lambda its `adjoint` left."""
    plan, setup, call = state.plan, state.setup, state.call
    n, m, d = plan.n, plan.m, plan.dim
    _, vol = plan.gradient_table()
    work = torch.empty((m, (d + 1) * d), dtype=torch.float64, device=plan.device)
    grad = torch.empty((n, d), dtype=torch.float64, device=plan.device)
    _hip.lib().diffhe_elast_shape_grad(plan.elems, plan.oriented_gradient_table(), vol, d, setup.lam1, setup.mu1, state.x,
                                       setup.dofs.g, state.lam, state.f_dofs, *state.e_s, n, m, call.B, state.Bp,
                                       *plan.shape_incidence(), work, grad, _stream(plan.device))
    return grad


def _stress_node_grad(solver, sigma_bar, vm_bar, u, E, node_major: bool) -> torch.Tensor:
    """(n, d) fp64 dL/dX on the plan's device of a stress evaluation at fixed u for the cotangents of sigma and vm."""
    call = _stress_call(solver, u, E, node_major)
    plan, nc, B, Bp = call.plan, call.nc, call.B, call.Bp
    n, m, d = plan.n, plan.m, plan.dim
    sb = call.rows_in(sigma_bar, m * nc, True) if sigma_bar is not None else None
    vb = call.rows_in(vm_bar, m, True) if vm_bar is not None else None
    work = torch.empty((m, (d + 1) * d), dtype=torch.float64, device=plan.device)
    grad = torch.empty((n, d), dtype=torch.float64, device=plan.device)
    _hip.lib().diffhe_stress_shape_grad(*call.head, sb, Bp, nc * Bp, vb, n, m, B, Bp, *plan.shape_incidence(), work, grad,
                                        _stream(plan.device))
    return grad


class _ShapeElasticSolve(_ElasticSolve):
    """`_ElasticSolve` that also keeps what the node-gradient kernel reads: E (`e_s`) and f (`f_dofs`) as the kernels read
    them, and the adjoint lambda."""
    keep_lambda = True
    e_s = f_dofs = None

    def _operator(self, E):
        *self.e_s, Bv = self.node_eng.kappa_device(E, self.call.mode, self.call.B, self.Bp, em=self.call.kappa_em)
        return (*self.setup.assemble(*self.e_s, Bv), Bv)

    def _body_force(self, f):
        self.f_dofs = super()._body_force(f)
        return self.f_dofs


# ---------------------------------------------------------------------------------------------
# diffhe::elastic_solve_shape / diffhe::elastic_solve_shape_backward: `diffhe::elastic_solve` with the nodes as an input.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("diffhe::elastic_solve_shape", mutates_args=())
def elastic_solve_shape(E: torch.Tensor, f: torch.Tensor, load: torch.Tensor, nodes: torch.Tensor, nodes_version: int,
                        handle: int, node_major: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u, token) of `diffhe::elastic_solve` for the `ShapeElasticFESolver` registered under `handle`, with the node
    coordinates as a differentiable input: the solver's mesh.nodes at version `nodes_version`, the tensor the plan is built
    from.  The adjoint state is always kept."""
    solver = _SOLVERS[handle]
    _check_nodes(solver.mesh, nodes, nodes_version)
    return _solve_result(*_solve_call(solver, _ShapeElasticSolve, E, f, load, node_major), True)


@elastic_solve_shape.register_fake
def _elastic_solve_shape_fake(E, f, load, nodes, nodes_version, handle, node_major):
    return _solve_fake(_SOLVERS[handle], E, f, load, node_major)


_Grads4 = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]


@torch.library.custom_op("diffhe::elastic_solve_shape_backward", mutates_args=())
def elastic_solve_shape_backward(gbar: torch.Tensor, token: torch.Tensor, need_e: bool, need_f: bool, need_load: bool,
                                 need_x: bool, e_like: torch.Tensor, f_like: torch.Tensor, load_like: torch.Tensor,
                                 nodes_like: torch.Tensor) -> _Grads4:
    """(dL/dE, dL/df, dL/dload, dL/dX) of the forward call named by `token` from ONE adjoint solve; unused ones come back
    empty.  The first three are `_ElasticSolve.adjoint`'s, unchanged."""
    state, grads = _run_adjoint(gbar, token, need_e, need_f, need_load)
    gx = _solve_node_grad(state) if need_x else None
    state.lam = None
    return _like_grads(gbar, (*grads, gx), (e_like, f_like, load_like, nodes_like))


@elastic_solve_shape_backward.register_fake
def _elastic_solve_shape_backward_fake(gbar, token, need_e, need_f, need_load, need_x, e_like, f_like, load_like,
                                       nodes_like):
    return _fake_grads(gbar, (need_e, need_f, need_load, need_x), (e_like, f_like, load_like, nodes_like))


_solve_setup_context, _solve_backward = _solve_autograd(
    "elastic_solve_shape", 4, 7, "diffhe: second-order derivatives of an elastic solve are not implemented (backward with "
    "create_graph=True while mesh.nodes requires grad, diffhe.elastic_shape)")


# ---------------------------------------------------------------------------------------------
# diffhe::elastic_stress_shape / diffhe::elastic_stress_shape_backward: `diffhe::elastic_stress` with the nodes as an input.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("diffhe::elastic_stress_shape", mutates_args=())
def elastic_stress_shape(u: torch.Tensor, E: torch.Tensor, nodes: torch.Tensor, nodes_version: int, handle: int,
                         node_major: bool, want_sigma: bool, want_vm: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sigma, vm) of `diffhe::elastic_stress` with the node coordinates as a differentiable input (the solver's mesh.nodes
    at version `nodes_version`); the output not asked for comes back empty."""
    solver = _SOLVERS[handle]
    _check_nodes(solver.mesh, nodes, nodes_version)
    return _stress_outputs(u, *_stress_forward(solver, u, E, node_major, want_sigma, want_vm))


@elastic_stress_shape.register_fake
def _elastic_stress_shape_fake(u, E, nodes, nodes_version, handle, node_major, want_sigma, want_vm):
    return _stress_fake(u, _stress_shapes(_SOLVERS[handle], u, E, node_major), want_sigma, want_vm)


@torch.library.custom_op("diffhe::elastic_stress_shape_backward", mutates_args=())
def elastic_stress_shape_backward(sigma_bar: torch.Tensor, vm_bar: torch.Tensor, u: torch.Tensor, E: torch.Tensor,
                                  nodes: torch.Tensor, handle: int, node_major: bool, need_u: bool, need_e: bool,
                                  need_x: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dL/du, dL/dE, dL/dX) of `elastic_stress_shape` for the cotangents of sigma and vm (empty = absent); unused ones come
    back empty.  The first two are `diffhe::elastic_stress_backward`'s, unchanged."""
    solver = _SOLVERS[handle]
    sb, vb = (sigma_bar if sigma_bar.numel() else None), (vm_bar if vm_bar.numel() else None)
    du = de = gx = None
    if need_u or need_e:
        du, de = _stress_adjoint(solver, sb, vb, u, E, node_major, need_u, need_e)
    if need_x:
        gx = _stress_node_grad(solver, sb, vb, u, E, node_major)
    return _like_grads(u, (du, de, gx), (u, E, nodes))


@elastic_stress_shape_backward.register_fake
def _elastic_stress_shape_backward_fake(sigma_bar, vm_bar, u, E, nodes, handle, node_major, need_u, need_e, need_x):
    return _fake_grads(u, (need_u, need_e, need_x), (u, E, nodes))


_stress_setup_context, _stress_backward = _stress_autograd(
    "elastic_stress_shape", 3, 8, "diffhe: second-order derivatives of an elastic stress evaluation are not implemented "
    "(backward with create_graph=True while mesh.nodes requires grad, diffhe.elastic_shape)")


class ShapeElasticFESolver(ElasticFESolver):
    """`ElasticFESolver` that also differentiates the solve and the stress methods with respect to `mesh.nodes` (see the
    module docstring)."""

    def _refuse_moving_nodes(self, what: str, eigenstrain: bool) -> None:
        if eigenstrain and self._moving_nodes():
            raise NotImplementedError(f"diffhe: an eigenstrain together with node gradients is not implemented ({what} "
                                      "while mesh.nodes requires grad, diffhe.elastic_shape)")

    def _solve_op(self, E: torch.Tensor, f_in: torch.Tensor, load_in: torch.Tensor, node_major: bool) -> torch.Tensor:
        if not self._moving_nodes():
            return super()._solve_op(E, f_in, load_in, node_major)
        nodes = self.mesh.nodes
        u, _token = torch.ops.diffhe.elastic_solve_shape(E, f_in, load_in, nodes, nodes._version, id(self), node_major)
        return u

    def _stress_eval_op(self, u: torch.Tensor, E: torch.Tensor, node_major: bool, want_sigma: bool, want_vm: bool):
        if not self._moving_nodes():
            return super()._stress_eval_op(u, E, node_major, want_sigma, want_vm)
        nodes = self.mesh.nodes
        return torch.ops.diffhe.elastic_stress_shape(u, E, nodes, nodes._version, id(self), node_major, want_sigma, want_vm)
