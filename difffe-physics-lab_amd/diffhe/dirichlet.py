"""Solves differentiable with respect to per-sample Dirichlet values (ours: the reference reads one dict of boundary
values per mesh and carries no gradient to it, although its README promises optimisation of boundary conditions).

`DifferentiableFESolver.forward(f, load=None, layout="sample", dirichlet=G)` -- inherited by `DifferentiableFESolver3D`
and `ShapeDifferentiableFESolver` -- takes the Dirichlet values G in ascending node-id order (`FEMesh.dirichlet_index()`),
(n_D,) for the batch or (B, n_D) per sample ((n_D,) or (n_D, B) with layout="node").  The keys of `mesh.dirichlet_nodes`
still say which nodes are Dirichlet nodes, its values are not used: the solve plan (which depends only on the nodes, the
elements and that SET) is the same for every G.  The call runs the custom op `diffhe::fe_solve_bc`.  With F the free and
D the Dirichlet nodes and K_b the unreduced stiffness of sample b:

    A_b x_b = M f_b + load_b - K_b[F, D] G_b,    u_b[F] = x_b,   u_b[D] = G_b
    dL/dG_b[j] = gbar_b[j] - (K_b lambda_b)_j    (j in D; lambda_b the adjoint the kappa / f / load gradients use)

so a backward with G among the inputs still costs ONE adjoint solve.  The reaction term's lumped mass is diagonal and
does not couple.  dL/dkappa is -lambda^T k0_e u_e with G in u.

The path classes of diffhe.solver solve with HOMOGENEOUS Dirichlet data (the zeros of `SolvePlan.zero_g`, no second
plan, no new mesh); the kernels of csrc/bc.hip add what G changes, on the boundary band only (O(n^((d-1)/d) B)): the lift
of the right-hand side (an extra load on the 1D chain), the Dirichlet rows of the returned u (never of the private
iterate, which is also the warm start and the adjoint's saved x), dL/dG with the unit-kappa products of the factored
kappa gradient, and the G part of the per-element kappa gradient.

Not covered (NotImplementedError): second order through G (a backward with create_graph=True while G requires grad) and
G together with node gradients (mesh.nodes requiring grad in ShapeDifferentiableFESolver).  `dirichlet=None` runs
diffhe::fe_solve exactly as before.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import solver as _solver
from .solver import K_ELEM, K_SAMPLE, K_SAMPLE_ELEM, K_SCALAR, _SOLVERS, _STATES, _TOKENS, _kappa_grad, _save_for_adjoint, \
    _state_of

__all__ = ("fe_solve_bc",)


def _solve_backward_bc(state, gbar, need_k: bool, need_f: bool, need_load: bool, need_g: bool):
    """`diffhe.solver._solve_backward` for a solve with per-call Dirichlet data: the path's adjoint, then the band
    kernels -- dL/dG, and the G part of dL/dkappa on the node-major paths (the chain's u already holds G) -- then the
    gradients shaped like the inputs.  Returns (grad_kappa, grad_f, grad_load, per-sample dL/dG) or None for each."""
    call, plan, eng = state.call, state.plan, state.eng
    B, n = call.B, plan.n
    g = gbar.detach().to(plan.device, torch.float64)
    g = g.reshape(n, B) if call.node_major else g.reshape(B, n).contiguous()
    lam, dk_sample, dk_elem, df, dload = state.adjoint(g, need_k, need_f, need_load)
    _u, lam_f, lsn, lsb, _g = state.shape_fields(lam)          # lambda (0 on D) and its strides, either layout
    chain = isinstance(state, _solver._ChainSolve)
    scalar_k = need_k and not chain and call.mode in (K_SCALAR, K_SAMPLE)
    gG = None
    if need_g or scalar_k:
        nd = plan.n_bc
        out = torch.empty((nd, B) if call.node_major else (B, nd), dtype=torch.float64, device=plan.device)
        osj, osb = (B, 1) if call.node_major else (1, nd)
        dots = torch.empty((nd, B), dtype=torch.float64, device=plan.device) if scalar_k else None
        eng.bc_grad(state.bc_kappa, lam_f, lsn, lsb, g, g.stride(0 if call.node_major else 1),
                    g.stride(1 if call.node_major else 0), out, osj, osb, call.bc if scalar_k else None, dots, B)
        gG = out if need_g else None
        if scalar_k:        # dL/dkappa_b = -lambda_b^T K_1 u_b: the u_b[D] = G_b part, -sum_j G_b[j] (K_1 lambda_b)_j
            dk_sample = dk_sample - dots.sum(dim=0)
    if need_k and not chain and call.mode in (K_ELEM, K_SAMPLE_ELEM):
        if call.mode == K_ELEM:
            dse, dsb = dk_elem.stride(0), 0
        elif call.kappa_em:
            dse, dsb = dk_elem.stride(0), dk_elem.stride(1)             # (m, B)
        else:
            dse, dsb = dk_elem.stride(1), dk_elem.stride(0)             # (B, m)
        eng.bc_grad_kappa(lam_f, lsn, lsb, call.bc, dk_elem, dse, dsb, call.mode == K_ELEM, B)
    grad_k = grad_f = grad_load = None
    if need_k:
        grad_k = _kappa_grad(call.mode, call.kappa_shape, dk_sample, dk_elem).to(call.kappa_device)
    if need_f:
        grad_f = (df if call.batched else df.sum(dim=0)).to(call.out_device)
    if need_load:
        grad_load = (dload if call.load_batched else dload.sum(dim=1 if call.node_major else 0)).to(call.out_device)
    return grad_k, grad_f, grad_load, gG


@torch.library.custom_op("diffhe::fe_solve_bc", mutates_args=())
def fe_solve_bc(kappa: torch.Tensor, f: torch.Tensor, load: torch.Tensor, g: torch.Tensor, handle: int, save: bool,
                node_major: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """`diffhe::fe_solve` with the Dirichlet values `g` as an input: (n_D,), (B, n_D), or (n_D, B) when node_major."""
    u, state = _solver._solve_forward(_SOLVERS[handle], kappa, f, load, node_major, dirichlet=g)
    token = next(_TOKENS) if save else 0
    if save:
        _STATES[token] = state
    return u, torch.tensor(token, dtype=torch.int64)


@fe_solve_bc.register_fake
def _fe_solve_bc_fake(kappa, f, load, g, handle, save, node_major=False):
    return _solver._fe_solve_fake(kappa, f, load, handle, save, node_major)


@torch.library.custom_op("diffhe::fe_solve_bc_backward", mutates_args=())
def fe_solve_bc_backward(gbar: torch.Tensor, token: torch.Tensor, need_k: bool, need_f: bool, need_load: bool,
                         need_g: bool, kappa_like: torch.Tensor, f_like: torch.Tensor, load_like: torch.Tensor,
                         g_like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dL/dkappa, dL/df, dL/dload, dL/dG) of the forward call named by `token` from ONE adjoint solve; unused gradients
    come back empty.  A (n_D,) G shared by the batch receives the sum over the samples."""
    state = _state_of(token)
    gk, gf, gl, gG = _solve_backward_bc(state, gbar, need_k, need_f, need_load, need_g)
    if need_g:
        if g_like.dim() == 1:
            gG = gG.sum(dim=1 if state.call.node_major else 0)
        gG = gG.to(g_like.device, g_like.dtype)
    return (gk if gk is not None else kappa_like.new_empty(0), gf if gf is not None else f_like.new_empty(0),
            gl.to(load_like.dtype) if gl is not None else load_like.new_empty(0),
            gG if gG is not None else g_like.new_empty(0))


@fe_solve_bc_backward.register_fake
def _fe_solve_bc_backward_fake(gbar, token, need_k, need_f, need_load, need_g, kappa_like, f_like, load_like, g_like):
    return (torch.empty_like(kappa_like) if need_k else kappa_like.new_empty(0),
            torch.empty_like(f_like) if need_f else f_like.new_empty(0),
            torch.empty_like(load_like) if need_load else load_like.new_empty(0),
            torch.empty_like(g_like) if need_g else g_like.new_empty(0))


def _bc_setup_context(ctx, inputs, output):
    kappa, f, load, g, handle, _save, node_major = inputs
    _save_for_adjoint(ctx, (kappa, f, load, g), output, handle, node_major)


def _bc_backward(ctx, grad_u, _grad_token):
    need_k, need_f, need_load, need_g = ctx.needs_input_grad[:4]
    if torch.is_grad_enabled():
        if need_g:
            raise NotImplementedError("diffhe: second-order derivatives through the Dirichlet values are not implemented "
                                      "(backward with create_graph=True while dirichlet= requires grad)")
        # kappa / f / load to second order: the differentiable restatement, with this call's G in u
        gk, gf, gl = _solver._second_order_backward(ctx, grad_u, dirichlet=ctx.saved_tensors[4])[:3]
        return gk, gf, gl, None, None, None, None
    token, kappa, f, load, g = ctx.saved_tensors[:5]
    gk, gf, gl, gG = torch.ops.diffhe.fe_solve_bc_backward(grad_u, token, need_k, need_f, need_load, need_g, kappa, f,
                                                           load, g)
    return ((gk if need_k else None), (gf if need_f else None), (gl if need_load else None), (gG if need_g else None),
            None, None, None)


torch.library.register_autograd("diffhe::fe_solve_bc", _bc_backward, setup_context=_bc_setup_context)
