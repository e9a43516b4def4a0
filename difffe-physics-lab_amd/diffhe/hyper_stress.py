"""Stress recovery of finite-strain solves: the ops behind `HyperelasticFESolver.cauchy_stress` / `cauchy_von_mises` /
`cauchy_stress_and_von_mises` / `energy_density` (ours: the reference solves linear scalar equations only).
`diffhe.hyperelastic` imports this module; this module does not import it: a solver reaches these ops as the object
registered under `handle`, read through the attributes `diffhe.elastic_stress` reads (`_plan()`, `mesh`, `nu`, `plane`,
`_lam1`, `_mu1`).

Kernels: csrc/hyper_stress.hip, include/diffhe_hyper_stress.h.  Per element e and sample b, with the element-constant
displacement gradient H[a][t] = sum_p u[(p, a)] g_p[t], F = I + H and J = det F:

    unit Cauchy stress   s = (1/J) [ mu' (H + H^T + H H^T) + lambda' ln J I ]        (= P1(F) F^T / J)
    stress               sigma = E_e s, symmetric, in the Voigt order and storage of `diffhe.elastic_stress`: nc = 3,
                         (xx, yy, xy) in 2D; nc = 6, (xx, yy, zz, yz, xz, xy) in 3D; a shear component is the tensor
                         component itself, and its cotangent is the derivative with respect to that one number
    out of plane (2D)    sigma_zz = E lambda' ln J / J (plane strain, F33 = 1): `cauchy_stress` returns the in-plane
                         components only, `cauchy_von_mises` includes sigma_zz
    von Mises            the formula of `diffhe.elastic_stress` on sigma; d vm / d sigma = (3/2) dev(sigma) / vm, defined as
                         0 where vm == 0
    energy density       w = E_e W1(F),  W1 = mu'/2 (tr F^T F - d) - mu' ln J + lambda'/2 (ln J)^2, per REFERENCE volume

This is the TRUE stress in the deformed body; the small-strain `stress` of `ElasticFESolver` on a finite-strain displacement
is wrong by O(|grad u|).  For |grad u| -> 0 the two agree to first order in |grad u| (plane strain in 2D).  An element with
J <= 0 gives NaN in its own entries of sigma, vm and w and leaves every other element and sample unchanged to the bit.

u is the full displacement as `forward` returns it, prescribed values included: the evaluation is a pure function of
(u, E, mesh, nu) and reads no Dirichlet data.  An explicit E evaluates the stress with another modulus than the solve
used (the relaxed stress of stress-constrained design); the batch rules are those of E in `diffhe.elastic`, and an
unbatched u with a batched E is broadcast.  The gradients come from one element pass (dL/dE, and the d x d tensor dL/dH
per element, which is not symmetric here) and one node pass over the per-node incidence list (dL/du), in fixed orders:
bitwise reproducible.  With the solve in front,

    E -> HyperelasticFESolver -> cauchy_von_mises -> pnorm

is one differentiable chain with ONE adjoint solve: the cotangent dL/du of this module's backward is the solve's gbar.

Both ops are pure functions of their tensors for the solver registered under `handle`: no adjoint state, backward
recomputes from the saved u and E.  The registry holds a solver weakly, so the autograd context keeps it alive and
registers it again before the backward op, as `_stress_autograd` of `diffhe.elastic_stress` does.

Not implemented: the Piola-Kirchhoff stresses PK1 and PK2, plane stress, eigenstrains, moving nodes, and backward with
create_graph=True (NotImplementedError).
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _hip
from .elastic_stress import _stress_call, _stress_shapes
from .plan import _stream
from .solver import K_ELEM, _SOLVERS, _fake_grads, _kappa_grad, _like_grads

__all__ = ()


def _cauchy_call(solver, u, E, node_major):
    """`_StressCall` of the linear stress ops with the head of this family's entries: no nu_z (sigma_zz is lam1 ln J / J)."""
    call = _stress_call(solver, u, E, node_major)
    call.head = (*call.head[:5], *call.head[6:])        # elems, gtab, dim, lam1, mu1 | u, E and its strides
    return call


def _cauchy_forward(solver, u, E, node_major, want_sigma, want_vm, want_w):
    """(sigma, vm, w) in the caller's layout, None for those not asked for: the kernel writes (m, nc, Bp) and (m, Bp)."""
    call = _cauchy_call(solver, u, E, node_major)
    plan, m, nc, Bp = call.plan, call.plan.m, call.nc, call.Bp
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=plan.device)  # noqa: E731
    sigma = new(m * nc, Bp) if want_sigma else None
    vm, w = (new(m, Bp) if want_vm else None), (new(m, Bp) if want_w else None)
    _hip.lib().diffhe_hyper_stress_eval(*call.head, plan.n, m, Bp, sigma, Bp, nc * Bp, vm, w, _stream(plan.device))
    s_shape, v_shape = _stress_shapes(solver, u, E, node_major)
    if sigma is not None:
        sigma = call.rows_out(sigma, m * nc).reshape(s_shape).to(u.device)
    vm, w = (None if t is None else call.rows_out(t, m).reshape(v_shape).to(u.device) for t in (vm, w))
    return sigma, vm, w


def _cauchy_adjoint(solver, sigma_bar, vm_bar, w_bar, u, E, node_major, need_u, need_e):
    """(dL/du, dL/dE) in the shapes of u and E, None for the one not asked for.  One element pass feeds both where the dE
    of the call is per sample; a field the batch shares takes its dE from the batch-summing entry."""
    call = _cauchy_call(solver, u, E, node_major)
    plan, eng, nc, B, Bp, mode = call.plan, call.eng, call.nc, call.B, call.Bp, call.mode
    d, n, m = plan.dim, plan.n, plan.m
    L, st = _hip.lib(), _stream(plan.device)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=plan.device)  # noqa: E731
    sb = call.rows_in(sigma_bar, m * nc, True) if sigma_bar is not None else None
    vb, wb = (call.rows_in(t, m, True) if t is not None else None for t in (vm_bar, w_bar))
    head = (*call.head, sb, Bp, nc * Bp, vb, wb)
    ubar = new(n * d, Bp) if need_u else None

    def adjoint(nodes, de_e, part, total):
        lists = plan.shape_incidence() if nodes else (None, None)
        L.diffhe_hyper_stress_adjoint(*head, *lists, n, m, B, Bp, new(d * d, m, Bp) if nodes else None,
                                      ubar if nodes else None, de_e, part, total, st)

    grad_u = grad_e = None
    fused = need_u and need_e and mode != K_ELEM
    if need_e:
        sums, de = eng.element_grad(mode, call.em, B, Bp, None,
                                    lambda de_e, osc, ose, part, total: adjoint(fused, de_e, part, total),
                                    lambda de, osc, ose: L.diffhe_hyper_stress_adjoint_shared(*head, n, m, B, Bp, de, st))
        grad_e = _kappa_grad(mode, E.shape, sums, de).to(E.device)
    if need_u:
        if not fused:
            adjoint(True, None, None, None)
        du = call.rows_out(ubar, n * d)
        if node_major:
            grad_u = du.reshape(n, d, B)
        else:
            du = du.reshape(B, n, d)
            grad_u = du if call.batched else du.sum(dim=0)
        grad_u = grad_u.to(u.device)
    return grad_u, grad_e


def _cauchy_shapes(solver, u, E, node_major):
    """-> (shape of sigma, shape of vm, shape of w)."""
    s_shape, v_shape = _stress_shapes(solver, u, E, node_major)
    return s_shape, v_shape, v_shape


@torch.library.custom_op("diffhe::hyper_stress", mutates_args=())
def hyper_stress(u: torch.Tensor, E: torch.Tensor, handle: int, node_major: bool, want_sigma: bool, want_vm: bool,
                 want_w: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(sigma, vm, w) -- Cauchy stress, its von Mises stress, strain-energy density -- of the displacement u and the
    modulus E for the `HyperelasticFESolver` registered under `handle`; an output not asked for comes back empty."""
    outs = _cauchy_forward(_SOLVERS[handle], u, E, node_major, want_sigma, want_vm, want_w)
    return tuple(u.new_empty(0) if t is None else t for t in outs)


@hyper_stress.register_fake
def _hyper_stress_fake(u, E, handle, node_major, want_sigma, want_vm, want_w):
    shapes = _cauchy_shapes(_SOLVERS[handle], u, E, node_major)
    return tuple(u.new_empty(shape if want else 0, dtype=torch.float64)
                 for shape, want in zip(shapes, (want_sigma, want_vm, want_w)))


@torch.library.custom_op("diffhe::hyper_stress_backward", mutates_args=())
def hyper_stress_backward(sigma_bar: torch.Tensor, vm_bar: torch.Tensor, w_bar: torch.Tensor, u: torch.Tensor,
                          E: torch.Tensor, handle: int, node_major: bool, need_u: bool,
                          need_e: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dL/du, dL/dE) of `hyper_stress` for the cotangents of sigma, vm and w (empty = absent); unused ones come back
    empty."""
    bars = (t if t.numel() else None for t in (sigma_bar, vm_bar, w_bar))
    grads = _cauchy_adjoint(_SOLVERS[handle], *bars, u, E, node_major, need_u, need_e)
    return _like_grads(u, grads, (u, E))


@hyper_stress_backward.register_fake
def _hyper_stress_backward_fake(sigma_bar, vm_bar, w_bar, u, E, handle, node_major, need_u, need_e):
    return _fake_grads(u, (need_u, need_e), (u, E))


_REFUSAL = ("diffhe: second-order derivatives of a finite-strain stress evaluation are not implemented (backward with "
            "create_graph=True, diffhe.hyperelastic)")


def _setup_context(ctx, inputs, output):
    u, E, ctx.handle, node_major = inputs[:4]
    ctx.node_major = bool(node_major)
    ctx.solver = _SOLVERS[ctx.handle]       # the registry holds it weakly: the graph keeps it alive for backward
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(u, E)


def _backward(ctx, grad_sigma, grad_vm, grad_w):
    if torch.is_grad_enabled():
        raise NotImplementedError(_REFUSAL)
    u, E = ctx.saved_tensors
    needs = tuple(bool(v) for v in ctx.needs_input_grad[:2])
    bars = (grad_sigma, grad_vm, grad_w)
    absent = lambda g: g is None or g.numel() == 0  # noqa: E731
    if not any(needs) or all(absent(g) for g in bars):
        return (None,) * 7
    empty = u.new_empty(0)
    _SOLVERS[ctx.handle] = ctx.solver
    grads = torch.ops.diffhe.hyper_stress_backward(*(empty if absent(g) else g.contiguous() for g in bars), u, E,
                                                   ctx.handle, ctx.node_major, *needs)
    return (*(g if need else None for g, need in zip(grads, needs)), *(None,) * 5)


torch.library.register_autograd("diffhe::hyper_stress", _backward, setup_context=_setup_context)
