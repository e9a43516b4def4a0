"""Stress recovery and eigenstrain for elastic solves: the ops behind `ElasticFESolver.stress` / `von_mises` /
`stress_and_von_mises` / `eigenstrain_load` and the plain-torch helpers `pnorm`, `thermal_strain`, `element_mean` (ours:
the reference solves scalar equations only).  `diffhe.elastic` re-exports every public name of this module; this module
does not import it: a solver reaches these ops as the object registered under `handle`, read through its attributes
(`_plan()`, `mesh`, `nu`, `plane`, `_lam1`, `_mu1`).

Stress recovery (csrc/stress.hip, include/diffhe_stress.h): `solver.stress(u, E=None)`, `solver.von_mises(u, E=None)`,
`solver.stress_and_von_mises(u, E=None)` and `pnorm(vm, p)`, differentiable in u and E.  Per element e and sample b, with
the element-constant displacement gradient H[a][t] = sum_p u[(p, a)] g_p[t] and eps = (H + H^T) / 2:

    unit stress   s = 2 mu' eps + lambda' tr(eps) I,   (lambda', mu') = lame_unit(nu, dim, plane)
    stress        sigma = E_e s
    Voigt order   diffhe.aniso's: nc = 3, (xx, yy, xy) in 2D; nc = 6, (xx, yy, zz, yz, xz, xy) in 3D.  A shear component
                  is the tensor component itself, not doubled; its cotangent is the derivative with respect to that one
                  number.
    out of plane  plane stress: sigma_zz = 0; plane strain: sigma_zz = E lambda' tr(eps) = nu (sigma_xx + sigma_yy).
                  `stress` returns the in-plane components only, `von_mises` includes sigma_zz.
    von Mises     vm^2 = 1/2 [(s_xx - s_yy)^2 + (s_yy - s_zz)^2 + (s_zz - s_xx)^2] + 3 (s_xy^2 + s_yz^2 + s_xz^2) of sigma,
                  absent components zero; d vm / d sigma = (3/2) dev(sigma) / vm, defined as 0 where vm == 0: no NaN or
                  Inf leaves the kernels.

u is the full displacement as `forward` returns it, prescribed values included: the evaluation is a pure function of
(u, E, mesh, nu, plane) and reads no Dirichlet data.  An explicit E evaluates the stress with another modulus than the
solve used (the relaxed stress rho^q E_0 D eps of stress-constrained SIMP); the batch rules are those of E in
`diffhe.elastic`, and an unbatched u with a batched E is broadcast.  The gradients come from one element pass (dL/dE, and
a symmetric tensor per element) and one node pass over the per-node incidence list (dL/du), in fixed orders: bitwise
reproducible.

Eigenstrain (csrc/eigenstrain.hip, the eigen instantiations of csrc/stress.hip, include/diffhe_eigenstrain.h): an initial
strain eps0 per element and sample -- thermal expansion, swelling, shrinkage, pre-stress.  nc0 = 3 components (xx, yy, xy)
in plane stress, 4 in plane strain, (xx, yy, xy, zz): the total eps_zz is 0 there, so an eps0_zz is constrained and loads
the body in plane; 6 in 3D; shear components are tensor components.  Layouts: (nc0,), (B, nc0), (m, nc0), (B, m, nc0), and
(nc0, m, B) with layout="node" -- `AnisotropicFESolver`'s -- with the batch rules of `_kappa_layout`.

    unit initial stress   s0 = 2 mu' eps0 + lambda' theta0 I in plane, theta0 = tr eps0 over ALL stored normal components
    load                  F0[(i, a)] = sum_{(e, p) at i} vol_e E_e sum_t s0_e[a][t] grad phi_p[t]: K(E) u = M f + load + F0
    stress                sigma = E (s(u) - s0) in plane; sigma_zz = E [lambda' (tr eps(u) - theta0) - 2 mu' eps0_zz] in
                          plane strain (NOT nu (sigma_xx + sigma_yy)), 0 in plane stress

`solver.eigenstrain_load(eps0, E=None)` is F0, differentiable in eps0 and E; `solver(f, load, eigenstrain=eps0)` adds it
to `load` in front of the unchanged solve, so that dL/dload = lambda flows back into dL/deps0 and the second E path, which
autograd adds to the solve's; `stress` / `von_mises` / `stress_and_von_mises(..., eigenstrain=eps0)` evaluate the stress
above with gradients to u, E and eps0.  `thermal_strain(alpha, dT, dim, plane)` and `element_mean(T, mesh)` (plain torch)
carry the temperature of a heat solve to eps0.  The gradient of an eps0 shared over elements or samples is a torch `sum`
of the kernel's per-element, per-sample array over the shared axes.

All ops here are pure functions of their tensors for the solver registered under `handle`: no adjoint state, backward
recomputes from the saved inputs.  The registry holds a solver weakly, so the autograd context of every op keeps it alive
and registers it again before the backward op (`_stress_autograd` for the three stress ops, `_load_setup_context` for the
load).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _hip
from .plan import padded_batch, _stream
from .solver import (K_ELEM, K_SAMPLE, K_SAMPLE_ELEM, K_SCALAR, _Engine, _SOLVERS, _kappa_grad, _kappa_layout,
                     _kappa_mode, _like_grads, _fake_grads, _tensor_mode)

__all__ = ("pnorm", "thermal_strain", "element_mean", "eigen_components")


# ---------------------------------------------------------------------------------------------
# Stress recovery: diffhe::elastic_stress / diffhe::elastic_stress_backward (csrc/stress.hip, include/diffhe_stress.h).
# A pure function of (u, E) for the solver registered under `handle`: no adjoint state, backward recomputes from u and E.
# ---------------------------------------------------------------------------------------------
@dataclass
class _StressCall:
    """One evaluation: the device views the kernels read and the facts both directions share."""
    plan: object
    eng: _Engine
    B: int
    Bp: int
    mode: int
    em: bool
    batched: bool           # u came with a batch dimension
    node_major: bool
    head: tuple             # the leading arguments of the three entries, up to e_sb
    nc: int

    def rows_in(self, t: torch.Tensor, rows: int, batched: bool) -> torch.Tensor:
        """(B, rows...) | (rows...) broadcast to the batch | node-major (rows..., B) -> (rows, Bp), padding samples zero."""
        B, Bp, dev = self.B, self.Bp, self.plan.device
        t = t.detach().to(dev, torch.float64)
        if self.node_major:
            src = t.reshape(rows, B)
            if Bp == B and src.is_contiguous():
                return src
            out = torch.zeros((rows, Bp), dtype=torch.float64, device=dev)
            out[:, :B] = src
            return out
        src = t.reshape(B, rows).contiguous() if batched else t.reshape(rows).contiguous()
        return self.eng.to_node_major(src, B, Bp, rows)

    def rows_out(self, x: torch.Tensor, rows: int) -> torch.Tensor:
        """(rows, Bp) -> (B, rows), or node-major (rows, B): the kernel's array itself when B needs no padding."""
        if self.node_major:
            return x if self.Bp == self.B else x[:, :self.B].contiguous()
        return self.eng.to_sample_major(x, self.B, self.Bp, rows)


def _stress_batch(u: torch.Tensor, node_major: bool) -> Optional[int]:
    return u.shape[2] if node_major else (u.shape[0] if u.dim() == 3 else None)


def _stress_shapes(solver, u, E, node_major):
    """-> (shape of sigma, shape of vm) for u and E as the op gets them."""
    m, d = solver.mesh.n_elements, solver.mesh.dim
    nc = d * (d + 1) // 2
    B_u = _stress_batch(u, node_major)
    _, B, _ = _kappa_layout(E, m, B_u, node_major)
    if node_major:
        return (m, nc, B), (m, B)
    return ((B, m, nc), (B, m)) if (B_u is not None or B > 1) else ((m, nc), (m,))


def _stress_call(solver: "ElasticFESolver", u, E, node_major) -> _StressCall:
    plan = solver._plan()
    d, n, m = plan.dim, plan.n, plan.m
    B_u = _stress_batch(u, node_major)
    mode, B, em = _kappa_layout(E, m, B_u, node_major)
    Bp = padded_batch(B)
    eng = _Engine(plan, 0.0, 0, 0, "gather")
    call = _StressCall(plan, eng, B, Bp, mode, em, B_u is not None, node_major, (), d * (d + 1) // 2)
    udev = call.rows_in(u, n * d, call.batched)
    kdev, kse, ksb, _ = eng.kappa_device(E, mode, B, Bp, em=em)
    gtab = plan.oriented_gradient_table()                        # the stress is linear in grad phi: its sign counts
    nu_z = solver.nu if solver.plane == "strain" else 0.0       # sigma_zz = nu_z (sigma_xx + sigma_yy), 2D only
    call.head = (plan.elems, gtab, d, solver._lam1, solver._mu1, nu_z, udev, kdev, kse, ksb)
    return call


def _stress_forward(solver, u, E, node_major, want_sigma, want_vm):
    """(sigma, vm) in the caller's layout, None for the one not asked for: the kernel writes (m, nc, Bp) and (m, Bp)."""
    call = _stress_call(solver, u, E, node_major)
    plan, m, nc, B, Bp = call.plan, call.plan.m, call.nc, call.B, call.Bp
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=plan.device)  # noqa: E731
    sigma, vm = (new(m * nc, Bp) if want_sigma else None), (new(m, Bp) if want_vm else None)
    _hip.lib().diffhe_stress_eval(*call.head, plan.n, m, Bp, sigma, Bp, nc * Bp, vm, _stream(plan.device))
    s_shape, v_shape = _stress_shapes(solver, u, E, node_major)
    if sigma is not None:
        sigma = call.rows_out(sigma, m * nc).reshape(s_shape).to(u.device)
    if vm is not None:
        vm = call.rows_out(vm, m).reshape(v_shape).to(u.device)
    return sigma, vm


def _stress_adjoint(solver, sigma_bar, vm_bar, u, E, node_major, need_u, need_e):
    """(dL/du, dL/dE) in the shapes of u and E, None for the one not asked for.  One element pass feeds both where the
    dE of the call is per sample; a field the batch shares takes its dE from the batch-summing entry."""
    call = _stress_call(solver, u, E, node_major)
    plan, eng, nc, B, Bp, mode = call.plan, call.eng, call.nc, call.B, call.Bp, call.mode
    d, n, m = plan.dim, plan.n, plan.m
    L, st = _hip.lib(), _stream(plan.device)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=plan.device)  # noqa: E731
    sb = call.rows_in(sigma_bar, m * nc, True) if sigma_bar is not None else None
    vb = call.rows_in(vm_bar, m, True) if vm_bar is not None else None
    head = (*call.head, sb, Bp, nc * Bp, vb)
    ubar = new(n * d, Bp) if need_u else None

    def adjoint(nodes, de_e, part, total):
        lists = plan.shape_incidence() if nodes else (None, None)
        L.diffhe_stress_adjoint(*head, *lists, n, m, B, Bp, new(nc, m, Bp) if nodes else None, ubar if nodes else None,
                                de_e, part, total, st)

    grad_u = grad_e = None
    fused = need_u and need_e and mode != K_ELEM
    if need_e:
        sums, de = eng.element_grad(mode, call.em, B, Bp, None,
                                    lambda de_e, osc, ose, part, total: adjoint(fused, de_e, part, total),
                                    lambda de, osc, ose: L.diffhe_stress_adjoint_shared(*head, n, m, B, Bp, de, st))
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


@torch.library.custom_op("diffhe::elastic_stress", mutates_args=())
def elastic_stress(u: torch.Tensor, E: torch.Tensor, handle: int, node_major: bool, want_sigma: bool,
                   want_vm: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sigma, vm) of the displacement u and the modulus E for the `ElasticFESolver` registered under `handle`; the
    output not asked for comes back empty."""
    return _stress_outputs(u, *_stress_forward(_SOLVERS[handle], u, E, node_major, want_sigma, want_vm))


def _stress_outputs(u, sigma, vm):
    """What a stress op returns: the output not asked for (None) comes back empty."""
    return (u.new_empty(0) if sigma is None else sigma), (u.new_empty(0) if vm is None else vm)


def _stress_fake(u, shapes, want_sigma: bool, want_vm: bool):
    """(sigma, vm) of a stress op's fake (meta) implementation for `shapes` = (shape of sigma, shape of vm)."""
    return (u.new_empty(shapes[0] if want_sigma else 0, dtype=torch.float64),
            u.new_empty(shapes[1] if want_vm else 0, dtype=torch.float64))


@elastic_stress.register_fake
def _elastic_stress_fake(u, E, handle, node_major, want_sigma, want_vm):
    return _stress_fake(u, _stress_shapes(_SOLVERS[handle], u, E, node_major), want_sigma, want_vm)


@torch.library.custom_op("diffhe::elastic_stress_backward", mutates_args=())
def elastic_stress_backward(sigma_bar: torch.Tensor, vm_bar: torch.Tensor, u: torch.Tensor, E: torch.Tensor, handle: int,
                            node_major: bool, need_u: bool, need_e: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dL/du, dL/dE) of `elastic_stress` for the cotangents of sigma and vm (empty = absent); unused ones come back
    empty."""
    grads = _stress_adjoint(_SOLVERS[handle], sigma_bar if sigma_bar.numel() else None,
                            vm_bar if vm_bar.numel() else None, u, E, node_major, need_u, need_e)
    return _like_grads(u, grads, (u, E))


@elastic_stress_backward.register_fake
def _elastic_stress_backward_fake(sigma_bar, vm_bar, u, E, handle, node_major, need_u, need_e):
    return _fake_grads(u, (need_u, need_e), (u, E))


def _stress_autograd(op: str, n_diff: int, n_in: int, refusal: str):
    """Register and return (setup_context, backward) of the stress op `op`, whose `n_in` inputs are `n_diff` differentiable
    tensors, then (..., handle, node_major, want_sigma, want_vm), and whose backward op diffhe::<op>_backward takes
    (sigma_bar, vm_bar, *tensors, handle, node_major, *needs).  The context keeps the solver: the registry holds it weakly,
    the graph keeps it alive and registers it again for the backward op.  refusal: the text of the create_graph=True
    error."""
    def setup_context(ctx, inputs, output):
        ctx.handle, ctx.node_major = inputs[n_in - 4], bool(inputs[n_in - 3])
        ctx.solver = _SOLVERS[ctx.handle]
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*inputs[:n_diff])

    def backward(ctx, grad_sigma, grad_vm):
        if torch.is_grad_enabled():
            raise NotImplementedError(refusal)
        tensors = ctx.saved_tensors
        needs = tuple(bool(v) for v in ctx.needs_input_grad[:n_diff])
        absent = lambda g: g is None or g.numel() == 0  # noqa: E731
        if not any(needs) or (absent(grad_sigma) and absent(grad_vm)):
            return (None,) * n_in
        empty = tensors[0].new_empty(0)
        _SOLVERS[ctx.handle] = ctx.solver
        grads = getattr(torch.ops.diffhe, op + "_backward")(
            empty if absent(grad_sigma) else grad_sigma.contiguous(), empty if absent(grad_vm) else grad_vm.contiguous(),
            *tensors, ctx.handle, ctx.node_major, *needs)
        return (*(g if need else None for g, need in zip(grads, needs)), *(None,) * (n_in - n_diff))

    torch.library.register_autograd("diffhe::" + op, backward, setup_context=setup_context)
    return setup_context, backward


_STRESS_REFUSAL = ("diffhe: second-order derivatives of an elastic stress evaluation are not implemented (backward with "
                   "create_graph=True, diffhe.elastic)")
_stress_setup_context, _stress_backward = _stress_autograd("elastic_stress", 2, 6, _STRESS_REFUSAL)


# ---------------------------------------------------------------------------------------------
# Eigenstrain (csrc/eigenstrain.hip and the eigen instantiations of csrc/stress.hip, include/diffhe_eigenstrain.h):
# diffhe::eigenstrain_load / eigenstrain_load_backward, the load F0(eps0, E), and diffhe::elastic_stress_eigen /
# elastic_stress_eigen_backward, the stress E (s(u) - s0).  Pure functions of their tensors for the solver registered under
# `handle`: backward recomputes from the saved inputs.
# ---------------------------------------------------------------------------------------------
def eigen_components(dim: int, plane: Optional[str]) -> int:
    """nc0: 6 in 3D, 4 in plane strain (xx, yy, xy, zz), 3 in plane stress."""
    return 6 if dim == 3 else (4 if plane == "strain" else 3)


def _eigen_batch(eps0, E, m: int, nc0: int, node_major: bool, B_hint: Optional[int]) -> Optional[int]:
    """The batch of one call: the hint (the batch of f, load or u), else that of whichever of eps0 and E shows one, the
    shapes that read only one way first; None: nothing is batched.  The shapes that read both ways -- (m, nc0) and (m,)
    with m equal to the batch -- are then classified WITH that batch, by the tie rule of `_kappa_layout`."""
    if B_hint is not None:
        return B_hint
    if eps0.dim() == 3:
        return eps0.shape[2] if (node_major and tuple(eps0.shape[:2]) == (nc0, m)) else eps0.shape[0]
    if E.dim() == 2:
        return E.shape[1] if (node_major and E.shape[0] == m) else E.shape[0]
    _, B_z, _ = _tensor_mode(eps0, nc0, m, None, node_major)
    return B_z if B_z is not None else _kappa_mode(E, m, None)[1]


@dataclass
class _EigenCall(_StressCall):
    """`_StressCall` (mode, em: those of E) with the eigenstrain of the call."""
    mode_z: int = 0
    em_z: bool = False
    nc0: int = 0
    zhead: tuple = ()       # lam1, mu1, plane_strain, E and its strides, eps0 and its strides

    def eps0_out(self):
        """(array, stride per component, per element) of the kernels' d / d eps0: (m, nc0, Bp) where the caller's
        (B, m, nc0) is one transposing pass away, else (nc0, m, Bp)."""
        m, nc0, Bp = self.plan.m, self.nc0, self.Bp
        if self.mode_z == K_SAMPLE_ELEM and not self.em_z:
            return torch.empty((m, nc0, Bp), dtype=torch.float64, device=self.plan.device), Bp, nc0 * Bp
        return torch.empty((nc0, m, Bp), dtype=torch.float64, device=self.plan.device), m * Bp, Bp

    def eps0_grad(self, d: torch.Tensor, shape) -> torch.Tensor:
        """That array in the shape of the caller's eps0.  A tensor shared over elements or samples is a torch `sum` of the
        contiguous (nc0, m, Bp) array (padding samples hold zeros) over the shared axes: a reduction whose order torch
        decides, like the batch sum of an unbatched u's gradient and autograd's sum over a broadcast load (DESIGN
        section 7, "Eigenstrain")."""
        m, nc0, B, Bp = self.plan.m, self.nc0, self.B, self.Bp
        if self.mode_z == K_SAMPLE_ELEM:
            if self.em_z:
                return (d if Bp == B else d[..., :B].contiguous()).reshape(shape)
            return self.eng.to_sample_major(d.view(m * nc0, Bp), B, Bp, m * nc0).reshape(shape)
        if self.mode_z == K_ELEM:
            return d.sum(dim=2).t().reshape(shape)
        if self.mode_z == K_SAMPLE:
            return d.sum(dim=1)[:, :B].t().reshape(shape)
        return d.sum(dim=(1, 2)).reshape(shape)


def _eigen_call(solver: "ElasticFESolver", eps0, E, node_major: bool, B_hint: Optional[int], collapse: bool,
                u=None) -> _EigenCall:
    """The device views and facts of one eigenstrain call.  collapse: with neither eps0 nor E batched the call is one
    sample whatever the hint says (a load every sample shares)."""
    plan = solver._plan()
    d, n, m = plan.dim, plan.n, plan.m
    nc0 = eigen_components(d, solver.plane)
    B0 = _eigen_batch(eps0, E, m, nc0, node_major, B_hint)
    mode_z, B, em_z = _kappa_layout(eps0, m, B0, node_major, nc0)
    mode, B_e, em = _kappa_layout(E, m, B0, node_major)
    if B_e != B:
        raise ValueError(f"E batch {B_e} does not match eigenstrain batch {B}")
    batched = B0 is not None
    if collapse and mode_z in (K_SCALAR, K_ELEM) and mode in (K_SCALAR, K_ELEM):
        B, batched = 1, False
    Bp = padded_batch(B)
    eng = _Engine(plan, 0.0, 0, 0, "gather")
    call = _EigenCall(plan, eng, B, Bp, mode, em, batched, node_major, (), d * (d + 1) // 2, mode_z, em_z, nc0)
    kdev, kse, ksb, _ = eng.kappa_device(E, mode, B, Bp, em=em)
    zdev, zc, ze, zb, _ = eng.tensor_device(eps0, mode_z, B, Bp, nc0, em=em_z)
    call.zhead = (solver._lam1, solver._mu1, int(solver.plane == "strain"), kdev, kse, ksb, zdev, zc, ze, zb)
    if u is not None:
        udev = call.rows_in(u, n * d, u.dim() == 3)
        call.head = (plan.elems, plan.oriented_gradient_table(), d, *call.zhead[:3], udev, *call.zhead[3:])
    return call


def _load_shape(call: _EigenCall):
    n, d = call.plan.n, call.plan.dim
    return (n, d, call.B) if call.node_major else ((call.B, n, d) if call.batched else (n, d))


def _hint(B_hint: int) -> Optional[int]:
    return None if B_hint < 0 else B_hint


@torch.library.custom_op("diffhe::eigenstrain_load", mutates_args=())
def eigenstrain_load_op(eps0: torch.Tensor, E: torch.Tensor, handle: int, node_major: bool, B_hint: int) -> torch.Tensor:
    """F0 of the eigenstrain eps0 and the modulus E for the `ElasticFESolver` registered under `handle`; B_hint: the
    batch of the right-hand side the load joins, -1 for none."""
    call = _eigen_call(_SOLVERS[handle], eps0, E, node_major, _hint(B_hint), True)
    plan = call.plan
    F0 = torch.empty((plan.n * plan.dim, call.Bp), dtype=torch.float64, device=plan.device)
    _, vol = plan.gradient_table()
    _hip.lib().diffhe_eigenstrain_load(*plan.shape_incidence(), plan.oriented_gradient_table(), vol, plan.dim, *call.zhead,
                                       plan.n, plan.m, call.B, call.Bp, F0, _stream(plan.device))
    return call.rows_out(F0, plan.n * plan.dim).reshape(_load_shape(call)).to(eps0.device)


@eigenstrain_load_op.register_fake
def _eigenstrain_load_fake(eps0, E, handle, node_major, B_hint):
    solver = _SOLVERS[handle]
    n, d, m = solver.mesh.n_nodes, solver.mesh.dim, solver.mesh.n_elements
    nc0 = eigen_components(d, solver.plane)
    B0 = _eigen_batch(eps0, E, m, nc0, node_major, _hint(B_hint))
    mode_z, B, _ = _kappa_layout(eps0, m, B0, node_major, nc0)
    mode, _, _ = _kappa_layout(E, m, B0, node_major)
    if mode_z in (K_SCALAR, K_ELEM) and mode in (K_SCALAR, K_ELEM):
        B, B0 = 1, None
    return eps0.new_empty((n, d, B) if node_major else ((B, n, d) if B0 is not None else (n, d)), dtype=torch.float64)


@torch.library.custom_op("diffhe::eigenstrain_load_backward", mutates_args=())
def eigenstrain_load_backward(gbar: torch.Tensor, eps0: torch.Tensor, E: torch.Tensor, handle: int, node_major: bool,
                              B_hint: int, need_z: bool, need_e: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dL/deps0, dL/dE) of `eigenstrain_load` for the cotangent of F0; unused ones come back empty."""
    call = _eigen_call(_SOLVERS[handle], eps0, E, node_major, _hint(B_hint), True)
    plan, B, Bp = call.plan, call.B, call.Bp
    L, st = _hip.lib(), _stream(plan.device)
    _, vol = plan.gradient_table()
    w = call.rows_in(gbar, plan.n * plan.dim, call.batched)
    head = (plan.elems, plan.oriented_gradient_table(), vol, plan.dim, *call.zhead, w, plan.n, plan.m, B, Bp)
    deps, osc, ose = call.eps0_out() if need_z else (None, 0, 0)
    grad_z = grad_e = None
    fused = need_z and need_e and call.mode != K_ELEM           # one element pass for both
    if need_e:
        sums, de = call.eng.element_grad(
            call.mode, call.em, B, Bp, None,
            lambda de_e, _osc, _ose, part, total: L.diffhe_eigenstrain_load_adjoint(
                *head, deps if fused else None, osc, ose, de_e, part, total, st),
            lambda de, _osc, _ose: L.diffhe_eigenstrain_load_adjoint_shared(*head, de, st))
        grad_e = _kappa_grad(call.mode, E.shape, sums, de).to(E.device)
    if need_z:
        if not fused:
            L.diffhe_eigenstrain_load_adjoint(*head, deps, osc, ose, None, None, None, st)
        grad_z = call.eps0_grad(deps, eps0.shape).to(eps0.device)
    return _like_grads(gbar, (grad_z, grad_e), (eps0, E))


@eigenstrain_load_backward.register_fake
def _eigenstrain_load_backward_fake(gbar, eps0, E, handle, node_major, B_hint, need_z, need_e):
    return _fake_grads(gbar, (need_z, need_e), (eps0, E))


def _load_setup_context(ctx, inputs, output):
    eps0, E, ctx.handle, node_major, ctx.B_hint = inputs
    ctx.node_major = bool(node_major)
    ctx.solver = _SOLVERS[ctx.handle]       # the registry holds it weakly: the graph keeps it alive for backward
    ctx.save_for_backward(eps0, E)


def _load_backward(ctx, grad_F):
    if torch.is_grad_enabled():
        raise NotImplementedError("diffhe: second-order derivatives of an eigenstrain load are not implemented (backward "
                                  "with create_graph=True, diffhe.elastic)")
    eps0, E = ctx.saved_tensors
    need_z, need_e = (bool(v) for v in ctx.needs_input_grad[:2])
    if not (need_z or need_e):
        return (None,) * 5
    _SOLVERS[ctx.handle] = ctx.solver
    dz, de = torch.ops.diffhe.eigenstrain_load_backward(grad_F.contiguous(), eps0, E, ctx.handle, ctx.node_major,
                                                        ctx.B_hint, need_z, need_e)
    return (dz if need_z else None, de if need_e else None, None, None, None)


torch.library.register_autograd("diffhe::eigenstrain_load", _load_backward, setup_context=_load_setup_context)


def _stress_shapes_eigen(solver, u, E, eps0, node_major):
    m, d = solver.mesh.n_elements, solver.mesh.dim
    nc, nc0 = d * (d + 1) // 2, eigen_components(d, solver.plane)
    B0 = _eigen_batch(eps0, E, m, nc0, node_major, _stress_batch(u, node_major))
    _, B, _ = _kappa_layout(eps0, m, B0, node_major, nc0)
    if node_major:
        return (m, nc, B), (m, B)
    return ((B, m, nc), (B, m)) if B0 is not None else ((m, nc), (m,))


@torch.library.custom_op("diffhe::elastic_stress_eigen", mutates_args=())
def elastic_stress_eigen(u: torch.Tensor, E: torch.Tensor, eps0: torch.Tensor, handle: int, node_major: bool,
                         want_sigma: bool, want_vm: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sigma, vm) of `elastic_stress` with the eigenstrain eps0: sigma = E (s(u) - s0)."""
    solver = _SOLVERS[handle]
    call = _eigen_call(solver, eps0, E, node_major, _stress_batch(u, node_major), False, u=u)
    plan, m, nc, Bp = call.plan, call.plan.m, call.nc, call.Bp
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=plan.device)  # noqa: E731
    sigma, vm = (new(m * nc, Bp) if want_sigma else None), (new(m, Bp) if want_vm else None)
    _hip.lib().diffhe_stress_eval_eigen(*call.head, plan.n, m, Bp, sigma, Bp, nc * Bp, vm, _stream(plan.device))
    s_shape, v_shape = _stress_shapes_eigen(solver, u, E, eps0, node_major)
    sigma = u.new_empty(0) if sigma is None else call.rows_out(sigma, m * nc).reshape(s_shape).to(u.device)
    vm = u.new_empty(0) if vm is None else call.rows_out(vm, m).reshape(v_shape).to(u.device)
    return sigma, vm


@elastic_stress_eigen.register_fake
def _elastic_stress_eigen_fake(u, E, eps0, handle, node_major, want_sigma, want_vm):
    return _stress_fake(u, _stress_shapes_eigen(_SOLVERS[handle], u, E, eps0, node_major), want_sigma, want_vm)


@torch.library.custom_op("diffhe::elastic_stress_eigen_backward", mutates_args=())
def elastic_stress_eigen_backward(sigma_bar: torch.Tensor, vm_bar: torch.Tensor, u: torch.Tensor, E: torch.Tensor,
                                  eps0: torch.Tensor, handle: int, node_major: bool, need_u: bool, need_e: bool,
                                  need_z: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dL/du, dL/dE, dL/deps0) of `elastic_stress_eigen` for the cotangents of sigma and vm (empty = absent); unused
    ones come back empty.  One element pass feeds all three where the dE of the call is per sample."""
    call = _eigen_call(_SOLVERS[handle], eps0, E, node_major, _stress_batch(u, node_major), False, u=u)
    plan, eng, nc, B, Bp, mode = call.plan, call.eng, call.nc, call.B, call.Bp, call.mode
    d, n, m = plan.dim, plan.n, plan.m
    L, st = _hip.lib(), _stream(plan.device)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=plan.device)  # noqa: E731
    sb = call.rows_in(sigma_bar, m * nc, True) if sigma_bar.numel() else None
    vb = call.rows_in(vm_bar, m, True) if vm_bar.numel() else None
    head = (*call.head, sb, Bp, nc * Bp, vb)
    ubar = new(n * d, Bp) if need_u else None
    deps, dzc, dze = call.eps0_out() if need_z else (None, 0, 0)

    def adjoint(side, de_e, part, total):
        """The element pass (and the node pass) with the side products u_bar and d / d eps0, or with dE alone."""
        nodes = side and need_u
        lists = plan.shape_incidence() if nodes else (None, None)
        L.diffhe_stress_adjoint_eigen(*head, *lists, n, m, B, Bp, new(nc, m, Bp) if nodes else None,
                                      ubar if nodes else None, de_e, part, total, deps if side else None, dzc, dze, st)

    grad_u = grad_e = grad_z = None
    side = need_u or need_z
    fused = side and need_e and mode != K_ELEM
    if need_e:
        sums, de = eng.element_grad(mode, call.em, B, Bp, None,
                                    lambda de_e, osc, ose, part, total: adjoint(fused, de_e, part, total),
                                    lambda de, osc, ose: L.diffhe_stress_adjoint_eigen_shared(*head, n, m, B, Bp, de, st))
        grad_e = _kappa_grad(mode, E.shape, sums, de).to(E.device)
    if side and not fused:
        adjoint(True, None, None, None)
    if need_u:
        du = call.rows_out(ubar, n * d)
        if node_major:
            grad_u = du.reshape(n, d, B)
        else:
            du = du.reshape(B, n, d)
            grad_u = du if u.dim() == 3 else du.sum(dim=0)
        grad_u = grad_u.to(u.device)
    if need_z:
        grad_z = call.eps0_grad(deps, eps0.shape).to(eps0.device)
    return _like_grads(u, (grad_u, grad_e, grad_z), (u, E, eps0))


@elastic_stress_eigen_backward.register_fake
def _elastic_stress_eigen_backward_fake(sigma_bar, vm_bar, u, E, eps0, handle, node_major, need_u, need_e, need_z):
    return _fake_grads(u, (need_u, need_e, need_z), (u, E, eps0))


_stress_eigen_setup_context, _stress_eigen_backward = _stress_autograd("elastic_stress_eigen", 3, 7, _STRESS_REFUSAL)


def thermal_strain(alpha, dT: torch.Tensor, dim: int, plane: Optional[str] = None) -> torch.Tensor:
    """The isotropic eigenstrain eps0 = alpha dT on the normal components, shears zero: (m, nc0) or (B, m, nc0) for dT (m,)
    or (B, m), nc0 = 6 in 3D, 3 in plane stress (the 2D default), 4 in plane strain (zz included: the expansion out of
    the plane is constrained).  alpha: a number or a tensor that broadcasts against dT, e.g. per element (m,).  Plain
    differentiable torch."""
    if dim not in (2, 3):
        raise ValueError(f"thermal_strain: dim must be 2 or 3, got {dim!r}")
    if dim == 3 and plane is not None:
        raise ValueError("plane= applies to 2D only")
    plane = None if dim == 3 else ("stress" if plane is None else plane)
    if dim == 2 and plane not in ("stress", "strain"):
        raise ValueError(f"Unknown plane: {plane!r} (\"stress\" or \"strain\")")
    if dT.dim() not in (1, 2):
        raise ValueError(f"thermal_strain: dT must be (m,) or (B, m), got {tuple(dT.shape)}")
    v = torch.as_tensor(alpha, dtype=dT.dtype, device=dT.device) * dT
    zero = torch.zeros_like(v)
    parts = {6: (v, v, v, zero, zero, zero), 4: (v, v, zero, v), 3: (v, v, zero)}[eigen_components(dim, plane)]
    return torch.stack(parts, dim=-1)


def element_mean(T: torch.Tensor, mesh) -> torch.Tensor:
    """The mean of a nodal field (n,) or (B, n) over the vertices of every element: (m,) or (B, m).  Plain differentiable
    torch; with `thermal_strain` it carries the temperature of a heat solve to an eigenstrain."""
    if T.dim() not in (1, 2) or T.shape[-1] != mesh.n_nodes:
        raise ValueError(f"element_mean: T must be (n,) or (B, n) with n={mesh.n_nodes}, got {tuple(T.shape)}")
    return T[..., mesh.elements.to(T.device).long()].mean(dim=-1)


def pnorm(vm: torch.Tensor, p: float = 8.0, weights: Optional[torch.Tensor] = None, dim: int = -1) -> torch.Tensor:
    """The weighted p-mean (sum_e w_e vm_e^p / sum_e w_e)^(1/p) over the element axis `dim` of a non-negative field: the
    last axis of `von_mises(..., layout="sample")`, the first (dim=0) of layout="node".  It lies between max(vm) m^(-1/p)
    and max(vm).  Plain differentiable torch, evaluated as vmax (sum w (vm / vmax)^p / sum w)^(1/p) with vmax detached, so
    that a large p neither overflows nor underflows; an all-zero row gives 0 with zero gradient."""
    p = float(p)
    if not p >= 1.0:
        raise ValueError(f"pnorm needs p >= 1, got {p!r}")
    if weights is None:
        w = torch.ones((), dtype=vm.dtype, device=vm.device)
        wsum = float(vm.shape[dim])
    else:
        w = torch.as_tensor(weights, dtype=vm.dtype, device=vm.device)
        if w.dim() == 1 and vm.dim() > 1:
            shape = [1] * vm.dim()
            shape[dim] = w.shape[0]
            w = w.reshape(shape)
        wsum = w.sum(dim=dim if w.dim() == vm.dim() else -1)
    vmax = vm.detach().abs().amax(dim=dim, keepdim=True)
    live = vmax > 0
    r = vm / torch.where(live, vmax, torch.ones_like(vmax))
    s = (w * r ** p).sum(dim=dim) / wsum
    live, vmax = live.squeeze(dim) & (s > 0), vmax.squeeze(dim)
    root = torch.where(live, s, torch.ones_like(s)) ** (1.0 / p)
    return torch.where(live, vmax * root, torch.zeros_like(root))
