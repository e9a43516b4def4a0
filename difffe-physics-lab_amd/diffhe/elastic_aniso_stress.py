"""Stress recovery and quadratic failure criteria for anisotropic elasticity: the ops behind
`AnisotropicElasticFESolver.tensor_stress` / `failure_index` / `tensor_stress_and_failure_index` and the plain-torch
criterion helpers `tsai_wu`, `tsai_hill`, `quadratic`, `split`, `von_mises_criterion`, `rotated_criterion` (ours: the
reference solves scalar equations only).  This module imports `diffhe.elastic_aniso` for the conventions of C; the solver
reaches it from inside its methods, as the object registered under `handle`.

Kernels: csrc/elastic_aniso_stress.hip, include/diffhe_elastic_aniso_stress.h.  Per element e and sample b, with the
element-constant displacement gradient H[a][t] = sum_p u[(p, a)] g_p[t]:

    strain          eps_I = H[a][a] on normals, H[a][t] + H[t][a] on shears: the engineering Voigt strain of
                    `diffhe.elastic_aniso`
    stress          sigma = C eps, in the Voigt order and storage of `diffhe.elastic_stress`: nc = 3, (xx, yy, xy) in 2D;
                    nc = 6, (xx, yy, zz, yz, xz, xy) in 3D; a shear component is the tensor component itself, and its
                    cotangent is the derivative with respect to that one number
    failure index   phi = q . sigma + sigma . Q sigma on those Voigt components, for a criterion (q, Q) per element and
                    sample; phi = 1 is the failure envelope of Tsai-Wu, Tsai-Hill, Hoffman and (vm / sigma_y)^2

A criterion is ONE tensor of nk = nv + nt components (9 in 2D, 27 in 3D): q first, then the upper triangle of the
symmetric Q, row-major, under the rule of C -- an off-diagonal component is one parameter that fills both entries, and
its gradient is the derivative with respect to that parameter.  Layouts: (nk,), (B, nk), (m, nk), (B, m, nk), and
(nk, m, B) with layout="node", resolved like C.  `rotated_criterion` turns a criterion with its material: phi'(sigma) =
phi(R^T sigma R) on the stress TENSOR, so the factors 2 that the Voigt shear entries need are inside the helper.  A von
Mises stress is not defined for a reduced plane stiffness, which does not determine sigma_zz: `von_mises_criterion` says
which plane assumption is meant.

u is the full displacement as `forward` returns it, prescribed values included: the evaluation is a pure function of
(u, C, criterion, mesh) and reads no Dirichlet data.  An explicit C evaluates the stress with another tensor than the
solve used (the relaxed stress of stress-constrained design); the batch rules are those of C in `diffhe.elastic_aniso`,
and an unbatched u with a batched C or criterion is broadcast.  C and the criterion have independent layouts.  The
gradients come from element passes (dL/dC; dL/d criterion; the symmetric tensor dL/dH per element) and the node pass of
`diffhe.elastic_stress` over the per-node incidence list (dL/du), in fixed orders: bitwise reproducible.  With the solve
in front,

    theta -> C(theta), (q, Q)(theta) -> AnisotropicElasticFESolver -> failure_index -> pnorm

is one differentiable chain with ONE adjoint solve: the cotangent dL/du of this module's backward is the solve's gbar.

Both ops are pure functions of their tensors for the solver registered under `handle`: no adjoint state, backward
recomputes from the saved u, C and criterion.  The registry holds a solver weakly, so the autograd context keeps it alive
and registers it again before the backward op (`_stress_autograd` of `diffhe.elastic_stress`).

Not implemented: strength ratios / reserve factors; maximum-stress and Puck-type non-smooth criteria; eigenstrains,
vibration modes and shape gradients with a tensor; moving nodes and backward with create_graph=True
(NotImplementedError).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _hip
from .elastic_aniso import (_from_blocks, _nv_of, _stiffness_device, _stiffness_layout, _t64, components, matrix,
                            voigt_pairs)
from .elastic_stress import _StressCall, _stress_autograd, _stress_batch, _stress_fake, _stress_outputs
from .plan import padded_batch, _stream
from .solver import (K_ELEM, K_SAMPLE, K_SAMPLE_ELEM, K_SCALAR, _Engine, _SOLVERS, _fake_grads, _kappa_layout,
                     _like_grads, _tensor_mode)

__all__ = ("tsai_wu", "tsai_hill", "quadratic", "split", "von_mises_criterion", "rotated_criterion")


# ---------------------------------------------------------------------------------------------
# Criterion helpers (plain differentiable torch; no device, no library).  Every one returns (..., nk).
# ---------------------------------------------------------------------------------------------
def _nv_of_criterion(nk: int) -> int:
    if nk not in (9, 27):
        raise ValueError(f"expected 9 (2D) or 27 (3D) criterion components in the last dimension, got {nk}")
    return 3 if nk == 9 else 6


def quadratic(q, Q) -> torch.Tensor:
    """(..., nk) components of the criterion phi = q . sigma + sigma . Q sigma from q (..., nv) and the matrix Q
    (..., nv, nv) (its symmetric part counts); q and Q broadcast."""
    q, Q = _t64(q), _t64(Q)
    nv = q.shape[-1] if q.dim() else 0
    if nv not in (3, 6) or Q.dim() < 2 or tuple(Q.shape[-2:]) != (nv, nv):
        raise ValueError(f"quadratic: expected q (..., nv) and Q (..., nv, nv) with nv = 3 or 6, got {tuple(q.shape)} and "
                         f"{tuple(Q.shape)}")
    if q.device != Q.device:
        q, Q = (q.to(Q.device), Q) if q.device.type == "cpu" else (q, Q.to(q.device))
    Qc = components(Q)
    lead = torch.broadcast_shapes(q.shape[:-1], Qc.shape[:-1])
    return torch.cat([q.expand(*lead, nv), Qc.expand(*lead, Qc.shape[-1])], dim=-1)


def split(criterion) -> Tuple[torch.Tensor, torch.Tensor]:
    """(..., nk) components -> (q (..., nv), Q (..., nv, nv) symmetric): the inverse of `quadratic`."""
    criterion = _t64(criterion)
    nv = _nv_of_criterion(criterion.shape[-1] if criterion.dim() else 0)
    return criterion[..., :nv], matrix(criterion[..., nv:])


def _voigt_rotation(R: torch.Tensor, nv: int) -> torch.Tensor:
    """M (..., nv, nv) with (R^T sigma R)_I = sum_J M_IJ sigma_J on Voigt vectors whose shear entries are tensor components:
    a shear entry J = (a, b) stands for sigma_ab and sigma_ba."""
    pairs = voigt_pairs(nv)
    pi, pj = (torch.tensor(v, device=R.device) for v in zip(*pairs))
    at = lambda rows, cols: R[..., rows[None, :], cols[:, None]]      # noqa: E731  [I, J] -> R[rows_J, cols_I]
    shear = (pi != pj).to(R.dtype)[None, :]
    return at(pi, pi) * at(pj, pj) + shear * at(pj, pi) * at(pi, pj)


def rotated_criterion(criterion, R) -> torch.Tensor:
    """(..., nk) components of the criterion of a material turned by R: phi'(sigma) = phi(R^T sigma R) on the stress
    tensor.  The conventions of `rotated`: in 2D R is the angle theta (the material's first axis points along
    (cos theta, sin theta)), in 3D a rotation matrix (..., 3, 3) whose columns are the material's axes.  The criterion and
    R broadcast; differentiable in both."""
    criterion = _t64(criterion)
    nv = _nv_of_criterion(criterion.shape[-1] if criterion.dim() else 0)
    R = _t64(R)
    if criterion.device != R.device:    # helpers build criteria on the CPU from Python numbers: they follow an angle field
        criterion, R = (criterion.to(R.device), R) if criterion.device.type == "cpu" else (criterion, R.to(criterion.device))
    if nv == 3:
        c, s = torch.cos(R), torch.sin(R)
        R = torch.stack([torch.stack([c, -s], dim=-1), torch.stack([s, c], dim=-1)], dim=-2)
    elif R.dim() < 2 or tuple(R.shape[-2:]) != (3, 3):
        raise ValueError(f"rotated_criterion: a 3D criterion takes a rotation matrix (..., 3, 3), got {tuple(R.shape)}")
    q, Q = split(criterion)
    M = _voigt_rotation(R, nv)
    return quadratic(torch.einsum("...ij,...i->...j", M, q), torch.einsum("...ia,...ij,...jb->...ab", M, Q, M))


def _material_axes(q, normal, shear) -> torch.Tensor:
    """The criterion with the linear terms q (a list of nv broadcastable entries) and Q of `_from_blocks(normal, shear)`."""
    Qc = _from_blocks(normal, shear)
    lead = torch.broadcast_shapes(Qc.shape[:-1], *[_t64(v).shape for v in q])
    qv = torch.stack([_t64(v).to(Qc.device, Qc.dtype).expand(lead) for v in q], dim=-1)
    return torch.cat([qv, Qc.expand(*lead, Qc.shape[-1])], dim=-1)


def tsai_wu(Xt, Xc, Yt, Yc, S, theta=0.0, f12=-0.5) -> torch.Tensor:
    """(..., 9) components of the Tsai-Wu criterion of a 2D ply with the fibres at the angle theta to the x axis: tensile
    and compressive strengths Xt, Xc along the fibres and Yt, Yc across (all positive), shear strength S, interaction
    F12 = f12 sqrt(F11 F22).  In the material axes phi = F1 s1 + F2 s2 + F11 s1^2 + F22 s2^2 + F66 t12^2 + 2 F12 s1 s2
    with F1 = 1/Xt - 1/Xc, F2 = 1/Yt - 1/Yc, F11 = 1/(Xt Xc), F22 = 1/(Yt Yc), F66 = 1/S^2.  The arguments broadcast and
    are differentiable."""
    Xt, Xc, Yt, Yc, S, f12 = (_t64(v) for v in (Xt, Xc, Yt, Yc, S, f12))
    F11, F22 = 1.0 / (Xt * Xc), 1.0 / (Yt * Yc)
    F12 = f12 * torch.sqrt(F11 * F22)
    crit = _material_axes([1.0 / Xt - 1.0 / Xc, 1.0 / Yt - 1.0 / Yc, 0.0], [[F11, F12], [F12, F22]], [1.0 / (S * S)])
    return rotated_criterion(crit, theta)


def tsai_hill(X, Y, S, theta=0.0) -> torch.Tensor:
    """(..., 9) components of the Tsai-Hill criterion of a 2D ply with the fibres at the angle theta: in the material axes
    phi = (s1 / X)^2 - s1 s2 / X^2 + (s2 / Y)^2 + (t12 / S)^2.  The arguments broadcast and are differentiable."""
    X, Y, S = (_t64(v) for v in (X, Y, S))
    x2 = 1.0 / (X * X)
    crit = _material_axes([0.0, 0.0, 0.0], [[x2, -0.5 * x2], [-0.5 * x2, 1.0 / (Y * Y)]], [1.0 / (S * S)])
    return rotated_criterion(crit, theta)


def von_mises_criterion(dim: int, plane: Optional[str] = None, nu=None, yield_stress=1.0) -> torch.Tensor:
    """(..., nk) components of (vm / yield_stress)^2 as a quadratic form of the stored stress components: 3D for dim = 3;
    for dim = 2 plane="stress" (the default: sigma_zz = 0) or plane="strain", which folds sigma_zz = nu (sigma_xx +
    sigma_yy) in and needs nu.  nu and yield_stress broadcast and are differentiable."""
    if dim not in (2, 3):
        raise ValueError(f"dim must be 2 or 3, got {dim!r}")
    if dim == 3 and plane is not None:
        raise ValueError("plane= applies to dim = 2 only")
    if dim == 2 and plane not in (None, "stress", "strain"):
        raise ValueError(f"Unknown plane: {plane!r} (\"stress\" or \"strain\")")
    if plane == "strain" and nu is None:
        raise ValueError("von_mises_criterion: plane=\"strain\" needs nu (sigma_zz = nu (sigma_xx + sigma_yy))")
    w = 1.0 / (_t64(yield_stress) * _t64(yield_stress))
    if plane == "strain":
        nu = _t64(nu)
        diag, off = (1.0 - nu + nu * nu) * w, (nu * nu - nu - 0.5) * w
    else:
        diag, off = w, -0.5 * w
    normal = [[diag if i == j else off for j in range(dim)] for i in range(dim)]
    return _material_axes([0.0] * (3 if dim == 2 else 6), normal, [3.0 * w] * (1 if dim == 2 else 3))


# ---------------------------------------------------------------------------------------------
# diffhe::elastic_aniso_stress / diffhe::elastic_aniso_stress_backward (csrc/elastic_aniso_stress.hip).  A pure function
# of (u, C, criterion) for the solver registered under `handle`; criterion: empty tensor = absent.
# ---------------------------------------------------------------------------------------------
def _criterion_layout(crit: torch.Tensor, nk: int, m: int, B_f: Optional[int], node_major: bool = False):
    """-> (mode, B, element-major) of one call: `_stiffness_layout` for a criterion of nk components."""
    try:
        _tensor_mode(crit, nk, m, B_f, node_major)
    except ValueError:
        raise ValueError(f"criterion shape {tuple(crit.shape)} not understood for a mesh with {m} elements: expected "
                         f"({nk},), ({m}, {nk}), (B, {nk}) or (B, {m}, {nk}) components (q, then the upper triangle of Q)"
                         + (f", or ({nk}, {m}, B) with layout='node'" if node_major else "")) from None
    return _kappa_layout(crit, m, B_f, node_major, nk)


def _layouts(solver, u, C, crit, node_major):
    """-> (batch of u or None, B, (mode, em) of C, (mode, em) of the criterion or None).  The batch is u's; an unbatched u
    takes the batch that C or the criterion shows."""
    m, nt, nk = solver.mesh.n_elements, solver.nt, solver.nv + solver.nt
    B_u = B0 = _stress_batch(u, node_major)
    if B0 is None:
        for t, nc, layout in ((C, nt, _stiffness_layout), (crit, nk, _criterion_layout)):
            if t is not None and B0 is None:
                layout(t, nc, m, None)                                       # the shape refusal, under its own name
                B0 = _tensor_mode(t, nc, m, None)[1]
    mode_c, B, em_c = _stiffness_layout(C, nt, m, B0, node_major)
    of_k = None
    if crit is not None:
        mode_k, B_k, em_k = _criterion_layout(crit, nk, m, B0, node_major)
        if B_k != B:
            raise ValueError(f"criterion batch {B_k} does not match the batch {B} of u and C")
        of_k = (mode_k, em_k)
    return B_u, B, (mode_c, em_c), of_k


def _shapes(solver, u, C, crit, node_major):
    """-> (shape of sigma, shape of phi) for u, C and the criterion as the op gets them: those of `_stress_shapes`."""
    m, nv = solver.mesh.n_elements, solver.nv
    B_u, B, _, _ = _layouts(solver, u, C, crit, node_major)
    if node_major:
        return (m, nv, B), (m, B)
    return ((B, m, nv), (B, m)) if (B_u is not None or B > 1) else ((m, nv), (m,))


def _aniso_stress_call(solver, u, C, crit, node_major):
    """-> (`_StressCall` whose mode / em are those of C and whose head is the leading arguments of the three entries,
    (mode, em) of the criterion or None)."""
    plan = solver._plan()
    d, n, nv, nt = plan.dim, plan.n, solver.nv, solver.nt
    B_u, B, (mode_c, em_c), of_k = _layouts(solver, u, C, crit, node_major)
    Bp = padded_batch(B)
    eng = _Engine(plan, 0.0, 0, 0, "gather")
    call = _StressCall(plan, eng, B, Bp, mode_c, em_c, B_u is not None, node_major, (), nv)
    udev = call.rows_in(u, n * d, call.batched)
    cdev, csc, cse, csb, _ = _stiffness_device(eng, C, mode_c, B, Bp, nt, em_c)
    kdev, ksc, kse, ksb = None, 0, 0, 0
    if crit is not None:
        kdev, ksc, kse, ksb, _ = eng.tensor_device(crit, of_k[0], B, Bp, nv + nt, of_k[1])
    gtab = plan.oriented_gradient_table()                        # the stress is linear in grad phi: its sign counts
    call.head = (plan.elems, gtab, d, udev, cdev, csc, cse, csb, kdev, ksc, kse, ksb)
    return call, of_k


def _aniso_stress_forward(solver, u, C, crit, node_major, want_sigma, want_phi):
    """(sigma, phi) in the caller's layout, None for the one not asked for: the kernel writes (m, nv, Bp) and (m, Bp)."""
    call, _ = _aniso_stress_call(solver, u, C, crit, node_major)
    plan, m, nv, Bp = call.plan, call.plan.m, call.nc, call.Bp
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=plan.device)  # noqa: E731
    sigma, phi = (new(m * nv, Bp) if want_sigma else None), (new(m, Bp) if want_phi else None)
    _hip.lib().diffhe_elastc_stress_eval(*call.head, plan.n, m, Bp, sigma, Bp, nv * Bp, phi, _stream(plan.device))
    s_shape, p_shape = _shapes(solver, u, C, crit, node_major)
    if sigma is not None:
        sigma = call.rows_out(sigma, m * nv).reshape(s_shape).to(u.device)
    if phi is not None:
        phi = call.rows_out(phi, m).reshape(p_shape).to(u.device)
    return sigma, phi


def _tensor_grad(mode: int, shape, sums, per_elem) -> torch.Tensor:
    """What `_Engine.element_grad` returns for a tensor of nc components, in the shape of the caller's tensor: the sums
    over the elements (nc, B), or the per-element gradient (m, nc) | (nc, m, B) | (B, m * nc)."""
    if mode == K_SCALAR:
        return sums.sum(dim=1).reshape(shape)
    if mode == K_SAMPLE:
        return sums.t().reshape(shape)
    return per_elem.reshape(shape)


def _aniso_stress_adjoint(solver, sigma_bar, phi_bar, u, C, crit, node_major, need_u, need_c, need_k):
    """(dL/du, dL/dC, dL/d criterion) in the shapes of u, C and the criterion, None for those not asked for.  dC and the
    criterion's gradient are launches of their own, each in the layout of its tensor; the element pass of dC feeds the
    node pass too where the dC of the call is per sample."""
    call, of_k = _aniso_stress_call(solver, u, C, crit, node_major)
    plan, eng, nv, B, Bp = call.plan, call.eng, call.nc, call.B, call.Bp
    d, n, m, nt = plan.dim, plan.n, plan.m, solver.nt
    L, st = _hip.lib(), _stream(plan.device)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=plan.device)  # noqa: E731
    sb = call.rows_in(sigma_bar, m * nv, True) if sigma_bar is not None else None
    pb = call.rows_in(phi_bar, m, True) if phi_bar is not None else None
    head = (*call.head, sb, Bp, nv * Bp, pb)
    ubar = new(n * d, Bp) if need_u else None
    none = (None, 0, 0, None, None)

    def adjoint(nodes, of_c=none, of_k=none):
        lists = plan.shape_incidence() if nodes else (None, None)
        L.diffhe_elastc_stress_adjoint(*head, *lists, n, m, B, Bp, new(nv, m, Bp) if nodes else None,
                                       ubar if nodes else None, *of_c, *of_k, st)

    grad_u = grad_c = grad_k = None
    fused = need_u and need_c and call.mode != K_ELEM
    if need_c:
        sums, dc = eng.element_grad(
            call.mode, call.em, B, Bp, nt,
            lambda dc_e, osc, ose, part, total: adjoint(fused, of_c=(dc_e, osc, ose, part, total)),
            lambda dc, osc, ose: L.diffhe_elastc_stress_adjoint_shared(*head, n, m, B, Bp, dc, osc, ose, None, 0, 0, st))
        grad_c = _tensor_grad(call.mode, C.shape, sums, dc).to(C.device)
    if need_k and phi_bar is not None:
        sums, dk = eng.element_grad(
            of_k[0], of_k[1], B, Bp, nv + nt,
            lambda dk_e, osc, ose, part, total: adjoint(False, of_k=(dk_e, osc, ose, part, total)),
            lambda dk, osc, ose: L.diffhe_elastc_stress_adjoint_shared(*head, n, m, B, Bp, None, 0, 0, dk, osc, ose, st))
        grad_k = _tensor_grad(of_k[0], crit.shape, sums, dk).to(crit.device)
    elif need_k:                                                   # sigma alone does not read the criterion
        grad_k = torch.zeros_like(crit)
    if need_u:
        if not fused:
            adjoint(True)
        du = call.rows_out(ubar, n * d)
        if node_major:
            grad_u = du.reshape(n, d, B)
        else:
            du = du.reshape(B, n, d)
            grad_u = du if call.batched else du.sum(dim=0)
        grad_u = grad_u.to(u.device)
    return grad_u, grad_c, grad_k


def _given(crit: torch.Tensor) -> Optional[torch.Tensor]:
    return crit if crit.numel() else None


@torch.library.custom_op("diffhe::elastic_aniso_stress", mutates_args=())
def elastic_aniso_stress(u: torch.Tensor, C: torch.Tensor, crit: torch.Tensor, handle: int, node_major: bool,
                         want_sigma: bool, want_phi: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sigma, phi) of the displacement u, the stiffness C and the criterion (empty: none, no phi) for the
    `AnisotropicElasticFESolver` registered under `handle`; the output not asked for comes back empty."""
    return _stress_outputs(u, *_aniso_stress_forward(_SOLVERS[handle], u, C, _given(crit), node_major, want_sigma,
                                                     want_phi))


@elastic_aniso_stress.register_fake
def _elastic_aniso_stress_fake(u, C, crit, handle, node_major, want_sigma, want_phi):
    return _stress_fake(u, _shapes(_SOLVERS[handle], u, C, _given(crit), node_major), want_sigma, want_phi)


@torch.library.custom_op("diffhe::elastic_aniso_stress_backward", mutates_args=())
def elastic_aniso_stress_backward(sigma_bar: torch.Tensor, phi_bar: torch.Tensor, u: torch.Tensor, C: torch.Tensor,
                                  crit: torch.Tensor, handle: int, node_major: bool, need_u: bool, need_c: bool,
                                  need_k: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dL/du, dL/dC, dL/d criterion) of `elastic_aniso_stress` for the cotangents of sigma and phi (empty = absent);
    unused ones come back empty."""
    grads = _aniso_stress_adjoint(_SOLVERS[handle], sigma_bar if sigma_bar.numel() else None,
                                  phi_bar if phi_bar.numel() else None, u, C, _given(crit), node_major, need_u, need_c,
                                  need_k and crit.numel() > 0)
    return _like_grads(u, grads, (u, C, crit))


@elastic_aniso_stress_backward.register_fake
def _elastic_aniso_stress_backward_fake(sigma_bar, phi_bar, u, C, crit, handle, node_major, need_u, need_c, need_k):
    return _fake_grads(u, (need_u, need_c, need_k), (u, C, crit))


_REFUSAL = ("diffhe: second-order derivatives of an anisotropic stress evaluation are not implemented (backward with "
            "create_graph=True, diffhe.elastic_aniso_stress)")
_setup_context, _backward = _stress_autograd("elastic_aniso_stress", 3, 7, _REFUSAL)


def _evaluate(solver, u, criterion, C, layout: str, want_sigma: bool, want_phi: bool):
    """The checks of the three public methods of `AnisotropicElasticFESolver`, then the op: (sigma, phi)."""
    n, d, m = solver.mesh.n_nodes, solver.mesh.dim, solver.mesh.n_elements
    if layout not in ("sample", "node"):
        raise ValueError(f"Unknown layout: {layout!r}")
    u = u if isinstance(u, torch.Tensor) else torch.as_tensor(u)
    if layout == "node":
        if u.dim() != 3 or tuple(u.shape[:2]) != (n, d):
            raise ValueError(f"layout='node': u must be (n, d, B) with n={n}, d={d}, got {tuple(u.shape)}")
    elif u.dim() not in (2, 3) or tuple(u.shape[-2:]) != (n, d):
        raise ValueError(f"u must be (n, d) or (B, n, d) with n={n}, d={d}, got {tuple(u.shape)}")
    C = solver.C if C is None else _t64(C)
    if want_phi:
        if criterion is None:
            raise ValueError("failure_index needs a criterion: (nk,) components, q first, then the upper triangle of Q "
                             "(diffhe.tsai_wu, tsai_hill, von_mises_criterion, quadratic)")
        criterion = _t64(criterion).to(torch.float64)
    solver._refuse_moving_nodes("stress", False)
    u, C, node = u.to(torch.float64), C.to(torch.float64), layout == "node"
    _layouts(solver, u, C, criterion if want_phi else None, node)          # the refusals, before the op
    _SOLVERS[id(solver)] = solver
    crit = criterion if want_phi else u.new_empty(0)
    return torch.ops.diffhe.elastic_aniso_stress(u, C, crit, id(solver), node, want_sigma, want_phi)
