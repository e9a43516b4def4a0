"""Solves differentiable with respect to per-sample Dirichlet values (ours: the reference reads one dict of boundary
values per mesh and carries no gradient to it, although its README promises optimisation of boundary conditions).

`DifferentiableFESolver.forward(f, load=None, layout="sample", dirichlet=G)` -- inherited by `DifferentiableFESolver3D`
and `ShapeDifferentiableFESolver` -- takes the Dirichlet values G in ascending node-id order (`FEMesh.dirichlet_index()`),
(n_D,) for the batch or (B, n_D) per sample ((n_D,) or (n_D, B) with layout="node").  The keys of `mesh.dirichlet_nodes`
still say which nodes are Dirichlet nodes, its values are not used: the solve plan (which depends only on the nodes, the
elements and that SET) is the same for every G.  G is the `dirichlet` input of the custom op `diffhe::fe_solve`.  With F
the free and D the Dirichlet nodes and K_b the unreduced stiffness of sample b:

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
G together with node gradients (mesh.nodes requiring grad in ShapeDifferentiableFESolver).  `dirichlet=None` takes none
of this: the paths read the mesh's own values.
"""
from __future__ import annotations

import torch

from . import solver as _solver
from .solver import K_ELEM, K_SAMPLE, K_SAMPLE_ELEM, K_SCALAR

__all__ = ("band_grads",)


def band_grads(state, g, lam, dk_sample, dk_elem, need_k: bool, need_g: bool):
    """The band step of `diffhe.solver._solve_backward` for a solve with per-call Dirichlet data, after the path's
    adjoint (cotangent `g` and `lam`, dk_* as `state.adjoint` took and returned them): dL/dG, and the G part of
    dL/dkappa on the node-major paths (the chain's u already holds G) -- added to `dk_elem` in place.
    Returns (dk_sample with its G part, per-sample dL/dG in the layout of G or None)."""
    call, plan, eng = state.call, state.plan, state.eng
    B = call.B
    _u, lam_f, lsn, lsb, _g = state.shape_fields(lam)          # lambda (0 on D) and its strides, either layout
    chain = isinstance(state, _solver._ChainSolve)
    scalar_k = need_k and not chain and call.mode in (K_SCALAR, K_SAMPLE)
    gG = None
    if need_g or scalar_k:
        nd = plan.n_bc
        out = torch.empty((nd, B) if call.node_major else (B, nd), dtype=torch.float64, device=plan.device)
        osj, osb = (B, 1) if call.node_major else (1, nd)
        dots = torch.empty((nd, B), dtype=torch.float64, device=plan.device) if scalar_k else None
        eng.bc_grad(call.kappa_s, lam_f, lsn, lsb, g, g.stride(0 if call.node_major else 1),
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
    return dk_sample, gG
