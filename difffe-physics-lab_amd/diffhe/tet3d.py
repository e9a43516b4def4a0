"""Differentiable P1 solves on 3D tetrahedral meshes (ours: the reference stops at 2D, solver.py:67).

`DifferentiableFESolver3D` is `DifferentiableFESolver` with the dimension gate lifted: same constructor, `.kappa`,
`forward(f, load=None, layout=...)`, options, kappa layouts and gradients; on 1D and 2D meshes it behaves exactly like
the base class, which stays the faithful mirror of the reference (it keeps refusing 3D meshes).  A 3D mesh -- P1
tetrahedra, `FEMesh.box` or any (n, 3) nodes with (m, 4) elements -- takes the general path: the element integrals of
`tet_integrals` (csrc/ell_assemble.hip), the deterministic gather assembly into an ELL pattern from which structurally zero
couplings are pruned (diffhe/plan.py), and the aggregation-multigrid PCG with its explicit adjoint.

Element convention (the reference has none to copy in 3D): stiffness k_pq = kappa g_p . g_q / (36 V) with the cofactor
vectors g_p = 6 V grad phi_p; load F_p += V/4 * mean of the four vertex values of f (m0 = V/16 for every pair, the 2D
rule area/3 * mean(f) lifted); tetrahedra with 6 V <= 1e-12 l^3 (l the longest edge from the first vertex) are
degenerate and contribute nothing.  `reaction=` uses the lumped mass V/4 per vertex.
"""
from __future__ import annotations

from .solver import DifferentiableFESolver

__all__ = ("DifferentiableFESolver3D",)


class DifferentiableFESolver3D(DifferentiableFESolver):
    """`DifferentiableFESolver` that also accepts 3D meshes of P1 tetrahedra (see the module docstring)."""

    _dims = (1, 2, 3)
