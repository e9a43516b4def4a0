"""Solves with an anisotropic conductivity tensor per element (ours: the reference's kappa is a scalar).

`AnisotropicFESolver` solves -div(K grad u) + c u = f on P1 triangles and P1 tetrahedra with a symmetric positive-definite
tensor K instead of the scalar kappa of `DifferentiableFESolver3D`, whose constructor options and
`forward(f, load=None, layout=...)` it keeps.  The element stiffness is K_e[p, q] = |e| grad phi_p^T K_e grad phi_q and

    dL/dK_e = -|e| sym(grad lambda (x) grad u)

comes from the same single adjoint solve as dL/df and dL/dload (csrc/aniso.hip: a gradient table, a row-gather tensor
assembly, the gradient kernels; no floating-point atomics, results bitwise reproducible).

Convention.  K is given in Voigt components: nc = 3 in 2D ordered (xx, yy, xy), nc = 6 in 3D ordered
(xx, yy, zz, yz, xz, xy).  An off-diagonal component is ONE parameter that fills both symmetric entries, so dL/dK_xy is
the derivative with respect to that parameter (the sum of the derivatives with respect to the two entries): what
autograd gives for a dense matrix built by `full`.  The helpers here (`voigt`, `full`, `rotated`,
`transverse_isotropic`) are plain differentiable torch: gradients flow on to angles, directions and principal
conductivities by ordinary autograd.

Layouts of the tensor (any of them may require grad; its gradient has its shape):
  (nc,)        one tensor for the whole mesh and batch (ONE matrix is stored for the batch)
  (B, nc)      one tensor per sample
  (m, nc)      a field shared by the batch -- its gradient is summed over the batch inside the kernel, in a fixed order
  (B, m, nc)   a field per sample; with layout="node" also (nc, m, B), batch innermost like f and u, and the gradient
               comes back in that layout
When B == m the shapes (B, nc) and (m, nc) coincide.  They are resolved like the scalar (m,) / (B,) of
`solver._kappa_mode`: an (m, nc) tensor is the element field, except when f itself carries a batch of exactly m samples;
then it is one tensor per sample.  Pass the (B, m, nc) form to say what you mean.

Every tensor solve takes the general path (ELL operator, aggregation-multigrid PCG; `method="ell-jacobi"` for plain
Jacobi), also on `FEMesh.rectangle` connectivity; `reaction=`, `load=`, non-zero Dirichlet values of the mesh,
`layout="node"` and batch padding work as in the base class.  On 3D meshes the solve plan keeps the couplings that are
exact zeros for every scalar kappa (a tensor fills them), next to the pruned plan scalar solves on the same mesh use.
By default the aggregation hierarchy is built from the unit operator and does not see the tensor: iteration counts grow
with the anisotropy.  `amg=dict(strength=0.25)` builds it from the operator being solved instead -- aggregates along the
strong couplings, a per-level eigenvalue bound for the smoother, kept on the solver (`refresh_hierarchy()`,
`amg["refresh"]`): 101 instead of more than 20000 iterations at ratio 100 on a 512^2 mesh (DESIGN section 7,
"Coefficient-aware hierarchy").  `validate=True` checks that every tensor is positive definite (ValueError; one device
synchronisation per call); without it an indefinite tensor shows up as the non-convergence warning.

Not implemented (NotImplementedError): `dirichlet=` (the band kernels of csrc/bc.hip read scalar tables); backward with
create_graph=True; P2 meshes; 1D meshes (a tensor is meaningless there); a class that combines this solver with
`ShapeDifferentiableFESolver`.  `diffhe.heat.HeatEquation` takes scalar-kappa solvers only.
"""
from __future__ import annotations

from typing import Optional

import torch

from .solver import K_SAMPLE_ELEM, _tensor_mode
from .tet3d import DifferentiableFESolver3D

__all__ = ("AnisotropicFESolver", "voigt", "full", "rotated", "transverse_isotropic")

_PAIRS = {3: ((0, 0), (1, 1), (0, 1)), 6: ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))}


def voigt(K: torch.Tensor) -> torch.Tensor:
    """(..., d, d) symmetric tensors -> (..., nc) Voigt components, d = 2 or 3 (an off-diagonal component is the mean
    of the two entries: the entry itself when K is symmetric)."""
    d = K.shape[-1]
    if K.dim() < 2 or K.shape[-2] != d or d not in (2, 3):
        raise ValueError(f"voigt: expected (..., 2, 2) or (..., 3, 3), got {tuple(K.shape)}")
    return torch.stack([K[..., i, j] if i == j else 0.5 * (K[..., i, j] + K[..., j, i])
                        for i, j in _PAIRS[d * (d + 1) // 2]], dim=-1)


def full(kv: torch.Tensor) -> torch.Tensor:
    """(..., nc) Voigt components -> (..., d, d) symmetric tensors, nc = 3 or 6."""
    nc = kv.shape[-1] if kv.dim() else 0
    if nc not in _PAIRS:
        raise ValueError(f"full: expected (..., 3) or (..., 6) Voigt components, got {tuple(kv.shape)}")
    d = 2 if nc == 3 else 3
    index = [[0] * d for _ in range(d)]
    for c, (i, j) in enumerate(_PAIRS[nc]):
        index[i][j] = index[j][i] = c
    return torch.stack([torch.stack([kv[..., index[i][j]] for j in range(d)], dim=-1) for i in range(d)], dim=-2)


def rotated(k_par, k_perp, theta) -> torch.Tensor:
    """(..., 3) Voigt components of the 2D tensor with conductivity k_par along the fibre direction (cos theta,
    sin theta) and k_perp across it: K = k_perp I + (k_par - k_perp) a a^T.  The arguments broadcast."""
    k_par, k_perp, theta = (torch.as_tensor(v, dtype=torch.float64) if not isinstance(v, torch.Tensor) else v
                            for v in (k_par, k_perp, theta))
    c, s = torch.cos(theta), torch.sin(theta)
    dk = k_par - k_perp
    return torch.stack(torch.broadcast_tensors(k_perp + dk * c * c, k_perp + dk * s * s, dk * c * s), dim=-1)


def transverse_isotropic(k_par, k_perp, direction: torch.Tensor) -> torch.Tensor:
    """(..., 6) Voigt components of the 3D tensor with conductivity k_par along `direction` (..., 3) -- normalised
    here -- and k_perp in the plane across it: K = k_perp I + (k_par - k_perp) a a^T."""
    k_par, k_perp = (torch.as_tensor(v, dtype=torch.float64) if not isinstance(v, torch.Tensor) else v
                     for v in (k_par, k_perp))
    if direction.shape[-1] != 3:
        raise ValueError(f"transverse_isotropic: direction must be (..., 3), got {tuple(direction.shape)}")
    a = direction / direction.norm(dim=-1, keepdim=True)
    dk = k_par - k_perp
    comps = [(k_perp if i == j else 0.0) + dk * a[..., i] * a[..., j] for i, j in _PAIRS[6]]
    return torch.stack(torch.broadcast_tensors(*comps), dim=-1)


def _positive_definite(kv: torch.Tensor, axis: int) -> torch.Tensor:
    """0-dim bool tensor: every tensor of `kv` (Voigt components along `axis`) is finite and positive definite
    (Sylvester's criterion on the leading minors)."""
    k = kv.detach().movedim(axis, -1)
    if k.shape[-1] == 3:
        xx, yy, xy = k.unbind(-1)
        minors = (xx, xx * yy - xy * xy, yy)
    else:
        xx, yy, zz, yz, xz, xy = k.unbind(-1)
        minors = (xx, xx * yy - xy * xy,
                  xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz))
    ok = torch.isfinite(k).all()
    for v in minors:
        ok = ok & (v > 0).all()         # NaN compares false
    return ok


class AnisotropicFESolver(DifferentiableFESolver3D):
    """`DifferentiableFESolver3D` with a symmetric positive-definite conductivity tensor in Voigt components as its
    coefficient (see the module docstring): P1 triangles and P1 tetrahedra, general path."""

    _dims = (2, 3)

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        from .shape import ShapeDifferentiableFESolver
        if issubclass(cls, ShapeDifferentiableFESolver):
            raise NotImplementedError("diffhe: node gradients (ShapeDifferentiableFESolver) together with a conductivity "
                                      "tensor are not implemented")

    def __init__(self, mesh, kappa: Optional[torch.Tensor] = None, *, validate: bool = False, **options):
        if mesh.dim == 1:
            raise NotImplementedError("diffhe: a conductivity tensor needs a 2D or 3D mesh (1D: use the scalar kappa of "
                                      "DifferentiableFESolver)")
        if mesh.dim not in (2, 3):
            raise NotImplementedError("Only 2D and 3D supported")
        if mesh.elements.shape[1] != mesh.dim + 1:
            raise NotImplementedError("diffhe: a conductivity tensor is implemented for P1 elements only (this mesh has "
                                      f"{mesh.elements.shape[1]} nodes per element)")
        nc = 3 if mesh.dim == 2 else 6
        if kappa is None:
            kappa = torch.tensor([1.0] * mesh.dim + [0.0] * (nc - mesh.dim), dtype=torch.float64)
        if not isinstance(kappa, torch.Tensor):
            kappa = torch.as_tensor(kappa, dtype=torch.float64)
        if kappa.dim() != 3:        # a per-sample field is checked against the batch of f at the first solve
            _tensor_mode(kappa, nc, mesh.n_elements, None)
        super().__init__(mesh, kappa, **options)
        self._nc = nc
        self.validate = bool(validate)

    def _tensor_components(self) -> int:
        return self._nc

    def _plan(self):
        from .plan import get_plan
        from .solver import _resolve_device
        return get_plan(self.mesh, _resolve_device(self._device), prune=False)

    def forward(self, f: torch.Tensor, load: Optional[torch.Tensor] = None, layout: str = "sample",
                dirichlet: Optional[torch.Tensor] = None) -> torch.Tensor:
        """As `DifferentiableFESolver.forward`, without `dirichlet=` (NotImplementedError)."""
        if dirichlet is not None:
            raise NotImplementedError("diffhe: dirichlet= together with a conductivity tensor is not implemented (the "
                                      "boundary-band kernels read scalar element tables); put the values into the mesh")
        if self.validate and layout in ("sample", "node"):
            node_major = layout == "node"
            B_f = (f.shape[1] if node_major else f.shape[0]) if f.dim() == 2 and tuple(f.shape) != (self.mesh.n_nodes, 1) \
                else None
            mode, _, em = _tensor_mode(self._kappa, self._nc, self.mesh.n_elements, B_f, node_major)
            if not bool(_positive_definite(self._kappa, 0 if (mode == K_SAMPLE_ELEM and em) else -1)):
                raise ValueError("diffhe: the conductivity tensor is not symmetric positive definite everywhere "
                                 "(validate=True)")
        return super().forward(f, load, layout)
