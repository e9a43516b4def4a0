"""Anisotropic linear elasticity: a stiffness tensor per element and sample with dL/dC (ours: the reference solves scalar
equations only).

`AnisotropicElasticFESolver(mesh, C)` is `ElasticFESolver` with a symmetric positive-definite stiffness matrix per element
and sample in place of `(E, nu, plane)`: it solves -div sigma(u) = f, sigma = C eps(u), on P1 triangles (d = 2) and P1
tetrahedra (d = 3), with the same `forward(f, load, layout=)`, `fixed=`, `tol`, `max_iter`, `method`, `amg` cycle options
and `last_info`; dL/dC, dL/df and dL/dload come from ONE adjoint solve.  Fibre angles of laminates, orthotropic and cubic
materials, homogenised cells, and gradients with respect to Poisson's ratio all go through C.

Convention.
  Strain order   the Voigt order of `diffhe.aniso`: (xx, yy, xy) in 2D, nv = 3; (xx, yy, zz, yz, xz, xy) in 3D, nv = 6.
  Shear          shear strains are ENGINEERING strains gamma = 2 eps, so C is the ordinary engineering stiffness matrix:
                 3 x 3 in 2D (the reduced plane-stress or plane-strain matrix is the caller's choice), 6 x 6 in 3D.
                 `isotropic(1, nu, 2, "stress")` is [[1, nu, 0], [nu, 1, 0], [0, 0, (1 - nu) / 2]] / (1 - nu^2).
  Components     C is passed as its upper triangle, row-major: nt = 6 components in 2D (11, 12, 13, 22, 23, 33), nt = 21
                 in 3D.  An off-diagonal component is ONE parameter that fills both symmetric entries -- the rule of
                 `diffhe.aniso` -- and its gradient is the derivative with respect to that parameter.
  Layouts        (nt,), (B, nt), (m, nt), (B, m, nt), and (nt, m, B) with layout="node"; resolved by the rule of
                 `AnisotropicFESolver` (`solver._tensor_mode`: an (m, nt) tensor is the element field unless f carries a
                 batch of exactly m samples).  Any of them may require grad, the gradient comes back in the shape of C; a
                 field the batch shares gets its gradient summed over the batch inside the kernel, in a fixed order.  The
                 (nt,) and (m, nt) layouts store ONE matrix for the batch.

The helpers `isotropic`, `orthotropic_2d`, `orthotropic_3d`, `cubic`, `rotated`, `matrix` and `components` are plain
differentiable torch: angles, moduli and nu are optimised by ordinary autograd through them.  All of them return
components (..., nt); `matrix` / `components` go between (..., nt) and (..., nv, nv).

Kernels: csrc/elastic_aniso.hip (include/diffhe_elastic_aniso.h), fp64, no atomics, bitwise reproducible: the block
row-gather assembly in the dof pattern of include/diffhe_elastic.h, dC_IJ[e] = -vol_e (eps_I(lambda) eps_J(u) +
[I != J] eps_J(lambda) eps_I(u)) per sample or summed over the batch, and the row bound below.

Hierarchy and smoother bounds.  The solver reuses the cached hierarchy of the isotropic unit operator (nu = 0.3, plane
stress in 2D, the solver's fixed set): the same plan entry an `ElasticFESolver` of those parameters on the same mesh uses.
That hierarchy's recorded Jacobi bounds hold for its own operator, not for an anisotropic one, so every call, after the
per-call Galerkin operators exist, runs `diffhe_ell_jacobi_row_bound` on every level -- the infinity norm of
D^-1/2 A D^-1/2, a rigorous bound of lambda_max(D^-1 A) -- copies the n_levels doubles to the host (ONE device
synchronisation per call) and overwrites the levels' bounds with them.  `last_info.jacobi_bounds` reports them,
`last_info.hierarchy` is "unit+row-bounds".  A diagonal that is not positive and finite makes the bound +inf: ValueError
("stiffness tensor not positive definite").  The adjoint reuses the forward's hierarchy.  `validate=True` checks C itself
with `torch.linalg.cholesky_ex` (one more synchronisation; ValueError).

Stress recovery: `tensor_stress`, `failure_index` and `tensor_stress_and_failure_index` (`diffhe.elastic_aniso_stress`)
give sigma = C eps(u) and a quadratic failure index per element and sample, differentiable in u, C and the criterion.

Not implemented (NotImplementedError): 1D and P2 meshes; backward with create_graph=True; `eigenstrain=`; `stress`,
`von_mises`, `stress_and_von_mises` (they read (E, nu); the stress of a tensor is `tensor_stress` / `failure_index`);
strength ratios and non-smooth (maximum-stress, Puck) criteria; moving nodes (mesh.nodes requiring grad, also for the
stress); vibration modes (`modes`: `ElasticEigenSolver` takes (E, nu) only); a per-call `dirichlet=`, Robin / flux data;
`amg=dict(strength=...)`.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from .elastic import (_ElasticOptions, _ElasticSolve, _batch_of, _check_mesh, _run_adjoint, _solve_autograd, _solve_call,
                      _solve_fake, _solve_result)
from .plan import _stream
from .solver import (K_SAMPLE, K_SAMPLE_ELEM, K_SCALAR, SolveInfo, _SOLVERS, _fake_grads, _kappa_layout, _like_grads,
                     _tensor_mode)

__all__ = ("AnisotropicElasticFESolver", "AnisoElasticInfo", "isotropic", "orthotropic_2d", "orthotropic_3d", "cubic",
           "rotated", "matrix", "components")

HIERARCHY_NU = 0.3      # the isotropic unit operator whose cached hierarchy the solver reuses


# ---------------------------------------------------------------------------------------------
# Helpers (plain differentiable torch; no device, no library)
# ---------------------------------------------------------------------------------------------
def voigt_pairs(nv: int) -> Tuple[Tuple[int, int], ...]:
    """The index pair of every Voigt component, in the order of `diffhe.aniso`."""
    if nv == 3:
        return ((0, 0), (1, 1), (0, 1))
    if nv == 6:
        return ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
    raise ValueError(f"nv must be 3 (2D) or 6 (3D), got {nv!r}")


def _nv_of(nt: int) -> int:
    if nt not in (6, 21):
        raise ValueError(f"expected 6 (2D) or 21 (3D) stiffness components in the last dimension, got {nt}")
    return 3 if nt == 6 else 6


def _t64(v) -> torch.Tensor:
    return v if isinstance(v, torch.Tensor) else torch.as_tensor(v, dtype=torch.float64)


def matrix(Cv: torch.Tensor) -> torch.Tensor:
    """(..., nt) components -> (..., nv, nv) symmetric matrices; an off-diagonal component fills both entries."""
    Cv = _t64(Cv)
    nv = _nv_of(Cv.shape[-1] if Cv.dim() else 0)
    index, c = [[0] * nv for _ in range(nv)], 0
    for i in range(nv):
        for j in range(i, nv):
            index[i][j] = index[j][i] = c
            c += 1
    return Cv[..., torch.tensor(index, device=Cv.device)]


def components(Cm: torch.Tensor) -> torch.Tensor:
    """(..., nv, nv) matrices -> (..., nt) components, the upper triangle row-major (an off-diagonal component is the
    mean of the two entries: the entry itself when the matrix is symmetric)."""
    Cm = _t64(Cm)
    nv = Cm.shape[-1] if Cm.dim() >= 2 else 0
    if nv not in (3, 6) or Cm.shape[-2] != nv:
        raise ValueError(f"components: expected (..., 3, 3) or (..., 6, 6), got {tuple(Cm.shape)}")
    return torch.stack([Cm[..., i, j] if i == j else 0.5 * (Cm[..., i, j] + Cm[..., j, i])
                        for i in range(nv) for j in range(i, nv)], dim=-1)


def _from_blocks(normal, shear) -> torch.Tensor:
    """Components of the matrix with the d x d block `normal` (rows of broadcastable entries) on the normal strains and
    the entries `shear` on the diagonal of the shear strains; no coupling between the two."""
    d, ns = len(normal), len(shear)
    nv = d + ns
    flat = [normal[i][j] if j < d else 0.0 for i in range(d) for j in range(i, nv)]
    flat += [shear[i] if j == i else 0.0 for i in range(ns) for j in range(i, ns)]
    ref = torch.broadcast_tensors(*[_t64(v) for v in flat if isinstance(v, torch.Tensor) or v != 0.0])[0]
    return torch.stack([_t64(v).to(ref.device, ref.dtype).expand(ref.shape) for v in flat], dim=-1)


def isotropic(E, nu, dim: int, plane: Optional[str] = None) -> torch.Tensor:
    """(..., nt) components of the isotropic stiffness with Young's modulus E and Poisson's ratio nu (both broadcast, both
    differentiable): 3D for dim = 3; for dim = 2 the reduced matrix of plane="stress" (the default) or "strain"."""
    E, nu = _t64(E), _t64(nu)
    if dim == 3 and plane is not None:
        raise ValueError("plane= applies to dim = 2 only")
    if dim == 2 and plane not in (None, "stress", "strain"):
        raise ValueError(f"Unknown plane: {plane!r} (\"stress\" or \"strain\")")
    if dim not in (2, 3):
        raise ValueError(f"dim must be 2 or 3, got {dim!r}")
    mu = E / (2.0 * (1.0 + nu))
    lam = E * nu / (1.0 - nu * nu) if (dim == 2 and plane != "strain") else E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    normal = [[lam + 2.0 * mu if i == j else lam for j in range(dim)] for i in range(dim)]
    return _from_blocks(normal, [mu] * (1 if dim == 2 else 3))


def rotated(C: torch.Tensor, R) -> torch.Tensor:
    """(..., nt) components of the stiffness C (..., nt) of a material turned by R: C'_ijkl = R_ia R_jb R_kc R_ld C_abcd.
    2D: R is the angle theta (the material's first axis points along (cos theta, sin theta)); 3D: a rotation matrix
    (..., 3, 3) whose columns are the material's axes.  C and R broadcast; differentiable in both."""
    C = _t64(C)
    nv = _nv_of(C.shape[-1] if C.dim() else 0)
    d = 2 if nv == 3 else 3
    R = _t64(R)
    if C.device != R.device:        # helpers build C on the CPU from Python numbers: it follows an angle field's device
        C, R = (C.to(R.device), R) if C.device.type == "cpu" else (C, R.to(C.device))
    if d == 2:
        c, s = torch.cos(R), torch.sin(R)
        R = torch.stack([torch.stack([c, -s], dim=-1), torch.stack([s, c], dim=-1)], dim=-2)
    elif R.dim() < 2 or tuple(R.shape[-2:]) != (3, 3):
        raise ValueError(f"rotated: a 3D stiffness takes a rotation matrix (..., 3, 3), got {tuple(R.shape)}")
    pairs = voigt_pairs(nv)
    V = [[0] * d for _ in range(d)]
    for I, (i, j) in enumerate(pairs):
        V[i][j] = V[j][i] = I
    V = torch.tensor(V, device=C.device)
    C4 = matrix(C)[..., V[:, :, None, None], V[None, None, :, :]]                  # (..., d, d, d, d)
    C4 = torch.einsum("...ia,...jb,...kc,...ld,...abcd->...ijkl", R, R, R, R, C4)
    pi, pj = (torch.tensor(v, device=C.device) for v in zip(*pairs))
    return components(C4[..., pi[:, None], pj[:, None], pi[None, :], pj[None, :]])


def orthotropic_2d(E1, E2, nu12, G12, theta=0.0) -> torch.Tensor:
    """(..., 6) components of the plane-stress stiffness of an orthotropic ply -- moduli E1 along the fibres and E2 across,
    major Poisson's ratio nu12 (nu21 = nu12 E2 / E1), shear modulus G12 -- with the fibres at the angle theta to the
    x axis.  The arguments broadcast and are differentiable."""
    E1, E2, nu12, G12 = (_t64(v) for v in (E1, E2, nu12, G12))
    den = 1.0 - nu12 * nu12 * E2 / E1
    q12 = nu12 * E2 / den
    return rotated(_from_blocks([[E1 / den, q12], [q12, E2 / den]], [G12]), theta)


def orthotropic_3d(E1, E2, E3, nu12, nu13, nu23, G23, G13, G12) -> torch.Tensor:
    """(..., 21) components of the orthotropic stiffness in its material axes: the inverse of the compliance with
    S_ii = 1 / E_i, S_12 = -nu12 / E1, S_13 = -nu13 / E1, S_23 = -nu23 / E2, and the shear moduli in the Voigt order
    (yz, xz, xy).  The arguments broadcast and are differentiable."""
    E1, E2, E3, nu12, nu13, nu23, G23, G13, G12 = torch.broadcast_tensors(
        *[_t64(v) for v in (E1, E2, E3, nu12, nu13, nu23, G23, G13, G12)])
    s12, s13, s23 = -nu12 / E1, -nu13 / E1, -nu23 / E2
    S = torch.stack([torch.stack([1.0 / E1, s12, s13], dim=-1), torch.stack([s12, 1.0 / E2, s23], dim=-1),
                     torch.stack([s13, s23, 1.0 / E3], dim=-1)], dim=-2)
    N = torch.linalg.inv(S)
    N = 0.5 * (N + N.transpose(-1, -2))
    return _from_blocks([[N[..., i, j] for j in range(3)] for i in range(3)], [G23, G13, G12])


def cubic(C11, C12, C44) -> torch.Tensor:
    """(..., 21) components of a cubic crystal's stiffness in its crystal axes.  The arguments broadcast."""
    C11, C12, C44 = (_t64(v) for v in (C11, C12, C44))
    return _from_blocks([[C11 if i == j else C12 for j in range(3)] for i in range(3)], [C44] * 3)


# ---------------------------------------------------------------------------------------------
# One call
# ---------------------------------------------------------------------------------------------
@dataclass
class AnisoElasticInfo(SolveInfo):
    """`SolveInfo` with the bound of lambda_max(D^-1 A) the call measured on every level of its hierarchy, the fine one
    first (empty: no hierarchy, method="ell-jacobi")."""
    jacobi_bounds: Tuple[float, ...] = ()


def _stiffness_layout(C: torch.Tensor, nt: int, m: int, B_f: Optional[int], node_major: bool = False):
    """-> (mode, B, element-major) of one call: `_kappa_layout` for a tensor of nt components."""
    try:
        _tensor_mode(C, nt, m, B_f, node_major)
    except ValueError:
        raise ValueError(f"stiffness tensor shape {tuple(C.shape)} not understood for a mesh with {m} elements: expected "
                         f"({nt},), ({m}, {nt}), (B, {nt}) or (B, {m}, {nt}) upper-triangle components"
                         + (f", or ({nt}, {m}, B) with layout='node'" if node_major else "")) from None
    return _kappa_layout(C, m, B_f, node_major, nt)


def _stiffness_device(eng, C: torch.Tensor, mode: int, B: int, Bp: int, nt: int, em: bool):
    """-> (tensor, stride per component, per element, per sample, Bv) as the kernels of csrc/elastic_aniso.hip index it:
    `_Engine.tensor_device` for nt components -- batch-shared tensors as they come, per-sample ones batch-innermost, so
    that the nt loads per element are coalesced.  It pads the batch for a conductivity (ones on the first d components);
    here the padding samples, which are a copy's whenever there are any, get the identity matrix."""
    cdev, csc, cse, csb, Bv = eng.tensor_device(C, mode, B, Bp, nt, em)
    if Bv > 1 and Bp > B:
        eye = components(torch.eye(_nv_of(nt), dtype=torch.float64, device=cdev.device))
        pad = torch.as_strided(cdev, (nt, eng.p.m if cse else 1, Bp - B), (csc, cse, 1), cdev.storage_offset() + B)
        pad[:] = eye.reshape(nt, 1, 1)
    return cdev, csc, cse, csb, Bv


class _AnisoElasticSolve(_ElasticSolve):
    """`_ElasticSolve` with the tensor assembly, the measured smoother bounds and dL/dC; `forward`, `adjoint`, the
    right-hand side, the layout helpers and the solves are the base class's."""
    Info = AnisoElasticInfo
    bounds_error = ("diffhe: stiffness tensor not positive definite (a diagonal entry of the assembled operator is not "
                    "positive and finite)")

    def _operator(self, C):
        """vals (d W, n d, Bv), lift (n d, Bv) of the block row-gather assembly (csrc/elastic_aniso.hip), and Bv."""
        plan, dofs, call = self.plan, self.setup.dofs, self.call
        cdev, csc, cse, csb, Bv = _stiffness_device(self.node_eng, C, call.mode, call.B, self.Bp, self.solver.nt,
                                                    call.kappa_em)
        gtab, vol = plan.gradient_table()
        vals = torch.empty((dofs.W, dofs.n, Bv), dtype=torch.float64, device=plan.device)
        lift = torch.empty((dofs.n, Bv), dtype=torch.float64, device=plan.device)
        self.eng.L.diffhe_elastc_assemble_rows(gtab, vol, plan.dim, cdev, csc, cse, csb, plan.ent_ptr, plan.contrib,
                                               plan.cols, dofs.is_bc, dofs.g, vals, lift, plan.n, plan.m, plan.W, Bv,
                                               _stream(plan.device))
        return vals, lift, Bv

    def _coeff_grad(self, lam):
        """dL/dC in the shape of C from the adjoint lambda and the saved iterate (`diffhe_elastc_grad*`)."""
        call, plan, B, Bp = self.call, self.plan, self.call.B, self.Bp
        L, st = self.eng.L, _stream(plan.device)
        gtab, vol = plan.gradient_table()
        args = (plan.elems, gtab, vol, plan.dim, lam, self.x, self.setup.dofs.g, plan.n, plan.m)
        sums, dc = self.node_eng.element_grad(
            call.mode, call.kappa_em, B, Bp, self.solver.nt,
            lambda dc_e, osc, ose, part, total: L.diffhe_elastc_grad(*args, Bp, dc_e, osc, ose, part, total, st),
            lambda dc, osc, ose: L.diffhe_elastc_grad_shared(*args, B, Bp, dc, osc, ose, st))
        if call.mode == K_SCALAR:               # (nt, B) sums over the elements: the one tensor takes their total
            dc = sums.sum(dim=1)
        elif call.mode == K_SAMPLE:
            dc = sums.t()
        return dc.reshape(call.e_shape)


# ---------------------------------------------------------------------------------------------
# torch.library custom ops diffhe::elastic_aniso_solve / diffhe::elastic_aniso_solve_backward, on the shared plumbing of
# diffhe::elastic_solve (diffhe.elastic): the solver and the state of the call travel as integer handles.  f / load: empty
# tensor = absent.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("diffhe::elastic_aniso_solve", mutates_args=())
def elastic_aniso_solve(C: torch.Tensor, f: torch.Tensor, load: torch.Tensor, handle: int, save: bool,
                        node_major: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u, token) of the `AnisotropicElasticFESolver` registered under `handle`; `token` names the saved adjoint state
    (0 when `save` is false)."""
    solver = _SOLVERS[handle]
    return _solve_result(*_solve_call(solver, _AnisoElasticSolve, C, f, load, node_major,
                                      lambda C_, m, B_rhs, node: _stiffness_layout(C_, solver.nt, m, B_rhs, node),
                                      hierarchy=(HIERARCHY_NU, solver._plane)), save)


@elastic_aniso_solve.register_fake
def _elastic_aniso_solve_fake(C, f, load, handle, save, node_major):
    return _solve_fake(_SOLVERS[handle], C, f, load, node_major, _SOLVERS[handle].nt)


@torch.library.custom_op("diffhe::elastic_aniso_solve_backward", mutates_args=())
def elastic_aniso_solve_backward(gbar: torch.Tensor, token: torch.Tensor, need_c: bool, need_f: bool, need_load: bool,
                                 c_like: torch.Tensor, f_like: torch.Tensor,
                                 load_like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dL/dC, dL/df, dL/dload) of the forward call named by `token` from ONE adjoint solve; unused ones come back empty."""
    _, grads = _run_adjoint(gbar, token, need_c, need_f, need_load)
    return _like_grads(gbar, grads, (c_like, f_like, load_like))


@elastic_aniso_solve_backward.register_fake
def _elastic_aniso_solve_backward_fake(gbar, token, need_c, need_f, need_load, c_like, f_like, load_like):
    return _fake_grads(gbar, (need_c, need_f, need_load), (c_like, f_like, load_like))


_setup_context, _backward = _solve_autograd(
    "elastic_aniso_solve", 3, 6, "diffhe: second-order derivatives of an anisotropic elastic solve are not implemented "
    "(backward with create_graph=True, diffhe.elastic_aniso)")


# ---------------------------------------------------------------------------------------------
# The public solver
# ---------------------------------------------------------------------------------------------
class AnisotropicElasticFESolver(_ElasticOptions):
    """Displacement of a linear-elastic body with a stiffness tensor per element and sample, differentiable with respect
    to the tensor, the body force f and the nodal load (see the module docstring).

    Parameters
    ----------
    mesh : FEMesh -- P1 triangles or P1 tetrahedra.
    C : tensor or Parameter -- upper-triangle components (nt,), (B, nt), (m, nt), (B, m, nt); (nt, m, B) with
        layout="node".  nt = 6 in 2D, 21 in 3D.  May require grad.
    fixed : None (clamp the nodes of mesh.dirichlet_nodes) or {(node, component): value}.
    validate : check every call that C is finite and positive definite (ValueError; one device synchronisation).
    device, tol, max_iter, method ("auto" or "ell-jacobi"), amg : as on `ElasticFESolver`.
    """

    _refusal_scope = "with a stiffness tensor"

    def __init__(self, mesh, C, *, fixed=None, validate: bool = False, device=None, tol: Optional[float] = None,
                 max_iter: int = 20000, method: str = "auto", amg: Optional[dict] = None, check_every: int = 25):
        super().__init__()
        _check_mesh(mesh, self._ONE_D, "diffhe: elasticity with a stiffness tensor is implemented for P1 elements only "
                                       "(this mesh has {k} nodes per element)")
        self._init_options(mesh, fixed, device, tol, max_iter, method, amg, check_every, "isotropic unit operator")
        self.validate = bool(validate)
        self.nv = 3 if mesh.dim == 2 else 6
        self.nt = self.nv * (self.nv + 1) // 2
        self._plane = "stress" if mesh.dim == 2 else None      # of the isotropic unit operator behind the hierarchy
        self._C = _t64(C).to(dtype=torch.float64)
        if self._C.dim() != 3:      # a per-sample field is checked against the batch of the right-hand side at the first solve
            _stiffness_layout(self._C, self.nt, mesh.n_elements, None)
        self.last_info = AnisoElasticInfo()

    @property
    def C(self) -> torch.Tensor:
        return self._C

    def _validate(self, mode: int, em: bool) -> None:
        Cm = matrix(self._C.detach().movedim(0, -1) if (mode == K_SAMPLE_ELEM and em) else self._C.detach())
        ok = torch.isfinite(Cm).all() & (torch.linalg.cholesky_ex(torch.nan_to_num(Cm)).info == 0).all()
        if not bool(ok):
            raise ValueError("diffhe: the stiffness tensor is not symmetric positive definite everywhere (validate=True)")

    def forward(self, f: Optional[torch.Tensor] = None, load: Optional[torch.Tensor] = None, layout: str = "sample",
                dirichlet=None, h=None, u_inf=None, flux=None, eigenstrain=None) -> torch.Tensor:
        """u for the body force f and the nodal load: (n, d), (B, n, d), or (n, d, B) with layout="node" -- the shape of
        the right-hand side.  f None: zero."""
        if eigenstrain is not None:
            raise NotImplementedError("diffhe: eigenstrain= is not implemented with a stiffness tensor (the eigenstrain "
                                      "kernels read (E, nu)); add the load C eps0 to load=")
        C = self._C
        f_in, load_in, node = self._rhs_inputs(C, f, load, layout, dirichlet=dirichlet, h=h, u_inf=u_inf, flux=flux)
        mode, _, em = _stiffness_layout(C, self.nt, self.mesh.n_elements, _batch_of(self, f_in, load_in, node)[0], node)
        if self.validate:
            self._validate(mode, em)
        _SOLVERS[id(self)] = self
        save = torch.is_grad_enabled() and (C.requires_grad or f_in.requires_grad or load_in.requires_grad)
        u, _token = torch.ops.diffhe.elastic_aniso_solve(C, f_in, load_in, id(self), save, node)
        return u

    # -- stress recovery: sigma = C eps(u) and the failure index (diffhe.elastic_aniso_stress) ---------------
    def tensor_stress(self, u: torch.Tensor, C=None, layout: str = "sample") -> torch.Tensor:
        """Stresses sigma = C eps(u) of the displacement u -- (n, d), (B, n, d), or (n, d, B) with layout="node", what
        `forward` returns; strided views are read as they are -- in Voigt components (xx, yy, xy | xx, yy, zz, yz, xz, xy;
        shear components are tensor components): (m, nc), (B, m, nc), or (m, nc, B) with layout="node", the shapes of
        `ElasticFESolver.stress`.  C: None for the solver's, or another tensor in any layout C takes (the relaxed stress
        of stress-constrained design); an unbatched u is broadcast to the batch of C.  u and C may require grad."""
        from . import elastic_aniso_stress
        return elastic_aniso_stress._evaluate(self, u, None, C, layout, True, False)[0]

    def failure_index(self, u: torch.Tensor, criterion, C=None, layout: str = "sample") -> torch.Tensor:
        """The failure index phi = q . sigma + sigma . Q sigma per element, (m,), (B, m), or (m, B) with layout="node"; no
        stress array is formed.  criterion: ONE tensor of nk = nv + nt components (9 in 2D, 27 in 3D), q first, then the
        upper triangle of Q -- `diffhe.tsai_wu`, `tsai_hill`, `von_mises_criterion`, `quadratic` -- as (nk,), (B, nk),
        (m, nk), (B, m, nk), or (nk, m, B) with layout="node"; it may require grad, and its gradient comes back in its
        shape.  Other arguments as `tensor_stress`."""
        from . import elastic_aniso_stress
        return elastic_aniso_stress._evaluate(self, u, criterion, C, layout, False, True)[1]

    def tensor_stress_and_failure_index(self, u: torch.Tensor, criterion, C=None,
                                        layout: str = "sample") -> Tuple[torch.Tensor, torch.Tensor]:
        """(`tensor_stress`, `failure_index`) from one pass over the elements, and one backward for both."""
        from . import elastic_aniso_stress
        return elastic_aniso_stress._evaluate(self, u, criterion, C, layout, True, True)

    # -- what exists for (E, nu) only -----------------------------------------------------------------
    def _no_stress(self, *args, **kwargs):
        raise NotImplementedError("diffhe: stress recovery is not implemented with a stiffness tensor by these methods "
                                  "(stress, von_mises and stress_and_von_mises read (E, nu): "
                                  "diffhe.elastic.ElasticFESolver; a reduced plane stiffness does not determine sigma_zz); "
                                  "the stress of a tensor is tensor_stress, failure_index and "
                                  "tensor_stress_and_failure_index, with diffhe.von_mises_criterion for (vm / sigma_y)^2")

    stress = von_mises = stress_and_von_mises = _no_stress

    def modes(self, *args, **kwargs):
        raise NotImplementedError("diffhe: vibration modes are not implemented with a stiffness tensor "
                                  "(diffhe.modal.ElasticEigenSolver takes (E, nu) only)")
