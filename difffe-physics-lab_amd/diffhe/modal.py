"""Vibration modes of linear-elastic bodies per sample, with d lambda / dE and d lambda / d rho (ours: the reference has
neither elasticity nor an eigensolver).

`ElasticEigenSolver(mesh, E, rho, k)` finds, for every sample b, the k smallest lambda = omega^2 and the mode shapes of

    K(E_b) phi = lambda M(rho_b) phi

on P1 triangles (d = 2) and P1 tetrahedra (d = 3).  K is the operator of `ElasticFESolver` -- same `nu`, `plane` and
`fixed` -- and M the LUMPED mass of a density per element: every component a of node i carries
m_{i,b} = sum_{(e, p) at i} rho_{e,b} vol_e / (d + 1); with rho = 1 that is `plan.lumped_mass()` repeated per component.
The boundary conditions are homogeneous: only the KEYS of `fixed` (or the nodes of `mesh.dirichlet_nodes` when `fixed` is
None) count, values are ignored, as `EigenFESolver` ignores them.  `frequency(lam)` turns lambda into Hz.

Method: the block inverse iteration with Rayleigh-Ritz of `diffhe.eigen` (`_BlockRun`, DESIGN section 7 "Eigenpairs" and
"Vibration modes") on the n d dofs.  Once per call the operator is assembled (`_ElasticSetup.assemble`), shifted by
sigma M(rho_b) on the diagonal of the free rows where `shift` = sigma > 0, and the Galerkin operators of the cached unit-E
hierarchy are formed (`_Engine.amg_setup`); every inner solve is `amg_pcg` -- `cg` with method="ell-jacobi" -- at
`inner_tol`, every A x one `diffhe_ell_apply`.  The Gram, rotation, residual and sign passes are the kernels of
csrc/eigen.hip reading a nodal mass per sample (include/diffhe_modal.h); the mass itself is one node pass
(`diffhe_modal_mass`).

Layouts.  E and rho each take (), (m,), (B,) / (B, 1) and (B, m), each read as `EigenFESolver` reads kappa: a 1D tensor
of m entries is the element field unless `batch=` equals m, and `batch=` is the batch where neither carries one.  The two
batches must agree.  Returns `lam` (B, k) ascending -- (k,) when nothing is batched -- and `phi` (B, k, n, d), or with
layout="node" (k, n, d, B), the block itself.  phi is M(rho_b)-orthonormal, zero on fixed dofs, signed so that
sum_{i,a} m_i phi_{i,a} > 0 (below 1e-8 in magnitude: the entry of largest magnitude is positive), and NON-differentiable.

Gradients (Hellmann-Feynman, phi M-normalised, no solve in backward):

    d lambda_i / d E_e   = phi_i^T K_e0 phi_i                                     (`diffhe_elast_grad`, u = phi_i)
    d lambda_i / d rho_e = -lambda_i vol_e / (d + 1) sum_{p in e} sum_a phi_i[(el_p, a)]^2     (`diffhe_modal_grad_rho`)

in the shape of E and rho; a field the batch shares gets its gradient summed over the batch inside the kernel.  For a
cluster of equal eigenvalues the gradient is that of the Rayleigh quotients of the returned basis: right for symmetric
functions of the cluster, not for one member of a degenerate pair.

A body with no fixed dof needs `shift > 0` (ValueError otherwise): its 3 (2D) or 6 (3D) rigid-body modes are then found as
lambda ~ 0 like any other mode; the returned lambda exclude the shift.  A partly constrained body that keeps a rigid mode
with shift = 0 surfaces as the non-convergence warning: the caller's error, as in `ElasticFESolver`.

Not implemented (NotImplementedError): 1D meshes, P2 meshes, `amg=dict(strength=...)`, node gradients, backward with
create_graph=True.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _hip
from .eigen import JACOBI_SWEEPS, MAX_BLOCK, EigenInfo, _BlockRun, _check_iteration
from .elastic import _amg_options, _check_mesh, _select_hierarchy, _setup_of, lame_unit, parse_fixed
from .plan import get_plan, padded_batch, _stream
from .solver import (K_ELEM, K_SAMPLE_ELEM, SolveInfo, _Engine, _SOLVERS, _fake_grads, _kappa_grad, _kappa_mode,
                     _like_grads, _register_state, _resolve_device, _state_of, _tie_state)

__all__ = ("ElasticEigenSolver", "frequency")


def frequency(lam: torch.Tensor) -> torch.Tensor:
    """The frequencies sqrt(max(lambda, 0)) / (2 pi) of the eigenvalues lambda = omega^2 (a rigid-body lambda of -1e-14
    is 0 Hz).  Plain differentiable torch; the derivative is defined as 0 where lambda <= 0 (the square root has none
    at 0), so the rigid-body modes of a free body put no NaN into the gradient of a loss over all modes."""
    pos = lam > 0.0
    root = torch.sqrt(torch.where(pos, lam, torch.ones_like(lam)))
    return torch.where(pos, root, torch.zeros_like(lam)) / (2.0 * math.pi)


def _field_layout(t: torch.Tensor, name: str, m: int, batch: Optional[int]):
    """-> (mode, batch implied or None) of one scalar field, E or rho: `_kappa_mode` as `_eigen_layout` calls it."""
    try:
        if t.dim() >= 3:
            raise ValueError
        return _kappa_mode(t, m, batch)
    except ValueError:
        raise ValueError(f"{name} shape {tuple(t.shape)} not understood for a mesh with {m} elements: expected (), "
                         f"({m},), (B,), (B, 1) or (B, {m})") from None


def _modal_layout(E: torch.Tensor, rho: torch.Tensor, m: int, batch: Optional[int]):
    """-> (mode of E, mode of rho, B, batched) of one call: each field read on its own as `_eigen_layout` reads kappa
    (`batch` decides how a (B,) field with B == m reads, and is the batch where neither field carries one)."""
    if batch is not None and int(batch) < 1:
        raise ValueError(f"batch must be >= 1, got {batch!r}")
    b = None if batch is None else int(batch)
    mode_e, Be = _field_layout(E, "E", m, b)
    mode_r, Br = _field_layout(rho, "rho", m, b)
    for name, Bk in (("E", Be), ("rho", Br)):
        if b is not None and Bk is not None and Bk != b:
            raise ValueError(f"{name} batch {Bk} does not match batch={batch}")
    if Be is not None and Br is not None and Be != Br:
        raise ValueError(f"rho batch {Br} does not match E batch {Be}")
    Bk = Be if Be is not None else Br
    B = Bk if Bk is not None else (b if b is not None else 1)
    return mode_e, mode_r, B, (Bk is not None or b is not None)


class _ModalRun(_BlockRun):
    """One modal call: the shifted dof operator and its Galerkin chain, the nodal mass per sample and the block buffers.
    After `run()` it keeps what the Hellmann-Feynman backward reads: the k columns, lambda and the plan."""

    def __init__(self, ms: "ElasticEigenSolver", E: torch.Tensor, rho: torch.Tensor, batch: Optional[int]):
        self.es, self.plan = ms, ms._plan()
        plan = self.plan
        self.setup = _setup_of(plan, ms.nu, ms.plane, ms._lam1, ms._mu1, ms._is_bc, ms._g)
        dofs = self.setup.dofs
        self.mode_e, self.mode_r, self.B, self.batched = _modal_layout(E, rho, plan.m, batch)
        self.Bp = padded_batch(self.B)
        self.k, self.p = ms.k, ms.k + ms.guard
        self.rows, self.vec, self.d = dofs.n, (plan.n, plan.dim), plan.dim
        n_free = dofs.n - int(ms._is_bc.sum())
        if self.p > n_free:
            raise ValueError(f"block of {self.p} vectors on a mesh with {n_free} free dofs")
        self.e_shape, self.e_device, self.r_shape, self.r_device = E.shape, E.device, rho.shape, rho.device
        self.L = _hip.lib()
        self.node_eng = _Engine(plan, 0.0, 0, 0, "gather")
        self.eng = _Engine(dofs, ms.inner_tol, int(ms.amg.get("max_iter", 20000)), 25, "gather", g=dofs.g)
        self.X = None

    # -- the problem: K(E) + sigma M(rho) against M(rho) on the dofs -------------------------------------------------------
    def _bc_rows(self):
        return None if self.setup.free.all() else ~self.setup.free

    def _setup(self, coeffs, Y: torch.Tensor, info: EigenInfo, keep: bool = False) -> None:
        """Mass, assembly, shift and the Galerkin operators, once; no solve."""
        E, rho = coeffs
        ms, plan, setup, L, B, Bp, d = self.es, self.plan, self.setup, self.L, self.B, self.Bp, self.d
        dofs, st = setup.dofs, _stream(plan.device)
        kdev, kse, ksb, Bve = self.node_eng.kappa_device(E, self.mode_e, B, Bp)
        rdev, rse, rsb, Bvr = self.node_eng.kappa_device(rho, self.mode_r, B, Bp)
        # a per-sample field of a batch of one, (1, m), has width 1: the entries take it as a shared field, stride 0
        ksb, rsb = (ksb if Bve > 1 else 0), (rsb if Bvr > 1 else 0)
        _, vol = plan.gradient_table()
        self.mass = self._new(plan.n, Bvr)
        L.diffhe_modal_mass(*plan.shape_incidence(), vol, d, rdev, rse, rsb, plan.n, plan.m, B if Bvr > 1 else 1, Bvr,
                            self.mass, st)
        self.mass_args = (self.mass, Bvr, 1 if Bvr > 1 else 0, d)      # mass, stride per node, per sample, dofs per node
        vals, _ = setup.assemble(kdev, kse, ksb, Bve)
        Bv = Bve
        if ms.shift > 0.0:
            Bv = max(Bve, Bvr)          # the operator carries the batch width of whichever of E and rho is per sample
            if Bv > Bve:
                vals = vals.expand(dofs.W, dofs.n, Bv).contiguous()
            add = (ms.shift * self.mass)[:, None, :].expand(plan.n, d, Bvr).reshape(dofs.n, Bvr)
            vals[0] += torch.where(setup.free[:, None], add, torch.zeros_like(add))     # slot 0: the diagonal
        self.vals, self.Bv = vals, Bv
        sinfo, self.amg = SolveInfo(), dict(ms.amg)
        self.hier, _ = _select_hierarchy(self.eng, setup, ms.method, self.amg, vals, Bv, Bp, sinfo)
        info.inner, info.path = sinfo, sinfo.path
        self._apart = self._new(L.diffhe_grad_kappa_blocks(dofs.n, Bp) * Bp)

    def _apply(self, x: torch.Tensor, y: torch.Tensor) -> None:
        dofs = self.setup.dofs
        self.L.diffhe_ell_apply(self.vals, dofs.cols, x, y, self._apart, dofs.n, dofs.W, self.Bp, self.Bv,
                                _stream(self.plan.device))

    def _inner_solve(self, rhs: torch.Tensor):
        if self.hier is not None:
            return self.eng.amg_pcg(self.hier, rhs, self.Bp, self.Bv, self.amg)
        return self.eng.cg(self.vals, rhs, self.Bp, self.Bv)

    def _rayleigh_ritz(self, Y, AY) -> None:
        L, p, n, Bp, st = self.L, self.p, self.rows, self.Bp, _stream(self.plan.device)
        b, mass = self.buf, self.mass_args
        L.diffhe_modal_gram(Y, AY, *mass, self.setup.dofs.is_bc, p, n, Bp, b["part"], b["GA"], b["GM"], st)
        L.diffhe_eig_ritz(b["GA"], b["GM"], p, Bp, JACOBI_SWEEPS, b["work"], b["C"], b["theta"], b["flag"], st)
        L.diffhe_modal_rotate(Y, AY, b["C"], b["theta"], *mass, p, n, Bp, b["X"], b["AX"], None, b["R"], st)
        L.diffhe_modal_residual(b["R"], b["theta"], *mass, p, n, Bp, b["part"], b["rho"], st)

    def _fix_sign(self, X, sgn) -> None:
        self.L.diffhe_modal_fix_sign(X, *self.mass_args, self.k, self.rows, self.Bp, self.buf["part"], sgn,
                                     _stream(self.plan.device))

    # -- what LOBPCG asks of the problem ------------------------------------------------------------------------------------
    def _free_mask(self):
        return self.setup.dofs.is_bc

    def _times_mass(self, x: torch.Tensor, y: torch.Tensor) -> None:
        n, d, Bp = self.plan.n, self.d, self.Bp
        torch.mul(x.view(n, d, Bp), self.mass[:, None, :], out=y.view(n, d, Bp))

    def _residual_norms(self) -> None:
        b = self.buf
        self.L.diffhe_modal_residual(b["R"], b["theta"], *self.mass_args, self.p, self.rows, self.Bp, b["part"], b["rho"],
                                     _stream(self.plan.device))

    def _release(self) -> None:
        # what backward needs: the k columns, lambda and the plan's element tables; operator, hierarchy and mass go
        self.lam = self.buf["theta"][:self.k] - self.es.shift                      # (k, Bp)
        self.g0, self.lam1, self.mu1 = self.setup.dofs.g, self.setup.lam1, self.setup.mu1
        self.vals = self.hier = self.mass = self.mass_args = self._apart = self.eng = self.setup = None

    def backward(self, glam: torch.Tensor, need_e: bool, need_r: bool):
        """(dL/dE, dL/drho) in the shapes of E and rho from the cotangent of lam.  dE: the strain-form gradient kernels
        (which compute -lam^T K_e0 u) with u = phi_i and lam = -lambda_bar_i phi_i, summed over i; drho: one element pass
        with the weights -lambda_bar_i lambda_i."""
        plan, eng, L, B, Bp, k = self.plan, self.node_eng, self.L, self.B, self.Bp, self.k
        st = _stream(plan.device)
        gp = torch.zeros((k, Bp), dtype=torch.float64, device=plan.device)
        gp[:, :B] = glam.detach().to(plan.device, torch.float64).reshape(B, k).t()
        gtab, vol = plan.gradient_table()

        def shaped(mode, shape, sums, elem):
            if mode == K_SAMPLE_ELEM:           # asked for element-major (m, B): no transposing pass per column
                elem = elem.t().contiguous()
            return _kappa_grad(mode, shape, sums, elem)

        grad_e = grad_r = None
        if need_e:
            acc = None
            for i in range(k):
                lamv = self.X[i] * (-gp[i])[None, :]
                args = (plan.elems, gtab, vol, plan.dim, self.lam1, self.mu1, lamv, self.X[i], self.g0, plan.n, plan.m)
                sums, elem = eng.element_grad(
                    self.mode_e, True, B, Bp, None,
                    lambda de_e, osc, ose, part, total: L.diffhe_elast_grad(*args, Bp, de_e, part, total, st),
                    lambda de, osc, ose: L.diffhe_elast_grad_shared(*args, B, Bp, de, st))
                part = elem if sums is None else sums
                acc = part if acc is None else acc + part
            sums, elem = (acc, None) if self.mode_e not in (K_ELEM, K_SAMPLE_ELEM) else (None, acc)
            grad_e = shaped(self.mode_e, self.e_shape, sums, elem).to(self.e_device)
        if need_r:
            w = -(gp * self.lam)
            args = (plan.elems, vol, plan.dim, self.X, w, k, plan.n, plan.m, B, Bp)
            sums, elem = eng.element_grad(
                self.mode_r, True, B, Bp, None,
                lambda dr_e, osc, ose, part, total: L.diffhe_modal_grad_rho(*args, dr_e, part, total, st),
                lambda dr, osc, ose: L.diffhe_modal_grad_rho_shared(*args, dr, st))
            grad_r = shaped(self.mode_r, self.r_shape, sums, elem).to(self.r_device)
        return grad_e, grad_r


# ---------------------------------------------------------------------------------------------
# torch.library custom ops diffhe::modal_solve / diffhe::modal_solve_backward: the solver and the state of the call travel
# as integer handles through the registries of diffhe.solver.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("diffhe::modal_solve", mutates_args=())
def modal_solve(E: torch.Tensor, rho: torch.Tensor, x0: Optional[torch.Tensor], handle: int, batch: int,
                node_layout: bool, save: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(lam, phi, token) of the `ElasticEigenSolver` registered under `handle`; batch < 1: none given; `token` names the
    saved state of the call (0 when `save` is false)."""
    run = _ModalRun(_SOLVERS[handle], E, rho, batch if batch >= 1 else None)
    lam, phi = run.run((E, rho), x0, node_layout)
    # fresh tensors (an op's outputs may not alias one another); with layout="node" phi is the block itself
    return lam.to(E.device), phi.to(E.device), _register_state(run, save)


@modal_solve.register_fake
def _modal_solve_fake(E, rho, x0, handle, batch, node_layout, save):
    ms = _SOLVERS[handle]
    n, d, m, k = ms.mesh.n_nodes, ms.mesh.dim, ms.mesh.n_elements, ms.k
    _, _, B, batched = _modal_layout(E, rho, m, batch if batch >= 1 else None)
    lam = E.new_empty((B, k) if batched else (k,), dtype=torch.float64)
    if node_layout:
        phi = E.new_empty((k, n, d, B), dtype=torch.float64)
    else:
        phi = E.new_empty((B, k, n, d) if batched else (k, n, d), dtype=torch.float64)
    return lam, phi, torch.empty((), dtype=torch.int64)


@torch.library.custom_op("diffhe::modal_solve_backward", mutates_args=())
def modal_solve_backward(glam: torch.Tensor, token: torch.Tensor, need_e: bool, need_r: bool, e_like: torch.Tensor,
                         r_like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dL/dE, dL/drho) of the call named by `token` from the cotangent of lam; no solve; unused ones come back empty."""
    return _like_grads(glam, _state_of(token).backward(glam, need_e, need_r), (e_like, r_like))


@modal_solve_backward.register_fake
def _modal_solve_backward_fake(glam, token, need_e, need_r, e_like, r_like):
    return _fake_grads(glam, (need_e, need_r), (e_like, r_like))


def _setup_context(ctx, inputs, output):
    """Save (token, E, rho) and tie the saved state of the call to them.  phi (and the token) are marked
    non-differentiable."""
    lam, phi, token = output
    ctx.mark_non_differentiable(phi, token)
    _tie_state(ctx, token, inputs[0], inputs[1])


def _backward(ctx, glam, _gphi, _gtoken):
    if torch.is_grad_enabled():
        raise NotImplementedError("diffhe: second-order derivatives of eigenvalues are not implemented (backward with "
                                  "create_graph=True, diffhe.modal)")
    token, E, rho = ctx.saved_tensors[:3]
    need_e, need_r = (bool(v) for v in ctx.needs_input_grad[:2])
    if not (need_e or need_r):
        return (None,) * 7
    ge, gr = torch.ops.diffhe.modal_solve_backward(glam.contiguous(), token, need_e, need_r, E, rho)
    return (ge if need_e else None, gr if need_r else None, None, None, None, None, None)


torch.library.register_autograd("diffhe::modal_solve", _backward, setup_context=_setup_context)


class ElasticEigenSolver(nn.Module):
    """The k smallest eigenpairs of K(E) phi = lambda M(rho) phi per sample -- the vibration modes of a linear-elastic
    body -- with `lam` differentiable with respect to E and rho (see the module docstring for the problem, the layouts,
    the gradients and their limits on degenerate clusters; phi is returned non-differentiable).

    Parameters
    ----------
    mesh : FEMesh -- P1 triangles or P1 tetrahedra.
    E, rho : float or tensor or Parameter -- (), (m,), (B,) / (B, 1) or (B, m) each; may require grad.
    k : number of eigenpairs; guard : extra block columns (block p = k + guard <= 16).
    nu, plane, fixed : as on `ElasticFESolver`; of `fixed` (and of mesh.dirichlet_nodes) only the keys count.
    tol : stop when |A x - theta M x|_{M^-1} / theta <= tol for the k columns of every sample; max_iter : outer iterations.
    shift : sigma >= 0, the inner solves run on K + sigma M(rho); required > 0 for a body with no fixed dof.  The returned
        lambda exclude it.
    seed : of the CPU generator the start block is drawn from.  inner_tol : relative residual of the inner solves.
    iteration : "subspace" (default) or "lobpcg", as on `EigenFESolver`.
    device, method ("auto" or "ell-jacobi"), amg : as on `ElasticFESolver`.
    """

    def __init__(self, mesh, E=1.0, rho=1.0, k: int = 4, *, nu: float = 0.3, plane: Optional[str] = None, fixed=None,
                 guard: int = 4, tol: float = 1e-8, max_iter: int = 200, shift: float = 0.0, seed: int = 0,
                 inner_tol: float = 1e-2, device=None, method: str = "auto", amg: Optional[dict] = None,
                 iteration: str = "subspace", **options):
        super().__init__()
        self.iteration = _check_iteration(iteration)
        for name in ("reaction", "warm_start"):
            if name in options:
                raise ValueError(f"{name}= is not an option of ElasticEigenSolver" + (" (use shift=)" if name == "reaction"
                                                                                       else ""))
        if options:
            raise TypeError(f"ElasticEigenSolver got unexpected options: {sorted(options)}")
        _check_mesh(mesh, "diffhe: vibration modes need a 2D or 3D mesh (a 1D bar is a tridiagonal pencil: dense-eigh "
                    "territory)",
                    "diffhe: vibration modes are implemented for P1 elements only (the row-sum lumped mass of a mesh with "
                    "{k} nodes per element is not positive)", dims="Only 2D and 3D meshes supported")
        if mesh.dim == 3 and plane is not None:
            raise ValueError("plane= applies to 2D meshes only (a 3D body needs no plane-stress / plane-strain choice)")
        self.plane = None if mesh.dim == 3 else ("stress" if plane is None else plane)
        self.nu = float(nu)
        self._lam1, self._mu1 = lame_unit(self.nu, mesh.dim, self.plane)
        if method not in ("auto", "ell-jacobi"):
            raise ValueError(f"Unknown method: {method!r}")
        k, guard = int(k), int(guard)
        if k < 1 or guard < 0 or k + guard > MAX_BLOCK:
            raise ValueError(f"need 1 <= k and guard >= 0 with k + guard <= {MAX_BLOCK}, got k={k}, guard={guard}")
        if not (float(tol) > 0.0) or not (0.0 < float(inner_tol) < 1.0) or int(max_iter) < 0:
            raise ValueError(f"need tol > 0, 0 < inner_tol < 1, max_iter >= 0, got {tol!r}, {inner_tol!r}, {max_iter!r}")
        if not (float(shift) >= 0.0):
            raise ValueError(f"shift must be >= 0, got {shift!r}")
        if fixed is None:
            keys = [(int(i), a) for i in mesh.dirichlet_nodes for a in range(mesh.dim)]
        elif hasattr(fixed, "keys"):
            keys = list(fixed.keys())
        else:
            raise ValueError("fixed= must be a mapping {(node, component): value}")
        self._is_bc, self._g = parse_fixed(mesh, {key: 0.0 for key in keys})      # homogeneous: the values are ignored
        if not self._is_bc.any() and float(shift) == 0.0:
            raise ValueError("diffhe: a body with no fixed dof needs shift > 0 (K alone is singular there: rigid-body "
                             "modes)")
        self.amg = _amg_options(amg, "diffhe: amg=dict(strength=...) is not implemented for vibration modes (the hierarchy "
                                     "is built from the unit-E operator)",
                                "diffhe: vibration modes use the smoothed-aggregation hierarchy of elasticity (amg "
                                "smoothed=0 is not implemented)")
        as64 = lambda v: (torch.tensor(float(v), dtype=torch.float64) if isinstance(v, (int, float))  # noqa: E731
                          else v.to(dtype=torch.float64))
        self.mesh, self.method, self.k, self.guard = mesh, method, k, guard
        self._E, self._rho = as64(E), as64(rho)
        _modal_layout(self._E, self._rho, mesh.n_elements, None)
        self.tol, self.max_iter, self.shift, self.seed = float(tol), int(max_iter), float(shift), int(seed)
        self.inner_tol = float(inner_tol)
        self._device = device
        self.last_info = EigenInfo()

    @property
    def E(self) -> torch.Tensor:
        return self._E

    @property
    def rho(self) -> torch.Tensor:
        return self._rho

    def _plan(self):
        return get_plan(self.mesh, _resolve_device(self._device), prune=False)

    def forward(self, batch: Optional[int] = None, x0: Optional[torch.Tensor] = None, layout: str = "sample"):
        """-> (lam, phi).  batch: the number of samples, where neither E nor rho says (or a field reads both ways); x0: a
        previous phi in the same `layout` as a warm start -- with k columns it is padded with seeded random guard
        columns, with k + guard columns it is the whole start block; layout: "sample" = phi (B, k, n, d), "node" = phi
        (k, n, d, B)."""
        if layout not in ("sample", "node"):
            raise ValueError(f"Unknown layout: {layout!r}")
        if self.mesh.nodes.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("diffhe: node gradients are not implemented for vibration modes (mesh.nodes "
                                      "requires grad)")
        E, rho = self._E, self._rho
        _modal_layout(E, rho, self.mesh.n_elements, batch)
        _SOLVERS[id(self)] = self
        save = torch.is_grad_enabled() and (E.requires_grad or rho.requires_grad)
        lam, phi, _token = torch.ops.diffhe.modal_solve(E, rho, None if x0 is None else x0.detach(), id(self),
                                                        -1 if batch is None else int(batch), layout == "node", save)
        return lam, phi
