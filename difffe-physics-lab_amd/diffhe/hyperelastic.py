"""Finite-strain compressible Neo-Hookean elasticity with Newton solves and dL/dE (ours: the reference solves linear
scalar equations only).

`HyperelasticFESolver(mesh, E, nu)` is the large-displacement counterpart of `ElasticFESolver`: on P1 triangles (plane
strain) and P1 tetrahedra it finds the displacement u with R(u, E) = F_ext for the energy per reference volume

    F = I + grad u,   J = det F
    W(F) = E [ mu1/2 (tr F^T F - d) - mu1 ln J + lam1/2 (ln J)^2 ]
    mu1 = 1 / (2 (1 + nu)),   lam1 = nu / ((1 + nu)(1 - 2 nu))         (the 3D Lame numbers of E = 1, also in plane strain)
    P1(F) = mu1 (F - F^-T) + lam1 ln J F^-T                             (first Piola-Kirchhoff stress of E = 1)
    R(u, E)_(p,i) = sum_e vol_e E_e [P1(F_e) g_p]_i                     (internal force; g_p = grad phi_p)

with a Young's modulus E per element and sample that may require grad.  Loads are DEAD loads per reference volume: the
body force f goes through the plan's load map and `load` is nodal, exactly as `ElasticFESolver` takes them, with the same
E layouts -- (), (B,), (m,), (B, m), (m, B) with layout="node" -- the same `fixed=` (rollers, prescribed values) and the
same shapes of f, load and u.  For small loads u tends to the plane-strain / 3D solution of `ElasticFESolver`.

Newton.  The load and the prescribed values are applied in `steps` equal increments, t = k / steps.  Every step starts
from the previous one (the first from `x0`, else from zero) with the fixed dofs set to t g and iterates per sample:

  residual     r = R(u) - t F_ext on the free dofs; the stop rule ||r|| <= newton_tol ||t F_ext|| (with F_ext = 0: the
               norm of the step's first residual, the one the prescribed values leave);
  tangent      K_T(u, E) assembled in the dof pattern of `ElasticFESolver`, the Galerkin operators on the CACHED unit-E
               hierarchy of (nu, plane strain | 3D), the smoother's row bounds measured (`_measure_row_bounds`);
  solve        K_T delta = -r by `eng.amg_pcg` / `eng.cg` to `linear_tol` (None: `tol`); samples that met the stop rule
               are frozen: zero right-hand side, alpha = 0;
  line search  per sample on Pi(u) = W(u) - t F_ext . u: Armijo with c = 1e-4, alpha halved up to `max_backtracks`
               times.  The energy kernel returns +inf for a state that inverts an element (J <= 0), so such a step is
               never taken and the tangent is never assembled there.  Pi is a sum of m rounded terms, so the test allows
               for that rounding: 16 eps (|W| + |F_ext . u| + sqrt(2 d mu1 W sum_e vol_e E_e)), the last term bounding
               sum_e vol_e E_e mu1 |grad u| by Cauchy-Schwarz.  The slack matters only where the predicted decrease is
               below it: at the last iterations, where Newton's full step is the right one.  Where the test still
               fails -- at very small strains the decrease of Pi lies below the rounding of its evaluation -- a step
               with a finite energy is also taken if it shrinks the residual, ||r(u + alpha delta)|| <=
               (1 - c alpha) ||r(u)||: one more residual pass, only in iterations where some sample fails the test.

`newton_iterations` counts tangent solves.  After the last step the tangent and its hierarchy are built once more at the
final u: they, and u, are what the adjoint reads.  The tangent of a hyperelastic energy is symmetric, so the adjoint is
`_ElasticSolve.adjoint` unchanged -- ONE linear solve K_T lambda = gbar, to `tol` -- followed by

    dL/dE_e = -vol_e P1(F_e(u)) : grad lambda_e,   dL/dload = lambda,   dL/df = M lambda.

Kernels: csrc/hyperelastic.hip (include/diffhe_hyperelastic.h): tangent, internal force, energy with min J, dL/dE per
sample and summed over the batch; fp64, no atomics, bitwise reproducible.  The operator is per sample even where E is
shared, because u is.

Reporting.  `last_info` is a `HyperInfo`: Newton and linear iterations, backtracks, the smallest J, the bounds of the
final tangent, and the relative residual and the step length of every iteration per sample.  Samples that exhaust `max_newton` or `max_backtracks` raise ONE RuntimeWarning
and are counted in `newton_not_converged`; the other samples are unaffected and nothing is raised.  A tangent whose
diagonal is not positive and finite raises ValueError ("tangent not positive definite: reduce the load or raise steps").

Stress recovery.  `cauchy_stress(u, E=None)`, `cauchy_von_mises`, `cauchy_stress_and_von_mises` and `energy_density`
give the Cauchy (true) stress sigma = E (1/J) [mu1 (F F^T - I) + lam1 ln J I] per element and sample, its von Mises stress
(with sigma_zz = E lam1 ln J / J of plane strain) and the energy density E W1(F) per reference volume, differentiable in
u and E (`diffhe.hyper_stress`; csrc/hyper_stress.hip, include/diffhe_hyper_stress.h).  After a solve,
`pnorm(solver.cauchy_von_mises(solver(f, load)))` is differentiable in E with one adjoint solve.

Not implemented (NotImplementedError): 1D and P2 meshes; plane="stress" (it needs a local solve for F33); backward with
create_graph=True; moving nodes; `eigenstrain=`, `dirichlet=`, Robin / flux data; the small-strain `stress`, `von_mises`
and `stress_and_von_mises` (the `cauchy_*` methods are the finite-strain ones), the Piola-Kirchhoff stresses PK1 and PK2,
and `modes`; `amg=dict(strength=...)`.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _hip, hyper_stress as _hyper_stress  # noqa: F401  (registers diffhe::hyper_stress)
from .elastic import (_ElasticOptions, _ElasticSolve, _batch_of, _check_mesh, _measure_row_bounds, _run_adjoint,
                      _select_hierarchy, _solve_autograd, _solve_call, _solve_fake, _solve_result, lame_unit)
from .elastic_stress import _stress_batch
from .plan import padded_batch, _stream
from .solver import SolveInfo, _Engine, _SOLVERS, _fake_grads, _kappa_grad, _kappa_layout, _like_grads

__all__ = ("HyperelasticFESolver", "HyperInfo")

ARMIJO_C = 1e-4
_EPS = 2.0 ** -52


@dataclass
class HyperInfo(SolveInfo):
    """`SolveInfo` of a Newton solve.  `iterations` is `linear_iterations`, `max_relres` is `max_newton_relres`;
    `not_converged` keeps the family's meaning, LINEAR systems that missed their tolerance -- here (tangent solve, sample)
    pairs of the forward plus the adjoint's -- and raises the family's warning (`_run_call`); Newton's count is
    `newton_not_converged`."""
    newton_iterations: Tuple[int, ...] = ()     # tangent solves per load step
    newton_not_converged: int = 0               # samples that exhausted max_newton or max_backtracks
    max_newton_relres: float = 0.0              # max over the samples of ||R - F_ext|| / ||F_ext|| at the returned u
    backtracks: int = 0                         # halvings of alpha, summed over samples and iterations
    linear_iterations: int = 0                  # iterations of all the tangent solves of the forward
    min_J: float = 1.0                          # smallest det F over elements and samples at the returned u
    jacobi_bounds: Tuple[float, ...] = ()       # measured on the final tangent, the fine level first
    # one row per residual evaluation, one column per sample (CPU tensors; gathered once, after the last step): the
    # relative residual that the stop rule saw, and the step length alpha the line search then took (0: frozen or none)
    relres_history: Optional[torch.Tensor] = None
    alpha_history: Optional[torch.Tensor] = None


class _HyperSolve(_ElasticSolve):
    """`_ElasticSolve` whose forward is the Newton loop of the module docstring; `adjoint`, the layout helpers and the
    load map are the base class's.  `vals`, `hier`, `x` (the FULL displacement) hold the final state for the adjoint."""
    Info = HyperInfo
    bounds_error = ("diffhe: tangent not positive definite: reduce the load or raise steps (a diagonal entry of the "
                    "assembled tangent is not positive and finite)")
    x0 = None

    # -- kernels ----------------------------------------------------------------------------------
    def _material(self):
        """elems, g_p = grad phi_p with its sign (F is LINEAR in it: `plan.oriented_gradient_table`), vol, dim, lam1, mu1."""
        plan, setup = self.plan, self.setup
        return (plan.elems, plan.oriented_gradient_table(), plan.gradient_table()[1], plan.dim, setup.lam1, setup.mu1)

    def _tangent(self, u: torch.Tensor) -> torch.Tensor:
        plan, dofs, Bp = self.plan, self.setup.dofs, self.Bp
        vals = torch.empty((dofs.W, dofs.n, Bp), dtype=torch.float64, device=plan.device)
        self.eng.L.diffhe_hyper_assemble_rows(*self._material(), *self.modulus, u, plan.ent_ptr, plan.contrib, plan.cols,
                                              dofs.is_bc, vals, plan.n, plan.m, plan.W, Bp, _stream(plan.device))
        return vals

    def _residual(self, u: torch.Tensor) -> torch.Tensor:
        plan, Bp = self.plan, self.Bp
        R = torch.empty((self.setup.dofs.n, Bp), dtype=torch.float64, device=plan.device)
        self.eng.L.diffhe_hyper_residual(*plan.shape_incidence(), *self._material(), *self.modulus, u, plan.n, plan.m, Bp,
                                         R, _stream(plan.device))
        return R

    def _energy(self, u: torch.Tensor):
        """(W (Bp,), min J (Bp,)); W = +inf where an element is inverted."""
        plan, Bp = self.plan, self.Bp
        nblk = self.eng.L.diffhe_grad_kappa_blocks(plan.m, Bp)
        part = torch.empty((2, nblk, Bp), dtype=torch.float64, device=plan.device)
        out = torch.empty((2, Bp), dtype=torch.float64, device=plan.device)
        self.eng.L.diffhe_hyper_energy(*self._material(), *self.modulus, u, plan.n, plan.m, Bp, part[0], part[1], out[0],
                                       out[1], _stream(plan.device))
        return out[0], out[1]

    def _coeff_grad(self, lam):
        """dL/dE in the shape of E from the adjoint lambda and the final displacement (`diffhe_hyper_grad*`)."""
        call, plan, B, Bp = self.call, self.plan, self.call.B, self.Bp
        L, st = self.eng.L, _stream(plan.device)
        args = (*self._material(), lam, self.x, plan.n, plan.m)
        sums, de = self.node_eng.element_grad(
            call.mode, call.kappa_em, B, Bp, None,
            lambda de_e, osc, ose, part, total: L.diffhe_hyper_grad(*args, Bp, de_e, part, total, st),
            lambda de, osc, ose: L.diffhe_hyper_grad_shared(*args, B, Bp, de, st))
        return _kappa_grad(call.mode, call.e_shape, sums, de)

    # -- the linear algebra of one tangent -----------------------------------------------------------
    def _hierarchy(self, eng: _Engine, vals: torch.Tensor, info: HyperInfo):
        """(hier or None, bounds) of the tangent `vals`; the row bound of the fine level is measured also where there is
        no hierarchy, for the check of the diagonal alone."""
        Bp, dofs = self.Bp, self.setup.dofs
        hier, bounds = _select_hierarchy(eng, self.setup, self.solver.method, self.amg, vals, Bp, Bp, info,
                                         self.bounds_error)
        if hier is None:
            fine = ((_hip.AmgLevel * 1)(), [dict(vals=vals, cols=dofs.cols, n=dofs.n, W=dofs.W)])
            _measure_row_bounds(eng, fine, Bp, self.bounds_error)
        return hier, bounds

    # -- forward: Newton ----------------------------------------------------------------------------
    def forward(self, call_in, info: HyperInfo) -> torch.Tensor:
        solver, setup, call = self.solver, self.setup, self.call
        dofs, B, dev = setup.dofs, call.B, self.plan.device
        Bp = self.Bp = self.Bv = padded_batch(B)
        kdev, kse, ksb, _ = self.node_eng.kappa_device(call_in.E, call.mode, B, Bp, em=call.kappa_em)
        self.modulus = (kdev, kse, ksb)
        lin_tol = self.eng.tol if solver.linear_tol is None else float(solver.linear_tol)
        lin = _Engine(dofs, lin_tol, solver.max_iter, solver.check_every, "gather", g=dofs.g)
        fixed = dofs.is_bc.bool()
        real = torch.arange(Bp, device=dev) < B

        F_ext = torch.zeros((dofs.n, Bp), dtype=torch.float64, device=dev)
        if call_in.f is not None:
            F_ext += self._apply_load_map(self._body_force(call_in.f))
        if call_in.load is not None:
            F_ext += self._to_dofs(call_in.load, call.load_batched)
        F_ext[fixed] = 0.0
        F_ext[:, B:] = 0.0
        # the rounding of Pi the Armijo test allows for (module docstring)
        vol = self.plan.gradient_table()[1]
        stiff = (vol.unsqueeze(1) * torch.as_strided(kdev, (self.plan.m, Bp), (kse, ksb))).sum(0)
        slack_scale = 2.0 * self.plan.dim * setup.mu1 * stiff

        if self.x0 is not None:
            u = self._to_dofs(self.x0, self.x0.dim() == 3).clone()
            u[:, B:] = 0.0
        else:
            u = torch.zeros((dofs.n, Bp), dtype=torch.float64, device=dev)
        gcol = (dofs.g * fixed).unsqueeze(1)

        newton_its, backtracks, lin_its, lin_bad = [], 0, 0, 0
        relres_rows, alpha_rows = [], []
        failed = torch.zeros(Bp, dtype=torch.bool, device=dev)      # exhausted max_backtracks
        done = relres = vals = hier = None
        for step in range(1, solver.steps + 1):
            t = step / solver.steps
            F_t = F_ext if step == solver.steps else t * F_ext
            u[:, :B] = torch.where(fixed.unsqueeze(1), t * gcol, u[:, :B])
            f_norm = torch.linalg.vector_norm(F_t, dim=0)
            ref, its = None, 0
            while True:
                r = self._residual(u) - F_t
                r[fixed] = 0.0
                r_norm = torch.linalg.vector_norm(r, dim=0)
                if ref is None:
                    ref = torch.where(f_norm > 0.0, f_norm, r_norm)
                done = (r_norm <= solver.newton_tol * ref) | ~real
                relres = torch.where(ref > 0.0, r_norm / ref, r_norm)
                active = ~done & ~failed
                relres_rows.append(relres[:B])
                if its >= solver.max_newton or not bool(active.any()):
                    alpha_rows.append(torch.zeros_like(relres[:B]))
                    break
                vals = hier = None              # the previous tangent and its Galerkin levels go before the next come
                vals = self._tangent(u)
                hier, _ = self._hierarchy(lin, vals, info)
                rhs = torch.where(active.unsqueeze(0), -r, torch.zeros_like(r))
                res = lin.amg_pcg(hier, rhs, Bp, Bp, self.amg) if hier is not None else lin.cg(vals, rhs, Bp, Bp)
                delta = torch.where(active.unsqueeze(0), res.x, torch.zeros_like(r))     # frozen samples: exactly 0
                its, lin_its, lin_bad = its + 1, lin_its + res.iterations, lin_bad + res.not_converged
                # per-sample backtracking on Pi(u) = W(u) - F_t . u
                w0, _ = self._energy(u)
                work0 = (F_t * u).sum(0)
                slope = (r * delta).sum(0)
                slack = 16.0 * _EPS * (w0.abs() + work0.abs() + torch.sqrt(slack_scale * w0.abs()))
                alpha = active.to(torch.float64)
                for trial in range(solver.max_backtracks + 1):
                    u_try = u + alpha.unsqueeze(0) * delta
                    w1, _ = self._energy(u_try)
                    ok = (w1 - (F_t * u_try).sum(0)) <= (w0 - work0) + ARMIJO_C * alpha * slope + slack
                    need = active & ~ok & (alpha > 0.0)
                    if bool(need.any()):        # rounding may hide the decrease of Pi: the residual decides there
                        r_try = self._residual(u_try) - F_t
                        r_try[fixed] = 0.0
                        shrinks = torch.linalg.vector_norm(r_try, dim=0) <= (1.0 - ARMIJO_C * alpha) * r_norm
                        need &= ~(shrinks & torch.isfinite(w1))
                    n_need = int(need.sum())
                    if n_need == 0:
                        break
                    if trial == solver.max_backtracks:
                        failed |= need
                        alpha = torch.where(need, torch.zeros_like(alpha), alpha)
                        u_try = u + alpha.unsqueeze(0) * delta
                        break
                    backtracks += n_need
                    alpha = torch.where(need, 0.5 * alpha, alpha)
                u = u_try
                alpha_rows.append(alpha[:B])
            newton_its.append(its)

        # the state the adjoint reads: the tangent and its hierarchy at the returned u
        vals = hier = None
        vals = self._tangent(u)
        self.hier, self.bounds = self._hierarchy(self.eng, vals, info)
        self.vals, self.x = vals, u
        _, min_j = self._energy(u)
        bad = int((~done).sum())
        info.newton_iterations, info.newton_not_converged = tuple(newton_its), bad
        info.max_newton_relres = info.max_relres = float(relres[:B].max())
        info.backtracks, info.min_J = backtracks, float(min_j[:B].min())
        info.linear_iterations = info.iterations = lin_its
        info.not_converged, info.jacobi_bounds = lin_bad, self.bounds
        info.relres_history, info.alpha_history = torch.stack(relres_rows).cpu(), torch.stack(alpha_rows).cpu()
        if bad:
            n_failed = int((failed & ~done).sum())
            warnings.warn(f"diffhe: {bad} of {B} Newton solves did not reach newton_tol={solver.newton_tol:g} in "
                          f"{solver.max_newton} iterations per load step ({n_failed} of them exhausted "
                          f"{solver.max_backtracks} backtracks; max relative residual {info.max_newton_relres:.2e}, "
                          f"path {info.path})", RuntimeWarning)
        return self._from_dofs(u)


# ---------------------------------------------------------------------------------------------
# torch.library custom ops diffhe::hyperelastic_solve / diffhe::hyperelastic_solve_backward, on the shared plumbing of
# diffhe::elastic_solve (diffhe.elastic): the solver and the state of the call travel as integer handles.  f / load / x0:
# empty tensor = absent.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("diffhe::hyperelastic_solve", mutates_args=())
def hyperelastic_solve(E: torch.Tensor, f: torch.Tensor, load: torch.Tensor, x0: torch.Tensor, handle: int, save: bool,
                       node_major: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u, token) of the `HyperelasticFESolver` registered under `handle`; `token` names the saved adjoint state (0 when
    `save` is false)."""
    solver = _SOLVERS[handle]

    def prepare(state):
        state.x0 = x0.detach() if x0.numel() else None

    return _solve_result(*_solve_call(solver, _HyperSolve, E, f, load, node_major,
                                      hierarchy=(solver.nu, solver.plane), prepare=prepare), save)


@hyperelastic_solve.register_fake
def _hyperelastic_solve_fake(E, f, load, x0, handle, save, node_major):
    return _solve_fake(_SOLVERS[handle], E, f, load, node_major)


@torch.library.custom_op("diffhe::hyperelastic_solve_backward", mutates_args=())
def hyperelastic_solve_backward(gbar: torch.Tensor, token: torch.Tensor, need_e: bool, need_f: bool, need_load: bool,
                                e_like: torch.Tensor, f_like: torch.Tensor,
                                load_like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dL/dE, dL/df, dL/dload) of the forward call named by `token` from ONE adjoint solve with the final tangent;
    unused ones come back empty."""
    _, grads = _run_adjoint(gbar, token, need_e, need_f, need_load)
    return _like_grads(gbar, grads, (e_like, f_like, load_like))


@hyperelastic_solve_backward.register_fake
def _hyperelastic_solve_backward_fake(gbar, token, need_e, need_f, need_load, e_like, f_like, load_like):
    return _fake_grads(gbar, (need_e, need_f, need_load), (e_like, f_like, load_like))


_setup_context, _backward = _solve_autograd(
    "hyperelastic_solve", 3, 7, "diffhe: second-order derivatives of a hyperelastic solve are not implemented (backward "
    "with create_graph=True, diffhe.hyperelastic)")


# ---------------------------------------------------------------------------------------------
# The public solver
# ---------------------------------------------------------------------------------------------
class HyperelasticFESolver(_ElasticOptions):
    """Displacement of a compressible Neo-Hookean body at finite strain per sample, differentiable with respect to the
    Young's modulus E per element, the body force f and the nodal load (see the module docstring).

    Parameters
    ----------
    mesh : FEMesh -- P1 triangles (plane strain) or P1 tetrahedra.
    E : float or tensor or Parameter -- (), (B,), (m,), (B, m); (m, B) with layout="node".  May require grad.
    nu : float, -1 < nu < 0.5.
    fixed : None (clamp the nodes of mesh.dirichlet_nodes) or {(node, component): value}.
    device, tol, max_iter, method ("auto" or "ell-jacobi"), amg, check_every : as on `ElasticFESolver`; `tol` is the
        tolerance of the adjoint's linear solve and, unless `linear_tol` is given, of Newton's.
    newton_tol : relative residual of the stop rule.  max_newton : tangent solves per load step.
    steps : equal load increments.  max_backtracks : halvings of the step per iteration.
    linear_tol : tolerance of Newton's linear solves (an inexact Newton method); None: `tol`.
    plane : None or "strain" (2D meshes); "stress" is not implemented.
    """

    _refusal_scope = "for finite-strain elasticity"

    def __init__(self, mesh, E=1.0, nu: float = 0.3, *, fixed=None, device=None, tol: Optional[float] = None,
                 max_iter: int = 20000, method: str = "auto", amg: Optional[dict] = None, check_every: int = 25,
                 newton_tol: float = 1e-8, max_newton: int = 25, steps: int = 1, max_backtracks: int = 10,
                 linear_tol: Optional[float] = None, plane: Optional[str] = None):
        super().__init__()
        _check_mesh(mesh, "diffhe: finite-strain elasticity needs a 2D or 3D mesh (a 1D bar has no Neo-Hookean solver "
                          "here)",
                    "diffhe: finite-strain elasticity is implemented for P1 elements only (this mesh has {k} nodes per "
                    "element)")
        if plane == "stress":
            raise NotImplementedError("diffhe: plane=\"stress\" is not implemented for finite-strain elasticity (it "
                                      "needs a local solve for F33 per element); 2D meshes are solved in plane strain")
        if plane not in (None, "strain") or (mesh.dim == 3 and plane is not None):
            raise ValueError(f"plane= is None or \"strain\", on 2D meshes only; got {plane!r}")
        self.plane = None if mesh.dim == 3 else "strain"
        self.nu = float(nu)
        self._lam1, self._mu1 = lame_unit(self.nu, mesh.dim, self.plane)
        self._init_options(mesh, fixed, device, tol, max_iter, method, amg, check_every, "unit-E operator")
        if not (float(newton_tol) > 0.0 and math.isfinite(float(newton_tol))):
            raise ValueError(f"newton_tol must be positive, got {newton_tol!r}")
        if int(max_newton) < 1 or int(steps) < 1 or int(max_backtracks) < 0:
            raise ValueError("max_newton and steps must be at least 1, max_backtracks at least 0")
        if linear_tol is not None and not float(linear_tol) > 0.0:
            raise ValueError(f"linear_tol must be positive, got {linear_tol!r}")
        self.newton_tol, self.max_newton, self.steps = float(newton_tol), int(max_newton), int(steps)
        self.max_backtracks, self.linear_tol = int(max_backtracks), linear_tol
        self._E = torch.tensor(float(E), dtype=torch.float64) if isinstance(E, (int, float)) else E.to(dtype=torch.float64)
        self.last_info = HyperInfo()

    @property
    def E(self) -> torch.Tensor:
        return self._E

    def forward(self, f: Optional[torch.Tensor] = None, load: Optional[torch.Tensor] = None, layout: str = "sample",
                x0: Optional[torch.Tensor] = None, dirichlet=None, h=None, u_inf=None, flux=None,
                eigenstrain=None) -> torch.Tensor:
        """u for the dead body force f and the dead nodal load: (n, d), (B, n, d), or (n, d, B) with layout="node" -- the
        shape of the right-hand side.  f None: zero.  x0: the start of Newton's iteration in the shape of u (its values
        on fixed dofs are replaced by the prescribed ones); it is not differentiated."""
        if eigenstrain is not None:
            raise NotImplementedError("diffhe: eigenstrain= is not implemented for finite-strain elasticity (an initial "
                                      "strain enters F multiplicatively there)")
        E = self._E
        f_in, load_in, node = self._rhs_inputs(E, f, load, layout, dirichlet=dirichlet, h=h, u_inf=u_inf, flux=flux)
        B_rhs = _batch_of(self, f_in, load_in, node)[0]
        _, B, _ = _kappa_layout(E, self.mesh.n_elements, B_rhs, node)
        x0_in = E.new_empty(0)
        if x0 is not None:
            x0_in = self._checked(x0, "x0", layout).detach()
            if x0_in.dim() == 3 and x0_in.shape[2 if node else 0] != B:
                raise ValueError(f"x0 batch {x0_in.shape[2 if node else 0]} does not match the batch {B}")
        _SOLVERS[id(self)] = self
        save = torch.is_grad_enabled() and (E.requires_grad or f_in.requires_grad or load_in.requires_grad)
        u, _token = torch.ops.diffhe.hyperelastic_solve(E, f_in, load_in, x0_in, id(self), save, node)
        return u

    # -- stress recovery: the Cauchy stress (diffhe.hyper_stress) ---------------------------------------
    def _cauchy_op(self, u, E, layout: str, want_sigma: bool, want_vm: bool, want_w: bool):
        n, d = self.mesh.n_nodes, self.mesh.dim
        if layout not in ("sample", "node"):
            raise ValueError(f"Unknown layout: {layout!r}")
        u = u if isinstance(u, torch.Tensor) else torch.as_tensor(u)
        if layout == "node":
            if u.dim() != 3 or tuple(u.shape[:2]) != (n, d):
                raise ValueError(f"layout='node': u must be (n, d, B) with n={n}, d={d}, got {tuple(u.shape)}")
        elif u.dim() not in (2, 3) or tuple(u.shape[-2:]) != (n, d):
            raise ValueError(f"u must be (n, d) or (B, n, d) with n={n}, d={d}, got {tuple(u.shape)}")
        if E is None:
            E = self._E
        elif not isinstance(E, torch.Tensor):
            E = torch.as_tensor(E, dtype=torch.float64)
        self._refuse_moving_nodes("stress", False)
        u, E, node = u.to(torch.float64), E.to(torch.float64), layout == "node"
        _kappa_layout(E, self.mesh.n_elements, _stress_batch(u, node), node)       # the refusals, before the op
        _SOLVERS[id(self)] = self
        return torch.ops.diffhe.hyper_stress(u, E, id(self), node, want_sigma, want_vm, want_w)

    def cauchy_stress(self, u: torch.Tensor, E=None, layout: str = "sample") -> torch.Tensor:
        """Cauchy (true) stresses sigma = E (1/J) [mu1 (F F^T - I) + lam1 ln J I] of the displacement u -- (n, d),
        (B, n, d), or (n, d, B) with layout="node", what `forward` returns -- in Voigt components (xx, yy, xy | xx, yy, zz,
        yz, xz, xy; shear components are tensor components): (m, nc), (B, m, nc), or (m, nc, B) with layout="node".  E:
        None for the solver's, or another modulus in any layout E takes (the relaxed stress of stress-constrained design);
        an unbatched u is broadcast to the batch of E.  u and E may require grad.  An element with det F <= 0 gets NaN."""
        return self._cauchy_op(u, E, layout, True, False, False)[0]

    def cauchy_von_mises(self, u: torch.Tensor, E=None, layout: str = "sample") -> torch.Tensor:
        """The von Mises stress of the Cauchy stress per element, (m,), (B, m), or (m, B) with layout="node"; in 2D it
        includes the out-of-plane sigma_zz = E lam1 ln J / J of plane strain.  No stress array is formed.  Its derivative
        is defined as 0 where the stress vanishes.  Arguments as `cauchy_stress`."""
        return self._cauchy_op(u, E, layout, False, True, False)[1]

    def cauchy_stress_and_von_mises(self, u: torch.Tensor, E=None,
                                    layout: str = "sample") -> Tuple[torch.Tensor, torch.Tensor]:
        """(`cauchy_stress`, `cauchy_von_mises`) from one pass over the elements, and one backward pass for both."""
        return self._cauchy_op(u, E, layout, True, True, False)[:2]

    def energy_density(self, u: torch.Tensor, E=None, layout: str = "sample") -> torch.Tensor:
        """The strain energy per reference volume w = E W1(F) per element, in the shape of `cauchy_von_mises`: the sum of
        vol_e w_e is the energy the Newton iteration minimises.  Arguments as `cauchy_stress`."""
        return self._cauchy_op(u, E, layout, False, False, True)[2]

    # -- what exists for small strains only -------------------------------------------------------------
    def _no_stress(self, *args, **kwargs):
        raise NotImplementedError("diffhe: stress recovery is not implemented for finite-strain elasticity by these "
                                  "methods (stress, von_mises and stress_and_von_mises evaluate the small-strain stress: "
                                  "diffhe.elastic.ElasticFESolver); the Cauchy stress of the deformed body is "
                                  "cauchy_stress, cauchy_von_mises and cauchy_stress_and_von_mises")

    stress = von_mises = stress_and_von_mises = _no_stress

    def modes(self, *args, **kwargs):
        raise NotImplementedError("diffhe: vibration modes are not implemented for finite-strain elasticity "
                                  "(diffhe.modal.ElasticEigenSolver linearises about the undeformed body)")
