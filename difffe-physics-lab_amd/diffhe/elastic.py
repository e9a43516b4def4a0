"""Linear elasticity per sample with dL/dE (ours: the reference solves scalar equations only).

`ElasticFESolver(mesh, E, nu)` solves -div sigma(u) = f, sigma = 2 mu eps(u) + lambda tr eps(u) I, for the displacement
u of a linear-elastic body on P1 triangles (d = 2) and P1 tetrahedra (d = 3), with a Young's modulus E per element and
sample that may require grad:

    mu = E / (2 (1 + nu)),   lambda = E nu / ((1 + nu)(1 - 2 nu))   in 3D and for plane="strain",
                             lambda = E nu / (1 - nu^2)             for plane="stress" (2D, the default).

nu is a Python float with -1 < nu < 0.5 (ValueError otherwise), not differentiated.  K(E) = sum_e E_e K_e0(nu) is linear
in E exactly as the scalar operator is linear in kappa, so the layouts, the explicit adjoint and the gradient story of
`DifferentiableFESolver` carry over: ONE adjoint solve gives dL/dE, dL/df and dL/dload.

Layouts.  E: (), (B,), (m,), (B, m), and (m, B) with layout="node" -- resolved by `solver._kappa_layout`, so the (B,) /
(m,) rule is the scalar solver's; the gradient comes back in the shape of E, and a field shared by the batch gets its
gradient summed over the batch inside the kernel, in a fixed order.  f (a nodal body-force density, None = zero) and
load (a nodal force vector: point loads; tractions, pressure and elastic foundations on boundary facets are
`diffhe.elastic_facets.TractionElasticFESolver`'s, which integrates them) are (n, d) or (B, n, d), with layout="node"
(n, d, B); u has the shape of the right-hand side.  F_a = M f_a + load_a per component a with the load map M of the
scalar solvers (`plan.Mvals`).  dL/dload = lambda and dL/df = M lambda with the adjoint lambda, which vanishes on fixed
dofs: dL/dload is zero there, and a fixed dof's f still reaches its free neighbours through M.

Dirichlet data per component: `fixed=None` clamps every node of `mesh.dirichlet_nodes` in all d components at zero
(non-zero values there are temperatures and raise ValueError); otherwise `fixed` maps (node, component) -> value: a
roller is one component, non-zero prescribed displacements go through the lift.  A rigid-body mode left free is the
caller's error and surfaces as the non-convergence warning.

Degrees of freedom: dof(i, a) = i d + a; device vectors are (n d, Bp), batch innermost: the contiguous node-major
(n, d, Bp).  The operator is stored as ELL rows of width d W in the pattern of include/diffhe_elastic.h, derived from
the plan's UNPRUNED node pattern (the Lame term fills couplings that vanish for a scalar kappa), assembled and
differentiated by csrc/elastic.hip (fp64, no atomics, bitwise reproducible) and solved by the generic entries of the
general path: aggregation-multigrid PCG ("ell-amgpcg"), or Jacobi PCG with method="ell-jacobi" ("ell-pcg") -- always
the general path, also on `FEMesh.rectangle` connectivity.  The hierarchy aggregates NODES and expands the aggregates
per component (`amg.build_hierarchy_blocks`): no aggregate mixes components, the tentative prolongation carries the d
translations exactly.  It is built from the unit-E operator and cached per (plan, nu, plane, fixed set); every level
carries `amg.jacobi_bound` of its unit operator for the cycle's Jacobi weights (elastic operators have positive
off-diagonals).  The coarse space has no rotations ("Elasticity").

Stress recovery and eigenstrain (`solver.stress`, `von_mises`, `stress_and_von_mises`, `eigenstrain_load`,
`solver(f, load, eigenstrain=eps0)`, `pnorm`, `thermal_strain`, `element_mean`): `diffhe.elastic_stress` holds their ops,
conventions and layouts; this module re-exports its public names.

Node gradients (mesh.nodes requiring grad): `diffhe.elastic_shape.ShapeElasticFESolver`, this class with dL/dX of the
solve and of the stress methods; `ElasticFESolver` itself refuses moving nodes.

The call pipeline of the elastic family lives here once ("Elasticity"): `_ElasticSolve` with the only
`forward` and `adjoint` and the hooks its subclasses override (diffhe.elastic_shape, elastic_aniso, elastic_facets);
`_select_hierarchy`, the hierarchy choice of the solves and of diffhe.modal; `_solve_call`, the one call builder;
`_solve_result`, `_solve_fake`, `_run_adjoint` and `_solve_autograd`, the plumbing of the four solve ops; and
`_ElasticOptions`, `_check_mesh`, `_amg_options`, the construction and argument checking the public solvers share.

Not implemented (NotImplementedError): 1D meshes, P2 meshes, backward with create_graph=True, a per-call `dirichlet=`,
Robin / flux data (h=, u_inf=, flux=: surface tractions, pressure and elastic foundations are `traction=`, `pressure=`,
`k_normal=`, `k_tangent=` of `diffhe.elastic_facets.TractionElasticFESolver`); `amg=dict(strength=...)`.
"""
from __future__ import annotations

import math
import threading
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _hip
from .elastic_stress import (_EigenCall, _StressCall, _eigen_batch, _eigen_call, _stress_adjoint,  # noqa: F401
                             _stress_backward, _stress_batch, _stress_call, _stress_eigen_backward,
                             _stress_eigen_setup_context, _stress_forward, _stress_setup_context, _stress_shapes,
                             eigen_components, eigenstrain_load_backward, eigenstrain_load_op, elastic_stress,
                             elastic_stress_backward, elastic_stress_eigen, elastic_stress_eigen_backward, element_mean,
                             pnorm, thermal_strain)    # the names this module held before they moved: they keep resolving
from .plan import get_plan, padded_batch, valid_batch_pad, _stream
from .solver import (SolveInfo, _Engine, _SOLVERS, _call_options, _kappa_grad, _kappa_layout, _like_grads, _fake_grads,
                     _register_state, _resolve_device, _run_call, _state_of, _tie_state)

__all__ = ("ElasticFESolver", "lame_unit", "parse_fixed", "dof_pattern", "pnorm", "thermal_strain", "element_mean",
           "eigen_components")


# ---------------------------------------------------------------------------------------------
# Host logic (numpy; no device, no library)
# ---------------------------------------------------------------------------------------------
def lame_unit(nu: float, dim: int, plane: Optional[str] = None) -> Tuple[float, float]:
    """(lambda', mu') of E = 1: mu' = 1 / (2 (1 + nu)); lambda' = nu / ((1 + nu)(1 - 2 nu)) in 3D and plane strain,
    nu / (1 - nu^2) in plane stress."""
    nu = float(nu)
    if not (-1.0 < nu < 0.5):
        raise ValueError(f"nu must satisfy -1 < nu < 0.5, got {nu!r}")
    if dim == 3 or plane == "strain":
        lam = nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    elif plane == "stress":
        lam = nu / (1.0 - nu * nu)
    else:
        raise ValueError(f"Unknown plane: {plane!r} (\"stress\" or \"strain\")")
    return lam, 1.0 / (2.0 * (1.0 + nu))


def parse_fixed(mesh, fixed=None) -> Tuple[np.ndarray, np.ndarray]:
    """-> (is_bc (n d,) uint8, g (n d,) float64) per dof.  None: every node of `mesh.dirichlet_nodes` clamped in all d
    components at zero; otherwise a mapping {(node, component): value}."""
    n, d = mesh.n_nodes, mesh.dim
    is_bc = np.zeros(n * d, dtype=np.uint8)
    g = np.zeros(n * d, dtype=np.float64)
    if fixed is None:
        bc = mesh.dirichlet_nodes
        if any(float(v) != 0.0 for v in bc.values()):
            raise ValueError("diffhe: mesh.dirichlet_nodes carries non-zero values; they are temperatures and mean "
                             "nothing for a displacement -- give the prescribed displacements per component with fixed=")
        if bc:
            idx = np.fromiter(bc.keys(), dtype=np.int64, count=len(bc))
            if idx.min() < 0 or idx.max() >= n:
                raise ValueError(f"mesh.dirichlet_nodes: node ids must lie in [0, {n})")
            is_bc.reshape(n, d)[idx] = 1
        return is_bc, g
    if not hasattr(fixed, "items"):
        raise ValueError("fixed= must be a mapping {(node, component): value}")
    for key, value in fixed.items():
        try:
            node, comp = key
            node, comp = int(node), int(comp)
        except (TypeError, ValueError):
            raise ValueError(f"fixed=: keys are (node, component) pairs, got {key!r}") from None
        if not 0 <= node < n:
            raise ValueError(f"fixed=: node {node} out of range [0, {n})")
        if not 0 <= comp < d:
            raise ValueError(f"fixed=: component {comp} out of range [0, {d}) on a {d}D mesh")
        value = float(value)
        if not math.isfinite(value):
            raise ValueError(f"fixed=: value of {key!r} is not finite")
        is_bc[node * d + comp] = 1
        g[node * d + comp] = value
    return is_bc, g


def dof_pattern(node_cols: np.ndarray, d: int) -> np.ndarray:
    """The dof ELL pattern (d W, n d) int32 of include/diffhe_elastic.h from the node pattern (W, n): row (i, a), slot
    s < d -> column (i, (a + s) mod d), the node's own block rotated so that slot 0 is the diagonal; slot k d + b, k >= 1
    -> column (node_cols[k, i], b); the d slots of an unused node slot point at the row itself."""
    W, n = node_cols.shape
    rows = np.arange(n * d, dtype=np.int64)
    i, a = rows // d, rows % d
    out = np.empty((d * W, n * d), dtype=np.int64)
    for s in range(d):
        out[s] = i * d + (a + s) % d
    for k in range(1, W):
        j = node_cols[k].astype(np.int64)[i]
        for b in range(d):
            out[k * d + b] = np.where(j == i, rows, j * d + b)
    if n * d * d * W >= 2 ** 31:
        raise ValueError("mesh too large for int32 dof entries")
    return out.astype(np.int32)


# ---------------------------------------------------------------------------------------------
# Per (plan, nu, plane, fixed set): the dof system and its hierarchy
# ---------------------------------------------------------------------------------------------
class _DofSystem:
    """What `_Engine` reads of a plan, for the n d dofs: its solve and layout helpers are generic in (n, W, cols)."""

    def __init__(self, plan, cols, is_bc, g):
        self.device, self.dim, self.m = plan.device, plan.dim, plan.m
        self.n, self.W, self.cols, self.is_bc, self.g = plan.n * plan.dim, plan.W * plan.dim, cols, is_bc, g


class _ElasticSetup:
    """The dof system of one (plan, nu, plane, fixed set) and the hierarchy of its unit-E operator, built on first use."""

    def __init__(self, plan, lam1, mu1, is_bc: np.ndarray, g: np.ndarray):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(plan.device)  # noqa: E731
        plan.ensure_ell()
        self.plan, self.lam1, self.mu1 = plan, float(lam1), float(mu1)
        self.cols_host = dof_pattern(plan.cols.cpu().numpy(), plan.dim)
        self.is_bc_host = is_bc
        self.dofs = _DofSystem(plan, dev(self.cols_host), dev(is_bc), dev(g))
        self.has_data = bool(np.any(g != 0.0))
        self.free = ~self.dofs.is_bc.bool()
        self._lock = threading.Lock()
        self._levels = None

    def assemble(self, kdev, kse, ksb, Bv):
        """vals (d W, n d, Bv), lift (n d, Bv) of the block row-gather assembly (csrc/elastic.hip)."""
        plan, dofs = self.plan, self.dofs
        gtab, vol = plan.gradient_table()
        vals = torch.empty((dofs.W, dofs.n, Bv), dtype=torch.float64, device=plan.device)
        lift = torch.empty((dofs.n, Bv), dtype=torch.float64, device=plan.device)
        _hip.lib().diffhe_elast_assemble_rows(gtab, vol, plan.dim, self.lam1, self.mu1, kdev, kse, ksb, plan.ent_ptr,
                                              plan.contrib, plan.cols, dofs.is_bc, dofs.g, vals, lift, plan.n, plan.m,
                                              plan.W, Bv, _stream(plan.device))
        return vals, lift

    def levels(self):
        """(device level dicts, (levels with the fine one, operator complexity)) of the unit-E hierarchy."""
        with self._lock:
            if self._levels is None:
                from .amg import build_hierarchy_blocks, hierarchy_stats
                one = torch.ones(1, dtype=torch.float64, device=self.plan.device)
                unit, _ = self.assemble(one, 0, 0, 1)
                host = build_hierarchy_blocks(self.cols_host, unit.reshape(self.dofs.W, self.dofs.n).cpu().numpy(),
                                              self.is_bc_host, self.plan.dim)
                self._levels = ([self.plan.upload_amg_level(lv, True) for lv in host],
                                hierarchy_stats(self.cols_host, host))
            return self._levels


def _setup_of(plan, nu, plane, lam1, mu1, is_bc, g) -> _ElasticSetup:
    key = (float(nu), plane, is_bc.tobytes(), g.tobytes())
    with plan._build_lock:
        cache = plan.__dict__.setdefault("_elastic_setups", {})
        if key not in cache:
            while len(cache) >= 4:
                cache.pop(next(iter(cache)))
            cache[key] = _ElasticSetup(plan, lam1, mu1, is_bc, g)
        return cache[key]


def _cycle_defaults(amg: dict, n_dofs: int, Bp: int) -> dict:
    """`amg` with the cycle options the caller left open filled in (in place): the Jacobi scale of elastic operators and
    a W-cycle from 12 M unknowns of the batch on.  Shared with `diffhe.modal`, whose inner solves run the same cycle."""
    if amg.get("scale") is None:
        amg["scale"] = 1.3
    if amg.get("gamma") is None:
        amg["gamma"] = 2 if n_dofs * Bp >= 12_000_000 else 1
    return amg


def _measure_row_bounds(eng: _Engine, hier, Bv: int, error: str) -> Tuple[float, ...]:
    """The row bound (diffhe_ell_jacobi_row_bound) of every level of the hierarchy `hier` of one call, written over the
    levels' recorded bounds (thousandths, rounded up: diffhe_amg_level.reserved).  ONE device synchronisation: the copy
    of the n_levels doubles.  A bound that is not finite raises ValueError(error).  For the calls whose operator is not a
    positive combination of the unit-E element matrices (diffhe.elastic_aniso, diffhe.elastic_facets)."""
    arr, chain = hier
    dev, st = eng.p.device, _stream(eng.p.device)
    part = torch.empty(_hip.ROW_BOUND_BLOCKS, dtype=torch.float64, device=dev)
    out = torch.empty(len(chain), dtype=torch.float64, device=dev)
    for l, lv in enumerate(chain):
        eng.L.diffhe_ell_jacobi_row_bound(lv["vals"], lv["cols"], lv["n"], lv["W"], Bv, part, out[l:], st)
    bounds = tuple(out.cpu().tolist())
    if not all(math.isfinite(b) for b in bounds):
        raise ValueError(error)
    for l, b in enumerate(bounds):
        arr[l].reserved = int(math.ceil(1000.0 * b))
    return bounds


def _select_hierarchy(eng: _Engine, setup: _ElasticSetup, method: str, amg: dict, vals, Bv: int, Bp: int, info: SolveInfo,
                      bounds_error: Optional[str] = None):
    """The hierarchy choice of every elastic solve and of `diffhe.modal`'s inner solves: -> (hier or None, bounds).  With
    method "ell-jacobi", or a mesh too small for a second level, None and `info.path` "ell-pcg"; otherwise the Galerkin
    operators of `vals` on the cached unit-E levels (`amg` gets its cycle defaults in place), `info.path` "ell-amgpcg"
    and the hierarchy fields of `info`.  bounds_error: the smoother's row bounds are measured on every level
    (`_measure_row_bounds`, which raises ValueError with this text) and `info.hierarchy` reads "unit+row-bounds"."""
    hier, bounds = None, ()
    if method != "ell-jacobi":
        levels, stats = setup.levels()
        if levels:
            _cycle_defaults(amg, setup.dofs.n, Bp)
            hier = eng.amg_setup(vals, Bv, bool(amg.get("fp32", 0)), levels)
            info.hierarchy, info.hierarchy_levels, info.operator_complexity = "unit", stats[0], stats[1]
            if bounds_error is not None:
                bounds = _measure_row_bounds(eng, hier, Bv, bounds_error)
                info.hierarchy = "unit+row-bounds"
    info.path = "ell-amgpcg" if hier is not None else "ell-pcg"
    return hier, bounds


# ---------------------------------------------------------------------------------------------
# One call
# ---------------------------------------------------------------------------------------------
@dataclass
class _ElasticCall:
    """The facts of one call `_run_call` and the adjoint read (none of the input tensors)."""
    B: int
    mode: int
    kappa_em: bool
    batched: bool
    node_major: bool
    out_device: torch.device
    e_shape: torch.Size
    e_device: torch.device
    f_batched: bool
    load_batched: bool


class _ElasticSolve:
    """One call's solve: forward() keeps what adjoint() needs -- the assembled operator, the hierarchy, the iterate -- and
    this object is the adjoint state the custom ops hold until the end of backward.  The ONE `forward` and the ONE
    `adjoint` of the elastic family; a solver path subclasses this and overrides the hooks `_operator`, `_body_force`,
    `_after_rhs`, `_coeff_grad` and the class attributes below, nothing else."""
    Info = SolveInfo                        # the class of `solver.last_info` after a call of this path
    bounds_error: Optional[str] = None      # set: the smoother's row bounds are measured per call; the ValueError's text
    bounds: Tuple[float, ...] = ()          # what was measured, the fine level first
    keep_lambda = False                     # the adjoint lambda stays in `lam` for what the op computes after `adjoint`
    lam = None

    def __init__(self, solver, setup: _ElasticSetup, call: _ElasticCall, tol: float, amg: dict):
        self.solver, self.setup, self.call, self.amg = solver, setup, call, amg
        self.plan = setup.plan
        self.eng = _Engine(setup.dofs, tol, solver.max_iter, solver.check_every, "gather", g=setup.dofs.g)
        self.node_eng = _Engine(self.plan, tol, solver.max_iter, solver.check_every, "gather")

    # -- layout -----------------------------------------------------------------------------------
    def _to_dofs(self, t: torch.Tensor, batched: bool, zero_fixed: bool = False) -> torch.Tensor:
        """(n, d) | (B, n, d) | node-major (n, d, B) -> (n d, Bp), padding samples zero."""
        call, dofs, Bp, B = self.call, self.setup.dofs, self.Bp, self.call.B
        t = t.detach().to(self.plan.device, torch.float64)
        mask = dofs.is_bc if zero_fixed else None
        if call.node_major:
            src = t.reshape(dofs.n, B)
            if Bp == B and src.is_contiguous() and not zero_fixed:
                return src
            out = torch.zeros((dofs.n, Bp), dtype=torch.float64, device=self.plan.device)
            out[:, :B] = src
            if zero_fixed:
                out[dofs.is_bc.bool()] = 0.0
            return out
        src = t.reshape(B, dofs.n).contiguous() if batched else t.reshape(dofs.n).contiguous()
        return self.eng.to_node_major(src, B, Bp, dofs.n, zero_mask=mask)

    def _from_dofs(self, x: torch.Tensor, add: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(n d, Bp) -> (B, n, d), or node-major (n, d, B); `add` (n d,) is added to every sample."""
        call, plan, B, Bp = self.call, self.plan, self.call.B, self.Bp
        if call.node_major:
            xo = x if Bp == B else x[:, :B]
            if add is not None:
                xo = xo + add.unsqueeze(1)
            return xo.reshape(plan.n, plan.dim, B)
        return self.eng.to_sample_major(x, B, Bp, self.setup.dofs.n, add=add).reshape(B, plan.n, plan.dim)

    def _apply_load_map(self, x: torch.Tensor) -> torch.Tensor:
        """y_a = M x_a per component a with the node-level load map of the plan: the (n, d, Bp) array is an (n, d Bp)
        node vector; where d Bp is no valid batch width the components go through one by one."""
        plan, Bp, d = self.plan, self.Bp, self.plan.dim
        if valid_batch_pad(d * Bp):
            return self.node_eng.load_vector(x, None, 1, d * Bp, free_rows=False).reshape(plan.n * d, Bp)
        xc = x.reshape(plan.n, d, Bp).permute(1, 0, 2).contiguous()
        yc = torch.stack([self.node_eng.load_vector(xc[a], None, 1, Bp, free_rows=False) for a in range(d)])
        return yc.permute(1, 0, 2).reshape(plan.n * d, Bp).contiguous()

    # -- hooks ------------------------------------------------------------------------------------
    def _operator(self, E: torch.Tensor):
        """-> (vals (d W, n d, Bv), lift (n d, Bv), Bv) of the call's coefficient: here the modulus as the kernels read it
        and the block row-gather assembly of csrc/elastic.hip."""
        kdev, kse, ksb, Bv = self.node_eng.kappa_device(E, self.call.mode, self.call.B, self.Bp, em=self.call.kappa_em)
        return (*self.setup.assemble(kdev, kse, ksb, Bv), Bv)

    def _body_force(self, f: torch.Tensor) -> torch.Tensor:
        """f as the dof vector (n d, Bp) the load map reads."""
        return self._to_dofs(f, self.call.f_batched)

    def _after_rhs(self, vals: torch.Tensor, rhs: torch.Tensor, Bv: int) -> None:
        """What a path adds to the stored operator and the finished right-hand side, in place: nothing here."""

    def _coeff_grad(self, lam: torch.Tensor) -> torch.Tensor:
        """dL/dE in the shape of E from the adjoint lambda and the saved iterate (`diffhe_elast_grad*`)."""
        call, setup, plan, B, Bp = self.call, self.setup, self.plan, self.call.B, self.Bp
        L, st = self.eng.L, _stream(plan.device)
        gtab, vol = plan.gradient_table()
        args = (plan.elems, gtab, vol, plan.dim, setup.lam1, setup.mu1, lam, self.x, setup.dofs.g, plan.n, plan.m)
        sums, de = self.node_eng.element_grad(
            call.mode, call.kappa_em, B, Bp, None,
            lambda de_e, osc, ose, part, total: L.diffhe_elast_grad(*args, Bp, de_e, part, total, st),
            lambda de, osc, ose: L.diffhe_elast_grad_shared(*args, B, Bp, de, st))
        return _kappa_grad(call.mode, call.e_shape, sums, de)

    # -- forward ----------------------------------------------------------------------------------
    def forward(self, call_in, info: SolveInfo) -> torch.Tensor:
        f, load = call_in.f, call_in.load
        setup, call, eng = self.setup, self.call, self.eng
        dofs, B = setup.dofs, call.B
        Bp = self.Bp = padded_batch(B)
        vals, lift, Bv = self._operator(call_in.E)
        rhs = -lift if Bv == Bp else (-lift).expand(dofs.n, Bp).contiguous()
        if f is not None:
            rhs += self._apply_load_map(self._body_force(f))
        if load is not None:
            rhs += self._to_dofs(load, call.load_batched)
        rhs[dofs.is_bc.bool()] = 0.0
        if Bp > B:
            rhs[:, B:] = 0.0
        self._after_rhs(vals, rhs, Bv)
        self.hier, self.bounds = _select_hierarchy(eng, setup, self.solver.method, self.amg, vals, Bv, Bp, info,
                                                   self.bounds_error)
        if self.bounds_error is not None:
            info.jacobi_bounds = self.bounds
        if self.hier is not None:
            x, its, bad, relres, *_ = eng.amg_pcg(self.hier, rhs, Bp, Bv, self.amg)
        else:
            x, its, bad, relres, *_ = eng.cg(vals, rhs, Bp, Bv)
        info.iterations, info.not_converged = its, bad
        info.max_relres = float(relres[:B].max())
        self.vals, self.x, self.Bv = vals, x, Bv
        return self._from_dofs(x, dofs.g if (setup.has_data or not call.node_major) else None)

    # -- adjoint ----------------------------------------------------------------------------------
    def adjoint(self, gbar: torch.Tensor, need_coeff: bool, need_f: bool, need_load: bool):
        """lambda = A^-1 gbar on the free dofs with the forward's operator, hierarchy and bounds, then the coefficient's
        gradient in its own shape (`_coeff_grad`), dL/df = M lambda and dL/dload = lambda in the caller's layout."""
        call, eng, B, Bp = self.call, self.eng, self.call.B, self.Bp
        info = self.solver.last_info
        rhs = self._to_dofs(gbar, True, zero_fixed=True)
        if self.hier is not None:
            res = eng.amg_pcg(self.hier, rhs, Bp, self.Bv, self.amg)
        else:
            res = eng.cg(self.vals, rhs, Bp, self.Bv)
        lam = res.x
        if self.keep_lambda:
            self.lam = lam
        info.adj_iterations, info.adj_max_relres = res.iterations, float(res.relres[:B].max())
        info.not_converged += res.not_converged
        grad_c = grad_f = grad_load = None
        if need_coeff:
            grad_c = self._coeff_grad(lam).to(call.e_device)
        if need_f:
            df = self._from_dofs(self._apply_load_map(lam))
            grad_f = (df if call.f_batched else df.sum(dim=0)).to(call.out_device)
        if need_load:
            dl = self._from_dofs(lam)
            dl = dl.clone() if call.node_major else dl
            grad_load = (dl if call.load_batched else dl.sum(dim=0)).to(call.out_device)
        return grad_c, grad_f, grad_load


@dataclass
class _Inputs:
    E: torch.Tensor
    f: Optional[torch.Tensor]
    load: Optional[torch.Tensor]
    B: int
    batched: bool
    node_major: bool
    out_device: torch.device


def _batch_of(solver, f: torch.Tensor, load: torch.Tensor, node_major: bool):
    """-> (B of the right-hand side or None, f batched, load batched) from the op's inputs (empty = absent)."""
    fb = f.numel() > 0 and f.dim() == 3
    lb = load.numel() > 0 and load.dim() == 3
    if node_major:
        return (f if f.numel() else load).shape[2], fb, lb
    B = f.shape[0] if fb else (load.shape[0] if lb else None)
    if fb and lb and f.shape[0] != load.shape[0]:
        raise ValueError(f"load batch {load.shape[0]} does not match f batch {f.shape[0]}")
    return B, fb, lb


def _solve_call(solver, State, coeff, f, load, node_major: bool, layout=_kappa_layout, hierarchy=None, prepare=None):
    """(u, state) of one call of any elastic solver: the ONE call builder.  State: the `_ElasticSolve` class of the path;
    coeff: E or C; layout(coeff, m, B_rhs, node_major) -> (mode, B, element-major): `_kappa_layout` or the tensor's;
    hierarchy: (nu, plane) of the unit operator whose cached hierarchy the call uses, None: the solver's own;
    prepare(state): what a path sets on the state before the solve (diffhe.elastic_facets)."""
    plan = solver._plan()
    nu, plane = hierarchy or (solver.nu, solver.plane)
    setup = _setup_of(plan, nu, plane, *lame_unit(nu, plan.dim, plane), solver._is_bc, solver._g)
    B_rhs, fb, lb = _batch_of(solver, f, load, node_major)
    mode, B, em = layout(coeff, plan.m, B_rhs, node_major)
    src = f if f.numel() else load
    call = _ElasticCall(B, mode, em, B_rhs is not None, node_major, src.device if src.numel() else coeff.device,
                        coeff.shape, coeff.device, fb, lb)
    tol, _, amg = _call_options(chain=False, lattice=False, closed_boundary=False, n=setup.dofs.n, mode=mode,
                                tol_user=solver._tol_user, mg_user=set(), mg={}, amg=solver.amg)
    solver.tol = tol
    state = State(solver, setup, call, tol, amg)
    if prepare is not None:
        prepare(state)
    u = _run_call(state, _Inputs(coeff, f if f.numel() else None, load if load.numel() else None, B, call.batched,
                                 node_major, call.out_device))
    return u, state


def _out_shape(solver, coeff, f, load, node_major, nc: int = 0):
    """The shape of u; nc: the components of a tensor coefficient, 0 for E."""
    n, d, m = solver.mesh.n_nodes, solver.mesh.dim, solver.mesh.n_elements
    B_rhs, _, _ = _batch_of(solver, f, load, node_major)
    if node_major:
        return (n, d, B_rhs)
    _, B, _ = _kappa_layout(coeff, m, B_rhs, False, nc)
    return (B, n, d) if (B_rhs is not None or B > 1) else (n, d)


# ---------------------------------------------------------------------------------------------
# What the four solve ops share (diffhe::elastic_solve here, elastic_solve_shape, elastic_aniso_solve, elastic_facet_solve
# in their modules).  The solver and the state of the call travel as integer handles through the registries of
# diffhe.solver; f / load: empty tensor = absent.  torch.library needs every op's explicit signature: the `def`s stay.
# ---------------------------------------------------------------------------------------------
def _solve_result(u: torch.Tensor, state: _ElasticSolve, save: bool):
    """What a forward op returns: u (a copy where it is a view, or the saved iterate itself) and the state's token."""
    return u.clone() if u._base is not None or u.data_ptr() == state.x.data_ptr() else u, _register_state(state, save)


def _solve_fake(solver, coeff, f, load, node_major, nc: int = 0):
    """(u, token) of a forward op's fake (meta) implementation."""
    like = f if f.numel() else (load if load.numel() else coeff)
    return (like.new_empty(_out_shape(solver, coeff, f, load, node_major, nc), dtype=torch.float64),
            torch.empty((), dtype=torch.int64))


def _run_adjoint(gbar: torch.Tensor, token: torch.Tensor, need_coeff: bool, need_f: bool, need_load: bool):
    """(state, (dL/dcoeff, dL/df, dL/dload)) of the call named by `token`: the ONE adjoint solve, for the cotangent of u
    as autograd hands it over (an unbatched call's gets its batch axis)."""
    state = _state_of(token)
    call = state.call
    g = gbar.detach()
    if not call.node_major and not call.batched and call.B == 1:
        g = g.unsqueeze(0)
    return state, state.adjoint(g, need_coeff, need_f, need_load)


def _solve_autograd(op: str, n_diff: int, n_in: int, refusal: str):
    """Register and return (setup_context, backward) of the solve op `op`, whose `n_in` inputs begin with `n_diff`
    differentiable tensors and whose backward op diffhe::<op>_backward takes (gbar, token, *needs, *those tensors).
    refusal: the text of the create_graph=True error."""
    def setup_context(ctx, inputs, output):
        _tie_state(ctx, output[1], *inputs[:n_diff])

    def backward(ctx, grad_u, _grad_token):
        if torch.is_grad_enabled():
            raise NotImplementedError(refusal)
        token, *tensors = ctx.saved_tensors[:n_diff + 1]
        needs = tuple(bool(v) for v in ctx.needs_input_grad[:n_diff])
        if not any(needs):
            return (None,) * n_in
        grads = getattr(torch.ops.diffhe, op + "_backward")(grad_u.contiguous(), token, *needs, *tensors)
        return (*(g if need else None for g, need in zip(grads, needs)), *(None,) * (n_in - n_diff))

    torch.library.register_autograd("diffhe::" + op, backward, setup_context=setup_context)
    return setup_context, backward


@torch.library.custom_op("diffhe::elastic_solve", mutates_args=())
def elastic_solve(E: torch.Tensor, f: torch.Tensor, load: torch.Tensor, handle: int, save: bool,
                  node_major: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u, token) of the `ElasticFESolver` registered under `handle`; `token` names the saved adjoint state (0 when
    `save` is false)."""
    return _solve_result(*_solve_call(_SOLVERS[handle], _ElasticSolve, E, f, load, node_major), save)


@elastic_solve.register_fake
def _elastic_solve_fake(E, f, load, handle, save, node_major):
    return _solve_fake(_SOLVERS[handle], E, f, load, node_major)


@torch.library.custom_op("diffhe::elastic_solve_backward", mutates_args=())
def elastic_solve_backward(gbar: torch.Tensor, token: torch.Tensor, need_e: bool, need_f: bool, need_load: bool,
                           e_like: torch.Tensor, f_like: torch.Tensor,
                           load_like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dL/dE, dL/df, dL/dload) of the forward call named by `token` from ONE adjoint solve; unused ones come back empty."""
    _, grads = _run_adjoint(gbar, token, need_e, need_f, need_load)
    return _like_grads(gbar, grads, (e_like, f_like, load_like))


@elastic_solve_backward.register_fake
def _elastic_solve_backward_fake(gbar, token, need_e, need_f, need_load, e_like, f_like, load_like):
    return _fake_grads(gbar, (need_e, need_f, need_load), (e_like, f_like, load_like))


_setup_context, _backward = _solve_autograd(
    "elastic_solve", 3, 6, "diffhe: second-order derivatives of an elastic solve are not implemented (backward with "
    "create_graph=True, diffhe.elastic)")


# ---------------------------------------------------------------------------------------------
# The public solvers: what `ElasticFESolver`, `AnisotropicElasticFESolver` (not an `ElasticFESolver`), through the former
# `TractionElasticFESolver` and `ShapeElasticFESolver`, and where it applies `ElasticEigenSolver` share of construction
# and argument checking.  Where the classes word a message differently the wording is a parameter.
# ---------------------------------------------------------------------------------------------
def _check_mesh(mesh, one_d: str, p1: str, dims: str = "Only 2D and 3D supported") -> None:
    """The mesh refusals (NotImplementedError): 1D (`one_d`), a dimension other than 2 and 3 (`dims`), elements other
    than P1 (`p1`, formatted with k = nodes per element)."""
    if mesh.dim == 1:
        raise NotImplementedError(one_d)
    if mesh.dim not in (2, 3):
        raise NotImplementedError(dims)
    if mesh.elements.shape[1] != mesh.dim + 1:
        raise NotImplementedError(p1.format(k=mesh.elements.shape[1]))


def _amg_options(amg: Optional[dict], strength: str,
                 smoothed: str = "diffhe: elasticity builds a smoothed-aggregation hierarchy (amg smoothed=0 is not "
                                 "implemented)") -> dict:
    """The options of the general path's aggregation-multigrid PCG, as on DifferentiableFESolver, with the caller's `amg`
    over the defaults and the two refusals (NotImplementedError with the texts `strength` and `smoothed`)."""
    out = dict(n_coarse=16, gamma=None, scale=None, fp32=0, max_iter=20000, smoothed=1)
    out.update(amg or {})
    if float(out.get("strength", 0) or 0) > 0.0:
        raise NotImplementedError(strength)
    if not out.get("smoothed", 1):
        raise NotImplementedError(smoothed)
    return out


class _ElasticOptions(nn.Module):
    """The private base of the elastic solvers: the solve options and Dirichlet data of the constructor, the plan, and
    the step from a call's (f, load, layout) to the op's inputs.  """
    _refusal_scope = "for elasticity"       # "node gradients are not implemented <scope>": the class names its coefficient
    _ONE_D = ("diffhe: elasticity needs a 2D or 3D mesh (a 1D bar is the scalar problem of DifferentiableFESolver with "
              "kappa = E A)")

    def _init_options(self, mesh, fixed, device, tol, max_iter, method, amg, check_every, hierarchy_of: str) -> None:
        """method, fixed= and the option attributes; hierarchy_of: the operator the strength refusal names."""
        if method not in ("auto", "ell", "ell-jacobi"):
            raise ValueError(f"Unknown method: {method!r}")
        self.mesh, self.method = mesh, method
        self._is_bc, self._g = parse_fixed(mesh, fixed)
        self.amg = _amg_options(amg, "diffhe: amg=dict(strength=...) is not implemented for elasticity (the hierarchy is "
                                     f"built from the {hierarchy_of})")
        self._device = device
        self._tol_user = tol
        self.tol, self.max_iter, self.check_every = tol, int(max_iter), int(check_every)

    def _plan(self):
        return get_plan(self.mesh, _resolve_device(self._device), prune=False)

    def _checked(self, t, name: str, layout: str):
        n, d = self.mesh.n_nodes, self.mesh.dim
        if t is None:
            return None
        t = t if isinstance(t, torch.Tensor) else torch.as_tensor(t)
        if layout == "node":
            if t.dim() != 3 or tuple(t.shape[:2]) != (n, d):
                raise ValueError(f"layout='node': f (and load) must be (n, d, B) with n={n}, d={d}, got {tuple(t.shape)}")
        elif t.dim() not in (2, 3) or tuple(t.shape[-2:]) != (n, d):
            raise ValueError(f"{name} must be (n, d) or (B, n, d) with n={n}, d={d}, got {tuple(t.shape)}")
        return t.to(torch.float64)

    def _moving_nodes(self) -> bool:
        return self.mesh.nodes.requires_grad and torch.is_grad_enabled()

    def _refuse_moving_nodes(self, what: str, eigenstrain: bool) -> None:
        """Moving nodes are `ShapeElasticFESolver`'s (diffhe.elastic_shape), which overrides this."""
        if self._moving_nodes():
            raise NotImplementedError(f"diffhe: node gradients are not implemented {self._refusal_scope} (mesh.nodes "
                                      "requires grad)")

    def _rhs_inputs(self, coeff: torch.Tensor, f, load, layout: str, *, dirichlet=None, h=None, u_inf=None, flux=None,
                    eigenstrain=None, eigenstrain_batch: bool = True, implied: Optional[int] = None, where=None):
        """-> (f_in, load_in, node) as the solve ops take them (empty tensor = absent; `node`: layout == "node") from the
        arguments of one `forward`: the refusals of scalar-solver data, the layout and shape checks, the eigenstrain's
        load joined to `load`, and a zero f where neither is given.  eigenstrain_batch: with layout="node" an eigenstrain
        alone may carry the batch (false: f or load must, and are checked before the load joins); implied: the batch
        that other data of the call carry (facet data), which an unbatched right-hand side is expanded to; where: the
        device of that zero f and of the default, None: the coefficient's."""
        if dirichlet is not None:
            raise NotImplementedError("diffhe: dirichlet= is not implemented for elasticity (the boundary-band kernels "
                                      "read scalar element tables); give prescribed displacements with fixed=")
        if h is not None or u_inf is not None or flux is not None:
            raise NotImplementedError("diffhe: Robin / flux data (h=, u_inf=, flux=) are not implemented for elasticity; "
                                      "integrate a traction into load=")
        if layout not in ("sample", "node"):
            raise ValueError(f"Unknown layout: {layout!r}")
        self._refuse_moving_nodes("solve", eigenstrain is not None)
        n, d, node = self.mesh.n_nodes, self.mesh.dim, layout == "node"
        where = coeff.device if where is None else where
        f64, load64 = self._checked(f, "f", layout), self._checked(load, "load", layout)
        if implied is not None and not node and not any(t is not None and t.dim() == 3 for t in (f64, load64)):
            base = f64 if f64 is not None else torch.zeros((n, d), dtype=torch.float64, device=where)
            f64 = base.reshape(1, n, d).expand(implied, n, d)
        if eigenstrain is not None and eigenstrain_batch:
            load64 = self._with_eigenstrain_load(eigenstrain, f64, load64, layout)
        if node:
            if f64 is None and load64 is None:
                raise ValueError("layout='node' needs f or load to carry the batch: (n, d, B)")
            if f64 is not None and load64 is not None and f64.shape != load64.shape:
                raise ValueError(f"layout='node': f (and load) must be (n, d, B) with one B, got {tuple(f64.shape)} and "
                                 f"{tuple(load64.shape)}")
        if eigenstrain is not None and not eigenstrain_batch:
            load64 = self._with_eigenstrain_load(eigenstrain, f64, load64, layout)
        empty = coeff.new_empty(0)
        if f64 is None and load64 is None:
            f64 = torch.zeros((n, d), dtype=torch.float64, device=where)
        return (empty if f64 is None else f64), (empty if load64 is None else load64), node



class ElasticFESolver(_ElasticOptions):
    """Displacement of a linear-elastic body per sample, differentiable with respect to the Young's modulus E per element,
    the body force f and the nodal load (see the module docstring).

    Parameters
    ----------
    mesh : FEMesh -- P1 triangles or P1 tetrahedra.
    E : float or tensor or Parameter -- (), (B,), (m,), (B, m); (m, B) with layout="node".  May require grad.
    nu : float, -1 < nu < 0.5.  plane : "stress" (default) or "strain", 2D meshes only.
    fixed : None (clamp the nodes of mesh.dirichlet_nodes) or {(node, component): value}.
    device, tol, max_iter, method ("auto" or "ell-jacobi"), amg : as on `DifferentiableFESolver`.
    """

    def __init__(self, mesh, E=1.0, nu: float = 0.3, *, plane: Optional[str] = None, fixed=None, device=None,
                 tol: Optional[float] = None, max_iter: int = 20000, method: str = "auto", amg: Optional[dict] = None,
                 check_every: int = 25):
        super().__init__()
        _check_mesh(mesh, self._ONE_D, "diffhe: elasticity is implemented for P1 elements only (this mesh has {k} nodes "
                                       "per element)")
        if mesh.dim == 3 and plane is not None:
            raise ValueError("plane= applies to 2D meshes only (a 3D body needs no plane-stress / plane-strain choice)")
        self.plane = None if mesh.dim == 3 else ("stress" if plane is None else plane)
        self.nu = float(nu)
        self._lam1, self._mu1 = lame_unit(self.nu, mesh.dim, self.plane)
        self._init_options(mesh, fixed, device, tol, max_iter, method, amg, check_every, "unit-E operator")
        self._E = torch.tensor(float(E), dtype=torch.float64) if isinstance(E, (int, float)) else E.to(dtype=torch.float64)
        self.last_info = SolveInfo()

    @property
    def E(self) -> torch.Tensor:
        return self._E

    def forward(self, f: Optional[torch.Tensor] = None, load: Optional[torch.Tensor] = None, layout: str = "sample",
                dirichlet=None, h=None, u_inf=None, flux=None, eigenstrain=None) -> torch.Tensor:
        """u for the body force f and the nodal load: (n, d), (B, n, d), or (n, d, B) with layout="node" -- the shape of
        the right-hand side.  f None: zero.  eigenstrain: an initial strain eps0 (layouts: `eigenstrain_load`), whose
        load F0(eps0, E) joins `load` in front of the unchanged solve; None takes exactly the path without it."""
        E = self._E
        f_in, load_in, node = self._rhs_inputs(E, f, load, layout, dirichlet=dirichlet, h=h, u_inf=u_inf, flux=flux,
                                               eigenstrain=eigenstrain)
        _kappa_layout(E, self.mesh.n_elements, _batch_of(self, f_in, load_in, node)[0], node)
        _SOLVERS[id(self)] = self
        return self._solve_op(E, f_in, load_in, node)

    def _solve_op(self, E: torch.Tensor, f_in: torch.Tensor, load_in: torch.Tensor, node_major: bool) -> torch.Tensor:
        save = torch.is_grad_enabled() and (E.requires_grad or f_in.requires_grad or load_in.requires_grad)
        u, _token = torch.ops.diffhe.elastic_solve(E, f_in, load_in, id(self), save, node_major)
        return u

    # -- eigenstrain ----------------------------------------------------------------------------------
    def _checked_eps0(self, eps0, layout: str) -> torch.Tensor:
        m, d = self.mesh.n_elements, self.mesh.dim
        nc0 = eigen_components(d, self.plane)
        eps0 = eps0 if isinstance(eps0, torch.Tensor) else torch.as_tensor(eps0, dtype=torch.float64)
        if layout == "node" and eps0.dim() == 3 and tuple(eps0.shape[:2]) == (nc0, m):
            return eps0.to(torch.float64)
        if eps0.dim() not in (1, 2, 3) or eps0.shape[-1] != nc0 or (eps0.dim() == 3 and eps0.shape[1] != m):
            if self.plane == "stress" and eps0.dim() >= 1 and eps0.shape[-1] == 4:
                raise ValueError("eigenstrain: plane stress takes 3 components (xx, yy, xy); a zz component has no effect "
                                 "there (it is plane strain that constrains it)")
            raise ValueError(f"eigenstrain must be ({nc0},), (B, {nc0}), ({m}, {nc0}) or (B, {m}, {nc0}) in Voigt components"
                             + (f", or ({nc0}, {m}, B) with layout='node'" if layout == "node" else "")
                             + f", got {tuple(eps0.shape)}")
        return eps0.to(torch.float64)

    def _modulus(self, E) -> torch.Tensor:
        if E is None:
            return self._E
        return (E if isinstance(E, torch.Tensor) else torch.as_tensor(E, dtype=torch.float64)).to(torch.float64)

    def _eigenstrain_load(self, eps0, E, layout: str, B_hint: Optional[int]) -> torch.Tensor:
        if layout not in ("sample", "node"):
            raise ValueError(f"Unknown layout: {layout!r}")
        self._refuse_moving_nodes("eigenstrain_load", True)
        eps0, E = self._checked_eps0(eps0, layout), self._modulus(E)
        m, nc0, node = self.mesh.n_elements, eigen_components(self.mesh.dim, self.plane), layout == "node"
        B0 = _eigen_batch(eps0, E, m, nc0, node, B_hint)                     # the refusals, before the op
        if _kappa_layout(eps0, m, B0, node, nc0)[1] != _kappa_layout(E, m, B0, node)[1]:
            raise ValueError("E batch does not match eigenstrain batch")
        _SOLVERS[id(self)] = self
        return torch.ops.diffhe.eigenstrain_load(eps0, E, id(self), node, -1 if B_hint is None else int(B_hint))

    def eigenstrain_load(self, eps0, E=None, layout: str = "sample") -> torch.Tensor:
        """The nodal load F0 = sum_e vol_e E_e B_e^T D eps0_e of an eigenstrain (initial strain: thermal expansion,
        swelling, pre-stress), as `load=` takes it: (n, d), (B, n, d), or (n, d, B) with layout="node".  eps0 in Voigt
        components -- (xx, yy, xy) in plane stress, (xx, yy, xy, zz) in plane strain, (xx, yy, zz, yz, xz, xy) in 3D, shear
        components not doubled -- as (nc0,), (B, nc0), (m, nc0), (B, m, nc0), or (nc0, m, B) with layout="node"; E: None
        for the solver's, or any layout E takes.  The batch is that of whichever shows one; an (m, nc0) or (m,) operand
        next to a batch of m reads as one value per sample, as kappa does next to f.  Differentiable in eps0 and E."""
        return self._eigenstrain_load(eps0, E, layout, None)

    def _with_eigenstrain_load(self, eps0, f64, load64, layout: str):
        """load + F0(eps0, E) for `forward`: the batch of f / load decides how eps0 reads; a load every sample shares stays
        unbatched where that layout exists."""
        node = layout == "node"
        src = f64 if f64 is not None else load64
        B_rhs = None if src is None else (src.shape[2] if node else (src.shape[0] if src.dim() == 3 else None))
        if load64 is not None and load64.dim() == 3 and not node:
            B_rhs = load64.shape[0]
        F0 = self._eigenstrain_load(eps0, None, layout, B_rhs)
        if node and src is not None and F0.shape[2] == 1 and src.shape[2] != 1:
            F0 = F0.expand(src.shape)
        return F0 if load64 is None else load64.to(F0.device) + F0

    # -- stress recovery ----------------------------------------------------------------------------
    def _stress_op(self, u, E, layout: str, want_sigma: bool, want_vm: bool, eigenstrain=None):
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
        self._refuse_moving_nodes("stress", eigenstrain is not None)
        u, E = u.to(torch.float64), E.to(torch.float64)
        if eigenstrain is not None:
            eps0 = self._checked_eps0(eigenstrain, layout)
            m, nc0, node = self.mesh.n_elements, eigen_components(self.mesh.dim, self.plane), layout == "node"
            B0 = _eigen_batch(eps0, E, m, nc0, node, _stress_batch(u, node))
            if _kappa_layout(eps0, m, B0, node, nc0)[1] != _kappa_layout(E, m, B0, node)[1]:
                raise ValueError("E batch does not match eigenstrain batch")
            _SOLVERS[id(self)] = self
            return torch.ops.diffhe.elastic_stress_eigen(u, E, eps0, id(self), node, want_sigma, want_vm)
        _kappa_layout(E, self.mesh.n_elements, _stress_batch(u, layout == "node"), layout == "node")
        _SOLVERS[id(self)] = self
        return self._stress_eval_op(u, E, layout == "node", want_sigma, want_vm)

    def _stress_eval_op(self, u: torch.Tensor, E: torch.Tensor, node_major: bool, want_sigma: bool, want_vm: bool):
        return torch.ops.diffhe.elastic_stress(u, E, id(self), node_major, want_sigma, want_vm)

    def stress(self, u: torch.Tensor, E=None, layout: str = "sample", eigenstrain=None) -> torch.Tensor:
        """Element stresses sigma = E (2 mu' eps + lambda' tr(eps) I) of the displacement u -- (n, d), (B, n, d), or
        (n, d, B) with layout="node", what `forward` returns -- in Voigt components (xx, yy, xy | xx, yy, zz, yz, xz, xy;
        shear components are tensor components): (m, nc), (B, m, nc), or (m, nc, B) with layout="node".  E: None for the
        solver's, or another modulus in any layout E takes (the relaxed stress of stress-constrained design); an
        unbatched u is broadcast to the batch of E.  eigenstrain: None, or the initial strain eps0 of the solve (layouts:
        `eigenstrain_load`): sigma = E (s(u) - s0), and in plane strain sigma_zz = E [lambda' (tr eps(u) - tr eps0) -
        2 mu' eps0_zz] enters `von_mises`.  u, E and eps0 may require grad."""
        return self._stress_op(u, E, layout, True, False, eigenstrain)[0]

    def von_mises(self, u: torch.Tensor, E=None, layout: str = "sample", eigenstrain=None) -> torch.Tensor:
        """The von Mises stress per element, (m,), (B, m), or (m, B) with layout="node"; in 2D it includes the
        out-of-plane sigma_zz (0 in plane stress, nu (sigma_xx + sigma_yy) in plane strain).  No stress array is formed.
        Its derivative is defined as 0 where the stress vanishes.  Arguments as `stress`."""
        return self._stress_op(u, E, layout, False, True, eigenstrain)[1]

    def stress_and_von_mises(self, u: torch.Tensor, E=None, layout: str = "sample",
                             eigenstrain=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(`stress`, `von_mises`) from one pass over the elements, and one backward pass for both cotangents."""
        return self._stress_op(u, E, layout, True, True, eigenstrain)
