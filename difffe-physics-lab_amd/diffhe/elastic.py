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
solve used (the relaxed stress rho^q E_0 D eps of stress-constrained SIMP); the batch rules are those of E above, and an
unbatched u with a batched E is broadcast.  The gradients come from one element pass (dL/dE, and a symmetric tensor per
element) and one node pass over the per-node incidence list (dL/du), in fixed orders: bitwise reproducible.

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

Node gradients (mesh.nodes requiring grad): `diffhe.elastic_shape.ShapeElasticFESolver`, this class with dL/dX of the
solve and of the stress methods; `ElasticFESolver` itself refuses moving nodes.

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
from .plan import get_plan, padded_batch, valid_batch_pad, _stream
from .solver import (K_ELEM, K_SAMPLE, K_SAMPLE_ELEM, K_SCALAR, SolveInfo, _Engine, _SOLVERS, _call_options, _kappa_grad,
                     _kappa_layout, _kappa_mode, _like_grads, _fake_grads, _register_state, _resolve_device, _run_call,
                     _state_of, _tensor_mode, _tie_state)

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


def _measure_row_bounds(state, Bv: int, error: str) -> Tuple[float, ...]:
    """The row bound (diffhe_ell_jacobi_row_bound) of every level of the hierarchy `state.hier` of one call, written over
    the levels' recorded bounds (thousandths, rounded up: diffhe_amg_level.reserved).  ONE device synchronisation: the
    copy of the n_levels doubles.  A bound that is not finite raises ValueError(error).  For the calls whose operator is
    not a positive combination of the unit-E element matrices (diffhe.elastic_aniso, diffhe.elastic_facets)."""
    arr, chain = state.hier
    dev, st = state.plan.device, _stream(state.plan.device)
    part = torch.empty(_hip.ROW_BOUND_BLOCKS, dtype=torch.float64, device=dev)
    out = torch.empty(len(chain), dtype=torch.float64, device=dev)
    for l, lv in enumerate(chain):
        state.eng.L.diffhe_ell_jacobi_row_bound(lv["vals"], lv["cols"], lv["n"], lv["W"], Bv, part, out[l:], st)
    bounds = tuple(out.cpu().tolist())
    if not all(math.isfinite(b) for b in bounds):
        raise ValueError(error)
    for l, b in enumerate(bounds):
        arr[l].reserved = int(math.ceil(1000.0 * b))
    return bounds


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
    this object is the adjoint state the custom ops hold until the end of backward."""

    def __init__(self, solver: "ElasticFESolver", setup: _ElasticSetup, call: _ElasticCall, tol: float, amg: dict):
        self.solver, self.setup, self.call, self.amg = solver, setup, call, amg
        self.plan = setup.plan
        self.eng = _Engine(setup.dofs, tol, solver.max_iter, solver.check_every, "gather", g=setup.dofs.g)
        self.node_eng = _Engine(self.plan, tol, solver.max_iter, solver.check_every, "gather")
        # a call whose nodes need grad (diffhe.elastic_shape) also keeps E and f as the kernels read them, and lambda
        self.shape, self.e_s, self.f_dofs, self.lam = False, None, None, None

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

    # -- forward ----------------------------------------------------------------------------------
    def forward(self, call_in, info: SolveInfo) -> torch.Tensor:
        E, f, load = call_in.E, call_in.f, call_in.load
        solver, setup, plan, call, eng = self.solver, self.setup, self.plan, self.call, self.eng
        dofs, B = setup.dofs, call.B
        Bp = self.Bp = padded_batch(B)
        kdev, kse, ksb, Bv = self.node_eng.kappa_device(E, call.mode, B, Bp, em=call.kappa_em)
        vals, lift = setup.assemble(kdev, kse, ksb, Bv)
        if self.shape:
            self.e_s = (kdev, kse, ksb)
        rhs = -lift if Bv == Bp else (-lift).expand(dofs.n, Bp).contiguous()
        if f is not None:
            f_dofs = self._to_dofs(f, call.f_batched)
            rhs += self._apply_load_map(f_dofs)
            if self.shape:
                self.f_dofs = f_dofs
        if load is not None:
            rhs += self._to_dofs(load, call.load_batched)
        rhs[dofs.is_bc.bool()] = 0.0
        if Bp > B:
            rhs[:, B:] = 0.0
        self.hier = None
        if solver.method != "ell-jacobi":
            levels, stats = setup.levels()
            if levels:
                amg = _cycle_defaults(self.amg, dofs.n, Bp)
                self.hier = eng.amg_setup(vals, Bv, bool(amg.get("fp32", 0)), levels)
                info.hierarchy, info.hierarchy_levels, info.operator_complexity = "unit", stats[0], stats[1]
        if self.hier is not None:
            info.path = "ell-amgpcg"
            x, its, bad, relres, *_ = eng.amg_pcg(self.hier, rhs, Bp, Bv, self.amg)
        else:
            info.path = "ell-pcg"
            x, its, bad, relres, *_ = eng.cg(vals, rhs, Bp, Bv)
        info.iterations, info.not_converged = its, bad
        info.max_relres = float(relres[:B].max())
        self.vals, self.x, self.Bv = vals, x, Bv
        return self._from_dofs(x, dofs.g if (setup.has_data or not call.node_major) else None)

    # -- adjoint ----------------------------------------------------------------------------------
    def adjoint(self, gbar: torch.Tensor, need_e: bool, need_f: bool, need_load: bool):
        """lambda = A^-1 gbar on the free dofs with the forward's operator and hierarchy, then dL/dE in the shape of E,
        dL/df = M lambda and dL/dload = lambda in the caller's layout."""
        call, setup, plan, eng, B, Bp = self.call, self.setup, self.plan, self.eng, self.call.B, self.Bp
        L, st = eng.L, _stream(plan.device)
        info = self.solver.last_info
        rhs = self._to_dofs(gbar, True, zero_fixed=True)
        if self.hier is not None:
            res = eng.amg_pcg(self.hier, rhs, Bp, self.Bv, self.amg)
        else:
            res = eng.cg(self.vals, rhs, Bp, self.Bv)
        lam = res.x
        if self.shape:
            self.lam = lam
        info.adj_iterations, info.adj_max_relres = res.iterations, float(res.relres[:B].max())
        info.not_converged += res.not_converged
        grad_e = grad_f = grad_load = None
        if need_e:
            gtab, vol = plan.gradient_table()
            args = (plan.elems, gtab, vol, plan.dim, setup.lam1, setup.mu1, lam, self.x, setup.dofs.g, plan.n, plan.m)
            sums, de = self.node_eng.element_grad(
                call.mode, call.kappa_em, B, Bp, None,
                lambda de_e, osc, ose, part, total: L.diffhe_elast_grad(*args, Bp, de_e, part, total, st),
                lambda de, osc, ose: L.diffhe_elast_grad_shared(*args, B, Bp, de, st))
            grad_e = _kappa_grad(call.mode, call.e_shape, sums, de)
            grad_e = grad_e.to(call.e_device)
        if need_f:
            df = self._from_dofs(self._apply_load_map(lam))
            grad_f = (df if call.f_batched else df.sum(dim=0)).to(call.out_device)
        if need_load:
            dl = self._from_dofs(lam)
            dl = dl.clone() if call.node_major else dl
            grad_load = (dl if call.load_batched else dl.sum(dim=0)).to(call.out_device)
        return grad_e, grad_f, grad_load


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


def _elastic_forward(solver: "ElasticFESolver", E, f, load, node_major, shape: bool = False):
    """(u, state) of one call.  shape: the state also keeps what the node-gradient kernel reads (diffhe.elastic_shape)."""
    plan = solver._plan()
    setup = _setup_of(plan, solver.nu, solver.plane, solver._lam1, solver._mu1, solver._is_bc, solver._g)
    B_rhs, fb, lb = _batch_of(solver, f, load, node_major)
    mode, B, em = _kappa_layout(E, plan.m, B_rhs, node_major)
    src = f if f.numel() else load
    call = _ElasticCall(B, mode, em, B_rhs is not None, node_major, src.device if src.numel() else E.device, E.shape,
                        E.device, fb, lb)
    tol, _, amg = _call_options(chain=False, lattice=False, closed_boundary=False, n=setup.dofs.n, mode=mode,
                                tol_user=solver._tol_user, mg_user=set(), mg={}, amg=solver.amg)
    solver.tol = tol
    state = _ElasticSolve(solver, setup, call, tol, amg)
    state.shape = shape
    u = _run_call(state, _Inputs(E, f if f.numel() else None, load if load.numel() else None, B, call.batched,
                                 node_major, call.out_device))
    return u, state


def _out_shape(solver, E, f, load, node_major):
    n, d, m = solver.mesh.n_nodes, solver.mesh.dim, solver.mesh.n_elements
    B_rhs, _, _ = _batch_of(solver, f, load, node_major)
    if node_major:
        return (n, d, B_rhs)
    _, B, _ = _kappa_layout(E, m, B_rhs, False)
    return (B, n, d) if (B_rhs is not None or B > 1) else (n, d)


# ---------------------------------------------------------------------------------------------
# torch.library custom ops diffhe::elastic_solve / diffhe::elastic_solve_backward; the solver and the state of the call
# travel as integer handles through the registries of diffhe.solver.  f / load: empty tensor = absent.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("diffhe::elastic_solve", mutates_args=())
def elastic_solve(E: torch.Tensor, f: torch.Tensor, load: torch.Tensor, handle: int, save: bool,
                  node_major: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u, token) of the `ElasticFESolver` registered under `handle`; `token` names the saved adjoint state (0 when
    `save` is false)."""
    u, state = _elastic_forward(_SOLVERS[handle], E, f, load, node_major)
    return u.clone() if u._base is not None or u.data_ptr() == state.x.data_ptr() else u, _register_state(state, save)


@elastic_solve.register_fake
def _elastic_solve_fake(E, f, load, handle, save, node_major):
    shape = _out_shape(_SOLVERS[handle], E, f, load, node_major)
    like = f if f.numel() else (load if load.numel() else E)
    return like.new_empty(shape, dtype=torch.float64), torch.empty((), dtype=torch.int64)


@torch.library.custom_op("diffhe::elastic_solve_backward", mutates_args=())
def elastic_solve_backward(gbar: torch.Tensor, token: torch.Tensor, need_e: bool, need_f: bool, need_load: bool,
                           e_like: torch.Tensor, f_like: torch.Tensor,
                           load_like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dL/dE, dL/df, dL/dload) of the forward call named by `token` from ONE adjoint solve; unused ones come back empty."""
    state = _state_of(token)
    call = state.call
    g = gbar.detach()
    if not call.node_major and not call.batched and call.B == 1:
        g = g.unsqueeze(0)
    grads = state.adjoint(g, need_e, need_f, need_load)
    return _like_grads(gbar, grads, (e_like, f_like, load_like))


@elastic_solve_backward.register_fake
def _elastic_solve_backward_fake(gbar, token, need_e, need_f, need_load, e_like, f_like, load_like):
    return _fake_grads(gbar, (need_e, need_f, need_load), (e_like, f_like, load_like))


def _setup_context(ctx, inputs, output):
    E, f, load = inputs[:3]
    _tie_state(ctx, output[1], E, f, load)


def _backward(ctx, grad_u, _grad_token):
    if torch.is_grad_enabled():
        raise NotImplementedError("diffhe: second-order derivatives of an elastic solve are not implemented (backward "
                                  "with create_graph=True, diffhe.elastic)")
    token, E, f, load = ctx.saved_tensors[:4]
    needs = tuple(bool(v) for v in ctx.needs_input_grad[:3])
    if not any(needs):
        return (None,) * 6
    ge, gf, gl = torch.ops.diffhe.elastic_solve_backward(grad_u.contiguous(), token, *needs, E, f, load)
    return (ge if needs[0] else None, gf if needs[1] else None, gl if needs[2] else None, None, None, None)


torch.library.register_autograd("diffhe::elastic_solve", _backward, setup_context=_setup_context)


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
    sigma, vm = _stress_forward(_SOLVERS[handle], u, E, node_major, want_sigma, want_vm)
    return (u.new_empty(0) if sigma is None else sigma), (u.new_empty(0) if vm is None else vm)


@elastic_stress.register_fake
def _elastic_stress_fake(u, E, handle, node_major, want_sigma, want_vm):
    s_shape, v_shape = _stress_shapes(_SOLVERS[handle], u, E, node_major)
    return (u.new_empty(s_shape if want_sigma else 0, dtype=torch.float64),
            u.new_empty(v_shape if want_vm else 0, dtype=torch.float64))


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


def _stress_setup_context(ctx, inputs, output):
    u, E, handle, node_major = inputs[:4]
    ctx.handle, ctx.node_major = handle, bool(node_major)
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(u, E)


def _stress_backward(ctx, grad_sigma, grad_vm):
    if torch.is_grad_enabled():
        raise NotImplementedError("diffhe: second-order derivatives of an elastic stress evaluation are not implemented "
                                  "(backward with create_graph=True, diffhe.elastic)")
    u, E = ctx.saved_tensors
    need_u, need_e = (bool(v) for v in ctx.needs_input_grad[:2])
    absent = lambda g: g is None or g.numel() == 0  # noqa: E731
    if not (need_u or need_e) or (absent(grad_sigma) and absent(grad_vm)):
        return (None,) * 6
    empty = u.new_empty(0)
    du, de = torch.ops.diffhe.elastic_stress_backward(empty if absent(grad_sigma) else grad_sigma.contiguous(),
                                                      empty if absent(grad_vm) else grad_vm.contiguous(), u, E,
                                                      ctx.handle, ctx.node_major, need_u, need_e)
    return (du if need_u else None, de if need_e else None, None, None, None, None)


torch.library.register_autograd("diffhe::elastic_stress", _stress_backward, setup_context=_stress_setup_context)


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
    s_shape, v_shape = _stress_shapes_eigen(_SOLVERS[handle], u, E, eps0, node_major)
    return (u.new_empty(s_shape if want_sigma else 0, dtype=torch.float64),
            u.new_empty(v_shape if want_vm else 0, dtype=torch.float64))


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


def _stress_eigen_setup_context(ctx, inputs, output):
    u, E, eps0, handle, node_major = inputs[:5]
    ctx.handle, ctx.node_major = handle, bool(node_major)
    ctx.solver = _SOLVERS[handle]           # the registry holds it weakly: the graph keeps it alive for backward
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(u, E, eps0)


def _stress_eigen_backward(ctx, grad_sigma, grad_vm):
    if torch.is_grad_enabled():
        raise NotImplementedError("diffhe: second-order derivatives of an elastic stress evaluation are not implemented "
                                  "(backward with create_graph=True, diffhe.elastic)")
    u, E, eps0 = ctx.saved_tensors
    needs = tuple(bool(v) for v in ctx.needs_input_grad[:3])
    absent = lambda g: g is None or g.numel() == 0  # noqa: E731
    if not any(needs) or (absent(grad_sigma) and absent(grad_vm)):
        return (None,) * 7
    empty = u.new_empty(0)
    _SOLVERS[ctx.handle] = ctx.solver
    grads = torch.ops.diffhe.elastic_stress_eigen_backward(empty if absent(grad_sigma) else grad_sigma.contiguous(),
                                                           empty if absent(grad_vm) else grad_vm.contiguous(), u, E, eps0,
                                                           ctx.handle, ctx.node_major, *needs)
    return (*(g if need else None for g, need in zip(grads, needs)), None, None, None, None)


torch.library.register_autograd("diffhe::elastic_stress_eigen", _stress_eigen_backward,
                                setup_context=_stress_eigen_setup_context)


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


class ElasticFESolver(nn.Module):
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
        if mesh.dim == 1:
            raise NotImplementedError("diffhe: elasticity needs a 2D or 3D mesh (a 1D bar is the scalar problem of "
                                      "DifferentiableFESolver with kappa = E A)")
        if mesh.dim not in (2, 3):
            raise NotImplementedError("Only 2D and 3D supported")
        if mesh.elements.shape[1] != mesh.dim + 1:
            raise NotImplementedError("diffhe: elasticity is implemented for P1 elements only (this mesh has "
                                      f"{mesh.elements.shape[1]} nodes per element)")
        if mesh.dim == 3 and plane is not None:
            raise ValueError("plane= applies to 2D meshes only (a 3D body needs no plane-stress / plane-strain choice)")
        self.plane = None if mesh.dim == 3 else ("stress" if plane is None else plane)
        self.nu = float(nu)
        self._lam1, self._mu1 = lame_unit(self.nu, mesh.dim, self.plane)
        if method not in ("auto", "ell", "ell-jacobi"):
            raise ValueError(f"Unknown method: {method!r}")
        self.mesh, self.method = mesh, method
        self._E = torch.tensor(float(E), dtype=torch.float64) if isinstance(E, (int, float)) else E.to(dtype=torch.float64)
        self._is_bc, self._g = parse_fixed(mesh, fixed)
        # the options of the general path's aggregation-multigrid PCG, as on DifferentiableFESolver
        self.amg = dict(n_coarse=16, gamma=None, scale=None, fp32=0, max_iter=20000, smoothed=1)
        self.amg.update(amg or {})
        if float(self.amg.get("strength", 0) or 0) > 0.0:
            raise NotImplementedError("diffhe: amg=dict(strength=...) is not implemented for elasticity (the hierarchy "
                                      "is built from the unit-E operator)")
        if not self.amg.get("smoothed", 1):
            raise NotImplementedError("diffhe: elasticity builds a smoothed-aggregation hierarchy (amg smoothed=0 is not "
                                      "implemented)")
        self._device = device
        self._tol_user = tol
        self.tol, self.max_iter, self.check_every = tol, int(max_iter), int(check_every)
        self.last_info = SolveInfo()

    @property
    def E(self) -> torch.Tensor:
        return self._E

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

    def forward(self, f: Optional[torch.Tensor] = None, load: Optional[torch.Tensor] = None, layout: str = "sample",
                dirichlet=None, h=None, u_inf=None, flux=None, eigenstrain=None) -> torch.Tensor:
        """u for the body force f and the nodal load: (n, d), (B, n, d), or (n, d, B) with layout="node" -- the shape of
        the right-hand side.  f None: zero.  eigenstrain: an initial strain eps0 (layouts: `eigenstrain_load`), whose
        load F0(eps0, E) joins `load` in front of the unchanged solve; None takes exactly the path without it."""
        if dirichlet is not None:
            raise NotImplementedError("diffhe: dirichlet= is not implemented for elasticity (the boundary-band kernels "
                                      "read scalar element tables); give prescribed displacements with fixed=")
        if h is not None or u_inf is not None or flux is not None:
            raise NotImplementedError("diffhe: Robin / flux data (h=, u_inf=, flux=) are not implemented for elasticity; "
                                      "integrate a traction into load=")
        if layout not in ("sample", "node"):
            raise ValueError(f"Unknown layout: {layout!r}")
        self._refuse_moving_nodes("solve", eigenstrain is not None)
        f64, load64 = self._checked(f, "f", layout), self._checked(load, "load", layout)
        if eigenstrain is not None:
            load64 = self._with_eigenstrain_load(eigenstrain, f64, load64, layout)
        if layout == "node":
            if f64 is None and load64 is None:
                raise ValueError("layout='node' needs f or load to carry the batch: (n, d, B)")
            if f64 is not None and load64 is not None and f64.shape != load64.shape:
                raise ValueError(f"layout='node': f (and load) must be (n, d, B) with one B, got {tuple(f64.shape)} and "
                                 f"{tuple(load64.shape)}")
        E = self._E
        empty = E.new_empty(0)
        if f64 is None and load64 is None:
            f64 = torch.zeros((self.mesh.n_nodes, self.mesh.dim), dtype=torch.float64, device=E.device)
        f_in, load_in = (empty if f64 is None else f64), (empty if load64 is None else load64)
        _kappa_layout(E, self.mesh.n_elements, _batch_of(self, f_in, load_in, layout == "node")[0], layout == "node")
        _SOLVERS[id(self)] = self
        return self._solve_op(E, f_in, load_in, layout == "node")

    def _moving_nodes(self) -> bool:
        return self.mesh.nodes.requires_grad and torch.is_grad_enabled()

    def _refuse_moving_nodes(self, what: str, eigenstrain: bool) -> None:
        """Moving nodes are `ShapeElasticFESolver`'s (diffhe.elastic_shape), which overrides this."""
        if self._moving_nodes():
            raise NotImplementedError("diffhe: node gradients are not implemented for elasticity (mesh.nodes requires "
                                      "grad)")

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
