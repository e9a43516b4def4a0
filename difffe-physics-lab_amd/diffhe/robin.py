"""Robin (convective) and flux boundary conditions with gradients (ours: the reference knows Dirichlet nodes and the
natural zero-flux boundary only).

`RobinFESolver(mesh, kappa, facets=None, **options)` solves -div(kappa grad u) + c u = f with u = g on the mesh's Dirichlet
nodes and, on the boundary facets Gamma_R it is given,

    kappa du/dn + h (u - u_inf) = q            h >= 0 the film coefficient, u_inf the ambient value, q a prescribed flux
                                               (h = 0: a pure flux condition), each constant per facet.

It is a `DifferentiableFESolver3D` (same options, kappa layouts, `reaction=`, `load=`, `layout=`) whose
`forward(f, h=None, u_inf=None, flux=None, load=None, layout="sample")` takes the three boundary quantities; any of them
may require grad.  `facets` is an index tensor into `mesh.boundary_facets()` (default: every boundary facet; a facet all
of whose nodes are Dirichlet nodes has no effect), fixed at construction.  With d nodes per facet (1: end point of a
chain, 2: edge, 3: face of a tetrahedron) and the consistent P1 facet mass M_F[p, q] = |F| (1 + delta_pq) / (d (d + 1)):

    A = K(kappa) + c M_L + sum_F h_F M_F,       F_p += (h_F u_inf_F + q_F) |F| / d,

then the Dirichlet elimination of the base class (a Dirichlet node on a facet keeps its identity row; its column goes to
the right-hand side with its value).  From the ONE adjoint solve lambda that gives dL/dkappa, dL/df and dL/dload (their
formulas are unchanged: the Robin term does not depend on kappa), with s_F = (|F| / d) sum_p lambda_p:

    dL/dq_F = s_F,      dL/du_inf_F = h_F s_F,      dL/dh_F = u_inf_F s_F - lambda_F^T M_F u_F.

Layouts of h, u_inf and flux, each on its own (n_F = number of facets of this solver, B = batch):
  ()           one value for all facets and samples          (n_F,)      per facet, shared by the batch
  (B,)         one value per sample                          (B, n_F)    per sample and facet -- (n_F, B) with
                                                                         layout="node", batch innermost like f and u
A gradient has the shape of its input (shared ones are summed over the batch inside the kernel, in a fixed order).  When
B == n_F a 1D tensor reads per sample if f or kappa carries that batch, like the scalar (m,) / (B,) kappa.  All are read
in place through their strides (csrc/robin.hip); nothing is copied or padded.

Every call takes the general path (ELL operator, aggregation-multigrid PCG), `FEMesh.rectangle` connectivity and 1D chains
included, with a stored operator -- never the factored kappa_b K_1 of closed boundaries: ONE matrix for the batch when
kappa and h are both shared by it, one per sample otherwise.  On `FEMesh.box` the pattern from which scalar-kappa zeros
are pruned lacks the diagonal of a boundary face's square, which a facet mass fills: such a mesh is solved on the
unpruned plan tensor solves use.  The "singular system" warning of a mesh without Dirichlet nodes is not raised when some
h_F > 0 (one device synchronisation, on such meshes only).  `validate=True` refuses negative or non-finite h (ValueError;
one device synchronisation per call).  The solve travels through the custom ops `diffhe::robin_solve` /
`diffhe::robin_solve_backward`, next to `diffhe::fe_solve`, which is unchanged.  Only what facet data adds is here: the
call itself -- options, state lifetime, warnings, the adjoint and the shaping of dL/dkappa, dL/df, dL/dload, the input
checks -- runs through the steps of diffhe.solver, and `_RobinSolve` is the general path's forward with two hooks filled.

Not implemented (NotImplementedError): `dirichlet=` (per-call Dirichlet values), backward with create_graph=True, P2
meshes, classes that combine this solver with `AnisotropicFESolver` or `ShapeDifferentiableFESolver` (conductivity
tensors, node gradients).  `diffhe.heat.HeatEquation` does not pass Robin data.
"""
from __future__ import annotations

import hashlib
import warnings
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from .plan import get_plan, _stream
from .solver import (_Call, _EllSolve, _SOLVERS, _adjoint_grads, _begin_call, _fake_grads, _fake_solve, _like_grads,
                     _register_state, _resolve_device, _run_call, _state_of, _tie_state)
from .tet3d import DifferentiableFESolver3D

__all__ = ("RobinFESolver",)

SCALAR, SAMPLE, FACET, BOTH = 0, 1, 2, 3


@dataclass
class _Datum:
    """One of h, u_inf, flux as the kernels read it: value of facet F and sample b at dev[F * sf + b * sb]."""
    dev: torch.Tensor
    sf: int
    sb: int
    kind: int
    shape: torch.Size
    device: torch.device

    @classmethod
    def of(cls, t: torch.Tensor, name: str, n_f: int, B: int, node_major: bool, device) -> "_Datum":
        if t.dim() == 0 or (t.dim() == 1 and t.shape[0] == 1 and n_f != 1 and B != 1):
            kind = SCALAR
        elif t.dim() == 1 and t.shape[0] == n_f and (B == 1 or B != n_f):
            kind = FACET
        elif t.dim() == 1 and t.shape[0] == B:
            kind = SAMPLE
        elif t.dim() == 2 and tuple(t.shape) == ((n_f, B) if node_major else (B, n_f)):
            kind = BOTH
        else:
            raise ValueError(f"{name} must be (), ({B},) per sample, ({n_f},) per facet or "
                             f"{(n_f, B) if node_major else (B, n_f)}, got {tuple(t.shape)}")
        dev = t.detach().to(device, torch.float64)
        if any(s == 0 for s, k in zip(dev.stride(), dev.shape) if k > 1):       # an expanded view: one plain copy
            dev = dev.contiguous()
        if kind == SCALAR:
            dev, sf, sb = dev.reshape(1), 0, 0
        elif kind == SAMPLE:
            sf, sb = 0, dev.stride(0)
        elif kind == FACET:
            sf, sb = dev.stride(0), 0
        elif node_major:
            sf, sb = dev.stride(0), dev.stride(1)
        else:
            sf, sb = dev.stride(1), dev.stride(0)
        return cls(dev, int(sf), int(sb), kind, t.shape, t.device)

    @property
    def per_sample(self) -> bool:
        return self.kind in (SAMPLE, BOTH)


class _RobinSolve(_EllSolve):
    """The general path with the facet terms added to the stored operator and the right-hand side (csrc/robin.hip).
    `tab`: the plan's facet table; `h`, `u_inf`, `flux`: the call's `_Datum`s -- boundary-sized, kept for the adjoint."""

    def _operator_form(self) -> Tuple[bool, bool]:
        """Never factored: h M_F does not scale with kappa.  One stored matrix per sample when h differs between them."""
        return False, self.h.per_sample

    def _boundary_terms(self, vals, rhs, Bv) -> None:
        plan, eng, tab, h, ui, q = self.plan, self.eng, self.tab, self.h, self.u_inf, self.flux
        eng.L.diffhe_robin_assemble(tab["fac"], tab["d"], tab["n_f"], tab["area"], tab["rows"], tab["row_ptr"],
                                    tab["ent_code"], tab["ent_slot"], tab["n_rows"], eng.g, h.dev, h.sf, h.sb, ui.dev,
                                    ui.sf, ui.sb, q.dev, q.sf, q.sb, vals, rhs, plan.n, Bv, self.call.B, self.Bp,
                                    _stream(plan.device))

    def facet_grads(self, lam: torch.Tensor, needs):
        """(dL/dh, dL/du_inf, dL/dflux), each in the shape of its input or None, from the adjoint lambda (n, Bp)."""
        plan, eng, tab, B, Bp = self.plan, self.eng, self.tab, self.call.B, self.Bp
        n_f, node_major = tab["n_f"], self.call.node_major
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=plan.device)  # noqa: E731
        outs, args = [], []
        for need, dat in zip(needs, (self.h, self.u_inf, self.flux)):
            if not need:
                outs.append(None)
                args += [None, 0, 0]
            elif dat.kind == BOTH:
                o = new(n_f, B) if node_major else new(B, n_f)
                outs.append(o)
                args += [o, *((B, 1) if node_major else (1, n_f))]
            elif dat.kind == FACET:             # summed over the batch inside the kernel
                outs.append(new(n_f))
                args += [outs[-1], 1, 0]
            else:                               # per facet and sample, then summed over the facets in two stages
                outs.append(new(n_f, B))
                args += [outs[-1], B, 1]
        h, ui = self.h, self.u_inf
        eng.L.diffhe_robin_grad(tab["fac"], tab["d"], n_f, tab["area"], lam, self.x, eng.g, B, Bp, h.dev, h.sf, h.sb,
                                ui.dev, ui.sf, ui.sb, *args, _stream(plan.device))
        grads = []
        for o, dat in zip(outs, (self.h, self.u_inf, self.flux)):
            if o is not None and dat.kind in (SCALAR, SAMPLE):
                part, tot = new(eng.L.diffhe_robin_sum_blocks(n_f), B), new(B)
                eng.L.diffhe_robin_sum_facets(o, n_f, B, part, tot, _stream(plan.device))
                o = tot.sum() if dat.kind == SCALAR else tot
            grads.append(None if o is None else o.reshape(dat.shape))
        return grads


def _robin_forward(solver, kappa, f, load, h, u_inf, flux, node_major):
    """The forward of a call with facet data: always the general path, as `_RobinSolve`.  -> (u, state)."""
    plan = solver._plan()
    tab = plan.robin_table(solver._facet_key, solver._facets_host)
    call = _Call.of(solver, plan, kappa, f, load, node_major)
    data = [_Datum.of(t, name, tab["n_f"], call.B, node_major, plan.device)
            for t, name in ((h, "h"), (u_inf, "u_inf"), (flux, "flux"))]
    state = _begin_call(solver, plan, call, _RobinSolve)
    state.tab, (state.h, state.u_inf, state.flux) = tab, data
    if plan.n_bc == 0 and call.reaction == 0.0 and not bool((data[0].dev > 0).any()):
        warnings.warn("diffhe: the system is singular (pure Neumann problem: no Dirichlet node, no reaction term, no "
                      "facet with h > 0); the returned values are not a solution", RuntimeWarning)
    return _run_call(state, call), state


def _robin_backward(state: _RobinSolve, gbar, needs):
    """(dL/dkappa, dL/df, dL/dload, dL/dh, dL/du_inf, dL/dflux) from ONE adjoint solve, None where not needed."""
    lam, *grads = _adjoint_grads(state, gbar, *needs[:3])
    facet = state.facet_grads(lam, needs[3:]) if any(needs[3:]) else [None, None, None]
    return (*grads[:3], *facet)


# ---------------------------------------------------------------------------------------------
# torch.library custom ops diffhe::robin_solve / diffhe::robin_solve_backward, next to diffhe::fe_solve: the solver and the
# adjoint state travel as integer handles through the registries of diffhe.solver.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("diffhe::robin_solve", mutates_args=())
def robin_solve(kappa: torch.Tensor, f: torch.Tensor, load: torch.Tensor, h: torch.Tensor, u_inf: torch.Tensor,
                flux: torch.Tensor, handle: int, save: bool, node_major: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u, token) = solve with the `RobinFESolver` registered under `handle`; arguments as diffhe::fe_solve, plus the
    facet data h, u_inf, flux in one of the layouts of the module docstring (a 0-dim zero for none)."""
    u, state = _robin_forward(_SOLVERS[handle], kappa, f, load, h, u_inf, flux, node_major)
    return u, _register_state(state, save)


@robin_solve.register_fake
def _robin_solve_fake(kappa, f, load, h, u_inf, flux, handle, save, node_major):
    return _fake_solve(_SOLVERS[handle], kappa, f, node_major)


_Grads6 = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]


@torch.library.custom_op("diffhe::robin_solve_backward", mutates_args=())
def robin_solve_backward(gbar: torch.Tensor, token: torch.Tensor, need_k: bool, need_f: bool, need_load: bool,
                         need_h: bool, need_u: bool, need_q: bool, kappa_like: torch.Tensor, f_like: torch.Tensor,
                         load_like: torch.Tensor, h_like: torch.Tensor, u_like: torch.Tensor,
                         q_like: torch.Tensor) -> _Grads6:
    """The six gradients of the forward call named by `token`, each with the device and dtype of its `*_like`; unused
    ones come back empty."""
    grads = _robin_backward(_state_of(token), gbar, (need_k, need_f, need_load, need_h, need_u, need_q))
    return _like_grads(gbar, grads, (kappa_like, f_like, load_like, h_like, u_like, q_like))


@robin_solve_backward.register_fake
def _robin_solve_backward_fake(gbar, token, need_k, need_f, need_load, need_h, need_u, need_q, kappa_like, f_like,
                               load_like, h_like, u_like, q_like):
    return _fake_grads(gbar, (need_k, need_f, need_load, need_h, need_u, need_q),
                       (kappa_like, f_like, load_like, h_like, u_like, q_like))


def _setup_context(ctx, inputs, output):
    """Save (token, kappa, f, load, h, u_inf, flux) and u when node-major (it may BE the saved iterate), and tie the
    adjoint state to them."""
    *tensors, _handle, _save, node_major = inputs
    _tie_state(ctx, output[1], *tensors, *((output[0],) if node_major else ()))


def _backward(ctx, grad_u, _grad_token):
    if torch.is_grad_enabled():
        raise NotImplementedError("diffhe: second-order derivatives of a solve with Robin / flux data are not implemented "
                                  "(backward with create_graph=True, diffhe.robin)")
    needs = tuple(bool(v) for v in ctx.needs_input_grad[:6])
    token, *tensors = ctx.saved_tensors[:7]
    grads = torch.ops.diffhe.robin_solve_backward(grad_u, token, *needs, *tensors)
    return (*(g if need else None for g, need in zip(grads, needs)), None, None, None)


torch.library.register_autograd("diffhe::robin_solve", _backward, setup_context=_setup_context)


class RobinFESolver(DifferentiableFESolver3D):
    """`DifferentiableFESolver3D` with Robin / flux data kappa du/dn + h (u - u_inf) = q on boundary facets and gradients
    with respect to h, u_inf and q (see the module docstring)."""

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        from .aniso import AnisotropicFESolver
        from .shape import ShapeDifferentiableFESolver
        if issubclass(cls, (AnisotropicFESolver, ShapeDifferentiableFESolver)):
            raise NotImplementedError("diffhe: Robin / flux data together with a conductivity tensor or node gradients "
                                      "are not implemented")

    def __init__(self, mesh, kappa=1.0, facets: Optional[torch.Tensor] = None, *, validate: bool = False, **options):
        if mesh.elements.shape[1] != mesh.dim + 1:
            raise NotImplementedError("diffhe: Robin / flux data are implemented for P1 elements only (this mesh has "
                                      f"{mesh.elements.shape[1]} nodes per element)")
        super().__init__(mesh, kappa, **options)
        every = mesh.boundary_facets()
        self._facet_key = None
        if facets is not None:
            idx = torch.as_tensor(facets).detach().to("cpu", torch.long).reshape(-1)
            if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= every.shape[0]:
                raise ValueError(f"facets must be a non-empty index tensor into mesh.boundary_facets() ({every.shape[0]} "
                                 "facets)")
            every = every[idx]
            self._facet_key = hashlib.blake2b(idx.numpy().tobytes(), digest_size=16).hexdigest()
        self.facets = every                         # (n_F, d) node ids, the order h, u_inf and flux are given in
        self._facets_host = every.numpy()
        self.validate = bool(validate)

    @property
    def n_facets(self) -> int:
        return self.facets.shape[0]

    def _plan(self):
        """The mesh's plan -- its unpruned twin when the pruned stiffness pattern lacks a coupling of a facet."""
        device = _resolve_device(self._device)
        plan = get_plan(self.mesh, device)
        if plan.robin_table(self._facet_key, self._facets_host) is None:
            plan = get_plan(self.mesh, device, prune=False)
            if plan.robin_table(self._facet_key, self._facets_host) is None:
                raise RuntimeError("diffhe: a facet couples two nodes that share no element")
        return plan

    def forward(self, f: torch.Tensor, h: Optional[torch.Tensor] = None, u_inf: Optional[torch.Tensor] = None,
                flux: Optional[torch.Tensor] = None, load: Optional[torch.Tensor] = None, layout: str = "sample",
                dirichlet: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Solve for nodal u.  f, load, layout as `DifferentiableFESolver.forward`; h, u_inf, flux: the film coefficient,
        ambient value and prescribed flux of this solver's facets, each (), (B,), (n_F,) or (B, n_F) -- (n_F, B) with
        layout="node" -- or None for zero.  A 2D one implies the batch, like a (B, n) load."""
        if dirichlet is not None:
            raise NotImplementedError("diffhe: dirichlet= together with Robin / flux data is not implemented; put the "
                                      "values into the mesh")
        data = [None if t is None else (t if isinstance(t, torch.Tensor) else torch.as_tensor(t)) for t in (h, u_inf, flux)]
        for t, name in zip(data, ("h", "u_inf", "flux")):
            if t is not None and (t.is_complex() or t.dim() > 2):
                raise ValueError(f"{name} must be a real tensor of at most two dimensions, got {tuple(t.shape)} {t.dtype}")
        f64, load64, node_major, transposed = self._checked_inputs(f, load, layout, "1D, 2D and 3D")
        if transposed:      # the general path of a chain works sample-major: transposing views in and out
            tr = [t.t() if t is not None and t.dim() == 2 else t for t in data]
            return self.forward(f.t(), *tr, load=None if load is None else load.t()).t()
        if f64.dim() == 1:              # (B, n_F) facet data imply the batch, like a (B, n) load
            implied = [t.shape[0] for t in data if t is not None and t.dim() == 2]
            if implied:
                f64 = f64.reshape(1, -1).expand(implied[0], -1)
        if self.validate and data[0] is not None:
            hv = data[0].detach()
            if not bool((torch.isfinite(hv) & (hv >= 0)).all()):
                raise ValueError("diffhe: the film coefficient h must be finite and >= 0 everywhere (validate=True)")
        d64 = [f64.new_zeros(()) if t is None else t.to(torch.float64) for t in data]
        _SOLVERS[id(self)] = self
        save = torch.is_grad_enabled() and any(t.requires_grad for t in (self._kappa, f64, load64, *d64))
        u, _token = torch.ops.diffhe.robin_solve(self._kappa, f64, load64, *d64, id(self), save, node_major)
        return u
