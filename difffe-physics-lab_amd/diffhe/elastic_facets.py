"""Tractions, pressure and elastic (Winkler) foundations on boundary facets of elastic bodies, with gradients (ours: the
reference solves scalar equations only).

`TractionElasticFESolver(mesh, E, nu, plane=, fixed=, facets=None, validate=False, **options)` is an `ElasticFESolver`
(same options, E layouts, `f`, `load=`, `eigenstrain=`, `layout=`, stress methods) whose
`forward(f, load, traction=None, pressure=None, k_normal=None, k_tangent=None, ...)` loads and supports the body on the
boundary facets Gamma it is given: on facet F with the OUTWARD unit normal n_F

    sigma(u) n = t_F - p_F n_F - S_F u,      S_F = k^n_F n_F n_F^T + k^t_F (I - n_F n_F^T)

t a dead traction with d components, p a pressure along -n, k^n, k^t >= 0 the normal and tangential stiffness per unit
area of an elastic foundation, each constant per facet; any of them may require grad.  `facets` is an index tensor into
`mesh.boundary_facets()` (default: every boundary facet), fixed at construction; `solver.facets` (n_F, d) are their node
ids in the order the data are given in, `solver.facet_normals` (n_F, d) and `solver.facet_areas` (n_F,) host tensors for
building t = sigma n.  With d nodes per facet (2: edge, 3: face of a tetrahedron) and the consistent P1 facet mass
M_F[p, q] = |F| (1 + delta_pq) / (d (d + 1)) of diffhe.robin:

    A[(p,a),(q,b)] += sum_F M_F[p,q] S_F[a,b],       F[(p,a)] += sum_F (|F| / d) (t_F[a] - p_F n_F[a]),

then the Dirichlet elimination of `ElasticFESolver` (a fixed dof on a facet keeps its identity row; its column goes to the
right-hand side with the prescribed value, through the foundation term as well).  From the ONE adjoint solve lambda that
gives dL/dE, dL/df and dL/dload (their formulas are unchanged: the facet terms do not depend on E) and the full
displacement u, with s_F = (|F| / d) sum_p lambda_p:

    dL/dt_F = s_F,      dL/dp_F = -s_F . n_F,      dL/dk^n_F = -sum_pq M_F[p,q] (lambda_p . n_F)(u_q . n_F),
    dL/dk^t_F = -sum_pq M_F[p,q] [lambda_p . u_q - (lambda_p . n_F)(u_q . n_F)].

The outward orientation comes from the owning element's node opposite the facet (a boundary facet has exactly one owner,
found on the host); areas and normals are computed on the device with the plan's facet table.

Layouts (n_F = number of facets of this solver, B = batch), each datum on its own:
  pressure, k_normal, k_tangent   (), (B,), (n_F,), (B, n_F) -- (n_F, B) with layout="node"; when B == n_F a 1D tensor
                                  reads per sample, the rule of `RobinFESolver`
  traction                        (d,), (B, d), (n_F, d), (B, n_F, d) -- (n_F, d, B) with layout="node"; when B == n_F a
                                  2D tensor reads per sample
A datum with a batch axis of its own implies the batch, like a batched load.  All are read in place through their
strides (csrc/elastic_facets.hip, include/diffhe_elastic_facets.h); nothing is copied or padded.  A gradient has the
shape of its input; shared axes are summed in a fixed order inside the kernel (the batch) or by the two-stage
`diffhe_robin_sum_facets` (the facets).

Paths.  All four data None: exactly `ElasticFESolver`'s call, `diffhe::elastic_solve` -- u and the gradients are bitwise
the base class's.  Traction and / or pressure only: the operator, the hierarchy and the smoother bounds are
`ElasticFESolver`'s; only the right-hand side gains the facet loads.  A stiffness given: the stored operator is per sample
whenever E OR a stiffness is per sample (a shared E is then read with a zero sample stride), the unit-E hierarchy is
reused and the smoother's bounds are measured per call on every level (`diffhe_ell_jacobi_row_bound`, as
`AnisotropicElasticFESolver` does; one device synchronisation) and reported in `last_info.jacobi_bounds`.  A body without
any fixed dof is accepted; held by no foundation either it raises the "singular system" warning (one device
synchronisation, on such bodies only).  `validate=True` refuses a negative or non-finite stiffness (ValueError; one
device synchronisation per call).  The solve travels through the custom ops `diffhe::elastic_facet_solve` /
`diffhe::elastic_facet_solve_backward`, next to `diffhe::elastic_solve`, which is unchanged.

Not implemented (NotImplementedError): backward with create_graph=True; mesh.nodes requiring grad (a follower pressure
with moving nodes); classes that combine this solver with `AnisotropicElasticFESolver` or `ShapeElasticFESolver`; P2 and
1D meshes; and what `ElasticFESolver` refuses.
"""
from __future__ import annotations

import hashlib
import warnings
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .elastic import (ElasticFESolver, _ElasticSolve, _batch_of, _run_adjoint, _solve_autograd, _solve_call, _solve_fake,
                      _solve_result)
from .plan import _stream
from .robin import BOTH, FACET, SAMPLE, SCALAR
from .solver import SolveInfo, _SOLVERS, _fake_grads, _kappa_layout, _like_grads

__all__ = ("TractionElasticFESolver", "ElasticFacetInfo", "opposite_nodes", "facet_geometry")

NAMES = ("traction", "pressure", "k_normal", "k_tangent")


# ---------------------------------------------------------------------------------------------
# Host logic (numpy / torch on the host; no device, no library)
# ---------------------------------------------------------------------------------------------
def opposite_nodes(elements: np.ndarray, facets: np.ndarray) -> np.ndarray:
    """(n_F,) int64: for every facet (n_F, d) the node of its owning element that is not on it.  elements (m, d + 1).
    A facet that is a facet of no element, or of more than one, raises ValueError: a boundary facet has one owner."""
    m, npe = elements.shape
    d = npe - 1
    if facets.ndim != 2 or facets.shape[1] != d:
        raise ValueError(f"facets must be (n_F, {d}) node ids")
    local = np.stack([np.delete(elements, q, axis=1) for q in range(npe)], axis=1).reshape(-1, d)    # opposite q
    both = np.concatenate([np.sort(local, axis=1), np.sort(facets, axis=1)])
    _, inv, cnt = np.unique(both, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    first = np.full(len(cnt), -1, dtype=np.int64)
    first[inv[:m * npe][::-1]] = np.arange(m * npe - 1, -1, -1)             # the element facet of every key
    own_count = np.bincount(inv[:m * npe], minlength=len(cnt))
    key = inv[m * npe:]
    if bool((own_count[key] != 1).any()):
        raise ValueError("diffhe: a facet that is not a boundary facet of this mesh (it must belong to exactly one element)")
    ef = first[key]
    return elements[ef // npe, ef % npe].astype(np.int64)


def facet_geometry(nodes: torch.Tensor, facets: torch.Tensor, opposite: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(areas (n_F,), normals (n_F, d)) of facets (n_F, d) on the host, fp64: the unit normal that points away from the
    opposite node.  A facet without extent gets area 0 and normal 0."""
    X = nodes.detach().to("cpu", torch.float64)
    P, Xo = X[facets], X[opposite]
    if X.shape[1] == 2:
        e = P[:, 1] - P[:, 0]
        nv = torch.stack([e[:, 1], -e[:, 0]], dim=1)
        size = nv.norm(dim=1)
    else:
        nv = torch.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], dim=1)
        size = 0.5 * nv.norm(dim=1)
    sign = torch.where(((P[:, 0] - Xo) * nv).sum(dim=1) >= 0, 1.0, -1.0)
    length = nv.norm(dim=1)
    unit = torch.where(length[:, None] > 0, sign[:, None] * nv / length.clamp_min(1e-300)[:, None], torch.zeros_like(nv))
    return size, unit


def _kind_of(t: torch.Tensor, name: str, n_f: int, B: int, node_major: bool, d: int) -> int:
    """SCALAR / SAMPLE / FACET / BOTH of one datum; d: trailing components (0: a scalar datum).  The rule of
    `robin._Datum.of` where n_F == B: the leading axis reads per sample unless the call has no batch."""
    lead = t.dim() - (1 if d else 0)                                # axes in front of the component axis
    comp_ok = not d or (t.dim() >= 1 and (t.shape[1] if (node_major and t.dim() == 3) else t.shape[-1]) == d)
    if comp_ok and (lead == 0 or (not d and lead == 1 and t.shape[0] == 1 and n_f != 1 and B != 1)):
        return SCALAR
    if comp_ok and lead == 1 and t.shape[0] == n_f and (B == 1 or B != n_f):
        return FACET
    if comp_ok and lead == 1 and t.shape[0] == B:
        return SAMPLE
    if comp_ok and lead == 2:
        want = ((n_f, d, B) if node_major else (B, n_f, d)) if d else ((n_f, B) if node_major else (B, n_f))
        if tuple(t.shape) == want:
            return BOTH
    if d:
        raise ValueError(f"{name} must be ({d},), ({B}, {d}) per sample, ({n_f}, {d}) per facet or "
                         f"{(n_f, d, B) if node_major else (B, n_f, d)}, got {tuple(t.shape)}")
    raise ValueError(f"{name} must be (), ({B},) per sample, ({n_f},) per facet or "
                     f"{(n_f, B) if node_major else (B, n_f)}, got {tuple(t.shape)}")


def _implied_batch(t: Optional[torch.Tensor], node_major: bool, d: int) -> Optional[int]:
    """The batch a datum with a batch axis AND a facet axis carries; None for every other shape."""
    if t is None or t.dim() != (3 if d else 2):
        return None
    return t.shape[-1] if node_major else t.shape[0]


@dataclass
class _Datum:
    """One facet datum as the kernels read it: component a of facet F and sample b at dev[F * sf + a * sc + b * sb]."""
    dev: torch.Tensor
    sf: int
    sc: int
    sb: int
    kind: int
    shape: torch.Size
    comps: int

    @classmethod
    def of(cls, t: torch.Tensor, name: str, n_f: int, B: int, node_major: bool, device, d: int) -> "_Datum":
        kind = _kind_of(t, name, n_f, B, node_major, d)
        dev = t.detach().to(device, torch.float64)
        if any(s == 0 for s, k in zip(dev.stride(), dev.shape) if k > 1):       # an expanded view: one plain copy
            dev = dev.contiguous()
        if kind == SCALAR and not d:
            dev = dev.reshape(1)
        st = dev.stride()
        sf = sc = sb = 0
        if d and node_major and kind == BOTH:       # (n_F, d, B)
            sf, sc, sb = st
        else:                                       # the axes in front of the components: none, (B), (n_F), (B, n_F) / (n_F, B)
            lead, sc = (st[:-1], st[-1]) if d else (st, 0)
            if kind == SAMPLE:
                sb = lead[0]
            elif kind == FACET:
                sf = lead[0]
            elif kind == BOTH:
                sf, sb = (lead[0], lead[1]) if node_major else (lead[1], lead[0])
        return cls(dev, int(sf), int(sc), int(sb), kind, t.shape, d)

    @property
    def per_sample(self) -> bool:
        return self.kind in (SAMPLE, BOTH)


@dataclass
class ElasticFacetInfo(SolveInfo):
    """`SolveInfo` with the bound of lambda_max(D^-1 A) a call with a foundation measured on every level of its hierarchy,
    the fine one first (empty: no foundation, or no hierarchy)."""
    jacobi_bounds: Tuple[float, ...] = ()


# ---------------------------------------------------------------------------------------------
# One call
# ---------------------------------------------------------------------------------------------
class _FacetElasticSolve(_ElasticSolve):
    """`_ElasticSolve` with the facet terms added to the stored operator and the right-hand side -- one launch after the
    right-hand side is formed --, the measured smoother bounds of a call with a foundation (`bounds_error` is set on such
    a call), and the facet gradients from the adjoint lambda it keeps (csrc/elastic_facets.hip).  `tab`: the plan's
    facet table; `data`: the call's (traction, pressure, k_normal, k_tangent) as `_Datum` or None -- boundary-sized, kept
    for the adjoint."""
    Info = ElasticFacetInfo
    keep_lambda = True                  # `facet_grads` reads lambda after `adjoint`
    tab = None
    data = (None, None, None, None)

    def _operator(self, E):
        """The isotropic operator, one matrix per sample also where only a foundation stiffness is per sample."""
        call, Bp = self.call, self.Bp
        kdev, kse, ksb, Bv = self.node_eng.kappa_device(E, call.mode, call.B, Bp, em=call.kappa_em)
        if Bv == 1 and Bp > 1 and any(z is not None and z.per_sample for z in self.data[2:]):
            Bv = Bp                     # for the foundation's sake: the shared E has ksb = 0
        return (*self.setup.assemble(kdev, kse, ksb, Bv), Bv)

    def _after_rhs(self, vals, rhs, Bv) -> None:
        plan, dofs, tab = self.plan, self.setup.dofs, self.tab
        t, p, kn, kt = self.data
        scalar = lambda z: (None, 0, 0) if z is None else (z.dev, z.sf, z.sb)  # noqa: E731
        self.eng.L.diffhe_elastf_assemble(
            tab["fac"], tab["d"], tab["n_f"], tab["area"], tab["normal"], tab["rows"], tab["row_ptr"], tab["ent_code"],
            tab["ent_slot"], tab["n_rows"], dofs.is_bc, dofs.g, *((None, 0, 0, 0) if t is None else (t.dev, t.sf, t.sc, t.sb)),
            *scalar(p), *scalar(kn), *scalar(kt), vals if (kn is not None or kt is not None) else None, rhs, plan.n, Bv,
            self.call.B, self.Bp, _stream(plan.device))


    def facet_grads(self, needs):
        """(dL/dtraction, dL/dpressure, dL/dk_normal, dL/dk_tangent), each in the shape of its input or None, from the
        adjoint lambda (n d, Bp) the adjoint solve left."""
        plan, eng, tab, B, Bp = self.plan, self.eng, self.tab, self.call.B, self.Bp
        n_f, d, node_major = tab["n_f"], tab["d"], self.call.node_major
        st = _stream(plan.device)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=plan.device)  # noqa: E731
        outs, args = [], []
        for k, (need, dat) in enumerate(zip(needs, self.data)):
            comps = dat.comps if dat is not None else 0
            if not need or dat is None:
                outs.append(None)
                strides = (0, 0, 0)
            elif dat.kind == BOTH:
                if comps:
                    outs.append(new(n_f, d, B) if node_major else new(B, n_f, d))
                    strides = (d * B, B, 1) if node_major else (d, 1, n_f * d)
                else:
                    outs.append(new(n_f, B) if node_major else new(B, n_f))
                    strides = (B, 0, 1) if node_major else (1, 0, n_f)
            elif dat.kind == FACET:             # summed over the batch inside the kernel
                outs.append(new(n_f, d) if comps else new(n_f))
                strides = (d, 1, 0) if comps else (1, 0, 0)
            else:                               # per facet and sample, then summed over the facets in two stages
                outs.append(new(d, n_f, B) if comps else new(n_f, B))
                strides = (B, n_f * B, 1) if comps else (B, 0, 1)
            args += [outs[-1], *strides] if k == 0 else [outs[-1], strides[0], strides[2]]    # only dt has components
        eng.L.diffhe_elastf_grad(tab["fac"], d, n_f, tab["area"], tab["normal"], self.lam, self.x, self.setup.dofs.g, B, Bp,
                                 *args, st)
        grads = []
        for o, dat in zip(outs, self.data):
            if o is not None and dat.kind in (SCALAR, SAMPLE):
                rows = o.reshape(-1, n_f, B)                    # one (n_F, B) array per component
                part, tot = new(eng.L.diffhe_robin_sum_blocks(n_f), B), new(rows.shape[0], B)
                for c in range(rows.shape[0]):
                    eng.L.diffhe_robin_sum_facets(rows[c], n_f, B, part, tot[c], st)
                o = tot.sum(dim=1) if dat.kind == SCALAR else tot.t()
            grads.append(None if o is None else o.reshape(dat.shape))
        return grads


_BOUNDS_ERROR = ("diffhe: a diagonal entry of the operator with its foundation is not positive and finite (a negative "
                 "stiffness?)")


def _facet_forward(solver: "TractionElasticFESolver", E, f, load, data, node_major):
    """(u, state) of one call with facet data (`data`: the four tensors, empty = absent): the shared call builder, with
    the facet table, the data as the kernels read them and the singular-system warning set up before the solve."""
    def prepare(state):
        plan, setup = state.plan, state.setup
        state.tab = tab = solver._table(plan)
        state.data = tuple(None if t.numel() == 0 else
                           _Datum.of(t, name, tab["n_f"], state.call.B, node_major, plan.device,
                                     plan.dim if name == "traction" else 0)
                           for t, name in zip(data, NAMES))
        if any(z is not None for z in state.data[2:]):
            state.bounds_error = _BOUNDS_ERROR         # a foundation: the smoother's bounds are measured per call
        if not setup.is_bc_host.any() and not any(z is not None and bool((z.dev > 0).any()) for z in state.data[2:]):
            warnings.warn("diffhe: the system is singular (a body with no fixed dof and no foundation stiffness > 0: its "
                          "rigid-body modes are free); the returned values are not a solution", RuntimeWarning)

    return _solve_call(solver, _FacetElasticSolve, E, f, load, node_major, prepare=prepare)


# ---------------------------------------------------------------------------------------------
# torch.library custom ops diffhe::elastic_facet_solve / diffhe::elastic_facet_solve_backward, next to
# diffhe::elastic_solve and on its shared plumbing (diffhe.elastic): the solver and the state of the call travel as integer
# handles through the registries of diffhe.solver.  f / load and the four facet data: empty tensor = absent.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("diffhe::elastic_facet_solve", mutates_args=())
def elastic_facet_solve(E: torch.Tensor, f: torch.Tensor, load: torch.Tensor, traction: torch.Tensor,
                        pressure: torch.Tensor, k_normal: torch.Tensor, k_tangent: torch.Tensor, handle: int, save: bool,
                        node_major: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u, token) of the `TractionElasticFESolver` registered under `handle`; arguments as diffhe::elastic_solve, plus the
    facet data in one of the layouts of the module docstring."""
    return _solve_result(*_facet_forward(_SOLVERS[handle], E, f, load, (traction, pressure, k_normal, k_tangent),
                                         node_major), save)


@elastic_facet_solve.register_fake
def _elastic_facet_solve_fake(E, f, load, traction, pressure, k_normal, k_tangent, handle, save, node_major):
    return _solve_fake(_SOLVERS[handle], E, f, load, node_major)


_Grads7 = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]


@torch.library.custom_op("diffhe::elastic_facet_solve_backward", mutates_args=())
def elastic_facet_solve_backward(gbar: torch.Tensor, token: torch.Tensor, need_e: bool, need_f: bool, need_load: bool,
                                 need_t: bool, need_p: bool, need_kn: bool, need_kt: bool, e_like: torch.Tensor,
                                 f_like: torch.Tensor, load_like: torch.Tensor, t_like: torch.Tensor,
                                 p_like: torch.Tensor, kn_like: torch.Tensor, kt_like: torch.Tensor) -> _Grads7:
    """The seven gradients of the forward call named by `token` from ONE adjoint solve, each with the device and dtype of
    its `*_like`; unused ones come back empty."""
    state, grads = _run_adjoint(gbar, token, need_e, need_f, need_load)
    facet_needs = (need_t, need_p, need_kn, need_kt)
    facet = state.facet_grads(facet_needs) if any(facet_needs) else [None] * 4
    return _like_grads(gbar, (*grads, *facet), (e_like, f_like, load_like, t_like, p_like, kn_like, kt_like))


@elastic_facet_solve_backward.register_fake
def _elastic_facet_solve_backward_fake(gbar, token, need_e, need_f, need_load, need_t, need_p, need_kn, need_kt, e_like,
                                       f_like, load_like, t_like, p_like, kn_like, kt_like):
    return _fake_grads(gbar, (need_e, need_f, need_load, need_t, need_p, need_kn, need_kt),
                       (e_like, f_like, load_like, t_like, p_like, kn_like, kt_like))


_setup_context, _backward = _solve_autograd(
    "elastic_facet_solve", 7, 10, "diffhe: second-order derivatives of an elastic solve with facet data are not "
    "implemented (backward with create_graph=True, diffhe.elastic_facets)")


# ---------------------------------------------------------------------------------------------
# The public solver
# ---------------------------------------------------------------------------------------------
class TractionElasticFESolver(ElasticFESolver):
    """`ElasticFESolver` with tractions, pressure and an elastic foundation sigma n = t - p n - S u on boundary facets and
    gradients with respect to t, p and the normal / tangential foundation stiffness (see the module docstring).

    facets : None (every boundary facet) or an index tensor into `mesh.boundary_facets()`.
    validate : check every call that the stiffnesses are finite and >= 0 (ValueError; one device synchronisation).
    """

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        from .elastic_aniso import AnisotropicElasticFESolver
        from .elastic_shape import ShapeElasticFESolver
        if issubclass(cls, (AnisotropicElasticFESolver, ShapeElasticFESolver)):
            raise NotImplementedError("diffhe: tractions, pressure and foundations together with a stiffness tensor or "
                                      "node gradients are not implemented")

    def __init__(self, mesh, E=1.0, nu: float = 0.3, *, plane: Optional[str] = None, fixed=None,
                 facets: Optional[torch.Tensor] = None, validate: bool = False, **options):
        super().__init__(mesh, E, nu, plane=plane, fixed=fixed, **options)      # refuses 1D and P2 meshes
        every = mesh.boundary_facets()
        self._facet_key = None
        if facets is not None:
            idx = torch.as_tensor(facets).detach().to("cpu", torch.long).reshape(-1)
            if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= every.shape[0]:
                raise ValueError(f"facets must be a non-empty index tensor into mesh.boundary_facets() ({every.shape[0]} "
                                 "facets)")
            every = every[idx]
            self._facet_key = hashlib.blake2b(idx.numpy().tobytes(), digest_size=16).hexdigest()
        self.facets = every                         # (n_F, d) node ids, the order the facet data are given in
        self._facets_host = every.numpy()
        self._opposite_host = opposite_nodes(mesh.elements.detach().to("cpu", torch.int64).numpy(), self._facets_host)
        self.facet_areas, self.facet_normals = facet_geometry(mesh.nodes, every, torch.from_numpy(self._opposite_host))
        self.validate = bool(validate)
        self.last_info = ElasticFacetInfo()

    @property
    def n_facets(self) -> int:
        return self.facets.shape[0]

    def _table(self, plan):
        tab = plan.elastic_facet_table(self._facet_key, self._facets_host, self._opposite_host)
        if tab is None:
            raise RuntimeError("diffhe: a facet couples two nodes that share no element")
        return tab

    def forward(self, f: Optional[torch.Tensor] = None, load: Optional[torch.Tensor] = None, traction=None, pressure=None,
                k_normal=None, k_tangent=None, layout: str = "sample", eigenstrain=None) -> torch.Tensor:
        """u as `ElasticFESolver.forward` returns it.  traction: (d,), (B, d), (n_F, d), (B, n_F, d) -- (n_F, d, B) with
        layout="node"; pressure, k_normal, k_tangent: (), (B,), (n_F,), (B, n_F) -- (n_F, B) with layout="node"; None:
        zero.  A datum with a batch and a facet axis implies the batch, like a (B, n, d) load.  All four None: exactly
        the base class's call."""
        data = [None if t is None else (t if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=torch.float64))
                for t in (traction, pressure, k_normal, k_tangent)]
        if all(t is None for t in data):
            return super().forward(f, load, layout, eigenstrain=eigenstrain)
        if layout not in ("sample", "node"):
            raise ValueError(f"Unknown layout: {layout!r}")
        if self.mesh.nodes.requires_grad:
            raise NotImplementedError("diffhe: facet data with moving nodes are not implemented (mesh.nodes requires "
                                      "grad: the normals and areas of a follower load would move with them)")
        d, node = self.mesh.dim, layout == "node"
        for t, name in zip(data, NAMES):
            if t is not None and (t.is_complex() or t.dim() > (3 if name == "traction" else 2)):
                raise ValueError(f"{name} must be a real tensor of at most {3 if name == 'traction' else 2} dimensions, "
                                 f"got {tuple(t.shape)} {t.dtype}")
        implied = [b for b in (_implied_batch(t, node, d if name == "traction" else 0) for t, name in zip(data, NAMES))
                   if b is not None]
        E = self._E
        # the facet data's device is u's when neither f nor load says it; an eigenstrain alone carries no batch here
        f_in, load_in, node = self._rhs_inputs(E, f, load, layout, eigenstrain=eigenstrain, eigenstrain_batch=False,
                                               implied=implied[0] if implied else None,
                                               where=next(t.device for t in data if t is not None))
        _, B, _ = _kappa_layout(E, self.mesh.n_elements, _batch_of(self, f_in, load_in, node)[0], node)
        for t, name in zip(data, NAMES):                       # the layout errors, before the op
            if t is not None:
                _kind_of(t, name, self.n_facets, B, node, d if name == "traction" else 0)
        if self.validate:
            for t, name in zip(data[2:], NAMES[2:]):
                if t is not None and not bool((torch.isfinite(t.detach()) & (t.detach() >= 0)).all()):
                    raise ValueError(f"diffhe: {name} must be finite and >= 0 everywhere (validate=True)")
        empty = E.new_empty(0)
        d_in = [empty if t is None else t.to(torch.float64) for t in data]
        _SOLVERS[id(self)] = self
        save = torch.is_grad_enabled() and any(t.requires_grad for t in (E, f_in, load_in, *d_in))
        u, _token = torch.ops.diffhe.elastic_facet_solve(E, f_in, load_in, *d_in, id(self), save, node)
        return u
