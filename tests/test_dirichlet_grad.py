"""Per-call Dirichlet values `forward(..., dirichlet=G)` and their gradients (diffhe.dirichlet, csrc/bc.hip): the ABI
entries, argument checks, a dense torch restatement with G differentiable (checked against finite differences), and on
the GPU -- every path, kappa layout and layout -- consistency with the mesh's own values, per-sample data against
separate solves, the restatement, exact identities at full size, batch sums, determinism, the single adjoint solve and
the plan that stays the same."""
import os
import re

import numpy as np
import pytest
import torch

from diffhe import DifferentiableFESolver, FEMesh, ShapeDifferentiableFESolver, _hip
from diffhe import solver as solver_mod
from diffhe.plan import _fingerprint, reference_order_integrals
from diffhe.tet3d import DifferentiableFESolver3D
from _util import RTOL_GRAD, RTOL_U

T64 = torch.float64
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "diffhe_hip.h")
BC_ENTRIES = ("diffhe_bc_lift", "diffhe_bc_grad", "diffhe_bc_scatter", "diffhe_bc_grad_kappa")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def _with_bc(mesh, fn):
    """mesh with Dirichlet values fn(x) (varying along the boundary), inserted in DESCENDING node order."""
    X = mesh.nodes.numpy()
    keys = sorted(mesh.dirichlet_nodes.keys(), reverse=True)
    return FEMesh(nodes=mesh.nodes, elements=mesh.elements, dirichlet_nodes={k: float(fn(X[k])) for k in keys})


def _jittered(mesh, amount, seed):
    """mesh with its interior nodes moved by up to `amount` cells at random."""
    rng = np.random.default_rng(seed)
    X = mesh.nodes.numpy().copy()
    h = (X.max(0) - X.min(0)) / np.array([len(np.unique(np.round(X[:, k], 12))) - 1 for k in range(X.shape[1])])
    move = rng.uniform(-amount, amount, X.shape) * h
    move[list(mesh.dirichlet_nodes)] = 0.0
    return FEMesh(nodes=torch.from_numpy(X + move), elements=mesh.elements, dirichlet_nodes=dict(mesh.dirichlet_nodes))


# ------------------------------------------------------------------------------------------------
# dense restatement: unreduced K_b, G differentiable
# ------------------------------------------------------------------------------------------------
def _dense_solve(k0, m0, el, mass, d_idx, kappa_be, f_bn, G_bd, load_bn=None, c=0.0):
    """u (B, n) of (K_b + c M_L) u = M f_b + load_b on the free rows, u = G_b on the Dirichlet nodes, K_b = sum_e
    kappa_eb k0_e unreduced; k0, m0 (m, npe, npe), el (m, npe), mass (n,) lumped.  Plain torch: autograd through
    torch.linalg.solve for kappa, f, load and G."""
    n, B = mass.shape[0], f_bn.shape[0]
    m, npe = el.shape
    idx = (el[:, :, None] * n + el[:, None, :]).reshape(-1)
    K = torch.zeros(B, n * n, dtype=T64).index_add(1, idx, (kappa_be[:, :, None, None] * k0[None]).reshape(B, -1))
    K = K.reshape(B, n, n)
    M = torch.zeros(n * n, dtype=T64).index_add(0, idx, m0.reshape(-1)).reshape(n, n)
    is_d = torch.zeros(n, dtype=torch.bool)
    is_d[d_idx] = True
    F = torch.nonzero(~is_d).reshape(-1)
    A = K + c * torch.diag(mass)
    rhs = f_bn @ M + (load_bn if load_bn is not None else 0.0)
    rhsF = rhs[:, F] - (K[:, F][:, :, d_idx] @ G_bd.unsqueeze(2)).squeeze(2)
    xF = torch.linalg.solve(A[:, F][:, :, F], rhsF)
    return torch.zeros(B, n, dtype=T64).index_copy(1, F, xF).index_copy(1, d_idx, G_bd)


def _host_tables_2d(mesh):
    """(k0, m0, el, mass) of a P1 triangle mesh on the host (reference-order integrals, area / 9 load map)."""
    coords = np.ascontiguousarray(mesh.nodes.numpy().T)
    el = mesh.elements.numpy()
    t, den = reference_order_integrals(coords, el.T)
    k0 = torch.from_numpy((t / den).T.reshape(-1, 3, 3).copy())
    area = den / 4.0
    m0 = torch.from_numpy(np.repeat((area / 9.0)[:, None], 9, 1).reshape(-1, 3, 3))
    mass = torch.zeros(mesh.n_nodes, dtype=T64).index_add(0, mesh.elements.reshape(-1),
                                                          torch.from_numpy(np.repeat(area / 3.0, 3)))
    return k0, m0, mesh.elements.long(), mass


def _plan_tables(solver):
    """(k0, m0, el, mass) of the solve's own plan, on the host."""
    plan = solver._plan()
    plan.ensure_ell()
    npe = plan.npe
    k0 = plan.k0.t().reshape(-1, npe, npe).cpu()
    m0 = plan.m0.t().reshape(-1, npe, npe).cpu()
    return k0, m0, plan.elems.long().t().cpu(), plan.lumped_mass().cpu()


# ------------------------------------------------------------------------------------------------
# CPU: ABI, mesh helpers, the restatement against finite differences, argument checks
# ------------------------------------------------------------------------------------------------
def test_abi_lists_the_dirichlet_entries():
    src = open(HEADER).read()
    m = re.search(r"#define\s+DIFFHE_ABI_VERSION\s+(\d+)", src)
    assert m and int(m.group(1)) == _hip.ABI_VERSION
    for name in BC_ENTRIES:     # their signatures: tests/test_abi.py, with every other entry's
        assert name in _hip.SIGNATURES


def test_dirichlet_index_and_values_are_in_ascending_node_order():
    mesh = FEMesh(nodes=torch.linspace(0, 1, 6, dtype=T64).unsqueeze(1),
                  elements=torch.stack([torch.arange(5), torch.arange(1, 6)], 1),
                  dirichlet_nodes={5: -2.0, 0: 1.5, 3: 0.25})
    assert mesh.dirichlet_index().tolist() == [0, 3, 5]
    assert mesh.dirichlet_index().dtype == torch.long
    v = mesh.dirichlet_values()
    assert v.dtype == T64 and v.tolist() == [1.5, 0.25, -2.0]
    rect = _with_bc(FEMesh.rectangle(4, 3), lambda x: x[0] + 10 * x[1])
    idx = rect.dirichlet_index()
    assert torch.equal(idx, torch.sort(idx).values)
    assert rect.dirichlet_values().tolist() == [rect.dirichlet_nodes[int(k)] for k in idx]


def test_fingerprint_does_not_see_dirichlet_argument():
    mesh = _with_bc(FEMesh.rectangle(4, 4), lambda x: x[0])
    solver = DifferentiableFESolver(mesh, 1.0)
    before = _fingerprint(mesh)
    for G in (torch.zeros(len(mesh.dirichlet_nodes), dtype=T64), torch.randn(3, len(mesh.dirichlet_nodes), dtype=T64)):
        solver._dirichlet64(G, None, False)
    assert _fingerprint(mesh) == before
    assert dict(mesh.dirichlet_nodes) == {k: float(mesh.nodes[k, 0]) for k in mesh.dirichlet_nodes}


@pytest.mark.parametrize("c", [0.0, 2.0])
def test_dense_restatement_matches_finite_differences(c):
    mesh = _with_bc(_jittered(FEMesh.rectangle(3, 3), 0.2, 1), lambda x: 0.3 + x[0] * x[1])
    k0, m0, el, mass = _host_tables_2d(mesh)
    d_idx = mesh.dirichlet_index()
    gen = torch.Generator().manual_seed(0)
    B, m, n, nd = 2, mesh.n_elements, mesh.n_nodes, len(d_idx)
    kap = (1 + 0.5 * torch.rand(B, m, generator=gen, dtype=T64)).requires_grad_()
    f = torch.randn(B, n, generator=gen, dtype=T64, requires_grad=True)
    G = torch.randn(B, nd, generator=gen, dtype=T64, requires_grad=True)
    w = torch.randn(B, n, generator=gen, dtype=T64)
    assert torch.autograd.gradcheck(lambda k, ff, g: (w * _dense_solve(k0, m0, el, mass, d_idx, k, ff, g, c=c)).sum(),
                                    (kap, f, G), eps=1e-6, atol=1e-7, rtol=1e-6)
    u = _dense_solve(k0, m0, el, mass, d_idx, kap, f, G, c=c)
    assert torch.equal(u[:, d_idx], G)


def test_wrong_dirichlet_shapes_raise_value_error():
    mesh = FEMesh.rectangle(4, 4, bc_value=1.0)
    n, nd = mesh.n_nodes, len(mesh.dirichlet_nodes)
    solver = DifferentiableFESolver(mesh, 1.0)
    f = torch.ones(3, n, dtype=T64)
    for bad in (torch.zeros(nd + 1, dtype=T64), torch.zeros(2, nd, dtype=T64), torch.zeros(3, nd - 1, dtype=T64),
                torch.zeros(1, 3, nd, dtype=T64)):
        with pytest.raises(ValueError):
            solver(f, dirichlet=bad)
    with pytest.raises(ValueError):
        solver(f.t().contiguous(), layout="node", dirichlet=torch.zeros(3, nd, dtype=T64))       # (B, n_D) in node
    with pytest.raises(ValueError):
        solver(f.t().contiguous(), layout="node", dirichlet=torch.zeros(nd, 2, dtype=T64))
    line = FEMesh.line(10, bc_left=1.0, bc_right=2.0)
    with pytest.raises(ValueError):
        DifferentiableFESolver(line, 1.0)(torch.ones(2, 11, dtype=T64), dirichlet=torch.zeros(2, 3, dtype=T64))


def test_dirichlet_with_node_gradients_raises():
    base = FEMesh.rectangle(4, 4, bc_value=1.0)
    mesh = FEMesh(nodes=base.nodes.clone().requires_grad_(True), elements=base.elements,
                  dirichlet_nodes=base.dirichlet_nodes)
    solver = ShapeDifferentiableFESolver(mesh, 1.0)
    with pytest.raises(NotImplementedError):
        solver(torch.ones(mesh.n_nodes, dtype=T64), dirichlet=mesh.dirichlet_values())


# ------------------------------------------------------------------------------------------------
# GPU cases: every path
# ------------------------------------------------------------------------------------------------
def _case(kind):
    """(solver class, mesh, options) of one path."""
    if kind == "chain":
        return DifferentiableFESolver, _with_bc(FEMesh.line(40, bc_left=0.0, bc_right=0.0), lambda x: 1.5 - 2 * x[0]), {}
    if kind == "chain-reaction":       # the chain with a reaction term takes the general path
        return DifferentiableFESolver, _with_bc(FEMesh.line(40), lambda x: 1.5 - 2 * x[0]), dict(reaction=3.0)
    if kind == "lattice-direct":
        return DifferentiableFESolver, _with_bc(FEMesh.rectangle(16, 12), lambda x: 0.7 + x[0] - x[1] ** 2), {}
    rect = _with_bc(FEMesh.rectangle(48, 40), lambda x: 0.7 + x[0] - x[1] ** 2)
    if kind == "lattice":
        return DifferentiableFESolver, rect, {}
    if kind == "lattice-assembled":
        return DifferentiableFESolver, rect, dict(operator="assembled")
    if kind == "lattice-reaction":
        return DifferentiableFESolver, rect, dict(reaction=2.0)
    if kind == "lattice-warm":
        return DifferentiableFESolver, rect, dict(warm_start=True)
    if kind == "ell":
        return DifferentiableFESolver, _with_bc(_jittered(FEMesh.rectangle(20, 16), 0.25, 3), lambda x: x[0] * x[1] - 0.2), {}
    if kind == "ell-lattice":
        return DifferentiableFESolver, _with_bc(FEMesh.rectangle(24, 24), lambda x: 0.5 + x[1]), dict(method="ell")
    if kind == "p2":
        return DifferentiableFESolver, _with_bc(FEMesh.rectangle_p2(6, 6), lambda x: 0.3 + x[0] ** 2), {}
    if kind == "box":
        return DifferentiableFESolver3D, _with_bc(FEMesh.box(5, 5, 5), lambda x: 0.4 + x[2] - x[0]), {}
    raise KeyError(kind)


KINDS = ("chain", "chain-reaction", "lattice-direct", "lattice", "lattice-assembled", "lattice-reaction", "lattice-warm",
         "ell", "ell-lattice", "p2", "box")
KMODES = ("scalar", "sample", "elem", "sample_elem")


def _kappa(kmode, B, m, seed):
    gen = torch.Generator().manual_seed(seed)
    if kmode == "scalar":
        k = torch.tensor(1.3, dtype=T64)
    elif kmode == "sample":
        k = 0.6 + torch.rand(B, generator=gen, dtype=T64)
    elif kmode == "elem":
        k = 0.6 + torch.rand(m, generator=gen, dtype=T64)
    else:
        k = 0.6 + torch.rand(B, m, generator=gen, dtype=T64)
    return k.to(DEV).requires_grad_(True)


def _inputs(mesh, B, seed):
    gen = torch.Generator().manual_seed(seed)
    n = mesh.n_nodes
    f = (1 + torch.randn(B, n, generator=gen, dtype=T64)).to(DEV).requires_grad_(True)
    load = (0.1 * torch.randn(B, n, generator=gen, dtype=T64)).to(DEV).requires_grad_(True)
    w = torch.randn(B, n, generator=gen, dtype=T64).to(DEV)
    return f, load, w


def _run(cls, mesh, opts, kappa, f, load, w, G=None, layout="sample"):
    """(u, dkappa, df, dload, dG) of L = sum w u."""
    solver = cls(mesh, kappa, device=DEV, **opts)
    if layout == "node":
        u = solver(f.t(), load=load.t(), layout="node", dirichlet=None if G is None else (G if G.dim() == 1 else G.t()))
        u = u.t()
    else:
        u = solver(f, load=load, dirichlet=G)
    inputs = [kappa, f, load] + ([G] if G is not None and G.requires_grad else [])
    grads = torch.autograd.grad((w * u).sum(), inputs)
    return (u.detach(),) + tuple(grads) + ((None,) if len(grads) == 3 else ())


@pytest.mark.gpu
@pytest.mark.parametrize("kmode", KMODES)
@pytest.mark.parametrize("kind", KINDS)
def test_mesh_values_as_argument_match_the_mesh_solve(kind, kmode):
    cls, mesh, opts = _case(kind)
    B = 3
    kappa = _kappa(kmode, B, mesh.n_elements, 1)
    f, load, w = _inputs(mesh, B, 2)
    ref = _run(cls, mesh, opts, kappa, f, load, w)
    got = _run(cls, mesh, opts, kappa, f, load, w, G=mesh.dirichlet_values().to(DEV))
    errs = {name: _rel(a, b) for name, a, b in zip(("u", "dkappa", "df", "dload"), got[:4], ref[:4])}
    print(f"{kind}/{kmode}: {errs}")
    assert errs["u"] < RTOL_U and max(errs["dkappa"], errs["df"], errs["dload"]) < RTOL_GRAD, errs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("chain", "lattice", "lattice-reaction", "ell", "p2", "box"))
def test_node_layout_matches_sample_layout(kind):
    cls, mesh, opts = _case(kind)
    B = 3
    kappa = _kappa("sample_elem", B, mesh.n_elements, 3)
    f, load, w = _inputs(mesh, B, 4)
    gen = torch.Generator().manual_seed(5)
    G = torch.randn(B, len(mesh.dirichlet_nodes), generator=gen, dtype=T64).to(DEV).requires_grad_(True)
    a = _run(cls, mesh, opts, kappa, f, load, w, G)
    b = _run(cls, mesh, opts, kappa, f, load, w, G, layout="node")
    errs = [_rel(x, y) for x, y in zip(b, a)]
    print(kind, errs)
    assert max(errs) < RTOL_GRAD, errs


@pytest.mark.gpu
@pytest.mark.parametrize("kmode", ("sample", "sample_elem"))
@pytest.mark.parametrize("kind", ("chain", "lattice", "lattice-assembled", "ell", "ell-lattice", "p2", "box"))
def test_per_sample_values_match_separate_solves(kind, kmode):
    cls, mesh, opts = _case(kind)
    B = 3
    kappa = _kappa(kmode, B, mesh.n_elements, 6)
    f, load, w = _inputs(mesh, B, 7)
    gen = torch.Generator().manual_seed(8)
    keys = mesh.dirichlet_index().tolist()
    G = (mesh.dirichlet_values() + torch.randn(B, len(keys), generator=gen, dtype=T64)).to(DEV)
    u, dk, df, _dl, _ = _run(cls, mesh, opts, kappa, f, load, w, G)
    worst = 0.0
    for b in range(B):
        mesh_b = FEMesh(nodes=mesh.nodes, elements=mesh.elements, dirichlet_nodes=dict(zip(keys, G[b].tolist())))
        kb = kappa.detach()[b:b + 1].clone().requires_grad_(True)
        fb = f.detach()[b:b + 1].clone().requires_grad_(True)
        ub = cls(mesh_b, kb, device=DEV, **opts)(fb, load=load.detach()[b:b + 1])
        dkb, dfb = torch.autograd.grad((w[b:b + 1] * ub).sum(), (kb, fb))
        e = (_rel(u[b], ub[0]), _rel(dk[b], dkb[0]), _rel(df[b], dfb[0]))
        worst = max(worst, *e)
        assert e[0] < RTOL_U and max(e[1:]) < RTOL_GRAD, (b, e)
    print(f"{kind}/{kmode}: worst {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("kmode", ("sample", "sample_elem", "elem", "scalar"))
@pytest.mark.parametrize("kind", ("chain", "lattice-direct", "lattice-reaction", "ell", "p2", "box", "chain-reaction"))
def test_gradients_match_dense_restatement(kind, kmode):
    cls, mesh, opts = _case(kind)
    if kind == "box":
        mesh = _with_bc(FEMesh.box(4, 4, 4), lambda x: 0.4 + x[2] - x[0])
    if kind == "p2":
        mesh = _with_bc(FEMesh.rectangle_p2(4, 4), lambda x: 0.3 + x[0] ** 2)
    B, m, nd = 2, mesh.n_elements, len(mesh.dirichlet_nodes)
    kappa = _kappa(kmode, B, m, 9)
    f, load, w = _inputs(mesh, B, 10)
    gen = torch.Generator().manual_seed(11)
    G = torch.randn(B, nd, generator=gen, dtype=T64).to(DEV).requires_grad_(True)
    u, dk, df, dl, dG = _run(cls, mesh, opts, kappa, f, load, w, G)
    solver = cls(mesh, kappa, device=DEV, **opts)
    k0, m0, el, mass = _plan_tables(solver)
    kc = kappa.detach().cpu().clone().requires_grad_(True)
    k_be = {"scalar": lambda k: k.expand(B, m), "sample": lambda k: k[:, None].expand(B, m),
            "elem": lambda k: k[None].expand(B, m), "sample_elem": lambda k: k}[kmode](kc)
    fc, lc, Gc = (t.detach().cpu().clone().requires_grad_(True) for t in (f, load, G))
    ud = _dense_solve(k0, m0, el, mass, mesh.dirichlet_index(), k_be, fc, Gc, lc, c=opts.get("reaction", 0.0))
    dkd, dfd, dld, dGd = torch.autograd.grad((w.cpu() * ud).sum(), (kc, fc, lc, Gc))
    errs = dict(u=_rel(u, ud), dk=_rel(dk, dkd), df=_rel(df, dfd), dload=_rel(dl, dld), dG=_rel(dG, dGd))
    print(f"{kind}/{kmode}: {errs}")
    assert errs["u"] < RTOL_U and max(v for k, v in errs.items() if k != "u") < RTOL_GRAD, errs


def _identity_check(cls, mesh, opts, kappa, B, layout="sample"):
    """u(G + t) = u(G) + t and sum_j dL/dG_j = sum_i w_i (K 1 = 0, no reaction) per sample."""
    n, nd = mesh.n_nodes, len(mesh.dirichlet_nodes)
    gen = torch.Generator().manual_seed(12)
    f = torch.ones(n, dtype=T64, device=DEV)
    G = (torch.rand(B, nd, generator=gen, dtype=T64) - 0.5).to(DEV).requires_grad_(True)
    t = torch.linspace(-1.0, 2.0, B, dtype=T64, device=DEV)
    w = torch.randn(B, n, generator=gen, dtype=T64).to(DEV)
    solver = cls(mesh, kappa, device=DEV, **opts)
    u = solver(f, dirichlet=G)
    (dG,) = torch.autograd.grad((w * u).sum(), (G,))
    with torch.no_grad():
        u2 = solver(f, dirichlet=G + t[:, None])
    e_shift = float(((u2 - u.detach() - t[:, None]).abs().amax(1) / (u.detach().abs().amax(1) + t.abs())).max())
    e_sum = float(((dG.sum(1) - w.sum(1)).abs() / w.abs().sum(1)).max())
    print(f"n={n} B={B} path={solver.last_info.path}: shift {e_shift:.2e}, gradient sum {e_sum:.2e}")
    assert e_shift < RTOL_U and e_sum < RTOL_GRAD, (e_shift, e_sum)


@pytest.mark.gpu
@pytest.mark.parametrize("kmode", ("sample", "sample_elem"))
def test_exact_identities_lattice_1024(kmode):
    mesh = FEMesh.rectangle(1024, 1024, bc_value=0.0)
    B = 256
    kappa = _kappa(kmode, B, mesh.n_elements, 13).detach()
    _identity_check(DifferentiableFESolver, mesh, {}, kappa, B)


@pytest.mark.gpu
def test_exact_identities_general_512():
    mesh = _jittered(FEMesh.rectangle(512, 512), 0.2, 14)
    _identity_check(DifferentiableFESolver, mesh, dict(method="ell"), _kappa("sample", 8, mesh.n_elements, 15).detach(), 8)


@pytest.mark.gpu
def test_exact_identities_box48():
    mesh = FEMesh.box(48, 48, 48)
    _identity_check(DifferentiableFESolver3D, mesh, {}, _kappa("sample_elem", 4, mesh.n_elements, 16).detach(), 4)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("chain", "lattice", "ell", "box"))
def test_shared_values_get_the_batch_sum(kind):
    cls, mesh, opts = _case(kind)
    B, nd = 3, len(mesh.dirichlet_nodes)
    kappa = _kappa("sample", B, mesh.n_elements, 17)
    f, load, w = _inputs(mesh, B, 18)
    g0 = mesh.dirichlet_values().to(DEV) + 0.1
    shared = g0.clone().requires_grad_(True)
    per = g0.expand(B, nd).clone().requires_grad_(True)
    us = _run(cls, mesh, opts, kappa, f, load, w, shared)
    up = _run(cls, mesh, opts, kappa, f, load, w, per)
    assert _rel(us[0], up[0]) < RTOL_U
    assert _rel(us[4], up[4].sum(0)) < RTOL_GRAD


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("chain", "lattice", "ell-lattice", "p2", "box"))
def test_deterministic_one_adjoint_solve_and_same_plan(kind, monkeypatch):
    cls, mesh, opts = _case(kind)
    B, nd = 3, len(mesh.dirichlet_nodes)
    kappa = _kappa("sample_elem", B, mesh.n_elements, 19)
    f, load, w = _inputs(mesh, B, 20)
    gen = torch.Generator().manual_seed(21)
    G = torch.randn(B, nd, generator=gen, dtype=T64).to(DEV).requires_grad_(True)
    a = _run(cls, mesh, opts, kappa, f, load, w, G)
    b = _run(cls, mesh, opts, kappa, f, load, w, G)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    solver = cls(mesh, kappa, device=DEV, **opts)
    plan = solver._plan()
    calls = []
    for path in (solver_mod._ChainSolve, solver_mod._LatticeSolve, solver_mod._EllSolve):
        orig = path.adjoint

        def counting(self, *args, _orig=orig):
            calls.append(type(self).__name__)
            return _orig(self, *args)
        monkeypatch.setattr(path, "adjoint", counting)
    u = solver(f, load=load, dirichlet=G)
    torch.autograd.grad((w * u).sum(), (kappa, f, load, G))
    assert len(calls) == 1, calls
    for s in range(3):
        with torch.no_grad():
            solver(f, dirichlet=G + s)
        assert solver._plan() is plan
    assert len(mesh.__dict__["_diffhe_plans"]) == 1


@pytest.mark.gpu
def test_second_order_through_dirichlet_raises_and_kappa_second_order_runs():
    cls, mesh, opts = _case("lattice-direct")
    kappa = torch.tensor([1.1, 0.9], dtype=T64, device=DEV, requires_grad=True)
    f = torch.ones(2, mesh.n_nodes, dtype=T64, device=DEV)
    G = mesh.dirichlet_values().to(DEV).requires_grad_(True)
    solver = cls(mesh, kappa, device=DEV, **opts)
    u = solver(f, dirichlet=G)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad((u ** 2).sum(), (kappa, G), create_graph=True)
    # G held fixed: a Hessian-vector product in kappa goes through the differentiable restatement, with G in u
    Gf = G.detach()
    (gk,) = torch.autograd.grad((solver(f, dirichlet=Gf) ** 2).sum(), (kappa,), create_graph=True)
    (gk_ref,) = torch.autograd.grad((solver(f) ** 2).sum(), (kappa,), create_graph=True)
    assert _rel(gk, gk_ref) < RTOL_GRAD
    h = torch.autograd.grad(gk.sum(), (kappa,))[0]
    h_ref = torch.autograd.grad(gk_ref.sum(), (kappa,))[0]
    assert _rel(h, h_ref) < 1e-8
