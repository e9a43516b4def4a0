"""Vibration modes of elastic bodies, K(E) phi = lambda M(rho) phi per sample, with d lambda / dE and d lambda / d rho
(diffhe.modal.ElasticEigenSolver, csrc/modal.hip, the per-sample-mass entries of csrc/eigen.hip, include/diffhe_modal.h).

The yardstick is a dense restatement written here (`dense_modes`), independent of the product code: the raw stiffness in
strain-displacement form from the helpers of tests/test_elasticity.py (K_e = vol_e E_e B^T D B), the nodal lumped mass
from rho_e vol_e / (d + 1), M^-1/2 K M^-1/2 on the free dofs, `torch.linalg.eigh`, autograd for the gradients.  The CPU
tests pin it (rigid-body modes, total mass, the two homogeneities, the count of zero eigenvalues of a free body) and check
the Hellmann-Feynman formulas, the host logic and the fifth signature table; the GPU tests hold the kernels and the
solver against it.

Tolerances, with their reasons (those of tests/test_eigen.py carry over):
  * eigenvalues: RTOL_U (1e-10) per eigenvalue with tol = 1e-8 -- |lambda - theta| <= rho^2 lambda^2 / gap is far below it,
    so this is the operator tolerance.  Rigid-body eigenvalues of a free body: |lambda| <= RTOL_U x the first elastic one;
  * eigenvectors of isolated eigenvalues, sign-aligned: max-norm error relative to |phi|_inf <= 10 tol (lambda_i + shift) /
    gap_i (Davis-Kahan; the residual the iteration stops on is relative to the eigenvalue lambda + shift of the operator it
    runs on).  The rigid-body cluster: its M-orthogonal projector, same bound with the gap of the cluster.  Every test
    computes the gaps from its dense spectrum and asserts the smallest relative gap of the modes it checks >= 1e-2, so a
    changed input cannot make the bound vacuous;
  * per-element gradients are first order in the eigenvector error: tol = 1e-11 and the same 10 tol lambda_i / gap_i;
    homogeneity (E_b d lambda / dE_b = lambda, rho_b d lambda / d rho_b = -lambda) is second order: RTOL_GRAD;
  * central differences, step 1e-5, tolerance 1e-7: the reasoning in the header of tests/test_robin.py;
  * kernels alone (mass, per-element d / d rho, the four block passes): 1e-12 relative to the largest reference entry --
    sums of at most a few hundred fp64 terms of one sign (mass, Gram diagonal, residual) or of order-one random terms.
    The per-sample and batch-shared TOTALS of d / d rho sum up to m or B m terms of mixed sign: 1e-11, as the totals of
    dL/dE in tests/test_stress.py.

`test_restatement_is_pinned` and `test_hellmann_feynman_formulas_equal_autograd` exercise the yardstick alone: they pin
what the other tests compare against and would pass without the product code, were it not for this module's import of
`diffhe.modal`.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from diffhe import FEMesh, _hip
from diffhe import modal
from _util import RTOL_GRAD, RTOL_U, rel_err
from test_elasticity import _box, _dense_K, _geometry, _left_nodes, _rand, _rect, _strain_matrix, _voigt_D
from test_stress import BY_VALUE, _declarations

T64 = torch.float64
DEV = "cuda:0"
NU = 0.3
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffhe_modal.h")
NAMES = ["diffhe_modal_fix_sign", "diffhe_modal_grad_rho", "diffhe_modal_grad_rho_shared", "diffhe_modal_gram",
         "diffhe_modal_mass", "diffhe_modal_residual", "diffhe_modal_rotate"]
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# the dense restatement
# ---------------------------------------------------------------------------------------------------------------------
def dense_mass(mesh, rho_bm):
    """(B, n) nodal lumped mass of rho (B, m): every vertex of element e gets rho_e vol_e / (d + 1)."""
    el = mesh.elements.long()
    npe = el.shape[1]
    _, vol = _geometry(mesh.nodes.to(T64), el)
    share = (rho_bm * vol / npe)[:, :, None].expand(-1, -1, npe).reshape(rho_bm.shape[0], -1)
    return torch.zeros(rho_bm.shape[0], mesh.n_nodes, dtype=T64).index_add(1, el.reshape(-1), share)


def fixed_dofs(mesh, fixed):
    return np.array(sorted(i * mesh.dim + a for i, a in fixed), dtype=np.int64)


def dense_modes(mesh, E_m, rho_m, plane, fixed):
    """All eigenpairs on the free dofs: lam (nf,) ascending, phi (nf, n d) M-orthonormal and zero on the fixed dofs, the
    mass per dof (n d,).  Differentiable in E_m (m,) and rho_m (m,)."""
    nd = mesh.n_nodes * mesh.dim
    K = _dense_K(mesh, E_m[None], NU, plane)[0]
    md = dense_mass(mesh, rho_m[None])[0].repeat_interleave(mesh.dim)
    free = torch.from_numpy(np.setdiff1d(np.arange(nd), fixed_dofs(mesh, fixed)))
    s = md[free] ** -0.5
    S = s[:, None] * K[free][:, free] * s[None, :]
    lam, V = torch.linalg.eigh(0.5 * (S + S.t()))
    phi = torch.zeros(len(lam), nd, dtype=T64).index_add(1, free, (s[:, None] * V).t())
    return lam, phi, md


def rel_gaps(lam_all, idx):
    """Distance of lam_all[i] to the nearest other eigenvalue over lam_all[i], i in idx."""
    lam_all = np.asarray(lam_all)
    return np.array([np.min(np.abs(np.delete(lam_all, i) - lam_all[i])) / abs(lam_all[i]) for i in idx])


def rigid_modes(mesh):
    X, (n, d) = mesh.nodes.to(T64), mesh.nodes.shape
    modes = [torch.eye(d, dtype=T64)[a].expand(n, d) for a in range(d)]
    for a in range(d):
        for b in range(a + 1, d):
            r = torch.zeros(n, d, dtype=T64)
            r[:, a], r[:, b] = -X[:, b], X[:, a]
            modes.append(r)
    return [r.reshape(-1) for r in modes]


def rect2d(seed=21):
    """The jittered rectangle(8, 6) on [0, 2] x [0, 1] and its clamped left edge."""
    mesh = _rect(8, 6, seed, x_range=(0.0, 2.0))
    return mesh, {(i, a): 0.0 for i in _left_nodes(8, 6) for a in range(2)}


def box3d(seed=22):
    """The jittered box(3, 3, 3) and its clamped x = 0 face."""
    mesh = _box(3, 3, 3, seed)
    face = [i for i in range(mesh.n_nodes) if float(FEMesh.box(3, 3, 3).nodes[i, 0]) == 0.0]
    return mesh, {(i, a): 0.0 for i in face for a in range(3)}


CASES = {"2d-stress": (rect2d, "stress"), "2d-strain": (rect2d, "strain"), "3d": (box3d, None)}


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement pinned
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_restatement_is_pinned(key):
    make, plane = CASES[key]
    mesh, _ = make()
    n, d, m = mesh.n_nodes, mesh.dim, mesh.n_elements
    E, rho = _rand((m,), 1, 0.5, 2.0), _rand((m,), 2, 0.5, 2.0)
    K = _dense_K(mesh, E[None], NU, plane)[0]
    nr = d + d * (d - 1) // 2
    modes = rigid_modes(mesh)
    assert len(modes) == nr
    bound = 1e-13 * float(K.abs().max()) * float(mesh.nodes.abs().max())
    for r in modes:                                         # raw K annihilates the rigid-body modes
        assert float((K @ r).abs().max()) <= bound
    _, vol = _geometry(mesh.nodes.to(T64), mesh.elements.long())
    mass = dense_mass(mesh, rho[None])[0]
    assert abs(float(mass.sum() - (rho * vol).sum())) <= 1e-13 * float((rho * vol).sum())     # total mass per component
    one = dense_mass(mesh, torch.ones(1, m, dtype=T64))[0]
    assert abs(float(one.sum() - vol.sum())) <= 1e-13 * float(vol.sum())
    lam, phi, md = dense_modes(mesh, E, rho, plane, {})
    lam_e = dense_modes(mesh, 2.5 * E, rho, plane, {})[0]
    lam_r = dense_modes(mesh, E, 2.5 * rho, plane, {})[0]
    first = float(lam[nr])
    print(f"{key}: rigid |lambda| max {float(lam[:nr].abs().max()):.2e}, first elastic {first:.4e}")
    assert int((lam < 1e-10 * first).sum()) == nr            # exactly 3 / 6 zero eigenvalues of the free body
    assert float(lam[:nr].abs().max()) <= 1e-12 * first
    assert rel_err(lam_e[nr:].numpy(), 2.5 * lam[nr:].numpy()) <= 1e-11     # lambda(cE, rho) = c lambda
    assert rel_err(lam_r[nr:].numpy(), lam[nr:].numpy() / 2.5) <= 1e-11     # lambda(E, c rho) = lambda / c
    G = (phi * md) @ phi.t()
    assert rel_err(G.numpy(), np.eye(len(lam))) <= 1e-12


@pytest.mark.parametrize("key", list(CASES))
def test_hellmann_feynman_formulas_equal_autograd(key):
    make, plane = CASES[key]
    mesh, fixed = make()
    m, d = mesh.n_elements, mesh.dim
    E = _rand((m,), 3, 0.5, 2.0).requires_grad_(True)
    rho = _rand((m,), 4, 0.5, 2.0).requires_grad_(True)
    lam, phi, _ = dense_modes(mesh, E, rho, plane, fixed)
    el = mesh.elements.long()
    G, vol = _geometry(mesh.nodes.to(T64), el)
    dof = (el[:, :, None] * d + torch.arange(d)[None, None, :]).reshape(m, -1)
    Bm = _strain_matrix(G)
    k0 = vol[:, None, None] * (Bm.transpose(1, 2) @ _voigt_D(NU, d, plane) @ Bm)
    for i in range(5):
        gE, gr = torch.autograd.grad(lam[i], (E, rho), retain_graph=True)
        pe = phi[i].detach()[dof]                                                  # (m, npe d)
        hf_E = torch.einsum("ep,epq,eq->e", pe, k0, pe)
        hf_r = -lam[i].detach() * vol / (d + 1) * (pe ** 2).sum(1)
        assert rel_err(hf_E.numpy(), gE.numpy()) <= RTOL_GRAD
        assert rel_err(hf_r.numpy(), gr.numpy()) <= RTOL_GRAD


# ---------------------------------------------------------------------------------------------------------------------
# CPU: host logic
# ---------------------------------------------------------------------------------------------------------------------
def test_import_from_the_package():
    import diffhe
    from diffhe import ElasticEigenSolver
    assert "ElasticEigenSolver" in diffhe.__all__ and ElasticEigenSolver is modal.ElasticEigenSolver is diffhe.modal.ElasticEigenSolver
    lam = torch.tensor([-1e-14, 0.0, 4.0 * np.pi ** 2], dtype=T64, requires_grad=True)
    f = modal.frequency(lam)
    assert f.tolist() == [0.0, 0.0, pytest.approx(1.0, abs=1e-15)]
    f.sum().backward()                  # a loss over all modes, rigid-body ones included: derivative 0 there, no NaN
    assert lam.grad[:2].tolist() == [0.0, 0.0]
    assert abs(float(lam.grad[2]) - 1.0 / (8.0 * np.pi ** 2)) <= 1e-15


def test_refusals_and_argument_validation():
    from diffhe import ElasticEigenSolver
    with pytest.raises(NotImplementedError, match="1D"):
        ElasticEigenSolver(FEMesh.line(10))
    with pytest.raises(NotImplementedError, match="P1"):
        ElasticEigenSolver(FEMesh.rectangle_p2(4, 4))
    with pytest.raises(ValueError, match="plane="):
        ElasticEigenSolver(FEMesh.box(2, 2, 2), plane="strain")
    mesh = FEMesh.rectangle(6, 5)
    m = mesh.n_elements
    with pytest.raises(NotImplementedError, match="strength"):
        ElasticEigenSolver(mesh, amg=dict(strength=0.25))
    with pytest.raises(ValueError, match="plane"):
        ElasticEigenSolver(mesh, plane="membrane")
    with pytest.raises(ValueError, match="nu"):
        ElasticEigenSolver(mesh, nu=0.5)
    for method in ("lattice", "ell"):
        with pytest.raises(ValueError, match="method"):
            ElasticEigenSolver(mesh, method=method)
    bare = FEMesh(nodes=mesh.nodes, elements=mesh.elements, dirichlet_nodes={})
    with pytest.raises(ValueError, match="shift"):
        ElasticEigenSolver(bare)
    with pytest.raises(ValueError, match="shift"):
        ElasticEigenSolver(mesh, fixed={})
    assert ElasticEigenSolver(bare, shift=1.0).shift == 1.0
    assert ElasticEigenSolver(bare, fixed={(0, 1): 3.0})._g.max() == 0.0          # a roller; the value is ignored
    some = FEMesh.rectangle(6, 5, bc_value=0.7)                                      # values of the mesh are ignored too
    assert int(ElasticEigenSolver(some)._is_bc.sum()) == 2 * len(some.dirichlet_nodes)
    for bad in (dict(k=0), dict(k=9, guard=8), dict(guard=-1), dict(tol=0.0), dict(shift=-1.0), dict(inner_tol=1.0),
                dict(reaction=1.0), dict(warm_start=True), dict(fixed={(0, 2): 0.0}), dict(fixed={(999, 0): 0.0}),
                dict(fixed=[(0, 0)])):
        with pytest.raises(ValueError):
            ElasticEigenSolver(mesh, **bad)
    for E, rho in ((torch.ones(2, m, 3, dtype=T64), 1.0), (1.0, torch.ones(5, 7, dtype=T64)),
                   (torch.ones(3, dtype=T64), torch.ones(4, dtype=T64)), (torch.ones(3, m, dtype=T64), torch.ones(2, 1, dtype=T64))):
        with pytest.raises(ValueError):
            ElasticEigenSolver(mesh, E, rho)
    es = ElasticEigenSolver(mesh, torch.ones(3, dtype=T64), torch.ones(m, dtype=T64), k=2)
    with pytest.raises(ValueError):
        es(layout="elements")
    with pytest.raises(ValueError):
        es(batch=4)                     # E carries 3 samples
    with pytest.raises(ValueError):
        es(batch=0)
    p, q = torch.nn.Parameter(torch.ones(m, dtype=T64)), torch.nn.Parameter(torch.ones(2, m, dtype=T64))
    ps = list(ElasticEigenSolver(mesh, p, q).parameters())
    assert len(ps) == 2 and ps[0] is p and ps[1] is q
    moving = FEMesh(nodes=mesh.nodes.clone().requires_grad_(True), elements=mesh.elements,
                    dirichlet_nodes=mesh.dirichlet_nodes)
    with pytest.raises(NotImplementedError, match="node gradients"):
        ElasticEigenSolver(moving)()


def test_layout_resolution_for_E_and_rho_together():
    from diffhe.modal import _modal_layout
    from diffhe.solver import K_ELEM, K_SAMPLE, K_SAMPLE_ELEM, K_SCALAR
    m = 60
    one = torch.ones
    assert _modal_layout(one(()), one(()), m, None) == (K_SCALAR, K_SCALAR, 1, False)
    assert _modal_layout(one(()), one(m), m, 4) == (K_SCALAR, K_ELEM, 4, True)
    assert _modal_layout(one(m), one(m), m, None) == (K_ELEM, K_ELEM, 1, False)
    assert _modal_layout(one(m), one(m), m, m) == (K_SAMPLE, K_SAMPLE, m, True)     # batch=B forces the per-sample reading
    assert _modal_layout(one(5), one(m), m, None) == (K_SAMPLE, K_ELEM, 5, True)
    assert _modal_layout(one(m), one(5, 1), m, None) == (K_ELEM, K_SAMPLE, 5, True)
    assert _modal_layout(one(5, m), one(5), m, 5) == (K_SAMPLE_ELEM, K_SAMPLE, 5, True)
    assert _modal_layout(one(()), one(5, m), m, None) == (K_SCALAR, K_SAMPLE_ELEM, 5, True)
    assert _modal_layout(one(m, m), one(m), m, None) == (K_SAMPLE_ELEM, K_ELEM, m, True)     # each field on its own
    for E, rho, batch in ((one(5, 7), one(()), None), (one(()), one(2, 3, m), None), (one(5), one(4), None),
                          (one(5, m), one(4, m), None), (one(5), one(()), 4), (one(()), one(5, 1), 4), (one(5), one(5), 0)):
        with pytest.raises(ValueError):
            _modal_layout(E, rho, m, batch)


def test_custom_ops_are_registered_with_shape_inference():
    """diffhe::modal_solve / diffhe::modal_solve_backward have fake (meta) implementations: tracing needs no GPU."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from diffhe import ElasticEigenSolver
    from diffhe.solver import _SOLVERS
    mesh = FEMesh.rectangle(4, 3)
    n, m = mesh.n_nodes, mesh.n_elements
    es = ElasticEigenSolver(mesh, k=3)
    _SOLVERS[id(es)] = es
    with FakeTensorMode():
        E = torch.empty(5, m, dtype=T64, requires_grad=True)
        rho = torch.empty(m, dtype=T64, requires_grad=True)
        lam, phi, tok = torch.ops.diffhe.modal_solve(E, rho, None, id(es), -1, False, True)
        assert lam.shape == (5, 3) and phi.shape == (5, 3, n, 2) and tok.shape == () and lam.dtype == T64
        assert lam.requires_grad and not phi.requires_grad
        gE, gr = torch.autograd.grad(lam.sum(), (E, rho), retain_graph=True)
        assert gE.shape == (5, m) and gr.shape == (m,)
        assert torch.autograd.grad(lam.sum(), rho)[0].shape == (m,)             # a subset: rho alone
        lam, phi, _ = torch.ops.diffhe.modal_solve(E.detach(), rho.detach(), None, id(es), 5, True, False)
        assert lam.shape == (5, 3) and phi.shape == (3, n, 2, 5)
        one = torch.empty((), dtype=T64)
        lam, phi, tok = torch.ops.diffhe.modal_solve(one, one, None, id(es), -1, False, False)
        assert lam.shape == (3,) and phi.shape == (3, n, 2)
        gE, gr = torch.ops.diffhe.modal_solve_backward(lam, tok, True, False, one, one)
        assert gE.shape == () and gr.numel() == 0


def test_fifth_signature_table_matches_the_fifth_header():
    decls = _declarations(HEADER)
    assert sorted(decls) == sorted(_hip.MODAL_SIGNATURES) == NAMES
    assert len(_hip.SIGNATURES) == 64 and len(_hip.ELASTIC_SIGNATURES) == 3 and len(_hip.STRESS_SIGNATURES) == 3
    assert len(_hip.EIGENSTRAIN_SIGNATURES) == 6
    others = set(_hip.SIGNATURES) | set(_hip.ELASTIC_SIGNATURES) | set(_hip.STRESS_SIGNATURES) | set(_hip.EIGENSTRAIN_SIGNATURES)
    assert not set(decls) & others
    for name, (ret, params) in decls.items():
        res, argtypes = _hip.MODAL_SIGNATURES[name]
        assert len(argtypes) == len(params), name
        for i, ((ctype, is_ptr), t) in enumerate(zip(params, argtypes)):
            if not is_ptr:
                assert t is BY_VALUE[ctype], (name, i, ctype, t)
            else:
                assert isinstance(t, type) and issubclass(t, _hip._Ptr) and t.elem == ctype, (name, i, ctype, t)
        assert ret == "int" and res is _hip._S, name
    if os.path.exists(_hip.LIB_PATH):
        L = _hip.lib()
        raw = ctypes.CDLL(_hip.LIB_PATH)
        for name in decls:
            fn = getattr(L, name)
            assert fn.restype is _hip._I and fn.errcheck is L.diffhe_to_node_major.errcheck, name
            assert hasattr(raw, name)
        with pytest.raises(_hip.HipExtensionError, match="diffhe_modal_mass"):      # refused on the host: no launch
            L.diffhe_modal_mass(None, None, None, 2, None, 0, 0, 4, 2, 1, 1, None, None)
        with pytest.raises(_hip.HipExtensionError, match="diffhe_modal_gram"):
            L.diffhe_modal_gram(None, None, None, 1, 0, 2, None, 4, 8, 4, None, None, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
def field_rows(t, m, B):
    """(B, m) rows of any scalar layout of E or rho."""
    t = t.detach().to("cpu", T64)
    if t.numel() == 1:
        return t.reshape(1, 1).expand(B, m)
    if t.dim() == 1 and t.shape[0] == m:
        return t.reshape(1, m).expand(B, m)
    if t.dim() == 1 or t.shape[1] == 1:
        return t.reshape(B, 1).expand(B, m)
    return t


def field_of(name, m, B, seed):
    if name == "scalar":
        return _rand((), seed, 0.5, 2.0)
    if name == "sample":
        return _rand((B,), seed, 0.5, 2.0)
    if name == "element":
        return _rand((m,), seed, 0.5, 2.0)
    return _rand((B, m), seed, 0.5, 2.0)


LAYOUTS = ["scalar", "sample", "element", "sample_element"]
KERNEL_MESHES = {"2d": lambda: _rect(7, 5, 31), "3d": lambda: _box(3, 3, 3, 32)}


def _plan_of(mesh):
    from diffhe.plan import get_plan, padded_batch
    from diffhe.solver import _Engine, _kappa_mode
    plan = get_plan(mesh, torch.device(DEV), prune=False)
    return plan, _Engine(plan, 0.0, 0, 0, "gather"), padded_batch, _kappa_mode


@gpu
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("which", list(KERNEL_MESHES))
def test_mass_kernel_against_the_dense_mass(which, name, B):
    mesh = KERNEL_MESHES[which]()
    n, m, d = mesh.n_nodes, mesh.n_elements, mesh.dim
    plan, eng, padded_batch, kappa_mode = _plan_of(mesh)
    rho = field_of(name, m, B, 40)
    mode, _ = kappa_mode(rho, m, B)
    Bp = padded_batch(B)
    rdev, rse, rsb, Bv = eng.kappa_device(rho, mode, B, Bp)
    assert Bv == (Bp if name in ("sample", "sample_element") else 1)
    L = _hip.lib()
    out = [torch.full((n, Bv), float("nan"), dtype=T64, device=DEV) for _ in range(2)]
    for mass in out:
        L.diffhe_modal_mass(*plan.shape_incidence(), plan.gradient_table()[1], d, rdev, rse, rsb, n, m,
                            B if Bv > 1 else 1, Bv, mass, None)
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1])
    got = out[0].cpu()
    want = dense_mass(mesh, field_rows(rho, m, B))
    real = B if Bv > 1 else 1
    assert rel_err(got[:, :real].t().numpy(), want[:real].numpy()) <= 1e-12
    if Bv > B:                                               # padding samples: rho = 1
        unit = dense_mass(mesh, torch.ones(1, m, dtype=T64))[0]
        assert rel_err(got[:, B:].t().numpy(), unit.expand(Bv - B, n).numpy()) <= 1e-12
    if name == "scalar" and which == "2d":                  # rho = 1: the plan's lumped mass
        one = torch.ones(1, dtype=T64, device=DEV)
        mass = torch.empty((n, 1), dtype=T64, device=DEV)
        L.diffhe_modal_mass(*plan.shape_incidence(), plan.gradient_table()[1], d, one, 0, 0, n, m, 1, 1, mass, None)
        assert rel_err(mass[:, 0].cpu().numpy(), plan.lumped_mass().cpu().numpy()) <= 1e-14


@gpu
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("which", list(KERNEL_MESHES))
def test_density_gradient_kernels_against_autograd(which, name, B):
    """dr = d / d rho of sum_{b,i} w[i, b] X_{i,b}^T M(rho_b) X_{i,b} for random columns X and weights w."""
    from diffhe.solver import _kappa_grad
    mesh = KERNEL_MESHES[which]()
    n, m, d, k = mesh.n_nodes, mesh.n_elements, mesh.dim, 3
    plan, eng, padded_batch, kappa_mode = _plan_of(mesh)
    rho = field_of(name, m, B, 41)
    mode, _ = kappa_mode(rho, m, B)
    Bp = padded_batch(B)
    X = _rand((k, n * d, Bp), 42, -1.0, 1.0)
    w = _rand((k, Bp), 43, -1.0, 1.0)
    rho_r = rho.clone().requires_grad_(True)
    md = dense_mass(mesh, _rows_grad(rho_r, m, B)).repeat_interleave(d, dim=1)   # (B, n d)
    (torch.einsum("kb,krb,br->", w[:, :B], X[:, :, :B] ** 2, md)).backward()
    L = _hip.lib()
    Xd, wd = X.to(DEV), w.to(DEV)
    args = (plan.elems, plan.gradient_table()[1], d, Xd, wd, k, n, m, B, Bp)
    got = []
    for _ in range(2):
        sums, elem = eng.element_grad(
            mode, False, B, Bp, None,
            lambda dr_e, osc, ose, part, total: L.diffhe_modal_grad_rho(*args, dr_e, part, total, None),
            lambda dr, osc, ose: L.diffhe_modal_grad_rho_shared(*args, dr, None))
        got.append(_kappa_grad(mode, rho.shape, sums, elem).cpu())
    assert torch.equal(got[0], got[1])
    assert got[0].shape == rho.shape
    tol = 1e-12 if name == "sample_element" else 1e-11       # no sum | sums of up to B m terms of mixed sign
    assert rel_err(got[0].numpy(), rho_r.grad.numpy()) <= tol


def _rows_grad(t, m, B):
    """`field_rows` that keeps the autograd graph."""
    if t.numel() == 1:
        return t.reshape(1, 1).expand(B, m)
    if t.dim() == 1 and t.shape[0] == m:
        return t.reshape(1, m).expand(B, m)
    if t.dim() == 1 or t.shape[1] == 1:
        return t.reshape(B, 1).expand(B, m)
    return t


def _unpack(G, p):
    """(p (p + 1) / 2, Bp) rows of the upper triangle -> (Bp, p, p) symmetric."""
    iu = torch.triu_indices(p, p)
    out = torch.zeros(G.shape[1], p, p, dtype=T64)
    out[:, iu[0], iu[1]] = G.t()
    out[:, iu[1], iu[0]] = G.t()
    return out


def _block_case(p, d, Bp, nodes=41, shared=False):
    gen = torch.Generator().manual_seed(1000 * p + 10 * d + Bp)
    rows = nodes * d
    Y = torch.randn(p, rows, Bp, generator=gen, dtype=T64)
    AY = torch.randn(p, rows, Bp, generator=gen, dtype=T64)
    mass = 0.5 + torch.rand(nodes, 1 if shared else Bp, generator=gen, dtype=T64)
    is_bc = (torch.rand(rows, generator=gen) < 0.15).to(torch.uint8)
    C = torch.randn(p, p, Bp, generator=gen, dtype=T64)
    theta = 0.5 + torch.rand(p, Bp, generator=gen, dtype=T64)
    return Y, AY, mass, is_bc, C, theta


def _run_block_entries(Y, AY, mass, is_bc, C, theta, d, modal=True):
    """The four passes on the device -> dict of CPU results."""
    L = _hip.lib()
    p, rows, Bp = Y.shape
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    Y, AY, mass, is_bc, C, theta = (dev(t) for t in (Y, AY, mass, is_bc, C, theta))
    new = lambda *s: torch.full(s, float("nan"), dtype=T64, device=DEV)  # noqa: E731
    nq, nblk = p * (p + 1) // 2, L.diffhe_eig_gram_blocks(rows, Bp)
    part = new(nblk * 2 * nq * Bp)
    GA, GM, X, AX, MX, R, rho, sgn = new(nq, Bp), new(nq, Bp), new(p, rows, Bp), new(p, rows, Bp), new(p, rows, Bp), \
        new(p, rows, Bp), new(p, Bp), new(p, Bp)
    if modal:
        margs = (mass, mass.shape[1], 1 if mass.shape[1] > 1 else 0, d)
        L.diffhe_modal_gram(Y, AY, *margs, is_bc, p, rows, Bp, part, GA, GM, None)
        L.diffhe_modal_rotate(Y, AY, C, theta, *margs, p, rows, Bp, X, AX, MX, R, None)
        L.diffhe_modal_residual(R, theta, *margs, p, rows, Bp, part, rho, None)
        flipped = X.clone()
        L.diffhe_modal_fix_sign(flipped, *margs, p, rows, Bp, part, sgn, None)
    else:
        mvec = mass.reshape(-1)
        L.diffhe_eig_gram(Y, AY, mvec, is_bc, p, rows, Bp, part, GA, GM, None)
        L.diffhe_eig_rotate(Y, AY, C, theta, mvec, p, rows, Bp, X, AX, MX, R, None)
        L.diffhe_eig_residual(R, theta, mvec, p, rows, Bp, part, rho, None)
        flipped = X.clone()
        L.diffhe_eig_fix_sign(flipped, mvec, p, rows, Bp, part, sgn, None)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dict(GA=GA, GM=GM, X=X, AX=AX, MX=MX, R=R, rho=rho, sgn=sgn, flipped=flipped).items()}


@gpu
@pytest.mark.parametrize("Bp", [4, 64, 128])
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("p", [5, 16])
def test_block_entries_with_a_per_sample_mass_against_einsum(p, d, Bp):
    """Lanes < 64 (Bp = 4), both rotation pass counts (p = 5: one, p = 16: two) and the row / d indexing."""
    Y, AY, mass, is_bc, C, theta = _block_case(p, d, Bp)
    got = _run_block_entries(Y, AY, mass, is_bc, C, theta, d)
    again = _run_block_entries(Y, AY, mass, is_bc, C, theta, d)
    for key in got:
        assert torch.equal(got[key], again[key]), key
    md = mass.repeat_interleave(d, dim=0)                                    # (rows, Bp)
    free = (1 - is_bc.to(T64))[:, None]
    GA = torch.einsum("irb,jrb->bij", Y * free, AY)
    GM = torch.einsum("irb,jrb->bij", Y * free * md, Y)
    iu = torch.triu_indices(p, p)
    assert rel_err(got["GA"].t().numpy(), GA[:, iu[0], iu[1]].numpy()) <= 1e-12
    assert rel_err(_unpack(got["GM"], p).numpy(), GM.numpy()) <= 1e-12
    X, AX = torch.einsum("jrb,jcb->crb", Y, C), torch.einsum("jrb,jcb->crb", AY, C)
    R = theta[:, None, :] * md * X - AX
    for key, want in (("X", X), ("AX", AX), ("MX", md * X), ("R", R)):
        assert rel_err(got[key].numpy(), want.numpy()) <= 1e-12, key
    rho = torch.sqrt((got["R"] ** 2 / md).sum(1)) / theta.abs()
    assert rel_err(got["rho"].numpy(), rho.numpy()) <= 1e-12
    s = (md * got["X"]).sum(1)
    assert float(s.abs().min()) >= 1e-6                                      # random columns: the sum decides every sign
    assert torch.equal(got["sgn"], torch.sign(s))
    assert torch.equal(got["flipped"], got["X"] * torch.sign(s)[:, None, :])


@gpu
@pytest.mark.parametrize("Bp", [4, 64])
def test_unit_density_and_one_component_reproduce_the_shared_mass_entries_bit_for_bit(Bp):
    """rho = 1, d = 1, the mass equal to plan.lumped_mass() for every sample: the accessor's two instantiations run the same
    arithmetic in the same order, so every output of the four passes is bitwise that of the diffhe_eig_* entries."""
    mesh = _rect(7, 5, 31)
    plan, _, _, _ = _plan_of(mesh)
    lumped = plan.lumped_mass().cpu()
    p, n = 8, mesh.n_nodes
    Y, AY, _, is_bc, C, theta = _block_case(p, 1, Bp, nodes=n)
    old = _run_block_entries(Y, AY, lumped[:, None], is_bc, C, theta, 1, modal=False)
    for mass in (lumped[:, None].expand(n, Bp), lumped[:, None]):            # per sample | shared, strides (1, 0)
        new = _run_block_entries(Y, AY, mass, is_bc, C, theta, 1)
        for key in old:
            assert torch.equal(old[key], new[key]), key


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the solver
# ---------------------------------------------------------------------------------------------------------------------
def solve(mesh, E, rho, k=6, **kw):
    from diffhe import ElasticEigenSolver
    call = {name: kw.pop(name) for name in ("batch", "x0", "layout") if name in kw}
    dev = lambda t: t.to(DEV) if isinstance(t, torch.Tensor) else t  # noqa: E731
    es = ElasticEigenSolver(mesh, dev(E), dev(rho), k, nu=NU, device=DEV, **kw)
    lam, phi = es(**call)
    return es, lam, phi


def as_rows(lam, phi, layout, batched=True):
    """lam (B, k), phi (B, k, n d) on the CPU from either layout."""
    lam, phi = lam.detach().cpu(), phi.detach().cpu()
    if layout == "node":
        phi = phi.permute(3, 0, 1, 2)
    elif not batched:
        phi = phi[None]
    return lam.reshape(phi.shape[0], -1), phi.reshape(phi.shape[0], phi.shape[1], -1)


def check_against_dense(mesh, plane, fixed, E, rho, lam, phi, tol, shift=0.0, n_rigid=0, vectors=True):
    """Eigenvalues to RTOL_U (rigid-body ones: RTOL_U x the first elastic), isolated eigenvectors sign-aligned to
    10 tol (lambda + shift) / gap, the rigid-body cluster through its M-orthogonal projector; M-orthonormality, zero
    fixed dofs, ascending order, the sign rule.  Returns the smallest relative gap it relied on."""
    B, k = lam.shape
    m = mesh.n_elements
    Er, rr = field_rows(E, m, B), field_rows(rho, m, B)
    bc = fixed_dofs(mesh, fixed)
    smallest = np.inf
    for b in range(B):
        ref_lam, ref_phi, md = dense_modes(mesh, Er[b], rr[b], plane, fixed)
        ref = ref_lam.numpy()
        first = ref[n_rigid]
        if n_rigid:
            assert float(lam[b, :n_rigid].abs().max()) <= RTOL_U * first
        err = float(((lam[b, n_rigid:] - ref_lam[n_rigid:k]).abs() / ref_lam[n_rigid:k]).max())
        print(f"sample {b}: eigenvalue error {err:.2e}")
        assert err <= RTOL_U
        assert bool((lam[b][1:] >= lam[b][:-1]).all())
        G = (phi[b] * md) @ phi[b].t()
        assert float((G - torch.eye(k, dtype=T64)).abs().max()) <= 1e-12
        if len(bc):
            assert float(phi[b][:, bc].abs().max()) == 0.0
        s = (phi[b] * md).sum(1)
        top = phi[b].max(1).values >= (1 - 1e-9) * phi[b].abs().max(1).values
        assert bool(torch.where(s.abs() >= 1e-8, s > 0, top).all())
        # the gaps of the elastic modes checked, relative to lambda; the rigid cluster's gap relative to lambda + shift
        rg = rel_gaps(ref, range(n_rigid, k))
        smallest = min(smallest, float(rg.min()))
        assert rg.min() >= 1e-2
        if not vectors:
            continue
        for j, i in enumerate(range(n_rigid, k)):
            r = ref_phi[i] * torch.sign((ref_phi[i] * md * phi[b, i]).sum())
            bound = 10 * tol * (ref[i] + shift) / (rg[j] * ref[i])
            e = float((phi[b, i] - r).abs().max() / r.abs().max())
            print(f"sample {b} mode {i}: eigenvector error {e:.2e} (bound {bound:.2e})")
            assert e <= bound
        if n_rigid:
            P = phi[b, :n_rigid].t() @ (phi[b, :n_rigid] * md)
            Pr = ref_phi[:n_rigid].t() @ (ref_phi[:n_rigid] * md)
            bound = 10 * tol * shift / first                 # lambda + shift = shift on the cluster, its gap `first`
            e = float((P - Pr).abs().max() / Pr.abs().max())
            print(f"sample {b}: rigid-body projector error {e:.2e} (bound {bound:.2e})")
            assert e <= bound
    return smallest


PAIRINGS = [(e, r) for e in LAYOUTS for r in LAYOUTS]


@gpu
@pytest.mark.parametrize("e_name,r_name", PAIRINGS)
def test_clamped_rectangle_every_layout_pairing(e_name, r_name):
    """Every (E layout, rho layout) pairing once; the plane and the output layout alternate over the pairings so that both
    planes and both layouts meet per-sample and shared fields of both kinds."""
    i = PAIRINGS.index((e_name, r_name))
    plane, layout = ("stress", "strain")[(i + i // 4) % 2], ("sample", "node")[(i // 2) % 2]
    mesh, fixed = rect2d()
    m, n, B, k = mesh.n_elements, mesh.n_nodes, 3, 6
    E, rho = field_of(e_name, m, B, 50), field_of(r_name, m, B, 51)
    batched = "sample" in e_name or "sample" in r_name
    es, lam, phi = solve(mesh, E, rho, k, plane=plane, fixed=fixed, layout=layout)
    Bo = B if batched else 1
    assert es.last_info.not_converged == 0 and es.last_info.gram_failures == 0
    assert tuple(lam.shape) == ((Bo, k) if batched else (k,))
    assert tuple(phi.shape) == ((k, n, 2, Bo) if layout == "node" else ((Bo, k, n, 2) if batched else (k, n, 2)))
    assert not phi.requires_grad and not lam.requires_grad
    check_against_dense(mesh, plane, fixed, E, rho, *as_rows(lam, phi, layout, batched), es.tol)


@gpu
@pytest.mark.parametrize("plane,e_name,r_name", [("stress", "sample_element", "sample_element"),
                                                 ("strain", "sample_element", "sample_element"),
                                                 ("stress", "element", "sample_element"),
                                                 ("strain", "sample_element", "element")])
def test_free_rectangle_finds_three_rigid_body_modes(plane, e_name, r_name):
    """The shift reaches the operator in each of its forms: E and rho per sample; a shared E expanded to the batch width of
    a per-sample rho; a shared rho whose (n d, 1) shift is broadcast onto per-sample values."""
    mesh, _ = rect2d()
    m, B, k = mesh.n_elements, 3, 8
    # seed 73 for the shared rho: with 53 the dense spectrum of one sample has a relative gap of 1.04e-2, too near the floor
    E, rho = field_of(e_name, m, B, 52), field_of(r_name, m, B, 73 if r_name == "element" else 53)
    shift = float(dense_modes(mesh, field_rows(E, m, B)[0], field_rows(rho, m, B)[0], plane, {})[0][3])   # ~ first elastic
    es, lam, phi = solve(mesh, E, rho, k, plane=plane, fixed={}, shift=shift)
    assert es.last_info.not_converged == 0 and tuple(lam.shape) == (B, k)
    check_against_dense(mesh, plane, {}, E, rho, *as_rows(lam, phi, "sample"), es.tol, shift=shift, n_rigid=3)


@gpu
@pytest.mark.parametrize("free", [False, True], ids=["clamped", "free"])
def test_box(free):
    mesh, fixed = box3d()
    m, B = mesh.n_elements, 2
    E, rho = _rand((B, m), 54, 0.5, 2.0), _rand((B, m), 55, 0.5, 2.0)
    if free:
        shift = float(dense_modes(mesh, E[0], rho[0], None, {})[0][6])
        es, lam, phi = solve(mesh, E, rho, 10, guard=4, fixed={}, shift=shift)
        assert es.last_info.not_converged == 0
        check_against_dense(mesh, None, {}, E, rho, *as_rows(lam, phi, "sample"), es.tol, shift=shift, n_rigid=6)
    else:
        es, lam, phi = solve(mesh, E, rho, 6, fixed=fixed)
        assert es.last_info.not_converged == 0 and tuple(phi.shape) == (B, 6, mesh.n_nodes, 3)
        check_against_dense(mesh, None, fixed, E, rho, *as_rows(lam, phi, "sample"), es.tol)


@gpu
@pytest.mark.parametrize("method", ["auto", "ell-jacobi"])
def test_multilevel_hierarchy_and_jacobi_pcg(method):
    """The 850-dof `multilevel_case` mesh of tests/test_elasticity.py: the aggregation hierarchy has >= 2 levels."""
    nx, ny, B = 24, 16, 2
    mesh = _rect(nx, ny, 13)
    fixed = {(i, a): 0.0 for i in _left_nodes(nx, ny) for a in range(2)}
    m = mesh.n_elements
    assert 2 * mesh.n_nodes == 850
    E, rho = _rand((B, m), 56, 0.5, 2.0), _rand((B, m), 57, 0.5, 2.0)
    es, lam, phi = solve(mesh, E, rho, 6, fixed=fixed, method=method)
    info = es.last_info
    print(f"{method}: path {info.path}, levels {info.inner.hierarchy_levels}, outer {info.outer_iterations}, inner "
          f"{info.inner_iterations}")
    if method == "auto":
        assert info.path == "ell-amgpcg" and info.inner.hierarchy_levels >= 2
    else:
        assert info.path == "ell-pcg" and info.inner.hierarchy_levels == 0
    assert info.not_converged == 0
    check_against_dense(mesh, "stress", fixed, E, rho, *as_rows(lam, phi, "sample"), es.tol)


# -- gradients --------------------------------------------------------------------------------------------------------
def dense_grads(mesh, plane, fixed, Er, rr, weights):
    """d / dE and d / d rho of sum_{b,i} weights[b, i] lambda_{b,i} through the dense restatement: (B, m) each, and the
    bound max_i 10 tol lambda_i / gap_i without the tol (per sample)."""
    gE, gr, amp = [], [], []
    k = weights.shape[1]
    for b in range(Er.shape[0]):
        Ec, rc = Er[b].clone().requires_grad_(True), rr[b].clone().requires_grad_(True)
        lam, _, _ = dense_modes(mesh, Ec, rc, plane, fixed)
        a, c = torch.autograd.grad((weights[b] * lam[:k]).sum(), (Ec, rc))
        gE.append(a)
        gr.append(c)
        rg = rel_gaps(lam.detach().numpy(), range(k))
        assert rg.min() >= 1e-2
        amp.append(float(np.max(10.0 / rg)))
    return torch.stack(gE), torch.stack(gr), amp


@gpu
@pytest.mark.parametrize("key", list(CASES))
def test_per_element_gradients_of_isolated_eigenvalues(key):
    tol = 1e-11
    make, plane = CASES[key]
    mesh, fixed = make()
    m, B, k = mesh.n_elements, 2, 3
    E0, r0 = _rand((B, m), 58, 0.5, 2.0), _rand((B, m), 59, 0.5, 2.0)
    E, rho = E0.to(DEV).requires_grad_(True), r0.to(DEV).requires_grad_(True)
    from diffhe import ElasticEigenSolver
    es = ElasticEigenSolver(mesh, E, rho, k, nu=NU, plane=plane, fixed=fixed, tol=tol, device=DEV)
    lam, _ = es()
    assert es.last_info.not_converged == 0
    w = torch.tensor([1.0, -0.5, 0.25], dtype=T64).expand(B, k)
    (lam * w.to(DEV)).sum().backward()
    gE, gr, amp = dense_grads(mesh, plane, fixed, E0, r0, w)
    for b in range(B):
        eE, er = rel_err(E.grad[b].cpu().numpy(), gE[b].numpy()), rel_err(rho.grad[b].cpu().numpy(), gr[b].numpy())
        print(f"{key} sample {b}: dE {eE:.2e}, drho {er:.2e} (bound {tol * amp[b]:.2e})")
        assert eE <= tol * amp[b] and er <= tol * amp[b]


@gpu
@pytest.mark.parametrize("free", [False, True], ids=["clamped", "free"])
def test_batch_of_one_with_per_sample_fields(free):
    """E and rho (1, m): what a training loop with batch size 1 passes.  Bp = 1, so the per-sample fields have width 1."""
    tol = 1e-11
    mesh, fixed = rect2d()
    fixed = {} if free else fixed
    m, k, nr = mesh.n_elements, (6 if free else 3), (3 if free else 0)
    E0, r0 = _rand((1, m), 71, 0.5, 2.0), _rand((1, m), 72, 0.5, 2.0)
    shift = float(dense_modes(mesh, E0[0], r0[0], "stress", {})[0][3]) if free else 0.0
    E, rho = E0.to(DEV).requires_grad_(True), r0.to(DEV).requires_grad_(True)
    es = modal.ElasticEigenSolver(mesh, E, rho, k, nu=NU, fixed=fixed, tol=tol, shift=shift, device=DEV)
    lam, phi = es()
    assert es.last_info.not_converged == 0
    assert tuple(lam.shape) == (1, k) and tuple(phi.shape) == (1, k, mesh.n_nodes, 2)
    check_against_dense(mesh, "stress", fixed, E0, r0, *as_rows(lam, phi, "sample"), 1e-8, shift=shift, n_rigid=nr)
    w = torch.zeros(1, k, dtype=T64)
    w[0, nr:nr + 3] = torch.tensor([1.0, -0.5, 0.25], dtype=T64)          # the elastic modes: isolated eigenvalues
    (lam * w.to(DEV)).sum().backward()
    assert E.grad.shape == (1, m) and rho.grad.shape == (1, m)
    Ec, rc = E0[0].clone().requires_grad_(True), r0[0].clone().requires_grad_(True)
    ref = dense_modes(mesh, Ec, rc, "stress", fixed)[0]
    gE, gr = torch.autograd.grad((w[0] * ref[:k]).sum(), (Ec, rc))
    rg = rel_gaps(ref.detach().numpy(), range(nr, nr + 3))
    assert rg.min() >= 1e-2
    bound = tol * float(np.max(10.0 * (ref.detach().numpy()[nr:nr + 3] + shift) / (rg * ref.detach().numpy()[nr:nr + 3])))
    eE, er = rel_err(E.grad[0].cpu().numpy(), gE.numpy()), rel_err(rho.grad[0].cpu().numpy(), gr.numpy())
    print(f"batch of one ({'free' if free else 'clamped'}): dE {eE:.2e}, drho {er:.2e} (bound {bound:.2e})")
    assert eE <= bound and er <= bound


@gpu
def test_a_shared_field_gets_the_sum_of_the_per_sample_gradients():
    tol = 1e-11
    mesh, fixed = rect2d()
    m, B, k = mesh.n_elements, 3, 3
    from diffhe import ElasticEigenSolver
    w = _rand((B, k), 60, 0.5, 1.5)
    for shared in ("E", "rho", "both"):
        E0 = _rand((m,) if shared in ("E", "both") else (B, m), 61, 0.5, 2.0)
        r0 = _rand((m,) if shared in ("rho", "both") else (B, m), 62, 0.5, 2.0)
        E, rho = E0.to(DEV).requires_grad_(True), r0.to(DEV).requires_grad_(True)
        es = ElasticEigenSolver(mesh, E, rho, k, nu=NU, fixed=fixed, tol=tol, device=DEV)
        lam, _ = es(batch=B)
        assert es.last_info.not_converged == 0 and tuple(lam.shape) == (B, k)
        (lam * w.to(DEV)).sum().backward()
        gE, gr, amp = dense_grads(mesh, "stress", fixed, field_rows(E0, m, B), field_rows(r0, m, B), w)
        bound = tol * max(amp)
        assert E.grad.shape == E0.shape and rho.grad.shape == r0.shape
        wantE = gE.sum(0) if E0.dim() == 1 else gE
        wantr = gr.sum(0) if r0.dim() == 1 else gr
        eE, er = rel_err(E.grad.cpu().numpy(), wantE.numpy()), rel_err(rho.grad.cpu().numpy(), wantr.numpy())
        print(f"shared {shared}: dE {eE:.2e}, drho {er:.2e} (bound {bound:.2e})")
        assert eE <= bound and er <= bound


@gpu
@pytest.mark.parametrize("key", ["2d-stress", "3d"])
def test_per_sample_scalars_are_homogeneous(key):
    """E_b d lambda / dE_b = lambda and rho_b d lambda / d rho_b = -lambda: second order in the eigenvector error."""
    make, plane = CASES[key]
    mesh, fixed = make()
    from diffhe import ElasticEigenSolver
    E = torch.tensor([0.7, 1.0, 2.2], dtype=T64, device=DEV, requires_grad=True)
    rho = torch.tensor([1.5, 0.6, 1.1], dtype=T64, device=DEV, requires_grad=True)
    lam, _ = ElasticEigenSolver(mesh, E, rho, 3, nu=NU, plane=plane, fixed=fixed, tol=1e-11, device=DEV)()
    for i in range(3):
        gE, gr = torch.autograd.grad(lam[:, i].sum(), (E, rho), retain_graph=True)
        want = lam[:, i].detach().cpu().numpy()
        assert rel_err((E.detach() * gE).cpu().numpy(), want) <= RTOL_GRAD
        assert rel_err((rho.detach() * gr).cpu().numpy(), -want) <= RTOL_GRAD
    one_E = torch.tensor(1.7, dtype=T64, device=DEV, requires_grad=True)               # one value for all: 0-dim gradients
    one_r = torch.tensor(0.8, dtype=T64, device=DEV, requires_grad=True)
    lam, _ = ElasticEigenSolver(mesh, one_E, one_r, 2, nu=NU, plane=plane, fixed=fixed, tol=1e-11, device=DEV)()
    lam[0].backward()
    assert one_E.grad.shape == () and one_r.grad.shape == ()
    assert abs(float(one_E.grad * one_E.detach() / lam[0].detach()) - 1.0) <= RTOL_GRAD
    assert abs(float(one_r.grad * one_r.detach() / lam[0].detach()) + 1.0) <= RTOL_GRAD


@gpu
def test_central_differences():
    """Directional derivatives of a weighted sum of isolated eigenvalues in (E, rho), step 1e-5, tolerance 1e-7."""
    from diffhe import ElasticEigenSolver
    mesh, fixed = rect2d()
    m, B = mesh.n_elements, 2
    E0, r0 = _rand((B, m), 63, 0.5, 2.0), _rand((B, m), 64, 0.5, 2.0)
    w = torch.tensor([[1.0, 0.5], [-0.3, 0.8]], dtype=T64, device=DEV)
    opts = dict(nu=NU, fixed=fixed, guard=3, tol=1e-11, device=DEV)

    def value(Ev, rv):
        lam, _ = ElasticEigenSolver(mesh, Ev.to(DEV), rv.to(DEV), 2, **opts)()
        return float((lam * w).sum())

    E, rho = E0.to(DEV).requires_grad_(True), r0.to(DEV).requires_grad_(True)
    lam, _ = ElasticEigenSolver(mesh, E, rho, 2, **opts)()
    (lam * w).sum().backward()
    gen = torch.Generator().manual_seed(65)
    for _ in range(2):
        vE, vr = (torch.randn(E0.shape, generator=gen, dtype=T64) for _ in range(2))
        fd = (value(E0 + 1e-5 * vE, r0 + 1e-5 * vr) - value(E0 - 1e-5 * vE, r0 - 1e-5 * vr)) / 2e-5
        an = float((E.grad.cpu() * vE).sum() + (rho.grad.cpu() * vr).sum())
        print("central difference", fd, "analytic", an)
        assert abs(fd - an) <= 1e-7 * max(abs(an), 1.0)


@gpu
def test_simp_chain_mixes_both_gradients():
    """sum_i lambda_i with E = rho^3 and mass ~ rho by autograd: the chain of examples/eigenfrequency_optimisation.py."""
    from diffhe import ElasticEigenSolver
    tol = 1e-11
    mesh, fixed = rect2d()
    m, B, k = mesh.n_elements, 2, 3
    x0 = _rand((B, m), 66, 0.5, 1.0)
    x = x0.to(DEV).requires_grad_(True)
    es = ElasticEigenSolver(mesh, x ** 3, x, k, nu=NU, fixed=fixed, tol=tol, device=DEV)
    lam, _ = es()
    assert es.last_info.not_converged == 0
    lam.sum().backward()
    amp, want = [], []
    for b in range(B):
        xc = x0[b].clone().requires_grad_(True)
        ref, _, _ = dense_modes(mesh, xc ** 3, xc, "stress", fixed)
        (g,) = torch.autograd.grad(ref[:k].sum(), xc)
        rg = rel_gaps(ref.detach().numpy(), range(k))
        assert rg.min() >= 1e-2
        amp.append(float(np.max(10.0 / rg)))
        want.append(g)
    for b in range(B):
        e = rel_err(x.grad[b].cpu().numpy(), want[b].numpy())
        print(f"SIMP chain sample {b}: {e:.2e} (bound {tol * amp[b]:.2e})")
        assert e <= tol * amp[b]


# -- remaining behaviour ----------------------------------------------------------------------------------------------
@gpu
def test_identical_calls_are_bitwise_equal_and_max_iter_one_warns():
    mesh, fixed = rect2d()
    m, B = mesh.n_elements, 3
    E, rho = _rand((B, m), 67, 0.5, 2.0), _rand((B, m), 68, 0.5, 2.0)
    _, lam0, phi0 = solve(mesh, E, rho, 4, fixed=fixed)
    _, lam1, phi1 = solve(mesh, E, rho, 4, fixed=fixed)
    assert torch.equal(lam0, lam1) and torch.equal(phi0, phi1)
    with pytest.warns(RuntimeWarning, match="did not reach"):
        es, _, _ = solve(mesh, E, rho, 4, fixed=fixed, max_iter=1)
    assert es.last_info.not_converged > 0 and es.last_info.outer_iterations == 1
    assert tuple(es.last_info.residual.shape) == (3, 4) and es.last_info.inner_solves == 8
    Eg, rg = E.to(DEV).requires_grad_(True), rho.to(DEV).requires_grad_(True)
    grads = []
    for _ in range(2):
        lam, _ = solve(mesh, Eg, rg, 4, fixed=fixed)[1:]
        grads.append(torch.autograd.grad(lam.sum(), (Eg, rg)))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


@gpu
def test_warm_start_needs_fewer_outer_iterations():
    mesh, fixed = rect2d()
    m, B = mesh.n_elements, 3
    E, rho = _rand((B, m), 69, 0.5, 2.0), _rand((B, m), 70, 0.5, 2.0)
    es, lam, phi = solve(mesh, E, rho, 4, fixed=fixed)
    moved = E * (1 + 0.01 * torch.sin(torch.arange(m, dtype=T64)))
    cold, _, _ = solve(mesh, moved, rho, 4, fixed=fixed)
    warm, lam_w, phi_w = solve(mesh, moved, rho, 4, fixed=fixed, x0=phi)
    print("outer iterations cold / warm:", cold.last_info.outer_iterations, warm.last_info.outer_iterations)
    assert warm.last_info.outer_iterations < cold.last_info.outer_iterations
    assert warm.last_info.not_converged == 0
    check_against_dense(mesh, "stress", fixed, moved, rho, *as_rows(lam_w, phi_w, "sample"), warm.tol)
    node, lam_n, phi_n = solve(mesh, moved, rho, 4, fixed=fixed, layout="node")
    again, lam_a, _ = solve(mesh, moved, rho, 4, fixed=fixed, layout="node", x0=phi_n)
    assert again.last_info.outer_iterations <= 2 and rel_err(lam_a.cpu().numpy(), lam_n.cpu().numpy()) <= RTOL_U
    with pytest.raises(ValueError, match="x0 must be"):
        solve(mesh, moved, rho, 4, fixed=fixed, x0=phi[:, :2])


@gpu
def test_second_order_backward_is_refused():
    from diffhe import ElasticEigenSolver
    mesh, fixed = rect2d()
    E = torch.full((mesh.n_elements,), 1.3, dtype=T64, device=DEV, requires_grad=True)
    lam, _ = ElasticEigenSolver(mesh, E, 1.0, 2, nu=NU, fixed=fixed, device=DEV)()
    (g,) = torch.autograd.grad(lam.sum(), E, retain_graph=True)
    assert g.shape == E.shape and bool(torch.isfinite(g).all())
    with pytest.raises(NotImplementedError, match="create_graph"):
        torch.autograd.grad(lam.sum(), E, create_graph=True)


@gpu
def test_example_raises_the_fundamental_frequency_at_fixed_volume():
    """examples/eigenfrequency_optimisation.py at 16 x 8 quads, 6 steps: f_1 of every design rises in every step."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eigenfrequency_optimisation",
                                                  os.path.join(root, "examples", "eigenfrequency_optimisation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rho, hist, _ = mod.optimise(ny=8, steps=6, device=DEV, verbose=False)
    f = torch.stack([h[0] for h in hist])                                   # (7, 3)
    print("f_1 per step:", f.t().tolist())
    assert tuple(rho.shape) == (3, 8, 16) and bool((f[1:] > f[:-1]).all())
    assert float((hist[-1][1] - torch.tensor([0.4, 0.5, 0.6], dtype=T64)).abs().max()) <= 1e-9
