"""Linear buckling of elastic bodies, (K(E) + lambda K_G(sigma0)) phi = 0 per sample, with d lambda / dE, d lambda / dload and
d lambda / d sigma0 (diffhe.buckling.LinearBucklingSolver, csrc/buckling.hip, include/diffhe_buckling.h).

The yardstick is a dense restatement written here, independent of the product code: K from the helpers of
tests/test_elasticity.py (K_e = vol_e E_e B^T D B), the prestress sigma0 = E D B u0 from a dense solve, K_G scattered from
vol_e G sigma G^T (x) I_d, mu from `torch.linalg.eigh` of -L^-1 K_G L^-T with L the Cholesky factor of K on the free dofs,
lambda = 1 / mu for the positive mu, gradients by torch autograd through all of it.  The CPU tests pin it (translations,
symmetry, the two homogeneities, the sign swap under a reversed load, no positive mu in biaxial tension) and check the
formula d lambda = lambda phi^T (dK + lambda dK_G) phi, the host logic and the fourteenth signature table; the GPU tests
hold the kernels and the solver against it.

Inputs: jittered meshes, nu = 0.3, E per element uniform in [0.5, 2], the left edge / face clamped, a total load of 1 spread
over the opposite edge / face.  2D: rectangle(12, 3) on [0, 2] x [0, 0.25] (96 free dofs); 3D: box(6, 2, 1) on
[0, 2] x [0, 0.4] x [0, 0.2] (108 free dofs).  Under transverse shear the negative mu are as large as the positive ones (3D:
[-476, 460]): the input of the shifted iteration.  k = 3, guard = 4.

Tolerances, with their reasons:
  * lambda: RTOL_U (1e-10) with tol = 1e-8 -- the K-norm residual bounds the error of mu by rho^2 mu / gap, far below it, so
    this is the operator tolerance;
  * modes, sign-aligned: max-norm error relative to |phi|_inf <= 10 tol mu_i / gap_i (Davis-Kahan in the K-inner product).
    Every test computes the gaps from its dense spectrum and asserts the smallest relative gap of the modes it checks
    >= 1e-2, so a changed input cannot make the bound vacuous;
  * gradients (per element dE through the prestress solve, dload, dsigma0) are first order in the mode error: tol = 1e-11
    and the same 10 tol mu_i / gap_i, plus the tolerance of the prestress solve; the homogeneity
    sum_e E_e d lambda_i / dE_e = lambda_i is second order: RTOL_GRAD;
  * central differences, step 1e-5, tolerance 1e-7: the reasoning in the header of tests/test_robin.py;
  * kernels alone: 1e-12 relative to the largest reference entry -- sums of a few hundred fp64 terms of order one; the
    batch-summed cotangent of a shared prestress sums up to B k terms of mixed sign per entry: 1e-11, as the totals of
    tests/test_modal.py.

`test_restatement_is_pinned` and `test_the_gradient_formula_equals_autograd` exercise the yardstick alone: they pin what the
other tests compare against and would pass without the product code, were it not for this module's import of
`diffhe.buckling`.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from diffhe import FEMesh, _hip
from diffhe import buckling
from _util import RTOL_GRAD, RTOL_U, rel_err
from test_elasticity import _dense_K, _geometry, _jitter, _rand, _strain_matrix, _voigt_D
from test_stress import BY_VALUE, _declarations

T64 = torch.float64
DEV = "cuda:0"
NU = 0.3
K_MODES, GUARD = 3, 4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffhe_buckling.h")
NAMES = ["diffhe_buckling_apply", "diffhe_buckling_grad_sigma", "diffhe_buckling_grad_sigma_shared", "diffhe_buckling_gram",
         "diffhe_buckling_rotate", "diffhe_buckling_step"]
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# the dense restatement
# ---------------------------------------------------------------------------------------------------------------------
def stress_tensor(sig, d):
    """(m, d, d) symmetric tensors from Voigt tensor components (m, nc)."""
    pairs = [(0, 0), (1, 1), (0, 1)] if d == 2 else [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
    S = torch.zeros(sig.shape[0], d, d, dtype=T64)
    for c, (s, t) in enumerate(pairs):
        S = S + sig[:, c, None, None] * (torch.eye(d, dtype=T64)[s][:, None] * torch.eye(d, dtype=T64)[t][None, :])
        if s != t:
            S = S + sig[:, c, None, None] * (torch.eye(d, dtype=T64)[t][:, None] * torch.eye(d, dtype=T64)[s][None, :])
    return S


def dense_G(mesh, sig):
    """(n, n) scalar operator G[a, b] = sum_e vol_e grad N_a . sigma_e grad N_b; differentiable in sig (m, nc)."""
    X, el = mesh.nodes.to(T64), mesh.elements.long()
    n, d = X.shape
    G, vol = _geometry(X, el)
    g = vol[:, None, None] * (G @ stress_tensor(sig, d) @ G.transpose(1, 2))                # (m, npe, npe)
    idx = (el[:, :, None] * n + el[:, None, :]).reshape(-1)
    return torch.zeros(n * n, dtype=T64).index_add(0, idx, g.reshape(-1)).reshape(n, n)


def dense_KG(mesh, sig):
    """(n d, n d) geometric stiffness G (x) I_d with dof = node d + component."""
    return torch.kron(dense_G(mesh, sig), torch.eye(mesh.dim, dtype=T64))


def fixed_dofs(mesh, fixed):
    return np.array(sorted(i * mesh.dim + a for i, a in fixed), dtype=np.int64)


def free_dofs(mesh, fixed):
    return torch.from_numpy(np.setdiff1d(np.arange(mesh.n_nodes * mesh.dim), fixed_dofs(mesh, fixed)))


def dense_prestress(mesh, E_m, load, plane, fixed):
    """sigma0 (m, nc) = E D B u0 of the dense solve K(E) u0 = load on the free dofs; differentiable in E_m and load."""
    X, el = mesh.nodes.to(T64), mesh.elements.long()
    n, d = X.shape
    free = free_dofs(mesh, fixed)
    K = _dense_K(mesh, E_m[None], NU, plane)[0]
    uf = torch.linalg.solve(K[free][:, free], load.reshape(-1)[free])
    u = torch.zeros(n * d, dtype=T64).index_add(0, free, uf)
    G, _ = _geometry(X, el)
    dofs = (el[:, :, None] * d + torch.arange(d)[None, None, :]).reshape(len(el), -1)
    eps = (_strain_matrix(G) @ u[dofs][:, :, None])[:, :, 0]
    return E_m[:, None] * (eps @ _voigt_D(NU, d, plane).t())


def dense_spectrum(mesh, E_m, sig, plane, fixed):
    """All pairs of N phi = mu K phi on the free dofs, N = -K_G(sig): mu (nf,) DESCENDING, phi (nf, n d) K-orthonormal and
    zero on the fixed dofs, K (n d, n d).  Differentiable in E_m (m,) and sig (m, nc)."""
    nd = mesh.n_nodes * mesh.dim
    free = free_dofs(mesh, fixed)
    K = _dense_K(mesh, E_m[None], NU, plane)[0]
    KG = dense_KG(mesh, sig)
    L = torch.linalg.cholesky(K[free][:, free])
    W = torch.linalg.solve_triangular(L, -KG[free][:, free], upper=False)
    A = torch.linalg.solve_triangular(L, W.t(), upper=False)
    mu, V = torch.linalg.eigh(0.5 * (A + A.t()))
    mu, V = mu.flip(0), V.flip(1)
    Phi = torch.linalg.solve_triangular(L.t(), V, upper=True)
    phi = torch.zeros(len(mu), nd, dtype=T64).index_add(1, free, Phi.t())
    return mu, phi, K


def dense_factors(mesh, E_m, load, plane, fixed, k=K_MODES):
    """lambda (k,) ascending of the load, through the dense prestress; differentiable in E_m and load."""
    mu, _, _ = dense_spectrum(mesh, E_m, dense_prestress(mesh, E_m, load, plane, fixed), plane, fixed)
    assert bool((mu[:k] > 0).all())
    return 1.0 / mu[:k], mu


def rel_gaps(mu_all, idx):
    """Distance of mu_all[i] to the nearest other eigenvalue over |mu_all[i]|, i in idx."""
    mu_all = np.asarray(mu_all)
    return np.array([np.min(np.abs(np.delete(mu_all, i) - mu_all[i])) / abs(mu_all[i]) for i in idx])


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def column2d():
    """The jittered rectangle(12, 3) on [0, 2] x [0, 0.25], its clamped left edge, the nodes of the right edge, E."""
    nx, ny = 12, 3
    mesh = _jitter(FEMesh.rectangle(nx, ny, x_range=(0.0, 2.0), y_range=(0.0, 0.25)), 31)
    left, right = [r * (nx + 1) for r in range(ny + 1)], [r * (nx + 1) + nx for r in range(ny + 1)]
    return mesh, {(i, a): 0.0 for i in left for a in range(2)}, right, _rand((mesh.n_elements,), 1, 0.5, 2.0)


def column3d():
    """The jittered box(6, 2, 1) on [0, 2] x [0, 0.4] x [0, 0.2], its clamped x = 0 face, the nodes of the x = 2 face, E."""
    kw = dict(x_range=(0.0, 2.0), y_range=(0.0, 0.4), z_range=(0.0, 0.2))
    X0 = FEMesh.box(6, 2, 1, **kw).nodes
    mesh = _jitter(FEMesh.box(6, 2, 1, **kw), 32)
    face0 = [i for i in range(mesh.n_nodes) if float(X0[i, 0]) == 0.0]
    face1 = [i for i in range(mesh.n_nodes) if abs(float(X0[i, 0]) - 2.0) < 1e-12]
    return mesh, {(i, a): 0.0 for i in face0 for a in range(3)}, face1, _rand((mesh.n_elements,), 2, 0.5, 2.0)


def end_load(mesh, nodes, component, total=-1.0):
    ld = torch.zeros(mesh.n_nodes, mesh.dim, dtype=T64)
    ld[nodes, component] = total / len(nodes)
    return ld


# key -> (mesh maker, plane, loaded component: 0 = axial compression, 1 = transverse shear)
CASES = {"2d-axial-stress": (column2d, "stress", 0), "2d-axial-strain": (column2d, "strain", 0),
         "2d-shear-stress": (column2d, "stress", 1), "2d-shear-strain": (column2d, "strain", 1),
         "3d-axial": (column3d, None, 0), "3d-shear": (column3d, None, 1)}


def case(key):
    make, plane, comp = CASES[key]
    mesh, fixed, end, E = make()
    return mesh, fixed, E, end_load(mesh, end, comp), plane


def biaxial_tension(nx=6, ny=4):
    """An unjittered rectangle on rollers (x fixed on the left edge, y on the bottom edge) under consistent nodal loads of
    unit tractions on the right and the top edge, uniform E: the P1 solution is exact, sigma0 = diag(1, 1) in every element,
    K_G is a positive definite Laplacian on the free dofs and no mu is positive."""
    mesh = FEMesh.rectangle(nx, ny, x_range=(0.0, 1.5), y_range=(0.0, 1.0))
    mesh = FEMesh(nodes=mesh.nodes.to(T64), elements=mesh.elements, dirichlet_nodes={})
    hx, hy = 1.5 / nx, 1.0 / ny
    fixed = {(r * (nx + 1), 0): 0.0 for r in range(ny + 1)}
    fixed.update({(c, 1): 0.0 for c in range(nx + 1)})
    ld = torch.zeros(mesh.n_nodes, 2, dtype=T64)
    for r in range(ny + 1):
        ld[r * (nx + 1) + nx, 0] += hy * (0.5 if r in (0, ny) else 1.0)
    for c in range(nx + 1):
        ld[ny * (nx + 1) + c, 1] += hx * (0.5 if c in (0, nx) else 1.0)
    return mesh, fixed, torch.full((mesh.n_elements,), 1.3, dtype=T64), ld


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement pinned
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["2d-axial-stress", "2d-shear-strain", "3d-shear"])
def test_restatement_is_pinned(key):
    mesh, fixed, E, load, plane = case(key)
    n, d = mesh.n_nodes, mesh.dim
    sig = dense_prestress(mesh, E, load, plane, fixed)
    KG = dense_KG(mesh, sig)
    scale = float(KG.abs().max())
    assert float((KG - KG.t()).abs().max()) <= 1e-14 * scale                           # symmetric
    for a in range(d):                                                                  # translations carry no K_G
        t = torch.eye(d, dtype=T64)[a].expand(n, d).reshape(-1)
        assert float((KG @ t).abs().max()) <= 1e-13 * scale
    mu, phi, K = dense_spectrum(mesh, E, sig, plane, fixed)
    k = K_MODES
    assert bool((mu[:k] > 0).all()) and rel_gaps(mu.numpy(), range(k)).min() >= 1e-2
    assert float((phi[:k] @ K @ phi[:k].t() - torch.eye(k, dtype=T64)).abs().max()) <= 1e-11
    lam = 1.0 / mu[:k]
    assert rel_err((torch.diagonal(phi[:k] @ KG @ phi[:k].t())).numpy(), (-1.0 / lam).numpy()) <= 1e-11
    lam_c, _ = dense_factors(mesh, E, 2.5 * load, plane, fixed)                         # lambda(c load) = lambda / c
    assert rel_err(lam_c.numpy(), (lam / 2.5).numpy()) <= 1e-10
    lam_e, _ = dense_factors(mesh, 3.0 * E, load, plane, fixed)                         # lambda(c E) = c lambda, load fixed
    assert rel_err(lam_e.numpy(), (3.0 * lam).numpy()) <= 1e-10
    mu_r, _, _ = dense_spectrum(mesh, E, dense_prestress(mesh, E, -load, plane, fixed), plane, fixed)
    assert rel_err(mu_r.numpy(), (-mu.flip(0)).numpy()) <= 1e-10                        # a reversed load swaps the signs


def test_restatement_has_no_positive_mu_in_biaxial_tension():
    mesh, fixed, E, load = biaxial_tension()
    sig = dense_prestress(mesh, E, load, "stress", fixed)
    want = torch.tensor([1.0, 1.0, 0.0], dtype=T64).expand(mesh.n_elements, 3)
    assert float((sig - want).abs().max()) <= 1e-12                                     # the patch test
    mu, _, _ = dense_spectrum(mesh, E, sig, "stress", fixed)
    assert float(mu.max()) < 0.0


@pytest.mark.parametrize("key", ["2d-axial-strain", "3d-shear"])
def test_the_gradient_formula_equals_autograd(key):
    """d lambda_i = lambda_i phi_i^T (dK + lambda_i dK_G) phi_i with (E, sigma0) as independent inputs: the partial
    derivatives the backward op returns."""
    mesh, fixed, E, load, plane = case(key)
    sig = dense_prestress(mesh, E, load, plane, fixed)
    Er, sr = E.clone().requires_grad_(True), sig.clone().requires_grad_(True)
    mu, phi, _ = dense_spectrum(mesh, Er, sr, plane, fixed)
    for i in range(K_MODES):
        gE, gs = torch.autograd.grad(1.0 / mu[i], (Er, sr), retain_graph=True)
        p, lam = phi[i].detach(), float(1.0 / mu[i].detach())
        Ec, sc = E.clone().requires_grad_(True), sig.clone().requires_grad_(True)
        form = lam * (p @ _dense_K(mesh, Ec[None], NU, plane)[0] @ p) + lam * lam * (p @ dense_KG(mesh, sc) @ p)
        fE, fs = torch.autograd.grad(form, (Ec, sc))
        assert rel_err(fE.numpy(), gE.numpy()) <= 1e-9 and rel_err(fs.numpy(), gs.numpy()) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# CPU: host logic
# ---------------------------------------------------------------------------------------------------------------------
def test_import_from_the_package_and_aggregate():
    import diffhe
    from diffhe import LinearBucklingSolver
    assert "LinearBucklingSolver" in diffhe.__all__
    assert LinearBucklingSolver is buckling.LinearBucklingSolver is diffhe.buckling.LinearBucklingSolver
    inf = float("inf")
    lam = torch.tensor([[2.0, 3.0, inf], [inf, inf, inf], [0.5, 4.0, 8.0]], dtype=T64, requires_grad=True)
    agg = buckling.aggregate(lam, p=6.0)
    want0 = (2.0 ** -6 + 3.0 ** -6) ** (-1.0 / 6.0)
    assert abs(float(agg[0]) - want0) <= 1e-14 and float(agg[1]) == inf
    assert 0.5 * 3 ** (-1.0 / 6.0) <= float(agg[2]) <= 0.5                               # a lower bound of the minimum
    torch.where(torch.isfinite(agg), agg, torch.zeros_like(agg)).sum().backward()
    assert bool(torch.isfinite(lam.grad).all()) and lam.grad[1].tolist() == [0.0, 0.0, 0.0] and float(lam.grad[0, 2]) == 0.0
    assert float(lam.grad[0, 0]) > float(lam.grad[0, 1]) > 0.0
    with pytest.raises(ValueError, match="p >= 1"):
        buckling.aggregate(lam, p=0.5)


def test_refusals_and_argument_validation():
    from diffhe import LinearBucklingSolver
    from diffhe.distributed import ShardedBatchSolve
    with pytest.raises(NotImplementedError, match="1D"):
        LinearBucklingSolver(FEMesh.line(10))
    with pytest.raises(NotImplementedError, match="P1"):
        LinearBucklingSolver(FEMesh.rectangle_p2(4, 4))
    with pytest.raises(ValueError, match="plane="):
        LinearBucklingSolver(FEMesh.box(2, 2, 2), plane="strain")
    mesh = FEMesh.rectangle(6, 5)
    n, m = mesh.n_nodes, mesh.n_elements
    with pytest.raises(NotImplementedError, match="stiffness tensor"):
        LinearBucklingSolver(mesh, torch.ones(2, m, 3, 3, dtype=T64))
    with pytest.raises(NotImplementedError, match="stiffness tensor"):
        LinearBucklingSolver(mesh, torch.eye(3, dtype=T64))
    with pytest.raises(NotImplementedError, match="strength"):
        LinearBucklingSolver(mesh, amg=dict(strength=0.25))
    for bad in (dict(k=0), dict(k=9, guard=8), dict(guard=-1), dict(tol=0.0), dict(inner_tol=1.0), dict(max_iter=-1),
                dict(method="lattice"), dict(nu=0.5), dict(plane="membrane"), dict(fixed={(0, 2): 0.0})):
        with pytest.raises(ValueError):
            LinearBucklingSolver(mesh, **bad)
    with pytest.raises(ValueError):
        LinearBucklingSolver(mesh, torch.ones(5, 7, dtype=T64))
    bs = LinearBucklingSolver(mesh, torch.ones(3, m, dtype=T64), k=2)
    load, sig = torch.zeros(n, 2, dtype=T64), torch.zeros(m, 3, dtype=T64)
    with pytest.raises(ValueError, match="not both"):
        bs(load=load, prestress=sig)
    with pytest.raises(ValueError, match="needs a load"):
        bs()
    with pytest.raises(ValueError, match="layout"):
        bs(load=load, layout="elements")
    with pytest.raises(ValueError, match="prestress shape"):
        bs(prestress=torch.zeros(m, 4, dtype=T64))
    with pytest.raises(ValueError, match="batch"):
        bs(prestress=torch.zeros(2, m, 3, dtype=T64))                                    # E carries 3 samples
    with pytest.raises(ValueError, match="batch"):
        bs(prestress=sig, batch=4)
    p = torch.nn.Parameter(torch.ones(m, dtype=T64))
    ps = list(LinearBucklingSolver(mesh, p).parameters())
    assert len(ps) == 1 and ps[0] is p
    moving = FEMesh(nodes=mesh.nodes.clone().requires_grad_(True), elements=mesh.elements,
                    dirichlet_nodes=mesh.dirichlet_nodes)
    with pytest.raises(NotImplementedError, match="node gradients"):
        LinearBucklingSolver(moving)(load=load)
    with pytest.raises(NotImplementedError, match="distributed"):
        ShardedBatchSolve(bs)
    with pytest.raises(NotImplementedError, match="distributed"):
        ShardedBatchSolve(bs.forward)


def test_layout_resolution_for_E_and_the_prestress():
    from diffhe.buckling import _buckling_layout
    from diffhe.solver import K_ELEM, K_SAMPLE, K_SAMPLE_ELEM, K_SCALAR
    m, nc = 60, 3
    one = torch.ones
    assert _buckling_layout(one(()), one(m, nc), m, nc, None) == (K_SCALAR, K_ELEM, 1, False)
    assert _buckling_layout(one(m), one(m, nc), m, nc, None) == (K_ELEM, K_ELEM, 1, False)
    assert _buckling_layout(one(m), one(m, nc), m, nc, 4) == (K_ELEM, K_ELEM, 4, True)
    assert _buckling_layout(one(5), one(m, nc), m, nc, None) == (K_SAMPLE, K_ELEM, 5, True)
    assert _buckling_layout(one(5, 1), one(5, m, nc), m, nc, None) == (K_SAMPLE, K_SAMPLE_ELEM, 5, True)
    assert _buckling_layout(one(5, m), one(m, nc), m, nc, 5) == (K_SAMPLE_ELEM, K_ELEM, 5, True)
    assert _buckling_layout(one(()), one(1, m, nc), m, nc, None) == (K_SCALAR, K_SAMPLE_ELEM, 1, True)
    assert _buckling_layout(one(m), one(m, m, nc), m, nc, None) == (K_SAMPLE, K_SAMPLE_ELEM, m, True)   # next to a batch of m
    for E, sig, batch in ((one(5), one(4, m, nc), None), (one(()), one(m, nc + 1), None), (one(()), one(nc, m), None),
                          (one(()), one(2, m, nc), 3), (one(5), one(m, nc), 4), (one(()), one(m, nc), 0),
                          (one(2, m, 3), one(m, nc), None)):
        with pytest.raises(ValueError):
            _buckling_layout(E, sig, m, nc, batch)


def test_custom_ops_are_registered_with_shape_inference():
    """diffhe::buckling_solve / diffhe::buckling_solve_backward have fake (meta) implementations: tracing needs no GPU."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from diffhe import LinearBucklingSolver
    from diffhe.solver import _SOLVERS
    mesh = FEMesh.rectangle(4, 3)
    n, m = mesh.n_nodes, mesh.n_elements
    bs = LinearBucklingSolver(mesh, k=3)
    _SOLVERS[id(bs)] = bs
    with FakeTensorMode():
        E = torch.empty(m, dtype=T64, requires_grad=True)
        sig = torch.empty(5, m, 3, dtype=T64, requires_grad=True)
        lam, phi, tok = torch.ops.diffhe.buckling_solve(E, sig, None, id(bs), -1, False, True)
        assert lam.shape == (5, 3) and phi.shape == (5, 3, n, 2) and tok.shape == () and lam.dtype == T64
        assert lam.requires_grad and not phi.requires_grad
        gE, gs = torch.autograd.grad(lam.sum(), (E, sig), retain_graph=True)
        assert gE.shape == (m,) and gs.shape == (5, m, 3)
        assert torch.autograd.grad(lam.sum(), sig)[0].shape == (5, m, 3)                 # a subset: the prestress alone
        lam, phi, _ = torch.ops.diffhe.buckling_solve(E.detach(), sig.detach(), None, id(bs), 5, True, False)
        assert lam.shape == (5, 3) and phi.shape == (3, n, 2, 5)
        one, shared = torch.empty((), dtype=T64), torch.empty(m, 3, dtype=T64)
        lam, phi, tok = torch.ops.diffhe.buckling_solve(one, shared, None, id(bs), -1, False, False)
        assert lam.shape == (3,) and phi.shape == (3, n, 2)
        gE, gs = torch.ops.diffhe.buckling_solve_backward(lam, tok, True, False, one, shared)
        assert gE.shape == () and gs.numel() == 0


def test_fourteenth_signature_table_matches_the_fourteenth_header():
    decls = _declarations(HEADER)
    assert sorted(decls) == sorted(_hip.BUCKLING_SIGNATURES) == NAMES
    others = set()
    for table in ("SIGNATURES", "ELASTIC_SIGNATURES", "STRESS_SIGNATURES", "EIGENSTRAIN_SIGNATURES", "MODAL_SIGNATURES",
                  "ELASTIC_SHAPE_SIGNATURES", "ELASTIC_ANISO_SIGNATURES", "ELASTIC_FACET_SIGNATURES", "FILTER_SIGNATURES",
                  "SAMPLE_SIGNATURES", "HYPERELASTIC_SIGNATURES", "HYPER_STRESS_SIGNATURES",
                  "ELASTIC_ANISO_STRESS_SIGNATURES"):
        others |= set(getattr(_hip, table))
    assert not set(decls) & others and len(_hip.SIGNATURES) == 64 and len(_hip.MODAL_SIGNATURES) == 7
    for name, (ret, params) in decls.items():
        res, argtypes = _hip.BUCKLING_SIGNATURES[name]
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
        with pytest.raises(_hip.HipExtensionError, match="diffhe_buckling_apply"):      # refused on the host: no launch
            L.diffhe_buckling_apply(None, None, None, None, None, 1.0, 4, 3, 2, 4, 4, None)
        with pytest.raises(_hip.HipExtensionError, match="diffhe_buckling_gram"):
            L.diffhe_buckling_gram(None, None, None, None, 4, 8, 4, None, None, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernels alone, through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
KERNEL_MESHES = {"2d": lambda: column2d()[0], "3d": lambda: column3d()[0]}
BATCHES = [3, 17]


def _plan_of(mesh):
    from diffhe.plan import get_plan, padded_batch
    from diffhe.solver import _Engine
    plan = get_plan(mesh, torch.device(DEV), prune=False)
    plan.ensure_ell()
    return plan, _Engine(plan, 0.0, 0, 0, "gather"), padded_batch


def _sigma_field(m, nc, B, shared, seed):
    """An indefinite prestress, (m, nc) shared or (B, m, nc), and its (B, m, nc) rows."""
    sig = _rand((m, nc) if shared else (B, m, nc), seed, -1.0, 1.0)
    return sig, (sig[None].expand(B, m, nc) if shared else sig)


def _assemble_G(plan, eng, sig, shared, B, Bp):
    from diffhe.solver import K_ELEM, K_SAMPLE_ELEM
    nc = sig.shape[-1]
    sdev, ssc, sse, ssb, Bg = eng.tensor_device(sig, K_ELEM if shared else K_SAMPLE_ELEM, B, Bp, nc)
    assert Bg == (1 if shared else Bp)
    gtab, vol = plan.gradient_table()
    G = torch.full((plan.W, plan.n, Bg), float("nan"), dtype=T64, device=DEV)
    _hip.lib().diffhe_aniso_assemble_rows(gtab, vol, plan.dim, sdev, ssc, sse, ssb if Bg > 1 else 0, plan.ent_ptr,
                                          plan.contrib, plan.cols, None, None, G, None, plan.n, plan.m, plan.W, Bg, None)
    return G, Bg


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["per-sample", "shared"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("which", list(KERNEL_MESHES))
def test_assembly_of_G_and_apply_against_the_dense_operator(which, B, shared):
    """G of an INDEFINITE stress through diffhe_aniso_assemble_rows without Dirichlet data, and y = scale (G (x) I_d) x."""
    mesh = KERNEL_MESHES[which]()
    n, m, d = mesh.n_nodes, mesh.n_elements, mesh.dim
    nc = d * (d + 1) // 2
    plan, eng, padded_batch = _plan_of(mesh)
    Bp = padded_batch(B)
    sig, rows = _sigma_field(m, nc, B, shared, 80)
    G0, Bg = _assemble_G(plan, eng, sig, shared, B, Bp)
    G1, _ = _assemble_G(plan, eng, sig, shared, B, Bp)
    assert torch.equal(G0, G1)
    cols = plan.cols.cpu().long()
    dense = torch.stack([dense_G(mesh, rows[b]) for b in range(1 if shared else B)])
    got = torch.zeros_like(dense)
    vals = G0.cpu()
    for k in range(plan.W):
        got[:, torch.arange(n), cols[k]] += vals[k, :, :dense.shape[0]].t()
    assert float(dense.min()) < 0.0 < float(dense.max())
    assert rel_err(got.numpy(), dense.numpy()) <= 1e-12
    # apply
    gen = torch.Generator().manual_seed(81)
    is_bc = (torch.rand(n * d, generator=gen) < 0.15).to(torch.uint8)
    x = torch.randn(n * d, Bp, generator=gen, dtype=T64) * (1 - is_bc.to(T64))[:, None]
    xd, bcd = x.to(DEV), is_bc.to(DEV)
    ys = [torch.full((n * d, Bp), float("nan"), dtype=T64, device=DEV) for _ in range(2)]
    for y in ys:
        _hip.lib().diffhe_buckling_apply(G0, plan.cols, bcd, xd, y, -1.0, n, plan.W, d, Bp, Bg, None)
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1])
    want = -torch.einsum("bij,jab->iab", dense.expand(B, n, n), x.reshape(n, d, Bp)[:, :, :B]).reshape(n * d, B)
    want = want * (1 - is_bc.to(T64))[:, None]
    got_y = ys[0].cpu()
    assert rel_err(got_y[:, :B].numpy(), want.numpy()) <= 1e-12
    assert float(got_y[is_bc.bool()].abs().max()) == 0.0


@gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("p", [7, 16])
def test_block_entries_against_einsum(p, d, B):
    """step, gram and rotate: lanes < 64 (Bp = 4 and 32), both rotation pass counts (p = 7: one, p = 16: two)."""
    from diffhe.plan import padded_batch
    L = _hip.lib()
    Bp, rows = padded_batch(B), 41 * d
    gen = torch.Generator().manual_seed(1000 * p + 10 * d + B)
    Y, KY, NY = (torch.randn(p, rows, Bp, generator=gen, dtype=T64) for _ in range(3))
    C = torch.randn(p, p, Bp, generator=gen, dtype=T64)
    mu = torch.randn(p, Bp, generator=gen, dtype=T64)
    is_bc = (torch.rand(rows, generator=gen) < 0.15).to(torch.uint8)
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    Yd, KYd, NYd, Cd, mud, bcd = (dev(t) for t in (Y, KY, NY, C, mu, is_bc))
    new = lambda *s: torch.full(s, float("nan"), dtype=T64, device=DEV)  # noqa: E731
    nq, nblk = p * (p + 1) // 2, L.diffhe_eig_gram_blocks(rows, Bp)

    def run():
        part = new(nblk * 2 * nq * Bp)
        GK, GN, X, KX, NX, R = new(nq, Bp), new(nq, Bp), new(p, rows, Bp), new(p, rows, Bp), new(p, rows, Bp), new(p, rows, Bp)
        L.diffhe_buckling_gram(Yd, KYd, NYd, bcd, p, rows, Bp, part, GK, GN, None)
        L.diffhe_buckling_rotate(Yd, KYd, NYd, Cd, mud, p, rows, Bp, X, KX, NX, R, None)
        y, dot, spart = new(rows, Bp), new(Bp), new(L.diffhe_grad_kappa_blocks(rows, Bp) * Bp)
        L.diffhe_buckling_step(Yd[0], KYd[0], NYd[0], mud[0], rows, Bp, y, spart, dot, None)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in dict(GK=GK, GN=GN, X=X, KX=KX, NX=NX, R=R, y=y, dot=dot).items()}

    got, again = run(), run()
    for key in got:
        assert torch.equal(got[key], again[key]), key
    free = (1 - is_bc.to(T64))[:, None]
    iu = torch.triu_indices(p, p)
    GK = torch.einsum("irb,jrb->bij", Y * free, KY)
    GN = torch.einsum("irb,jrb->bij", Y * free, NY)
    assert rel_err(got["GK"].t().numpy(), GK[:, iu[0], iu[1]].numpy()) <= 1e-12
    assert rel_err(got["GN"].t().numpy(), GN[:, iu[0], iu[1]].numpy()) <= 1e-12
    X, KX, NX = (torch.einsum("jrb,jcb->crb", t, C) for t in (Y, KY, NY))
    for key, want in (("X", X), ("KX", KX), ("NX", NX), ("R", NX - mu[:, None, :] * KX)):
        assert rel_err(got[key].numpy(), want.numpy()) <= 1e-12, key
    assert rel_err(got["y"].numpy(), (mu[0][None, :] * Y[0] + KY[0]).numpy()) <= 1e-12
    assert rel_err(got["dot"].numpy(), (KY[0] * NY[0]).sum(0).numpy()) <= 1e-12


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["per-sample", "shared"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("which", list(KERNEL_MESHES))
def test_prestress_cotangent_kernels_against_autograd(which, B, shared):
    """ds = d / d sigma0 of sum_{b,i} w[i, b] X_{i,b}^T K_G(sigma0_b) X_{i,b} for random columns X and weights w."""
    from diffhe.solver import K_ELEM, K_SAMPLE_ELEM
    mesh = KERNEL_MESHES[which]()
    n, m, d, k = mesh.n_nodes, mesh.n_elements, mesh.dim, 3
    nc = d * (d + 1) // 2
    plan, eng, padded_batch = _plan_of(mesh)
    Bp = padded_batch(B)
    sig, _ = _sigma_field(m, nc, B, shared, 82)
    X = _rand((k, n * d, Bp), 83, -1.0, 1.0)
    w = _rand((k, Bp), 84, -1.0, 1.0)
    sr = sig.clone().requires_grad_(True)
    total = 0.0
    for b in range(B):
        KG = dense_KG(mesh, sr if shared else sr[b])
        total = total + (w[:, b] * torch.einsum("kr,rs,ks->k", X[:, :, b], KG, X[:, :, b])).sum()
    total.backward()
    L = _hip.lib()
    gtab, vol = plan.gradient_table()
    args = (plan.elems, gtab, vol, d, X.to(DEV), w.to(DEV), k, n, m, B, Bp)
    got = []
    for _ in range(2):
        _, ds = eng.element_grad(
            K_ELEM if shared else K_SAMPLE_ELEM, False, B, Bp, nc,
            lambda ds_e, osc, ose, part, tot: L.diffhe_buckling_grad_sigma(*args, ds_e, osc, ose, part, tot, None),
            lambda ds, osc, ose: L.diffhe_buckling_grad_sigma_shared(*args, ds, osc, ose, None))
        got.append(ds.reshape(sig.shape).cpu())
    assert torch.equal(got[0], got[1])
    assert rel_err(got[0].numpy(), sr.grad.numpy()) <= (1e-11 if shared else 1e-12)
    if not shared:      # the per-sample totals, two stages: (nc, Bp) sums over the elements
        part = torch.empty(L.diffhe_grad_kappa_blocks(m, Bp), nc, Bp, dtype=T64, device=DEV)
        tot = torch.empty(nc, Bp, dtype=T64, device=DEV)
        L.diffhe_buckling_grad_sigma(*args, None, 0, 0, part, tot, None)
        assert rel_err(tot[:, :B].cpu().numpy(), sr.grad.sum(1).t().numpy()) <= 1e-11
        assert float(tot[:, B:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the solver
# ---------------------------------------------------------------------------------------------------------------------
def make_solver(mesh, E, plane, fixed, **kw):
    from diffhe import LinearBucklingSolver
    kw.setdefault("guard", GUARD)
    return LinearBucklingSolver(mesh, E.to(DEV) if isinstance(E, torch.Tensor) else E, kw.pop("k", K_MODES), nu=NU,
                                plane=plane, fixed=fixed, device=DEV, **kw)


def check_against_dense(mesh, plane, fixed, E_bm, load, lam, phi, tol):
    """lam (B, k), phi (B, k, n d) on the CPU against the dense model per sample: the k smallest positive lambda to RTOL_U,
    the modes sign-aligned to 10 tol mu_i / gap_i, K-orthonormality, phi^T K_G phi = -1 / lambda, zero fixed dofs, ascending
    order.  Returns the smallest relative gap it relied on and the number of negative mu of the dense spectra."""
    B, k = lam.shape
    bc = fixed_dofs(mesh, fixed)
    smallest, negative = np.inf, 0
    for b in range(B):
        sig = dense_prestress(mesh, E_bm[b], load, plane, fixed)
        mu, ref_phi, K = dense_spectrum(mesh, E_bm[b], sig, plane, fixed)
        assert bool((mu[:k] > 0).all())
        negative += int((mu < 0).sum())
        ref = 1.0 / mu[:k]
        err = float(((lam[b] - ref).abs() / ref).max())
        print(f"sample {b}: lambda {lam[b].tolist()} error {err:.2e}")
        assert err <= RTOL_U
        assert bool((lam[b][1:] >= lam[b][:-1]).all()) and bool((lam[b] > 0).all())
        ortho = float((phi[b] @ K @ phi[b].t() - torch.eye(k, dtype=T64)).abs().max())
        print(f"sample {b}: K-orthonormality {ortho:.2e}")
        assert ortho <= 1e-11
        kg = torch.diagonal(phi[b] @ dense_KG(mesh, sig) @ phi[b].t())
        assert rel_err(kg.numpy(), (-1.0 / ref).numpy()) <= RTOL_U
        assert float(phi[b][:, bc].abs().max()) == 0.0
        s = phi[b].sum(1)
        top = phi[b].max(1).values >= (1 - 1e-9) * phi[b].abs().max(1).values
        assert bool(torch.where(s.abs() >= 1e-8, s > 0, top).all())
        rg = rel_gaps(mu.numpy(), range(k))
        smallest = min(smallest, float(rg.min()))
        assert rg.min() >= 1e-2
        for i in range(k):
            r = ref_phi[i] * torch.sign(ref_phi[i] @ K @ phi[b, i])
            bound = 10 * tol / rg[i]
            e = float((phi[b, i] - r).abs().max() / r.abs().max())
            print(f"sample {b} mode {i}: mode error {e:.2e} (bound {bound:.2e})")
            assert e <= bound
    return smallest, negative


@gpu
@pytest.mark.parametrize("key", list(CASES))
def test_solver_against_the_dense_model(key):
    """The two 2D loads in both planes and the 3D column.  The shear loads are the input of the shifted iteration: the
    returned lambda are the dense model's smallest positive ones, `last_info` reports negative Ritz values, nothing is
    missing."""
    mesh, fixed, E, load, plane = case(key)
    bs = make_solver(mesh, E, plane, fixed)
    lam, phi = bs(load=load.to(DEV))
    info = bs.last_info
    print(key, "outer", info.outer_iterations, "inner solves", info.inner_solves, "inner iterations", info.inner_iterations,
          "shifts", info.shifts.tolist(), "negative Ritz", info.negative_ritz, "path", info.path,
          "rho", info.residual.tolist())
    assert lam.shape == (K_MODES,) and phi.shape == (K_MODES, mesh.n_nodes, mesh.dim)
    assert info.not_converged == 0 and info.missing == 0 and info.gram_failures == 0
    assert info.outer_iterations <= bs.max_iter and info.block == K_MODES + GUARD
    assert info.prestress is not None and info.prestress.not_converged == 0
    gap, negative = check_against_dense(mesh, plane, fixed, E[None], load, lam.cpu()[None],
                                        phi.cpu().reshape(1, K_MODES, -1), bs.tol)
    print(key, "smallest relative gap", gap)
    assert negative > 0
    if "shear" in key:
        assert info.negative_ritz > 0 and float(info.shifts.min()) > 0.0


@gpu
@pytest.mark.parametrize("layout", ["sample", "node"])
def test_a_field_per_sample(layout):
    """E (B, m) with B = 3 under one load: the prestress solve broadcasts the load, sigma0 comes per sample."""
    mesh, fixed, _, load, plane = case("2d-axial-stress")
    B = 3
    E = _rand((B, mesh.n_elements), 90, 0.5, 2.0)
    bs = make_solver(mesh, E, plane, fixed)
    lam, phi = bs(load=load.to(DEV), layout=layout)
    assert lam.shape == (B, K_MODES)
    assert phi.shape == ((K_MODES, mesh.n_nodes, 2, B) if layout == "node" else (B, K_MODES, mesh.n_nodes, 2))
    assert bs.last_info.not_converged == 0 and bs.last_info.missing == 0 and tuple(bs.last_info.shifts.shape) == (B,)
    rows = phi.cpu().permute(3, 0, 1, 2) if layout == "node" else phi.cpu()
    check_against_dense(mesh, plane, fixed, E, load, lam.cpu(), rows.reshape(B, K_MODES, -1), bs.tol)


@gpu
def test_a_given_prestress_reproduces_the_load_call_bitwise():
    mesh, fixed, E, load, plane = case("3d-shear")
    bs = make_solver(mesh, E, plane, fixed)
    lam, phi = bs(load=load.to(DEV))
    sigma = bs.inner.stress(bs.inner(load=load.to(DEV)))
    lam_s, phi_s = bs(prestress=sigma)
    assert bs.last_info.prestress is None
    assert torch.equal(lam, lam_s) and torch.equal(phi, phi_s)
    lam_b, phi_b = bs(prestress=sigma[None].expand(2, *sigma.shape).contiguous())      # the same stress per sample
    assert lam_b.shape == (2, K_MODES) and rel_err(lam_b.cpu().numpy(), lam.cpu().expand(2, K_MODES).numpy()) <= RTOL_U


@gpu
def test_biaxial_tension_gives_inf_one_warning_and_a_zero_gradient():
    mesh, fixed, E0, load = biaxial_tension()
    E = E0.to(DEV).requires_grad_(True)
    bs = make_solver(mesh, E, "stress", fixed)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        lam, phi = bs(load=load.to(DEV))
    assert [w.category for w in caught] == [RuntimeWarning] and "missing" in str(caught[0].message)
    assert bool(torch.isinf(lam).all()) and bool((lam > 0).all()) and float(phi.abs().max()) == 0.0
    assert bs.last_info.missing == K_MODES and bs.last_info.not_converged == 0
    assert bs.last_info.negative_ritz == K_MODES + GUARD
    lam.sum().backward()
    assert bool((E.grad == 0.0).all())
    assert float(buckling.aggregate(lam)) == float("inf")


def dense_total_grads(mesh, plane, fixed, E_m, load, weights):
    """d / dE and d / dload of sum_i weights[i] lambda_i through the dense prestress, and max_i 10 mu_i / gap_i."""
    Ec, lc = E_m.clone().requires_grad_(True), load.clone().requires_grad_(True)
    lam, mu = dense_factors(mesh, Ec, lc, plane, fixed, len(weights))
    gE, gl = torch.autograd.grad((weights * lam).sum(), (Ec, lc))
    rg = rel_gaps(mu.detach().numpy(), range(len(weights)))
    assert rg.min() >= 1e-2
    return gE, gl, float(np.max(10.0 / rg)), lam.detach()


@gpu
@pytest.mark.parametrize("key", ["2d-axial-stress", "2d-shear-strain", "3d-axial", "3d-shear"])
def test_total_gradients_to_E_and_the_load(key):
    """dL/dE per element THROUGH the prestress solve and dL/dload, one adjoint solve; homogeneity of degree one in E."""
    tol = 1e-11
    mesh, fixed, E0, load0, plane = case(key)
    E, load = E0.to(DEV).requires_grad_(True), load0.to(DEV).requires_grad_(True)
    bs = make_solver(mesh, E, plane, fixed, tol=tol)
    lam, _ = bs(load=load)
    assert bs.last_info.not_converged == 0 and bs.last_info.missing == 0
    w = torch.tensor([1.0, -0.5, 0.25], dtype=T64)
    (lam * w.to(DEV)).sum().backward()
    gE, gl, amp, ref = dense_total_grads(mesh, plane, fixed, E0, load0, w)
    bound = tol * amp + float(bs.inner.tol)
    eE, el = rel_err(E.grad.cpu().numpy(), gE.numpy()), rel_err(load.grad.cpu().numpy(), gl.numpy())
    print(f"{key}: dE {eE:.2e}, dload {el:.2e} (bound {bound:.2e}); rho {bs.last_info.residual.tolist()}")
    assert eE <= bound and el <= bound
    assert float(load.grad.cpu().reshape(-1)[fixed_dofs(mesh, fixed)].abs().max()) == 0.0
    for i in range(K_MODES):
        E.grad = None
        lam_i, _ = bs(load=load0.to(DEV))
        lam_i[i].backward()
        h = abs(float((E.grad * E.detach()).sum() / lam_i[i].detach()) - 1.0)
        print(f"{key} mode {i}: homogeneity {h:.2e}")
        assert h <= RTOL_GRAD


@gpu
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-sample"])
def test_gradient_to_a_given_prestress(shared):
    tol = 1e-11
    mesh, fixed, E0, load, plane = case("2d-shear-stress")
    B = 1 if shared else 2
    sig0 = torch.stack([dense_prestress(mesh, E0, c * load, plane, fixed) for c in (1.0, 1.3)[:B]])
    sig_in = sig0[0] if shared else sig0
    sig, E = sig_in.to(DEV).requires_grad_(True), E0.to(DEV).requires_grad_(True)
    bs = make_solver(mesh, E, plane, fixed, tol=tol)
    lam, _ = bs(prestress=sig)
    assert bs.last_info.not_converged == 0 and lam.shape == ((K_MODES,) if shared else (B, K_MODES))
    w = torch.tensor([1.0, -0.5, 0.25], dtype=T64)
    (lam * w.to(DEV)).sum().backward()
    gE = torch.zeros_like(E0)
    for b in range(B):
        Ec, sc = E0.clone().requires_grad_(True), sig0[b].clone().requires_grad_(True)
        mu, _, _ = dense_spectrum(mesh, Ec, sc, plane, fixed)
        a, c = torch.autograd.grad((w / mu[:K_MODES]).sum(), (Ec, sc))
        rg = rel_gaps(mu.detach().numpy(), range(K_MODES))
        assert rg.min() >= 1e-2
        bound = tol * float(np.max(10.0 / rg))
        got = sig.grad.cpu() if shared else sig.grad.cpu()[b]
        e = rel_err(got.numpy(), c.numpy())
        print(f"sample {b}: dsigma0 {e:.2e} (bound {bound:.2e})")
        assert e <= bound
        gE += a
    assert rel_err(E.grad.cpu().numpy(), gE.numpy()) <= bound                           # the partial derivative, sigma0 fixed


@gpu
def test_central_difference():
    """A directional derivative of a weighted sum of the factors in (E, load), step 1e-5, tolerance 1e-7."""
    mesh, fixed, E0, load0, plane = case("2d-axial-stress")
    w = torch.tensor([1.0, 0.5, -0.3], dtype=T64, device=DEV)

    def value(Ev, lv):
        lam, _ = make_solver(mesh, Ev, plane, fixed, tol=1e-11)(load=lv.to(DEV))
        return float((lam * w).sum())

    E, load = E0.to(DEV).requires_grad_(True), load0.to(DEV).requires_grad_(True)
    lam, _ = make_solver(mesh, E, plane, fixed, tol=1e-11)(load=load)
    (lam * w).sum().backward()
    gen = torch.Generator().manual_seed(91)
    vE = torch.randn(E0.shape, generator=gen, dtype=T64)
    vl = torch.randn(load0.shape, generator=gen, dtype=T64) * load0.abs().max()
    fd = (value(E0 + 1e-5 * vE, load0 + 1e-5 * vl) - value(E0 - 1e-5 * vE, load0 - 1e-5 * vl)) / 2e-5
    an = float((E.grad.cpu() * vE).sum() + (load.grad.cpu() * vl).sum())
    print("central difference", fd, "analytic", an)
    assert abs(fd - an) <= 1e-7 * max(abs(an), 1.0)


@gpu
def test_warm_start_identical_calls_and_second_order_refusal():
    mesh, fixed, E0, load, plane = case("3d-shear")
    ld = load.to(DEV)
    cold = make_solver(mesh, E0, plane, fixed)
    lam, phi = cold(load=ld)
    lam2, phi2 = make_solver(mesh, E0, plane, fixed)(load=ld)
    assert torch.equal(lam, lam2) and torch.equal(phi, phi2)                            # bitwise reproducible
    warm = make_solver(mesh, E0, plane, fixed)
    lam_w, phi_w = warm(load=ld, x0=phi)
    print("outer iterations cold / warm:", cold.last_info.outer_iterations, warm.last_info.outer_iterations)
    assert warm.last_info.outer_iterations <= cold.last_info.outer_iterations and warm.last_info.not_converged == 0
    assert rel_err(lam_w.cpu().numpy(), lam.cpu().numpy()) <= RTOL_U
    with pytest.raises(ValueError, match="x0 must be"):
        warm(load=ld, x0=phi[:2])
    with pytest.warns(RuntimeWarning, match="did not reach"):
        short = make_solver(mesh, E0, plane, fixed, max_iter=1)
        short(load=ld)
    assert short.last_info.not_converged > 0 and short.last_info.outer_iterations == 1
    E = E0.to(DEV).requires_grad_(True)
    lam_g, _ = make_solver(mesh, E, plane, fixed)(load=ld)
    (g,) = torch.autograd.grad(lam_g.sum(), E, retain_graph=True)
    assert g.shape == E.shape and bool(torch.isfinite(g).all())
    with pytest.raises(NotImplementedError, match="create_graph"):
        torch.autograd.grad(lam_g.sum(), E, create_graph=True)
