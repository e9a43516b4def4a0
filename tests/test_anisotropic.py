"""Solves with a conductivity tensor per element (diffhe.aniso.AnisotropicFESolver, csrc/aniso.hip): a dense torch
restatement pinned by central differences, the host logic (layouts, helpers, validation, refusals), and on the GPU the
kernels against that restatement for every layout, the scalar solver for isotropic tensors, a rotation identity and a
sparse-LU yardstick at a size with a real multigrid hierarchy, second-order convergence, determinism.  Every GPU solve
here must converge without a RuntimeWarning."""
import contextlib
import types
import warnings

import numpy as np
import pytest
import torch

from diffhe import AnisotropicFESolver, FEMesh, ShapeDifferentiableFESolver
from diffhe import aniso
from diffhe import solver as solver_mod
from diffhe.tet3d import DifferentiableFESolver3D
from _util import RTOL_GRAD, RTOL_U, rel_err

T64 = torch.float64
DEV = "cuda:0"
_VOIGT = {2: ((0, 0), (1, 1), (0, 1)), 3: ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))}


# ------------------------------------------------------------------------------------------------
# dense restatement (independent of the product code), differentiable in the Voigt components
# ------------------------------------------------------------------------------------------------
def _full(kv, d):
    """(..., nc) Voigt components -> (..., d, d): an off-diagonal component is ONE parameter for both entries."""
    rows = []
    for i in range(d):
        rows.append(torch.stack([kv[..., _VOIGT[d].index((min(i, j), max(i, j)))] for j in range(d)], -1))
    return torch.stack(rows, -2)


def _geometry(X, el):
    """grad phi (m, npe, d), element size (m), load matrix entries m0 (m, npe, npe) of P1 triangles / tetrahedra."""
    P = X[el]
    m, d = el.shape[0], X.shape[1]
    if d == 2:
        x, y = P[..., 0], P[..., 1]
        det = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
        b = torch.stack([y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]], 1)
        cc = torch.stack([x[:, 2] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 0]], 1)
        G = torch.stack([b, cc], 2) / det[:, None, None]
        size = 0.5 * det.abs()
        m0 = (size / 9.0)[:, None, None].expand(m, 3, 3)
    else:
        a, b, cv = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], P[:, 3] - P[:, 0]
        g1, g2, g3 = torch.cross(b, cv, dim=1), torch.cross(cv, a, dim=1), torch.cross(a, b, dim=1)
        det = (a * g1).sum(1)
        G = torch.stack([-(g1 + g2 + g3), g1, g2, g3], 1) / det[:, None, None]
        size = det.abs() / 6.0
        m0 = (size / 16.0)[:, None, None].expand(m, 4, 4)
    return G, size, m0


def _dense_solve(mesh, kv_bme, f_bn, load_bn=None, c=0.0):
    """u (B, n) of (K(kv_b) + c M_L) u = M f + load on the free rows, u = g on the Dirichlet nodes.  K is the index_add
    of |e| G K_e G^T with K_e from the Voigt components kv_bme (B, m, nc); load map F_p = |e| / (d+1) * mean f, lumped
    mass |e| / (d+1) per vertex and the Dirichlet elimination of `_dense_solve` in tests/test_shape_grad.py."""
    X = mesh.nodes.to(T64)
    n, d = X.shape
    el = mesh.elements.long()
    m, npe = el.shape
    G, size, m0 = _geometry(X, el)
    B = f_bn.shape[0]
    ke = size[None, :, None, None] * torch.einsum("epa,beac,eqc->bepq", G, _full(kv_bme, d), G)
    idx = (el[:, :, None] * n + el[:, None, :]).reshape(-1)
    K = torch.zeros(B, n * n, dtype=T64).index_add(1, idx, ke.reshape(B, -1)).reshape(B, n, n)
    M = torch.zeros(n * n, dtype=T64).index_add(0, idx, m0.reshape(-1)).reshape(n, n)
    ml = torch.zeros(n, dtype=T64).index_add(0, el.reshape(-1), (size / npe)[:, None].expand(m, npe).reshape(-1))
    bc = mesh.dirichlet_nodes
    bcn = np.array(sorted(bc), dtype=np.int64)
    free = np.setdiff1d(np.arange(n), bcn)
    g = torch.zeros(n, dtype=T64)
    if len(bcn):
        g[bcn] = torch.tensor([float(bc[int(k)]) for k in bcn], dtype=T64)
    A = K + c * torch.diag(ml)
    F = f_bn @ M.t() - A[:, :, bcn] @ g[bcn]
    if load_bn is not None:
        F = F + load_bn
    uf = torch.linalg.solve(A[:, free][:, :, free], F[:, free].unsqueeze(2)).squeeze(2)
    u = g.expand(B, n).clone()
    u[:, free] = uf
    return u


# ------------------------------------------------------------------------------------------------
# meshes and tensors
# ------------------------------------------------------------------------------------------------
def _jittered(mesh, amount, seed, keep_boundary=True):
    rng = np.random.default_rng(seed)
    X = mesh.nodes.numpy().copy()
    d = X.shape[1]
    h = np.array([np.ptp(X[:, k]) for k in range(d)]) / np.array(
        [max(len(np.unique(np.round(X[:, k], 12))) - 1, 1) for k in range(d)])
    move = rng.uniform(-amount, amount, X.shape) * h
    if keep_boundary:
        move[np.array(sorted(mesh.dirichlet_nodes), dtype=np.int64)] = 0.0
    return FEMesh(nodes=torch.from_numpy(X + move), elements=mesh.elements.clone(),
                  dirichlet_nodes=dict(mesh.dirichlet_nodes))


def _permuted(mesh, seed):
    """The same mesh with nodes and elements renumbered at random: no lattice numbering left."""
    rng = np.random.default_rng(seed)
    n = mesh.n_nodes
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    el = inv[mesh.elements.numpy()][rng.permutation(mesh.n_elements)]
    return FEMesh(nodes=mesh.nodes[perm].clone(), elements=torch.from_numpy(el),
                  dirichlet_nodes={int(inv[k]): v for k, v in mesh.dirichlet_nodes.items()})


def _with_bc_data(mesh, fn):
    X = mesh.nodes.numpy()
    return FEMesh(nodes=mesh.nodes, elements=mesh.elements,
                  dirichlet_nodes={k: float(fn(X[k])) for k in mesh.dirichlet_nodes})


def _partly_neumann(mesh, value=0.1):
    return FEMesh(nodes=mesh.nodes, elements=mesh.elements,
                  dirichlet_nodes={k: value for k in list(mesh.dirichlet_nodes)[::2]})


def _spd_voigt(shape, d, seed, lo=0.5, hi=4.0):
    """Random SPD tensors Q diag(lambda) Q^T in Voigt components, shape + (nc,): eigenvalues in [lo, hi], ratio <= 8."""
    gen = torch.Generator().manual_seed(seed)
    Q = torch.linalg.qr(torch.randn(*shape, d, d, generator=gen, dtype=T64)).Q
    lam = lo + (hi - lo) * torch.rand(*shape, d, generator=gen, dtype=T64)
    K = Q @ torch.diag_embed(lam) @ Q.transpose(-1, -2)
    return torch.stack([0.5 * (K[..., i, j] + K[..., j, i]) for i, j in _VOIGT[d]], -1)


def _small_meshes():
    rect = _with_bc_data(_jittered(FEMesh.rectangle(6, 5), 0.2, 2), lambda x: 0.3 + x[0] * x[1])
    box = _partly_neumann(_jittered(FEMesh.box(3, 3, 2), 0.15, 3, keep_boundary=False))
    return {"rect": rect, "rect_permuted": _permuted(rect, 5), "box": box}


@contextlib.contextmanager
def _strict():
    """Every solve in these tests converges: a RuntimeWarning (non-convergence, singular system) is an error."""
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        yield


def _converged(solver):
    assert solver.last_info.not_converged == 0, solver.last_info
    assert solver.last_info.path in ("ell-amgpcg", "ell-pcg")


# ------------------------------------------------------------------------------------------------
# host tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rect", "box"])
def test_dense_restatement_against_central_differences(name):
    """Pins the yardstick: autograd through the dense solve against central differences in EVERY tensor component."""
    if name == "rect":
        mesh = _with_bc_data(_jittered(FEMesh.rectangle(3, 3), 0.2, 2), lambda x: 0.3 + x[0] * x[1])
    else:
        mesh = _partly_neumann(_jittered(FEMesh.box(2, 2, 2), 0.15, 3, keep_boundary=False))
    d, n, m = mesh.dim, mesh.n_nodes, mesh.n_elements
    gen = torch.Generator().manual_seed(11)
    f = 1 + 0.5 * torch.randn(1, n, generator=gen, dtype=T64)
    load = 0.1 * torch.randn(1, n, generator=gen, dtype=T64)
    w = torch.rand(1, n, generator=gen, dtype=T64)
    kv = _spd_voigt((m,), d, 12).requires_grad_(True)

    def loss(k):
        return (w * _dense_solve(mesh, k[None], f, load, c=0.7) ** 2).sum()

    (grad,) = torch.autograd.grad(loss(kv), kv)
    # central differences with step h: truncation ~ h^2 |L'''| ~ 1e-12, rounding ~ eps |L| / h ~ 1e-10 of the loss;
    # 1e-7 of the largest gradient entry leaves room for both and is far below any wrong factor (a missing factor 2 on
    # an off-diagonal component is an error of order 1)
    h = 1e-6
    fd = torch.zeros_like(grad)
    with torch.no_grad():
        for e in range(m):
            for c in range(kv.shape[1]):
                kp, km = kv.detach().clone(), kv.detach().clone()
                kp[e, c] += h
                km[e, c] -= h
                fd[e, c] = (loss(kp) - loss(km)) / (2 * h)
    assert float(grad.abs().max()) > 0
    assert rel_err(grad.numpy(), fd.numpy()) < 1e-7


def test_layout_classification():
    K_SCALAR, K_SAMPLE, K_ELEM, K_SAMPLE_ELEM = (solver_mod.K_SCALAR, solver_mod.K_SAMPLE, solver_mod.K_ELEM,
                                                 solver_mod.K_SAMPLE_ELEM)
    mode = solver_mod._tensor_mode
    lay = solver_mod._kappa_layout
    for nc, m in ((3, 40), (6, 48)):
        assert mode(torch.ones(nc), nc, m, None) == (K_SCALAR, None, False)
        assert mode(torch.ones(nc), nc, m, 5) == (K_SCALAR, None, False)
        assert mode(torch.ones(5, nc), nc, m, 5) == (K_SAMPLE, 5, False)
        assert mode(torch.ones(5, nc), nc, m, None) == (K_SAMPLE, 5, False)              # B from the tensor
        assert mode(torch.ones(m, nc), nc, m, None) == (K_ELEM, None, False)
        assert mode(torch.ones(m, nc), nc, m, 5) == (K_ELEM, None, False)
        assert mode(torch.ones(m, nc), nc, m, m) == (K_SAMPLE, m, False)                 # as _kappa_mode: f's batch == m
        assert solver_mod._kappa_mode(torch.ones(m), m, m)[0] == K_SAMPLE               # ... the rule it mirrors
        assert mode(torch.ones(5, m, nc), nc, m, 5) == (K_SAMPLE_ELEM, 5, False)
        assert mode(torch.ones(nc, m, 5), nc, m, 5, True) == (K_SAMPLE_ELEM, 5, True)    # layout='node'
        assert mode(torch.ones(nc, m, nc), nc, m, nc, True) == (K_SAMPLE_ELEM, nc, True)  # reads both ways: node layout
        assert mode(torch.ones(nc, m, nc), nc, m, nc, False) == (K_SAMPLE_ELEM, nc, False)
        # through the call's layout function: the batch of f and of the tensor must agree
        assert lay(torch.ones(nc), m, None, False, nc) == (K_SCALAR, 1, False)
        assert lay(torch.ones(m, nc), m, 7, False, nc) == (K_ELEM, 7, False)
        assert lay(torch.ones(7, m, nc), m, 7, False, nc) == (K_SAMPLE_ELEM, 7, False)
        assert lay(torch.ones(nc, m, 7), m, 7, True, nc) == (K_SAMPLE_ELEM, 7, True)
        with pytest.raises(ValueError):
            lay(torch.ones(4, nc), m, 5, False, nc)
        for bad in (torch.ones(nc + 1), torch.ones(m), torch.ones(m, nc + 1), torch.ones(nc, m), torch.ones(5, m + 1, nc),
                    torch.ones(nc, m, 5), torch.ones(()), torch.ones(2, 5, m, nc)):
            with pytest.raises(ValueError):
                mode(bad, nc, m, 5, False)
    mesh = FEMesh.rectangle(3, 3)
    with pytest.raises(ValueError):
        AnisotropicFESolver(mesh, torch.ones(4))
    with pytest.raises(ValueError):
        AnisotropicFESolver(mesh, torch.ones(mesh.n_elements, 6))
    s = AnisotropicFESolver(mesh)
    assert s.kappa.tolist() == [1.0, 1.0, 0.0] and s._tensor_components() == 3
    assert AnisotropicFESolver(FEMesh.box(2, 2, 2)).kappa.tolist() == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    assert DifferentiableFESolver3D(mesh)._tensor_components() == 0


def test_voigt_full_round_trip():
    gen = torch.Generator().manual_seed(3)
    for d in (2, 3):
        A = torch.randn(4, 5, d, d, generator=gen, dtype=T64)
        K = A + A.transpose(-1, -2)
        kv = aniso.voigt(K)
        assert kv.shape == (4, 5, d * (d + 1) // 2)
        assert torch.equal(aniso.full(kv), K)
        assert torch.equal(aniso.voigt(aniso.full(kv)), kv)
        assert torch.equal(aniso.full(kv), _full(kv, d))                    # the convention of the yardstick
        for c, (i, j) in enumerate(_VOIGT[d]):
            assert torch.equal(kv[..., c], K[..., i, j])
    # one parameter fills both entries: its gradient is the sum of the two entry gradients
    kv = torch.tensor([2.0, 3.0, 0.5], dtype=T64, requires_grad=True)
    W = torch.tensor([[1.0, 10.0], [100.0, 1000.0]], dtype=T64)
    (g,) = torch.autograd.grad((aniso.full(kv) * W).sum(), kv)
    assert g.tolist() == [1.0, 1000.0, 110.0]
    with pytest.raises(ValueError):
        aniso.full(torch.ones(4))
    with pytest.raises(ValueError):
        aniso.voigt(torch.ones(2, 3))


def test_rotated_helpers():
    theta = torch.linspace(-3.0, 3.0, 13, dtype=T64)
    k = torch.tensor(1.7, dtype=T64)
    iso = aniso.full(aniso.rotated(k, k, theta))
    assert torch.equal(iso, (k * torch.eye(2, dtype=T64)).expand(13, 2, 2))
    # the fibre direction carries k_par, the normal k_perp
    kv = aniso.rotated(5.0, 0.5, theta)
    a = torch.stack([torch.cos(theta), torch.sin(theta)], -1)
    nrm = torch.stack([-torch.sin(theta), torch.cos(theta)], -1)
    K = aniso.full(kv)
    assert torch.allclose((K @ a[..., None])[..., 0], 5.0 * a, rtol=0, atol=1e-14)
    assert torch.allclose((K @ nrm[..., None])[..., 0], 0.5 * nrm, rtol=0, atol=1e-14)
    # differentiable in the angle
    th = torch.tensor(0.4, dtype=T64, requires_grad=True)
    (g,) = torch.autograd.grad(aniso.rotated(3.0, 1.0, th)[2], th)
    assert abs(float(g) - 2.0 * np.cos(0.8)) < 1e-14
    # 3D: a fibre along a (non-unit) direction; k_par == k_perp is k I
    dirs = torch.tensor([[0.0, 0.0, 2.0], [1.0, 1.0, 0.0], [1.0, -2.0, 0.5]], dtype=T64)
    K3 = aniso.full(aniso.transverse_isotropic(4.0, 1.0, dirs))
    unit = dirs / dirs.norm(dim=1, keepdim=True)
    assert torch.allclose((K3 @ unit[..., None])[..., 0], 4.0 * unit, rtol=0, atol=1e-14)
    assert torch.allclose(torch.linalg.eigvalsh(K3), torch.tensor([1.0, 1.0, 4.0], dtype=T64).expand(3, 3), atol=1e-13)
    assert torch.allclose(aniso.full(aniso.transverse_isotropic(k, k, dirs)), (k * torch.eye(3, dtype=T64)).expand(3, 3, 3),
                          rtol=0, atol=1e-15)
    # in the plane it is the 2D helper
    t = 0.7
    k3 = aniso.transverse_isotropic(3.0, 1.0, torch.tensor([np.cos(t), np.sin(t), 0.0], dtype=T64))
    k2 = aniso.rotated(3.0, 1.0, t)
    assert torch.allclose(k3[[0, 1, 5]], k2, rtol=0, atol=1e-15) and torch.equal(k3[[2, 3, 4]], torch.tensor([1.0, 0, 0], dtype=T64))


def test_validate_raises_on_an_indefinite_tensor():
    """The check runs before anything touches the device: no GPU needed to be refused."""
    mesh = FEMesh.rectangle(3, 3)
    m, n = mesh.n_elements, mesh.n_nodes
    f = torch.ones(2, n, dtype=T64)
    good = _spd_voigt((2, m), 2, 1)
    bad = good.clone()
    bad[1, 7] = torch.tensor([1.0, 1.0, 1.5])                     # det < 0
    for kv in (bad, bad[1], bad[:, 7], bad[1, 7]):
        with pytest.raises(ValueError, match="positive definite"):
            AnisotropicFESolver(mesh, kv, validate=True)(f)
    with pytest.raises(ValueError, match="positive definite"):    # (nc, m, B), layout='node'
        AnisotropicFESolver(mesh, bad.permute(2, 1, 0).contiguous(), validate=True)(f.t().contiguous(), layout="node")
    nan = good.clone()
    nan[0, 0, 2] = float("nan")
    with pytest.raises(ValueError, match="positive definite"):
        AnisotropicFESolver(mesh, nan, validate=True)(f)
    neg = good.clone()
    neg[0, 3] = torch.tensor([2.0, -1.0, 0.0])
    with pytest.raises(ValueError, match="positive definite"):
        AnisotropicFESolver(mesh, neg, validate=True)(f)
    box = FEMesh.box(2, 2, 2)
    k3 = _spd_voigt((box.n_elements,), 3, 2)
    k3[5] = torch.tensor([1.0, 1.0, 1.0, 0.9, 0.9, -0.9])         # leading minors 1, 0.19 > 0, det < 0
    with pytest.raises(ValueError, match="positive definite"):
        AnisotropicFESolver(box, k3, validate=True)(torch.ones(box.n_nodes, dtype=T64))
    assert bool(aniso._positive_definite(good, -1)) and bool(aniso._positive_definite(_spd_voigt((9,), 3, 4), -1))


def test_refused_combinations():
    rect = FEMesh.rectangle(3, 3)
    kv = torch.tensor([2.0, 1.0, 0.3], dtype=T64)
    with pytest.raises(NotImplementedError, match="dirichlet="):
        AnisotropicFESolver(rect, kv)(torch.ones(rect.n_nodes, dtype=T64), dirichlet=rect.dirichlet_values())
    with pytest.raises(NotImplementedError, match="P1"):
        AnisotropicFESolver(FEMesh.rectangle_p2(2, 2), kv)
    with pytest.raises(NotImplementedError, match="1D"):
        AnisotropicFESolver(FEMesh.line(5), kv)
    with pytest.raises(NotImplementedError, match="ShapeDifferentiableFESolver"):
        type("Both", (AnisotropicFESolver, ShapeDifferentiableFESolver), {})
    with pytest.raises(NotImplementedError, match="ShapeDifferentiableFESolver"):
        type("Both", (ShapeDifferentiableFESolver, AnisotropicFESolver), {})
    # backward with create_graph=True: autograd runs the backward with grad mode on; refused before any solve
    s = AnisotropicFESolver(rect, kv)
    solver_mod._SOLVERS[id(s)] = s
    ctx = types.SimpleNamespace(needs_input_grad=(True, True, False, False, False), handle=id(s))
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="create_graph"):
        solver_mod._fe_backward(ctx, torch.ones(rect.n_nodes, dtype=T64), None)


# ------------------------------------------------------------------------------------------------
# GPU: against the dense yardstick
# ------------------------------------------------------------------------------------------------
def _layout_tensor(layout, B, m, d, seed):
    """(leaf in the API's layout, function leaf -> (B, m, nc) for the yardstick)."""
    nc = d * (d + 1) // 2
    if layout == "homogeneous":
        return _spd_voigt((), d, seed), lambda k: k.expand(B, m, nc)
    if layout == "sample":
        return _spd_voigt((B,), d, seed), lambda k: k[:, None, :].expand(B, m, nc)
    if layout == "element":
        return _spd_voigt((m,), d, seed), lambda k: k[None].expand(B, m, nc)
    return _spd_voigt((B, m), d, seed), lambda k: k


def _compare_with_dense(mesh, layout, B=3, reaction=0.0, node=False, seed=0, **options):
    d, n, m = mesh.dim, mesh.n_nodes, mesh.n_elements
    gen = torch.Generator().manual_seed(100 + seed)
    f0 = 1 + 0.5 * torch.randn(B, n, generator=gen, dtype=T64)
    l0 = 0.2 * torch.randn(B, n, generator=gen, dtype=T64)
    w = 0.5 + torch.rand(B, n, generator=gen, dtype=T64)
    k0, expand = _layout_tensor(layout, B, m, d, 200 + seed)
    # yardstick
    kd, fd, ld = (t.clone().requires_grad_(True) for t in (k0, f0, l0))
    ud = _dense_solve(mesh, expand(kd), fd, ld, c=reaction)
    (w * ud ** 2).sum().backward()
    # HIP
    kh = (k0.permute(2, 1, 0).contiguous() if node else k0.clone()).to(DEV).requires_grad_(True)
    fh = (f0.t().contiguous() if node else f0.clone()).to(DEV).requires_grad_(True)
    lh = (l0.t().contiguous() if node else l0.clone()).to(DEV).requires_grad_(True)
    wh = (w.t().contiguous() if node else w).to(DEV)
    solver = AnisotropicFESolver(mesh, kh, device=DEV, reaction=reaction, validate=True, **options)
    with _strict():
        uh = solver(fh, load=lh, layout="node" if node else "sample")
        _converged(solver)
        (wh * uh ** 2).sum().backward()
        _converged(solver)
    back = (lambda t: t.permute(2, 1, 0)) if node else (lambda t: t)
    tr = (lambda t: t.t()) if node else (lambda t: t)
    assert kh.grad.shape == kh.shape
    print(f"{layout} node={node}: u {rel_err(tr(uh).detach().cpu().numpy(), ud.detach().numpy()):.2e} "
          f"dK {rel_err(back(kh.grad).cpu().numpy(), kd.grad.numpy()):.2e} "
          f"df {rel_err(tr(fh.grad).cpu().numpy(), fd.grad.numpy()):.2e} "
          f"dload {rel_err(tr(lh.grad).cpu().numpy(), ld.grad.numpy()):.2e} iters {solver.last_info.iterations}")
    assert rel_err(tr(uh).detach().cpu().numpy(), ud.detach().numpy()) < RTOL_U
    assert rel_err(back(kh.grad).cpu().numpy(), kd.grad.numpy()) < RTOL_GRAD
    assert rel_err(tr(fh.grad).cpu().numpy(), fd.grad.numpy()) < RTOL_GRAD
    assert rel_err(tr(lh.grad).cpu().numpy(), ld.grad.numpy()) < RTOL_GRAD
    return solver, uh, kh, fh, lh


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["homogeneous", "sample", "element", "sample_element"])
@pytest.mark.parametrize("name", ["rect", "rect_permuted", "box"])
def test_dense_parity(name, layout):
    mesh = _small_meshes()[name]
    assert mesh.n_nodes <= 200
    solver, *_ = _compare_with_dense(mesh, layout, seed=len(name) + len(layout))
    assert not solver.last_info.factored


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_permuted", "box"])
def test_dense_parity_with_reaction(name):
    _compare_with_dense(_small_meshes()[name], "sample_element", reaction=3.0, seed=7)
    _compare_with_dense(_small_meshes()[name], "homogeneous", reaction=3.0, seed=8)


@pytest.mark.gpu
def test_dense_parity_jacobi_method():
    solver, *_ = _compare_with_dense(_small_meshes()["rect"], "element", seed=9, method="ell-jacobi")
    assert solver.last_info.path == "ell-pcg"


@pytest.mark.gpu
@pytest.mark.parametrize("name,B", [("rect", 3), ("rect_permuted", 4), ("box", 3)])
def test_node_layout_dense_parity_and_bitwise_equal_to_sample_layout(name, B):
    mesh = _small_meshes()[name]
    _, un, kn, fn, ln = _compare_with_dense(mesh, "sample_element", B=B, node=True, seed=21)
    _, us, ks, fs, ls = _compare_with_dense(mesh, "sample_element", B=B, node=False, seed=21)
    assert torch.equal(un.t(), us)
    assert torch.equal(kn.grad.permute(2, 1, 0), ks.grad)
    assert torch.equal(fn.grad.t(), fs.grad)
    assert torch.equal(ln.grad.t(), ls.grad)


# ------------------------------------------------------------------------------------------------
# GPU: isotropic tensors against the scalar solver; the unpruned 3D pattern
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect2d", "box"])
def test_isotropic_tensor_matches_the_scalar_solver(name):
    if name == "rect2d":
        mesh = _permuted(_with_bc_data(_jittered(FEMesh.rectangle(12, 10), 0.2, 4), lambda x: 0.2 + x[0] - x[1]), 6)
    else:
        mesh = FEMesh.box(5, 4, 4, bc_value=0.25)         # axis-aligned: the scalar solver prunes its pattern here
    d, n, m, B = mesh.dim, mesh.n_nodes, mesh.n_elements, 5
    nc = d * (d + 1) // 2
    gen = torch.Generator().manual_seed(31)
    kappa = (0.5 + 2.0 * torch.rand(B, m, generator=gen, dtype=T64))
    f = 1 + 0.5 * torch.randn(B, n, generator=gen, dtype=T64)
    w = (0.5 + torch.rand(B, n, generator=gen, dtype=T64)).to(DEV)
    ks = kappa.clone().to(DEV).requires_grad_(True)
    scalar = DifferentiableFESolver3D(mesh, ks, device=DEV, method="ell")
    kt0 = torch.zeros(B, m, nc, dtype=T64)
    kt0[..., :d] = kappa[..., None]
    kt = kt0.to(DEV).requires_grad_(True)
    tensor = AnisotropicFESolver(mesh, kt, device=DEV)
    with _strict():
        us = scalar(f.to(DEV))
        (w * us ** 2).sum().backward()
        assert scalar.last_info.not_converged == 0
        ut = tensor(f.to(DEV))
        _converged(tensor)
        (w * ut ** 2).sum().backward()
        _converged(tensor)
    if name == "box":
        from diffhe.plan import get_plan
        pruned, fullp = get_plan(mesh, torch.device(DEV)), tensor._plan()
        assert pruned is not fullp and pruned.pruned_entries > 0 and fullp.pruned_entries == 0 and fullp.W > pruned.W
        assert get_plan(mesh, torch.device(DEV)) is pruned and tensor._plan() is fullp      # both stay cached
    trace = kt.grad[..., :d].sum(-1)
    print(f"{name}: u {rel_err(ut.detach().cpu().numpy(), us.detach().cpu().numpy()):.2e} "
          f"trace {rel_err(trace.cpu().numpy(), ks.grad.cpu().numpy()):.2e}")
    assert rel_err(ut.detach().cpu().numpy(), us.detach().cpu().numpy()) < RTOL_U
    assert rel_err(trace.cpu().numpy(), ks.grad.cpu().numpy()) < RTOL_GRAD


@pytest.mark.gpu
def test_box_with_off_diagonals_uses_the_unpruned_pattern():
    """On the axis-aligned box a scalar kappa leaves 6 of the 14 couplings of a node exactly zero; a tensor with
    off-diagonal components fills them.  A solve that stayed on the pruned pattern misses the dense yardstick here."""
    mesh = FEMesh.box(4, 4, 4, bc_value=0.2)
    n, m, B = mesh.n_nodes, mesh.n_elements, 2
    kv = _spd_voigt((B, m), 3, 41)
    assert float(kv[..., 3:].abs().mean()) > 0.1
    gen = torch.Generator().manual_seed(42)
    f = 1 + 0.5 * torch.randn(B, n, generator=gen, dtype=T64)
    ud = _dense_solve(mesh, kv, f)
    solver = AnisotropicFESolver(mesh, kv.to(DEV), device=DEV)
    with _strict():
        uh = solver(f.to(DEV))
        _converged(solver)
    assert solver._plan().W == 15
    print(f"box 4^3: u {rel_err(uh.cpu().numpy(), ud.numpy()):.2e}")
    assert rel_err(uh.cpu().numpy(), ud.numpy()) < RTOL_U


# ------------------------------------------------------------------------------------------------
# GPU: 64^2, where the multigrid hierarchy is real -- rotation identity and a sparse-LU yardstick
# ------------------------------------------------------------------------------------------------
def _mesh64():
    base = _with_bc_data(_jittered(FEMesh.rectangle(64, 64), 0.2, 8), lambda x: 0.1 * np.sin(3 * x[0]) + 0.2 * x[1])
    return _permuted(base, 9)


def _smooth_field(mesh, B, seed):
    """(B, m, 3) smooth SPD fields: fibre angle and principal conductivities vary smoothly with the element centroid;
    eigenvalue ratio <= 4.5 / 0.5 = 9."""
    c = mesh.nodes[mesh.elements].mean(1)                              # (m, 2)
    gen = torch.Generator().manual_seed(seed)
    ph = 6.28 * torch.rand(B, 4, generator=gen, dtype=T64)
    x, y = c[None, :, 0], c[None, :, 1]
    theta = 1.2 * torch.sin(2.0 * x + ph[:, 0:1]) + 0.8 * torch.cos(3.0 * y + ph[:, 1:2])
    k_par = 3.0 + 1.5 * torch.sin(4.0 * x * y + ph[:, 2:3])            # [1.5, 4.5]
    k_perp = 1.0 + 0.5 * torch.cos(5.0 * (x - y) + ph[:, 3:4])         # [0.5, 1.5]
    return aniso.rotated(k_par, k_perp, theta)


def _rotation(angle):
    return torch.tensor([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]], dtype=T64)


@pytest.mark.gpu
def test_rotation_identity_64():
    """The same problem in a rotated frame -- nodes X R^T, tensors R K R^T -- has the same u and, rotated back, the same
    tensor gradient.  Both sides are iterative solves of differently rounded systems."""
    mesh = _mesh64()
    n, m, B = mesh.n_nodes, mesh.n_elements, 2
    R = _rotation(0.6)
    kv = _smooth_field(mesh, B, 51)
    lam = torch.linalg.eigvalsh(aniso.full(kv))
    assert float((lam[..., 1] / lam[..., 0]).max()) <= 10.0
    kv_rot = aniso.voigt(R @ aniso.full(kv) @ R.t())
    mesh_rot = FEMesh(nodes=mesh.nodes @ R.t(), elements=mesh.elements, dirichlet_nodes=dict(mesh.dirichlet_nodes))
    gen = torch.Generator().manual_seed(52)
    f = (1 + 0.5 * torch.randn(B, n, generator=gen, dtype=T64)).to(DEV)
    w = (0.5 + torch.rand(B, n, generator=gen, dtype=T64)).to(DEV)
    out = []
    for msh, k in ((mesh, kv), (mesh_rot, kv_rot)):
        kh = k.to(DEV).requires_grad_(True)
        solver = AnisotropicFESolver(msh, kh, device=DEV)
        with _strict():
            u = solver(f)
            _converged(solver)
            assert solver.last_info.path == "ell-amgpcg"
            (w * u ** 2).sum().backward()
            _converged(solver)
        out.append((u.detach().cpu(), kh.grad.cpu(), solver.last_info.iterations))
    (u0, g0, it0), (u1, g1, it1) = out

    def entry_gradient(gv):          # the symmetric matrix of derivatives per ENTRY: half the parameter's on each side
        return aniso.full(gv * torch.tensor([1.0, 1.0, 0.5], dtype=T64))

    back = aniso.voigt(R.t() @ entry_gradient(g1) @ R) * torch.tensor([1.0, 1.0, 2.0], dtype=T64)
    print(f"rotation 64^2: u {rel_err(u1.numpy(), u0.numpy()):.2e} dK {rel_err(back.numpy(), g0.numpy()):.2e} "
          f"iterations {it0} / {it1}")
    assert rel_err(u1.numpy(), u0.numpy()) < RTOL_U
    assert rel_err(back.numpy(), g0.numpy()) < RTOL_GRAD


def _sparse_lu_reference(mesh, kv_bme, f_bn, w_bn):
    """numpy / scipy restatement with the explicit adjoint: u (B, n) and dL/dK (B, m, 3) of L = sum w u^2, 2D."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    X, el = mesh.nodes.numpy(), mesh.elements.numpy()
    n, m = len(X), len(el)
    x, y = X[el][..., 0], X[el][..., 1]
    det = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    G = np.stack([np.stack([y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]], 1),
                  np.stack([x[:, 2] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 0]], 1)], 2) / det[:, None, None]
    area = 0.5 * np.abs(det)
    rows, cols = np.repeat(el, 3, axis=1).reshape(-1), np.tile(el, (1, 3)).reshape(-1)
    M = sp.csr_matrix((np.repeat(area / 9.0, 9), (rows, cols)), shape=(n, n))
    bcn = np.array(sorted(mesh.dirichlet_nodes), dtype=np.int64)
    g = np.zeros(n)
    g[bcn] = [float(mesh.dirichlet_nodes[int(k)]) for k in bcn]
    free = np.setdiff1d(np.arange(n), bcn)
    us, gs = [], []
    for kv, f, w in zip(kv_bme.numpy(), f_bn.numpy(), w_bn.numpy()):
        Kf = np.empty((m, 2, 2))
        Kf[:, 0, 0], Kf[:, 1, 1], Kf[:, 0, 1], Kf[:, 1, 0] = kv[:, 0], kv[:, 1], kv[:, 2], kv[:, 2]
        ke = area[:, None, None] * np.einsum("epa,eac,eqc->epq", G, Kf, G)
        K = sp.csr_matrix((ke.reshape(-1), (rows, cols)), shape=(n, n))
        lu = spla.splu(K[free][:, free].tocsc())
        u = g.copy()
        u[free] = lu.solve((M @ f - K @ g)[free])
        lam = np.zeros(n)
        lam[free] = lu.solve((2.0 * w * u)[free])
        gl, gu = np.einsum("ep,epa->ea", lam[el], G), np.einsum("ep,epa->ea", u[el], G)
        gs.append(-area[:, None] * np.stack([gl[:, 0] * gu[:, 0], gl[:, 1] * gu[:, 1],
                                             gl[:, 0] * gu[:, 1] + gl[:, 1] * gu[:, 0]], 1))
        us.append(u)
    return np.stack(us), np.stack(gs)


@pytest.mark.gpu
def test_sparse_lu_yardstick_64():
    mesh = _mesh64()
    n, B = mesh.n_nodes, 8
    kv = _smooth_field(mesh, B, 61)
    gen = torch.Generator().manual_seed(62)
    f = 1 + 0.5 * torch.randn(B, n, generator=gen, dtype=T64)
    w = 0.5 + torch.rand(B, n, generator=gen, dtype=T64)
    u_ref, g_ref = _sparse_lu_reference(mesh, kv, f, w)
    kh = kv.to(DEV).requires_grad_(True)
    solver = AnisotropicFESolver(mesh, kh, device=DEV)
    with _strict():
        u = solver(f.to(DEV))
        _converged(solver)
        (w.to(DEV) * u ** 2).sum().backward()
        _converged(solver)
    print(f"sparse LU 64^2 x 8: u {rel_err(u.detach().cpu().numpy(), u_ref):.2e} "
          f"dK {rel_err(kh.grad.cpu().numpy(), g_ref):.2e} iterations {solver.last_info.iterations} + "
          f"{solver.last_info.adj_iterations}")
    assert rel_err(u.detach().cpu().numpy(), u_ref) < RTOL_U
    assert rel_err(kh.grad.cpu().numpy(), g_ref) < RTOL_GRAD


# ------------------------------------------------------------------------------------------------
# GPU: second-order convergence, determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_second_order_convergence():
    """u = sin pi x sin pi y on rectangle(N, N), K = [[3, 1.2], [1.2, 1]] constant, f = pi^2 [(Kxx + Kyy) sin sin
    - 2 Kxy cos cos].  The discretisation is fully specified, so the nodal error is a property of the scheme: a CPU
    restatement gives 4.23e-3, 1.0618e-3, 2.66e-4 at N = 32, 64, 128 (orders 1.994, 1.998)."""
    kv = torch.tensor([3.0, 1.0, 1.2], dtype=T64)
    errs = []
    for N in (32, 64, 128):
        mesh = FEMesh.rectangle(N, N)
        x, y = mesh.nodes[:, 0], mesh.nodes[:, 1]
        exact = torch.sin(np.pi * x) * torch.sin(np.pi * y)
        f = np.pi ** 2 * ((kv[0] + kv[1]) * exact - 2.0 * kv[2] * torch.cos(np.pi * x) * torch.cos(np.pi * y))
        solver = AnisotropicFESolver(mesh, kv, device=DEV)
        with _strict():
            u = solver(f.to(DEV))
            _converged(solver)
        errs.append(float((u.cpu() - exact).abs().max()))
    orders = [float(np.log2(errs[i] / errs[i + 1])) for i in range(2)]
    print(f"convergence: errors {errs} orders {orders}")
    assert orders[0] >= 1.9 and orders[1] >= 1.9
    assert abs(errs[1] - 1.0618e-3) <= 0.05 * 1.0618e-3


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["sample_element", "element"])
def test_determinism(layout):
    mesh = _permuted(_with_bc_data(_jittered(FEMesh.rectangle(40, 36), 0.2, 4), lambda x: 0.2 + x[0] * x[1]), 5)
    n, m, B = mesh.n_nodes, mesh.n_elements, 6
    gen = torch.Generator().manual_seed(71)
    f0 = 1 + 0.5 * torch.randn(B, n, generator=gen, dtype=T64)
    l0 = 0.2 * torch.randn(B, n, generator=gen, dtype=T64)
    k0 = _smooth_field(mesh, B, 72) if layout == "sample_element" else _smooth_field(mesh, 1, 72)[0]
    runs = []
    for _ in range(2):
        kh, fh, lh = (t.clone().to(DEV).requires_grad_(True) for t in (k0, f0, l0))
        solver = AnisotropicFESolver(mesh, kh, device=DEV)
        with _strict():
            u = solver(fh, load=lh)
            _converged(solver)
            (u ** 2).sum().backward()
            _converged(solver)
        runs.append((u.detach().clone(), kh.grad.clone(), fh.grad.clone(), lh.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert runs[0][1].shape == k0.shape and float(runs[0][1].abs().max()) > 0


@pytest.mark.gpu
def test_create_graph_is_refused():
    mesh = _small_meshes()["rect"]
    kh = _spd_voigt((mesh.n_elements,), 2, 81).to(DEV).requires_grad_(True)
    solver = AnisotropicFESolver(mesh, kh, device=DEV)
    u = solver(torch.ones(mesh.n_nodes, dtype=T64, device=DEV))
    with pytest.raises(NotImplementedError, match="create_graph"):
        torch.autograd.grad((u ** 2).sum(), kh, create_graph=True)
