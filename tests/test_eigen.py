"""Smallest eigenpairs of K(kappa) phi = lambda M_L phi per sample and d lambda / d kappa (diffhe.eigen).

The yardstick is a dense restatement written here (`dense_eig`): K and the lumped mass from the element forms of
tests/test_robin.py, M^-1/2 K M^-1/2 on the free nodes, `torch.linalg.eigh`, autograd for d lambda / d kappa.  It is itself
pinned on the CPU to the closed form of the lumped P1 operator on `FEMesh.rectangle` (kappa times the anisotropic 5-point
stencil, every interior lumped mass hx hy):

    lambda_pq = kappa [ (4 / hx^2) sin^2(p pi hx / 2 Lx) + (4 / hy^2) sin^2(q pi hy / 2 Ly) ],

p, q >= 1 with Dirichlet data on the boundary, p, q >= 0 (cosine modes) on the same lattice with no Dirichlet node.

Tolerances, with their reasons:
  * eigenvalues: RTOL_U (1e-10) with tol = 1e-8.  |lambda - theta| <= rho^2 lambda^2 / gap is <= 1e-15 lambda on these
    meshes, so 1e-10 is the project's operator tolerance, not a solver allowance;
  * eigenvectors of isolated eigenvalues, sign fixed first: max-norm error relative to |phi|_inf <= 10 tol lambda_i / gap_i,
    gap_i the distance to the nearest other eigenvalue of the dense spectrum (Davis-Kahan; the 10 covers its constant and the
    change of norm).  Clusters: the M-orthogonal projector onto the span, same bound with the gap of the cluster;
  * per-element gradients are first order in the eigenvector error: run with tol = 1e-11 (the rounding floor of rho is about
    eps lambda_max / lambda_min ~ 1e-13 here) and held to the same 10 tol lambda_i / gap_i; the per-sample scalar gradient
    obeys kappa_b d lambda / d kappa_b = lambda to second order (homogeneity): RTOL_GRAD;
  * central differences, step 1e-5, tolerance 1e-7: the reasoning in the header of tests/test_robin.py;
  * the Ritz kernel alone on pencils with cond(G_M) < 10: 1e-12 (a p <= 16 Jacobi iteration in fp64).
"""
import math
import warnings

import numpy as np
import pytest
import torch

from diffhe import FEMesh
from _util import RTOL_GRAD, RTOL_U, rel_err

T64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# the dense restatement
# ---------------------------------------------------------------------------------------------------------------------
def element_forms(nodes, el):
    """Unit-kappa stiffness and load matrix of every P1 triangle / tetrahedron, (m, npe, npe) each (tests/test_robin.py)."""
    P = nodes[el]
    dim = nodes.shape[1]
    ones = torch.ones(len(el), 1, dtype=T64)
    A = torch.cat([ones[:, None].expand(-1, dim + 1, 1), P], dim=2)
    size = torch.linalg.det(A).abs() / math.factorial(dim)
    G = torch.linalg.inv(A)[:, 1:, :]
    k0 = size[:, None, None] * (G.transpose(1, 2) @ G)
    m0 = (size / (dim + 1) ** 2)[:, None, None].expand(-1, dim + 1, dim + 1)
    return k0, m0


def dense_pencil(mesh, kappa_e):
    """K (n, n) (differentiable in kappa_e (m,)), the lumped mass (n,) and the mask of the free nodes."""
    n, el = mesh.n_nodes, mesh.elements
    npe = el.shape[1]
    k0, m0 = element_forms(mesh.nodes, el)
    rows = el[:, :, None].expand(-1, npe, npe).reshape(-1)
    cols = el[:, None, :].expand(-1, npe, npe).reshape(-1)
    K = torch.zeros(n * n, dtype=T64).index_add(0, rows * n + cols, (kappa_e[:, None, None] * k0).reshape(-1)).reshape(n, n)
    M = torch.zeros(n * n, dtype=T64).index_add(0, rows * n + cols, m0.reshape(-1)).reshape(n, n)
    free = torch.ones(n, dtype=torch.bool)
    free[list(mesh.dirichlet_nodes.keys())] = False
    return K, M.sum(1), free


def dense_eig(mesh, kappa_e):
    """All eigenpairs of the free block: lam (nf,) ascending, phi (nf, n) M-orthonormal, zero on the Dirichlet nodes."""
    K, mass, free = dense_pencil(mesh, kappa_e)
    s = mass[free] ** -0.5
    S = s[:, None] * K[free][:, free] * s[None, :]
    lam, V = torch.linalg.eigh(0.5 * (S + S.t()))
    phi = torch.zeros(len(lam), mesh.n_nodes, dtype=T64)
    phi[:, free] = (s[:, None] * V).t()
    return lam, phi, mass


def closed_form(nx, ny, Lx, Ly, kappa=1.0, neumann=False):
    hx, hy = Lx / nx, Ly / ny
    lo = 0 if neumann else 1
    p = np.arange(lo, nx + (1 if neumann else 0))[:, None]
    q = np.arange(lo, ny + (1 if neumann else 0))[None, :]
    lam = kappa * (4 / hx ** 2 * np.sin(p * np.pi * hx / (2 * Lx)) ** 2 + 4 / hy ** 2 * np.sin(q * np.pi * hy / (2 * Ly)) ** 2)
    return np.sort(lam.reshape(-1))


def gaps(lam_all, idx):
    """Distance of lam_all[i] to the nearest other eigenvalue, i in idx."""
    lam_all = np.asarray(lam_all)
    return np.array([np.min(np.abs(np.delete(lam_all, i) - lam_all[i])) for i in idx])


def kappa_rows(kappa, m, B):
    """(B, m) rows of any scalar-kappa layout."""
    k = kappa.detach().to("cpu", T64)
    if k.numel() == 1:
        return k.reshape(1, 1).expand(B, m)
    if k.dim() == 1 and k.shape[0] == m and B != m:
        return k.reshape(1, m).expand(B, m)
    if k.dim() == 1 or (k.dim() == 2 and k.shape[1] == 1):
        return k.reshape(B, 1).expand(B, m)
    return k


def jittered(mesh, seed=0, amount=0.25, permute=True):
    """Interior nodes moved by up to `amount` of the smallest spacing, node ids shuffled: no lattice left."""
    rng = np.random.default_rng(seed)
    X = mesh.nodes.numpy().copy()
    lo, hi = X.min(0), X.max(0)
    interior = np.all((X > lo + 1e-9) & (X < hi - 1e-9), axis=1)
    spacing = min(np.diff(np.unique(np.round(X[:, k], 12))).min() for k in range(X.shape[1]))
    X[interior] += rng.uniform(-amount * spacing, amount * spacing, (int(interior.sum()), X.shape[1]))
    el = mesh.elements.numpy().copy()
    bc = dict(mesh.dirichlet_nodes)
    if permute:
        perm = rng.permutation(len(X))
        Xn = np.empty_like(X)
        Xn[perm] = X
        X, el = Xn, perm[el]
        bc = {int(perm[k]): v for k, v in bc.items()}
    return FEMesh(nodes=torch.from_numpy(X), elements=torch.from_numpy(el), dirichlet_nodes=bc)


LATTICE = dict(nx=16, ny=12, x_range=(0.0, 1.5), y_range=(0.0, 1.0))


def lattice_mesh():
    return FEMesh.rectangle(**LATTICE)


def field(m, seed, B=None, lo=0.6, hi=1.6):
    gen = torch.Generator().manual_seed(seed)
    shape = (m,) if B is None else (B, m)
    return lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=T64)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the yardstick pinned, the Hellmann-Feynman formula, host logic
# ---------------------------------------------------------------------------------------------------------------------
def test_import_from_the_package():
    from diffhe import EigenFESolver
    import diffhe
    assert "EigenFESolver" in diffhe.__all__ and EigenFESolver is diffhe.eigen.EigenFESolver


def test_dense_restatement_matches_the_closed_form():
    mesh = lattice_mesh()
    lam, phi, mass = dense_eig(mesh, torch.full((mesh.n_elements,), 1.3, dtype=T64))
    exact = closed_form(16, 12, 1.5, 1.0, 1.3)
    print("dense vs closed form:", rel_err(lam.numpy(), exact))
    assert rel_err(lam.numpy(), exact) <= RTOL_U
    assert np.allclose(lam[:5].numpy() / 1.3, [14.19, 27.14, 42.96, 48.16, 55.91], atol=5e-3)
    assert (gaps(lam.numpy(), range(5)) / lam[:5].numpy()).min() >= 0.1
    G = (phi * mass) @ phi.t()
    assert rel_err(G.numpy(), np.eye(len(lam))) <= 1e-12


def cosine_bound(lam_cos, h):
    """Both the cosine form and the spectrum of the triangulation are second-order consistent with the continuum eigenvalue
    lambda_c: each within lambda_c^2 h^2 / 12 per direction of it to leading order, so within 4 lambda_c^2 h^2 / 12 of each
    other (lambda_c ~ lam_cos at the low modes this is used for)."""
    return 4.0 * lam_cos ** 2 * h ** 2 / 12.0


def test_cosine_form_without_dirichlet_nodes_is_second_order_close():
    """Without Dirichlet nodes the cosine closed form is NOT the exact spectrum of this triangulation: the two corners that
    belong to one triangle carry the lumped mass hx hy / 6, the other two hx hy / 3, not the hx hy / 4 of the 5-point
    Neumann stencil (measured: 2.8e-5 relative at lambda_2).  It is pinned to the h^2 level only; the lambda_1 = 0 mode is
    exact."""
    mesh = lattice_mesh()
    mesh = FEMesh(nodes=mesh.nodes, elements=mesh.elements, dirichlet_nodes={})
    lam, _, _ = dense_eig(mesh, torch.ones(mesh.n_elements, dtype=T64))
    exact = closed_form(16, 12, 1.5, 1.0, 1.0, neumann=True)
    print("neumann dense vs cosine form:", (lam[:6].numpy() - exact[:6]))
    assert abs(float(lam[0])) <= 1e-12 * float(lam[1])
    assert np.all(np.abs(lam[1:6].numpy() - exact[1:6]) <= cosine_bound(exact[1:6], 1.5 / 16))


def test_square_has_the_exact_pairs_used_by_the_cluster_tests():
    lam = closed_form(8, 8, 1.0, 1.0)
    assert lam[1] == lam[2] and lam[4] == lam[5] and lam[0] < lam[1] < lam[3] < lam[4]


def test_hellmann_feynman_equals_autograd_on_a_random_field():
    mesh = lattice_mesh()
    kap = field(mesh.n_elements, 3).requires_grad_(True)
    lam, phi, _ = dense_eig(mesh, kap)
    k0, _ = element_forms(mesh.nodes, mesh.elements)
    for i in range(5):
        (g,) = torch.autograd.grad(lam[i], kap, retain_graph=True)
        pe = phi[i].detach()[mesh.elements]                               # (m, 3)
        hf = torch.einsum("ep,epq,eq->e", pe, k0, pe)
        assert rel_err(hf.numpy(), g.numpy()) <= RTOL_GRAD


def test_refusals_and_argument_validation():
    from diffhe import EigenFESolver
    with pytest.raises(NotImplementedError):
        EigenFESolver(FEMesh.line(10))
    with pytest.raises(NotImplementedError):
        EigenFESolver(FEMesh.rectangle_p2(4, 4))
    mesh = FEMesh.rectangle(6, 5)
    m = mesh.n_elements
    with pytest.raises(NotImplementedError):
        EigenFESolver(mesh, torch.ones(2, m, 3, dtype=T64))
    with pytest.raises(NotImplementedError):
        EigenFESolver(mesh, torch.ones(4, 3, dtype=T64))
    bare = FEMesh(nodes=mesh.nodes, elements=mesh.elements, dirichlet_nodes={})
    with pytest.raises(ValueError):
        EigenFESolver(bare)
    assert EigenFESolver(bare, shift=1.0).inner.reaction == 1.0
    for bad in (dict(k=0), dict(k=9, guard=8), dict(guard=-1), dict(tol=0.0), dict(shift=-1.0), dict(reaction=1.0)):
        with pytest.raises(ValueError):
            EigenFESolver(mesh, **bad)
    es = EigenFESolver(mesh, torch.ones(3, dtype=T64), k=2)
    with pytest.raises(ValueError):
        es(layout="elements")
    with pytest.raises(ValueError):
        es(batch=4)                     # kappa carries 3 samples
    p = torch.nn.Parameter(torch.ones(m, dtype=T64))
    assert list(EigenFESolver(mesh, p).parameters())[0] is p


def test_layout_resolution():
    from diffhe.eigen import _eigen_layout
    from diffhe.solver import K_ELEM, K_SAMPLE, K_SAMPLE_ELEM, K_SCALAR
    m = 60
    one = torch.ones
    assert _eigen_layout(one(()), m, None) == (K_SCALAR, 1, False)
    assert _eigen_layout(one(()), m, 4) == (K_SCALAR, 4, True)
    assert _eigen_layout(one(m), m, None) == (K_ELEM, 1, False)
    assert _eigen_layout(one(m), m, 3) == (K_ELEM, 3, True)
    assert _eigen_layout(one(m), m, m) == (K_SAMPLE, m, True)           # batch=B forces the per-sample reading
    assert _eigen_layout(one(5), m, None) == (K_SAMPLE, 5, True)
    assert _eigen_layout(one(5, 1), m, None) == (K_SAMPLE, 5, True)
    assert _eigen_layout(one(5, m), m, None) == (K_SAMPLE_ELEM, 5, True)
    with pytest.raises(ValueError):
        _eigen_layout(one(5, 7), m, None)
    with pytest.raises(ValueError):
        _eigen_layout(one(5), m, 0)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def solve(mesh, kappa, k=4, **kw):
    from diffhe import EigenFESolver
    call = {name: kw.pop(name) for name in ("batch", "x0", "layout") if name in kw}
    es = EigenFESolver(mesh, kappa.to("cuda") if isinstance(kappa, torch.Tensor) else kappa, k, **kw)
    lam, phi = es(**call)
    return es, lam, phi


def as_rows(lam, phi, layout, batched=True):
    """lam (B, k), phi (B, k, n) on the CPU from either layout."""
    lam, phi = lam.detach().cpu(), phi.detach().cpu()
    if layout == "node":
        phi = phi.permute(2, 0, 1)
    elif not batched:
        phi = phi[None]
    return lam.reshape(phi.shape[0], -1), phi


def check_against_dense(mesh, kappa, lam, phi, tol, vectors=True, shift=0.0):
    """Eigenvalues to RTOL_U; isolated eigenvectors (sign fixed by the reference) to 10 tol lambda / gap; M-orthonormality,
    zero Dirichlet rows, ascending order.  shift: the residual the iteration stops on is relative to the eigenvalue
    lambda + shift of the operator it runs on, so that is the lambda of the bound (lambda_1 = 0 would give no bound)."""
    B, k = lam.shape
    rows = kappa_rows(kappa, mesh.n_elements, B)
    bc = list(mesh.dirichlet_nodes.keys())
    for b in range(B):
        ref_lam, ref_phi, mass = dense_eig(mesh, rows[b])
        err = rel_err(lam[b].numpy(), ref_lam[:k].numpy())
        print(f"sample {b}: eigenvalue rel_err {err:.2e}")
        assert err <= RTOL_U
        assert bool((lam[b][1:] >= lam[b][:-1]).all())
        G = (phi[b] * mass) @ phi[b].t()
        assert float((G - torch.eye(k, dtype=T64)).abs().max()) <= 1e-12
        if bc:
            assert float(phi[b][:, bc].abs().max()) == 0.0
        if not vectors:
            continue
        gap = gaps(ref_lam.numpy(), range(k))
        for i in range(k):
            r = ref_phi[i] * torch.sign((ref_phi[i] * mass * phi[b, i]).sum())
            bound = 10 * tol * (float(ref_lam[i]) + shift) / gap[i]
            e = float((phi[b, i] - r).abs().max() / r.abs().max())
            print(f"sample {b} mode {i}: eigenvector error {e:.2e} (bound {bound:.2e})")
            assert e <= bound


def layouts_kappa(mesh, name):
    m = mesh.n_elements
    if name == "scalar":
        return torch.tensor(1.3, dtype=T64), 1, False
    if name == "sample":
        return torch.tensor([0.7, 1.0, 2.2], dtype=T64), 3, True
    if name == "element":
        return field(m, 5), 1, False
    return field(m, 6, B=3), 3, True


@gpu
@pytest.mark.parametrize("layout", ["sample", "node"])
@pytest.mark.parametrize("name", ["scalar", "sample", "element", "sample_element"])
def test_lattice_path_every_layout(name, layout):
    mesh = lattice_mesh()
    kappa, B, batched = layouts_kappa(mesh, name)
    es, lam, phi = solve(mesh, kappa, 4, layout=layout)
    assert es.last_info.path.startswith("lattice") and es.last_info.not_converged == 0
    assert tuple(lam.shape) == ((B, 4) if batched else (4,))
    n = mesh.n_nodes
    assert tuple(phi.shape) == ((4, n, B) if layout == "node" else ((B, 4, n) if batched else (4, n)))
    assert not phi.requires_grad
    lam_r, phi_r = as_rows(lam, phi, layout, batched)
    check_against_dense(mesh, kappa, lam_r, phi_r, es.tol)
    mass = dense_eig(mesh, kappa_rows(kappa, mesh.n_elements, B)[0])[2]
    # the sign convention: sum m phi > 0, or -- antisymmetric modes, |sum| < 1e-8 -- the entry of largest magnitude positive
    # (a positive entry within rounding of the largest magnitude: +max and -min tie on such modes)
    s = (phi_r * mass).sum(2)
    top = phi_r.max(2).values >= (1 - 1e-9) * phi_r.abs().max(2).values
    assert bool(torch.where(s.abs() >= 1e-8, s > 0, top).all())


@gpu
@pytest.mark.parametrize("name", ["scalar", "sample", "element", "sample_element"])
def test_general_path_on_a_jittered_permuted_mesh(name):
    mesh = jittered(FEMesh.rectangle(14, 12, (0.0, 1.4), (0.0, 1.0)))
    kappa, B, batched = layouts_kappa(mesh, name)
    es, lam, phi = solve(mesh, kappa, 4)
    assert es.last_info.path.startswith("ell") and es.last_info.not_converged == 0
    lam_r, phi_r = as_rows(lam, phi, "sample", batched)
    check_against_dense(mesh, kappa, lam_r, phi_r, es.tol)


@gpu
def test_box_with_a_random_field():
    """Relative gaps inside the first eight fall to 1e-3 here: eigenvalues (and the invariants), not single vectors."""
    mesh = FEMesh.box(5, 5, 5)
    kappa = field(mesh.n_elements, 7, B=2)
    es, lam, phi = solve(mesh, kappa, 8, guard=4)
    assert es.last_info.path.startswith("ell") and es.last_info.not_converged == 0
    check_against_dense(mesh, kappa, *as_rows(lam, phi, "sample"), es.tol, vectors=False)


@gpu
def test_full_block_of_sixteen():
    mesh = lattice_mesh()
    kappa = field(mesh.n_elements, 8, B=2)
    es, lam, phi = solve(mesh, kappa, 5, guard=11)
    assert es.last_info.block == 16 and es.last_info.not_converged == 0
    check_against_dense(mesh, kappa, *as_rows(lam, phi, "sample"), es.tol)


@gpu
def test_batch_forces_the_per_sample_reading():
    mesh = FEMesh.rectangle(3, 2)            # m = 12 elements, 2 free nodes
    kappa = torch.linspace(0.5, 2.0, 12, dtype=T64)
    es, lam, phi = solve(mesh, kappa, 1, guard=1, batch=12)
    assert tuple(lam.shape) == (12, 1) and tuple(phi.shape) == (12, 1, mesh.n_nodes)
    check_against_dense(mesh, kappa.reshape(12, 1), *as_rows(lam, phi, "sample"), es.tol)
    es, lam, phi = solve(mesh, kappa, 1, guard=1)
    assert tuple(lam.shape) == (1,)
    check_against_dense(mesh, kappa.reshape(1, 12), *as_rows(lam, phi, "sample", False), es.tol)


@gpu
def test_warm_start_needs_fewer_outer_iterations():
    mesh = lattice_mesh()
    kappa = field(mesh.n_elements, 9, B=3)
    es, lam, phi = solve(mesh, kappa, 4)
    moved = kappa * (1 + 0.01 * torch.sin(torch.arange(mesh.n_elements, dtype=T64)))
    cold, lam_c, _ = solve(mesh, moved, 4)
    warm, lam_w, phi_w = solve(mesh, moved, 4, x0=phi)
    print("outer iterations cold / warm:", cold.last_info.outer_iterations, warm.last_info.outer_iterations)
    assert warm.last_info.outer_iterations < cold.last_info.outer_iterations
    assert warm.last_info.not_converged == 0
    check_against_dense(mesh, moved, *as_rows(lam_w, phi_w, "sample"), warm.tol)
    node, lam_n, phi_n = solve(mesh, moved, 4, layout="node")
    again, lam_a, _ = solve(mesh, moved, 4, layout="node", x0=phi_n)
    # a converged block restarted (its guard columns are new random ones) is at the stopping rule within a step or two
    assert again.last_info.outer_iterations <= 2 and rel_err(lam_a.cpu().numpy(), lam_n.cpu().numpy()) <= RTOL_U


@gpu
def test_shift_on_a_mesh_without_dirichlet_nodes():
    """The lambda_1 = 0 mode, the dense restatement, the cosine form to its h^2 level; the returned lambda exclude the
    shift."""
    base = lattice_mesh()
    mesh = FEMesh(nodes=base.nodes, elements=base.elements, dirichlet_nodes={})
    kappa = torch.tensor([1.0, 2.5], dtype=T64)
    es, lam, phi = solve(mesh, kappa, 4, shift=3.0)
    assert es.last_info.not_converged == 0
    lam = lam.cpu()
    exact = closed_form(16, 12, 1.5, 1.0, 1.0, neumann=True)[:4]
    for b in range(2):
        print("shifted:", lam[b].numpy(), float(kappa[b]) * exact)
        # the cosine form is second-order close only on this triangulation (see the CPU test above); the dense
        # restatement below is held to RTOL_U
        assert np.all(np.abs(lam[b].numpy() / float(kappa[b]) - exact) <= cosine_bound(exact, 1.5 / 16) + 1e-9)
        assert abs(float(lam[b, 0])) <= RTOL_U * float(lam[b, 1])
    check_against_dense(mesh, kappa, *as_rows(lam, phi, "sample"), es.tol, shift=3.0)


@gpu
def test_dirichlet_values_of_the_mesh_are_ignored():
    zero = lattice_mesh()
    some = FEMesh.rectangle(bc_value=0.7, **LATTICE)
    kappa = field(zero.n_elements, 10, B=2)
    _, lam0, phi0 = solve(zero, kappa, 3)
    _, lam1, phi1 = solve(some, kappa, 3)
    # the same operator and the same start block: equal up to rounding
    assert rel_err(lam1.cpu().numpy(), lam0.cpu().numpy()) <= 1e-13
    assert rel_err(phi1.cpu().numpy(), phi0.cpu().numpy()) <= RTOL_U
    jm = jittered(some, seed=2)
    es, lam, phi = solve(jm, kappa, 3)
    check_against_dense(jm, kappa, *as_rows(lam, phi, "sample"), es.tol)


@gpu
def test_identical_calls_are_bitwise_equal_and_max_iter_one_warns():
    mesh = jittered(FEMesh.rectangle(14, 12, (0.0, 1.4), (0.0, 1.0)))
    kappa = field(mesh.n_elements, 11, B=3)
    _, lam0, phi0 = solve(mesh, kappa, 4)
    _, lam1, phi1 = solve(mesh, kappa, 4)
    assert torch.equal(lam0, lam1) and torch.equal(phi0, phi1)
    with pytest.warns(RuntimeWarning, match="did not reach"):
        es, _, _ = solve(mesh, kappa, 4, max_iter=1)
    assert es.last_info.not_converged > 0 and es.last_info.outer_iterations == 1
    assert tuple(es.last_info.residual.shape) == (3, 4) and es.last_info.inner_solves == 1 + 8


# -- clusters ---------------------------------------------------------------------------------------------------------
@gpu
def test_cluster_projector_and_gradient_of_the_sum():
    """rectangle(8, 8): lambda_2 = lambda_3 exactly.  The span is compared through its M-orthogonal projector, the gradient
    through the symmetric function lambda_2 + lambda_3 (single members of the pair are not differentiable)."""
    mesh = FEMesh.rectangle(8, 8)
    tol = 1e-11
    kap = torch.ones(mesh.n_elements, dtype=T64, device="cuda", requires_grad=True)
    from diffhe import EigenFESolver
    es = EigenFESolver(mesh, kap, 4, tol=tol)
    lam, phi = es()
    assert es.last_info.not_converged == 0
    kc = torch.ones(mesh.n_elements, dtype=T64, requires_grad=True)
    ref_lam, ref_phi, mass = dense_eig(mesh, kc)
    assert rel_err(lam.detach().cpu().numpy(), ref_lam[:4].detach().numpy()) <= RTOL_U
    gap = float(min(ref_lam[1] - ref_lam[0], ref_lam[3] - ref_lam[2]))
    bound = 10 * tol * float(ref_lam[2]) / gap          # 10 tol lambda / gap of the cluster: ~3e-10
    P = phi.cpu()[1:3].t() @ (phi.cpu()[1:3] * mass)
    Pr = ref_phi.detach()[1:3].t() @ (ref_phi.detach()[1:3] * mass)
    print("projector error", float((P - Pr).abs().max()), "bound", bound)
    assert float((P - Pr).abs().max()) <= bound * float(Pr.abs().max())
    (lam[1] + lam[2]).backward()
    (g_ref,) = torch.autograd.grad(ref_lam[1] + ref_lam[2], kc)
    e = rel_err(kap.grad.cpu().numpy(), g_ref.numpy())
    print("cluster gradient rel_err", e, "bound", bound)
    assert e <= bound


# -- gradients --------------------------------------------------------------------------------------------------------
def dense_grad(mesh, rows, weights):
    """d/d kappa of sum_{b,i} weights[b,i] lambda_{b,i} by autograd through the dense restatement: (B, m)."""
    out = []
    for b in range(rows.shape[0]):
        kc = rows[b].clone().requires_grad_(True)
        lam, _, _ = dense_eig(mesh, kc)
        (g,) = torch.autograd.grad((weights[b] * lam[:weights.shape[1]]).sum(), kc)
        out.append(g)
    return torch.stack(out)


@gpu
@pytest.mark.parametrize("which", ["lattice", "general", "lattice64"])
def test_per_element_gradient_of_isolated_eigenvalues(which):
    tol = 1e-11
    mesh = lattice_mesh() if which.startswith("lattice") else jittered(FEMesh.rectangle(14, 12, (0.0, 1.4), (0.0, 1.0)))
    B = 64 if which == "lattice64" else 2         # 64 samples: the lattice strip kernel of the per-element gradient
    kappa = field(mesh.n_elements, 12, B=B)
    from diffhe import EigenFESolver
    kap = kappa.to("cuda").requires_grad_(True)
    es = EigenFESolver(mesh, kap, 3, tol=tol)
    lam, _ = es()
    assert es.last_info.not_converged == 0
    w = torch.tensor([1.0, -0.5, 0.25], dtype=T64).expand(B, 3)
    (lam * w.to("cuda")).sum().backward()
    check = range(B) if B == 2 else (0, 63)
    ref = dense_grad(mesh, kappa[list(check)], w[list(check)])
    for j, b in enumerate(check):
        ref_lam = dense_eig(mesh, kappa[b])[0].numpy()
        bound = float(np.max(10 * tol * ref_lam[:3] / gaps(ref_lam, range(3))))        # 10 tol lambda_i / gap_i
        e = rel_err(kap.grad[b].cpu().numpy(), ref[j].numpy())
        print(f"{which} sample {b}: gradient rel_err {e:.2e} (bound {bound:.2e})")
        assert e <= bound


@gpu
def test_shared_field_and_box_gradients():
    tol = 1e-11
    from diffhe import EigenFESolver
    mesh = lattice_mesh()                           # (m,) field: the gradient is one (m,) tensor
    kappa = field(mesh.n_elements, 13)
    kap = kappa.to("cuda").requires_grad_(True)
    lam, _ = EigenFESolver(mesh, kap, 2, tol=tol)()
    lam[1].backward()
    ref_lam = dense_eig(mesh, kappa)[0].numpy()
    ref = dense_grad(mesh, kappa[None], torch.tensor([[0.0, 1.0]], dtype=T64))[0]
    bound = 10 * tol * ref_lam[1] / gaps(ref_lam, [1])[0]                               # 10 tol lambda_2 / gap_2
    assert rel_err(kap.grad.cpu().numpy(), ref.numpy()) <= bound
    box = FEMesh.box(5, 5, 5)                       # clusters: the symmetric function sum of the first k, gap to k + 1
    kappa = field(box.n_elements, 14, B=2)
    kap = kappa.to("cuda").requires_grad_(True)
    k = 4
    es = EigenFESolver(box, kap, k, tol=tol)
    lam, _ = es()
    assert es.last_info.not_converged == 0
    lam.sum().backward()
    ref = dense_grad(box, kappa, torch.ones(2, k, dtype=T64))
    for b in range(2):
        ref_lam = dense_eig(box, kappa[b])[0].numpy()
        bound = 10 * tol * ref_lam[k - 1] / (ref_lam[k] - ref_lam[k - 1])               # 10 tol lambda_k / gap of the span
        e = rel_err(kap.grad[b].cpu().numpy(), ref[b].numpy())
        print(f"box sample {b}: gradient rel_err {e:.2e} (bound {bound:.2e})")
        assert e <= bound


@gpu
@pytest.mark.parametrize("which", ["lattice", "general"])
def test_per_sample_scalar_gradient_is_homogeneous(which):
    """kappa_b d lambda / d kappa_b = lambda (K is linear in kappa): second order in the eigenvector error."""
    mesh = lattice_mesh() if which == "lattice" else jittered(FEMesh.rectangle(14, 12, (0.0, 1.4), (0.0, 1.0)))
    from diffhe import EigenFESolver
    kap = torch.tensor([0.7, 1.0, 2.2], dtype=T64, device="cuda", requires_grad=True)
    lam, _ = EigenFESolver(mesh, kap, 3, tol=1e-11)()
    for i in range(3):
        (g,) = torch.autograd.grad(lam[:, i].sum(), kap, retain_graph=True)
        assert rel_err((kap.detach() * g).cpu().numpy(), lam[:, i].detach().cpu().numpy()) <= RTOL_GRAD
    one = torch.tensor(1.7, dtype=T64, device="cuda", requires_grad=True)          # one kappa for all: a 0-dim gradient
    lam, _ = EigenFESolver(mesh, one, 2, tol=1e-11)()
    lam[0].backward()
    assert one.grad.shape == () and abs(float(one.grad * one.detach() / lam[0].detach()) - 1.0) <= RTOL_GRAD


@gpu
def test_central_differences():
    """Directional derivatives of a weighted sum of isolated eigenvalues, step 1e-5, tolerance 1e-7."""
    from diffhe import EigenFESolver
    mesh = FEMesh.rectangle(7, 5, (0.0, 1.4), (0.0, 1.0))
    kappa = field(mesh.n_elements, 15, B=2)
    w = torch.tensor([[1.0, 0.5], [-0.3, 0.8]], dtype=T64, device="cuda")

    def value(kv):
        lam, _ = EigenFESolver(mesh, kv.to("cuda"), 2, guard=3, tol=1e-11)()
        return float((lam * w).sum())

    kap = kappa.to("cuda").requires_grad_(True)
    lam, _ = EigenFESolver(mesh, kap, 2, guard=3, tol=1e-11)()
    (lam * w).sum().backward()
    gen = torch.Generator().manual_seed(16)
    for _ in range(3):
        v = torch.randn(kappa.shape, generator=gen, dtype=T64)
        fd = (value(kappa + 1e-5 * v) - value(kappa - 1e-5 * v)) / 2e-5
        an = float((kap.grad.cpu() * v).sum())
        print("central difference", fd, "analytic", an)
        assert abs(fd - an) <= 1e-7 * max(abs(an), 1.0)


# -- the Ritz kernel alone --------------------------------------------------------------------------------------------
def pack(G):
    """(B, p, p) symmetric -> (p (p + 1) / 2, B), rows of the upper triangle."""
    p = G.shape[1]
    iu = torch.triu_indices(p, p)
    return G[:, iu[0], iu[1]].t().contiguous()


@gpu
@pytest.mark.parametrize("p", [2, 5, 8, 16])
def test_ritz_kernel_against_eigh(p):
    from diffhe import _hip
    B = 64
    gen = torch.Generator().manual_seed(100 + p)
    S = torch.randn(B, p, p, generator=gen, dtype=T64)
    T = torch.randn(B, p, p, generator=gen, dtype=T64)
    GM = torch.eye(p, dtype=T64) + 0.5 * S @ S.transpose(1, 2) / p           # cond < 10
    GA = T @ T.transpose(1, 2) + torch.eye(p, dtype=T64)
    GM[3] = GM[3] - 2.0 * torch.eye(p, dtype=T64)                            # sample 3: indefinite
    dev = "cuda"
    ga, gm = pack(GA).to(dev), pack(GM).to(dev)
    work = torch.empty(2 * p * p * B, dtype=T64, device=dev)
    C = torch.full((p, p, B), float("nan"), dtype=T64, device=dev)
    theta = torch.full((p, B), float("nan"), dtype=T64, device=dev)
    flag = torch.full((B,), -1, dtype=torch.int32, device=dev)
    L = _hip.lib()
    _hip.check(L.diffhe_eig_ritz(_hip.ptr(ga), _hip.ptr(gm), p, B, 30, _hip.ptr(work), _hip.ptr(C), _hip.ptr(theta),
                                 _hip.ptr(flag), None), "diffhe_eig_ritz")
    torch.cuda.synchronize()
    C, theta, flag = C.cpu().permute(2, 0, 1), theta.cpu().t(), flag.cpu()
    assert flag[3] == 1 and int(flag.sum()) == 1
    assert bool(torch.isfinite(C).all()) and bool(torch.isfinite(theta).all())
    worst_l = worst_r = 0.0
    for b in range(B):
        if b == 3:
            continue
        Lc = torch.linalg.cholesky(GM[b])
        W = torch.linalg.solve_triangular(Lc, GA[b], upper=False)
        At = torch.linalg.solve_triangular(Lc, W.t(), upper=False)
        ref = torch.linalg.eigvalsh(0.5 * (At + At.t()))
        worst_l = max(worst_l, float(((theta[b] - ref).abs() / ref.abs()).max()))
        res = GA[b] @ C[b] - GM[b] @ C[b] * theta[b][None, :]
        worst_r = max(worst_r, float(res.abs().max() / GA[b].abs().max()))
        assert bool((theta[b][1:] >= theta[b][:-1]).all())
    print(f"p = {p}: eigenvalues {worst_l:.2e}, residual {worst_r:.2e}")
    assert worst_l <= 1e-12 and worst_r <= 1e-12


# -- one full-size run ------------------------------------------------------------------------------------------------
@gpu
def test_full_size_lattice_against_the_closed_form():
    """rectangle(1024, 1024) x 8, k = 4, one kappa per sample: lambda_pq kappa_b; lambda_2 = lambda_3 compared as values."""
    mesh = FEMesh.rectangle(1024, 1024)
    kappa = torch.linspace(0.5, 2.25, 8, dtype=T64)
    es, lam, phi = solve(mesh, kappa, 4, layout="node")
    info = es.last_info
    print("1024^2 x 8:", info.path, "outer", info.outer_iterations, "solves", info.inner_solves, "pcg", info.inner_iterations,
          "max rho", float(info.residual.max()))
    assert info.not_converged == 0
    exact = closed_form(1024, 1024, 1.0, 1.0)[:4]
    lam = lam.cpu()
    for b in range(8):
        assert rel_err(lam[b].numpy(), float(kappa[b]) * exact) <= RTOL_U
    assert tuple(phi.shape) == (4, mesh.n_nodes, 8)
