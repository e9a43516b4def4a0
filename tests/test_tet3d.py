"""3D P1 tetrahedra: FEMesh.box, the tetrahedral element integrals, the pruned stiffness pattern, and
DifferentiableFESolver3D against a dense torch restatement of the 3D assembly (autograd through torch.linalg.solve)
and against closed-form / 2D-path solutions."""
import numpy as np
import pytest
import torch

from diffhe import FEMesh, DifferentiableFESolver
from diffhe.plan import (boundary_faces, build_ell_pattern, reference_order_integrals, _lumped_mass)
from _util import rel_err, RTOL_U, RTOL_GRAD

T64 = torch.float64
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------
# dense restatement (numpy geometry through the inverse Jacobian, torch assembly / solve for autograd)
# ------------------------------------------------------------------------------------------------
def _tet_forms(nodes, elems):
    """(k0 (m, 4, 4), m0 (m, 4, 4), vol (m)) from grad phi = rows 1..3 of inv([[1 1 1 1], [x], [y], [z]])."""
    P = nodes[elems]                                                   # (m, 4, 3)
    A = np.concatenate([np.ones((len(elems), 1, 4)), P.transpose(0, 2, 1)], axis=1)
    grads = np.linalg.inv(A)[:, :, 1:]                                 # (m, 4, 3): grad phi_p
    vol = np.abs(np.linalg.det(A)) / 6.0
    k0 = np.einsum("epd,eqd->epq", grads, grads) * vol[:, None, None]
    m0 = np.broadcast_to((vol / 16.0)[:, None, None], (len(elems), 4, 4)).copy()
    return k0, m0, vol


def _dense_solve(mesh, kappa_be, f, load=None, c=0.0):
    """u (B, n) of (K(kappa_b) + c M_L) u = M f + load on the free rows, u = g on the Dirichlet nodes; differentiable
    in kappa_be (B, m), f (B, n) and load (B, n)."""
    nodes, elems = mesh.nodes.numpy(), mesh.elements.numpy()
    n, m = mesh.n_nodes, mesh.n_elements
    k0, m0, vol = _tet_forms(nodes, elems)
    B = f.shape[0]
    idx = torch.from_numpy((elems[:, :, None] * n + elems[:, None, :]).reshape(-1))
    kv = (kappa_be[:, :, None] * torch.from_numpy(k0.reshape(m, 16))).reshape(B, -1)
    K = torch.zeros(B, n * n, dtype=T64).index_add(1, idx, kv).reshape(B, n, n)
    M = torch.zeros(n * n, dtype=T64).index_add(0, idx, torch.from_numpy(m0.reshape(-1))).reshape(n, n)
    bc = np.array(sorted(mesh.dirichlet_nodes))
    free = np.setdiff1d(np.arange(n), bc)
    g = torch.zeros(n, dtype=T64)
    g[bc] = torch.tensor([mesh.dirichlet_nodes[int(k)] for k in bc], dtype=T64)
    F = f @ M.t() - K[:, :, bc] @ g[bc]
    if load is not None:
        F = F + load
    A = K[:, free][:, :, free]
    if c:
        ml = np.zeros(n)
        np.add.at(ml, elems.reshape(-1), np.repeat(vol / 4.0, 4))
        A = A + c * torch.diag(torch.from_numpy(ml[free]))
    uf = torch.linalg.solve(A, F[:, free].unsqueeze(2)).squeeze(2)
    u = g.expand(B, n).clone()
    u[:, free] = uf
    return u


def _jittered_box(nx=4, ny=3, nz=4, seed=0, partial=True):
    """box with EVERY node jittered, renumbered at random; partial Dirichlet boundary (faces x = 0 and z = 1) with
    non-zero data g = 0.3 + x y, or none of that (partial=False keeps the box's closed boundary and zero data)."""
    base = FEMesh.box(nx, ny, nz, (0.0, 1.0), (0.0, 0.8), (0.0, 1.2))
    rng = np.random.default_rng(seed)
    X = base.nodes.numpy()
    h = np.array([1.0 / nx, 0.8 / ny, 1.2 / nz])
    nodes = X + rng.uniform(-0.15, 0.15, X.shape) * h
    n = len(nodes)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    if partial:
        bc = {int(inv[i]): 0.3 + X[i, 0] * X[i, 1] for i in range(n)
              if np.isclose(X[i, 0], 0.0) or np.isclose(X[i, 2], 1.2)}
    else:
        bc = {int(inv[k]): v for k, v in base.dirichlet_nodes.items()}
    return FEMesh(nodes=torch.from_numpy(nodes[perm]), elements=torch.from_numpy(inv[base.elements.numpy()]),
                  dirichlet_nodes=bc)


# ------------------------------------------------------------------------------------------------
# host
# ------------------------------------------------------------------------------------------------
def test_box_layout():
    nx, ny, nz = 3, 4, 5
    xr, yr, zr = (0.0, 1.3), (-0.2, 0.5), (0.1, 2.0)
    mesh = FEMesh.box(nx, ny, nz, xr, yr, zr, bc_value=0.25)
    n = (nx + 1) * (ny + 1) * (nz + 1)
    assert mesh.dim == 3 and mesh.n_nodes == n and mesh.n_elements == 6 * nx * ny * nz
    assert tuple(mesh.elements.shape) == (6 * nx * ny * nz, 4) and mesh.nodes.dtype == T64
    X, el = mesh.nodes.numpy(), mesh.elements.numpy()
    # node id (k (ny+1) + j)(nx+1) + i, x fastest
    k, rest = np.divmod(np.arange(n), (nx + 1) * (ny + 1))
    j, i = np.divmod(rest, nx + 1)
    assert np.allclose(X[:, 0], xr[0] + i * (xr[1] - xr[0]) / nx) and np.allclose(X[:, 2], zr[0] + k * (zr[1] - zr[0]) / nz)
    assert np.allclose(X[:, 1], yr[0] + j * (yr[1] - yr[0]) / ny)
    # cube 0, first tetrahedron: path x, then y, then z from the corner
    assert el[0].tolist() == [0, 1, 1 + nx + 1, 1 + nx + 1 + (nx + 1) * (ny + 1)]
    _, _, vol = _tet_forms(X, el)
    hx, hy, hz = (xr[1] - xr[0]) / nx, (yr[1] - yr[0]) / ny, (zr[1] - zr[0]) / nz
    assert np.allclose(vol, hx * hy * hz / 6.0, rtol=1e-12)
    box_vol = (xr[1] - xr[0]) * (yr[1] - yr[0]) * (zr[1] - zr[0])
    assert abs(vol.sum() - box_vol) < 1e-12 * box_vol
    assert abs(_lumped_mass(X, el).sum() - box_vol) < 1e-12 * box_vol
    # conformity: interior faces shared by exactly two tetrahedra, 4 (nx ny + ny nz + nz nx) boundary faces
    f = np.sort(np.concatenate([el[:, [1, 2, 3]], el[:, [0, 2, 3]], el[:, [0, 1, 3]], el[:, [0, 1, 2]]]), axis=1)
    _, cnt = np.unique(f, axis=0, return_counts=True)
    assert cnt.max() == 2
    nb = 4 * (nx * ny + ny * nz + nz * nx)
    assert (cnt == 1).sum() == nb and len(boundary_faces(el)) == nb
    # Dirichlet set = the boundary nodes, with bc_value
    on = ((i == 0) | (i == nx) | (j == 0) | (j == ny) | (k == 0) | (k == nz))
    assert sorted(mesh.dirichlet_nodes) == np.nonzero(on)[0].tolist()
    assert set(mesh.dirichlet_nodes.values()) == {0.25}
    assert set(np.unique(boundary_faces(el))) == set(np.nonzero(on)[0].tolist())


def test_tet_reference_order_integrals():
    rng = np.random.default_rng(1)
    nodes = rng.uniform(-1.0, 1.0, (40, 3))
    el = np.stack([rng.choice(40, 4, replace=False) for _ in range(60)])
    tn, dn = reference_order_integrals(np.ascontiguousarray(nodes.T), el.T)
    k0, _, _ = _tet_forms(nodes, el)
    got = (tn / dn).T.reshape(-1, 4, 4)
    assert np.max(np.abs(got - k0) / np.abs(k0).max(axis=(1, 2))[:, None, None]) < 1e-13
    # the degeneracy threshold is relative to the element's size: a tiny tetrahedron is kept (k0 scales with its size),
    # a flat one -- coplanar to rounding -- contributes zeros, den = 1
    base = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    flat = base.copy()
    flat[3] = [0.3, 0.3, 1e-14]
    coplanar = base.copy()
    coplanar[3] = [0.5, 0.5, 0.0]
    X = np.concatenate([base, 1e-8 * base, flat, coplanar])
    els = np.arange(16).reshape(4, 4)
    tn, dn = reference_order_integrals(np.ascontiguousarray(X.T), els.T)
    k_unit = tn[:, 0] / dn[0]
    assert np.abs(tn[:, 1]).max() > 0 and np.allclose(tn[:, 1] / dn[1], 1e-8 * k_unit, rtol=1e-12)
    for c in (2, 3):
        assert np.all(tn[:, c] == 0.0) and dn[c] == 1.0
    assert _lumped_mass(X, els)[8:].sum() == 0.0


def test_tet_pattern_pruning():
    mesh = FEMesh.box(5, 4, 3, (0.0, 1.0), (0.0, 0.7), (0.0, 1.9))
    el, n = mesh.elements.numpy(), mesh.n_nodes
    tn, _ = reference_order_integrals(np.ascontiguousarray(mesh.nodes.numpy().T), el.T)
    full = build_ell_pattern(el, n)
    pruned = build_ell_pattern(el, n, zero=(tn == 0.0))
    assert full["W"] == 15 and pruned["W"] == 7 and full["pruned"] == 0 and pruned["pruned"] > 0
    # the dropped entries are exact zeros of every contribution (not tiny values); every kept coupling is an axis neighbour
    zero_c = (tn == 0.0)
    dropped = pruned["slot_of"] < 0
    assert np.all(zero_c[dropped]) and not np.any(dropped[[0, 5, 10, 15]])
    X = mesh.nodes.numpy()
    cols = pruned["cols"]
    for k in range(1, 7):
        used = cols[k] != np.arange(n)
        d = np.abs(X[cols[k][used]] - X[used])
        assert np.all((d > 1e-12).sum(axis=1) == 1)       # exactly one coordinate differs
    # on a jittered, renumbered box nothing is an exact zero: pruning removes nothing
    jm = _jittered_box(4, 4, 4, seed=2, partial=False)
    tn2, _ = reference_order_integrals(np.ascontiguousarray(jm.nodes.numpy().T), jm.elements.numpy().T)
    p2 = build_ell_pattern(jm.elements.numpy(), jm.n_nodes, zero=(tn2 == 0.0))
    p2full = build_ell_pattern(jm.elements.numpy(), jm.n_nodes)
    assert p2["pruned"] == 0 and p2["W"] == p2full["W"] and np.array_equal(p2["cols"], p2full["cols"])
    assert np.array_equal(p2["slot_of"], p2full["slot_of"])


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
def _kappa_be(kappa, B, m):
    if kappa.numel() == 1:
        return kappa.reshape(1, 1).expand(B, m)
    if kappa.dim() == 1 and kappa.shape[0] == m:
        return kappa.reshape(1, m).expand(B, m)
    if kappa.dim() == 1:
        return kappa.reshape(B, 1).expand(B, m)
    return kappa


@pytest.mark.gpu
@pytest.mark.parametrize("layout_k", ["scalar", "sample", "elem", "sample_elem"])
def test_dense_parity(layout_k):
    from diffhe.tet3d import DifferentiableFESolver3D
    mesh = _jittered_box()
    n, m, B = mesh.n_nodes, mesh.n_elements, 3
    rng = np.random.default_rng(5)
    k_np = {"scalar": np.array(1.3), "sample": rng.uniform(0.5, 2.0, B), "elem": rng.uniform(0.5, 2.0, m),
            "sample_elem": rng.uniform(0.5, 2.0, (B, m))}[layout_k]
    f0 = torch.from_numpy(rng.standard_normal((B, n)) + 1.0)
    w = torch.from_numpy(rng.standard_normal((B, n)))

    def loss(u):
        return (w * u).sum() + 0.5 * (u ** 2).sum()

    kd = torch.tensor(k_np, dtype=T64, device=DEV, requires_grad=True)
    fd = f0.clone().to(DEV).requires_grad_(True)
    solver = DifferentiableFESolver3D(mesh, kd, device=DEV)
    u = solver(fd)
    loss(u.cpu()).backward()
    assert solver.last_info.path.startswith("ell-") and solver.last_info.not_converged == 0
    kc = torch.tensor(k_np, dtype=T64, requires_grad=True)
    fc = f0.clone().requires_grad_(True)
    uo = _dense_solve(mesh, _kappa_be(kc, B, m), fc)
    loss(uo).backward()
    assert rel_err(u.detach().cpu().numpy(), uo.detach().numpy()) < RTOL_U
    assert rel_err(kd.grad.cpu().numpy(), kc.grad.numpy()) < RTOL_GRAD
    assert rel_err(fd.grad.cpu().numpy(), fc.grad.numpy()) < RTOL_GRAD
    # layout="node": (n, B) in and out, same solution
    un = DifferentiableFESolver3D(mesh, kd.detach(), device=DEV)(f0.t().contiguous().to(DEV), layout="node")
    assert rel_err(un.t().cpu().numpy(), uo.detach().numpy()) < RTOL_U


@pytest.mark.gpu
def test_load_and_reaction():
    from diffhe.tet3d import DifferentiableFESolver3D
    mesh = _jittered_box(seed=7)
    n, m, B, c = mesh.n_nodes, mesh.n_elements, 2, 3.5
    rng = np.random.default_rng(8)
    k_np = rng.uniform(0.5, 2.0, (B, m))
    f0 = torch.from_numpy(rng.standard_normal((B, n)))
    l0 = torch.from_numpy(0.01 * rng.standard_normal((B, n)))
    kd = torch.tensor(k_np, device=DEV, requires_grad=True)
    fd, ld = f0.to(DEV).requires_grad_(True), l0.to(DEV).requires_grad_(True)
    solver = DifferentiableFESolver3D(mesh, kd, device=DEV, reaction=c)
    u = solver(fd, load=ld)
    (u.cpu() ** 2).sum().backward()
    kc = torch.tensor(k_np, requires_grad=True)
    fc, lc = f0.clone().requires_grad_(True), l0.clone().requires_grad_(True)
    uo = _dense_solve(mesh, kc, fc, load=lc, c=c)
    (uo ** 2).sum().backward()
    assert rel_err(u.detach().cpu().numpy(), uo.detach().numpy()) < RTOL_U
    for a, b in ((kd, kc), (fd, fc), (ld, lc)):
        assert rel_err(a.grad.cpu().numpy(), b.grad.numpy()) < RTOL_GRAD


@pytest.mark.gpu
def test_assembled_operator_bitwise():
    """The stored ELL values of the reference-order gather on tetrahedra (what operator='assembled' and every per-sample
    kappa use) equal a numpy restatement of its operation order bit for bit: per entry, (kappa t) / den summed in
    element order, Dirichlet rows -> identity rows, Dirichlet columns -> 0.  On the pruned box pattern and a jittered mesh."""
    from diffhe import _hip
    from diffhe.plan import get_plan, _stream
    from diffhe.tet3d import DifferentiableFESolver3D
    for mesh in (FEMesh.box(4, 3, 5, (0.0, 1.0), (0.0, 0.6), (0.0, 1.7)), _jittered_box(seed=11)):
        n, m, Bv = mesh.n_nodes, mesh.n_elements, 2
        rng = np.random.default_rng(3)
        kap = rng.uniform(0.5, 2.0, (m, Bv))
        plan = get_plan(mesh, torch.device(DEV))
        plan.ensure_ell()
        W = plan.W
        vals = torch.empty((W, n, Bv), dtype=T64, device=DEV)
        lift = torch.empty((n, Bv), dtype=T64, device=DEV)
        kd = torch.from_numpy(kap).to(DEV)
        L = _hip.lib()
        _hip.check(L.diffhe_ell_assemble_rows_ref(_hip.ptr(plan.tnum), _hip.ptr(plan.den), _hip.ptr(kd), Bv, 1,
                                                  _hip.ptr(plan.ent_ptr), _hip.ptr(plan.contrib), _hip.ptr(plan.cols), None,
                                                  _hip.ptr(plan.is_bc), _hip.ptr(plan.g), _hip.ptr(vals), _hip.ptr(lift),
                                                  n, m, W, Bv, _stream(torch.device(DEV))), "assemble_rows_ref")
        got, cols = vals.cpu().numpy(), plan.cols.cpu().numpy()
        # restatement
        el = mesh.elements.numpy()
        tn, dn = reference_order_integrals(np.ascontiguousarray(mesh.nodes.numpy().T), el.T)
        e_idx = np.repeat(np.arange(m), 16)
        pq = np.tile(np.arange(16), m)
        r, c = el[e_idx, pq // 4], el[e_idx, pq % 4]
        order = np.lexsort((pq, e_idx, c, r))                    # per (row, col): element order, then local entry
        r, c, e_s, pq_s = r[order], c[order], e_idx[order], pq[order]
        key = r * n + c
        first = np.r_[True, key[1:] != key[:-1]]
        ent = np.cumsum(first) - 1
        pos = np.arange(len(key)) - np.flatnonzero(first)[ent]
        ukey = key[first]
        for b in range(Bv):
            term = (kap[e_s, b] * tn[pq_s, e_s]) / dn[e_s]
            v = np.zeros(len(ukey))
            for p_ in range(pos.max() + 1):
                sel = pos == p_
                v[ent[sel]] = v[ent[sel]] + term[sel]
            is_bc = plan.is_bc.cpu().numpy().astype(bool)
            ur, uc = ukey // n, ukey % n
            v = np.where(is_bc[ur], np.where(ur == uc, 1.0, 0.0), np.where(is_bc[uc] & (ur != uc), 0.0, v))
            want = dict(zip(ukey.tolist(), v.tolist()))
            for k in range(W):
                for i in range(n):
                    j = int(cols[k, i])
                    exp = want.get(i * n + j, 0.0) if (k == 0 or j != i) else 0.0
                    assert np.float64(got[k, i, b]).tobytes() == np.float64(exp).tobytes(), (k, i, b)
            # entries missing from the (pruned) pattern are exact zeros
            stored = set((np.arange(n)[None, :] * n + cols).reshape(-1).tolist())
            assert all(val == 0.0 for kk, val in want.items() if kk not in stored)
        # and the solver with operator="assembled" solves that operator
        f0 = torch.ones(Bv, n, dtype=T64)
        ks = torch.tensor([0.8, 1.6], dtype=T64)
        u = DifferentiableFESolver3D(mesh, ks.to(DEV), device=DEV, operator="assembled")(f0.to(DEV))
        uo = _dense_solve(mesh, _kappa_be(ks, Bv, m), f0)
        assert rel_err(u.cpu().numpy(), uo.numpy()) < RTOL_U


@pytest.mark.gpu
def test_extrusion_matches_2d_lattice():
    from diffhe.tet3d import DifferentiableFESolver3D
    nx, ny, nz = 12, 10, 5
    box = FEMesh.box(nx, ny, nz, (0.0, 1.0), (0.0, 1.0), (0.0, 0.5))
    X = box.nodes.numpy()
    side = (np.isclose(X[:, 0], 0.0) | np.isclose(X[:, 0], 1.0) | np.isclose(X[:, 1], 0.0) | np.isclose(X[:, 1], 1.0))
    mesh = FEMesh(nodes=box.nodes, elements=box.elements, dirichlet_nodes=dict.fromkeys(np.nonzero(side)[0].tolist(), 0.0))
    s3 = DifferentiableFESolver3D(mesh, 1.7, device=DEV)
    u3 = s3(torch.ones(mesh.n_nodes, dtype=T64, device=DEV)).cpu().numpy().reshape(nz + 1, ny + 1, nx + 1)
    rect = FEMesh.rectangle(nx, ny)
    s2 = DifferentiableFESolver(rect, 1.7, device=DEV)
    u2 = s2(torch.ones(rect.n_nodes, dtype=T64, device=DEV)).cpu().numpy().reshape(ny + 1, nx + 1)
    assert s2.last_info.path.startswith("lattice-")
    for k in range(nz + 1):
        assert rel_err(u3[k], u2) < 1e-10, k


def _dst_box_solution(N, kappas):
    """Exact solution of kappa_b * h (6 I - axis neighbours) u = h^3 on the (N-1)^3 interior grid of the unit cube, zero
    on the boundary: the Kuhn-tetrahedra system of FEMesh.box(N, N, N) with f = 1 (7-point, couplings -h)."""
    k = np.arange(1, N)
    S = np.sin(np.pi * np.outer(k, k) / N)                               # S S = N/2 I
    lam = 4.0 * np.sin(k * np.pi / (2 * N)) ** 2
    h = 1.0 / N
    s1 = S @ np.ones(N - 1)
    rhs_hat = h * h * s1[:, None, None] * s1[None, :, None] * s1[None, None, :]
    den = lam[:, None, None] + lam[None, :, None] + lam[None, None, :]
    scale = (2.0 / N) ** 3
    out = []
    for kap in kappas:
        uh = rhs_hat / (kap * den)
        u = scale * np.einsum("ia,jb,kc,abc->ijk", S, S, S, uh, optimize=True)
        full = np.zeros((N + 1, N + 1, N + 1))
        full[1:-1, 1:-1, 1:-1] = u                                        # axes (x, y, z); node arrays are (z, y, x)
        out.append(full.transpose(2, 1, 0).reshape(-1))
    return np.stack(out)


@pytest.mark.gpu
def test_box_40_cubed_batch_64_against_dst():
    from diffhe.tet3d import DifferentiableFESolver3D
    N, B = 40, 64
    mesh = FEMesh.box(N, N, N)
    kap = np.random.default_rng(4).uniform(0.5, 2.0, B)
    solver = DifferentiableFESolver3D(mesh, torch.from_numpy(kap).to(DEV), device=DEV)
    u = solver(torch.ones(B, mesh.n_nodes, dtype=T64, device=DEV)).cpu().numpy()
    assert solver.last_info.factored and solver.last_info.not_converged == 0
    assert solver._plan().W == 7
    ref = _dst_box_solution(N, kap)
    for b in range(B):
        assert rel_err(u[b], ref[b]) < 1e-10, b


@pytest.mark.gpu
def test_second_order_convergence():
    from diffhe.tet3d import DifferentiableFESolver3D
    errs = []
    for N in (8, 16, 32):
        mesh = FEMesh.box(N, N, N)
        X = mesh.nodes.numpy()
        ue = np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]) * np.sin(np.pi * X[:, 2])
        f = torch.from_numpy(3 * np.pi ** 2 * ue).to(DEV)
        u = DifferentiableFESolver3D(mesh, 1.0, device=DEV)(f).cpu().numpy()
        errs.append(np.abs(u - ue).max())
    assert errs[0] / errs[1] >= 3.5 and errs[1] / errs[2] >= 3.5, errs


@pytest.mark.gpu
def test_hessian_vector_product():
    from diffhe.tet3d import DifferentiableFESolver3D
    mesh = _jittered_box(3, 3, 3, seed=13)
    n, m = mesh.n_nodes, mesh.n_elements
    rng = np.random.default_rng(14)
    k_np = rng.uniform(0.5, 2.0, m)
    f0 = torch.from_numpy(rng.standard_normal(n) + 1.0)
    v = torch.from_numpy(rng.standard_normal(m))

    def hvp(kappa, u_of):
        u = u_of(kappa)
        (g,) = torch.autograd.grad((u ** 2).sum(), kappa, create_graph=True)
        (h,) = torch.autograd.grad((g * v.to(g.device)).sum(), kappa)
        return g.detach().cpu().numpy(), h.cpu().numpy()

    kd = torch.tensor(k_np, device=DEV, requires_grad=True)
    solver = DifferentiableFESolver3D(mesh, kd, device=DEV)
    g_gpu, h_gpu = hvp(kd, lambda k: solver(f0.to(DEV)))
    kc = torch.tensor(k_np, requires_grad=True)
    g_ref, h_ref = hvp(kc, lambda k: _dense_solve(mesh, k.reshape(1, m), f0.reshape(1, n))[0])
    assert rel_err(g_gpu, g_ref) < RTOL_GRAD
    assert rel_err(h_gpu, h_ref) < 1e-9


@pytest.mark.gpu
def test_determinism():
    from diffhe.tet3d import DifferentiableFESolver3D
    rng = np.random.default_rng(21)
    box = FEMesh.box(10, 9, 8)
    cases = [(box, torch.from_numpy(rng.uniform(0.5, 2.0, 8)), True),                 # factored route (closed box)
             (box, torch.from_numpy(rng.uniform(0.5, 2.0, (8, box.n_elements))), False),
             (_jittered_box(6, 5, 6, seed=22), torch.from_numpy(rng.uniform(0.5, 2.0, 8)), False)]
    for mesh, k0, factored in cases:
        f0 = torch.from_numpy(rng.standard_normal((8, mesh.n_nodes)))
        outs = []
        for _ in range(2):
            k = k0.clone().to(DEV).requires_grad_(True)
            f = f0.clone().to(DEV).requires_grad_(True)
            s = DifferentiableFESolver3D(mesh, k, device=DEV)
            u = s(f)
            (u ** 2).sum().backward()
            assert s.last_info.factored == factored
            outs.append([t.detach().cpu().numpy() for t in (u, k.grad, f.grad)])
        for a, b in zip(*outs):
            assert a.tobytes() == b.tobytes()
