"""Linear elasticity (diffhe.elastic.ElasticFESolver, csrc/elastic.hip, include/diffhe_elastic.h).

The oracle is a dense torch restatement in STRAIN-DISPLACEMENT form, K_e = vol_e E_e B^T D B with the Voigt matrix D,
Dirichlet elimination and `torch.linalg.solve`, gradients by autograd -- deliberately another formulation than the
kernel's index formula.  The CPU tests pin that restatement to closed forms (rigid-body modes, patch test, uniaxial
tension) and check the host logic (fixed=, the dof pattern, the block hierarchy, the second signature table); the GPU
tests hold the kernels and the solver against it."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from diffhe import FEMesh, _hip
from diffhe import amg as amg_mod
from diffhe import elastic
from diffhe.plan import build_ell_pattern
from _util import GOLDEN, RTOL_GRAD, RTOL_U, rel_err

T64 = torch.float64
DEV = "cuda:0"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffhe_elastic.h")


# ------------------------------------------------------------------------------------------------
# dense restatement (independent of the product code)
# ------------------------------------------------------------------------------------------------
def _geometry(X, el):
    """grad phi (m, npe, d) and element size (m) of P1 triangles / tetrahedra."""
    P = X[el]
    if X.shape[1] == 2:
        x, y = P[..., 0], P[..., 1]
        det = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
        b = torch.stack([y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]], 1)
        c = torch.stack([x[:, 2] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 0]], 1)
        return torch.stack([b, c], 2) / det[:, None, None], 0.5 * det.abs()
    a, b, c = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], P[:, 3] - P[:, 0]
    g1, g2, g3 = torch.cross(b, c, dim=1), torch.cross(c, a, dim=1), torch.cross(a, b, dim=1)
    det = (a * g1).sum(1)
    return torch.stack([-(g1 + g2 + g3), g1, g2, g3], 1) / det[:, None, None], det.abs() / 6.0


def _voigt_D(nu, d, plane):
    """The Voigt matrix of E = 1 (engineering shear strains)."""
    if d == 2 and plane == "stress":
        return torch.tensor([[1, nu, 0], [nu, 1, 0], [0, 0, (1 - nu) / 2]], dtype=T64) / (1 - nu * nu)
    if d == 2:
        return torch.tensor([[1 - nu, nu, 0], [nu, 1 - nu, 0], [0, 0, (1 - 2 * nu) / 2]], dtype=T64) / ((1 + nu) * (1 - 2 * nu))
    lam, mu = nu / ((1 + nu) * (1 - 2 * nu)), 1 / (2 * (1 + nu))
    D = torch.zeros(6, 6, dtype=T64)
    D[:3, :3] = lam
    D[:3, :3] += 2 * mu * torch.eye(3, dtype=T64)
    D[3:, 3:] = mu * torch.eye(3, dtype=T64)
    return D


def _strain_matrix(G):
    """B (m, nv, npe*d): Voigt strains (xx, yy, xy | xx, yy, zz, yz, xz, xy) from the element's dofs p*d + a."""
    m, npe, d = G.shape
    Bm = torch.zeros(m, 3 if d == 2 else 6, npe * d, dtype=T64)
    for p in range(npe):
        for a in range(d):
            Bm[:, a, p * d + a] = G[:, p, a]
        if d == 2:
            Bm[:, 2, p * 2], Bm[:, 2, p * 2 + 1] = G[:, p, 1], G[:, p, 0]
        else:
            Bm[:, 3, p * 3 + 1], Bm[:, 3, p * 3 + 2] = G[:, p, 2], G[:, p, 1]
            Bm[:, 4, p * 3], Bm[:, 4, p * 3 + 2] = G[:, p, 2], G[:, p, 0]
            Bm[:, 5, p * 3], Bm[:, 5, p * 3 + 1] = G[:, p, 1], G[:, p, 0]
    return Bm


def _dense_K(mesh, E_bm, nu, plane):
    """(B, n d, n d) raw stiffness, no Dirichlet data; differentiable in E_bm (B, m)."""
    X, el = mesh.nodes.to(T64), mesh.elements.long()
    n, d = X.shape
    m, npe = el.shape
    G, vol = _geometry(X, el)
    Bm = _strain_matrix(G)
    k0 = vol[:, None, None] * (Bm.transpose(1, 2) @ _voigt_D(nu, d, plane) @ Bm)           # (m, npe d, npe d)
    dof = (el[:, :, None] * d + torch.arange(d)[None, None, :]).reshape(m, npe * d)
    idx = (dof[:, :, None] * (n * d) + dof[:, None, :]).reshape(-1)
    ke = E_bm[:, :, None, None] * k0[None]
    return torch.zeros(E_bm.shape[0], (n * d) ** 2, dtype=T64).index_add(1, idx, ke.reshape(E_bm.shape[0], -1)).reshape(
        E_bm.shape[0], n * d, n * d)


def _load_map(mesh):
    """(n, n) load matrix of the scalar solvers: F_p = |e| / (d + 1) * mean f."""
    X, el = mesh.nodes.to(T64), mesh.elements.long()
    n, npe = X.shape[0], el.shape[1]
    _, vol = _geometry(X, el)
    idx = (el[:, :, None] * n + el[:, None, :]).reshape(-1)
    m0 = (vol / npe ** 2)[:, None].expand(-1, npe * npe).reshape(-1)
    return torch.zeros(n * n, dtype=T64).index_add(0, idx, m0).reshape(n, n)


def _fixed_arrays(mesh, fixed):
    nd = mesh.n_nodes * mesh.dim
    idx = np.array(sorted(node * mesh.dim + comp for node, comp in fixed), dtype=np.int64)
    g = torch.zeros(nd, dtype=T64)
    for (node, comp), v in fixed.items():
        g[node * mesh.dim + comp] = float(v)
    return idx, np.setdiff1d(np.arange(nd), idx), g


def _dense_solve(mesh, E_bm, nu, plane, fixed, f=None, load=None):
    """u (B, n, d): K(E_b) u = M f + load on the free dofs, u = g on the fixed ones."""
    n, d = mesh.n_nodes, mesh.dim
    B = E_bm.shape[0]
    K = _dense_K(mesh, E_bm, nu, plane)
    bc, free, g = _fixed_arrays(mesh, fixed)
    F = torch.zeros(B, n * d, dtype=T64)
    if f is not None:
        F = F + torch.einsum("ij,bja->bia", _load_map(mesh), f.expand(B, n, d)).reshape(B, n * d)
    if load is not None:
        F = F + load.expand(B, n, d).reshape(B, n * d)
    F = F - K[:, :, bc] @ g[bc]
    uf = torch.linalg.solve(K[:, free][:, :, free], F[:, free].unsqueeze(2)).squeeze(2)
    u = g.expand(B, n * d).clone()
    u[:, free] = uf
    return u.reshape(B, n, d)


# ------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------
def _jitter(mesh, seed, amount=0.15):
    """The mesh with every node moved by up to `amount` of the smallest grid step; no Dirichlet nodes."""
    X = mesh.nodes.to(T64).clone()
    h = min(float(torch.unique(X[:, a]).diff().min()) for a in range(X.shape[1]))
    gen = torch.Generator().manual_seed(seed)
    X += amount * h * (2 * torch.rand(X.shape, generator=gen, dtype=T64) - 1)
    return FEMesh(nodes=X, elements=mesh.elements, dirichlet_nodes={})


def _rect(nx, ny, seed=0, **kw):
    return _jitter(FEMesh.rectangle(nx, ny, **kw), seed)


def _box(nx, ny, nz, seed=0):
    return _jitter(FEMesh.box(nx, ny, nz), seed)


def _boundary_nodes(mesh):
    return sorted(set(mesh.boundary_facets().reshape(-1).tolist()))


def _left_nodes(nx, ny):
    return [r * (nx + 1) for r in range(ny + 1)]


def _rand(shape, seed, lo=0.0, hi=1.0):
    return lo + (hi - lo) * torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=T64)


# ------------------------------------------------------------------------------------------------
# CPU: the restatement against closed forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,plane", [(_rect(3, 2), "stress"), (_rect(3, 2), "strain"), (_box(2, 2, 2), None)],
                         ids=["2d-stress", "2d-strain", "3d"])
def test_raw_stiffness_annihilates_the_rigid_body_modes(mesh, plane):
    X, (n, d) = mesh.nodes, mesh.nodes.shape
    K = _dense_K(mesh, _rand((1, mesh.n_elements), 1, 0.5, 2.0), 0.3, plane)[0]
    modes = [torch.eye(d, dtype=T64)[a].expand(n, d) for a in range(d)]
    for a in range(d):
        for b in range(a + 1, d):           # infinitesimal rotation in the (a, b) plane
            r = torch.zeros(n, d, dtype=T64)
            r[:, a], r[:, b] = -X[:, b], X[:, a]
            modes.append(r)
    assert len(modes) == d + d * (d - 1) // 2
    bound = 1e-13 * float(K.abs().max()) * float(X.abs().max())
    for r in modes:
        assert float((K @ r.reshape(-1)).abs().max()) <= bound


@pytest.mark.parametrize("mesh,plane", [(_rect(4, 3), "stress"), (_rect(4, 3), "strain"), (_box(3, 3, 3), None)],
                         ids=["2d-stress", "2d-strain", "3d"])
def test_patch_test_reproduces_a_linear_displacement(mesh, plane):
    """u = A x + c on every boundary dof, f = 0: the interior dofs reproduce it.  E is one random positive value for the
    mesh: a constant strain is in equilibrium only where the stress E_e D eps does not jump between elements, so a
    heterogeneous field has no linear solution to reproduce (with one, the interior misses A x + c by 3.5 %)."""
    X, (n, d) = mesh.nodes, mesh.nodes.shape
    A, c = _rand((d, d), 2, -1, 1), _rand((d,), 3, -1, 1)
    exact = X @ A.t() + c
    bnodes = _boundary_nodes(mesh)
    assert n - len(bnodes) == (6 if d == 2 else 8)
    fixed = {(i, a): float(exact[i, a]) for i in bnodes for a in range(d)}
    u = _dense_solve(mesh, _rand((1, 1), 4, 0.5, 2.0).expand(1, mesh.n_elements), 0.3, plane, fixed)[0]
    assert float((u - exact).abs().max()) <= 1e-12 * float(exact.abs().max())


@pytest.mark.parametrize("plane", ["stress", "strain"])
def test_uniaxial_tension_closed_form(plane):
    nx, ny, E, nu, sigma = 4, 3, 2.5, 0.3, 0.7
    mesh = FEMesh.rectangle(nx, ny, x_range=(0.0, 2.0))
    mesh = FEMesh(nodes=mesh.nodes, elements=mesh.elements, dirichlet_nodes={})
    X, n = mesh.nodes, mesh.n_nodes
    fixed = {(i, 0): 0.0 for i in range(n) if X[i, 0] == 0.0}
    fixed.update({(i, 1): 0.0 for i in range(n) if X[i, 1] == 0.0})
    load = torch.zeros(n, 2, dtype=T64)
    right = [r * (nx + 1) + nx for r in range(ny + 1)]
    for a, b in zip(right[:-1], right[1:]):                     # sigma * (edge length) / 2 per edge end
        half = 0.5 * sigma * float(X[b, 1] - X[a, 1])
        load[a, 0] += half
        load[b, 0] += half
    u = _dense_solve(mesh, torch.full((1, mesh.n_elements), E, dtype=T64), nu, plane, fixed, load=load)[0]
    if plane == "stress":
        exact = torch.stack([sigma * X[:, 0] / E, -nu * sigma * X[:, 1] / E], 1)
    else:
        exact = torch.stack([sigma * (1 - nu * nu) * X[:, 0] / E, -nu * (1 + nu) * sigma * X[:, 1] / E], 1)
    assert float((u - exact).abs().max()) <= 1e-12 * float(exact.abs().max())


def test_lame_numbers_match_the_voigt_matrix():
    for d, plane in ((2, "stress"), (2, "strain"), (3, None)):
        lam, mu = elastic.lame_unit(0.3, d, plane)
        D = _voigt_D(0.3, d, plane)
        assert abs(float(D[0, 1]) - lam) <= 1e-15 and abs(float(D[-1, -1]) - mu) <= 1e-15
        assert abs(float(D[0, 0]) - (lam + 2 * mu)) <= 1e-15
    for bad in (-1.0, 0.5, 0.7, float("nan")):
        with pytest.raises(ValueError, match="nu"):
            elastic.lame_unit(bad, 3)
    with pytest.raises(ValueError, match="plane"):
        elastic.lame_unit(0.3, 2, "membrane")


# ------------------------------------------------------------------------------------------------
# CPU: host logic
# ------------------------------------------------------------------------------------------------
def test_fixed_parsing():
    mesh = FEMesh.rectangle(3, 2)
    is_bc, g = elastic.parse_fixed(mesh)
    assert is_bc.dtype == np.uint8 and is_bc.shape == (24,) and not g.any()
    assert sorted(np.nonzero(is_bc.reshape(12, 2).all(1))[0].tolist()) == sorted(mesh.dirichlet_nodes)
    assert int(is_bc.sum()) == 2 * len(mesh.dirichlet_nodes)
    is_bc, g = elastic.parse_fixed(mesh, {(0, 0): 0.0, (0, 1): 0.0, (5, 1): 0.25})
    assert np.nonzero(is_bc)[0].tolist() == [0, 1, 11] and g[11] == 0.25 and g.sum() == 0.25
    with pytest.raises(ValueError, match="fixed="):
        elastic.parse_fixed(FEMesh.rectangle(3, 2, bc_value=1.0))
    with pytest.raises(ValueError, match="component 2"):
        elastic.parse_fixed(mesh, {(0, 2): 0.0})
    with pytest.raises(ValueError, match="component -1"):
        elastic.parse_fixed(mesh, {(0, -1): 0.0})
    with pytest.raises(ValueError, match="node 12"):
        elastic.parse_fixed(mesh, {(12, 0): 0.0})
    with pytest.raises(ValueError, match="pairs"):
        elastic.parse_fixed(mesh, {3: 0.0})
    with pytest.raises(ValueError, match="mapping"):
        elastic.parse_fixed(mesh, [(0, 0)])


def _eliminated(K, bc):
    """Dirichlet elimination of a dense matrix as the assembly kernels do it: identity rows, zeroed columns."""
    A = K.clone()
    A[bc, :] = 0.0
    A[:, bc] = 0.0
    A[bc, bc] = 1.0
    return A


def _through_pattern(A, cols):
    """(W, n) ELL values of the dense A in the pattern `cols`: unused slots (k > 0 pointing at the row) hold 0."""
    W, n = cols.shape
    rows = np.arange(n)[None, :].repeat(W, 0)
    vals = A.numpy()[rows, cols]
    vals[(np.arange(W)[:, None] > 0) & (cols == rows)] = 0.0
    return vals


@pytest.mark.parametrize("mesh", [_rect(4, 3), _box(2, 2, 2)], ids=["2d", "3d"])
def test_dof_pattern_holds_every_coupling(mesh):
    n, d = mesh.nodes.shape
    node_cols = build_ell_pattern(mesh.elements.numpy(), n)["cols"]
    cols = elastic.dof_pattern(node_cols, d)
    W = node_cols.shape[0]
    assert cols.shape == (d * W, n * d) and cols.dtype == np.int32
    rows = np.arange(n * d)
    assert np.array_equal(cols[0], rows)                                           # slot 0 is the diagonal
    for r in rows:
        real = [int(c) for k, c in enumerate(cols[:, r]) if k == 0 or c != r]
        assert len(real) == len(set(real))                                         # no column twice
        # the padding points at the row itself: every slot of an unused node slot does
        for k in range(1, W):
            if node_cols[k, r // d] == r // d:
                assert (cols[k * d:(k + 1) * d, r] == r).all()
    K = _dense_K(mesh, torch.ones(1, mesh.n_elements, dtype=T64), 0.3, "stress" if d == 2 else None)[0]
    have = np.zeros((n * d, n * d), dtype=bool)
    have[rows[None, :].repeat(d * W, 0), cols] = True
    assert not (K.numpy() != 0.0)[~have].any()                                     # every coupling of the dense K has a slot
    assert np.allclose(_through_pattern(K, cols).sum(0), K.numpy().sum(1), atol=1e-12 * float(K.abs().max()))


@pytest.mark.parametrize("case", ["2d", "3d"])
def test_no_aggregate_mixes_components(case):
    if case == "2d":
        mesh, nx, ny = _rect(14, 10), 14, 10
        fixed = {(i, a): 0.0 for i in _left_nodes(nx, ny) for a in range(2)}
        fixed[(nx, 1)] = 0.0                                                       # a roller: one component of a node
        plane = "stress"
    else:
        mesh = _box(4, 4, 3)
        fixed = {(i, a): 0.0 for i in range(mesh.n_nodes) if i % 5 == 0 for a in range(3)}
        plane = None
    n, d = mesh.nodes.shape
    cols = elastic.dof_pattern(build_ell_pattern(mesh.elements.numpy(), n)["cols"], d)
    bc, _, _ = _fixed_arrays(mesh, fixed)
    is_bc = np.zeros(n * d, dtype=np.uint8)
    is_bc[bc] = 1
    K = _dense_K(mesh, torch.ones(1, mesh.n_elements, dtype=T64), 0.3, plane)[0]
    levels = amg_mod.build_hierarchy_blocks(cols, _through_pattern(_eliminated(K, bc), cols), is_bc, d, min_coarse=16)
    assert len(levels) >= 2
    comp, node, n_fine = np.arange(n * d) % d, np.arange(n * d) // d, n * d
    for lv in levels:
        agg = lv["agg"]
        assert agg.shape == (n_fine,) and lv["n"] == int(agg.max()) + 1 == len(lv["comp"])
        members = agg >= 0
        assert np.array_equal(lv["comp"][agg[members]], comp[members])             # one component per aggregate
        assert len(np.unique(agg[members])) == lv["n"]                             # no empty coarse dof
        first = {}                                                                 # node aggregates: a node's dofs share the coarse node
        for i in np.nonzero(members)[0]:
            assert first.setdefault(int(node[i]), int(lv["node"][agg[i]])) == int(lv["node"][agg[i]])
        assert np.array_equal(lv["cols"][0], np.arange(lv["n"]))
        assert lv["lam"] > 0 and lv["lam_parent"] > 0
        comp, node, n_fine = lv["comp"], lv["node"], lv["n"]
    if case == "2d":
        assert (levels[0]["agg"][bc] == -1).all() and levels[0]["agg"][nx * 2] >= 0   # the roller's free component stays


def _scalar_unit_operator(nx, ny):
    """ELL pattern and unit-kappa values of the eliminated scalar P1 operator on FEMesh.rectangle(nx, ny): elementwise
    numpy only (no BLAS), so the arrays -- and the hierarchy built from them -- are reproducible bit for bit."""
    mesh = FEMesh.rectangle(nx, ny)
    X, el = mesh.nodes.numpy(), mesh.elements.numpy()
    n = len(X)
    x, y = X[el][..., 0], X[el][..., 1]
    b = np.stack([y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]], 1)
    c = np.stack([x[:, 2] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 0]], 1)
    area = 0.5 * np.abs(b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
    ke = (b[:, :, None] * b[:, None, :] + c[:, :, None] * c[:, None, :]) / (4.0 * area)[:, None, None]
    K = np.zeros((n, n))
    np.add.at(K, (el[:, :, None].repeat(3, 2), el[:, None, :].repeat(3, 1)), ke)
    is_bc = np.zeros(n, dtype=bool)
    is_bc[list(mesh.dirichlet_nodes)] = True
    K[is_bc, :] = 0.0
    K[:, is_bc] = 0.0
    K[is_bc, is_bc] = 1.0
    cols = build_ell_pattern(el, n)["cols"]
    return cols, _through_pattern(torch.from_numpy(K), cols), is_bc


_SA_KEYS = ("cols", "ent_ptr", "contrib", "weights", "agg", "agg_ptr", "agg_members", "agg_weights", "p_cols", "p_vals")


def test_scalar_hierarchies_are_unchanged():
    """`build_hierarchy_sa` on rectangle(12, 9) against the arrays it gave before diffhe.amg learnt about vector-valued
    unknowns (tests/golden/amg_sa_rectangle_12x9.npz), bitwise."""
    cols, vals, is_bc = _scalar_unit_operator(12, 9)
    levels = amg_mod.build_hierarchy_sa(cols, vals, is_bc)
    with np.load(os.path.join(GOLDEN, "amg_sa_rectangle_12x9.npz"), allow_pickle=False) as z:
        assert int(z["n_levels"]) == len(levels) >= 1
        for li, lv in enumerate(levels):
            assert (int(z[f"l{li}_n"]), int(z[f"l{li}_W"])) == (lv["n"], lv["W"])
            for key in _SA_KEYS:
                want, got = z[f"l{li}_{key}"], np.asarray(lv[key])
                assert want.dtype == got.dtype and want.shape == got.shape and want.tobytes() == got.tobytes(), (li, key)
    assert "lam" not in levels[0] and "node" not in levels[0]


BY_VALUE = {"int": _hip._I, "long long": _hip._L, "double": _hip._D}


def _declarations(header):
    """name -> (return type, [(type, is pointer)]) of every diffhe_* function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    text = re.sub(r"typedef struct.*?\}\s*\w+;", "", text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][A-Za-z_ ]*?\**)\s*\b(diffhe_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = []
        for a in ([] if args.strip() == "void" else args.split(",")):
            m = re.match(r"(.+?)\s*(\*?)\s*\w+$", re.sub(r"\bconst\b", "", a).strip())
            params.append((m.group(1).strip(), bool(m.group(2))))
        out[name] = (" ".join(ret.split()), params)
    return out


def test_second_signature_table_matches_the_second_header():
    """Arity, by-value types, pointer element types and the status errcheck of every diffhe_elast_* entry, binding against
    include/diffhe_elastic.h; the first table and its header keep their 64 entries."""
    decls = _declarations(HEADER)
    assert sorted(decls) == sorted(_hip.ELASTIC_SIGNATURES) and len(decls) == 3
    assert all(name.startswith("diffhe_elast_") for name in decls)
    assert not set(decls) & set(_hip.SIGNATURES) and len(_hip.SIGNATURES) == 64
    for name, (ret, params) in decls.items():
        res, argtypes = _hip.ELASTIC_SIGNATURES[name]
        assert len(argtypes) == len(params), name
        for i, ((ctype, is_ptr), t) in enumerate(zip(params, argtypes)):
            if not is_ptr:
                assert t is BY_VALUE[ctype], (name, i, ctype, t)
            else:
                assert isinstance(t, type) and issubclass(t, _hip._Ptr) and t.elem == ctype, (name, i, ctype, t)
        assert ret == "int" and res is _hip._S, name
    if os.path.exists(_hip.LIB_PATH):
        L = _hip.lib()
        for name in decls:
            fn = getattr(L, name)
            assert fn.restype is _hip._I and fn.errcheck is L.diffhe_to_node_major.errcheck, name
        with pytest.raises(_hip.HipExtensionError, match="diffhe_elast_grad_shared"):
            L.diffhe_elast_grad_shared(None, None, None, 2, 1.0, 1.0, None, None, None, 4, 2, 1, 1, None, None)
        assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "diffhe_elast_assemble_rows")


def test_refusals_on_the_host():
    from diffhe import ElasticFESolver
    with pytest.raises(NotImplementedError, match="2D or 3D"):
        ElasticFESolver(FEMesh.line(4))
    with pytest.raises(NotImplementedError, match="P1 elements only"):
        ElasticFESolver(FEMesh.rectangle_p2(2, 2))
    with pytest.raises(ValueError, match="plane="):
        ElasticFESolver(FEMesh.box(2, 2, 2), plane="stress")
    with pytest.raises(ValueError, match="plane"):
        ElasticFESolver(FEMesh.rectangle(2, 2), plane="membrane")
    with pytest.raises(ValueError, match="nu"):
        ElasticFESolver(FEMesh.rectangle(2, 2), nu=0.5)
    with pytest.raises(ValueError, match="fixed="):
        ElasticFESolver(FEMesh.rectangle(2, 2, bc_value=3.0))
    with pytest.raises(NotImplementedError, match="strength"):
        ElasticFESolver(FEMesh.rectangle(2, 2), amg=dict(strength=0.25))
    mesh = FEMesh.rectangle(3, 2)
    n = mesh.n_nodes
    solver = ElasticFESolver(mesh)
    f = torch.zeros(n, 2, dtype=T64)
    with pytest.raises(NotImplementedError, match="dirichlet="):
        solver(f, dirichlet=torch.zeros(len(mesh.dirichlet_nodes)))
    for name in ("h", "u_inf", "flux"):
        with pytest.raises(NotImplementedError, match="Robin"):
            solver(f, **{name: torch.zeros(1)})
    moving = FEMesh(nodes=mesh.nodes.clone().requires_grad_(True), elements=mesh.elements,
                    dirichlet_nodes=mesh.dirichlet_nodes)
    with pytest.raises(NotImplementedError, match="node gradients"):
        ElasticFESolver(moving)(f)
    # a wrong-shaped right-hand side: the messages of the base class, with the component axis
    with pytest.raises(ValueError, match=r"f must be \(n, d\) or \(B, n, d\) with n=12, d=2, got \(12,\)"):
        solver(torch.zeros(n, dtype=T64))
    with pytest.raises(ValueError, match=r"f must be .* got \(2, 12, 3\)"):
        solver(torch.zeros(2, n, 3, dtype=T64))
    with pytest.raises(ValueError, match=r"load must be .* got \(12, 1\)"):
        solver(f, load=torch.zeros(n, 1, dtype=T64))
    with pytest.raises(ValueError, match=r"layout='node': f \(and load\) must be \(n, d, B\)"):
        solver(torch.zeros(2, n, 2, dtype=T64), layout="node")
    with pytest.raises(ValueError, match="Unknown layout"):
        solver(f, layout="dof")
    with pytest.raises(ValueError, match="does not match"):
        solver(torch.zeros(3, n, 2, dtype=T64), load=torch.zeros(2, n, 2, dtype=T64))
    with pytest.raises(ValueError, match="kappa batch 2 does not match f batch 3"):
        ElasticFESolver(mesh, torch.ones(2, mesh.n_elements, dtype=T64))(torch.zeros(3, n, 2, dtype=T64))


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
NU = 0.3


def _case_2d(nx=7, ny=5, seed=5):
    """Jittered rectangle, left edge clamped, one extra roller dof, one non-zero prescribed displacement."""
    mesh = _rect(nx, ny, seed)
    fixed = {(i, a): 0.0 for i in _left_nodes(nx, ny) for a in range(2)}
    fixed[(nx, 1)] = 0.0                            # roller: bottom right corner, u_y
    fixed[((ny + 1) * (nx + 1) - 1, 0)] = 0.05      # top right corner, u_x prescribed
    return mesh, fixed


def _e_layouts(m, B, seed=11):
    field = _rand((B, m), seed, 0.5, 2.0)
    return {"scalar": torch.tensor(1.7, dtype=T64), "sample": _rand((B,), seed + 1, 0.5, 2.0), "elem": field[0].clone(),
            "sample_elem": field}


def _as_bm(E, m, B):
    """Any E layout as (B, m), differentiably."""
    if E.dim() == 0:
        return E.expand(B, m)
    if E.dim() == 1:
        return E[None, :].expand(B, m) if E.shape[0] == m else E[:, None].expand(B, m)
    return E


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_assembly_kernel_against_the_dense_matrix(dim):
    from diffhe.elastic import _setup_of, lame_unit, parse_fixed
    from diffhe.plan import get_plan
    if dim == 2:
        mesh, plane = _rect(5, 4, 7), "strain"
        fixed = {(i, a): 0.0 for i in _left_nodes(5, 4) for a in range(2)}
        fixed[(5, 1)], fixed[(29, 0)] = 0.0, 0.3
    else:
        mesh, plane = _box(3, 2, 2, 7), None
        fixed = {(i, a): 0.0 for i in range(mesh.n_nodes) if i % 4 == 0 for a in range(3)}
        fixed[(3, 2)], fixed[(mesh.n_nodes - 1, 1)] = 0.0, -0.2
    n, d, m, B = mesh.n_nodes, mesh.dim, mesh.n_elements, 3
    plan = get_plan(mesh, torch.device(DEV), prune=False)
    lam1, mu1 = lame_unit(NU, d, plane)
    setup = _setup_of(plan, NU, plane, lam1, mu1, *parse_fixed(mesh, fixed))
    cols = setup.cols_host
    assert np.array_equal(cols, setup.dofs.cols.cpu().numpy())
    bc, free, g = _fixed_arrays(mesh, fixed)
    field = _rand((B, m), 8, 0.5, 2.0)
    Kall = _dense_K(mesh, torch.cat([field, torch.ones(1, m, dtype=T64)]), NU, plane)         # padding sample: E = 1
    # Bv = 1: a field the batch shares
    vals, lift = setup.assemble(field[0].to(DEV).contiguous(), 1, 0, 1)
    Bp = 4
    kp = torch.ones(m, Bp, dtype=T64)
    kp[:, :B] = field.t()
    vals_b, lift_b = setup.assemble(kp.to(DEV).contiguous(), Bp, 1, Bp)
    torch.cuda.synchronize()
    assert vals.shape == (d * plan.W, n * d, 1) and vals_b.shape == (d * plan.W, n * d, Bp)
    for b, (v, lf) in enumerate([(vals[:, :, 0], lift[:, 0])] + [(vals_b[:, :, s], lift_b[:, s]) for s in range(Bp)]):
        K = Kall[0 if b == 0 else b - 1]
        bound = 1e-13 * float(K.abs().max())
        want = _through_pattern(_eliminated(K, bc), cols)
        assert float(np.abs(v.cpu().numpy() - want).max()) <= bound, b
        want_lift = K[:, bc] @ g[bc]
        want_lift[bc] = 0.0
        assert float((lf.cpu() - want_lift).abs().max()) <= bound, b


@pytest.mark.gpu
@pytest.mark.parametrize("plane", ["stress", "strain"])
@pytest.mark.parametrize("e_layout", ["scalar", "sample", "elem", "sample_elem"])
def test_forward_every_layout(e_layout, plane):
    from diffhe import ElasticFESolver
    mesh, fixed = _case_2d()
    n, m, B = mesh.n_nodes, mesh.n_elements, 3
    E = _e_layouts(m, B)[e_layout]
    f, load = _rand((B, n, 2), 21, -1, 1), _rand((B, n, 2), 22, -0.1, 0.1)
    want = _dense_solve(mesh, _as_bm(E, m, B), NU, plane, fixed, f, load)
    solver = ElasticFESolver(mesh, E.to(DEV), NU, plane=plane, fixed=fixed, device=DEV, tol=1e-13)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        u = solver(f.to(DEV), load.to(DEV))
        info = solver.last_info
        assert u.shape == (B, n, 2) and info.not_converged == 0 and info.path in ("ell-amgpcg", "ell-pcg")
        assert rel_err(u.cpu().numpy(), want.numpy()) <= RTOL_U
        u_nm = solver(f.permute(1, 2, 0).contiguous().to(DEV), load.permute(1, 2, 0).contiguous().to(DEV), layout="node")
        assert u_nm.shape == (n, 2, B)
        assert rel_err(u_nm.permute(2, 0, 1).cpu().numpy(), want.numpy()) <= RTOL_U
        if e_layout == "sample_elem":      # the field element-major, like f and u
            s2 = ElasticFESolver(mesh, E.t().contiguous().to(DEV), NU, plane=plane, fixed=fixed, device=DEV, tol=1e-13)
            u_em = s2(f.permute(1, 2, 0).contiguous().to(DEV), load.permute(1, 2, 0).contiguous().to(DEV), layout="node")
            assert rel_err(u_em.permute(2, 0, 1).cpu().numpy(), want.numpy()) <= RTOL_U
        if e_layout in ("scalar", "elem"):  # B absent: (n, d) in, (n, d) out; f None means zero
            u1 = solver(f[1].to(DEV), load[1].to(DEV))
            assert u1.shape == (n, 2)
            assert rel_err(u1.cpu().numpy(), want[1].numpy()) <= RTOL_U
            u0 = solver(None, load[2].to(DEV))
            want0 = _dense_solve(mesh, _as_bm(E, m, 1), NU, plane, fixed, None, load[2:3])[0]
            assert u0.shape == (n, 2) and rel_err(u0.cpu().numpy(), want0.numpy()) <= RTOL_U
    # the prescribed values are exact
    assert float(u[:, 7, 1].abs().max()) == 0.0 and bool((u[:, n - 1, 0] == 0.05).all())


def _loss(u, w):
    return (w * u).sum() + 0.5 * (u ** 2).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("e_layout", ["scalar", "sample", "elem", "sample_elem"])
def test_gradients_every_layout(e_layout):
    from diffhe import ElasticFESolver
    mesh, fixed = _case_2d()
    n, m, B = mesh.n_nodes, mesh.n_elements, 3
    E0 = _e_layouts(m, B)[e_layout]
    f0, load0, w = _rand((B, n, 2), 21, -1, 1), _rand((B, n, 2), 22, -0.1, 0.1), _rand((B, n, 2), 23, -1, 1)
    Er, fr, lr = (t.clone().requires_grad_(True) for t in (E0, f0, load0))
    _loss(_dense_solve(mesh, _as_bm(Er, m, B), NU, "stress", fixed, fr, lr), w).backward()
    E, f, load = (t.to(DEV).requires_grad_(True) for t in (E0, f0, load0))
    solver = ElasticFESolver(mesh, E, NU, fixed=fixed, device=DEV, tol=1e-13)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _loss(solver(f, load), w.to(DEV)).backward()
    assert solver.last_info.not_converged == 0 and solver.last_info.adj_iterations > 0
    assert E.grad.shape == E0.shape and f.grad.shape == f0.shape and load.grad.shape == load0.shape
    assert rel_err(E.grad.cpu().numpy(), Er.grad.numpy()) <= RTOL_GRAD
    assert rel_err(f.grad.cpu().numpy(), fr.grad.numpy()) <= RTOL_GRAD
    assert rel_err(load.grad.cpu().numpy(), lr.grad.numpy()) <= RTOL_GRAD
    bc, _, _ = _fixed_arrays(mesh, fixed)
    assert float(load.grad.reshape(B, -1)[:, bc].abs().max()) == 0.0             # dL/dload = lambda: zero on fixed dofs
    # node layout, the field element-major where it is per sample: the same numbers
    En = (E0.t().contiguous() if e_layout == "sample_elem" else E0).to(DEV).requires_grad_(True)
    fn, ln = (t.permute(1, 2, 0).contiguous().to(DEV).requires_grad_(True) for t in (f0, load0))
    s2 = ElasticFESolver(mesh, En, NU, fixed=fixed, device=DEV, tol=1e-13)
    _loss(s2(fn, ln, layout="node"), w.permute(1, 2, 0).to(DEV)).backward()
    gE = En.grad.t() if e_layout == "sample_elem" else En.grad
    assert rel_err(gE.cpu().numpy(), Er.grad.numpy()) <= RTOL_GRAD
    assert rel_err(fn.grad.permute(2, 0, 1).cpu().numpy(), fr.grad.numpy()) <= RTOL_GRAD
    assert rel_err(ln.grad.permute(2, 0, 1).cpu().numpy(), lr.grad.numpy()) <= RTOL_GRAD
    # one right-hand side for the batch: its gradient is the sum over the samples
    if e_layout == "sample":
        f1, l1 = (t[0].clone().to(DEV).requires_grad_(True) for t in (f0, load0))
        fr1, lr1 = (t[0].clone().requires_grad_(True) for t in (f0, load0))
        _loss(_dense_solve(mesh, _as_bm(E0, m, B), NU, "stress", fixed, fr1, lr1), w).backward()
        s3 = ElasticFESolver(mesh, E0.to(DEV), NU, fixed=fixed, device=DEV, tol=1e-13)
        _loss(s3(f1, l1), w.to(DEV)).backward()
        assert f1.grad.shape == (n, 2) and rel_err(f1.grad.cpu().numpy(), fr1.grad.numpy()) <= RTOL_GRAD
        assert rel_err(l1.grad.cpu().numpy(), lr1.grad.numpy()) <= RTOL_GRAD


@pytest.mark.gpu
def test_shared_field_gradient_is_reproducible_and_the_sum_of_the_per_sample_ones():
    from diffhe import ElasticFESolver
    mesh, fixed = _case_2d()
    n, m, B = mesh.n_nodes, mesh.n_elements, 3
    field = _rand((m,), 31, 0.5, 2.0)
    f, w = _rand((B, n, 2), 21, -1, 1).to(DEV), _rand((B, n, 2), 23, -1, 1).to(DEV)

    def grad_of(E):
        E = E.to(DEV).requires_grad_(True)
        solver = ElasticFESolver(mesh, E, NU, fixed=fixed, device=DEV, tol=1e-13)
        _loss(solver(f), w).backward()
        return E.grad.cpu()

    first, second = grad_of(field), grad_of(field)
    assert first.shape == (m,) and torch.equal(first, second)                     # fixed order: bitwise
    per_sample = grad_of(field[None, :].expand(B, m).contiguous())
    assert per_sample.shape == (B, m)
    assert rel_err(per_sample.sum(0).numpy(), first.numpy()) <= RTOL_GRAD


@pytest.mark.gpu
def test_3d_displacement_and_all_three_gradients():
    from diffhe import ElasticFESolver
    nx, ny, nz = 3, 3, 2
    mesh = _box(nx, ny, nz, 9)
    n, m, B = mesh.n_nodes, mesh.n_elements, 2
    fixed = {(i, a): 0.0 for i in range(n) if i % (nx + 1) == 0 for a in range(3)}          # face x = 0
    E0, f0, load0, w = _rand((B, m), 41, 0.5, 2.0), _rand((B, n, 3), 42, -1, 1), _rand((B, n, 3), 43, -0.1, 0.1), \
        _rand((B, n, 3), 44, -1, 1)
    Er, fr, lr = (t.clone().requires_grad_(True) for t in (E0, f0, load0))
    want = _dense_solve(mesh, Er, NU, None, fixed, fr, lr)
    _loss(want, w).backward()
    E, f, load = (t.to(DEV).requires_grad_(True) for t in (E0, f0, load0))
    solver = ElasticFESolver(mesh, E, NU, fixed=fixed, device=DEV, tol=1e-13)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        u = solver(f, load)
        _loss(u, w.to(DEV)).backward()
    assert u.shape == (B, n, 3) and solver.last_info.not_converged == 0
    assert rel_err(u.detach().cpu().numpy(), want.detach().numpy()) <= RTOL_U
    assert rel_err(E.grad.cpu().numpy(), Er.grad.numpy()) <= RTOL_GRAD
    assert rel_err(f.grad.cpu().numpy(), fr.grad.numpy()) <= RTOL_GRAD
    assert rel_err(load.grad.cpu().numpy(), lr.grad.numpy()) <= RTOL_GRAD


@pytest.fixture(scope="module")
def multilevel_case():
    nx, ny, B = 24, 16, 2
    mesh = _rect(nx, ny, 13)
    fixed = {(i, a): 0.0 for i in _left_nodes(nx, ny) for a in range(2)}
    n, m = mesh.n_nodes, mesh.n_elements
    assert 2 * n == 850
    E0, load0, w = _rand((B, m), 51, 0.5, 2.0), torch.zeros(B, n, 2, dtype=T64), _rand((B, n, 2), 53, -1, 1)
    load0[:, [r * (nx + 1) + nx for r in range(ny + 1)], 1] = -_rand((B, 1), 52, 0.5, 1.0)   # a shear load on the tip
    Er = E0.clone().requires_grad_(True)
    want = _dense_solve(mesh, Er, NU, "stress", fixed, None, load0)
    _loss(want, w).backward()
    return mesh, fixed, E0, load0, w, want.detach(), Er.grad


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["auto", "ell-jacobi"])
def test_multilevel_hierarchy_and_jacobi_agree_with_the_dense_solve(multilevel_case, method):
    from diffhe import ElasticFESolver
    mesh, fixed, E0, load0, w, want, want_grad = multilevel_case
    E = E0.to(DEV).requires_grad_(True)
    solver = ElasticFESolver(mesh, E, NU, fixed=fixed, device=DEV, tol=1e-13, method=method)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        u = solver(None, load0.to(DEV))
        info = solver.last_info
        print(f"elastic 24x16 {method}: path {info.path}, {info.iterations} iterations, relres {info.max_relres:.1e}, "
              f"levels {info.hierarchy_levels}, operator complexity {info.operator_complexity:.2f}")
        _loss(u, w.to(DEV)).backward()
    if method == "auto":
        assert info.path == "ell-amgpcg" and info.hierarchy_levels >= 2 and info.operator_complexity > 1.0
    else:
        assert info.path == "ell-pcg" and info.hierarchy_levels == 0
    assert info.not_converged == 0 and solver.last_info.adj_iterations > 0
    assert rel_err(u.detach().cpu().numpy(), want.numpy()) <= RTOL_U
    assert rel_err(E.grad.cpu().numpy(), want_grad.numpy()) <= RTOL_GRAD


@pytest.mark.gpu
def test_second_order_backward_is_refused():
    from diffhe import ElasticFESolver
    mesh, fixed = _case_2d()
    E = torch.full((mesh.n_elements,), 1.3, dtype=T64, device=DEV, requires_grad=True)
    solver = ElasticFESolver(mesh, E, NU, fixed=fixed, device=DEV)
    u = solver(torch.ones(mesh.n_nodes, 2, dtype=T64, device=DEV))
    (gE,) = torch.autograd.grad(u.sum(), E, retain_graph=True)
    assert gE.shape == E.shape and bool(torch.isfinite(gE).all())
    with pytest.raises(NotImplementedError, match="create_graph=True"):
        torch.autograd.grad(u.sum(), E, create_graph=True)
