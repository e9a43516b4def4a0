"""Eigenstrain and thermal loads of elastic solves (ElasticFESolver.eigenstrain_load, `eigenstrain=` of the solve and of
stress / von_mises / stress_and_von_mises, diffhe.elastic.thermal_strain / element_mean, csrc/eigenstrain.hip, the eigen
instantiations of csrc/stress.hip, include/diffhe_eigenstrain.h).

The oracle is an independent dense torch restatement in B^T D form, differentiated by autograd in fp64 on the CPU: Voigt
matrix D and strain-displacement matrix B_e with ENGINEERING shear strains, F0 = sum_e vol_e E_e B_e^T D eps0_e,
sigma_e = E_e D (B_e u_e - eps0_e), plane strain through the 4 x 4 block (xx, yy, xy, zz) of the 3D matrix, then the von
Mises stress from the deviator of the full 3 x 3 tensor.  The geometry, B_e and the mesh helpers are those of
tests/test_stress.py.  The CPU tests pin the oracle to closed forms at 1e-12 and check the fourth signature table, the two
torch helpers and the host refusals; the GPU tests hold the kernels and the Python layer against it.

Bounds, relative to the largest oracle entry (`rel_err`), as in test_stress.py and test_elasticity.py.  Kernel values
without a solve -- F0 (at most 24 incident element terms per dof), sigma, vm, per-element dE and d eps0 (no sum), u_bar:
1e-12, some 60 fp64 operations per value and no cancellation beyond the terms themselves.  Per-sample and batch-shared
totals of mixed sign (up to m or B m terms): 1e-11.  Anything through a multigrid-PCG solve (tol 1e-13, condition of the
small meshes): 1e-10.
"""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from diffhe import DifferentiableFESolver, ElasticFESolver, FEMesh, _hip
from diffhe import elastic
from _util import rel_err
from test_stress import BY_VALUE, _declarations, _geometry, _jitter, _mixed_orientation, _rand, _strain_matrix

T64 = torch.float64
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "diffhe_eigenstrain.h")
NU = 0.3
NAMES = ["diffhe_eigenstrain_load", "diffhe_eigenstrain_load_adjoint", "diffhe_eigenstrain_load_adjoint_shared",
         "diffhe_stress_adjoint_eigen", "diffhe_stress_adjoint_eigen_shared", "diffhe_stress_eval_eigen"]


# ------------------------------------------------------------------------------------------------
# the oracle (independent of the product code)
# ------------------------------------------------------------------------------------------------
def _nc0(d, plane):
    return 6 if d == 3 else (4 if plane == "strain" else 3)


def _voigt_D(nu, d, plane):
    """The Voigt matrix of E = 1 for engineering shear strains in the order of eps0: (xx, yy, xy) in plane stress,
    (xx, yy, xy, zz) in plane strain -- that block of the 3D matrix -- and (xx, yy, zz, yz, xz, xy) in 3D."""
    if d == 2 and plane == "stress":
        return torch.tensor([[1, nu, 0], [nu, 1, 0], [0, 0, (1 - nu) / 2]], dtype=T64) / (1 - nu * nu)
    lam, mu = nu / ((1 + nu) * (1 - 2 * nu)), 1 / (2 * (1 + nu))
    D = torch.zeros(6, 6, dtype=T64)
    D[:3, :3] = lam
    D[:3, :3] += 2 * mu * torch.eye(3, dtype=T64)
    D[3:, 3:] = mu * torch.eye(3, dtype=T64)
    if d == 3:
        return D
    idx = torch.tensor([0, 1, 5, 2])
    return D[idx][:, idx]


def _engineering(eps0, d):
    """eps0 (..., nc0) in tensor components -> engineering shear strains."""
    nc = d * (d + 1) // 2
    scale = torch.ones(eps0.shape[-1], dtype=T64)
    scale[d:nc] = 2.0
    return eps0 * scale


def _strain_rows(mesh, plane):
    """(B_e (m, nc0, npe*d), vol (m)): the strain-displacement matrix with a zero zz row in plane strain."""
    G, vol = _geometry(mesh.nodes.to(T64), mesh.elements.long())
    Bm = _strain_matrix(G)
    if mesh.dim == 2 and plane == "strain":
        Bm = torch.cat([Bm, torch.zeros(Bm.shape[0], 1, Bm.shape[2], dtype=T64)], 1)
    return Bm, vol


def _dofs(mesh):
    el, d = mesh.elements.long(), mesh.dim
    return (el[:, :, None] * d + torch.arange(d)[None, None, :]).reshape(el.shape[0], -1)


def _oracle_load(mesh, E, eps0, nu, plane):
    """E (B, m), eps0 (B, m, nc0) -> F0 (B, n, d)."""
    n, d = mesh.nodes.shape
    Bm, vol = _strain_rows(mesh, plane)
    fe = torch.einsum("m,bm,mvk,vw,bmw->bmk", vol, E, Bm, _voigt_D(nu, d, plane), _engineering(eps0, d))
    B = E.shape[0]
    return torch.zeros(B, n * d, dtype=T64).index_add(1, _dofs(mesh).reshape(-1), fe.reshape(B, -1)).reshape(B, n, d)


def _oracle_stress(mesh, u, E, eps0, nu, plane):
    """u (B, n, d), E (B, m), eps0 (B, m, nc0) -> sigma (B, m, nc) in plane, sigma_zz (B, m) (2D; None in 3D), vm."""
    d = mesh.dim
    nc = d * (d + 1) // 2
    B, m = E.shape
    Bm, _ = _strain_rows(mesh, plane)
    ue = u[:, mesh.elements.long()].reshape(B, m, -1)
    strain = torch.einsum("mvk,bmk->bmv", Bm, ue) - _engineering(eps0, d)
    full = E[:, :, None] * torch.einsum("vw,bmw->bmv", _voigt_D(nu, d, plane), strain)
    sigma = full[..., :nc]
    szz = full[..., 3] if (d == 2 and plane == "strain") else (torch.zeros(B, m, dtype=T64) if d == 2 else None)
    pairs = [(0, 0), (1, 1), (0, 1)] if d == 2 else [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
    S = torch.zeros(B, m, 3, 3, dtype=T64)
    entries = [(pairs[k], sigma[..., k]) for k in range(nc)] + [((t, a), sigma[..., k]) for k, (a, t) in enumerate(pairs)
                                                                  if a != t]
    if d == 2:
        entries.append(((2, 2), szz))
    for (a, t), v in entries:
        onehot = torch.zeros(3, 3, dtype=T64)
        onehot[a, t] = 1.0
        S = S + v[..., None, None] * onehot
    dev = S - (S.diagonal(dim1=-2, dim2=-1).sum(-1) / 3.0)[..., None, None] * torch.eye(3, dtype=T64)
    return sigma, szz, torch.sqrt(1.5 * (dev * dev).sum(dim=(-2, -1)))


def _load_map(mesh):
    """(n, n) load map M of the solvers, F = M f: every vertex of an element gets |e| / (d + 1) times the mean of f."""
    n, npe = mesh.n_nodes, mesh.elements.shape[1]
    el = mesh.elements.long()
    _, vol = _geometry(mesh.nodes.to(T64), el)
    idx = (el[:, :, None] * n + el[:, None, :]).reshape(-1)
    return torch.zeros(n * n, dtype=T64).index_add(0, idx, (vol / npe ** 2)[:, None].expand(-1, npe * npe).reshape(-1)).reshape(n, n)


def _dense_solve(mesh, E, nu, plane, fixed, rhs):
    """u (B, n, d) of K(E_b) u = rhs_b on the free dofs with u = value on `fixed` {(node, component): value} (through the
    lift), K_e = vol_e E_e B^T D B; rhs (B, n, d) or (n, d).  Differentiable in E and rhs."""
    n, d = mesh.nodes.shape
    B, m = E.shape
    Bm, vol = _strain_rows(mesh, plane)
    k0 = vol[:, None, None] * (Bm.transpose(1, 2) @ _voigt_D(nu, d, plane) @ Bm)
    dof = _dofs(mesh)
    idx = (dof[:, :, None] * (n * d) + dof[:, None, :]).reshape(-1)
    K = torch.zeros(B, (n * d) ** 2, dtype=T64).index_add(1, idx, (E[:, :, None, None] * k0[None]).reshape(B, -1))
    K = K.reshape(B, n * d, n * d)
    fixed_dofs = np.array([i * d + a for i, a in fixed], dtype=np.int64)
    g = torch.zeros(n * d, dtype=T64)
    g[torch.from_numpy(fixed_dofs)] = torch.tensor([float(v) for v in fixed.values()], dtype=T64)
    free = torch.from_numpy(np.setdiff1d(np.arange(n * d), fixed_dofs))
    r = rhs.reshape(-1, n * d).expand(B, n * d) - K @ g
    uf = torch.linalg.solve(K[:, free][:, :, free], r[:, free].unsqueeze(2)).squeeze(2)
    return (g[None].expand(B, -1).clone().index_add(1, free, uf)).reshape(B, n, d)


# ------------------------------------------------------------------------------------------------
# meshes, layouts, data
# ------------------------------------------------------------------------------------------------
MESHES = {
    "2d-stress": (_jitter(FEMesh.rectangle(7, 5), 0), "stress"),
    "2d-strain": (_jitter(FEMesh.rectangle(7, 5), 0), "strain"),
    "3d": (_jitter(FEMesh.box(3, 3, 2), 1), None),
    "2d-blocks": (_jitter(FEMesh.rectangle(13, 12), 2), "stress"),          # 312 elements: two blocks at Bp = 1
}
MESHES["2d-84"] = (_jitter(FEMesh.rectangle(7, 6), 3), "strain")            # 84 elements: an (m,) field at B = 70
MESHES["2d-mixed"] = (_mixed_orientation(MESHES["2d-strain"][0]), "strain")
E_KINDS = ("scalar", "sample", "elem", "sample_elem", "elem_major")          # the five layouts of E
Z_KINDS = ("tensor", "sample", "field", "sample_field")                      # the four of eps0; "node": (nc0, m, B)


def _modulus(kind, read, B, m, seed=5):
    """E in the caller's layout `kind` (batch B) and the map to the oracle's (Bo, m) for the layout it is `read` as."""
    shape = {"scalar": (), "sample": (B,), "elem": (m,), "sample_elem": (B, m), "elem_major": (m, B)}[kind]
    expand = {"scalar": lambda t: t.expand(1, m), "sample": lambda t: t[:, None].expand(B, m), "elem": lambda t: t[None, :],
              "sample_elem": lambda t: t, "elem_major": lambda t: t.t()}[read]
    return _rand(shape, seed, 0.5, 2.0), expand


def _eigenstrain(kind, read, B, m, nc0, seed=6):
    """eps0 in the caller's layout `kind` and the map to the oracle's (Bo, m, nc0) for the layout it is `read` as."""
    shape = {"tensor": (nc0,), "sample": (B, nc0), "field": (m, nc0), "sample_field": (B, m, nc0), "node": (nc0, m, B)}[kind]
    expand = {"tensor": lambda t: t.expand(1, m, nc0), "sample": lambda t: t[:, None, :].expand(B, m, nc0),
              "field": lambda t: t[None], "sample_field": lambda t: t, "node": lambda t: t.permute(2, 1, 0)}[read]
    return _rand(shape, seed, -1e-2, 1e-2), expand


def _reads(zkind, ekind, B, m, layout, known):
    """-> (how eps0 is read, how E is read, batched) by the documented rules (`elastic._eigen_batch`, `_kappa_layout`).
    rectangle(7, 5) has 70 elements, so at B = 70 some shapes read both ways.  known: the call has a batch of B from a
    shape that reads one way only (f, load, u, a (B, m, nc0) or (nc0, m, B) eps0, a two-dimensional E); then an (m, nc0)
    eps0 and an (m,) E next to B = m are one value per sample, as kappa is next to f.  Otherwise a (70, nc0) eps0 and a
    (70,) E ARE fields.  A square E under layout="node" is element-major."""
    z, e = zkind, ekind
    if B == m and B > 1:
        if known:
            z, e = ("sample" if z == "field" else z), ("sample" if e == "elem" else e)
        else:
            z, e = ("field" if z == "sample" else z), ("elem" if e == "sample" else e)
        if e == "sample_elem" and layout == "node":
            e = "elem_major"
    batched = B > 1 and (z in ("sample", "sample_field", "node") or e in ("sample", "sample_elem", "elem_major"))
    return z, e, batched


def _expanded(t_map, Bo):
    """The oracle's operand at the batch of the call: an unbatched one broadcast."""
    return lambda t: t_map(t).expand(Bo, *t_map(t).shape[1:])


def _batch_shows(zkind, ekind):
    """Does an operand show the batch by a shape that reads one way only (`elastic._eigen_batch`)?"""
    return zkind in ("sample_field", "node") or ekind in ("sample_elem", "elem_major")


def _load_cases():
    """(mesh key, B, layout, eps0 kind, E kind): every eps0 layout x every E layout that is legal with it x both layouts
    on one mesh at B = 3 (padding) and B = 70 (two lane groups; 70 = m: the tie rule), the other meshes and widths on the
    layouts that take another path in the kernels."""
    out = []
    for B, layout in itertools.product((3, 70), ("sample", "node")):
        zkinds = Z_KINDS + (("node",) if layout == "node" else ())
        ekinds = E_KINDS if layout == "node" else E_KINDS[:4]
        out += [("2d-strain", B, layout, z, e) for z, e in itertools.product(zkinds, ekinds)]
    for key in ("2d-stress", "3d", "2d-mixed"):
        out += [(key, 1, "sample", "tensor", "scalar"), (key, 1, "sample", "field", "elem"),
                (key, 3, "sample", "sample_field", "sample_elem"), (key, 3, "sample", "sample", "elem"),
                (key, 70, "sample", "field", "sample_elem"), (key, 3, "node", "node", "elem_major")]
    out += [("2d-blocks", 1, "sample", "field", "elem"), ("2d-blocks", 1, "sample", "tensor", "scalar")]
    return out


def _case_id(c):
    return "-".join(str(v) for v in c)


def _operands(case):
    """-> (solver, mesh, plane, eps0, its oracle map, E, its oracle map, batched) of a case."""
    key, B, layout, zkind, ekind = case
    mesh, plane = MESHES[key]
    m, nc0 = mesh.n_elements, _nc0(mesh.dim, plane)
    zread, eread, batched = _reads(zkind, ekind, B, m, layout, _batch_shows(zkind, ekind))
    Bo = B if batched else 1
    eps0, z_map = _eigenstrain(zkind, zread, B, m, nc0)
    E, e_map = _modulus(ekind, eread, B, m)
    solver = ElasticFESolver(mesh, 1.0, NU, plane=plane, device=DEV)
    return solver, mesh, plane, eps0, _expanded(z_map, Bo), E, _expanded(e_map, Bo), batched


def _load_to_caller(F0, batched, layout):
    if layout == "node":
        return F0.permute(1, 2, 0)
    return F0 if batched else F0[0]


def _e_bound(ekind):
    return 1e-12 if ekind in ("sample_elem", "elem_major") else 1e-11


def _z_bound(zkind):
    return 1e-12 if zkind in ("sample_field", "node") else 1e-11


# ------------------------------------------------------------------------------------------------
# CPU: the oracle against closed forms (1e-12, the bound the project uses for its oracles)
# ------------------------------------------------------------------------------------------------
CPU_MESHES = {"2d-stress": (_jitter(FEMesh.rectangle(4, 3), 3), "stress"), "2d-strain": (_jitter(FEMesh.rectangle(4, 3), 3), "strain"),
              "3d": (_jitter(FEMesh.box(2, 2, 2), 4), None)}


def _strain_tensor(eps0, d):
    """The symmetric d x d tensor of eps0 (nc0) in tensor components."""
    pairs = [(0, 0), (1, 1), (0, 1)] if d == 2 else [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
    T = torch.zeros(d, d, dtype=T64)
    for k, (a, t) in enumerate(pairs):
        T[a, t] = T[t, a] = eps0[k]
    return T


def _rigid_fixed(mesh, u_exact):
    """{(node, component): value}: just the rigid motions, prescribed at the exact displacement -- all components of the
    node nearest the origin, d - 1 of the node farthest along x, and in 3D one more of the node farthest along y."""
    X, d = mesh.nodes.to(T64), mesh.dim
    a = int(X.norm(dim=1).argmin())
    b = int((X[:, 0] - X[:, 1:].abs().sum(1)).argmax())
    keys = [(a, c) for c in range(d)] + [(b, c) for c in range(1, d)]
    if d == 3:
        c3 = int((X[:, 1] - X[:, 0].abs() - X[:, 2].abs()).argmax())
        keys.append((c3, 2))
    return {(i, c): float(u_exact[i, c]) for i, c in keys}


def _compatible(mesh, plane):
    """A constant eigenstrain with shear (zz = 0 in plane strain) and its exact displacement u = eps0 x."""
    d, nc0 = mesh.dim, _nc0(mesh.dim, plane)
    eps0 = _rand((nc0,), 3, -1e-2, 1e-2)
    if nc0 == 4:
        eps0[3] = 0.0
    return mesh, plane, eps0, mesh.nodes.to(T64) @ _strain_tensor(eps0, d).t()


@pytest.mark.parametrize("key", ["2d-stress", "2d-strain", "3d"])
def test_oracle_compatible_eigenstrain_is_stress_free(key):
    """Any constant eps0 with a heterogeneous E and only the rigid motions fixed: u = eps0 x, sigma = 0, vm = 0."""
    mesh, plane, eps0, u_exact = _compatible(*CPU_MESHES[key])
    m, nc0 = mesh.n_elements, eps0.shape[0]
    E = _rand((1, m), 2, 0.5, 2.0)
    z = eps0.expand(1, m, nc0)
    u = _dense_solve(mesh, E, NU, plane, _rigid_fixed(mesh, u_exact), _oracle_load(mesh, E, z, NU, plane))
    sigma, szz, vm = _oracle_stress(mesh, u, E, z, NU, plane)
    scale = float(eps0.abs().max())
    assert float((u[0] - u_exact).abs().max()) <= 1e-12 * float(u_exact.abs().max())
    assert float(sigma.abs().max()) <= 1e-12 * scale and float(vm.abs().max()) <= 1e-12 * scale
    assert szz is None or float(szz.abs().max()) <= 1e-12 * scale


def test_oracle_plane_strain_free_thermal_expansion():
    """eps0 = a (1, 1, 0, 1), free body: in plane u = (1 + nu) a x, sigma = 0; sigma_zz = -E a."""
    mesh, plane = CPU_MESHES["2d-strain"]
    m, a = mesh.n_elements, 3e-3
    E = _rand((1, m), 2, 0.5, 2.0)
    z = (a * torch.tensor([1.0, 1.0, 0.0, 1.0], dtype=T64)).expand(1, m, 4)
    u_exact = (1 + NU) * a * mesh.nodes.to(T64)
    u = _dense_solve(mesh, E, NU, plane, _rigid_fixed(mesh, u_exact), _oracle_load(mesh, E, z, NU, plane))
    sigma, szz, vm = _oracle_stress(mesh, u, E, z, NU, plane)
    assert float((u[0] - u_exact).abs().max()) <= 1e-12 * float(u_exact.abs().max())
    assert float(sigma.abs().max()) <= 1e-12 * a
    assert float((szz + E * a).abs().max()) <= 1e-12 * a and float((vm - E * a).abs().max()) <= 1e-12 * a


def _clamped_stress(d, plane, E, a):
    """sigma on the normals and sigma_zz of a fully clamped body under eps0 = a I: by hand from the definitions."""
    lam, mu = elastic.lame_unit(NU, d, plane)
    n_normal = 3 if (d == 3 or plane == "strain") else 2
    s0 = 2 * mu * a + lam * n_normal * a                        # 2 mu' eps0_aa + lambda' theta0
    szz = E * (lam * (0.0 - n_normal * a) - 2 * mu * a) if plane == "strain" else None
    return -E * s0, szz


@pytest.mark.parametrize("key", ["2d-stress", "2d-strain", "3d"])
def test_oracle_fully_clamped_thermal_stress(key):
    mesh, plane = CPU_MESHES[key]
    n, d, m, a = mesh.n_nodes, mesh.dim, mesh.n_elements, 2e-3
    nc0 = _nc0(d, plane)
    E = _rand((1, m), 2, 0.5, 2.0)
    z = elastic.thermal_strain(a, torch.ones(1, m, dtype=T64), d, plane)
    assert z.shape == (1, m, nc0)
    fixed = {(i, c): 0.0 for i in range(n) for c in range(d)}
    u = _dense_solve(mesh, E, NU, plane, fixed, _oracle_load(mesh, E, z, NU, plane))
    sigma, szz, _ = _oracle_stress(mesh, u, E, z, NU, plane)
    want, want_zz = _clamped_stress(d, plane, E, a)
    closed = {"3d": -E * a / (1 - 2 * NU), "2d-stress": -E * a / (1 - NU), "2d-strain": -E * a / (1 - 2 * NU)}[key]
    assert float(u.abs().max()) == 0.0
    assert float((want - closed).abs().max()) <= 1e-12 * a
    assert float((sigma[..., :d] - want[..., None]).abs().max()) <= 1e-12 * a and float(sigma[..., d:].abs().max()) <= 1e-12 * a
    if plane == "strain":
        assert float((szz - want_zz).abs().max()) <= 1e-12 * a and float((want_zz - closed).abs().max()) <= 1e-12 * a


# ------------------------------------------------------------------------------------------------
# CPU: the fourth signature table, the torch helpers, host refusals
# ------------------------------------------------------------------------------------------------
def test_fourth_signature_table_matches_the_fourth_header():
    decls = _declarations(HEADER)
    assert sorted(decls) == sorted(_hip.EIGENSTRAIN_SIGNATURES) == NAMES
    assert len(_hip.SIGNATURES) == 64 and len(_hip.ELASTIC_SIGNATURES) == 3 and len(_hip.STRESS_SIGNATURES) == 3
    assert not set(decls) & (set(_hip.SIGNATURES) | set(_hip.ELASTIC_SIGNATURES) | set(_hip.STRESS_SIGNATURES))
    for name, (ret, params) in decls.items():
        res, argtypes = _hip.EIGENSTRAIN_SIGNATURES[name]
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
        with pytest.raises(_hip.HipExtensionError, match="diffhe_eigenstrain_load"):    # refused on the host: no launch
            L.diffhe_eigenstrain_load(None, None, None, None, 2, 1.0, 1.0, 0, None, 0, 0, None, 1, 0, 0, 4, 2, 1, 1, None,
                                      None)


def test_thermal_strain_and_element_mean():
    mesh = FEMesh.rectangle(3, 2)
    n, m = mesh.n_nodes, mesh.n_elements
    dT = _rand((2, m), 1, 0.0, 50.0).requires_grad_(True)
    alpha = _rand((m,), 2, 1e-5, 2e-5)
    for dim, plane, nc0, normals in ((2, None, 3, [0, 1]), (2, "stress", 3, [0, 1]), (2, "strain", 4, [0, 1, 3]),
                                     (3, None, 6, [0, 1, 2])):
        for a, t in ((1.2e-5, dT), (alpha, dT), (1.2e-5, dT[0])):
            z = elastic.thermal_strain(a, t, dim, plane)
            assert z.shape == (*t.shape, nc0) and z.dtype == T64
            shears = [k for k in range(nc0) if k not in normals]
            assert all(torch.equal(z[..., k], torch.as_tensor(a, dtype=T64) * t) for k in normals)
            assert bool((z[..., shears] == 0).all())
    g, = torch.autograd.grad(elastic.thermal_strain(alpha, dT, 2, "strain").sum(), (dT,))
    assert torch.allclose(g, (3 * alpha).expand(2, m))
    with pytest.raises(ValueError, match="plane"):
        elastic.thermal_strain(1.0, dT, 3, "strain")
    with pytest.raises(ValueError, match="plane"):
        elastic.thermal_strain(1.0, dT, 2, "shell")
    with pytest.raises(ValueError, match="dT"):
        elastic.thermal_strain(1.0, torch.ones(2, 3, m), 2)
    T = _rand((2, n), 3).requires_grad_(True)
    Tm = elastic.element_mean(T, mesh)
    want = torch.stack([T[:, mesh.elements[:, p].long()] for p in range(3)]).mean(0)
    assert Tm.shape == (2, m) and torch.allclose(Tm, want, rtol=0, atol=1e-15)
    assert elastic.element_mean(T[0], mesh).shape == (m,)
    gT, = torch.autograd.grad(Tm.sum(), (T,))
    counts = torch.bincount(mesh.elements.reshape(-1).long(), minlength=n).to(T64) / 3.0
    assert torch.allclose(gT, counts.expand(2, n))
    with pytest.raises(ValueError, match="element_mean"):
        elastic.element_mean(torch.ones(n + 1), mesh)


def test_refusals_on_the_host():
    mesh = FEMesh.rectangle(3, 2)
    n, m = mesh.n_nodes, mesh.n_elements
    u = torch.zeros(n, 2, dtype=T64)
    for plane, nc0 in (("stress", 3), ("strain", 4)):
        solver = ElasticFESolver(mesh, torch.ones(2, m, dtype=T64), plane=plane)
        calls = [lambda z, **kw: solver.eigenstrain_load(z, **kw), lambda z, **kw: solver(eigenstrain=z, **kw),
                 lambda z, **kw: solver.stress(u, eigenstrain=z, **kw), lambda z, **kw: solver.von_mises(u, eigenstrain=z, **kw),
                 lambda z, **kw: solver.stress_and_von_mises(u, eigenstrain=z, **kw)]
        for call in calls:
            with pytest.raises(ValueError, match="eigenstrain"):                    # a wrong trailing dimension
                call(torch.zeros(m, nc0 + 2, dtype=T64))
            with pytest.raises(ValueError, match="eigenstrain"):
                call(torch.zeros(2, m + 1, nc0, dtype=T64))
            with pytest.raises(ValueError, match="batch"):                          # the solver's E has B = 2
                call(torch.zeros(3, m, nc0, dtype=T64))
            with pytest.raises(ValueError, match="batch"):
                call(torch.zeros(3, nc0, dtype=T64))
        with pytest.raises(ValueError, match="Unknown layout"):
            solver.eigenstrain_load(torch.zeros(nc0, dtype=T64), layout="element")
        with pytest.raises(ValueError, match="batch"):
            solver.eigenstrain_load(torch.zeros(2, m, nc0, dtype=T64), E=torch.ones(3, m, dtype=T64))
    stress = ElasticFESolver(mesh, 1.0, plane="stress")
    with pytest.raises(ValueError, match="plane stress takes 3 components"):         # zz has no effect in plane stress
        stress.eigenstrain_load(torch.zeros(m, 4, dtype=T64))
    with pytest.raises(ValueError, match="plane stress takes 3 components"):
        stress.von_mises(u, eigenstrain=torch.zeros(4, dtype=T64))
    with pytest.raises(NotImplementedError):                                         # the class's own refusals
        ElasticFESolver(FEMesh.line(4), 1.0)
    with pytest.raises(NotImplementedError, match="P1"):
        ElasticFESolver(FEMesh.rectangle_p2(2, 2), 1.0)


# ------------------------------------------------------------------------------------------------
# GPU: the load
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", _load_cases(), ids=_case_id)
def test_eigenstrain_load_and_its_gradients_match_the_oracle(case):
    key, B, layout, zkind, ekind = case
    solver, mesh, plane, eps0, z_map, E, e_map, batched = _operands(case)
    n, d = mesh.n_nodes, mesh.dim
    Bo = B if batched else 1
    eps0.requires_grad_(True)
    E.requires_grad_(True)
    want = _load_to_caller(_oracle_load(mesh, e_map(E), z_map(eps0), NU, plane), batched, layout)
    F0 = solver.eigenstrain_load(eps0, E, layout)
    assert F0.shape == want.shape == ((n, d, Bo) if layout == "node" else ((Bo, n, d) if batched else (n, d)))
    assert F0.dtype == T64 and F0.device == eps0.device
    err = rel_err(F0.detach(), want.detach())
    w = _rand(want.shape, 11, -1, 1)
    dz0, de0 = torch.autograd.grad((w * want).sum(), (eps0, E))
    dz, de = torch.autograd.grad((w * F0).sum(), (eps0, E))
    dz2, de2 = torch.autograd.grad((w * solver.eigenstrain_load(eps0, E, layout)).sum(), (eps0, E))
    ez, ee = rel_err(dz, dz0), rel_err(de, de0)
    print(f"{_case_id(case)}: rel_err F0 {err:.2e} d/deps0 {ez:.2e} (bound {_z_bound(zkind):g}) d/dE {ee:.2e} "
          f"(bound {_e_bound(ekind):g})")
    assert dz.shape == eps0.shape and de.shape == E.shape
    assert err <= 1e-12 and ez <= _z_bound(zkind) and ee <= _e_bound(ekind)
    assert torch.equal(dz, dz2) and torch.equal(de, de2)                 # two runs: bitwise, the torch reduction included
    dz_only, = torch.autograd.grad((w * solver.eigenstrain_load(eps0, E.detach(), layout)).sum(), (eps0,))
    de_only, = torch.autograd.grad((w * solver.eigenstrain_load(eps0.detach(), E, layout)).sum(), (E,))
    assert rel_err(dz_only, dz0) <= _z_bound(zkind) and rel_err(de_only, de0) <= _e_bound(ekind)


@pytest.mark.gpu
def test_E_defaults_to_the_solvers_and_second_order_is_refused():
    mesh, plane = MESHES["2d-strain"]
    m = mesh.n_elements
    E = _rand((3, m), 1, 0.5, 2.0).requires_grad_(True)
    solver = ElasticFESolver(mesh, E, NU, plane=plane, device=DEV)
    eps0 = _rand((m, 4), 2, -1e-2, 1e-2).requires_grad_(True)
    F0 = solver.eigenstrain_load(eps0)
    want = _oracle_load(mesh, E, eps0[None].expand(3, m, 4), NU, plane)
    assert F0.shape == (3, mesh.n_nodes, 2) and rel_err(F0.detach(), want.detach()) <= 1e-12
    F0.sum().backward()
    assert E.grad is not None and E.grad.shape == (3, m) and eps0.grad.shape == (m, 4)
    with pytest.raises(NotImplementedError, match="second-order"):
        solver.eigenstrain_load(eps0).sum().backward(create_graph=True)
    with pytest.raises(NotImplementedError, match="second-order"):
        solver.von_mises(torch.ones(mesh.n_nodes, 2, dtype=T64), eigenstrain=eps0).sum().backward(create_graph=True)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2d-strain", "2d-stress", "3d"])
def test_both_addressings_of_the_entries_agree_bitwise(key):
    """eps0, d / d eps0, sigma and its cotangent as (nc, m, Bp) and as (m, nc, Bp) through the strides; the adjoints
    without dE outputs give the same side products; the padding sample gets zeros."""
    from diffhe.plan import get_plan, _stream
    mesh, plane = MESHES[key]
    dev = torch.device(DEV)
    plan = get_plan(mesh, dev, prune=False)
    d, n, m, B, Bp = mesh.dim, mesh.n_nodes, mesh.n_elements, 3, 4
    nc, nc0 = d * (d + 1) // 2, _nc0(d, plane)
    lam1, mu1 = elastic.lame_unit(NU, d, plane)
    L, st = _hip.lib(), _stream(dev)
    gtab, vol = plan.oriented_gradient_table(), plan.gradient_table()[1]
    inc_ptr, inc = plan.shape_incidence()
    E = _rand((m, Bp), 2, 0.5, 2.0).to(dev)
    z_mc = _rand((m, nc0, Bp), 3, -1e-2, 1e-2).to(dev)
    z_cm = z_mc.permute(1, 0, 2).contiguous()
    zs = {"mc": (z_mc, Bp, nc0 * Bp, 1), "cm": (z_cm, m * Bp, Bp, 1)}
    new = lambda *shape: torch.full(shape, float("nan"), dtype=T64, device=dev)  # noqa: E731
    head = lambda z: (lam1, mu1, int(plane == "strain"), E, Bp, 1, *zs[z])  # noqa: E731
    # the load and its adjoint
    F = {z: new(n * d, Bp) for z in zs}
    for z in zs:
        L.diffhe_eigenstrain_load(inc_ptr, inc, gtab, vol, d, *head(z), n, m, B, Bp, F[z], st)
    assert bool(torch.isfinite(F["mc"]).all()) and torch.equal(F["mc"], F["cm"]) and bool((F["mc"][:, B:] == 0).all())
    w = _rand((n * d, Bp), 4, -1, 1).to(dev)
    outs = []
    for z, (osc, ose, shape), with_de in (("mc", (Bp, nc0 * Bp, (m, nc0, Bp)), True), ("cm", (m * Bp, Bp, (nc0, m, Bp)), True),
                                          ("cm", (m * Bp, Bp, (nc0, m, Bp)), False)):
        dz, de = new(*shape), new(m, Bp)
        L.diffhe_eigenstrain_load_adjoint(plan.elems, gtab, vol, d, *head(z), w, n, m, B, Bp, dz, osc, ose,
                                          de if with_de else None, None, None, st)
        outs.append((dz if shape[0] == m else dz.permute(1, 0, 2), de))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[2][0])
    assert bool(torch.isfinite(outs[0][0]).all()) and bool(torch.isfinite(outs[0][1]).all())
    assert bool((outs[0][0][..., B:] == 0).all()) and bool((outs[0][1][:, B:] == 0).all())
    # the stress entries
    u = _rand((n * d, Bp), 1, -1e-2, 1e-2).to(dev)
    shead = lambda z: (plan.elems, gtab, d, lam1, mu1, int(plane == "strain"), u, E, Bp, 1, *zs[z])  # noqa: E731
    s_cm, s_mc, vm, vm_only = new(nc, m, Bp), new(m, nc, Bp), new(m, Bp), new(m, Bp)
    L.diffhe_stress_eval_eigen(*shead("cm"), n, m, Bp, s_cm, m * Bp, Bp, vm, st)
    L.diffhe_stress_eval_eigen(*shead("mc"), n, m, Bp, s_mc, Bp, nc * Bp, None, st)
    L.diffhe_stress_eval_eigen(*shead("mc"), n, m, Bp, None, 0, 0, vm_only, st)
    assert bool(torch.isfinite(s_cm).all()) and torch.equal(s_cm.permute(1, 0, 2), s_mc) and torch.equal(vm, vm_only)
    sbar_mc, vbar = _rand((m, nc, Bp), 5, -1, 1).to(dev), _rand((m, Bp), 6, -1, 1).to(dev)
    sbar_cm = sbar_mc.permute(1, 0, 2).contiguous()
    outs = []
    for z, sbar, (osc, ose), (dzc, dze, shape), with_de in (
            ("mc", sbar_mc, (Bp, nc * Bp), (Bp, nc0 * Bp, (m, nc0, Bp)), True),
            ("cm", sbar_cm, (m * Bp, Bp), (m * Bp, Bp, (nc0, m, Bp)), True),
            ("cm", sbar_cm, (m * Bp, Bp), (m * Bp, Bp, (nc0, m, Bp)), False)):
        ubar, de, dz = new(n * d, Bp), new(m, Bp), new(*shape)
        L.diffhe_stress_adjoint_eigen(*shead(z), sbar, osc, ose, vbar, inc_ptr, inc, n, m, B, Bp, new(nc, m, Bp), ubar,
                                      de if with_de else None, None, None, dz, dzc, dze, st)
        outs.append((ubar, de, dz if shape[0] == m else dz.permute(1, 0, 2)))
    for k in (0, 2):
        assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[0][k], outs[2][k])
        assert bool(torch.isfinite(outs[0][k]).all()) and bool((outs[0][k][..., B:] == 0).all())
    assert torch.equal(outs[0][1], outs[1][1]) and bool((outs[0][1][:, B:] == 0).all())


# ------------------------------------------------------------------------------------------------
# GPU: the stress with an eigenstrain
# ------------------------------------------------------------------------------------------------
def _stress_cases():
    """(mesh key, B or None for an unbatched u, layout, eps0 kind, E kind)."""
    out = []
    for key in ("2d-stress", "2d-strain", "3d"):
        out += [(key, None, "sample", "tensor", "scalar"), (key, None, "sample", "field", "elem")]
        for B in (3, 70):
            out += [(key, B, "sample", z, e) for z, e in (("tensor", "sample"), ("sample", "elem"), ("field", "sample_elem"),
                                                          ("sample_field", "scalar"), ("sample_field", "sample_elem"))]
            out += [(key, B, "node", "node", "elem_major"), (key, B, "node", "field", "elem")]
    out += [("2d-blocks", None, "sample", "field", "elem"), ("2d-mixed", 3, "sample", "sample_field", "sample_elem"),
            ("2d-mixed", None, "sample", "field", "elem")]
    return out


def _stress_operands(case):
    """u always shows the batch, so (m, nc0) and (m,) next to B = m tie to one value per sample."""
    key, B, layout, zkind, ekind = case
    mesh, plane = MESHES[key]
    n, d, m, Bo = mesh.n_nodes, mesh.dim, mesh.n_elements, B or 1
    zread, eread, _ = _reads(zkind, ekind, Bo, m, layout, True)
    eps0, z_map = _eigenstrain(zkind, zread, Bo, m, _nc0(d, plane))
    E, e_map = _modulus(ekind, eread, Bo, m)
    z_map, e_map = _expanded(z_map, Bo), _expanded(e_map, Bo)
    if B is None:
        u, u_map = _rand((n, d), 7, -1e-2, 1e-2), lambda t: t[None]
    elif layout == "node":
        u, u_map = _rand((n, d, B), 7, -1e-2, 1e-2), lambda t: t.permute(2, 0, 1)
    else:
        u, u_map = _rand((B, n, d), 7, -1e-2, 1e-2), lambda t: t
    return ElasticFESolver(mesh, 1.0, NU, plane=plane, device=DEV), mesh, plane, u, u_map, eps0, z_map, E, e_map


def _stress_to_caller(sig, vm, B, layout):
    if B is None:
        return sig[0], vm[0]
    return (sig.permute(1, 2, 0), vm.t()) if layout == "node" else (sig, vm)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _stress_cases(), ids=_case_id)
def test_stress_with_eigenstrain_and_its_gradients_match_the_oracle(case):
    """Values of all three methods, then L = sum w_s sigma + sum w_vm vm (both cotangents in one backward) and each term
    alone, to u, E and eps0."""
    key, B, layout, zkind, ekind = case
    solver, mesh, plane, u, u_map, eps0, z_map, E, e_map = _stress_operands(case)
    for t in (u, E, eps0):
        t.requires_grad_(True)
    o_sig, _, o_vm = _oracle_stress(mesh, u_map(u), e_map(E), z_map(eps0), NU, plane)
    o_sig, o_vm = _stress_to_caller(o_sig, o_vm, B, layout)
    sig, vm = solver.stress_and_von_mises(u, E, layout, eigenstrain=eps0)
    s1, v1 = solver.stress(u, E, layout, eigenstrain=eps0), solver.von_mises(u, E, layout, eigenstrain=eps0)
    assert sig.shape == o_sig.shape and vm.shape == o_vm.shape and sig.device == u.device and vm.dtype == T64
    es, ev = rel_err(sig.detach(), o_sig.detach()), rel_err(vm.detach(), o_vm.detach())
    print(f"{_case_id(case)}: rel_err sigma {es:.2e} vm {ev:.2e}")
    assert es <= 1e-12 and ev <= 1e-12
    assert torch.equal(s1, sig) and torch.equal(v1, vm)
    w_s, w_v = _rand(o_sig.shape, 11, -1, 1), _rand(o_vm.shape, 12, -1, 1)
    losses = lambda s, v: {"both": (w_s * s).sum() + (w_v * v).sum(), "sigma": (w_s * s).sum(), "vm": (w_v * v).sum()}  # noqa: E731
    want = {k: torch.autograd.grad(Lk, (u, E, eps0), retain_graph=True) for k, Lk in losses(o_sig, o_vm).items()}
    got = {k: torch.autograd.grad(Lk, (u, E, eps0), retain_graph=True) for k, Lk in losses(sig, vm).items()}
    again = torch.autograd.grad(losses(sig, vm)["both"], (u, E, eps0), retain_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(got["both"], again))              # two runs: bitwise
    for k in got:
        (du, de, dz), (du0, de0, dz0) = got[k], want[k]
        assert du.shape == u.shape and de.shape == E.shape and dz.shape == eps0.shape
        eu, ee, ez = rel_err(du, du0), rel_err(de, de0), rel_err(dz, dz0)
        print(f"{_case_id(case)} {k}: rel_err dL/du {eu:.2e} dL/dE {ee:.2e} (bound {_e_bound(ekind):g}) dL/deps0 {ez:.2e} "
              f"(bound {_z_bound(zkind):g})")
        assert eu <= 1e-12 and ee <= _e_bound(ekind) and ez <= _z_bound(zkind), k
    # one input alone
    dz_only, = torch.autograd.grad((w_v * solver.von_mises(u.detach(), E.detach(), layout, eigenstrain=eps0)).sum(), (eps0,))
    du_only, = torch.autograd.grad((w_s * solver.stress(u, E.detach(), layout, eigenstrain=eps0.detach())).sum(), (u,))
    assert rel_err(dz_only, want["vm"][2]) <= _z_bound(zkind) and rel_err(du_only, want["sigma"][0]) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2d-stress", "2d-strain", "3d"])
def test_eigenstrain_none_is_bitwise_the_call_without_the_keyword(key):
    mesh, plane = MESHES[key]
    n, d, m = mesh.n_nodes, mesh.dim, mesh.n_elements
    left = [i for i in range(n) if float(mesh.nodes[i, 0]) < 0.1]
    fixed = {(i, a): 0.0 for i in left for a in range(d)}
    E = _rand((3, m), 1, 0.5, 2.0)
    solver = ElasticFESolver(mesh, E, NU, plane=plane, fixed=fixed, device=DEV, tol=1e-13)
    load = _rand((n, d), 2, -1, 1)
    u0, u1 = solver(load=load), solver(load=load, eigenstrain=None)
    assert torch.equal(u0, u1)
    for method in (solver.stress, solver.von_mises):
        assert torch.equal(method(u0), method(u0, eigenstrain=None))
    a, b = solver.stress_and_von_mises(u0), solver.stress_and_von_mises(u0, eigenstrain=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2d-strain", "3d"])
@pytest.mark.parametrize("B", [3, 70])
def test_a_batch_equals_its_samples_one_at_a_time(key, B):
    """Per-sample layouts: bitwise (bound 1e-13); no padding lane contributes."""
    mesh, plane = MESHES[key]
    solver = ElasticFESolver(mesh, 1.0, NU, plane=plane, device=DEV)
    n, d, m, nc0 = mesh.n_nodes, mesh.dim, mesh.n_elements, _nc0(mesh.dim, plane)
    u = _rand((B, n, d), 1, -1e-2, 1e-2).requires_grad_(True)
    E = _rand((B, m), 2, 0.5, 2.0).requires_grad_(True)
    z = _rand((B, m, nc0), 3, -1e-2, 1e-2).requires_grad_(True)
    F0 = solver.eigenstrain_load(z, E)
    sig, vm = solver.stress_and_von_mises(u, E, eigenstrain=z)
    w_f, w_s, w_v = _rand(F0.shape, 4, -1, 1), _rand(sig.shape, 5, -1, 1), _rand(vm.shape, 6, -1, 1)
    g_load = torch.autograd.grad((w_f * F0).sum(), (z, E))
    g_str = torch.autograd.grad((w_s * sig).sum() + (w_v * vm).sum(), (u, E, z))
    one_load = [torch.zeros_like(t) for t in g_load]
    one_str = [torch.zeros_like(t) for t in g_str]
    F1 = torch.zeros_like(F0)
    for b in range(B):
        ub, Eb, zb = (t[b].detach().requires_grad_(True) for t in (u, E, z))
        Fb = solver.eigenstrain_load(zb, Eb)
        F1[b] = Fb.detach()
        for acc, g in zip(one_load, torch.autograd.grad((w_f[b] * Fb).sum(), (zb, Eb))):
            acc[b] = g
        sb, vb = solver.stress_and_von_mises(ub, Eb, eigenstrain=zb)
        for acc, g in zip(one_str, torch.autograd.grad((w_s[b] * sb).sum() + (w_v[b] * vb).sum(), (ub, Eb, zb))):
            acc[b] = g
    errs = [rel_err(F0.detach(), F1)] + [rel_err(a, b) for a, b in zip((*g_load, *g_str), (*one_load, *one_str))]
    print(f"{key} B={B}: batch against single samples: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-13
    assert torch.equal(F0.detach(), F1) and all(torch.equal(a, b) for a, b in zip((*g_load, *g_str), (*one_load, *one_str)))
    # the sums of one tensor / one modulus per sample see no padding lane either; a (B, 1) modulus shows the batch, so
    # that (70, nc0) next to it is one tensor per sample on the mesh of 70 elements too
    zs, Es = _rand((B, nc0), 7, -1e-2, 1e-2).requires_grad_(True), _rand((B, 1), 8, 0.5, 2.0).requires_grad_(True)
    gz, ge = torch.autograd.grad((w_f * solver.eigenstrain_load(zs, Es)).sum(), (zs, Es))
    assert gz.shape == (B, nc0) and ge.shape == (B, 1)
    for b in (0, B - 1):
        zb, Eb = zs[b].detach().requires_grad_(True), Es[b, 0].detach().requires_grad_(True)
        gzb, geb = torch.autograd.grad((w_f[b] * solver.eigenstrain_load(zb, Eb)).sum(), (zb, Eb))
        assert rel_err(gz[b], gzb) <= 1e-13 and abs(float(ge[b, 0] - geb)) <= 1e-13 * float(ge.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2d-84", "3d"])
@pytest.mark.parametrize("B", [3, 70])
def test_shared_field_gradients_are_reproducible_and_the_sum_over_the_batch(key, B):
    mesh, plane = MESHES[key]
    solver = ElasticFESolver(mesh, 1.0, NU, plane=plane, device=DEV)
    n, d, m, nc0 = mesh.n_nodes, mesh.dim, mesh.n_elements, _nc0(mesh.dim, plane)
    u = _rand((B, n, d), 1, -1e-2, 1e-2)
    zb = _rand((B, m, nc0), 3, -1e-2, 1e-2)
    E = _rand((m,), 2, 0.5, 2.0)                             # m is 84 and 90: an (m,) field also next to B = 70
    w_f, w_v = _rand((B, n, d), 4, -1, 1), _rand((B, m), 5, -1, 1)

    def grads(Ein, zin):
        Ein, zin = Ein.clone().requires_grad_(True), zin.clone().requires_grad_(True)
        L = (w_f * solver.eigenstrain_load(zin, Ein)).sum() + (w_v * solver.von_mises(u, Ein, eigenstrain=zin)).sum()
        return torch.autograd.grad(L, (Ein, zin))

    (e1, _), (e2, _) = grads(E, zb), grads(E, zb)
    assert e1.shape == (m,) and torch.equal(e1, e2)
    per_sample, _ = grads(E[None].expand(B, m), zb)
    err = rel_err(e1, per_sample.sum(0))
    # a field of eps0 the batch shares: the torch reduction of the kernel's per-sample array
    z_shared = zb[0]
    Eb = _rand((B, m), 6, 0.5, 2.0)
    (_, z1), (_, z2) = grads(Eb, z_shared), grads(Eb, z_shared)
    _, z_per = grads(Eb, z_shared[None].expand(B, m, nc0))
    err_z = rel_err(z1, z_per.sum(0))
    print(f"{key} B={B}: shared-field dE against the summed per-sample field {err:.2e}, d eps0 {err_z:.2e}")
    assert z1.shape == (m, nc0) and torch.equal(z1, z2)
    assert err <= 1e-11 and err_z <= 1e-11


# ------------------------------------------------------------------------------------------------
# GPU: through the solve
# ------------------------------------------------------------------------------------------------
def _roller_problem(key):
    """Left side: x clamped (a roller), one node also in y (and z), one dof with a non-zero prescribed value."""
    mesh, plane = MESHES[key]
    n, d = mesh.n_nodes, mesh.dim
    X = mesh.nodes
    left = [i for i in range(n) if float(X[i, 0]) < 0.1]
    fixed = {(i, 0): 0.0 for i in left}
    fixed.update({(left[0], a): 0.0 for a in range(1, d)})
    if d == 3:
        fixed[(left[-1], 2)] = 0.0
        fixed[(left[-1], 1)] = 0.0
    right = int(X[:, 0].argmax())
    fixed[(right, 1)] = 2e-3                                    # a prescribed displacement: through the lift
    return mesh, plane, fixed


@pytest.mark.gpu
@pytest.mark.parametrize("key,B,zkind", [("2d-strain", 3, "sample_field"), ("2d-stress", 3, "field"), ("3d", 3, "sample_field"),
                                         ("2d-strain", None, "field"), ("2d-stress", 70, "sample")])
def test_solve_with_eigenstrain_matches_the_dense_solve_and_its_autograd(key, B, zkind):
    mesh, plane, fixed = _roller_problem(key)
    n, d, m, nc0, Bo = mesh.n_nodes, mesh.dim, mesh.n_elements, _nc0(mesh.dim, plane), B or 1
    E0 = _rand((Bo, m) if B else (m,), 1, 0.5, 2.0)
    E_map = (lambda t: t) if B else (lambda t: t[None])
    z0, z_map = _eigenstrain(zkind, _reads(zkind, "sample_elem", Bo, m, "sample", True)[0], Bo, m, nc0)
    z_map = _expanded(z_map, Bo)
    f0, load0 = _rand((Bo, n, d) if B else (n, d), 2, -1e-2, 1e-2), _rand((n, d), 3, -1e-3, 1e-3)
    f_map = (lambda t: t) if B else (lambda t: t[None])
    w = _rand((Bo, n, d), 4, -1, 1)

    M = _load_map(mesh)

    def dense(E, z, f, load):
        rhs = load[None] + _oracle_load(mesh, E_map(E), z_map(z), NU, plane) + M @ f_map(f)
        return _dense_solve(mesh, E_map(E), NU, plane, fixed, rhs)

    leaves = [t.clone().requires_grad_(True) for t in (E0, z0, f0, load0)]
    u_d = dense(*leaves)
    want = torch.autograd.grad((w * u_d).sum(), leaves)
    E, z, f, load = (t.clone().requires_grad_(True) for t in (E0, z0, f0, load0))
    solver = ElasticFESolver(mesh, E, NU, plane=plane, fixed=fixed, device=DEV, tol=1e-13)
    u = solver(f, load, eigenstrain=z)
    assert u.shape == ((Bo, n, d) if B else (n, d)) and solver.last_info.not_converged == 0
    got = torch.autograd.grad((w.reshape(u.shape) * u).sum(), (E, z, f, load))
    errs = [rel_err(u.detach().reshape(Bo, n, d), u_d.detach())] + [rel_err(a, b) for a, b in zip(got, want)]
    print(f"{key} B={B} {zkind}: rel_err u, dE, d eps0, df, dload: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-10
    # the E gradient holds both paths: through K(E) and through F0(E)
    Ed = E0.clone().requires_grad_(True)
    solver_d = ElasticFESolver(mesh, Ed, NU, plane=plane, fixed=fixed, device=DEV, tol=1e-13)
    F0 = solver_d.eigenstrain_load(z0, Ed.detach())
    u_pre = solver_d(f0, load0 + F0)
    assert rel_err(u_pre.detach(), u.detach()) <= 1e-10                              # the same solve ...
    g_pre, = torch.autograd.grad((w.reshape(u_pre.shape) * u_pre).sum(), (Ed,))
    assert rel_err(g_pre, want[0]) > 1e-3                                            # ... but one path of dE missing


@pytest.mark.gpu
@pytest.mark.parametrize("zkind", ["tensor", "node"])
def test_solve_with_eigenstrain_in_node_layout(zkind):
    """layout="node", f and load (n, d, B): one eps0 for everything with a shared E -- a load no sample distinguishes, (n, d, 1),
    expanded to the batch of f -- and a field per sample, (nc0, m, B)."""
    mesh, plane, fixed = _roller_problem("2d-strain")
    n, d, m, nc0, B = mesh.n_nodes, mesh.dim, mesh.n_elements, 4, 3
    E0 = _rand((m,), 1, 0.5, 2.0)
    z0, z_map = _eigenstrain(zkind, zkind, B, m, nc0)
    z_map = _expanded(z_map, B)
    f0, load0 = _rand((n, d, B), 2, -1e-2, 1e-2), _rand((n, d, B), 3, -1e-3, 1e-3)
    w = _rand((n, d, B), 4, -1, 1)
    M = _load_map(mesh)
    leaves = [t.clone().requires_grad_(True) for t in (E0, z0, f0, load0)]
    E_bm = leaves[0][None].expand(B, m)
    rhs = leaves[3].permute(2, 0, 1) + _oracle_load(mesh, E_bm, z_map(leaves[1]), NU, plane) + M @ leaves[2].permute(2, 0, 1)
    u_d = _dense_solve(mesh, E_bm, NU, plane, fixed, rhs).permute(1, 2, 0)
    want = torch.autograd.grad((w * u_d).sum(), leaves)
    E, z, f, load = (t.clone().requires_grad_(True) for t in (E0, z0, f0, load0))
    solver = ElasticFESolver(mesh, E, NU, plane=plane, fixed=fixed, device=DEV, tol=1e-13)
    u = solver(f, load, layout="node", eigenstrain=z)
    assert u.shape == (n, d, B) and solver.last_info.not_converged == 0
    got = torch.autograd.grad((w * u).sum(), (E, z, f, load))
    errs = [rel_err(u.detach(), u_d.detach())] + [rel_err(a, b) for a, b in zip(got, want)]
    print(f"node layout {zkind}: rel_err u, dE, d eps0, df, dload: " + " ".join(f"{e:.2e}" for e in errs))
    assert all(a.shape == b.shape for a, b in zip(got, want)) and max(errs) <= 1e-10
    u_only = solver(load=None, f=None, layout="node", eigenstrain=z0) if zkind == "node" else None   # eps0 carries the batch
    assert u_only is None or u_only.shape == (n, d, B)


@pytest.mark.gpu
def test_backward_works_after_the_caller_dropped_the_solver():
    """The graph of the two eigenstrain ops keeps their solver alive (the handle registry holds it weakly)."""
    import gc
    mesh, plane = MESHES["2d-strain"]
    n, m = mesh.n_nodes, mesh.n_elements
    z, E = _rand((m, 4), 1, -1e-2, 1e-2).requires_grad_(True), _rand((m,), 2, 0.5, 2.0).requires_grad_(True)
    u = _rand((n, 2), 3, -1e-2, 1e-2)
    F0 = ElasticFESolver(mesh, 1.0, NU, plane=plane, device=DEV).eigenstrain_load(z, E)
    vm = ElasticFESolver(mesh, 1.0, NU, plane=plane, device=DEV).von_mises(u, E, eigenstrain=z)
    gc.collect()
    dz, de = torch.autograd.grad(F0.sum() + vm.sum(), (z, E))
    want = torch.autograd.grad(_oracle_load(mesh, E[None], z[None], NU, plane).sum()
                               + _oracle_stress(mesh, u[None], E[None], z[None], NU, plane)[2].sum(), (z, E))
    assert rel_err(dz, want[0]) <= 1e-12 and rel_err(de, want[1]) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("design", ["h", "E"])
def test_example_checks_its_gradient_and_lowers_the_thermal_stress(design):
    import importlib.util
    spec = importlib.util.spec_from_file_location("thermal_stress", os.path.join(ROOT, "examples", "thermal_stress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    first, last, fd_err = mod.run(ny=8, steps=10, design=design, verbose=False)
    print(f"example {design}: pnorm(vm) " + " ".join(f"{float(a):.3e}->{float(b):.3e}" for a, b in zip(first, last))
          + f"  central difference {fd_err:.1e}")
    assert fd_err < 1e-5 and bool((last < first).all())


def _solved_closed_form(key, eps0, fixed, E):
    mesh, plane = MESHES[key]
    solver = ElasticFESolver(mesh, E, NU, plane=plane, fixed=fixed, device=DEV, tol=1e-13, max_iter=4000)
    u = solver(eigenstrain=eps0)
    return solver, u


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2d-stress", "2d-strain", "3d"])
def test_closed_form_compatible_eigenstrain_on_the_gpu(key):
    """u = eps0 x, sigma = 0, vm = 0 in every element; the zero-vm elements give finite, zero gradients."""
    mesh, plane, eps0, u_exact = _compatible(*MESHES[key])
    m = mesh.n_elements
    E = _rand((m,), 2, 0.5, 2.0)
    solver, u = _solved_closed_form(key, eps0, _rigid_fixed(mesh, u_exact), E)
    scale = float(eps0.abs().max())
    err_u = rel_err(u, u_exact)
    sig, vm = solver.stress_and_von_mises(u, eigenstrain=eps0)
    print(f"{key}: compatible eigenstrain: rel_err u {err_u:.2e} max |sigma| / |eps0| {float(sig.abs().max()) / scale:.2e}")
    assert err_u <= 1e-10 and float(sig.abs().max()) <= 1e-10 * scale and float(vm.abs().max()) <= 1e-10 * scale
    # exactly stress-free input: vm == 0, its gradients finite and zero
    ue, Ee, ze = u_exact.clone().requires_grad_(True), E.clone().requires_grad_(True), eps0.clone().requires_grad_(True)
    zero, z0 = torch.zeros_like(ue, requires_grad=True), torch.zeros_like(eps0, requires_grad=True)
    vm0 = solver.von_mises(zero, Ee, eigenstrain=z0)
    assert bool((vm0 == 0).all())
    grads = torch.autograd.grad((_rand(vm0.shape, 1, 0.5, 1.0) * vm0).sum(), (zero, Ee, z0))
    assert all(bool(torch.isfinite(g).all()) and bool((g == 0).all()) for g in grads)
    vm1 = solver.von_mises(ue, Ee, eigenstrain=ze)                                  # stress-free up to rounding
    grads = torch.autograd.grad(vm1.sum(), (ue, Ee, ze))
    assert all(bool(torch.isfinite(g).all()) for g in grads)


@pytest.mark.gpu
def test_closed_form_plane_strain_free_expansion_on_the_gpu():
    mesh, plane = MESHES["2d-strain"]
    m, a = mesh.n_elements, 3e-3
    E = _rand((m,), 2, 0.5, 2.0)
    eps0 = a * torch.tensor([1.0, 1.0, 0.0, 1.0], dtype=T64)
    u_exact = (1 + NU) * a * mesh.nodes.to(T64)
    solver, u = _solved_closed_form("2d-strain", eps0, _rigid_fixed(mesh, u_exact), E)
    sig, vm = solver.stress_and_von_mises(u, eigenstrain=eps0)
    err_u, err_vm = rel_err(u, u_exact), rel_err(vm, E * a)
    print(f"plane strain free expansion: rel_err u {err_u:.2e} vm = |sigma_zz| {err_vm:.2e}")
    assert err_u <= 1e-10 and float(sig.abs().max()) <= 1e-10 * a and err_vm <= 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2d-stress", "2d-strain", "3d"])
def test_closed_form_fully_clamped_on_the_gpu(key):
    mesh, plane = MESHES[key]
    n, d, m, a = mesh.n_nodes, mesh.dim, mesh.n_elements, 2e-3
    E = _rand((m,), 2, 0.5, 2.0)
    eps0 = elastic.thermal_strain(a, torch.ones(m, dtype=T64), d, plane)
    fixed = {(i, c): 0.0 for i in range(n) for c in range(d)}
    solver, u = _solved_closed_form(key, eps0, fixed, E)
    sig, vm = solver.stress_and_von_mises(u, eigenstrain=eps0)
    want, want_zz = _clamped_stress(d, plane, E, a)
    assert float(u.abs().max()) == 0.0
    assert rel_err(sig[:, :d], want[:, None].expand(m, d)) <= 1e-12 and float(sig[:, d:].abs().max()) <= 1e-12 * a
    want_vm = (want - want_zz).abs() if plane == "strain" else (want.abs() if d == 2 else torch.zeros(m, dtype=T64))
    assert float((vm - want_vm).abs().max()) <= 1e-12 * a


@pytest.mark.gpu
def test_chain_from_conductivity_to_the_thermal_von_mises_pnorm():
    """kappa -> T (DifferentiableFESolver) -> element_mean -> thermal_strain -> elastic solve -> pnorm(von_mises):
    dL/dkappa against a dense autograd restatement of the whole chain."""
    heat_mesh = FEMesh.rectangle(7, 5)
    mesh = FEMesh(nodes=heat_mesh.nodes, elements=heat_mesh.elements, dirichlet_nodes={})
    plane, alpha, p = "stress", 1e-3, 6.0
    n, m = mesh.n_nodes, mesh.n_elements
    X, el = mesh.nodes.to(T64), mesh.elements.long()
    left = [i for i in range(n) if float(X[i, 0]) == 0.0]
    fixed = {(i, a): 0.0 for i in left for a in range(2)}
    kappa0, E0 = _rand((m,), 1, 0.5, 2.0), _rand((m,), 2, 0.5, 2.0)
    q = 1.0 + _rand((n,), 3)

    # dense: the heat solve K(kappa) T = M q with T = 0 on the mesh's Dirichlet nodes
    kd = kappa0.clone().requires_grad_(True)
    G, vol = _geometry(X, el)
    ke = vol[:, None, None] * torch.einsum("mpa,mqa->mpq", G, G)
    K = torch.zeros(n * n, dtype=T64).index_add(0, (el[:, :, None] * n + el[:, None, :]).reshape(-1),
                                                 (kd[:, None, None] * ke).reshape(-1)).reshape(n, n)
    mass = _load_map(mesh)
    bc =np.array(sorted(heat_mesh.dirichlet_nodes), dtype=np.int64)
    assert all(float(v) == 0.0 for v in heat_mesh.dirichlet_nodes.values())
    free = torch.from_numpy(np.setdiff1d(np.arange(n), bc))
    T_d = torch.zeros(n, dtype=T64).index_add(0, free, torch.linalg.solve(K[free][:, free], (mass @ q)[free]))
    z_d = elastic.thermal_strain(alpha, elastic.element_mean(T_d, mesh), 2, plane)
    u_d = _dense_solve(mesh, E0[None], NU, plane, fixed, _oracle_load(mesh, E0[None], z_d[None], NU, plane))
    J_d = elastic.pnorm(_oracle_stress(mesh, u_d, E0[None], z_d[None], NU, plane)[2][0], p)
    g_d, = torch.autograd.grad(J_d, (kd,))
    # the package
    kappa = kappa0.clone().requires_grad_(True)
    heat = DifferentiableFESolver(heat_mesh, kappa, device=DEV, tol=1e-13)
    T = heat(q)
    z = elastic.thermal_strain(alpha, elastic.element_mean(T, mesh), 2, plane)
    solver = ElasticFESolver(mesh, E0, NU, plane=plane, fixed=fixed, device=DEV, tol=1e-13)
    u = solver(eigenstrain=z)
    J = elastic.pnorm(solver.von_mises(u, eigenstrain=z), p)
    g, = torch.autograd.grad(J, (kappa,))
    eT, eJ, eg = rel_err(T.detach().cpu(), T_d.detach()), abs(float(J.detach()) - float(J_d.detach())) / float(J_d.detach()), rel_err(g.cpu(), g_d)
    print(f"chain: rel_err T {eT:.2e} J {eJ:.2e} dJ/dkappa {eg:.2e}")
    assert eT <= 1e-10 and eJ <= 1e-10 and eg <= 1e-10
