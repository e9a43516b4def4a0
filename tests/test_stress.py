"""Stress recovery of elastic solves (ElasticFESolver.stress / von_mises / stress_and_von_mises, diffhe.elastic.pnorm,
csrc/stress.hip, include/diffhe_stress.h).

The oracle is a dense torch restatement in STRAIN-DISPLACEMENT form, sigma_e = E_e D(nu, plane) B_e u_e with the Voigt
matrix D and the strain-displacement matrix B_e (engineering shear strains, so that D's shear row gives the tensor
component of the stress), then the von Mises stress from the deviator of the full 3 x 3 tensor -- another formulation than
the kernel's index formula -- differentiated by autograd in fp64 on the CPU.  The CPU tests pin it to closed forms and
check `pnorm`, the third signature table and the host refusals; the GPU tests hold the kernels against it.

Bounds.  Random u of order 1 and E in [0.5, 2]: the largest stress is of the size of the summed terms, so errors are taken
relative to the largest oracle entry (`rel_err`).  Values, dL/du (at most 24 element terms per dof) and per-element
dL/dE (no sum): 1e-12, about 40 fp64 operations per value and no cancellation.  Per-sample and batch-shared totals of
dL/dE sum up to m or B m terms of mixed sign: 1e-11.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from diffhe import ElasticFESolver, FEMesh, _hip
from diffhe import elastic
from _util import RTOL_GRAD, rel_err

T64 = torch.float64
DEV = "cuda:0"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffhe_stress.h")
NU = 0.3


# ------------------------------------------------------------------------------------------------
# the oracle (independent of the product code)
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
    """The Voigt matrix of E = 1 for engineering shear strains."""
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
    """B (m, nc, npe*d): Voigt strains (xx, yy, 2 xy | xx, yy, zz, 2 yz, 2 xz, 2 xy) from the element's dofs p*d + a."""
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


def _oracle(mesh, u, E, nu, plane):
    """u (B, n, d), E (B, m) -> sigma (B, m, nc) in the package's Voigt order, vm (B, m)."""
    X, el = mesh.nodes.to(T64), mesh.elements.long()
    d = X.shape[1]
    B, m = E.shape
    G, _ = _geometry(X, el)
    ue = u[:, el].reshape(B, m, -1)                                   # dofs p*d + a of every element
    strain = torch.einsum("mvk,bmk->bmv", _strain_matrix(G), ue)
    sigma = E[:, :, None] * torch.einsum("vw,bmw->bmv", _voigt_D(nu, d, plane), strain)
    S = torch.zeros(B, m, 3, 3, dtype=T64)
    pairs = [(0, 0), (1, 1), (0, 1)] if d == 2 else [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
    full = []
    for k, (a, t) in enumerate(pairs):
        full.append(((a, t), sigma[..., k]))
        if a != t:
            full.append(((t, a), sigma[..., k]))
    if d == 2 and plane == "strain":                                  # sigma_zz = E lambda (eps_xx + eps_yy)
        full.append(((2, 2), E * (nu / ((1 + nu) * (1 - 2 * nu))) * (strain[..., 0] + strain[..., 1])))
    for (a, t), v in full:
        onehot = torch.zeros(3, 3, dtype=T64)
        onehot[a, t] = 1.0
        S = S + v[..., None, None] * onehot
    dev = S - (S.diagonal(dim1=-2, dim2=-1).sum(-1) / 3.0)[..., None, None] * torch.eye(3, dtype=T64)
    return sigma, torch.sqrt(1.5 * (dev * dev).sum(dim=(-2, -1)))


def _dense_solve(mesh, E_bm, nu, plane, fixed_dofs, load):
    """u (B, n, d) of K(E_b) u = load with u = 0 on `fixed_dofs`, K_e = vol_e E_e B^T D B, differentiable in E_bm."""
    X, el = mesh.nodes.to(T64), mesh.elements.long()
    n, d = X.shape
    m, npe = el.shape
    B = E_bm.shape[0]
    G, vol = _geometry(X, el)
    Bm = _strain_matrix(G)
    k0 = vol[:, None, None] * (Bm.transpose(1, 2) @ _voigt_D(nu, d, plane) @ Bm)
    dof = (el[:, :, None] * d + torch.arange(d)[None, None, :]).reshape(m, npe * d)
    idx = (dof[:, :, None] * (n * d) + dof[:, None, :]).reshape(-1)
    K = torch.zeros(B, (n * d) ** 2, dtype=T64).index_add(1, idx, (E_bm[:, :, None, None] * k0[None]).reshape(B, -1))
    K = K.reshape(B, n * d, n * d)
    free = np.setdiff1d(np.arange(n * d), np.asarray(fixed_dofs))
    uf = torch.linalg.solve(K[:, free][:, :, free], load.reshape(1, n * d)[:, free].expand(B, -1).unsqueeze(2)).squeeze(2)
    u = torch.zeros(B, n * d, dtype=T64)
    u = u.index_add(1, torch.from_numpy(free), uf)
    return u.reshape(B, n, d)


# ------------------------------------------------------------------------------------------------
# meshes and data
# ------------------------------------------------------------------------------------------------
def _jitter(mesh, seed, amount=0.15):
    X = mesh.nodes.to(T64).clone()
    h = min(float(torch.unique(X[:, a]).diff().min()) for a in range(X.shape[1]))
    gen = torch.Generator().manual_seed(seed)
    X += amount * h * (2 * torch.rand(X.shape, generator=gen, dtype=T64) - 1)
    return FEMesh(nodes=X, elements=mesh.elements, dirichlet_nodes={})


def _rand(shape, seed, lo=0.0, hi=1.0):
    return lo + (hi - lo) * torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=T64)


MESHES = {
    "2d-stress": (_jitter(FEMesh.rectangle(7, 5), 0), "stress"),
    "2d-strain": (_jitter(FEMesh.rectangle(7, 5), 0), "strain"),
    "3d": (_jitter(FEMesh.box(3, 3, 2), 1), None),
    "2d-blocks": (_jitter(FEMesh.rectangle(13, 12), 2), "stress"),          # 312 elements: two blocks at Bp = 1
    "2d-84": (_jitter(FEMesh.rectangle(7, 6), 3), "strain"),                # 84 elements: an (m,) field at B = 70
}



def _mixed_orientation(mesh):
    """The mesh with the first two vertices of every other element swapped: clockwise and counter-clockwise triangles."""
    el = mesh.elements.clone()
    el[::2, :2] = el[::2, :2].flip(1)
    return FEMesh(nodes=mesh.nodes, elements=el, dirichlet_nodes={})


MESHES["2d-mixed"] = (_mixed_orientation(MESHES["2d-strain"][0]), "strain")
KINDS = ("scalar", "sample", "elem", "sample_elem", "elem_major")             # the five layouts of E


def _read_as(kind, B, m, layout="sample"):
    """The layout a tensor of `kind`'s shape is read as.  rectangle(7, 5) has 70 elements, so at B = 70 two shapes read
    both ways and the package's documented rules decide (`solver._kappa_layout`): a (70,) vector with a batch of 70 is one
    value per sample, and a square (70, 70) field under layout="node" is element-major.  The oracle follows them."""
    if kind == "elem" and B == m and B > 1:
        return "sample"
    if kind == "sample_elem" and B == m and layout == "node":
        return "elem_major"
    return kind


def _modulus(kind, B, m, layout="sample", seed=5):
    """E in the caller's layout `kind`, and the same field as (B, m) for the oracle (a function of E: autograd passes)."""
    shape = {"scalar": (), "sample": (B,), "elem": (m,), "sample_elem": (B, m), "elem_major": (m, B)}[kind]
    E = _rand(shape, seed, 0.5, 2.0)
    expand = {"scalar": lambda t: t.expand(B, m), "sample": lambda t: t[:, None].expand(B, m),
              "elem": lambda t: t[None, :].expand(B, m), "sample_elem": lambda t: t,
              "elem_major": lambda t: t.t()}[_read_as(kind, B, m, layout)]
    return E, expand


def _cases():
    """(mesh key, B or None for an unbatched u, layout, E kind): every batch width and thread mapping on the small
    meshes, every E layout under both layouts."""
    out = []
    for key in ("2d-stress", "2d-strain", "3d"):
        out += [(key, None, "sample", k) for k in ("scalar", "elem")]
        for B in (3, 70):
            out += [(key, B, "sample", k) for k in KINDS[:4]]
            out += [(key, B, "node", k) for k in KINDS]
    out += [("2d-blocks", None, "sample", k) for k in ("scalar", "elem")]
    out += [("2d-mixed", 3, "sample", "sample_elem"), ("2d-mixed", None, "sample", "elem")]
    return out


def _case_id(c):
    return f"{c[0]}-B{c[1] or '1u'}-{c[2]}-{c[3]}"


def _displacement(mesh, B, layout, seed=7):
    """u in the caller's layout and the map to the oracle's (B, n, d)."""
    n, d = mesh.nodes.shape
    if B is None:
        return _rand((n, d), seed, -1, 1), lambda t: t[None]
    if layout == "node":
        return _rand((n, d, B), seed, -1, 1), lambda t: t.permute(2, 0, 1)
    return _rand((B, n, d), seed, -1, 1), lambda t: t


def _to_caller(sig, vm, B, layout):
    """The oracle's (B, m, nc), (B, m) in the layout the solver returns."""
    if B is None:
        return sig[0], vm[0]
    if layout == "node":
        return sig.permute(1, 2, 0), vm.t()
    return sig, vm


# ------------------------------------------------------------------------------------------------
# CPU: the oracle against closed forms
# ------------------------------------------------------------------------------------------------
CPU_MESHES = {"2d": _jitter(FEMesh.rectangle(4, 3), 3), "3d": _jitter(FEMesh.box(2, 2, 2), 4)}


def _eval_oracle(mesh, u, E0, plane):
    m = mesh.n_elements
    sig, vm = _oracle(mesh, u[None], torch.full((1, m), E0, dtype=T64), NU, plane)
    return sig[0], vm[0]


@pytest.mark.parametrize("plane", ["stress", "strain"])
def test_oracle_uniaxial_tension(plane):
    mesh, E0, s0 = CPU_MESHES["2d"], 2.5, 0.7
    X = mesh.nodes
    if plane == "stress":
        u = torch.stack([s0 * X[:, 0] / E0, -NU * s0 * X[:, 1] / E0], 1)
        vm_exact = s0
    else:       # sigma_yy = 0 with eps_zz = 0: sigma_zz = nu sigma_0
        u = torch.stack([s0 * (1 - NU * NU) * X[:, 0] / E0, -s0 * NU * (1 + NU) * X[:, 1] / E0], 1)
        vm_exact = s0 * math.sqrt(1 - NU + NU * NU)
    sig, vm = _eval_oracle(mesh, u, E0, plane)
    want = torch.tensor([s0, 0.0, 0.0], dtype=T64).expand_as(sig)
    assert float((sig - want).abs().max()) <= 1e-12 * s0
    assert float((vm - vm_exact).abs().max()) <= 1e-12 * s0


@pytest.mark.parametrize("plane", ["stress", "strain"])
def test_oracle_pure_shear(plane):
    mesh, E0, gamma = CPU_MESHES["2d"], 1.7, -0.4
    X = mesh.nodes
    mu = E0 / (2 * (1 + NU))
    sig, vm = _eval_oracle(mesh, torch.stack([gamma * X[:, 1], torch.zeros_like(X[:, 1])], 1), E0, plane)
    want = torch.tensor([0.0, 0.0, mu * gamma], dtype=T64).expand_as(sig)
    assert float((sig - want).abs().max()) <= 1e-12 * abs(mu * gamma)
    assert float((vm - math.sqrt(3.0) * mu * abs(gamma)).abs().max()) <= 1e-12 * abs(mu * gamma)


def test_oracle_hydrostatic_3d():
    mesh, E0, alpha = CPU_MESHES["3d"], 1.3, 0.2
    lam, mu = E0 * NU / ((1 + NU) * (1 - 2 * NU)), E0 / (2 * (1 + NU))
    p = (3 * lam + 2 * mu) * alpha
    sig, vm = _eval_oracle(mesh, alpha * mesh.nodes, E0, None)
    want = torch.tensor([p, p, p, 0.0, 0.0, 0.0], dtype=T64).expand_as(sig)
    assert float((sig - want).abs().max()) <= 1e-12 * p
    assert float(vm.abs().max()) <= 1e-12 * p


@pytest.mark.parametrize("key,plane", [("2d", "stress"), ("2d", "strain"), ("3d", None)])
def test_oracle_rigid_body_motion_is_stress_free(key, plane):
    mesh, E0, omega = CPU_MESHES[key], 2.0, 0.3
    X, d = mesh.nodes, mesh.nodes.shape[1]
    W = torch.zeros(d, d, dtype=T64)
    W[0, 1], W[1, 0] = -omega, omega
    if d == 3:
        W[0, 2], W[2, 0], W[1, 2], W[2, 1] = 0.5 * omega, -0.5 * omega, -0.2 * omega, 0.2 * omega
    sig, vm = _eval_oracle(mesh, X @ W.t() + _rand((d,), 1, -1, 1), E0, plane)
    assert float(sig.abs().max()) <= 1e-12 * E0 * omega and float(vm.abs().max()) <= 1e-12 * E0 * omega


# ------------------------------------------------------------------------------------------------
# CPU: pnorm
# ------------------------------------------------------------------------------------------------
def _naive_pnorm(vm, p, w=None):
    w = torch.ones(vm.shape[-1], dtype=T64) if w is None else w
    return ((w * vm ** p).sum(-1) / w.sum()) ** (1.0 / p)


@pytest.mark.parametrize("p", [2.0, 8.0])
def test_pnorm_equals_the_naive_formula_and_its_gradient(p):
    vm = _rand((4, 37), 0, 0.1, 3.0).requires_grad_(True)
    w = _rand((37,), 1, 0.2, 1.0)
    for weights in (None, w):
        got, want = elastic.pnorm(vm, p, weights), _naive_pnorm(vm, p, weights)
        assert got.shape == (4,) and rel_err(got.detach(), want.detach()) <= 1e-14
        g_got, = torch.autograd.grad(got.sum(), vm)
        g_want, = torch.autograd.grad(want.sum(), vm)
        assert rel_err(g_got, g_want) <= 1e-13
    assert rel_err(elastic.pnorm(vm, p, w).detach(), elastic.pnorm(vm, p).detach()) > 1e-3       # weights honoured
    # node layout: elements first
    assert rel_err(elastic.pnorm(vm.t(), p, w, dim=0).detach(), _naive_pnorm(vm, p, w).detach()) <= 1e-14
    assert elastic.pnorm(vm[0], p).shape == ()


@pytest.mark.parametrize("scale", [1e150, 1e-150])
def test_pnorm_neither_overflows_nor_underflows(scale):
    vm = (scale * _rand((3, 50), 2, 0.5, 1.0)).requires_grad_(True)
    J = elastic.pnorm(vm, 32.0)
    g, = torch.autograd.grad(J.sum(), vm)
    vmax = vm.detach().amax(1)
    assert bool(torch.isfinite(J).all()) and bool(torch.isfinite(g).all())
    assert bool((J.detach() <= vmax * (1 + 1e-14)).all()) and bool((J.detach() >= vmax * 50 ** (-1 / 32.0) * (1 - 1e-14)).all())
    assert rel_err(J.detach() / scale, _naive_pnorm(vm.detach() / scale, 32.0)) <= 1e-13


def test_pnorm_of_a_zero_row_is_zero_with_zero_gradient():
    vm = _rand((3, 20), 3, 0.5, 1.0)
    vm[1] = 0.0
    vm.requires_grad_(True)
    J = elastic.pnorm(vm, 8.0)
    g, = torch.autograd.grad(J.sum(), vm)
    J = J.detach()
    assert float(J[1]) == 0.0 and bool((g[1] == 0).all()) and bool(torch.isfinite(g).all()) and float(J[0]) > 0


# ------------------------------------------------------------------------------------------------
# CPU: the third signature table, host refusals
# ------------------------------------------------------------------------------------------------
BY_VALUE = {"int": _hip._I, "long long": _hip._L, "double": _hip._D}


def _declarations(header):
    """name -> (return type, [(type, is pointer)]) of every diffhe_* function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][A-Za-z_ ]*?\**)\s*\b(diffhe_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = []
        for a in ([] if args.strip() == "void" else args.split(",")):
            m = re.match(r"(.+?)\s*(\*?)\s*\w+$", re.sub(r"\bconst\b", "", a).strip())
            params.append((m.group(1).strip(), bool(m.group(2))))
        out[name] = (" ".join(ret.split()), params)
    return out


def test_third_signature_table_matches_the_third_header():
    decls = _declarations(HEADER)
    assert sorted(decls) == sorted(_hip.STRESS_SIGNATURES) == ["diffhe_stress_adjoint", "diffhe_stress_adjoint_shared",
                                                               "diffhe_stress_eval"]
    assert all(name.startswith("diffhe_stress_") for name in decls)
    assert not set(decls) & (set(_hip.SIGNATURES) | set(_hip.ELASTIC_SIGNATURES))
    assert len(_hip.SIGNATURES) == 64 and len(_hip.ELASTIC_SIGNATURES) == 3
    for name, (ret, params) in decls.items():
        res, argtypes = _hip.STRESS_SIGNATURES[name]
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
        with pytest.raises(_hip.HipExtensionError, match="diffhe_stress_eval"):      # refused on the host: no launch
            L.diffhe_stress_eval(None, None, 2, 1.0, 1.0, 0.0, None, None, 0, 0, 4, 2, 1, None, 0, 0, None, None)


def test_refusals_on_the_host():
    mesh = FEMesh.rectangle(3, 2)
    n, m = mesh.n_nodes, mesh.n_elements
    solver = ElasticFESolver(mesh, torch.ones(2, m, dtype=T64))
    for method in (solver.stress, solver.von_mises, solver.stress_and_von_mises):
        with pytest.raises(ValueError, match=r"\(n, d\) or \(B, n, d\)"):
            method(torch.zeros(n, 3, dtype=T64))
        with pytest.raises(ValueError, match=r"\(n, d\) or \(B, n, d\)"):
            method(torch.zeros(n * 2, dtype=T64))
        with pytest.raises(ValueError, match="layout='node'"):
            method(torch.zeros(2, n, 2, dtype=T64), layout="node")
        with pytest.raises(ValueError, match="layout='node'"):
            method(torch.zeros(n, 2, dtype=T64), layout="node")
        with pytest.raises(ValueError, match="Unknown layout"):
            method(torch.zeros(n, 2, dtype=T64), layout="element")
        with pytest.raises(ValueError, match="batch"):                              # the solver's E has B = 2
            method(torch.zeros(3, n, 2, dtype=T64))
        with pytest.raises(ValueError, match="batch"):
            method(torch.zeros(3, n, 2, dtype=T64), E=torch.ones(4, m, dtype=T64))
        with pytest.raises(ValueError, match="batch"):
            method(torch.zeros(n, 2, 3, dtype=T64), E=torch.ones(4, m, dtype=T64), layout="node")
    with pytest.raises(ValueError, match="p >= 1"):
        elastic.pnorm(torch.ones(3, dtype=T64), 0.5)


# ------------------------------------------------------------------------------------------------
# GPU: values
# ------------------------------------------------------------------------------------------------
def _solver(key, E=1.0):
    mesh, plane = MESHES[key]
    return ElasticFESolver(mesh, E, NU, plane=plane, device=DEV), mesh, plane


@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_stress_and_von_mises_match_the_oracle(case):
    key, B, layout, kind = case
    solver, mesh, plane = _solver(key)
    m, d = mesh.n_elements, mesh.dim
    nc = d * (d + 1) // 2
    Bo = B or 1
    u, u_map = _displacement(mesh, B, layout)
    E, e_map = _modulus(kind, Bo, m, layout)
    want_s, want_v = _to_caller(*_oracle(mesh, u_map(u), e_map(E), NU, plane), B, layout)
    sig, vm = solver.stress(u, E, layout), solver.von_mises(u, E, layout)
    both = solver.stress_and_von_mises(u, E, layout)
    assert sig.shape == want_s.shape == {None: (m, nc), "node": (m, nc, Bo), "sample": (Bo, m, nc)}[B and layout]
    assert vm.shape == want_v.shape and sig.device == u.device and vm.dtype == T64
    es, ev = rel_err(sig, want_s), rel_err(vm, want_v)
    print(f"{_case_id(case)}: rel_err sigma {es:.2e} vm {ev:.2e}")
    assert es <= 1e-12 and ev <= 1e-12
    assert torch.equal(both[0], sig) and torch.equal(both[1], vm)


@pytest.mark.gpu
def test_an_unbatched_u_is_broadcast_to_the_batch_of_E_and_device_inputs_stay_on_the_device():
    solver, mesh, plane = _solver("2d-strain")
    m, n = mesh.n_elements, mesh.n_nodes
    u, E = _rand((n, 2), 1, -1, 1), _rand((3, m), 2, 0.5, 2.0)
    want_s, want_v = _oracle(mesh, u[None].expand(3, n, 2), E, NU, plane)
    sig, vm = solver.stress_and_von_mises(u.to(DEV), E)
    assert sig.shape == (3, m, 3) and sig.device == torch.device(DEV)
    assert rel_err(sig.cpu(), want_s) <= 1e-12 and rel_err(vm.cpu(), want_v) <= 1e-12
    # layout="node" with B == Bp: the kernel's own arrays, no pass in between
    un = _rand((n, 2, 4), 3, -1, 1)
    En = _rand((m, 4), 4, 0.5, 2.0)
    want_s, want_v = _oracle(mesh, un.permute(2, 0, 1), En.t(), NU, plane)
    sig, vm = solver.stress_and_von_mises(un.to(DEV), En.to(DEV), layout="node")
    for t in (sig, vm):         # the whole of its allocation, in order: nothing was sliced or transposed out of a larger one
        assert t.is_contiguous() and t.storage_offset() == 0 and t.untyped_storage().nbytes() == 8 * t.numel()
    assert rel_err(sig.cpu(), want_s.permute(1, 2, 0)) <= 1e-12 and rel_err(vm.cpu(), want_v.t()) <= 1e-12


# ------------------------------------------------------------------------------------------------
# GPU: gradients
# ------------------------------------------------------------------------------------------------
def _losses(sig, vm, w_s, w_v):
    return {"both": (w_s * sig).sum() + (w_v * vm).sum(), "sigma": (w_s * sig).sum(), "vm": (w_v * vm).sum()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_gradients_match_the_oracles_autograd(case):
    """L = sum w_s sigma + sum w_vm vm (both cotangents in one backward), and each term alone."""
    key, B, layout, kind = case
    solver, mesh, plane = _solver(key)
    m = mesh.n_elements
    Bo = B or 1
    u, u_map = _displacement(mesh, B, layout)
    E, e_map = _modulus(kind, Bo, m, layout)
    u.requires_grad_(True)
    E.requires_grad_(True)
    o_sig, o_vm = _to_caller(*_oracle(mesh, u_map(u), e_map(E), NU, plane), B, layout)
    w_s, w_v = _rand(o_sig.shape, 11, -1, 1), _rand(o_vm.shape, 12, -1, 1)
    want = {k: torch.autograd.grad(L, (u, E), retain_graph=True) for k, L in _losses(o_sig, o_vm, w_s, w_v).items()}
    sig, vm = solver.stress_and_von_mises(u, E, layout)
    got = {k: torch.autograd.grad(L, (u, E), retain_graph=True) for k, L in _losses(sig, vm, w_s, w_v).items()}
    got["sigma alone"] = torch.autograd.grad((w_s * solver.stress(u, E, layout)).sum(), (u, E))
    got["vm alone"] = torch.autograd.grad((w_v * solver.von_mises(u, E, layout)).sum(), (u, E))
    want["sigma alone"], want["vm alone"] = want["sigma"], want["vm"]
    bound_e = 1e-12 if _read_as(kind, Bo, m, layout) in ("sample_elem", "elem_major") else 1e-11
    for k in got:
        (du, de), (du0, de0) = got[k], want[k]
        assert du.shape == u.shape and de.shape == E.shape and du.device == u.device and de.device == E.device
        eu, ee = rel_err(du, du0), rel_err(de, de0)
        print(f"{_case_id(case)} {k}: rel_err dL/du {eu:.2e} dL/dE {ee:.2e} (bound {bound_e:g})")
        assert eu <= 1e-12 and ee <= bound_e, k
    # one input alone
    du_only, = torch.autograd.grad((w_s * solver.stress(u, E.detach(), layout)).sum(), (u,))
    de_only, = torch.autograd.grad((w_v * solver.von_mises(u.detach(), E, layout)).sum(), (E,))
    assert rel_err(du_only, want["sigma"][0]) <= 1e-12 and rel_err(de_only, want["vm"][1]) <= bound_e


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2d-strain", "3d"])
@pytest.mark.parametrize("B", [3, 70])
def test_padding_samples_contribute_nothing(key, B):
    """The gradients of a batch equal those of its samples computed one at a time (Bp = 1: no padding at all)."""
    solver, mesh, plane = _solver(key)
    n, d, m = mesh.n_nodes, mesh.dim, mesh.n_elements
    u, E = _rand((B, n, d), 1, -1, 1).requires_grad_(True), _rand((B, m), 2, 0.5, 2.0).requires_grad_(True)
    sig, vm = solver.stress_and_von_mises(u, E)
    w_s, w_v = _rand(sig.shape, 3, -1, 1), _rand(vm.shape, 4, -1, 1)
    du, de = torch.autograd.grad((w_s * sig).sum() + (w_v * vm).sum(), (u, E))
    du1, de1 = torch.zeros_like(du), torch.zeros_like(de)
    for b in range(B):
        ub, Eb = u[b].detach().requires_grad_(True), E[b].detach().requires_grad_(True)
        s1, v1 = solver.stress_and_von_mises(ub, Eb)
        du1[b], de1[b] = torch.autograd.grad((w_s[b] * s1).sum() + (w_v[b] * v1).sum(), (ub, Eb))
    eu, ee = rel_err(du, du1), rel_err(de, de1)
    print(f"{key} B={B}: batch against single samples: dL/du {eu:.2e} dL/dE {ee:.2e}")
    assert eu <= 1e-13 and ee <= 1e-13
    # the sums of a scalar per sample see no padding lane either
    Es = _rand((B,), 5, 0.5, 2.0).requires_grad_(True)
    des, = torch.autograd.grad((w_v * solver.von_mises(u.detach(), Es)).sum(), (Es,))
    des1 = torch.stack([torch.autograd.grad((w_v[b] * solver.von_mises(u[b].detach(), Es[b])).sum(), (Es,))[0][b]
                        for b in range(B)])
    assert rel_err(des, des1) <= 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2d-stress", "2d-strain", "3d"])
def test_zero_stress_has_zero_finite_gradients(key):
    solver, mesh, _ = _solver(key)
    n, d, m = mesh.n_nodes, mesh.dim, mesh.n_elements
    for B, kind in ((None, "elem"), (3, "sample_elem"), (3, "elem"), (70, "sample")):
        shape = (n, d) if B is None else (B, n, d)
        u = torch.zeros(shape, dtype=T64, requires_grad=True)
        E = _modulus(kind, B or 1, m)[0].requires_grad_(True)
        vm = solver.von_mises(u, E)
        assert bool((vm == 0).all())
        du, de = torch.autograd.grad((_rand(vm.shape, 1, 0.5, 1.0) * vm).sum(), (u, E))
        assert bool(torch.isfinite(du).all()) and bool(torch.isfinite(de).all())
        assert bool((du == 0).all()) and bool((de == 0).all())
        sig, vm = solver.stress_and_von_mises(u, E)
        du, de = torch.autograd.grad((_rand(sig.shape, 2, -1, 1) * sig).sum() + vm.sum(), (u, E))
        assert bool(torch.isfinite(du).all()) and bool((de == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2d-84", "3d"])
@pytest.mark.parametrize("B", [3, 70])
def test_shared_field_gradient_is_reproducible_and_the_sum_over_the_batch(key, B):
    solver, mesh, _ = _solver(key)
    n, d, m = mesh.n_nodes, mesh.dim, mesh.n_elements
    u = _rand((B, n, d), 1, -1, 1)
    E = _rand((m,), 2, 0.5, 2.0).requires_grad_(True)
    w_s, w_v = _rand((B, m, d * (d + 1) // 2), 3, -1, 1), _rand((B, m), 4, -1, 1)

    def grad_of(Ein, wrt):
        sig, vm = solver.stress_and_von_mises(u, Ein)
        return torch.autograd.grad((w_s * sig).sum() + (w_v * vm).sum(), (wrt,))[0]

    g1, g2 = grad_of(E, E), grad_of(E, E)
    assert g1.shape == (m,) and torch.equal(g1, g2)
    Eb = E.detach()[None].expand(B, m).clone().requires_grad_(True)
    per_sample = grad_of(Eb, Eb)
    err = rel_err(g1, per_sample.sum(0))
    print(f"{key} B={B}: shared-field dE against the summed per-sample field: {err:.2e}")
    assert err <= 1e-13


@pytest.mark.gpu
def test_an_explicit_E_is_the_one_that_is_used_and_differentiated():
    mesh, plane = MESHES["2d-stress"]
    m, n = mesh.n_elements, mesh.n_nodes
    E_solver = _rand((3, m), 1, 0.5, 2.0).requires_grad_(True)
    E_arg = _rand((3, m), 2, 0.5, 2.0).requires_grad_(True)
    solver = ElasticFESolver(mesh, E_solver, NU, plane=plane, device=DEV)
    u = _rand((3, n, 2), 3, -1, 1)
    want_own, _ = _oracle(mesh, u, E_solver.detach(), NU, plane)
    want_arg, want_vm = _oracle(mesh, u, E_arg, NU, plane)
    assert rel_err(solver.stress(u).detach(), want_own) <= 1e-12
    sig = solver.stress(u, E_arg)
    assert rel_err(sig.detach(), want_arg.detach()) <= 1e-12 and rel_err(sig.detach(), want_own) > 1e-2
    vm = solver.von_mises(u, E=E_arg)
    vm.sum().backward()
    assert E_solver.grad is None
    assert rel_err(E_arg.grad, torch.autograd.grad(want_vm.sum(), (E_arg,))[0]) <= 1e-12
    solver.von_mises(u).sum().backward()                       # E=None: the solver's
    assert E_solver.grad is not None and E_solver.grad.shape == (3, m)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["2d-strain", "3d"])
def test_both_stress_addressings_of_the_entries_agree_bitwise(key):
    """sigma and its cotangent as (nc, m, Bp) and as (m, nc, Bp) through (osc, ose); the vm-only call leaves a stress
    array it is not given alone; the adjoint without dE outputs gives the same u_bar."""
    from diffhe.elastic import lame_unit
    from diffhe.plan import get_plan, _stream
    mesh, plane = MESHES[key]
    dev = torch.device(DEV)
    plan = get_plan(mesh, dev, prune=False)
    d, n, m, B, Bp = mesh.dim, mesh.n_nodes, mesh.n_elements, 3, 4
    nc = d * (d + 1) // 2
    lam1, mu1 = lame_unit(NU, d, plane)
    L, st = _hip.lib(), _stream(dev)
    u, E = _rand((n * d, Bp), 1, -1, 1).to(dev), _rand((m, Bp), 2, 0.5, 2.0).to(dev)
    head = (plan.elems, plan.oriented_gradient_table(), d, lam1, mu1, NU, u, E, Bp, 1)
    new = lambda *shape: torch.full(shape, float("nan"), dtype=T64, device=dev)  # noqa: E731
    s_cm, s_mc, vm, vm_only = new(nc, m, Bp), new(m, nc, Bp), new(m, Bp), new(m, Bp)
    L.diffhe_stress_eval(*head, n, m, Bp, s_cm, m * Bp, Bp, vm, st)
    L.diffhe_stress_eval(*head, n, m, Bp, s_mc, Bp, nc * Bp, None, st)
    L.diffhe_stress_eval(*head, n, m, Bp, None, 0, 0, vm_only, st)
    assert bool(torch.isfinite(s_cm).all()) and torch.equal(s_cm.permute(1, 0, 2), s_mc) and torch.equal(vm, vm_only)
    sbar_mc, vbar = _rand((m, nc, Bp), 3, -1, 1).to(dev), _rand((m, Bp), 4, -1, 1).to(dev)
    sbar_cm = sbar_mc.permute(1, 0, 2).contiguous()
    inc_ptr, inc = plan.shape_incidence()
    outs = []
    for sbar, osc, ose, with_de in ((sbar_mc, Bp, nc * Bp, True), (sbar_cm, m * Bp, Bp, True), (sbar_cm, m * Bp, Bp, False)):
        ubar, de = new(n * d, Bp), new(m, Bp)
        L.diffhe_stress_adjoint(*head, sbar, osc, ose, vbar, inc_ptr, inc, n, m, B, Bp, new(nc, m, Bp), ubar,
                                de if with_de else None, None, None, st)
        outs.append((ubar, de))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[2][0])
    assert bool(torch.isfinite(outs[0][0]).all()) and bool(torch.isfinite(outs[0][1]).all())
    assert bool((outs[0][0][:, B:] == 0).all()) and bool((outs[0][1][:, B:] == 0).all())      # the padding sample


@pytest.mark.gpu
def test_second_order_is_refused():
    solver, mesh, _ = _solver("2d-stress")
    u = _rand((mesh.n_nodes, 2), 1, -1, 1).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="second-order"):
        solver.von_mises(u).sum().backward(create_graph=True)


# ------------------------------------------------------------------------------------------------
# GPU: end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_to_end_pnorm_of_a_solved_cantilever():
    """Measured on the MI355X: see DESIGN section 7, "Stress recovery"."""
    nx, ny, B = 7, 5, 3
    mesh, plane = MESHES["2d-stress"]
    n, m = mesh.n_nodes, mesh.n_elements
    left = [r * (nx + 1) for r in range(ny + 1)]
    fixed = {(i, a): 0.0 for i in left for a in range(2)}
    load = torch.zeros(n, 2, dtype=T64)
    load[(ny // 2) * (nx + 1) + nx, 1] = -1.0
    E0 = _rand((B, m), 9, 0.5, 2.0)
    E = E0.clone().requires_grad_(True)
    solver = ElasticFESolver(mesh, E, NU, plane=plane, fixed=fixed, device=DEV, tol=1e-13)
    u = solver(load=load)
    vm = solver.von_mises(u)
    J = elastic.pnorm(vm, 8).sum()
    J.backward()
    Ed = E0.clone().requires_grad_(True)
    u_d = _dense_solve(mesh, Ed, NU, plane, [i * 2 + a for i, a in fixed], load)
    _, vm_d = _oracle(mesh, u_d, Ed, NU, plane)
    elastic.pnorm(vm_d, 8).sum().backward()
    G, _ = _geometry(mesh.nodes.to(T64), mesh.elements.long())
    h_min = float(1.0 / G.norm(dim=2).max())                   # the smallest height of an element: 1 / |grad phi_p|
    length = float(mesh.nodes[:, 0].max() - mesh.nodes[:, 0].min())
    delta_u = rel_err(u.detach().cpu(), u_d.detach())
    err_vm, err_g = rel_err(vm.detach().cpu(), vm_d.detach()), rel_err(E.grad, Ed.grad)
    print(f"end to end: delta_u {delta_u:.2e} L/h_min {length / h_min:.1f} rel_err vm {err_vm:.2e} dJ/dE {err_g:.2e}")
    assert u.shape == (B, n, 2) and vm.shape == (B, m)
    assert err_vm <= 10 * delta_u * length / h_min + 1e-12
    assert err_g <= RTOL_GRAD * length / h_min
