"""The low half of the CG residual's fp32 pair dropped once the solve nears its energy-rule stop (F_RDROP, then F_RSINGLE:
the default where the pair is carried and that rule is in force) against mg={'resid_drop_lo': 0}
(DIFFHE_PCG_RESID_KEEP_LO), which keeps both halves to the end.  The shapes of test_residual_pair.py, default mg."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from diffhe import FEMesh, DifferentiableFESolver, _hip
from oracle import p1_oracle as orc
from _util import rel_err, RTOL_U, RTOL_GRAD
from test_residual_pair import SHAPES

pytestmark = pytest.mark.gpu
T64 = torch.float64
DEV = "cuda:0"
LOADS = ("ones", "normal", "point")
# The default tol_energy of lattices below 10^5 nodes (1e-11 x 0.1, solver.py _call_options): all three shapes
TOL_ENERGY = 1e-11 * 0.1
# max over the batch of |u_drop - u_keep|_A / |u_keep|_A, MEASURED on an MI355X (the larger of the two batches), per
# shape and load.  Asserted with a factor 10 over the measured value for rounding-order changes, never tighter than
# 2^-48 (one rounding of a split: a measured 0 cannot be held on another compiler) and never looser than
# 0.05 x tol_energy.
#   Iterations 6 ... 9 in these cases, the last 3 or 4 updates of each without a low half (the transition included).
MEASURED = {("smallest", "ones"): 2.203e-15, ("smallest", "normal"): 1.482e-15, ("smallest", "point"): 1.307e-15,
            ("tail", "ones"): 2.955e-15, ("tail", "normal"): 1.527e-15, ("tail", "point"): 1.970e-15,
            ("nonsquare", "ones"): 8.912e-15, ("nonsquare", "normal"): 5.387e-15, ("nonsquare", "point"): 5.499e-15}


def _inputs(shape, B, load):
    nx, ny = SHAPES[shape]
    mesh = FEMesh.rectangle(nx, ny)
    gen = torch.Generator().manual_seed(2000 + 7 * B + nx)
    kappa = 0.5 + 1.5 * torch.rand(B, generator=gen, dtype=T64)
    if load == "ones":
        f = torch.ones(B, mesh.n_nodes, dtype=T64)
    elif load == "normal":
        f = torch.randn(B, mesh.n_nodes, generator=gen, dtype=T64)
    else:   # one loaded node per sample, an interior one, a different one for each sample
        f = torch.zeros(B, mesh.n_nodes, dtype=T64)
        rows = 1 + torch.randint(0, ny - 1, (B,), generator=gen)
        cols = 1 + torch.randint(0, nx - 1, (B,), generator=gen)
        f[torch.arange(B), rows * (nx + 1) + cols] = 1.0
    return mesh, kappa, f


@functools.lru_cache(maxsize=None)
def _oracle(shape, B, load, b):
    mesh, kappa, f = _inputs(shape, B, load)
    bn, bv = np.array(list(mesh.dirichlet_nodes.keys())), np.array(list(mesh.dirichlet_nodes.values()))
    return orc.solve_with_adjoint(mesh.nodes.numpy(), mesh.elements.numpy(), bn, bv, float(kappa[b]), f[b].numpy(),
                                  lambda u_: 2 * u_, sparse=True, refine=1)


@functools.lru_cache(maxsize=None)
def _unit_stiffness(shape):
    """K_1 of the shape's mesh (scipy sparse, every row): u and the differences vanish on the Dirichlet nodes, and the
    RELATIVE energy norm of sample b does not see its scalar kappa_b."""
    nx, ny = SHAPES[shape]
    mesh = FEMesh.rectangle(nx, ny)
    return orc.assemble_sparse(mesh.nodes.numpy(), mesh.elements.numpy(), 1.0, np.zeros(mesh.n_nodes))[0].tocsr()


def _rel_energy(shape, d, u):
    """max over the batch of sqrt(d^T K d / u^T K u); d, u (B, n)."""
    K = _unit_stiffness(shape)
    d, u = d.cpu().numpy().T, u.cpu().numpy().T
    return float(np.sqrt(np.max(np.einsum("ib,ib->b", d, K @ d) / np.einsum("ib,ib->b", u, K @ u))))


def _traffic_reset():
    _hip.lib().diffhe_traffic_account(1, None, None)


def _traffic():
    got = ctypes.c_double()
    _hip.lib().diffhe_traffic_account(0, ctypes.byref(got), None)
    return got.value


def _solve(mesh, kappa, f, **kw):
    mg = kw.pop("mg", {})
    solver = DifferentiableFESolver(mesh, kappa.to(DEV), device=DEV, mg=mg, **kw)
    _traffic_reset()
    u = solver(f.to(DEV))
    return u, solver.last_info, _traffic()


@pytest.mark.parametrize("load", LOADS)
@pytest.mark.parametrize("B", [64, 256])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dropping_the_low_half_against_keeping_it(shape, B, load):
    """Same iterations and stop rules, every sample converged; the default run really dropped (and the other did not);
    the accounted bytes differ by exactly 4 n Bp for the transition update and 8 n Bp for each one after it; u moves by
    no more than ten times what was measured and never more than 0.05 x tol_energy in relative energy norm; both runs
    meet the oracle; the default path is bitwise reproducible."""
    mesh, kappa, f = _inputs(shape, B, load)
    ud0, _, _ = _solve(mesh, kappa, f)
    uk, ik, bytes_k = _solve(mesh, kappa, f, mg=dict(resid_drop_lo=0))
    # counted on the second run of each configuration's plan (the first also accounts the plan's cached copies)
    ud, idr, bytes_d = _solve(mesh, kappa, f)
    diff = _rel_energy(shape, ud - uk, uk)
    print(f"{shape} B={B} {load}: its {idr.iterations} / {ik.iterations}, single updates {idr.resid_single_updates} / "
          f"{ik.resid_single_updates}, rules {idr.stop_rules}, |u_drop - u_keep|_A / |u|_A = {diff:.3e}, est "
          f"{idr.err_est:.2e} / {ik.err_est:.2e}, relres {idr.max_relres:.2e} / {ik.max_relres:.2e}, bytes keep - drop = "
          f"{(bytes_k - bytes_d) / (4.0 * mesh.n_nodes * B):.3f} fp32 vectors")
    assert idr.path == ik.path == "lattice-mgpcg" and idr.tol_energy == ik.tol_energy == TOL_ENERGY
    assert ik.flags & _hip.PCG_RESID_KEEP_LO and not idr.flags & (_hip.PCG_RESID_KEEP_LO | _hip.PCG_RESID_FP64)
    assert "pair of fp32" in idr.precision and "pair of fp32" in ik.precision
    assert "lo is dropped" in idr.precision and "lo is dropped" not in ik.precision
    assert ik.iterations >= 3, "this shape and load cannot tell a run that drops from one that does not"
    assert idr.iterations == ik.iterations and idr.stop_rules == ik.stop_rules
    assert idr.not_converged == ik.not_converged == 0
    assert idr.resid_single_updates >= 1 and ik.resid_single_updates == 0
    assert idr.resid_single_updates < idr.iterations       # the first update of a solve always carries the pair
    nb = mesh.n_nodes * B
    assert bytes_k - bytes_d == 4.0 * nb + 8.0 * nb * (idr.resid_single_updates - 1), (bytes_k, bytes_d)
    assert torch.equal(ud, ud0)
    assert (shape, load) in MEASURED, "no measured value for this case"
    assert diff <= min(max(10 * MEASURED[(shape, load)], 2.0 ** -48), 0.05 * TOL_ENERGY)
    for b in (0, B - 1):
        uo = _oracle(shape, B, load, b)[0]
        ed, ek = rel_err(ud[b].cpu().numpy(), uo), rel_err(uk[b].cpu().numpy(), uo)
        print(f"  sample {b}: vs oracle drop {ed:.2e}, keep {ek:.2e}")
        assert ed < RTOL_U and ek < RTOL_U


@pytest.mark.parametrize("shape", list(SHAPES))
def test_nothing_changes_without_the_energy_rule(shape):
    """An explicit tol switches the energy rule off: no update drops anything and the result is bitwise that of
    resid_drop_lo=0."""
    B = 64
    mesh, kappa, f = _inputs(shape, B, "normal")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)    # "did not reach tol": by construction
        u, info, _ = _solve(mesh, kappa, f, tol=1e-300, max_iter=5, mg=dict(floor=0))
        uk, ik, _ = _solve(mesh, kappa, f, tol=1e-300, max_iter=5, mg=dict(floor=0, resid_drop_lo=0))
    assert info.path == "lattice-mgpcg" and info.tol_energy == 0.0 and info.iterations == ik.iterations == 5
    assert info.resid_single_updates == ik.resid_single_updates == 0
    assert torch.equal(u, uk)


def test_forward_and_backward_at_the_smallest_shape():
    """Default settings, both solves of a step: u, dL/dkappa and dL/df against the oracle at the suite's RTOLs, and both
    solves dropped the low half."""
    B = 64
    mesh, kappa0, f0 = _inputs("smallest", B, "normal")
    kappa = kappa0.clone().to(DEV).requires_grad_(True)
    f = f0.clone().to(DEV).requires_grad_(True)
    solver = DifferentiableFESolver(mesh, kappa, device=DEV)
    u = solver(f)
    (u ** 2).sum().backward()
    info = solver.last_info
    print(f"its {info.iterations} / {info.adj_iterations}, single updates {info.resid_single_updates} / "
          f"{info.adj_resid_single_updates}, rules {info.stop_rules} / {info.adj_stop_rules}")
    assert info.path == "lattice-mgpcg" and info.not_converged == 0
    assert info.resid_single_updates >= 1 and info.adj_resid_single_updates >= 1
    for b in (0, B - 1):
        uo, dk, df = _oracle("smallest", B, "normal", b)
        assert rel_err(u[b].detach().cpu().numpy(), uo) < RTOL_U
        assert rel_err(f.grad[b].cpu().numpy(), df) < RTOL_GRAD
        assert abs(float(kappa.grad[b]) - dk.sum()) < RTOL_GRAD * abs(dk.sum())


def test_the_residual_is_replaced_when_the_energy_rule_runs_out():
    """mg={'trust_its': 6} (development: the energy rule is trusted for 6 iterations, not 10) forces the rare path on a
    solve of 7 iterations whose drop condition holds after the 4th: the low half is dropped, the solve reaches the end
    of the trusted iterations, the residual is recomputed from the iterate as a whole pair, and the residual rule
    finishes the solve.  No update after the replacement drops."""
    B, trust = 64, 6
    mesh, kappa, f = _inputs("tail", B, "normal")
    u, info, _ = _solve(mesh, kappa, f, mg=dict(trust_its=trust))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)    # stopped at the cap on purpose
        _, capped, _ = _solve(mesh, kappa, f, max_iter=trust, mg=dict(trust_its=trust))
    print(f"its {info.iterations}, single updates {info.resid_single_updates} (first {trust} iterations: "
          f"{capped.resid_single_updates}), rules {info.stop_rules}, relres {info.max_relres:.2e}")
    assert info.path == "lattice-mgpcg" and info.not_converged == 0
    assert info.stop_rules == {"cap": 0, "residual": B, "energy": 0}
    assert info.iterations > trust and capped.iterations == trust
    assert 1 <= info.resid_single_updates == capped.resid_single_updates < trust
    for b in (0, B - 1):
        assert rel_err(u[b].cpu().numpy(), _oracle("tail", B, "normal", b)[0]) < RTOL_U
