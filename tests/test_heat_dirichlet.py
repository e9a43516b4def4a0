"""Time-dependent Dirichlet data in diffhe.heat.HeatEquation (`step(u, f, g)`, `forward(u0, n, f, g)`): the Dirichlet rows
hold g(t_k) at every step for backward Euler and Crank-Nicolson, and dL/dg of every step matches a dense time-stepping
restatement."""
import pytest
import torch

from diffhe import FEMesh
from diffhe.heat import HeatEquation
from _util import RTOL_GRAD, RTOL_U
from test_dirichlet_grad import DEV, T64, _dense_solve, _plan_tables, _rel


def _setup(B, K, seed):
    mesh = FEMesh.rectangle(12, 10, bc_value=0.0)
    idx = mesh.dirichlet_index()
    gen = torch.Generator().manual_seed(seed)
    X = mesh.nodes[idx]
    gs = [(torch.sin(3.0 * k * 0.1 + X[:, 0])[None] * (1 + 0.5 * torch.rand(B, 1, generator=gen, dtype=T64))
           + 0.2 * X[:, 1][None]).to(DEV).requires_grad_(True) for k in range(K + 1)]
    u0 = torch.randn(B, mesh.n_nodes, generator=gen, dtype=T64).to(DEV)
    f = (1 + torch.rand(B, mesh.n_nodes, generator=gen, dtype=T64)).to(DEV)
    kappa = torch.tensor([0.8, 1.4][:B], dtype=T64, device=DEV)
    return mesh, idx, gs, u0, f, kappa


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_dirichlet_rows_follow_g(theta):
    B, K, dt = 2, 5, 0.02
    mesh, idx, gs, u0, f, kappa = _setup(B, K, 1)
    heat = HeatEquation(mesh, kappa, dt=dt, theta=theta, device=DEV)
    hist = heat(u0, K, f=f, g=lambda t: gs[round(t / dt)], return_all=True)
    for k in range(K + 1):
        err = _rel(hist[k][:, idx.to(DEV)], gs[k])
        assert err < 1e-14, (k, err)
    # the mesh's own values are untouched and still used without g
    assert set(mesh.dirichlet_nodes.values()) == {0.0}
    u_plain = heat(u0, 1, f=f)
    assert float(u_plain[:, idx.to(DEV)].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_gradient_to_every_step_matches_dense_time_stepping(theta):
    B, K, dt = 2, 4, 0.05
    mesh, idx, gs, u0, f, kappa = _setup(B, K, 2)
    heat = HeatEquation(mesh, kappa, dt=dt, theta=theta, device=DEV)
    gen = torch.Generator().manual_seed(3)
    w1, w2 = (torch.randn(B, mesh.n_nodes, generator=gen, dtype=T64).to(DEV) for _ in range(2))
    hist = heat(u0, K, f=f, g=lambda t: gs[round(t / dt)], return_all=True)
    loss = (w1 * hist[-1]).sum() + (w2 * hist[2]).sum()
    grads = torch.autograd.grad(loss, gs)

    k0, m0, el, mass = _plan_tables(heat.solver)
    c = 1.0 / (theta * dt)
    gc = [g.detach().cpu().clone().requires_grad_(True) for g in gs]
    k_be = kappa.cpu()[:, None].expand(B, mesh.n_elements)
    u = u0.cpu().index_copy(1, idx, gc[0])
    dense = [u]
    for k in range(K):
        load = c * mass * u
        if theta == 1.0:
            u = _dense_solve(k0, m0, el, mass, idx, k_be, f.cpu(), gc[k + 1], load, c)
        else:
            w = _dense_solve(k0, m0, el, mass, idx, k_be, f.cpu(), 0.5 * (u[:, idx] + gc[k + 1]), load, c)
            u = 2.0 * w - u
        dense.append(u)
    assert _rel(hist[-1], dense[-1]) < RTOL_U
    loss_d = (w1.cpu() * dense[-1]).sum() + (w2.cpu() * dense[2]).sum()
    grads_d = torch.autograd.grad(loss_d, gc)
    errs = [_rel(a, b) for a, b in zip(grads, grads_d)]
    print(f"theta={theta}: dL/dg per step {['%.1e' % e for e in errs]}")
    assert max(errs) < RTOL_GRAD, errs
