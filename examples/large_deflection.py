#!/usr/bin/env python3
"""Large deflection of a cantilever: linear against Neo-Hookean, and a modulus recovered from the bent shape (needs an
MI355X).

A slender cantilever (plane strain, clamped on the left) carries a dead shear load on its tip.  Part 1 prints the tip
deflection against the load for `ElasticFESolver(plane="strain")` and `HyperelasticFESolver`, all load levels as ONE
batch: the linear answer grows in proportion to the load, the Neo-Hookean beam stiffens as it bends and shortens.

Part 2 fits a two-zone Young's modulus -- a soft root, a stiff tip half -- to the deflected shape observed at several
load levels, again one batch.  The modulus is one field for the whole batch, so dL/dE is summed over the load
levels inside the kernel, from the one adjoint solve with the final tangent; Adam on the logarithms of the two zone
values keeps them positive.  The linear solver fitted to the same data stops at a larger misfit: the data are not linear
in the load.  With the defaults (60 steps) the Neo-Hookean misfit falls from 1.2e-1 to 2.7e-4 with E = (0.62, 1.04) on the
way to the true (0.6, 1.8) -- the stiff tip half bends little and is slow to identify; more steps bring it on -- and the
linear fit stalls at 2.7e-2.

    python examples/large_deflection.py [--nx 48] [--ny 4] [--steps 60]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
import torch  # noqa: E402
from diffhe import ElasticFESolver, FEMesh, HyperelasticFESolver  # noqa: E402

T64 = torch.float64
LENGTH, HEIGHT = 1.0, 0.1
LOADS = (0.5e-5, 1e-5, 2e-5, 4e-5, 8e-5)             # total tip load per level; E is of order 1


def cantilever(nx, ny):
    m = FEMesh.rectangle(nx, ny, x_range=(0.0, LENGTH), y_range=(0.0, HEIGHT))
    left = torch.nonzero(m.nodes[:, 0] == 0.0).reshape(-1).tolist()
    tip = torch.nonzero(m.nodes[:, 0] == LENGTH).reshape(-1)
    return FEMesh(nodes=m.nodes, elements=m.elements, dirichlet_nodes=dict.fromkeys(left, 0.0)), tip


def zones(mesh, values):
    """(m,) modulus field: values[0] on the root half, values[1] on the tip half."""
    x = mesh.nodes[mesh.elements.long()].mean(1)[:, 0].to(values.device)
    return torch.where(x < 0.5 * LENGTH, values[0], values[1])


def fit(solver_of, mesh, load, data, steps, verbose, label):
    log_e = torch.zeros(2, dtype=T64, device=load.device, requires_grad=True)        # start at E = 1 in both zones
    opt = torch.optim.Adam([log_e], lr=0.1)
    scale = float((data ** 2).sum())
    u, misfit = None, None
    for step in range(steps + 1):
        opt.zero_grad()
        warm = u is not None and label == "neo-hookean"          # Newton starts from the last design's answer
        solver = solver_of(zones(mesh, log_e.exp()), warm)
        u = solver(None, load, x0=u) if warm else solver(None, load)
        misfit = ((u - data) ** 2).sum() / scale
        misfit.backward()
        u = u.detach()
        if verbose and (step % 10 == 0 or step == steps):
            print(f"  {label:12s} step {step:3d}  misfit {float(misfit.detach()):.3e}  E = {log_e.detach().exp().tolist()}")
        if step < steps:
            opt.step()
    return log_e.detach().exp(), float(misfit.detach())


def main(steps=60, nx=48, ny=4, device="cuda:0", verbose=True):
    """-> (tip deflections linear, Neo-Hookean, recovered (E_root, E_tip) by the Neo-Hookean fit, by the linear fit)."""
    dev = torch.device(device)
    mesh, tip = cantilever(nx, ny)
    n, B = mesh.n_nodes, len(LOADS)
    load = torch.zeros(B, n, 2, dtype=T64, device=dev)
    load[:, tip.to(dev), 1] = -torch.tensor(LOADS, dtype=T64, device=dev)[:, None] / len(tip)
    e_true = torch.tensor([0.6, 1.8], dtype=T64, device=dev)
    # two load steps from rest, one from a warm start
    hyper_of = lambda E, warm=False: HyperelasticFESolver(mesh, E, 0.3, device=dev, steps=1 if warm else 2)  # noqa: E731
    linear_of = lambda E, warm=False: ElasticFESolver(mesh, E, 0.3, plane="strain", device=dev)  # noqa: E731

    # 1. tip deflection against load
    with torch.no_grad():
        hyper = hyper_of(zones(mesh, e_true))
        data = hyper(None, load)
        u_lin = linear_of(zones(mesh, e_true))(None, load)
    info = hyper.last_info
    tip_h, tip_l = data[:, tip.to(dev), 1].mean(1), u_lin[:, tip.to(dev), 1].mean(1)
    if verbose:
        print(f"Newton iterations {info.newton_iterations}, {info.linear_iterations} linear iterations, "
              f"{info.backtracks} backtracks, min J {info.min_J:.3f}")
        print("   load      tip deflection / length:  linear   Neo-Hookean")
        for k, P in enumerate(LOADS):
            print(f"  {P:.2e}                         {float(tip_l[k]) / LENGTH:9.4f}   {float(tip_h[k]) / LENGTH:9.4f}")

    # 2. the two-zone modulus from the bent shapes
    e_hyper, m_hyper = fit(hyper_of, mesh, load, data, steps, verbose, "neo-hookean")
    e_linear, m_linear = fit(linear_of, mesh, load, data, steps, verbose, "linear")
    if verbose:
        print(f"true E = {e_true.tolist()}; Neo-Hookean fit {e_hyper.tolist()} (misfit {m_hyper:.2e}); "
              f"linear fit {e_linear.tolist()} (misfit {m_linear:.2e})")
    return tip_l.tolist(), tip_h.tolist(), e_hyper.tolist(), e_linear.tolist()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=48)
    ap.add_argument("--ny", type=int, default=4)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    main(args.steps, args.nx, args.ny, args.device)
