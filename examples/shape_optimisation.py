#!/usr/bin/env python3
"""r-adaptivity with node gradients (needs an MI355X): move the interior nodes of FEMesh.rectangle(N, N) to minimise
the discrete potential energy Pi(X) = -1/2 F(X)^T u(X) of -lap u = f, u = 0 on the boundary, for a forcing with a sharp
peak.  Pi(X) - Pi = 1/2 |u - u_h|_E^2 (Galerkin), so lowering Pi lowers the energy error; Pi is estimated by a fine
solve (FEMesh.rectangle(512, 512)).  Each step: one solve + adjoint with diffhe.ShapeDifferentiableFESolver, a
projected gradient step (boundary nodes slide along their edge, corners stay), halved until Pi decreases and no
triangle inverts.  A moved mesh builds a new solve plan (cheap at this size).

    python examples/shape_optimisation.py [--n 16] [--steps 10]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
import torch  # noqa: E402
from diffhe import FEMesh, DifferentiableFESolver, ShapeDifferentiableFESolver  # noqa: E402

T64 = torch.float64
PEAK, SIGMA = (0.3, 0.35), 0.05


def forcing(X):
    r2 = (X[:, 0] - PEAK[0]) ** 2 + (X[:, 1] - PEAK[1]) ** 2
    return torch.exp(-r2 / (2 * SIGMA ** 2)) / SIGMA ** 2


def areas(X, el):
    P = X[el]
    return 0.5 * ((P[:, 1, 0] - P[:, 0, 0]) * (P[:, 2, 1] - P[:, 0, 1])
                  - (P[:, 2, 0] - P[:, 0, 0]) * (P[:, 1, 1] - P[:, 0, 1]))


def potential(X, el, bc, solver_cls, device, grad=False):
    """Pi = -1/2 F^T u with F_p = area/3 * mean f (the solver's load map); F is restated here so that autograd sees
    its dependence on X (the solver gives u(X) and its node gradient)."""
    X = X.detach().clone().requires_grad_(grad)
    mesh = FEMesh(nodes=X, elements=el, dirichlet_nodes=bc)
    f = forcing(X)
    u = solver_cls(mesh, 1.0, device=device)(f.to(device)).cpu()
    F_u = (areas(X, el) / 9.0 * f[el].sum(1) * u[el].sum(1)).sum()
    Pi = -0.5 * F_u
    if grad:
        Pi.backward()
        return float(Pi), X.grad
    return float(Pi), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    device = "cuda:0"
    fine = FEMesh.rectangle(512, 512)
    Pi_ref, _ = potential(fine.nodes, fine.elements, fine.dirichlet_nodes, DifferentiableFESolver, device)
    mesh = FEMesh.rectangle(args.n, args.n)
    X, el, bc = mesh.nodes.clone(), mesh.elements, mesh.dirichlet_nodes
    h = 1.0 / args.n
    # projection: x fixed on the edges x = 0, 1; y fixed on y = 0, 1 (corners: both)
    lock = torch.stack([(X[:, 0] <= 0.0) | (X[:, 0] >= 1.0), (X[:, 1] <= 0.0) | (X[:, 1] >= 1.0)], 1)
    Pi, g = potential(X, el, bc, ShapeDifferentiableFESolver, device, grad=True)
    print(f"step  0: Pi = {Pi:.10f}   energy error {Pi - Pi_ref:.6e}")
    step = 0.3 * h
    for k in range(1, args.steps + 1):
        d = torch.where(lock, torch.zeros_like(g), -g)
        d = d / d.norm(dim=1).max()                 # largest move = `step`
        while True:
            Xn = X + step * d
            if bool((areas(Xn, el) > 0).all()):
                Pn, gn = potential(Xn, el, bc, ShapeDifferentiableFESolver, device, grad=True)
                if Pn < Pi:
                    break
            step *= 0.5
            if step < 1e-8 * h:
                print("no descent step found")
                return
        X, Pi, g = Xn, Pn, gn
        print(f"step {k:2d}: Pi = {Pi:.10f}   energy error {Pi - Pi_ref:.6e}   (largest node move {step:.2e})")
        step = min(2.0 * step, 0.3 * h)


if __name__ == "__main__":
    main()
