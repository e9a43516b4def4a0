#!/usr/bin/env python3
"""3D Poisson on P1 tetrahedra (needs an MI355X): -lap u = 3 pi^2 sin(pi x) sin(pi y) sin(pi z) on the unit cube,
u = 0 on the boundary, solved on FEMesh.box(N, N, N) with diffhe.tet3d.DifferentiableFESolver3D; nodal error against
the exact solution and its ratio per halving of h (second order: ~4), plus dL/dkappa of one scalar kappa.

    python examples/poisson_3d.py
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
import torch  # noqa: E402
from diffhe import FEMesh  # noqa: E402
from diffhe.tet3d import DifferentiableFESolver3D  # noqa: E402


if __name__ == "__main__":
    print("   N     nodes   tetrahedra   max nodal error   ratio   iterations   dL/dkappa (L = sum u^2 h^3)")
    prev = None
    for N in (8, 16, 32):
        mesh = FEMesh.box(N, N, N)
        x = mesh.nodes.cuda()
        exact = torch.sin(math.pi * x[:, 0]) * torch.sin(math.pi * x[:, 1]) * torch.sin(math.pi * x[:, 2])
        kappa = torch.tensor(1.0, dtype=torch.float64, device="cuda", requires_grad=True)
        solver = DifferentiableFESolver3D(mesh, kappa)
        u = solver(3.0 * math.pi ** 2 * exact)
        ((u ** 2).sum() / N ** 3).backward()
        err = float((u.detach() - exact).abs().max())
        ratio = f"{prev / err:5.2f}" if prev else "    -"
        print(f"{N:4d} {mesh.n_nodes:9d} {mesh.n_elements:12d}   {err:15.3e}   {ratio}   {solver.last_info.iterations:10d}"
              f"   {float(kappa.grad):.6f}")
        prev = err
