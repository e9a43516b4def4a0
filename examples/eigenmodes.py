"""Eigenmodes with diffhe.EigenFESolver.

(a) The first modes of a rectangular membrane against the closed form of the lumped P1 operator,
    lambda_pq = (4 / hx^2) sin^2(p pi hx / 2 Lx) + (4 / hy^2) sin^2(q pi hy / 2 Ly), and the continuum values
    pi^2 (p^2 / Lx^2 + q^2 / Ly^2) they converge to.
(b) A batch of kappa designs optimised with Adam through lam[:, 0]: raise the fundamental eigenvalue of each design under
    a fixed mean kappa (the material budget), every step warm-started from the previous eigenvectors (`x0=phi`).

    python examples/eigenmodes.py [--n 96] [--batch 8] [--steps 30]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "difffe-physics-lab_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from diffhe import EigenFESolver, FEMesh  # noqa: E402


def membrane(n):
    Lx, Ly = 1.5, 1.0
    nx, ny = 3 * n // 2, n
    mesh = FEMesh.rectangle(nx, ny, (0.0, Lx), (0.0, Ly))
    es = EigenFESolver(mesh, 1.0, k=5)
    lam, _ = es()
    hx, hy = Lx / nx, Ly / ny
    pq = sorted(((p, q) for p in range(1, 6) for q in range(1, 6)), key=lambda t: t[0] ** 2 / Lx ** 2 + t[1] ** 2 / Ly ** 2)[:5]
    print(f"(a) membrane {Lx} x {Ly}, {nx} x {ny} cells: {es.last_info.outer_iterations} outer iterations, "
          f"{es.last_info.inner_solves} inner solves ({es.last_info.path})")
    for (p, q), v in zip(pq, lam.cpu().tolist()):
        disc = 4 / hx ** 2 * math.sin(p * math.pi * hx / (2 * Lx)) ** 2 + 4 / hy ** 2 * math.sin(q * math.pi * hy / (2 * Ly)) ** 2
        cont = math.pi ** 2 * (p ** 2 / Lx ** 2 + q ** 2 / Ly ** 2)
        print(f"    mode ({p},{q}): computed {v:.10f}  lumped-P1 closed form {disc:.10f}  continuum {cont:.6f}")


def designs(n, B, steps):
    mesh = FEMesh.rectangle(n, n)
    m = mesh.n_elements
    gen = torch.Generator().manual_seed(0)
    # kappa = budget * m * softmax(theta): positive, mean kappa fixed at `budget` for every design
    theta = (0.05 * torch.randn(B, m, generator=gen, dtype=torch.float64)).cuda().requires_grad_(True)
    budget = torch.linspace(0.8, 1.6, B, dtype=torch.float64).cuda()[:, None]
    opt = torch.optim.Adam([theta], lr=0.05)
    phi = None
    for step in range(steps):
        kappa = budget * m * torch.softmax(theta, dim=1)
        es = EigenFESolver(mesh, kappa, k=2, guard=4, tol=1e-8)
        lam, phi = es(x0=phi)
        loss = -(lam[:, 0] / budget[:, 0]).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        if step % 5 == 0 or step == steps - 1:
            print(f"    step {step:3d}: lambda_1 / budget = {np.array2string((lam[:, 0] / budget[:, 0]).detach().cpu().numpy(), precision=3)}"
                  f"  ({es.last_info.outer_iterations} outer iterations)")
    print(f"(b) uniform kappa would give lambda_1 / budget = {2 * 4 * n * n * math.sin(math.pi / (2 * n)) ** 2:.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=96)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    membrane(a.n)
    print("(b) raising the fundamental eigenvalue under a fixed mean kappa")
    designs(a.n // 2, a.batch, a.steps)
