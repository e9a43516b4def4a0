#!/usr/bin/env python3
"""Fibre angles of a cantilevered ply sized by strength, not by compliance (needs an MI355X).

The ply and the three load cases of examples/laminate_orientation.py, as ONE batch.  That example stops where the
strength question starts: a laminate is sized by a failure criterion in its material axes.  Here the Tsai-Wu index
phi_e = q . sigma_e + sigma_e . Q sigma_e is evaluated per element and load case by
`AnisotropicElasticFESolver.failure_index`, with the criterion turned with the fibres, `diffhe.tsai_wu(..., theta=theta_e)`.
The chain

    theta_e -> C(theta_e), (q, Q)(theta_e) -> solve -> failure_index -> pnorm

is differentiable with ONE adjoint solve per step.  The script first runs the compliance design of the other example for
`--compliance-steps` steps, prints the failure index of that field, then lowers the p-norm of the index (its positive
part, p = 8, summed over the load cases) for `--steps` steps with Adam and prints both designs side by side.

    python examples/laminate_failure.py [--nx 32] [--ny 16] [--compliance-steps 40] [--steps 20]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from diffhe import AnisotropicElasticFESolver, FEMesh, tsai_wu  # noqa: E402
from diffhe.elastic import pnorm  # noqa: E402
from diffhe.elastic_aniso import orthotropic_2d  # noqa: E402
from laminate_orientation import E1, E2, G12, NU12, T64, load_cases, neighbour_pairs  # noqa: E402

XT, XC, YT, YC, S12 = 60.0, 40.0, 3.0, 9.0, 4.0      # strengths along / across the fibres and in shear, in the units of the load


def evaluate(mesh, theta, load, pairs, dev):
    """(compliance (3,), failure index (3, m), smoothing term, solver) of the angle field theta."""
    solver = AnisotropicElasticFESolver(mesh, orthotropic_2d(E1, E2, NU12, G12, theta), device=dev)
    u = solver(None, load)
    phi = solver.failure_index(u, tsai_wu(XT, XC, YT, YC, S12, theta=theta))
    smooth = 1e-3 * ((theta[pairs[:, 0]] - theta[pairs[:, 1]]) ** 2).mean()
    return (load * u).sum(dim=(1, 2)), phi, smooth, solver


def report(name, compliance, phi):
    agg = pnorm(phi.detach().clamp_min(0.0), 8.0)
    print(f"{name:28s} compliance {float(compliance.sum()):8.4f}   max Tsai-Wu index per case "
          + " ".join(f"{float(v):7.4f}" for v in phi.detach().amax(dim=1))
          + f"   p-norm (summed) {float(agg.sum()):7.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=32)
    ap.add_argument("--ny", type=int, default=16)
    ap.add_argument("--compliance-steps", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    dev = torch.device(args.device)

    grid = FEMesh.rectangle(args.nx, args.ny, x_range=(0.0, 2.0))
    left = torch.nonzero(grid.nodes[:, 0] == 0.0).reshape(-1).tolist()
    mesh = FEMesh(nodes=grid.nodes, elements=grid.elements, dirichlet_nodes=dict.fromkeys(left, 0.0))
    load = load_cases(mesh.nodes.to(T64)).to(dev)
    pairs = neighbour_pairs(mesh.elements).to(dev)

    theta = torch.zeros(mesh.n_elements, dtype=T64, device=dev, requires_grad=True)      # all fibres along x
    with torch.no_grad():
        compliance, phi, _, _ = evaluate(mesh, theta, load, pairs, dev)
    report("fibres along x", compliance, phi)

    opt = torch.optim.Adam([theta], lr=0.05)
    for _ in range(args.compliance_steps):
        opt.zero_grad()
        compliance, phi, smooth, _ = evaluate(mesh, theta, load, pairs, dev)
        (compliance.sum() + smooth).backward()
        opt.step()
    with torch.no_grad():
        compliance, phi, _, _ = evaluate(mesh, theta, load, pairs, dev)
    report(f"compliance design ({args.compliance_steps} steps)", compliance, phi)
    start = float(pnorm(phi.clamp_min(0.0), 8.0).sum())

    opt = torch.optim.Adam([theta], lr=0.02)
    for step in range(args.steps):
        opt.zero_grad()
        compliance, phi, smooth, solver = evaluate(mesh, theta, load, pairs, dev)
        (pnorm(phi.clamp_min(0.0), 8.0).sum() + smooth).backward()
        opt.step()
    with torch.no_grad():
        compliance, phi, _, _ = evaluate(mesh, theta, load, pairs, dev)
    report(f"strength design (+{args.steps} steps)", compliance, phi)
    end = float(pnorm(phi.clamp_min(0.0), 8.0).sum())
    info = solver.last_info
    print(f"p-norm of the Tsai-Wu index: {start:.4f} -> {end:.4f} ({end / start:.3f} of the compliance design's); last step "
          f"{info.iterations} + {info.adj_iterations} iterations (one forward, one adjoint solve)")
    assert math.isfinite(end)


if __name__ == "__main__":
    main()
