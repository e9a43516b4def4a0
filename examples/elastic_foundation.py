#!/usr/bin/env python3
"""Recover the stiffness of the ground under a beam from its surface displacements (needs an MI355X).

A beam (plane stress, no fixed dof anywhere) rests on a Winkler foundation: on every edge of its bottom side
sigma n = -(k_n n n^T + k_t (I - n n^T)) u, with a normal stiffness k_n that varies along the beam -- a soft patch in the
ground -- and a known tangential stiffness k_t.  Three load cases press on its top side as ONE batch: a uniform load, a
load on the left half and a load with a shear part.  The vertical displacements of the top nodes are observed.

`TractionElasticFESolver` returns dL/dk_normal per facet, summed over the three load cases inside the kernel, from the
one adjoint solve of the batch; Adam on log k_n keeps it positive.

    python examples/elastic_foundation.py [--nx 32] [--ny 4] [--steps 300]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
import torch  # noqa: E402
from diffhe import FEMesh, TractionElasticFESolver  # noqa: E402

T64 = torch.float64
LENGTH, HEIGHT = 4.0, 0.5


def beam(nx, ny):
    """The beam without Dirichlet nodes: the ground alone holds it."""
    m = FEMesh.rectangle(nx, ny, x_range=(0.0, LENGTH), y_range=(0.0, HEIGHT))
    return FEMesh(nodes=m.nodes, elements=m.elements, dirichlet_nodes={})


def sides(mesh):
    """Indices into mesh.boundary_facets() of the bottom and the top edges."""
    y = mesh.nodes[mesh.boundary_facets()][:, :, 1]                 # (n_F, 2)
    return torch.nonzero((y == 0.0).all(1)).reshape(-1), torch.nonzero((y == HEIGHT).all(1)).reshape(-1)


def main(steps=300, nx=32, ny=4, device="cuda:0", verbose=True):
    """-> (first misfit, last misfit, largest relative error of the recovered k_n)."""
    dev = torch.device(device)
    mesh = beam(nx, ny)
    bottom, top = sides(mesh)
    solver = TractionElasticFESolver(mesh, 50.0, 0.3, facets=torch.cat([bottom, top]), device=dev)
    nb, n_f = len(bottom), solver.n_facets
    mid = mesh.nodes[solver.facets].mean(1).to(dev)                 # (n_F, 2) edge midpoints, bottom edges first
    x = mid[:, 0] / LENGTH
    on_top = torch.arange(n_f, device=dev) >= nb
    # three load cases on the top side, (B, n_F, 2): uniform, left half, inclined
    t = torch.zeros(3, n_f, 2, dtype=T64, device=dev)
    t[0, :, 1] = -1.0
    t[1, :, 1] = -2.0 * (x < 0.5)
    t[2, :, 0], t[2, :, 1] = 0.3, -1.0 - torch.sin(math.pi * x)
    t *= on_top[None, :, None]
    k_t = 2.0 * (~on_top)                                           # known, (n_F,)
    k_true = (6.0 - 4.0 * torch.exp(-((x[:nb] - 0.6) / 0.15) ** 2))  # a soft patch under the beam
    top_nodes = torch.unique(solver.facets[nb:]).to(dev)

    def k_normal(log_k):
        return torch.cat([log_k.exp(), torch.zeros(n_f - nb, dtype=T64, device=dev)])

    with torch.no_grad():
        data = solver(traction=t, k_normal=k_normal(k_true.log()), k_tangent=k_t)[:, top_nodes, 1]
    scale = float((data ** 2).sum())
    log_k = torch.full_like(k_true, math.log(4.0)).requires_grad_(True)
    opt = torch.optim.Adam([log_k], lr=0.05)
    first = last = err = None
    for step in range(steps + 1):
        opt.zero_grad()
        u = solver(traction=t, k_normal=k_normal(log_k), k_tangent=k_t)
        misfit = ((u[:, top_nodes, 1] - data) ** 2).sum() / scale
        misfit.backward()
        last = float(misfit.detach())
        first = last if first is None else first
        err = float(((log_k.detach().exp() - k_true) / k_true).abs().max())
        if verbose and (step % 25 == 0 or step == steps):
            print(f"step {step:4d}  misfit {last:.3e}  k_n error: max {err:.4f} (relative)  (iterations "
                  f"{solver.last_info.iterations} + {solver.last_info.adj_iterations})")
        if step < steps:
            opt.step()
    return first, last, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=32)
    ap.add_argument("--ny", type=int, default=4)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    main(args.steps, args.nx, args.ny, args.device)
