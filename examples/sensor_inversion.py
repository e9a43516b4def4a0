#!/usr/bin/env python3
"""Recover the film coefficient of a convectively cooled plate from a few dozen thermocouples (needs an MI355X).

The plate of `convective_cooling.py` -- heated inside by a few patterns f_b, losing heat through every boundary edge with
one film coefficient PER EDGE -- but the temperatures are not known at the mesh nodes: `--sensors` thermocouples sit at
scattered coordinates inside the plate.  `PointSampler` locates them once and reads every solved field there; its
transpose carries the residuals of the readings back to the nodes, from where `RobinFESolver` takes dL/dh in its one
adjoint solve.  Adam on log h keeps h positive.

At the end the recovered temperature field is carried to a mesh twice as fine with a second sampler (the nodes of the fine
mesh as points) and compared with a solve on that mesh.

    python examples/sensor_inversion.py [--n 12] [--sensors 40] [--experiments 6] [--steps 300]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from convective_cooling import forcings, plate  # noqa: E402
from diffhe import PointSampler, RobinFESolver  # noqa: E402

T64 = torch.float64


def film(mid):
    return 2.0 + 1.5 * torch.sin(3.0 * mid[:, 0]) * torch.cos(2.0 * mid[:, 1]) + mid[:, 1]


def run(n=12, sensors=40, experiments=6, steps=300, device="cuda:0", verbose=True):
    """-> (first misfit, last misfit, largest relative error of the recovered h, relative error of the transfer)."""
    dev = torch.device(device)
    mesh = plate(n)
    solver = RobinFESolver(mesh, 1.0, device=dev)
    mid = mesh.nodes[solver.facets].mean(1)                         # (n_F, 2) edge midpoints
    f = forcings(mesh.nodes, experiments).to(dev)
    h_true = film(mid).to(dev)
    u_inf = torch.tensor(0.5, dtype=T64, device=dev)
    where = 0.03 + 0.94 * torch.rand(sensors, 2, generator=torch.Generator().manual_seed(0), dtype=T64)
    probe = PointSampler(mesh, where, device=dev)
    with torch.no_grad():
        readings = probe(solver(f, h=h_true, u_inf=u_inf))          # (experiments, sensors)
    if verbose:
        print(f"{sensors} sensors in {mesh.n_elements} elements: {probe.info['touched_nodes']} of {mesh.n_nodes} nodes "
              f"touched, at most {probe.info['candidates_max']} candidates per sensor; {len(h_true)} unknowns, "
              f"{readings.numel()} readings")
    scale = float((readings ** 2).sum())
    log_h = torch.full_like(h_true, math.log(2.0)).requires_grad_(True)
    opt = torch.optim.Adam([log_h], lr=0.05)
    first = last = None
    for step in range(steps + 1):
        opt.zero_grad()
        u = solver(f, h=log_h.exp(), u_inf=u_inf)
        misfit = ((probe(u) - readings) ** 2).sum() / scale
        misfit.backward()
        last = float(misfit.detach())
        first = last if first is None else first
        err = float(((log_h.detach().exp() - h_true) / h_true).abs().max())
        if verbose and (step % 50 == 0 or step == steps):
            print(f"step {step:4d}  misfit {last:.3e}  h error: max {err:.4f} (relative)")
        if step < steps:
            opt.step()
    # the recovered field on a mesh twice as fine, next to a solve there with the true film coefficient
    fine = plate(2 * n)
    fine_solver = RobinFESolver(fine, 1.0, device=dev)
    with torch.no_grad():
        carried = PointSampler(mesh, fine.nodes, device=dev)(solver(f, h=log_h.exp(), u_inf=u_inf))
        direct = fine_solver(forcings(fine.nodes, experiments).to(dev),
                             h=film(fine.nodes[fine_solver.facets].mean(1)).to(dev), u_inf=u_inf)
    transfer = float((carried - direct).abs().max() / direct.abs().max())
    if verbose:
        print(f"carried to the {2 * n} x {2 * n} mesh: {carried.shape[1]} nodes, differs from a solve there by {transfer:.2e} "
              "(relative, max; the discretisation error of the coarse mesh)")
    return first, last, err, transfer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--sensors", type=int, default=40)
    ap.add_argument("--experiments", type=int, default=6)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    run(args.n, args.sensors, args.experiments, args.steps, args.device)


if __name__ == "__main__":
    main()
