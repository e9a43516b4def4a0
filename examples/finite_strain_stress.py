#!/usr/bin/env python3
"""True stress in a bent cantilever, and a modulus layout that lowers it (needs an MI355X).

The cantilever of examples/large_deflection.py (plane strain, clamped on the left, a dead shear load on its tip), all load
levels as ONE batch.

Part 1 prints, per load level, the peak and the p-norm (p = 8) of the von Mises stress three ways: the linear analysis
(`ElasticFESolver` solve and `von_mises`), the small-strain `von_mises` formula applied to the Neo-Hookean displacement
-- wrong by O(|grad u|): the rigid rotation of the tip half reads as strain -- and the Cauchy von Mises stress of the
Neo-Hookean solve, `HyperelasticFESolver.cauchy_von_mises`: the stress in the deformed body.  The linear analysis grows in
proportion to the load; the true stress grows more slowly, because the bent beam shortens the lever arm of the dead load
(with the defaults, at the largest load: peak 3.09e-2 against 3.20e-2), and the small-strain formula on the bent shape
overshoots it by 47 % there (4.54e-2).

Part 2 takes a few Adam steps on a two-zone modulus -- root half and tip half, the mean of the two held at 1 -- that
minimise the p-norm of the Cauchy von Mises stress summed over the load levels:

    E -> HyperelasticFESolver -> cauchy_von_mises -> pnorm

is one differentiable chain with one adjoint solve per step.  In the linear theory the stress of this statically
determinate beam does not depend on E at all; here it does, through the deformed shape: the steps soften the root half
(the beam bends more and the lever arm shortens further), and the sum of the p-norms falls from 3.998e-2 to 3.821e-2 in
the 8 default steps with E = (0.47, 1.53).

    python examples/finite_strain_stress.py [--nx 48] [--ny 4] [--steps 8]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch  # noqa: E402
from diffhe import ElasticFESolver, HyperelasticFESolver  # noqa: E402
from diffhe.elastic import pnorm  # noqa: E402
from large_deflection import LOADS, cantilever, zones  # noqa: E402

T64 = torch.float64
P = 8.0


def main(steps=8, nx=48, ny=4, device="cuda:0", verbose=True):
    """-> (rows of part 1: (load, peak and p-norm linear, small-strain formula on the Neo-Hookean u, Cauchy), the objective
    of every step of part 2, the final (E_root, E_tip))."""
    dev = torch.device(device)
    mesh, tip = cantilever(nx, ny)
    n, B = mesh.n_nodes, len(LOADS)
    load = torch.zeros(B, n, 2, dtype=T64, device=dev)
    load[:, tip.to(dev), 1] = -torch.tensor(LOADS, dtype=T64, device=dev)[:, None] / len(tip)
    one = torch.ones(2, dtype=T64, device=dev)

    # 1. the stress over the load sweep, three ways
    with torch.no_grad():
        E = zones(mesh, one)
        hyper = HyperelasticFESolver(mesh, E, 0.3, device=dev, steps=2)
        linear = ElasticFESolver(mesh, E, 0.3, plane="strain", device=dev)
        u_h, u_l = hyper(None, load), linear(None, load)
        fields = (linear.von_mises(u_l), linear.von_mises(u_h), hyper.cauchy_von_mises(u_h))
    rows = [(LOADS[k], *(float(v) for vm in fields for v in (vm[k].max(), pnorm(vm[k], P)))) for k in range(B)]
    if verbose:
        print(f"Newton iterations {hyper.last_info.newton_iterations}, min J {hyper.last_info.min_J:.3f}")
        print("   load       linear analysis        small-strain formula     Cauchy (true) stress")
        print("              peak       p-norm      peak       p-norm        peak       p-norm")
        for row in rows:
            print(f"  {row[0]:.2e}  " + "  ".join(f"{v:.4e}" for v in row[1:]))

    # 2. a few steps on the two-zone modulus at a fixed mean
    theta = torch.zeros((), dtype=T64, device=dev, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=0.1)
    history, u = [], None
    for step in range(steps + 1):
        opt.zero_grad()
        t = 0.8 * torch.tanh(theta)                              # E = (1 + t, 1 - t): positive, mean 1
        values = torch.stack([1.0 + t, 1.0 - t])
        solver = HyperelasticFESolver(mesh, zones(mesh, values), 0.3, device=dev, steps=2 if u is None else 1)
        u = solver(None, load) if u is None else solver(None, load, x0=u)
        objective = pnorm(solver.cauchy_von_mises(u), P).sum()
        objective.backward()
        u = u.detach()
        history.append(float(objective.detach()))
        if verbose:
            print(f"  step {step:2d}  sum of p-norms {history[-1]:.6e}  E = {values.detach().tolist()}  "
                  f"dJ/dtheta {float(theta.grad):+.3e}")
        if step < steps:
            opt.step()
    return rows, history, values.detach().tolist()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=48)
    ap.add_argument("--ny", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    main(args.steps, args.nx, args.ny, args.device)
