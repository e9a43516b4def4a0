#!/usr/bin/env python3
"""Shape optimisation of a cantilever on the HIP solve path (needs an MI355X): taper a beam of fixed area so that it is
as stiff as possible under several load cases, or so that its peak von Mises stress is as low as possible.

The beam is `FEMesh.rectangle(4 N, N)` on [0, 4] x [-1/2, 1/2], clamped at x = 0.  Its height profile h(x; theta) is
piecewise linear in K = 5 control heights, and the node coordinates are plain torch of them,

    X_i = (x_i, eta_i h(x_i; theta)),      eta_i in [-1/2, 1/2] the reference ordinate of node i,

with theta rescaled so that the area, summed by torch over the triangles of the moved mesh, stays what it was.  Three
load cases run as ONE batch (a tip force at mid-height, one at the top corner, a pressure along the top edge).
`ShapeElasticFESolver` returns dL/dX from the one adjoint solve of the batch (and, behind --stress, the explicit
dependence of the stress on X on top of it); autograd carries it through X(theta) to the five parameters.  The update is
a multiplicative gradient step with backtracking, so that the objective falls in every iteration.  Every new theta is a
new mesh: a new plan, dof system and multigrid hierarchy ("Elastic shape derivative", has their cost).

    python examples/elastic_shape_optimisation.py [N] [iterations] [--stress]

Objective: the summed compliance sum_b load_b . u_b, or with --stress the summed p-norm (p = 8) of the von Mises stress.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
import torch  # noqa: E402
from diffhe import FEMesh, ShapeElasticFESolver  # noqa: E402
from diffhe.elastic import pnorm  # noqa: E402

T64 = torch.float64
LENGTH, CONTROLS = 4.0, 5


def reference(N):
    """The reference beam: (mesh of 4 N x N quads, x (n,), eta (n,), the clamped dofs, loads (3, n, 2))."""
    mesh = FEMesh.rectangle(4 * N, N, x_range=(0.0, LENGTH), y_range=(-0.5, 0.5))
    x, eta = mesh.nodes[:, 0].to(T64), mesh.nodes[:, 1].to(T64)
    n = mesh.n_nodes
    fixed = {(i, a): 0.0 for i in torch.nonzero(x == 0.0).flatten().tolist() for a in range(2)}
    tip = torch.nonzero(x == LENGTH).flatten()
    top = torch.nonzero(eta == 0.5).flatten()
    loads = torch.zeros(3, n, 2, dtype=T64)
    loads[0, tip[len(tip) // 2], 1] = -1.0                      # tip force at mid-height
    loads[1, tip[-1], 1] = -1.0                                 # tip force at the top corner
    loads[2, top, 1] = -1.0 / len(top)                          # pressure along the top edge
    return mesh, x, eta, fixed, loads


def area_of(X, elements):
    P = X[elements]
    a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    return 0.5 * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).abs().sum()


def nodes_of(theta, x, eta, elements, area0):
    """X(theta) at the area `area0`: the profile is linear in theta and so is the area, so one rescaling fixes it."""
    s = x / LENGTH * (CONTROLS - 1)
    k = s.floor().clamp(max=CONTROLS - 2).long()
    t = s - k
    height = lambda th: (1 - t) * th[k] + t * th[k + 1]  # noqa: E731
    raw = torch.stack([x, eta * height(theta)], 1)
    theta = theta * (area0 / area_of(raw, elements))
    return torch.stack([x, eta * height(theta)], 1)


def optimise(size=16, iters=20, objective="compliance", device="cuda", step=0.08, verbose=True):
    """-> [(objective, area)] of the start and of every accepted iterate."""
    mesh, x, eta, fixed, loads = reference(size)
    elements = mesh.elements.long()
    area0 = float(area_of(mesh.nodes.to(T64), elements))
    loads_dev = loads.to(device)

    def evaluate(theta, grad):
        theta = theta.clone().requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            X = nodes_of(theta, x, eta, elements, area0)
            moved = FEMesh(nodes=X, elements=mesh.elements, dirichlet_nodes={})
            solver = ShapeElasticFESolver(moved, 1.0, 0.3, fixed=fixed, device=device, tol=1e-11)
            u = solver(None, loads_dev)
            if objective == "stress":
                value = pnorm(solver.von_mises(u), 8.0).sum()
            else:
                value = (loads_dev * u).sum()
            if grad:
                value.backward()
        return float(value), float(area_of(X.detach(), elements)), theta.grad

    theta = torch.ones(CONTROLS, dtype=T64)
    value, area, g = evaluate(theta, True)
    history = [(value, area)]
    if verbose:
        print(f"it   0  {objective} {value:.6e}  area {area:.12f}")
    for it in range(1, iters + 1):
        direction = g / g.abs().max().clamp(min=1e-300)         # g . theta = 0: the area constraint undoes a scaling
        trial_step = step
        for _ in range(8):                                      # backtracking: accept the first step that lowers the objective
            trial = theta * torch.exp(-trial_step * direction)
            trial_value, trial_area, _ = evaluate(trial, False)
            if trial_value < value:
                break
            trial_step *= 0.5
        else:
            break
        theta = trial
        value, area, g = evaluate(theta, True)
        history.append((value, area))
        if verbose:
            print(f"it {it:3d}  {objective} {value:.6e}  area {area:.12f}  theta "
                  + " ".join(f"{v:.3f}" for v in theta.tolist()))
    return history


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    N = int(args[0]) if len(args) > 0 else 16
    iterations = int(args[1]) if len(args) > 1 else 20
    optimise(N, iterations, "stress" if "--stress" in sys.argv else "compliance")
