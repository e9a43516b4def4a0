#!/usr/bin/env python3
"""Thermal-stress design through two coupled solves (needs an MI355X).

A 2 x 1 plate is held at the reference temperature on its left edge, where it is also clamped, and heated through its
right edge by a hot gas: kappa dT/dn + h (T - T_gas) = 0 there (`RobinFESolver`).  The temperature expands the plate,
eps0 = alpha (T - T_ref) I, the clamp resists, and the von Mises stress of the constrained expansion is what a designer
wants small.  The whole chain

    h or E  ->  T (heat solve)  ->  element_mean  ->  thermal_strain  ->  u (elastic solve, eigenstrain=)  ->
    von_mises(u, eigenstrain=)  ->  pnorm

is differentiable end to end with ONE adjoint solve per physical solve.  Several designs run as one batch:

    --design h   the film coefficient per edge of the heated side, (B, n_F): each design keeps its own mean film
                 coefficient exactly (h = mean * n_F * softmax(theta): the heat has to get in) and redistributes it
                 along the edge
    --design E   a Young's modulus per element, E = E_min + (1 - E_min) rho^3, (B, m): each design keeps its own mean
                 density through a quadratic penalty, 10 (mean / target - 1)^2

The objective per design is pnorm(vm, p) / its starting value (plus that penalty).  It is printed per iteration, and one
gradient entry -- with respect to log h of one edge, or to the density parameter of one element -- is checked against a
central difference through both solves.

    python examples/thermal_stress.py [--ny 16] [--steps 30] [--design h] [--p 8]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
import torch  # noqa: E402
from diffhe import ElasticFESolver, FEMesh, RobinFESolver  # noqa: E402
from diffhe.elastic import element_mean, pnorm, thermal_strain  # noqa: E402

T64 = torch.float64
ALPHA, NU, E_MIN = 1e-3, 0.3, 1e-3


def plate(ny):
    """-> (heat mesh: T = 0 on the left edge; elastic mesh: the same triangles; clamped dofs; facets of the right edge)."""
    nx = 2 * ny
    base = FEMesh.rectangle(nx, ny, x_range=(0.0, 2.0))
    left = [r * (nx + 1) for r in range(ny + 1)]
    heat = FEMesh(nodes=base.nodes, elements=base.elements, dirichlet_nodes={i: 0.0 for i in left})
    body = FEMesh(nodes=base.nodes, elements=base.elements, dirichlet_nodes={})
    every = heat.boundary_facets()
    right = torch.nonzero((heat.nodes[every][:, :, 0] > 2.0 - 1e-12).all(dim=1)).reshape(-1)
    return heat, body, {(i, a): 0.0 for i in left for a in range(2)}, right


def run(ny=16, steps=30, design="h", p=8.0, targets=(1.0, 2.0, 4.0), device="cuda:0", verbose=True):
    """-> (objective per design before, after, relative error of the checked gradient entry)."""
    dev = torch.device(device)
    heat_mesh, mesh, fixed, right = plate(ny)
    n, m, B = mesh.n_nodes, mesh.n_elements, len(targets)
    heat = RobinFESolver(heat_mesh, 1.0, facets=right, device=dev, tol=1e-12)
    n_f = heat.n_facets
    no_source = torch.zeros(n, dtype=T64, device=dev)
    target = torch.tensor(targets, dtype=T64, device=dev)
    if design == "h":
        theta = torch.zeros(B, n_f, dtype=T64, device=dev, requires_grad=True)           # uniform start
        fields = lambda th: (target[:, None] * n_f * torch.softmax(th, dim=1),  # noqa: E731
                             torch.ones(B, m, dtype=T64, device=dev))
        penalty = lambda th: 0.0  # noqa: E731
    elif design == "E":
        target = target / (2.0 * target.max())                                            # mean densities <= 0.5
        theta = torch.logit(target)[:, None].expand(B, m).clone().requires_grad_(True)    # logit rho, uniform start
        fields = lambda th: (torch.full((B, n_f), 2.0, dtype=T64, device=dev),  # noqa: E731
                             E_MIN + (1 - E_MIN) * torch.sigmoid(th) ** 3)
        penalty = lambda th: 10.0 * (torch.sigmoid(th).mean(1) / target - 1.0) ** 2  # noqa: E731
    else:
        raise SystemExit(f"unknown design {design!r}")

    def stress_norm(h, E):
        """pnorm of the thermal von Mises stress per design, (B,), of film coefficients (B, n_F) and moduli (B, m)."""
        T = heat(no_source, h=h, u_inf=1.0)                                               # (B, n): T - T_ref
        eps0 = thermal_strain(ALPHA, element_mean(T, mesh), 2, "stress")                  # (B, m, 3)
        solver = ElasticFESolver(mesh, E, NU, plane="stress", fixed=fixed, device=dev, tol=1e-12)
        u = solver(eigenstrain=eps0)
        return pnorm(solver.von_mises(u, eigenstrain=eps0), p), solver

    with torch.no_grad():
        J0, _ = stress_norm(*fields(theta))

    def objective(th):
        J, solver = stress_norm(*fields(th))
        return J / J0 + penalty(th), J, solver

    # One gradient entry against a central difference through both solves: of the film coefficient itself (log h of one
    # edge, which changes the heat that gets in; the softmax parameters only redistribute it and move the objective
    # 1000 times less) or of the density parameter of one element.  The objective is of order one and smooth: a step of
    # 1e-4 leaves a truncation error of order 1e-8, the solves' tolerance of 1e-12 divided by the step another 1e-8
    # absolute, against an entry of order 1e-2 or more -- 1e-6 relative, so the two must agree to 1e-5.
    h0, E0 = (t.detach() for t in fields(theta))
    if design == "h":
        var = h0.log().requires_grad_(True)
        checked = lambda v: (stress_norm(v.exp(), E0)[0] / J0).sum()  # noqa: E731
    else:
        var = theta.detach().clone().requires_grad_(True)
        checked = lambda v: objective(v)[0].sum()  # noqa: E731
    g, = torch.autograd.grad(checked(var), (var,))
    entry, eps = (0, int(g[0].abs().argmax())), 1e-4
    with torch.no_grad():
        bump = torch.zeros_like(var)
        bump[entry] = eps
        fd = float((checked(var + bump) - checked(var - bump)) / (2 * eps))
    fd_err = abs(float(g[entry]) - fd) / max(abs(fd), 1e-300)
    if verbose:
        print(f"gradient entry {entry}: adjoint {float(g[entry]):+.8e}  central difference {fd:+.8e}  rel. error {fd_err:.1e}")
    assert fd_err < 1e-5, "the adjoint gradient does not match the central difference"

    opt = torch.optim.Adam([theta], lr=0.05)
    first = None
    for it in range(steps + 1):
        opt.zero_grad()
        total, J, solver = objective(theta)
        total.sum().backward()
        first = J.detach().clone() if first is None else first
        if verbose:
            info = solver.last_info
            print(f"iteration {it:3d}  objective " + "  ".join(f"{float(v):.4f}" for v in total.detach())
                  + "  pnorm(vm) " + "  ".join(f"{float(v):.4e}" for v in J.detach())
                  + f"  (elastic iterations {info.iterations} + {info.adj_iterations})")
        if it < steps:
            opt.step()
    return first.cpu(), J.detach().cpu(), fd_err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, default=16)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--design", default="h", choices=("h", "E"))
    ap.add_argument("--p", type=float, default=8.0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    first, last, _ = run(args.ny, args.steps, args.design, args.p, device=args.device)
    print("pnorm of the thermal von Mises stress per design: " + "  ".join(f"{float(a):.4e} -> {float(b):.4e}"
                                                                           for a, b in zip(first, last)))


if __name__ == "__main__":
    main()
