#!/usr/bin/env python3
"""Eigenfrequency maximisation on the HIP solve path (needs an MI355X): raise the fundamental frequency of the plate of
examples/cantilever_compliance.py -- 2 x 1, clamped along its left edge, vibrating in its plane -- at a prescribed amount
of material.

Design variable: one density rho in (0, 1) per QUAD (both of its triangles share it), rho = sigmoid(z), filtered by a
3 x 3 mean.  Stiffness is the SIMP modulus E = E_min + (1 - E_min) rho^3, the mass is proportional to rho.
`ElasticEigenSolver` returns the smallest eigenvalues lambda = omega^2 of K(E) phi = lambda M(rho) phi for every design of
the batch; autograd carries d lambda / dE and d lambda / d rho (Hellmann-Feynman, no solve in backward) through both
interpolations to z.  Objective: lambda_1 relative to its starting value.  The volume constraint holds exactly in every
step: a shift c per design, found by bisection, makes the mean of the filtered sigmoid(z + c) the prescribed fraction (the
shift is a constant of the step for autograd, so a step moves material rather than adding it).  Several designs
(different volume fractions) are optimised AT ONCE as one batch; plain Adam; every solve is warm-started with the modes
of the step before.

Spurious local modes.  With E ~ rho^3 and mass ~ rho the stiffness-to-mass ratio of an element falls like rho^2: regions
the optimiser empties become floppy AND heavy for their stiffness, and the lowest "modes" of the model turn into
localised flapping of nearly void material that no real structure has -- the optimiser then chases those instead of the
structure's own frequency (Pedersen 2000; Du and Olhoff 2007).  The remedy used here is the mass interpolation of Du and
Olhoff: below rho = 0.1 the mass goes like c rho^6 (c = 1e5, continuous at 0.1) instead of rho, so that the ratio grows
again as rho -> 0 and void regions carry no low mode.  `--plain` switches it off to show the difference.

    python examples/eigenfrequency_optimisation.py [NY] [steps] [--plain]       the mesh is 2 NY x NY quads
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch  # noqa: E402
from diffhe import ElasticEigenSolver  # noqa: E402
from diffhe.modal import frequency  # noqa: E402
from cantilever_compliance import _filter, cantilever  # noqa: E402

T64 = torch.float64


def mass_density(rho, plain=False):
    """rho, and below 0.1 the sixth-power branch of Du and Olhoff that keeps void regions free of local modes."""
    return rho if plain else torch.where(rho > 0.1, rho, 1e5 * rho ** 6)


def at_volume(z, vol, iters=50):
    """The filtered density of sigmoid(z + c) with the shift c (B, 1, 1) that gives every design its volume fraction."""
    with torch.no_grad():
        lo, hi = torch.full_like(vol, -20.0), torch.full_like(vol, 20.0)
        for _ in range(iters):
            c = 0.5 * (lo + hi)
            over = _filter(torch.sigmoid(z + c.view(-1, 1, 1))).mean(dim=(1, 2)) > vol
            lo, hi = torch.where(over, lo, c), torch.where(over, c, hi)
    return _filter(torch.sigmoid(z + (0.5 * (lo + hi)).view(-1, 1, 1)))


def optimise(ny=16, steps=30, volumes=(0.4, 0.5, 0.6), k=3, e_min=1e-3, nu=0.3, lr=0.05, plain=False, device="cuda",
             verbose=True):
    mesh, fixed, _ = cantilever(ny)
    nx, B, m = 2 * ny, len(volumes), mesh.n_elements
    vol = torch.tensor(volumes, dtype=T64, device=device)
    z = torch.logit(vol).view(B, 1, 1).expand(B, ny, nx).clone().requires_grad_(True)
    per_triangle = lambda x: x.reshape(B, ny * nx, 1).expand(B, ny * nx, 2).reshape(B, m)  # noqa: E731
    opt = torch.optim.Adam([z], lr=lr)
    history, lam0, phi = [], None, None
    t0 = time.perf_counter()
    for it in range(steps + 1):                                # the last pass only evaluates
        rho = at_volume(z, vol)
        solver = ElasticEigenSolver(mesh, per_triangle(e_min + (1.0 - e_min) * rho ** 3),
                                    per_triangle(mass_density(rho, plain)), k, nu=nu, plane="stress", fixed=fixed,
                                    device=device)
        lam, phi = solver(x0=phi)                              # (B, k), (B, k, n, 2): warm start from the last design
        if lam0 is None:
            lam0 = lam[:, 0].detach()
        volume = rho.mean(dim=(1, 2))
        history.append((frequency(lam[:, 0]).detach().cpu(), volume.detach().cpu(), solver.last_info.outer_iterations))
        if verbose and (it % 5 == 0 or it == steps):
            print(f"  step {it:3d}: f_1 " + " ".join(f"{float(v):8.5f}" for v in history[-1][0])
                  + "   volume " + " ".join(f"{float(v):.3f}" for v in history[-1][1])
                  + f"   outer iterations {history[-1][2]}")
        if it == steps:
            break
        opt.zero_grad()
        (-(lam[:, 0] / lam0).sum()).backward()
        opt.step()
    return at_volume(z, vol).detach(), history, time.perf_counter() - t0


if __name__ == "__main__":
    plain = "--plain" in sys.argv
    argv = [a for a in sys.argv[1:] if a != "--plain"]
    ny = int(argv[0]) if len(argv) > 0 else 16
    steps = int(argv[1]) if len(argv) > 1 else 30
    rho, hist, dt = optimise(ny, steps, plain=plain)
    first, last = hist[0], hist[-1]
    rising = min(len(hist) - 1, 10)
    monotone = all(bool((hist[i + 1][0] > hist[i][0]).all()) for i in range(rising))
    print(f"{2 * ny}x{ny} quads, {len(first[0])} designs at once, {steps} Adam steps in {dt:.1f} s; fundamental frequency "
          + ", ".join(f"{float(a):.5f} -> {float(b):.5f}" for a, b in zip(first[0], last[0]))
          + "; volume " + ", ".join(f"{float(a):.3f} -> {float(b):.3f}" for a, b in zip(first[1], last[1]))
          + f"; rising over the first {rising} steps: {monotone}")
    rows = ["".join(" .:-=+*#%@"[min(9, int(10 * float(v)))] for v in row[:: max(1, ny // 32)])
            for row in rho[1].flip(0)[:: max(1, ny // 16)]]
    print("\n".join(rows))
