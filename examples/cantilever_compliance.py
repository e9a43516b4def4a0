#!/usr/bin/env python3
"""Structural topology optimisation on the HIP solve path (needs an MI355X): minimise the compliance of a cantilever
-- a 2 x 1 plate clamped along its left edge, loaded downwards at the middle of its right edge -- the problem users of a
differentiable FE package bring under "topology optimisation (minimise compliance)".  The scalar twin on the heat
equation is examples/topology_optimisation.py.

Design variable: one density rho in [0, 1] per QUAD of `FEMesh.rectangle` (both of its triangles share it), Young's
modulus E_e = E_min + (1 - E_min) rho^p (SIMP, p = 3), volume fraction mean(rho) <= V, plane stress, nu = 0.3.
Objective: the compliance C = load^T u; its gradient with respect to the per-element E is what `ElasticFESolver` returns
through its explicit adjoint (one more solve with the same operator and hierarchy).  Update: optimality criteria with
a density filter (3 x 3 mean), bisection on the volume multiplier.  Several designs (different volume fractions) are
optimised AT ONCE as one batch: E has shape (B, n_elements).

    python examples/cantilever_compliance.py [NY] [iterations]          the mesh is 2 NY x NY quads
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from diffhe import ElasticFESolver, FEMesh  # noqa: E402

T64 = torch.float64


def cantilever(ny):
    """2 x 1 plate, 2 ny x ny quads, no Dirichlet nodes of its own -> (mesh, fixed dofs of the left edge, tip node)."""
    nx = 2 * ny
    mesh = FEMesh.rectangle(nx, ny, x_range=(0.0, 2.0))
    mesh.dirichlet_nodes = {}
    fixed = {(r * (nx + 1), a): 0.0 for r in range(ny + 1) for a in range(2)}
    return mesh, fixed, (ny // 2) * (nx + 1) + nx


def _filter(x):
    return F.avg_pool2d(F.pad(x.unsqueeze(1), (1, 1, 1, 1), mode="replicate"), 3, stride=1).squeeze(1)


def optimise(ny=32, iters=40, volumes=(0.3, 0.4, 0.5), p=3.0, e_min=1e-3, nu=0.3, device="cuda", verbose=True):
    mesh, fixed, tip = cantilever(ny)
    nx, B = 2 * ny, len(volumes)
    vol = torch.tensor(volumes, dtype=T64, device=device).view(B, 1, 1)
    rho = vol.expand(B, ny, nx).clone()                      # uniform start at the volume fraction
    load = torch.zeros(mesh.n_nodes, 2, dtype=T64, device=device)
    load[tip, 1] = -1.0
    history, n_its, missed = [], 0, 0
    t0 = time.perf_counter()
    for it in range(iters):
        rho_f = _filter(rho).requires_grad_(True)
        eq = e_min + (1.0 - e_min) * rho_f ** p                          # (B, ny, nx) per quad
        E = eq.reshape(B, ny * nx, 1).expand(B, ny * nx, 2).reshape(B, 2 * ny * nx)   # both triangles of a quad
        solver = ElasticFESolver(mesh, E, nu, plane="stress", fixed=fixed, device=device)
        u = solver(None, load)                                           # (B, n, 2): one load for every design
        C = (u * load).sum(dim=(1, 2))                                   # compliance
        C.sum().backward()
        dC = _filter(rho_f.grad)                                         # <= 0: more material never hurts
        lo = torch.full((B, 1, 1), 1e-12, dtype=T64, device=device)
        hi = torch.full((B, 1, 1), 1e12, dtype=T64, device=device)
        for _ in range(60):                                              # bisection on the volume multiplier
            mid = torch.sqrt(lo * hi)
            cand = (rho * torch.sqrt((-dC).clamp_min(0) / mid)).clamp(0.0, 1.0)
            cand = torch.minimum(torch.maximum(cand, rho - 0.2), rho + 0.2)
            too_much = cand.mean(dim=(1, 2), keepdim=True) > vol
            lo = torch.where(too_much, mid, lo)
            hi = torch.where(too_much, hi, mid)
        rho = cand.detach()
        history.append(C.detach().cpu())
        n_its += solver.last_info.iterations + solver.last_info.adj_iterations
        missed += solver.last_info.not_converged
        if verbose and (it % 10 == 0 or it == iters - 1):
            print(f"  iteration {it:3d}: compliance " + " ".join(f"{float(c):9.3f}" for c in C)
                  + "   volume " + " ".join(f"{float(v):.3f}" for v in rho.mean(dim=(1, 2))))
    dt = time.perf_counter() - t0
    if verbose:
        print(f"  mean PCG iterations per step (forward + adjoint): {n_its / iters:.1f}; systems that missed the "
              f"tolerance: {missed}")
    return rho, torch.stack(history), dt


if __name__ == "__main__":
    ny = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    rho, hist, dt = optimise(ny, iters)
    print(f"{2 * ny}x{ny} quads, {hist.shape[1]} designs at once, {iters} iterations in {dt:.1f} s "
          f"({iters * hist.shape[1] / dt:.0f} differentiable solves/s); compliance "
          + ", ".join(f"{float(a):.2f} -> {float(b):.2f}" for a, b in zip(hist[0], hist[-1])))
    rows = ["".join(" .:-=+*#%@"[min(9, int(10 * float(v)))] for v in row[:: max(1, ny // 32)])
            for row in rho[1].flip(0)[:: max(1, ny // 16)]]
    print("\n".join(rows))
