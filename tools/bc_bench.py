#!/usr/bin/env python3
"""ms per fwd + adjoint step with per-sample Dirichlet values (`dirichlet=`, a (B, n_D) tensor requiring grad) against
the same step with the mesh's own values (`solver(f)`), and what the old way costs: a new mesh dict per step, so a new
solve plan per step.

    python tools/bc_bench.py [--steps 5] [--rounds 3] [--cases lat1024,lat1024f,general512,box64] [--rebuild]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bc_bench.py --steps 2 --rounds 1

Step = forward solve + backward of L = sum w u with kappa requiring grad (both variants run the adjoint solve); with
`dirichlet=` the backward also returns dL/dG.  Times: host clock around synchronised steps, the two variants alternated in
one process, best of --rounds rounds of --steps.  --rebuild times one step on a fresh mesh dict (plan build included).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
import torch  # noqa: E402
from diffhe import DifferentiableFESolver, FEMesh  # noqa: E402
from diffhe.tet3d import DifferentiableFESolver3D  # noqa: E402

T64 = torch.float64
DEV = "cuda:0"


def jitter(mesh, amount, seed):
    rng = np.random.default_rng(seed)
    X = mesh.nodes.numpy().copy()
    cells = np.array([len(np.unique(X[:, k])) - 1 for k in range(X.shape[1])])
    move = rng.uniform(-amount, amount, X.shape) / cells
    move[np.array(sorted(mesh.dirichlet_nodes), dtype=np.int64)] = 0.0
    return FEMesh(nodes=torch.from_numpy(X + move), elements=mesh.elements, dirichlet_nodes=dict(mesh.dirichlet_nodes))


# name -> (mesh, solver class, batch, kappa layout, solver options)
CASES = {
    "lat1024": lambda: (FEMesh.rectangle(1024, 1024, bc_value=0.5), DifferentiableFESolver, 256, "sample", {}),
    "lat1024f": lambda: (FEMesh.rectangle(1024, 1024, bc_value=0.5), DifferentiableFESolver, 256, "field", {}),
    "general512": lambda: (jitter(FEMesh.rectangle(512, 512, bc_value=0.5), 0.2, 2), DifferentiableFESolver, 64,
                           "sample", dict(method="ell")),
    "box64": lambda: (FEMesh.box(64, 64, 64, bc_value=0.5), DifferentiableFESolver3D, 64, "sample", {}),
}


def sync():
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="lat1024,lat1024f,general512,box64")
    ap.add_argument("--rebuild", action="store_true")
    args = ap.parse_args()
    for name in args.cases.split(","):
        mesh, cls, B, kmode, opts = CASES[name]()
        n, m, nd = mesh.n_nodes, mesh.n_elements, len(mesh.dirichlet_nodes)
        gen = torch.Generator().manual_seed(0)
        if kmode == "field":
            kappa = (0.5 + torch.rand(B, m, generator=gen, dtype=T64)).to(DEV).requires_grad_(True)
        else:
            kappa = (0.5 + torch.rand(B, generator=gen, dtype=T64)).to(DEV).requires_grad_(True)
        f = torch.ones(B, n, dtype=T64, device=DEV)
        w = torch.randn(B, n, generator=gen, dtype=T64).to(DEV)
        G = (0.5 + 0.1 * torch.randn(B, nd, generator=gen, dtype=T64)).to(DEV).requires_grad_(True)
        solver = cls(mesh, kappa, device=DEV, **opts)
        t0 = time.perf_counter()
        solver._plan()
        sync()
        plan_s = time.perf_counter() - t0

        def step_plain():
            u = solver(f)
            torch.autograd.grad((w * u).sum(), (kappa,))

        def step_bc():
            u = solver(f, dirichlet=G)
            torch.autograd.grad((w * u).sum(), (kappa, G))

        for fn in (step_plain, step_bc):        # warm-up: band lists, caches, allocator
            fn()
        sync()
        best = {"plain": float("inf"), "dirichlet": float("inf")}
        for _ in range(args.rounds):
            for key, fn in (("plain", step_plain), ("dirichlet", step_bc)):
                sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn()
                sync()
                best[key] = min(best[key], (time.perf_counter() - t0) / args.steps * 1e3)
        row = dict(case=name, n=n, B=B, n_dirichlet=nd, band_rows=solver._plan().dirichlet_band()["n_rows"],
                   kappa=kmode, path=solver.last_info.path, plain_ms=round(best["plain"], 3),
                   dirichlet_ms=round(best["dirichlet"], 3),
                   overhead_pct=round(100.0 * (best["dirichlet"] / best["plain"] - 1.0), 2),
                   plan_build_s=round(plan_s, 3))
        if args.rebuild:    # the old way: new values in the mesh dict -> a new plan at every step
            keys = list(mesh.dirichlet_nodes)
            mesh.dirichlet_nodes = {k: 0.25 for k in keys}
            sync()
            t0 = time.perf_counter()
            step_plain()
            sync()
            row["rebuild_step_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        print(json.dumps(row), flush=True)
        del solver, mesh
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
