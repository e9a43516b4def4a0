"""3D timing: FEMesh.box(N, N, N) (P1 Kuhn tetrahedra, 6 N^3 elements) x B samples through DifferentiableFESolver3D,
with the pruned 7-column stiffness pattern and with the full 15-column one (DIFFHE_TET_PRUNE=0), alternated round by
round in one process.  Two kappa layouts per variant: one scalar per sample (closed box: the factored route, one unit
matrix for the batch) and one per-element field per sample (per-sample matrices).  Prints one JSON line.

    python tools/box3d_bench.py [N] [B] [steps] [rounds]
"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "difffe-physics-lab_amd"))
import torch
from diffhe import FEMesh
from diffhe.tet3d import DifferentiableFESolver3D

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 2
dev = torch.device("cuda", 0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def run_variant(prune):
    os.environ["DIFFHE_TET_PRUNE"] = "1" if prune else "0"
    mesh = FEMesh.box(N, N, N)                       # a fresh mesh object: a fresh plan, built under this setting
    gen = torch.Generator(device=dev).manual_seed(0)
    f = 1 + 0.3 * torch.randn(B, mesh.n_nodes, generator=gen, dtype=torch.float64, device=dev)
    res = {}
    probe = DifferentiableFESolver3D(mesh, 1.0, device=dev)
    res["plan_build_s"], plan = timed(lambda: (probe._plan().ensure_ell(), probe._plan())[1])
    res["W"], res["MW"], res["pruned_entries"] = plan.W, plan.MW, plan.pruned_entries
    kappas = {"sample": 0.5 + 1.5 * torch.rand(B, generator=gen, dtype=torch.float64, device=dev),
              "field": 0.5 + 1.5 * torch.rand(B, mesh.n_elements, generator=gen, dtype=torch.float64, device=dev)}
    for name, k0 in kappas.items():
        kappa = k0.clone().requires_grad_(True)
        s = DifferentiableFESolver3D(mesh, kappa, device=dev)

        def fwd():
            with torch.no_grad():
                return s(f)

        def step():
            kappa.grad = None
            u = s(f)
            (0.5 * (u * u).sum() / B).backward()

        first_fwd, _ = timed(fwd)            # includes the aggregation hierarchy of the plan (first layout only)
        first_step, _ = timed(step)
        tf = [timed(fwd)[0] for _ in range(steps)]
        ts = [timed(step)[0] for _ in range(steps)]
        info = s.last_info
        res[name] = dict(first_fwd_s=round(first_fwd, 3), first_step_s=round(first_step, 3),
                         fwd_ms=round(1e3 * statistics.median(tf), 2), step_ms=round(1e3 * statistics.median(ts), 2),
                         iters=info.iterations, adj_iters=info.adj_iterations, path=info.path, factored=info.factored,
                         max_relres=info.max_relres, not_converged=info.not_converged)
        del s, kappa
    del probe, plan, mesh
    torch.cuda.empty_cache()
    return res


out = {"tool": "box3d_bench", "N": N, "B": B, "nodes": (N + 1) ** 3, "elements": 6 * N ** 3, "steps": steps,
       "rounds": []}
for r in range(rounds):
    order = (True, False) if r % 2 == 0 else (False, True)       # alternate which variant goes first
    out["rounds"].append({("pruned" if p else "full"): run_variant(p) for p in order})
for v in ("pruned", "full"):
    out[v] = {k: {q: statistics.median(rd[v][k][q] for rd in out["rounds"]) for q in ("fwd_ms", "step_ms")}
              for k in ("sample", "field")}
print(json.dumps(out), flush=True)
