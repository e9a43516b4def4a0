"""Stress-recovery timing: the kernels of csrc/stress.hip next to diffhe_elast_grad, and the optimisation step of
examples/stress_minimisation.py next to the compliance step.  One process; prints JSON lines.

    python tools/stress_bench.py kernels2d [N] [B]     jittered N x N mesh (default 512, 64)
    python tools/stress_bench.py kernels3d [N] [B]     FEMesh.box(N, N, N) (default 32, 16)
    python tools/stress_bench.py step [NY] [steps]     the 2 NY x NY cantilever of the examples, three designs as a batch
    options: --kernel-reps R (default 20)

kernels*: HIP events around `--kernel-reps` back-to-back launches after two warm-up launches, on random u (n d, Bp),
E (m, Bp) uniform in [0.5, 2] and random cotangents.  Per entry: ms, the algorithmic bytes the entry accounts for
(diffhe_traffic_account) and TB/s of those.  The adjoint is timed whole (element pass writing T and dE, then the node
pass) and as the element pass alone (dE only: no T, no node pass); `diffhe_stress_adjoint` has no node-pass-only form, so
the node pass with the T write is the difference of the two.  `diffhe_elast_grad`, the existing kernel that gathers the
same rows of u (and as many of lambda), runs on the same arrays as the yardstick.
step: forward + loss + backward of (a) J = pnorm(von_mises(u, E = rho^(1/2)), 8) summed over the designs and (b) the
compliance load . u, both with E = rho^3 on the same mesh and batch; host clock around a device synchronise, median.
"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffhe import ElasticFESolver, FEMesh, _hip  # noqa: E402
from diffhe.elastic import lame_unit, pnorm  # noqa: E402
from diffhe.plan import get_plan, _stream  # noqa: E402


def _option(name, default, kind=float):
    if name in sys.argv:
        i = sys.argv.index(name)
        value = kind(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return value
    return default


kernel_reps = _option("--kernel-reps", 20, int)
mode = sys.argv[1] if len(sys.argv) > 1 else "kernels2d"
arg = lambda i, default: int(sys.argv[i]) if len(sys.argv) > i else default  # noqa: E731
dev = torch.device("cuda", 0)
T64 = torch.float64


def bench_mesh(N, dim):
    """Jittered N x N square (interior nodes moved by up to a quarter step) or the N^3 box."""
    m = FEMesh.rectangle(N, N) if dim == 2 else FEMesh.box(N, N, N)
    nodes = m.nodes.numpy().copy()
    if dim == 2:
        rng = np.random.default_rng(0)
        interior = np.all((nodes > 1e-9) & (nodes < 1 - 1e-9), axis=1)
        nodes[interior] += rng.uniform(-0.25 / N, 0.25 / N, (int(interior.sum()), 2))
    return FEMesh(nodes=torch.from_numpy(nodes), elements=m.elements, dirichlet_nodes={})


def kernel_ms(fn):
    """(mean ms over `kernel_reps` back-to-back launches between two events, accounted bytes of one call)."""
    L = _hip.lib()
    fn()
    L.diffhe_traffic_account(1, None, None)
    fn()
    acc = ctypes.c_double(0.0)
    L.diffhe_traffic_account(1, ctypes.byref(acc), None)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(kernel_reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / kernel_reps, acc.value


def kernels(N, dim, B, label):
    mesh = bench_mesh(N, dim)
    d, n, m = mesh.dim, mesh.n_nodes, mesh.n_elements
    nc = d * (d + 1) // 2
    Bp = B
    plan = get_plan(mesh, dev, prune=False)
    L, st = _hip.lib(), _stream(dev)
    lam1, mu1 = lame_unit(0.3, d, "strain" if d == 2 else None)
    nu_z = 0.3
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=T64, device=dev)  # noqa: E731
    new = lambda *shape: torch.empty(*shape, dtype=T64, device=dev)  # noqa: E731
    u, lam = rnd(n * d, Bp), rnd(n * d, Bp)
    E = 0.5 + 1.5 * torch.rand(m, Bp, generator=gen, dtype=T64, device=dev)
    sbar, vbar = rnd(m * nc, Bp), rnd(m, Bp)
    sigma, vm, work, ubar, de, de_s = new(m * nc, Bp), new(m, Bp), new(nc, m, Bp), new(n * d, Bp), new(m, Bp), new(m)
    gtab_raw, vol = plan.gradient_table()
    gtab = plan.oriented_gradient_table()
    inc_ptr, inc = plan.shape_incidence()
    head = (plan.elems, gtab, d, lam1, mu1, nu_z, u, E, Bp, 1)
    cot = (sbar, Bp, nc * Bp, vbar)
    entries = {
        "stress_eval sigma+vm": lambda: L.diffhe_stress_eval(*head, n, m, Bp, sigma, Bp, nc * Bp, vm, st),
        "stress_eval vm only": lambda: L.diffhe_stress_eval(*head, n, m, Bp, None, 0, 0, vm, st),
        "stress_adjoint whole (T, dE, node pass)": lambda: L.diffhe_stress_adjoint(
            *head, *cot, inc_ptr, inc, n, m, B, Bp, work, ubar, de, None, None, st),
        "stress_adjoint element pass alone (dE)": lambda: L.diffhe_stress_adjoint(
            *head, *cot, None, None, n, m, B, Bp, None, None, de, None, None, st),
        "stress_adjoint_shared": lambda: L.diffhe_stress_adjoint_shared(*head, *cot, n, m, B, Bp, de_s, st),
        "elast_grad (yardstick)": lambda: L.diffhe_elast_grad(plan.elems, gtab_raw, vol, d, lam1, mu1, lam, u, None, n, m,
                                                              Bp, de, None, None, st),
        "elast_grad_shared (yardstick)": lambda: L.diffhe_elast_grad_shared(plan.elems, gtab_raw, vol, d, lam1, mu1, lam,
                                                                            u, None, n, m, B, Bp, de_s, st),
    }
    out = dict(tool="stress_bench", mode=label, N=N, n=n, m=m, d=d, B=B, kernel_reps=kernel_reps, kernels={})
    for name, fn in entries.items():
        ms, nbytes = kernel_ms(fn)
        out["kernels"][name] = dict(ms=round(ms, 4), MB=round(nbytes / 1e6, 1), TBps=round(nbytes / (1e9 * ms), 3))
    whole, alone = (out["kernels"][k]["ms"] for k in ("stress_adjoint whole (T, dE, node pass)",
                                                        "stress_adjoint element pass alone (dE)"))
    out["node_pass_and_T_write_ms"] = round(whole - alone, 4)
    print(json.dumps(out), flush=True)


def step(ny, steps):
    from cantilever_compliance import cantilever
    mesh, fixed, tip = cantilever(ny)
    nx, B = 2 * ny, 3
    n, m = mesh.n_nodes, mesh.n_elements
    load = torch.zeros(n, 2, dtype=T64, device=dev)
    load[tip, 1] = -1.0
    gen = torch.Generator(device=dev).manual_seed(0)
    rho = (0.3 + 0.4 * torch.rand(B, ny * nx, generator=gen, dtype=T64, device=dev)).requires_grad_(True)
    per_triangle = lambda q: q.reshape(B, ny * nx, 1).expand(B, ny * nx, 2).reshape(B, m)  # noqa: E731

    def solve():
        rho.grad = None
        solver = ElasticFESolver(mesh, per_triangle(1e-3 + (1 - 1e-3) * rho ** 3), 0.3, plane="stress", fixed=fixed,
                                 device=dev)
        return solver, solver(None, load)

    def step_stress():
        solver, u = solve()
        pnorm(solver.von_mises(u, E=per_triangle(rho.sqrt())), 8.0).sum().backward()
        return solver

    def step_compliance():
        solver, u = solve()
        (u * load).sum().backward()
        return solver

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, s

    out = dict(tool="stress_bench", mode="step", quads=f"{nx}x{ny}", n=n, m=m, B=B, steps=steps)
    sides = {"stress": step_stress, "compliance": step_compliance}
    for fn in sides.values():
        fn()
        fn()
    times = {k: [] for k in sides}
    for r in range(2):
        for k in (("stress", "compliance") if r == 0 else ("compliance", "stress")):
            for _ in range(steps):
                t, s = timed(sides[k])
                times[k].append(t)
            out[k + "_iters"] = (s.last_info.iterations, s.last_info.adj_iterations)
    for k, t in times.items():
        out[k + "_step_ms"] = round(1e3 * statistics.median(t), 2)
    out["stress_over_compliance"] = round(out["stress_step_ms"] / out["compliance_step_ms"], 3)
    print(json.dumps(out), flush=True)


if mode == "kernels2d":
    kernels(arg(2, 512), 2, arg(3, 64), "kernels2d")
elif mode == "kernels3d":
    kernels(arg(2, 32), 3, arg(3, 16), "kernels3d")
elif mode == "step":
    step(arg(2, 32), arg(3, 5))
else:
    raise SystemExit(f"unknown mode {mode!r}")
