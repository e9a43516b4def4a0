"""The density filter (diffhe.filters) next to its yardsticks, one process, sides alternated.  Prints JSON lines.

    python tools/filter_bench.py 2d [N] [B] [reps] [rounds]     jittered N x N triangles, R = 2.5 h     (default 512, 64)
    python tools/filter_bench.py 3d [N] [B] [reps] [rounds]     FEMesh.box(N, N, N), R = 1.5 h         (default 32, 16)
    options: --radius-h r (R in units of h = 1 / N)   --no-solve (skip the ElasticFESolver step)   --max-iter K

(a) the table: build time (second build; the first loads the code objects) next to the plan `ElasticFESolver` builds on the
same mesh, neighbours per row, table bytes; (b) forward and adjoint apply on an element-major (m, B) field, HIP events
around `reps` launches; (c) a sample-major (B, m) field two ways -- through the strides, and a transpose with torch around the
element-major call -- alternated over `rounds`; (d) the yardsticks:
`diffhe_ell_spmv_shared` on the node pattern of the same mesh and batch as time per (stored entry x sample), and a device
copy of x for the ratio of measured time to the algorithmic 16 B per value; (e) one filter forward + adjoint as a share
of the `ElasticFESolver` forward + adjoint step it feeds.
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "difffe-physics-lab_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffhe import DensityFilter, ElasticFESolver, FEMesh, _hip  # noqa: E402
from diffhe.plan import _stream, padded_batch  # noqa: E402


def _option(name, default, kind=float):
    if name in sys.argv:
        i = sys.argv.index(name)
        value = kind(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return value
    return default


def _flag(name):
    if name in sys.argv:
        sys.argv.remove(name)
        return True
    return False


radius_h = _option("--radius-h", None)
max_iter = _option("--max-iter", 3000, int)
no_solve = _flag("--no-solve")
mode = sys.argv[1] if len(sys.argv) > 1 else "2d"
arg = lambda i, default: int(sys.argv[i]) if len(sys.argv) > i else default  # noqa: E731
dev = torch.device("cuda", 0)
T64 = torch.float64
TOOL = "filter_bench"


def clamped_mesh(N, dim):
    """Jittered N x N square (interior nodes moved by up to a quarter step) or the N^3 box; clamped on x = 0."""
    m = FEMesh.rectangle(N, N) if dim == 2 else FEMesh.box(N, N, N)
    nodes = m.nodes.numpy().copy()
    if dim == 2:
        rng = np.random.default_rng(0)
        interior = np.all((nodes > 1e-9) & (nodes < 1 - 1e-9), axis=1)
        nodes[interior] += rng.uniform(-0.25 / N, 0.25 / N, (int(interior.sum()), 2))
    left = np.nonzero(np.isclose(nodes[:, 0], 0.0))[0].tolist()
    return FEMesh(nodes=torch.from_numpy(nodes), elements=m.elements, dirichlet_nodes=dict.fromkeys(left, 0.0))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_ms(fn, reps):
    """Mean over `reps` back-to-back calls between two events, after two warm-up calls."""
    fn()
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def run(N, dim, B, reps, rounds):
    R = (radius_h if radius_h is not None else (2.5 if dim == 2 else 1.5)) / N
    mesh = clamped_mesh(N, dim)
    m, n = mesh.n_elements, mesh.n_nodes
    out = dict(tool=TOOL, mode=mode, N=N, dim=dim, m=m, n=n, B=B, R=R, reps=reps, rounds=rounds)

    # (a) the table next to the solver's plan
    first = timed(lambda: DensityFilter(mesh, R, device=dev))
    filt = DensityFilter(mesh, R, device=dev)
    E = torch.ones(B, m, dtype=T64, device=dev)
    solver = ElasticFESolver(clamped_mesh(N, dim), E, 0.3, device=dev, max_iter=max_iter)
    plan_s = timed(lambda: solver._plan().ensure_ell())
    nn = filt.n_neighbours
    out["table"] = dict(first_build_s=round(first, 3), build_s=round(filt.info["build_seconds"], 4), plan_s=round(plan_s, 3),
                        neighbours=filt.info["neighbours"], per_row=[int(nn.min()), round(float(nn.double().mean()), 2),
                                                                       int(nn.max())],
                        cells=filt.info["cells"], table_MB=round(1e-6 * filt.info["table_bytes"], 2))
    print(json.dumps(out), flush=True)

    # (b) element-major apply, (d) its yardsticks
    gen = torch.Generator(device=dev).manual_seed(0)
    x_nm = torch.rand(m, B, generator=gen, dtype=T64, device=dev)
    x_sm = x_nm.t().contiguous()
    y_nm = torch.empty_like(x_nm)
    fwd = kernel_ms(lambda: filt._apply(x_nm, False, True), reps)
    adj = kernel_ms(lambda: filt._apply(x_nm, True, True), reps)
    copy = kernel_ms(lambda: y_nm.copy_(x_nm), reps)
    plan = solver._plan()
    plan.ensure_ell()
    Bp = padded_batch(B)
    f_nm, F = torch.rand(n, Bp, generator=gen, dtype=T64, device=dev), torch.empty(n, Bp, dtype=T64, device=dev)
    L, st = _hip.lib(), _stream(dev)
    spmv = kernel_ms(lambda: L.diffhe_ell_spmv_shared(plan.Mvals, plan.Mcols, f_nm, None, 1, None, None, F, n, plan.MW, Bp,
                                                      st), reps)
    total = filt.info["neighbours"]
    ka = dict(tool=TOOL, mode=mode + "-apply", forward_ms=round(fwd, 4), adjoint_ms=round(adj, 4), copy_ms=round(copy, 4),
              algorithmic_MB=round(16e-6 * m * B, 2), forward_over_copy=round(fwd / copy, 2),
              adjoint_over_copy=round(adj / copy, 2), spmv_ms=round(spmv, 4), spmv_entries=plan.MW * n, spmv_Bp=Bp,
              ps_per_entry_sample=dict(forward=round(1e9 * fwd / (total * B), 3), adjoint=round(1e9 * adj / (total * B), 3),
                                       spmv=round(1e9 * spmv / (plan.MW * n * Bp), 3)))
    print(json.dumps(ka), flush=True)

    # (c) a sample-major field both ways, alternated; the results must agree bit for bit
    variants = ("strided", "transpose")
    want = filt._apply(x_nm, False, True).t()
    per = {v: [] for v in variants}
    for r in range(rounds):
        for v in (variants if r % 2 == 0 else variants[::-1]):
            assert torch.equal(filt._apply(x_sm, False, False, v), want), v
            per[v].append(kernel_ms(lambda: filt._apply(x_sm, False, False, v), reps))
    print(json.dumps(dict(tool=TOOL, mode=mode + "-sample-major",
                          forward_ms={v: [round(t, 4) for t in ts] for v, ts in per.items()},
                          median_ms={v: round(statistics.median(ts), 4) for v, ts in per.items()})), flush=True)

    # (e) the share of one filter forward + adjoint in the elastic step it feeds
    if no_solve:
        return
    rho = (0.3 + 0.4 * torch.rand(B, m, generator=gen, dtype=T64, device=dev)).requires_grad_(True)
    load = torch.zeros(n, dim, dtype=T64, device=dev)
    load[n - 1, dim - 1] = -1.0

    def step(filtered):
        rho.grad = None
        dens = filt(rho) if filtered else rho
        u = ElasticFESolver(solver.mesh, 1e-3 + (1.0 - 1e-3) * dens ** 3, 0.3, device=dev, max_iter=max_iter)(None, load)
        (u * load).sum().backward()

    t_first = timed(lambda: step(True))
    ts = {k: [] for k in (True, False)}
    for r in range(rounds):
        for k in ((True, False) if r % 2 == 0 else (False, True)):
            ts[k].append(timed(lambda: step(k)))
    pair = kernel_ms(lambda: (filt._apply(x_sm, False, False), filt._apply(x_sm, True, False)), reps)
    print(json.dumps(dict(tool=TOOL, mode=mode + "-share", first_step_s=round(t_first, 2),
                          step_ms_filtered=[round(1e3 * t, 1) for t in ts[True]],
                          step_ms_plain=[round(1e3 * t, 1) for t in ts[False]], filter_pair_ms=round(pair, 4),
                          share=round(pair / (1e3 * statistics.median(ts[True])), 5))), flush=True)


if mode == "2d":
    run(arg(2, 512), 2, arg(3, 64), arg(4, 20), arg(5, 3))
elif mode == "3d":
    run(arg(2, 32), 3, arg(3, 16), arg(4, 20), arg(5, 3))
else:
    raise SystemExit(f"unknown mode {mode!r}")
