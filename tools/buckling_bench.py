"""Linear-buckling timing: every entry of csrc/buckling.hip next to its yardstick on the same arrays, one
`LinearBucklingSolver` call split into inner solves and block kernels, and one forward + backward next to an
`ElasticFESolver` step on the same mesh.  One process; prints JSON lines.

    python tools/buckling_bench.py kernels2d [N] [B]        jittered N x N mesh clamped on the left (default 512, 64)
    python tools/buckling_bench.py kernels3d [N] [B]        FEMesh.box(N, N, N) clamped on x = 0 (default 32, 16)
    python tools/buckling_bench.py solve2d|solve3d [N] [B] [axial|shear]    one call, k = 4 + 4, tol 1e-8
    python tools/buckling_bench.py step2d|step3d [N] [B] [axial|shear]      forward + backward next to an elastic step
    options: --kernel-reps R (default 20)  --rounds K (default 5)  --max-iter I (default 200)

kernels: E (B, m) uniform in [0.5, 2], a random indefinite prestress per sample, random blocks, p = 8.  After two warm-up
launches of every entry, `--rounds` rounds visit all entries in turn -- a new entry and its yardstick alternate in the same
process -- each visit being `--kernel-reps` back-to-back launches between two HIP events; a figure is the median over the
rounds of the mean per launch, with the spread (max - min) between the rounds.  The pairs: `diffhe_buckling_apply` against
`diffhe_ell_apply` on the d x d-block dof pattern of K; gram and rotate against their `diffhe_modal_*` twins under a nodal
mass per sample; `diffhe_buckling_grad_sigma` (k = 4 columns) against `diffhe_elast_grad` (one column).  Every yardstick is
scaled by the ratio of the algorithmic bytes (diffhe_traffic_account; `diffhe_ell_apply` accounts nothing of its own: its
bytes are the operator's values once and the two vectors): `ratio` is time(new) / (time(yardstick) x byte ratio).
solve: the product's run object with a host clock around the set-up, each inner solve, each pair of operator applications
and each Rayleigh-Ritz group, closed by a device synchronise.  The load is a total of 1 on the edge / face opposite the
clamp, along -x (axial) or -y (shear).
step: `lam, _ = solver(load=...)`, `aggregate(lam).sum().backward()` for E (B, m) requiring grad, next to
`ElasticFESolver` with the compliance of the same load, both after one untimed call.
"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffhe import ElasticFESolver, FEMesh, LinearBucklingSolver, _hip  # noqa: E402
from diffhe import buckling  # noqa: E402
from diffhe.elastic import _setup_of  # noqa: E402
from diffhe.plan import _stream  # noqa: E402
from diffhe.solver import K_SAMPLE_ELEM, _Engine  # noqa: E402


def _option(name, default, kind=float):
    if name in sys.argv:
        i = sys.argv.index(name)
        value = kind(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return value
    return default


kernel_reps = _option("--kernel-reps", 20, int)
rounds = _option("--rounds", 5, int)
max_iter = _option("--max-iter", 200, int)
mode = sys.argv[1] if len(sys.argv) > 1 else "kernels2d"
dim = 3 if mode.endswith("3d") else 2
N = int(sys.argv[2]) if len(sys.argv) > 2 else (512 if dim == 2 else 32)
B = int(sys.argv[3]) if len(sys.argv) > 3 else (64 if dim == 2 else 16)
which = sys.argv[4] if len(sys.argv) > 4 else "axial"
dev = torch.device("cuda", 0)
T64 = torch.float64


def bench_mesh():
    """Jittered N x N square (interior nodes moved by up to a quarter step) or the N^3 box, the fixed dofs of the clamped
    x = 0 side and the nodes of the x = 1 side."""
    m = FEMesh.rectangle(N, N) if dim == 2 else FEMesh.box(N, N, N)
    nodes = m.nodes.numpy().copy()
    x0 = nodes[:, 0].copy()
    if dim == 2:
        rng = np.random.default_rng(0)
        interior = np.all((nodes > 1e-9) & (nodes < 1 - 1e-9), axis=1)
        nodes[interior] += rng.uniform(-0.25 / N, 0.25 / N, (int(interior.sum()), 2))
    mesh = FEMesh(nodes=torch.from_numpy(nodes), elements=m.elements, dirichlet_nodes={})
    left, right = np.nonzero(x0 < 1e-9)[0], np.nonzero(x0 > 1 - 1e-9)[0]
    return mesh, {(int(i), a): 0.0 for i in left for a in range(dim)}, right


def end_load(mesh, right):
    ld = torch.zeros(mesh.n_nodes, dim, dtype=T64, device=dev)
    ld[torch.from_numpy(right).to(dev), 0 if which == "axial" else 1] = -1.0 / len(right)
    return ld


def accounted_bytes(fn):
    L = _hip.lib()
    fn()
    L.diffhe_traffic_account(1, None, None)
    fn()
    acc = ctypes.c_double(0.0)
    L.diffhe_traffic_account(1, ctypes.byref(acc), None)
    return acc.value


def kernel_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(kernel_reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / kernel_reps


def kernels(p=8, k=4):
    mesh, fixed, _ = bench_mesh()
    d, n, m = dim, mesh.n_nodes, mesh.n_elements
    nc, rows, Bp = d * (d + 1) // 2, n * d, B
    L, st = _hip.lib(), _stream(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=T64, device=dev)  # noqa: E731
    new = lambda *shape: torch.empty(*shape, dtype=T64, device=dev)  # noqa: E731
    inner = ElasticFESolver(mesh, 1.0, 0.3, fixed=fixed, device=dev)
    plan = inner._plan()
    setup = _setup_of(plan, inner.nu, inner.plane, inner._lam1, inner._mu1, inner._is_bc, inner._g)
    dofs, eng = setup.dofs, _Engine(plan, 0.0, 0, 0, "gather")
    E = 0.5 + 1.5 * torch.rand(B, m, generator=gen, dtype=T64, device=dev)
    kdev, kse, ksb, Bv = eng.kappa_device(E, K_SAMPLE_ELEM, B, Bp)
    vals, _ = setup.assemble(kdev, kse, ksb, Bv)
    sig = rnd(B, m, nc)
    sdev, ssc, sse, ssb, Bg = eng.tensor_device(sig, K_SAMPLE_ELEM, B, Bp, nc)
    gtab, vol = plan.gradient_table()
    G = new(plan.W, n, Bg)
    L.diffhe_aniso_assemble_rows(gtab, vol, d, sdev, ssc, sse, ssb, plan.ent_ptr, plan.contrib, plan.cols, None, None, G,
                                 None, n, m, plan.W, Bg, st)
    del sig, sdev, kdev
    Y, KY, NY, C = rnd(p, rows, Bp), rnd(p, rows, Bp), rnd(p, rows, Bp), rnd(p, p, Bp)
    mu = 0.5 + torch.rand(p, Bp, generator=gen, dtype=T64, device=dev)
    mass = 0.5 + torch.rand(n, Bp, generator=gen, dtype=T64, device=dev)
    M = (mass, Bp, 1, d)
    w = rnd(k, Bp)
    nq, nblk = p * (p + 1) // 2, L.diffhe_eig_gram_blocks(rows, Bp)
    part, GA, GM = new(nblk * 2 * nq * Bp), new(nq, Bp), new(nq, Bp)
    X, KX, NX, R = new(p, rows, Bp), new(p, rows, Bp), new(p, rows, Bp), new(p, rows, Bp)
    y, apart = new(rows, Bp), new(L.diffhe_grad_kappa_blocks(rows, Bp) * Bp)
    ds, de = new(m * nc, Bp), new(m, Bp)
    lamv = rnd(rows, Bp)
    entries = {
        "buckling_apply": lambda: L.diffhe_buckling_apply(G, plan.cols, dofs.is_bc, Y[0], y, -1.0, n, plan.W, d, Bp, Bg, st),
        "ell_apply": lambda: L.diffhe_ell_apply(vals, dofs.cols, Y[0], y, apart, dofs.n, dofs.W, Bp, Bv, st),
        "buckling_gram": lambda: L.diffhe_buckling_gram(Y, KY, NY, dofs.is_bc, p, rows, Bp, part, GA, GM, st),
        "modal_gram": lambda: L.diffhe_modal_gram(Y, KY, *M, dofs.is_bc, p, rows, Bp, part, GA, GM, st),
        "buckling_rotate": lambda: L.diffhe_buckling_rotate(Y, KY, NY, C, mu, p, rows, Bp, X, KX, NX, R, st),
        "modal_rotate": lambda: L.diffhe_modal_rotate(Y, KY, C, mu, *M, p, rows, Bp, X, KX, None, R, st),
        "buckling_grad_sigma": lambda: L.diffhe_buckling_grad_sigma(plan.elems, gtab, vol, d, Y, w, k, n, m, B, Bp, ds, Bp,
                                                                    nc * Bp, None, None, st),
        "elast_grad": lambda: L.diffhe_elast_grad(plan.elems, gtab, vol, d, setup.lam1, setup.mu1, lamv, Y[0], dofs.g, n, m,
                                                  Bp, de, None, None, st),
    }
    nbytes = {name: accounted_bytes(fn) for name, fn in entries.items()}
    nbytes["ell_apply"] = 8.0 * (Bv * dofs.W * dofs.n + 2.0 * Bp * rows)       # the entry accounts nothing of its own
    for fn in entries.values():
        fn()
    times = {name: [] for name in entries}
    for _ in range(rounds):
        for name, fn in entries.items():            # new, yardstick, new, yardstick, ...: the pair alternates
            times[name].append(kernel_ms(fn))
    med = {key: statistics.median(t) for key, t in times.items()}
    spread = {key: max(t) - min(t) for key, t in times.items()}
    out = dict(tool="buckling_bench", mode=mode, N=N, rows=rows, m=m, B=B, p=p, k=k, W_node=plan.W, W_dof=dofs.W,
               kernel_reps=kernel_reps, rounds=rounds, kernels={}, pairs={})
    for name in entries:
        out["kernels"][name] = dict(ms=round(med[name], 4), spread_ms=round(spread[name], 4), MB=round(nbytes[name] / 1e6, 1),
                                    TBps=round(nbytes[name] / (1e9 * med[name]), 3))
    for a, b in (("buckling_apply", "ell_apply"), ("buckling_gram", "modal_gram"), ("buckling_rotate", "modal_rotate"),
                 ("buckling_grad_sigma", "elast_grad")):
        byte_ratio = nbytes[a] / nbytes[b]
        out["pairs"][a] = dict(yardstick=b, byte_ratio=round(byte_ratio, 4), time_ratio=round(med[a] / med[b], 4),
                               ratio=round(med[a] / (med[b] * byte_ratio), 3))
    print(json.dumps(out), flush=True)


class _TimedRun(buckling._BucklingRun):
    """The product's run object with a clock around its groups of device work."""
    clock = None

    def _timed(self, key, fn, *args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*args, **kw)
        torch.cuda.synchronize()
        self.clock[key] = self.clock.get(key, 0.0) + time.perf_counter() - t0
        return out

    def _setup(self, *args, **kw):
        return self._timed("setup", super()._setup, *args, **kw)

    def _inner_solve(self, rhs):
        return self._timed("inner", super()._inner_solve, rhs)

    def _apply_column(self, i, Y, KY):
        return self._timed("apply", super()._apply_column, i, Y, KY)

    def _rayleigh_ritz(self, Y, KY):
        return self._timed("block", super()._rayleigh_ritz, Y, KY)


def problem():
    mesh, fixed, right = bench_mesh()
    gen = torch.Generator(device=dev).manual_seed(0)
    E = 0.5 + 1.5 * torch.rand(B, mesh.n_elements, generator=gen, dtype=T64, device=dev)
    return mesh, fixed, E, end_load(mesh, right)


def solve():
    mesh, fixed, E, load = problem()
    bs = LinearBucklingSolver(mesh, E, 4, guard=4, fixed=fixed, device=dev, max_iter=max_iter)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sigma = bs.inner.stress(bs.inner(load=load))            # also builds the plan and the hierarchy: reported, not split
    torch.cuda.synchronize()
    prestress = time.perf_counter() - t0
    clock = {}
    run = _TimedRun(bs, E, sigma, None)
    run.clock = clock
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        run.run((E, sigma), None, True)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    info = bs.last_info
    its = max(info.outer_iterations, 1)
    out = dict(tool="buckling_bench", mode=mode, load=which, N=N, dofs=dim * mesh.n_nodes, m=mesh.n_elements, B=B, k=bs.k,
               block=bs.k + bs.guard, path=info.path, levels=info.inner.hierarchy_levels,
               outer_iterations=info.outer_iterations, inner_solves=info.inner_solves, inner_iterations=info.inner_iterations,
               not_converged=info.not_converged, missing=info.missing, negative_ritz=info.negative_ritz,
               max_shift=round(float(info.shifts.max()), 4), max_rho=float(info.residual.max()),
               first_call_prestress_ms=round(1e3 * prestress, 1), total_ms=round(1e3 * total, 1),
               setup_ms=round(1e3 * clock["setup"], 1), inner_ms_per_outer=round(1e3 * clock["inner"] / its, 2),
               # the first Rayleigh-Ritz and the first p applications belong to the start block: its + 1 groups
               apply_ms_per_outer=round(1e3 * clock["apply"] / (its + 1), 2),
               block_ms_per_outer=round(1e3 * clock["block"] / (its + 1), 2))
    print(json.dumps(out), flush=True)


def step():
    import warnings
    mesh, fixed, E0, load = problem()

    def buckling_step(E):
        bs = LinearBucklingSolver(mesh, E, 4, guard=4, fixed=fixed, device=dev, max_iter=max_iter)
        lam, _ = bs(load=load)
        buckling.aggregate(lam).sum().backward()
        return bs

    def elastic_step(E):
        es = ElasticFESolver(mesh, E, 0.3, fixed=fixed, device=dev)
        u = es(load=load)
        (u * load).sum().backward()
        return es

    out = dict(tool="buckling_bench", mode=mode, load=which, N=N, dofs=dim * mesh.n_nodes, B=B)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name, fn in (("elastic", elastic_step), ("buckling", buckling_step)):
            for rep in range(2):                        # the first call builds the plan, the hierarchy and the code objects
                E = E0.clone().requires_grad_(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                solver = fn(E)
                torch.cuda.synchronize()
                out[name + "_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            if name == "buckling":
                info = solver.last_info
                out.update(outer_iterations=info.outer_iterations, inner_solves=info.inner_solves,
                           not_converged=info.not_converged)
    out["ratio"] = round(out["buckling_ms"] / out["elastic_ms"], 1)
    print(json.dumps(out), flush=True)


if mode.startswith("kernels"):
    kernels()
elif mode.startswith("solve"):
    solve()
elif mode.startswith("step"):
    step()
else:
    raise SystemExit(f"unknown mode {mode!r}")
