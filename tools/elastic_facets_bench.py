"""Facet loads and foundations of elastic bodies next to the solver without them, one process, alternated round by round.
Prints JSON lines.

    python tools/elastic_facets_bench.py pair2d [N] [B] [steps] [rounds]    jittered N x N mesh, left edge clamped
    python tools/elastic_facets_bench.py pair3d [N] [B] [steps] [rounds]    FEMesh.box(N, N, N), face x = 0 clamped
    options: --max-iter K (cap of both PCGs, default 3000)  --kernel-reps R (default 20)

(a) a fwd + adjoint step of `TractionElasticFESolver` with `traction=` (per sample and facet) on the side x = 1, next to
the same step of `ElasticFESolver` with that traction integrated into `load=` by hand: iterations, the median of
steps x rounds ms, and the ratio of every alternating pair of rounds (its spread is the noise the ratio is read against);
(b) the kernel times of `diffhe_elastf_assemble` (with a foundation) / `diffhe_elastf_grad` next to
`diffhe_robin_assemble` / `diffhe_robin_grad` on the same facets (HIP events around `--kernel-reps` launches) with the
ratio of algorithmic bytes -- the yardstick is the scalar kernel's time scaled by that ratio; (c) the foundation case:
`k_normal` per sample and facet on the side y = 0 (z = 0 in 3D), iterations, step time, and the bound kernels of every
level plus the host copy, per call.
"""
import functools
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "difffe-physics-lab_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffhe import ElasticFESolver, FEMesh, TractionElasticFESolver, _hip  # noqa: E402
from diffhe.elastic import _setup_of  # noqa: E402
from diffhe.plan import padded_batch, _stream  # noqa: E402
from diffhe.solver import K_SAMPLE_ELEM, _Engine  # noqa: E402


def _option(name, default, kind=float):
    if name in sys.argv:
        i = sys.argv.index(name)
        value = kind(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return value
    return default


max_iter = _option("--max-iter", 3000, int)
kernel_reps = _option("--kernel-reps", 20, int)
mode = sys.argv[1] if len(sys.argv) > 1 else "pair2d"
arg = lambda i, default: int(sys.argv[i]) if len(sys.argv) > i else default  # noqa: E731
dev = torch.device("cuda", 0)
T64 = torch.float64
TOOL = "elastic_facets_bench"


@functools.lru_cache(maxsize=None)
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


def side(mesh, axis, value):
    """Indices into mesh.boundary_facets() of the facets on the plane x_axis = value."""
    x = mesh.nodes[mesh.boundary_facets()][:, :, axis]
    return torch.nonzero(torch.isclose(x, torch.full_like(x, value)).all(1)).reshape(-1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_ms(fn):
    """Mean over `kernel_reps` back-to-back launches between two events, after two warm-up launches."""
    fn()
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(kernel_reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / kernel_reps


def info_of(solver, t):
    i = solver.last_info
    return dict(step_ms=round(1e3 * statistics.median(t), 2), min_ms=round(1e3 * min(t), 2), max_ms=round(1e3 * max(t), 2),
                iters=i.iterations, adj_iters=i.adj_iterations, path=i.path, not_converged=i.not_converged,
                max_relres=i.max_relres, levels=i.hierarchy_levels, hierarchy=i.hierarchy)


def pair(N, dim, B, steps, rounds, label):
    mesh = clamped_mesh(N, dim)
    d, n, m = mesh.dim, mesh.n_nodes, mesh.n_elements
    gen = torch.Generator(device=dev).manual_seed(0)
    E = (0.5 + 1.5 * torch.rand(B, m, generator=gen, dtype=T64, device=dev)).requires_grad_(True)
    right = side(mesh, 0, 1.0)
    plain = ElasticFESolver(mesh, E, 0.3, device=dev, max_iter=max_iter)
    facet = TractionElasticFESolver(mesh, E, 0.3, facets=right, device=dev, max_iter=max_iter)
    nF = facet.n_facets
    t = torch.zeros(B, nF, d, dtype=T64, device=dev)
    t[:, :, 1] = -1.0 - torch.rand(B, nF, generator=gen, dtype=T64, device=dev)
    t.requires_grad_(True)
    # the same traction integrated by hand: |F| / d t_F to every node of the facet
    share = (facet.facet_areas.to(dev) / d)[None, :, None] * t.detach()
    load = torch.zeros(B, n, d, dtype=T64, device=dev)
    for p in range(d):
        load.index_add_(1, facet.facets[:, p].to(dev), share)
    load.requires_grad_(True)

    def step_plain():
        E.grad = load.grad = None
        u = plain(None, load)
        (0.5 * (u * u).sum() / B).backward()

    def step_facet():
        E.grad = t.grad = None
        u = facet(traction=t)
        (0.5 * (u * u).sum() / B).backward()

    sides = {"load": step_plain, "traction": step_facet}
    out = dict(tool=TOOL, mode=label, N=N, n=n, m=m, d=d, B=B, n_facets=nF, steps=steps, rounds=rounds, max_iter=max_iter)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        first = {}
        for k, fn in sides.items():                                       # plan, hierarchy (shared), code objects
            first[k] = round(timed(fn), 2)
            print(json.dumps(dict(tool=TOOL, progress=f"first {k} step", seconds=first[k])), flush=True)
        for fn in sides.values():
            fn()
        times = {k: [] for k in sides}
        per_round = {k: [] for k in sides}
        for r in range(rounds):
            for k in (("load", "traction") if r % 2 == 0 else ("traction", "load")):
                ts = [timed(sides[k]) for _ in range(steps)]
                times[k] += ts
                per_round[k].append(statistics.median(ts))
    out.update(first_step_s=first, warnings=len(caught), load=info_of(plain, times["load"]),
               traction=info_of(facet, times["traction"]))
    out["step_traction_over_load"] = round(out["traction"]["step_ms"] / out["load"]["step_ms"], 4)
    out["pair_ratios"] = [round(a / b, 4) for a, b in zip(per_round["traction"], per_round["load"])]
    out["load_round_spread"] = round(max(per_round["load"]) / min(per_round["load"]), 4)
    print(json.dumps(out), flush=True)

    # (b) the band kernels alone next to the scalar ones, on the same facets
    plan = plain._plan()
    Bp = padded_batch(B)
    L, st = _hip.lib(), _stream(dev)
    setup = _setup_of(plan, plain.nu, plain.plane, plain._lam1, plain._mu1, plain._is_bc, plain._g)
    dofs, W = setup.dofs, plan.W
    tab = facet._table(plan)
    rtab = plan.robin_table("bench-right", facet._facets_host)
    eng = _Engine(plan, 1e-12, 100, 25, "gather")
    nd = n * d
    rnd = lambda *shape: torch.rand(shape, generator=gen, dtype=T64, device=dev)  # noqa: E731
    x, lam = rnd(nd, Bp), rnd(nd, Bp)
    vals, rhs = torch.zeros(d * W, nd, Bp, dtype=T64, device=dev), torch.zeros(nd, Bp, dtype=T64, device=dev)
    svals, srhs = torch.zeros(W, n, Bp, dtype=T64, device=dev), torch.zeros(n, Bp, dtype=T64, device=dev)
    td, pd, kn, kt = rnd(B, nF, d), rnd(B, nF), rnd(B, nF), rnd(B, nF)
    o3, o1 = torch.empty(3, B, nF, dtype=T64, device=dev), torch.empty(B, nF, d, dtype=T64, device=dev)
    head = (tab["fac"], d, nF, tab["area"], tab["normal"])
    band = (tab["rows"], tab["row_ptr"], tab["ent_code"], tab["ent_slot"], tab["n_rows"])
    rband = (rtab["rows"], rtab["row_ptr"], rtab["ent_code"], rtab["ent_slot"], rtab["n_rows"])
    ms = dict(
        assemble_elastic=kernel_ms(lambda: L.diffhe_elastf_assemble(
            *head, *band, dofs.is_bc, dofs.g, td, d, 1, nF * d, pd, 1, nF, kn, 1, nF, kt, 1, nF, vals, rhs, n, Bp, B, Bp, st)),
        assemble_scalar=kernel_ms(lambda: L.diffhe_robin_assemble(
            rtab["fac"], d, nF, rtab["area"], *rband, eng.g, kn, 1, nF, pd, 1, nF, kt, 1, nF, svals, srhs, n, Bp, B, Bp, st)),
        grad_elastic=kernel_ms(lambda: L.diffhe_elastf_grad(
            *head, lam, x, dofs.g, B, Bp, o1, d, 1, nF * d, o3[0], 1, nF, o3[1], 1, nF, o3[2], 1, nF, st)),
        grad_scalar=kernel_ms(lambda: L.diffhe_robin_grad(
            rtab["fac"], d, nF, rtab["area"], lam[:n], x[:n], eng.g, B, Bp, kn, 1, nF, pd, 1, nF, o3[0], 1, nF, o3[1], 1, nF,
            o3[2], 1, nF, st)))
    # algorithmic bytes, as the entries account them: rhs read + written and the blocks / entries of the band rows;
    # lambda and u of the facet nodes and the outputs
    by = dict(assemble_elastic=tab["n_rows"] * (2 * d * Bp + 2 * d ** 3 * Bp), assemble_scalar=rtab["n_rows"] * (d * Bp + 2 * Bp),
              grad_elastic=nF * (2 * d * d * B + (d + 3) * B), grad_scalar=nF * (2 * d * B + 3 * B))
    kb = dict(tool=TOOL, mode=label + "-kernels", N=N, B=B, n_facets=nF, band_rows=tab["n_rows"], scalar_band_rows=rtab["n_rows"],
              kernel_ms={k: round(v, 4) for k, v in ms.items()}, algorithmic_MB={k: round(8e-6 * v, 3) for k, v in by.items()})
    for kind in ("assemble", "grad"):
        ratio = by[kind + "_elastic"] / by[kind + "_scalar"]
        kb[kind] = dict(byte_ratio=round(ratio, 3), yardstick_ms=round(ms[kind + "_scalar"] * ratio, 4),
                        elastic_over_yardstick=round(ms[kind + "_elastic"] / (ms[kind + "_scalar"] * ratio), 3))
    print(json.dumps(kb), flush=True)

    # (c) the foundation case: k_normal per sample and facet on the lower side, the left side still clamped
    low = side(mesh, d - 1, 0.0)
    found = TractionElasticFESolver(mesh, E, 0.3, facets=torch.cat([right, low]), device=dev, max_iter=max_iter)
    nF2 = found.n_facets
    t2 = torch.cat([t.detach(), torch.zeros(B, len(low), d, dtype=T64, device=dev)], dim=1)
    k2 = torch.cat([torch.zeros(B, nF, dtype=T64, device=dev), 0.5 + rnd(B, len(low))], dim=1).requires_grad_(True)

    def step_found():
        E.grad = k2.grad = None
        u = found(traction=t2, k_normal=k2)
        (0.5 * (u * u).sum() / B).backward()

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        step_found()
        ts = [timed(step_found) for _ in range(steps)]
    fo = dict(tool=TOOL, mode=label + "-foundation", N=N, B=B, n_facets=nF2, foundation_facets=len(low), warnings=len(caught),
              foundation=info_of(found, ts), jacobi_bounds=[round(b, 4) for b in found.last_info.jacobi_bounds])
    kdev, kse, ksb, Bv = eng.kappa_device(E.detach(), K_SAMPLE_ELEM, B, Bp)
    levels, _ = setup.levels()
    vals, _ = setup.assemble(kdev, kse, ksb, Bv)
    arr, chain = _Engine(dofs, 1e-12, 100, 25, "gather", g=dofs.g).amg_setup(vals, Bv, False, levels)
    part = torch.empty(_hip.ROW_BOUND_BLOCKS, dtype=T64, device=dev)
    res = torch.empty(len(chain), dtype=T64, device=dev)

    def bounds():
        for l, lv in enumerate(chain):
            L.diffhe_ell_jacobi_row_bound(lv["vals"], lv["cols"], lv["n"], lv["W"], Bv, part, res[l:], st)

    fo["bounds"] = dict(levels=len(chain), kernels_ms=round(kernel_ms(bounds), 4),
                        with_host_copy_ms=round(1e3 * statistics.median(
                            [timed(lambda: (bounds(), res.cpu())) for _ in range(6)]), 4))
    print(json.dumps(fo), flush=True)


if mode == "pair2d":
    pair(arg(2, 512), 2, arg(3, 64), arg(4, 3), arg(5, 2), "pair2d")
elif mode == "pair3d":
    pair(arg(2, 32), 3, arg(3, 16), arg(4, 3), arg(5, 2), "pair3d")
else:
    raise SystemExit(f"unknown mode {mode!r}")
