"""Anisotropic stress-recovery timing: the kernels of csrc/elastic_aniso_stress.hip next to their linear twins of
csrc/stress.hip on the same arrays, at C = isotropic(E_e, 0.3).  One process; prints one JSON line.

    python tools/elastic_aniso_stress_bench.py kernels2d [N] [B]     jittered N x N mesh (default 512, 64)
    python tools/elastic_aniso_stress_bench.py kernels3d [N] [B]     FEMesh.box(N, N, N) (default 32, 16)
    options: --kernel-reps R (default 20)  --rounds K (default 7)

u (n d, Bp) is random, E (m, Bp) uniform in [0.5, 2]; the new entries read C = isotropic(E, 0.3) per element and sample
(nt, m, Bp) -- plane stress in 2D -- and a random criterion per element and sample (nk, m, Bp), the twins read E itself;
the batch-summed entries read sample 0's fields, shared.  The cotangents are random.  After two warm-up launches of every
entry, `--rounds` rounds visit all entries in turn -- a new entry and its twin alternate in the same process -- each
visit being `--kernel-reps` back-to-back launches between two HIP events; a figure is the median over the rounds of the
mean per launch.  Per entry: ms, the algorithmic bytes the entry accounts for (diffhe_traffic_account) and TB/s of those.
Per new entry also its yardstick, the twin's time x the ratio of the algorithmic bytes, and the ratio of its time to
that.  The fused failure index is also timed against the torch composition q . sigma + sigma . Q sigma from a stored
sigma: `phi_from_stored_sigma` is the stress launch plus that composition.
"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "difffe-physics-lab_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffhe import FEMesh, _hip  # noqa: E402
from diffhe.elastic import lame_unit  # noqa: E402
from diffhe.elastic_aniso import isotropic, matrix  # noqa: E402
from diffhe.plan import get_plan, _stream  # noqa: E402


def _option(name, default, kind=float):
    if name in sys.argv:
        i = sys.argv.index(name)
        value = kind(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return value
    return default


kernel_reps = _option("--kernel-reps", 20, int)
rounds = _option("--rounds", 7, int)
mode = sys.argv[1] if len(sys.argv) > 1 else "kernels2d"
arg = lambda i, default: int(sys.argv[i]) if len(sys.argv) > i else default  # noqa: E731
dev = torch.device("cuda", 0)
T64 = torch.float64


def bench_mesh(N, dim):
    """Jittered N x N square (interior nodes moved by up to a quarter step) or the N^3 box: tools/stress_bench.py's."""
    m = FEMesh.rectangle(N, N) if dim == 2 else FEMesh.box(N, N, N)
    nodes = m.nodes.numpy().copy()
    if dim == 2:
        rng = np.random.default_rng(0)
        interior = np.all((nodes > 1e-9) & (nodes < 1 - 1e-9), axis=1)
        nodes[interior] += rng.uniform(-0.25 / N, 0.25 / N, (int(interior.sum()), 2))
    return FEMesh(nodes=torch.from_numpy(nodes), elements=m.elements, dirichlet_nodes={})


def accounted_bytes(fn):
    L = _hip.lib()
    L.diffhe_traffic_account(1, None, None)
    fn()
    acc = ctypes.c_double(0.0)
    L.diffhe_traffic_account(1, ctypes.byref(acc), None)
    return acc.value


def visit_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(kernel_reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / kernel_reps


def kernels(N, dim, B, label):
    mesh = bench_mesh(N, dim)
    d, n, m = mesh.dim, mesh.n_nodes, mesh.n_elements
    nv = d * (d + 1) // 2
    nt = nv * (nv + 1) // 2
    nk = nv + nt
    Bp = B
    plan = get_plan(mesh, dev, prune=False)
    L, st = _hip.lib(), _stream(dev)
    plane = "stress" if d == 2 else None
    lam1, mu1 = lame_unit(0.3, d, plane)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=T64, device=dev)  # noqa: E731
    new = lambda *shape: torch.empty(*shape, dtype=T64, device=dev)  # noqa: E731
    u = (0.02 / N) * rnd(n * d, Bp)
    E = 0.5 + 1.5 * torch.rand(m, Bp, generator=gen, dtype=T64, device=dev)
    C = isotropic(E, 0.3, d, plane).permute(2, 0, 1).contiguous()               # (nt, m, Bp)
    K = rnd(nk, m, Bp)
    C0, K0, E0 = C[:, :, 0].t().contiguous(), K[:, :, 0].t().contiguous(), E[:, 0].contiguous()     # (m, nt), (m, nk), (m)
    sbar, pbar = rnd(m * nv, Bp), rnd(m, Bp)
    sigma, phi, ubar, work = new(m * nv, Bp), new(m, Bp), new(n * d, Bp), new(nv, m, Bp)
    de, de_s, dc, dk, dc_s, dk_s = new(m, Bp), new(m), new(nt, m, Bp), new(nk, m, Bp), new(m, nt), new(m, nk)
    gtab = plan.oriented_gradient_table()
    lists, none = plan.shape_incidence(), (None, None)
    mb = m * Bp
    aniso = (plan.elems, gtab, d, u, C, mb, Bp, 1, K, mb, Bp, 1)
    aniso0 = (plan.elems, gtab, d, u, C0, 1, nt, 0, K0, 1, nk, 0)
    linear = (plan.elems, gtab, d, lam1, mu1, 0.0, u, E, Bp, 1)
    linear0 = (plan.elems, gtab, d, lam1, mu1, 0.0, u, E0, 1, 0)
    acot, lcot = (sbar, Bp, nv * Bp, pbar), (sbar, Bp, nv * Bp, pbar)
    no, of_c, of_k = (None, 0, 0, None, None), (dc, mb, Bp, None, None), (dk, mb, Bp, None, None)
    q = K[:nv].permute(1, 2, 0)                                                  # (m, Bp, nv) views for the torch composition
    Qm = matrix(K[nv:].permute(1, 2, 0))

    def phi_torch():
        s = sigma.view(m, nv, Bp).permute(0, 2, 1)
        return (q * s).sum(-1) + torch.einsum("ebi,ebij,ebj->eb", s, Qm, s)

    def stress_then_torch():
        L.diffhe_elastc_stress_eval(*aniso, n, m, Bp, sigma, Bp, nv * Bp, None, st)
        return phi_torch()

    twin_adjoint = lambda: L.diffhe_stress_adjoint(*linear, *lcot, *lists, n, m, B, Bp, work, ubar, de, None, None,  # noqa: E731
                                                   st)
    twin_element = lambda: L.diffhe_stress_adjoint(*linear, *lcot, *none, n, m, B, Bp, None, None, de, None, None,  # noqa: E731
                                                   st)
    twin_shared = lambda: L.diffhe_stress_adjoint_shared(*linear0, *lcot, n, m, B, Bp, de_s, st)  # noqa: E731
    # name -> (new entry, twin)
    pairs = {
        "eval sigma": (lambda: L.diffhe_elastc_stress_eval(*aniso, n, m, Bp, sigma, Bp, nv * Bp, None, st),
                       lambda: L.diffhe_stress_eval(*linear, n, m, Bp, sigma, Bp, nv * Bp, None, st)),
        "eval sigma+phi (twin: sigma+vm)": (
            lambda: L.diffhe_elastc_stress_eval(*aniso, n, m, Bp, sigma, Bp, nv * Bp, phi, st),
            lambda: L.diffhe_stress_eval(*linear, n, m, Bp, sigma, Bp, nv * Bp, phi, st)),
        "eval phi only (twin: vm only)": (lambda: L.diffhe_elastc_stress_eval(*aniso, n, m, Bp, None, 0, 0, phi, st),
                                          lambda: L.diffhe_stress_eval(*linear, n, m, Bp, None, 0, 0, phi, st)),
        "adjoint whole (T, dC, node pass; twin: T, dE, node pass)": (
            lambda: L.diffhe_elastc_stress_adjoint(*aniso, *acot, *lists, n, m, B, Bp, work, ubar, *of_c, *no, st),
            twin_adjoint),
        "adjoint du alone (T, node pass)": (
            lambda: L.diffhe_elastc_stress_adjoint(*aniso, *acot, *lists, n, m, B, Bp, work, ubar, *no, *no, st),
            lambda: L.diffhe_stress_adjoint(*linear, *lcot, *lists, n, m, B, Bp, work, ubar, None, None, None, st)),
        "adjoint dC alone (twin: dE alone)": (
            lambda: L.diffhe_elastc_stress_adjoint(*aniso, *acot, *none, n, m, B, Bp, None, None, *of_c, *no, st),
            twin_element),
        "adjoint d criterion alone (twin: dE alone)": (
            lambda: L.diffhe_elastc_stress_adjoint(*aniso, *acot, *none, n, m, B, Bp, None, None, *no, *of_k, st),
            twin_element),
        "adjoint_shared dC (twin: dE)": (
            lambda: L.diffhe_elastc_stress_adjoint_shared(*aniso0, *acot, n, m, B, Bp, dc_s, 1, nt, None, 0, 0, st),
            twin_shared),
        "adjoint_shared d criterion (twin: dE)": (
            lambda: L.diffhe_elastc_stress_adjoint_shared(*aniso0, *acot, n, m, B, Bp, None, 0, 0, dk_s, 1, nk, st),
            twin_shared),
    }
    flat = [(name, side, fn) for name, fns in pairs.items() for side, fn in zip(("new", "twin"), fns)]
    flat += [("phi_from_stored_sigma", "new", stress_then_torch), ("phi_torch_composition_alone", "new", phi_torch)]
    nbytes = {}
    for name, side, fn in flat:                                  # two warm-up launches; the second is accounted
        fn()
        nbytes[name, side] = accounted_bytes(fn)
    torch.cuda.synchronize()
    L.diffhe_elastc_stress_eval(*aniso, n, m, Bp, sigma, Bp, nv * Bp, phi, st)
    phi_gap = float((phi_torch() - phi).abs().max() / phi.abs().max())
    finite = bool(torch.isfinite(phi).all() and torch.isfinite(ubar).all() and torch.isfinite(dc).all()
                  and torch.isfinite(dk).all() and torch.isfinite(dc_s).all() and torch.isfinite(dk_s).all())
    samples = {key[:2]: [] for key in flat}
    for _ in range(rounds):
        for name, side, fn in flat:
            samples[name, side].append(visit_ms(fn))
    out = dict(tool="elastic_aniso_stress_bench", mode=label, N=N, n=n, m=m, d=d, B=B, kernel_reps=kernel_reps,
               rounds=rounds, finite=finite, phi_fused_vs_torch=phi_gap, kernels={}, torch={})
    for name in pairs:
        ms, twin = statistics.median(samples[name, "new"]), statistics.median(samples[name, "twin"])
        ratio = nbytes[name, "new"] / nbytes[name, "twin"]
        out["kernels"][name] = dict(
            ms=round(ms, 4), MB=round(nbytes[name, "new"] / 1e6, 1), TBps=round(nbytes[name, "new"] / (1e9 * ms), 3),
            spread=round((max(samples[name, "new"]) - min(samples[name, "new"])) / ms, 3),
            twin_ms=round(twin, 4), twin_MB=round(nbytes[name, "twin"] / 1e6, 1), byte_ratio=round(ratio, 3),
            yardstick_ms=round(twin * ratio, 4), over_yardstick=round(ms / (twin * ratio), 3))
    fused = statistics.median(samples["eval phi only (twin: vm only)", "new"])
    for name in ("phi_from_stored_sigma", "phi_torch_composition_alone"):
        ms = statistics.median(samples[name, "new"])
        out["torch"][name] = dict(ms=round(ms, 4), fused_phi_ms=round(fused, 4), times_fused=round(ms / fused, 2))
    print(json.dumps(out), flush=True)


if mode == "kernels2d":
    kernels(arg(2, 512), 2, arg(3, 64), "kernels2d")
elif mode == "kernels3d":
    kernels(arg(2, 32), 3, arg(3, 16), "kernels3d")
else:
    raise SystemExit(f"unknown mode {mode!r}")
