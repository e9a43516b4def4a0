"""The fused passes around the full-multigrid start of the lattice solve (the default on the fp32-stored, batch-shared
path: prolongation + residual in one strip pass, conversion of the right-hand side + its first restriction in one pass,
z0 written where p0 lives) against mg={'split_start': 1} (DIFFHE_PCG_SPLIT_START), which keeps the separate passes.
The fusions change where values are formed, never a stored value: the two settings are compared by EQUALITY."""
import ctypes
import functools
import os
import re
import warnings

import numpy as np
import pytest
import torch

from diffhe import FEMesh, DifferentiableFESolver, _hip
from oracle import p1_oracle as orc
from _util import rel_err, RTOL_U

pytestmark = pytest.mark.gpu
T64 = torch.float64
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strip_threshold():
    """(least row width W = nx + 1, least row count ny + 1) of strip_geom(...).use, read from csrc/lattice.h."""
    src = open(os.path.join(ROOT, "difffe-physics-lab_amd", "csrc", "lattice.h")).read()
    min_w = int(re.search(r"constexpr int kStripMinW = (\d+);", src).group(1))
    m = re.search(r"if \(Bp < kWave \|\| L\.W < kStripMinW \|\| L\.ny \+ 1 < (\d+)\) return none;", src)
    return min_w, int(m.group(1))


MIN_W, MIN_ROWS = _strip_threshold()
# (nx, ny, width of the domain; its height is 1).
# "tail": the smallest lattice that halves and takes the strip kernels, W = 129 (the last strip is a TAIL strip).  Its
# cells are square (a 2 x 1 domain): on the unit square the same 128 x 64 lattice has cells twice as long in y as in x,
# and the hierarchy then halves x alone first (plan.coarsening_step) -- that one is "tail_unit", where, as on "xonly"
# (cells four times as long, W = 257, 65 rows), every fusion must stand aside.  "nonsquare": W = 161, several row tiles
# per strip, cells 1.4 : 1 (still halved in both directions).
SHAPES = {"tail": (MIN_W, MIN_ROWS, 2.0), "nonsquare": (160, 224, 1.0), "tail_unit": (MIN_W, MIN_ROWS, 1.0),
          "xonly": (256, 64, 1.0)}
FUSED = ("tail", "nonsquare")
BATCHES = (64, 128, 256)   # the one-, two- and four-sample-per-lane kernel forms
LOADS = ("random", "point")


@functools.lru_cache(maxsize=None)
def _inputs(shape, B, load):
    nx, ny, width = SHAPES[shape]
    mesh = FEMesh.rectangle(nx, ny, (0.0, width), (0.0, 1.0))
    gen = torch.Generator().manual_seed(3000 + 7 * B + nx)
    kappa = 0.5 + 1.5 * torch.rand(B, generator=gen, dtype=T64)
    if load == "random":
        f = torch.rand(B, mesh.n_nodes, generator=gen, dtype=T64)
    else:   # one loaded node per sample, an interior one, a different one for each sample
        f = torch.zeros(B, mesh.n_nodes, dtype=T64)
        rows = 1 + torch.randint(0, ny - 1, (B,), generator=gen)
        cols = 1 + torch.randint(0, nx - 1, (B,), generator=gen)
        f[torch.arange(B), rows * (nx + 1) + cols] = 1.0
    return mesh, kappa, f


@functools.lru_cache(maxsize=None)
def _oracle(shape, B, b):
    mesh, kappa, f = _inputs(shape, B, "random")
    bn, bv = np.array(list(mesh.dirichlet_nodes.keys())), np.array(list(mesh.dirichlet_nodes.values()))
    return orc.solve_with_adjoint(mesh.nodes.numpy(), mesh.elements.numpy(), bn, bv, float(kappa[b]), f[b].numpy(),
                                  lambda u_: 2 * u_, sparse=True, refine=1)[0]


def _traffic_reset():
    _hip.lib().diffhe_traffic_account(1, None, None)


def _traffic():
    got = ctypes.c_double()
    _hip.lib().diffhe_traffic_account(0, ctypes.byref(got), None)
    return got.value


def _step(shape, B, load, split, max_iter=None, backward=True, **mg):
    """One forward solve (its accounted bytes) and, if asked, the backward of sum u^2.  max_iter given: tol so small and
    no attainable-accuracy floor, so nothing stops before max_iter (an explicit tol also switches the energy rule off);
    None: the default stop."""
    mesh, kappa0, f = _inputs(shape, B, load)
    kappa = kappa0.clone().to(DEV).requires_grad_(backward)
    mg = dict(mg, split_start=int(split))
    kw = {} if max_iter is None else dict(tol=1e-300, max_iter=max_iter)
    if max_iter is not None:
        mg["floor"] = 0
    solver = DifferentiableFESolver(mesh, kappa, device=DEV, mg=mg, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)    # "did not reach tol": by construction
        _traffic_reset()
        u = solver(f.to(DEV))
        nbytes = _traffic()
        info = solver.last_info
        grad = None
        if backward:
            (u ** 2).sum().backward()
            grad = kappa.grad.detach().clone()
    return u.detach(), grad, info, nbytes


@pytest.mark.parametrize("load", LOADS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", FUSED)
def test_fused_start_is_bitwise_the_split_start(shape, B, load):
    """u and dL/dkappa of the default equal those of the split start bit for bit after 0, 1 and 3 iterations (nothing
    stops early) and with the default stop, where iteration counts, stop rules and max_relres agree too; two runs of
    the default are bitwise equal."""
    for max_iter in (0, 1, 3, None):
        ud, gd, idf, _ = _step(shape, B, load, False, max_iter)
        us, gs, isp, _ = _step(shape, B, load, True, max_iter)
        print(f"{shape} B={B} {load} max_iter={max_iter}: its {idf.iterations}/{isp.iterations} adj "
              f"{idf.adj_iterations}/{isp.adj_iterations} relres {idf.max_relres:.3e}/{isp.max_relres:.3e} "
              f"max|du| {float((ud - us).abs().max()):.3e} max|dg| {float((gd - gs).abs().max()):.3e}")
        assert idf.path == isp.path == "lattice-mgpcg"
        assert idf.flags & _hip.PCG_FP32 and idf.flags & _hip.PCG_FMG and not idf.flags & _hip.PCG_WARM
        assert isp.flags & _hip.PCG_SPLIT_START and not idf.flags & _hip.PCG_SPLIT_START
        assert isp.flags == idf.flags | _hip.PCG_SPLIT_START
        assert torch.equal(ud, us)
        assert torch.equal(gd, gs)
        assert idf.iterations == isp.iterations and idf.adj_iterations == isp.adj_iterations
        assert idf.stop_rules == isp.stop_rules and idf.adj_stop_rules == isp.adj_stop_rules
        assert idf.max_relres == isp.max_relres and idf.adj_max_relres == isp.adj_max_relres
        assert idf.not_converged == isp.not_converged
        if max_iter is None:
            assert idf.not_converged == 0
            ud2, gd2, _, _ = _step(shape, B, load, False, None)
            assert torch.equal(ud, ud2) and torch.equal(gd, gd2)
        else:
            assert idf.iterations == max_iter and idf.stop_rules["cap"] == B


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", FUSED)
def test_fused_start_accounts_three_fp32_vectors_less(shape, B):
    """diffhe_traffic_account around a forward solve of 3 iterations, on a plan that has solved before: the default
    accounts 12 n Bp bytes less than the split start -- 4 n Bp for each of the three fusions."""
    mesh = _inputs(shape, B, "random")[0]
    _step(shape, B, "random", False, 3, backward=False)   # a plan's first solve also accounts its cached copies
    _, _, idf, bytes_d = _step(shape, B, "random", False, 3, backward=False)
    _, _, isp, bytes_s = _step(shape, B, "random", True, 3, backward=False)
    saved = (bytes_s - bytes_d) / (4.0 * mesh.n_nodes * B)      # in units of one fp32 vector
    print(f"{shape} B={B}: bytes split - fused = {saved:.6f} fp32 vectors of {bytes_s / (mesh.n_nodes * B):.1f} B per "
          f"node and sample")
    assert idf.iterations == isp.iterations == 3
    assert abs(saved - 3.0) < 1e-6, (bytes_s, bytes_d)


@pytest.mark.parametrize("case", ["xonly", "tail_unit", "fp64"])
def test_where_the_fusions_do_not_apply_the_old_sequence_runs(case):
    """A first coarsening in x only, and fp64-stored cycle vectors (mg fp32 = 0): both settings account the same bytes
    and give the same u -- the flag has nothing to switch there."""
    shape, mg = ("tail", dict(fp32=0)) if case == "fp64" else (case, {})
    B = 128
    _step(shape, B, "random", False, 3, backward=False, **mg)
    ud, _, idf, bytes_d = _step(shape, B, "random", False, 3, backward=False, **mg)
    us, _, isp, bytes_s = _step(shape, B, "random", True, 3, backward=False, **mg)
    print(f"{case}: bytes {bytes_d:.0f} / {bytes_s:.0f}, flags {idf.flags:#x} / {isp.flags:#x}")
    assert idf.path == isp.path == "lattice-mgpcg" and idf.flags & _hip.PCG_FMG
    assert bool(idf.flags & _hip.PCG_FP32) == (case != "fp64")
    assert bytes_d == bytes_s
    assert torch.equal(ud, us)


@pytest.mark.parametrize("B", BATCHES)
def test_fused_start_meets_the_oracle(B):
    """After 12 iterations the default meets the refined oracle at the suite's RTOL_U on the first and the last sample
    of the smallest shape: the two settings are not wrong together."""
    u, _, info, _ = _step("tail", B, "random", False, 12, backward=False)
    assert info.iterations == 12 and not info.flags & _hip.PCG_SPLIT_START
    for b in (0, B - 1):
        err = rel_err(u[b].cpu().numpy(), _oracle("tail", B, b))
        print(f"B={B} sample {b}: vs oracle {err:.2e}")
        assert err < RTOL_U
