"""The lattice path's V-cycle, full-multigrid start and PCG driver (csrc/lattice_cycle.hip, lattice_pcg.hip and the strip,
two-samples-per-lane and fused kernel families they dispatch to) against the numpy model of oracle/lattice_model.py.

Every other lattice test solves to convergence (a converged PCG returns the right u for any symmetric positive-definite
preconditioner: a wrong cycle only costs iterations) or compares two settings of the same kernels.  Here the PCG is cut
after k = 0, 1 and 3 iterations (tol = 1e-300, no floor, no energy rule, max_iter = k): the solve returns x_k + z_k / rs, a
deterministic function of the level matrices and b; from a zero start x_0 = M b is the cycle applied once.

The GPU tests hand the model what the device holds: the level matrices of _Engine.lattice_assemble, the coefficient
copies of _LatticeSolve._cycle_coeffs / _Engine.pack_cycle_coeffs / plan.shared_fp32 and the dense inverse of
plan.dense_coarse, read back.  The CPU tests build the same hierarchy with numpy.

Tolerances are not picked.  Per case the model runs twice on the CPU on the columns _subset(B): float64 and longdouble
with every sum reversed (fp64 cases), or fp32-stored with fp64 arithmetic and fp32-stored with fp32 arithmetic and the
sums reversed (fp32 cases).  The tolerance is 16 x the largest difference of the two (relative to |x|_inf per sample, over
k), never below 2^-46 for fp64 cases.  The factor covers FMA contraction and the block-partial summation orders, which
the model does not reproduce.  test_cases_tell_single_defects_apart keeps that tolerance meaningful: every applicable
mutation of the model moves x_0, x_1 or x_3 by more than 100 x the case's tolerance.

The cases of _shift_warm_cases run what reaction=, every HeatEquation step and EigenFESolver(shift=) run: a factored
operator with the diagonal shift c M_L (dia_strip_shift_kernel on the strip levels, the shift_at terms of the generic
kernels below, no dense level, the driver's one-pass start on a cycle that splits it), reaction terms on the stored
diagonals of unfactored operators, and the warm start (DIFFHE_PCG_WARM: x = g + FMG(b - A g) / rs, or the guess's own
residual).  The shifts are c x the lumped mass of each level's own triangulation; the `graded` lattice makes that mass
differ from node to node, so that a shift read from the wrong row or column shows.

The tests print every figure before they assert (run with -s); the MEASURED table at the end of this file records one run.
"""
import functools
import os
import types
import warnings

import numpy as np
import pytest
import torch

from diffhe import FEMesh, _hip
from diffhe.plan import coarsening_step, lattice_elements, padded_batch
from oracle import lattice_model as lm
from oracle import p1_oracle as orc

T64 = torch.float64
DEV = "cuda:0"
EPS = float(np.finfo(np.float64).eps)
TOL_FLOOR = 2.0 ** -46
KS = (0, 1, 3)
N_COARSE = 8            # DifferentiableFESolver's mg["n_coarse"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "difffe-physics-lab_amd", "csrc")
T = lm.thresholds(*(open(os.path.join(CSRC, f)).read() for f in ("lattice.h", "lattice_layout.h", "lattice_cycle.hip")))
MIN_W, MIN_ROWS = T["min_w"], T["min_rows"]
POINT = 4.0             # |point load| / |random part| of a right-hand side
GRADING = 2.2           # variant "graded": last spacing / first spacing per direction; the lumped mass spans 4.8 x
MG_DEFAULT = dict(nu=2, n_coarse=N_COARSE, fp32=1, fmg=0, floor=0, tol_energy=0.0)


def _subset(B):
    return np.array(sorted({c for c in (0, 1, 31, 32, B - 1, 64, 127) if c < B}), dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
# (nx, ny, width of the domain; its height is 1).  tail: the smallest lattice that halves and takes the strip kernels,
# W = 129 (the last strip is a TAIL strip), square cells; cheb: odd sizes, no coarsening, the whole cycle is the Chebyshev
# semi-iteration; two: two strip levels; wide: W > 300; tall: W = 161, several row tiles; unit / xonly: cells twice / four
# times as long in y as in x, the hierarchy halves x alone first.
SHAPES = {"simple": (40, 48, 1.0), "cheb": (MIN_W - 1, MIN_ROWS - 1, 2.0), "tail": (MIN_W, MIN_ROWS, 2.0),
          "two": (2 * MIN_W, 2 * MIN_ROWS, 2.0), "wide": (320, 128, 2.5), "tall": (160, 224, 1.0),
          "unit": (MIN_W, MIN_ROWS, 1.0), "xonly": (2 * MIN_W, MIN_ROWS, 1.0)}


class Case(types.SimpleNamespace):
    pass


def _case(shape, B, tag, variant="plain", c=0.0, warm=False, **mg):
    """c: the reaction coefficient (the operator gains c M_L: a factored one as a shift, others on their diagonals);
    warm: the solve starts from a guess (_guess)."""
    case = Case(shape=shape, B=B, Bp=padded_batch(B), variant=variant, mg=dict(MG_DEFAULT, **mg), c=float(c), warm=bool(warm))
    case.fp32 = bool(case.mg["fp32"])
    case.id = f"{shape}-{variant}-B{B}of{case.Bp}-{tag}"
    return case


# the two magnitudes of a reaction term c M_L.  On the `tail` lattice (h = 1 / 64, unit diagonal 4): 40 h^2 = 1e-2, a small
# part of the diagonal (a reaction term); 1e4 h^2 = 2.4, comparable (a backward-Euler step of dt = 1e-4)
C_SMALL, C_LARGE = 40.0, 1.0e4


def _shift_warm_cases():
    """Solves with a reaction term and / or from a guess.  Ids end in the reaction coefficient and in `warm`."""
    out = []
    fp = lambda fp32: f"fp{32 if fp32 else 64}"   # noqa: E731
    ctag = lambda c: "c40" if c == C_SMALL else "c1e4"   # noqa: E731
    for fp32 in (0, 1):
        # the generic kernels' shift terms, down to the Chebyshev level
        out.append(_case("simple", 5, f"{fp(fp32)}-c40", c=C_SMALL, fp32=fp32))
    out.append(_case("cheb", 64, "fp32-c1e4", c=C_LARGE))
    out.append(_case("cheb", 64, "fp64-c40", c=C_SMALL, fp32=0))
    # the shifted strip kernels on a lattice whose lumped mass differs from node to node
    for B in (64, 128, 70):
        for fp32 in (0, 1):
            for fmg in (0, 1):
                for c in (C_SMALL, C_LARGE):
                    out.append(_case("tail", B, f"{fp(fp32)}{'-fmg' if fmg else ''}-{ctag(c)}", variant="graded", c=c, fp32=fp32,
                                     fmg=fmg))
    out.append(_case("tail", 128, "fp32-fmg-c1e4-decades", variant="graded", c=C_LARGE, fmg=1, kappa="decades"))
    for B in (64, 128):     # four diagonals: STRIP_SHIFT(4), and a Gershgorin bound on the Chebyshev level
        out.append(_case("tail", B, "fp32-c1e4", variant="skew", c=C_LARGE))
        out.append(_case("tail", B, "fp64-c40", variant="skew", c=C_SMALL, fp32=0))
    out.append(_case("tail", 128, "fp32-fmg-c1e4", variant="pinned", c=C_LARGE, fmg=1))
    out.append(_case("tail", 128, "fp64-c1e4", variant="pinned", c=C_LARGE, fp32=0))
    for cyc in (1, 2):      # two shifted strip levels; the driver's have_b1 start against the split one
        for split in (0, 1):
            out.append(_case("two", 128, f"fp32-fmg{cyc}-split{split}-c1e4", c=C_LARGE, fmg=1, fmg_cycles=cyc,
                             split_start=split))
    out.append(_case("unit", 128, "fp32-c1e4", c=C_LARGE))          # semi-coarsening with a shift
    out.append(_case("xonly", 128, "fp64-c40", c=C_SMALL, fp32=0))
    # unfactored operators: the term sits on the stored diagonals of every level, whose rows no longer sum to zero
    out.append(_case("tail", 128, "fp32-h16-c1e4", variant="field", c=C_LARGE, h16=1))
    out.append(_case("tail", 128, "fp32-c40", variant="neumann", c=C_SMALL))
    # warm starts, with and without a shift
    for B in (64, 128):
        for fp32 in (0, 1):
            for fmg in (0, 1):
                for c in (0.0, C_LARGE):
                    out.append(_case("tail", B, f"{fp(fp32)}{'-fmg' if fmg else ''}{'-c1e4' if c else ''}-warm",
                                     variant="graded" if c else "plain", c=c, warm=True, fp32=fp32, fmg=fmg))
    out.append(_case("tail", 128, "fp32-fmg-c40-warm", variant="graded", c=C_SMALL, warm=True, fmg=1))
    out.append(_case("two", 128, "fp32-fmg-c1e4-warm", c=C_LARGE, warm=True, fmg=1))
    return out


def _cases():
    out = []
    for fp32 in (0, 1):
        out.append(_case("simple", 5, f"fp{32 if fp32 else 64}", fp32=fp32))
        for B in (64, 128):
            out.append(_case("cheb", B, f"fp{32 if fp32 else 64}", fp32=fp32))
    for B in (64, 128, 192, 256, 70):
        out.append(_case("tail", B, "fp64", fp32=0))
        out.append(_case("tail", B, "fp32"))
        out.append(_case("tail", B, "fp32-unfused", fused=0))
    out.append(_case("tail", 256, "fp32-pre2", pre4=0))
    for B in (64, 128):
        out.append(_case("tail", B, "fp32-densescalar", dense_mfma=0))
        out.append(_case("tail", B, "fp32-nostrip2", strip2=0))
    for B in (64, 128, 256):
        out.append(_case("tail", B, "fp32-fmg", fmg=1))
    out.append(_case("tail", 128, "fp64-fmg", fp32=0, fmg=1))
    for B in (128, 256):
        out.append(_case("two", B, "fp32"))
        for cyc in (1, 2):
            for split in (0, 1):
                out.append(_case("two", B, f"fp32-fmg{cyc}-split{split}", fmg=1, fmg_cycles=cyc, split_start=split))
    out.append(_case("wide", 128, "fp32"))
    for B in (64, 256):
        out.append(_case("tall", B, "fp32"))
        out.append(_case("tall", B, "fp64", fp32=0))
    for shape in ("unit", "xonly"):
        out.append(_case(shape, 128, "fp32"))
        out.append(_case(shape, 128, "fp64", fp32=0))
    for B in (64, 128):
        out.append(_case("tail", B, "fp32", variant="skew"))
        out.append(_case("tail", B, "fp64", variant="skew", fp32=0))
        out.append(_case("tail", B, "fp32-h16", variant="field", h16=1))
        out.append(_case("tail", B, "fp32-noh16", variant="field", h16=0))
        out.append(_case("tail", B, "fp64", variant="field", fp32=0))
    out.append(_case("tail", 128, "fp32", variant="decades"))
    out.append(_case("tail", 128, "fp32", variant="pinned"))
    out.append(_case("tail", 128, "fp64", variant="pinned", fp32=0))
    out.append(_case("tail", 128, "fp32", variant="neumann"))
    for step in (0, 1):
        for pair in (0, 1):
            if not (step and pair):          # both on: the default, "tail-plain-B128of128-fp32"
                out.append(_case("tail", 128, f"fp32-step{step}-pair{pair}", cg_fp32_steplength=step, resid_pair=pair))
    return out


CASES = _cases() + _shift_warm_cases()
_IDS = [c.id for c in CASES]
assert len(set(_IDS)) == len(_IDS)


def _seed(case):
    return sum(map(ord, case.id)) % 100000


# ------------------------------------------------------------------------------------------------------------------
# geometry, coefficients and right-hand sides (numpy)
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _geometry(shape, variant):
    """-> (nodes2d (ny + 1, nx + 1, 2), bc2d): FEMesh.rectangle's nodes and Dirichlet boundary; the variants move interior
    nodes (skew), pin interior nodes (pinned) or free one edge (neumann)."""
    nx, ny, width = SHAPES[shape]
    nodes, _, bn, _ = orc.mesh_rectangle(nx, ny, (0.0, width), (0.0, 1.0))
    xy = nodes.reshape(ny + 1, nx + 1, 2).copy()
    bc = np.zeros((ny + 1) * (nx + 1), dtype=bool)
    bc[bn] = True
    bc = bc.reshape(ny + 1, nx + 1)
    rng = np.random.default_rng(21)
    if variant == "skew":       # interior nodes moved as in test_lattice_strip_kernels_batch64: a fourth diagonal
        xy[1:-1, 1:-1] += rng.uniform(-0.2, 0.2, (ny - 1, nx - 1, 2)) * np.array([width / nx, 1.0 / ny])
    if variant == "pinned":     # 0.1 % of the nodes, as in test_lattice_with_many_interior_dirichlet_nodes
        pick = rng.choice(bc.size, max(4, int(0.001 * bc.size)), replace=False)
        bc.reshape(-1)[pick] = True
    if variant == "neumann":    # the edge x = width is free
        bc[1:-1, -1] = False
    if variant == "graded":     # axis-aligned, spacings in geometric progression: the last cell GRADING x the first in x and y
        for axis, (cells, length) in enumerate(((nx, width), (ny, 1.0))):
            t = (GRADING ** (np.arange(cells + 1) / (cells - 1)) - 1.0) / (GRADING ** (cells / (cells - 1)) - 1.0)
            xy[:, :, axis] = (length * t)[None, :] if axis == 0 else (length * t)[:, None]
    return xy, bc


def _lumped(xy):
    """(n) lumped P1 mass of the lattice's triangulation: a third of the area of every triangle at the node."""
    ny, nx = xy.shape[0] - 1, xy.shape[1] - 1
    el, p = lattice_elements(nx, ny), xy.reshape(-1, 2)
    d1, d2 = p[el[:, 1]] - p[el[:, 0]], p[el[:, 2]] - p[el[:, 0]]
    area = 0.5 * np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
    m = np.zeros(len(p))
    np.add.at(m, el.reshape(-1), np.repeat(area / 3.0, 3))
    return m


def _reaction(case, gxy, gbc):
    """c M_L of one level as _Engine.reaction_shifts / add_reaction take it: the level's own lumped mass, 0 on Dirichlet rows."""
    return np.where(gbc.reshape(-1), 0.0, case.c * _lumped(gxy))


def _hierarchy(xy, bc):
    """The level geometries of SolvePlan: [(nodes2d, bc2d), ...] by plan.coarsening_step."""
    out = []
    while len(out) < 16:
        out.append((xy, bc))
        step = coarsening_step(xy)
        if step is None:
            break
        xy, bc = xy[::step[0], ::step[1]], bc[::step[0], ::step[1]]
    return out


def _traits(case):
    """What the driver derives from the mesh: (closed boundary, regular cells, factored, dense level index or None)."""
    xy, bc = _geometry(case.shape, case.variant)
    closed = bool(bc[0].all() and bc[-1].all() and bc[:, 0].all() and bc[:, -1].all())
    dx, dy = np.abs(np.diff(xy[:, :, 0], axis=1)), np.abs(np.diff(xy[:, :, 1], axis=0))
    skew = max(float(np.abs(np.diff(xy[:, :, 1], axis=1)).max()), float(np.abs(np.diff(xy[:, :, 0], axis=0)).max()))
    hmin, hmax = min(float(dx.min()), float(dy.min())), max(float(dx.max()), float(dy.max()))
    regular = bool(hmin > 0 and hmax <= 2.0 * hmin and skew <= 1e-12 * hmax)
    factored = closed and case.variant != "field"
    geo = [dict(nx=g[0].shape[1] - 1, ny=g[0].shape[0] - 1) for g in _hierarchy(xy, bc)]
    didx = lm.dense_level(geo)
    # a reaction term leaves no dense level: a factored operator carries it as a shift, which no inverse of K_1 holds
    return closed, regular, factored, didx, didx if factored and not case.c else None


def _kappa(case):
    """Per-sample scalars (B) or, variant field, per-sample element fields (m, B) of a log-normal field, sigma 0.4."""
    nx, ny, _ = SHAPES[case.shape]
    rng = np.random.default_rng(_seed(case) + 7)
    if case.variant == "field":
        return np.exp(0.4 * rng.standard_normal((2 * nx * ny, case.B)))
    if case.variant == "decades" or case.mg.get("kappa") == "decades":
        return 10.0 ** rng.uniform(-2.0, 2.0, case.B)
    return rng.uniform(0.5, 2.0, case.B)


def _rhs(case):
    """(n, B): random right-hand sides whose norms spread over four decades plus one point load per sample, at a different
    interior node for each sample; 0 on Dirichlet rows."""
    nx, ny, _ = SHAPES[case.shape]
    _, bc = _geometry(case.shape, case.variant)
    rng = np.random.default_rng(_seed(case) + 1)
    n = (nx + 1) * (ny + 1)
    amp = 10.0 ** np.linspace(-2.0, 2.0, case.B)[rng.permutation(case.B)]
    b = rng.standard_normal((n, case.B)) * amp
    # the loaded node: anywhere (odd samples) or next to a Dirichlet node (even samples), where a defect of the transfers
    # at Dirichlet rows shows most
    free = ~bc
    near = free.copy()
    near[1:-1, 1:-1] &= bc[:-2, 1:-1] | bc[2:, 1:-1] | bc[1:-1, :-2] | bc[1:-1, 2:]
    near[0], near[-1], near[:, 0], near[:, -1] = False, False, False, False
    free, near = np.nonzero(free.reshape(-1))[0], np.nonzero(near.reshape(-1))[0]
    node = rng.choice(free, case.B, replace=False)
    node[0::2] = rng.choice(np.setdiff1d(near, node[1::2]), len(node[0::2]), replace=False)
    b[node, np.arange(case.B)] += POINT * np.sqrt(n) * amp
    b[bc.reshape(-1)] = 0.0
    return b


def _dia(xy, bc, kap):
    """The symmetric diagonals (4, n, B') of sum_e kappa_e k0_e on the lattice xy, Dirichlet rows made identity rows
    (kap (m, B') -- one column of ones: the unit matrix K_1)."""
    ny, nx = xy.shape[0] - 1, xy.shape[1] - 1
    n, W = (nx + 1) * (ny + 1), nx + 1
    el = lattice_elements(nx, ny)
    k0, _ = orc.element_matrices(xy.reshape(n, 2), el)
    rows = np.broadcast_to(el[:, :, None], k0.shape)
    diff = el[:, None, :] - el[:, :, None]
    e_idx = np.broadcast_to(np.arange(len(el))[:, None, None], k0.shape)
    v = np.zeros((4, n, kap.shape[1]))
    flat = bc.reshape(-1)
    for k, off in enumerate((0, 1, W, nx)):
        m = diff == off
        np.add.at(v[k], rows[m], k0[m][:, None] * kap[e_idx[m]])
        if k:
            dead = flat.copy()
            dead[:n - off] |= flat[off:]
            v[k][dead] = 0.0
    v[0][flat] = 1.0
    return v


def _coarse_kappa(kap, fine, coarse):
    """Per-element fields one level down: the mean over the children of the same orientation."""
    (fny, fnx), (cny, cnx) = fine, coarse
    k = kap.reshape(cny, fny // cny, cnx, fnx // cnx, 2, kap.shape[1])
    return k.mean(axis=(1, 3)).reshape(2 * cnx * cny, kap.shape[1])


def _pack_h16(vals, nx, osc):
    """dia_pack_h16_kernel in numpy: fp16 couplings times 1 / osc_b and the fp32 diagonal that keeps every row sum."""
    nd, n, _ = vals.shape
    h = lambda a: (a / osc).astype(np.float32).astype(np.float16)   # noqa: E731
    d = vals[0].copy()
    o16 = np.empty((nd - 1,) + vals.shape[1:], dtype=np.float16)
    for k, off in enumerate([1, nx + 1, nx][:nd - 1], 1):
        o16[k - 1] = h(vals[k])
        lost = vals[k] - osc * o16[k - 1].astype(np.float64)
        d[:n - off] += lost[:n - off]
        d[off:] += lost[:n - off]
    return d.astype(np.float32), o16


def _copies(levels, case, Bv):
    """The coefficient copies of _LatticeSolve._cycle_coeffs, made on the host, added to the level dicts."""
    mg = case.mg
    if not mg["fp32"]:
        return
    if Bv != 1 and mg.get("h16", 1):
        free_diag = np.where(levels[0]["is_bc"][:, None], 0.0, levels[0]["vals"][0])
        mant, expo = np.frexp(free_diag.max(axis=0))
        osc = np.ldexp(1.0, expo - (mant == 0.5))
        for lv in levels:
            lv["d32"], lv["o16"] = _pack_h16(lv["vals"], lv["nx"], osc)
            lv["vals32"], lv["osc"] = lv["d32"], osc
    elif Bv != 1:
        for lv in levels:
            lv["vals32"] = lv["vals"].astype(np.float32)
    elif mg.get("strip2", 1) and case.Bp % 64 == 0 and levels[0].get("shift") is None:
        for lv in levels:
            lv["vals32"] = lv["vals"].astype(np.float32)
            lv["rd32"] = (1.0 / lv["vals"][0]).astype(np.float32)


def _dense_inverse(lv, fp32):
    """plan._dense_coarse_build: the level's matrix inverted on the host, symmetrised, in the cycle's storage type."""
    d, n, W = lv["vals"], lv["vals"].shape[1], lv["nx"] + 1
    K = np.zeros((n, n))
    i = np.arange(n)
    K[i, i] = d[0]
    for k, off in enumerate([1, W, lv["nx"]][:lv["nd"] - 1], 1):
        j = i[:n - off]
        K[j, j + off] = K[j + off, j] = d[k][:n - off]
    inv = np.linalg.inv(K)
    inv = 0.5 * (inv + inv.T)
    return inv.astype(np.float32) if fp32 else inv


@functools.lru_cache(maxsize=None)
def _cpu_setup(idx):
    """-> (levels, scale or None, Bv): the case's hierarchy with every value computed on the host, the real columns."""
    case = CASES[idx]
    xy, bc = _geometry(case.shape, case.variant)
    closed, regular, factored, didx_all, didx = _traits(case)
    geo = _hierarchy(xy, bc)
    if didx is not None:
        geo = geo[:didx + 1]
    kap = _kappa(case)
    if factored:
        scale, k_l, Bv = kap, np.ones((2 * (xy.shape[0] - 1) * (xy.shape[1] - 1), 1)), 1
    else:
        nx, ny, _ = SHAPES[case.shape]
        scale, Bv = None, case.Bp
        k_l = kap if kap.ndim == 2 else np.broadcast_to(kap[None, :], (2 * nx * ny, case.B)).copy()
    levels = []
    for l, (gxy, gbc) in enumerate(geo):
        if l and k_l.shape[1] > 1:
            k_l = _coarse_kappa(k_l, (geo[l - 1][0].shape[0] - 1, geo[l - 1][0].shape[1] - 1),
                                (gxy.shape[0] - 1, gxy.shape[1] - 1))
        elif l:
            k_l = np.ones((2 * (gxy.shape[0] - 1) * (gxy.shape[1] - 1), 1))
        v = _dia(gxy, gbc, k_l)
        nd = 4 if np.any(v[3]) else 3
        if case.c and not factored:             # _Engine.add_reaction: on the stored diagonal of every level
            v[0] += _reaction(case, gxy, gbc)[:, None]
        levels.append(dict(nx=gxy.shape[1] - 1, ny=gxy.shape[0] - 1, nd=nd, is_bc=gbc.reshape(-1).copy(),
                           vals=v[:nd, :, 0] if Bv == 1 else v[:nd]))
        if case.c and factored:                 # _Engine.reaction_shifts
            levels[-1]["shift"] = _reaction(case, gxy, gbc)
    _copies(levels, case, Bv)
    if didx is not None and case.mg.get("dense_coarse", 1):
        levels[-1]["dense_inv"] = _dense_inverse(levels[-1], case.fp32)
    return levels, scale, Bv


def _forms(case, levels, scale, Bv):
    closed, regular, factored, didx_all, _ = _traits(case)
    mg = case.mg
    step = bool(closed and regular and didx_all is not None and mg.get("cg_fp32_steplength", 1))
    return lm.level_forms(levels, Bv, case.Bp, T, case.fp32, scale=scale, fused=mg.get("fused", 1), pre4=mg.get("pre4", 1),
                          dense_mfma=mg.get("dense_mfma", 1), split_start=mg.get("split_start", 0), fp32_step=step,
                          resid_pair=mg.get("resid_pair", 1), fmg=mg["fmg"], warm=case.warm)


def _model(case, levels, scale, Bv, second=False, columns=None, mutate=()):
    """The case's model: the first run (float64 arithmetic) or the second (longdouble / float32 arithmetic, sums
    reversed)."""
    forms = _forms(case, levels, scale, Bv)
    kw = dict(scale=scale, n_coarse=N_COARSE, coarse_lmax=lm.gershgorin_lmax(levels[-1]), fp32=case.fp32, columns=columns,
              fmg=case.mg["fmg"], fmg_cycles=case.mg.get("fmg_cycles", 1), warm=case.warm, mutate=mutate)
    if not second:
        return lm.LatticeModel(levels, forms, **kw)
    if case.fp32:
        return lm.LatticeModel(levels, forms, arith32=True, reverse=True, **kw)
    return lm.LatticeModel(levels, forms, dtype=np.longdouble, reverse=True, **kw)


def _rel(x, ref):
    """max_i |x - ref| / |ref|_inf per column."""
    ref = np.asarray(ref, dtype=np.longdouble)
    return np.asarray(np.max(np.abs(np.asarray(x, dtype=np.longdouble) - ref), axis=0) / np.max(np.abs(ref), axis=0),
                      dtype=np.float64)


def _tolerance(ra, rb, fp32):
    """16 x the largest difference of the two runs (x relative to |x|_inf per sample, over k); fp64 cases: never below
    2^-46.  -> (spread, tol)."""
    sx = max(float(_rel(ra.snap[k][0], rb.snap[k][0]).max()) for k in KS)
    return sx, 16.0 * sx if fp32 else max(16.0 * sx, TOL_FLOOR)


def _relres_scale(levels, scale, b):
    """What an error of x does to the relative residual, per sample: |relres(x + dx) - relres(x)| <= |A dx|_2 / |b|_2 <=
    sqrt(n) |A|_inf |dx|_inf / |b|_2.  The residual's own evaluation in fp64 adds at most (7 + 2) eps |A| |x| per row, the
    same expression with 9 eps in the place of the relative error of x.  -> (factor per sample, that addend)."""
    v = np.abs(levels[0]["vals"])
    v = v[:, :, None] if v.ndim == 2 else v
    rowsum = (v[0] + 2.0 * v[1:].sum(axis=0)).max(axis=0) * (1.0 if scale is None else np.maximum(scale, 1.0))
    if levels[0].get("shift") is not None:      # |s_b K_1 + diag(shift)|_inf <= s_b |K_1|_inf + max shift
        rowsum = rowsum + float(np.max(levels[0]["shift"]))
    return np.sqrt(v.shape[1]) * rowsum / np.linalg.norm(b, axis=0), 9 * EPS


@functools.lru_cache(maxsize=None)
def _guess(idx):
    """The guess of a warm case (n, B), None for the others: the model's x_1 of the same right-hand side from a cold
    start on the host-computed hierarchy, times a factor in [0.9, 1.1] per sample, plus noise of 1e-3 |x_1|_inf; 0 on
    Dirichlet rows.  An input like b: the same array goes to the model and to the device."""
    case = CASES[idx]
    if not case.warm:
        return None
    levels, scale, Bv = _cpu_setup(idx)
    cold = Case(**dict(vars(case), warm=False))
    x1 = np.asarray(_model(cold, levels, scale, Bv).pcg(_rhs(case), (1,)).snap[1][0], dtype=np.float64)
    rng = np.random.default_rng(_seed(case) + 3)
    g = x1 * rng.uniform(0.9, 1.1, case.B) + 1e-3 * np.max(np.abs(x1), axis=0) * rng.standard_normal(x1.shape)
    g[levels[0]["is_bc"]] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def _reference(idx):
    """Per case, on the host-computed hierarchy: both runs on the subset, and the tolerance."""
    case = CASES[idx]
    levels, scale, Bv = _cpu_setup(idx)
    b, sub, g = _rhs(case), _subset(case.B), _guess(idx)
    ra = _model(case, levels, scale, Bv, columns=sub).pcg(b, KS, g)
    rb = _model(case, levels, scale, Bv, second=True, columns=sub).pcg(b, KS, g)
    return ra, rb, _tolerance(ra, rb, case.fp32)


# ------------------------------------------------------------------------------------------------------------------
# CPU: the model is a multigrid, the cases reach their forms and tell single defects apart
# ------------------------------------------------------------------------------------------------------------------
def test_model_is_a_multigrid():
    """The model's PCG run to 1e-10 meets a sparse direct solve of the oracle's matrix, with a zero and a full-multigrid
    start, fp64 and fp32-stored; the cycle's matrix on a small level is symmetric and positive definite."""
    import scipy.sparse.linalg as spla
    nx, ny = 32, 24
    nodes, el, bn, _ = orc.mesh_rectangle(nx, ny, (0.0, 1.0), (0.0, 1.0))
    xy = nodes.reshape(ny + 1, nx + 1, 2)
    bc = np.zeros(len(nodes), dtype=bool)
    bc[bn] = True
    geo = _hierarchy(xy, bc.reshape(ny + 1, nx + 1))
    assert [g[0].shape[:2] for g in geo] == [(25, 33), (13, 17), (7, 9), (4, 5)]
    levels = []
    for gxy, gbc in geo:
        v = _dia(gxy, gbc, np.ones((2 * (gxy.shape[0] - 1) * (gxy.shape[1] - 1), 1)))
        levels.append(dict(nx=gxy.shape[1] - 1, ny=gxy.shape[0] - 1, nd=3, is_bc=gbc.reshape(-1), vals=v[:3, :, 0]))
    K, _ = orc.assemble_sparse(nodes, el, 1.0, np.zeros(len(nodes)))
    K = K.tolil()
    K[bn, :] = 0.0
    K[:, bn] = 0.0
    K[bn, bn] = 1.0
    rng = np.random.default_rng(5)
    b = rng.standard_normal((len(nodes), 3))
    b[bn] = 0.0
    scale = np.array([0.5, 1.0, 1.7])
    exact = spla.splu(K.tocsc()).solve(b) / scale
    # the model's level-0 operator is the oracle's matrix
    probe = lm.LatticeModel(levels, lm.level_forms(levels, 1, 4, T, False), scale=scale)
    assert np.abs(probe._A0(exact) - b).max() <= 1e-12 * np.abs(b).max()
    for fp32 in (False, True):
        for fmg in (False, True):
            forms = lm.level_forms(levels, 1, 4, T, fp32)
            model = lm.LatticeModel(levels, forms, scale=scale, n_coarse=N_COARSE, fp32=fp32, fmg=fmg)
            res = model.pcg(b, ks=(0, 12))
            print(f"fp32={fp32} fmg={fmg}: relres after 0 / 12 iterations {res.snap[0][1].max():.2e} / "
                  f"{res.snap[12][1].max():.2e}, error {_rel(res.snap[12][0], exact).max():.2e}")
            assert float(res.snap[12][1].max()) <= 1e-10 and float(_rel(res.snap[12][0], exact).max()) < 1e-8
            assert float(res.snap[0][1].max()) < (0.05 if fmg else 0.5)       # one cycle / the start already help
    M = lm.LatticeModel(levels, lm.level_forms(levels, 1, 4, T, False), n_coarse=N_COARSE).cycle_matrix(1)
    assert M.shape == (221, 221) and np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max()
    free = ~levels[1]["is_bc"]
    assert np.linalg.eigvalsh(0.5 * (M + M.T)[np.ix_(free, free)]).min() > 0


def test_model_is_a_multigrid_with_a_shift_and_from_a_guess():
    """On the graded TAIL lattice with per-sample scales and the shift c M_L re-discretised per level, c = 40 and 1e4: the
    model's level-0 operator is scale_b K + diag(shift) of the oracle's matrices, its PCG contracts from a zero, a
    full-multigrid and a warm start and meets a sparse direct solve."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    idx = _IDS.index("tail-graded-B64of64-fp64-c40")
    xy, bc = _geometry("tail", "graded")
    nodes, flat = xy.reshape(-1, 2), bc.reshape(-1)
    K, _ = orc.assemble_sparse(nodes, lattice_elements(*SHAPES["tail"][:2]), 1.0, np.zeros(len(nodes)))
    free = sp.diags((~flat).astype(np.float64))
    K = (free @ K @ free + sp.diags(flat.astype(np.float64))).tocsc()     # identity Dirichlet rows
    scale = np.array([0.5, 1.0, 1.7])
    b = _rhs(CASES[idx])[:, :3]
    for c in (C_SMALL, C_LARGE):
        case = Case(**dict(vars(CASES[idx]), c=c, B=3, Bp=4))
        geo = _hierarchy(xy, bc)
        assert [g[0].shape[:2] for g in geo] == [(65, 129), (33, 65), (17, 33), (9, 17), (5, 9), (3, 5)]
        levels = []
        for gxy, gbc in geo:
            v = _dia(gxy, gbc, np.ones((2 * (gxy.shape[0] - 1) * (gxy.shape[1] - 1), 1)))
            levels.append(dict(nx=gxy.shape[1] - 1, ny=gxy.shape[0] - 1, nd=3, is_bc=gbc.reshape(-1), vals=v[:3, :, 0],
                               shift=_reaction(case, gxy, gbc)))
        shift = levels[0]["shift"]
        assert np.all(shift[~flat] > 0) and not np.any(shift[flat])
        exact = np.stack([spla.splu((s * K + sp.diags(shift)).tocsc()).solve(b[:, j]) for j, s in enumerate(scale)], axis=1)
        probe = lm.LatticeModel(levels, lm.level_forms(levels, 1, 4, T, False), scale=scale)
        assert np.abs(probe._A0(exact) - b).max() <= 1e-12 * np.abs(b).max()
        cold = {}
        for fp32 in (False, True):
            for fmg in (False, True):
                for warm in (False, True):
                    forms = lm.level_forms(levels, 1, 4, T, fp32, scale=scale, fmg=fmg, warm=warm)
                    model = lm.LatticeModel(levels, forms, scale=scale, n_coarse=N_COARSE, fp32=fp32, fmg=fmg, warm=warm)
                    guess = 1.05 * cold[fp32, fmg] if warm else None
                    res = model.pcg(b, ks=(0, 1, 3, 12), x_init=guess)
                    cold.setdefault((fp32, fmg), np.asarray(res.snap[1][0]))
                    rr = [float(res.snap[k][1].max()) for k in (0, 3, 12)]
                    print(f"c={c:g} fp32={fp32} fmg={fmg} warm={warm}: relres after 0 / 3 / 12 iterations "
                          f"{rr[0]:.2e} / {rr[1]:.2e} / {rr[2]:.2e}, error {_rel(res.snap[12][0], exact).max():.2e}")
                    assert rr[2] <= 1e-10 and float(_rel(res.snap[12][0], exact).max()) < 1e-8
                    assert rr[0] < (0.1 if fmg or warm else 0.5) and rr[1] < 1e-2 * rr[0] + 1e-12


def test_heat_equation_takes_the_dispatch_the_shifted_warm_cases_pin():
    """HeatEquation's default options on the TAIL lattice with one kappa per sample: a factored operator with the shift
    M_L / (theta dt), the fp32 cycle, the full-multigrid start and a warm forward solve -- level for level the forms of
    the first step (cold: nothing kept yet) and of every later one (warm) are those of the cases above."""
    from diffhe.heat import HeatEquation
    cold = CASES[_IDS.index("tail-graded-B128of128-fp32-fmg-c1e4")]
    warm = CASES[_IDS.index("tail-graded-B128of128-fp32-fmg-c1e4-warm")]
    heat = HeatEquation(_mesh(cold), torch.from_numpy(_kappa(cold)), dt=1.0 / C_LARGE)
    s = heat.solver
    assert s.reaction == cold.c == warm.c and s.warm_start == "forward" and s.operator == "auto"
    assert (s.mg["fp32"], s.mg["fmg"], s.mg["nu"], s.mg["n_coarse"]) == (1, 1, 2, N_COARSE)
    assert _traits(cold)[:3] == (True, False, True)         # closed, graded cells, one scalar per sample: factored
    for case, is_warm in ((cold, False), (warm, True)):
        idx = _IDS.index(case.id)
        levels, scale, Bv = _cpu_setup(idx)
        assert Bv == 1 and all(lv.get("shift") is not None for lv in levels)
        product = lm.level_forms(levels, 1, padded_batch(case.B), T, s.mg["fp32"], scale=scale, fmg=s.mg["fmg"],
                                 warm=is_warm, fp32_step=0)
        assert product == _forms(case, levels, scale, Bv)
        D = product[None]
        assert (D["cvt_restrict"], D["prolong_resid"], D["warm"]) == ((True, False, False), (False, False, True))[is_warm]
        assert (D["rupd"], D["rpair"], D["step2"], D["p32"]) == (True, True, False, True)


def _expected_forms(case):
    """Which form each level takes, written down per case family by hand: {level: (pre, post, coarse)} + driver facts."""
    s, v, mg, Bp = case.shape, case.variant, case.mg, case.Bp
    two = Bp % 128 == 0
    spl = 2 if two else 1
    pre_spl = 4 if (Bp % 256 == 0 and mg.get("pre4", 1) and v != "skew") else spl
    simple = ("simple+residual+restrict", "prolong+simple", None)
    if not case.fp32 or (v != "field" and not mg.get("strip2", 1)):
        strip = ("strip_first2+strip_resid_restrict", "strip_prolong_sweep+sweep", None)
    elif v in ("field", "neumann"):
        fused_ps = two and mg.get("h16", 1) and mg.get("fused", 1)
        strip = ("fused_pre2", "fused_post2", None) if fused_ps else \
            ("strip_first2+strip_resid_restrict", "strip_prolong_sweep+sweep", None)
    elif mg.get("fused", 1):
        strip = (f"fused_pre{pre_spl}", f"fused_post{spl}", None)
    else:
        strip = (("strip2" if two else "strip") + "_first2+" + ("strip2" if two else "strip") + "_resid_restrict",
                 ("strip2" if two else "strip") + "_prolong_sweep+sweep", None)
    dense = (None, None, "dense_small" if Bp < 64 else
             "dense_mfma" if case.fp32 and mg.get("dense_mfma", 1) else "dense_solve")
    cheb = (None, None, "chebyshev")
    semi = (("strip2" if case.fp32 and two else "strip") + "_first2+residual+restrict", "prolong+strip_sweeps", None)
    if case.c and _traits(case)[2]:
        # a factored operator with a shift: the strip levels run dia_strip_shift_kernel whatever the storage type and the
        # batch (never strip2_* or fused_*), the hierarchy runs down to the last level the lattice can be halved to --
        # tail 128 x 64 -> 4 x 2, two 256 x 128 -> 4 x 2, simple 40 x 48 -> 5 x 6, unit 128 x 64 -> 64 x 64 -> 2 x 2,
        # xonly 256 x 64 -> 128 x 64 -> 64 x 64 -> 2 x 2 -- and that level is the Chebyshev semi-iteration
        strip = ("strip_first2+strip_resid_restrict", "strip_prolong_sweep+sweep", None)
        semi = ("strip_first2+residual+restrict", "prolong+strip_sweeps", None)
        return {"simple": [simple] * 3 + [cheb], "cheb": [cheb], "tail": [strip] + [simple] * 4 + [cheb],
                "two": [strip, strip] + [simple] * 4 + [cheb], "unit": [semi] + [simple] * 5 + [cheb],
                "xonly": [semi, semi] + [simple] * 5 + [cheb]}[s]
    if s == "simple":
        return [simple, dense]
    if s == "cheb":
        return [cheb]
    if s == "tail" and v in ("field", "neumann"):
        return [strip] + [simple] * 4 + [cheb]
    if s == "tail":
        return [strip, simple, dense]
    if s == "two":
        return [strip, strip, simple, dense]
    if s == "wide":
        return [strip, strip, simple, dense]
    if s == "tall":
        return [strip, simple, simple, dense]
    if s == "unit":
        return [semi, simple, dense]
    return [semi, semi, simple, dense]        # xonly


@pytest.mark.parametrize("idx", range(len(CASES)), ids=_IDS)
def test_cases_reach_the_forms_they_are_named_after(idx):
    """The dispatch of lattice.h / lattice_cycle.hip / lattice_pcg.hip restated (lattice_model.level_forms, thresholds
    parsed from the sources) gives, per case, the kernel form of every level that the case was written for."""
    case = CASES[idx]
    levels, scale, Bv = _cpu_setup(idx)
    forms = _forms(case, levels, scale, Bv)
    got = [(forms[l]["pre"], forms[l]["post"], forms[l]["coarse"]) for l in range(len(levels))]
    print(case.id, got, forms[None], [forms[l]["tile"] for l in range(len(levels))])
    assert got == _expected_forms(case)
    mg, D = case.mg, forms[None]
    strip0 = case.Bp >= 64 and case.shape != "simple"
    assert forms[0]["strip"] == strip0 and D["cg"] == ("fused_step" if strip0 else "unfused")
    shared = Bv == 1
    shifted = bool(case.c) and shared          # a factored operator with a reaction term carries it as a shift
    assert shifted == (levels[0].get("shift") is not None)
    assert D["rupd"] == (strip0 and case.fp32 and shared)
    assert D["rpair"] == (D["rupd"] and bool(mg.get("resid_pair", 1)))
    # the fp32 step length asks for cells no longer than twice their width ("unit", 2 : 1, still is; "xonly", 4 : 1, is
    # not), no skew, a closed boundary and a hierarchy that reaches the dense level ("cheb" has one level)
    regular = case.shape not in ("xonly", "cheb") and case.variant in ("plain", "decades", "pinned")
    assert D["step2"] == bool(D["rupd"] and regular and mg.get("cg_fp32_steplength", 1) and mg.get("strip2", 1)
                              and not shifted)
    # the start of a full-multigrid solve: the driver converts and restricts b in one pass whatever the operator, the
    # cycle fuses prolongation and residual of the fine level only without a shift; a warm start takes neither
    assert D["fused_start"] == bool(case.fp32 and shared and strip0 and not mg.get("split_start", 0)
                                    and case.shape in ("tail", "two", "wide", "tall"))
    fusable = D["fused_start"]
    assert D["cvt_restrict"] == bool(fusable and mg["fmg"] and not case.warm)
    assert D["prolong_resid"] == bool(fusable and mg["fmg"] and not case.warm and not shifted)
    assert D["warm"] == case.warm
    if shifted:     # no level of a shifted hierarchy reads a coefficient copy or runs the initial-guess cycle
        assert not any(forms[l]["coef32"] or forms[l]["guess"] for l in range(len(levels)))
        assert all(lv.get("vals32") is None and lv.get("rd32") is None for lv in levels)
    if case.shape == "wide":
        assert [forms[l]["tile"] for l in (0, 1)] == ["four", "short"] and levels[0]["nx"] + 1 > T["small_w"]
    if case.shape == "two" and not shifted:      # the initial-guess cycle of the full-multigrid start runs on level 1
        assert [forms[l]["guess"] for l in range(4)] == [False, True, False, False]
    if case.variant == "graded":    # what makes an index defect of the shift loads visible
        m = _lumped(_geometry(case.shape, case.variant)[0]).reshape(levels[0]["ny"] + 1, -1)[1:-1, 1:-1]
        assert m.max() >= 4.0 * m.min() and np.all(m[1:] != m[:-1]) and np.all(m[:, 1:] != m[:, :-1])
    if case.shape == "tail" and case.variant == "plain":
        assert levels[0]["nx"] + 1 == MIN_W + 1 and (MIN_W + 1) % 4 == 1      # W = 129: the last strip is one column
    assert (levels[0]["nd"] == 4) == (case.variant == "skew")


def _skip_reason(mut, case, probe):
    """Why a mutation is not asked of a case (None: it is)."""
    if mut in lm.EQUIVALENT:
        return "mathematically the same cycle"
    if not probe.applies(mut):
        return "the hierarchy has nothing the mutation would break"
    if mut == "cheby_degree_off" and case.fp32 and probe.nl > 1:
        # below a hierarchy the semi-iteration solves a 5 x 3 lattice (3 free nodes) at degree >= n_coarse = 8: one step
        # more or less changes its result by less than the fp32 store resolves after two levels of interpolation.  The
        # single-level "cheb" cases and the fp64 cases of the same hierarchies ask for it
        return "below the resolution of the fp32 store"
    if mut == "h16_no_rowsum" and _traits(case)[0]:
        # the row sums move the diagonal by at most 2^-11 of itself (fp16 couplings), so one cycle by at most 4.9e-4 of
        # x, and 100 x the fp32 tolerance is 3e-4 .. 4e-4: on a closed lattice of this size the rule cannot resolve it.
        # What the row sums protect is the smooth modes, lambda_min(D^-1 A) << 2^-11: the lattice with a free edge asks
        return "at most 2^-11 of the diagonal: within 100 x the fp32 tolerance on a closed lattice"
    if mut == "cheby_degree_off" and case.c and probe.nl > 1:
        # a hierarchy with a reaction term has no dense level and ends on a 4 x 2 (5 x 6, 2 x 2) lattice, where c M_L --
        # which grows by 4 per level while K stays as it is -- dominates the diagonal: the operator is well conditioned
        # there and below, the smoothers of the finer levels leave that level next to nothing to correct.  Measured by the
        # model, not assumed: with the coarsest solve returning 0 the iterates move by _coarsest_share, and the last of
        # the >= 8 Chebyshev steps changes that solve by at most 1 / T_7(sigma) + 1 / T_8(sigma) of itself
        # (cheby_last_step_share, 7e-3 on the 4 x 2 lattice).  The single-level shifted "cheb" cases ask for the degree
        idx = _IDS.index(case.id)
        share = _coarsest_share(idx) * probe.cheby_last_step_share()
        if not share > 100.0 * _reference(idx)[2][1]:
            return "one Chebyshev step of the coarsest level moves the iterates by less than 100 x the tolerance"
    if mut in ("shift_tail", "shift_dropped_residual") and case.fp32 and probe.shift_share() < 1e-2:
        # a shift of less than 1 % of the diagonal, dropped in the eight columns of the two clamped strips (of 129) or in
        # the one residual that feeds the restriction: a perturbation of the cycle of at most 1e-2 x the share of it that
        # is touched, against 100 x the fp32 tolerance = 1e-4 .. 3e-4.  The fp64 cases of the same lattice and the fp32
        # cases at c = 1e4 (the shift 40 % of the diagonal) ask
        return "a partial defect of a shift below 1 % of the diagonal: within 100 x the fp32 tolerance"
    return None


def _moved(r, ref):
    """The largest distance of two runs' iterates over k; a run that has left the finite numbers has moved without bound."""
    with np.errstate(invalid="ignore"):
        moved = max(float(_rel(r.snap[k][0], ref.snap[k][0]).max()) for k in KS)
    return moved if np.isfinite(moved) else float("inf")


@functools.lru_cache(maxsize=None)
def _coarsest_share(idx):
    """How far x_0, x_1, x_3 move when the coarsest level's solve returns 0: no defect of that solve can do more."""
    case = CASES[idx]
    levels, scale, Bv = _cpu_setup(idx)
    r0 = _model(case, levels, scale, Bv, columns=_subset(case.B), mutate=("coarse_zero",)).pcg(_rhs(case), KS, _guess(idx))
    return _moved(r0, _reference(idx)[0])


@pytest.mark.parametrize("idx", range(len(CASES)), ids=_IDS)
def test_cases_tell_single_defects_apart(idx):
    """Each mutation of the model that applies to the case moves x_0, x_1 or x_3 by more than 100 x the case's tolerance."""
    case = CASES[idx]
    levels, scale, Bv = _cpu_setup(idx)
    ra, _, (spread, tol) = _reference(idx)
    b, sub = _rhs(case), _subset(case.B)
    probe = _model(case, levels, scale, Bv, columns=sub)
    seen = {}
    for mut in lm.MUTATIONS:
        if _skip_reason(mut, case, probe):
            continue
        with np.errstate(all="ignore"):     # a smoother without the shift in its diagonal diverges: that is the finding
            seen[mut] = _moved(_model(case, levels, scale, Bv, columns=sub, mutate=(mut,)).pcg(b, KS, _guess(idx)), ra)
    print(f"LATTICECYCLE-MUT {case.id} spread={spread:.3e} tol={tol:.3e} " +
          " ".join(f"{m}={v:.2e}" for m, v in seen.items()))
    missed = {mut: moved for mut, moved in seen.items() if not moved > 100.0 * tol}
    assert not missed, (case.id, missed, tol, spread)


_ORDER = [i for i, c in enumerate(CASES) if c.Bp <= 64 and not c.fp32]


@pytest.mark.parametrize("mut", lm.EQUIVALENT)
@pytest.mark.parametrize("idx", _ORDER, ids=lambda i: _IDS[i])
def test_sweep_order_is_immaterial(idx, mut):
    """The order of the two post-sweeps, and of the two pre-sweeps, changes nothing but roundings (see EQUIVALENT in the
    model): the fp64 iterates of the model with that order swapped lie within the case's own tolerance of the model's."""
    case = CASES[idx]
    levels, scale, Bv = _cpu_setup(idx)
    ra, _, (spread, tol) = _reference(idx)
    rm = _model(case, levels, scale, Bv, columns=_subset(case.B), mutate=(mut,)).pcg(_rhs(case), KS, _guess(idx))
    assert _moved(rm, ra) <= tol


def test_every_mutation_applies_to_some_case():
    asked = set()
    for idx, c in enumerate(CASES):
        levels, scale, Bv = _cpu_setup(idx)
        probe = _model(c, levels, scale, Bv, columns=_subset(c.B))
        asked |= {mut for mut in lm.MUTATIONS if _skip_reason(mut, c, probe) is None}
    assert asked == set(lm.MUTATIONS) - set(lm.EQUIVALENT)


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _mesh(case):
    xy, bc = _geometry(case.shape, case.variant)
    nx, ny, _ = SHAPES[case.shape]
    return FEMesh(nodes=torch.from_numpy(xy.reshape(-1, 2).copy()), elements=torch.from_numpy(lattice_elements(nx, ny)),
                  dirichlet_nodes=dict.fromkeys(np.nonzero(bc.reshape(-1))[0].tolist(), 0.0))


def _device_setup(case):
    """The driver's own set-up calls (_LatticeSolve.forward) -> (engine, arguments of lattice_pcg, the model's level dicts
    read back from the device, scale, Bv)."""
    from diffhe.plan import get_plan
    from diffhe.solver import _Engine, _LatticeSolve, K_SAMPLE, K_SAMPLE_ELEM
    dev = torch.device(DEV)
    plan = get_plan(_mesh(case), dev)
    closed, regular, factored, didx_all, didx = _traits(case)
    assert plan.is_lattice and plan.closed_boundary == closed and plan.regular_cells == regular
    assert plan.dense_level() == didx_all
    eng = _Engine(plan, 1e-300, 0, 1, "gather")
    kap, B, Bp, mg = _kappa(case), case.B, case.Bp, case.mg
    field = kap.ndim == 2
    kt = torch.from_numpy(np.ascontiguousarray(kap.T if field else kap))
    vals, Bv, scale, _, _ = eng.lattice_assemble(kt, K_SAMPLE_ELEM if field else K_SAMPLE, B, Bp, factor=closed,
                                                 n_levels=None if didx is None else didx + 1)
    assert (Bv == 1) == factored
    # the reaction term as _LatticeSolve.forward adds it: the shifts of a factored operator, else on the stored diagonals
    shift = eng.reaction_shifts(case.c, len(vals)) if case.c and factored else None
    if case.c and not factored:
        eng.add_reaction(vals, case.c, lattice=True)
    stand_in = types.SimpleNamespace(mg=mg, Bp=Bp, eng=eng, plan=plan, shift=shift, factored=factored)
    vals32, rdiag32, off16 = _LatticeSolve._cycle_coeffs(stand_in, vals, Bv)
    dense = plan.dense_coarse(didx, vals, case.fp32) if didx is not None else None
    torch.cuda.synchronize()
    host = lambda t: t.detach().cpu().numpy()   # noqa: E731
    levels = []
    for l, v in enumerate(vals):
        lev = plan.levels[l]
        hv = host(v)
        lv = dict(nx=lev.nx, ny=lev.ny, nd=lev.nd, is_bc=host(lev.is_bc).astype(bool),
                  vals=hv[:, :, 0] if Bv == 1 else hv[:, :, :B], full=hv)
        if off16 is not None:
            lv["d32"], lv["o16"], lv["osc"] = host(vals32[l])[:, :B], host(off16[0][l])[:, :, :B], host(off16[1])[:B]
            lv["vals32"] = lv["d32"]
        elif vals32 is not None and Bv != 1:
            lv["vals32"] = host(vals32[l])[:, :, :B]
        elif vals32 is not None:
            lv["vals32"], lv["rd32"] = host(vals32[l])[:, :, 0], host(rdiag32[l]).reshape(-1)
        if shift is not None:
            lv["shift"] = host(shift[l]).reshape(-1)
        levels.append(lv)
    if dense is not None:
        levels[-1]["dense_inv"] = host(dense[1])
    sc = None if scale is None else host(scale)[:B]
    if shift is not None:       # as in production: no shared fp32 copy of a shifted operator
        assert vals32 is None and rdiag32 is None and off16 is None
    args = dict(vals=vals, Bv=Bv, scale=scale, vals32=vals32, dense=dense, rdiag32=rdiag32, off16=off16, shift=shift)
    return eng, args, levels, sc, Bv


def _solve(eng, args, b_dev, case, k, x0=None):
    """_Engine.lattice_pcg with max_iter = k on outputs pre-filled with garbage (a warm start's x is the guess's clone)."""
    n, Bp = b_dev.shape
    eng.max_iter = k
    inner = eng._solve

    def prefilled(Bp_, launch, x=None, **kw):
        def go(x_, relres, iters, st):
            relres.fill_(float("nan"))
            iters.fill_(-7)
            st.fill_(-1)
            launch(x_, relres, iters, st)
        return inner(Bp_, go, x=torch.full((n, Bp), float("nan"), dtype=T64, device=DEV) if x is None else x, **kw)

    eng._solve = prefilled
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            res = eng.lattice_pcg(args["vals"], args["Bv"], args["scale"], b_dev, Bp, case.mg, args["vals32"], args["dense"],
                                  x0=x0, shift=args["shift"], rdiag32=args["rdiag32"], off16=args["off16"])
        torch.cuda.synchronize()
    finally:
        del eng._solve
    return res


def _expected_flags(case):
    mg = case.mg
    closed, regular, _, didx_all, _ = _traits(case)
    step = closed and regular and didx_all is not None and mg.get("cg_fp32_steplength", 1)
    return (mg["fp32"] * _hip.PCG_FP32 | mg["fmg"] * _hip.PCG_FMG | (mg.get("fmg_cycles", 1) - 1) << _hip.PCG_FMG_CYCLES_SHIFT
            | _hip.PCG_NO_FLOOR | (0 if mg.get("fused", 1) else _hip.PCG_UNFUSED)
            | (0 if mg.get("dense_mfma", 1) else _hip.PCG_DENSE_SCALAR) | (0 if mg.get("pre4", 1) else _hip.PCG_PRE2)
            | (0 if mg.get("resid_pair", 1) else _hip.PCG_RESID_FP64) | (_hip.PCG_WARM if case.warm else 0)
            | (_hip.PCG_SPLIT_START if mg.get("split_start", 0) else 0) | (_hip.PCG_CLOSED_FP32_STEP if step else 0))


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=_IDS)
def test_truncated_lattice_pcg_is_the_models(idx):
    """x and relres of diffhe_lattice_pcg_solve after 0, 1 and 3 iterations against the model of the levels the device
    holds: the first run on every real column, the second on the subset; padding columns exactly 0."""
    case = CASES[idx]
    eng, args, levels, scale, Bv = _device_setup(case)
    B, Bp = case.B, case.Bp
    forms = _forms(case, levels, scale, Bv)
    if case.fp32 and Bv != 1:       # the packing did not fall back: the coefficient form is the one the case is about
        assert (args["off16"] is not None) == bool(case.mg.get("h16", 1))
    b, sub = _rhs(case), _subset(B)
    lmax = lm.gershgorin_lmax(dict(levels[-1], vals=levels[-1]["full"]))
    kw = dict(scale=scale, n_coarse=N_COARSE, coarse_lmax=lmax, fp32=case.fp32, fmg=case.mg["fmg"],
              fmg_cycles=case.mg.get("fmg_cycles", 1), warm=case.warm)
    guess = _guess(idx)
    r_all = lm.LatticeModel(levels, forms, **kw).pcg(b, KS, guess)
    r_a = lm.LatticeModel(levels, forms, columns=sub, **kw).pcg(b, KS, guess)
    second = dict(arith32=True, reverse=True) if case.fp32 else dict(dtype=np.longdouble, reverse=True)
    r_b = lm.LatticeModel(levels, forms, columns=sub, **second, **kw).pcg(b, KS, guess)
    spread, tol = _tolerance(r_a, r_b, case.fp32)
    rscale = _relres_scale(levels, scale, b)
    b_pad = np.zeros((b.shape[0], Bp))
    b_pad[:, :B] = b
    b_dev = torch.from_numpy(b_pad).to(DEV)
    x0 = keep = None
    if case.warm:               # the guess, 0 in the padding columns; the solve must leave the caller's tensor as it is
        g_pad = np.zeros((b.shape[0], Bp))
        g_pad[:, :B] = guess
        x0 = torch.from_numpy(g_pad).to(DEV)
        keep = x0.clone()
    fails = []
    for k in KS:
        res = _solve(eng, args, b_dev, case, k, x0)
        if case.warm:
            assert torch.equal(x0, keep) and res.x.data_ptr() != x0.data_ptr() and res.flags & _hip.PCG_WARM
        x, relres = res.x.cpu().numpy(), res.relres.cpu().numpy()
        ma, mb = r_all.snap[k], r_b.snap[k]
        da, db = _rel(x[:, :B], ma[0]), _rel(x[:, sub], mb[0])
        tol_r = (tol + rscale[1]) * rscale[0] * np.max(np.abs(ma[0]), axis=0)
        ra_, rb_ = np.abs(relres[:B] - ma[1]) / tol_r, np.abs(relres[sub] - np.asarray(mb[1], dtype=np.float64)) / tol_r[sub]
        print(f"LATTICECYCLE {case.id} k={k} spread={spread:.3e} tol={tol:.3e} gpu_vs_first={da.max():.3e} "
              f"gpu_vs_second={db.max():.3e} relres_vs_first/bound={ra_.max():.3e} relres_vs_second/bound={rb_.max():.3e} "
              f"relres={relres[:B].max():.3e}")
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(relres))
        assert (res.iterations, res.not_converged) == (k, B if k else 0)
        assert res.flags == _expected_flags(case), (hex(res.flags), hex(_expected_flags(case)))
        rule = res.rule.cpu().numpy()
        assert not np.any(rule[:B]) and np.all(rule[B:] == 1)       # the cap ended the real samples; b = 0: solved by 0
        assert not np.any(x[:, B:]) and not np.any(relres[B:])       # exactly what a zero right-hand side gives
        if not (da.max() <= tol and db.max() <= tol and ra_.max() <= 1.0 and rb_.max() <= 1.0):
            fails.append((k, float(da.max()), float(db.max()), float(ra_.max()), float(rb_.max())))
    assert not fails, (case.id, tol, fails)


@pytest.mark.gpu
@pytest.mark.parametrize("cyc", (1, 2))
def test_shifted_start_forms_agree(cyc):
    """Two shifted strip levels, full-multigrid start: the driver's start (b converted and restricted in one pass, the
    level-1 right-hand side handed to a cycle that, because of the shift, prolongs and takes the residual in two passes)
    against DIFFHE_PCG_SPLIT_START on the same scales and right-hand sides, x after 0, 1 and 3 iterations -- within the
    case's tolerance (computed on the CPU from the model on the host-built hierarchy)."""
    idx = _IDS.index(f"two-plain-B128of128-fp32-fmg{cyc}-split0-c1e4")
    fused = CASES[idx]
    split = Case(**dict(vars(fused), mg=dict(fused.mg, split_start=1)))     # the same id: the same kappa and b
    tol = _reference(idx)[2][1]
    b_dev = torch.from_numpy(_rhs(fused)).to(DEV)
    xs = []
    for case in (fused, split):
        eng, args, levels, scale, Bv = _device_setup(case)
        assert args["shift"] is not None and len(levels) == 7
        res = [_solve(eng, args, b_dev, case, k) for k in KS]
        assert all(r.flags == _expected_flags(case) for r in res)
        xs.append([r.x.cpu().numpy() for r in res])
    for k, xa, xb in zip(KS, *xs):
        d = float(_rel(xb, xa).max())
        print(f"LATTICECYCLE-START fmg{cyc} k={k} split1_vs_split0={d:.3e} tol={tol:.3e}")
        assert d <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("tag,mg,storage", [("fp64", dict(fp32=0), "fp64"), ("fp32", dict(fp32=1), "shared-fp32"),
                                            ("field", dict(fp32=1), "fp16-rowsum"),
                                            ("field-noh16", dict(fp32=1, h16=0), "fp32")])
def test_solver_reports_the_path_and_coefficient_storage(tag, mg, storage):
    """DifferentiableFESolver on the TAIL lattice: the path, the coefficient storage and the flags it reports are the
    ones the truncated solves above were given."""
    from diffhe import DifferentiableFESolver
    case = _case("tail", 128, "report", variant="field" if tag.startswith("field") else "plain", **mg)
    kap = _kappa(case)
    kt = torch.from_numpy(np.ascontiguousarray(kap.T if kap.ndim == 2 else kap)).to(DEV)
    solver = DifferentiableFESolver(_mesh(case), kt, device=DEV, tol=1e-300, max_iter=1, mg=dict(mg, floor=0, fmg=0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        solver(torch.from_numpy(np.ascontiguousarray(_rhs(case).T)).to(DEV))
    info = solver.last_info
    assert info.path == "lattice-mgpcg" and info.coeff_storage == storage and info.iterations == 1
    assert info.flags & ~_hip.PCG_FMG == _expected_flags(case) & ~_hip.PCG_FMG


# MEASURED on an MI355X, the largest over k = 0, 1, 3, relative to |x|_inf per sample: the spread of the two model runs,
# the tolerance derived from it, the GPU's distance from the first model run (all columns) and from the second (subset),
# and the largest |relres - model| over its bound.  Recorded, not asserted: every assertion's numbers come from the CPU.
#   case                                              spread       tol  vs first vs second   relres
#   simple-plain-B5of8-fp64                          2.1e-16   1.4e-14   5.5e-16   3.8e-16  1.7e-04
#   cheb-plain-B64of64-fp64                          6.3e-16   1.4e-14   2.8e-15   8.2e-16  1.4e-04
#   cheb-plain-B128of128-fp64                        2.1e-15   3.4e-14   2.6e-15   9.2e-16  4.0e-05
#   simple-plain-B5of8-fp32                          1.7e-07   2.7e-06   6.2e-15   1.7e-07  4.8e-05
#   cheb-plain-B64of64-fp32                          5.9e-07   9.5e-06   2.9e-07   6.5e-07  8.9e-05
#   cheb-plain-B128of128-fp32                        5.4e-07   8.7e-06   3.6e-07   6.3e-07  1.0e-04
#   tail-plain-B64of64-fp64                          6.9e-16   1.4e-14   2.6e-15   3.9e-16  1.4e-04
#   tail-plain-B64of64-fp32                          1.6e-07   2.5e-06   2.0e-07   2.1e-07  1.5e-04
#   tail-plain-B64of64-fp32-unfused                  1.4e-07   2.2e-06   1.1e-07   2.0e-07  1.5e-04
#   tail-plain-B128of128-fp64                        1.3e-15   2.1e-14   1.7e-15   3.6e-16  1.1e-04
#   tail-plain-B128of128-fp32                        1.3e-07   2.0e-06   2.2e-07   1.1e-07  1.9e-04
#   tail-plain-B128of128-fp32-unfused                1.9e-07   3.1e-06   1.9e-07   1.5e-07  8.0e-05
#   tail-plain-B192of192-fp64                        1.6e-15   2.5e-14   1.6e-15   5.8e-16  7.4e-05
#   tail-plain-B192of192-fp32                        1.4e-07   2.2e-06   2.2e-07   1.9e-07  2.0e-04
#   tail-plain-B192of192-fp32-unfused                1.7e-07   2.8e-06   1.4e-07   1.7e-07  1.1e-04
#   tail-plain-B256of256-fp64                        7.5e-16   1.4e-14   2.2e-15   1.2e-15  9.3e-05
#   tail-plain-B256of256-fp32                        1.8e-07   2.8e-06   2.3e-07   1.8e-07  1.7e-04
#   tail-plain-B256of256-fp32-unfused                1.5e-07   2.4e-06   2.1e-07   1.2e-07  1.2e-04
#   tail-plain-B70of128-fp64                         6.5e-16   1.4e-14   1.7e-15   5.4e-16  1.0e-04
#   tail-plain-B70of128-fp32                         1.9e-07   3.0e-06   2.1e-07   3.0e-07  1.2e-04
#   tail-plain-B70of128-fp32-unfused                 8.0e-08   1.3e-06   1.4e-07   1.2e-07  2.2e-04
#   tail-plain-B256of256-fp32-pre2                   1.6e-07   2.6e-06   1.8e-07   2.2e-07  1.6e-04
#   tail-plain-B64of64-fp32-densescalar              1.8e-07   2.8e-06   1.8e-07   1.6e-07  1.3e-04
#   tail-plain-B64of64-fp32-nostrip2                 1.4e-07   2.3e-06   1.2e-07   1.3e-07  1.5e-04
#   tail-plain-B128of128-fp32-densescalar            1.7e-07   2.7e-06   2.1e-07   2.0e-07  1.4e-04
#   tail-plain-B128of128-fp32-nostrip2               2.1e-07   3.4e-06   1.3e-07   1.7e-07  8.8e-05
#   tail-plain-B64of64-fp32-fmg                      2.3e-08   3.6e-07   7.5e-09   2.1e-08  7.0e-05
#   tail-plain-B128of128-fp32-fmg                    1.1e-08   1.8e-07   7.2e-09   1.2e-08  1.0e-04
#   tail-plain-B256of256-fp32-fmg                    2.2e-08   3.6e-07   7.8e-09   2.2e-08  6.9e-05
#   tail-plain-B128of128-fp64-fmg                    8.9e-16   1.4e-14   1.4e-15   6.9e-16  8.0e-05
#   two-plain-B128of128-fp32                         1.4e-07   2.2e-06   2.2e-07   1.5e-07  8.8e-05
#   two-plain-B128of128-fp32-fmg1-split0             4.1e-08   6.6e-07   8.7e-09   4.4e-08  1.8e-05
#   two-plain-B128of128-fp32-fmg1-split1             4.3e-08   7.0e-07   1.3e-08   4.5e-08  1.6e-05
#   two-plain-B128of128-fp32-fmg2-split0             4.0e-08   6.5e-07   1.1e-08   4.0e-08  2.2e-05
#   two-plain-B128of128-fp32-fmg2-split1             3.5e-08   5.6e-07   9.5e-09   3.4e-08  1.5e-05
#   two-plain-B256of256-fp32                         1.3e-07   2.1e-06   3.0e-07   1.9e-07  1.2e-04
#   two-plain-B256of256-fp32-fmg1-split0             2.7e-08   4.3e-07   9.7e-09   2.7e-08  3.2e-05
#   two-plain-B256of256-fp32-fmg1-split1             3.8e-08   6.0e-07   1.2e-08   3.7e-08  2.3e-05
#   two-plain-B256of256-fp32-fmg2-split0             3.0e-08   4.9e-07   1.1e-08   3.3e-08  2.5e-05
#   two-plain-B256of256-fp32-fmg2-split1             4.5e-08   7.2e-07   8.3e-09   4.7e-08  2.3e-05
#   wide-plain-B128of128-fp32                        9.9e-08   1.6e-06   2.9e-07   1.5e-07  1.0e-04
#   tall-plain-B64of64-fp32                          2.5e-07   4.1e-06   1.9e-07   3.5e-07  5.2e-05
#   tall-plain-B64of64-fp64                          1.3e-15   2.1e-14   4.3e-15   1.5e-15  8.3e-05
#   tall-plain-B256of256-fp32                        1.7e-07   2.8e-06   2.9e-07   2.1e-07  8.1e-05
#   tall-plain-B256of256-fp64                        2.1e-15   3.4e-14   5.7e-15   2.5e-15  5.2e-05
#   unit-plain-B128of128-fp32                        2.5e-07   4.1e-06   1.5e-07   2.3e-07  1.0e-04
#   unit-plain-B128of128-fp64                        1.3e-15   2.1e-14   2.5e-15   8.2e-16  5.9e-05
#   xonly-plain-B128of128-fp32                       2.2e-07   3.4e-06   1.6e-07   2.2e-07  9.9e-05
#   xonly-plain-B128of128-fp64                       1.7e-15   2.7e-14   8.6e-15   3.0e-15  3.4e-05
#   tail-skew-B64of64-fp32                           2.4e-07   3.9e-06   2.4e-07   2.2e-07  4.2e-05
#   tail-skew-B64of64-fp64                           1.5e-15   2.3e-14   1.9e-15   5.4e-16  2.8e-05
#   tail-field-B64of64-fp32-h16                      1.5e-07   2.5e-06   1.1e-07   1.5e-07  3.9e-05
#   tail-field-B64of64-fp32-noh16                    1.0e-07   1.6e-06   1.1e-07   1.0e-07  7.2e-05
#   tail-field-B64of64-fp64                          6.9e-16   1.4e-14   1.7e-15   4.3e-16  4.8e-05
#   tail-skew-B128of128-fp32                         1.7e-07   2.7e-06   2.3e-07   2.5e-07  9.7e-05
#   tail-skew-B128of128-fp64                         8.2e-16   1.4e-14   2.7e-15   5.8e-16  4.9e-05
#   tail-field-B128of128-fp32-h16                    1.5e-07   2.4e-06   1.9e-07   1.5e-07  6.1e-05
#   tail-field-B128of128-fp32-noh16                  1.3e-07   2.1e-06   1.2e-07   1.3e-07  4.8e-05
#   tail-field-B128of128-fp64                        1.6e-15   2.6e-14   1.9e-15   6.4e-16  3.0e-05
#   tail-decades-B128of128-fp32                      1.4e-07   2.2e-06   1.8e-07   1.4e-07  1.7e-04
#   tail-pinned-B128of128-fp32                       2.3e-07   3.8e-06   4.4e-07   1.6e-07  1.6e-04
#   tail-pinned-B128of128-fp64                       1.0e-15   1.6e-14   9.7e-15   4.0e-16  7.8e-04
#   tail-neumann-B128of128-fp32                      1.1e-07   1.8e-06   1.6e-07   1.8e-07  1.9e-04
#   tail-plain-B128of128-fp32-step0-pair0            1.5e-07   2.4e-06   2.0e-07   2.0e-07  2.0e-04
#   tail-plain-B128of128-fp32-step0-pair1            2.2e-07   3.6e-06   2.2e-07   1.5e-07  9.0e-05
#   tail-plain-B128of128-fp32-step1-pair0            2.2e-07   3.6e-06   2.2e-07   1.5e-07  9.0e-05
#
# The cases with a reaction term (c40, c1e4) and from a guess (warm), one run on an MI355X, same columns.  No kernel fell
# outside its tolerance: the largest distance is 0.17 of it (xonly-plain-B128of128-fp64-c40).  The shifted kernels compute
# in fp64 whatever they store, so the fp32 cases lie next to the first model run (fp64 arithmetic) and at the spread from
# the second; both start forms of the shifted `two` cases returned the same bits (split1 vs split0: 0.0 at k = 0, 1, 3).
#   case                                              spread       tol  vs first vs second   relres
#   simple-plain-B5of8-fp64-c40                       3.8e-16   1.4e-14   5.0e-16   2.1e-16  9.6e-05
#   simple-plain-B5of8-fp32-c40                       9.3e-08   1.5e-06   5.8e-15   9.3e-08  1.7e-04
#   cheb-plain-B64of64-fp32-c1e4                      2.3e-07   3.6e-06   1.2e-09   2.3e-07  2.6e-05
#   cheb-plain-B64of64-fp64-c40                       7.4e-16   1.4e-14   1.2e-15   5.1e-16  1.2e-04
#   tail-graded-B64of64-fp64-c40                      4.8e-16   1.4e-14   1.5e-15   2.3e-16  1.0e-04
#   tail-graded-B64of64-fp64-c1e4                     3.4e-16   1.4e-14   4.4e-16   2.8e-16  1.0e-04
#   tail-graded-B64of64-fp64-fmg-c40                  7.6e-16   1.4e-14   1.0e-15   2.9e-16  4.4e-05
#   tail-graded-B64of64-fp64-fmg-c1e4                 2.0e-16   1.4e-14   3.2e-16   1.8e-16  7.3e-05
#   tail-graded-B64of64-fp32-c40                      1.8e-07   3.0e-06   1.0e-07   1.8e-07  1.5e-04
#   tail-graded-B64of64-fp32-c1e4                     9.6e-08   1.5e-06   8.9e-08   9.6e-08  2.8e-04
#   tail-graded-B64of64-fp32-fmg-c40                  3.6e-08   5.7e-07   7.2e-09   4.1e-08  6.3e-05
#   tail-graded-B64of64-fp32-fmg-c1e4                 1.7e-09   2.8e-08   2.6e-09   1.7e-09  5.2e-04
#   tail-graded-B128of128-fp64-c40                    1.1e-15   1.8e-14   2.1e-15   2.4e-16  8.4e-05
#   tail-graded-B128of128-fp64-c1e4                   3.2e-16   1.4e-14   5.5e-16   2.8e-16  1.3e-04
#   tail-graded-B128of128-fp64-fmg-c40                3.8e-16   1.4e-14   1.1e-15   4.7e-16  4.9e-05
#   tail-graded-B128of128-fp64-fmg-c1e4               1.3e-16   1.4e-14   5.5e-16   2.0e-16  6.3e-05
#   tail-graded-B128of128-fp32-c40                    1.3e-07   2.1e-06   1.1e-07   1.3e-07  1.4e-04
#   tail-graded-B128of128-fp32-c1e4                   1.0e-07   1.6e-06   1.1e-07   1.0e-07  3.2e-04
#   tail-graded-B128of128-fp32-fmg-c40                3.7e-08   5.8e-07   9.1e-09   3.7e-08  1.7e-05
#   tail-graded-B128of128-fp32-fmg-c1e4               5.1e-09   8.1e-08   9.2e-09   5.1e-09  2.8e-04
#   tail-graded-B70of128-fp64-c40                     4.9e-16   1.4e-14   1.8e-15   2.4e-16  1.0e-04
#   tail-graded-B70of128-fp64-c1e4                    3.8e-16   1.4e-14   4.4e-16   1.6e-16  1.0e-04
#   tail-graded-B70of128-fp64-fmg-c40                 5.8e-16   1.4e-14   1.0e-15   3.0e-16  4.6e-05
#   tail-graded-B70of128-fp64-fmg-c1e4                2.6e-16   1.4e-14   4.4e-16   9.6e-17  5.8e-05
#   tail-graded-B70of128-fp32-c40                     1.6e-07   2.6e-06   1.2e-07   1.2e-07  7.3e-05
#   tail-graded-B70of128-fp32-c1e4                    7.8e-08   1.3e-06   9.1e-08   7.8e-08  3.2e-04
#   tail-graded-B70of128-fp32-fmg-c40                 7.0e-08   1.1e-06   9.6e-09   7.0e-08  3.6e-05
#   tail-graded-B70of128-fp32-fmg-c1e4                4.2e-09   6.7e-08   2.8e-09   4.2e-09  2.9e-04
#   tail-graded-B128of128-fp32-fmg-c1e4-decades       1.5e-08   2.4e-07   1.1e-08   1.5e-08  5.3e-05
#   tail-skew-B64of64-fp32-c1e4                       8.4e-08   1.3e-06   8.4e-08   8.3e-08  1.8e-04
#   tail-skew-B64of64-fp64-c40                        5.8e-16   1.4e-14   1.2e-15   4.3e-16  5.3e-05
#   tail-skew-B128of128-fp32-c1e4                     1.1e-07   1.8e-06   1.1e-07   1.1e-07  2.0e-04
#   tail-skew-B128of128-fp64-c40                      5.3e-16   1.4e-14   1.1e-15   3.8e-16  5.3e-05
#   tail-pinned-B128of128-fp32-fmg-c1e4               3.5e-09   5.6e-08   2.7e-09   2.6e-09  3.8e-04
#   tail-pinned-B128of128-fp64-c1e4                   4.5e-16   1.4e-14   5.2e-16   2.4e-16  1.6e-04
#   two-plain-B128of128-fp32-fmg1-split0-c1e4         3.0e-09   4.8e-08   2.6e-09   3.0e-09  1.6e-04
#   two-plain-B128of128-fp32-fmg1-split1-c1e4         4.2e-09   6.7e-08   2.9e-09   4.2e-09  1.6e-04
#   two-plain-B128of128-fp32-fmg2-split0-c1e4         1.3e-09   2.1e-08   2.6e-09   2.2e-09  3.2e-04
#   two-plain-B128of128-fp32-fmg2-split1-c1e4         3.0e-09   4.8e-08   2.8e-09   3.0e-09  1.1e-04
#   unit-plain-B128of128-fp32-c1e4                    7.7e-08   1.2e-06   7.3e-08   7.7e-08  2.9e-04
#   xonly-plain-B128of128-fp64-c40                    1.6e-15   2.5e-14   4.2e-15   1.7e-15  3.2e-05
#   tail-field-B128of128-fp32-h16-c1e4                9.2e-08   1.5e-06   1.6e-07   9.2e-08  2.9e-04
#   tail-neumann-B128of128-fp32-c40                   1.3e-07   2.2e-06   1.4e-07   1.6e-07  1.9e-04
#   tail-plain-B64of64-fp64-warm                      1.4e-15   2.3e-14   1.2e-15   9.5e-16  2.7e-05
#   tail-graded-B64of64-fp64-c1e4-warm                2.5e-16   1.4e-14   4.4e-16   2.1e-16  3.4e-05
#   tail-plain-B64of64-fp64-fmg-warm                  5.0e-16   1.4e-14   1.7e-15   4.9e-16  3.5e-05
#   tail-graded-B64of64-fp64-fmg-c1e4-warm            2.2e-16   1.4e-14   3.8e-16   2.0e-16  4.3e-05
#   tail-plain-B64of64-fp32-warm                      7.7e-09   1.2e-07   1.5e-08   1.1e-08  2.2e-04
#   tail-graded-B64of64-fp32-c1e4-warm                1.2e-08   1.9e-07   7.5e-09   1.2e-08  1.0e-04
#   tail-plain-B64of64-fp32-fmg-warm                  9.7e-10   1.6e-08   4.5e-10   1.1e-09  1.2e-04
#   tail-graded-B64of64-fp32-fmg-c1e4-warm            1.5e-10   2.5e-09   2.4e-10   2.4e-10  4.8e-04
#   tail-plain-B128of128-fp64-warm                    9.1e-16   1.5e-14   1.7e-15   3.4e-16  4.1e-05
#   tail-graded-B128of128-fp64-c1e4-warm              2.9e-16   1.4e-14   4.4e-16   2.4e-16  6.9e-05
#   tail-plain-B128of128-fp64-fmg-warm                7.5e-16   1.4e-14   1.5e-15   4.7e-16  3.0e-05
#   tail-graded-B128of128-fp64-fmg-c1e4-warm          2.5e-16   1.4e-14   3.3e-16   2.5e-16  4.3e-05
#   tail-plain-B128of128-fp32-warm                    9.1e-09   1.4e-07   1.6e-08   7.7e-09  2.2e-04
#   tail-graded-B128of128-fp32-c1e4-warm              4.5e-09   7.1e-08   7.4e-09   4.5e-09  3.6e-04
#   tail-plain-B128of128-fp32-fmg-warm                1.1e-09   1.7e-08   6.9e-10   1.2e-09  1.5e-04
#   tail-graded-B128of128-fp32-fmg-c1e4-warm          1.9e-10   3.1e-09   2.8e-10   1.6e-10  3.0e-04
#   tail-graded-B128of128-fp32-fmg-c40-warm           2.8e-09   4.4e-08   6.5e-10   2.8e-09  5.0e-05
#   two-plain-B128of128-fp32-fmg-c1e4-warm            4.2e-10   6.8e-09   2.1e-10   2.8e-10  1.3e-04
