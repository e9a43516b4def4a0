"""A plain numpy model of the lattice solve (include/diffhe_hip.h: diffhe_lattice_pcg_solve; csrc/lattice_cycle.hip:
vcycle, coarse_solve, fmg_start; csrc/lattice_pcg.hip: the driver), written from the mathematics and the comments of
those units.  Test infrastructure: no device, no kernels, one (n, B) array per vector.

A PCG that is cut after k iterations (tol = 1e-300, no floor, no energy rule) is a deterministic function of the level
matrices and b, and what the solve returns is x_k + z_k / rs -- so with a zero start and k = 0 it returns M b, the cycle
applied once to the right-hand side.  A converged solve never shows M: it returns the right u for any symmetric
positive-definite preconditioner.  tests/test_lattice_cycle.py holds the kernels to this model.

Levels are host dicts, finest first:
  nx, ny, nd (3 or 4), is_bc (n) and vals (nd, n) batch-shared or (nd, n, B) per sample -- the SYMMETRIC DIAGONALS
  D_k[i] = K[i, i + off_k], off = (0, 1, W, nx), W = nx + 1 (the fourth couples (R, c) with (R + 1, c - 1)); optionally
  shift (n)                             batch-shared diagonal shift, A_b = scale_b K + diag(shift);
  vals32 (nd, n), rd32 (n)              fp32 copies and reciprocal diagonal of a batch-shared matrix;
  vals32 (nd, n, B)                     plain fp32 copies of per-sample matrices;
  d32 (n, B), o16 (nd - 1, n, B), osc (B)   fp32 diagonal (every row sum of the fp64 matrix kept), fp16 couplings times
                                        1 / osc_b;
  dense_inv (n, n)                      on the last level: its solve is (1 / s_b) inv rhs.
`forms` (level_forms below) says per level which kernel family the device takes: only what changes a VALUE is read here
(which coefficient copy a level reads, where the initial-guess form of the cycle runs, whether the search directions are
stored in fp32).

dtype: np.float64 or np.longdouble for all arithmetic; reverse: every stencil, restriction and interpolation sum takes
its terms in reverse order.  fp32: the cycle's vectors, r32 = (float)(rs r), the stored directions and the coefficient
copies are rounded to float32 where the fp32 cycle stores them (arithmetic stays in `dtype`).  arith32: the cycle's
arithmetic is float32 as well (the fused passes and the two-samples-per-lane kernels compute in fp32, not only store in
it).  r.z is accumulated, as the kernels do it, from the last sweep's result BEFORE it is rounded for storage.

Pinned by truncated solves, besides the cold cycle: the diagonal shift of a factored operator (every level's own shift in
the smoother's diagonal, the residuals, the Chebyshev level and the CG's operator; SHIFT_MUTATIONS) and the warm start
(pcg(x_init=...): where rs enters, which residual feeds the start, where the pending correction and the guess are added;
WARM_MUTATIONS).  The coarsest level's spectrum bound ignores the shift, as the device's does (gershgorin_lmax).
Still held by converged solves only: the stopping rules (floor, energy estimate, the low half of the residual pair being
dropped near the stop), the adjoint solve's warm start from the previous lambda, and the direct (single dense level) solve.
"""
from __future__ import annotations

import math
import re

import numpy as np

OMEGAS = (0.56, 1.39)                   # Chebyshev weights for the interval [0.5, 2] of D^-1 A (nu = 2)

# defects of the diagonal shift of a factored operator, A_b = scale_b K_1 + diag(shift), and of the warm start
SHIFT_MUTATIONS = ("shift_dropped_coarse", "shift_not_rediscretised", "shift_scaled", "shift_not_in_diag",
                   "shift_dropped_residual", "shift_dropped_A0", "shift_row_off", "shift_col_off", "shift_tail")
WARM_MUTATIONS = ("warm_guess_dropped", "warm_residual_of_b", "warm_rs_missing", "warm_pending_twice")
# single defects a model can be given (tests: each must move a truncated iterate far beyond the comparison's tolerance)
MUTATIONS = ("pre_weight_slot", "restrict_corner_quarter", "restrict_corners_swapped", "restrict_writes_dirichlet",
             "prolong_corrects_dirichlet", "halo_east_dropped", "halo_east_dropped_tail", "diag4_mirrored",
             "coarse_no_scale", "cheby_degree_off", "final_z_omitted", "rs_not_undone", "h16_no_rowsum",
             "fmg_pending_dropped", "guess_from_zero", "post_order", "pre_order") + SHIFT_MUTATIONS + WARM_MUTATIONS
# not a defect but a measure: the coarsest level's solve returns 0 -- how far the iterates move then bounds what any defect
# of that solve can do to them
PROBES = ("coarse_zero",)
# pairs that are equal in exact arithmetic: two sweeps are polynomials in D^-1 A applied to the same right-hand side,
#   x'' = (I - w_b D^-1 A)(I - w_a D^-1 A) x + (w_a + w_b - w_a w_b D^-1 A) D^-1 rhs,
# symmetric in (w_a, w_b) -- the order of the two post-sweeps, and of the two pre-sweeps, changes roundings only
EQUIVALENT = ("post_order", "pre_order")


# ---------------------------------------------------------------------------------------------------------------------
# which kernel form a level takes: the dispatch of csrc/lattice.h, lattice_cycle.hip and lattice_pcg.hip restated
# ---------------------------------------------------------------------------------------------------------------------
def thresholds(lattice_h: str, layout_h: str, cycle_hip: str) -> dict:
    """The constants of the dispatch, parsed out of the texts of csrc/lattice.h, lattice_layout.h and lattice_cycle.hip."""
    m = re.search(r"if \(Bp < kWave \|\| L\.W < kStripMinW \|\| L\.ny \+ 1 < (\d+)\) return none;", lattice_h)
    return dict(min_w=int(re.search(r"constexpr int kStripMinW = (\d+);", lattice_h).group(1)), min_rows=int(m.group(1)),
                small_w=int(re.search(r"const bool small = L\.W <= (\d+);", cycle_hip).group(1)),
                part_blocks=int(re.search(r"constexpr int kPartBlocks = (\d+);", layout_h).group(1)), wave=64)


def strip_use(lv, Bp, T, spl=1):
    """strip_geom(L, Bp, rw, spl).use"""
    return not (Bp < T["wave"] or lv["nx"] + 1 < T["min_w"] or lv["ny"] + 1 < T["min_rows"]) and Bp // (T["wave"] * spl) >= 1


def level_forms(levels, Bv, Bp, T, fp32, scale=None, fused=1, pre4=1, dense_mfma=1, split_start=0, fp32_step=1,
                resid_pair=1, nu=2, fmg=0, warm=0):
    """Per level dict(pre, post, coarse, guess, coef32, tile); plus, under key None, the driver's forms.
    levels: dicts with nx, ny, nd and the PRESENCE of vals32 / rd32 / o16 / shift / dense_inv (values are not read).

    A level with a shift (Bv == 1 only) has no shared fp32 copy (shared32_ok), hence no two-samples-per-lane kernels, no
    fused passes, no initial-guess cycle and no fp32 step length: its strip levels run dia_strip_shift_kernel ("strip_*"),
    the others the generic kernels with their shift_at terms, and -- there is no dense inverse of a shifted operator -- the
    last level is the Chebyshev semi-iteration.
    The start of a full-multigrid solve is two facts, which differ with a shift: the DRIVER (Solve::fused_start,
    lattice_pcg.hip) converts and restricts b in one pass and hands fmg_start the level-1 right-hand side (`cvt_restrict`,
    = have_b1) without looking at the shift; the CYCLE (prolong_resid_ok, lattice_cycle.hip) takes prolongation and residual
    of the fine level as one strip pass (`prolong_resid`) only without one.  A warm start (`warm`, DIFFHE_PCG_WARM) forces
    the split start on both: the start's right-hand side is then the residual pass's fp32 copy, not b's."""
    nl, wave = len(levels), T["wave"]
    out = {}
    halves = lambda l: l + 1 < nl and levels[l]["nx"] == 2 * levels[l + 1]["nx"] and levels[l]["ny"] == 2 * levels[l + 1]["ny"]  # noqa: E731
    hfuse = 0 if not fused else (2 if Bp % (2 * wave) == 0 else 1)
    for l, lv in enumerate(levels):
        has32 = lv.get("vals32") is not None
        shared32 = Bv == 1 and has32 and lv.get("rd32") is not None and lv.get("shift") is None and Bp % wave == 0
        s2 = shared32 and Bp % (2 * wave) == 0
        if shared32:
            fok = 3
        else:
            fok = 3 if (Bv == Bp and Bv != 1 and Bp % (2 * wave) == 0 and has32 and lv.get("o16") is not None
                        and lv.get("shift") is None and scale is None) else 0
        strip = strip_use(lv, Bp, T)
        f = dict(strip=strip, coef32=bool(fp32 and strip and (shared32 or (Bv != 1 and has32))), guess=False, tile=None)
        if l == nl - 1:
            if lv.get("dense_inv") is not None and Bv == 1 and (lv["nx"] + 1) * (lv["ny"] + 1) <= T["part_blocks"]:
                f["coarse"] = ("dense_mfma" if dense_mfma and fp32 and Bp >= wave else
                               "dense_solve" if Bp >= wave else "dense_small")
            else:
                f["coarse"] = "chebyshev"
            f["pre"] = f["post"] = None
            out[l] = f
            continue
        f["coarse"] = None
        fmask = fok if (fp32 and hfuse and nu == 2 and halves(l) and strip) else 0
        if fmask:
            spl = hfuse if Bv == 1 else 2
            spl_pre = 4 if (pre4 and Bv == 1 and spl == 2 and Bp % (4 * wave) == 0 and lv["nd"] == 3) else spl
            f["pre"], f["post"], f["guess"] = f"fused_pre{spl_pre}", f"fused_post{spl}", l > 0
            f["tile"] = "short" if lv["nx"] + 1 <= T["small_w"] else "four"
        else:
            two = fp32 and s2 and strip_use(lv, Bp, T, 2)
            f["pre"] = ("strip2" if two else "strip") + "_first2" if strip and nu >= 2 else "simple"
            f["pre"] += ("+strip2_resid_restrict" if fp32 and s2 else "+strip_resid_restrict") if strip and halves(l) \
                else "+residual+restrict"
            f["post"] = (("strip2" if two else "strip") + "_prolong_sweep+sweep") if strip and halves(l) \
                else "prolong+" + ("strip_sweeps" if strip else "simple")
        out[l] = f
    L0 = levels[0]
    strip0 = strip_use(L0, Bp, T)
    rupd = bool(strip0 and fp32 and Bv == 1)
    shared32_0 = (Bv == 1 and L0.get("vals32") is not None and L0.get("rd32") is not None and L0.get("shift") is None
                  and Bp % wave == 0)
    cspl = 2 if Bp % (2 * wave) == 0 else 1
    fusable = bool(not split_start and fp32 and Bv == 1 and nl > 1 and strip0 and halves(0))
    out[None] = dict(cg="fused_step" if strip0 else "unfused", rupd=rupd, rpair=bool(rupd and resid_pair),
                     step2=bool(fp32 and rupd and fp32_step and Bp % wave == 0 and strip_use(L0, Bp, T, cspl) and shared32_0),
                     p32=bool(fp32 and strip0), warm=bool(warm),
                     # what the two facts of the start share, before the start itself, a guess or a shift are looked at
                     fused_start=fusable,
                     cvt_restrict=bool(fusable and fmg and not warm and Bp % wave == 0),
                     prolong_resid=bool(fusable and fmg and not warm and L0.get("shift") is None))
    return out


def dense_level(levels, max_nodes=1200):
    """plan.dense_level(): index of the first level with at most max_nodes nodes, or None."""
    return next((i for i, lv in enumerate(levels) if (lv["nx"] + 1) * (lv["ny"] + 1) <= max_nodes), None)


def gershgorin_lmax(level):
    """H.coarse_lmax as cycle_coarse_bound sets it: 2, or on a 4-diagonal coarsest level the Gershgorin bound of
    D^-1 A over all rows and stored samples, times 1 + 1e-9, where that lies in (2, 1e3).
    dia_gershgorin_kernel reads the stored diagonals alone: neither the per-sample scale nor a shift enters.  That is the
    bound of D^-1 K_1; with a shift s >= 0 every row's sum_j |a_ij| / a_ii only shrinks, (d + o) / d >= (s_b d + s + s_b o)
    / (s_b d + s), so it still bounds the shifted operator's spectrum (from further above), and the model takes the same
    number."""
    if level["nd"] != 4:
        return 2.0
    v = np.asarray(level["vals"], dtype=np.float64)
    v = v[:, :, None] if v.ndim == 2 else v
    n, W = v.shape[1], level["nx"] + 1
    s = np.zeros_like(v[0])
    for k, off in ((1, 1), (2, W), (3, level["nx"])):
        s[:n - off] += np.abs(v[k][:n - off])
        s[off:] += np.abs(v[k][:n - off])
    bound = float(np.max(1.0 + s / v[0]))
    return bound * (1.0 + 1e-9) if 2.0 < bound < 1e3 else 2.0


# ---------------------------------------------------------------------------------------------------------------------
class Result:
    """snap[k] = (x (n, B), relres (B)): what the solve returns with max_iter = k; iters (B) for the last k."""


class LatticeModel:
    def __init__(self, levels, forms, scale=None, omegas=OMEGAS, n_coarse=4, coarse_lmax=2.0, fp32=False, arith32=False,
                 dtype=np.float64, reverse=False, columns=None, fmg=False, fmg_cycles=1, warm=False, mutate=()):
        unknown = set(mutate) - set(MUTATIONS) - set(PROBES)
        assert not unknown, unknown
        assert not arith32 or fp32
        self.mutate, self.reverse = frozenset(mutate), bool(reverse)
        self.fp32, self.arith32, self.dtype = bool(fp32), bool(arith32), dtype
        self.ct = np.float32 if arith32 else dtype          # the type the cycle computes in
        self.columns = None if columns is None else np.asarray(columns, dtype=np.int64)
        self.omegas, self.nu, self.n_coarse, self.lmax = tuple(omegas), len(omegas), int(n_coarse), float(coarse_lmax)
        self.fmg, self.fmg_cycles, self.warm = bool(fmg) and len(levels) > 1, int(fmg_cycles), bool(warm)
        self.forms, self.nl = forms, len(levels)
        self.shared = np.asarray(levels[0]["vals"]).ndim == 2
        self.scale = None if scale is None else self._cols(np.asarray(scale, dtype=np.float64)).astype(dtype)
        self._shift0 = None if levels[0].get("shift") is None else np.asarray(levels[0]["shift"], dtype=np.float64).reshape(-1)
        self._nxy0 = (int(levels[0]["nx"]), int(levels[0]["ny"]))
        self.shift_index_delta = {}      # per index defect of the shift: max |shift read - shift| / diagonal, level 0
        self.lv = [self._level(l, lv) for l, lv in enumerate(levels)]

    # -- set-up ----------------------------------------------------------------------------------------------------
    def _cols(self, a):
        """The columns asked for of an array whose LAST axis is the sample axis."""
        return a if self.columns is None else a[..., self.columns]

    def _level(self, l, lv):
        dt, ct = self.dtype, self.ct
        nx, ny, nd = int(lv["nx"]), int(lv["ny"]), int(lv["nd"])
        W, n = nx + 1, (nx + 1) * (ny + 1)
        bc = np.asarray(lv["is_bc"]).astype(bool).reshape(n)
        v = np.asarray(lv["vals"], dtype=np.float64)
        v = v[:, :, None] if v.ndim == 2 else self._cols(v)
        L = dict(nx=nx, ny=ny, nd=nd, W=W, n=n, bc=bc, free=(~bc)[:, None], unit=False)
        L["A64"] = v.astype(dt)                                   # the outer CG's operator (level 0) in fp64
        L["shift"] = self._shift(l, lv, L)
        rsn = None if self.scale is None else np.where(L["free"], self.scale[None, :], dt(1.0))   # row_scale
        L["rsn"] = rsn
        c = v
        if self.fp32 and self.forms[l]["coef32"]:
            if lv.get("o16") is not None:                         # fp32 diagonal + osc * fp16 couplings
                osc = self._cols(np.asarray(lv["osc"], dtype=np.float64))
                o = self._cols(np.asarray(lv["o16"]).astype(np.float64)) * osc
                d = self._cols(np.asarray(lv["d32"]).astype(np.float64))
                if "h16_no_rowsum" in self.mutate:
                    d = v[0].astype(np.float32).astype(np.float64)
                c = np.concatenate([d[None], o], axis=0)
                L["rcp32"] = L["h16"] = True                      # the reciprocal diagonal is taken in fp32
            else:
                c32 = np.asarray(lv["vals32"]).astype(np.float64)
                c = c32[:, :, None] if c32.ndim == 2 else self._cols(c32)
                if lv.get("rd32") is not None:                    # batch-shared: unit form with the stored reciprocal
                    L["unit"] = True
                    L["rd"] = np.asarray(lv["rd32"]).astype(np.float64).reshape(n, 1).astype(ct)
                    L["ib"] = None if self.scale is None else (
                        (ct(1.0) / self.scale.astype(np.float32)).astype(ct) if self.arith32 else dt(1.0) / self.scale)
                else:
                    L["rcp32"] = True
        elif self.arith32:
            c = c.astype(np.float32)
        L["c"] = c.astype(ct)
        # the terms of a stencil row in the order dia_row adds them: diagonal, then per diagonal +off, -off
        offs = [1, W, nx][:nd - 1]
        col = np.arange(n) % W
        plus = {k + 1: L["c"][k + 1] for k in range(nd - 1)}
        minus = {k + 1: L["c"][k + 1] for k in range(nd - 1)}
        L["halo_tail_live"] = False
        if l == 0:
            c0 = 4 * ((W - 1) // 4)                               # first column of the last strip of four
            if "halo_east_dropped" in self.mutate:
                plus[1] = np.where((col % 4 == 3)[:, None], 0, plus[1]).astype(ct)
            if c0 >= 1:
                hit = (col == c0 - 1)                              # the east coupling of column c0 - 1, seen from c0
                L["halo_tail_live"] = bool(np.any(minus[1][hit] != 0))
                if "halo_east_dropped_tail" in self.mutate:
                    minus[1] = np.where(hit[:, None], 0, minus[1]).astype(ct)
        if nd == 4 and "diag4_mirrored" in self.mutate:
            offs[2] = W + 1                                       # (R + 1, c + 1); nothing past the right edge
            keep = (col < nx)[:, None]
            plus[3], minus[3] = np.where(keep, plus[3], 0).astype(ct), np.where(keep, minus[3], 0).astype(ct)
        mk = lambda o: [("d", 0, 0)] + [t for k, off in enumerate(o, 1) for t in (("+", k, off), ("-", k, off))]  # noqa: E731
        L["terms"], L["terms0"] = mk(offs), mk([1, W, nx][:nd - 1])
        L["plus"], L["minus"] = plus, minus
        if l == self.nl - 1 and lv.get("dense_inv") is not None and self.shared:
            L["dense"] = np.asarray(lv["dense_inv"]).astype(np.float64).astype(ct)
        return L

    def _shift(self, l, lv, L):
        """The level's diagonal shift (n, 1) or None, with whatever defect it was given."""
        sh = lv.get("shift")
        if sh is None:
            return None
        n, W, mut = L["n"], L["W"], self.mutate
        sh = np.asarray(sh, dtype=np.float64).reshape(n).copy()
        free, col = ~L["bc"], np.arange(n) % W
        if l >= 1 and "shift_dropped_coarse" in mut:
            sh[:] = 0.0
        if l >= 1 and "shift_not_rediscretised" in mut:      # the fine level's nodal values at the coarse nodes
            nx0, ny0 = self._nxy0
            ry, rx = ny0 // L["ny"], nx0 // L["nx"]
            rows, cols = np.divmod(np.arange(n), W)
            sh = np.where(free, self._shift0[rows * ry * (nx0 + 1) + cols * rx], 0.0)
        for name, off in (("shift_row_off", W), ("shift_col_off", 1)):
            moved = np.zeros(n)
            moved[off:] = sh[:n - off]                       # row R + 1 (column c + 1) reads the shift of row R (column c)
            if off == 1:
                moved[col == 0] = 0.0
            moved = np.where(free, moved, 0.0)
            # live: some free node reads another FREE node's different shift (not only the boundary's 0)
            src_free = np.zeros(n, dtype=bool)
            src_free[off:] = free[:n - off]
            if off == 1:
                src_free[col == 0] = False
            if l == 0:       # what the defect does to the fine level's diagonal, relative: the size of its effect on x
                d0 = np.asarray(lv["vals"], dtype=np.float64)[0].reshape(n, -1).min(axis=1)
                smin = 1.0 if self.scale is None else float(np.min(self.scale))
                live = free & src_free
                self.shift_index_delta[name] = float(np.max(np.abs(moved - sh)[live] / (smin * d0 + sh)[live])) if live.any() else 0.0
            if name in mut:
                sh = moved
        if "shift_tail" in mut and self.forms[l]["strip"]:   # the strips that take the clamped (TAIL) body: both edges
            rw = 4 if self.fp32 else 8
            sh = np.where((col < rw) | (col >= rw * -(-(W - rw) // rw)), 0.0, sh)
        return sh.reshape(n, 1)

    def _sh(self, L):
        """diag(shift) as the operators add it: (n, 1), or (n, B) where a defect scales it per sample; None: no shift."""
        if L["shift"] is None or "shift_scaled" not in self.mutate or L["rsn"] is None:
            return L["shift"]
        return L["rsn"].astype(np.float64) * L["shift"]

    def shift_share(self):
        """The largest part the shift has of a free row's diagonal on level 0 (0 without one)."""
        L = self.lv[0]
        if L["shift"] is None:
            return 0.0
        d = np.asarray(L["A64"][0], dtype=np.float64) * (1.0 if L["rsn"] is None else np.asarray(L["rsn"], dtype=np.float64))
        return float(np.max(np.where(L["free"], L["shift"] / (d + L["shift"]), 0.0)))

    def applies(self, mutation):
        """Whether this model has what the mutation would break."""
        lv, nl = self.lv, self.nl
        dense = lv[-1].get("dense") is not None
        shifted = self._shift0 is not None and bool(np.any(self._shift0))
        return {"pre_weight_slot": nl > 1, "restrict_corner_quarter": self._full(), "restrict_corners_swapped": self._full(),
                "restrict_writes_dirichlet": nl > 1, "prolong_corrects_dirichlet": self._dirichlet_interpolates(),
                "halo_east_dropped": True,
                "halo_east_dropped_tail": lv[0]["halo_tail_live"], "diag4_mirrored": any(L["nd"] == 4 for L in lv),
                "coarse_no_scale": dense and self.scale is not None, "cheby_degree_off": not dense,
                "final_z_omitted": True, "rs_not_undone": self.fp32,
                "h16_no_rowsum": any(L.get("h16") for L in lv),
                "fmg_pending_dropped": self.fmg, "guess_from_zero": self.fmg and any(self.forms[l]["guess"] for l in range(nl)),
                "post_order": nl > 1, "pre_order": nl > 1,
                "shift_dropped_coarse": shifted and nl > 1, "shift_not_rediscretised": shifted and nl > 1,
                "shift_scaled": shifted and self.scale is not None and bool(np.any(self.scale != 1)),
                "shift_not_in_diag": shifted, "shift_dropped_residual": shifted and nl > 1, "shift_dropped_A0": shifted,
                "shift_row_off": shifted and self.shift_index_delta.get("shift_row_off", 0.0) > 0.0,
                "shift_col_off": shifted and self.shift_index_delta.get("shift_col_off", 0.0) > 0.0,
                "shift_tail": shifted and bool(self.forms[0]["strip"]),
                "warm_guess_dropped": self.warm, "warm_residual_of_b": self.warm,
                "warm_rs_missing": self.warm and self.fmg and self.fp32,
                "warm_pending_twice": self.warm and self.fmg}[mutation]

    def _dirichlet_interpolates(self):
        """Some fine Dirichlet node interpolates from a free coarse node (never on a boundary that is Dirichlet as a
        whole: its nodes interpolate from coarse boundary nodes, where every correction is 0)."""
        keep, self.mutate = self.mutate, frozenset({"prolong_corrects_dirichlet"})
        try:
            return any(np.any(self._prolong(l, self.lv[l + 1]["free"].astype(np.float64))[self.lv[l]["bc"]])
                       for l in range(self.nl - 1))
        finally:
            self.mutate = keep

    def _full(self):
        return any(self._steps(l) == (2, 2) for l in range(self.nl - 1))

    def _steps(self, l):
        F, C = self.lv[l], self.lv[l + 1]
        return (2 if F["ny"] == 2 * C["ny"] else 1, 2 if F["nx"] == 2 * C["nx"] else 1)      # (rows, columns)

    # -- storage and operators -------------------------------------------------------------------------------------
    def _st(self, v):
        """A vector of the cycle as it is stored."""
        return v.astype(np.float32).astype(self.ct) if self.fp32 else v

    def _sum(self, terms):
        acc = None
        for t in (reversed(terms) if self.reverse else terms):
            acc = t if acc is None else acc + t
        return acc

    def _K(self, L, x, c=None):
        """K x, unscaled, of the level's cycle coefficients with whatever defect they were given -- or, c given, of those
        (nd, n, 1 or B) values as they are."""
        n = L["n"]
        c0, plus, minus, terms = (L["c"][0], L["plus"], L["minus"], L["terms"]) if c is None else (c[0], c, c, L["terms0"])
        acc = np.zeros((n, x.shape[1]), dtype=np.result_type(x.dtype, c0.dtype))
        for kind, k, off in (reversed(terms) if self.reverse else terms):
            if kind == "d":
                acc += c0 * x
            elif kind == "+":
                acc[:n - off] += plus[k][:n - off] * x[off:]
            else:
                acc[off:] += minus[k][:n - off] * x[:n - off]
        return acc

    def _A(self, L, x, drop_shift=False):
        """The cycle's operator of the level: row_scale K x + shift x."""
        y = self._K(L, x)
        if L["rsn"] is not None:
            y = L["rsn"].astype(y.dtype) * y
        if L["shift"] is not None and not drop_shift:
            y = y + self._sh(L).astype(y.dtype) * x
        return y

    def _dinv(self, L):
        d = L["c"][0]
        if L["rsn"] is not None:
            d = L["rsn"].astype(d.dtype) * d
        if L["shift"] is not None and "shift_not_in_diag" not in self.mutate:
            d = d + self._sh(L).astype(d.dtype)
        if L.get("rcp32"):
            return (np.float32(1.0) / d.astype(np.float32)).astype(self.ct)
        return self.ct(1.0) / d

    def _sweep(self, L, rhs, x, w):
        w = self.ct(w)
        if L["unit"]:                 # b / s_b - K_1 x, times the stored reciprocal diagonal of K_1
            res = rhs if L["ib"] is None else rhs * L["ib"]
            if x is None:
                return (w * L["rd"]) * res
            return x + (w * L["rd"]) * (res - self._K(L, x))
        dinv = self._dinv(L)
        if x is None:
            return w * rhs * dinv
        return x + w * (rhs - self._A(L, x)) * dinv

    # -- transfers -------------------------------------------------------------------------------------------------
    def _restrict(self, l, r):
        """P^T r: centre 1; W, E, S, N and the quad-diagonal neighbours (R - 1, c + 1), (R + 1, c - 1) one half each
        (one direction only on a semi-coarsened pair); coarse Dirichlet rows get 0."""
        F, C = self.lv[l], self.lv[l + 1]
        sy, sx = self._steps(l)
        B = r.shape[1]
        p = np.zeros((F["ny"] + 3, F["nx"] + 3, B), dtype=r.dtype)
        p[1:-1, 1:-1] = r.reshape(F["ny"] + 1, F["nx"] + 1, B)
        ri, ci = 1 + sy * np.arange(C["ny"] + 1)[:, None], 1 + sx * np.arange(C["nx"] + 1)[None, :]
        at = lambda dr, dc: p[ri + dr, ci + dc]   # noqa: E731
        half, terms = r.dtype.type(0.5), []
        if sx == 2:
            terms += [at(0, -1), at(0, 1)]
        if sy == 2:
            terms += [at(-1, 0), at(1, 0)]
        out = at(0, 0)
        if sx == 2 and sy == 2:
            swap = "restrict_corners_swapped" in self.mutate
            corners = [at(-1, -1), at(1, 1)] if swap else [at(-1, 1), at(1, -1)]
            if "restrict_corner_quarter" in self.mutate:
                out = out + r.dtype.type(0.25) * self._sum(corners)
            else:
                terms += corners
        out = (out + half * self._sum(terms)).reshape(C["n"], B)
        if "restrict_writes_dirichlet" not in self.mutate:
            out = np.where(C["free"], out, 0)
        return out.astype(r.dtype)

    def _prolong(self, l, e):
        """P e by P1 interpolation on the nested triangulations; 0 on fine Dirichlet nodes."""
        F, C = self.lv[l], self.lv[l + 1]
        sy, sx = self._steps(l)
        B = e.shape[1]
        e2 = e.reshape(C["ny"] + 1, C["nx"] + 1, B)
        v = np.zeros((F["ny"] + 1, F["nx"] + 1, B), dtype=e.dtype)
        half = e.dtype.type(0.5)
        two = (lambda a, b: half * (b + a)) if self.reverse else (lambda a, b: half * (a + b))
        if sx == 2 and sy == 2:
            v[0::2, 0::2] = e2
            v[0::2, 1::2] = two(e2[:, :-1], e2[:, 1:])
            v[1::2, 0::2] = two(e2[:-1, :], e2[1:, :])
            v[1::2, 1::2] = two(e2[:-1, 1:], e2[1:, :-1])        # midpoint of the quad diagonal b-d
        elif sx == 2:
            v[:, 0::2] = e2
            v[:, 1::2] = two(e2[:, :-1], e2[:, 1:])
        else:
            v[0::2, :] = e2
            v[1::2, :] = two(e2[:-1, :], e2[1:, :])
        v = v.reshape(F["n"], B)
        if "prolong_corrects_dirichlet" not in self.mutate:
            v = np.where(F["free"], v, 0)
        return v.astype(e.dtype)

    # -- the cycle -------------------------------------------------------------------------------------------------
    def coarse_solve(self, l, rhs):
        """The dense inverse times 1 / s_b, or the Chebyshev semi-iteration of coarse_solve (lattice_cycle.hip)."""
        L = self.lv[l]
        if "coarse_zero" in self.mutate:
            self._wide = np.zeros_like(rhs)
            return self._wide
        if L.get("dense") is not None:
            x = L["dense"] @ rhs
            if self.scale is not None and "coarse_no_scale" not in self.mutate:
                si = (np.float32(1.0) / self.scale.astype(np.float32)) if self.arith32 else self.dtype(1.0) / self.scale
                x = si.astype(x.dtype) * x
            self._wide = x
            return self._st(x)
        deg, theta, delta, sigma = self._cheby(L)
        if "cheby_degree_off" in self.mutate:
            deg -= 1
        rho = 1.0 / sigma
        dinv, ct = self._dinv(L), self.ct
        dn = ct(1.0 / theta) * rhs * dinv
        d = self._st(dn)
        self._wide = dn
        x = self._st(dn)
        for _ in range(1, deg):
            rho_new = 1.0 / (2.0 * sigma - rho)
            dn = ct(rho_new * rho) * d + ct(2.0 * rho_new / delta) * (rhs - self._A(L, x)) * dinv
            d = self._st(dn)
            self._wide = x + dn
            x = self._st(self._wide)
            rho = rho_new
        return x

    def _cheby(self, L):
        """(degree, theta, delta, sigma) of the semi-iteration on level L, as coarse_solve chooses them."""
        lmin = 0.5 * (0.5 * (1.0 - math.cos(math.pi / L["nx"])) + 0.5 * (1.0 - math.cos(math.pi / L["ny"])))
        lmax = self.lmax
        deg = min(max(int(math.ceil(1.5 * math.sqrt(lmax / lmin))), self.n_coarse), 400)
        theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
        return deg, theta, delta, theta / delta

    def cheby_last_step_share(self):
        """A bound of what the last step of the coarsest level's semi-iteration changes, as a part of that level's
        solution: the error polynomials of degree k - 1 and k are at most 1 / T_(k-1)(sigma) and 1 / T_k(sigma) on the
        interval the iteration is built for, so the two results differ by at most their sum."""
        deg, _, _, sigma = self._cheby(self.lv[-1])
        t = lambda k: math.cosh(k * math.acosh(sigma))   # noqa: E731
        return 1.0 / t(deg - 1) + 1.0 / t(deg)

    def cycle(self, rhs, l0=0, guess=None):
        """z = V(rhs) on levels l0 .. last from a zero guess; guess given: the new ITERATE from the initial guess
        P guess (two sweeps from it, then the correction of the coarser levels and the post-sweeps)."""
        last, w, nu = self.nl - 1, self.omegas, self.nu
        rhs_l, cur = {l0: rhs.astype(self.ct)}, {}
        for l in range(l0, last + 1):
            L = self.lv[l]
            if l == last:
                cur[l] = self.coarse_solve(l, rhs_l[l])
                break
            if l == l0 and guess is not None:
                x = None if "guess_from_zero" in self.mutate else self._prolong(l, guess)
                for s in range(nu):
                    x = self._st(self._sweep(L, rhs_l[l], x, w[s]))
            else:
                pre = [w[s % nu] for s in range(nu)]
                if "pre_weight_slot" in self.mutate:
                    pre = [w[0]] * nu
                if "pre_order" in self.mutate:
                    pre = pre[::-1]
                x = None
                for ws in pre:
                    x = self._st(self._sweep(L, rhs_l[l], x, ws))
            cur[l] = x
            r = self._st(rhs_l[l] - self._A(L, x, drop_shift="shift_dropped_residual" in self.mutate))
            rhs_l[l + 1] = self._st(self._restrict(l, r))
        for l in range(last - 1, l0 - 1, -1):
            L = self.lv[l]
            x = self._st(cur[l] + self._prolong(l, cur[l + 1]))
            post = [w[nu - 1 - s] for s in range(nu)]
            if "post_order" in self.mutate:
                post = post[::-1]
            for ws in post:
                self._wide = self._sweep(L, rhs_l[l], x, ws)
                x = self._st(self._wide)
            cur[l] = x
        return cur[l0]

    def cycle_matrix(self, l0=0):
        """The dense matrix of cycle(., l0) of a batch-shared hierarchy: the cycle applied to the identity."""
        assert self.shared and self.scale is None
        return self.cycle(np.eye(self.lv[l0]["n"], dtype=self.ct), l0)

    def fmg_start(self, b0):
        """fmg_start (lattice_cycle.hip): -> (iterate, the fine level's last correction, not yet added)."""
        last = self.nl - 1
        bl = {0: b0.astype(self.ct)}
        for l in range(last):
            bl[l + 1] = self._st(self._restrict(l, bl[l]))
        coarse = self.cycle(bl[last], last)
        for l in range(last - 1, -1, -1):
            L = self.lv[l]
            cycles = 1 if l == 0 else self.fmg_cycles
            c0 = 0
            if l > 0 and self.forms[l]["guess"]:
                it = self.cycle(bl[l], l, guess=coarse)
                if cycles == 1:
                    coarse = it
                    continue
                x, c0 = it, 1
            else:
                x = self._st(self._prolong(l, coarse))
            for c in range(c0, cycles):
                r = self._st(bl[l] - self._A(L, x))
                e = self.cycle(r, l)
                if l == 0 and c == cycles - 1:
                    return x, e
                x = self._st(x + e)
            coarse = x
        raise AssertionError("unreachable: level 0 returns")

    # -- the PCG ---------------------------------------------------------------------------------------------------
    def _A0(self, x):
        """The fp64 operator of level 0: what the CG and the true residual apply."""
        L = self.lv[0]
        y = self._K(L, x, L["A64"])
        if L["rsn"] is not None:
            y = L["rsn"] * y
        if L["shift"] is not None and "shift_dropped_A0" not in self.mutate:
            y = y + self._sh(L).astype(self.dtype) * x
        return y

    def _pAp32(self, p):
        """cgstep2_kernel: p . (K_1 p) with the stencil and the products in float32 on the fp32 copies, accumulated per
        sample in fp64, times s_b."""
        L = self.lv[0]
        p32 = p.astype(np.float32)
        kp = self._K(L, p32, L["c"].astype(np.float32))
        s = np.sum((p32 * kp).astype(np.float64), axis=0).astype(self.dtype)
        return s if self.scale is None else s * self.scale

    def pcg(self, b, ks=(0, 1, 3), x_init=None):
        """The solve from a cold (zero or full-multigrid) start, or (x_init (n, B), a model built with warm=True) from the
        caller's guess; -> Result with snap[k] for every k of ks."""
        dt = self.dtype
        b = np.asarray(b, dtype=np.float64)
        if self.columns is not None and b.shape[1] != len(self.columns):
            b = b[:, self.columns]
        b = b.astype(dt)
        D = self.forms[None]
        bb = np.sum(b * b, axis=0)
        rs = np.ones(b.shape[1], dtype=dt)
        if self.fp32:                                            # S_INIT: rs |b| in [1, 2)
            e = np.frexp(np.sqrt(bb.astype(np.float64)))[1] - 1
            rs = np.where(bb > 0, np.ldexp(1.0, -e), 1.0).astype(dt)
        active = bb > 0
        rin_of = lambda r: self._st((r * rs).astype(self.ct)) if self.fp32 else r   # noqa: E731

        def precondition(r):
            rin = rin_of(r)
            z = self.cycle(rin)
            return z.astype(dt), np.sum(rin.astype(dt) * self._wide.astype(dt), axis=0)

        assert (x_init is not None) == self.warm
        mut = self.mutate
        if self.warm:
            # PCGRun::start() with DIFFHE_PCG_WARM: x holds the caller's guess g.  rs comes from b.b as in a cold solve; b
            # itself is never converted (no pcg_cvt_kernel).  The residual pass leaves r = b - A g in fp64 and its copy
            # (float)(rs r); with the full-multigrid start that copy (fp64 cycle: r itself) is the start's right-hand
            # side, and pcg_setx_kernel (add = 1) writes x = (x0 + e0) / rs + g in fp64 -- the start's iterate, its pending
            # correction e0 once, the scale undone on both, the guess added unscaled.  Then the residual of that x.
            # Without the start the guess is the iterate and r its residual.
            g = np.asarray(x_init, dtype=np.float64)
            if self.columns is not None and g.shape[1] != len(self.columns):
                g = g[:, self.columns]
            g = g.astype(dt)
            r = b.copy() if "warm_residual_of_b" in mut else b - self._A0(g)
            if self.fmg:
                x0, e0 = self.fmg_start(rin_of(r))
                pend = 0 if "fmg_pending_dropped" in mut else 2 if "warm_pending_twice" in mut else 1
                x = x0.astype(dt) + dt(pend) * e0.astype(dt)
                x = x if "warm_rs_missing" in mut else x / rs
                if "warm_guess_dropped" not in mut:
                    x = x + g
                r = b - self._A0(x)
            else:
                x = np.zeros_like(b) if "warm_guess_dropped" in mut else g
        elif self.fmg:
            x0, e0 = self.fmg_start(rin_of(b))
            x = x0.astype(dt) if "fmg_pending_dropped" in self.mutate else x0.astype(dt) + e0.astype(dt)
            x = x / rs                                           # pcg_setx_kernel, in fp64
            r = b - self._A0(x)
        else:
            x, r = np.zeros_like(b), b.copy()
        z, rz = precondition(r)
        res = Result()
        res.snap = {}
        iters = np.zeros(b.shape[1], dtype=np.int64)

        def snap(k):
            xr = x.copy()
            if "final_z_omitted" not in self.mutate:
                xr = xr + (z if "rs_not_undone" in self.mutate else z / rs)
            t = b - self._A0(xr)
            with np.errstate(divide="ignore", invalid="ignore"):
                rr = np.where(bb > 0, np.sqrt(np.sum(t * t, axis=0) / np.where(bb > 0, bb, 1)), 0.0)
            res.snap[k] = (xr, rr)

        p = None
        for it in range(max(ks) + 1):
            if it in ks:
                snap(it)
            if it == max(ks):
                break
            pn = z if p is None else z + beta * p
            p = pn.astype(np.float32).astype(dt) if D["p32"] else pn      # the direction as it is stored
            Ap = self._A0(p)
            pAp = self._pAp32(p) if D["step2"] else np.sum(p * Ap, axis=0)
            go = active & (pAp > 0)
            alpha = np.where(go, (rz / np.where(go, pAp, 1)) / rs, 0).astype(dt)
            x = x + alpha * p
            r = r - alpha * Ap
            iters = iters + active
            z, rz_new = precondition(r)
            beta = np.where(active, rz_new / np.where(active, rz, 1), 0).astype(dt)
            rz = np.where(active, rz_new, rz)
        res.iters = iters
        return res
