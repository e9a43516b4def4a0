"""A plain numpy model of the general path's multigrid cycle, Galerkin products and PCG drivers (include/diffhe_hip.h:
diffhe_ell_amg_pcg_solve, diffhe_ell_cg_solve, diffhe_ell_galerkin), written from the mathematics and the header's
comments.  Test infrastructure: no device, no kernels, one (n, B) array per vector and one Python loop over the ELL slots.

A PCG that is cut after k iterations (tol = 1e-300, no floor) is a deterministic function of (A, M, b): its k-th iterate
shows the preconditioner M itself (x_1 = alpha M b), which a converged solve never does -- a converged PCG returns the
right answer for any symmetric positive-definite M.  tests/test_amg_cycle.py holds the kernels to this model.

The hierarchy is what the kernels read, as host arrays: per level a dict with
  cols (W, n) int, vals (W, n) batch-shared or (W, n, B) per sample (slot 0 = diagonal, padding slots point at the row
  itself and hold 0), and optionally
  agg (n) node -> node of the next level (-1: none)             piecewise-constant aggregation, or
  p_cols, p_vals (p_width, n) rows of the prolongation P (-1: no entry)       smoothed aggregation,
  reserved (int, thousandths of a bound of lambda_max(D^-1 A)), dense_inv (n, n) on the last level.
Restriction is the TRANSPOSE OF P built here from p_cols / p_vals (or agg) -- not the CSR tables (agg_ptr, agg_members,
agg_weights) the kernel walks, so a comparison also proves that those tables are that transpose.

dtype: np.float64 or np.longdouble for all arithmetic.  reverse: every ELL row sum and every restriction sum takes its
terms in reverse order (two evaluations of the same mathematics, whose difference measures the rounding spread).
flags & PCG_FP32 restates the fp32-stored cycle: every vector of the cycle is rounded to fp32 when it is stored (arithmetic
stays in `dtype`), the cycle reads float32(rs * r) with rs = 2^-ilogb(|b|), per-sample matrices are read through their fp32
copy, the CG's step length is divided by rs.  r.z is accumulated, as the header's cycle does it, from the last sweep's
result BEFORE that is rounded for storage.
"""
from __future__ import annotations

import numpy as np

PCG_FP32, PCG_NO_FLOOR = 1, 16          # DIFFHE_PCG_FP32, DIFFHE_PCG_NO_FLOOR
OMEGA = (0.56, 1.39)                    # Chebyshev weights for the interval [0.5, 2] of D^-1 A
U = 2.0 ** -53                          # unit roundoff of the attainable-accuracy floor

# single defects a model can be given (tests: each must move a truncated iterate far beyond the comparison's tolerance)
MUTATIONS = ("post_not_reversed", "post_dropped", "gamma_1", "scale_1", "p_last_entry_dropped", "restrict_first_64",
             "reserved_ignored", "dense_as_sweeps", "galerkin_value_1e-6")


def ell_apply(cols, vals, x, reverse=False):
    """A x for ELL values (W, n, 1 or B) against x (n, B)."""
    W = cols.shape[0]
    s = np.zeros_like(x)
    for k in (range(W - 1, -1, -1) if reverse else range(W)):
        s += vals[k] * x[cols[k]]
    return s


def galerkin(vals_fine, ent_ptr, contrib, weights=None):
    """The gather lists of diffhe_ell_galerkin in numpy: coarse entry e = sum_c weights[c] * fine entry contrib[c],
    c in [ent_ptr[e], ent_ptr[e + 1]).  vals_fine (W, n) or (W, n, B) -> flat coarse values (len(ent_ptr) - 1[, B])."""
    flat = vals_fine.reshape(vals_fine.shape[0] * vals_fine.shape[1], -1)
    terms = flat[contrib] if weights is None else flat[contrib] * np.asarray(weights)[:, None]
    out = np.zeros((len(ent_ptr) - 1, flat.shape[1]), dtype=flat.dtype)
    seg = np.repeat(np.arange(len(ent_ptr) - 1), np.diff(ent_ptr))
    np.add.at(out, seg, terms)
    return out if vals_fine.ndim == 3 else out[:, 0]


class Result:
    """x (n, B), iters (B), relres (B) of a truncated or stopped PCG; its: iterations of the loop, not_converged: the
    samples still active at its last poll; ratios: per iteration, r.r / threshold of the samples active in it (nan
    elsewhere); snap[k]: (x, iters, relres) after k iterations for every k asked for."""


class AmgModel:
    def __init__(self, levels, n_coarse, gamma, scale, flags=0, dtype=np.float64, reverse=False, columns=None,
                 mutate=()):
        unknown = set(mutate) - set(MUTATIONS)
        assert not unknown, unknown
        self.dtype, self.reverse, self.mutate = dtype, bool(reverse), frozenset(mutate)
        self.n_coarse, self.flags = int(n_coarse), int(flags)
        self.gamma = 1 if "gamma_1" in self.mutate else int(gamma)
        self.scale = dtype(1.0) if "scale_1" in self.mutate else dtype(scale)
        self.fp32 = bool(flags & PCG_FP32)
        self.columns = None if columns is None else np.asarray(columns, dtype=np.int64)
        self.shared = np.asarray(levels[0]["vals"]).ndim == 2
        self.nl = len(levels)
        self.lv = [self._level(l, lv) for l, lv in enumerate(levels)]
        # the outer CG always applies the fp64 values of the fine level
        self.A0 = self._values(levels[0]["vals"], False)
        self.maxdiag = np.max(self._values(levels[0]["vals"], False)[0], axis=0).astype(np.float64)

    # -- set-up ----------------------------------------------------------------------------------------------------
    def _values(self, vals, cycle):
        v = np.asarray(vals)
        if v.ndim == 2:
            v = v[:, :, None]
        elif self.columns is not None:
            v = v[:, :, self.columns]
        if cycle and self.fp32 and not self.shared:      # per-sample matrices: the cycle reads their fp32 copy
            v = v.astype(np.float32)
        return v.astype(self.dtype)

    def _level(self, l, lv):
        L = dict(n=int(lv["cols"].shape[1]), W=int(lv["cols"].shape[0]), cols=np.asarray(lv["cols"], dtype=np.int64))
        vals = np.asarray(lv["vals"])
        if "galerkin_value_1e-6" in self.mutate and l == 1:
            vals = vals.copy()
            vals[0, L["n"] // 2] *= 1.0 + 1e-6           # one coarse diagonal entry (of every sample)
        L["vals"] = self._values(vals, True)
        res = int(lv.get("reserved") or 0)
        f = 2000.0 / res if (res > 2000 and "reserved_ignored" not in self.mutate) else 1.0
        L["w"] = (self.dtype(OMEGA[0]) * self.dtype(f), self.dtype(OMEGA[1]) * self.dtype(f))
        L["rescaled"] = res > 2000
        dinv = lv.get("dense_inv")
        L["dense"] = None
        if (l == self.nl - 1 and l > 0 and dinv is not None and self.shared and L["n"] <= 128):
            L["dense"] = np.asarray(dinv).astype(self.dtype)
        if l < self.nl - 1:
            if lv.get("p_cols") is not None:
                pc, pv = np.array(lv["p_cols"], dtype=np.int64), np.asarray(lv["p_vals"], dtype=np.float64)
                L["smoothed"] = True
            else:
                agg = np.asarray(lv["agg"], dtype=np.int64)
                pc, pv = agg[None, :].copy(), np.ones((1, len(agg)))
                L["smoothed"] = False
            if "p_last_entry_dropped" in self.mutate and L["smoothed"]:
                pw = pc.shape[0]
                last = (pw - 1) - np.argmax((pc >= 0)[::-1], axis=0)
                has = (pc >= 0).any(axis=0)
                pc[last[has], np.nonzero(has)[0]] = -1
            L["p_cols"], L["p_vals"] = pc, pv.astype(self.dtype)
            # P^T: for every next-level node the fine nodes of its column, in ascending order
            k, i = np.nonzero(pc >= 0)
            I = pc[k, i]
            order = np.lexsort((k, i, I))
            i, I, w = i[order], I[order], pv[k, i][order]
            pos = np.arange(len(I)) - np.searchsorted(I, I)          # rank inside the column
            L["longest_column"] = int(pos.max()) + 1 if len(pos) else 0
            if "restrict_first_64" in self.mutate:
                keep = pos < 64
                i, I, w = i[keep], I[keep], w[keep]
            if self.reverse:
                i, I, w = i[::-1], I[::-1], w[::-1]
            seg = np.nonzero(np.r_[True, I[1:] != I[:-1]])[0] if len(I) else np.zeros(0, dtype=np.int64)
            L["r_fine"], L["r_w"], L["r_seg"], L["r_coarse"] = i, w.astype(self.dtype)[:, None], seg, I[seg]
        return L

    def applies(self, mutation):
        """Whether this hierarchy has what the mutation would break (a W-cycle, a dense level, ...)."""
        lv = self.lv
        return {"post_not_reversed": self.nl > 1, "post_dropped": self.nl > 1,
                "gamma_1": self.gamma > 1 and self.nl > 2, "scale_1": float(self.scale) != 1.0 and self.nl > 1,
                "p_last_entry_dropped": any(L.get("smoothed") for L in lv),
                "restrict_first_64": any(L.get("longest_column", 0) > 64 for L in lv),
                "reserved_ignored": any(L["rescaled"] and L["dense"] is None for L in lv),
                "dense_as_sweeps": lv[-1]["dense"] is not None,
                "galerkin_value_1e-6": self.nl > 1 and lv[1]["dense"] is None}[mutation]

    # -- the cycle -------------------------------------------------------------------------------------------------
    def _st(self, v):
        """A vector of the cycle as it is stored."""
        return v.astype(np.float32).astype(self.dtype) if self.fp32 else v

    def _sweep(self, L, rhs, x, w):
        d = L["vals"][0]
        if x is None:
            return w * rhs / d
        return x + w * (rhs - ell_apply(L["cols"], L["vals"], x, self.reverse)) / d

    def _restrict(self, L, r, nc):
        out = np.zeros((nc, r.shape[1]), dtype=self.dtype)
        if len(L["r_fine"]):
            out[L["r_coarse"]] = np.add.reduceat(L["r_w"] * r[L["r_fine"]], L["r_seg"], axis=0)
        return out

    def _prolong(self, L, e):
        pc, pv = L["p_cols"], L["p_vals"]
        s = np.zeros((pc.shape[1], e.shape[1]), dtype=self.dtype)
        for k in (range(pc.shape[0] - 1, -1, -1) if self.reverse else range(pc.shape[0])):
            ok = pc[k] >= 0
            s[ok] += pv[k][ok, None] * e[pc[k][ok]]
        return s

    def cycle(self, l, rhs):
        """x ~ A_l^-1 rhs from a zero guess: two pre-sweeps of weighted Jacobi, `gamma` coarse corrections (one when the
        next level is the last), x += scale P e, two post-sweeps with the weights reversed; the last level is n_coarse
        sweeps or the dense product."""
        L = self.lv[l]
        rhs = np.asarray(rhs, dtype=self.dtype)
        w0, w1 = L["w"]
        last = l == self.nl - 1
        if last and L["dense"] is not None and "dense_as_sweeps" not in self.mutate:
            return self._st(L["dense"] @ rhs)
        x = None
        for s in range(self.n_coarse if last else 2):
            wide = self._sweep(L, rhs, x, w1 if s & 1 else w0)
            x = self._st(wide)
        if not last:
            visits = 1 if l + 1 == self.nl - 1 else self.gamma
            for _ in range(visits):
                r = self._st(rhs - ell_apply(L["cols"], L["vals"], x, self.reverse))
                rc = self._st(self._restrict(L, r, self.lv[l + 1]["n"]))
                e = self.cycle(l + 1, rc)
                pe = self._prolong(L, e)
                x = self._st(x + self.scale * pe)
            post = [w0, w1] if "post_not_reversed" in self.mutate else [w1, w0]
            if "post_dropped" in self.mutate:
                post = post[:1]
            for w in post:
                wide = self._sweep(L, rhs, x, w)
                x = self._st(wide)
        if l == 0:
            self._wide = wide
        return x

    def cycle_matrix(self, l):
        """The dense matrix of cycle(l, .) of a batch-shared hierarchy: the cycle applied to the identity."""
        assert self.shared
        return self.cycle(l, np.eye(self.lv[l]["n"], dtype=self.dtype))

    # -- the PCG ---------------------------------------------------------------------------------------------------
    def _precondition(self, r, rs):
        rin = (r * rs).astype(np.float32).astype(self.dtype) if self.fp32 else r
        z = self.cycle(0, rin)
        return z, np.sum(rin * self._wide, axis=0)

    def pcg(self, b, k, tol=1e-300, check_every=1, keep=()):
        """k iterations at most of the PCG of diffhe_ell_amg_pcg_solve from x = 0 (b: (n, B), the columns of
        `columns` when given)."""
        b = np.asarray(b)
        if self.columns is not None and b.shape[1] != len(self.columns):
            b = b[:, self.columns]
        b = b.astype(self.dtype)
        A = lambda v: ell_apply(self.lv[0]["cols"], self.A0, v, self.reverse)     # noqa: E731
        bb = np.sum(b * b, axis=0)
        rs = np.ones(b.shape[1], dtype=self.dtype)
        if self.fp32:
            e = np.frexp(np.sqrt(bb.astype(np.float64)))[1] - 1           # ilogb(|b|)
            rs = np.where(bb > 0, np.ldexp(1.0, -e), 1.0).astype(self.dtype)
        floor = None
        if not (self.flags & PCG_NO_FLOOR):
            floor = (0.5 * U * 2.0 * self.maxdiag) ** 2
        return _pcg_loop(A, lambda r: self._precondition(r, rs), b, bb, rs, k, tol, check_every, keep, floor, self.dtype)


def jacobi_pcg(cols, vals, b, k, tol=1e-300, check_every=1, keep=(), dtype=np.float64, reverse=False, columns=None):
    """k iterations at most of diffhe_ell_cg_solve: PCG with z = r / D from x = 0, stopped on `tol` alone."""
    cols = np.asarray(cols, dtype=np.int64)
    v = np.asarray(vals)
    v = v[:, :, None] if v.ndim == 2 else (v if columns is None else v[:, :, columns])
    v = v.astype(dtype)
    b = np.asarray(b)
    if columns is not None:
        b = b[:, columns]
    b = b.astype(dtype)
    bb = np.sum(b * b, axis=0)

    def prec(r):
        z = r / v[0]
        return z, np.sum(r * z, axis=0)
    return _pcg_loop(lambda x: ell_apply(cols, v, x, reverse), prec, b, bb, np.ones(b.shape[1], dtype=dtype), k, tol,
                     check_every, keep, None, dtype)


def _pcg_loop(A, prec, b, bb, rs, k, tol, check_every, keep, floor, dtype):
    """x = 0, r = b, z = M r, p = z; per iteration and sample alpha = r.z / p.Ap (0 once the sample has stopped),
    x += alpha p, r -= alpha A p, z = M r; a sample stops when r.r <= max(tol^2 b.b, floor |x|^2) and counts the
    iterations it was active in; beta = r.z_new / r.z_old.  A sample with b = 0 is never active.  The loop polls the
    number of active samples every check_every iterations and at k, and ends when it is 0."""
    B = b.shape[1]
    x, r = np.zeros_like(b), b.copy()
    z, rz = prec(r)
    tol2 = dtype(tol) * dtype(tol) * bb
    active = bb > 0
    iters = np.zeros(B, dtype=np.int64)
    p = z.copy()
    res = Result()
    res.snap, res.ratios = {}, []
    it, n_active = 0, -1

    def relres(xv):
        t = b - A(xv)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(bb > 0, np.sqrt(np.sum(t * t, axis=0) / np.where(bb > 0, bb, 1)), 0.0)

    while it < k:
        Ap = A(p)
        pAp = np.sum(p * Ap, axis=0)
        go = active & (pAp > 0)
        alpha = np.where(go, (rz / np.where(go, pAp, 1)) / rs, 0).astype(dtype)
        x = x + alpha * p
        r = r - alpha * Ap
        rr = np.sum(r * r, axis=0)
        z, rz_new = prec(r)
        thr = tol2.copy()
        if floor is not None:
            thr = np.maximum(thr, floor.astype(dtype) * np.sum(x * x, axis=0))
        with np.errstate(all="ignore"):
            res.ratios.append(np.where(active, rr / thr, np.nan).astype(np.float64))
        iters = iters + active
        stop = active & (rr <= thr)
        cont = active & ~stop
        beta = np.where(cont, rz_new / np.where(cont, rz, 1), 0).astype(dtype)
        rz = np.where(cont, rz_new, rz)
        active = cont
        p = z + beta * p
        it += 1
        if it in keep:
            res.snap[it] = (x.copy(), iters.copy(), relres(x))
        if it % check_every == 0 or it == k:
            n_active = int(active.sum())
            if n_active == 0:
                break
    res.x, res.iters, res.relres = x, iters, relres(x)
    res.its, res.not_converged = it, max(n_active, 0)
    return res
