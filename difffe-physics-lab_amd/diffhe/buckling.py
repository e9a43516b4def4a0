"""Linear buckling of elastic bodies per sample: critical load factors and modes, with d lambda / dE and
d lambda / d sigma0 (ours: the reference has neither elasticity nor an eigensolver).

`LinearBucklingSolver(mesh, E, k)` finds, for every sample b, the k smallest POSITIVE lambda and the modes of

    (K(E_b) + lambda K_G(sigma0_b)) phi = 0        on the free dofs,

the multiples of the applied load at which the body loses stability, on P1 triangles (d = 2, both `plane=` settings) and P1
tetrahedra (d = 3).  K is the operator of `ElasticFESolver` -- same `nu`, `plane` and `fixed` -- and sigma0 the element
stress of the linear prestress solve K(E) u0 = M f + load, as `ElasticFESolver.stress` returns it: Voigt order (xx, yy, xy |
xx, yy, zz, yz, xz, xy), shear components are tensor components.  For P1 elements the geometric stiffness is
K_G = G(sigma0) (x) I_d with the scalar operator G[a, b] = sum_e vol_e grad N_a . sigma0_e grad N_b on the NODE pattern: the
stiffness of `AnisotropicFESolver` with the stress in the conductivity's place, symmetric and in general indefinite.  In 2D
only the in-plane components enter, for both `plane=` settings (a sigma_zz of plane strain does no work on in-plane modes).

`forward(f, load)` runs the prestress solve and `stress()` of an `ElasticFESolver` of its own (`solver.inner`), both
differentiable torch ops; `forward(prestress=sigma0)` takes the stress as given -- (m, nc) shared by the batch or (B, m, nc)
-- and makes no solve: a thermal or residual prestress from `stress(..., eigenstrain=)`.

Method ("Linear buckling").  With N = -K_G and mu = 1 / lambda the problem is N phi = mu K phi with K
symmetric positive definite: A = K^-1 N is self-adjoint in the K-inner product and the k LARGEST POSITIVE mu are wanted.
The iteration is `diffhe.eigen._BlockRun` on p = k + guard <= 16 dof vectors with the right-hand matrix carried as a block:
per outer iteration and column, d_i = K^-1 r_i to `inner_tol` with the cached multigrid PCG of the elastic solves
(r_i = N x_i - mu_i K x_i), y_i = (mu_i + s_b) x_i + d_i = (A + s_b) x_i, then K y_i and N y_i explicitly, then the passes
of csrc/buckling.hip and the dense Ritz step of csrc/eigen.hip: Gram matrices Y^T K Y and Y^T N Y, Ritz on (-GN, GK) -- so
that the Cholesky factor is the SPD matrix's and nu = -mu comes back ascending, the wanted pairs first -- and the rotation
X = Y C with R = N X - mu K X.  The per-sample shift s_b >= 0 is half the magnitude of the most negative Ritz value seen so
far in the run (it never decreases): a load that puts part of the body in tension gives negative mu as large as the
positive ones, and plain subspace iteration would converge to the wrong end of the spectrum; with the shift the spectrum
of A + s_b lies in [-|mu_min| / 2, mu_max + |mu_min| / 2] and the positive end dominates.  The operator, G and the
hierarchy are built once per call.

Stopping measure.  rho_i = sqrt(max(d_i^T r_i, 0)) / mu_i for the K-normalised x_i: with d_i = K^-1 r_i this is
|A x_i - mu_i x_i|_K / mu_i, the K-norm of the eigen-residual relative to mu.  It is exactly as accurate as the inner
solve: d_i comes from a PCG run to `inner_tol`, whose iterate is K-orthogonal to its error, so the measure is
|d_i|_K <= |K^-1 r_i|_K, short by the K-norm of the inner error.  It costs no pass of its own (the pass that forms y_i leaves
the dot product), but it is known one outer iteration late: rho of the block X_t comes out of the inner solves of
iteration t + 1, the iteration stops when rho <= tol for the k columns of every sample, and the block returned is X_{t+1},
which has had one more iteration than the one the measure certifies.  The error of mu_i is bounded by rho_i^2 mu_i / gap_i.

Returns `lam` (B, k) ascending and positive -- (k,) when nothing carries a batch -- and `phi` (B, k, n, d), or with
layout="node" (k, n, d, B), the block itself.  phi is K-orthonormal per sample, so phi^T K_G phi = -1 / lambda; zero on
fixed dofs; signed like `ElasticEigenSolver`'s modes with a unit mass (sum of the entries > 0, else the entry of largest
magnitude positive); NON-differentiable.  Where a sample has fewer than k positive Ritz values -- pure tension has none --
the missing lambda are +inf and their phi are 0; `last_info.missing` counts them and ONE RuntimeWarning reports them.  A
column without a positive Ritz value counts as done, but while any is missing at least `MIN_OUTER_MISSING` outer iterations
run, so that a positive mu the start block hardly contains can still grow into it.

Gradients.  From (K + lambda K_G) phi = 0 and phi^T K phi = 1:  d lambda_i = lambda_i phi_i^T (dK + lambda_i dK_G) phi_i.  One
custom-op pair, diffhe::buckling_solve / diffhe::buckling_solve_backward, over (E, sigma0); backward makes NO solve:

    dL/dE       `diffhe_elast_grad` with u = phi_i and the adjoint vector -lambda_bar_i lambda_i phi_i, summed over i
    dL/dsigma0  `diffhe_buckling_grad_sigma` with the weights lambda_bar_i lambda_i^2

in the shapes of E and sigma0 (a field the batch shares gets its gradient summed over the batch inside the kernel).  The
dependence of sigma0 on E and on the loads flows through the stress and solve ops of `solver.inner`: ONE adjoint solve per
call whatever k is.  Entries that are +inf get zero gradient.  For a cluster of equal eigenvalues the gradient is that of
the Rayleigh quotients of the returned basis: right for symmetric functions of the cluster, not for one member of a
degenerate pair (as in `diffhe.eigen`).

`aggregate(lam, p)` is the smooth lower bound of min lambda used in design.

Not implemented (NotImplementedError): 1D meshes, P2 meshes, a stiffness tensor (`AnisotropicElasticFESolver`), node
gradients, backward with create_graph=True, the `diffhe.distributed` helpers.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _hip
from .eigen import JACOBI_SWEEPS, MAX_BLOCK, EigenInfo, _BlockRun, _check_iteration
from .elastic import ElasticFESolver, _check_mesh, _select_hierarchy, _setup_of
from .modal import _field_layout
from .plan import padded_batch, _stream
from .solver import (K_ELEM, K_SAMPLE_ELEM, SolveInfo, _Engine, _SOLVERS, _fake_grads, _kappa_grad, _like_grads,
                     _register_state, _state_of, _tie_state)

__all__ = ("LinearBucklingSolver", "BucklingInfo", "aggregate")

MIN_OUTER_MISSING = 3       # outer iterations that run at least while a wanted column has no positive Ritz value


@dataclass
class BucklingInfo(EigenInfo):
    """`EigenInfo` of the last buckling call (`residual` is the measure rho of the module docstring) plus:"""
    shifts: Optional[torch.Tensor] = None       # (B,) the final s_b, on the CPU
    negative_ritz: int = 0      # negative Ritz values seen: per sample the most in any block of the run, summed over samples
    missing: int = 0            # (sample, mode) pairs returned as +inf
    prestress: Optional[SolveInfo] = None       # the prestress solve's record; None with prestress=


def aggregate(lam: torch.Tensor, p: float = 8.0, dim: int = -1) -> torch.Tensor:
    """A smooth lower bound of min lambda over `dim`: 1 / |mu|_p with mu = 1 / lambda, which lies between
    min(lambda) k^(-1/p) and min(lambda).  +inf entries (mu = 0) are ignored; a row of them alone gives +inf with zero
    gradient.  Plain differentiable torch, evaluated with the largest mu detached so that a large p does not overflow."""
    p = float(p)
    if not p >= 1.0:
        raise ValueError(f"aggregate needs p >= 1, got {p!r}")
    live = torch.isfinite(lam) & (lam > 0)
    mu = torch.where(live, 1.0 / torch.where(live, lam, torch.ones_like(lam)), torch.zeros_like(lam))
    top = mu.detach().amax(dim=dim, keepdim=True)
    some = top > 0
    r = mu / torch.where(some, top, torch.ones_like(top))
    norm = (top * (r ** p).sum(dim=dim, keepdim=True) ** (1.0 / p)).squeeze(dim)
    some = some.squeeze(dim)
    return torch.where(some, 1.0 / torch.where(some, norm, torch.ones_like(norm)), torch.full_like(norm, float("inf")))


def _voigt(dim: int) -> int:
    return dim * (dim + 1) // 2


def _buckling_layout(E: torch.Tensor, sigma: torch.Tensor, m: int, nc: int, batch: Optional[int]):
    """-> (mode of E, mode of sigma0, B, batched) of one call.  sigma0 is (m, nc), shared by the batch, or (B, m, nc); E is
    read as `ElasticEigenSolver` reads it, next to the batch of sigma0 where `batch` is not given."""
    if batch is not None and int(batch) < 1:
        raise ValueError(f"batch must be >= 1, got {batch!r}")
    b = None if batch is None else int(batch)
    if sigma.dim() == 2 and tuple(sigma.shape) == (m, nc):
        mode_s, Bs = K_ELEM, None
    elif sigma.dim() == 3 and tuple(sigma.shape[1:]) == (m, nc):
        mode_s, Bs = K_SAMPLE_ELEM, sigma.shape[0]
    else:
        raise ValueError(f"prestress shape {tuple(sigma.shape)} not understood for a mesh with {m} elements: expected "
                         f"({m}, {nc}) or (B, {m}, {nc}) in Voigt components, as `stress` returns them")
    mode_e, Be = _field_layout(E, "E", m, b if b is not None else Bs)
    for name, Bk in (("E", Be), ("prestress", Bs)):
        if b is not None and Bk is not None and Bk != b:
            raise ValueError(f"{name} batch {Bk} does not match batch={batch}")
    if Be is not None and Bs is not None and Be != Bs:
        raise ValueError(f"prestress batch {Bs} does not match E batch {Be}")
    Bk = Be if Be is not None else Bs
    B = Bk if Bk is not None else (b if b is not None else 1)
    return mode_e, mode_s, B, (Bk is not None or b is not None)


class _BucklingRun(_BlockRun):
    """One buckling call: the dof operator K and its Galerkin chain, G on the node pattern, the block N Y next to K Y, the
    shifts and the block buffers.  After `run()` it keeps what backward reads: the k columns, lambda and the plan."""
    Info = BucklingInfo

    def __init__(self, bs: "LinearBucklingSolver", E: torch.Tensor, sigma: torch.Tensor, batch: Optional[int]):
        self.es, self.plan = bs, bs._plan()
        plan, inner = self.plan, bs.inner
        self.setup = _setup_of(plan, inner.nu, inner.plane, inner._lam1, inner._mu1, inner._is_bc, inner._g)
        dofs = self.setup.dofs
        self.nc = _voigt(plan.dim)
        self.mode_e, self.mode_s, self.B, self.batched = _buckling_layout(E, sigma, plan.m, self.nc, batch)
        self.Bp = padded_batch(self.B)
        self.k, self.p = bs.k, bs.k + bs.guard
        self.rows, self.vec, self.d = dofs.n, (plan.n, plan.dim), plan.dim
        n_free = dofs.n - int(inner._is_bc.sum())
        if self.p > n_free:
            raise ValueError(f"block of {self.p} vectors on a mesh with {n_free} free dofs")
        self.e_shape, self.e_device, self.s_shape, self.s_device = E.shape, E.device, sigma.shape, sigma.device
        self.L = _hip.lib()
        self.node_eng = _Engine(plan, 0.0, 0, 0, "gather")
        self.eng = _Engine(dofs, bs.inner_tol, int(bs.amg.get("max_iter", 20000)), 25, "gather", g=dofs.g)
        self.X = None

    # -- the problem: N = -G(sigma0) (x) I_d against K(E) on the dofs ----------------------------------------------------------
    def _bc_rows(self):
        return None if self.setup.free.all() else ~self.setup.free

    def _setup(self, coeffs, Y: torch.Tensor, info: BucklingInfo, keep: bool = False) -> None:
        """K, its Galerkin operators and G, once; no solve."""
        E, sigma = coeffs
        bs, plan, setup, L, B, Bp = self.es, self.plan, self.setup, self.L, self.B, self.Bp
        dofs, st = setup.dofs, _stream(plan.device)
        kdev, kse, ksb, Bv = self.node_eng.kappa_device(E, self.mode_e, B, Bp)
        # a per-sample field of a batch of one has width 1: the entries take it as a shared field, stride 0
        self.vals, _ = setup.assemble(kdev, kse, ksb if Bv > 1 else 0, Bv)
        self.Bv = Bv
        sinfo, self.amg = SolveInfo(), dict(bs.amg)
        self.hier, _ = _select_hierarchy(self.eng, setup, bs.method, self.amg, self.vals, Bv, Bp, sinfo)
        info.inner, info.path = sinfo, sinfo.path
        # G: the tensor assembly of csrc/aniso.hip with the stress in the conductivity's place and no Dirichlet data (its
        # padding samples carry the identity: a body in tension, no positive mu)
        sdev, ssc, sse, ssb, Bg = self.node_eng.tensor_device(sigma, self.mode_s, B, Bp, self.nc)
        gtab, vol = plan.gradient_table()
        self.G, self.Bg = self._new(plan.W, plan.n, Bg), Bg
        L.diffhe_aniso_assemble_rows(gtab, vol, plan.dim, sdev, ssc, sse, ssb if Bg > 1 else 0, plan.ent_ptr, plan.contrib,
                                     plan.cols, None, None, self.G, None, plan.n, plan.m, plan.W, Bg, st)
        p, n = self.p, self.rows
        self._apart = self._new(L.diffhe_grad_kappa_blocks(n, Bp) * Bp)
        if bs.iteration == "subspace":
            self.NY, self.NX = self._new(p, n, Bp), self._new(p, n, Bp)
        else:                   # LOBPCG carries K_G S and K S as blocks of the basis
            self.NY = self.NX = None
        self.mu, self.coef, self.dots = self._new(p, Bp), self._new(p, Bp), self._new(p, Bp)
        self.shift = torch.zeros(Bp, dtype=torch.float64, device=plan.device)
        self.neg_seen = torch.zeros(Bp, dtype=torch.int64, device=plan.device)
        self.info, self._outer = info, 0

    def _apply_column(self, i: int, Y, KY) -> None:
        """K y_i (identity on the fixed rows, where y is 0) and N y_i = -(G (x) I_d) y_i."""
        plan, dofs, L, st = self.plan, self.setup.dofs, self.L, _stream(self.plan.device)
        L.diffhe_ell_apply(self.vals, dofs.cols, Y[i], KY[i], self._apart, dofs.n, dofs.W, self.Bp, self.Bv, st)
        L.diffhe_buckling_apply(self.G, plan.cols, dofs.is_bc, Y[i], self.NY[i], -1.0, plan.n, plan.W, self.d, self.Bp,
                                self.Bg, st)

    def _inner_solve(self, rhs: torch.Tensor):
        if self.hier is not None:
            return self.eng.amg_pcg(self.hier, rhs, self.Bp, self.Bv, self.amg)
        return self.eng.cg(self.vals, rhs, self.Bp, self.Bv)

    def _next_column(self, i: int, res, Y, KY) -> None:
        """y_i = (mu_i + s) x_i + d_i with d_i^T r_i left in `dots`, then K y_i and N y_i."""
        b = self.buf
        self._outer += i == 0
        self.L.diffhe_buckling_step(b["X"][i], res.x, b["R"][i], self.coef[i], self.rows, self.Bp, Y[i], self._apart,
                                    self.dots[i], _stream(self.plan.device))
        self._apply_column(i, Y, KY)

    def _rayleigh_ritz(self, Y, KY) -> None:
        """rho of the last block from the dots of its inner solves; then Gram -> Ritz on (-GN, GK) -> rotate, the shifts
        and the coefficients mu + s of the next block."""
        L, p, n, Bp, st = self.L, self.p, self.rows, self.Bp, _stream(self.plan.device)
        b = self.buf
        if self._outer:
            pos = self.mu > 0.0
            torch.where(pos, self.dots.clamp_min(0.0).sqrt() / torch.where(pos, self.mu, torch.ones_like(self.mu)),
                        torch.zeros_like(self.mu), out=b["rho"])
        else:
            b["rho"].fill_(float("inf"))            # not measured yet
        L.diffhe_buckling_gram(Y, KY, self.NY, self.setup.dofs.is_bc, p, n, Bp, b["part"], b["GM"], b["GA"], st)
        b["GA"].neg_()
        L.diffhe_eig_ritz(b["GA"], b["GM"], p, Bp, JACOBI_SWEEPS, b["work"], b["C"], b["theta"], b["flag"], st)
        torch.neg(b["theta"], out=self.mu)          # theta = -mu ascending: mu descending, the positive ones first
        L.diffhe_buckling_rotate(Y, KY, self.NY, b["C"], self.mu, p, n, Bp, b["X"], b["AX"], self.NX, b["R"], st)
        torch.maximum(self.shift, 0.5 * b["theta"].clamp_min(0.0).amax(dim=0), out=self.shift)
        torch.add(self.mu, self.shift[None, :], out=self.coef)
        torch.maximum(self.neg_seen, (b["theta"] > 0.0).sum(dim=0), out=self.neg_seen)

    # -- what LOBPCG asks of the problem: the pencil (K_G, K), theta = -mu, no shift --------------------------------------------
    def _free_mask(self):
        return self.setup.dofs.is_bc

    def _lobpcg_apply(self, blk, j: int) -> None:
        """K_G s_j = (G (x) I_d) s_j into A S and K s_j into B S."""
        plan, dofs, L, st = self.plan, self.setup.dofs, self.L, _stream(self.plan.device)
        L.diffhe_buckling_apply(self.G, plan.cols, dofs.is_bc, blk["S"][j], blk["AS"][j], 1.0, plan.n, plan.W, self.d,
                                self.Bp, self.Bg, st)
        L.diffhe_ell_apply(self.vals, dofs.cols, blk["S"][j], blk["BS"][j], self._apart, dofs.n, dofs.W, self.Bp, self.Bv, st)

    def _lobpcg_column(self, i: int, res, blk) -> None:
        """w_i into the W slot with w_i^T r_i left in `dots` (the step entry with a zero coefficient: one pass for both),
        then its operator columns."""
        b, j = self.buf, self.p + i
        self._outer += i == 0
        self.L.diffhe_buckling_step(b["X"][i], res.x, b["R"][i], self.coef[i], self.rows, self.Bp, blk["S"][j],
                                    self._apart, self.dots[i], _stream(self.plan.device))
        self._lobpcg_apply(blk, j)

    def _lobpcg_pre(self) -> None:
        """rho of the block the inner solves just read, from their dots (the measure is known one iteration late).  A
        column without a positive mu has nothing to measure (rho 0: it counts as done, as under "subspace"); for mu > 0 a dot
        that is not positive cannot come from a solve with K and measures nothing: rho = inf."""
        b = self.buf
        if self._outer:
            pos = self.mu > 0.0
            inf = torch.full_like(self.mu, float("inf"))
            measured = torch.where(self.dots > 0.0, self.dots.clamp_min(0.0).sqrt() / torch.where(pos, self.mu,
                                                                                              torch.ones_like(self.mu)), inf)
            torch.where(pos, measured, torch.zeros_like(self.mu), out=b["rho"])
        else:
            b["rho"].fill_(float("inf"))            # not measured yet
            self.coef.zero_()                       # stays 0: the step entry then copies w_i
        self._had_mu = self.mu > 0.0 if self._outer else None

    def _lobpcg_post(self) -> None:
        """mu of the new block.  A column that had no positive mu when its residual would have been measured but has one
        now -- Ritz on [X | W] can turn up k positive values in one step from a start block that had none -- has NOT been
        measured: its rho is inf until the next iteration measures it, so the run cannot stop on it."""
        b = self.buf
        torch.neg(b["theta"], out=self.mu)          # theta = -mu ascending: mu descending, the positive ones first
        if self._had_mu is not None:
            b["rho"].masked_fill_((self.mu > 0.0) & ~self._had_mu, float("inf"))
        torch.maximum(self.neg_seen, (b["theta"] > 0.0).sum(dim=0), out=self.neg_seen)

    def _status(self) -> Tuple[int, int]:
        """The one host read of an outer iteration.  A wanted column without a positive Ritz value counts as done (its
        rho is 0), but keeps the iteration running for its first `MIN_OUTER_MISSING` rounds."""
        b, k, B = self.buf, self.k, self.B
        above = (~(b["rho"][:k, :B] <= self.es.tol)).sum()
        missing = (~(self.mu[:k, :B] > 0.0)).sum()
        vals = torch.stack([above, b["flag"][:B].sum().to(above.dtype), missing]).cpu()
        above, failed, self._missing = int(vals[0]), int(vals[1]), int(vals[2])
        if not above and self._missing and self._outer < MIN_OUTER_MISSING:
            above = self._missing
        return above, failed

    def _fix_sign(self, X, sgn) -> None:
        """The sign rule of `ElasticEigenSolver` under a unit mass; the columns without a positive mu are zeroed."""
        one = torch.ones(1, dtype=torch.float64, device=self.plan.device)
        self.L.diffhe_modal_fix_sign(X, one, 0, 0, self.d, self.k, self.rows, self.Bp, self.buf["part"], sgn,
                                     _stream(self.plan.device))
        X[:self.k] *= (self.mu[:self.k] > 0.0).to(torch.float64)[:, None, :]

    def _eigenvalues(self) -> torch.Tensor:
        mu = self.mu[:self.k, :self.B]
        pos = mu > 0.0
        lam = torch.where(pos, 1.0 / torch.where(pos, mu, torch.ones_like(mu)), torch.full_like(mu, float("inf")))
        return lam.t().contiguous()

    def _release(self) -> None:
        # what backward needs: the k columns, lambda (0 where it is +inf) and the plan's element tables
        info, B, k = self.info, self.B, self.k
        mu = self.mu[:k]
        pos = mu > 0.0
        self.lam = torch.where(pos, 1.0 / torch.where(pos, mu, torch.ones_like(mu)), torch.zeros_like(mu))     # (k, Bp)
        info.shifts = self.shift[:B].cpu()
        info.negative_ritz = int(self.neg_seen[:B].sum())
        info.missing = int((~pos[:, :B]).sum())
        if info.missing:
            warnings.warn(f"diffhe: {info.missing} of {B * k} buckling factors are missing (fewer than {k} positive Ritz "
                          "values: the prestress leaves the sample that few ways to buckle); they are returned as +inf "
                          "with zero modes", RuntimeWarning)
        self.g0, self.lam1, self.mu1 = self.setup.dofs.g, self.setup.lam1, self.setup.mu1
        self.vals = self.hier = self.G = self.NY = self.NX = self._apart = self.eng = self.setup = None
        self.coef = self.dots = self.neg_seen = self.info = self._had_mu = None

    def backward(self, glam: torch.Tensor, need_e: bool, need_s: bool):
        """(dL/dE, dL/dsigma0) in the shapes of E and sigma0 from the cotangent of lam.  dE: the strain-form gradient
        kernels (which compute -lam^T K_e0 u) with u = phi_i and lam = -lambda_bar_i lambda_i phi_i, summed over i;
        dsigma0: one element pass with the weights lambda_bar_i lambda_i^2.  +inf entries carry weight 0."""
        plan, eng, L, B, Bp, k, nc = self.plan, self.node_eng, self.L, self.B, self.Bp, self.k, self.nc
        st = _stream(plan.device)
        gp = torch.zeros((k, Bp), dtype=torch.float64, device=plan.device)
        gp[:, :B] = glam.detach().to(plan.device, torch.float64).reshape(B, k).t()
        gl = torch.where(self.lam > 0.0, gp * self.lam, torch.zeros_like(gp))      # lambda_bar lambda, 0 where missing
        gtab, vol = plan.gradient_table()
        grad_e = grad_s = None
        if need_e:
            acc = None
            for i in range(k):
                lamv = self.X[i] * (-gl[i])[None, :]
                args = (plan.elems, gtab, vol, plan.dim, self.lam1, self.mu1, lamv, self.X[i], self.g0, plan.n, plan.m)
                sums, elem = eng.element_grad(
                    self.mode_e, True, B, Bp, None,
                    lambda de_e, osc, ose, part, total: L.diffhe_elast_grad(*args, Bp, de_e, part, total, st),
                    lambda de, osc, ose: L.diffhe_elast_grad_shared(*args, B, Bp, de, st))
                part = elem if sums is None else sums
                acc = part if acc is None else acc + part
            sums, elem = (acc, None) if self.mode_e not in (K_ELEM, K_SAMPLE_ELEM) else (None, acc)
            if self.mode_e == K_SAMPLE_ELEM:        # asked for element-major (m, B): no transposing pass per column
                elem = elem.t().contiguous()
            grad_e = _kappa_grad(self.mode_e, self.e_shape, sums, elem).to(self.e_device)
        if need_s:
            w = gl * self.lam
            args = (plan.elems, gtab, vol, plan.dim, self.X, w, k, plan.n, plan.m, B, Bp)
            _, ds = eng.element_grad(
                self.mode_s, False, B, Bp, nc,
                lambda ds_e, osc, ose, part, total: L.diffhe_buckling_grad_sigma(*args, ds_e, osc, ose, part, total, st),
                lambda ds, osc, ose: L.diffhe_buckling_grad_sigma_shared(*args, ds, osc, ose, st))
            grad_s = ds.reshape(self.s_shape).to(self.s_device)
        return grad_e, grad_s


# ---------------------------------------------------------------------------------------------
# torch.library custom ops diffhe::buckling_solve / diffhe::buckling_solve_backward: the solver and the state of the call
# travel as integer handles through the registries of diffhe.solver.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("diffhe::buckling_solve", mutates_args=())
def buckling_solve(E: torch.Tensor, sigma: torch.Tensor, x0: Optional[torch.Tensor], handle: int, batch: int,
                   node_layout: bool, save: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(lam, phi, token) of the `LinearBucklingSolver` registered under `handle` for the prestress sigma; batch < 1: none
    given; `token` names the saved state of the call (0 when `save` is false)."""
    run = _BucklingRun(_SOLVERS[handle], E, sigma, batch if batch >= 1 else None)
    lam, phi = run.run((E, sigma), x0, node_layout)
    # fresh tensors (an op's outputs may not alias one another); with layout="node" phi is the block itself
    return lam.to(E.device), phi.to(E.device), _register_state(run, save)


@buckling_solve.register_fake
def _buckling_solve_fake(E, sigma, x0, handle, batch, node_layout, save):
    bs = _SOLVERS[handle]
    n, d, m, k = bs.mesh.n_nodes, bs.mesh.dim, bs.mesh.n_elements, bs.k
    _, _, B, batched = _buckling_layout(E, sigma, m, _voigt(d), batch if batch >= 1 else None)
    lam = E.new_empty((B, k) if batched else (k,), dtype=torch.float64)
    if node_layout:
        phi = E.new_empty((k, n, d, B), dtype=torch.float64)
    else:
        phi = E.new_empty((B, k, n, d) if batched else (k, n, d), dtype=torch.float64)
    return lam, phi, torch.empty((), dtype=torch.int64)


@torch.library.custom_op("diffhe::buckling_solve_backward", mutates_args=())
def buckling_solve_backward(glam: torch.Tensor, token: torch.Tensor, need_e: bool, need_s: bool, e_like: torch.Tensor,
                            s_like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dL/dE, dL/dsigma0) of the call named by `token` from the cotangent of lam; no solve; unused ones come back empty."""
    return _like_grads(glam, _state_of(token).backward(glam, need_e, need_s), (e_like, s_like))


@buckling_solve_backward.register_fake
def _buckling_solve_backward_fake(glam, token, need_e, need_s, e_like, s_like):
    return _fake_grads(glam, (need_e, need_s), (e_like, s_like))


def _setup_context(ctx, inputs, output):
    """Save (token, E, sigma0) and tie the saved state of the call to them.  phi (and the token) are marked
    non-differentiable."""
    lam, phi, token = output
    ctx.mark_non_differentiable(phi, token)
    _tie_state(ctx, token, inputs[0], inputs[1])


def _backward(ctx, glam, _gphi, _gtoken):
    if torch.is_grad_enabled():
        raise NotImplementedError("diffhe: second-order derivatives of buckling factors are not implemented (backward with "
                                  "create_graph=True, diffhe.buckling)")
    token, E, sigma = ctx.saved_tensors[:3]
    need_e, need_s = (bool(v) for v in ctx.needs_input_grad[:2])
    if not (need_e or need_s):
        return (None,) * 7
    ge, gs = torch.ops.diffhe.buckling_solve_backward(glam.contiguous(), token, need_e, need_s, E, sigma)
    return (ge if need_e else None, gs if need_s else None, None, None, None, None, None)


torch.library.register_autograd("diffhe::buckling_solve", _backward, setup_context=_setup_context)


class LinearBucklingSolver(nn.Module):
    """The k smallest positive load factors lambda of (K(E) + lambda K_G(sigma0)) phi = 0 per sample and their modes --
    linear buckling of an elastic body -- with `lam` differentiable with respect to E and the prestress, and through the
    prestress solve with respect to the loads (see the module docstring for the problem, the method, the stopping measure,
    the gradients and their limits on degenerate clusters; phi is returned non-differentiable).

    Parameters
    ----------
    mesh : FEMesh -- P1 triangles or P1 tetrahedra.
    E : float or tensor or Parameter -- (), (m,), (B,) / (B, 1) or (B, m); may require grad.
    k : number of load factors; guard : extra block columns (block p = k + guard <= 16).
    nu, plane, fixed : as on `ElasticFESolver`; the modes are zero on the fixed dofs whatever value `fixed` prescribes.
    tol : stop when rho_i = |A x_i - mu_i x_i|_K / mu_i <= tol for the k columns of every sample; max_iter : outer
        iterations.
    inner_tol : relative residual of the inner solves d_i = K^-1 r_i; the stopping measure is as accurate as they are.
    seed : of the CPU generator the start block is drawn from.
    method ("auto" or "ell-jacobi"), amg, device : as on `ElasticFESolver`, also for the prestress solve (`solver.inner`).
    iteration : "subspace" (default), the shifted block iteration of the module docstring, or "lobpcg": Rayleigh-Ritz on
        span{X, K^-1 R, P} of the pencil (K_G, K), theta = -mu, which picks the wanted end of the spectrum by itself -- no
        shift (`last_info.shifts` is 0) and fewer outer iterations ("LOBPCG"); the stopping measure, the
        sign rule, the +inf handling and the gradients are the same.
    """
    _no_distributed = "diffhe: the diffhe.distributed helpers are not implemented for LinearBucklingSolver"

    def __init__(self, mesh, E=1.0, k: int = 4, *, nu: float = 0.3, plane: Optional[str] = None, fixed=None,
                 guard: int = 4, tol: float = 1e-8, max_iter: int = 200, inner_tol: float = 1e-3, seed: int = 0,
                 method: str = "auto", amg: Optional[dict] = None, device=None, iteration: str = "subspace"):
        super().__init__()
        self.iteration = _check_iteration(iteration)
        _check_mesh(mesh, "diffhe: linear buckling needs a 2D or 3D mesh (a 1D bar carries no bending: Euler buckling of a "
                    "rod is not in the P1 bar model)",
                    "diffhe: linear buckling is implemented for P1 elements only (K_G = G (x) I_d is read from the node "
                    "pattern of a mesh with {k} nodes per element otherwise)", dims="Only 2D and 3D meshes supported")
        if method not in ("auto", "ell-jacobi"):
            raise ValueError(f"Unknown method: {method!r}")
        k, guard = int(k), int(guard)
        if k < 1 or guard < 0 or k + guard > MAX_BLOCK:
            raise ValueError(f"need 1 <= k and guard >= 0 with k + guard <= {MAX_BLOCK}, got k={k}, guard={guard}")
        if not (float(tol) > 0.0) or not (0.0 < float(inner_tol) < 1.0) or int(max_iter) < 0:
            raise ValueError(f"need tol > 0, 0 < inner_tol < 1, max_iter >= 0, got {tol!r}, {inner_tol!r}, {max_iter!r}")
        if isinstance(E, torch.Tensor) and (E.dim() >= 3 or (E.dim() == 2 and E.shape[0] == E.shape[1] and E.shape[0] in (3, 6)
                                                             and E.shape[1] not in (1, mesh.n_elements))):
            raise NotImplementedError("diffhe: linear buckling with a stiffness tensor (AnisotropicElasticFESolver) is not "
                                      "implemented (a Young's modulus per element only)")
        self.inner = ElasticFESolver(mesh, E, nu, plane=plane, fixed=fixed, device=device, method=method, amg=amg)
        self.amg = self.inner.amg
        self.mesh, self.method, self.k, self.guard = mesh, method, k, guard
        _field_layout(self.inner.E, "E", mesh.n_elements, None)
        self.tol, self.max_iter, self.seed, self.inner_tol = float(tol), int(max_iter), int(seed), float(inner_tol)
        self.last_info = BucklingInfo()

    @property
    def E(self) -> torch.Tensor:
        return self.inner.E

    @property
    def nu(self) -> float:
        return self.inner.nu

    @property
    def plane(self) -> Optional[str]:
        return self.inner.plane

    def _plan(self):
        return self.inner._plan()

    def _prestress(self, f, load, batch: Optional[int]):
        """sigma0 of the linear prestress solve, through the differentiable solve and stress ops of `self.inner`; where
        `batch` is given and the right-hand side carries none, it is expanded to it (so that E reads as it will)."""
        n, d = self.mesh.n_nodes, self.mesh.dim
        if batch is not None:
            rhs = [None if t is None else (t if isinstance(t, torch.Tensor) else torch.as_tensor(t)) for t in (f, load)]
            if not any(t is not None and t.dim() == 3 for t in rhs):
                rhs = [None if t is None else t.reshape(1, n, d).expand(int(batch), n, d) for t in rhs]
            f, load = rhs
        u = self.inner(f, load)
        return self.inner.stress(u)

    def forward(self, f: Optional[torch.Tensor] = None, load: Optional[torch.Tensor] = None, *, prestress=None,
                batch: Optional[int] = None, x0: Optional[torch.Tensor] = None, layout: str = "sample"):
        """-> (lam, phi).  f, load: the body force and the nodal load of the prestress solve, (n, d) or (B, n, d), as
        `ElasticFESolver` takes them; prestress: sigma0 itself, (m, nc) or (B, m, nc), in place of them (no solve) -- both
        or neither is a ValueError.  batch: the number of samples, where nothing says (or E reads both ways); x0: a
        previous phi in the same `layout` as a warm start -- with k columns it is padded with seeded random guard columns,
        with k + guard columns it is the whole start block; layout: "sample" = phi (B, k, n, d), "node" = phi
        (k, n, d, B)."""
        if layout not in ("sample", "node"):
            raise ValueError(f"Unknown layout: {layout!r}")
        loaded = f is not None or load is not None
        if prestress is not None and loaded:
            raise ValueError("give either f / load (the prestress solve is made here) or prestress=, not both")
        if prestress is None and not loaded:
            raise ValueError("a buckling call needs a load: give f and / or load, or prestress=")
        if self.mesh.nodes.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("diffhe: node gradients are not implemented for linear buckling (mesh.nodes requires "
                                      "grad)")
        E, m, nc = self.inner.E, self.mesh.n_elements, _voigt(self.mesh.dim)
        info = None
        if prestress is None:
            sigma = self._prestress(f, load, batch)
            info = self.inner.last_info
        else:
            sigma = prestress if isinstance(prestress, torch.Tensor) else torch.as_tensor(prestress)
            sigma = sigma.to(torch.float64)
        _buckling_layout(E, sigma, m, nc, batch)
        _SOLVERS[id(self)] = self
        save = torch.is_grad_enabled() and (E.requires_grad or sigma.requires_grad)
        lam, phi, _token = torch.ops.diffhe.buckling_solve(E, sigma, None if x0 is None else x0.detach(), id(self),
                                                           -1 if batch is None else int(batch), layout == "node", save)
        self.last_info.prestress = info
        return lam, phi
