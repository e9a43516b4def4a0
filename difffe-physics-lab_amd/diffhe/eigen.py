"""Smallest eigenpairs of K(kappa) phi = lambda M_L phi per sample, with d lambda / d kappa (ours: the reference has no
eigensolver; its habit would be a dense `torch.linalg.eigh` of an assembled matrix, O(n^3)).

`EigenFESolver(mesh, kappa, k)` finds, for every sample b, the k smallest eigenvalues and their vectors of the P1
stiffness operator of `DifferentiableFESolver` against the LUMPED mass M_L (`plan.lumped_mass()`, the mean-value rule of
`reaction=` and `diffhe.heat`): the fundamental frequencies of a membrane, the slowest decay rates of `HeatEquation`.
Boundary conditions are HOMOGENEOUS Dirichlet on the mesh's Dirichlet nodes: only the keys of `mesh.dirichlet_nodes`
are used, its values are ignored (the kernels read `plan.zero_g()`).

Method: block inverse iteration with Rayleigh-Ritz on p = k + guard <= 16 vectors ("Eigenpairs").
The operator is assembled and its multigrid hierarchy built ONCE per call, by the inner solver's own path object (set up
by `solver._begin_call`, as for any solve), whose saved operators every later solve reuses.  Each outer iteration solves A d_i = theta_i M x_i - A x_i for the p columns
(A = K + shift M_L; the correction form of A y_i = theta_i M x_i started from x_i) to the loose relative tolerance
`inner_tol`, applies A to Y = X + D explicitly, and runs four HIP passes of csrc/eigen.hip: per-sample Gram matrices,
a dense Ritz step per sample (Cholesky + cyclic Jacobi, one sample per lane), the block rotation X = Y C, and the
residual norms rho = |A x - theta M x|_{M^-1} / theta of the M-normalised Ritz vectors -- computed from the explicit
A Y, so they certify the result whatever the inner tolerance was.  The iteration stops when rho <= tol for the first k
columns of every sample (one host read per outer iteration); what is left above `tol` at `max_iter` is counted in
`last_info.not_converged` and warned about.  The iteration itself is `_BlockRun`, which `diffhe.modal` runs on the dofs of
an elastic body with a mass per sample; `_EigenRun` is the scalar problem on it.

`iteration="lobpcg"` swaps the outer iteration for LOBPCG on the same inner solves and stopping measure: Rayleigh-Ritz on the
basis [X | W | P] -- W the p inner solves of the residuals, P the previous step -- carried as one (3p, rows, Bp) buffer next
to A S and M S, by the three passes of csrc/lobpcg.hip ("LOBPCG"); `last_info.iteration` and
`last_info.basis_drops` report it.  The default, "subspace", is the iteration described above, unchanged.

kappa layouts are the scalar ones of the base class, read as for a call whose f carries no batch: () one value,
(m,) per element, (B,) or (B, 1) per sample, (B, m) per sample and element; `batch=B` forces the per-sample reading of
a (B,) kappa when B == m.  Returns `lam` (B, k) ascending -- (k,) when neither kappa nor `batch=` carries a batch -- and
`phi` (B, k, n), or with layout="node" (k, n, B), the block's own layout, without a transposing pass.  phi is
M_L-orthonormal per sample, zero on the Dirichlet nodes, and signed so that sum_i m_i phi_i > 0 (where that sum is below
1e-8 in magnitude: the entry of largest magnitude is positive).

Gradients.  `lam` is differentiable with respect to kappa in every layout by the Hellmann-Feynman formula
d lambda_i / d kappa_e = phi_i^T k0_e phi_i (phi M-normalised), evaluated by the gradient kernels of the solve
(u = phi_i, adjoint vector = -lambda_bar_i phi_i): deterministic, no solve in backward.  `phi` is returned
NON-differentiable: its derivative needs deflated indefinite solves (out of scope).  For a cluster of equal eigenvalues
the returned vectors are an arbitrary M-orthonormal basis of the eigenspace and the gradient is that of their Rayleigh
quotients: correct for symmetric functions of the cluster such as its sum, NOT for a single member of a degenerate pair.

Not covered (NotImplementedError): 1D meshes (a tridiagonal pencil is dense-eigh territory), P2 meshes (row-sum lumping
is not positive there), conductivity tensors, Robin terms, the `diffhe.distributed` helpers; interior eigenvalues and the
consistent mass matrix are not offered.  A mesh without Dirichlet nodes needs `shift > 0` (ValueError otherwise): the
inner solves then run on K + shift M_L through the `reaction=` mechanism, the returned lambda exclude the shift, and the
lambda_1 = 0 mode is found like any other.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _hip
from .plan import padded_batch, _stream
from .solver import (DifferentiableFESolver, K_ELEM, K_SAMPLE_ELEM, SolveInfo, _Call, _LatticeSolve, _SOLVERS, _begin_call,
                     _kappa_grad, _kappa_mode, _register_state, _state_of, _tie_state)
from .tet3d import DifferentiableFESolver3D

__all__ = ("EigenFESolver", "EigenInfo")

MAX_BLOCK = 16          # kMaxP of csrc/eigen.hip
JACOBI_SWEEPS = 30      # cap of the cyclic Jacobi sweeps (quadratic convergence: 6-9 are taken at p = 16)
ITERATIONS = ("subspace", "lobpcg")
LOBPCG_REFRESH = 8      # outer iterations between two fresh applications of the operators to X ("LOBPCG")
LOBPCG_RETRIES = 2      # of those refreshes, the first so many also let a sample that gave up P try [X | W | P] again


def _check_iteration(iteration) -> str:
    if iteration not in ITERATIONS:
        raise ValueError(f"Unknown iteration: {iteration!r} (expected 'subspace' or 'lobpcg')")
    return iteration


@dataclass
class EigenInfo:
    """Diagnostics of the last eigen call."""
    path: str = ""
    outer_iterations: int = 0
    inner_solves: int = 0
    inner_iterations: int = 0           # PCG iterations summed over the inner solves (each counts its slowest sample)
    inner_not_converged: int = 0        # (solve, sample) pairs whose inner solve missed `inner_tol`
    inner_tol: float = 0.0
    block: int = 0                      # p = k + guard
    residual: Optional[torch.Tensor] = None     # (B, k) final rho per (sample, mode), on the CPU
    not_converged: int = 0              # (sample, mode) pairs above `tol` when the iteration ended
    gram_failures: int = 0              # samples whose Gram matrix was not positive definite in the last Ritz step
    iteration: str = "subspace"         # the outer iteration that ran: "subspace" or "lobpcg"
    basis_drops: int = 0                # "lobpcg": (outer iteration, sample) pairs whose Ritz step fell back to a smaller basis
    inner: SolveInfo = field(default_factory=SolveInfo)     # the inner solver's record of the set-up solve


def _eigen_layout(kappa: torch.Tensor, m: int, batch: Optional[int]):
    """-> (mode, B, batched) of an eigen call: `_kappa_mode` as for a call whose f carries no batch, unless `batch` is
    given (it then decides how a (B,) kappa with B == m reads, and is the batch of a kappa that carries none)."""
    if batch is not None and int(batch) < 1:
        raise ValueError(f"batch must be >= 1, got {batch!r}")
    if kappa.dim() >= 3 or (kappa.dim() == 2 and kappa.shape[1] not in (1, m) and kappa.shape[1] in (3, 6)):
        raise NotImplementedError("diffhe: eigenpairs with a conductivity tensor are not implemented (scalar kappa only)")
    mode, Bk = _kappa_mode(kappa, m, None if batch is None else int(batch))
    if batch is not None and Bk is not None and Bk != int(batch):
        raise ValueError(f"kappa batch {Bk} does not match batch={batch}")
    B = Bk if Bk is not None else (int(batch) if batch is not None else 1)
    return mode, B, (Bk is not None or batch is not None)


class _BlockRun:
    """The block inverse iteration with Rayleigh-Ritz of DESIGN section 7 "Eigenpairs" on vectors of `rows` unknowns, each
    shaped `vec` -- (n,) for the scalar operator, (n, d) for a displacement.  A subclass supplies the problem: `_setup`
    (assemble once, hierarchy once), `_apply` (y = A x), `_inner_solve`, the four mass-weighted passes (`_rayleigh_ritz`,
    `_fix_sign`), `_bc_rows` and `_release`; and sets es, plan, L, B, Bp, batched, k, p, rows, vec before `run`.  After
    `run()` X holds the k returned columns.

    The right-hand matrix of the pencil is the subclass's business: the two mass-weighted problems read a diagonal mass in
    their passes; a pencil whose right-hand matrix is an operator (`diffhe.buckling`) carries it as a block next to A Y and
    overrides the three column hooks `_apply_column`, `_next_column` and `_eigenvalues`, whose defaults are the inverse
    iteration of the mass-weighted problems."""
    Info = EigenInfo        # the class of `last_info` after a run

    def _new(self, *shape, dtype=torch.float64):
        return torch.empty(shape, dtype=dtype, device=self.plan.device)

    def _start_block(self, x0, node_layout: bool) -> torch.Tensor:
        """(p, rows, Bp): seeded random columns (one draw per column, shared by the samples), the leading ones replaced
        by `x0` where given; zero on the Dirichlet rows."""
        plan, p, n, B, Bp, vec = self.plan, self.p, self.rows, self.B, self.Bp, tuple(self.vec)
        gen = torch.Generator().manual_seed(int(self.es.seed))
        cols = torch.randn(p, n, generator=gen, dtype=torch.float64).to(plan.device)
        Y = cols[:, :, None].expand(p, n, Bp).contiguous()
        if x0 is not None:
            x = x0.detach().to(plan.device, torch.float64)
            nv = len(vec)
            if node_layout:
                ok = x.dim() == 2 + nv and tuple(x.shape[1:-1]) == vec and x.shape[-1] == B
                x = x.reshape(x.shape[0], n, B) if ok else x
            else:
                if x.dim() == 1 + nv and not self.batched:
                    x = x[None]
                ok = x.dim() == 2 + nv and x.shape[0] == B and tuple(x.shape[2:]) == vec
                x = x.reshape(B, x.shape[1], n).permute(1, 2, 0) if ok else x
            if not ok or not (self.k <= x.shape[0] <= p):
                dims = ", ".join(str(v) for v in vec)
                want = f"(c, {dims}, {B})" if node_layout else f"({B}, c, {dims})"
                raise ValueError(f"x0 must be a previous phi, {want} with {self.k} <= c <= {p}, got {tuple(x0.shape)}")
            Y[:x.shape[0], :, :B] = x
        bc = self._bc_rows()
        if bc is not None:
            Y[:, bc, :] = 0.0
        return Y

    def _status(self) -> Tuple[int, int]:
        """The one host read of an outer iteration: ((sample, mode) pairs above tol, samples with a failed Gram matrix).
        A rho that is not a number counts as above tol."""
        b, k, B = self.buf, self.k, self.B
        above = (~(b["rho"][:k, :B] <= self.es.tol)).sum()
        both = torch.stack([above, b["flag"][:B].sum().to(above.dtype)]).cpu()
        return int(both[0]), int(both[1])

    # -- the column hooks -----------------------------------------------------------------------------------------------
    def _apply_column(self, i: int, Y, AY) -> None:
        """Column i of the operator blocks from column i of Y."""
        self._apply(Y[i], AY[i])

    def _next_column(self, i: int, res, Y, AY) -> None:
        """Column i of the next block from the inner solve `res` of column i of R, and its operator blocks."""
        torch.add(self.buf["X"][i], res.x, out=Y[i])
        self._apply_column(i, Y, AY)

    def _eigenvalues(self) -> torch.Tensor:
        """(B, k) returned eigenvalues from the Ritz values of the last block."""
        return (self.buf["theta"][:self.k, :self.B] - self.es.shift).t().contiguous()

    # -- the iteration --------------------------------------------------------------------------------------------------
    def run(self, coeffs, x0, node_layout: bool):
        """coeffs: what `_setup` assembles from (kappa, or E and rho)."""
        es = self.es
        info = self.Info(inner_tol=float(es.inner_tol), block=self.p, iteration=es.iteration)
        Y = self._start_block(x0, node_layout)
        self._setup(coeffs, Y, info, keep=x0 is not None and self.p == self.k)
        if es.iteration == "lobpcg":
            above, failed = self._iterate_lobpcg(info, Y)
        else:
            above, failed = self._iterate_subspace(info, Y)
        return self._finish(info, above, failed, node_layout)

    def _iterate_subspace(self, info, Y) -> Tuple[int, int]:
        """Block inverse iteration: Rayleigh-Ritz on Y = X + D alone.  -> the last `_status()`."""
        es, L = self.es, self.L
        p, n, Bp = self.p, self.rows, self.Bp
        nblk = L.diffhe_eig_gram_blocks(n, Bp)
        nq = p * (p + 1) // 2
        self.buf = dict(X=self._new(p, n, Bp), AX=self._new(p, n, Bp), R=self._new(p, n, Bp), GA=self._new(nq, Bp),
                        GM=self._new(nq, Bp), part=self._new(nblk * 2 * nq * Bp), work=self._new(2 * p * p * Bp),
                        C=self._new(p, p, Bp), theta=self._new(p, Bp), rho=self._new(p, Bp),
                        flag=self._new(Bp, dtype=torch.int32))
        b = self.buf
        AY = self._new(p, n, Bp)
        for i in range(p):
            self._apply_column(i, Y, AY)
        self._rayleigh_ritz(Y, AY)
        above, failed = self._status()
        while above and info.outer_iterations < es.max_iter:
            info.outer_iterations += 1
            for i in range(p):
                res = self._inner_solve(b["R"][i])
                info.inner_solves += 1
                info.inner_iterations += res.iterations
                info.inner_not_converged += res.not_converged
                self._next_column(i, res, Y, AY)
            self._rayleigh_ritz(Y, AY)
            above, failed = self._status()
        return above, failed

    # -- LOBPCG: Ritz on span{X, W, P} ("LOBPCG") -----------------------------------------------------------
    # A subclass supplies `_lobpcg_apply` (columns j of A S and B S from column j of S) and the free-row mask; the defaults
    # below are those of the mass-weighted pencils, (A, M) with M diagonal: `_times_mass` and `_residual_norms`.
    refresh = LOBPCG_REFRESH

    def _lobpcg_apply(self, blk, j: int) -> None:
        self._apply(blk["S"][j], blk["AS"][j])
        self._times_mass(blk["S"][j], blk["BS"][j])

    def _lobpcg_column(self, i: int, res, blk) -> None:
        """w_i = the inner solve of column i of R into the W slot, with its operator columns."""
        j = self.p + i
        blk["S"][j].copy_(res.x)
        self._lobpcg_apply(blk, j)

    def _lobpcg_pre(self) -> None:
        """Before the Ritz step of an outer iteration (what measures the block that is about to be replaced)."""

    def _lobpcg_post(self) -> None:
        """After the rotation: the stopping measure of the new block from R and theta."""
        self._residual_norms()

    def _lobpcg_ritz(self, cur, nxt, q: int) -> None:
        """Gram -> Ritz -> rotate on the leading q columns of `cur` into `nxt`: X', P', R' = A X' - theta B X', theta."""
        L, p, n, Bp, B, st = self.L, self.p, self.rows, self.Bp, self.B, _stream(self.plan.device)
        b = self.buf
        self._lobpcg_pre()
        L.diffhe_lobpcg_gram(cur["S"], cur["AS"], cur["BS"], self._free_mask(), q, n, Bp, b["part"], b["GA"], b["GM"], st)
        L.diffhe_lobpcg_ritz(b["GA"], b["GM"], q, p, Bp, JACOBI_SWEEPS, b["C"], b["theta"], b["used"], b["flag"], st)
        L.diffhe_lobpcg_rotate(cur["S"], cur["AS"], cur["BS"], b["C"], b["theta"], q, p, n, Bp, nxt["S"], nxt["AS"],
                               nxt["BS"], b["R"], st)
        b["drops"] += ((b["used"][:B] < q) & (b["flag"][:B] == 0)).sum()
        b["used"].masked_fill_(b["used"] == q, 0)      # what stays marks the samples that fell back: they keep to [X | W]
        b["X"] = nxt["S"][:p]
        self._lobpcg_post()

    def _iterate_lobpcg(self, info, Y) -> Tuple[int, int]:
        """The basis [X | W | P] as one (3p, rows, Bp) buffer next to A S and B S, in a ping-pong pair.  -> the last
        `_status()`."""
        es, L = self.es, self.L
        p, n, Bp = self.p, self.rows, self.Bp
        q3 = 3 * p
        nq = q3 * (q3 + 1) // 2
        part = max(L.diffhe_lobpcg_gram_blocks(n, Bp) * 2 * nq, L.diffhe_eig_gram_blocks(n, Bp) * 2 * p) * Bp
        self.buf = b = dict(R=self._new(p, n, Bp), GA=self._new(nq, Bp), GM=self._new(nq, Bp), part=self._new(part),
                            C=self._new(q3, p, Bp), theta=self._new(p, Bp), rho=self._new(p, Bp),
                            flag=self._new(Bp, dtype=torch.int32),
                            used=torch.zeros(Bp, dtype=torch.int32, device=self.plan.device),
                            drops=torch.zeros((), dtype=torch.int64, device=self.plan.device))
        cur, nxt = (dict(S=self._new(q3, n, Bp), AS=self._new(q3, n, Bp), BS=self._new(q3, n, Bp)) for _ in range(2))
        cur["S"][:p] = Y
        for j in range(p):
            self._lobpcg_apply(cur, j)
        self._lobpcg_ritz(cur, nxt, p)          # Ritz on the start block alone
        cur, nxt = nxt, cur
        above, failed = self._status()
        q = 2 * p                               # no P yet: the first iteration (cold or warm) runs on [X | W]
        while above and info.outer_iterations < es.max_iter:
            info.outer_iterations += 1
            for i in range(p):
                res = self._inner_solve(b["R"][i])
                info.inner_solves += 1
                info.inner_iterations += res.iterations
                info.inner_not_converged += res.not_converged
                self._lobpcg_column(i, res, cur)
            if info.outer_iterations % self.refresh == 0:       # drift control: A X and B X afresh, not rotated
                for j in range(p):
                    self._lobpcg_apply(cur, j)
                if info.outer_iterations <= LOBPCG_RETRIES * self.refresh:
                    b["used"].zero_()                           # ... and a sample that gave up P may try it again
            self._lobpcg_ritz(cur, nxt, q)
            cur, nxt = nxt, cur
            q = q3
            above, failed = self._status()
        info.basis_drops = int(b["drops"])
        b["X"] = b["X"].clone()                 # the p columns alone outlive the run, not the basis they sit in
        return above, failed

    def _finish(self, info, above: int, failed: int, node_layout: bool):
        """Sign rule, `last_info`, the warnings and the returned layout, from the buffers either iteration leaves."""
        es, plan, L, b = self.es, self.plan, self.L, self.buf
        k, n, B, Bp = self.k, self.rows, self.B, self.Bp
        sgn = self._new(k, Bp)
        self._fix_sign(b["X"], sgn)
        info.not_converged, info.gram_failures = above, failed
        info.residual = b["rho"][:k, :B].t().cpu()
        es.last_info = info
        if failed:
            warnings.warn(f"diffhe: the Gram matrix of {failed} of {B} samples was not positive definite in the last Ritz "
                          "step (linearly dependent or non-finite block); their eigenpairs are not valid", RuntimeWarning)
        if above:
            warnings.warn(f"diffhe: {above} of {B * k} eigenpairs did not reach tol={es.tol:g} in {es.max_iter} outer "
                          f"iterations (max relative residual {float(info.residual.max()):.2e}, path {info.path})",
                          RuntimeWarning)
        lam = self._eigenvalues()                                              # (B, k)
        self.X = b["X"][:k]
        if node_layout:
            phi = (self.X if Bp == B else self.X[:, :, :B]).reshape(k, *self.vec, B)
        else:
            phi = self._new(B, k, n)
            for i in range(k):      # column i of every sample into phi[:, i, :]: one transposing pass per column
                L.diffhe_to_sample_major(self.X[i], None, phi[:, i], k * n, n, B, Bp, _stream(plan.device))
            phi = phi.reshape(B, k, *self.vec)
            if not self.batched:
                phi = phi[0]
        if not self.batched:
            lam = lam[0]
        self._release()
        self.buf = None
        return lam, phi


class _EigenRun(_BlockRun):
    """One eigen call: the inner solver's path state (assembled operators, hierarchy) plus the block buffers.  After
    `run()` it keeps what the Hellmann-Feynman backward reads -- the k returned columns and the call's facts."""

    def __init__(self, es: "EigenFESolver", kappa: torch.Tensor, batch: Optional[int]):
        inner = es.inner
        if inner._tensor_components():
            raise NotImplementedError("diffhe: eigenpairs with a conductivity tensor are not implemented")
        self.es, self.plan = es, inner._plan()
        plan = self.plan
        self.mode, self.B, self.batched = _eigen_layout(kappa, plan.m, batch)
        self.Bp = padded_batch(self.B)
        self.k, self.p = es.k, es.k + es.guard
        self.rows, self.vec = plan.n, (plan.n,)
        if self.p > plan.n - plan.n_bc:
            raise ValueError(f"block of {self.p} vectors on a mesh with {plan.n - plan.n_bc} free nodes")
        self.kappa_shape, self.kappa_device = kappa.shape, kappa.device
        self.L = _hip.lib()
        self.mass = plan.lumped_mass()
        self.state = None
        self.X = None

    # -- the problem: K(kappa) against the plan's lumped mass -------------------------------------------------------------
    def _bc_rows(self):
        return self.plan.bc_index() if self.plan.n_bc else None

    def _setup(self, kappa: torch.Tensor, Y: torch.Tensor, info: EigenInfo, keep: bool = False) -> None:
        """Assemble once and build (or reuse) the hierarchy once: the inner solver's path object solves the LAST column,
        A y = M y_{p-1} to `inner_tol` -- one step of inverse iteration on a guard column, not wasted -- and keeps the
        operators every later solve and every application of A reads.  keep: leave the column as it is (a warm start
        without guard columns: a solve to `inner_tol` would throw its accuracy away)."""
        inner, plan, B, n = self.es.inner, self.plan, self.B, self.plan.n
        f0 = torch.zeros((B, n), dtype=torch.float64, device=plan.device)
        load0 = (self.mass[:, None] * Y[-1])[:, :B].t().contiguous()
        call = _Call.of(inner, plan, kappa, f0, load0, False)
        state = _begin_call(inner, plan, call, homogeneous=True)
        sinfo = SolveInfo()
        state.forward(call, sinfo)               # no warning per inner solve: `run` reports what the iteration missed
        inner.last_info = sinfo
        if not keep:
            Y[-1][:, :B] = state.x[:, :B]
        self.state, self.lattice = state, isinstance(state, _LatticeSolve)
        if self.lattice:
            eng = state.eng
            shift = state.shift[:1] if state.shift is not None else None
            self._lev = eng.lattice_levels(state.vals[:1], shift=shift)
            self._apart = self._new(self.L.diffhe_lattice_blocks(n, self.Bp) * self.Bp)
        else:
            self._apart = self._new(self.L.diffhe_grad_kappa_blocks(n, self.Bp) * self.Bp)
            self._kscale = None if state.inv_kappa is None else (1.0 / state.inv_kappa)
        info.inner, info.path = sinfo, sinfo.path
        info.inner_solves, info.inner_iterations = 1, int(sinfo.iterations)
        info.inner_not_converged = int(sinfo.not_converged)
        self._scratch = SolveInfo()

    def _apply(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """y = A x with the saved operator (identity on the Dirichlet rows, where x is 0)."""
        state, plan, L, st = self.state, self.plan, self.L, _stream(self.plan.device)
        if self.lattice:
            L.diffhe_lattice_apply(self._lev, state.Bv, state.scale, x, y, self._apart, self.Bp, st)
            return
        L.diffhe_ell_apply(state.vals, plan.cols, x, y, self._apart, plan.n, plan.W, self.Bp, state.Bv, st)
        if self._kscale is not None:             # factored general path: A_b = kappa_b K_1
            y *= self._kscale

    def _inner_solve(self, rhs: torch.Tensor):
        return self.state._adjoint_solve(rhs, self._scratch)

    def _rayleigh_ritz(self, Y, AY) -> None:
        """Gram -> Ritz -> rotate -> residual: X, AX, R = theta M X - A X, theta, rho from the block Y and A Y."""
        L, plan, p, n, Bp, st = self.L, self.plan, self.p, self.plan.n, self.Bp, _stream(self.plan.device)
        b = self.buf
        L.diffhe_eig_gram(Y, AY, self.mass, plan.is_bc, p, n, Bp, b["part"], b["GA"], b["GM"], st)
        L.diffhe_eig_ritz(b["GA"], b["GM"], p, Bp, JACOBI_SWEEPS, b["work"], b["C"], b["theta"], b["flag"], st)
        L.diffhe_eig_rotate(Y, AY, b["C"], b["theta"], self.mass, p, n, Bp, b["X"], b["AX"], None, b["R"], st)
        L.diffhe_eig_residual(b["R"], b["theta"], self.mass, p, n, Bp, b["part"], b["rho"], st)

    def _fix_sign(self, X, sgn) -> None:
        self.L.diffhe_eig_fix_sign(X, self.mass, self.k, self.plan.n, self.Bp, self.buf["part"], sgn,
                                   _stream(self.plan.device))

    # -- what LOBPCG asks of the problem ------------------------------------------------------------------------------------
    def _free_mask(self):
        return self.plan.is_bc

    def _times_mass(self, x: torch.Tensor, y: torch.Tensor) -> None:
        torch.mul(x, self.mass[:, None], out=y)

    def _residual_norms(self) -> None:
        b = self.buf
        self.L.diffhe_eig_residual(b["R"], b["theta"], self.mass, self.p, self.plan.n, self.Bp, b["part"], b["rho"],
                                   _stream(self.plan.device))

    def _release(self) -> None:
        # what backward needs: the k columns and the engine (element tables, zero Dirichlet data); nothing else stays
        self.eng = self.state.eng
        self.state = self._lev = self._apart = self._scratch = None

    def backward(self, glam: torch.Tensor) -> torch.Tensor:
        """dL/dkappa = sum_i lambda_bar_{b,i} phi_{b,i}^T k0_e phi_{b,i} in the shape of kappa, by the solve's gradient
        kernels (which compute -lam^T k0 u) with u = phi_i and lam = -lambda_bar_i phi_i."""
        plan, eng, B, Bp, k, mode = self.plan, self.eng, self.B, self.Bp, self.k, self.mode
        g = glam.detach().to(plan.device, torch.float64).reshape(B, k)
        gp = torch.zeros((k, Bp), dtype=torch.float64, device=plan.device)
        gp[:, :B] = g.t()
        acc = None
        for i in range(k):
            lamv = self.X[i] * (-gp[i])[None, :]
            sums, elem = eng.grad_kappa(lamv, self.X[i], B, Bp, mode, True)     # (B,) | (m,) | element-major (m, B)
            part = elem if sums is None else sums
            acc = part if acc is None else acc + part
        if mode == K_SAMPLE_ELEM:
            grad = _kappa_grad(mode, self.kappa_shape, None, acc.t().contiguous())
        elif mode == K_ELEM:
            grad = _kappa_grad(mode, self.kappa_shape, None, acc)
        else:
            grad = _kappa_grad(mode, self.kappa_shape, acc, None)
        return grad.to(self.kappa_device)


# ---------------------------------------------------------------------------------------------
# torch.library custom ops diffhe::eig_solve / diffhe::eig_solve_backward: the solver and the state of the call travel as
# integer handles through the registries of diffhe.solver.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("diffhe::eig_solve", mutates_args=())
def eig_solve(kappa: torch.Tensor, x0: Optional[torch.Tensor], handle: int, batch: int, node_layout: bool,
              save: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(lam, phi, token) of the `EigenFESolver` registered under `handle`; batch < 1: none given; `token` names the saved
    state of the call (0 when `save` is false)."""
    es = _SOLVERS[handle]
    run = _EigenRun(es, kappa, batch if batch >= 1 else None)
    lam, phi = run.run(kappa, x0, node_layout)
    # fresh tensors (an op's outputs may not alias one another); with layout="node" phi is the block itself
    return lam.to(kappa.device), phi.to(kappa.device), _register_state(run, save)


@eig_solve.register_fake
def _eig_solve_fake(kappa, x0, handle, batch, node_layout, save):
    es = _SOLVERS[handle]
    n, m, k = es.mesh.n_nodes, es.mesh.n_elements, es.k
    _, B, batched = _eigen_layout(kappa, m, batch if batch >= 1 else None)
    lam = kappa.new_empty((B, k) if batched else (k,), dtype=torch.float64)
    if node_layout:
        phi = kappa.new_empty((k, n, B), dtype=torch.float64)
    else:
        phi = kappa.new_empty((B, k, n) if batched else (k, n), dtype=torch.float64)
    return lam, phi, torch.empty((), dtype=torch.int64)


@torch.library.custom_op("diffhe::eig_solve_backward", mutates_args=())
def eig_solve_backward(glam: torch.Tensor, token: torch.Tensor, kappa_like: torch.Tensor) -> torch.Tensor:
    """dL/dkappa of the call named by `token` from the cotangent of lam; no solve."""
    return _state_of(token).backward(glam).to(kappa_like.device, kappa_like.dtype)


@eig_solve_backward.register_fake
def _eig_solve_backward_fake(glam, token, kappa_like):
    return torch.empty_like(kappa_like)


def _setup_context(ctx, inputs, output):
    """Save (token, kappa) and tie the saved state of the call to them.  phi (and the token) are marked
    non-differentiable."""
    lam, phi, token = output
    ctx.mark_non_differentiable(phi, token)
    _tie_state(ctx, token, inputs[0])


def _backward(ctx, glam, _gphi, _gtoken):
    if torch.is_grad_enabled():
        raise NotImplementedError("diffhe: second-order derivatives of eigenvalues are not implemented (backward with "
                                  "create_graph=True, diffhe.eigen)")
    token, kappa = ctx.saved_tensors[:2]
    grad = torch.ops.diffhe.eig_solve_backward(glam, token, kappa) if ctx.needs_input_grad[0] else None
    return grad, None, None, None, None, None


torch.library.register_autograd("diffhe::eig_solve", _backward, setup_context=_setup_context)


class EigenFESolver(nn.Module):
    """The k smallest eigenpairs of K(kappa) phi = lambda M_L phi per sample, `lam` differentiable with respect to kappa
    (see the module docstring for the problem, the layouts, the gradient and its limits on degenerate clusters; phi is
    returned non-differentiable).

    Parameters
    ----------
    mesh : FEMesh -- P1 triangles (lattice or general path) or P1 tetrahedra; the VALUES of `mesh.dirichlet_nodes` are
        ignored, the boundary conditions are homogeneous.
    kappa : float or tensor or Parameter -- (), (m,), (B,) / (B, 1) or (B, m); may require grad.
    k : number of eigenpairs; guard : extra block columns (block p = k + guard <= 16; the convergence rate of mode i per
        outer iteration is lambda_i / lambda_{p+1}).
    tol : stop when |A x - theta M x|_{M^-1} / theta <= tol for the k columns of every sample; max_iter : outer iterations.
    shift : sigma >= 0, the inner solves run on K + sigma M_L (`reaction=` of the inner solver); required > 0 on a mesh
        without Dirichlet nodes.  The returned lambda exclude it.
    seed : of the CPU generator the start block is drawn from.
    inner_tol : relative residual of the inner correction solves (their right-hand side is the current eigen-residual, so
        the absolute accuracy asked of them tightens as the iteration converges).
    iteration : "subspace" (default), the block inverse iteration with Rayleigh-Ritz on the p new columns alone, or
        "lobpcg", Rayleigh-Ritz on span{X, W, P} with W the same inner solves and P the previous step: fewer outer
        iterations for the same inner solves each ("LOBPCG"); every other option keeps its meaning.
    solver_options : passed to the inner `DifferentiableFESolver` (2D) / `DifferentiableFESolver3D` (3D): device, method,
        mg, amg, operator, assembly, ...
    """

    def __init__(self, mesh, kappa=1.0, k: int = 4, *, guard: int = 4, tol: float = 1e-8, max_iter: int = 200,
                 shift: float = 0.0, seed: int = 0, inner_tol: float = 1e-2, iteration: str = "subspace", **solver_options):
        super().__init__()
        self.iteration = _check_iteration(iteration)
        if mesh.dim == 1:
            raise NotImplementedError("diffhe: eigenpairs on 1D meshes are not implemented (a tridiagonal pencil is "
                                      "dense-eigh territory)")
        if mesh.dim not in (2, 3):
            raise NotImplementedError("Only 2D and 3D meshes supported")
        if mesh.elements.shape[1] != mesh.dim + 1:
            raise NotImplementedError("diffhe: eigenpairs are implemented for P1 elements only (the row-sum lumped mass "
                                      f"of a mesh with {mesh.elements.shape[1]} nodes per element is not positive)")
        k, guard = int(k), int(guard)
        if k < 1 or guard < 0 or k + guard > MAX_BLOCK:
            raise ValueError(f"need 1 <= k and guard >= 0 with k + guard <= {MAX_BLOCK}, got k={k}, guard={guard}")
        if not (float(tol) > 0.0) or not (0.0 < float(inner_tol) < 1.0) or int(max_iter) < 0:
            raise ValueError(f"need tol > 0, 0 < inner_tol < 1, max_iter >= 0, got {tol!r}, {inner_tol!r}, {max_iter!r}")
        if not (float(shift) >= 0.0):
            raise ValueError(f"shift must be >= 0, got {shift!r}")
        if not mesh.dirichlet_nodes and float(shift) == 0.0:
            raise ValueError("diffhe: a mesh without Dirichlet nodes needs shift > 0 (K alone is singular there)")
        for name in ("reaction", "warm_start"):
            if name in solver_options:
                raise ValueError(f"{name}= is not an option of EigenFESolver" + (" (use shift=)" if name == "reaction" else ""))
        if isinstance(kappa, torch.Tensor) and (kappa.dim() >= 3 or (kappa.dim() == 2 and kappa.shape[1] in (3, 6)
                                                                      and kappa.shape[1] not in (1, mesh.n_elements))):
            raise NotImplementedError("diffhe: eigenpairs with a conductivity tensor are not implemented (scalar kappa only)")
        self.mesh, self.k, self.guard = mesh, k, guard
        self.tol, self.max_iter, self.shift, self.seed = float(tol), int(max_iter), float(shift), int(seed)
        self.inner_tol = float(inner_tol)
        cls = DifferentiableFESolver if mesh.dim == 2 else DifferentiableFESolver3D
        self.inner = cls(mesh, kappa, tol=self.inner_tol, reaction=self.shift, **solver_options)
        self.last_info = EigenInfo()

    @property
    def kappa(self) -> torch.Tensor:
        return self.inner.kappa

    def forward(self, batch: Optional[int] = None, x0: Optional[torch.Tensor] = None, layout: str = "sample"):
        """-> (lam, phi).  batch: the number of samples, where kappa does not say (or reads both ways); x0: a previous
        phi in the same `layout` as a warm start -- with k columns it is padded with seeded random guard columns, with
        k + guard columns it is the whole start block; layout: "sample" = phi (B, k, n), "node" = phi (k, n, B)."""
        if layout not in ("sample", "node"):
            raise ValueError(f"Unknown layout: {layout!r}")
        kappa = self.inner.kappa
        _eigen_layout(kappa, self.mesh.n_elements, batch)
        _SOLVERS[id(self)] = self
        save = torch.is_grad_enabled() and kappa.requires_grad
        lam, phi, _token = torch.ops.diffhe.eig_solve(kappa, None if x0 is None else x0.detach(), id(self),
                                                      -1 if batch is None else int(batch), layout == "node", save)
        return lam, phi
