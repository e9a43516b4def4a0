"""Differentiable P1-FEM solve of -div(kappa grad u) = f with Dirichlet data, on MI355X.

Mirror of the reference operator `DifferentiableFESolver` (reference
diffhe/solver.py:21-183): same constructor, `.kappa`, `forward(f) -> u`, same
unbatched semantics (float64 output, Dirichlet values exact, gradients to kappa
and f).  The work is done by hand-written HIP kernels behind the C ABI of
include/diffhe_hip.h; the adjoint is explicit, not autograd
replay.  There is no CPU fallback: without the HIP library or a GPU, `forward`
raises.

Extensions over the reference (which has no batch dimension, solver.py:54):
  f      (n,) | (n,1) | (B,n)
  kappa  python scalar | 0-dim / 1-element tensor | (m,) per element |
         (B,1) or (B,) per sample | (B,m) per sample and element
"""
from __future__ import annotations

import ctypes
import itertools
import math
import os
import threading
import warnings
import weakref
from dataclasses import dataclass, replace
from typing import Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import _hip
from .mesh import FEMesh
from .plan import SolvePlan, get_plan, padded_batch, status_buffer, _stream

# kappa layouts
K_SCALAR, K_SAMPLE, K_ELEM, K_SAMPLE_ELEM = 0, 1, 2, 3


@dataclass
class SolveInfo:
    """Diagnostics of the last solve (the reference silently returns garbage on
    failure; we surface it instead)."""
    path: str = ""
    iterations: int = 0
    not_converged: int = 0
    max_relres: float = 0.0
    adj_iterations: int = 0
    adj_max_relres: float = 0.0
    err_est: float = 0.0        # lattice path: max over samples of the estimated relative energy-norm error
    adj_err_est: float = 0.0
    # lattice path: how many samples each rule stopped, forward / adjoint: {"residual": ., "energy": ., "cap": .}
    # ("cap" = neither rule fired before the iteration cap; the direct dense path iterates nothing and reports {})
    stop_rules: Optional[dict] = None
    adj_stop_rules: Optional[dict] = None
    # lattice path, residual carried as a pair of fp32 vectors: how many of the solve's residual updates wrote no low
    # half (one that still read it, then hi alone); 0 where the pair is kept whole or not carried at all
    resid_single_updates: int = 0
    adj_resid_single_updates: int = 0
    tol_energy: float = 0.0     # the energy-norm tolerance in force for this call (0: residual rule alone)
    # lattice path, fp32-stored V-cycle: where its coefficients come from -- "shared-fp32" (batch-shared matrix, scalar
    # loads), "fp16-rowsum" (per-sample matrices: fp32 diagonal + scaled fp16 couplings), "fp32" (per-sample plain fp32
    # copies: asked for, or the fallback when a sample's couplings span more than fp16 holds), "fp64" (no copies)
    coeff_storage: str = ""
    factored: bool = False      # one scalar kappa per sample (or for all) kept as K_b = kappa_b K_1: ONE unit matrix for the batch
    flags: int = 0              # lattice path: the `flags` word handed to diffhe_lattice_pcg_solve (DIFFHE_PCG_* in include/diffhe_hip.h)
    precision: str = ""         # what is stored / computed in which precision in THIS solve, derived from those flags
    # general path with a multigrid preconditioner: "unit" (hierarchy of the unit-kappa operator, plan-cached) or "operator"
    # (amg=dict(strength=theta): built from the operator that was being solved, kept on the solver); its levels, the fine
    # one included; its operator complexity sum_l nnz_l / nnz_0; the calls since it was built (0: built by this call)
    hierarchy: str = ""
    hierarchy_levels: int = 0
    operator_complexity: float = 0.0
    hierarchy_age: int = 0


def _resolve_device(device) -> torch.device:
    if device is not None:
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("diffhe runs on a ROCm GPU only (no CPU fallback)")
        return device
    if not torch.cuda.is_available():
        raise RuntimeError("diffhe: no ROCm GPU visible -- the HIP solve path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _kappa_mode(kappa: torch.Tensor, m: int, B: Optional[int]):
    """Classify kappa -> (mode, B implied or None)."""
    if kappa.numel() == 1:
        return K_SCALAR, None
    if kappa.dim() == 1:
        if kappa.shape[0] == m and (B is None or B == 1 or B != m):
            return K_ELEM, None
        return K_SAMPLE, kappa.shape[0]
    if kappa.dim() == 2:
        if kappa.shape[1] == 1:
            return K_SAMPLE, kappa.shape[0]
        if kappa.shape[1] == m:
            return K_SAMPLE_ELEM, kappa.shape[0]
    raise ValueError(f"kappa shape {tuple(kappa.shape)} not understood for a mesh with {m} elements")


def _tensor_mode(kappa: torch.Tensor, nc: int, m: int, B: Optional[int], node_major: bool = False):
    """Classify a conductivity TENSOR in Voigt components (diffhe.aniso; nc = 3 in 2D, 6 in 3D) -> (mode, B implied or
    None, element-major).  (nc,) one tensor for mesh and batch; (m, nc) a field shared by the batch; (B, nc) one tensor
    per sample; (B, m, nc) a field per sample -- with layout='node' also (nc, m, B), batch innermost (a shape that reads
    both ways is read that way, as a square scalar field is).  (X, nc) with X == m is the element field, as a scalar
    (m,) kappa is in `_kappa_mode` -- also when m happens to equal the batch B, UNLESS that batch comes with f: then,
    exactly as there, B == m reads as one tensor per sample."""
    shape = tuple(kappa.shape)
    if shape == (nc,):
        return K_SCALAR, None, False
    if kappa.dim() == 2 and shape[1] == nc:
        if shape[0] == m and (B is None or B == 1 or B != m):
            return K_ELEM, None, False
        return K_SAMPLE, shape[0], False
    if kappa.dim() == 3:
        if node_major and B is not None and shape == (nc, m, B):
            return K_SAMPLE_ELEM, B, True
        if shape[1:] == (m, nc):
            return K_SAMPLE_ELEM, shape[0], False
    raise ValueError(f"conductivity tensor shape {shape} not understood for a mesh with {m} elements: expected "
                     f"({nc},), ({m}, {nc}), (B, {nc}) or (B, {m}, {nc}) in Voigt components"
                     + (f", or ({nc}, {m}, B) with layout='node'" if node_major else ""))


class _Solved(NamedTuple):
    """What one iterative solve of `_Engine` hands back."""
    x: torch.Tensor                         # (n, Bp)
    iterations: int
    not_converged: int                      # samples that missed the tolerance
    relres: torch.Tensor                    # (Bp,) true relative residual per sample
    est: Optional[torch.Tensor] = None      # lattice path: (Bp,) estimated relative energy-norm error
    rule: Optional[torch.Tensor] = None     # lattice path: (Bp,) int32, the rule that stopped each sample
    flags: int = 0                          # lattice path: the `flags` word handed to diffhe_lattice_pcg_solve
    single_updates: int = 0                 # lattice path: residual updates that wrote no low half (status word 3)


class _Engine:
    """Thin, stateless driver of the C ABI for one plan and one batch geometry: nothing is assigned after construction.
    ref_order: per-sample lattice matrices in the reference's exact operation order (operator="assembled").
    g: the (n,) Dirichlet data the kernels read -- the plan's (None), or zeros when the data comes per call."""

    def __init__(self, plan: SolvePlan, tol: float, max_iter: int, check_every: int, assembly: str, *,
                 ref_order: bool = False, g: Optional[torch.Tensor] = None):
        self.p = plan
        self.tol, self.max_iter, self.check_every, self.assembly = tol, max_iter, check_every, assembly
        self.ref_order = ref_order
        self.g = plan.g if g is None else g
        self.L = _hip.lib()

    # -- layout helpers -----------------------------------------------------------------
    def to_node_major(self, src, B, Bp, n, zero_mask=None):
        """(B, n) rows -- or one (n,) vector broadcast to all B samples -- to (n, Bp)."""
        p = self.p
        dst = torch.empty((n, Bp), dtype=torch.float64, device=p.device)
        ld = 0 if src.dim() == 1 else src.stride(0)
        self.L.diffhe_to_node_major(src, ld, zero_mask, dst, n, B, Bp, _stream(p.device))
        return dst

    def to_sample_major(self, src, B, Bp, n, add=None):
        p = self.p
        dst = torch.empty((B, n), dtype=torch.float64, device=p.device)
        self.L.diffhe_to_sample_major(src, add, dst, n, n, B, Bp, _stream(p.device))
        return dst

    def kappa_device(self, kappa, mode, B, Bp, em=False):
        """-> (tensor, stride_e, stride_b, Bv) in the layout the kernels index.  Per-sample fields are (m, Bp), padding
        samples = 1: from the API's (B, m) by one transposing pass, or from an element-major (m, B) tensor
        (layout='node'), used as it is when B needs no padding."""
        p = self.p
        k = kappa.detach().to(p.device, torch.float64)
        if mode == K_SCALAR:
            return k.reshape(1).contiguous(), 0, 0, 1
        if mode == K_ELEM:
            return k.reshape(p.m).contiguous(), 1, 0, 1
        if mode == K_SAMPLE:
            kp = torch.ones(Bp, dtype=torch.float64, device=p.device)
            kp[:B] = k.reshape(B)
            return kp, 0, 1, Bp
        if em and Bp == B and k.is_contiguous():
            return k, Bp, 1, Bp
        if em:
            kp = torch.ones((p.m, Bp), dtype=torch.float64, device=p.device)
            kp[:, :B] = k
        else:
            kp = self.to_node_major(k.reshape(B, p.m).contiguous(), B, Bp, p.m)
            if Bp > B:
                kp[:, B:] = 1.0
        return kp, Bp, 1, Bp

    def assemble(self, kdev, kse, ksb, Bv):
        p, L = self.p, self.L
        st = _stream(p.device)
        vals = torch.empty((p.W, p.n, Bv), dtype=torch.float64, device=p.device)
        lift = torch.empty((p.n, Bv), dtype=torch.float64, device=p.device)
        if p.is_p2:
            # quadratic triangles (ours; no reference operator to be bit-identical with): kappa * k0, gathered
            L.diffhe_ell_assemble_rows(p.k0, kdev, kse, ksb, p.ent_ptr, p.contrib, p.cols, None, p.is_bc, self.g, vals,
                                       lift, p.n, p.m, p.W, Bv, st)
        elif self.assembly == "atomic" and Bv > 1:
            vals.zero_()
            L.diffhe_ell_assemble_atomic(p.coords, p.elems, p.dim, kdev, kse, ksb, p.slot_of, vals, p.n, p.m, p.W, Bv,
                                         st)
            lift.zero_()  # apply_dirichlet returns F - lift: feed F = 0, negate
            L.diffhe_ell_apply_dirichlet(p.cols, p.is_bc, self.g, vals, lift, p.n, p.W, Bv, st)
            lift.neg_()
        else:
            # reference operation order: values bit-identical to the reference's K (include/diffhe_hip.h)
            L.diffhe_ell_assemble_rows_ref(p.tnum, p.den, kdev, kse, ksb, p.ent_ptr, p.contrib, p.cols, None, p.is_bc,
                                           self.g, vals, lift, p.n, p.m, p.W, Bv, st)
        return vals, lift

    def tensor_device(self, kappa, mode, B, Bp, nc, em=False):
        """-> (tensor, stride per component, per element, per sample, Bv) as the kernels of csrc/aniso.hip index it.
        Batch-shared tensors are used as they come; per-sample ones go batch-innermost with the padding samples set to
        the identity: (nc, Bp), a field given (nc, m, B) (layout='node') as it is -- padded if B needs it -- and the
        API's (B, m, nc) by the one transposing pass of scalar fields, which leaves it (m, nc, Bp)."""
        p = self.p
        k = kappa.detach().to(p.device, torch.float64)
        d = p.dim
        if mode == K_SCALAR:
            return k.reshape(nc).contiguous(), 1, 0, 0, 1
        if mode == K_ELEM:
            return k.reshape(p.m, nc).contiguous(), 1, nc, 0, 1
        eye = torch.zeros(nc, dtype=torch.float64, device=p.device)
        eye[:d] = 1.0
        if mode == K_SAMPLE:
            kp = eye.reshape(nc, 1).repeat(1, Bp)
            kp[:, :B] = k.reshape(B, nc).t()
            return kp, Bp, 0, 1, Bp
        if em:
            if Bp == B and k.is_contiguous():
                return k, p.m * Bp, Bp, 1, Bp
            kp = eye.reshape(nc, 1, 1).repeat(1, p.m, Bp)
            kp[:, :, :B] = k
            return kp, p.m * Bp, Bp, 1, Bp
        kp = self.to_node_major(k.reshape(B, p.m * nc).contiguous(), B, Bp, p.m * nc)      # (m, nc, Bp)
        if Bp > B:
            kp.view(p.m, nc, Bp)[:, :, B:] = eye.reshape(1, nc, 1)
        return kp, Bp, nc * Bp, 1, Bp

    def assemble_tensor(self, kdev, ksc, kse, ksb, Bv):
        """vals (W, n, Bv), lift (n, Bv) of K_e[p,q] = |e| grad phi_p^T K_e grad phi_q (csrc/aniso.hip)."""
        p = self.p
        gtab, vol = p.gradient_table()
        vals = torch.empty((p.W, p.n, Bv), dtype=torch.float64, device=p.device)
        lift = torch.empty((p.n, Bv), dtype=torch.float64, device=p.device)
        self.L.diffhe_aniso_assemble_rows(gtab, vol, p.dim, kdev, ksc, kse, ksb, p.ent_ptr, p.contrib, p.cols, p.is_bc,
                                          self.g, vals, lift, p.n, p.m, p.W, Bv, _stream(p.device))
        return vals, lift

    def element_grad(self, mode, em, B, Bp, nc, per_sample, shared):
        """The one dispatch of the coefficient gradients (csrc/element_grad.h) -> (per-sample sums, per-element gradient),
        one of the two None.  A field the batch shares (K_ELEM): summed over the batch inside the kernel, (m,).  One
        field per sample (K_SAMPLE_ELEM): per element and sample, left element-major (m, B) for `em`, else transposed
        back to (B, m).  Otherwise the sums over the elements per sample in two stages, (B,).
        nc: None, or the components per element of a tensor: (m, nc), (nc, m, B) or (B, m * nc), (nc, B).
        per_sample(dk_e, osc, ose, part, dk_sum) and shared(dk, osc, ose) launch the family's two entries."""
        p = self.p
        m, w = p.m, nc or 1
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=p.device)  # noqa: E731
        lead = (nc,) if nc else ()
        if mode == K_ELEM:
            dk = new(m, *lead)
            shared(dk, 1, w)
            return None, dk
        if mode != K_SAMPLE_ELEM:
            part, dk_sum = new(self.L.diffhe_grad_kappa_blocks(m, Bp), w, Bp), new(*lead, Bp)
            per_sample(None, 0, 0, part, dk_sum)
            return dk_sum[..., :B], None
        if em:
            dk_e = new(*lead, m, Bp)
            per_sample(dk_e, m * Bp, Bp, None, None)
            return None, dk_e if Bp == B else dk_e[..., :B]
        dk_e = new(m * w, Bp)
        per_sample(dk_e, Bp, w * Bp, None, None)
        return None, self.to_sample_major(dk_e, B, Bp, m * w)

    def grad_tensor(self, lam, x, B, Bp, nc, mode, em):
        """dL/dK = -|e| sym(grad lambda (x) grad u) in the shape of the caller's tensor: per element and sample, summed
        over the batch inside the kernel (a shared field), or summed over the elements per sample in two stages (one
        tensor per sample; the tensor of the whole batch is the sum of those)."""
        p, L = self.p, self.L
        gtab, vol = p.gradient_table()
        args, st = (p.elems, gtab, vol, p.dim, lam, x, self.g, p.n, p.m), _stream(p.device)
        dk_sum, dk_e = self.element_grad(
            mode, em, B, Bp, nc,
            lambda dk_e, osc, ose, part, dk_sum: L.diffhe_aniso_grad(*args, Bp, dk_e, osc, ose, part, dk_sum, st),
            lambda dk, osc, ose: L.diffhe_aniso_grad_shared(*args, B, Bp, dk, osc, ose, st))
        if mode == K_SCALAR:
            return dk_sum.sum(dim=1)
        if mode == K_SAMPLE:
            return dk_sum.t().contiguous()
        return dk_e if mode == K_ELEM or em else dk_e.reshape(B, p.m, nc)

    def reaction_shifts(self, c, n_levels):
        """Per-level (n,) diagonal shifts c * M_L (0 on Dirichlet rows) of a FACTORED lattice operator, cached on the plan."""
        p = self.p
        with p._lock:       # solvers with different c may share the plan (and run on different threads)
            cache = p.__dict__.setdefault("_shift_cache", {})
            if c not in cache:
                while len(cache) >= 4:
                    cache.pop(next(iter(cache)))
                cache[c] = [c * torch.where(lev.is_bc.bool(), torch.zeros_like(lev.lumped_mass()), lev.lumped_mass())
                            for lev in p.levels]
            return cache[c][:n_levels]

    def add_reaction(self, vals, c, lattice):
        """A += c M_L on the free rows (M_L = lumped mass, diagonal): the stored main diagonal is slot 0 of both
        formats.  Lattice: one entry of `vals` per multigrid level, each with its own (re-discretised) lumped mass."""
        p = self.p
        for li, v in enumerate(vals):
            lev = p.levels[li] if lattice else None
            mass = lev.lumped_mass() if lattice else p.lumped_mass()
            is_bc = lev.is_bc if lattice else p.is_bc
            v[0] += (c * torch.where(is_bc.bool(), torch.zeros_like(mass), mass)).unsqueeze(1)

    def load_vector(self, f_nm, lift, Bv, Bp, lift_scale=None, lattice=False, free_rows=True):
        """F = M f - lift_scale * lift on the free rows, 0 on Dirichlet rows; free_rows=False: M f on every row (with
        lift None: dL/df = M^T lambda, M symmetric)."""
        p = self.p
        F = torch.empty((p.n, Bp), dtype=torch.float64, device=p.device)
        is_bc = p.is_bc if free_rows else None
        if lattice:   # load matrix stored as symmetric diagonals of level 0: no ELL pattern needed
            lev = p.levels[0]
            self.L.diffhe_lattice_apply_shared(lev.nx, lev.ny, 4, lev.Mvals, f_nm, lift, Bv, lift_scale, is_bc, F, Bp,
                                               _stream(p.device))
            return F
        self.L.diffhe_ell_spmv_shared(p.Mvals, p.Mcols, f_nm, lift, Bv, lift_scale, is_bc, F, p.n, p.MW, Bp,
                                      _stream(p.device))
        return F

    def _solve(self, Bp, launch, x=None, **lattice) -> _Solved:
        """The part the three iterative solves share: x (n, Bp) unless the caller brings a start, the per-sample outputs,
        `launch(x, relres, iters, status)`, then the counts the entry left in this thread's pinned status buffer."""
        p = self.p
        if x is None:
            x = torch.empty((p.n, Bp), dtype=torch.float64, device=p.device)
        relres = torch.empty(Bp, dtype=torch.float64, device=p.device)
        iters = torch.empty(Bp, dtype=torch.int32, device=p.device)
        st = status_buffer()
        launch(x, relres, iters, st)
        if lattice:
            lattice["single_updates"] = int(st[3])
        return _Solved(x, int(st[0]), int(st[1]), relres, **lattice)

    def cg(self, vals, rhs, Bp, Bv) -> _Solved:
        p, L = self.p, self.L
        work = torch.empty(L.diffhe_cg_workspace_doubles(p.n, Bp), dtype=torch.float64, device=p.device)
        return self._solve(Bp, lambda x, relres, iters, st: L.diffhe_ell_cg_solve(
            vals, p.cols, rhs, x, p.n, p.W, Bp, Bv, self.tol, self.max_iter, self.check_every, work, relres, iters, st,
            _stream(p.device)))

    # -- lattice path -----------------------------------------------------------------------
    def lattice_assemble(self, kappa, mode, B, Bp, factor=True, n_levels=None, em=False):
        """Per-level symmetric-diagonal operators.  -> (vals per level, Bv, scale, lift, lift_scale).

        One scalar kappa per sample is kept factored, K_b = kappa_b * K_1 (solver.py:88,139 are
        linear in kappa): ONE unit matrix per level is assembled for the whole batch and the
        kernels scale the free rows by kappa_b.  factor=False assembles one matrix per sample
        instead (entries sum_e kappa_b k0_e, rounded like the reference's): kappa_b (K_1 x) differs from
        that in the last bit of every entry, which ill-conditioned systems amplify by their condition number."""
        p, L = self.p, self.L
        st = _stream(p.device)
        scale = None
        if factor and mode in (K_SCALAR, K_SAMPLE):     # no kappa in the matrices: one scale per sample (or for all)
            k = kappa.detach().to(p.device, torch.float64)
            kl, kse, ksb, Bv = None, 0, 0, 1
            if mode == K_SCALAR:
                scale = k.reshape(1).expand(Bp).contiguous()
            else:
                scale = torch.ones(Bp, dtype=torch.float64, device=p.device)
                scale[:B] = k.reshape(B)
        else:
            kl, kse, ksb, Bv = self.kappa_device(kappa, mode, B, Bp, em)
        vals, lift = [], None
        for li, lev in enumerate(p.levels[:n_levels] if n_levels else p.levels):
            if li > 0 and mode in (K_ELEM, K_SAMPLE_ELEM):   # coarse kappa = mean of the 4 children
                kc = torch.empty((lev.m, Bv), dtype=torch.float64, device=p.device)
                prev = p.levels[li - 1]
                L.diffhe_lattice_restrict_kappa(kl, kc, lev.nx, lev.ny, prev.nx // lev.nx, prev.ny // lev.ny, Bv, st)
                kl = kc
            v = torch.empty((lev.nd, lev.n, Bv), dtype=torch.float64, device=p.device)
            lf = torch.empty((lev.n, Bv), dtype=torch.float64, device=p.device) if li == 0 else None
            if li == 0 and mode == K_SAMPLE_ELEM and p.closed_boundary and not self.ref_order:
                # one kappa FIELD per sample on a lattice closed by Dirichlet data, default: entries
                # sum_e kappa_e * fl(t_e / den_e) with the batch-shared quotients precomputed in the reference's
                # rounding -- ONE rounding away from the reference's fl(fl(kappa_e t_e) / den_e) per contribution (a
                # cond * eps effect in u, like the factored form) instead of twelve IEEE fp64 divisions per node and
                # sample (10.3 -> 3 ms at 1024^2 x 256).  NOT on lattices with Neumann parts (cond ~ 1e7 there: a last-bit
                # difference of the entries shows as 4e-10 in u, which is why per-sample scalars are left unfactored on
                # them, `closed_` in _LatticeSolve.forward) -- they, per-sample SCALARS that are not factored, and
                # operator="assembled" keep the bit-identical order below
                self._lattice_rows(lev, "k0ref", kl, kse, ksb, self.g, v, lf, Bv, st)
            elif li == 0 and kl is not None:   # the operator the solution is defined by: reference operation order
                L.diffhe_ell_assemble_rows_ref(lev.tnum, lev.den, kl, kse, ksb, lev.ent_ptr, lev.contrib, lev.cols,
                                               lev.store_slot, lev.is_bc, self.g, v, lf, lev.n, lev.m, 7, Bv, st)
            else:
                self._lattice_rows(lev, "k0", kl, kse, ksb, self.g if li == 0 else lev.zero_g(), v, lf, Bv, st)
            vals.append(v)
            if li == 0:
                lift = lf
        return vals, Bv, scale, lift, scale

    def _lattice_rows(self, lev, which, kl, kse, ksb, g, v, lf, Bv, st):
        """kappa * k0 gathered into the symmetric diagonals of a lattice level (+ the Dirichlet lift).  The lattice form of
        the gather (contribution lists written into the kernel, each kappa_e read once per node) gives bitwise the values
        of the list-driven kernel (tests/test_robustness.py)."""
        L = self.L
        local = lev.k0 if which == "k0" else lev.k0ref()
        # congruent triangles (bit for bit): one (9, 2) table instead of the (9, m) array -- same values
        small = lev.compact(which)
        L.diffhe_lattice_assemble_rows(small if small is not None else local, 1 if small is not None else 0, kl, kse, ksb,
                                       lev.is_bc, g, v, lf, lev.nx, lev.ny, lev.nd, Bv, st)

    def pack_cycle_coeffs(self, vals, Bv):
        """Per-sample matrices, fp32-stored V-cycle: (fp32 diagonals, fp16 off-diagonals, per-sample scales) per level --
        8 instead of 12 B of coefficients per node and sample (3 diagonals); every row sum of the fp64 matrix is kept.
        The off-diagonals of sample b are stored divided by a power of two >= that sample's largest free-row diagonal of
        the fine level (one reduction pass), so kappa of any magnitude -- and samples of very different magnitudes in
        one batch -- stay inside the fp16 range.  Contrast INSIDE a sample is what fp16 cannot hold: couplings below
        2^-19 of the scale (fewer than 5 bits left; 0 from 2^-25 on, which would leave rows with a vanishing diagonal)
        are reported by the packing kernel and the caller falls back to plain fp32 copies: returns (None, None, None)."""
        p, L = self.p, self.L
        st = _stream(p.device)
        lev0 = (_hip.MgLevel * 1)()
        lev0[0].nx, lev0[0].ny, lev0[0].nd = p.levels[0].nx, p.levels[0].ny, p.levels[0].nd
        lev0[0].vals, lev0[0].is_bc = vals[0].data_ptr(), p.levels[0].is_bc.data_ptr()
        dmax = torch.empty(Bv, dtype=torch.float64, device=p.device)
        L.diffhe_lattice_max_diag(lev0, Bv, dmax, st)
        # power of two >= dmax (exact: frexp); samples without a positive finite diagonal (padding is kappa = 1) get 1
        mant, expo = torch.frexp(dmax)
        scales = torch.ldexp(torch.ones_like(dmax), expo - (mant == 0.5).to(expo.dtype))
        ok = torch.isfinite(dmax) & (dmax > 0)
        scales = torch.where(ok, scales, torch.ones_like(scales)).contiguous()
        flags = torch.zeros(1, dtype=torch.int32, device=p.device)
        d32, o16 = [], []
        for lev, v in zip(p.levels, vals):
            one = (_hip.MgLevel * 1)()
            one[0].nx, one[0].ny, one[0].nd, one[0].vals = lev.nx, lev.ny, lev.nd, v.data_ptr()
            d = torch.empty((lev.n, Bv), dtype=torch.float32, device=p.device)
            o = torch.empty((lev.nd - 1, lev.n, Bv), dtype=torch.float16, device=p.device)
            L.diffhe_lattice_pack_h16(one, Bv, scales, d, o, flags, st)
            d32.append(d)
            o16.append(o)
        if not bool(ok.all()) or int(flags[0]) != 0:
            return None, None, None
        return d32, o16, scales

    def lattice_levels(self, vals, vals32=None, dense=None, shift=None, rdiag32=None, off16=None):
        """Level descriptors for the C ABI.  dense = (level index, inverse tensor): the hierarchy is cut at that
        level, whose solve becomes one dense product (diffhe_mg_level.dense_inv).  shift = per-level (n,) diagonal
        shifts of a factored operator (diffhe_mg_level.shift)."""
        off16, oscales = off16 if off16 is not None else (None, None)
        nl = len(vals) if dense is None else dense[0] + 1
        arr = (_hip.MgLevel * nl)()
        for i, (lev, v) in enumerate(zip(self.p.levels[:nl], vals[:nl])):
            arr[i].nx, arr[i].ny, arr[i].nd, arr[i].reserved = lev.nx, lev.ny, lev.nd, 0
            arr[i].vals, arr[i].is_bc = v.data_ptr(), lev.is_bc.data_ptr()
            arr[i].vals32 = vals32[i].data_ptr() if vals32 is not None and vals32[i] is not None else None
            arr[i].dense_inv = dense[1].data_ptr() if dense is not None and i == nl - 1 else None
            arr[i].shift = shift[i].data_ptr() if shift is not None else None
            arr[i].rdiag32 = rdiag32[i].data_ptr() if rdiag32 is not None and rdiag32[i] is not None else None
            arr[i].offdiag16 = off16[i].data_ptr() if off16 is not None and off16[i] is not None else None
            arr[i].mask32 = lev.mask32().data_ptr() if (arr[i].rdiag32 or arr[i].offdiag16) else None
            arr[i].offdiag_scales = oscales.data_ptr() if arr[i].offdiag16 else None
        return arr

    def lattice_pcg(self, vals, Bv, scale, rhs, Bp, mg, vals32=None, dense=None, x0=None, shift=None, rdiag32=None,
                    off16=None):
        """x0: (n, Bp) initial guess (warm start; left untouched) or None for the cold full-multigrid start."""
        p, L = self.p, self.L
        arr = self.lattice_levels(vals, vals32, dense, shift, rdiag32, off16)
        nl = len(arr)
        warm = x0 is not None and x0.shape == (p.n, Bp)
        work = torch.empty(L.diffhe_lattice_pcg_workspace_doubles(arr, nl, Bp), dtype=torch.float64, device=p.device)
        # per-sweep Jacobi damping: Chebyshev weights for the interval [0.5, 2] of D^-1 A when nu == 2
        omegas = mg.get("omegas") or ([0.56, 1.39] if mg["nu"] == 2 else [mg["omega"]] * mg["nu"])
        om = (ctypes.c_double * len(omegas))(*omegas)
        est = torch.empty(Bp, dtype=torch.float64, device=p.device)
        rule = torch.empty(Bp, dtype=torch.int32, device=p.device)
        closed_step = (p.closed_boundary and p.regular_cells and p.dense_level() is not None
                       and int(mg.get("cg_fp32_steplength", 1)))
        flags = (int(mg.get("fp32", 0)) * _hip.PCG_FP32 | int(mg.get("fmg", 0)) * _hip.PCG_FMG
                 | ((int(mg.get("fmg_cycles", 1)) - 1) << _hip.PCG_FMG_CYCLES_SHIFT)
                 | (0 if int(mg.get("floor", 1)) else _hip.PCG_NO_FLOOR)
                 | (_hip.PCG_WARM if warm else 0)
                 | (0 if int(mg.get("fused", 1)) else _hip.PCG_UNFUSED)
                 | (0 if int(mg.get("dense_mfma", 1)) else _hip.PCG_DENSE_SCALAR)
                 | (0 if int(mg.get("pre4", 1)) else _hip.PCG_PRE2)
                 | (0 if int(mg.get("resid_pair", 1)) else _hip.PCG_RESID_FP64)
                 | (0 if int(mg.get("resid_drop_lo", 1)) else _hip.PCG_RESID_KEEP_LO)
                 | ((int(mg.get("trust_its", 0)) & 15) << _hip.PCG_TRUST_ITS_SHIFT)   # development, tests
                 | (_hip.PCG_SPLIT_START if int(mg.get("split_start", 0)) else 0)    # A/B runs, tests
                 | (_hip.PCG_CLOSED_FP32_STEP if closed_step else 0))
        # a multigrid-preconditioned CG that has not converged in a few hundred iterations never will:
        # bound the loop so a defect surfaces as `not_converged` instead of minutes of GPU time
        return self._solve(Bp, lambda x, relres, iters, st: L.diffhe_lattice_pcg_solve(
            arr, nl, Bv, scale, rhs, x, Bp, self.tol, float(mg.get("tol_energy", 0.0) or 0.0), min(self.max_iter, 500),
            len(omegas), mg["n_coarse"], om, flags, work, relres, est, iters, rule, st, _stream(p.device)),
            x=x0.clone() if warm else None, est=est, rule=rule, flags=flags)

    # -- general path with the aggregation-multigrid preconditioner ---------------------------------
    def amg_setup(self, vals, Bv, fp32=True, levels=None, dense_coarse=False):
        """Per-solve coarse operators (Galerkin sums of the fine values) + the level descriptor array.
        fp32: per-sample matrices also get an fp32 copy of every level's values for the fp32 cycle.
        dense_coarse (batch-shared, plan-cached hierarchies): the last level (<= 128 nodes) gets the inverse of its
        matrix and is solved by one dense product instead of n_coarse Jacobi sweeps."""
        p, L = self.p, self.L
        st = _stream(p.device)
        chain = [dict(n=p.n, W=p.W, vals=vals, cols=p.cols)]
        for lv in (levels if levels is not None else p.amg_levels):
            vc = torch.empty((lv["W"], lv["n"], Bv), dtype=torch.float64, device=p.device)
            L.diffhe_ell_galerkin(chain[-1]["vals"], lv["ent_ptr"], lv["contrib"], lv.get("weights"), vc, lv["n"],
                                  lv["W"], Bv, st)
            chain[-1].update(agg=lv["agg"], agg_ptr=lv["agg_ptr"], agg_members=lv["agg_members"],
                             agg_weights=lv.get("agg_weights"), p_cols=lv.get("p_cols"), p_vals=lv.get("p_vals"))
            if "lam_parent" in lv:
                chain[-1]["lam"] = lv["lam_parent"]
            chain.append(dict(n=lv["n"], W=lv["W"], vals=vc, cols=lv["cols"], lam=lv.get("lam")))
        arr = (_hip.AmgLevel * len(chain))()
        for i, lv in enumerate(chain):
            arr[i].n, arr[i].W = lv["n"], lv["W"]
            arr[i].vals, arr[i].cols = lv["vals"].data_ptr(), lv["cols"].data_ptr()
            if lv.get("lam"):       # the level's own bound of lambda_max(D^-1 A), thousandths rounded up (diffhe_amg_level)
                arr[i].reserved = int(math.ceil(1000.0 * lv["lam"]))
            if fp32 and Bv != 1:
                lv["vals32"] = lv["vals"].to(torch.float32)
                arr[i].vals32 = lv["vals32"].data_ptr()
            if "agg" in lv:
                arr[i].agg, arr[i].agg_ptr = lv["agg"].data_ptr(), lv["agg_ptr"].data_ptr()
                arr[i].agg_members = lv["agg_members"].data_ptr()
                if lv.get("p_cols") is not None:      # smoothed aggregation: P as ELL rows, P^T weights
                    arr[i].agg_weights, arr[i].p_cols = lv["agg_weights"].data_ptr(), lv["p_cols"].data_ptr()
                    arr[i].p_vals, arr[i].p_width = lv["p_vals"].data_ptr(), int(lv["p_cols"].shape[0])
        last = chain[-1]
        if dense_coarse and Bv == 1 and len(chain) > 1 and last["n"] <= 128:
            nc = last["n"]
            dense = torch.zeros((nc, nc), dtype=torch.float64, device=p.device)
            rows = torch.arange(nc, device=p.device).repeat(last["W"])
            dense.index_put_((rows, last["cols"].reshape(-1).long()), last["vals"].reshape(-1), accumulate=True)
            inv, info = torch.linalg.inv_ex(dense)  # a singular last level keeps its Jacobi sweeps
            inv = 0.5 * (inv + inv.t())            # symmetric to the last bit: the cycle stays a symmetric preconditioner
            if int(info) == 0 and bool(torch.isfinite(inv).all()):
                last["dense_inv"] = inv.contiguous()
                arr[len(chain) - 1].dense_inv = last["dense_inv"].data_ptr()
        return arr, chain      # keep `chain` alive: it owns the coarse value tensors

    def representative_operator(self, vals, Bv, B):
        """abar (W, n) = mean over the REAL samples of a_b / s_b, s_b the mean free-row diagonal of sample b: the one
        matrix the batch-shared aggregates and prolongation are built from (csrc/coarsen.hip)."""
        p, L = self.p, self.L
        st = _stream(p.device)
        Br = B if Bv > 1 else 1
        nblk = (p.n + _hip.ELL_SCALE_CHUNK - 1) // _hip.ELL_SCALE_CHUNK
        part = torch.empty((nblk, Bv), dtype=torch.float64, device=p.device)
        sums = torch.empty(Bv, dtype=torch.float64, device=p.device)
        L.diffhe_ell_sample_scales(vals, p.is_bc, p.n, Bv, part, sums, st)
        weight = (max(p.n - p.n_bc, 1) / sums).contiguous()          # 1 / s_b
        abar = torch.empty((p.W, p.n), dtype=torch.float64, device=p.device)
        L.diffhe_ell_mean_operator(vals, weight, p.n, p.W, Bv, Br, abar, st)
        return abar

    def strength_filter(self, abar, theta):
        """-> (strong columns (W, n) int32, filtered values (W, n)) of diffhe_ell_strength_filter on the plan's pattern."""
        p = self.p
        strong = torch.empty((p.W, p.n), dtype=torch.int32, device=p.device)
        filt = torch.empty((p.W, p.n), dtype=torch.float64, device=p.device)
        self.L.diffhe_ell_strength_filter(abar, p.cols, p.n, p.W, float(theta), strong, filt, _stream(p.device))
        return strong, filt

    def operator_levels(self, vals, Bv, B, theta):
        """Device-side level dicts of the coefficient-aware hierarchy of THIS call's operator (diffhe.amg), and its
        (levels, operator complexity).  Representative operator and fine-level filter on the device, the levels on the
        host, as the unit hierarchy's are."""
        from .amg import build_hierarchy_sa, hierarchy_stats
        p = self.p
        abar = self.representative_operator(vals, Bv, B)
        strong, filt = self.strength_filter(abar, theta)
        cols = p.cols.cpu().numpy()
        host = build_hierarchy_sa(cols, None, p.is_bc.cpu().numpy(), strength=theta, rep_vals=abar.cpu().numpy(),
                                  fine_filter=(strong.cpu().numpy(), filt.cpu().numpy()))
        return [p.upload_amg_level(lv, True) for lv in host], hierarchy_stats(cols, host)

    def amg_pcg(self, amg, rhs, Bp, Bv, opts) -> _Solved:
        p, L = self.p, self.L
        arr, chain = amg
        nl = len(chain)
        work = torch.empty(L.diffhe_ell_amg_workspace_doubles(arr, nl, Bp), dtype=torch.float64, device=p.device)
        return self._solve(Bp, lambda x, relres, iters, st: L.diffhe_ell_amg_pcg_solve(
            arr, nl, Bv, rhs, x, Bp, self.tol, min(self.max_iter, int(opts.get("max_iter", 20000))), int(opts["n_coarse"]),
            int(opts["gamma"]), float(opts["scale"]),
            (_hip.PCG_FP32 if int(opts.get("fp32", 0)) else 0) | (0 if int(opts.get("floor", 1)) else _hip.PCG_NO_FLOOR),
            work, relres, iters, st,
            _stream(p.device)))

    def grad_kappa_factored(self, vals, lift, lam, x, Bp):
        """dL/dkappa_b = -lam^T K_1 u for a batch-shared (factored) lattice operator in one strip pass:
        lam^T (A_1 x + K_1[free,bc] g).  Returns None below the strip-kernel threshold."""
        p, L = self.p, self.L
        arr = self.lattice_levels(vals[:1])
        part = torch.empty(L.diffhe_lattice_blocks(p.n, Bp) * Bp, dtype=torch.float64, device=p.device)
        out = torch.empty(Bp, dtype=torch.float64, device=p.device)
        # bound as a plain int, not a checked status: DIFFHE_E_TOOBIG (-3) is an answer here, every other code an error
        rc = L.diffhe_lattice_bilinear(arr, 1, None, x, lam, lift, part, out, Bp, _stream(p.device))
        if rc == -3:
            return None
        _hip.check(rc, "diffhe_lattice_bilinear")
        return -out

    def grad_kappa(self, lam, x, B, Bp, mode, em):
        """dL/dkappa = -lambda^T k0 u -> (per-sample sums, per-element gradient) as `element_grad` leaves them."""
        p, L = self.p, self.L
        args, st = (p.elems, p.element_stiffness(), lam, x, self.g, p.npe, p.m), _stream(p.device)

        def per_sample(dk_e, osc, ose, part, dk_sum):
            if dk_e is not None and p.is_lattice and Bp >= 64:
                # lattice mesh, per-element gradient of every sample: strip pass (each nodal value read once per wave)
                lev = p.levels[0]
                small = lev.compact("k0")
                L.diffhe_lattice_grad_kappa(lev.nx, lev.ny, small if small is not None else lev.k0,
                                            1 if small is not None else 0, lam, x, self.g, dk_e, Bp, st)
                return
            if part is None:    # this entry always leaves the totals
                part = torch.empty((L.diffhe_grad_kappa_blocks(p.m, Bp), Bp), dtype=torch.float64, device=p.device)
                dk_sum = torch.empty(Bp, dtype=torch.float64, device=p.device)
            L.diffhe_p1_grad_kappa(*args, Bp, dk_e, part, dk_sum, st)

        return self.element_grad(mode, em, B, Bp, None, per_sample,
                                 lambda dk, osc, ose: L.diffhe_p1_grad_kappa_shared(*args, B, Bp, dk, st))

    # -- per-call Dirichlet data (csrc/bc.hip): boundary band only ------------------------------------------
    def bc_lift(self, kappa_s, G, rhs, rsn, rsb, B):
        """rhs_b -= K_b[F, D] G_b on the free rows with a Dirichlet neighbour; rhs (i, b) at i*rsn + b*rsb."""
        p, band = self.p, self.p.dirichlet_band()
        (kdev, kse, ksb), (gdev, gsj, gsb) = kappa_s, G
        self.L.diffhe_bc_lift(p.elems, p.npe, p.m, p.element_stiffness(), kdev, kse, ksb, band["d_slot"], gdev, gsj,
                              gsb, band["rows"], band["row_ptr"], band["row_inc"], band["n_rows"], rhs, rsn, rsb, B,
                              _stream(p.device))

    def bc_scatter(self, G, u, usn, usb, B):
        """u_b[j] = G_b[j] on the Dirichlet rows; u (i, b) at i*usn + b*usb."""
        p, band = self.p, self.p.dirichlet_band()
        gdev, gsj, gsb = G
        self.L.diffhe_bc_scatter(band["d_idx"], band["n_d"], gdev, gsj, gsb, u, usn, usb, B, _stream(p.device))

    def bc_grad(self, kappa_s, lam, lsn, lsb, gbar, gsn, gsb, out, osj, osb, G=None, dots=None, B=1):
        """out_b[j] = gbar_b[j] - (K_b lam_b)_j on the Dirichlet nodes (dL/dG_b); dots (n_D, B): G_b[j] (K_1 lam_b)_j."""
        p, band = self.p, self.p.dirichlet_band()
        kdev, kse, ksb = kappa_s
        gdev, Gsj, Gsb = G if G is not None else (None, 0, 0)
        self.L.diffhe_bc_grad(p.elems, p.npe, p.m, p.element_stiffness(), kdev, kse, ksb, band["d_slot"], band["d_idx"],
                              band["d_ptr"], band["d_inc"], band["n_d"], lam, lsn, lsb, gbar, gsn, gsb, out, osj, osb,
                              gdev, Gsj, Gsb, dots, B, _stream(p.device))

    def bc_grad_kappa(self, lam, lsn, lsb, G, dk, dse, dsb, shared, B):
        """dk (e, b) at e*dse + b*dsb -= lam_b^T k0_e G_b on the elements that touch a Dirichlet node (shared: dk (e) at
        e*dse, minus the sum over the batch)."""
        p, band = self.p, self.p.dirichlet_band()
        gdev, gsj, gsb = G
        self.L.diffhe_bc_grad_kappa(p.elems, p.npe, p.m, p.element_stiffness(), band["d_slot"], band["band_elems"],
                                    band["n_be"], lam, lsn, lsb, gdev, gsj, gsb, dk, dse, dsb, int(shared), B,
                                    _stream(p.device))


def _precision_text(flags: int, coeff_storage: str, Bv: int, Bp: int, fused_lib: int, recompute_ap: bool) -> str:
    """Plain-words account of the precisions of one lattice solve, from the flag word actually passed to
    diffhe_lattice_pcg_solve and the library's own switches (nothing here is a literal about 'the' configuration)."""
    if not flags & _hip.PCG_FP32:
        return "fp64 throughout: every vector stored fp64, all arithmetic fp64"
    spl2 = Bp % 128 == 0 and fused_lib == 2
    packed = not flags & _hip.PCG_UNFUSED and fused_lib != 0 and (
        (coeff_storage == "shared-fp32" and Bp % 64 == 0) or (coeff_storage == "fp16-rowsum" and spl2))
    parts = ["iterate x, residual r, right-hand side, the updates x += alpha p and r -= alpha A p and EVERY reduction "
             "(r.r, r.z, p.Ap accumulation, energy estimate): fp64",
             "CG search directions p and all V-cycle (preconditioner) vectors: STORED fp32"]
    if packed:
        parts.append("V-cycle arithmetic: fp32 (" + (("packed, two samples per lane" + (
            " (four in the way-down pass)" if Bp % 256 == 0 and not flags & _hip.PCG_PRE2 and coeff_storage == "shared-fp32" else ""))
            if spl2 else "one sample per lane")
                     + "; coefficients: "
                     + {"shared-fp32": "batch-shared fp32 copies, scalar loads",
                        "fp16-rowsum": "per-sample fp32 diagonal + scaled fp16 couplings, row sums kept"}[coeff_storage]
                     + "); it is a preconditioner only")
    else:
        parts.append("V-cycle arithmetic: fp64 in registers on the fp32-stored vectors"
                     + ("" if coeff_storage in ("", "fp64") else f" (coefficients: {coeff_storage})"))
    if Bv == 1 and recompute_ap:
        parts.append("A p is never stored: the residual update recomputes it in fp64 from the stored fp32 p")
        if not flags & _hip.PCG_RESID_FP64:
            parts.append("r is carried as a pair of fp32 vectors (hi = the V-cycle's input, lo = the remainder: 48 bits, "
                         "updated in fp64 registers) where the fused CG loop runs; mg={'resid_pair': 0} keeps it fp64")
            if not flags & _hip.PCG_RESID_KEEP_LO:
                parts.append("with the energy rule in force lo is dropped once every active sample's estimate is within "
                             "2^16 of its stop level (r is then hi alone, 24 bits per update; info.resid_single_updates "
                             "counts those updates); mg={'resid_drop_lo': 0} keeps both halves")
        if flags & _hip.PCG_CLOSED_FP32_STEP and Bp % 64 == 0 and coeff_storage == "shared-fp32":
            parts.append("p.Ap: stencil in fp32 on the stored p, accumulated fp64 -- enters the STEP LENGTH alpha only "
                         "(closed regular lattice); r = b - A x holds in fp64 whatever alpha is")
        else:
            parts.append("p.Ap: fp64 stencil")
    else:
        parts.append("A p: fp64, stored")
    return "; ".join(parts)


def _rule_counts(rule: torch.Tensor, B: int) -> dict:
    c = torch.bincount(rule[:B].to(torch.int64), minlength=3).tolist()
    return {"cap": c[0], "residual": c[1], "energy": c[2]}



def _kappa_layout(kappa: torch.Tensor, m: int, B_f: Optional[int], node_major: bool, nc: int = 0):
    """-> (mode, B, kappa_em) of one call; B_f is f's batch, None for one unbatched forcing.  layout='node': per-sample
    kappa fields may come element-major, (m, B), like f and u -- no transposing pass for kappa or its gradient either
    (a square (m, m) tensor is read that way).  nc > 0: kappa is a conductivity tensor of nc Voigt components
    (`_tensor_mode`)."""
    if nc:
        mode, B_k, kappa_em = _tensor_mode(kappa, nc, m, B_f, node_major)
    else:
        kappa_em = bool(node_major and kappa.dim() == 2 and tuple(kappa.shape) == (m, B_f))
        mode, B_k = (K_SAMPLE_ELEM, B_f) if kappa_em else _kappa_mode(kappa, m, B_f)
    B = B_f if B_f is not None else (B_k if B_k is not None else 1)
    if B_k is not None and B_k != B:
        raise ValueError(f"kappa batch {B_k} does not match f batch {B}")
    return mode, B, kappa_em


def _kappa_strided(kappa: torch.Tensor, mode: int, kappa_em: bool, B: int, m: int, device):
    """-> (kappa on the device, stride per element, stride per sample): kappa as the 1D scan and the node-gradient
    kernel read it, in the caller's layout."""
    k = kappa.detach().to(device, torch.float64)
    if mode == K_SCALAR:
        return k.reshape(1).contiguous(), 0, 0
    if mode == K_SAMPLE:
        return k.reshape(B).contiguous(), 0, 1
    if mode == K_ELEM:
        return k.reshape(m).contiguous(), 1, 0
    if kappa_em:                                                     # (m, B), layout='node'
        return k.contiguous(), B, 1
    return k.reshape(B, m).contiguous(), 1, m                        # (B, m)


def _kappa_grad(mode: int, shape, per_sample=None, per_elem=None) -> torch.Tensor:
    """dL/dkappa in the shape of the caller's kappa, from the per-sample sums over the elements (B,) or from the
    per-element gradient: (B, m) -- (m, B) for an element-major kappa -- or (m,) already summed over the batch."""
    if mode == K_SCALAR:
        g = (per_sample if per_sample is not None else per_elem).sum()
    elif mode == K_SAMPLE:
        g = per_sample if per_sample is not None else per_elem.sum(1)
    elif mode == K_ELEM:
        g = per_elem if per_elem.dim() == 1 else per_elem.sum(0)
    else:
        g = per_elem
    return g.reshape(shape)


@dataclass
class _Call:
    """The inputs of one solve, normalised once.  The adjoint state keeps `facts()`: none of the input tensors."""
    B: int
    mode: int                       # kappa layout, K_*
    kappa_em: bool                  # per-sample kappa fields given element-major, (m, B)
    batched: bool                   # f came with a batch dimension
    node_major: bool                # f, load and u are (n, B)
    out_device: torch.device
    kappa_shape: torch.Size
    kappa_device: torch.device
    load_batched: bool
    reaction: float
    kappa: Optional[torch.Tensor] = None
    f_dev: Optional[torch.Tensor] = None       # (B, n) or (n,); layout='node': a (B, n) view of (n, B) data
    load_dev: Optional[torch.Tensor] = None    # (B, n) or None
    # per-call Dirichlet data (`dirichlet=`): (device values, stride per Dirichlet node, stride per sample), G_b[j] at
    # j * sj + b * sb (sb = 0: one G for the batch); None: the mesh's.  Boundary-sized: the adjoint state keeps it
    bc: Optional[tuple] = None
    # kappa and f as the band kernels (a call with `dirichlet=`) and the node-gradient kernel (`shape`) read them:
    # (device view of the op's input, stride per element / node, stride per sample).  Views, kept with the state too
    kappa_s: Optional[tuple] = None
    f_s: Optional[tuple] = None
    nc: int = 0                     # kappa is a conductivity tensor of nc Voigt components (diffhe.aniso); 0: a scalar

    @classmethod
    def of(cls, solver, plan: SolvePlan, kappa, f, load, node_major, dirichlet=None, shape=False) -> "_Call":
        if load is not None and load.numel() == 0:
            load = None
        batched, n, out_device = f.dim() == 2, plan.n, f.device
        if node_major and (plan.is_chain or not batched):
            raise ValueError("layout='node' takes (n, B) tensors on 2D meshes")
        if node_major:
            f = f.t()                       # a (B, n) VIEW for the shape logic below; the data stays (n, B)
            load = load.t() if load is not None else None
        nc = solver._tensor_components()
        mode, B, kappa_em = _kappa_layout(kappa, plan.m, f.shape[0] if batched else None, node_major, nc)
        f_dev = f.detach().to(plan.device, torch.float64)
        f_s = None
        if shape:       # one forcing for the batch, or the (B, n) view through its strides
            f_s = (f_dev.contiguous(), 1, 0) if f_dev.dim() == 1 else (f_dev, f_dev.stride(1), f_dev.stride(0))
        f_dev = f_dev if node_major else f_dev.contiguous()      # node-major: a transposed view of contiguous (n, B) data
        load_dev = None
        if load is not None:      # extra nodal load, added to the assembled F on the free rows
            load_dev = load.detach().to(plan.device, torch.float64)
            load_dev = (load_dev.reshape(1, n).expand(B, n) if load_dev.dim() == 1 else load_dev).contiguous()   # (B, n)
            if load_dev.shape != (B, n):
                raise ValueError(f"load must be (n,) or (B,n) with B={B}, n={n}, got {tuple(load.shape)}")
        bc = None
        if dirichlet is not None:
            gd = dirichlet.detach().to(plan.device, torch.float64)
            if gd.dim() == 1 and gd.shape[0] == plan.n_bc:
                bc = (gd.contiguous(), 1, 0)
            elif gd.dim() == 2 and tuple(gd.shape) == ((plan.n_bc, B) if node_major else (B, plan.n_bc)):
                bc = (gd, gd.stride(0), gd.stride(1)) if node_major else (gd, gd.stride(1), gd.stride(0))
            else:
                raise ValueError(f"dirichlet must be ({plan.n_bc},) or "
                                 f"{(plan.n_bc, B) if node_major else (B, plan.n_bc)}, got {tuple(dirichlet.shape)}")
        kappa_s = None
        if shape or bc is not None:
            kappa_s = _kappa_strided(kappa, mode, kappa_em, B, plan.m, plan.device)
        return cls(B, mode, kappa_em, batched, node_major, out_device, kappa.shape, kappa.device,
                   load is not None and load.dim() == 2, float(solver.reaction), kappa, f_dev, load_dev, bc, kappa_s, f_s,
                   nc)

    def facts(self) -> "_Call":
        return replace(self, kappa=None, f_dev=None, load_dev=None)


def _call_options(*, chain: bool, lattice: bool, closed_boundary: bool, n: int, mode: int, tol_user: Optional[float],
                  mg_user, mg: dict, amg: dict) -> Tuple[float, dict, dict]:
    """(tol, mg, amg) of ONE call, DESIGN section 4 "Stopping rule": `chain` (a 1D chain mesh, whichever path it takes),
    `lattice` (route taken), `closed_boundary` (every lattice edge node Dirichlet), `n` nodes, kappa `mode`, the user's
    `tol_user` (None: automatic) and `mg_user` keys.  `mg` / `amg` are copied: nothing sticks to the next call."""
    mg, amg, tol = dict(mg), dict(amg), tol_user
    if mode in (K_ELEM, K_SAMPLE_ELEM):
        # per-element gradients amplify the rough part of the solver error, which keeps converging after the true
        # residual has stalled: no attainable-accuracy floor (288 x 296: dL/dkappa_e 2.2e-10 -> 1.4e-11)
        if "floor" not in mg_user:
            mg["floor"] = 0
        amg.setdefault("floor", 0)     # honoured as given when the caller put a "floor" key into solver.amg
    closed = lattice and closed_boundary
    if tol is None:
        # relative residual: 1e-12 on closed lattices with one kappa per sample (multigrid keeps error ~ residual);
        # one or two more decades for per-element fields, Neumann parts, the general path and systems below 10^5 nodes
        simple = mode in (K_SCALAR, K_SAMPLE)
        tol = 1e-12 if (chain or (closed and simple and n >= 100_000)) else \
            (1e-13 if (closed or not lattice) and simple else 1e-14)
    # the energy norm controls nodal values only on closed lattices (with Neumann parts the near-constant mode carries
    # no energy: the estimate fell 40x below the nodal error): elsewhere the residual decides alone
    if not closed and "tol_energy" not in mg_user:
        mg["tol_energy"] = 0.0
    # an explicit `tol` is a request on the RESIDUAL: the energy-norm stop steps aside unless asked for too
    if tol_user is not None and "tol_energy" not in mg_user:
        mg["tol_energy"] = 0.0
    if "tol_energy" not in mg_user and mg.get("tol_energy"):
        # calibrated on nodal error; per-element gradients (products of grad u and grad lambda) ran 20-60x above the
        # estimate: two more decades for them, one more for small systems, like `tol`
        if mode in (K_ELEM, K_SAMPLE_ELEM):
            mg["tol_energy"] *= 1e-2
        if n < 100_000:
            mg["tol_energy"] *= 0.1
    return tol, mg, amg


def _select_path(plan: SolvePlan, solver, reaction: float) -> type:
    """The path class of one call."""
    # the scan solver inverts a pure path-graph Laplacian: with a reaction term the chain takes the general path
    if reaction and plan.is_p2:
        raise NotImplementedError("reaction term with P2 elements: the lumped P2 mass vanishes at the vertices")
    if plan.is_chain and reaction == 0.0:
        return _ChainSolve
    # lattice fast path unless more than 2 % of the nodes are interior Dirichlet nodes (5 % on 256^2: 99 geometric-
    # multigrid iterations, parity missed; the aggregation path takes 33)
    if plan.is_lattice and solver.method == "auto" and plan.n_bc_interior <= 0.02 * plan.n:
        return _LatticeSolve
    return _EllSolve


class _PathSolve:
    """One call's solve on one path: forward() keeps what adjoint() needs as named fields -- no input tensor, right-hand
    side or assembly temporary -- and this object is the adjoint state the custom ops hold until the end of backward.
    adjoint(g, need_k, need_f, need_load) -> (lambda in the path's layout, per-sample dL/dkappa sums, per-element
    dL/dkappa as `_kappa_grad` takes them, dL/df and dL/dload per sample in the caller's layout)."""
    Info = SolveInfo        # the class of `solver.last_info` after a call on this path (`_run_call`)

    def __init__(self, solver, plan: SolvePlan, call: _Call, tol: float, mg: dict, amg: dict, homogeneous: bool = False):
        self.solver, self.plan, self.call, self.mg, self.amg = solver, plan, call.facts(), mg, amg
        # per-call Dirichlet data: the path solves with homogeneous data, csrc/bc.hip adds G
        zero_g = homogeneous or call.bc is not None
        self.eng = _Engine(plan, tol, solver.max_iter, solver.check_every, solver.assembly,
                           ref_order=solver.operator == "assembled", g=plan.zero_g() if zero_g else None)


class _ChainSolve(_PathSolve):
    """1D chain: one scan per sample ("chain1d-scan-ref" in the reference's operation order, "chain1d-scan")."""

    def forward(self, call: _Call, info: SolveInfo) -> torch.Tensor:
        plan, L, B, n = self.plan, self.eng.L, call.B, self.plan.n
        f_dev, batched = call.f_dev, call.batched
        self.kdev, self.kse, self.ksb = call.kappa_s or _kappa_strided(call.kappa, call.mode, False, B, plan.m,
                                                                       plan.device)
        load_dev = call.load_dev
        if call.bc is not None:
            # per-call Dirichlet data: the lift -K_b[F, D] G_b enters as an extra load, the scan sees homogeneous data
            lift = torch.zeros((B, n), dtype=torch.float64, device=plan.device)
            self.eng.bc_lift(call.kappa_s, call.bc, lift, 1, n, B)
            load_dev = lift if load_dev is None else load_dev + lift
        if load_dev is not None:
            # the 1D load map of solver.py:95-96 is diagonal (h/2 from each side): an extra load is a change of forcing
            f_dev = (f_dev if batched else f_dev.reshape(1, n).expand(B, n)) + load_dev / plan.lumped_mass()
            batched = True
        self.u = torch.empty((B, n), dtype=torch.float64, device=plan.device)      # Dirichlet values included
        # reference-order mode (default): the system the reference assembled in fp64 (rounded diagonal), see chain1d.hip
        self.chain_flags = _hip.CHAIN_REFERENCE_ORDER if self.solver.chain == "reference" else 0
        info.path = "chain1d-scan-ref" if self.chain_flags else "chain1d-scan"
        ns = L.diffhe_chain1d_stage_doubles(n, B, plan.max_seg_len, self.chain_flags)   # 0: every segment in registers
        stage = torch.empty(ns, dtype=torch.float64, device=plan.device) if ns > 0 else None
        L.diffhe_chain1d_solve(plan.x, self.kdev, self.ksb, self.kse, f_dev, n if batched else 0, plan.seg, plan.n_seg,
                               self.eng.g, self.u, n, n, B, plan.max_seg_len, self.chain_flags, stage,
                               _stream(plan.device))
        if call.bc is not None:     # u keeps G in its Dirichlet rows: the adjoint's dL/dkappa reads u as it is
            self.eng.bc_scatter(call.bc, self.u, 1, n, B)
        return self.u

    def adjoint(self, g: torch.Tensor, need_k: bool, need_f: bool, need_load: bool):
        """One fused pass: df = M^T lambda (the adjoint of the scan), dL/dkappa per element and its per-sample sums."""
        plan, L, B, m, n = self.plan, self.eng.L, self.call.B, self.plan.m, self.plan.n
        df = torch.empty((B, n), dtype=torch.float64, device=plan.device)
        want_e = self.call.mode in (K_ELEM, K_SAMPLE_ELEM)
        dk_e = torch.empty((B, m), dtype=torch.float64, device=plan.device) if want_e else None
        part = torch.empty((B, plan.n_seg), dtype=torch.float64, device=plan.device)
        ns = L.diffhe_chain1d_stage_doubles(n, B, plan.max_seg_len, self.chain_flags)
        stage = torch.empty(ns, dtype=torch.float64, device=plan.device) if ns > 0 else None
        L.diffhe_chain1d_adjoint(plan.x, self.kdev, self.ksb, self.kse, g, n, self.u, n, plan.seg, plan.n_seg, df, n,
                                 dk_e, m, part, n, B, plan.max_seg_len, self.chain_flags, stage, _stream(plan.device))
        dk_sample = part.sum(dim=1)                      # (B,) tiny host-side glue
        # the chain's extra load went in as forcing: dL/dload = df / lumped mass
        return df, dk_sample, dk_e, df, df / plan.lumped_mass() if need_load else None

    def shape_fields(self, lam):
        """(u, lambda, node stride, sample stride, Dirichlet data) for the node-gradient kernel: (B, n) arrays."""
        plan = self.plan
        lam = torch.where(plan.is_bc.bool(), torch.zeros((), dtype=torch.float64, device=plan.device),
                          lam / plan.lumped_mass())  # lambda = df / lumped mass, as grad_load
        return self.u, lam.contiguous(), 1, plan.n, None


class _NodeMajorSolve(_PathSolve):
    """The lattice and general paths: the kernels work on (n, Bp) arrays, `x` is the eliminated-system solution."""
    lattice = False     # the load matrix is stored as lattice diagonals (True) or as ELL rows

    def _rhs(self, call: _Call, lift, Bv, lift_scale=None) -> torch.Tensor:
        """F = M f - lift_scale * lift (+ load) on the free rows, 0 on Dirichlet rows: (n, Bp)."""
        eng, plan, B, Bp = self.eng, self.plan, call.B, self.Bp
        if not call.node_major:
            f_nm = eng.to_node_major(call.f_dev, B, Bp, plan.n)          # API layout: one transposing pass
        elif Bp == B and call.f_dev.t().is_contiguous():
            f_nm = call.f_dev.t()                                        # (n, B) data: used as it is
        else:
            f_nm = torch.zeros((plan.n, Bp), dtype=torch.float64, device=plan.device)   # ... or padded
            f_nm[:, :B] = call.f_dev.t()
        rhs = eng.load_vector(f_nm, lift, Bv, Bp, lift_scale, lattice=self.lattice)
        if call.load_dev is not None:
            rhs += eng.to_node_major(call.load_dev, B, Bp, plan.n, zero_mask=plan.is_bc)
        if call.bc is not None:     # per-call Dirichlet data: - K_b[F, D] G_b on the boundary band
            eng.bc_lift(call.kappa_s, call.bc, rhs, Bp, 1, B)
        return rhs

    def _adjoint_rhs(self, g: torch.Tensor) -> torch.Tensor:
        plan, B, Bp = self.plan, self.call.B, self.Bp
        if not self.call.node_major:
            return self.eng.to_node_major(g, B, Bp, plan.n, zero_mask=plan.is_bc)
        # the adjoint right-hand side must vanish on Dirichlet rows (lambda_bc = 0): a cotangent that already does
        # (L = sum u^2 with zero Dirichlet data) is used as it is
        dirty = plan.n_bc > 0 and bool((g[plan.bc_index()] != 0).any())
        if Bp == B and g.is_contiguous() and not dirty:
            return g
        rhs = torch.zeros((plan.n, Bp), dtype=torch.float64, device=plan.device)
        rhs[:, :B] = g
        if dirty:
            rhs[plan.bc_index()] = 0.0
        return rhs

    def adjoint(self, g: torch.Tensor, need_k: bool, need_f: bool, need_load: bool):
        """lambda = A^-1 g on the free rows with the forward's operators and preconditioner, then the gradient pieces."""
        eng, call, B, Bp, n = self.eng, self.call, self.call.B, self.Bp, self.plan.n
        info = self.solver.last_info
        lam, its, bad, relres, *_ = self._adjoint_solve(self._adjoint_rhs(g), info)
        info.adj_iterations = its
        info.adj_max_relres = float(relres[:B].max())
        info.not_converged += bad
        dk_sample, dk_elem = self._grad_kappa(lam) if need_k else (None, None)
        df = dload = None
        if need_f:
            df = eng.load_vector(lam, None, 1, Bp, lattice=self.lattice, free_rows=False)
            df = df[:, :B] if call.node_major else eng.to_sample_major(df, B, Bp, n)
        if need_load:
            dload = lam[:, :B].clone() if call.node_major else eng.to_sample_major(lam, B, Bp, n)
        return lam, dk_sample, dk_elem, df, dload

    def _grad_kappa(self, lam):
        """-> (per-sample sums, per-element gradient) of dL/dkappa = -lambda^T k0 u, as `_kappa_grad` takes them: the
        per-element one (B, m) like the API's kappa, or left element-major (m, B) when kappa came that way."""
        eng, call = self.eng, self.call
        if call.nc:     # a conductivity tensor: the gradient comes back in the caller's shape (`_solve_backward`)
            return None, eng.grad_tensor(lam, self.x, call.B, self.Bp, call.nc, call.mode, call.kappa_em)
        return eng.grad_kappa(lam, self.x, call.B, self.Bp, call.mode, call.kappa_em)

    def shape_fields(self, lam):
        """(u, lambda, node stride, sample stride, Dirichlet data) for the node-gradient kernel: (n, Bp) arrays."""
        return self.x, lam, self.Bp, 1, self.eng.g


class _LatticeSolve(_NodeMajorSolve):
    """2D lattice: geometric-multigrid PCG ("lattice-mgpcg"), or one dense product on small meshes ("lattice-direct")."""
    lattice = True

    def forward(self, call: _Call, info: SolveInfo) -> torch.Tensor:
        solver, plan, eng, B, mode, reaction = self.solver, self.plan, self.eng, call.B, call.mode, call.reaction
        info.path = "lattice-mgpcg"
        Bp = self.Bp = padded_batch(B)
        self.kappa_value = call.kappa.detach().to(plan.device, torch.float64).reshape(-1)[0] if mode == K_SCALAR else None
        # scalar kappa per sample stays factored on closed lattices only (with Neumann parts, cond ~ 1e7, the last-bit
        # difference between kappa_b (K_1 x) and (sum_e kappa_b k0_e) x shows as 4e-10 in u)
        closed_ = plan.closed_boundary and solver.operator != "assembled"
        self.factored = factored = closed_ and mode in (K_SCALAR, K_SAMPLE)
        # a factored operator (plan-constant unit matrices) replaces the levels from ~33^2 nodes down by ONE dense
        # product with a cached inverse -- the whole solve on meshes that small; not with a reaction term, which a
        # factored operator carries as a batch-shared diagonal SHIFT and per-sample matrices on their diagonals
        didx = plan.dense_level() if (factored and self.mg.get("dense_coarse", 1) and reaction == 0.0) else None
        vals, Bv, scale, lift, lift_scale = eng.lattice_assemble(call.kappa, mode, B, Bp, factor=closed_,
                                                                 n_levels=None if didx is None else didx + 1,
                                                                 em=call.kappa_em)
        self.shift = eng.reaction_shifts(reaction, len(vals)) if reaction and factored else None
        if reaction and not factored:
            eng.add_reaction(vals, reaction, lattice=True)
        rhs = self._rhs(call, lift, Bv, lift_scale)
        self.vals32, self.rdiag32, self.off16 = self._cycle_coeffs(vals, Bv)
        info.coeff_storage = ("fp64" if not self.mg.get("fp32") else
                              ("fp16-rowsum" if self.off16 is not None else "fp32") if Bv != 1 else "shared-fp32")
        self.direct, self.dense = didx == 0, None
        if didx is not None:
            if self.direct:
                info.path = "lattice-direct"
                self.mg = dict(self.mg, fp32=0)        # the direct product runs in fp64
            self.dense = plan.dense_coarse(didx, vals, bool(self.mg.get("fp32")))
        self.wkey = (Bp, mode, reaction)
        x, its, bad, relres, est, rule, flags, info.resid_single_updates = eng.lattice_pcg(
            vals, Bv, scale, rhs, Bp, self.mg, self.vals32, self.dense,
            x0=plan.warm_get(("u",) + self.wkey) if solver.warm_start else None, shift=self.shift, rdiag32=self.rdiag32,
            off16=self.off16)
        if solver.warm_start and not bad:
            # the next solve starts from a copy; but with layout='node' and no padding the caller's u IS x: keep a
            # private copy then, an in-place edit of u must not move the next warm start
            shares = call.node_major and Bp == B and not plan.has_dirichlet_data and call.bc is None
            plan.warm_put(("u",) + self.wkey, x.clone() if shares else x)
        info.stop_rules = _rule_counts(rule, B) if not self.direct else {}
        info.flags = flags
        info.precision = _precision_text(flags, info.coeff_storage, Bv, Bp, int(eng.L.diffhe_lattice_fused_passes()),
                                         bool(eng.L.diffhe_lattice_recompute_ap()))
        info.tol_energy = float(self.mg.get("tol_energy", 0.0) or 0.0)
        info.factored = bool(factored)
        info.iterations, info.not_converged = its, bad
        info.max_relres = float(relres[:B].max())
        info.err_est = float(est[:B].max())
        self.vals, self.x, self.Bv, self.scale = vals, x, Bv, scale
        self.lift = lift if Bv == 1 else None
        return _from_node_major(eng, x, B, Bp, plan.n, call.node_major, call.bc)

    def _cycle_coeffs(self, vals, Bv):
        """fp32-stored V-cycle -> (vals32, rdiag32, off16): fp32 copies of per-sample matrices; a batch-SHARED matrix
        also gets the reciprocal of its main diagonal, for the two-samples-per-lane strip kernels."""
        mg, Bp = self.mg, self.Bp
        vals32 = rdiag32 = off16 = None
        if mg.get("fp32") and Bv != 1 and mg.get("h16", 1) and Bp > 1:
            d32_, o16_, osc_ = self.eng.pack_cycle_coeffs(vals, Bv)   # fp32 diagonal + fp16 off-diagonals (row sums kept)
            if d32_ is not None:
                vals32, off16 = d32_, (o16_, osc_)
        if mg.get("fp32") and Bv != 1 and vals32 is None:
            vals32 = [v.float() for v in vals]
        elif mg.get("fp32") and Bv == 1 and mg.get("strip2", 1) and Bp % 64 == 0 and self.shift is None:
            # a factored operator is the unit-kappa K_1 of the mesh: plan-constant, its copies are cached
            vals32, rdiag32 = self.plan.shared_fp32(vals, cacheable=self.factored)
        return vals32, rdiag32, off16

    def _adjoint_solve(self, rhs, info):
        plan, eng, B = self.plan, self.eng, self.call.B
        ws = self.solver.warm_start is True
        res = eng.lattice_pcg(self.vals, self.Bv, self.scale, rhs, self.Bp, self.mg, self.vals32, self.dense,
                              x0=plan.warm_get(("lambda",) + self.wkey) if ws else None, shift=self.shift,
                              rdiag32=self.rdiag32, off16=self.off16)
        if ws and not res.not_converged:
            plan.warm_put(("lambda",) + self.wkey, res.x)
        info.adj_stop_rules = _rule_counts(res.rule, B) if not self.direct else {}
        info.adj_err_est = float(res.est[:B].max())
        info.adj_resid_single_updates = res.single_updates
        return res

    def _grad_kappa(self, lam):
        """Scalar kappa per sample or for all with ONE stored matrix: dL/dkappa_b in one strip pass, above the strip
        kernels' threshold.  The bilinear form must see K alone: factored operators keep the reaction term apart
        (`shift`), assembled ones carry it in `vals`."""
        call = self.call
        if call.mode in (K_SCALAR, K_SAMPLE) and self.Bv == 1 and (self.factored or not call.reaction):
            dk_sum = self.eng.grad_kappa_factored(self.vals, self.lift, lam, self.x, self.Bp)
            if dk_sum is not None:
                scaled = call.mode == K_SCALAR and not self.factored       # vals carry kappa: K = kappa K_1
                return (dk_sum / self.kappa_value if scaled else dk_sum)[:call.B], None
        return super()._grad_kappa(lam)


class _EllSolve(_NodeMajorSolve):
    """General meshes: ELL operator, aggregation-multigrid PCG ("ell-amgpcg") or Jacobi PCG ("ell-pcg")."""

    def _operator_form(self) -> Tuple[bool, bool]:
        """-> (the call may keep its operator factored, it stores one matrix per sample even for a kappa the batch
        shares).  For subclasses that add terms of their own to the operator (`_boundary_terms`)."""
        return True, False

    def _boundary_terms(self, vals, rhs, Bv) -> None:
        """Terms a subclass adds to the stored operator `vals` (W, n, Bv) and the right-hand side `rhs` (n, Bp) in place:
        after the assembly, the reaction term and `_rhs`, before the hierarchy is built from `vals`."""

    def forward(self, call: _Call, info: SolveInfo) -> torch.Tensor:
        solver, plan, eng, B, mode = self.solver, self.plan, self.eng, call.B, call.mode
        plan.ensure_ell()
        Bp = self.Bp = padded_batch(B)
        may_factor, per_sample = self._operator_form()
        # scalar kappa per sample on a boundary closed by Dirichlet data: FACTORED like on closed lattices, ONE unit
        # matrix K_1 for the batch and K_1 x = F_b / kappa_b, its aggregation hierarchy plan-constant.  Not with a
        # reaction term, operator="assembled" or Neumann parts ("General meshes")
        factored = (may_factor and not call.nc and mode in (K_SCALAR, K_SAMPLE) and call.reaction == 0.0
                    and solver.operator != "assembled" and not plan.is_p2 and solver.method != "ell-jacobi"
                    and plan.closed_boundary_general())
        self.inv_kappa = None
        if factored:
            vals, lift = eng.assemble(torch.ones(1, dtype=torch.float64, device=plan.device), 0, 0, 1)
            Bv = 1
            kpad = torch.ones(Bp, dtype=torch.float64, device=plan.device)
            kpad[:B] = call.kappa.detach().to(plan.device, torch.float64).reshape(-1)      # (B,), or one scalar for all
            self.inv_kappa = 1.0 / kpad
            rhs = self._rhs(call, lift, 1, kpad)                   # F_b = M f_b - kappa_b lift_1
            rhs *= self.inv_kappa                                  # ... / kappa_b: K_1 x = F_b / kappa_b
        else:
            if call.nc:     # conductivity tensor (diffhe.aniso): one matrix for the batch, or one per sample
                kdev, ksc, kse, ksb, Bv = eng.tensor_device(call.kappa, mode, B, Bp, call.nc, em=call.kappa_em)
                vals, lift = eng.assemble_tensor(kdev, ksc, kse, ksb, Bv)
            else:
                kdev, kse, ksb, Bv = eng.kappa_device(call.kappa, mode, B, Bp, em=call.kappa_em)
                if per_sample:      # a kappa shared by the batch is read with ksb = 0 into every sample's matrix
                    Bv = Bp
                vals, lift = eng.assemble(kdev, kse, ksb, Bv)
            if call.reaction:
                eng.add_reaction([vals], call.reaction, lattice=False)
            rhs = self._rhs(call, lift, Bv)
            self._boundary_terms(vals, rhs, Bv)
        self.amg_hier = self._amg_hierarchy(vals, Bv, factored) if solver.method != "ell-jacobi" else None
        if self.amg_hier is not None:
            info.path = "ell-amgpcg"
            info.hierarchy, info.hierarchy_levels, info.operator_complexity, info.hierarchy_age = self.hier_info
            x, its, bad, relres, *_ = eng.amg_pcg(self.amg_hier, rhs, Bp, Bv, self.amg)
        else:
            info.path = "ell-pcg"
            x, its, bad, relres, *_ = eng.cg(vals, rhs, Bp, Bv)
        info.iterations, info.not_converged = its, bad
        info.max_relres = float(relres[:B].max())
        info.factored = bool(factored)
        self.vals, self.x, self.Bv = vals, x, Bv
        return _from_node_major(eng, x, B, Bp, plan.n, call.node_major, call.bc)

    def _amg_hierarchy(self, vals, Bv, factored):
        """The aggregation-multigrid hierarchy of this call (None: no coarse level, Jacobi PCG), after the automatic
        `amg` options of the general path."""
        solver, plan, eng, amg = self.solver, self.plan, self.eng, self.amg
        if factored and "fp32" not in solver._amg_user:
            # the fp32-stored cycle, off for kappa FIELDS (contrast breaks it), suits the contrast-free unit operator
            amg["fp32"] = 1
        theta = float(amg.get("strength", 0) or 0)
        if theta > 0.0:
            return self._operator_hierarchy(vals, Bv, factored, theta)
        smoothed = bool(amg.get("smoothed", 1))
        amg_levels = plan.ensure_amg(smoothed=smoothed)
        if amg.get("scale") is None:
            amg["scale"] = 1.3 if amg.get("smoothed", 1) else 1.8
        if amg.get("gamma") is None:      # None = automatic (the default); an explicit 1 or 2 is honoured
            # W-cycle where the fine level dominates the cycle (>= 12 M node-samples), V-cycle below
            amg["gamma"] = 2 if smoothed and plan.n * self.Bp >= 12_000_000 else 1
        fp32 = bool(amg.get("fp32", 0))
        self.hier_info = ("unit", len(amg_levels) + 1, plan.unit_amg_complexity(smoothed), 0) if amg_levels else None
        if amg_levels and factored:          # plan-constant hierarchy of the unit operator: built once
            return plan.unit_amg((smoothed, fp32), lambda: eng.amg_setup(vals, 1, fp32, amg_levels, dense_coarse=True))
        if amg_levels:                       # at least one coarse level: aggregation-AMG PCG
            return eng.amg_setup(vals, Bv, fp32, amg_levels)
        return None

    def _operator_hierarchy(self, vals, Bv, factored, theta):
        """amg=dict(strength=theta): the hierarchy of the operator being solved ("Coefficient-aware
        hierarchy").  It depends on the coefficient, so it lives on the SOLVER: built by the first general-path call from
        that call's assembled operator (reaction and facet terms included), reused by later calls -- a stale hierarchy is
        still an SPD preconditioner, only iteration counts drift -- until `refresh_hierarchy()` or every
        amg["refresh"]-th call.  A factored solve's operator is the plan-constant K_1: its hierarchy is plan-cached."""
        solver, plan, eng, amg = self.solver, self.plan, self.eng, self.amg
        if not amg.get("smoothed", 1):
            raise ValueError("amg strength > 0 builds a smoothed-aggregation hierarchy: it needs smoothed=1")
        if amg.get("scale") is None:
            amg["scale"] = 1.3
        if amg.get("gamma") is None:
            amg["gamma"] = 2 if plan.n * self.Bp >= 12_000_000 else 1
        fp32 = bool(amg.get("fp32", 0))
        if factored:
            def build():
                levels, stats = eng.operator_levels(vals, 1, 1, theta)
                return (eng.amg_setup(vals, 1, fp32, levels, dense_coarse=True) if levels else None), stats
            hier, stats = plan.unit_amg((True, fp32, theta), build)
            self.hier_info = ("operator", stats[0], stats[1], 0) if hier else None
            return hier
        levels, stats, age = solver._hierarchy_levels(plan, theta, int(amg.get("refresh", 0) or 0),
                                                      lambda: eng.operator_levels(vals, Bv, self.call.B, theta))
        self.hier_info = ("operator", stats[0], stats[1], age) if levels else None
        return eng.amg_setup(vals, Bv, fp32, levels) if levels else None

    def _adjoint_solve(self, rhs, info):
        """The forward's preconditioner and saved (per-sample) coarse operators; factored: lambda_b = K_1^-1 (g_b / kappa_b)."""
        eng = self.eng
        if self.inv_kappa is not None:
            rhs = rhs * self.inv_kappa
        if self.amg_hier is not None:
            return eng.amg_pcg(self.amg_hier, rhs, self.Bp, self.Bv, self.amg)
        return eng.cg(self.vals, rhs, self.Bp, self.Bv)


def _begin_call(solver, plan: SolvePlan, call: _Call, path: Optional[type] = None,
                homogeneous: bool = False) -> _PathSolve:
    """The path object of one call, before its forward: the path class (`_select_path`, unless the caller forces one),
    the per-call options (`_call_options`), `solver.tol`.  homogeneous: solve with zero Dirichlet data, whatever the mesh
    carries."""
    if path is None:
        path = _select_path(plan, solver, call.reaction)
    tol, mg, amg = _call_options(chain=plan.is_chain, lattice=path is _LatticeSolve, closed_boundary=plan.closed_boundary,
                                 n=plan.n, mode=call.mode, tol_user=solver._tol_user, mg_user=solver._mg_user,
                                 mg=solver.mg, amg=solver.amg)
    solver.tol = tol          # `solver.tol` reports the tolerance of the last call
    return path(solver, plan, call, tol, mg, amg, homogeneous)


def _run_call(state: _PathSolve, call: _Call) -> torch.Tensor:
    """The forward solve of a call that `_begin_call` set up: u as the caller gets it (a call without a batch loses the
    batch dimension; on f's device), the solver's `last_info`, the warning when a system missed the tolerance."""
    solver, info = state.solver, state.Info()
    u = state.forward(call, info)
    solver.last_info = info
    if info.not_converged:
        warnings.warn(f"diffhe: {info.not_converged} of {call.B} systems did not reach tol={solver.tol:g} "
                      f"(max relative residual {info.max_relres:.2e}, path {info.path})", RuntimeWarning)
    out = u if call.batched or call.B > 1 or call.node_major else u[0]
    return out.to(call.out_device)


def _solve_forward(solver, kappa, f, load=None, node_major=False, dirichlet=None, shape=False):
    """u = (K(kappa) + c M_L)^{-1} (F(f) + load) with Dirichlet elimination (c = solver.reaction, 0 for the reference's
    problem).  Returns (u, state): the path object that keeps what the explicit adjoint needs.  node_major (2D paths):
    f, load and u are (n, B), the solver's own layout: no layout change (with B a valid padded batch and zero Dirichlet
    data, u IS the solver's iterate).  dirichlet: per-call Dirichlet values (diffhe.dirichlet), None: the mesh's.
    shape: the state also keeps what the node-gradient kernel reads (diffhe.shape)."""
    plan: SolvePlan = solver._plan()
    call = _Call.of(solver, plan, kappa, f, load, node_major, dirichlet, shape)
    # a tensor coefficient (diffhe.aniso) always takes the general path, lattice meshes included (as with method="ell"):
    # the lattice fast path has no tensor assembly and no coarse re-discretisation of a tensor
    state = _begin_call(solver, plan, call, _EllSolve if call.nc else None)
    if plan.n_bc == 0 and call.reaction == 0.0:
        # K is singular (constants in its null space): the reference returns garbage of size 1e15 (solver.py:174),
        # the 1D scan NaN, the iterative paths stop at the iteration cap -- either way it is said out loud
        warnings.warn("diffhe: the system is singular (pure Neumann problem: no Dirichlet node, no reaction term); "
                      "the returned values are not a solution", RuntimeWarning)
    return _run_call(state, call), state


def _from_node_major(eng, x, B, Bp, n, node_major, bc=None):
    """u in the caller's layout from the eliminated-system solution x (n, Bp), Dirichlet values added.  bc: per-call
    Dirichlet data, written into the Dirichlet rows of a buffer of its own (x stays the private iterate)."""
    p = eng.p
    if bc is not None:
        if node_major:
            u = (x if Bp == B else x[:, :B]).clone(memory_format=torch.contiguous_format)
            eng.bc_scatter(bc, u, B, 1, B)
        else:
            u = eng.to_sample_major(x, B, Bp, n)
            eng.bc_scatter(bc, u, 1, n, B)
        return u
    if not node_major:
        return eng.to_sample_major(x, B, Bp, n, add=p.g)
    xo = x if Bp == B else x[:, :B]
    return xo + p.g.unsqueeze(1) if p.has_dirichlet_data else xo   # zero Dirichlet data: u IS x, nothing is copied


def _adjoint_grads(state: _PathSolve, gbar, need_k, need_f, need_load, need_g=False):
    """The path's adjoint ONCE for the cotangent `gbar` of u, then the gradients of the inputs every solve op has, shaped,
    summed over the batch where the input had none, and placed like the inputs.  A call with `dirichlet=` has its band step
    here (diffhe.dirichlet: dL/dG and the G part of dL/dkappa), between the two: it corrects the per-sample and
    per-element dL/dkappa BEFORE they are summed into the shape of kappa.
    Returns (lambda in the path's layout, grad_kappa, grad_f, grad_load, grad_G), None for each gradient not asked for."""
    call, plan = state.call, state.plan
    g = gbar.detach().to(plan.device, torch.float64)
    g = g.reshape(plan.n, call.B) if call.node_major else g.reshape(call.B, plan.n).contiguous()
    lam, dk_sample, dk_elem, df, dload = state.adjoint(g, need_k, need_f, need_load)
    dg = None
    if call.bc is not None:
        dk_sample, dg = _dirichlet.band_grads(state, g, lam, dk_sample, dk_elem, need_k, need_g)
    grad_k = grad_f = grad_load = grad_g = None
    if need_k:
        grad_k = dk_elem.reshape(call.kappa_shape) if call.nc else _kappa_grad(call.mode, call.kappa_shape, dk_sample, dk_elem)
        grad_k = grad_k.to(call.kappa_device)
    if need_f:
        grad_f = (df if call.batched else df.sum(dim=0)).to(call.out_device)
    if need_load:
        grad_load = (dload if call.load_batched else dload.sum(dim=1 if call.node_major else 0)).to(call.out_device)
    if need_g:      # a (n_D,) G shared by the batch receives the sum over the samples
        grad_g = dg if call.bc[0].dim() == 2 else dg.sum(dim=1 if call.node_major else 0)
    return lam, grad_k, grad_f, grad_load, grad_g


def _solve_backward(state: _PathSolve, gbar, need_k, need_f, need_load=False, need_g=False, need_x=False):
    """Explicit adjoint: lambda = K_free^{-1} gbar_free with the saved operators,
    dL/dkappa = -lambda^T k0 u, dL/df = M^T lambda, dL/dload = lambda, dL/dG (`_adjoint_grads`: the path's adjoint ONCE),
    then what the same lambda gives for the node coordinates (diffhe.shape; dL/dX stays (n, dim) fp64 on the plan's
    device: the mesh's nodes may live elsewhere).
    Returns (grad_kappa, grad_f, grad_load, grad_G, grad_X), None for each one not asked for."""
    lam, *grads = _adjoint_grads(state, gbar, need_k, need_f, need_load, need_g)
    return (*grads, _shape._node_grad(state, lam) if need_x else None)


# ---------------------------------------------------------------------------------------------
# torch.library custom ops: diffhe::fe_solve (forward) and diffhe::fe_solve_backward (adjoint).
# Non-tensor context (the solver, the per-call adjoint state) travels as integer handles.  The registries, the lifetime of
# a saved state and the shapes the ops return are here once, for the ops of diffhe.robin and diffhe.eigen too.
# ---------------------------------------------------------------------------------------------
_SOLVERS: "weakref.WeakValueDictionary[int, DifferentiableFESolver]" = weakref.WeakValueDictionary()
_STATES: Dict[int, object] = {}
_TOKENS = itertools.count(1)


class _StateGuard:
    """Owned by the autograd context of one differentiated solve: when the graph is freed (backward without
    retain_graph, or the output tensor dropped) the saved adjoint state goes with it -- the lifetime autograd gives
    its own saved tensors, so `backward(retain_graph=True)`, repeated backward passes and gradcheck work."""

    def __init__(self, token: int):
        self.token = token

    def __del__(self):
        _STATES.pop(self.token, None)


def _state_of(token: torch.Tensor):
    state = _STATES.get(int(token))
    if state is None:
        raise RuntimeError("diffhe: adjoint state of this solve is gone (its autograd graph was freed)")
    return state


def _register_state(state, save: bool) -> torch.Tensor:
    """The token a forward op returns: it names `state` in `_STATES` until the autograd graph of the call is freed
    (`_tie_state`: no cap on pending solves); 0, and nothing kept, when `save` is false."""
    token = next(_TOKENS) if save else 0
    if save:
        _STATES[token] = state
    return torch.tensor(token, dtype=torch.int64)


def _tie_state(ctx, token: torch.Tensor, *saved) -> None:
    """For a `setup_context`: save (token, *saved) for backward and tie the adjoint state that `token` names to them."""
    real = not isinstance(token, torch._subclasses.FakeTensor)
    # A sentinel among the saved tensors dies with them at the end of a backward that does not retain the graph and
    # takes the adjoint state along, BEFORE the caller lets go of u: a state that overlaps the next step's forward
    # solve costs new device allocations ("Lifetime of the adjoint state").  It stays LAST: the
    # backward functions read `ctx.saved_tensors[:k]`.
    sentinel = (torch.empty(0),) if real else ()
    ctx.save_for_backward(token, *saved, *sentinel)
    if real:
        weakref.finalize(sentinel[0], _STATES.pop, int(token), None)
        ctx.state_guard = _StateGuard(int(token))           # and in any case together with the graph


def _fake_solve(solver, kappa, f, node_major):
    """(u, token) of a forward op's fake (meta) implementation."""
    token = torch.empty((), dtype=torch.int64)
    if node_major:
        return f.new_empty(tuple(f.shape), dtype=torch.float64), token
    n, m = solver.mesh.n_nodes, solver.mesh.n_elements
    _, B, _ = _kappa_layout(kappa, m, f.shape[0] if f.dim() == 2 else None, False, solver._tensor_components())
    return f.new_empty((B, n) if (f.dim() == 2 or B > 1) else (n,), dtype=torch.float64), token


def _like_grads(gbar, grads, likes):
    """What a backward op returns: each gradient with the device and dtype of its `*_like`, an empty tensor for None."""
    return tuple(gbar.new_empty(0) if g is None else g.to(like.device, like.dtype) for g, like in zip(grads, likes))


def _fake_grads(gbar, needs, likes):
    """`_like_grads` for a backward op's fake (meta) implementation."""
    return tuple(torch.empty_like(like) if need else gbar.new_empty(0) for need, like in zip(needs, likes))


def _fe_setup_context(ctx, inputs, output):
    """Save (token, kappa, f, load, dirichlet | None, nodes | None) and u when node-major (it may BE the saved iterate:
    autograd then refuses a backward after an in-place edit), and tie the adjoint state to them."""
    kappa, f, load, handle, _save, node_major, dirichlet, nodes, _version = inputs
    ctx.handle, ctx.node_major = handle, bool(node_major)
    _tie_state(ctx, output[1], kappa, f, load, dirichlet, nodes, *((output[0],) if node_major else ()))


@torch.library.custom_op("diffhe::fe_solve", mutates_args=())
def fe_solve(kappa: torch.Tensor, f: torch.Tensor, load: torch.Tensor, handle: int, save: bool, node_major: bool = False,
             dirichlet: Optional[torch.Tensor] = None, nodes: Optional[torch.Tensor] = None,
             nodes_version: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u, token) = solve with the solver registered under `handle`; `token` names the saved
    adjoint state (0 when `save` is false).  `load`: extra nodal load vector, empty for none.
    node_major: f, load and u are (n, B) instead of (B, n).
    dirichlet: the Dirichlet values of this call, (n_D,), (B, n_D), or (n_D, B) when node_major; None: the mesh's.
    nodes: the node coordinates as a differentiable input -- the solver's mesh.nodes at version `nodes_version` (the
    tensor the plan is built from); None: no node gradient."""
    solver = _SOLVERS[handle]
    if nodes is not None:
        _shape._check_nodes(solver.mesh, nodes, nodes_version)
    u, state = _solve_forward(solver, kappa, f, load, node_major, dirichlet, nodes is not None)
    return u, _register_state(state, save)


@fe_solve.register_fake
def _fe_solve_fake(kappa, f, load, handle, save, node_major=False, dirichlet=None, nodes=None, nodes_version=0):
    return _fake_solve(_SOLVERS[handle], kappa, f, node_major)


_Grads = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]


@torch.library.custom_op("diffhe::fe_solve_backward", mutates_args=())
def fe_solve_backward(gbar: torch.Tensor, token: torch.Tensor, need_k: bool, need_f: bool, need_load: bool,
                      need_g: bool, need_x: bool, kappa_like: torch.Tensor, f_like: torch.Tensor, load_like: torch.Tensor,
                      g_like: Optional[torch.Tensor] = None, nodes_like: Optional[torch.Tensor] = None) -> _Grads:
    """(dL/dkappa, dL/df, dL/dload, dL/dG, dL/dX) of the forward call named by `token` from ONE adjoint solve, each with
    the device and dtype of its `*_like`; unused gradients come back empty."""
    grads = _solve_backward(_state_of(token), gbar, need_k, need_f, need_load, need_g, need_x)
    return _like_grads(gbar, grads, (kappa_like, f_like, load_like, g_like, nodes_like))


@fe_solve_backward.register_fake
def _fe_solve_backward_fake(gbar, token, need_k, need_f, need_load, need_g, need_x, kappa_like, f_like, load_like,
                            g_like=None, nodes_like=None):
    return _fake_grads(gbar, (need_k, need_f, need_load, need_g, need_x),
                       (kappa_like, f_like, load_like, g_like, nodes_like))


def _element_forms(plan: SolvePlan):
    """Unit-kappa element stiffness and load matrices (m, npe, npe) and the (m, npe) connectivity, as torch tensors
    built from the plan's coordinates -- the differentiable restatement of reference solver.py:86-96 (1D) and :125-145
    (2D P1), and of the P1 tetrahedra of csrc/ell_assemble.hip (3D), used by the second-order path only."""
    cached = plan.__dict__.get("_element_forms")
    if cached is not None:
        return cached
    if plan.npe != plan.dim + 1:
        raise NotImplementedError("diffhe: second-order derivatives are implemented for P1 elements only")
    el = plan.elems.long().t().contiguous()                          # (m, npe)
    X = plan.coords.to(torch.float64)                                # (dim, n)
    if plan.dim == 1:
        h = (X[0][el[:, 1]] - X[0][el[:, 0]]).abs()
        k0 = torch.tensor([[1.0, -1.0], [-1.0, 1.0]], dtype=torch.float64, device=h.device)[None] / h[:, None, None]
        m0 = torch.eye(2, dtype=torch.float64, device=h.device)[None] * (0.5 * h)[:, None, None]
    elif plan.dim == 3:
        P = X.t()[el]                                                # (m, 4, 3)
        a, b, c = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], P[:, 3] - P[:, 0]
        g1, g2, g3 = torch.cross(b, c, dim=1), torch.cross(c, a, dim=1), torch.cross(a, b, dim=1)
        G = torch.stack([-(g1 + g2 + g3), g1, g2, g3], 1)            # (m, 4, 3): 6 V grad phi_p
        det = (a * g1).sum(1)
        l2 = torch.maximum(torch.maximum((a * a).sum(1), (b * b).sum(1)), (c * c).sum(1))
        keep = det.abs() > 1e-12 * (l2 * l2.sqrt())                  # degenerate tetrahedra: nothing, as in ell_assemble.hip
        safe = torch.where(keep, det.abs(), torch.ones_like(det))
        zero = torch.zeros((), dtype=torch.float64, device=det.device)
        k0 = torch.where(keep[:, None, None], G @ G.transpose(1, 2) / (6.0 * safe)[:, None, None], zero)
        m0 = torch.where(keep[:, None, None], (safe / 96.0)[:, None, None].expand(-1, 4, 4), zero).contiguous()
    else:
        x, y = X[0][el], X[1][el]                                    # (m, 3)
        b = torch.stack([y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]], 1)
        c = torch.stack([x[:, 2] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 0]], 1)
        area = 0.5 * ((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])).abs()
        # degenerate triangles are skipped silently, as in the reference (solver.py:120-121), the first-order kernels
        # (ell_assemble.hip) and plan.py: no contribution to K or F instead of a division by ~0
        keep = (area >= 1e-15)[:, None, None]
        safe = torch.where(area >= 1e-15, area, torch.ones_like(area))
        k0 = torch.where(keep, (b[:, :, None] * b[:, None, :] + c[:, :, None] * c[:, None, :]) / (4.0 * safe)[:, None, None],
                         torch.zeros((), dtype=torch.float64, device=area.device))
        m0 = torch.where(keep, (safe / 9.0)[:, None, None].expand(-1, 3, 3), torch.zeros((), dtype=torch.float64,
                                                                                      device=area.device)).contiguous()
    plan.__dict__["_element_forms"] = (el, k0, m0)
    return el, k0, m0


def _second_order_backward(ctx, grad_u, need_k, need_f, need_load):
    """The adjoint written with differentiable pieces, for backward(create_graph=True) / Hessian-vector products:

        lambda = A(kappa)^-1 gbar          a solve of the SAME solver class on the mesh with homogeneous Dirichlet data
                                           (gbar enters as `load`: rows of Dirichlet nodes dropped), itself differentiable;
        u      = the forward solve again   (recorded this time: the first one's graph ends at the custom op);
        dL/dkappa_e = - lambda_e^T k0_e u_e,   dL/df = M^T lambda,   dL/dload = lambda      plain torch gathers / sums.

    Costs two HIP solves per first-order gradient instead of one, and element-local torch temporaries of (B, m, npe):
    meant for the sizes Hessian-vector products are taken at, not for the first-order hot path (which never comes here).
    Each further derivative of the result runs the explicit adjoint of those two solves (or, with create_graph again,
    this function recursively)."""
    solver = _SOLVERS.get(ctx.handle)
    if solver is None:
        raise RuntimeError("diffhe: the solver of this solve is gone; second-order backward needs it alive")
    _token, kappa, f, load, dirichlet = ctx.saved_tensors[:5]
    node_major = ctx.node_major
    plan = solver._plan()
    el, k0, m0 = _element_forms(plan)
    m, n = plan.m, plan.n
    twin = solver._adjoint_twin()
    _SOLVERS[id(twin)] = twin
    g = grad_u.to(torch.float64)
    lam, _ = torch.ops.diffhe.fe_solve(kappa, torch.zeros_like(g), g, id(twin), True, node_major)
    # per-call Dirichlet data is not differentiated here (`_fe_backward` refuses second order through it)
    u, _ = torch.ops.diffhe.fe_solve(kappa, f, load, ctx.handle, True, node_major,
                                     None if dirichlet is None else dirichlet.detach())
    # (B, n) views for the element-local maps
    lam_b = (lam.t() if node_major else lam).reshape(-1, n)
    u_b = (u.t() if node_major else u).reshape(-1, n)
    B = lam_b.shape[0]
    gk = gf = gl = None
    if need_k:
        mode, _, kappa_em = _kappa_layout(kappa, m, B if f.dim() == 2 else None, node_major)
        s_be = -torch.einsum("bep,epq,beq->be", lam_b[:, el], k0, u_b[:, el])      # (B, m)
        gk = _kappa_grad(mode, kappa.shape, per_elem=s_be.t() if kappa_em else s_be)
    if need_f:
        y = torch.einsum("epq,beq->bep", m0, lam_b[:, el])                          # M^T lambda, M symmetric per element
        gf_b = torch.zeros_like(lam_b).index_add_(1, el.reshape(-1), y.reshape(B, -1))
        gf = (gf_b.t() if node_major else gf_b).reshape(f.shape) if f.dim() == lam.dim() else gf_b.sum(0).reshape(f.shape)
    if need_load:
        gl = lam.reshape(load.shape) if load.dim() == lam.dim() else lam_b.sum(0).reshape(load.shape)
    return gk, gf, gl


_GRAD_ARGS = (0, 1, 2, 6, 7)      # kappa, f, load, dirichlet, nodes among the arguments of diffhe::fe_solve


def _input_grads(needs_input_grad, grads=None):
    """`needs_input_grad` has one entry per argument that REACHED the op -- the dispatcher drops trailing arguments equal
    to their defaults, so a call without dirichlet / nodes sees 5 or 6 of the schema's 9 -- and autograd wants as many
    values back.  Without `grads`: (need_k, need_f, need_load, need_g, need_x), False for what was not passed; with
    them: the five gradients placed among that many values, None where not needed."""
    n = len(needs_input_grad)
    needs = tuple(i < n and needs_input_grad[i] for i in _GRAD_ARGS)
    if grads is None:
        return needs
    out = [None] * n
    for i, need, g in zip(_GRAD_ARGS, needs, grads):
        if need:
            out[i] = g
    return tuple(out)


def _fe_backward(ctx, grad_u, _grad_token):
    need_k, need_f, need_load, need_g, need_x = _input_grads(ctx.needs_input_grad)
    if torch.is_grad_enabled():
        # backward(create_graph=True) / autograd.grad(..., create_graph=True): the caller wants a gradient it can
        # differentiate again.  The explicit adjoint below is not recorded by autograd (what it returns would carry no
        # graph, a Hessian-vector product through it would silently be zero): take the differentiable restatement.
        if need_x:
            raise NotImplementedError("diffhe: second-order derivatives through the node coordinates are not "
                                      "implemented (backward with create_graph=True while mesh.nodes requires grad)")
        if need_g:
            raise NotImplementedError("diffhe: second-order derivatives through the Dirichlet values are not implemented "
                                      "(backward with create_graph=True while dirichlet= requires grad)")
        solver = _SOLVERS.get(ctx.handle)
        if solver is not None and solver._tensor_components():
            raise NotImplementedError("diffhe: second-order derivatives of a solve with a conductivity tensor are not "
                                      "implemented (backward with create_graph=True, diffhe.aniso)")
        grads = _second_order_backward(ctx, grad_u, need_k, need_f, need_load)
    else:
        token, kappa, f, load, dirichlet, nodes = ctx.saved_tensors[:6]
        grads = torch.ops.diffhe.fe_solve_backward(grad_u, token, need_k, need_f, need_load, need_g, need_x, kappa, f,
                                                   load, dirichlet, nodes)
    return _input_grads(ctx.needs_input_grad, grads)


torch.library.register_autograd("diffhe::fe_solve", _fe_backward, setup_context=_fe_setup_context)


class DifferentiableFESolver(nn.Module):
    """Assemble and solve the P1 system of a mesh for a forcing (reference solver.py:21-43).

    Parameters
    ----------
    mesh : FEMesh
    kappa : float or torch.Tensor -- diffusion coefficient (see module docstring).
    device, tol, max_iter, check_every, assembly, method, mg, chain : HIP-path knobs (ours; the
        reference has none).  `assembly` is "gather" (deterministic) or "atomic" (general
        path); `method="ell"` forces the general ELL path on lattice meshes; `mg` overrides
        the multigrid parameters (nu, n_coarse, omega) of the lattice path.
    """

    _dims = (1, 2)        # mesh dimensions forward() accepts: the reference's (diffhe.tet3d adds 3)

    def __init__(self, mesh: FEMesh, kappa: float = 1.0, *, device=None, tol: Optional[float] = None,
                 max_iter: int = 20000, check_every: int = 25, assembly: str = "gather", method: str = "auto",
                 mg: Optional[dict] = None, chain: str = "reference", warm_start=False, reaction: float = 0.0,
                 operator: str = "auto", amg: Optional[dict] = None):
        super().__init__()
        self.mesh = mesh
        if isinstance(kappa, (int, float)):
            self._kappa = torch.tensor(kappa, dtype=torch.float64)        # reference solver.py:36-37
        else:
            self._kappa = kappa.to(dtype=torch.float64)                  # reference solver.py:38-39
        if assembly not in ("gather", "atomic"):
            raise ValueError(f"Unknown assembly: {assembly!r}")
        if method not in ("auto", "ell", "ell-jacobi"):
            raise ValueError(f"Unknown method: {method!r}")
        if chain not in ("reference", "exact"):
            raise ValueError(f"Unknown chain mode: {chain!r}")
        if operator not in ("auto", "assembled"):
            raise ValueError(f"Unknown operator: {operator!r}")
        # 2D lattices with one scalar kappa per sample (or for all): "auto" keeps the operator FACTORED on closed
        # lattices, K_b = kappa_b K_1 -- no matrix traffic, but not the matrix the reference assembles: its entries
        # fl(sum_e fl(fl(kappa_b t_e) / den_e)) carry roundings that depend on kappa_b, and the two solutions differ by
        # ~cond * eps (1024^2: 3e-11 in u, 8e-11 in dL/dkappa -- inside the 1e-10 tolerance, measured against the
        # refined oracle).  "assembled" stores one matrix per sample in the reference's operation
        # order (bit-identical to its K): ~1e-12 from the refined oracle, at per-element-kappa speed.
        self.operator = operator
        # 1D chains: "reference" reproduces the solution of the matrix the reference assembles in fp64 (its rounded
        # diagonal costs 4e-10 in u at 10^4 elements); "exact" is the plain scan, 1e-15 from the exact solution of the
        # unrounded system and ~1.5x faster
        self.chain = chain
        # reaction >= 0 (ours; the reference solves pure diffusion): the problem becomes -div(kappa grad u) + c u = f,
        # discretised as (K + c M_L) u = F with the LUMPED mass M_L = row sums of the reference's load matrix
        # (solver.py:95-96, :143-145).  One backward-Euler step of the heat equation is this with c = 1 / dt
        # (diffhe/heat.py).  A fixed number, not differentiated.
        if not (float(reaction) >= 0.0):
            raise ValueError(f"reaction must be >= 0, got {reaction!r}")
        self.reaction = float(reaction)
        # warm_start (lattice path): the forward and the adjoint solve start from the previous solution on this mesh
        # and batch size (kept on the mesh's plan, so a loop that builds a new solver per step -- the reference's
        # pattern -- still benefits), corrected by one full-multigrid pass on its residual.  For optimisation loops
        # whose kappa moves a little per step; results meet the same stopping rule, only the iteration count changes.
        # Costs two (n, B) fp64 vectors of device memory per mesh; `plan.warm.clear()` drops them.
        # "forward": only the forward solve (an adjoint right-hand side that changes direction from step to step, as
        # the data misfit of an inverse problem does near its minimum, makes a poor guess: config 5 took 3.6 + 6.3
        # iterations warm against 5 + 5 cold, 3.6 + 5 with "forward").
        if warm_start not in (False, True, "forward"):
            raise ValueError(f"Unknown warm_start: {warm_start!r}")
        self.warm_start = warm_start
        # "ell": general path (aggregation-AMG PCG) even on lattice meshes; "ell-jacobi": general path
        # with the plain Jacobi preconditioner
        self.method = method
        # aggregation AMG of the general path: V-cycle (gamma = 1) with the coarse correction scaled by 1.8
        # (over-correction compensates the piecewise-constant interpolation; < 2 keeps the cycle a contraction)
        # fp32 = 1 stores the cycle's vectors (and reads copies of per-sample matrix values) in fp32, like mg["fp32"]:
        # +13 % on benign fields, but OFF by default -- this cycle is a much weaker preconditioner than the geometric one
        # (50-250 iterations), and on high-contrast fields (kappa spanning 1e5) the fp32 roundings inside it stall or
        # break the CG long before 1e-14 (randomised sweep: 2000 iterations, diverging samples; fp64 cycle: 123)
        # max_iter: this cycle's iteration counts grow with coefficient contrast and element anisotropy (78 on a benign
        # 84k-node mesh, 4467 on an 86k-node one with an iid e^-4..e^4 field per sample and 6:1 elements, randomised sweep
        # seed 802 case 6) but the CG keeps converging; a cap of 2000 left that case at 2e-9.
        # smoothed = 1 (round 3): smoothed aggregation -- the prolongation of the same aggregates smoothed by one damped
        # Jacobi step of the unit-kappa operator (batch-shared), coarse operators as weighted Galerkin sums per sample:
        # about half the iterations of the piecewise-constant hierarchy (512^2 through this path: 82 -> see DESIGN);
        # scale None = 1.3 smoothed / 1.8 piecewise constant
        # strength = theta > 0 (opt-in, absent = 0): aggregates and prolongation from the operator being solved instead of
        # the unit-kappa one -- strong couplings c_ij >= theta max_k c_ik, theta halved per level; the hierarchy is kept on
        # this solver (`refresh_hierarchy`, refresh = k: rebuilt every k-th call, 0 = never).  For anisotropic tensors
        # and scalar fields of high contrast ("Coefficient-aware hierarchy")
        self.amg = dict(n_coarse=16, gamma=None, scale=None, fp32=0, max_iter=20000, smoothed=1)   # gamma None: 1, or 2 on big problems
        for item in filter(None, os.environ.get("DIFFHE_AMG", "").split(",")):  # e.g. "scale=1.0,gamma=2,max_iter=20000"
            key, val = item.split("=")
            self.amg[key] = float(val) if key in ("scale", "strength") else int(val)
        self.amg.update(amg or {})
        self._amg_user = set((amg or {}).keys()) | {i.split("=")[0] for i in os.environ.get("DIFFHE_AMG", "").split(",") if i}
        # fp32 = 1: the V-cycle (a preconditioner) STORES its vectors in fp32; all arithmetic, the
        # outer CG, its residual, the solution and every dot product stay fp64 (same 1e-10 parity)
        # fmg = 1: the CG starts from a full-multigrid iterate instead of 0 (3 iterations fewer at 1024^2)
        # floor = 1: the stop is `tol` or half the residual level fp64 can attain (u |A| |x|), whichever is larger
        # tol_energy: per sample the CG also stops once the ESTIMATED relative energy-norm error of the iterate,
        # sqrt(r.z / u^T A u) (r.z is the dot the CG computes anyway; with a multigrid preconditioner it is e^T A e),
        # is below it.  Nodal values and per-element gradients -- what the 1e-10 parity tolerance is stated in -- are
        # bounded by the energy norm far more tightly than by the residual: on the 1024^2 bench workload the
        # estimate is 3-10x ABOVE the measured nodal error at every iteration (2.6e-11 vs 7.8e-12 after 5), while the
        # relative residual is still 6e-9 there.  1e-11 leaves >= 10x to the tolerance; 0 turns the criterion off.
        self.mg = dict(nu=2, n_coarse=8, omega=0.8, omegas=None, fp32=1, fmg=1, floor=1, tol_energy=1e-11)
        for item in filter(None, os.environ.get("DIFFHE_MG", "").split(",")):   # e.g. "nu=1,omega=0.85"
            key, val = item.split("=")
            if key == "omegas":
                self.mg[key] = [float(v) for v in val.split(":")]
            else:
                self.mg[key] = float(val) if key in ("omega", "tol_energy") else int(val)
        self.mg.update(mg or {})
        self._mg_user = set((mg or {}).keys()) | {i.split("=")[0] for i in os.environ.get("DIFFHE_MG", "").split(",") if i}
        self._device = device
        if os.environ.get("DIFFHE_TOL"):
            tol = float(os.environ["DIFFHE_TOL"])
        # relative-residual stop; None = chosen per mesh at the first solve (1e-12 or 1e-13, see _call_options)
        self._tol_user = tol
        self.tol, self.max_iter, self.check_every, self.assembly = tol, max_iter, check_every, assembly
        self.last_info = SolveInfo()
        self._hier_lock = threading.Lock()
        self._hier_cache: Dict[tuple, dict] = {}

    def refresh_hierarchy(self) -> None:
        """Drop the coefficient-aware hierarchies this solver keeps (amg=dict(strength=theta)): the next general-path call
        builds one from its own operator.  Adjoint states of earlier calls keep the hierarchy they solved with."""
        with self._hier_lock:
            self._hier_cache.clear()

    def _hierarchy_levels(self, plan: SolvePlan, theta: float, refresh: int, build):
        """(levels, (n_levels, operator complexity), age) of the operator hierarchy for (plan, theta): cached under the
        solver's lock, `build()` on the first call and -- refresh = k > 0 -- again once k calls have used it."""
        key = (id(plan), float(theta), True)
        with self._hier_lock:
            ent = self._hier_cache.get(key)
            if ent is not None and ent["plan"] is plan:
                ent["age"] += 1
                if not (refresh > 0 and ent["age"] >= refresh):
                    return ent["levels"], ent["stats"], ent["age"]
            while len(self._hier_cache) >= 4:
                self._hier_cache.pop(next(iter(self._hier_cache)))
            levels, stats = build()
            self._hier_cache[key] = dict(plan=plan, levels=levels, stats=stats, age=0)
            return levels, stats, 0

    @property
    def kappa(self) -> torch.Tensor:
        return self._kappa

    def _plan(self) -> SolvePlan:
        return get_plan(self.mesh, _resolve_device(self._device))

    def _tensor_components(self) -> int:
        """Voigt components of the coefficient when it is a conductivity tensor (diffhe.aniso), 0 for a scalar kappa."""
        return 0

    def _adjoint_twin(self) -> "DifferentiableFESolver":
        """This solver on the same mesh with HOMOGENEOUS Dirichlet data: u = A^-1 load, the adjoint solve as a
        differentiable call (second-order path).  Built once per solver; options are re-read at every use."""
        twin = self.__dict__.get("_twin")
        if twin is None:
            mesh0 = self.mesh.__dict__.get("_diffhe_zero_twin")
            if mesh0 is None:
                mesh0 = FEMesh(nodes=self.mesh.nodes, elements=self.mesh.elements,
                               dirichlet_nodes={k: 0.0 for k in self.mesh.dirichlet_nodes})
                self.mesh.__dict__["_diffhe_zero_twin"] = mesh0
            twin = type(self)(mesh0, self._kappa, device=self._device)
            self.__dict__["_twin"] = twin
        for name in ("tol", "_tol_user", "max_iter", "check_every", "assembly", "method", "chain", "warm_start",
                     "reaction", "operator", "_mg_user", "_amg_user"):
            setattr(twin, name, getattr(self, name))
        twin.mg, twin.amg, twin.warm_start = dict(self.mg), dict(self.amg), False
        return twin

    def forward(self, f: torch.Tensor, load: Optional[torch.Tensor] = None, layout: str = "sample",
                dirichlet: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Solve for nodal u.  f: (n,), (n,1) or (B,n); returns float64 (n,) or (B,n)
        on f's device (reference solver.py:49-67 returns CPU float64).
        load (ours): (n,) or (B,n) nodal load added to the assembled load vector F on the free rows (differentiable) --
        the M_L u_prev / dt term of a time step, point sources, a Neumann flux integrated by the caller.
        layout (ours): "sample" = the shapes above; "node" = f, load and u are (n, B), the batch INNERMOST -- the layout
        the kernels work in, so a caller that keeps its batch that way (an optimisation loop over kappa, say) pays no
        transposing pass in or out (3 x 16 B per node and sample of a fwd + adjoint step); 2D meshes, same results.
        dirichlet (ours): the Dirichlet values of this call in ascending node-id order (`mesh.dirichlet_index()`),
        (n_D,) for the batch or (B, n_D) per sample -- (n_D,) or (n_D, B) with layout="node"; batch rules of `load`.
        The values of `mesh.dirichlet_nodes` are then not used, only its keys; the solve plan is the same, and the
        values may require grad (a shared (n_D,) tensor receives the sum over the batch).  See diffhe.dirichlet."""
        f64, load64, node_major, transposed = self._checked_inputs(f, load, layout)
        if transposed:      # the 1D scan works sample-major: transposing views in and out
            g64 = None if dirichlet is None else self._dirichlet64(dirichlet, f.shape[1], True)
            return self.forward(f.t(), None if load is None else load.t(),
                                dirichlet=g64 if g64 is None or g64.dim() == 1 else g64.t()).t()
        g64 = None
        if dirichlet is not None:
            g64 = self._dirichlet64(dirichlet, f64.shape[1 if node_major else 0] if f64.dim() == 2 else None, node_major)
            if g64.dim() == 2 and f64.dim() == 1:                           # a (B, n_D) G implies the batch, like load
                f64 = f64.reshape(1, -1).expand(g64.shape[0], -1)
        return self._solve_op(f64, load64, g64, node_major)

    def _checked_inputs(self, f, load, layout: str, dims: str = "1D and 2D"):
        """f, load and layout of a `forward` call checked -> (f64, load64, node_major, transposed): float64 tensors,
        load64 empty for no load, a (B, n) load having given its batch to an f without one.  transposed: layout="node" on
        a 1D mesh, whose paths work sample-major -- nothing is converted, the caller calls `forward` again on transposed
        views and transposes what comes back."""
        if self.mesh.dim not in self._dims:
            raise NotImplementedError(f"Only {dims} supported")         # reference solver.py:67
        if layout not in ("sample", "node"):
            raise ValueError(f"Unknown layout: {layout!r}")
        n = self.mesh.n_nodes
        if layout == "node":
            if f.dim() != 2 or f.shape[0] != n or (load is not None and tuple(load.shape) != tuple(f.shape)):
                raise ValueError(f"layout='node': f (and load) must be (n, B) with n={n}, got {tuple(f.shape)}")
            if self.mesh.dim == 1:
                return None, None, True, True
            f64 = f.to(torch.float64)
            return f64, f64.new_empty(0) if load is None else load.to(torch.float64), True, False
        f64 = f.to(torch.float64)
        if f64.dim() == 2 and f64.shape == (n, 1):
            f64 = f64.reshape(n)                                          # (n,1) works in the reference too
        elif f64.dim() == 2 and f64.shape[1] != n:
            raise ValueError(f"f must be (n,) or (B,n) with n={n}, got {tuple(f.shape)}")
        elif f64.dim() == 1 and f64.shape[0] != n:
            raise ValueError(f"f must have {n} nodal values, got {f64.shape[0]}")
        if load is None:
            return f64, f64.new_empty(0), False, False
        load64 = load.to(torch.float64)
        if load64.shape[-1] != n or load64.dim() not in (1, 2):
            raise ValueError(f"load must be (n,) or (B,n) with n={n}, got {tuple(load.shape)}")
        if load64.dim() == 2 and f64.dim() == 1:
            f64 = f64.reshape(1, n).expand(load64.shape[0], n)
        return f64, load64, False, False

    def _dirichlet64(self, dirichlet, B: Optional[int], node_major: bool) -> torch.Tensor:
        """`dirichlet=` checked and as float64: (n_D,), or (B, n_D) / layout="node" (n_D, B) with B the batch of f (None:
        f has none, any B)."""
        nd = len(self.mesh.dirichlet_nodes)
        g = dirichlet if isinstance(dirichlet, torch.Tensor) else torch.as_tensor(dirichlet)
        if g.is_complex():
            raise ValueError(f"dirichlet must be a real tensor, got {g.dtype}")
        if g.dim() == 1:
            ok = g.shape[0] == nd
        elif g.dim() == 2:
            gb, gn = (g.shape[1], g.shape[0]) if node_major else (g.shape[0], g.shape[1])
            ok = gn == nd and (B is None or gb == B)
        else:
            ok = False
        if not ok:
            want = f"({nd},) or " + (f"({nd}, B)" if node_major else f"(B, {nd})") + (f" with B={B}" if B else "")
            raise ValueError(f"dirichlet must be {want} (one value per Dirichlet node), got {tuple(g.shape)}")
        return g.to(torch.float64)

    def _solve_op(self, f64: torch.Tensor, load64: torch.Tensor, g64: Optional[torch.Tensor],
                  node_major: bool) -> torch.Tensor:
        """u = the diffhe::fe_solve op on checked float64 inputs (load64 empty: no extra load; g64: `dirichlet=` or None)."""
        _SOLVERS[id(self)] = self
        save = torch.is_grad_enabled() and (self._kappa.requires_grad or f64.requires_grad or load64.requires_grad
                                            or (g64 is not None and g64.requires_grad))
        u, _token = torch.ops.diffhe.fe_solve(self._kappa, f64, load64, id(self), save, node_major, g64)
        return u

    # reference-private names kept as aliases; both run the HIP path
    def _solve_1d(self, f: torch.Tensor) -> torch.Tensor:
        return self.forward(f)

    def _solve_2d(self, f: torch.Tensor) -> torch.Tensor:
        return self.forward(f)


# The two steps of `_solve_backward` that live with their derivations (and `_check_nodes`).  Both modules import this one,
# hence at the end; their functions are looked up at call time.
from . import dirichlet as _dirichlet, shape as _shape  # noqa: E402
