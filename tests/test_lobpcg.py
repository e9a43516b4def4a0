"""The opt-in LOBPCG outer iteration of `EigenFESolver`, `ElasticEigenSolver` and `LinearBucklingSolver`
(iteration="lobpcg": diffhe.eigen._BlockRun, csrc/lobpcg.hip, include/diffhe_lobpcg.h).

The yardsticks are the dense restatements of tests/test_eigen.py, tests/test_modal.py and tests/test_buckling.py, imported
with their cases and checking helpers, and for the iteration itself the numpy statement of tests/_lobpcg_model.py, which is
pinned here against `numpy.linalg.eigh`.

Tolerances, with their reasons:
  * the model on a 40 x 40 pencil: 1e-12 of max|theta| -- the error of a Ritz value is the square of its vector's, and the
    model stops on a residual of 1e-9 relative to |A x| + |theta| |B x|;
  * Gram and rotation entries alone: 1e-12 relative to the largest reference entry -- sums of at most 48 (rotation) or 37
    (Gram) fp64 terms of order one;
  * the Ritz entry alone: C^T GB C = I and C^T GA C = diag(theta) to 1e-10 and theta to 1e-11 of max|theta| against numpy on
    the SCALED pencil: GB = D M D with cond(M) ~ 10 and D spanning four decades (cond(GB) ~ 1e8 before the scaling the
    kernel applies, ~ 10 after it), so what is left is the rounding of a 48 x 48 factorisation and ~10 Jacobi sweeps;
  * the solvers: the bounds of the files the cases come from (lambda to RTOL_U = 1e-10, modes to 10 tol lambda / gap,
    gradients at tol = 1e-11 to the same amplification) -- the stopping measures are the same under either iteration;
  * outer iterations: strictly fewer than "subspace" on the same call, and at most LOBPCG_CAPS[case]: the count measured on
    an MI355X x 1.5, rounded up -- the margin is for the seeded start block and the rounding of the inner solves elsewhere.
"""
import ctypes
import math
import os
import warnings

import numpy as np
import pytest
import torch

from diffhe import FEMesh, _hip
from diffhe import buckling, eigen
from _util import RTOL_GRAD, RTOL_U, rel_err
import _lobpcg_model as model
import test_buckling as tb
import test_eigen as te
import test_modal as tm
from test_elasticity import _rand
from test_stress import BY_VALUE, _declarations

T64 = torch.float64
DEV = "cuda:0"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffhe_lobpcg.h")
NAMES = ["diffhe_lobpcg_gram", "diffhe_lobpcg_gram_blocks", "diffhe_lobpcg_ritz", "diffhe_lobpcg_rotate"]
gpu = pytest.mark.gpu

# outer iterations of iteration="lobpcg" on the cases of tests/test_buckling.py (k = 3, guard = 4, tol = 1e-8) measured on an
# MI355X, and the caps: the measured count x 1.5, rounded up
LOBPCG_MEASURED = {"2d-axial-stress": 10, "2d-axial-strain": 10, "2d-shear-stress": 19, "2d-shear-strain": 20, "3d-axial": 9,
                   "3d-shear": 17}
LOBPCG_CAPS = {key: math.ceil(1.5 * count) for key, count in LOBPCG_MEASURED.items()}


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the numpy model of the iteration
# ---------------------------------------------------------------------------------------------------------------------
def _pencil(kind, n=40, seed=0):
    rng = np.random.default_rng(seed)

    def spd(decades):
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        return Q @ np.diag(np.logspace(0, decades, n)) @ Q.T

    B = spd(2)
    if kind == "spd":
        A = spd(3)
    else:
        A = rng.standard_normal((n, n))
        A = 0.5 * (A + A.T)
    L = np.linalg.cholesky(B)
    At = np.linalg.solve(L, np.linalg.solve(L, A).T)
    return A, B, np.linalg.eigh(0.5 * (At + At.T))[0], rng


@pytest.mark.parametrize("kind", ["spd", "indefinite"])
def test_model_reaches_eigh_on_a_random_pencil(kind):
    """A SPD with T = A^-1 (the mass-weighted solvers) and A indefinite with T = B^-1 (buckling: B = K)."""
    A, B, ref, rng = _pencil(kind)
    p = 4
    inv = np.linalg.inv(A if kind == "spd" else B)
    theta, X, its, sizes = model.lobpcg(A, B, rng.standard_normal((40, p)), T=lambda R: inv @ R, tol=1e-9, max_iter=300)
    print(kind, "iterations", its, "fallbacks", [s for s in sizes if s[0] != s[1]])
    assert its < 300 and sizes[0][0] == 2 * p and all(s[0] == 3 * p for s in sizes[1:])
    assert np.abs(theta - ref[:p]).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(X.T @ B @ X - np.eye(p)).max() <= 1e-10
    if kind == "indefinite":
        assert ref[0] < 0.0 < ref[-1]


def test_model_falls_back_when_P_is_linearly_dependent():
    A, B, ref, rng = _pencil("indefinite", seed=1)
    p = 4
    X0 = rng.standard_normal((40, p))
    inv = np.linalg.inv(B)
    # a P block that is a combination of the X and W blocks next to it: the Ritz step drops to [X | W] and returns exactly
    # what it returns on [X | W] alone
    W1 = inv @ (A @ X0 - B @ X0)
    S = np.concatenate([X0, W1, 2.0 * W1 - X0 @ np.ones((p, p))], axis=1)
    C, theta, used, flag = model.ritz(S.T @ A @ S, S.T @ B @ S, p)
    assert (used, flag) == (2 * p, 0) and np.all(C[2 * p:] == 0.0)
    Cw, thw, usedw, _ = model.ritz(S[:, :2 * p].T @ A @ S[:, :2 * p], S[:, :2 * p].T @ B @ S[:, :2 * p], p)
    assert usedw == 2 * p and np.array_equal(C[:2 * p], Cw) and np.array_equal(theta, thw)
    # and inside the iteration: a dependent P0 is handed in, the drop is recorded, eigh is still reached
    theta, X, its, sizes = model.lobpcg(A, B, X0, T=lambda R: inv @ R, tol=1e-9, max_iter=300, P0=np.tile(X0[:, :1], (1, p)))
    assert sizes[1] == (3 * p, 2 * p) and its < 300
    assert np.abs(theta - ref[:p]).max() <= 1e-12 * np.abs(ref).max()
    # a non-finite matrix and a singular X block: identity rotation and the flag
    G = S.T @ B @ S
    G[0, 0] = np.nan
    C, theta, used, flag = model.ritz(S.T @ A @ S, G, p)
    assert flag == 1 and np.array_equal(C[:p], np.eye(p)) and np.all(theta == 0.0)
    Z = np.concatenate([X0[:, :1]] * p, axis=1)
    assert model.ritz(Z.T @ A @ Z, Z.T @ B @ Z, p)[3] == 1


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the binding and the arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_fifteenth_signature_table_matches_the_fifteenth_header():
    decls = _declarations(HEADER)
    assert sorted(decls) == sorted(_hip.LOBPCG_SIGNATURES) == NAMES
    others = set()
    for table in ("SIGNATURES", "ELASTIC_SIGNATURES", "STRESS_SIGNATURES", "EIGENSTRAIN_SIGNATURES", "MODAL_SIGNATURES",
                  "ELASTIC_SHAPE_SIGNATURES", "ELASTIC_ANISO_SIGNATURES", "ELASTIC_FACET_SIGNATURES", "FILTER_SIGNATURES",
                  "SAMPLE_SIGNATURES", "HYPERELASTIC_SIGNATURES", "HYPER_STRESS_SIGNATURES",
                  "ELASTIC_ANISO_STRESS_SIGNATURES", "BUCKLING_SIGNATURES"):
        others |= set(getattr(_hip, table))
    assert not set(decls) & others and len(_hip.SIGNATURES) == 64 and len(_hip.BUCKLING_SIGNATURES) == 6
    for name, (ret, params) in decls.items():
        res, argtypes = _hip.LOBPCG_SIGNATURES[name]
        assert len(argtypes) == len(params), name
        for i, ((ctype, is_ptr), t) in enumerate(zip(params, argtypes)):
            if not is_ptr:
                assert t is BY_VALUE[ctype], (name, i, ctype, t)
            else:
                assert isinstance(t, type) and issubclass(t, _hip._Ptr) and t.elem == ctype, (name, i, ctype, t)
        # the block count is a value, every other entry returns a status
        assert ret == "int" and res is (_hip._I if name.endswith("_blocks") else _hip._S), name
    if os.path.exists(_hip.LIB_PATH):
        L = _hip.lib()
        raw = ctypes.CDLL(_hip.LIB_PATH)
        for name in decls:
            fn = getattr(L, name)
            assert fn.restype is _hip._I and hasattr(raw, name)
            assert (fn.errcheck is L.diffhe_to_node_major.errcheck) == (not name.endswith("_blocks")), name
        assert L.diffhe_lobpcg_gram_blocks(0, 64) == 0 and L.diffhe_lobpcg_gram_blocks(37, 3) == 0
        assert 1 <= L.diffhe_lobpcg_gram_blocks(1 << 20, 64) <= 32
        with pytest.raises(_hip.HipExtensionError, match="diffhe_lobpcg_gram"):         # refused on the host: no launch
            L.diffhe_lobpcg_gram(None, None, None, None, 6, 8, 4, None, None, None, None)
        with pytest.raises(_hip.HipExtensionError, match="diffhe_lobpcg_ritz"):
            L.diffhe_lobpcg_ritz(None, None, 6, 2, 4, 30, None, None, None, None, None)
        with pytest.raises(_hip.HipExtensionError, match="diffhe_lobpcg_rotate"):
            L.diffhe_lobpcg_rotate(None, None, None, None, None, 6, 2, 8, 4, None, None, None, None, None)


def test_iteration_is_validated_on_all_three_classes_and_reported():
    from diffhe import EigenFESolver, ElasticEigenSolver, LinearBucklingSolver
    mesh = FEMesh.rectangle(6, 5)
    for cls in (EigenFESolver, ElasticEigenSolver, LinearBucklingSolver):
        assert cls(mesh).iteration == "subspace"
        solver = cls(mesh, iteration="lobpcg")
        assert solver.iteration == "lobpcg"
        for bad in ("LOBPCG", "davidson", None, 1):
            with pytest.raises(ValueError, match="iteration"):
                cls(mesh, iteration=bad)
        info = solver.last_info
        assert info.iteration == "subspace" and info.basis_drops == 0        # nothing has run yet
    assert isinstance(LinearBucklingSolver(mesh).last_info, buckling.BucklingInfo)
    assert eigen.EigenInfo(iteration="lobpcg", basis_drops=3).basis_drops == 3
    assert eigen.ITERATIONS == ("subspace", "lobpcg") and eigen.LOBPCG_REFRESH >= 1
    assert eigen._BlockRun.refresh == eigen.LOBPCG_REFRESH


def test_custom_ops_keep_their_fake_implementations_under_lobpcg():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from diffhe import EigenFESolver, ElasticEigenSolver, LinearBucklingSolver
    from diffhe.solver import _SOLVERS
    mesh = FEMesh.rectangle(4, 3)
    n, m = mesh.n_nodes, mesh.n_elements
    es = EigenFESolver(mesh, k=2, iteration="lobpcg")
    ms = ElasticEigenSolver(mesh, k=3, iteration="lobpcg")
    bs = LinearBucklingSolver(mesh, k=3, iteration="lobpcg")
    for s in (es, ms, bs):
        _SOLVERS[id(s)] = s
    with FakeTensorMode():
        kap = torch.empty(5, m, dtype=T64, requires_grad=True)
        lam, phi, _ = torch.ops.diffhe.eig_solve(kap, None, id(es), -1, False, True)
        assert lam.shape == (5, 2) and phi.shape == (5, 2, n) and lam.requires_grad and not phi.requires_grad
        assert torch.autograd.grad(lam.sum(), kap)[0].shape == (5, m)
        E, rho = torch.empty(m, dtype=T64, requires_grad=True), torch.empty(4, m, dtype=T64)
        lam, phi, _ = torch.ops.diffhe.modal_solve(E, rho, None, id(ms), -1, True, True)
        assert lam.shape == (4, 3) and phi.shape == (3, n, 2, 4)
        assert torch.autograd.grad(lam.sum(), E)[0].shape == (m,)
        sig = torch.empty(5, m, 3, dtype=T64, requires_grad=True)
        lam, phi, _ = torch.ops.diffhe.buckling_solve(E, sig, None, id(bs), -1, False, True)
        assert lam.shape == (5, 3) and phi.shape == (5, 3, n, 2)
        gE, gs = torch.autograd.grad(lam.sum(), (E, sig))
        assert gE.shape == (m,) and gs.shape == (5, m, 3)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the entries alone, through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
ROWS, N_BC = 37, 5


def _nan(*shape, dtype=T64):
    if dtype is T64:
        return torch.full(shape, float("nan"), dtype=T64, device=DEV)
    return torch.full(shape, -7, dtype=dtype, device=DEV)


def _packed_rows(G):
    """(B, q, q) -> (B, nq): the upper triangle by rows."""
    q = G.shape[-1]
    iu = torch.triu_indices(q, q)
    return G[:, iu[0], iu[1]]


@gpu
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("p,blocks", [(1, 2), (1, 3), (5, 2), (5, 3), (16, 2), (16, 3)])
def test_gram_and_rotate_against_einsum(p, blocks, B):
    """q = 2, 3, 10, 15, 32, 48: a ragged last tile and the full size; lanes < 64 (Bp = 4 and 32); every pass count of the
    rotation (1 to 8 output columns per pass)."""
    from diffhe.plan import padded_batch
    L = _hip.lib()
    Bp, q, n = padded_batch(B), blocks * p, ROWS
    gen = torch.Generator().manual_seed(100 * q + B)
    S, AS, BS = (torch.randn(3 * p, n, Bp, generator=gen, dtype=T64) for _ in range(3))
    C = torch.randn(q, p, Bp, generator=gen, dtype=T64)
    theta = torch.randn(p, Bp, generator=gen, dtype=T64)
    is_bc = torch.zeros(n, dtype=torch.uint8)
    is_bc[torch.randperm(n, generator=gen)[:N_BC]] = 1
    Sd, ASd, BSd, Cd, thd, bcd = (t.to(DEV).contiguous() for t in (S, AS, BS, C, theta, is_bc))
    nq, nblk = q * (q + 1) // 2, L.diffhe_lobpcg_gram_blocks(n, Bp)
    assert 1 <= nblk <= 32

    def run():
        part, GA, GB = _nan(nblk * 2 * nq * Bp), _nan(nq, Bp), _nan(nq, Bp)
        S2, AS2, BS2, R = _nan(3 * p, n, Bp), _nan(3 * p, n, Bp), _nan(3 * p, n, Bp), _nan(p, n, Bp)
        L.diffhe_lobpcg_gram(Sd, ASd, BSd, bcd, q, n, Bp, part, GA, GB, None)
        L.diffhe_lobpcg_rotate(Sd, ASd, BSd, Cd, thd, q, p, n, Bp, S2, AS2, BS2, R, None)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in dict(GA=GA, GB=GB, S2=S2, AS2=AS2, BS2=BS2, R=R).items()}

    got, again = run(), run()
    for key in got:
        assert torch.equal(got[key].nan_to_num(nan=-3.0), again[key].nan_to_num(nan=-3.0)), key
    free = (1 - is_bc.to(T64))[:, None]
    GA = torch.einsum("irb,jrb->bij", S[:q] * free, AS[:q])
    GB = torch.einsum("irb,jrb->bij", S[:q] * free, BS[:q])
    assert rel_err(got["GA"].t().numpy(), _packed_rows(GA).numpy()) <= 1e-12
    assert rel_err(got["GB"].t().numpy(), _packed_rows(GB).numpy()) <= 1e-12
    CP = C.clone()
    CP[:p] = 0.0
    want = {}
    for key, blk in (("S2", S), ("AS2", AS), ("BS2", BS)):
        want[key] = (torch.einsum("jrb,jcb->crb", blk[:q], C), torch.einsum("jrb,jcb->crb", blk[:q], CP))
        assert rel_err(got[key][:p].numpy(), want[key][0].numpy()) <= 1e-12, key
        assert rel_err(got[key][2 * p:].numpy(), want[key][1].numpy()) <= 1e-12, key       # P'
        assert bool(torch.isnan(got[key][p:2 * p]).all()), key                             # the W slot is not touched
    R = want["AS2"][0] - theta[:, None, :] * want["BS2"][0]
    assert rel_err(got["R"].numpy(), R.numpy()) <= 1e-12


@gpu
@pytest.mark.parametrize("B", [3, 17])
def test_rotate_on_the_start_block_writes_no_P(B):
    from diffhe.plan import padded_batch
    L = _hip.lib()
    p, n, Bp = 5, ROWS, padded_batch(B)
    gen = torch.Generator().manual_seed(7 + B)
    S, AS, BS = (torch.randn(3 * p, n, Bp, generator=gen, dtype=T64) for _ in range(3))
    C, theta = torch.randn(p, p, Bp, generator=gen, dtype=T64), torch.randn(p, Bp, generator=gen, dtype=T64)
    outs = [_nan(3 * p, n, Bp) for _ in range(3)]
    R = _nan(p, n, Bp)
    L.diffhe_lobpcg_rotate(S.to(DEV), AS.to(DEV), BS.to(DEV), C.to(DEV), theta.to(DEV), p, p, n, Bp, *outs, R, None)
    torch.cuda.synchronize()
    for got, blk in zip(outs, (S, AS, BS)):
        assert rel_err(got[:p].cpu().numpy(), torch.einsum("jrb,jcb->crb", blk[:p], C).numpy()) <= 1e-12
        assert bool(torch.isnan(got[p:]).all())
    assert bool(torch.isfinite(R).all())


@gpu
@pytest.mark.parametrize("blocks", [1, 2])
def test_rotate_with_the_whole_lds_window(blocks):
    """p = 16 at Bp = 64: q x OC = 16 x 8 and 32 x 4 columns of C for 64 lanes, the 64 KiB of dynamic LDS the launch may ask
    for; two sample chunks (Bp = 128) at q = 32."""
    L = _hip.lib()
    p, n = 16, ROWS
    q, Bp = blocks * p, 64 * blocks
    gen = torch.Generator().manual_seed(70 + blocks)
    S, AS, BS = (torch.randn(3 * p, n, Bp, generator=gen, dtype=T64) for _ in range(3))
    C, theta = torch.randn(q, p, Bp, generator=gen, dtype=T64), torch.randn(p, Bp, generator=gen, dtype=T64)
    outs = [_nan(3 * p, n, Bp) for _ in range(3)]
    R = _nan(p, n, Bp)
    L.diffhe_lobpcg_rotate(S.to(DEV), AS.to(DEV), BS.to(DEV), C.to(DEV), theta.to(DEV), q, p, n, Bp, *outs, R, None)
    torch.cuda.synchronize()
    CP = C.clone()
    CP[:p] = 0.0
    want = [torch.einsum("jrb,jcb->crb", blk[:q], C) for blk in (S, AS, BS)]
    for got, blk, w in zip(outs, (S, AS, BS), want):
        assert rel_err(got[:p].cpu().numpy(), w.numpy()) <= 1e-12
        if blocks == 2:
            assert rel_err(got[2 * p:].cpu().numpy(), torch.einsum("jrb,jcb->crb", blk[:q], CP).numpy()) <= 1e-12
    assert rel_err(R.cpu().numpy(), (want[1] - theta[:, None, :] * want[2]).numpy()) <= 1e-12


def _ritz_case(p, blocks, B, seed):
    """Per sample: M SPD with eigenvalues in [1, 10], D spanning four decades, GB = D M D (condition ~ 1e8), GA = D Z D
    with Z symmetric indefinite of order one.  -> (GA, GB (B, q, q), reference theta (B, p) of the scaled pencil (Z, M))."""
    q = blocks * p
    rng = np.random.default_rng(seed)
    GA, GB, ref = np.zeros((B, q, q)), np.zeros((B, q, q)), np.zeros((B, p))
    for b in range(B):
        Q, _ = np.linalg.qr(rng.standard_normal((q, q)))
        M = Q @ np.diag(np.linspace(1.0, 10.0, q)) @ Q.T
        M = 0.5 * (M + M.T)
        Z = rng.standard_normal((q, q))
        Z = 0.5 * (Z + Z.T)
        D = np.logspace(0.0, -4.0, q)[rng.permutation(q)] if q > 1 else np.ones(1)
        GA[b], GB[b] = D[:, None] * Z * D[None, :], D[:, None] * M * D[None, :]
        Lc = np.linalg.cholesky(M)
        At = np.linalg.solve(Lc, np.linalg.solve(Lc, Z).T)
        ref[b] = np.linalg.eigh(0.5 * (At + At.T))[0][:p]
    return GA, GB, ref


def _run_ritz(GA, GB, p, Bp, cap=None):
    """GA, GB (B, q, q) numpy -> C (B, q, p), theta (B, p), used (B,), flag (B,) on the CPU; the padding samples carry the
    identity pencil.  Runs twice and asserts bitwise equality."""
    L = _hip.lib()
    B, q = GA.shape[0], GA.shape[1]
    nq = q * (q + 1) // 2
    pk = lambda G: torch.cat([_packed_rows(torch.from_numpy(G)),  # noqa: E731
                              _packed_rows(torch.eye(q, dtype=T64)[None].expand(Bp - B, q, q))]).t().contiguous().to(DEV)
    GAd, GBd = pk(GA), pk(GB)
    assert tuple(GAd.shape) == (nq, Bp)
    outs = []
    for _ in range(2):
        C, theta = _nan(q, p, Bp), _nan(p, Bp)
        used, flag = torch.zeros(Bp, dtype=torch.int32, device=DEV), _nan(Bp, dtype=torch.int32)
        if cap is not None:
            used[:len(cap)] = torch.tensor(cap, dtype=torch.int32)
        L.diffhe_lobpcg_ritz(GAd, GBd, q, p, Bp, eigen.JACOBI_SWEEPS, C, theta, used, flag, None)
        torch.cuda.synchronize()
        outs.append((C.cpu(), theta.cpu(), used.cpu(), flag.cpu()))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    C, theta, used, flag = outs[0]
    assert bool(torch.isfinite(C).all()) and bool(torch.isfinite(theta).all())
    assert bool((flag[B:] == 0).all()) and bool((used[B:] == q).all())              # padding samples raise nothing
    return C.permute(2, 0, 1)[:B].numpy(), theta.t()[:B].numpy(), used[:B].numpy(), flag[:B].numpy()


@gpu
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("p,blocks", [(1, 2), (1, 3), (5, 1), (5, 2), (5, 3), (16, 2), (16, 3)])
def test_ritz_entry_against_numpy(p, blocks, B):
    from diffhe.plan import padded_batch
    GA, GB, ref = _ritz_case(p, blocks, B, 1000 * p + 10 * blocks + B)
    q = blocks * p
    if q >= 10:
        assert 1e7 <= np.linalg.cond(GB[0]) <= 1e10
    C, theta, used, flag = _run_ritz(GA, GB, p, padded_batch(B))
    assert np.all(flag == 0) and np.all(used == q)
    for b in range(B):
        eb = np.abs(C[b].T @ GB[b] @ C[b] - np.eye(p)).max()
        ea = np.abs(C[b].T @ GA[b] @ C[b] - np.diag(theta[b])).max()
        et = np.abs(theta[b] - ref[b]).max() / np.abs(ref[b]).max()
        if b == 0:
            print(f"q={q} sample 0: C^T GB C - I {eb:.2e}, C^T GA C - diag {ea:.2e}, theta {et:.2e}")
        assert eb <= 1e-10 and ea <= 1e-10 and et <= 1e-11
        assert np.all(np.diff(theta[b]) >= 0.0)


@gpu
@pytest.mark.parametrize("p", [1, 5, 16])
def test_ritz_entry_falls_back_and_flags(p):
    """Sample 0: the P block duplicates the W block -> basis 2p, valid pairs of [X | W], no flag.  Sample 1: W and P both
    duplicate X -> basis p.  Sample 2: a NaN in GB -> flag, identity rotation.  Sample 3: full rank, for comparison."""
    q, n, B, Bp = 3 * p, 60, 4, 4
    rng = np.random.default_rng(40 + p)
    A = rng.standard_normal((n, n))
    A = 0.5 * (A + A.T)
    X, W, P = (rng.standard_normal((n, p)) for _ in range(3))
    bases = [np.concatenate(cols, axis=1) for cols in ((X, W, W), (X, X, X), (X, W, P), (X, W, P))]
    GA = np.stack([S.T @ A @ S for S in bases])
    GB = np.stack([S.T @ S for S in bases])
    GB[2, q - 1, q - 1] = np.nan
    C, theta, used, flag = _run_ritz(GA, GB, p, Bp)
    assert flag.tolist() == [0, 0, 1, 0] and used.tolist() == [2 * p, p, p, q]
    for b, m in ((0, 2 * p), (1, p), (3, q)):
        assert np.all(C[b][m:] == 0.0)
        Gb, Ga = GB[b][:m, :m], GA[b][:m, :m]
        Cm = C[b][:m]
        assert np.abs(Cm.T @ Gb @ Cm - np.eye(p)).max() <= 1e-10
        assert np.abs(Cm.T @ Ga @ Cm - np.diag(theta[b])).max() <= 1e-10 * max(1.0, np.abs(theta[b]).max())
        Lc = np.linalg.cholesky(Gb)
        At = np.linalg.solve(Lc, np.linalg.solve(Lc, Ga).T)
        ref = np.linalg.eigh(0.5 * (At + At.T))[0][:p]
        assert np.abs(theta[b] - ref).max() <= 1e-11 * np.abs(ref).max()
    assert np.array_equal(C[2][:p], np.eye(p)) and np.all(C[2][p:] == 0.0) and np.all(theta[2] == 0.0)
    # `used` is read as well: a sample whose last step ran on [X | W] (or on [X]) starts on [X | W], the others on q
    GB[2, q - 1, q - 1] = GB[3, q - 1, q - 1]
    C2, theta2, used2, flag2 = _run_ritz(GA, GB, p, Bp, cap=[2 * p, p, q, 0])
    assert flag2.tolist() == [0, 0, 0, 0] and used2.tolist() == [2 * p, p, q, q]
    assert np.array_equal(C2[0], C[0]) and np.array_equal(C2[3], C[3]) and np.array_equal(theta2[3], theta[3])
    _, _, used3, _ = _run_ritz(GA, GB, p, Bp, cap=[0, 0, p, 2 * p])
    assert used3.tolist() == [2 * p, p, 2 * p, 2 * p]
    if p > 1:       # a stale value that is no multiple of p is rounded down to one: [X] is still reached, nothing is flagged
        _, _, used4, flag4 = _run_ritz(GA, GB, p, Bp, cap=[2 * p + 1, 2 * p + 1, 3 * p - 1, 1])
        assert used4.tolist() == [2 * p, p, 2 * p, 2 * p] and flag4.tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: buckling
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", list(tb.CASES))
def test_buckling_against_the_dense_model_in_fewer_outer_iterations(key):
    mesh, fixed, E, load, plane = tb.case(key)
    k = tb.K_MODES
    bs = tb.make_solver(mesh, E, plane, fixed, iteration="lobpcg")
    lam, phi = bs(load=load.to(DEV))
    info = bs.last_info
    ref = tb.make_solver(mesh, E, plane, fixed, iteration="subspace")
    lam_s, _ = ref(load=load.to(DEV))
    print(key, "outer lobpcg / subspace", info.outer_iterations, ref.last_info.outer_iterations, "inner iterations",
          info.inner_iterations, ref.last_info.inner_iterations, "drops", info.basis_drops, "negative Ritz",
          info.negative_ritz, "rho", info.residual.tolist())
    assert info.iteration == "lobpcg" and ref.last_info.iteration == "subspace"
    assert lam.shape == (k,) and phi.shape == (k, mesh.n_nodes, mesh.dim)
    assert info.not_converged == 0 and info.missing == 0 and info.gram_failures == 0
    assert tuple(info.shifts.shape) == (1,) and bool((info.shifts == 0.0).all())
    assert info.block == k + tb.GUARD and info.prestress is not None and info.prestress.not_converged == 0
    tb.check_against_dense(mesh, plane, fixed, E[None], load, lam.cpu()[None], phi.cpu().reshape(1, k, -1), bs.tol)
    assert rel_err(lam.cpu().numpy(), lam_s.cpu().numpy()) <= 2 * RTOL_U
    assert ref.last_info.not_converged == 0
    assert info.outer_iterations < ref.last_info.outer_iterations
    assert info.outer_iterations <= LOBPCG_CAPS[key]


@gpu
@pytest.mark.parametrize("key", ["2d-shear-stress", "3d-shear"])
def test_buckling_does_not_stop_on_columns_it_has_not_measured(key):
    """A start block WITHOUT a positive Ritz value: the p modes of the most negative mu of the dense model plus a tenth of
    a K-normalised random column each.  Ritz on [X | W] turns up k positive mu in the first iteration (dense model: 28, 18,
    12 in 2D), for columns whose residual was never measured -- they had no positive mu when the inner solves ran.  The run
    must not take them for converged: it goes on and reaches the dense model's lambda."""
    mesh, fixed, E, load, plane = tb.case(key)
    k, p, n, d = tb.K_MODES, tb.K_MODES + tb.GUARD, mesh.n_nodes, mesh.dim
    sig = tb.dense_prestress(mesh, E, load, plane, fixed)
    mu, phi, K = tb.dense_spectrum(mesh, E, sig, plane, fixed)
    assert float(mu[-p]) < 0.0
    free = torch.zeros(n * d, dtype=T64)
    free[tb.free_dofs(mesh, fixed)] = 1.0
    r = torch.randn(p, n * d, generator=torch.Generator().manual_seed(5), dtype=T64) * free
    r = r / torch.sqrt(torch.einsum("ir,rs,is->i", r, K, r))[:, None]
    x0 = phi[-p:] + 0.1 * r
    G = x0 @ tb.dense_KG(mesh, sig) @ x0.t()
    Lc = torch.linalg.cholesky(x0 @ K @ x0.t())
    start = torch.linalg.eigvalsh(torch.linalg.solve_triangular(Lc, torch.linalg.solve_triangular(Lc, -G, upper=False).t(),
                                                                upper=False))
    assert float(start.max()) < 0.0                                    # the start block has no positive Ritz value
    bs = tb.make_solver(mesh, E, plane, fixed, iteration="lobpcg")
    lam, phi_g = bs(load=load.to(DEV), x0=x0.reshape(p, n, d).to(DEV))
    info = bs.last_info
    print(key, "outer", info.outer_iterations, "negative Ritz", info.negative_ritz, "lambda", lam.tolist())
    assert info.negative_ritz == p                                     # seen by the run as well
    assert info.outer_iterations > 1 and info.not_converged == 0 and info.missing == 0
    assert bool((info.residual > 0.0).all())                           # every returned column was measured
    tb.check_against_dense(mesh, plane, fixed, E[None], load, lam.cpu()[None], phi_g.cpu().reshape(1, k, -1), bs.tol)


@gpu
def test_buckling_batch_with_padding_samples_and_both_layouts():
    """B = 3 in a padded batch of 4: the padding sample raises no flag, no warning and leaks nothing."""
    mesh, fixed, _, load, plane = tb.case("2d-shear-stress")
    B, k = 3, tb.K_MODES
    E = _rand((B, mesh.n_elements), 90, 0.5, 2.0)
    for layout in ("sample", "node"):
        bs = tb.make_solver(mesh, E, plane, fixed, iteration="lobpcg")
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            lam, phi = bs(load=load.to(DEV), layout=layout)
        assert bs.last_info.not_converged == 0 and bs.last_info.gram_failures == 0
        assert bool(torch.isfinite(lam).all()) and bool(torch.isfinite(phi).all())
        rows = phi.cpu().permute(3, 0, 1, 2) if layout == "node" else phi.cpu()
        tb.check_against_dense(mesh, plane, fixed, E, load, lam.cpu(), rows.reshape(B, k, -1), bs.tol)


@gpu
@pytest.mark.parametrize("key", ["2d-axial-stress", "2d-shear-strain", "3d-axial", "3d-shear"])
def test_buckling_total_gradients(key):
    tol = 1e-11
    mesh, fixed, E0, load0, plane = tb.case(key)
    E, load = E0.to(DEV).requires_grad_(True), load0.to(DEV).requires_grad_(True)
    bs = tb.make_solver(mesh, E, plane, fixed, tol=tol, iteration="lobpcg")
    lam, _ = bs(load=load)
    assert bs.last_info.not_converged == 0 and bs.last_info.missing == 0
    w = torch.tensor([1.0, -0.5, 0.25], dtype=T64)
    (lam * w.to(DEV)).sum().backward()
    gE, gl, amp, _ = tb.dense_total_grads(mesh, plane, fixed, E0, load0, w)
    bound = tol * amp + float(bs.inner.tol)
    eE, el = rel_err(E.grad.cpu().numpy(), gE.numpy()), rel_err(load.grad.cpu().numpy(), gl.numpy())
    print(f"{key}: dE {eE:.2e}, dload {el:.2e} (bound {bound:.2e}); outer {bs.last_info.outer_iterations}")
    assert eE <= bound and el <= bound
    assert float(load.grad.cpu().reshape(-1)[tb.fixed_dofs(mesh, fixed)].abs().max()) == 0.0
    for i in range(tb.K_MODES):
        E.grad = None
        lam_i, _ = bs(load=load0.to(DEV))
        lam_i[i].backward()
        h = abs(float((E.grad * E.detach()).sum() / lam_i[i].detach()) - 1.0)
        print(f"{key} mode {i}: homogeneity {h:.2e}")
        assert h <= RTOL_GRAD


@gpu
def test_buckling_biaxial_tension_and_warm_start():
    mesh, fixed, E0, load = tb.biaxial_tension()
    E = E0.to(DEV).requires_grad_(True)
    bs = tb.make_solver(mesh, E, "stress", fixed, iteration="lobpcg")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        lam, phi = bs(load=load.to(DEV))
    assert [w.category for w in caught] == [RuntimeWarning] and "missing" in str(caught[0].message)
    assert bool(torch.isinf(lam).all()) and bool((lam > 0).all()) and float(phi.abs().max()) == 0.0
    assert bs.last_info.missing == tb.K_MODES and bs.last_info.not_converged == 0
    assert bs.last_info.outer_iterations >= buckling.MIN_OUTER_MISSING
    lam.sum().backward()
    assert bool((E.grad == 0.0).all())
    # warm start: a converged block is at the stopping rule after the one iteration that measures it
    mesh, fixed, E0, load, plane = tb.case("3d-shear")
    cold = tb.make_solver(mesh, E0, plane, fixed, iteration="lobpcg")
    lam, phi = cold(load=load.to(DEV))
    lam2, phi2 = tb.make_solver(mesh, E0, plane, fixed, iteration="lobpcg")(load=load.to(DEV))
    assert torch.equal(lam, lam2) and torch.equal(phi, phi2)                            # bitwise reproducible
    warm = tb.make_solver(mesh, E0, plane, fixed, iteration="lobpcg")
    lam_w, _ = warm(load=load.to(DEV), x0=phi)
    assert warm.last_info.outer_iterations == 1 and warm.last_info.not_converged == 0
    assert rel_err(lam_w.cpu().numpy(), lam.cpu().numpy()) <= RTOL_U


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the mass-weighted solvers
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ["lattice", "general", "box"])
def test_eigen_solver_against_the_dense_model(which):
    if which == "lattice":
        mesh, k, vectors = te.lattice_mesh(), 4, True
    elif which == "general":
        mesh, k, vectors = te.jittered(FEMesh.rectangle(14, 12, (0.0, 1.4), (0.0, 1.0))), 4, True
    else:
        mesh, k, vectors = FEMesh.box(5, 5, 5), 8, False      # relative gaps fall to 1e-3 there (tests/test_eigen.py)
    kappa = te.field(mesh.n_elements, 6, B=3)
    es, lam, phi = te.solve(mesh, kappa, k, iteration="lobpcg")
    ref, lam_s, _ = te.solve(mesh, kappa, k)
    info = es.last_info
    print(which, "outer lobpcg / subspace", info.outer_iterations, ref.last_info.outer_iterations, "drops", info.basis_drops)
    assert info.iteration == "lobpcg" and info.not_converged == 0 and info.gram_failures == 0
    assert info.path.startswith("lattice" if which == "lattice" else "ell")
    te.check_against_dense(mesh, kappa, *te.as_rows(lam, phi, "sample"), es.tol, vectors=vectors)
    assert info.outer_iterations <= ref.last_info.outer_iterations


@gpu
def test_eigen_solver_shift_without_dirichlet_nodes_and_gradient():
    base = te.lattice_mesh()
    mesh = FEMesh(nodes=base.nodes, elements=base.elements, dirichlet_nodes={})
    kappa = torch.tensor([1.0, 2.5], dtype=T64)
    es, lam, phi = te.solve(mesh, kappa, 4, shift=3.0, iteration="lobpcg", layout="node")
    assert es.last_info.not_converged == 0
    lam_r, phi_r = te.as_rows(lam, phi, "node")
    assert float(lam_r[:, 0].abs().max()) <= RTOL_U * float(lam_r[:, 1].min())
    te.check_against_dense(mesh, kappa, lam_r, phi_r, es.tol, shift=3.0)
    # d lambda / d kappa per element at tol = 1e-11, lattice and general path
    from diffhe import EigenFESolver
    tol = 1e-11
    for mesh in (te.lattice_mesh(), te.jittered(FEMesh.rectangle(14, 12, (0.0, 1.4), (0.0, 1.0)))):
        field = te.field(mesh.n_elements, 12, B=2)
        kap = field.to("cuda").requires_grad_(True)
        es = EigenFESolver(mesh, kap, 3, tol=tol, iteration="lobpcg")
        lam, _ = es()
        assert es.last_info.not_converged == 0
        w = torch.tensor([1.0, -0.5, 0.25], dtype=T64).expand(2, 3)
        (lam * w.to("cuda")).sum().backward()
        want = te.dense_grad(mesh, field, w)
        for b in range(2):
            ref_lam = te.dense_eig(mesh, field[b])[0].numpy()
            bound = float(np.max(10 * tol * ref_lam[:3] / te.gaps(ref_lam, range(3))))
            e = rel_err(kap.grad[b].cpu().numpy(), want[b].numpy())
            print(f"sample {b}: gradient rel_err {e:.2e} (bound {bound:.2e})")
            assert e <= bound


@gpu
@pytest.mark.parametrize("key", list(tm.CASES))
def test_modal_solver_and_gradients_against_the_dense_model(key):
    make, plane = tm.CASES[key]
    mesh, fixed = make()
    m, B, k = mesh.n_elements, 2, 3
    E0, r0 = _rand((B, m), 58, 0.5, 2.0), _rand((B, m), 59, 0.5, 2.0)
    es, lam, phi = tm.solve(mesh, E0, r0, k, plane=plane, fixed=fixed, iteration="lobpcg")
    assert es.last_info.iteration == "lobpcg" and es.last_info.not_converged == 0 and es.last_info.gram_failures == 0
    tm.check_against_dense(mesh, plane, fixed, E0, r0, *tm.as_rows(lam, phi, "sample"), es.tol)
    tol = 1e-11
    from diffhe import ElasticEigenSolver
    E, rho = E0.to(DEV).requires_grad_(True), r0.to(DEV).requires_grad_(True)
    es = ElasticEigenSolver(mesh, E, rho, k, nu=tm.NU, plane=plane, fixed=fixed, tol=tol, device=DEV, iteration="lobpcg")
    lam, _ = es()
    assert es.last_info.not_converged == 0
    w = torch.tensor([1.0, -0.5, 0.25], dtype=T64).expand(B, k)
    (lam * w.to(DEV)).sum().backward()
    gE, gr, amp = tm.dense_grads(mesh, plane, fixed, E0, r0, w)
    for b in range(B):
        eE, er = rel_err(E.grad[b].cpu().numpy(), gE[b].numpy()), rel_err(rho.grad[b].cpu().numpy(), gr[b].numpy())
        print(f"{key} sample {b}: dE {eE:.2e}, drho {er:.2e} (bound {tol * amp[b]:.2e})")
        assert eE <= tol * amp[b] and er <= tol * amp[b]


@gpu
def test_modal_solver_on_a_free_body_with_a_shift():
    mesh, _ = tm.rect2d()
    m, B, k = mesh.n_elements, 3, 8
    E, rho = tm.field_of("sample_element", m, B, 52), tm.field_of("element", m, B, 73)
    shift = float(tm.dense_modes(mesh, tm.field_rows(E, m, B)[0], tm.field_rows(rho, m, B)[0], "stress", {})[0][3])
    es, lam, phi = tm.solve(mesh, E, rho, k, plane="stress", fixed={}, shift=shift, iteration="lobpcg")
    assert es.last_info.not_converged == 0 and tuple(lam.shape) == (B, k)
    tm.check_against_dense(mesh, "stress", {}, E, rho, *tm.as_rows(lam, phi, "sample"), es.tol, shift=shift, n_rigid=3)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the default is what it was
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_call_without_iteration_is_bitwise_the_subspace_call():
    mesh = te.lattice_mesh()
    kappa = te.field(mesh.n_elements, 6, B=3)
    (_, lam, phi), (_, lam_s, phi_s) = te.solve(mesh, kappa, 4), te.solve(mesh, kappa, 4, iteration="subspace")
    assert torch.equal(lam, lam_s) and torch.equal(phi, phi_s)
    make, plane = tm.CASES["2d-stress"]
    mesh, fixed = make()
    E, rho = _rand((2, mesh.n_elements), 58, 0.5, 2.0), _rand((2, mesh.n_elements), 59, 0.5, 2.0)
    (_, lam, phi) = tm.solve(mesh, E, rho, 3, plane=plane, fixed=fixed)
    (_, lam_s, phi_s) = tm.solve(mesh, E, rho, 3, plane=plane, fixed=fixed, iteration="subspace")
    assert torch.equal(lam, lam_s) and torch.equal(phi, phi_s)
    mesh, fixed, E, load, plane = tb.case("2d-shear-stress")
    a, b = tb.make_solver(mesh, E, plane, fixed), tb.make_solver(mesh, E, plane, fixed, iteration="subspace")
    (lam, phi), (lam_s, phi_s) = a(load=load.to(DEV)), b(load=load.to(DEV))
    assert torch.equal(lam, lam_s) and torch.equal(phi, phi_s)
    assert a.last_info.iteration == "subspace" and a.last_info.basis_drops == 0 and float(a.last_info.shifts.min()) > 0.0
    assert math.isfinite(float(lam.sum()))
