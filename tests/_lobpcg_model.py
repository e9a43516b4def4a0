"""A numpy statement of the LOBPCG outer iteration of `diffhe.eigen._BlockRun` ("LOBPCG") for one sample
of the pencil A x = theta B x, B symmetric positive definite, the p smallest theta wanted.  Dense matrices, an exact
preconditioner T (a callable r -> w) unless another is given; `numpy.linalg.eigh` stands where the kernel runs cyclic Jacobi.

    S = [X | W | P]                      W = T R, P the previous step; [X | W] on the first iteration and after a warm start
    GA = S^T A S, GB = S^T B S           from the carried blocks A S and B S
    ritz: scale by diag(GB)^-1/2, Cholesky with the pivot test d > 1e-8, eigh of L^-1 GA L^-T, the p smallest theta;
          a failed factorisation retries on [X | W], then on [X]; a sample that fell back from 3p stays on [X | W];
          the first `retries` refreshes lift that
    X' = S C, P' = S C_P (C with its X rows zeroed), the same combinations of A S and B S, R' = A X' - theta B X'
    every `refresh` iterations A X and B X are applied afresh instead of rotated

Written for tests/test_lobpcg.py; it shares no code with the product.
"""
import numpy as np

PIVOT = 1e-8


def cholesky(G):
    """Lower factor of G by columns with the relative pivot test (unit diagonal after scaling), or None."""
    m = G.shape[0]
    L = np.zeros_like(G)
    for j in range(m):
        d = G[j, j] - L[j, :j] @ L[j, :j]
        if not (np.isfinite(d) and d > PIVOT * G[j, j]):
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (G[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def ritz(GA, GB, p, cap=0):
    """-> (C (q, p), theta (p,), size used, flag).  q = GA.shape[0] is p, 2p or 3p; the sizes tried are q, then the
    smaller multiples of p down to p.  cap: the size the sample's last Ritz step used -- a sample that once fell back from
    3p stays on [X | W] (a cap below 2p counts as 2p; 0: none).  A non-finite input or a failure on [X] gives the
    identity rotation and flag 1."""
    q = GA.shape[0]
    C, theta = np.zeros((q, p)), np.zeros(p)
    top = min(q, max(cap, 2 * p)) if cap > 0 else q
    if np.isfinite(GA).all() and np.isfinite(GB).all():
        for m in range(top, 0, -p):
            d = np.diag(GB)[:m]
            if not (d > 0).all():
                continue
            s = 1.0 / np.sqrt(d)
            L = cholesky(GB[:m, :m] * s[:, None] * s[None, :])
            if L is None:
                continue
            W = np.linalg.solve(L, GA[:m, :m] * s[:, None] * s[None, :])
            At = np.linalg.solve(L, W.T)
            th, V = np.linalg.eigh(0.5 * (At + At.T))
            C[:m] = s[:, None] * np.linalg.solve(L.T, V[:, :p])
            return C, th[:p], m, 0
    C[:p] = np.eye(p)
    return C, theta, p, 1


def lobpcg(A, B, X0, T=None, tol=1e-13, max_iter=200, refresh=8, retries=2, P0=None):
    """-> (theta (p,), X (n, p), iterations, sizes used per iteration).  The stopping measure is
    |R_i| / (|A x_i| + |theta_i| |B x_i|) in the 2-norm, for every column.  P0: a P block to enter the first three-block iteration with (a test makes it dependent on purpose)."""
    n, p = X0.shape
    if T is None:
        Binv = np.linalg.inv(B)
        T = lambda R: Binv @ R  # noqa: E731
    S, AS, BS = np.zeros((n, 3 * p)), np.zeros((n, 3 * p)), np.zeros((n, 3 * p))
    S[:, :p] = X0
    AS[:, :p], BS[:, :p] = A @ X0, B @ X0
    C, theta, _, flag = ritz(S[:, :p].T @ AS[:, :p], S[:, :p].T @ BS[:, :p], p)
    assert flag == 0
    for blk in (S, AS, BS):
        blk[:, :p] = blk[:, :p] @ C
    R = AS[:, :p] - BS[:, :p] * theta
    have_p, sizes, it, cap = False, [], 0, 0
    norm = lambda M: np.linalg.norm(M, axis=0)  # noqa: E731
    while it < max_iter and (norm(R) / (norm(AS[:, :p]) + np.abs(theta) * norm(BS[:, :p]))).max() > tol:
        it += 1
        W = T(R)
        S[:, p:2 * p], AS[:, p:2 * p], BS[:, p:2 * p] = W, A @ W, B @ W
        if P0 is not None and it == 2:
            S[:, 2 * p:], AS[:, 2 * p:], BS[:, 2 * p:] = P0, A @ P0, B @ P0
        if it % refresh == 0:
            AS[:, :p], BS[:, :p] = A @ S[:, :p], B @ S[:, :p]
            if it <= retries * refresh:
                cap = 0
        q = 3 * p if have_p else 2 * p
        C, theta, used, flag = ritz(S[:, :q].T @ AS[:, :q], S[:, :q].T @ BS[:, :q], p, cap=cap)
        cap = used if used < q else 0
        assert flag == 0
        sizes.append((q, used))
        CP = C.copy()
        CP[:p] = 0.0
        for blk in (S, AS, BS):
            new_x, new_p = blk[:, :q] @ C, blk[:, :q] @ CP
            blk[:, :p], blk[:, 2 * p:] = new_x, new_p
        R = AS[:, :p] - BS[:, :p] * theta
        have_p = True
    return theta, S[:, :p].copy(), it, sizes
