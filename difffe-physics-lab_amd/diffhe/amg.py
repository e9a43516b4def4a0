"""Aggregation hierarchy for general (unstructured) P1 meshes -- host side.

The general ELL path has no geometric hierarchy to lean on, so its multigrid preconditioner is
algebraic: nodes are grouped into aggregates (roots = a distance-2 maximal independent set of the
mesh graph, every other node joins an adjacent aggregate), the prolongation is piecewise constant,
and the coarse operators are the Galerkin products P^T A P -- which for piecewise-constant P are
plain sums of fine-matrix entries, so they are rebuilt PER SAMPLE on the device from gather lists
(`diffhe_ell_galerkin`) while the aggregates and patterns, computed here once per mesh with
vectorised numpy, are shared by the whole batch.  Dirichlet nodes belong to no aggregate (their
rows are identity rows and their residual is zero).

Nothing here has a counterpart in the reference (it solves with a dense LU, solver.py:174).
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np


def aggregate(cols: np.ndarray, active: np.ndarray, seed: int = 0) -> np.ndarray:
    """Node -> aggregate id (or -1 for inactive nodes) for the graph given by ELL columns
    `cols` (W, n) (slot 0 = the node itself, unused slots point at the node itself).

    Roots are picked as strict priority maxima within graph distance 2 (Luby rounds), so two
    roots are never adjacent or share a neighbour; each remaining node joins the aggregate of an
    adjacent root, else of an adjacent already-aggregated node; isolated leftovers become singletons.
    Deterministic for a given seed.
    """
    W, n = cols.shape
    rng = np.random.default_rng(seed)
    prio = rng.permutation(n).astype(np.float64) + 1.0
    prio[~active] = -np.inf
    state = np.zeros(n, dtype=np.int8)            # 0 undecided, 1 root, 2 within distance 2 of a root
    state[~active] = 2
    idx_all = np.arange(n)
    while True:
        cand = state == 0
        if not cand.any():
            break
        pc = np.where(cand, prio, -np.inf)
        m1 = pc[cols].max(axis=0)                  # max over the closed neighbourhood
        m2 = m1[cols].max(axis=0)                  # ... over distance 2
        new_root = cand & (pc >= m2)
        state[new_root] = 1
        near1 = new_root[cols].any(axis=0)
        near2 = near1[cols].any(axis=0)
        state[near2 & (state == 0)] = 2
    roots = np.nonzero(state == 1)[0]
    agg = np.full(n, -1, dtype=np.int64)
    agg[roots] = np.arange(len(roots))
    # distance-1 neighbours of a root join it (a node is adjacent to at most one root)
    nb = agg[cols]                                 # (W, n) aggregate of each neighbour, -1 if none
    join = nb.max(axis=0)
    take = active & (agg < 0) & (join >= 0)
    agg[take] = join[take]
    # the rest (distance 2 from every root) joins any adjacent aggregate; repeat until stable
    for _ in range(8):
        left = active & (agg < 0)
        if not left.any():
            break
        join = agg[cols].max(axis=0)
        take = left & (join >= 0)
        if not take.any():
            break
        agg[take] = join[take]
    left = np.nonzero(active & (agg < 0))[0]       # disconnected leftovers: singletons
    if len(left):
        base = int(agg.max()) + 1
        agg[left] = base + np.arange(len(left))
    del idx_all
    return agg


def coarse_pattern(cols: np.ndarray, agg: np.ndarray):
    """Galerkin gather lists for piecewise-constant aggregation.

    Returns dict(n, W, cols (W,n) i32, ent_ptr (W*n+1) i32, contrib i32) for the coarse level:
    coarse entry (I, slot) at slot*n + I sums the fine entries listed in contrib[ent_ptr[.]:ent_ptr[.+1]]
    (fine entry index = k*n_fine + i).  Slot 0 is the diagonal."""
    Wf, nf = cols.shape
    nc = int(agg.max()) + 1
    k_idx, i_idx = np.meshgrid(np.arange(Wf, dtype=np.int64), np.arange(nf, dtype=np.int64), indexing="ij")
    j_idx = cols.astype(np.int64)
    real = (k_idx == 0) | (j_idx != i_idx)         # drop the padding slots (they point at the row itself)
    I = agg[i_idx]
    J = agg[j_idx]
    keep = real & (I >= 0) & (J >= 0)
    I, J = I[keep], J[keep]
    fine_entry = (k_idx * nf + i_idx)[keep]
    # coarse entries: unique (I, J), diagonal first within each row
    rows_all = np.concatenate([np.arange(nc, dtype=np.int64), I])
    cols_all = np.concatenate([np.arange(nc, dtype=np.int64), J])
    offd = (rows_all != cols_all).astype(np.int64)
    key = (rows_all * 2 + offd) * nc + cols_all
    order = np.argsort(key, kind="stable")
    ks = key[order]
    new = np.ones(len(ks), dtype=bool)
    new[1:] = ks[1:] != ks[:-1]
    entry_id = np.cumsum(new) - 1
    ent_rows = rows_all[order][new]
    ent_cols = cols_all[order][new]
    row_start = np.searchsorted(ent_rows, np.arange(nc))
    slot = np.arange(len(ent_rows)) - row_start[ent_rows]
    W = int(slot.max()) + 1
    ccols = np.tile(np.arange(nc, dtype=np.int32), W)
    cidx = slot * nc + ent_rows
    ccols[cidx] = ent_cols.astype(np.int32)
    inv = np.empty(len(order), dtype=np.int64)
    inv[order] = np.arange(len(order))
    contrib_entry = cidx[entry_id[inv[nc:]]]
    corder = np.argsort(contrib_entry, kind="stable")
    contrib = fine_entry[corder]
    ent_ptr = np.zeros(W * nc + 1, dtype=np.int64)
    np.cumsum(np.bincount(contrib_entry, minlength=W * nc), out=ent_ptr[1:])
    if ent_ptr[-1] >= 2 ** 31 or Wf * nf >= 2 ** 31:
        raise ValueError("mesh too large for int32 gather lists")
    return dict(n=nc, W=W, cols=ccols.reshape(W, nc), ent_ptr=ent_ptr.astype(np.int32), contrib=contrib.astype(np.int32))


def members_csr(agg: np.ndarray, nc: int):
    """CSR of aggregate members: (ptr (nc+1) i32, members i32 sorted by aggregate then node id)."""
    act = np.nonzero(agg >= 0)[0]
    order = np.argsort(agg[act], kind="stable")
    members = act[order].astype(np.int32)
    ptr = np.zeros(nc + 1, dtype=np.int64)
    np.cumsum(np.bincount(agg[act], minlength=nc), out=ptr[1:])
    return ptr.astype(np.int32), members


def build_hierarchy(cols: np.ndarray, is_bc: np.ndarray, min_coarse: int = 64, max_levels: int = 12) -> List[Dict]:
    """Levels below the fine one: each dict holds the aggregation of the PREVIOUS level (agg, agg_ptr,
    agg_members) and the pattern / Galerkin lists of this level (n, W, cols, ent_ptr, contrib)."""
    levels: List[Dict] = []
    active = ~is_bc.astype(bool)
    cur_cols = cols
    while len(levels) < max_levels - 1:
        n_active = int(active.sum())
        if n_active <= min_coarse:
            break
        agg = aggregate(cur_cols, active, seed=len(levels))
        nc = int(agg.max()) + 1
        if nc >= 0.7 * n_active:                   # not coarsening any more (e.g. disconnected graph)
            break
        pat = coarse_pattern(cur_cols, agg)
        ptr, members = members_csr(agg, nc)
        pat.update(agg=agg.astype(np.int32), agg_ptr=ptr, agg_members=members)
        levels.append(pat)
        cur_cols = pat["cols"]
        active = np.ones(nc, dtype=bool)
    return levels


# ---------------------------------------------------------------------------------------------------------------------
# Smoothed aggregation (round 3): same aggregates, prolongation smoothed by one damped-Jacobi step of the UNIT-kappa
# operator, P = (I - omega D_1^-1 A_1) P_0.  P is batch-shared (built once per mesh from A_1); the coarse operators stay
# per sample, A_c^b = P^T A_b P, as WEIGHTED sums of fine entries (gather lists with weights P_iI P_jJ).  Halves the
# iteration count of the piecewise-constant hierarchy (256^2, CPU prototype: 68 -> 34) for ~1.6x denser coarse levels.
# ---------------------------------------------------------------------------------------------------------------------
def _ell_to_csr(cols: np.ndarray, vals: np.ndarray):
    """(csr matrix, ELL index k*n+i of every stored nonzero in csr order) from an ELL pattern (slot 0 = diagonal,
    padding slots point at the row itself)."""
    import scipy.sparse as sp
    W, n = cols.shape
    k_idx, i_idx = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    real = (k_idx == 0) | (cols != i_idx)
    r, c, e = i_idx[real], cols[real].astype(np.int64), (k_idx * n + i_idx)[real]
    order = np.lexsort((c, r))
    A = sp.csr_matrix((vals[real][order], (r[order], c[order])), shape=(n, n))
    A.sum_duplicates()
    assert A.nnz == len(order), "duplicate ELL entries"
    return A, e[order]


def _csr_to_ell(A):
    """ELL pattern (W, n) with slot 0 = diagonal for a square CSR matrix with a full diagonal; also the slot index k*n+i of
    every CSR nonzero (in CSR order)."""
    n = A.shape[0]
    A = A.tocsr()
    A.sort_indices()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr))
    colsA = A.indices.astype(np.int64)
    isd = colsA == rows
    # rank within the row with the diagonal first
    pos = np.arange(A.nnz) - A.indptr[rows]
    dpos = np.zeros(n, dtype=np.int64)
    dpos[rows[isd]] = pos[isd]
    slot = np.where(isd, 0, np.where(pos < dpos[rows], pos + 1, pos))
    W = int(slot.max()) + 1
    ell = np.tile(np.arange(n, dtype=np.int32), W).reshape(W, n)
    ell[slot, rows] = colsA.astype(np.int32)
    return ell, slot * n + rows


def smoothed_level(A1, ell_index_f, cols_f, active, seed, omega=2.0 / 3.0, drop=0.0, agg=None, AF=None):
    """One coarsening step.  A1: unit-kappa CSR matrix of the fine level; ell_index_f: ELL entry index (k*n_f + i) of each
    of its nonzeros (CSR order); cols_f: its ELL pattern (for the aggregation).  Returns the level dict (device arrays as
    numpy) and the coarse unit matrix with ITS ell index.
    Coefficient-aware hierarchy: A1 is the representative operator of the level, `agg` its aggregates on the strong graph
    and `AF` its strength-filtered matrix, which smooths the prolongation instead of A1 (rows of AF without an
    off-diagonal are not smoothed); the gather lists and the coarse matrix still run over the full pattern of A1."""
    import scipy.sparse as sp
    nf = A1.shape[0]
    if agg is None:
        agg = aggregate(cols_f, active, seed=seed)
    nc = int(agg.max()) + 1
    rows = np.nonzero(agg >= 0)[0]
    P0 = sp.csr_matrix((np.ones(len(rows)), (rows, agg[rows])), shape=(nf, nc))
    if AF is None:
        d = A1.diagonal()
        S = sp.identity(nf, format="csr") - sp.diags(omega / d) @ A1
    else:
        d = AF.diagonal()
        smooth = (np.diff(AF.indptr) > 1) & (d > 0)
        S = sp.identity(nf, format="csr") - sp.diags(np.where(smooth, omega / np.where(smooth, d, 1.0), 0.0)) @ AF
    P = (sp.diags((agg >= 0).astype(np.float64)) @ S @ P0).tocsr()       # inactive (Dirichlet) rows interpolate nothing
    if drop > 0.0:
        P.data[np.abs(P.data) < drop] = 0.0
    P.eliminate_zeros()
    P.sort_indices()
    # --- weighted Galerkin gather lists: coarse entry (I, J) = sum over fine nonzeros (i, j) of P_iI a_ij P_jJ.  The
    # coarse PATTERN is the set of (I, J) these lists reach (structural: a fine entry whose unit value happens to be
    # exactly 0 -- the quad diagonal of a right-angled lattice -- still carries a per-sample value) ---
    fi = np.repeat(np.arange(nf, dtype=np.int64), np.diff(A1.indptr))
    fj = A1.indices.astype(np.int64)
    pn = np.diff(P.indptr).astype(np.int64)
    keep = (pn[fi] > 0) & (pn[fj] > 0)
    fi, fj, fe, fa = fi[keep], fj[keep], ell_index_f[keep], A1.data[keep]
    ca = pn[fi]                                                    # expand over the nonzeros of P's row i ...
    t1 = np.repeat(np.arange(len(fi)), ca)
    a_loc = np.arange(len(t1)) - np.repeat(np.cumsum(ca) - ca, ca)
    pa = P.indptr[fi[t1]] + a_loc
    cb = pn[fj[t1]]                                                # ... then over those of row j
    t2 = np.repeat(np.arange(len(t1)), cb)
    b_loc = np.arange(len(t2)) - np.repeat(np.cumsum(cb) - cb, cb)
    pb = P.indptr[fj[t1[t2]]] + b_loc
    I, J = P.indices[pa[t2]].astype(np.int64), P.indices[pb].astype(np.int64)
    w = P.data[pa[t2]] * P.data[pb]
    fine_entry = fe[t1[t2]]
    # coarse unit matrix P^T A_1 P on that pattern (+ a structural diagonal for every coarse node)
    keys = np.concatenate([I * nc + J, np.arange(nc, dtype=np.int64) * (nc + 1)])
    data = np.concatenate([w * fa[t1[t2]], np.zeros(nc)])
    ckey, inv = np.unique(keys, return_inverse=True)
    cval = np.zeros(len(ckey))
    np.add.at(cval, inv, data)
    crow_u = ckey // nc
    indptr = np.zeros(nc + 1, dtype=np.int64)
    np.cumsum(np.bincount(crow_u, minlength=nc), out=indptr[1:])
    Ac = sp.csr_matrix((cval, (ckey % nc).astype(np.int32), indptr), shape=(nc, nc))
    cols_c, ell_index_c = _csr_to_ell(Ac)
    Wc = cols_c.shape[0]
    loc = inv[:len(I)]
    centry = ell_index_c[loc]
    order = np.argsort(centry, kind="stable")
    ent_ptr = np.zeros(Wc * nc + 1, dtype=np.int64)
    np.cumsum(np.bincount(centry, minlength=Wc * nc), out=ent_ptr[1:])
    if ent_ptr[-1] >= 2 ** 31:
        raise ValueError("mesh too large for int32 gather lists")
    # --- transfer operators for the device: P as ELL rows (prolongation), P^T as CSR (restriction) ---
    pw = int(pn.max()) if len(pn) else 1
    p_cols = np.full((pw, nf), -1, dtype=np.int32)
    p_vals = np.zeros((pw, nf), dtype=np.float64)
    prow = np.repeat(np.arange(nf, dtype=np.int64), pn)
    ploc = np.arange(P.nnz) - P.indptr[prow]
    p_cols[ploc, prow] = P.indices
    p_vals[ploc, prow] = P.data
    PT = P.T.tocsr()
    PT.sort_indices()
    level = dict(n=nc, W=Wc, cols=cols_c, ent_ptr=ent_ptr.astype(np.int32), contrib=fine_entry[order].astype(np.int32),
                 weights=w[order], agg=agg.astype(np.int32), agg_ptr=PT.indptr.astype(np.int32),
                 agg_members=PT.indices.astype(np.int32), agg_weights=PT.data.astype(np.float64),
                 p_cols=p_cols, p_vals=p_vals)
    return level, Ac, ell_index_c


def build_hierarchy_sa(cols: np.ndarray, unit_vals: np.ndarray, is_bc: np.ndarray, min_coarse: int = 64,
                       max_levels: int = 12, strength: float = 0.0, rep_vals: np.ndarray = None,
                       fine_filter=None) -> List[Dict]:
    """Smoothed-aggregation levels below the fine one.  cols (W, n), unit_vals (W, n): ELL pattern and UNIT-kappa values
    of the Dirichlet-eliminated fine matrix (identity rows on Dirichlet nodes).  Each dict: the coarse pattern and
    weighted Galerkin lists (n, W, cols, ent_ptr, contrib, weights) and the transfers from the level above (p_cols,
    p_vals: P as ELL rows; agg_ptr, agg_members, agg_weights: P^T as CSR; agg: the underlying aggregates).
    strength > 0: the coefficient-aware hierarchy of `rep_vals` (W, n), the representative operator of the batch in the
    same pattern (None: unit_vals) -- `_build_hierarchy_operator`.  fine_filter: (strong_cols, filtered values) of the
    fine level when the device has computed them already (diffhe_ell_strength_filter), else `strength_filter` does."""
    if strength and strength > 0.0:
        return _build_hierarchy_operator(cols, unit_vals if rep_vals is None else rep_vals, is_bc, float(strength),
                                         min_coarse, max_levels, fine_filter)
    levels: List[Dict] = []
    A1, ell_idx = _ell_to_csr(cols, unit_vals)
    active = ~is_bc.astype(bool)
    cur_cols = cols
    while len(levels) < max_levels - 1:
        n_active = int(active.sum())
        if n_active <= min_coarse:
            break
        lev, Ac, ell_c = smoothed_level(A1, ell_idx, cur_cols, active, seed=len(levels))
        if lev["n"] >= 0.7 * n_active:
            break
        levels.append(lev)
        A1, ell_idx, cur_cols = Ac, ell_c, lev["cols"]
        active = np.ones(lev["n"], dtype=bool)
    return levels


# ---------------------------------------------------------------------------------------------------------------------
# Coefficient-aware hierarchy (amg=dict(strength=theta)): aggregates on the graph of STRONG couplings of the operator
# that is being solved, prolongation smoothed by its strength-filtered matrix.  The classical recipe of smoothed
# aggregation (Vanek, Mandel, Brezina 1996), with a symmetrised row-relative strength measure.  Aggregates and P stay
# batch-shared: they come from ONE representative matrix (csrc/coarsen.hip), the per-sample coarse operators stay the
# exact P^T A_b P over the full pattern.
# ---------------------------------------------------------------------------------------------------------------------
def couplings(cols: np.ndarray, vals: np.ndarray, rows=None) -> np.ndarray:
    """c_ij = max(-a_ij, 0) / sqrt(a_ii a_jj) per slot, (W, n) -- or (W, len(rows)) for the given rows; 0 on the diagonal
    slot, on padding slots and where a_ii a_jj <= 0."""
    W, n = cols.shape
    i_idx = np.arange(n) if rows is None else np.asarray(rows)
    cj, a = (cols, vals) if rows is None else (cols[:, i_idx], vals[:, i_idx])
    real = (np.arange(W)[:, None] > 0) & (cj != i_idx[None, :])
    d = vals[0]
    prod = d[i_idx][None, :] * d[cj]
    ok = real & (prod > 0)
    c = np.zeros(cj.shape)
    c[ok] = np.maximum(-a[ok], 0.0) / np.sqrt(prod[ok])
    return c


def strength_filter(cols: np.ndarray, vals: np.ndarray, theta: float):
    """numpy restatement of diffhe_ell_strength_filter (include/diffhe_hip.h), operation for operation: -> (strong_cols
    (W, n) int32 with weak and padding slots pointing at the row itself, filtered values (W, n) with the weak
    off-diagonals lumped to the diagonal in slot order)."""
    W, n = cols.shape
    i_idx = np.arange(n)[None, :]
    real = (np.arange(W)[:, None] > 0) & (cols != i_idx)
    c = couplings(cols, vals)
    own = real & (c > 0) & (c >= theta * c.max(axis=0)[None, :])
    back = np.zeros((W, n), dtype=bool)              # does row j = cols[k, i] call i strong?
    for kk in range(1, W):
        back |= (cols[kk][cols] == i_idx) & own[kk][cols]
    strong = own & back & real
    filt = np.where(strong, vals, 0.0)
    diag = vals[0].copy()
    for k in range(1, W):
        diag = diag + np.where(real[k] & ~strong[k], vals[k], 0.0)
    filt[0] = diag
    strong_cols = np.where(strong, cols, np.broadcast_to(i_idx, (W, n))).astype(np.int32)
    return strong_cols, filt


def aggregate_strong(strong_cols: np.ndarray, cols: np.ndarray, vals: np.ndarray, active: np.ndarray,
                     seed: int = 0) -> np.ndarray:
    """`aggregate` on the strong graph.  A node without a strong neighbour is no root: it joins the adjacent aggregate
    (full pattern) it is most strongly coupled to; only a node with no aggregated neighbour at all stays a singleton."""
    n = cols.shape[1]
    has = (strong_cols != np.arange(n)[None, :]).any(axis=0)
    agg = aggregate(strong_cols, active & has, seed=seed)
    lone = np.nonzero(active & ~has)[0]
    for _ in range(8):
        if not len(lone):
            break
        nb = agg[cols[:, lone]]                      # the node's own slots read -1: it has no aggregate yet
        score = np.where(nb >= 0, couplings(cols, vals, lone), -1.0)
        best = score.argmax(axis=0)
        ar = np.arange(len(lone))
        ok = score[best, ar] >= 0.0
        if not ok.any():
            break
        agg[lone[ok]] = nb[best, ar][ok]
        lone = lone[~ok]
    if len(lone):
        agg[lone] = int(agg.max()) + 1 + np.arange(len(lone))
    return agg


def _build_hierarchy_operator(cols, rep_vals, is_bc, theta, min_coarse, max_levels, fine_filter):
    """Levels of the coefficient-aware hierarchy: per level, strength filter at theta * 0.5^l -> aggregates on the strong
    graph -> P = (I - omega D_F^-1 A_F) P_0 -> weighted gather lists over the FULL pattern -> coarse representative
    P^T Abar P, the next level's operator."""
    levels: List[Dict] = []
    rep_vals = np.ascontiguousarray(rep_vals, dtype=np.float64)
    A1, ell_idx = _ell_to_csr(cols, rep_vals)
    active = ~is_bc.astype(bool)
    cur_cols, cur_vals = cols, rep_vals
    while len(levels) < max_levels - 1:
        n_active = int(active.sum())
        if n_active <= min_coarse:
            break
        if fine_filter is not None and not levels:
            strong_cols, filt = fine_filter
        else:
            strong_cols, filt = strength_filter(cur_cols, cur_vals, theta * 0.5 ** len(levels))
        agg = aggregate_strong(strong_cols, cur_cols, cur_vals, active, seed=len(levels))
        AF, _ = _ell_to_csr(cur_cols, np.ascontiguousarray(filt))
        AF.eliminate_zeros()
        lev, Ac, ell_c = smoothed_level(A1, ell_idx, cur_cols, active, seed=len(levels), agg=agg, AF=AF)
        if lev["n"] >= 0.7 * n_active:
            break
        lev["lam_parent"], lev["lam"] = jacobi_bound(A1), jacobi_bound(Ac)
        levels.append(lev)
        A1, ell_idx, cur_cols = Ac, ell_c, lev["cols"]
        cur_vals = np.zeros(lev["W"] * lev["n"])
        cur_vals[ell_c] = Ac.data
        cur_vals = cur_vals.reshape(lev["W"], lev["n"])
        active = np.ones(lev["n"], dtype=bool)
    return levels


def jacobi_bound(A, safety: float = 1.1) -> float:
    """safety x lambda_max(D^-1 A) of a symmetric CSR matrix with a positive diagonal: what the cycle's Jacobi weights
    have to cover on this level.  2.05 for a scalar kappa on a reasonable mesh; positive off-diagonals (anisotropic
    tensors, obtuse triangles) raise it.  Lanczos from a fixed start vector (deterministic); capped by Gershgorin."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    n = A.shape[0]
    d = A.diagonal()
    if n == 0 or not np.all(d > 0):
        return 0.0
    gersh = float((np.asarray(abs(A).sum(axis=1)).reshape(-1) / d).max())
    Dm = sp.diags(1.0 / np.sqrt(d))
    M = (Dm @ A @ Dm).tocsr()
    if n <= 64:
        lam = float(np.linalg.eigvalsh(M.toarray())[-1])
    else:
        try:
            lam = float(spla.eigsh(M, k=1, which="LA", tol=1e-3, v0=np.ones(n), return_eigenvectors=False)[0])
        except spla.ArpackNoConvergence:
            return gersh
    return min(safety * lam, gersh)


# ---------------------------------------------------------------------------------------------------------------------
# Vector-valued unknowns (diffhe.elastic): d components per node, dof = node * d + component on the fine level.  The
# aggregates are NODE aggregates expanded per component, so no aggregate mixes components and the tentative prolongation
# is P_node (x) I_d: it carries the d translations exactly (no rotations).  Coarse dofs keep a (node, component) label --
# coarse node = aggregate of nodes -- so the rule recurses.  An (aggregate, component) pair whose members are all fixed
# gets no coarse dof: coarse dofs are numbered over the pairs that have a free member, sorted by (node, component).
# ---------------------------------------------------------------------------------------------------------------------
def node_graph(cols: np.ndarray, node_of: np.ndarray, n_nodes: int) -> np.ndarray:
    """ELL pattern (slot 0 = the node itself, unused slots point at the node itself) of the node graph under a dof
    pattern `cols` (W, n): nodes I != J are adjacent when some dof of I couples to some dof of J."""
    import scipy.sparse as sp
    W, n = cols.shape
    r = np.broadcast_to(node_of[None, :], (W, n)).reshape(-1)
    c = node_of[cols.reshape(-1)]
    A = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n_nodes, n_nodes))
    A = (A + sp.identity(n_nodes, format="csr")).tocsr()
    A.sum_duplicates()
    return _csr_to_ell(A)[0]


def build_hierarchy_blocks(cols: np.ndarray, unit_vals: np.ndarray, is_bc: np.ndarray, d: int, min_coarse: int = 64,
                           max_levels: int = 12) -> List[Dict]:
    """Smoothed-aggregation levels below the fine one for d unknowns per node.  cols (W, n), unit_vals (W, n): ELL pattern
    and unit-coefficient values of the Dirichlet-eliminated fine matrix over the n = nodes * d dofs, dof = node * d +
    component; is_bc (n,) per dof.  Per level: `aggregate` on the node graph (a node is active when one of its dofs is),
    the aggregates expanded per component, the prolongation smoothed with the level's unit operator
    (`smoothed_level(..., agg=...)`).  Level dicts as `build_hierarchy_sa` returns them, plus `node` / `comp` (the label
    of every coarse dof) and `lam_parent` / `lam`: `jacobi_bound` of the unit operator above and on this level -- these
    operators have positive off-diagonals, the cycle's Jacobi weights need the bound (diffhe_amg_level.reserved)."""
    levels: List[Dict] = []
    A1, ell_idx = _ell_to_csr(cols, np.ascontiguousarray(unit_vals, dtype=np.float64))
    n = cols.shape[1]
    node_of, comp_of = np.arange(n, dtype=np.int64) // d, np.arange(n, dtype=np.int64) % d
    active = ~is_bc.astype(bool)
    cur_cols = cols
    lam_parent = jacobi_bound(A1)
    while len(levels) < max_levels - 1:
        n_active = int(active.sum())
        if n_active <= min_coarse:
            break
        n_nodes = int(node_of.max()) + 1
        node_active = np.zeros(n_nodes, dtype=bool)
        node_active[node_of[active]] = True
        agg_node = aggregate(node_graph(cur_cols, node_of, n_nodes), node_active, seed=len(levels))
        pair = agg_node[node_of] * d + comp_of                      # (aggregate, component) of every dof
        label, inv = np.unique(pair[active], return_inverse=True)   # ... numbered over the pairs with a free member
        agg = np.full(len(node_of), -1, dtype=np.int64)
        agg[active] = inv.reshape(-1)
        lev, Ac, ell_c = smoothed_level(A1, ell_idx, cur_cols, active, seed=len(levels), agg=agg)
        if lev["n"] >= 0.7 * n_active:
            break
        lev["node"], lev["comp"] = (label // d).astype(np.int64), (label % d).astype(np.int64)
        lev["lam_parent"], lev["lam"] = lam_parent, jacobi_bound(Ac)
        levels.append(lev)
        A1, ell_idx, cur_cols, lam_parent = Ac, ell_c, lev["cols"], lev["lam"]
        node_of, comp_of = lev["node"], lev["comp"]
        active = np.ones(lev["n"], dtype=bool)
    return levels


def hierarchy_stats(cols: np.ndarray, levels: List[Dict]):
    """(number of levels, the fine one included; operator complexity sum_l nnz_l / nnz_0) of a hierarchy."""
    def nnz(c):
        c = np.asarray(c)
        return int(c.shape[1] + (c[1:] != np.arange(c.shape[1])[None, :]).sum())
    n0 = nnz(cols)
    return len(levels) + 1, float((n0 + sum(nnz(lv["cols"]) for lv in levels)) / n0)
