"""A plain numpy model of the boundary-band operations (csrc/bc.hip, csrc/robin.hip, csrc/elastic_facets.hip) and of the
host tables they run over (diffhe/plan.py: dirichlet_band, robin_table, elastic_facet_table).  No GPU, no torch.

Every function is written from the formula in the unit's header comment: values are float64, every product and sum is
carried in `dt` (np.longdouble unless a test asks for float64 to measure the model's own rounding).  A function returns
the value and S, the same expression evaluated on absolute values (every subtraction an addition): S scales the
tolerances of tests/test_boundary_band.py.

Conventions: fac (d, nF) int, coords (dim, n), nodal fields (rows, B), facet data (nF, B) or None (absent), traction
(nF, d, B).  An assembled operator comes as its nonzero couplings: `pairs` (P, 2) = (row, column), sorted, and values
(P, B); `dense` scatters them into (B, N, N)."""
import numpy as np

LD = np.longdouble


def _abs_pair(f):
    """f(A, neg): the expression with A = identity, neg = -1, and with A = abs, neg = +1."""
    return f(lambda a: a, -1.0), f(np.abs, 1.0)


def _col(x, dt):
    return None if x is None else np.asarray(x, dtype=dt)


# ---------------------------------------------------------------------------------------------------------------------
# facet tables
# ---------------------------------------------------------------------------------------------------------------------
def _edges(coords, fac, A, dt):
    """a = x1 - x0 and (3D) b = x2 - x0 as (dim, nF); on absolute values a difference is a sum."""
    X = np.asarray(coords, dtype=dt)
    minus = (lambda x, y: x - y) if A(-1.0) < 0 else (lambda x, y: x + y)
    a = minus(A(X[:, fac[1]]), A(X[:, fac[0]]))
    b = minus(A(X[:, fac[2]]), A(X[:, fac[0]])) if fac.shape[0] == 3 else None
    return a, b, minus


def _normal_vector(coords, fac, A, dt):
    """The unnormalised normal (dim, nF): (dy, -dx) of an edge, a x b of a triangle."""
    a, b, minus = _edges(coords, fac, A, dt)
    if fac.shape[0] == 2:
        return np.stack([a[1], A(-1.0) * a[0]]), a, b
    return np.stack([minus(a[1] * b[2], a[2] * b[1]), minus(a[2] * b[0], a[0] * b[2]), minus(a[0] * b[1], a[1] * b[0])]), a, b


def _norm(nv, nva):
    """|nv| and its S: the square root turns an error dx of x = |nv|^2 into dx / (2 |nv|), so S = sum(nva^2) / |nv|, which
    is at least the root of sum(nva^2) (0 where |nv| = 0: such a facet is degenerate by either threshold)."""
    nrm = np.sqrt((nv * nv).sum(0))
    return nrm, np.where(nrm > 0, (nva * nva).sum(0) / np.where(nrm > 0, nrm, 1), 0)


def facet_area(coords, fac, dt=LD):
    """|F| (nF) and S: 1 for an end point, the length of an edge (0 below 1e-15), half |a x b| of a triangle (0 when
    |a x b| <= 1e-12 max(|a|^2, |b|^2))."""
    d, nF = fac.shape
    if d == 1:
        return np.ones(nF, dtype=dt), np.ones(nF, dtype=dt)
    nv, a, b = _normal_vector(coords, fac, lambda x: x, dt)
    nva = _normal_vector(coords, fac, np.abs, dt)[0]
    nrm, S = _norm(nv, nva)
    if d == 2:
        ok = nrm >= dt(1e-15)
        return np.where(ok, nrm, 0), np.where(ok, S, 0)
    ok = nrm > dt(1e-12) * np.maximum((a * a).sum(0), (b * b).sum(0))
    return np.where(ok, nrm / 2, 0), np.where(ok, S / 2, 0)


def facet_normal(coords, fac, opp, dt=LD):
    """-> (area, S_area, normal (d, nF), S_normal, out, S_out): the unit normal oriented away from the node `opp`, 0 for a
    degenerate facet; out = (x_0 - x_opp) . nv decides the sign (out >= 0: nv itself) -- a facet whose |out| is within
    rounding of 0 (S_out) has no defined orientation.  S_normal bounds d(nv / |nv|): |d nv| / |nv| + |n| d|nv| / |nv|."""
    area, S_area = facet_area(coords, fac, dt)
    nv = _normal_vector(coords, fac, lambda x: x, dt)[0]
    nva = _normal_vector(coords, fac, np.abs, dt)[0]
    X = np.asarray(coords, dtype=dt)
    out = ((X[:, fac[0]] - X[:, opp]) * nv).sum(0)
    S_out = ((np.abs(X[:, fac[0]]) + np.abs(X[:, opp])) * nva).sum(0)
    nrm, S_nrm = _norm(nv, nva)
    live = area > 0
    safe = np.where(live, nrm, 1)
    sign = np.where(out >= 0, 1, -1)
    normal = np.where(live, sign * nv / safe, 0)
    S_normal = np.where(live, nva / safe + np.abs(nv) * S_nrm / (safe * safe), 0)
    return area, S_area, normal, S_normal, out, S_out


def facet_mass(d, dt=LD):
    """M_F / |F|: (1 + delta_pq) / (d (d + 1))."""
    return (np.ones((d, d), dtype=dt) + np.eye(d, dtype=dt)) / dt(d * (d + 1))


# ---------------------------------------------------------------------------------------------------------------------
# assembled operators as coupling lists
# ---------------------------------------------------------------------------------------------------------------------
class _Couplings:
    """Sums contributions (row, col) -> (B,) values; rows and cols index N unknowns."""

    def __init__(self, N, rows, cols, B, dt):
        self.N = N
        keys = np.unique(np.concatenate([np.asarray(r, dtype=np.int64) * N + np.asarray(c, dtype=np.int64)
                                         for r, c in zip(rows, cols)]) if rows else np.zeros(0, dtype=np.int64))
        self.keys = keys
        self.val, self.S = np.zeros((len(keys), B), dtype=dt), np.zeros((len(keys), B), dtype=dt)

    def add(self, r, c, v, s):
        at = np.searchsorted(self.keys, np.asarray(r, dtype=np.int64) * self.N + np.asarray(c, dtype=np.int64))
        np.add.at(self.val, at, v)
        np.add.at(self.S, at, s)

    def result(self):
        return np.stack([self.keys // self.N, self.keys % self.N], 1), self.val, self.S


def dense(pairs, val, N):
    """(B, N, N) of a coupling list."""
    out = np.zeros((val.shape[1], N, N), dtype=val.dtype)
    out[:, pairs[:, 0], pairs[:, 1]] = val.T
    return out


def pair_index(pairs, N, row, col):
    """Position of the couplings (row, col) in `pairs`, -1 where absent."""
    keys = pairs[:, 0] * N + pairs[:, 1]
    want = np.asarray(row, dtype=np.int64) * N + np.asarray(col, dtype=np.int64)
    at = np.searchsorted(keys, want)
    at = np.minimum(at, max(len(keys) - 1, 0))
    return np.where(keys[at] == want, at, -1) if len(keys) else np.full(want.shape, -1)


# ---------------------------------------------------------------------------------------------------------------------
# Robin
# ---------------------------------------------------------------------------------------------------------------------
def robin_system(fac, area, is_bc, g, h, uinf, q, n, B, dt=LD):
    """What sum_F h_F M_F and the facet loads add to a system with Dirichlet nodes `is_bc` (values g):
    -> (pairs, A (P, B), S_A, rhs (n, B), S_rhs).  Free rows only; a Dirichlet column goes to the right-hand side with
    its value; rhs_p += (h u_inf + q) |F| / d.  h, uinf, q: (nF, B), (nF, 1) or None."""
    d, nF = fac.shape
    area, g, h, uinf, q = (_col(x, dt) for x in (area, g, h, uinf, q))
    M = facet_mass(d, dt)
    ones = np.ones((1, B), dtype=dt)
    free = [~is_bc[fac[p]] for p in range(d)]
    todo = [(p, c) for p in range(d) for c in range(d)] if h is not None else []
    A = _Couplings(n, [fac[p][free[p] & ~is_bc[fac[c]]] for p, c in todo], [fac[c][free[p] & ~is_bc[fac[c]]] for p, c in todo],
                   B, dt)
    rhs, S_rhs = np.zeros((n, B), dtype=dt), np.zeros((n, B), dtype=dt)
    for p, c in todo:
        m = h * (area * M[p, c])[:, None] * ones                     # (nF, B)
        keep = free[p] & ~is_bc[fac[c]]
        A.add(fac[p][keep], fac[c][keep], m[keep], np.abs(m[keep]))
        lift = free[p] & is_bc[fac[c]]
        t = m[lift] * g[fac[c][lift]][:, None]
        np.add.at(rhs, fac[p][lift], -t)
        np.add.at(S_rhs, fac[p][lift], np.abs(t))
    for p in range(d):
        t = np.zeros((nF, B), dtype=dt)
        s = np.zeros((nF, B), dtype=dt)
        if h is not None and uinf is not None:
            t, s = t + h * uinf, s + np.abs(h * uinf)
        if q is not None:
            t, s = t + q, s + np.abs(q)
        w = (area / dt(d))[:, None]
        np.add.at(rhs, fac[p][free[p]], (t * w)[free[p]])
        np.add.at(S_rhs, fac[p][free[p]], (s * w)[free[p]])
    return (*A.result(), rhs, S_rhs)


def robin_grads(fac, area, lam, u, g, h, uinf, dt=LD):
    """Per facet and sample, from the adjoint lam (n, B) and u + g: s = (|F| / d) sum_p lam_p,
    dq = s, du_inf = h s, dh = -lam_F^T M_F u_F + u_inf s.  -> {name: (value (nF, B), S)}."""
    d, nF = fac.shape
    area, lam, u, h, uinf = (_col(x, dt) for x in (area, lam, u, h, uinf))
    g = np.zeros(lam.shape[0], dtype=dt) if g is None else _col(g, dt)
    M = facet_mass(d, dt)

    def f(A, neg):
        le = [A(lam[fac[p]]) for p in range(d)]
        ue = [A(u[fac[p]]) + A(g[fac[p]])[:, None] for p in range(d)]
        w = area[:, None]
        s = sum(le) * (w / dt(d))
        lmu = sum(le[p] * M[p, c] * ue[c] for p in range(d) for c in range(d)) * w
        hv = A(h) if h is not None else 0 * s
        uv = A(uinf) if uinf is not None else 0 * s
        return {"dh": neg * lmu + uv * s, "du": hv * s, "dq": s + 0 * lmu}

    val, S = _abs_pair(f)
    return {k: (val[k], S[k]) for k in val}


# ---------------------------------------------------------------------------------------------------------------------
# elastic facets
# ---------------------------------------------------------------------------------------------------------------------
def elastic_system(fac, area, normal, is_bc, g, t, p, kn, kt, n, B, dt=LD):
    """What the foundation blocks M_F[p, c] S_F, S_F = kn n n^T + kt (I - n n^T), and the loads (t - p n) |F| / d add to
    an elastic system with fixed dofs `is_bc` (n d) (values g): -> (pairs over dofs, A (P, B), S_A, rhs (n d, B), S_rhs).
    Fixed rows are skipped, fixed columns lifted.  t (nF, d, B) / (nF, d, 1), p, kn, kt (nF, B) / (nF, 1), or None."""
    d, nF = fac.shape
    area, normal, g, t, p, kn, kt = (_col(x, dt) for x in (area, normal, g, t, p, kn, kt))
    is_bc = np.asarray(is_bc, dtype=bool)
    M = facet_mass(d, dt)
    N = n * d
    ones = np.ones((1, B), dtype=dt)
    stiff = kn is not None or kt is not None
    zero = np.zeros((nF, 1), dtype=dt)
    knv, ktv = (kn if kn is not None else zero), (kt if kt is not None else zero)
    todo = [(pp, c, a, b) for pp in range(d) for c in range(d) for a in range(d) for b in range(d)] if stiff else []
    rowcol = lambda pp, c, a, b: (fac[pp] * d + a, fac[c] * d + b)                                   # noqa: E731
    sel = []
    for pp, c, a, b in todo:
        r, cc = rowcol(pp, c, a, b)
        sel.append(~is_bc[r] & ~is_bc[cc])
    A = _Couplings(N, [rowcol(*x)[0][k] for x, k in zip(todo, sel)], [rowcol(*x)[1][k] for x, k in zip(todo, sel)], B, dt)
    rhs, S_rhs = np.zeros((N, B), dtype=dt), np.zeros((N, B), dtype=dt)
    for (pp, c, a, b), keep in zip(todo, sel):
        r, cc = rowcol(pp, c, a, b)
        nn = (normal[a] * normal[b])[:, None]
        w = (area * M[pp, c])[:, None]
        v = (knv * nn + ktv * ((1 if a == b else 0) - nn)) * w * ones
        s = (np.abs(knv) * np.abs(nn) + np.abs(ktv) * ((1 if a == b else 0) + np.abs(nn))) * w * ones
        A.add(r[keep], cc[keep], v[keep], s[keep])
        lift = ~is_bc[r] & is_bc[cc]
        gl = g[cc[lift]][:, None]
        np.add.at(rhs, r[lift], -v[lift] * gl)
        np.add.at(S_rhs, r[lift], s[lift] * np.abs(gl))
    for pp in range(d):
        for a in range(d):
            r = fac[pp] * d + a
            v, s = np.zeros((nF, B), dtype=dt), np.zeros((nF, B), dtype=dt)
            if t is not None:
                v, s = v + t[:, a], s + np.abs(t[:, a])
            if p is not None:
                v, s = v - p * normal[a][:, None], s + np.abs(p * normal[a][:, None])
            w = (area / dt(d))[:, None]
            keep = ~is_bc[r]
            np.add.at(rhs, r[keep], (v * w)[keep])
            np.add.at(S_rhs, r[keep], (s * w)[keep])
    return (*A.result(), rhs, S_rhs)


def elastic_grads(fac, area, normal, lam, u, g, dt=LD):
    """Per facet and sample, from the adjoint lam (n d, B) and u + g: s = (|F| / d) sum_p lam_p (a vector),
    dt = s, dp = -s . n, dkn = -sum M_F[p, q] (lam_p . n)(u_q . n), dkt = -sum M_F[p, q] lam_p . u_q - dkn.
    -> {name: (value, S)}; dt is (nF, d, B), the others (nF, B)."""
    d, nF = fac.shape
    area, normal, lam, u = (_col(x, dt) for x in (area, normal, lam, u))
    g = np.zeros(lam.shape[0], dtype=dt) if g is None else _col(g, dt)
    M = facet_mass(d, dt)

    def f(A, neg):
        le = [[A(lam[fac[p] * d + a]) for a in range(d)] for p in range(d)]
        ue = [[A(u[fac[p] * d + a]) + A(g[fac[p] * d + a])[:, None] for a in range(d)] for p in range(d)]
        nv = [A(normal[a])[:, None] for a in range(d)]
        w = area[:, None]
        s = [sum(le[p][a] for p in range(d)) * (w / dt(d)) for a in range(d)]
        ln = [sum(le[p][a] * nv[a] for a in range(d)) for p in range(d)]
        un = [sum(ue[p][a] * nv[a] for a in range(d)) for p in range(d)]
        nn = sum(M[p, c] * ln[p] * un[c] for p in range(d) for c in range(d)) * w
        full = sum(M[p, c] * le[p][a] * ue[c][a] for p in range(d) for c in range(d) for a in range(d)) * w
        # on absolute values dkt = |full| + |nn|; as a value -full + nn
        return {"dt": np.stack(s, 1), "dp": neg * sum(s[a] * nv[a] for a in range(d)), "dkn": neg * nn,
                "dkt": (nn - full) if neg < 0 else (nn + full)}

    val, S = _abs_pair(f)
    return {k: (val[k], S[k]) for k in val}


def dof_slot(k, a, b, d):
    """The dof slot of include/diffhe_elastic.h: row component a, node slot k, column component b."""
    return (b - a + d) % d if k == 0 else k * d + b


# ---------------------------------------------------------------------------------------------------------------------
# per-sample Dirichlet values
# ---------------------------------------------------------------------------------------------------------------------
def _k_terms(elems, k0, kappa, is_d, row_d, col_d, B, dt):
    """The terms of the UNREDUCED K_b[i, j] = sum_e kappa_eb k0_e[p, q] with row i Dirichlet == row_d and column j
    Dirichlet == col_d: yields (e-mask, p, q, coefficient (count, B))."""
    npe, m = elems.shape
    k0 = _col(k0, dt)
    kap = np.ones((m, 1), dtype=dt) if kappa is None else _col(kappa, dt)
    for p in range(npe):
        for q in range(npe):
            keep = (is_d[elems[p]] == row_d) & (is_d[elems[q]] == col_d)
            if keep.any():
                yield keep, p, q, kap[keep] * k0[p * npe + q][keep][:, None] * np.ones((1, B), dtype=dt)


def bc_lift(elems, k0, kappa, is_d, d_slot, G, n, dt=LD):
    """(K_b[F, D] G_b) (n, B) and S: what diffhe_bc_lift subtracts from the free rows.  kappa (m, B), (m, 1) or None
    (unit); G (n_D, B)."""
    G = _col(G, dt)
    B = G.shape[1]
    acc, S = np.zeros((n, B), dtype=dt), np.zeros((n, B), dtype=dt)
    for keep, p, q, coef in _k_terms(elems, k0, kappa, is_d, False, True, B, dt):
        t = coef * G[d_slot[elems[q][keep]]]
        np.add.at(acc, elems[p][keep], t)
        np.add.at(S, elems[p][keep], np.abs(t))
    return acc, S


def bc_grad(elems, k0, kappa, is_d, d_idx, d_slot, lam, gbar, G, dt=LD):
    """-> (out (n_D, B), S_out, dots (n_D, B), S_dots): out_b[j] = gbar_b[j] - (K_b lam_b)_j on the Dirichlet nodes with
    lam = 0 on them, dots_b[j] = G_b[j] (K_1 lam_b)_j with the unit-kappa K_1.  gbar (n, B) or None, G (n_D, B) or None."""
    lam = _col(lam, dt)
    B = lam.shape[1]
    nD = len(d_idx)
    kl, S, unit, Su = (np.zeros((nD, B), dtype=dt) for _ in range(4))
    for kap, tgt, St in ((kappa, kl, S), (None, unit, Su)):
        for keep, p, q, coef in _k_terms(elems, k0, kap, is_d, True, False, B, dt):
            t = coef * lam[elems[q][keep]]
            np.add.at(tgt, d_slot[elems[p][keep]], t)
            np.add.at(St, d_slot[elems[p][keep]], np.abs(t))
    gb = np.zeros((nD, B), dtype=dt) if gbar is None else _col(gbar, dt)[d_idx]
    if G is None:
        return gb - kl, np.abs(gb) + S, None, None
    G = _col(G, dt)
    return gb - kl, np.abs(gb) + S, G * unit, np.abs(G) * Su


def bc_grad_kappa(elems, k0, is_d, d_slot, lam, G, dt=LD):
    """lam_b^T k0_e G_b (m, B) and S: what diffhe_bc_grad_kappa subtracts from dk (rows lam on free nodes, columns G on
    Dirichlet nodes; 0 on an element that touches no Dirichlet node, or only such nodes)."""
    lam, G = _col(lam, dt), _col(G, dt)
    B = lam.shape[1]
    m = elems.shape[1]
    acc, S = np.zeros((m, B), dtype=dt), np.zeros((m, B), dtype=dt)
    for keep, p, q, coef in _k_terms(elems, k0, None, is_d, False, True, B, dt):
        t = lam[elems[p][keep]] * coef * G[d_slot[elems[q][keep]]]
        acc[keep] += t
        S[keep] += np.abs(t)
    return acc, S


# ---------------------------------------------------------------------------------------------------------------------
# the two-stage facet sum, in the kernel's order (additions only: bitwise)
# ---------------------------------------------------------------------------------------------------------------------
SUM_CHUNK = 128


def sum_blocks(nF):
    return 0 if nF < 1 else (nF + SUM_CHUNK - 1) // SUM_CHUNK


def sum_facets(src):
    """src (nF, B) float64 -> (part (blocks, B), out (B)): chunks of 128 rows added in row order, then the chunk sums
    added in order, all in float64."""
    src = np.asarray(src, dtype=np.float64)
    nF, B = src.shape
    part = np.zeros((sum_blocks(nF), B))
    for k in range(part.shape[0]):
        s = np.zeros(B)
        for r in range(k * SUM_CHUNK, min((k + 1) * SUM_CHUNK, nF)):
            s = s + src[r]
        part[k] = s
    out = np.zeros(B)
    for k in range(part.shape[0]):
        out = out + part[k]
    return part, out


# ---------------------------------------------------------------------------------------------------------------------
# band tables, by brute force
# ---------------------------------------------------------------------------------------------------------------------
def _slot_of(cols, row, col):
    """The first slot k with cols[k, row] == col, or None."""
    for k in range(cols.shape[0]):
        if cols[k, row] == col:
            return k
    return None


def _facet_table(facets, cols, is_bc):
    """Rows, per row the entries (F, p, c) in facet order; is_bc None: every node on a facet is a row and no column is
    lifted (the elastic table)."""
    nF, d = facets.shape
    per_row = {}
    for F in range(nF):
        for p in range(d):
            row = int(facets[F, p])
            if is_bc is not None and is_bc[row]:
                continue
            for c in range(d):
                col = int(facets[F, c])
                if is_bc is not None and is_bc[col]:
                    slot = -1
                else:
                    slot = _slot_of(cols, row, col)
                    if slot is None:
                        return None
                per_row.setdefault(row, []).append((F * 16 + p * 4 + c, slot))
    rows = sorted(per_row)
    row_ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    code, slot = [], []
    for k, r in enumerate(rows):
        code += [e[0] for e in per_row[r]]
        slot += [e[1] for e in per_row[r]]
        row_ptr[k + 1] = len(code)
    i32 = lambda a: np.asarray(a, dtype=np.int32)                    # noqa: E731
    return dict(d=d, n_f=nF, fac=i32(facets.T).copy(), rows=i32(rows), n_rows=len(rows), row_ptr=row_ptr, ent_code=i32(code),
                ent_slot=i32(slot))


def robin_table(facets, is_bc, cols):
    """SolvePlan.robin_table without the device arrays: facets (nF, d), cols (W, n).  None when a coupling of a free row
    and a free column has no slot."""
    return _facet_table(np.asarray(facets), np.asarray(cols), np.asarray(is_bc, dtype=bool))


def elastic_table(facets, cols):
    """SolvePlan.elastic_facet_table without the device arrays: every node on a facet is a row, no slot is -1."""
    return _facet_table(np.asarray(facets), np.asarray(cols), None)


def dirichlet_band(elements, is_bc):
    """SolvePlan.dirichlet_band without the device arrays: elements (m, npe), is_bc (n) bool."""
    elements, is_bc = np.asarray(elements), np.asarray(is_bc, dtype=bool)
    m, npe = elements.shape
    n = len(is_bc)
    d_idx = [i for i in range(n) if is_bc[i]]
    d_slot = np.full(n, -1, dtype=np.int32)
    for j, i in enumerate(d_idx):
        d_slot[i] = j
    inc = {}
    band = []
    for e in range(m):
        if not any(is_bc[v] for v in elements[e]):
            continue
        band.append(e)
        for p in range(npe):
            inc.setdefault(int(elements[e, p]), []).append(e * npe + p)
    rows = sorted(i for i in inc if not is_bc[i])

    def csr(nodes):
        ptr, flat = np.zeros(len(nodes) + 1, dtype=np.int32), []
        for k, i in enumerate(nodes):
            flat += inc.get(i, [])
            ptr[k + 1] = len(flat)
        return ptr, np.asarray(flat, dtype=np.int32)

    row_ptr, row_inc = csr(rows)
    d_ptr, d_inc = csr(d_idx)
    i32 = lambda a: np.asarray(a, dtype=np.int32)                    # noqa: E731
    return dict(n_d=len(d_idx), d_idx=i32(d_idx), d_slot=d_slot, rows=i32(rows), n_rows=len(rows), row_ptr=row_ptr,
                row_inc=row_inc, d_ptr=d_ptr, d_inc=d_inc, band_elems=i32(band), n_be=len(band))
