"""The boundary-band kernels through their thirteen ABI entries -- diffhe_bc_lift / _grad / _scatter / _grad_kappa
(csrc/bc.hip), diffhe_robin_facet_table / _assemble / _grad / _sum_blocks / _sum_facets (csrc/robin.hip) and
diffhe_elastf_facet_table / _assemble / _grad (csrc/elastic_facets.hip) -- called directly on seeded synthetic inputs:
random facet and element lists into n nodes, random coordinates, fields and Dirichlet subsets, band tables from the
brute-force builders of tests/_band_model.py; no mesh, no plan, no solve.  The host builders of diffhe/plan.py
(dirichlet_band, robin_table, elastic_facet_table) are held against the same brute-force builders on small real meshes.

The reference is tests/_band_model.py: the formulas of the unit headers in numpy, values float64, sums longdouble.  The
CPU tests at the top pin that model to the dense restatements of test_robin.py, test_elastic_facets.py and
test_dirichlet_grad.py (operator, load and autograd gradients) and measure its own rounding.

Tolerances are derived by the method of tests/test_element_grad.py: |kernel - model| <= c * 2^-53 * S, S the model's
expression on absolute values, c the roundings on the longest chain from an input to the result, counted for the
kernel and for a float64 evaluation of the model's formula; a row that sums k terms adds k, a sum over the batch B.
With d nodes per facet, npe per element, inv_d = 1 / d and inv_dd = 1 / (d (d + 1)) rounded once each:

  facet tables     area: x1 - x0, the products of the cross product, their difference, the squares, two additions, the
                   root (the half is exact): 7, and 7 for the model: c = 14 on S_area (S of the squared norm over the
                   norm: the root divides an error by 2 |nv|).  normal: the sign over the norm and the product on top:
                   9 + 9 = 18 on S_normal.  An end point's |F| = 1 and a degenerate facet's zeros are exact.
  robin_assemble   vals: inv_dd, a * inv_dd (the factor 2 is exact), times h: 3, the model's |F| M[p, c] h the same:
                   c = 6 + k, k = the entries of the band row + 1 (the value already in vals).
                   rhs: h * u_inf, + q, (a * inv_d: 2, in parallel), the product: 5 (a lifted term, 3 + 1, is shorter):
                   c = 10 + k.
  robin_grad       u + g, the d - 1 additions of sum_p, the product sl * su, + lu, times a * inv_dd, u_inf s - .: d + 4,
                   taken as d + 5: c = 2 (d + 5), + B for an output summed over the batch.
  elastf_assemble  vals: kn - kt, n_a n_q, their product, + kt: 3 on the longest path, a * inv_dd beside it, the
                   product: 4; the model's kn nn + kt (delta - nn) times |F| M: 5: c = 9 + k, k = the entries of the band
                   node + 1.  rhs: a lifted term is the above times g: 5 and 6; every entry lifts up to d columns:
                   c = 11 + d * entries + 1.
  elastf_grad      u + g, u . n (product and d - 1 additions), sum_p (d - 1), sln * sun, + lnun, times a * inv_dd,
                   nn - full: 2 d + 4, taken as 2 d + 5: c = 2 (2 d + 5), + B for a batch sum.
  bc_lift, bc_grad k0 * v, the npe additions of the element row, times kappa: npe + 2; c = 2 (npe + 2) + k + 1, k = the
                   (element, node) pairs of the band row, + 1 for rhs - . / gbar - . (dots: times G instead).
  bc_grad_kappa    the element row against G (npe + 1), times lambda, npe additions, dk - .: c = 2 (2 npe + 3), + B for
                   the batch-shared kernel.
  bc_scatter, robin_sum_facets, robin_sum_blocks: copies, additions in a stated order, an integer: bitwise.

Every output buffer sits between two guards and holds, wherever the kernel must not write, alternately a NaN with a
recognisable payload and a random finite value (a `+=` leaves a NaN's payload alone; it cannot leave a finite value
alone); all of it is compared bit for bit afterwards.  lam and u hold NaN in padding samples (b >= B), g holds NaN
where the kernels have no business reading it, and every input datum is followed by NaN.  Every kernel runs twice on
the same inputs: the two results are bitwise equal.

Deliberately not asserted: the SIGN of the normal of a facet whose opposite node lies in the facet's own plane (a
convention for invalid input; its area and its normal up to the sign are asserted).  Padding samples: the kernels of
bc.hip take B and pad for themselves, and the gradient kernels loop over b < B, so none of their outputs has a padding
sample that is written -- asserted; padding samples of vals and rhs of the two assemble kernels are specified (the
coefficient the batch shares, or the unit coefficient where it comes per sample; an untouched right-hand side) and
asserted; nothing else about padding samples is specified, and nothing else is read."""
import numpy as np
import pytest
import torch

import _band_model as bm
from diffhe import FEMesh, _hip

T64 = torch.float64
DEV = "cuda:0"
EPS = 2.0 ** -53
LD = np.longdouble
PAYLOAD = np.uint64(0x7FF8DEAD0BADBEEF)
GUARD = 256
BADARG, BATCHPAD = -1, -4
DATA_LAYOUTS = ("null", "scalar", "sample", "facet", "bf", "fb")


# ---------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------
def poison(k):
    return np.full(k, PAYLOAD, dtype=np.uint64).view(np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def batch_pad(B):
    return (B + 63) // 64 * 64 if B >= 64 else 1 << (B - 1).bit_length()


def second_block(Bp):
    """One band row more than the first block holds: 4 waves of 64 / min(Bp, 64) rows."""
    return 4 * (64 // min(Bp, 64)) + 1


def dv(a, tail=False):
    """A host array on the device; tail: followed by NaN (an input datum read through strides)."""
    a = np.ascontiguousarray(a)
    if tail:
        return torch.from_numpy(np.concatenate([a.ravel(), np.full(GUARD, np.nan)])).to(DEV)[:a.size]
    return torch.from_numpy(a).to(DEV)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


class Out:
    """An output of `size` doubles between two guards.  `addr`: the flat positions the kernel is to write; prefill: the
    kernel adds to what is there (random values at addr).  Everything else alternates payload NaN / random finite."""

    def __init__(self, size, rng, addr, prefill):
        init = poison(size)
        init[1::2] = rng.standard_normal(len(init[1::2]))
        self.addr = np.asarray(addr, dtype=np.int64).ravel()
        assert len(np.unique(self.addr)) == len(self.addr) and (len(self.addr) == 0 or
                                                                (0 <= self.addr.min() and self.addr.max() < size))
        if prefill:
            init[self.addr] = rng.standard_normal(len(self.addr))
        self.size, self.init = size, np.concatenate([poison(GUARD), init, poison(GUARD)])
        self.dev = None

    def fresh(self):
        self.dev = torch.from_numpy(self.init.copy()).to(DEV)
        return self.dev[GUARD:GUARD + self.size]

    def before(self):
        return self.init[GUARD + self.addr]

    def after(self):
        return self.dev.cpu().numpy()

    def untouched(self, after, what):
        keep = np.ones(len(after), dtype=bool)
        keep[GUARD + self.addr] = False
        assert (bits(after)[keep] == bits(self.init)[keep]).all(), f"{what}: written outside the addressed entries"

    def close(self, after, ref, S, c, what):
        """Bitwise untouched outside addr; at addr within c * 2^-53 * S of ref (both shaped like addr)."""
        self.untouched(after, what)
        got = after[GUARD + self.addr]
        assert np.isfinite(got).all(), what
        excess = np.abs(got - np.asarray(ref, dtype=LD).ravel()) - c * EPS * np.asarray(S, dtype=LD).ravel()
        assert (excess <= 0).all(), f"{what}: {float(excess.max()):.3e} over c * 2^-53 * S, c = {c}"

    def same(self, after, ref, what):
        self.untouched(after, what)
        assert (bits(after[GUARD + self.addr]) == bits(np.asarray(ref, dtype=np.float64).ravel())).all(), what


def same_bits(a, b, what):
    assert (bits(a) == bits(b)).all(), f"{what}: two runs differ"


def lay(I, B, major, pad=0):
    """Strides (si, sb) and the size of an (I, B) array stored item-major (I, B + pad) or sample-major (B, I)."""
    return (B + pad, 1, I * (B + pad)) if major == "item" else (1, I, I * B)


def addr2(I, B, si, sb):
    return (np.arange(I)[:, None] * si + np.arange(B)[None, :] * sb)


def stored(full, si, sb, size):
    """The flat buffer that holds full (I, B) at i * si + b * sb, NaN elsewhere."""
    buf = np.full(size, np.nan)
    buf[addr2(full.shape[0], full.shape[1], si, sb)] = full
    return buf


def datum(rng, layout, nF, B, lo, hi):
    """A facet datum in one of the six layouts -> (full (nF, B) or None, device buffer or None, sf, sb)."""
    if layout == "null":
        return None, None, 0, 0
    shape, sf, sb = {"scalar": ((1, 1), 0, 0), "sample": ((1, B), 0, 1), "facet": ((nF, 1), 1, 0), "bf": ((nF, B), 1, nF),
                     "fb": ((nF, B), B, 1)}[layout]
    v = rng.uniform(lo, hi, shape)
    full = np.broadcast_to(v, (nF, B)).copy()
    buf = v.T.ravel() if layout == "bf" else v.ravel()
    return full, dv(buf, tail=True), sf, sb


def padded(full, sb, Bp, unit):
    """(nF, Bp) of a datum (nF, B): a padding sample reads the shared value, or `unit` where the datum comes per sample."""
    if full is None:
        return None
    nF, B = full.shape
    out = np.empty((nF, Bp))
    out[:, :B] = full
    out[:, B:] = unit if sb != 0 else full[:, :1]
    return out


def status(L, name, args):
    """The status an entry returns (the binding raises on a non-zero one, under the entry's name)."""
    try:
        getattr(L, name)(*args)
        return 0
    except _hip.HipExtensionError as err:
        assert name in str(err)
        for code in (BADARG, BATCHPAD):
            if L.diffhe_status_string(code).decode() in str(err):
                return code
        raise


# ---------------------------------------------------------------------------------------------------------------------
# synthetic bands
# ---------------------------------------------------------------------------------------------------------------------
def facets_over(rng, pool, nF, d, fixed=None):
    """(nF, d) facets (or elements) of distinct nodes drawn from `pool`; fixed (nF, k): nodes every one must hold (distinct
    in a row); the local order is shuffled."""
    k = 0 if fixed is None else fixed.shape[1]
    fac = rng.choice(pool, size=(nF, d))
    if k:
        fac[:, :k] = fixed
    for _ in range(500):
        s = np.sort(fac, 1)
        bad = (s[:, 1:] == s[:, :-1]).any(1)
        if not bad.any():
            return rng.permuted(fac, axis=1)
        fac[bad, k:] = rng.choice(pool, size=(int(bad.sum()), d - k))
    raise AssertionError("no distinct facets")


def cycle(nodes, count, *more):
    """(count, 1 + len(more)): row k holds nodes[k % len(nodes)], and more[j][k % len(more[j])]."""
    ar = np.arange(count)
    return np.stack([np.asarray(x)[ar % len(x)] for x in (nodes, *more)], 1)


def pattern(rng, fac, n):
    """A node pattern cols (W, n) that holds every coupling of the facets: slot 0 the node itself, the neighbours in a
    shuffled order, unused slots (one spare at least) point at the node itself."""
    nb = [[] for _ in range(n)]
    for nodes in fac.tolist():
        for i in nodes:
            for j in nodes:
                if i != j and j not in nb[i]:
                    nb[i].append(j)
    W = 2 + max(len(x) for x in nb)
    cols = np.tile(np.arange(n), (W, 1))
    for i, x in enumerate(nb):
        if x:
            cols[1:1 + len(x), i] = rng.permutation(x)
    return cols.astype(np.int32)


def only_rows(tab, keep):
    """A facet table without the rows whose node is not in `keep`: the kernels take any list of band rows."""
    take = np.isin(tab["rows"], keep)
    counts = np.diff(tab["row_ptr"])
    ent = np.repeat(take, counts)
    row_ptr = np.concatenate([[0], np.cumsum(counts[take])]).astype(np.int32)
    return {**tab, "rows": tab["rows"][take], "n_rows": int(take.sum()), "row_ptr": row_ptr, "ent_code": tab["ent_code"][ent],
            "ent_slot": tab["ent_slot"][ent]}


def facet_band(d, n_rows, seed, elastic):
    """A seeded facet band with exactly n_rows band rows R.  Robin: the rows are the free nodes, Dirichlet nodes sit on
    the facets too and three nodes on none.  Elastic: every node on a facet is a row of the table and fixed dofs come per
    dof; the d - 1 further nodes the facets need are taken out of the table again, so that nothing may be written there."""
    rng = np.random.default_rng([seed, d, n_rows, int(elastic)])
    nD = d - 1 if elastic else max(3, n_rows // 4)
    n = n_rows + nD + 3
    perm = rng.permutation(n)
    R, D = np.sort(perm[:n_rows]), perm[n_rows:n_rows + nD]
    nF = n_rows + 2
    fac = facets_over(rng, np.concatenate([R, D]), nF, d, fixed=cycle(R, nF))
    cols = pattern(rng, fac, n)
    x = dict(d=d, n=n, nF=nF, fac=fac, cols=cols, W=cols.shape[0], area=rng.uniform(0.5, 1.5, nF), rng=rng, R=R)
    if elastic:
        is_bc = rng.random(n * d) < 0.25
        nv = rng.standard_normal((d, nF))
        x.update(is_bc=is_bc, normal=nv / np.sqrt((nv * nv).sum(0)), tab=only_rows(bm.elastic_table(fac, cols), R),
                 g=np.where(is_bc, rng.standard_normal(n * d), np.nan))
    else:
        is_bc = np.zeros(n, dtype=bool)
        is_bc[D] = True
        x.update(is_bc=is_bc, tab=bm.robin_table(fac, is_bc, cols), g=np.where(is_bc, rng.standard_normal(n), np.nan))
    assert x["tab"]["n_rows"] == n_rows and np.array_equal(x["tab"]["rows"], R)
    x["dev"] = {k: dv(v) for k, v in x["tab"].items() if isinstance(v, np.ndarray)}
    x["dev"].update(area=dv(x["area"]), g=dv(x["g"]), is_bc=dv(is_bc.astype(np.uint8)))
    if elastic:
        x["dev"]["normal"] = dv(x["normal"])
    return x


def table_entries(tab):
    """(row node, F, p, c, slot) of every entry of a facet table."""
    row = np.repeat(tab["rows"], np.diff(tab["row_ptr"])).astype(np.int64)
    code = tab["ent_code"].astype(np.int64)
    return row, code >> 4, (code >> 2) & 3, code & 3, tab["ent_slot"].astype(np.int64)


def fields(rng, rows, B, Bp):
    """lam and u (rows, Bp) with NaN in the padding samples."""
    lam, u = rng.standard_normal((rows, Bp)), rng.standard_normal((rows, Bp))
    lam[:, B:] = np.nan
    u[:, B:] = np.nan
    return lam, u


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the model against the dense restatements
# ---------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


def _robin_dense_system(mesh, fac, kappa_e, h):
    """A (n, n) of test_robin.dense_solve, restated: K(kappa) + sum_F h_F M_F (no reaction term)."""
    import test_robin as tr
    n, el = mesh.n_nodes, mesh.elements
    npe, d = el.shape[1], fac.shape[1]
    k0, _ = tr.element_forms(mesh.nodes, el)
    rows = el[:, :, None].expand(-1, npe, npe).reshape(-1)
    cols = el[:, None, :].expand(-1, npe, npe).reshape(-1)
    A = torch.zeros(n * n, dtype=T64).index_add(0, rows * n + cols, (kappa_e[:, None, None] * k0).reshape(-1)).reshape(n, n)
    if h is None:                                                        # the load matrix instead
        m0 = tr.element_forms(mesh.nodes, el)[1]
        return torch.zeros(n * n, dtype=T64).index_add(0, rows * n + cols, m0.reshape(-1)).reshape(n, n)
    size = tr.facet_sizes(mesh.nodes, fac)
    MF = size[:, None, None] * (torch.ones(d, d, dtype=T64) + torch.eye(d, dtype=T64)) / (d * (d + 1))
    fr = fac[:, :, None].expand(-1, d, d).reshape(-1)
    fc = fac[:, None, :].expand(-1, d, d).reshape(-1)
    return A + torch.zeros(n * n, dtype=T64).index_add(0, fr * n + fc, (h[:, None, None] * MF).reshape(-1)).reshape(n, n)


@pytest.mark.parametrize("name", ["jittered2d", "box", "line"])
def test_robin_model_against_the_dense_restatement_and_autograd(name):
    import test_robin as tr
    mesh, reaction, _ = tr.case_mesh(name)
    assert reaction == 0.0
    fac = mesh.boundary_facets()
    B, n, nF, d = 2, mesh.n_nodes, len(fac), fac.shape[1]
    kappa, f, load, h, ui, q, w = tr.make_inputs(mesh, nF, B, "sample_elem", "both", seed=5)
    is_bc = np.zeros(n, dtype=bool)
    g = np.zeros(n)
    for k, v in mesh.dirichlet_nodes.items():
        is_bc[k], g[k] = True, v
    free = ~is_bc
    facT = fac.numpy().T
    area, _ = bm.facet_area(mesh.nodes.numpy().T, facT)
    assert _rel(area, tr.facet_sizes(mesh.nodes, fac).numpy()) <= 1e-14
    pairs, A, _, rhs, _ = bm.robin_system(facT, area, is_bc, g, h.numpy().T, ui.numpy().T, q.numpy().T, n, B)
    Am = bm.dense(pairs, A, n)
    zero = torch.zeros(nF, dtype=T64)
    lam, u0 = np.zeros((n, B)), np.zeros((n, B))
    auto = []
    for b in range(B):
        leaves = [t[b].clone().requires_grad_(True) for t in (h, ui, q)]
        u = tr.dense_solve(mesh, fac, kappa[b], f[b], load[b], *leaves)
        auto.append(torch.autograd.grad(tr.loss(u, w[b]), leaves))
        # the operator and the load the facet terms add, from the restated system
        Ab = _robin_dense_system(mesh, fac, kappa[b], h[b])
        dA = (Ab - _robin_dense_system(mesh, fac, kappa[b], zero)).numpy()
        size = tr.facet_sizes(mesh.nodes, fac)
        dF = torch.zeros(n, dtype=T64).index_add(0, fac.reshape(-1), (((h[b] * ui[b] + q[b]) * size / d)[:, None]
                                                                       .expand(-1, d)).reshape(-1)).numpy()
        assert _rel(np.asarray(Am[b], dtype=np.float64)[free][:, free], dA[free][:, free]) <= 1e-14
        assert not Am[b][is_bc].any() and not Am[b][:, is_bc].any()
        assert _rel(np.asarray(rhs[:, b], dtype=np.float64)[free], dF[free] - dA[free][:, is_bc] @ g[is_bc]) <= 1e-14
        assert not rhs[is_bc].any()
        # the restated system reproduces dense_solve, and gives the adjoint: A_ff lam_f = dL/du_f, lam = 0 on D
        ud = u.detach().numpy()
        gbar = 2.0 * ud + w[b].numpy()
        Aff = Ab.numpy()[free][:, free]
        Fb = (_robin_dense_system(mesh, fac, kappa[b], None) @ f[b] + load[b]).numpy() + dF
        assert _rel(np.linalg.solve(Aff, Fb[free] - Ab.numpy()[free][:, is_bc] @ g[is_bc]), ud[free]) <= 1e-12
        lam[free, b] = np.linalg.solve(Aff.T, gbar[free])
        u0[free, b] = ud[free]
    gr = bm.robin_grads(facT, area, lam, u0, g, h.numpy().T, ui.numpy().T)
    for k, key in enumerate(("dh", "du", "dq")):
        ref = np.stack([a[k].numpy() for a in auto], 1)                 # (nF, B)
        assert _rel(gr[key][0], ref) <= 1e-12, (name, key)


@pytest.mark.parametrize("case", ["2d", "3d"])
def test_elastic_facet_model_against_the_dense_restatement_and_autograd(case):
    import test_elastic_facets as te
    from test_elasticity import _box, _dense_K, _fixed_arrays, _rand, _rect
    mesh = _rect(3, 2, 4) if case == "2d" else _box(1, 1, 1, 5)
    d, B, n = mesh.dim, 2, mesh.n_nodes
    plane = "stress" if d == 2 else None
    fac = mesh.boundary_facets()
    nF = fac.shape[0]
    fixed = {(0, a): 0.0 for a in range(d)}
    fixed[(int(fac[1, 0]), 0)] = 0.03
    E, w, f = _rand((B, mesh.n_elements), 6, 0.5, 2.0), _rand((B, n, d), 7, -1, 1), _rand((B, n, d), 8, -1, 1)
    args = [_rand((B, nF, d), 9, -1, 1), _rand((B, nF), 10, -1, 1), _rand((B, nF), 11, 0.5, 2), _rand((B, nF), 12, 0.5, 2)]
    leaves = [a.clone().requires_grad_(True) for a in args]
    u = te._dense_solve(mesh, E, te.NU, plane, fixed, fac, *leaves, f=f)
    auto = torch.autograd.grad((w * u).sum(), leaves)
    # geometry
    opp = te._opposite(mesh, fac).numpy()
    facT = fac.numpy().T
    area, _, normal, _, out, S_out = bm.facet_normal(mesh.nodes.to(T64).numpy().T, facT, opp)
    a_ref, n_ref = te._facet_geo(mesh, fac)
    assert _rel(area, a_ref.numpy()) <= 1e-14 and _rel(normal, n_ref.numpy().T) <= 1e-14
    assert (np.abs(out) > 1e-6 * S_out).all()
    # operator and load
    bc, free, g = _fixed_arrays(mesh, fixed)
    is_bc = np.zeros(n * d, dtype=bool)
    is_bc[bc] = True
    t, p, kn, kt = (a.numpy() for a in args)
    pairs, A, _, rhs, _ = bm.elastic_system(facT, area, normal, is_bc, g.numpy(), t.transpose(1, 2, 0), p.T, kn.T, kt.T, n, B)
    Am = np.asarray(bm.dense(pairs, A, n * d), dtype=np.float64)
    Kf, Ff = te._facet_system(mesh, fac, *args)
    Kf, Ff = Kf.numpy(), Ff.numpy()
    for b in range(B):
        assert _rel(Am[b][free][:, free], Kf[b][free][:, free]) <= 1e-14
        assert not Am[b][is_bc].any() and not Am[b][:, is_bc].any()
        assert _rel(np.asarray(rhs[:, b], dtype=np.float64)[free], Ff[b][free] - Kf[b][free][:, bc] @ g.numpy()[bc]) <= 1e-14
    assert not rhs[is_bc].any()
    # gradients: K_ff lam_f = dL/du_f = w_f, lam = 0 on the fixed dofs; u without its fixed values, g beside it
    K = (_dense_K(mesh, E, te.NU, plane).numpy() + Kf)
    lam, u0 = np.zeros((n * d, B)), np.zeros((n * d, B))
    for b in range(B):
        lam[free, b] = np.linalg.solve(K[b][free][:, free].T, w[b].reshape(-1).numpy()[free])
        u0[free, b] = u[b].detach().reshape(-1).numpy()[free]
    gr = bm.elastic_grads(facT, area, normal, lam, u0, g.numpy())
    assert _rel(gr["dt"][0], auto[0].numpy().transpose(1, 2, 0)) <= 1e-12
    for key, a in zip(("dp", "dkn", "dkt"), auto[1:]):
        assert _rel(gr[key][0], a.numpy().T) <= 1e-12, key


def test_dirichlet_band_model_against_the_dense_restatement_and_autograd():
    import test_dirichlet_grad as tg
    mesh = tg._with_bc(tg._jittered(FEMesh.rectangle(4, 3), 0.2, 1), lambda x: 0.3 + x[0] * x[1])
    k0, m0, el, mass = tg._host_tables_2d(mesh)
    d_idx = mesh.dirichlet_index()
    gen = torch.Generator().manual_seed(0)
    B, m, n, nd = 2, mesh.n_elements, mesh.n_nodes, len(d_idx)
    kap = (1 + 0.5 * torch.rand(B, m, generator=gen, dtype=T64)).requires_grad_()
    f = torch.randn(B, n, generator=gen, dtype=T64)
    G = torch.randn(B, nd, generator=gen, dtype=T64, requires_grad=True)
    w = torch.randn(B, n, generator=gen, dtype=T64)
    u = tg._dense_solve(k0, m0, el, mass, d_idx, kap, f, G)
    dkap, dG = torch.autograd.grad((w * u).sum(), (kap, G))
    is_d = np.zeros(n, dtype=bool)
    is_d[d_idx.numpy()] = True
    free = ~is_d
    band = bm.dirichlet_band(el.numpy(), is_d)
    assert np.array_equal(band["d_idx"], d_idx.numpy())
    elems, k0m = el.numpy().T, k0.reshape(m, 9).numpy().T
    kv, Gv = kap.detach().numpy().T, G.detach().numpy().T
    idx = (el[:, :, None] * n + el[:, None, :]).reshape(-1)
    K = torch.zeros(B, n * n, dtype=T64).index_add(1, idx, (kap.detach()[:, :, None, None] * k0[None]).reshape(B, -1))
    K = K.reshape(B, n, n).numpy()
    lam = np.zeros((n, B))
    for b in range(B):
        lam[free, b] = np.linalg.solve(K[b][free][:, free].T, w[b].numpy()[free])
    # the lift
    lift, _ = bm.bc_lift(elems, k0m, kv, is_d, band["d_slot"], Gv, n)
    for b in range(B):
        assert _rel(np.asarray(lift[:, b], dtype=np.float64)[free], K[b][free][:, is_d] @ Gv[:, b]) <= 1e-14
    assert not lift[is_d].any()
    only = np.setdiff1d(np.nonzero(free)[0], band["rows"])
    assert not lift[only].any()                                       # rows outside the band: nothing to lift
    # dL/dG
    out, _, dots, _ = bm.bc_grad(elems, k0m, kv, is_d, band["d_idx"], band["d_slot"], lam, w.numpy().T, Gv)
    assert _rel(out, dG.numpy().T) <= 1e-12
    # dL/dkappa = -lam^T k0_e u_e: the part of the free nodes' u, restated here, and the G part, the model's
    uf = np.where(free[:, None], u.detach().numpy().T, 0.0)
    part_u = -np.einsum("peb,pqe,qeb->eb", lam[elems], k0.numpy().transpose(1, 2, 0), uf[elems])
    gpart, _ = bm.bc_grad_kappa(elems, k0m, is_d, band["d_slot"], lam, Gv)
    assert _rel(part_u - np.asarray(gpart, dtype=np.float64), dkap.numpy().T) <= 1e-12
    rest = np.setdiff1d(np.arange(m), band["band_elems"])
    assert not gpart[rest].any()
    # the lift term of a kappa per sample: sum_j G_j (K_1 lam)_j = sum_e lam^T k0_e G
    assert _rel(dots.sum(0), gpart.sum(0)) <= 1e-13


def _rounding_cases():
    """(name, c, evaluate(dt) -> [(value, S), ...]) on mid-size synthetic inputs."""
    rng = np.random.default_rng(77)
    d, n, nF, B, npe, m = 3, 40, 60, 5, 4, 50
    fac = facets_over(rng, np.arange(n), nF, d).T
    coords = rng.random((d, n))
    opp = (fac[0] + 1 + rng.integers(0, n - 3, nF)) % n
    is_bc = rng.random(n) < 0.3
    is_dof = rng.random(n * d) < 0.3
    area = rng.uniform(0.5, 1.5, nF)
    nv = rng.standard_normal((d, nF))
    nv /= np.sqrt((nv * nv).sum(0))
    r = lambda *s: rng.standard_normal(s)                                # noqa: E731
    h, ui, q, lam, u, g = r(nF, B), r(nF, B), r(nF, B), r(n, B), r(n, B), r(n)
    t, lam3, u3, g3 = r(nF, d, B), r(n * d, B), r(n * d, B), r(n * d)
    elems = facets_over(rng, np.arange(n), m, npe).T
    k0, kap = r(npe * npe, m), rng.uniform(0.5, 1.5, (m, B))
    d_idx = np.nonzero(is_bc)[0]
    d_slot = np.full(n, -1)
    d_slot[d_idx] = np.arange(len(d_idx))
    G = r(len(d_idx), B)
    pick = lambda x, *k: [(x[i], x[i + 1]) for i in k]                   # noqa: E731
    kf = d * int(np.bincount(fac.ravel()).max())        # entries of the fullest band row: d per facet on the node
    ke = int(np.bincount(elems.ravel()).max())          # (element, node) pairs of the fullest row
    return [
        ("facet_area", 14, lambda dt: pick(bm.facet_area(coords, fac, dt), 0)),
        ("facet_normal", 18, lambda dt: pick(bm.facet_normal(coords, fac, opp, dt), 2)),
        ("robin_system", 6 + kf, lambda dt: pick(bm.robin_system(fac, area, is_bc, g, h, ui, q, n, B, dt), 1, 3)),
        ("robin_grads", 2 * (d + 5), lambda dt: list(bm.robin_grads(fac, area, lam, u, g, h, ui, dt).values())),
        ("elastic_system", 9 + kf, lambda dt: pick(bm.elastic_system(fac, area, nv, is_dof, g3, t, h, ui, q, n, B, dt), 1, 3)),
        ("elastic_grads", 2 * (2 * d + 5), lambda dt: list(bm.elastic_grads(fac, area, nv, lam3, u3, g3, dt).values())),
        ("bc_lift", 2 * (npe + 2) + ke, lambda dt: pick(bm.bc_lift(elems, k0, kap, is_bc, d_slot, G, n, dt), 0)),
        ("bc_grad", 2 * (npe + 2) + ke, lambda dt: pick(bm.bc_grad(elems, k0, kap, is_bc, d_idx, d_slot, lam, u, G, dt), 0, 2)),
        ("bc_grad_kappa", 2 * (2 * npe + 3), lambda dt: pick(bm.bc_grad_kappa(elems, k0, is_bc, d_slot, lam, G, dt), 0)),
    ]


def test_the_models_rounding_is_far_below_the_tolerances():
    """The float64 evaluation of the model is within HALF the tolerance of the longdouble one (it owns half of every
    count); the longdouble evaluation the GPU tests use rounds 2^11 times finer: its share is below a thousandth."""
    worst = {}
    for name, c, run in _rounding_cases():
        for (v64, _), (vld, S) in zip(run(np.float64), run(LD)):
            assert vld.dtype == LD and v64.dtype == np.float64
            live = S > 0
            ratio = float((np.abs(v64 - vld)[live] / (0.5 * c * EPS * S[live])).max())
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert (np.abs(v64 - vld)[~live] == 0).all()
    print("float64 model against longdouble, as a fraction of half the tolerance:", worst)
    assert max(worst.values()) <= 1.0, worst
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_band_table_builders_on_a_hand_made_band():
    """Two triangles 0-1-2 and 1-2-3, node 3 Dirichlet, one edge (2, 3) and one edge (1, 2) as facets."""
    cols = np.array([[0, 1, 2, 3], [1, 0, 0, 1], [2, 2, 1, 2], [0, 3, 3, 3]])
    tab = bm.robin_table(np.array([[2, 3], [1, 2]]), np.array([0, 0, 0, 1], dtype=bool), cols)
    assert tab["rows"].tolist() == [1, 2] and tab["row_ptr"].tolist() == [0, 2, 6]
    assert tab["ent_code"].tolist() == [16 + 0, 16 + 1, 0, 1, 16 + 4, 16 + 5]
    assert tab["ent_slot"].tolist() == [0, 2, 0, -1, 2, 0]
    el = bm.elastic_table(np.array([[2, 3], [1, 2]]), cols)
    assert el["rows"].tolist() == [1, 2, 3] and -1 not in el["ent_slot"].tolist()
    assert bm.robin_table(np.array([[0, 3]]), np.zeros(4, dtype=bool), cols) is None          # 0 and 3 share no slot
    band = bm.dirichlet_band(np.array([[0, 1, 2], [1, 2, 3]]), np.array([0, 0, 0, 1], dtype=bool))
    assert band["d_idx"].tolist() == [3] and band["d_slot"].tolist() == [-1, -1, -1, 0]
    assert band["rows"].tolist() == [1, 2] and band["row_inc"].tolist() == [3, 4] and band["band_elems"].tolist() == [1]
    assert band["d_ptr"].tolist() == [0, 1] and band["d_inc"].tolist() == [5]
    part, out = bm.sum_facets(np.arange(260.0)[:, None] * np.ones((1, 2)))
    assert part.shape == (3, 2) and out.tolist() == [260 * 259 / 2] * 2 and bm.sum_blocks(0) == 0 and bm.sum_blocks(129) == 2


# ---------------------------------------------------------------------------------------------------------------------
# GPU: facet tables
# ---------------------------------------------------------------------------------------------------------------------
def table_inputs(d, nF, seed):
    """Random facets and opposite nodes into random coordinates; with nF >= 257, the named degenerate facets in front:
    a facet of one node twice, coincident nodes, a collinear triangle, one below and one above each threshold, and one
    facet whose opposite node is its own first node (in its plane)."""
    rng = np.random.default_rng([seed, d, nF])
    n = min(max(nF, 8) + 8, 4099)
    coords = rng.random((d, n))
    fac = facets_over(rng, np.arange(8, n), nF, d)
    opp = rng.integers(8, n, nF)
    while True:                                                         # the owner's opposite node: any node off the facet
        clash = (fac == opp[:, None]).any(1)
        if not clash.any():
            break
        opp[clash] = rng.integers(8, n, int(clash.sum()))
    special = 0
    if nF >= 257 and d == 2:
        coords[:, :4] = np.array([[0, 0], [0, 0], [0.5e-15, 0], [2e-15, 0]]).T
        fac[:5] = [[0, 0], [0, 1], [0, 2], [0, 3], [20, 21]]
        opp[4] = 20
        special = 5
    if nF >= 257 and d == 3:
        coords[:, :6] = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 0.5e-12, 0], [1, 2e-12, 0]]).T
        fac[:6] = [[0, 0, 2], [0, 1, 2], [0, 2, 3], [0, 2, 4], [0, 2, 5], [20, 21, 22]]
        opp[5] = 20
        special = 6
    return coords, fac.astype(np.int32), opp.astype(np.int32), n, special, rng


@pytest.mark.gpu
@pytest.mark.parametrize("nF", [1, 257, 262149])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_robin_facet_table(d, nF):
    L = _hip.lib()
    coords, fac, _, n, special, rng = table_inputs(d, nF, 1)
    ref, S = bm.facet_area(coords, fac.T)
    if special:
        assert not ref[:special - 2].any() and ref[special - 2] > 0     # degenerate ones, then the one above the threshold
    out = Out(nF, rng, np.arange(nF), False)
    runs = []
    for _ in range(2):
        L.diffhe_robin_facet_table(dv(coords), dv(fac.T), d, n, nF, out.fresh(), stream())
        runs.append(out.after())
    out.close(runs[0], ref, S, 14, "area")
    zero = np.nonzero(ref == 0)[0]
    assert (bits(runs[0][GUARD + zero]) == 0).all()                     # exact zeros; an end point's 1 is exact too
    if d == 1:
        out.same(runs[0], np.ones(nF), "area of end points")
    same_bits(*runs, "area")


@pytest.mark.gpu
@pytest.mark.parametrize("nF", [1, 257, 262149])
@pytest.mark.parametrize("d", [2, 3])
def test_elastf_facet_table(d, nF):
    L = _hip.lib()
    coords, fac, opp, n, special, rng = table_inputs(d, nF, 2)
    area, S_area, normal, S_normal, sgn, S_sgn = bm.facet_normal(coords, fac.T, opp)
    decided = np.abs(sgn) > 1e-6 * S_sgn                                # the opposite node is off the facet's plane
    if special:
        assert not area[:special - 2].any() and area[special - 2] > 0 and decided[special - 2]
        assert not decided[special - 1] and area[special - 1] > 0
    if nF >= 257:
        assert decided[area > 0].mean() > 0.99
        assert (sgn[decided] > 0).any() and (sgn[decided] < 0).any()    # owners on both sides
    oa, on = Out(nF, rng, np.arange(nF), False), Out(d * nF, rng, np.arange(d * nF), False)
    runs = []
    for _ in range(2):
        L.diffhe_elastf_facet_table(dv(coords), dv(fac.T), dv(opp), d, n, nF, oa.fresh(), on.fresh(), stream())
        runs.append((oa.after(), on.after()))
    oa.close(runs[0][0], area, S_area, 14, "area")
    on.untouched(runs[0][1], "normal")
    got = runs[0][1][GUARD:GUARD + d * nF].reshape(d, nF)
    assert np.isfinite(got).all()
    dead = area == 0
    assert (bits(got[:, dead]) == 0).all() and (bits(runs[0][0][GUARD:GUARD + nF][dead]) == 0).all()
    # off-plane owners: the signed normal; in-plane ones: up to the sign
    err = np.where(decided[None, :], np.abs(got - normal), np.minimum(np.abs(got - normal), np.abs(got + normal)))
    excess = err - 18 * EPS * S_normal
    assert (excess <= 0).all(), f"normal: {float(excess.max()):.3e} over 18 * 2^-53 * S"
    same_bits(runs[0][0], runs[1][0], "area")
    same_bits(runs[0][1], runs[1][1], "normal")


# ---------------------------------------------------------------------------------------------------------------------
# GPU: diffhe_robin_assemble
# ---------------------------------------------------------------------------------------------------------------------
NODE_SHAPES = [(rows, max(1, Bp - 1), Bp) for Bp in (1, 4, 64, 128) for rows in (1, second_block(Bp))]
_BANDS = {}


def band_of(d, n_rows, elastic):
    key = (d, n_rows, elastic)
    if key not in _BANDS:
        _BANDS[key] = facet_band(d, n_rows, 3, elastic)
    return _BANDS[key]


def vals_targets(x, blocks):
    """The (slot, row, column) triples of `vals` the table addresses, once each: Robin per node (blocks = 1), elastic per
    dof (blocks = d: node slot k, row dof (i, a), column dof (j, q) -> dof slot of include/diffhe_elastic.h)."""
    row, F, _, c, slot = table_entries(x["tab"])
    keep = slot >= 0
    row, col, slot = row[keep], x["fac"][F[keep], c[keep]].astype(np.int64), slot[keep]
    assert (x["cols"][slot, row] == col).all()
    trip = np.unique(np.stack([slot, row, col], 1), axis=0)
    if blocks == 1:
        return trip
    d = blocks
    out = [(bm.dof_slot(k, a, q, d), i * d + a, j * d + q) for k, i, j in trip.tolist() for a in range(d) for q in range(d)
           if not x["is_bc"][i * d + a] and not x["is_bc"][j * d + q]]
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def robin_assemble_case(x, B, Bp, Bv, layouts, seed=0):
    L = _hip.lib()
    d, n, nF, tab, D = x["d"], x["n"], x["nF"], x["tab"], x["dev"]
    rng = np.random.default_rng([seed, B, Bp, Bv])
    if Bv == 1 and Bp > 1:
        assert layouts[0] in ("null", "scalar", "facet")
    (h, hd, hsf, hsb), (ui, ud, usf, usb), (q, qd, qsf, qsb) = (datum(rng, lay_, nF, B, lo, hi) for lay_, lo, hi in
                                                                zip(layouts, (0.5, -1, -1), (1.5, 1, 1)))
    hP = padded(h, hsb, Bp, 1.0) if h is not None else np.zeros((nF, 1))
    pairs, A, SA, rhs, Srhs = bm.robin_system(x["fac"].T, x["area"], x["is_bc"], x["g"], hP, padded(ui, usb, Bp, 0.0),
                                              padded(q, qsb, Bp, 0.0), n, Bp)
    trip = vals_targets(x, 1)
    at = bm.pair_index(pairs, n, trip[:, 1], trip[:, 2])
    assert (at >= 0).all() and len(np.unique(at)) == len(pairs)
    vals = Out(x["W"] * n * Bv, rng, ((trip[:, 0] * n + trip[:, 1]) * Bv)[:, None] + np.arange(Bv), True)
    rows = tab["rows"].astype(np.int64)
    out_rhs = Out(n * Bp, rng, (rows * Bp)[:, None] + np.arange(B), True)
    k = int(np.diff(tab["row_ptr"]).max()) + 1
    runs = []
    for _ in range(2):
        L.diffhe_robin_assemble(D["fac"], d, nF, D["area"], D["rows"], D["row_ptr"], D["ent_code"], D["ent_slot"],
                                tab["n_rows"], D["g"], hd, hsf, hsb, ud, usf, usb, qd, qsf, qsb, vals.fresh(), out_rhs.fresh(),
                                n, Bv, B, Bp, stream())
        runs.append((vals.after(), out_rhs.after()))
    v0 = vals.before().reshape(-1, Bv)
    vals.close(runs[0][0], v0 + A[at][:, :Bv], np.abs(v0) + SA[at][:, :Bv], 6 + k, "vals (padding samples included)")
    r0 = out_rhs.before().reshape(-1, B)
    # padding samples of rhs on the band rows are not addressed: they come back bit-identical
    out_rhs.close(runs[0][1], r0 + rhs[rows][:, :B], np.abs(r0) + Srhs[rows][:, :B], 10 + k, "rhs")
    same_bits(runs[0][0], runs[1][0], "vals")
    same_bits(runs[0][1], runs[1][1], "rhs")


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True], ids=["Bv=Bp", "Bv=1"])
@pytest.mark.parametrize("d,rows,B,Bp", [(d, *s) for d in (1, 2, 3) for s in NODE_SHAPES] + [(2, 8200, 63, 64)], ids=str)
def test_robin_assemble_shapes(d, rows, B, Bp, shared):
    layouts = ("facet", "fb", "bf") if shared else ("fb", "sample", "bf")
    robin_assemble_case(band_of(d, rows, False), B, Bp, 1 if shared else Bp, layouts)


def rotations(layouts, k):
    return [tuple(layouts[(i + j) % len(layouts)] for j in range(k)) for i in range(len(layouts))]


@pytest.mark.gpu
@pytest.mark.parametrize("B,Bp", [(3, 4), (70, 128)], ids=["B3", "B70"])
@pytest.mark.parametrize("layouts", rotations(DATA_LAYOUTS, 3), ids="-".join)
def test_robin_assemble_layouts(layouts, B, Bp):
    robin_assemble_case(band_of(2, 5, False), B, Bp, Bp, layouts, seed=1)
    if layouts[0] in ("null", "scalar", "facet"):
        robin_assemble_case(band_of(3, 5, False), B, Bp, 1, layouts, seed=2)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: diffhe_robin_grad, diffhe_robin_sum_facets, diffhe_robin_sum_blocks
# ---------------------------------------------------------------------------------------------------------------------
GRAD_LAYOUTS = ("bf", "fb", "sum", "null")
GROUP_SHAPES = [(items, B) for items in (1, 5) for B in (1, 3, 64, 70, 130)]
GROUP_PAST_THE_CAP = (32772, 70)          # 8192 blocks of four items at 64 lanes per item, and four items more


def grad_out(rng, layout, nF, B):
    """A scalar gradient output per facet and sample in both orders, summed over the batch, or absent
    -> (Out or None, sf, sb)."""
    if layout == "null":
        return None, 0, 0
    sf, sb, size = {"bf": (1, nF, nF * B), "fb": (B, 1, nF * B), "sum": (1, 0, nF)}[layout]
    return Out(size, rng, addr2(nF, B if sb else 1, sf, sb), False), sf, sb


def check_grad(out, after, sb, ref, S, c, B, what):
    if sb:
        out.close(after, ref, S, c, what)
    else:
        out.close(after, ref.astype(LD).sum(1), S.astype(LD).sum(1), c + B, what + " summed over the batch")


def facet_inputs(d, nF, B, seed, comps):
    rng = np.random.default_rng([seed, d, nF, B])
    n = min(max(d + 2, nF // 2), 4099)
    Bp = batch_pad(B)
    lam, u = fields(rng, n * comps, B, Bp)
    fac = facets_over(rng, np.arange(n), nF, d)
    return dict(rng=rng, n=n, Bp=Bp, fac=fac, area=rng.uniform(0.5, 1.5, nF), lam=lam, u=u, g=rng.standard_normal(n * comps))


def robin_grad_case(d, nF, B, data_layouts, out_layouts, with_g=True, seed=0):
    L = _hip.lib()
    x = facet_inputs(d, nF, B, seed, 1)
    rng, Bp = x["rng"], x["Bp"]
    (h, hd, hsf, hsb), (ui, ud, usf, usb) = (datum(rng, lay_, nF, B, -1, 1) for lay_ in data_layouts)
    ref = bm.robin_grads(x["fac"].T, x["area"], x["lam"][:, :B], x["u"][:, :B], x["g"] if with_g else None, h, ui)
    outs = [grad_out(rng, lay_, nF, B) for lay_ in out_layouts]
    D = [dv(x["fac"].T.astype(np.int32)), dv(x["area"]), dv(x["lam"]), dv(x["u"]), dv(x["g"]) if with_g else None]
    runs = []
    for _ in range(2):
        args = [a for o, sf, sb in outs for a in (o.fresh() if o else None, sf, sb)]
        L.diffhe_robin_grad(D[0], d, nF, D[1], D[2], D[3], D[4], B, Bp, hd, hsf, hsb, ud, usf, usb, *args, stream())
        runs.append([o.after() if o else None for o, _, _ in outs])
    for k, key in enumerate(("dh", "du", "dq")):
        o, _, sb = outs[k]
        if o is not None:
            check_grad(o, runs[0][k], sb, *ref[key], 2 * (d + 5), B, key)
            same_bits(runs[0][k], runs[1][k], key)


@pytest.mark.gpu
@pytest.mark.parametrize("d,nF,B", [(d, *s) for d in (1, 2, 3) for s in GROUP_SHAPES] + [(2, *GROUP_PAST_THE_CAP)], ids=str)
def test_robin_grad_shapes(d, nF, B):
    if (nF, B) == GROUP_PAST_THE_CAP:                                      # one call: the model of this size takes a second
        return robin_grad_case(d, nF, B, ("fb", "sample"), ("fb", "sum", "bf"))
    robin_grad_case(d, nF, B, ("fb", "bf"), ("fb", "bf", "fb"))
    robin_grad_case(d, nF, B, ("facet", "sample"), ("sum", "sum", "sum"), seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 70], ids=["B3", "B70"])
@pytest.mark.parametrize("layouts", rotations(DATA_LAYOUTS, 2), ids="-".join)
def test_robin_grad_layouts(layouts, B):
    k = DATA_LAYOUTS.index(layouts[0])
    robin_grad_case(2, 5, B, layouts, tuple(GRAD_LAYOUTS[(k + j) % 4] for j in range(3)), with_g=k % 2 == 0, seed=2)
    only = [["null"] * 3 for _ in range(3)]
    for j in range(3):                                                    # one output alone
        only[j][j] = GRAD_LAYOUTS[(k + j) % 3]
        robin_grad_case(3, 5, B, layouts, tuple(only[j]), seed=3 + j)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("nF", [1, 128, 129, 16385])
def test_robin_sum_facets_is_the_ordered_sum(nF, B):
    L = _hip.lib()
    rng = np.random.default_rng([nF, B])
    src = rng.standard_normal((nF, B)) * 10.0 ** rng.integers(-3, 4, (nF, 1))
    nblk = L.diffhe_robin_sum_blocks(nF)
    assert nblk == bm.sum_blocks(nF) == (nF + 127) // 128
    ref_part, ref_out = bm.sum_facets(src)
    part, out = Out(nblk * B, rng, np.arange(nblk * B), False), Out(B, rng, np.arange(B), False)
    runs = []
    for _ in range(2):
        L.diffhe_robin_sum_facets(dv(src), nF, B, part.fresh(), out.fresh(), stream())
        runs.append((part.after(), out.after()))
    part.same(runs[0][0], ref_part, "chunk sums")
    out.same(runs[0][1], ref_out, "totals")
    same_bits(runs[0][0], runs[1][0], "chunk sums")
    same_bits(runs[0][1], runs[1][1], "totals")


@pytest.mark.gpu
def test_robin_sum_blocks():
    L = _hip.lib()
    for nF in (-3, 0, 1, 127, 128, 129, 16385, 2 ** 27 - 1):
        assert L.diffhe_robin_sum_blocks(nF) == bm.sum_blocks(nF)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: diffhe_elastf_assemble, diffhe_elastf_grad
# ---------------------------------------------------------------------------------------------------------------------
T_LAYOUTS = ("null", "const", "bfd", "fdb")


def traction(rng, layout, nF, d, B):
    """-> (full (nF, d, B) or None, device buffer, tsf, tsc, tsb): one vector, (B, nF, d) or (nF, d, B)."""
    if layout == "null":
        return None, None, 0, 0, 0
    if layout == "const":
        v = rng.uniform(-1, 1, d)
        return np.broadcast_to(v[None, :, None], (nF, d, B)).copy(), dv(v, tail=True), 0, 1, 0
    full = rng.uniform(-1, 1, (nF, d, B))
    if layout == "bfd":
        return full, dv(full.transpose(2, 0, 1), tail=True), d, 1, nF * d
    return full, dv(full, tail=True), d * B, B, 1


def elastf_assemble_case(x, B, Bp, Bv, t_layout, layouts, seed=0):
    L = _hip.lib()
    d, n, nF, tab, D = x["d"], x["n"], x["nF"], x["tab"], x["dev"]
    rng = np.random.default_rng([seed, B, Bp, Bv])
    if Bv == 1 and Bp > 1:
        assert all(s in ("null", "scalar", "facet") for s in layouts[1:])
    t, td, tsf, tsc, tsb = traction(rng, t_layout, nF, d, B)
    (p, pd, psf, psb), (kn, nd_, nsf, nsb), (kt, kd, ksf, ksb) = (datum(rng, lay_, nF, B, lo, 1.5) for lay_, lo in
                                                                  zip(layouts, (-1.5, 0.5, 0.5)))
    stiff = kn is not None or kt is not None
    unit = nsb != 0 or ksb != 0                   # a stiffness per sample: padding samples take kn = kt = 1, absent or not
    knP, ktP = padded(kn, nsb, Bp, 1.0), padded(kt, ksb, Bp, 1.0)
    if stiff and unit:
        knP = knP if knP is not None else np.zeros((nF, Bp))
        ktP = ktP if ktP is not None else np.zeros((nF, Bp))
        knP[:, B:], ktP[:, B:] = 1.0, 1.0
    if stiff and knP is None:
        knP = np.zeros((nF, 1))
    tP = None if t is None else np.concatenate([t, np.zeros((nF, d, Bp - B))], 2)
    g = np.where(x["is_bc"], x["g"], 0.0)
    pairs, A, SA, rhs, Srhs = bm.elastic_system(x["fac"].T, x["area"], x["normal"], x["is_bc"], g, tP, padded(p, psb, Bp, 0.0),
                                                knP, ktP, n, Bp)
    own = np.isin(pairs[:, 0] // d, x["R"])                               # the table holds the rows R only
    pairs, A, SA = pairs[own], A[own], SA[own]
    nd = n * d
    trip = vals_targets(x, d) if stiff else np.zeros((0, 3), dtype=np.int64)
    at = bm.pair_index(pairs, nd, trip[:, 1], trip[:, 2])
    assert (at >= 0).all() and len(np.unique(at)) == len(pairs)
    vals = Out(d * x["W"] * nd * Bv, rng, ((trip[:, 0] * nd + trip[:, 1]) * Bv)[:, None] + np.arange(Bv), True)
    dofs = (tab["rows"].astype(np.int64)[:, None] * d + np.arange(d)).ravel()
    dofs = dofs[~x["is_bc"][dofs]]                                        # fixed rows are skipped
    out_rhs = Out(nd * Bp, rng, (dofs * Bp)[:, None] + np.arange(B), True)
    entries = int(np.diff(tab["row_ptr"]).max())
    runs = []
    for _ in range(2):
        L.diffhe_elastf_assemble(D["fac"], d, nF, D["area"], D["normal"], D["rows"], D["row_ptr"], D["ent_code"],
                                 D["ent_slot"], tab["n_rows"], D["is_bc"], D["g"], td, tsf, tsc, tsb, pd, psf, psb, nd_, nsf,
                                 nsb, kd, ksf, ksb, vals.fresh(), out_rhs.fresh(), n, Bv, B, Bp, stream())
        runs.append((vals.after(), out_rhs.after()))
    v0 = vals.before().reshape(-1, Bv)
    vals.close(runs[0][0], v0 + A[at][:, :Bv], np.abs(v0) + SA[at][:, :Bv], 9 + entries + 1, "vals (padding samples included)")
    r0 = out_rhs.before().reshape(-1, B)
    out_rhs.close(runs[0][1], r0 + rhs[dofs][:, :B], np.abs(r0) + Srhs[dofs][:, :B], 11 + d * entries + 1, "rhs")
    same_bits(runs[0][0], runs[1][0], "vals")
    same_bits(runs[0][1], runs[1][1], "rhs")


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True], ids=["Bv=Bp", "Bv=1"])
@pytest.mark.parametrize("d,rows,B,Bp", [(d, *s) for d in (2, 3) for s in NODE_SHAPES] + [(2, 8200, 63, 64)], ids=str)
def test_elastf_assemble_shapes(d, rows, B, Bp, shared):
    layouts = ("fb", "facet", "scalar") if shared else ("fb", "bf", "sample")
    elastf_assemble_case(band_of(d, rows, True), B, Bp, 1 if shared else Bp, "bfd" if shared else "fdb", layouts)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Bp", [(3, 4), (70, 128)], ids=["B3", "B70"])
@pytest.mark.parametrize("layouts", rotations(DATA_LAYOUTS, 3), ids="-".join)
def test_elastf_assemble_layouts(layouts, B, Bp):
    k = DATA_LAYOUTS.index(layouts[0])
    elastf_assemble_case(band_of(2 + k % 2, 5, True), B, Bp, Bp, T_LAYOUTS[k % 4], layouts, seed=1)
    if all(s in ("null", "scalar", "facet") for s in layouts[1:]):
        elastf_assemble_case(band_of(3 - k % 2, 5, True), B, Bp, 1, T_LAYOUTS[(k + 1) % 4], layouts, seed=2)


def elastf_grad_case(d, nF, B, t_layout, out_layouts, with_g=True, seed=0):
    L = _hip.lib()
    x = facet_inputs(d, nF, B, seed, d)
    rng, Bp = x["rng"], x["Bp"]
    nv = rng.standard_normal((d, nF))
    nv /= np.sqrt((nv * nv).sum(0))
    ref = bm.elastic_grads(x["fac"].T, x["area"], nv, x["lam"][:, :B], x["u"][:, :B], x["g"] if with_g else None)
    # dL/dt: (B, nF, d), (nF, d, B), summed over the batch (nF, d), or absent
    tf, tc, tb, tsize = {"bfd": (d, 1, nF * d, nF * d * B), "fdb": (d * B, B, 1, nF * d * B), "sum": (d, 1, 0, nF * d),
                         "null": (0, 0, 0, 0)}[t_layout]
    Bt = B if tb else 1
    t_addr = np.arange(nF)[:, None, None] * tf + np.arange(d)[None, :, None] * tc + np.arange(Bt)[None, None, :] * tb
    dt_out = Out(tsize, rng, t_addr, False) if t_layout != "null" else None
    outs = [grad_out(rng, lay_, nF, B) for lay_ in out_layouts]
    D = [dv(x["fac"].T.astype(np.int32)), dv(x["area"]), dv(nv), dv(x["lam"]), dv(x["u"]), dv(x["g"]) if with_g else None]
    runs = []
    for _ in range(2):
        args = [a for o, sf, sb in outs for a in (o.fresh() if o else None, sf, sb)]
        L.diffhe_elastf_grad(D[0], d, nF, D[1], D[2], D[3], D[4], D[5], B, Bp, dt_out.fresh() if dt_out else None, tf, tc, tb,
                             *args, stream())
        runs.append([dt_out.after() if dt_out else None] + [o.after() if o else None for o, _, _ in outs])
    c = 2 * (2 * d + 5)
    if dt_out is not None:
        v, S = ref["dt"]
        if tb:
            dt_out.close(runs[0][0], v, S, c, "dt")
        else:
            dt_out.close(runs[0][0], v.sum(2, keepdims=True), S.sum(2, keepdims=True), c + B, "dt summed over the batch")
        same_bits(runs[0][0], runs[1][0], "dt")
    for k, key in enumerate(("dp", "dkn", "dkt")):
        o, _, sb = outs[k]
        if o is not None:
            check_grad(o, runs[0][k + 1], sb, *ref[key], c, B, key)
            same_bits(runs[0][k + 1], runs[1][k + 1], key)


@pytest.mark.gpu
@pytest.mark.parametrize("d,nF,B", [(d, *s) for d in (2, 3) for s in GROUP_SHAPES] + [(2, *GROUP_PAST_THE_CAP)], ids=str)
def test_elastf_grad_shapes(d, nF, B):
    if (nF, B) == GROUP_PAST_THE_CAP:                                      # one call: the model of this size takes seconds
        return elastf_grad_case(d, nF, B, "sum", ("fb", "sum", "bf"))
    elastf_grad_case(d, nF, B, "fdb", ("fb", "bf", "fb"))
    elastf_grad_case(d, nF, B, "sum", ("sum", "sum", "sum"), seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 70], ids=["B3", "B70"])
@pytest.mark.parametrize("k", range(4))
def test_elastf_grad_layouts(k, B):
    tl = ("bfd", "fdb", "sum", "null")
    elastf_grad_case(2 + k % 2, 5, B, tl[k], tuple(GRAD_LAYOUTS[(k + 1 + j) % 4] for j in range(3)), with_g=k % 2 == 0, seed=2)
    only = ["null"] * 4
    only[k] = ("bfd", "bf", "sum", "fb")[k]                                # one output alone: dt, dp, dkn, dkt in turn
    elastf_grad_case(3 - k % 2, 5, B, only[0], tuple(only[1:]), seed=3)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernels of bc.hip
# ---------------------------------------------------------------------------------------------------------------------
KAPPA_LAYOUTS = ("null", "scalar", "sample", "elem", "eb", "be")
_BC = {}


def bc_band(npe, nR, nD, nb, cover, seed=0, all_d=True):
    """Elements (m, npe) around a Dirichlet set D of nD nodes: nb band elements with one Dirichlet node each at least
    (cover: element k holds the free node R[k % nR] and the Dirichlet node D[k % nD], so that the band has exactly nR rows,
    and forty more elements hold R[0]: a band row in many elements), one element of Dirichlet nodes only (all_d, when D
    has npe nodes), seven interior elements that touch no Dirichlet node; in a shuffled order."""
    key = (npe, nR, nD, nb, cover, seed, all_d)
    if key in _BC:
        return _BC[key]
    rng = np.random.default_rng([seed, npe, nR, nD, nb])
    n = nR + nD + npe + 3
    perm = rng.permutation(n)
    R, D, inner = perm[:nR], perm[nR:nR + nD], perm[nR + nD:]
    pool = np.concatenate([R, D])
    assert len(pool) >= npe and (not cover or nb >= max(nR, nD))
    if cover:
        parts = [facets_over(rng, pool, nb, npe, fixed=cycle(D, nb, R)),
                 facets_over(rng, pool, 40, npe, fixed=cycle(D, 40, R[:1]))]
    else:
        parts = [facets_over(rng, pool, nb, npe, fixed=rng.choice(D, size=(nb, 1)))]
    if all_d and nD >= npe:
        parts.append(rng.permutation(D)[None, :npe])
    parts.append(facets_over(rng, inner if cover else np.concatenate([R, inner]), 7, npe))
    el = rng.permutation(np.concatenate(parts))
    is_d = np.zeros(n, dtype=bool)
    is_d[D] = True
    band = bm.dirichlet_band(el, is_d)
    assert band["n_d"] == nD and (not cover or band["n_rows"] == nR)
    x = dict(npe=npe, n=n, m=len(el), elems=el.T.astype(np.int32).copy(), is_d=is_d, band=band,
             k0=rng.standard_normal((npe * npe, len(el))))
    x["dev"] = {k: dv(v) for k, v in band.items() if isinstance(v, np.ndarray)}
    x["dev"].update(elems=dv(x["elems"]), k0=dv(x["k0"]))
    _BC[key] = x
    return x


def kappa_datum(rng, layout, m, B):
    """-> (full (m, B) or None, device buffer, kse, ksb)."""
    if layout == "null":
        return None, None, 0, 0
    shape, kse, ksb = {"scalar": ((1, 1), 0, 0), "sample": ((1, B), 0, 1), "elem": ((m, 1), 1, 0), "eb": ((m, B), B, 1),
                       "be": ((m, B), 1, m)}[layout]
    v = rng.uniform(0.5, 1.5, shape)
    return np.broadcast_to(v, (m, B)).copy(), dv(v.T.ravel() if layout == "be" else v.ravel(), tail=True), kse, ksb


def placed(rng, full, major, pad=0):
    """An input (I, B) in one of the two orders -> (device buffer, si, sb)."""
    si, sb, size = lay(full.shape[0], full.shape[1], major, pad)
    return dv(stored(full, si, sb, size), tail=True), si, sb


def bc_lift_case(x, B, kl, gm, rm, seed=0):
    L = _hip.lib()
    npe, n, m, band, D = x["npe"], x["n"], x["m"], x["band"], x["dev"]
    rng = np.random.default_rng([seed, B, npe])
    kap, kd, kse, ksb = kappa_datum(rng, kl, m, B)
    G = rng.standard_normal((band["n_d"], B))
    Gd, gsj, gsb = placed(rng, G, gm)
    acc, S = bm.bc_lift(x["elems"], x["k0"], kap, x["is_d"], band["d_slot"], G, n)
    pad = batch_pad(B) - B                                                 # node-major rows as wide as the solver's
    rsn, rsb, size = lay(n, B, rm, pad)
    rows = band["rows"].astype(np.int64)
    out = Out(size, rng, rows[:, None] * rsn + np.arange(B) * rsb, True)
    runs = []
    for _ in range(2):
        L.diffhe_bc_lift(D["elems"], npe, m, D["k0"], kd, kse, ksb, D["d_slot"], Gd, gsj, gsb, D["rows"], D["row_ptr"],
                         D["row_inc"], band["n_rows"], out.fresh(), rsn, rsb, B, stream())
        runs.append(out.after())
    r0 = out.before().reshape(-1, B)
    k = int(np.diff(band["row_ptr"]).max())
    out.close(runs[0], r0 - acc[rows], np.abs(r0) + S[rows], 2 * (npe + 2) + k + 1, "rhs")
    same_bits(*runs, "rhs")


def bc_grad_case(x, B, kl, majors, with_gbar, with_dots, seed=0):
    L = _hip.lib()
    npe, n, m, band, D = x["npe"], x["n"], x["m"], x["band"], x["dev"]
    nD = band["n_d"]
    rng = np.random.default_rng([seed, B, npe, 1])
    kap, kd, kse, ksb = kappa_datum(rng, kl, m, B)
    lam = np.where(x["is_d"][:, None], np.nan, rng.standard_normal((n, B)))     # never read on a Dirichlet node
    gbar, G = rng.standard_normal((n, B)), rng.standard_normal((nD, B))
    ld, lsn, lsb = placed(rng, lam, majors[0])
    gd, gsn, gsb = placed(rng, gbar, majors[1]) if with_gbar else (None, 0, 0)
    Gd, Gsj, Gsb = placed(rng, G, majors[2]) if with_dots else (None, 0, 0)
    ref, S, dref, dS = bm.bc_grad(x["elems"], x["k0"], kap, x["is_d"], band["d_idx"], band["d_slot"], np.nan_to_num(lam),
                                  gbar if with_gbar else None, G if with_dots else None)
    osj, osb, size = lay(nD, B, majors[3], 1)
    out = Out(size, rng, addr2(nD, B, osj, osb), False)
    dots = Out(nD * B, rng, np.arange(nD * B), False) if with_dots else None
    runs = []
    for _ in range(2):
        L.diffhe_bc_grad(D["elems"], npe, m, D["k0"], kd, kse, ksb, D["d_slot"], D["d_idx"], D["d_ptr"], D["d_inc"], nD, ld,
                         lsn, lsb, gd, gsn, gsb, out.fresh(), osj, osb, Gd, Gsj, Gsb, dots.fresh() if dots else None, B,
                         stream())
        runs.append((out.after(), dots.after() if dots else None))
    c = 2 * (npe + 2) + int(np.diff(band["d_ptr"]).max()) + 1
    out.close(runs[0][0], ref, S, c, "dL/dG")
    same_bits(runs[0][0], runs[1][0], "dL/dG")
    if dots:
        dots.close(runs[0][1], dref, dS, c, "dots")
        same_bits(runs[0][1], runs[1][1], "dots")


def bc_scatter_case(x, B, gm, um, seed=0):
    L = _hip.lib()
    band, D, n = x["band"], x["dev"], x["n"]
    nD = band["n_d"]
    rng = np.random.default_rng([seed, B, 2])
    G = rng.standard_normal((nD, B))
    Gd, gsj, gsb = placed(rng, G, gm)
    usn, usb, size = lay(n, B, um, batch_pad(B) - B)
    u = Out(size, rng, band["d_idx"].astype(np.int64)[:, None] * usn + np.arange(B) * usb, False)
    runs = []
    for _ in range(2):
        L.diffhe_bc_scatter(D["d_idx"], nD, Gd, gsj, gsb, u.fresh(), usn, usb, B, stream())
        runs.append(u.after())
    u.same(runs[0], G, "u on the Dirichlet rows")
    same_bits(*runs, "u")


def bc_grad_kappa_case(x, B, shared, majors, seed=0):
    L = _hip.lib()
    npe, n, m, band, D = x["npe"], x["n"], x["m"], x["band"], x["dev"]
    rng = np.random.default_rng([seed, B, npe, 3])
    lam = np.where(x["is_d"][:, None], np.nan, rng.standard_normal((n, B)))
    G = rng.standard_normal((band["n_d"], B))
    ld, lsn, lsb = placed(rng, lam, majors[0])
    Gd, gsj, gsb = placed(rng, G, majors[1])
    ref, S = bm.bc_grad_kappa(x["elems"], x["k0"], x["is_d"], band["d_slot"], np.nan_to_num(lam), G)
    be = band["band_elems"].astype(np.int64)
    if shared:
        dse, dsb, size = 2, 0, 2 * m                                       # a strided dk (e): every other double
        dk = Out(size, rng, be * dse, True)
    else:
        dse, dsb, size = lay(m, B, majors[2], 1)
        dk = Out(size, rng, be[:, None] * dse + np.arange(B) * dsb, True)
    runs = []
    for _ in range(2):
        L.diffhe_bc_grad_kappa(D["elems"], npe, m, D["k0"], D["d_slot"], D["band_elems"], band["n_be"], ld, lsn, lsb, Gd, gsj,
                               gsb, dk.fresh(), dse, dsb, int(shared), B, stream())
        runs.append(dk.after())
    c = 2 * (2 * npe + 3)
    if shared:
        d0 = dk.before()
        dk.close(runs[0], d0 - ref[be].sum(1), np.abs(d0) + S[be].sum(1), c + B, "dk summed over the batch")
    else:
        d0 = dk.before().reshape(-1, B)
        dk.close(runs[0], d0 - ref[be], np.abs(d0) + S[be], c, "dk")
    same_bits(*runs, "dk")


BC_NODE_SHAPES = [(items, max(1, Bp - 1)) for Bp in (1, 4, 64, 128) for items in (1, second_block(Bp))]


@pytest.mark.gpu
@pytest.mark.parametrize("npe,items,B", [(npe, *s) for npe in (2, 3, 4, 6) for s in BC_NODE_SHAPES] + [(3, 32772, 64)], ids=str)
def test_bc_node_kernels_shapes(npe, items, B):
    """bc_lift with `items` band rows; bc_grad and bc_scatter with `items` Dirichlet nodes."""
    other = max(npe, 3)
    k = KAPPA_LAYOUTS.index("eb") + npe % 2
    bc_lift_case(bc_band(npe, items, other, max(items, other), True), B, KAPPA_LAYOUTS[k], "item", "item")
    x = bc_band(npe, other, items, max(items, other), True)
    bc_grad_case(x, B, KAPPA_LAYOUTS[k], ("item", "item", "item", "item"), True, True)
    bc_scatter_case(x, B, "item", "item")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 70], ids=["B3", "B70"])
@pytest.mark.parametrize("kl", KAPPA_LAYOUTS)
@pytest.mark.parametrize("npe", [2, 3, 4, 6])
def test_bc_node_kernels_layouts(npe, kl, B):
    k = KAPPA_LAYOUTS.index(kl)
    mj = ("item", "sample")
    x = bc_band(npe, 5, npe + 1, 9, True, seed=1)
    assert (np.isin(x["elems"], np.nonzero(x["is_d"])[0]).all(0)).any()             # an element of Dirichlet nodes only
    assert int(np.diff(x["band"]["row_ptr"]).max()) >= 20                             # a band row in many elements
    bc_lift_case(x, B, kl, mj[k % 2], mj[(k // 2) % 2], seed=1)
    bc_grad_case(x, B, kl, tuple(mj[(k >> j) % 2] for j in range(4)), k % 3 != 0, k % 2 == 0, seed=1)
    bc_grad_case(x, B, kl, tuple(mj[1 - (k >> j) % 2] for j in range(4)), k % 3 == 0, k % 2 == 1, seed=2)
    bc_scatter_case(x, B, mj[k % 2], mj[(k // 2) % 2], seed=1)
    bc_scatter_case(x, B, mj[1 - k % 2], mj[k % 2], seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("npe,items,B", [(npe, *s) for npe in (2, 3, 4, 6) for s in GROUP_SHAPES] + [(3, *GROUP_PAST_THE_CAP)],
                         ids=str)
def test_bc_grad_kappa_shapes(npe, items, B):
    extra = 1 if items > 1 else 0                                          # the element of Dirichlet nodes only
    x = bc_band(npe, max(npe + 2, items // 2), max(npe, items // 4), items - extra, False, all_d=bool(extra))
    assert x["band"]["n_be"] == items
    bc_grad_kappa_case(x, B, False, ("item", "item", "item"))
    bc_grad_kappa_case(x, B, True, ("item", "item", "item"), seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 70], ids=["B3", "B70"])
@pytest.mark.parametrize("k", range(8))
@pytest.mark.parametrize("npe", [2, 3, 4, 6])
def test_bc_grad_kappa_layouts(npe, k, B):
    mj = ("item", "sample")
    x = bc_band(npe, 5, npe + 1, 9, True, seed=1)
    majors = tuple(mj[(k >> j) % 2] for j in range(3))
    bc_grad_kappa_case(x, B, False, majors, seed=2)
    bc_grad_kappa_case(x, B, True, majors, seed=3)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: status codes and no-ops (nothing here launches a kernel that reads a bad argument)
# ---------------------------------------------------------------------------------------------------------------------
def _variants(L, name, base, bad, batchpad=(), ok=()):
    """base: ordered {argument: value}.  bad / batchpad / ok: lists of {argument: value} overrides."""
    assert status(L, name, list(base.values())) == 0, name
    for expect, cases in ((BADARG, bad), (BATCHPAD, batchpad), (0, ok)):
        for over in cases:
            assert set(over) <= set(base), over
            assert status(L, name, list({**base, **over}.values())) == expect, (name, over, expect)


def _neg(*names):
    return [{k: -1} for k in names]


@pytest.mark.gpu
def test_status_codes_of_the_robin_entries():
    L = _hip.lib()
    x = band_of(2, 5, False)
    D, tab, rng = x["dev"], x["tab"], np.random.default_rng(0)
    nF, n, B, Bp = x["nF"], x["n"], 3, 4
    one = dv(np.ones(nF * 128))
    area, vals, rhs = Out(nF, rng, [], False), Out(x["W"] * n * 128, rng, [], True), Out(n * 128, rng, [], True)
    base = dict(coords=dv(np.random.default_rng(1).random((2, n))), fac=D["fac"], dim=2, n=n, nF=nF, area=area.fresh(), s=stream())
    _variants(L, "diffhe_robin_facet_table", base,
              [{"coords": None}, {"fac": None}, {"area": None}, {"dim": 0}, {"dim": 4}, {"nF": 0}, {"n": 0}, {"nF": 1 << 27}])
    base = dict(fac=D["fac"], d=2, nF=nF, area=D["area"], rows=D["rows"], row_ptr=D["row_ptr"], ent_code=D["ent_code"],
                ent_slot=D["ent_slot"], n_rows=tab["n_rows"], g=D["g"], h=one, hsf=1, hsb=0, uinf=one, usf=1, usb=nF, q=one,
                qsf=B, qsb=1, vals=vals.fresh(), rhs=rhs.fresh(), n=n, Bv=Bp, B=B, Bp=Bp, s=stream())
    _variants(L, "diffhe_robin_assemble", base,
              [{"fac": None}, {"area": None}, {"g": None}, {"vals": None}, {"rhs": None}, {"d": 0}, {"d": 4}, {"nF": 0}, {"n": 0},
               {"n_rows": -1}, {"B": 0}, {"Bp": 2}, {"Bv": 2}, {"Bv": 0}, {"rows": None}, {"row_ptr": None}, {"ent_code": None},
               {"ent_slot": None}, {"Bv": 1, "hsb": 1}, *_neg("hsf", "hsb", "usf", "usb", "qsf", "qsb")],
              [{"Bp": 3, "Bv": 3}, {"B": 70, "Bp": 96, "Bv": 96}, {"B": 70, "Bp": 96, "Bv": 1}],
              [{"n_rows": 0}, {"n_rows": 0, "rows": None, "row_ptr": None, "ent_code": None, "ent_slot": None},
               {"Bv": 1}, {"Bv": 1, "hsb": 1, "h": None}, {"Bv": 1, "hsb": 1, "B": 1, "Bp": 1}])
    vals.fresh(), rhs.fresh()                                             # no band row: nothing is written
    L.diffhe_robin_assemble(*list({**base, "n_rows": 0, "vals": vals.dev[GUARD:-GUARD], "rhs": rhs.dev[GUARD:-GUARD]}.values()))
    vals.untouched(vals.after(), "vals of n_rows = 0")
    rhs.untouched(rhs.after(), "rhs of n_rows = 0")
    lam = dv(np.zeros((n, Bp)))
    base = dict(fac=D["fac"], d=2, nF=nF, area=D["area"], lam=lam, u=lam, g=None, B=B, Bp=Bp, h=one, hsf=1, hsb=0, uinf=one,
                usf=1, usb=nF, dh=None, dhf=1, dhb=nF, du=None, duf=B, dub=1, dq=None, dqf=1, dqb=0, s=stream())
    _variants(L, "diffhe_robin_grad", base,
              [{"fac": None}, {"area": None}, {"lam": None}, {"u": None}, {"d": 0}, {"d": 4}, {"nF": 0}, {"B": 0}, {"Bp": 2},
               *_neg("hsf", "hsb", "usf", "usb", "dhf", "dhb", "duf", "dub", "dqf", "dqb")])
    # (the base call requests no output: DIFFHE_OK, and there is no buffer it could have written)
    part, tot = Out(4 * B, rng, [], False), Out(B, rng, [], False)
    base = dict(src=one, nF=nF, B=B, part=part.fresh(), out=tot.fresh(), s=stream())
    _variants(L, "diffhe_robin_sum_facets", base, [{"src": None}, {"part": None}, {"out": None}, {"nF": 0}, {"B": 0}])
    assert L.diffhe_robin_sum_blocks(0) == 0


@pytest.mark.gpu
def test_status_codes_of_the_elastic_facet_entries():
    L = _hip.lib()
    x = band_of(2, 5, True)
    D, tab, rng = x["dev"], x["tab"], np.random.default_rng(0)
    nF, n, d, B, Bp = x["nF"], x["n"], 2, 3, 4
    one = dv(np.ones(nF * d * 128))
    area, normal = Out(nF, rng, [], False), Out(d * nF, rng, [], False)
    base = dict(coords=dv(np.random.default_rng(1).random((2, n))), fac=D["fac"], opp=dv(np.zeros(nF, dtype=np.int32)), dim=2, n=n,
                nF=nF, area=area.fresh(), normal=normal.fresh(), s=stream())
    _variants(L, "diffhe_elastf_facet_table", base,
              [{"coords": None}, {"fac": None}, {"opp": None}, {"area": None}, {"normal": None}, {"dim": 1}, {"dim": 4}, {"nF": 0},
               {"n": 0}])
    vals, rhs = Out(d * x["W"] * n * d * 128, rng, [], True), Out(n * d * 128, rng, [], True)
    base = dict(fac=D["fac"], d=d, nF=nF, area=D["area"], normal=D["normal"], rows=D["rows"], row_ptr=D["row_ptr"],
                ent_code=D["ent_code"], ent_slot=D["ent_slot"], n_rows=tab["n_rows"], is_bc=D["is_bc"], g=D["g"], t=one, tsf=d,
                tsc=1, tsb=0, p=one, psf=1, psb=0, kn=one, nsf=1, nsb=0, kt=one, ksf=B, ksb=1, vals=vals.fresh(), rhs=rhs.fresh(),
                n=n, Bv=Bp, B=B, Bp=Bp, s=stream())
    _variants(L, "diffhe_elastf_assemble", base,
              [{"fac": None}, {"area": None}, {"normal": None}, {"is_bc": None}, {"g": None}, {"rhs": None}, {"vals": None},
               {"d": 1}, {"d": 4}, {"nF": 0}, {"n": 0}, {"n_rows": -1}, {"B": 0}, {"Bp": 2}, {"Bv": 2}, {"rows": None},
               {"row_ptr": None}, {"ent_code": None}, {"ent_slot": None}, {"Bv": 1}, {"Bv": 1, "ksb": 0, "nsb": 1},
               *_neg("tsf", "tsc", "tsb", "psf", "psb", "nsf", "nsb", "ksf", "ksb")],
              [{"Bp": 3, "Bv": 3}, {"B": 70, "Bp": 96, "Bv": 96}],
              [{"n_rows": 0}, {"kn": None, "kt": None, "vals": None}, {"t": None, "p": None, "kn": None, "kt": None},
               {"Bv": 1, "ksb": 0}, {"Bv": 1, "kt": None}])
    for over in ({"n_rows": 0}, {"t": None, "p": None, "kn": None, "kt": None}):   # nothing to do: nothing is written
        vals.fresh(), rhs.fresh()
        L.diffhe_elastf_assemble(*list({**base, **over, "vals": vals.dev[GUARD:-GUARD], "rhs": rhs.dev[GUARD:-GUARD]}.values()))
        vals.untouched(vals.after(), f"vals of {over}")
        rhs.untouched(rhs.after(), f"rhs of {over}")
    lam = dv(np.zeros((n * d, Bp)))
    base = dict(fac=D["fac"], d=d, nF=nF, area=D["area"], normal=D["normal"], lam=lam, x=lam, g=None, B=B, Bp=Bp, dt=None, tf=d,
                tc=1, tb=0, dp=None, pf=1, pb=nF, dkn=None, nf=B, nb=1, dkt=None, kf=1, kb=0, s=stream())
    _variants(L, "diffhe_elastf_grad", base,
              [{"fac": None}, {"area": None}, {"normal": None}, {"lam": None}, {"x": None}, {"d": 1}, {"d": 4}, {"nF": 0}, {"B": 0},
               {"Bp": 2}, *_neg("tf", "tc", "tb", "pf", "pb", "nf", "nb", "kf", "kb")])


@pytest.mark.gpu
def test_status_codes_of_the_dirichlet_entries():
    L = _hip.lib()
    x = bc_band(3, 5, 4, 9, True, seed=1)
    D, band, rng = x["dev"], x["band"], np.random.default_rng(0)
    n, m, B = x["n"], x["m"], 3
    one = dv(np.ones(max(n, m) * B))
    mesh = dict(elems=D["elems"], npe=3, m=m, k0=D["k0"])
    bad_mesh = [{"elems": None}, {"k0": None}, {"d_slot": None}, {"npe": 1}, {"npe": 7}, {"m": 0}]
    outs = {k: Out(max(n, m) * B, rng, [], True) for k in ("rhs", "out", "dots", "u", "dk")}
    check = []

    def unchanged(name, base, over, *keys):
        for k in keys:
            outs[k].fresh()
        args = {**base, **over, **{k: outs[k].dev[GUARD:-GUARD] for k in keys}}
        assert status(L, name, list(args.values())) == 0, (name, over)
        for k in keys:
            outs[k].untouched(outs[k].after(), f"{name} {over}: {k}")
        check.append(name)

    base = dict(**mesh, kappa=one, kse=B, ksb=1, d_slot=D["d_slot"], G=one, gsj=B, gsb=1, rows=D["rows"], row_ptr=D["row_ptr"],
                row_inc=D["row_inc"], n_rows=band["n_rows"], rhs=outs["rhs"].fresh(), rsn=B, rsb=1, B=B, s=stream())
    _variants(L, "diffhe_bc_lift", base,
              bad_mesh + [{"G": None}, {"rhs": None}, {"B": 0}, {"n_rows": -1}, {"rows": None}, {"row_ptr": None},
                          {"row_inc": None}, *_neg("kse", "ksb", "gsj", "gsb", "rsn", "rsb")], ok=[{"kappa": None}])
    unchanged("diffhe_bc_lift", base, {"n_rows": 0, "rows": None, "row_ptr": None, "row_inc": None}, "rhs")
    base = dict(**mesh, kappa=one, kse=B, ksb=1, d_slot=D["d_slot"], d_idx=D["d_idx"], d_ptr=D["d_ptr"], d_inc=D["d_inc"],
                n_d=band["n_d"], lam=one, lsn=B, lsb=1, gbar=one, gsn=B, gsb=1, out=outs["out"].fresh(), osj=B, osb=1, G=one, Gsj=B,
                Gsb=1, dots=outs["dots"].fresh(), B=B, s=stream())
    _variants(L, "diffhe_bc_grad", base,
              bad_mesh + [{"lam": None}, {"out": None}, {"G": None}, {"B": 0}, {"n_d": -1}, {"d_idx": None}, {"d_ptr": None},
                          {"d_inc": None}, *_neg("kse", "ksb", "lsn", "lsb", "gsn", "gsb", "osj", "osb", "Gsj", "Gsb")],
              ok=[{"gbar": None}, {"dots": None, "G": None}, {"dots": None, "G": None, "Gsj": -1}])
    unchanged("diffhe_bc_grad", base, {"n_d": 0, "d_idx": None, "d_ptr": None, "d_inc": None}, "out", "dots")
    base = dict(d_idx=D["d_idx"], n_d=band["n_d"], G=one, gsj=B, gsb=1, u=outs["u"].fresh(), usn=B, usb=1, B=B, s=stream())
    _variants(L, "diffhe_bc_scatter", base,
              [{"G": None}, {"u": None}, {"B": 0}, {"n_d": -1}, {"d_idx": None}, *_neg("gsj", "gsb", "usn", "usb")])
    unchanged("diffhe_bc_scatter", base, {"n_d": 0, "d_idx": None}, "u")
    base = dict(**mesh, d_slot=D["d_slot"], band_elems=D["band_elems"], n_be=band["n_be"], lam=one, lsn=B, lsb=1, G=one, gsj=B,
                gsb=1, dk=outs["dk"].fresh(), dse=B, dsb=1, shared=0, B=B, s=stream())
    _variants(L, "diffhe_bc_grad_kappa", base,
              bad_mesh + [{"lam": None}, {"G": None}, {"dk": None}, {"B": 0}, {"n_be": -1}, {"band_elems": None},
                          *_neg("lsn", "lsb", "gsj", "gsb", "dse", "dsb")], ok=[{"shared": 1, "dsb": 0, "dse": 1}])
    unchanged("diffhe_bc_grad_kappa", base, {"n_be": 0, "band_elems": None}, "dk")
    unchanged("diffhe_bc_grad_kappa", base, {"n_be": 0, "shared": 1}, "dk")
    assert len(check) == 5


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the host table builders of diffhe/plan.py on small real meshes
# ---------------------------------------------------------------------------------------------------------------------
def _interior_dirichlet():
    base = FEMesh.rectangle(6, 5)
    bc = {k: 0.1 * k for k in list(base.dirichlet_nodes)[::3]}
    bc.update({0: 0.2, 1: 0.3, 2: 0.4})                                    # two boundary edges of Dirichlet nodes only
    bc.update({16: 1.0, 17: -1.0, 25: 0.5})                                # interior nodes of the 7 x 6 lattice
    return FEMesh(nodes=base.nodes, elements=base.elements, dirichlet_nodes=bc)


def _table_meshes():
    import test_robin as tr
    out = {name: tr.case_mesh(name)[0] for name in ("jittered2d", "box", "line")}
    out["interior"] = _interior_dirichlet()
    return out


def _host(tab):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in tab.items()}


def _same_table(got, ref, cols, facets, lifted):
    for key in ("d", "n_f", "n_rows"):
        assert got[key] == ref[key], key
    for key in ("fac", "rows", "row_ptr", "ent_code", "ent_slot"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], ref[key]), key
    assert (np.diff(got["rows"]) > 0).all()
    row, F, p, c, slot = table_entries(got)
    assert (facets[F, p] == row).all()
    for a, b in zip(got["row_ptr"][:-1], got["row_ptr"][1:]):
        assert (np.diff(F[a:b] * 16 + p[a:b] * 4 + c[a:b]) > 0).all()     # facet order inside a row
    col = facets[F, c]
    assert ((slot < 0) == lifted[col]).all()
    assert (cols[slot[slot >= 0], row[slot >= 0]] == col[slot >= 0]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("subset", ["all", "subset", "dirichlet-only"])
@pytest.mark.parametrize("name", ["jittered2d", "box", "line", "interior"])
def test_plan_robin_table_against_the_brute_force_builder(name, subset):
    from diffhe.plan import get_plan
    mesh = _table_meshes()[name]
    every = mesh.boundary_facets().numpy()
    is_bc = np.zeros(mesh.n_nodes, dtype=bool)
    is_bc[list(mesh.dirichlet_nodes)] = True
    on_d = is_bc[every].all(1)
    facets = {"all": every, "subset": every[~on_d][::2], "dirichlet-only": every[on_d]}[subset]
    assert len(facets) > 0
    plan = get_plan(mesh, torch.device(DEV), prune=False)
    tab = plan.robin_table(("test", name, subset), facets)
    got = _host(tab)
    cols = plan.cols.cpu().numpy()
    ref = bm.robin_table(facets, is_bc, cols)
    _same_table(got, ref, cols, facets, is_bc)
    assert (got["n_rows"] == 0) == (subset == "dirichlet-only")
    area, S = bm.facet_area(mesh.nodes.numpy().T, facets.T)
    assert (np.abs(got["area"] - area) <= 14 * EPS * S).all()
    assert plan.robin_table(("test", name, subset), facets) is tab                     # built once per (plan, facet set)


@pytest.mark.gpu
@pytest.mark.parametrize("subset", ["all", "subset"])
@pytest.mark.parametrize("name", ["jittered2d", "box", "interior"])
def test_plan_elastic_facet_table_against_the_brute_force_builder(name, subset):
    from diffhe.elastic_facets import opposite_nodes
    from diffhe.plan import get_plan
    mesh = _table_meshes()[name]
    every = mesh.boundary_facets().numpy()
    facets = every if subset == "all" else every[1::3]
    opp = opposite_nodes(mesh.elements.numpy(), facets)
    plan = get_plan(mesh, torch.device(DEV), prune=False)
    got = _host(plan.elastic_facet_table(("test", name, subset), facets, opp))
    cols = plan.cols.cpu().numpy()
    _same_table(got, bm.elastic_table(facets, cols), cols, facets, np.zeros(mesh.n_nodes, dtype=bool))
    assert (got["ent_slot"] >= 0).all() and np.array_equal(got["rows"], np.unique(facets))
    area, S_area, normal, S_normal, out, S_out = bm.facet_normal(mesh.nodes.numpy().T, facets.T, opp)
    assert (np.abs(out) > 1e-6 * S_out).all()
    assert (np.abs(got["area"] - area) <= 14 * EPS * S_area).all()
    assert (np.abs(got["normal"] - normal) <= 18 * EPS * S_normal).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["jittered2d", "box", "line", "interior"])
def test_plan_dirichlet_band_against_the_brute_force_builder(name):
    from diffhe.plan import get_plan
    mesh = _table_meshes()[name]
    is_bc = np.zeros(mesh.n_nodes, dtype=bool)
    is_bc[list(mesh.dirichlet_nodes)] = True
    got = _host(get_plan(mesh, torch.device(DEV)).dirichlet_band())
    ref = bm.dirichlet_band(mesh.elements.numpy(), is_bc)
    assert sorted(got) == sorted(ref)
    for key, v in ref.items():
        if isinstance(v, np.ndarray):
            assert got[key].dtype == np.int32 and np.array_equal(got[key], v), key
        else:
            assert got[key] == v, key


@pytest.mark.gpu
def test_robin_table_is_none_on_the_pruned_box_pattern_and_the_solver_takes_the_unpruned_plan():
    import test_robin as tr
    from diffhe import RobinFESolver
    from diffhe.plan import get_plan
    mesh = tr.case_mesh("box")[0]
    facets = mesh.boundary_facets().numpy()
    is_bc = np.zeros(mesh.n_nodes, dtype=bool)
    is_bc[list(mesh.dirichlet_nodes)] = True
    pruned = get_plan(mesh, torch.device(DEV))
    pruned.ensure_ell()
    assert pruned.prune and pruned.pruned_entries
    assert pruned.robin_table("every", facets) is None
    assert bm.robin_table(facets, is_bc, pruned.cols.cpu().numpy()) is None            # a face diagonal has no slot
    solver = RobinFESolver(mesh, 1.0, device=DEV)
    plan = solver._plan()
    assert not plan.prune
    got = _host(plan.robin_table(solver._facet_key, solver._facets_host))
    cols = plan.cols.cpu().numpy()
    _same_table(got, bm.robin_table(facets, is_bc, cols), cols, facets, is_bc)
