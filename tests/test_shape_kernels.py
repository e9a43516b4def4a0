"""The node-coordinate gradient kernels called directly: diffhe_p1_shape_grad (csrc/shape.hip), diffhe_elast_shape_grad and
diffhe_stress_shape_grad (csrc/elastic_shape.hip, csrc/stress_form.h) and the node pass they share (csrc/shape_gather.h),
on seeded synthetic host arrays -- random element lists into n nodes, random tables and nodal fields; no mesh, no solver,
no plan -- against a numpy model: values per element and sample in float64, every sum over samples and over incidence
lists in longdouble.

Formulas (d the dimension, NPE = d + 1 vertices, g_p = grad phi_p the constant P1 gradients, A_e the element size;
what element e adds to the coordinate k of its vertex p is work[e, p d + k], the node gradient is the sum of these rows over
the node's incidence list):

  scalar   dL/dX of lambda^T (K(X) u - F(X) + c M_L(X) u) = 0, u the full field (u + g):
           work[e, p] = A_e [ (q_e - tr T_e) I + T_e + T_e^T ] g_p
           T_e = sum_b kappa_eb grad u_eb (x) grad lambda_eb,      grad v = sum_p v_p g_p
           q_e = sum_b [ load_eb - c sum_p lambda_pb u_pb / (d+1) ]
           load_eb = (sum_p lambda_pb)(sum_p f_pb) / (d+1)^2 (2D, 3D),   sum_p lambda_pb f_pb / 2 (1D)
           g_p and A_e come from the coordinates; a degenerate element (det = 0) adds nothing.
  elastic  H_w[a][t] = sum_p w_(p,a) g_p[t] for w = u + g and w = lambda, S(H) = 2 mu1 sym(H) + lam1 tr(H) I:
           work[e, p] = A_e [ sum_b E_eb ( H_u^T S(H_l) + H_l^T S(H_u) - (S(H_u) : H_l) I ) + q_e I ] g_p
           q_e = sum_b sum_a (sum_p lambda_(p,a)) (sum_p f_(p,a)) / (d+1)^2;   g_p (table) and A_e (vol) are inputs.
  stress   sigma = E S(H_u) at fixed u; nn = (sigma_xx, sigma_yy, sigma_zz) with sigma_zz = nu_z (sigma_xx + sigma_yy) in
           2D; vm = sqrt(3/2 |dev nn|^2 + 3 sum shear^2).  With the cotangent c = sigma_bar + vm_bar d vm / d sigma
           (d vm / d nn_i = 3/2 (nn_i - mean nn) / vm, d vm / d sigma_shear = 3 sigma_shear / vm, 0 where vm = 0; in 2D the
           sigma_zz part reaches xx and yy through nu_z) and P = dL/dH = E (2 mu1 sym(C) + lam1 tr(C) I):
           work[e, p] = -(sum_b H_u^T P_b) g_p.

Bounds.  |kernel - model| <= c * 2^-53 * S: S is the model evaluated on absolute values (every input replaced by its
magnitude, every subtraction by an addition), c the number of roundings on the longest chain from an input to the result,
kernel plus model; an fma only shortens a chain, a product of two inexact factors adds their chains, a sum of n terms adds
n to the longest of theirs.  The kernel's chains (the float64 model follows the same formulas up to the sum over the
samples and is exact enough to be free from there on, so its chain is no longer):

  scalar   g_p = cofactor / det: 2 (the 1 / det and the product; see below).  u + g: 1.  grad u: 1 + 2 + 1 + NPE = NPE + 4,
           grad lambda: NPE + 3.  A term of T: the two and 2 products, 2 NPE + 9.  tr T: + d.  (q - tr) g: + 1 + 2 + 1; the
           terms (T + T^T) g are shorter by d; joining them: + d; the size (|det| / 6 in 3D) and its product: + 2.
           chain = 2 NPE + 2 d + 15 = 4 d + 17.  (q's own chain, 2 NPE + 3, is shorter than T's.)
  elastic  H_u: 2 NPE fmas (the lift first), H_l: NPE.  S(H): + d + 2.  S_u : H_l: 3 NPE + d + 2 + d^2.  The bracket starts
           from it and adds 2 d fmas: 3 NPE + d^2 + 3 d + 2.  E: + 1.  q I: + 1.  The contraction with g_p: + d, vol: + 1.
           chain = 3 NPE + d^2 + 4 d + 5 = d^2 + 7 d + 8.
  stress   sigma_bar alone: H NPE, P: d + 3, H^T P: + d, the contraction: + d + 1: chain = NPE + 3 d + 4 = 4 d + 5.
           With vm_bar: k_nn = NPE + d + 5 roundings to a normal stress (H, S, E, the nu_z sum), see below for
           k_c = 2 k_nn + 11 to the cotangent; then as before: chain = NPE + k_c + 3 d + 4 = 8 d + 28.
  samples  the loop b += LB and the log2 LB levels of the butterfly are at most B additions on a chain (kernel only).

  c_elem = 2 chain + B for work.  A node's sum over its list adds len(list) roundings whatever the order (the longdouble
  reference adds none): c = c_elem + len(list), S summed over the list.

Two places need more than a count:
  * The scalar entry's 1 / det.  Coordinates are multiples of 2^-8 in [0, 2): differences, cofactors and determinants are
    exact in float64 (at most 30 bits), so 1 / det and the product with it are the only geometric roundings -- two per
    gradient component, no conditioning factor -- and an element is degenerate exactly when det == 0: otherwise
    |det| >= 2^-16 (2D) or 2^-24 (3D), far from the kernel's thresholds (area < 1e-15; |det| <= 1e-12 l^3 <= 4.2e-11).
    The host asserts this for the drawn inputs.  The model takes g_p from integer cofactors (coordinates * 256 in int64).
  * The von Mises branch.  dev = nn - mean and vm come from cancelled differences, so per (e, b) their errors are
    absolute: with A = sum_k |sigma_k| on absolute values (sigma_zz included), err(dev_i) <= (k_nn + 4) eps 4/3 A and,
    from |nn_i - nn_j| <= sqrt 2 vm and |shear| <= vm / sqrt 3, relerr(vm) <= (1.74 (k_nn + 1) + 8) eps A / vm.  With
    |dev_i| <= sqrt(2/3) vm this gives err(3/2 dev_i vm_bar / vm) <= (4.5 k_nn + 27) eps |vm_bar| A / vm and less for the
    shear components.  So on absolute values every component of vm_bar d vm / d sigma is replaced by 3 |vm_bar| A / vm,
    vm from the longdouble model, with k_cn = 2 k_nn + 9 >= (4.5 k_nn + 27) / 3 roundings, and k_c = k_cn + 2 after the
    sum with sigma_bar and the nu_z fma.  The bound widens exactly where the operation is ill-conditioned; no case is
    excluded and no seed rejected.  Where u = 0 on an element vm = 0 exactly and the vm_bar part is exactly 0.

Shapes (LB = min(next power of two >= B, 64) lanes per element; the scalar entry takes LB = 1 unless the batch is
innermost; a 256-thread block holds 4 * (64 / LB) elements, at most 8192 blocks are launched):
  B = 1, 2, 3, 5, 9, 17, 33, 64 with the smallest valid pad: LB = 1 ... 64, idle lanes wherever B < LB, and the rule
      "component ci is written by lane ci % LB" on both sides of LB = NC = (d+1) d (6 in 2D, 12 in 3D);
  (B, Bp) = (70, 128), (129, 192): two and three trips of b += LB, the last one ragged;
  each with m = 1 and with m = 4 * (64 / LB) + 1: a second block that holds one element, its other waves and groups idle;
  m = 8192 * 4 + 1 at B = 64 (LB = 64) and m = 8192 * 16 + 1 at B = 9 (LB = 16): one element past the block cap, the
      second trip of e += stride, for every entry and dimension with one layout each.  The LB = 1 cap (beyond 2 097 152
      elements) is left out: it runs the same e += stride line and its numpy model would take far more than a few seconds;
  sample-major scalar calls (LB = 1) at m = 257: their second block;
  the gather: n = 1 048 600, d = 2, m = 5 (past 8192 blocks of 256, almost every list empty: exactly 0.0 over NaN);
      n = 700 000, d = 3; one node in all of m = 300 elements (a long list, summed in list order);
  degenerate rows: the scalar entry with a repeated node, three collinear and four coplanar grid points (det == 0 exactly),
      the table entries with a zero table column and vol = 0 -- rows of magnitude 0.0, everything else bitwise unchanged
      when those elements' nodal data changes;
  vm = 0: elements with u = 0.

Padding samples (b >= B) hold NaN in u, lambda, f, the cotangents and the per-sample coefficients; work and grad are
pre-filled with NaN: every entry of both must come back finite."""
import itertools
import math

import numpy as np
import pytest
import torch

from diffhe import _hip

T64 = torch.float64
DEV = "cuda:0"
EPS = 2.0 ** -53
LD = np.longdouble
LAM1, MU1 = 0.5769230769230769, 0.3846153846153846      # nu = 0.3
CHUNK = 1024                                             # elements per pass of the model (bounds its memory)
VOIGT = {2: [(0, 0), (1, 1), (0, 1)], 3: [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]}
ENTRY_ID = {"p1": 1, "elast": 2, "stress": 3}


def group_lanes(B):
    LB = 1
    while LB < B and LB < 64:
        LB <<= 1
    return LB


def smallest_pad(B):
    return group_lanes(B) if B <= 64 else 64 * ((B + 63) // 64)


def second_block(LB):
    """One element more than the first block holds: 4 waves of 64 / LB elements."""
    return 4 * (64 // LB) + 1


def chain(entry, d, vm=True):
    """Roundings on the kernel's longest chain to a row of work, without the sample additions (module docstring)."""
    if entry == "p1":
        return 4 * d + 17
    if entry == "elast":
        return d * d + 7 * d + 8
    return 8 * d + 28 if vm else 4 * d + 5


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def incidence(elems, n):
    """(inc_ptr (n+1), inc) by the rule of SolvePlan.shape_incidence: a stable argsort of the flattened (m, npe) list --
    per node the codes e * npe + p in element order."""
    flat = elems.T.reshape(-1)
    order = np.argsort(flat, kind="stable").astype(np.int32)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=n), out=ptr[1:])
    return ptr.astype(np.int32), order


def _distinct_elems(rng, n, npe, m):
    el = rng.integers(0, n, size=(npe, m))
    for p in range(1, npe):
        while True:
            dup = (el[p][None, :] == el[:p]).any(axis=0)
            if not dup.any():
                break
            el[p, dup] = rng.integers(0, n, size=int(dup.sum()))
    return el


def make_case(entry, d, m, B, Bp, n=None, elems=None, ndeg=0, nzero=0, seed=0):
    """Seeded host arrays of one case, the real samples only (the runners add the padding): elems (npe, m) into n nodes
    with its incidence list; u / lam / f (dofs, B), g (dofs); the coefficient (kappa or E) as a scalar, per element, per
    sample and per both; the scalar entry's coords (d, n), the table entries' gtab (npe d, m) and vol (m), the stress
    entry's cotangents sbar (nc, m, B), vbar (m, B).  ndeg elements are degenerate and nzero carry u = 0; both kinds sit on
    nodes of their own (x["deg"], x["zero"]: the elements; x["deg_nodes"]: the former's nodes)."""
    npe = d + 1
    rng = np.random.default_rng([seed, ENTRY_ID[entry], d, m, B])
    if n is None:
        n = min(max(npe + 2, m // 2), 4099)
    if elems is None:
        elems = _distinct_elems(rng, n, npe, m) if entry == "p1" else rng.integers(0, n, size=(npe, m))
    elems = np.array(elems, dtype=np.int64)
    special = ndeg + nzero
    where = rng.choice(m, size=special, replace=False) if special else np.zeros(0, dtype=np.int64)
    own = n + np.arange(special * npe).reshape(special, npe).T          # (npe, special)
    if special:
        elems[:, where] = own
    n_all = n + special * npe
    nd = 1 if entry == "p1" else d
    dofs = n_all * nd
    x = {"entry": entry, "d": d, "npe": npe, "m": m, "B": B, "Bp": Bp, "n": n_all, "nd": nd,
         "deg": where[:ndeg], "zero": where[ndeg:], "deg_nodes": own[:, :ndeg].reshape(-1),
         "u": rng.standard_normal((dofs, B)), "lam": rng.standard_normal((dofs, B)), "g": rng.standard_normal(dofs),
         "f": rng.standard_normal((dofs, B)),
         "coef": {"s": 1.3, "e": rng.random(m) + 0.5, "b": rng.random(B) + 0.5, "eb": rng.random((m, B)) + 0.5}}
    if entry == "p1":
        x["fshared"] = rng.standard_normal(n_all)
        units = rng.integers(0, 512, size=(d, n_all))
        for i in range(ndeg):                       # det == 0 exactly, three ways
            nodes, kind = own[:, i], i % 3
            if kind == 0 or d == 1:
                if i % 2 == 0:
                    elems[1, where[i]] = nodes[0]                                   # a repeated node
                else:
                    units[:, nodes[1]] = units[:, nodes[0]]                          # 1D: two nodes at one point
            elif kind == 1 or d == 2:
                step = np.array([3, 5, 7][:d]) if kind == 1 else np.array([6, 1, 2][:d])
                base = rng.integers(0, 256, size=d)
                for j in range(3):                                                   # three collinear grid points
                    units[:, nodes[j]] = base + j * step
            else:
                base, s, t = rng.integers(0, 256, size=3), np.array([5, 1, 2]), np.array([1, 7, 3])
                for j, off in enumerate((0 * s, s, t, s + t)):                       # four coplanar grid points
                    units[:, nodes[j]] = base + off
        x["coords"] = units / 256.0
    else:
        x["gtab"] = rng.standard_normal((npe * d, m))
        x["vol"] = rng.random(m) + 0.5
        x["gtab"][:, x["deg"]] = 0.0
        x["vol"][x["deg"]] = 0.0
    if entry == "stress":
        nc = d * (d + 1) // 2
        x["sbar"] = rng.standard_normal((nc, m, B))
        x["vbar"] = rng.standard_normal((m, B))
        rows = (own[:, ndeg:].reshape(-1)[:, None] * d + np.arange(d)[None, :]).reshape(-1)
        x["u"][rows] = 0.0
    x["elems"] = elems.astype(np.int32)
    x["inc_ptr"], x["inc"] = incidence(x["elems"], n_all)
    return x


def with_other_nodal_data(x, nodes):
    """A copy of the case with every nodal value on `nodes` replaced by other finite values."""
    rng = np.random.default_rng(99)
    y = dict(x)
    rows = (np.asarray(nodes)[:, None] * x["nd"] + np.arange(x["nd"])[None, :]).reshape(-1)
    for key in ("u", "lam", "f", "g"):
        y[key] = x[key].copy()
        y[key][rows] = 3.0 + rng.random((len(rows),) + x[key].shape[1:])
    if "fshared" in x:
        y["fshared"] = x["fshared"].copy()
        y["fshared"][nodes] = -2.5
    return y


def subset(x, idx):
    """The case restricted to the elements idx (its per-element rows of work are those of the whole case)."""
    y = dict(x)
    y["m"] = len(idx)
    y["elems"] = x["elems"][:, idx]
    y["coef"] = dict(x["coef"], e=x["coef"]["e"][idx], eb=x["coef"]["eb"][idx])
    for key in ("gtab", "sbar"):
        if key in x:
            y[key] = x[key][:, idx]
    for key in ("vol", "vbar"):
        if key in x:
            y[key] = x[key][idx]
    return y


def coef_host(x, lay):
    """The coefficient of layout lay as (m, B) values."""
    c, shape = x["coef"], (x["m"], x["B"])
    if lay == "s":
        return np.full(shape, c["s"])
    if lay == "e":
        return np.broadcast_to(c["e"][:, None], shape)
    if lay == "b":
        return np.broadcast_to(c["b"][None, :], shape)
    return c["eb"]          # "eb" (m, Bp) and the element-major "em" (Bp, m)


P1_OPTS = [dict(kappa=k, f=f, c=c, g=g) for k, f, c, g in
           itertools.product(("s", "b", "e", "eb"), (None, "shared", "sample"), (0.0, 0.7), (False, True))]
P1_FULL = dict(kappa="eb", f="sample", c=0.7, g=True)
EL_OPTS = [dict(E=e, g=g, f=f) for e, g, f in itertools.product(("s", "e", "b", "eb", "em"), (False, True), (False, True))]
EL_FULL = dict(E="eb", g=True, f=True)


def stress_opts(d):
    return [dict(E=e, nu_z=z, sig=s, vm=v, lay=lay)
            for z in ((0.0, 0.3) if d == 2 else (0.0,)) for e in ("s", "e", "b", "eb", "em")
            for s, v in ((True, False), (False, True), (True, True)) for lay in (("cm", "mc") if s else ("cm",))]


def stress_full(d):
    return dict(E="eb", nu_z=0.3 if d == 2 else 0.0, sig=True, vm=True, lay="cm")


def options(entry, d):
    return {"p1": P1_OPTS, "elast": EL_OPTS}.get(entry) or stress_opts(d)


def full_option(entry, d):
    return {"p1": P1_FULL, "elast": EL_FULL}.get(entry) or stress_full(d)


def c_elem(x, opt):
    return 2 * chain(x["entry"], x["d"], opt.get("vm", True)) + x["B"]


# ---------------------------------------------------------------------------------------------------------------------
# the model: -> W (m, npe, d) longdouble.  dt is the type of the values per element and sample (float64: the reference;
# longdouble: its own check); ab evaluates the same expression on absolute values (S of the bound).
# ---------------------------------------------------------------------------------------------------------------------
def p1_geometry(x, dt=np.float64):
    """grad phi_p (m, npe, d), the element size (m) and det != 0 (m) from integer cofactors: the coordinates are multiples
    of 2^-8, so cofactors and determinants are exact and the one rounding is the division."""
    d, m = x["d"], x["m"]
    units = np.rint(x["coords"] * 256.0).astype(np.int64)
    assert (units == x["coords"] * 256.0).all() and units.min() >= 0 and units.max() < 512
    P = units[:, x["elems"].astype(np.int64)]                 # (d, npe, m)
    e = [P[:, i + 1, :] - P[:, 0, :] for i in range(d)]      # edge vectors from vertex 0, (d, m) each
    if d == 1:
        cof, det = [np.ones((1, m), dtype=np.int64)], e[0][0]
    elif d == 2:
        cof = [np.stack([e[1][1], -e[1][0]]), np.stack([-e[0][1], e[0][0]])]
        det = e[0][0] * e[1][1] - e[0][1] * e[1][0]
    else:
        cof = [np.cross(e[1], e[2], axis=0), np.cross(e[2], e[0], axis=0), np.cross(e[0], e[1], axis=0)]
        det = (e[0] * cof[0]).sum(axis=0)
    cof = np.stack([-sum(cof)] + cof)                        # (npe, d, m): vertex 0 closes the partition of unity
    ok = det != 0
    # the kernel's view of "degenerate" is the same: a nonzero determinant is far above both of its thresholds
    if ok.any() and d > 1:
        assert np.abs(det[ok]).min() * 2.0 ** (-8 * d) >= (2.0 ** -16 if d == 2 else 2.0 ** -24)
        assert 1e-12 * 12.0 ** 1.5 < 2.0 ** -25
    safe = np.where(ok, det, 1).astype(dt)
    G = np.where(ok, 256 * cof.astype(dt) / safe, 0).transpose(2, 0, 1)
    size = np.where(ok, np.abs(safe) / dt(256.0 ** d) / math.factorial(d), 0)
    return G, size, ok


def _chunks(m):
    return [slice(lo, min(lo + CHUNK, m)) for lo in range(0, m, CHUNK)]


def _mat(d, f):
    """A d x d matrix as nested lists of whatever f(a, t) returns (arrays over elements and samples)."""
    return [[f(a, t) for t in range(d)] for a in range(d)]


def _bsum(v):
    """The sum over the samples (the last axis) in longdouble."""
    return v.sum(axis=1, dtype=LD)


def _contract(x, M, Gc, scale):
    """rows (mc, npe, d) of work: scale * sum_t M[k][t] g_p[t], in longdouble."""
    d, npe = x["d"], x["npe"]
    Gl = Gc.astype(LD)
    out = np.zeros((Gc.shape[0], npe, d), dtype=LD)
    for p in range(npe):
        for k in range(d):
            out[:, p, k] = scale * sum(M[k][t] * Gl[:, p, t] for t in range(d))
    return out


def p1_model(x, opt, dt=np.float64, ab=False):
    d, npe, m = x["d"], x["npe"], x["m"]
    A = np.abs if ab else (lambda a: a)
    G, size, _ = p1_geometry(x, dt)
    G = A(G)
    U, Lm = A(x["u"].astype(dt)), A(x["lam"].astype(dt))
    if opt["g"]:
        U = U + A(x["g"].astype(dt))[:, None]
    F = None
    if opt["f"] == "sample":
        F = A(x["f"].astype(dt))
    elif opt["f"] == "shared":
        F = A(x["fshared"].astype(dt))[:, None]
    kap = coef_host(x, opt["kappa"]).astype(dt)
    W = np.zeros((m, npe, d), dtype=LD)
    for sl in _chunks(m):
        v = x["elems"][:, sl]
        Up, Lp, Gc = U[v], Lm[v], G[sl]                                    # (npe, mc, B), (mc, npe, d)
        gu = [sum(Up[p] * Gc[:, p, k, None] for p in range(npe)) for k in range(d)]
        gl = [sum(Lp[p] * Gc[:, p, k, None] for p in range(npe)) for k in range(d)]
        T = _mat(d, lambda a, k: _bsum(kap[sl] * gu[a] * gl[k]))
        qb = dt(opt["c"]) * sum(Lp[p] * Up[p] for p in range(npe)) / npe
        qb = qb if ab else -qb
        if F is not None:
            Fp = F[v]
            qb = qb + (0.5 * (Lp[0] * Fp[0] + Lp[1] * Fp[1]) if d == 1 else Lp.sum(axis=0) * Fp.sum(axis=0) / (npe * npe))
        tr = sum(T[a][a] for a in range(d))
        head = _bsum(qb) + tr if ab else _bsum(qb) - tr
        M = _mat(d, lambda k, j: T[k][j] + T[j][k] + (head if k == j else 0.0))
        W[sl] = _contract(x, M, Gc, size[sl].astype(LD))
    return W


def _grad_matrix(Vp, Gc):
    """H[a][t] = sum_p v_(p,a) g_p[t] from Vp (npe, d, mc, B) and Gc (mc, npe, d)."""
    npe, d = Vp.shape[0], Vp.shape[1]
    return _mat(d, lambda a, t: sum(Vp[p, a] * Gc[:, p, t, None] for p in range(npe)))


def _unit_stress(H, lam1, mu1):
    """S(H) = 2 mu1 sym(H) + lam1 tr(H) I."""
    d = len(H)
    tr = sum(H[a][a] for a in range(d))
    return _mat(d, lambda a, t: mu1 * (H[a][t] + H[t][a]) + (lam1 * tr if a == t else 0.0))


def _dof_fields(x, v, fields):
    """fields (dofs, B) at the dofs (p, a) of the elements v (npe, mc) -> (npe, d, mc, B) each."""
    d = x["d"]
    dof = v.astype(np.int64)[:, None, :] * d + np.arange(d)[None, :, None]
    return [f[dof] for f in fields]


def elast_model(x, opt, dt=np.float64, ab=False):
    d, npe, m = x["d"], x["npe"], x["m"]
    A = np.abs if ab else (lambda a: a)
    G = A(x["gtab"].astype(dt)).reshape(npe, d, m).transpose(2, 0, 1)
    U, Lm = A(x["u"].astype(dt)), A(x["lam"].astype(dt))
    if opt["g"]:
        U = U + A(x["g"].astype(dt))[:, None]
    F = A(x["f"].astype(dt)) if opt["f"] else None
    Ee = coef_host(x, opt["E"]).astype(dt)
    W = np.zeros((m, npe, d), dtype=LD)
    for sl in _chunks(m):
        v, Gc, Ec = x["elems"][:, sl], G[sl], Ee[sl]
        Up, Lp = _dof_fields(x, v, (U, Lm))
        Hu, Hl = _grad_matrix(Up, Gc), _grad_matrix(Lp, Gc)
        Su, Sl = _unit_stress(Hu, dt(LAM1), dt(MU1)), _unit_stress(Hl, dt(LAM1), dt(MU1))
        dot = sum(Su[a][t] * Hl[a][t] for a in range(d) for t in range(d))
        q = 0.0
        if F is not None:
            Fp, = _dof_fields(x, v, (F,))
            sl_, sf_ = Lp.sum(axis=0), Fp.sum(axis=0)
            q = _bsum(sum(sl_[a] * sf_[a] for a in range(d)) / (npe * npe))

        def bracket(k, t):
            s = sum(Hu[a][k] * Sl[a][t] + Hl[a][k] * Su[a][t] for a in range(d))
            if k == t:
                s = s + dot if ab else s - dot
            return _bsum(Ec * s) + (q if k == t else 0.0)
        W[sl] = _contract(x, _mat(d, bracket), Gc, A(x["vol"][sl]).astype(LD))
    return W


def _stress_of(x, opt, U, Gc, Ec, v, dt):
    """H, sigma (nested d x d of (mc, B)) and the out-of-plane normal stress (mc, B) of the elements v."""
    d = x["d"]
    Up, = _dof_fields(x, v, (U,))
    H = _grad_matrix(Up, Gc)
    s = _unit_stress(H, dt(LAM1), dt(MU1))
    sg = _mat(d, lambda a, t: Ec * s[a][t])
    szz = dt(opt["nu_z"]) * (sg[0][0] + sg[1][1]) if d == 2 else sg[2][2]
    return H, sg, szz


def stress_model(x, opt, dt=np.float64, ab=False):
    d, npe, m, B = x["d"], x["npe"], x["m"], x["B"]
    nv = VOIGT[d]
    A = np.abs if ab else (lambda a: a)
    G = x["gtab"].astype(dt).reshape(npe, d, m).transpose(2, 0, 1)
    U = x["u"].astype(dt)
    U_ld = x["u"].astype(LD) if ab and opt["vm"] else None
    Ee = coef_host(x, opt["E"]).astype(dt)
    W = np.zeros((m, npe, d), dtype=LD)
    for sl in _chunks(m):
        v, mc, Ec = x["elems"][:, sl], x["elems"][:, sl].shape[1], Ee[sl]
        H, sg, szz = _stress_of(x, opt, A(U), A(G[sl]), Ec, v, dt)
        cv = [A(x["sbar"][k, sl].astype(dt)) if opt["sig"] else np.zeros((mc, B), dtype=dt) for k in range(len(nv))]
        if opt["vm"]:
            vbar = A(x["vbar"][sl].astype(dt))
            if ab:          # the magnitude of every component of vm_bar d vm / d sigma: 3 |vm_bar| A / vm
                _, sgr, szzr = _stress_of(x, opt, U_ld, G[sl].astype(LD), Ec.astype(LD), v, LD)
                vm = _von_mises(sgr, szzr, d)[0]
                total = sum(sg[a][t] for a, t in nv) + (szz if d == 2 else 0.0)
                cn = np.divide(3.0 * vbar * total, vm, out=np.zeros((mc, B), dtype=LD), where=vm > 0)
                cv = [c + cn + (dt(opt["nu_z"]) * cn if d == 2 and k < 2 else 0.0) for k, c in enumerate(cv)]
            else:
                vm, dev = _von_mises(sg, szz, d)
                w = np.divide(vbar, vm, out=np.zeros((mc, B), dtype=dt), where=vm > 0)
                for i in range(d):
                    cv[i] = cv[i] + 1.5 * dev[i] * w
                if d == 2:
                    cv[0] = cv[0] + dt(opt["nu_z"]) * (1.5 * dev[2] * w)
                    cv[1] = cv[1] + dt(opt["nu_z"]) * (1.5 * dev[2] * w)
                for k in range(d, len(nv)):
                    cv[k] = cv[k] + 3.0 * sg[nv[k][0]][nv[k][1]] * w
        trc = sum(cv[:d])
        P = _mat(d, lambda a, t: None)
        for k, (a, t) in enumerate(nv):
            if k < d:
                P[a][a] = Ec * (2.0 * dt(MU1) * cv[k] + dt(LAM1) * trc)
            else:
                P[a][t] = P[t][a] = Ec * (dt(MU1) * cv[k])
        N = _mat(d, lambda k, t: _bsum(sum(H[a][k] * P[a][t] for a in range(d))))
        W[sl] = _contract(x, N, A(G[sl]), LD(1.0) if ab else LD(-1.0))
    return W


def _von_mises(sg, szz, d):
    """vm and the deviator of the three normal stresses, vm^2 = 3/2 |dev|^2 + 3 sum shear^2."""
    nn = [sg[0][0], sg[1][1], szz]
    mean = (nn[0] + nn[1] + nn[2]) / 3.0
    dev = [c - mean for c in nn]
    shear = sum(sg[a][t] ** 2 for a, t in VOIGT[d][d:])
    return np.sqrt(1.5 * (dev[0] ** 2 + dev[1] ** 2 + dev[2] ** 2) + 3.0 * shear), dev


MODEL = {"p1": p1_model, "elast": elast_model, "stress": stress_model}


def model(x, opt, dt=np.float64, ab=False):
    return MODEL[x["entry"]](x, opt, dt, ab)


def node_sums(x, W):
    """(n, d) longdouble: the rows W (m, npe, d) summed over each node's incidence list."""
    out = np.zeros((x["n"], x["d"]), dtype=LD)
    np.add.at(out, x["elems"].T.reshape(-1).astype(np.int64), np.asarray(W, dtype=LD).reshape(-1, x["d"]))
    return out


def list_order_sums(x, work):
    """(n, d) float64: the returned rows added left to right in list order from 0.0 -- the gather's documented contract."""
    d, ptr, inc = x["d"], x["inc_ptr"].astype(np.int64), x["inc"].astype(np.int64)
    w = work.reshape(-1, d)
    ln = np.diff(ptr)
    s = np.zeros((x["n"], d))
    for j in range(int(ln.max())):
        sel = np.nonzero(ln > j)[0]
        s[sel] = s[sel] + w[inc[ptr[sel] + j]]
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pad(a, Bp, fill):
    out = np.full(a.shape[:-1] + (Bp,), fill, dtype=np.float64)
    out[..., :a.shape[-1]] = a
    return out


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _coef_dev(x, lay, fill):
    """The coefficient of layout lay on the device with its (per element, per sample) strides."""
    c, m, Bp = x["coef"], x["m"], x["Bp"]
    if lay == "s":
        return _t(np.array([c["s"]])), 0, 0
    if lay == "e":
        return _t(c["e"]), 1, 0
    if lay == "b":
        return _t(_pad(c["b"], Bp, fill)), 0, 1
    if lay == "eb":
        return _t(_pad(c["eb"], Bp, fill)), Bp, 1
    return _t(_pad(c["eb"], Bp, fill).T), 1, m           # "em": (Bp, m)


def _outputs(x):
    work = torch.full((x["m"], x["npe"] * x["d"]), float("nan"), dtype=T64, device=DEV)
    grad = torch.full((x["n"], x["d"]), float("nan"), dtype=T64, device=DEV)
    return work, grad


def _common_dev(x):
    return _t(x["elems"]), _t(x["inc_ptr"]), _t(x["inc"])


def run(x, opt, fill=float("nan"), major="node"):
    """One call of the case's entry -> (work (m, npe d), grad (n, d)) as numpy.  fill: what the padding holds; major: the
    scalar entry's node-major (n, Bp) or sample-major (B, n) fields."""
    L = _hip.lib()
    entry, d, n, m, B, Bp = x["entry"], x["d"], x["n"], x["m"], x["B"], x["Bp"]
    elems, inc_ptr, inc = _common_dev(x)
    work, grad = _outputs(x)
    assert x["inc_ptr"][-1] == len(x["inc"]) == m * x["npe"] and x["elems"].min() >= 0 and x["elems"].max() < n
    if entry == "p1":
        if major == "node":
            lay, sn, sb = (lambda a: _t(_pad(a, Bp, fill))), Bp, 1
        else:
            lay, sn, sb = (lambda a: _t(a.T)), 1, n
        kap, kse, ksb = _coef_dev(x, opt["kappa"], fill)
        f, fsn, fsb = None, 0, 0
        if opt["f"] == "sample":
            f, fsn, fsb = lay(x["f"]), sn, sb
        elif opt["f"] == "shared":
            f, fsn, fsb = _t(x["fshared"]), 1, 0
        L.diffhe_p1_shape_grad(_t(x["coords"]), elems, d, n, m, B, lay(x["u"]), _t(x["g"]) if opt["g"] else None,
                               lay(x["lam"]), sn, sb, kap, kse, ksb, f, fsn, fsb, float(opt["c"]), inc_ptr, inc, work, grad,
                               _stream())
    elif entry == "elast":
        E, ese, esb = _coef_dev(x, opt["E"], fill)
        L.diffhe_elast_shape_grad(elems, _t(x["gtab"]), _t(x["vol"]), d, LAM1, MU1, _t(_pad(x["u"], Bp, fill)),
                                  _t(x["g"]) if opt["g"] else None, _t(_pad(x["lam"], Bp, fill)),
                                  _t(_pad(x["f"], Bp, fill)) if opt["f"] else None, E, ese, esb, n, m, B, Bp, inc_ptr, inc,
                                  work, grad, _stream())
    else:
        nc = d * (d + 1) // 2
        E, ese, esb = _coef_dev(x, opt["E"], fill)
        sbar, osc, ose = None, 0, 0
        if opt["sig"]:
            sb_ = _pad(x["sbar"], Bp, fill)                                   # (nc, m, Bp)
            sbar, osc, ose = (_t(sb_), m * Bp, Bp) if opt["lay"] == "cm" else (_t(sb_.transpose(1, 0, 2)), Bp, nc * Bp)
        vbar = _t(_pad(x["vbar"], Bp, fill)) if opt["vm"] else None
        L.diffhe_stress_shape_grad(elems, _t(x["gtab"]), d, LAM1, MU1, float(opt["nu_z"]), _t(_pad(x["u"], Bp, fill)), E,
                                   ese, esb, sbar, osc, ose, vbar, n, m, B, Bp, inc_ptr, inc, work, grad, _stream())
    return work.cpu().numpy(), grad.cpu().numpy()


def _ratio(err, bound):
    """max err / bound; an entry with bound 0 must be met exactly."""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    assert (err[bound == 0] == 0).all(), "a value whose bound is 0 is not exactly 0"
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def compare(x, opt, work, grad, WS=None):
    """-> (largest error / bound of work, of grad) against the model (WS: its values and S, where the caller has them),
    after the finiteness and empty-list checks."""
    d, npe, m = x["d"], x["npe"], x["m"]
    assert np.isfinite(work).all() and np.isfinite(grad).all(), "NaN from the padding or the pre-fill"
    W, S = WS or (model(x, opt), model(x, opt, ab=True))
    c = c_elem(x, opt)
    rw = _ratio(np.abs(work.reshape(m, npe, d) - W), c * EPS * S)
    ln = np.diff(x["inc_ptr"].astype(np.int64))
    rg = _ratio(np.abs(grad - node_sums(x, W)), (c + ln)[:, None] * EPS * node_sums(x, S))
    assert (grad[ln == 0] == 0.0).all(), "a node with an empty list is not 0.0"
    return rw, rg


def bitwise_checks(x, opt, work, grad, major="node"):
    again = run(x, opt, major=major)
    assert np.array_equal(again[0], work) and np.array_equal(again[1], grad), "two runs differ"
    assert np.array_equal(list_order_sums(x, work), grad), "grad is not the list-order float64 sum of work"
    if major == "node":
        other = run(x, opt, fill=7.25, major=major)
        assert np.array_equal(other[0], work) and np.array_equal(other[1], grad), "the padding reaches the real samples"


def check_case(x, opts, label, majors=("node",)):
    """Every option of the case against the model; the bitwise checks on the last one.  Prints the largest ratios."""
    rw = rg = 0.0
    for opt in opts:
        got, WS = {}, (model(x, opt), model(x, opt, ab=True))
        for major in majors:
            got[major] = run(x, opt, major=major)
            a, b = compare(x, opt, *got[major], WS=WS)
            rw, rg = max(rw, a), max(rg, b)
        if len(majors) == 2:
            # two kernels' results, no model between them: each within chain + B roundings of the exact value
            between = (c_elem(x, opt) + x["B"]) * EPS * WS[1].reshape(x["m"], -1)
            assert _ratio(np.abs(got["node"][0] - got["sample"][0]), between) <= 1.0, f"{label}: node- and sample-major"
    for major in majors:
        bitwise_checks(x, opts[-1], *got[major], major=major)
    print(f"\nshape-kernels {label}: work {rw:.3f} grad {rg:.3f} of the bound")
    assert rw <= 1.0 and rg <= 1.0, f"{label}: error / bound = {rw:.3f} (work), {rg:.3f} (grad)"


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = [("p1", 1), ("p1", 2), ("p1", 3), ("elast", 2), ("elast", 3), ("stress", 2), ("stress", 3)]
ENTRY_IDS = [f"{e}{d}" for e, d in ENTRIES]
# (B, Bp): LB = 1, 2, 4, 8, 16, 32, 64, 64 with idle lanes wherever B < LB; then two and three ragged trips of b += LB
BATCHES = [(B, smallest_pad(B)) for B in (1, 2, 3, 5, 9, 17, 33, 64)] + [(70, 128), (129, 192)]
# (m, B, Bp): one element, and one element more than a block of 4 * (64 / LB) holds
SMALL = [(m, B, Bp) for B, Bp in BATCHES for m in (1, second_block(group_lanes(B)))]
# one element past the 8192-block cap: the second trip of e += stride at LB = 64 and at LB = 16
CAPS = [(8192 * 4 + 1, 64, 64), (8192 * 16 + 1, 9, 16)]
# sample-major scalar calls take LB = 1 whatever B: their second block, with a short and a long sample loop
SAMPLE_MAJOR = [(257, 3, 4), (257, 70, 128)]
GATHERS = ["cap2d", "cap3d", "long"]


def small_case(entry, d, m, B, Bp):
    return make_case(entry, d, m, B, Bp), options(entry, d), ("node", "sample") if entry == "p1" else ("node",)


def cap_case(entry, d, m, B, Bp):
    """Past the block cap the option matrix is one layout per entry (the richest), the shape is whole."""
    return make_case(entry, d, m, B, Bp), [full_option(entry, d)], ("node",)


def gather_case(entry, which):
    """The node pass: n * d > 8192 * 256 with almost every list empty (2D, 3D), and one list of 300 entries."""
    if which == "long":
        d, m, n = 2, 300, 40
        rng = np.random.default_rng(7)
        elems = 1 + (_distinct_elems(rng, n - 1, d + 1, m) if entry == "p1" else rng.integers(0, n - 1, size=(d + 1, m)))
        elems[0] = 0                                        # node 0 is vertex 0 of every element
    else:
        d, m, n = (2, 5, 1048600) if which == "cap2d" else (3, 5, 700000)
        elems = None
    x = make_case(entry, d, m, 3, 4, n=n, elems=elems)
    return x, [full_option(entry, d)], ("node", "sample") if entry == "p1" else ("node",)


def degenerate_case(entry, d):
    return make_case(entry, d, 45, 5, 8, ndeg=6)


def all_cases():
    """(label, builder) of every GPU case: what the float64-against-longdouble check of the model runs over."""
    out = []
    for (e, d), (m, B, Bp) in itertools.product(ENTRIES, SMALL):
        out.append((f"{e}{d}-m{m}-B{B}", lambda e=e, d=d, m=m, B=B, Bp=Bp: small_case(e, d, m, B, Bp)))
    for (e, d), (m, B, Bp) in itertools.product(ENTRIES, CAPS):
        out.append((f"{e}{d}-cap-m{m}-B{B}", lambda e=e, d=d, m=m, B=B, Bp=Bp: cap_case(e, d, m, B, Bp)))
    for d, (m, B, Bp) in itertools.product((1, 2, 3), SAMPLE_MAJOR):
        out.append((f"p1{d}-samplemajor-m{m}-B{B}", lambda d=d, m=m, B=B, Bp=Bp: small_case("p1", d, m, B, Bp)))
    for e, which in itertools.product(("p1", "elast"), GATHERS):
        out.append((f"{e}-gather-{which}", lambda e=e, which=which: gather_case(e, which)))
    for e, d in ENTRIES:
        out.append((f"{e}{d}-degenerate", lambda e=e, d=d: (degenerate_case(e, d), [full_option(e, d)], ("node",))))
    for d in (2, 3):
        out.append((f"stress{d}-vm0", lambda d=d: (make_case("stress", d, 45, 5, 8, nzero=6), [stress_full(d)], ("node",))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m,B,Bp", SMALL, ids=lambda v: str(v))
@pytest.mark.parametrize("entry,d", ENTRIES, ids=ENTRY_IDS)
def test_small_shapes(entry, d, m, B, Bp):
    x, opts, majors = small_case(entry, d, m, B, Bp)
    check_case(x, opts, f"{entry}{d} m={m} B={B} Bp={Bp}", majors)


@pytest.mark.gpu
@pytest.mark.parametrize("m,B,Bp", SAMPLE_MAJOR, ids=lambda v: str(v))
@pytest.mark.parametrize("d", [1, 2, 3])
def test_sample_major_second_block(d, m, B, Bp):
    x, opts, majors = small_case("p1", d, m, B, Bp)
    check_case(x, opts, f"p1{d} sample-major m={m} B={B}", majors)


@pytest.mark.gpu
@pytest.mark.parametrize("m,B,Bp", CAPS, ids=lambda v: str(v))
@pytest.mark.parametrize("entry,d", ENTRIES, ids=ENTRY_IDS)
def test_block_cap(entry, d, m, B, Bp):
    x, opts, majors = cap_case(entry, d, m, B, Bp)
    check_case(x, opts, f"{entry}{d} cap m={m} B={B} Bp={Bp}", majors)


@pytest.mark.gpu
@pytest.mark.parametrize("which", GATHERS)
@pytest.mark.parametrize("entry", ["p1", "elast"])
def test_gather(entry, which):
    x, opts, majors = gather_case(entry, which)
    ln = np.diff(x["inc_ptr"].astype(np.int64))
    assert ln.max() == 300 if which == "long" else (x["n"] * x["d"] > 8192 * 256 and (ln == 0).sum() >= x["n"] - 20)
    check_case(x, opts, f"{entry} gather {which} n={x['n']} d={x['d']}", majors)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,d", ENTRIES, ids=ENTRY_IDS)
def test_degenerate_elements(entry, d):
    """Rows of degenerate elements are 0.0 in magnitude, and nothing else depends on those elements' nodal data."""
    x = degenerate_case(entry, d)
    if entry == "p1":
        assert not p1_geometry(x)[2][x["deg"]].any() and p1_geometry(x)[2].sum() >= x["m"] - len(x["deg"]) - 2
    rw = rg = 0.0
    for opt in options(entry, d)[-4:] + [full_option(entry, d)]:
        for major in (("node", "sample") if entry == "p1" else ("node",)):
            work, grad = run(x, opt, major=major)
            a, b = compare(x, opt, work, grad)
            rw, rg = max(rw, a), max(rg, b)
            assert (work[x["deg"]] == 0.0).all()
            work2, grad2 = run(with_other_nodal_data(x, x["deg_nodes"]), opt, major=major)
            assert np.array_equal(work2, work) and np.array_equal(grad2, grad)
    print(f"\nshape-kernels {entry}{d} degenerate: work {rw:.3f} grad {rg:.3f} of the bound")
    assert rw <= 1.0 and rg <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("d", [2, 3])
def test_von_mises_zero(d):
    """u = 0 on some elements: vm = 0 exactly, the kernel defines d vm / d sigma = 0 there -- vm_bar adds exactly 0."""
    x = make_case("stress", d, 45, 5, 8, nzero=6)
    rw = rg = 0.0
    for nu_z in ((0.0, 0.3) if d == 2 else (0.0,)):
        got = {}
        for name, s, v in (("both", True, True), ("sig", True, False), ("vm", False, True)):
            opt = dict(E="eb", nu_z=nu_z, sig=s, vm=v, lay="cm")
            got[name] = run(x, opt)
            a, b = compare(x, opt, *got[name])
            rw, rg = max(rw, a), max(rg, b)
        assert (got["vm"][0][x["zero"]] == 0.0).all()
        assert np.array_equal(got["both"][0][x["zero"]], got["sig"][0][x["zero"]])
    print(f"\nshape-kernels stress{d} vm=0: work {rw:.3f} grad {rg:.3f} of the bound")
    assert rw <= 1.0 and rg <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# CPU self-checks of the model
# ---------------------------------------------------------------------------------------------------------------------
def _jittered_mesh(d):
    """Grid coordinates in units of 2^-8 with a jitter, and both orientations: 24 triangles or 48 tetrahedra."""
    rng = np.random.default_rng(d)
    if d == 2:
        nx, ny, h = 5, 4, 64
        idx = np.arange(nx * ny).reshape(nx, ny)
        units = np.stack(np.meshgrid(np.arange(nx) * h, np.arange(ny) * h, indexing="ij")).reshape(2, -1)
        a, b, c, e = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
        elems = np.concatenate([np.stack([a, b, c]), np.stack([a, e, c])], axis=1)
    else:
        k, h = 3, 128
        idx = np.arange(k ** 3).reshape(k, k, k)
        units = np.stack(np.meshgrid(*(np.arange(k) * h,) * 3, indexing="ij")).reshape(3, -1)
        tets = []
        for perm in itertools.permutations(range(3)):        # Kuhn: six tetrahedra per cube, alternating orientation
            corner = [np.zeros(3, dtype=int)]
            for ax in perm:
                corner.append(corner[-1] + np.eye(3, dtype=int)[ax])
            tets.append(np.stack([idx[c[0]:k - 1 + c[0], c[1]:k - 1 + c[1], c[2]:k - 1 + c[2]].ravel() for c in corner]))
        elems = np.concatenate(tets, axis=1)
    units = units + rng.integers(-h // 6, h // 6 + 1, size=units.shape)
    units -= units.min()
    return units / 256.0, elems


def _mesh_case(entry, d, B=3):
    coords, elems = _jittered_mesh(d)
    x = make_case(entry, d, elems.shape[1], B, smallest_pad(B), n=coords.shape[1], elems=elems)
    x["coords"] = coords
    if entry != "p1":
        G, size, ok = p1_geometry(x)
        assert ok.all()
        x["gtab"], x["vol"] = G.transpose(1, 2, 0).reshape((d + 1) * d, -1).copy(), size
    return x


def _torch_geometry(X, elems):
    """grad phi (m, npe, d) and sizes (m) as differentiable functions of the nodes X (n, d)."""
    P = X[torch.from_numpy(elems.astype(np.int64))].permute(1, 0, 2)               # (m, npe, d)
    Amat = torch.cat([torch.ones_like(P[..., :1]), P], dim=-1)                      # rows (1, x_p)
    G = torch.linalg.inv(Amat)[:, 1:, :].transpose(1, 2)                           # phi_p = coefficients of column p
    return G, torch.linalg.det(Amat).abs() / math.factorial(X.shape[1])


def _torch_unit_stress(H):
    tr = H.diagonal(dim1=-2, dim2=-1).sum(-1)
    return MU1 * (H + H.transpose(-1, -2)) + LAM1 * tr[..., None, None] * torch.eye(H.shape[-1], dtype=T64)


def _autograd_node_gradient(x, opt):
    """dL/dX (n, d) by torch.autograd through a dense restatement of the differentiated functional."""
    entry, d, npe = x["entry"], x["d"], x["npe"]
    X = torch.from_numpy(x["coords"].T.copy()).requires_grad_(True)
    G, vol = _torch_geometry(X, x["elems"])
    el = torch.from_numpy(x["elems"].astype(np.int64))
    t = torch.from_numpy
    coef = t(np.ascontiguousarray(coef_host(x, opt.get("kappa") or opt.get("E"))))   # (m, B)
    if entry == "p1":
        U = t(x["u"]) + (t(x["g"])[:, None] if opt["g"] else 0.0)
        Up, Lp = U[el], t(x["lam"])[el]                                             # (npe, m, B)
        gu, gl = torch.einsum("peb,epk->ebk", Up, G), torch.einsum("peb,epk->ebk", Lp, G)
        dens = coef * (gu * gl).sum(-1) + opt["c"] * (Lp * Up).sum(0) / npe
        if opt["f"]:
            Fp = (t(x["f"]) if opt["f"] == "sample" else t(x["fshared"])[:, None].expand(-1, x["B"]))[el]
            dens = dens - ((Lp * Fp).sum(0) / 2 if d == 1 else Lp.sum(0) * Fp.sum(0) / npe ** 2)
        sign, L = -1.0, (vol[:, None] * dens).sum()          # dL/dX = -d/dX lambda^T (K u - F + c M u)
    else:
        dof = el[:, None, :] * d + torch.arange(d)[None, :, None]
        U = t(x["u"]) + (t(x["g"])[:, None] if opt.get("g") else 0.0)
        Hu = torch.einsum("paeb,ept->ebat", U[dof], G)
        if entry == "elast":
            Lp = t(x["lam"])[dof]
            Hl = torch.einsum("paeb,ept->ebat", Lp, G)
            dens = coef * (_torch_unit_stress(Hu) * Hl).sum((-1, -2))
            if opt["f"]:
                dens = dens - (Lp.sum(0) * t(x["f"])[dof].sum(0)).sum(0) / npe ** 2
            sign, L = -1.0, (vol[:, None] * dens).sum()
        else:
            sg = coef[..., None, None] * _torch_unit_stress(Hu)
            L = torch.zeros((), dtype=T64)
            if opt["sig"]:
                L = L + sum((t(x["sbar"][k]) * sg[..., a, b]).sum() for k, (a, b) in enumerate(VOIGT[d]))
            if opt["vm"]:
                n0, n1 = sg[..., 0, 0], sg[..., 1, 1]
                n2 = opt["nu_z"] * (n0 + n1) if d == 2 else sg[..., 2, 2]
                shear = sum(sg[..., a, b] ** 2 for a, b in VOIGT[d][d:])
                vm = torch.sqrt(0.5 * ((n0 - n1) ** 2 + (n1 - n2) ** 2 + (n2 - n0) ** 2) + 3.0 * shear)
                L = L + (t(x["vbar"]) * vm).sum()
            sign = 1.0
    L.backward()
    return sign * X.grad.numpy()


@pytest.mark.parametrize("entry,d", ENTRIES[1:], ids=ENTRY_IDS[1:])
def test_model_matches_autograd(entry, d):
    """The model's dL/dX on a small jittered mesh against torch.autograd through the functional itself, u and lambda held
    fixed: both are float64 evaluations of one rational expression on well-shaped elements -- 1e-12 relative."""
    x = _mesh_case(entry, d)
    worst = 0.0
    for opt in options(entry, d):
        mine = node_sums(x, model(x, opt)).astype(np.float64)
        auto = _autograd_node_gradient(x, opt)
        worst = max(worst, np.abs(mine - auto).max() / np.abs(auto).max())
    print(f"\nshape-kernels model vs autograd {entry}{d}: {worst:.2e} relative")
    assert worst < 1e-12


ALL_CASES = all_cases()


@pytest.mark.parametrize("label,build", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_model_float64_against_longdouble(label, build):
    """On every GPU case's inputs the float64 model and an all-longdouble evaluation of it differ by less than the model's
    own share, c / 2 = chain, of the bound: the reference is not what the bound has to absorb.  Past the block cap every
    64th element (and the last) stands for the case: a row of work depends on no other element."""
    x, opts, _ = build()
    if x["m"] > 4096:
        x = subset(x, np.unique(np.concatenate([np.arange(0, x["m"], 64), [x["m"] - 1]])))
    worst = 0.0
    for opt in opts:
        W, S, Wl = model(x, opt), model(x, opt, ab=True), model(x, opt, dt=LD)
        worst = max(worst, _ratio(np.abs(W - Wl), chain(x["entry"], x["d"], opt.get("vm", True)) * EPS * S))
        ln = np.diff(incidence(x["elems"], x["n"])[0].astype(np.int64))
        assert _ratio(np.abs(node_sums(x, W) - node_sums(x, Wl)),
                      (chain(x["entry"], x["d"], opt.get("vm", True)) + ln)[:, None] * EPS * node_sums(x, S)) <= 1.0
    assert worst <= 1.0, f"{label}: the float64 model is {worst:.3f} of its share of the bound from longdouble"
