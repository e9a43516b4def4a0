"""The element-gradient kernels through their three ABI pairs: diffhe_p1_grad_kappa(_shared) (npe 3 / 4 / 6),
diffhe_aniso_grad(_shared) (2D / 3D) and diffhe_elast_grad(_shared) (2D / 3D) -- the skeleton of csrc/element_grad.h with
AnisoForm and KappaForm, and the kernels of the same shape that ell_assemble.hip and elastic.hip keep -- called directly on
seeded synthetic inputs: random element lists into n nodes, random tables and nodal fields; no mesh, no solve; at the
smallest shapes at which that loop can go wrong.

The reference is a numpy evaluation of the same formulas, values in float64 and sums in longdouble:

  kappa    dk[e, b]    = -lam_e^T k0_e (u_e + g_e)
  tensor   dK_c[e, b]  = -|e| sym_c(grad lam (x) grad u),    grad v = sum_p v_p g_p
  E        dE[e, b]    = -|e| [lam1 tr(Hl) tr(Hu) + mu1 Hl : (Hu + Hu^T)],   H[a][t] = sum_p v[(p, a)] g_p[t]

Tolerances are derived, c * 2^-53 * S: S is the same expression evaluated on absolute values and c the number of
roundings on the longest chain from an input to the result, counted for the kernel AND for the float64 reference (each
errs by at most its own chain, so the two differ by at most the sum; a fused multiply-add only shortens a chain).
With NPE = d + 1 nodes per element and one rounding for u + g:

  kappa    per value: the npe^2 terms le k0 ue take 2 products each on top of u + g, and npe^2 additions join them:
           chain = npe^2 + 3.
  tensor   grad lam takes NPE roundings, grad u NPE + 1; a product of the two, the second product and the addition of an
           off-diagonal component, the factor |e|: chain = 2 NPE + 5.
  E        Hl NPE, Hu NPE + 1; the longer branch is mu1 Hl : (Hu + Hu^T): Hu + Hu^T, the product, d^2 additions, then
           mu1, the addition of the lam1 branch and |e|: chain = 2 NPE + d^2 + 6  (the lam1 branch, 2 NPE + 2 d + 3,
           is shorter for d = 2 and d = 3).

  c_value = 2 chain (kernel + reference).  A total over the m elements per sample adds at most m roundings whatever the
  order of the sum (the longdouble reference adds none): c_total = 2 chain + m, S summed over the elements.  A sum over
  the B samples of the batch: c_batch = 2 chain + B, S summed over the samples.

Padding samples (b >= B) hold NaN in lam: nothing the assertions read may depend on them."""
import numpy as np
import pytest
import torch

from diffhe import _hip

T64 = torch.float64
DEV = "cuda:0"
EPS = 2.0 ** -53

# (name, ABI pair, nodes per element, dimension)
FAMILIES = [("kappa3", "kappa", 3, 0), ("kappa4", "kappa", 4, 0), ("kappa6", "kappa", 6, 0),
            ("tensor2", "tensor", 3, 2), ("tensor3", "tensor", 4, 3), ("E2", "E", 3, 2), ("E3", "E", 4, 3)]


def _second_block(Bp):
    """One element more than the first block holds: 4 waves of 64 / min(Bp, 64) elements."""
    return 4 * (64 // min(Bp, 64)) + 1


# per-sample kernel, (m, B, Bp): lane folding below 64 and two sample chunks at 128; a block with idle waves and a second
# block holding one element; m = 8200 at Bp = 64 is past the 2048-block cap (a second trip of the grid-stride loop)
SAMPLE_SHAPES = [(m, max(1, Bp - 1), Bp) for Bp in (1, 4, 64, 128) for m in (1, _second_block(Bp))] + [(8200, 63, 64)]
# batch-shared kernel, (m, B, Bp): padding samples excluded, a second trip of the lane loop at B = 70; m = 65541 is past
# the 16384-block cap
SHARED_SHAPES = [(5, 1, 1), (5, 3, 4), (5, 70, 128), (65541, 3, 4)]


def chain(kind, npe, d):
    return {"kappa": npe * npe + 3, "tensor": 2 * npe + 5, "E": 2 * npe + d * d + 6}[kind]


def make_inputs(kind, npe, d, m, B, Bp, seed=0):
    """Seeded host arrays of one case: elems (npe, m) into n nodes, the family's tables, lam / u (dofs, Bp), g (dofs)."""
    rng = np.random.default_rng([seed, npe, d, m, Bp])
    n = min(max(npe + 2, m // 2), 4099)
    dofs = n * (d if kind == "E" else 1)
    x = {"n": n, "m": m, "B": B, "Bp": Bp, "npe": npe, "d": d, "kind": kind,
         "elems": rng.integers(0, n, size=(npe, m)).astype(np.int32),
         "lam": rng.standard_normal((dofs, Bp)), "u": rng.standard_normal((dofs, Bp)), "g": rng.standard_normal(dofs)}
    x["lam"][:, B:] = np.nan
    if kind == "kappa":
        x["k0"] = rng.standard_normal((npe * npe, m))
    else:
        x["gtab"] = rng.standard_normal((npe * d, m))
        x["vol"] = rng.random(m) + 0.5
    if kind == "E":
        x["lam1"], x["mu1"] = 0.5769230769230769, 0.3846153846153846      # nu = 0.3
    return x


def reference(x):
    """-> (values (NC, m, B) float64, S of the values (NC, m, B)) by the formulas of the module docstring."""
    kind, npe, d, m, B = x["kind"], x["npe"], x["d"], x["m"], x["B"]
    el = x["elems"]

    def both(f):      # the expression and the same on absolute values
        return f(lambda a: a, -1.0), f(np.abs, 1.0)

    if kind == "kappa":
        def f(A, sign):
            le = [A(x["lam"][el[p], :B]) for p in range(npe)]
            ue = [A(x["u"][el[p], :B]) + A(x["g"][el[p]])[:, None] for p in range(npe)]
            acc = np.zeros((m, B))
            for p in range(npe):
                for q in range(npe):
                    acc += le[p] * A(x["k0"][p * npe + q])[:, None] * ue[q]
            return (sign * acc)[None]
        return both(f)
    G = x["gtab"].reshape(npe, d, m)
    if kind == "tensor":
        def f(A, sign):
            gl = [sum(A(x["lam"][el[p], :B]) * A(G[p, t])[:, None] for p in range(npe)) for t in range(d)]
            gu = [sum((A(x["u"][el[p], :B]) + A(x["g"][el[p]])[:, None]) * A(G[p, t])[:, None] for p in range(npe))
                  for t in range(d)]
            pairs = [(0, 0), (1, 1), (0, 1)] if d == 2 else [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
            w = [gl[i] * gu[i] if i == j else gl[i] * gu[j] + gl[j] * gu[i] for i, j in pairs]
            return sign * x["vol"][None, :, None] * np.stack(w)
        return both(f)

    def f(A, sign):
        def H(v, with_g):
            out = [[0.0] * d for _ in range(d)]
            for a in range(d):
                for p in range(npe):
                    vp = A(v[el[p] * d + a, :B])
                    if with_g:
                        vp = vp + A(x["g"][el[p] * d + a])[:, None]
                    for t in range(d):
                        out[a][t] = out[a][t] + vp * A(G[p, t])[:, None]
            return out
        Hl, Hu = H(x["lam"], False), H(x["u"], True)
        trl, tru = sum(Hl[a][a] for a in range(d)), sum(Hu[a][a] for a in range(d))
        ee = sum(Hl[a][t] * (Hu[a][t] + Hu[t][a]) for a in range(d) for t in range(d))
        return (sign * x["vol"][:, None] * (x["lam1"] * (trl * tru) + x["mu1"] * ee))[None]
    return both(f)


def _dev(x):
    return {k: torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v for k, v in x.items()}


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def run_sample(L, X, want_e, want_sum, em=True):
    """The per-sample entry of the family -> (dk_e as (NC, m, Bp) or None, dk_sum (NC, Bp) or None).  em: the tensor's
    (nc, m, Bp) layout, else its (m, nc, Bp) one (returned transposed to the former)."""
    kind, m, Bp, n, d = X["kind"], X["m"], X["Bp"], X["n"], X["d"]
    nc = {"kappa": 1, "E": 1, "tensor": d * (d + 1) // 2}[kind]
    new = lambda *s: torch.full(s, float("nan"), dtype=T64, device=DEV)  # noqa: E731
    dk_e = (new(nc, m, Bp) if em else new(m, nc, Bp)) if want_e else None
    part = new(L.diffhe_grad_kappa_blocks(m, Bp), nc, Bp) if want_sum else None
    dk_sum = new(nc, Bp) if want_sum else None
    if kind == "kappa":
        L.diffhe_p1_grad_kappa(X["elems"], X["k0"], X["lam"], X["u"], X["g"], X["npe"], m, Bp, dk_e, part, dk_sum, _stream())
    elif kind == "tensor":
        osc, ose = (m * Bp, Bp) if em else (Bp, nc * Bp)
        L.diffhe_aniso_grad(X["elems"], X["gtab"], X["vol"], d, X["lam"], X["u"], X["g"], n, m, Bp, dk_e, osc, ose, part,
                            dk_sum, _stream())
    else:
        L.diffhe_elast_grad(X["elems"], X["gtab"], X["vol"], d, X["lam1"], X["mu1"], X["lam"], X["u"], X["g"], n, m, Bp,
                            dk_e, part, dk_sum, _stream())
    if want_e and not em:
        dk_e = dk_e.permute(1, 0, 2).contiguous()
    return dk_e, dk_sum


def run_shared(L, X, em=True):
    """The batch-shared entry of the family -> dk (NC, m).  em: the tensor's (nc, m) layout, else (m, nc)."""
    kind, m, B, Bp, n, d = X["kind"], X["m"], X["B"], X["Bp"], X["n"], X["d"]
    nc = {"kappa": 1, "E": 1, "tensor": d * (d + 1) // 2}[kind]
    dk = torch.full((nc, m) if em else (m, nc), float("nan"), dtype=T64, device=DEV)
    if kind == "kappa":
        L.diffhe_p1_grad_kappa_shared(X["elems"], X["k0"], X["lam"], X["u"], X["g"], X["npe"], m, B, Bp, dk, _stream())
    elif kind == "tensor":
        osc, ose = (m, 1) if em else (1, nc)
        L.diffhe_aniso_grad_shared(X["elems"], X["gtab"], X["vol"], d, X["lam"], X["u"], X["g"], n, m, B, Bp, dk, osc, ose,
                                   _stream())
    else:
        L.diffhe_elast_grad_shared(X["elems"], X["gtab"], X["vol"], d, X["lam1"], X["mu1"], X["lam"], X["u"], X["g"], n, m,
                                   B, Bp, dk, _stream())
    return dk if em else dk.t().contiguous()


def _close(got, ref, S, c, what):
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), what
    excess = np.abs(got - np.asarray(ref, dtype=np.longdouble)) - c * EPS * np.asarray(S, dtype=np.longdouble)
    assert (excess <= 0).all(), f"{what}: {excess.max():.3e} over c * 2^-53 * S, c = {c}"


@pytest.mark.gpu
@pytest.mark.parametrize("m,B,Bp", SAMPLE_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("name,kind,npe,d", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_per_sample(name, kind, npe, d, m, B, Bp):
    L = _hip.lib()
    x = make_inputs(kind, npe, d, m, B, Bp)
    X = _dev(x)
    ref, S = reference(x)
    c = 2 * chain(kind, npe, d)
    dk_e, dk_sum = run_sample(L, X, True, True)
    _close(dk_e[:, :, :B], ref, S, c, "per-element values")
    _close(dk_sum[:, :B], ref.astype(np.longdouble).sum(axis=1), S.astype(np.longdouble).sum(axis=1), c + m,
           "per-sample totals")
    # bitwise by construction: the values do not depend on what else is asked for, on the output strides, or on the run
    again_e, again_sum = run_sample(L, X, True, True)
    assert torch.equal(again_e[:, :, :B], dk_e[:, :, :B]) and torch.equal(again_sum[:, :B], dk_sum[:, :B])
    only_sum = run_sample(L, X, False, True)[1]
    assert torch.equal(only_sum[:, :B], dk_sum[:, :B])
    if kind != "kappa":       # the scalar entry always leaves the totals
        only_e = run_sample(L, X, True, False)[0]
        assert torch.equal(only_e[:, :, :B], dk_e[:, :, :B])
    if kind == "tensor":
        other_e, other_sum = run_sample(L, X, True, True, em=False)
        assert torch.equal(other_e[:, :, :B], dk_e[:, :, :B]) and torch.equal(other_sum[:, :B], dk_sum[:, :B])


@pytest.mark.gpu
@pytest.mark.parametrize("m,B,Bp", SHARED_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("name,kind,npe,d", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_batch_shared(name, kind, npe, d, m, B, Bp):
    L = _hip.lib()
    x = make_inputs(kind, npe, d, m, B, Bp)
    X = _dev(x)
    ref, S = reference(x)
    dk = run_shared(L, X)
    _close(dk, ref.astype(np.longdouble).sum(axis=2), S.astype(np.longdouble).sum(axis=2), 2 * chain(kind, npe, d) + B,
           "batch sums")
    assert torch.equal(run_shared(L, X), dk)
    if kind == "tensor":
        assert torch.equal(run_shared(L, X, em=False), dk)
