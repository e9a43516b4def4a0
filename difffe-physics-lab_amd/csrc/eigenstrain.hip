// Eigenstrain loads of a linear-elastic solve (ours: the reference has scalar unknowns only): the nodal load
// F0 = sum_e vol_e E_e B_e^T D eps0_e of an initial strain per element and sample -- thermal expansion, swelling,
// pre-stress -- and its adjoint with respect to eps0 and the Young's modulus E (definitions:
// include/diffhe_eigenstrain.h; the stress entries of that header are the eigen instantiations of stress.hip).
//
// Data layout as in elastic.hip and stress.hip: dof-major, batch innermost, lanes over samples (node_map), so node ids,
// gradients and list entries are wave-uniform and every access is one contiguous segment; Bp = 1 spreads rows over lanes.
// fp64, no atomics anywhere: every sum has a fixed order, results are bitwise reproducible.
//
// The load is a node pass over the per-node incidence list (shape.hip's) that recomputes the unit initial stress s0 of
// every incident (element, vertex): nc0 + 1 gathered doubles per incidence, where a stored s0 would cost an element pass
// writing and a node pass reading (nc, m, Bp).  The adjoint is an element pass on the loop of element_grad.h (NC = 1: dE)
// that writes d / d eps0 of the element as a side product, the form of the stress adjoint.
#include "common.h"
#include "diffhe_eigenstrain.h"
#include "eigen_field.h"
#include "element_grad.h"
#include "launch.h"

namespace {

using namespace diffhe;

// ---------------------------------------------------------------------------------------
// F0[(i, a), b] = sum over the incidence list of node i (codes e * NPE + p, element order) of
// vol_e E_e sum_t s0_e[a][t] g_p[t].  Samples b >= B: 0.
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void eigen_load_kernel(const int* __restrict__ inc_ptr, const int* __restrict__ inc,
                                                          const double* __restrict__ gtab,
                                                          const double* __restrict__ vol, const EigenField<DIM> ef,
                                                          const double* __restrict__ E, i64 ese, i64 esb, int n, int m,
                                                          int B, int Bp, double* __restrict__ F0) {
  constexpr int NPE = DIM + 1, NC = DIM * (DIM + 1) / 2;
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  for (int i = nm.node0; i < n; i += nm.stride) {
    double acc[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) acc[a] = 0.0;
    if (nm.b < B)
      for (int j = inc_ptr[i]; j < inc_ptr[i + 1]; ++j) {
        const int code = inc[j];
        const int e = code / NPE, p = code - e * NPE;
        double z[EigenField<DIM>::NZ], s0[NC], S[DIM][DIM];
        ef.read(e, nm.b, z);
        ef.initial_stress(z, s0);
        const double ve = vol[e] * E[(i64)e * ese + (i64)nm.b * esb];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          S[voigt_row<DIM>(k)][voigt_col<DIM>(k)] = s0[k];
          S[voigt_col<DIM>(k)][voigt_row<DIM>(k)] = s0[k];
        }
        double r[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) r[a] = 0.0;
#pragma unroll
        for (int t = 0; t < DIM; ++t) {
          const double g = gtab[(i64)(p * DIM + t) * m + e];
#pragma unroll
          for (int a = 0; a < DIM; ++a) r[a] = fma(S[a][t], g, r[a]);
        }
#pragma unroll
        for (int a = 0; a < DIM; ++a) acc[a] = fma(ve, r[a], acc[a]);
      }
#pragma unroll
    for (int a = 0; a < DIM; ++a) F0[((i64)i * DIM + a) * Bp + nm.b] = acc[a];
  }
}

// ---------------------------------------------------------------------------------------
// The adjoint as a form of element_grad.h: out[0] = dE[e, b] = vol s0 : sym(W), W[a][t] = sum_p w[(p, a)] g_p[t], and,
// where `deps` is given, vol E times the transposed unit-stress map of W to deps at c*osc + e*ose + b.
// Samples b >= B: dE = 0, d eps0 = 0, w not read.
// ---------------------------------------------------------------------------------------
template <int DIM>
struct EigenLoadAdjointForm {
  static constexpr int NC = 1;
  static constexpr int NPE = DIM + 1, NV = DIM * (DIM + 1) / 2, NZ = EigenField<DIM>::NZ;
  const int* __restrict__ elems;
  const double* __restrict__ gtab;
  const double* __restrict__ vol;
  EigenField<DIM> ef;
  const double* __restrict__ E;
  i64 ese, esb;
  const double* __restrict__ w;
  double* __restrict__ deps;
  i64 osc, ose;
  int m, B;

  struct Elem {
    int e;
    int node[NPE];
    double G[NPE][DIM];
    double ve;
    double z[NZ];     // the eigenstrain of the element where the batch shares it (zb == 0)
  };

  __device__ __forceinline__ void load(int e, Elem& el) const {
    el.e = e;
    el.ve = vol[e];
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
      el.node[p] = elems[(i64)p * m + e];
#pragma unroll
      for (int t = 0; t < DIM; ++t) el.G[p][t] = gtab[(i64)(p * DIM + t) * m + e];
    }
    if (ef.zb == 0) ef.read(e, 0, el.z);
  }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* out) const {
    const int nz = ef.count();
    if (b >= B) {
      out[0] = 0.0;
      if (deps)
        for (int k = 0; k < nz; ++k) deps[k * osc + el.e * ose + b] = 0.0;
      return;
    }
    double W[DIM][DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = 0; t < DIM; ++t) W[a][t] = 0.0;
#pragma unroll
    for (int p = 0; p < NPE; ++p)
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const double wp = w[((i64)el.node[p] * DIM + a) * Bp + b];
#pragma unroll
        for (int t = 0; t < DIM; ++t) W[a][t] = fma(wp, el.G[p][t], W[a][t]);
      }
    double c[NV];       // the cotangent of the unit initial stress: a shear one with respect to that one number
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int a = voigt_row<DIM>(k), t = voigt_col<DIM>(k);
      c[k] = k < DIM ? W[a][a] : W[a][t] + W[t][a];
    }
    double z[NZ], s0[NV];
    if (ef.zb) {
      ef.read(el.e, b, z);
    } else {
#pragma unroll
      for (int k = 0; k < NZ; ++k) z[k] = el.z[k];
    }
    ef.initial_stress(z, s0);
    double de = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) de = fma(s0[k], c[k], de);
    out[0] = el.ve * de;
    if (deps) {
      double dz[NZ];
      ef.transpose(el.ve * E[(i64)el.e * ese + (i64)b * esb], c, 0.0, dz);
#pragma unroll
      for (int k = 0; k < NZ; ++k)
        if (k < nz) deps[k * osc + el.e * ose + b] = dz[k];
    }
  }
};

template <int DIM>
EigenField<DIM> field_of(const double* eps0, i64 zc, i64 ze, i64 zb, double lam1, double mu1, int plane_strain) {
  return EigenField<DIM>{eps0, zc, ze, zb, lam1, mu1, DIM == 2 && plane_strain ? 1 : 0};
}

template <int DIM>
EigenLoadAdjointForm<DIM> adjoint_form(const int* elems, const double* gtab, const double* vol, double lam1, double mu1,
                                       int plane_strain, const double* E, i64 e_se, i64 e_sb, const double* eps0, i64 zc,
                                       i64 ze, i64 zb, const double* w, double* deps, i64 osc, i64 ose, int m, int B) {
  return EigenLoadAdjointForm<DIM>{elems, gtab, vol, field_of<DIM>(eps0, zc, ze, zb, lam1, mu1, plane_strain), E, e_se, e_sb,
                                   w,     deps, osc, ose, m, B};
}

// what every entry refuses: pointers, dim, sizes, the strides, the int32 codes e * npe + p
bool bad_common(const double* gtab, const double* vol, int dim, const double* E, i64 e_se, i64 e_sb, const double* eps0,
                i64 zc, i64 ze, i64 zb, int n, int m, int B, int Bp) {
  return !gtab || !vol || !E || (dim != 2 && dim != 3) || n < 1 || m < 1 || e_se < 0 || e_sb < 0 ||
         bad_eigen(eps0, zc, ze, zb) || B < 1 || B > Bp || (i64)m * (dim + 1) >= (1LL << 31);
}

int components(int dim, int plane_strain) { return dim == 3 ? 6 : (plane_strain ? 4 : 3); }

double modulus_bytes(i64 e_se, i64 e_sb, int m, int Bp) { return 8.0 * (e_se ? (double)m : 1.0) * (e_sb ? (double)Bp : 1.0); }

}  // namespace

// =========================================================================================
// C ABI (include/diffhe_eigenstrain.h)
// =========================================================================================
extern "C" int diffhe_eigenstrain_load(const int* inc_ptr, const int* inc, const double* gtab, const double* vol, int dim,
                                       double lam1, double mu1, int plane_strain, const double* E, long long e_se,
                                       long long e_sb, const double* eps0, long long zc, long long ze, long long zb, int n,
                                       int m, int B, int Bp, double* F0, void* stream) {
  if (bad_common(gtab, vol, dim, E, e_se, e_sb, eps0, zc, ze, zb, n, m, B, Bp) || !inc_ptr || !inc || !F0)
    return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  // eps0 and E once, F0 once per dof
  diffhe::account(8.0 * Bp * (double)dim * n + eigen_bytes(components(dim, plane_strain), ze, zb, m, Bp) +
                  modulus_bytes(e_se, e_sb, m, Bp));
  const dim3 grid = diffhe::node_grid(n, Bp);
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(eigen_load_kernel<D()>, grid, dim3(256), 0, (hipStream_t)stream, inc_ptr, inc, gtab, vol,
                       field_of<D()>(eps0, zc, ze, zb, lam1, mu1, plane_strain), E, e_se, e_sb, n, m, B, Bp, F0);
  });
  return diffhe::check_launch();
}

extern "C" int diffhe_eigenstrain_load_adjoint(const int* elems, const double* gtab, const double* vol, int dim,
                                               double lam1, double mu1, int plane_strain, const double* E, long long e_se,
                                               long long e_sb, const double* eps0, long long zc, long long ze,
                                               long long zb, const double* w, int n, int m, int B, int Bp, double* deps,
                                               long long osc, long long ose, double* de_e, double* de_part,
                                               double* de_sum, void* stream) {
  if (bad_common(gtab, vol, dim, E, e_se, e_sb, eps0, zc, ze, zb, n, m, B, Bp) || !elems || !w ||
      (deps && (osc < 1 || ose < 1)))
    return DIFFHE_E_BADARG;
  if ((de_part == nullptr) != (de_sum == nullptr) || (!deps && !de_e && !de_part)) return DIFFHE_E_BADARG;
  const int nc0 = components(dim, plane_strain);
  // w once per dof, eps0, d eps0 (which reads E) and dE per element
  const double bytes = 8.0 * Bp * ((double)dim * n + (deps ? (double)nc0 * m : 0.0) + (de_e ? (double)m : 0.0)) +
                       eigen_bytes(nc0, ze, zb, m, Bp) + (deps ? modulus_bytes(e_se, e_sb, m, Bp) : 0.0);
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return diffhe::launch_element_grad(adjoint_form<D()>(elems, gtab, vol, lam1, mu1, plane_strain, E, e_se, e_sb, eps0,
                                                         zc, ze, zb, w, deps, osc, ose, m, B),
                                       m, Bp, de_e, 0, Bp, de_part, de_sum, bytes, stream);
  });
}

extern "C" int diffhe_eigenstrain_load_adjoint_shared(const int* elems, const double* gtab, const double* vol, int dim,
                                                      double lam1, double mu1, int plane_strain, const double* E,
                                                      long long e_se, long long e_sb, const double* eps0, long long zc,
                                                      long long ze, long long zb, const double* w, int n, int m, int B,
                                                      int Bp, double* de, void* stream) {
  if (bad_common(gtab, vol, dim, E, e_se, e_sb, eps0, zc, ze, zb, n, m, B, Bp) || !elems || !w || !de)
    return DIFFHE_E_BADARG;
  // w once per dof, eps0, dE per element; E is not read: dE = vol s0 : sym(W)
  const double bytes = 8.0 * (Bp * (double)dim * n + (double)m) + eigen_bytes(components(dim, plane_strain), ze, zb, m, Bp);
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return diffhe::launch_element_grad_shared(adjoint_form<D()>(elems, gtab, vol, lam1, mu1, plane_strain, E, e_se, e_sb,
                                                                eps0, zc, ze, zb, w, nullptr, 0, 0, m, B),
                                              m, B, Bp, de, 0, 1, bytes, stream);
  });
}
