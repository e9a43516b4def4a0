// Stress recovery of a finite-strain Neo-Hookean solve (ours: the reference has linear scalar equations only): the Cauchy
// stress sigma = E (1/J) [mu1 (H + H^T + H H^T) + lam1 ln J I] in Voigt components, its von Mises stress, the strain-energy
// density w = E W1(F), and their adjoint with respect to the displacement u and the Young's modulus E (definitions:
// include/diffhe_hyper_stress.h).  u is the full displacement, so no Dirichlet data is read; gtab is the ORIENTED gradient
// table of hyperelastic.hip, and the deformation of an element (H, J, ln J, F^-T, P1, W1) is that unit's, deformation.h.
//
// Data layout as in hyperelastic.hip: dof-major, batch innermost, lanes over samples (node_map) ALWAYS, so element data --
// node ids, gradients, list entries -- is wave-uniform and every access is one contiguous segment.  fp64, no atomics
// anywhere: every sum has a fixed order, results are bitwise reproducible.
//
// The adjoint is the element pass and the node pass of stress.hip.  The element pass runs on the element loop of
// element_grad.h with the form below (NC = 1: dE) and writes T = dL/dH of the element as a side product; T is a full d x d
// tensor here (the Cauchy stress is not linear in H), so the node pass is this unit's own: stress.hip's reads a symmetric
// tensor of nc components.  An element with J <= 0 has ln J = NaN, which reaches every number of its own (e, b) and no other.
#include "common.h"
#include "deformation.h"
#include "diffhe_hyper_stress.h"
#include "element_grad.h"
#include "stress_form.h"
#include "launch.h"

namespace {

using namespace diffhe;

// What both directions read of an element and a sample.
template <int DIM>
struct CauchyElement {
  static constexpr int NPE = DIM + 1, NV = DIM * (DIM + 1) / 2;
  const int* __restrict__ elems;
  const double* __restrict__ gtab;
  double lam1, mu1;
  const double* __restrict__ u;
  const double* __restrict__ E;
  i64 ese, esb;
  int m;

  struct Elem {
    int e;
    int node[NPE];
    double G[NPE][DIM];
  };

  __device__ __forceinline__ void load(int e, Elem& el) const {
    el.e = e;
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
      el.node[p] = elems[(i64)p * m + e];
#pragma unroll
      for (int t = 0; t < DIM; ++t) el.G[p][t] = gtab[(i64)(p * DIM + t) * m + e];
    }
  }

  __device__ __forceinline__ double modulus(int e, int b) const { return E[(i64)e * ese + (i64)b * esb]; }

  // 1 / J, and NaN for J <= 0 (ln J is NaN there): every component of the stress carries it
  __device__ __forceinline__ double inverse_volume(const Deformation<DIM>& D) const { return 1.0 / D.J + 0.0 * D.lnJ; }

  // the unit Cauchy stress s (NV) with b - I = H + H^T + H H^T; returns the out-of-plane s_zz of plane strain (3D: 0)
  __device__ __forceinline__ double unit_stress(const Deformation<DIM>& D, double r, double* s) const {
    const double c = lam1 * D.lnJ;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int a = voigt_row<DIM>(k), t = voigt_col<DIM>(k);
      double bb = D.H[a][t] + D.H[t][a];
#pragma unroll
      for (int q = 0; q < DIM; ++q) bb = fma(D.H[a][q], D.H[t][q], bb);
      s[k] = r * (k < DIM ? fma(mu1, bb, c) : mu1 * bb);
    }
    return DIM == 2 ? r * c : 0.0;
  }
};

// The three normal stresses of sigma (NV): in 2D the third is sigma_zz.
template <int DIM>
__device__ __forceinline__ void cauchy_normal_stresses(const double* sg, double sg_zz, double* nn) {
  nn[0] = sg[0];
  nn[1] = sg[1];
  nn[2] = DIM == 2 ? sg_zz : sg[2];
}

// ---------------------------------------------------------------------------------------
// sigma at c*osc + e*ose + b and / or vm (m, Bp) and / or w (m, Bp); a NULL output is neither computed nor stored.
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void hyper_stress_eval_kernel(const CauchyElement<DIM> el_of, int Bp,
                                                                 double* __restrict__ sigma, i64 osc, i64 ose,
                                                                 double* __restrict__ vm, double* __restrict__ w) {
  constexpr int NV = DIM * (DIM + 1) / 2;
  const NodeMap nm = node_map(Bp);  // "nodes" are elements here
  if (nm.b >= Bp) return;
  for (int e = nm.node0; e < el_of.m; e += nm.stride) {
    typename CauchyElement<DIM>::Elem el;
    el_of.load(e, el);
    Deformation<DIM> D;
    D.from(el.node, el.G, el_of.u, Bp, nm.b);
    const double Ee = el_of.modulus(e, nm.b);
    if (sigma || vm) {
      double sg[NV];
      const double szz = el_of.unit_stress(D, el_of.inverse_volume(D), sg);
#pragma unroll
      for (int k = 0; k < NV; ++k) sg[k] *= Ee;
      if (sigma) {
#pragma unroll
        for (int k = 0; k < NV; ++k) sigma[k * osc + e * ose + nm.b] = sg[k];
      }
      if (vm) {
        double nn[3];
        cauchy_normal_stresses<DIM>(sg, Ee * szz, nn);
        vm[(i64)e * Bp + nm.b] = von_mises<DIM>(sg, nn);
      }
    }
    if (w) w[(i64)e * Bp + nm.b] = Ee * D.energy(el_of.lam1, el_of.mu1);   // NaN for J <= 0 through ln J
  }
}

// ---------------------------------------------------------------------------------------
// The element pass of the adjoint as a form of element_grad.h: out[0] = dE[e, b] = C:s + w_bar W1 and, where `work` is
// given (NODES), T = dL/dH to work (d*d, m, Bp) (include/diffhe_hyper_stress.h).  Samples b >= B: dE = 0, T = 0, no cotangent
// read.  NODES is a template argument so that the passes without a node pass -- dE alone, and the batch-summing kernel --
// carry neither F^-T nor P1 nor T.
// ---------------------------------------------------------------------------------------
template <int DIM, bool NODES>
struct CauchyAdjointForm {
  static constexpr int NC = 1;
  static constexpr int NV = DIM * (DIM + 1) / 2;
  typedef typename CauchyElement<DIM>::Elem Elem;
  CauchyElement<DIM> el_of;
  const double* __restrict__ sigma_bar;
  i64 osc, ose;
  const double* __restrict__ vm_bar;
  const double* __restrict__ w_bar;
  double* __restrict__ work;
  int B;

  __device__ __forceinline__ void load(int e, Elem& el) const { el_of.load(e, el); }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* out) const {
    const i64 mb = (i64)el_of.m * Bp, at = (i64)el.e * Bp + b;
    if (b >= B) {
      out[0] = 0.0;
      if constexpr (NODES) {
#pragma unroll
        for (int k = 0; k < DIM * DIM; ++k) work[k * mb + at] = 0.0;
      }
      return;
    }
    const double lam1 = el_of.lam1, mu1 = el_of.mu1;
    Deformation<DIM> D;
    D.from(el.node, el.G, el_of.u, Bp, b);
    const double Ee = el_of.modulus(el.e, b);
    double de = 0.0, T[DIM][DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = 0; t < DIM; ++t) T[a][t] = 0.0;

    if (sigma_bar || vm_bar) {
      // the combined cotangent c (NV) of sigma and c_zz of sigma_zz
      double s[NV], c[NV], czz = 0.0;
      const double r = el_of.inverse_volume(D);
      const double szz = el_of.unit_stress(D, r, s);
#pragma unroll
      for (int k = 0; k < NV; ++k) c[k] = sigma_bar ? sigma_bar[k * osc + el.e * ose + b] : 0.0;
      if (vm_bar) {
        double sg[NV], nn[3];
#pragma unroll
        for (int k = 0; k < NV; ++k) sg[k] = Ee * s[k];
        cauchy_normal_stresses<DIM>(sg, Ee * szz, nn);
        const double vm = von_mises<DIM>(sg, nn);
        if (vm > 0.0) {                                   // d vm / d sigma = 0 where vm == 0
          const double wv = vm_bar[at] / vm;
          const double mean = ((nn[0] + nn[1]) + nn[2]) / 3.0;
          double cn[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) cn[i] = 1.5 * (nn[i] - mean) * wv;
#pragma unroll
          for (int i = 0; i < DIM; ++i) c[i] += cn[i];
          if (DIM == 2) czz = cn[2];
#pragma unroll
          for (int k = DIM; k < NV; ++k) c[k] = fma(3.0 * sg[k], wv, c[k]);
        }
      }
      // C:s and tr3 C; a shear cotangent stands for both entries of C, each c / 2
      double cs = czz * szz, tr3 = czz;
#pragma unroll
      for (int k = 0; k < NV; ++k) cs = fma(c[k], s[k], cs);
#pragma unroll
      for (int i = 0; i < DIM; ++i) tr3 += c[i];
      de = cs;
      if constexpr (NODES) {
        double Cm[DIM][DIM];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const int a = voigt_row<DIM>(k), t = voigt_col<DIM>(k);
          Cm[a][t] = Cm[t][a] = k < DIM ? c[k] : 0.5 * c[k];
        }
        const double k1 = 2.0 * mu1 * r, k2 = fma(lam1 * tr3, r, -cs);
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
          for (int t = 0; t < DIM; ++t) {
            double cf = Cm[a][t];                         // (C F)[a][t], F = I + H
#pragma unroll
            for (int q = 0; q < DIM; ++q) cf = fma(Cm[a][q], D.H[q][t], cf);
            T[a][t] = Ee * fma(k1, cf, k2 * D.Fit[a][t]);
          }
      }
    }
    if (w_bar) {
      const double wb = w_bar[at];
      de = fma(wb, D.energy(lam1, mu1), de);
      if constexpr (NODES) {
        double P[DIM][DIM];
        D.piola(lam1, mu1, P);
        const double we = wb * Ee;
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
          for (int t = 0; t < DIM; ++t) T[a][t] = fma(we, P[a][t], T[a][t]);
      }
    }
    out[0] = de;
    if constexpr (NODES) {
#pragma unroll
      for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int t = 0; t < DIM; ++t) work[(a * DIM + t) * mb + at] = T[a][t];
    }
  }
};

// ---------------------------------------------------------------------------------------
// Node pass: u_bar[(i, a), b] = sum over the incidence list of node i (codes e * NPE + p, element order) of
// sum_t T_e[a][t] g_p[t], T (d*d, m, Bp) row-major.  Samples b >= B: 0.
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void hyper_stress_node_kernel(const int* __restrict__ inc_ptr,
                                                                 const int* __restrict__ inc,
                                                                 const double* __restrict__ gtab,
                                                                 const double* __restrict__ work, int n, int m, int B,
                                                                 int Bp, double* __restrict__ u_bar) {
  constexpr int NPE = DIM + 1;
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  const i64 mb = (i64)m * Bp;
  for (int i = nm.node0; i < n; i += nm.stride) {
    double acc[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) acc[a] = 0.0;
    if (nm.b < B)
      for (int j = inc_ptr[i]; j < inc_ptr[i + 1]; ++j) {
        const int code = inc[j];
        const int e = code / NPE, p = code - e * NPE;
#pragma unroll
        for (int t = 0; t < DIM; ++t) {
          const double g = gtab[(i64)(p * DIM + t) * m + e];
#pragma unroll
          for (int a = 0; a < DIM; ++a) acc[a] = fma(work[(a * DIM + t) * mb + (i64)e * Bp + nm.b], g, acc[a]);
        }
      }
#pragma unroll
    for (int a = 0; a < DIM; ++a) u_bar[((i64)i * DIM + a) * Bp + nm.b] = acc[a];
  }
}

template <int DIM, bool NODES>
CauchyAdjointForm<DIM, NODES> form_of(const int* elems, const double* gtab, double lam1, double mu1, const double* u,
                               const double* E, i64 e_se, i64 e_sb, int m, const double* sigma_bar, i64 osc, i64 ose,
                               const double* vm_bar, const double* w_bar, double* work, int B) {
  return CauchyAdjointForm<DIM, NODES>{CauchyElement<DIM>{elems, gtab, lam1, mu1, u, E, e_se, e_sb, m}, sigma_bar, osc, ose,
                                vm_bar, w_bar, work, B};
}

// what every entry refuses: pointers, dim, sizes, the E strides, the int32 codes e * npe + p
bool bad_common(const int* elems, const double* gtab, int dim, const double* u, const double* E, i64 e_se, i64 e_sb, int n,
                int m) {
  return !elems || !gtab || !u || !E || (dim != 2 && dim != 3) || n < 1 || m < 1 || e_se < 0 || e_sb < 0 ||
         (i64)m * (dim + 1) >= (1LL << 31);
}

// ... and of the cotangents: at least one, a stress array with positive strides
bool bad_cotangents(const double* sigma_bar, i64 osc, i64 ose, const double* vm_bar, const double* w_bar) {
  return (!sigma_bar && !vm_bar && !w_bar) || (sigma_bar && (osc < 1 || ose < 1));
}

// bytes of E as the kernels read it: a field per sample, one field, one number per sample, one number
double modulus_bytes(i64 e_se, i64 e_sb, int m, int Bp) { return 8.0 * (e_se ? (double)m : 1.0) * (e_sb ? (double)Bp : 1.0); }

// per-element doubles of the arrays given: a stress array, vm, w
double element_doubles(int nc, const void* sigma, const void* vm, const void* w) {
  return (sigma ? (double)nc : 0.0) + (vm ? 1.0 : 0.0) + (w ? 1.0 : 0.0);
}

}  // namespace

// =========================================================================================
// C ABI (include/diffhe_hyper_stress.h)
// =========================================================================================
extern "C" int diffhe_hyper_stress_eval(const int* elems, const double* gtab, int dim, double lam1, double mu1,
                                        const double* u, const double* E, long long e_se, long long e_sb, int n, int m,
                                        int Bp, double* sigma, long long osc, long long ose, double* vm, double* w,
                                        void* stream) {
  if (bad_common(elems, gtab, dim, u, E, e_se, e_sb, n, m) || (!sigma && !vm && !w) || (sigma && (osc < 1 || ose < 1)))
    return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nc = dim * (dim + 1) / 2;
  // u once per dof, E, the outputs
  diffhe::account(8.0 * Bp * ((double)dim * n + element_doubles(nc, sigma, vm, w) * m) + modulus_bytes(e_se, e_sb, m, Bp));
  const dim3 grid = diffhe::node_grid(m, Bp);
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(hyper_stress_eval_kernel<D()>, grid, dim3(256), 0, (hipStream_t)stream,
                       CauchyElement<D()>{elems, gtab, lam1, mu1, u, E, e_se, e_sb, m}, Bp, sigma, osc, ose, vm, w);
  });
  return diffhe::check_launch();
}

extern "C" int diffhe_hyper_stress_adjoint(const int* elems, const double* gtab, int dim, double lam1, double mu1,
                                           const double* u, const double* E, long long e_se, long long e_sb,
                                           const double* sigma_bar, long long osc, long long ose, const double* vm_bar,
                                           const double* w_bar, const int* inc_ptr, const int* inc, int n, int m, int B,
                                           int Bp, double* work, double* u_bar, double* de_e, double* de_part,
                                           double* de_sum, void* stream) {
  if (bad_common(elems, gtab, dim, u, E, e_se, e_sb, n, m) || bad_cotangents(sigma_bar, osc, ose, vm_bar, w_bar) || B < 1 ||
      B > Bp)
    return DIFFHE_E_BADARG;
  const bool nodes = u_bar != nullptr;
  if ((work != nullptr) != nodes || (inc_ptr != nullptr) != nodes || (inc != nullptr) != nodes) return DIFFHE_E_BADARG;
  if ((de_part == nullptr) != (de_sum == nullptr) || (!nodes && !de_e && !de_part)) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nc = dim * (dim + 1) / 2;
  // element pass: u once per dof, E, the cotangents, T and dE per element
  const double bytes = 8.0 * Bp * ((double)dim * n + (element_doubles(nc, sigma_bar, vm_bar, w_bar) +
                                                     (nodes ? (double)dim * dim : 0.0) + (de_e ? 1.0 : 0.0)) * m) +
                       modulus_bytes(e_se, e_sb, m, Bp);
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    constexpr int DIM = D();
    const int status = diffhe::dispatch_bool(nodes, [&](auto N) {
      return diffhe::launch_element_grad(
          form_of<DIM, N()>(elems, gtab, lam1, mu1, u, E, e_se, e_sb, m, sigma_bar, osc, ose, vm_bar, w_bar, work, B), m, Bp,
          de_e, 0, Bp, de_part, de_sum, bytes, stream);
    });
    if (status != DIFFHE_OK || !nodes) return status;
    diffhe::account(8.0 * Bp * ((double)DIM * DIM * m + (double)DIM * n));   // node pass: T once, u_bar once per dof
    hipLaunchKernelGGL(hyper_stress_node_kernel<DIM>, diffhe::node_grid(n, Bp), dim3(256), 0, (hipStream_t)stream,
                       inc_ptr, inc, gtab, (const double*)work, n, m, B, Bp, u_bar);
    return diffhe::check_launch();
  });
}

extern "C" int diffhe_hyper_stress_adjoint_shared(const int* elems, const double* gtab, int dim, double lam1, double mu1,
                                                  const double* u, const double* E, long long e_se, long long e_sb,
                                                  const double* sigma_bar, long long osc, long long ose,
                                                  const double* vm_bar, const double* w_bar, int n, int m, int B, int Bp,
                                                  double* de, void* stream) {
  if (bad_common(elems, gtab, dim, u, E, e_se, e_sb, n, m) || bad_cotangents(sigma_bar, osc, ose, vm_bar, w_bar) || !de ||
      B < 1 || B > Bp)
    return DIFFHE_E_BADARG;
  const int nc = dim * (dim + 1) / 2;
  const double bytes = 8.0 * (Bp * ((double)dim * n + element_doubles(nc, sigma_bar, vm_bar, w_bar) * m) + (double)m) +
                       modulus_bytes(e_se, e_sb, m, Bp);
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return diffhe::launch_element_grad_shared(
        form_of<D(), false>(elems, gtab, lam1, mu1, u, E, e_se, e_sb, m, sigma_bar, osc, ose, vm_bar, w_bar, nullptr, B), m,
        B, Bp, de, 0, 1, bytes, stream);
  });
}
