// Stress recovery of an anisotropic elastic solve (ours: the reference has scalar unknowns only): sigma = C eps(u) in Voigt
// components with a stiffness matrix per element and sample, the fused quadratic failure index phi = q.sigma +
// sigma.Q sigma with a criterion (q, Q) per element and sample, and their adjoint with respect to the displacement u, the
// stiffness and the criterion (definitions: include/diffhe_elastic_aniso_stress.h).  u is the full displacement, so no
// Dirichlet data is read; gtab is the ORIENTED gradient table of stress.hip.  C and Q are read as the row-major upper
// triangle of their matrices, as elastic_aniso.hip reads C: an off-diagonal component fills both symmetric entries.
//
// Data layout as in stress.hip: dof-major, batch innermost, lanes over samples (node_map) ALWAYS, so element data -- node
// ids, gradients, list entries -- is wave-uniform and every access is one contiguous segment.  fp64, no atomics anywhere:
// every sum has a fixed order, results are bitwise reproducible.
//
// Neither matrix is ever held whole: a product with C or Q walks the upper triangle once and every component it loads
// feeds its (at most two) entries of the result at once, so what lives across a product is the nv-vector it builds.  The
// adjoint runs on the element loop of element_grad.h with two forms, instantiated apart so that neither carries the
// other's outputs: StiffnessGradForm (NC = nt: dC, and T = dL/dH in Voigt components as a side product where a node pass
// follows; t = C c is the very product that gave sigma = C eps) and CriterionGradForm (NC = nk: dq, dQ; it needs C for
// sigma only).  The node pass is stress.hip's, stress_node.h.
#include "common.h"
#include "diffhe_elastic_aniso_stress.h"
#include "element_grad.h"
#include "stress_node.h"
#include "launch.h"

namespace {

using namespace diffhe;

// What both directions read of an element and a sample.
template <int DIM>
struct AnisoStressElement {
  static constexpr int NPE = DIM + 1, NV = DIM * (DIM + 1) / 2, NT = NV * (NV + 1) / 2, NK = NV + NT;
  const int* __restrict__ elems;
  const double* __restrict__ gtab;
  const double* __restrict__ u;
  const double* __restrict__ C;
  i64 csc, cse, csb;
  const double* __restrict__ crit;
  i64 ksc, kse, ksb;
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

  // the engineering Voigt strain of sample b: H[a][a]; H[a][t] + H[t][a]
  __device__ __forceinline__ void strain(const Elem& el, int Bp, int b, double* eps) const {
    double H[DIM][DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = 0; t < DIM; ++t) H[a][t] = 0.0;
#pragma unroll
    for (int p = 0; p < NPE; ++p)
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const double up = u[((i64)el.node[p] * DIM + a) * Bp + b];
#pragma unroll
        for (int t = 0; t < DIM; ++t) H[a][t] = fma(up, el.G[p][t], H[a][t]);
      }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int a = voigt_row<DIM>(k), t = voigt_col<DIM>(k);
      eps[k] = k < DIM ? H[a][a] : H[a][t] + H[t][a];
    }
  }

  // y = C x for the stiffness of element e and sample b: sigma = C eps, and t = C c in the adjoint
  __device__ __forceinline__ void stiffness_times(int e, int b, const double* x, double* y) const {
    const double* __restrict__ Cp = C + (i64)e * cse + (i64)b * csb;
#pragma unroll
    for (int I = 0; I < NV; ++I) y[I] = 0.0;
    int t = 0;
#pragma unroll
    for (int I = 0; I < NV; ++I)
#pragma unroll
      for (int J = I; J < NV; ++J, ++t) {
        const double c = Cp[t * csc];
        y[I] = fma(c, x[J], y[I]);
        if (J != I) y[J] = fma(c, x[I], y[J]);
      }
  }

  // phi = q.sg + sg.Q sg
  __device__ __forceinline__ double failure_index(int e, int b, const double* sg) const {
    const double* __restrict__ Kp = crit + (i64)e * kse + (i64)b * ksb;
    double phi = 0.0;
#pragma unroll
    for (int I = 0; I < NV; ++I) phi = fma(Kp[I * ksc], sg[I], phi);
    int t = NV;
#pragma unroll
    for (int I = 0; I < NV; ++I)
#pragma unroll
      for (int J = I; J < NV; ++J, ++t) {
        const double w = Kp[t * ksc] * sg[I];
        phi = fma(J == I ? w : 2.0 * w, sg[J], phi);
      }
    return phi;
  }

  // c += pb (q + 2 Q sg): the cotangent of sigma that phi_bar = pb sends through phi
  __device__ __forceinline__ void add_failure_cotangent(int e, int b, double pb, const double* sg, double* c) const {
    const double* __restrict__ Kp = crit + (i64)e * kse + (i64)b * ksb;
    const double pb2 = 2.0 * pb;
#pragma unroll
    for (int I = 0; I < NV; ++I) c[I] = fma(pb, Kp[I * ksc], c[I]);
    int t = NV;
#pragma unroll
    for (int I = 0; I < NV; ++I)
#pragma unroll
      for (int J = I; J < NV; ++J, ++t) {
        const double w = pb2 * Kp[t * ksc];
        c[I] = fma(w, sg[J], c[I]);
        if (J != I) c[J] = fma(w, sg[I], c[J]);
      }
  }
};

// ---------------------------------------------------------------------------------------
// sigma at c*osc + e*ose + b and / or phi (m, Bp); a NULL output is neither computed nor stored.
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void aniso_stress_eval_kernel(const AnisoStressElement<DIM> el_of, int Bp,
                                                                 double* __restrict__ sigma, i64 osc, i64 ose,
                                                                 double* __restrict__ phi) {
  constexpr int NV = DIM * (DIM + 1) / 2;
  const NodeMap nm = node_map(Bp);  // "nodes" are elements here
  if (nm.b >= Bp) return;
  for (int e = nm.node0; e < el_of.m; e += nm.stride) {
    typename AnisoStressElement<DIM>::Elem el;
    double eps[NV], sg[NV];
    el_of.load(e, el);
    el_of.strain(el, Bp, nm.b, eps);
    el_of.stiffness_times(e, nm.b, eps, sg);
    if (sigma) {
#pragma unroll
      for (int k = 0; k < NV; ++k) sigma[k * osc + e * ose + nm.b] = sg[k];
    }
    if (phi) phi[(i64)e * Bp + nm.b] = el_of.failure_index(e, nm.b, sg);
  }
}

// what the two adjoint forms share: the element, the cotangents, the batch
template <int DIM>
struct AnisoStressBars {
  AnisoStressElement<DIM> el_of;
  const double* __restrict__ sigma_bar;
  i64 osc, ose;
  const double* __restrict__ phi_bar;
  int B;
};

// ---------------------------------------------------------------------------------------
// dC as a form of element_grad.h: out (nt) = c_I eps_J + [I != J] c_J eps_I with c = sigma_bar + phi_bar (q + 2 Q sigma)
// and, where `work` is given (NODES), t = C c to work (nv, m, Bp) (include/diffhe_elastic_aniso_stress.h).  Samples
// b >= B: zeros, no cotangent read.  NODES is a template argument so that the passes without a node pass -- dC alone, and
// the batch-summing kernel -- never form t.
// ---------------------------------------------------------------------------------------
template <int DIM, bool NODES>
struct StiffnessGradForm {
  static constexpr int NV = DIM * (DIM + 1) / 2, NC = NV * (NV + 1) / 2;
  typedef typename AnisoStressElement<DIM>::Elem Elem;
  AnisoStressBars<DIM> in;
  double* __restrict__ work;

  __device__ __forceinline__ void load(int e, Elem& el) const { in.el_of.load(e, el); }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* out) const {
    const AnisoStressElement<DIM>& el_of = in.el_of;
    const i64 mb = (i64)el_of.m * Bp, at = (i64)el.e * Bp + b;
    if (b >= in.B) {
#pragma unroll
      for (int t = 0; t < NC; ++t) out[t] = 0.0;
      if constexpr (NODES) {
#pragma unroll
        for (int k = 0; k < NV; ++k) work[k * mb + at] = 0.0;
      }
      return;
    }
    double eps[NV], c[NV];
    el_of.strain(el, Bp, b, eps);
#pragma unroll
    for (int k = 0; k < NV; ++k) c[k] = in.sigma_bar ? in.sigma_bar[k * in.osc + el.e * in.ose + b] : 0.0;
    if (in.phi_bar) {
      double sg[NV];
      el_of.stiffness_times(el.e, b, eps, sg);
      el_of.add_failure_cotangent(el.e, b, in.phi_bar[at], sg, c);
    }
    int t = 0;
#pragma unroll
    for (int I = 0; I < NV; ++I)
#pragma unroll
      for (int J = I; J < NV; ++J, ++t) out[t] = J == I ? c[I] * eps[I] : fma(c[I], eps[J], c[J] * eps[I]);
    if constexpr (NODES) {
      double tt[NV];
      el_of.stiffness_times(el.e, b, c, tt);
#pragma unroll
      for (int k = 0; k < NV; ++k) work[k * mb + at] = tt[k];
    }
  }
};

// ---------------------------------------------------------------------------------------
// d(q, Q) as a form of element_grad.h: out (nk) = phi_bar sigma_I, then (1 + [I != J]) phi_bar sigma_I sigma_J.  C is read
// for sigma and nothing else.  Samples b >= B: zeros, no cotangent read.
// ---------------------------------------------------------------------------------------
template <int DIM>
struct CriterionGradForm {
  static constexpr int NV = DIM * (DIM + 1) / 2, NC = NV + NV * (NV + 1) / 2;
  typedef typename AnisoStressElement<DIM>::Elem Elem;
  AnisoStressBars<DIM> in;

  __device__ __forceinline__ void load(int e, Elem& el) const { in.el_of.load(e, el); }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* out) const {
    if (b >= in.B) {
#pragma unroll
      for (int t = 0; t < NC; ++t) out[t] = 0.0;
      return;
    }
    double eps[NV], sg[NV], ps[NV];
    in.el_of.strain(el, Bp, b, eps);
    in.el_of.stiffness_times(el.e, b, eps, sg);
    const double pb = in.phi_bar[(i64)el.e * Bp + b];
#pragma unroll
    for (int I = 0; I < NV; ++I) out[I] = ps[I] = pb * sg[I];
    int t = NV;
#pragma unroll
    for (int I = 0; I < NV; ++I)
#pragma unroll
      for (int J = I; J < NV; ++J, ++t) out[t] = J == I ? ps[I] * sg[I] : 2.0 * (ps[I] * sg[J]);
  }
};

// ---------------------------------------------------------------------------------------
// The element pass of a call that wants dL/du alone: T to work, dC formed by nobody (the compiler drops it).
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void aniso_stress_tensor_kernel(const StiffnessGradForm<DIM, true> form, int Bp) {
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  for (int e = nm.node0; e < form.in.el_of.m; e += nm.stride) {
    typename AnisoStressElement<DIM>::Elem el;
    double dc[StiffnessGradForm<DIM, true>::NC];
    form.load(e, el);
    form.eval(el, Bp, nm.b, dc);
  }
}

// The leading arguments of the three entries, as the C ABI passes them.
struct Head {
  const int* elems;
  const double* gtab;
  int dim;
  const double* u;
  const double* C;
  i64 csc, cse, csb;
  const double* crit;
  i64 ksc, kse, ksb;
};

template <int DIM>
AnisoStressElement<DIM> element_of(const Head& h, int m, bool with_crit) {
  return AnisoStressElement<DIM>{h.elems, h.gtab, h.u,   h.C,   h.csc, h.cse, h.csb, with_crit ? h.crit : nullptr,
                                 h.ksc,   h.kse,  h.ksb, m};
}

template <int DIM>
AnisoStressBars<DIM> bars_of(const Head& h, int m, const double* sigma_bar, i64 osc, i64 ose, const double* phi_bar, int B) {
  return AnisoStressBars<DIM>{element_of<DIM>(h, m, phi_bar != nullptr), sigma_bar, osc, ose, phi_bar, B};
}

// what every entry refuses: pointers, dim, sizes, the strides of C and the criterion, the int32 codes e * npe + p
bool bad_common(const Head& h, int n, int m) {
  return !h.elems || !h.gtab || !h.u || !h.C || (h.dim != 2 && h.dim != 3) || n < 1 || m < 1 || h.csc < 0 || h.cse < 0 ||
         h.csb < 0 || (h.crit && (h.ksc < 0 || h.kse < 0 || h.ksb < 0)) || (i64)m * (h.dim + 1) >= (1LL << 31);
}

// ... and of the cotangents: at least one, a stress array with positive strides, a criterion behind phi_bar
bool bad_cotangents(const Head& h, const double* sigma_bar, i64 osc, i64 ose, const double* phi_bar) {
  return (!sigma_bar && !phi_bar) || (sigma_bar && (osc < 1 || ose < 1)) || (phi_bar && !h.crit);
}

// bytes of a tensor of nc components as the kernels read it: per element or one, per sample or one
double tensor_bytes(int nc, i64 se, i64 sb, int m, int Bp) {
  return 8.0 * nc * (se ? (double)m : 1.0) * (sb ? (double)Bp : 1.0);
}

// bytes of what an element pass reads: u once per dof, C, the criterion and the cotangents given
double read_bytes(const Head& h, int n, int m, int Bp, bool with_crit, const void* sigma_bar, const void* phi_bar) {
  const int nv = h.dim * (h.dim + 1) / 2, nt = nv * (nv + 1) / 2;
  return 8.0 * Bp * ((double)h.dim * n + ((sigma_bar ? (double)nv : 0.0) + (phi_bar ? 1.0 : 0.0)) * m) +
         tensor_bytes(nt, h.cse, h.csb, m, Bp) + (with_crit ? tensor_bytes(nv + nt, h.kse, h.ksb, m, Bp) : 0.0);
}

}  // namespace

// =========================================================================================
// C ABI (include/diffhe_elastic_aniso_stress.h)
// =========================================================================================
extern "C" int diffhe_elastc_stress_eval(const int* elems, const double* gtab, int dim, const double* u, const double* C,
                                         long long c_sc, long long c_se, long long c_sb, const double* crit,
                                         long long k_sc, long long k_se, long long k_sb, int n, int m, int Bp,
                                         double* sigma, long long osc, long long ose, double* phi, void* stream) {
  const Head h{elems, gtab, dim, u, C, c_sc, c_se, c_sb, crit, k_sc, k_se, k_sb};
  if (bad_common(h, n, m) || (!sigma && !phi) || (sigma && (osc < 1 || ose < 1)) || (phi && !crit)) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nv = dim * (dim + 1) / 2;
  diffhe::account(read_bytes(h, n, m, Bp, phi != nullptr, nullptr, nullptr) +
                  8.0 * Bp * ((sigma ? (double)nv : 0.0) + (phi ? 1.0 : 0.0)) * m);
  const dim3 grid = diffhe::node_grid(m, Bp);
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(aniso_stress_eval_kernel<D()>, grid, dim3(256), 0, (hipStream_t)stream,
                       element_of<D()>(h, m, phi != nullptr), Bp, sigma, osc, ose, phi);
  });
  return diffhe::check_launch();
}

extern "C" int diffhe_elastc_stress_adjoint(const int* elems, const double* gtab, int dim, const double* u,
                                            const double* C, long long c_sc, long long c_se, long long c_sb,
                                            const double* crit, long long k_sc, long long k_se, long long k_sb,
                                            const double* sigma_bar, long long osc, long long ose, const double* phi_bar,
                                            const int* inc_ptr, const int* inc, int n, int m, int B, int Bp, double* work,
                                            double* u_bar, double* dc_e, long long dc_sc, long long dc_se,
                                            double* dc_part, double* dc_sum, double* dk_e, long long dk_sc,
                                            long long dk_se, double* dk_part, double* dk_sum, void* stream) {
  const Head h{elems, gtab, dim, u, C, c_sc, c_se, c_sb, crit, k_sc, k_se, k_sb};
  if (bad_common(h, n, m) || bad_cotangents(h, sigma_bar, osc, ose, phi_bar) || B < 1 || B > Bp) return DIFFHE_E_BADARG;
  const bool nodes = u_bar != nullptr;
  if ((work != nullptr) != nodes || (inc_ptr != nullptr) != nodes || (inc != nullptr) != nodes) return DIFFHE_E_BADARG;
  if ((dc_part == nullptr) != (dc_sum == nullptr) || (dk_part == nullptr) != (dk_sum == nullptr)) return DIFFHE_E_BADARG;
  const bool want_c = dc_e || dc_part, want_k = dk_e || dk_part;
  if ((!nodes && !want_c && !want_k) || (want_k && !phi_bar)) return DIFFHE_E_BADARG;
  if ((dc_e && (dc_sc < 1 || dc_se < 1)) || (dk_e && (dk_sc < 1 || dk_se < 1))) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nv = dim * (dim + 1) / 2, nt = nv * (nv + 1) / 2;
  const double reads = read_bytes(h, n, m, Bp, phi_bar != nullptr, sigma_bar, phi_bar);
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    constexpr int DIM = D();
    const AnisoStressBars<DIM> in = bars_of<DIM>(h, m, sigma_bar, osc, ose, phi_bar, B);
    int status = DIFFHE_OK;
    const double t_bytes = nodes ? 8.0 * Bp * (double)nv * m : 0.0;
    if (want_c) {          // dC, with T as its side product where a node pass follows
      const double bytes = reads + t_bytes + (dc_e ? 8.0 * Bp * (double)nt * m : 0.0);
      status = diffhe::dispatch_bool(nodes, [&](auto N) {
        return diffhe::launch_element_grad(StiffnessGradForm<DIM, N()>{in, work}, m, Bp, dc_e, dc_sc, dc_se, dc_part,
                                           dc_sum, bytes, stream);
      });
    } else if (nodes) {    // T alone
      diffhe::account(reads + t_bytes);
      hipLaunchKernelGGL(aniso_stress_tensor_kernel<DIM>, diffhe::node_grid(m, Bp), dim3(256), 0, (hipStream_t)stream,
                         StiffnessGradForm<DIM, true>{in, work}, Bp);
      status = diffhe::check_launch();
    }
    if (status != DIFFHE_OK) return status;
    if (want_k) {
      const double bytes = read_bytes(h, n, m, Bp, false, nullptr, phi_bar) + (dk_e ? 8.0 * Bp * (double)(nv + nt) * m : 0.0);
      status = diffhe::launch_element_grad(CriterionGradForm<DIM>{in}, m, Bp, dk_e, dk_sc, dk_se, dk_part, dk_sum, bytes,
                                           stream);
      if (status != DIFFHE_OK) return status;
    }
    if (!nodes) return status;
    diffhe::account(8.0 * Bp * ((double)nv * m + (double)DIM * n));   // node pass: T once, u_bar once per dof
    hipLaunchKernelGGL(stress_node_kernel<DIM>, diffhe::node_grid(n, Bp), dim3(256), 0, (hipStream_t)stream, inc_ptr, inc,
                       gtab, (const double*)work, n, m, B, Bp, u_bar);
    return diffhe::check_launch();
  });
}

extern "C" int diffhe_elastc_stress_adjoint_shared(const int* elems, const double* gtab, int dim, const double* u,
                                                   const double* C, long long c_sc, long long c_se, long long c_sb,
                                                   const double* crit, long long k_sc, long long k_se, long long k_sb,
                                                   const double* sigma_bar, long long osc, long long ose,
                                                   const double* phi_bar, int n, int m, int B, int Bp, double* dc,
                                                   long long dc_sc, long long dc_se, double* dk, long long dk_sc,
                                                   long long dk_se, void* stream) {
  const Head h{elems, gtab, dim, u, C, c_sc, c_se, c_sb, crit, k_sc, k_se, k_sb};
  if (bad_common(h, n, m) || bad_cotangents(h, sigma_bar, osc, ose, phi_bar) || B < 1 || B > Bp) return DIFFHE_E_BADARG;
  if ((!dc && !dk) || (dk && !phi_bar)) return DIFFHE_E_BADARG;
  if ((dc && (dc_sc < 1 || dc_se < 1)) || (dk && (dk_sc < 1 || dk_se < 1))) return DIFFHE_E_BADARG;
  const int nv = dim * (dim + 1) / 2, nt = nv * (nv + 1) / 2;
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    constexpr int DIM = D();
    const AnisoStressBars<DIM> in = bars_of<DIM>(h, m, sigma_bar, osc, ose, phi_bar, B);
    int status = DIFFHE_OK;
    if (dc) {
      const double bytes = read_bytes(h, n, m, Bp, phi_bar != nullptr, sigma_bar, phi_bar) + 8.0 * nt * m;
      status = diffhe::launch_element_grad_shared(StiffnessGradForm<DIM, false>{in, nullptr}, m, B, Bp, dc, dc_sc, dc_se,
                                                  bytes, stream);
    }
    if (status != DIFFHE_OK || !dk) return status;
    const double bytes = read_bytes(h, n, m, Bp, false, nullptr, phi_bar) + 8.0 * (nv + nt) * m;
    return diffhe::launch_element_grad_shared(CriterionGradForm<DIM>{in}, m, B, Bp, dk, dk_sc, dk_se, bytes, stream);
  });
}
