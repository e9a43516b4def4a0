// Vibration modes of elastic bodies (diffhe.modal): the lumped mass of a density per element and sample, and the
// Hellmann-Feynman gradient of the eigenvalues with respect to that density (definitions: include/diffhe_modal.h).  The
// block passes of the iteration are the kernels of eigen.hip under their per-sample mass accessor.
//
// Data layout as in elastic.hip: batch innermost, lanes over samples (node_map), so node ids, element sizes and list
// entries are wave-uniform and every access is one contiguous segment.  fp64, no atomics: every sum has a fixed order,
// results are bitwise reproducible.
#include "common.h"
#include "diffhe_modal.h"
#include "element_grad.h"
#include "launch.h"

namespace {

using namespace diffhe;

// ---------------------------------------------------------------------------------------
// mass[i, b] = sum over the incidence list of node i (codes e * NPE + p, element order) of rho[e, b] vol_e / NPE.
// Samples b >= B: rho = 1, not read.
// ---------------------------------------------------------------------------------------
template <int NPE>
__global__ __launch_bounds__(256) void modal_mass_kernel(const int* __restrict__ inc_ptr, const int* __restrict__ inc,
                                                          const double* __restrict__ vol,
                                                          const double* __restrict__ rho, i64 rse, i64 rsb, int n, int B,
                                                          int Bv, double* __restrict__ mass) {
  const NodeMap nm = node_map(Bv);
  if (nm.b >= Bv) return;
  const double share = 1.0 / NPE;
  const bool real = nm.b < B;
  for (int i = nm.node0; i < n; i += nm.stride) {
    double acc = 0.0;
    for (int j = inc_ptr[i]; j < inc_ptr[i + 1]; ++j) {
      const int e = inc[j] / NPE;
      const double r = real ? rho[(i64)e * rse + (i64)nm.b * rsb] : 1.0;
      acc += r * (vol[e] * share);
    }
    mass[(i64)i * Bv + nm.b] = acc;
  }
}

// ---------------------------------------------------------------------------------------
// d lambda / d rho as a form of element_grad.h (NC = 1): vol_e / (DIM + 1) sum_i w[i, b] sum_p sum_a X[i, (el_p, a), b]^2.
// ---------------------------------------------------------------------------------------
template <int DIM>
struct GradRhoForm {
  static constexpr int NC = 1;
  static constexpr int NPE = DIM + 1;
  const int* __restrict__ elems;
  const double* __restrict__ vol;
  const double* __restrict__ X;
  const double* __restrict__ w;
  int k, n, m, B;

  struct Elem {
    int node[NPE];
    double share;
  };

  __device__ __forceinline__ void load(int e, Elem& el) const {
    el.share = vol[e] / NPE;
#pragma unroll
    for (int p = 0; p < NPE; ++p) el.node[p] = elems[(i64)p * m + e];
  }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* out) const {
    if (b >= B) {
      out[0] = 0.0;
      return;
    }
    const i64 cs = (i64)n * DIM * Bp;
    double s = 0.0;
    for (int i = 0; i < k; ++i) {
      const double* x = X + i * cs + b;
      double q = 0.0;
#pragma unroll
      for (int p = 0; p < NPE; ++p)
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
          const double v = x[((i64)el.node[p] * DIM + a) * Bp];
          q = fma(v, v, q);
        }
      s = fma(w[(i64)i * Bp + b], q, s);
    }
    out[0] = el.share * s;
  }
};

bool bad_grad(const int* elems, const double* vol, int dim, const double* X, const double* w, int k, int n, int m, int B,
              int Bp) {
  return !elems || !vol || !X || !w || (dim != 2 && dim != 3) || k < 1 || n < 1 || m < 1 || B < 1 || B > Bp;
}

}  // namespace

extern "C" int diffhe_modal_mass(const int* inc_ptr, const int* inc, const double* vol, int dim, const double* rho,
                                 long long r_se, long long r_sb, int n, int m, int B, int Bv, double* mass,
                                 void* stream) {
  if (!inc_ptr || !inc || !vol || !rho || !mass || (dim != 2 && dim != 3) || n < 1 || m < 1 || B < 1 || B > Bv)
    return DIFFHE_E_BADARG;
  if (r_se < 0 || r_sb < 0) return DIFFHE_E_BADARG;   // Bv == 1: the one sample is b = 0, r_sb multiplies nothing
  if (!valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  account(8.0 * Bv * ((double)n + (r_se ? (double)m : 0)));
  dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(modal_mass_kernel<D() + 1>, node_grid(n, Bv), dim3(256), 0, (hipStream_t)stream, inc_ptr, inc, vol,
                       rho, r_se, r_sb, n, B, Bv, mass);
  });
  return check_launch();
}

extern "C" int diffhe_modal_grad_rho(const int* elems, const double* vol, int dim, const double* X, const double* w, int k,
                                     int n, int m, int B, int Bp, double* dr_e, double* dr_part, double* dr_sum,
                                     void* stream) {
  if (bad_grad(elems, vol, dim, X, w, k, n, m, B, Bp)) return DIFFHE_E_BADARG;
  if (!dr_e && !dr_part) return DIFFHE_E_BADARG;
  if ((dr_part == nullptr) != (dr_sum == nullptr)) return DIFFHE_E_BADARG;
  const double bytes = 8.0 * Bp * ((double)k * dim * n + k + (dr_e ? (double)m : 0));
  return dispatch_dim<2, 3>(dim, [&](auto D) {
    return launch_element_grad(GradRhoForm<D()>{elems, vol, X, w, k, n, m, B}, m, Bp, dr_e, 0, Bp, dr_part, dr_sum, bytes,
                               stream);
  });
}

extern "C" int diffhe_modal_grad_rho_shared(const int* elems, const double* vol, int dim, const double* X, const double* w,
                                            int k, int n, int m, int B, int Bp, double* dr, void* stream) {
  if (bad_grad(elems, vol, dim, X, w, k, n, m, B, Bp) || !dr) return DIFFHE_E_BADARG;
  const double bytes = 8.0 * (Bp * ((double)k * dim * n + k) + (double)m);
  return dispatch_dim<2, 3>(dim, [&](auto D) {
    return launch_element_grad_shared(GradRhoForm<D()>{elems, vol, X, w, k, n, m, B}, m, B, Bp, dr, 0, 1, bytes, stream);
  });
}
