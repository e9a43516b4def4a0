// Shape derivative of a linear-elastic solve and of a stress evaluation: dL/dX for the node coordinates X (ours: the
// reference has scalar unknowns only; definitions: include/diffhe_elastic_shape.h).  The vector analogue of shape.hip.
//
// Solve.  With R = K(X, E) u - M(X) f - load = 0 on the free dofs, the adjoint lambda (0 on fixed dofs), the displacement
// gradients H_w[a][t] = sum_p w[(p, a)] g_p[t] of the full u and of lambda, and S(H) = 2 mu1 sym(H) + lam1 tr(H) I,
//
//   lambda^T K u = sum_e A_e E_e S(H_u) : H_lambda,      d g_q[t] / d x_p[k] = -g_q[k] g_p[t],      d A / d x_p = A g_p,
//
// so that element e adds to its vertex p
//
//   A_e [ sum_b E_eb ( H_u^T S(H_lambda) + H_lambda^T S(H_u) - (S(H_u) : H_lambda) I ) + q_e I ] g_p,
//   q_e = sum_b sum_a (sum_p lambda_(p,a)) (sum_p f_(p,a)) / (d+1)^2      (F_(p,a) = A_e/(d+1) * mean_q f_(q,a)).
//
// Stress.  sigma = E S(H_u) at fixed u has no size factor; with T = dL/dH_u, the symmetric tensor of the stress adjoint's
// element pass (stress_form.h: the one statement of the cotangent chain), vertex p gets -(sum_b H_u^T T_b) g_p.
//
// Both are odd in g: the table is the plan's oriented one.  Two passes, no floating-point atomics (bitwise reproducible):
//   the element kernels: one group of LB lanes per element reduces its samples (lanes over the contiguous samples,
//     LB = min(next power of two >= B, 64), a loop b += LB beyond) to d^2 (+ 1) numbers by a fixed-order xor butterfly and
//     writes the (d+1) d vertex contributions to work (m, (d+1) d);
//   shape_gather_kernel (shape_gather.h): per node, the contributions of its incident (element, vertex) pairs in the
//     fixed order of the incidence list.
// A lane accumulates H_u and H_lambda while it reads the nodal values, so it never holds the 2 (d+1) d of them; the lift
// enters as the element's own H_g, formed once per element.
#include "diffhe_elastic_shape.h"
#include "shape_gather.h"
#include "stress_form.h"
#include "launch.h"

namespace {

using namespace diffhe;

// S(H) = 2 mu1 sym(H) + lam1 tr(H) I
template <int D>
__device__ __forceinline__ void unit_stress_tensor(const double (*H)[D], double lam1, double mu1, double (*S)[D]) {
  double tr = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a) tr += H[a][a];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int t = 0; t < D; ++t) S[a][t] = a == t ? fma(2.0 * mu1, H[a][a], lam1 * tr) : mu1 * (H[a][t] + H[t][a]);
}

// out[p d + k] = scale * sum_t M[k][t] G[p][t], component ci = p d + k written by lane ci % LB of the group
template <int D>
__device__ __forceinline__ void write_vertices(const double (*M)[D], const double (*G)[D], double scale, int LB, int sub,
                                               double* __restrict__ out) {
  constexpr int NC = (D + 1) * D;
#pragma unroll
  for (int ci = 0; ci < NC; ++ci) {
    if (ci % LB != sub) continue;
    const int p = ci / D, k = ci % D;
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < D; ++t) s = fma(M[k][t], G[p][t], s);
    out[ci] = scale * s;
  }
}

template <int D>
__global__ __launch_bounds__(256) void elast_shape_elem_kernel(const int* __restrict__ elems,
                                                               const double* __restrict__ gtab,
                                                               const double* __restrict__ vol, int m, int B, int Bp,
                                                               int LB, double lam1, double mu1,
                                                               const double* __restrict__ u, const double* __restrict__ g,
                                                               const double* __restrict__ lam,
                                                               const double* __restrict__ f, const double* __restrict__ E,
                                                               i64 ese, i64 esb, double* __restrict__ work) {
  constexpr int NPE = D + 1, NC = NPE * D;
  const GroupMap gm = group_map(LB);               // a group of LB lanes per element
  const int sub = gm.sub;
  for (i64 e = gm.item0; e < m; e += gm.stride) {
    int v[NPE];
    double G[NPE][D], Hg[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int t = 0; t < D; ++t) Hg[a][t] = 0.0;
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
      v[p] = elems[(i64)p * m + e];
#pragma unroll
      for (int t = 0; t < D; ++t) G[p][t] = gtab[(i64)(p * D + t) * m + e];
      if (g) {                                      // the lift: prescribed values are part of the full u
#pragma unroll
        for (int a = 0; a < D; ++a) {
          const double gp = g[(i64)v[p] * D + a];
#pragma unroll
          for (int t = 0; t < D; ++t) Hg[a][t] = fma(gp, G[p][t], Hg[a][t]);
        }
      }
    }
    const double size = vol[e];
    double M[D][D], q = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
      for (int t = 0; t < D; ++t) M[k][t] = 0.0;
    for (int b = sub; b < B; b += LB) {             // padding samples (b >= B) carry no gradient
      double Hu[D][D], Hl[D][D], load = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int t = 0; t < D; ++t) {
          Hu[a][t] = Hg[a][t];
          Hl[a][t] = 0.0;
        }
#pragma unroll
      for (int a = 0; a < D; ++a) {
        double sl = 0.0, sf = 0.0;
#pragma unroll
        for (int p = 0; p < NPE; ++p) {
          const i64 o = ((i64)v[p] * D + a) * Bp + b;
          const double up = u[o], lp = lam[o];
#pragma unroll
          for (int t = 0; t < D; ++t) {
            Hu[a][t] = fma(up, G[p][t], Hu[a][t]);
            Hl[a][t] = fma(lp, G[p][t], Hl[a][t]);
          }
          sl += lp;
          if (f) sf += f[o];
        }
        load = fma(sl, sf, load);
      }
      q += load / (double)(NPE * NPE);
      double Su[D][D], Sl[D][D];
      unit_stress_tensor<D>(Hu, lam1, mu1, Su);
      unit_stress_tensor<D>(Hl, lam1, mu1, Sl);
      double dot = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int t = 0; t < D; ++t) dot = fma(Su[a][t], Hl[a][t], dot);
      const double Ee = E[e * ese + (i64)b * esb];
#pragma unroll
      for (int k = 0; k < D; ++k)
#pragma unroll
        for (int t = 0; t < D; ++t) {
          double s = k == t ? -dot : 0.0;
#pragma unroll
          for (int a = 0; a < D; ++a) s = fma(Hu[a][k], Sl[a][t], fma(Hl[a][k], Su[a][t], s));
          M[k][t] = fma(Ee, s, M[k][t]);
        }
    }
    group_sum(LB, M, q);
#pragma unroll
    for (int k = 0; k < D; ++k) M[k][k] += q;
    // a degenerate element has a zero row in the table and size 0: every contribution is +-0
    write_vertices<D>(M, G, size, LB, sub, work + e * NC);
  }
}

template <int D>
__global__ __launch_bounds__(256) void stress_shape_elem_kernel(const StressAdjointForm<D, false> form, int m, int B,
                                                                int Bp, int LB, double* __restrict__ work) {
  constexpr int NPE = D + 1, NC = NPE * D, NV = D * (D + 1) / 2;
  const GroupMap gm = group_map(LB);
  const int sub = gm.sub;
  for (i64 e = gm.item0; e < m; e += gm.stride) {
    typename StressAdjointForm<D, false>::Elem el;
    form.load((int)e, el);
    double N[D][D];
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
      for (int t = 0; t < D; ++t) N[k][t] = 0.0;
    for (int b = sub; b < B; b += LB) {             // padding samples (b >= B): no cotangent read, no gradient
      double H[D][D], s[NV], c[NV], T[NV], szz, czz;
      form.el_of.displacement_gradient(el, Bp, b, H);
      const double Ee = form.cotangent(el, Bp, b, H, s, c, szz, czz);
      form.tensor(c, czz, Ee, T);
      double P[D][D];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        P[voigt_row<D>(k)][voigt_col<D>(k)] = T[k];
        P[voigt_col<D>(k)][voigt_row<D>(k)] = T[k];
      }
#pragma unroll
      for (int k = 0; k < D; ++k)
#pragma unroll
        for (int t = 0; t < D; ++t)
#pragma unroll
          for (int a = 0; a < D; ++a) N[k][t] = fma(H[a][k], P[a][t], N[k][t]);
    }
    group_sum(LB, N);
    write_vertices<D>(N, el.G, -1.0, LB, sub, work + e * NC);
  }
}

// the grid of an element pass
dim3 element_grid(int m, int LB) { return dim3(group_grid(m, LB, 8192)); }

// what both entries refuse: pointers, dim, sizes, the batch, the E strides, the int32 codes e * npe + p
bool bad_common(const int* elems, const double* gtab, int dim, const double* u, const double* E, i64 e_se, i64 e_sb, int n,
                int m, int B, int Bp, const int* inc_ptr, const int* inc, const double* work, const double* grad) {
  return !elems || !gtab || !u || !E || !inc_ptr || !inc || !work || !grad || (dim != 2 && dim != 3) || n < 1 || m < 1 ||
         B < 1 || B > Bp || e_se < 0 || e_sb < 0 || (i64)m * (dim + 1) >= (1LL << 31);
}

// bytes of E as the kernels read it, and of the two passes' own traffic: work written and read once, the gradient
double modulus_bytes(i64 e_se, i64 e_sb, int m, int B) { return 8.0 * (e_se ? (double)m : 1.0) * (e_sb ? (double)B : 1.0); }
double pass_bytes(int dim, int n, int m) { return 8.0 * (2.0 * (dim + 1) * dim * m + (double)dim * n); }

}  // namespace

extern "C" int diffhe_elast_shape_grad(const int* elems, const double* gtab, const double* vol, int dim, double lam1,
                                       double mu1, const double* u, const double* g, const double* lam, const double* f,
                                       const double* E, long long e_se, long long e_sb, int n, int m, int B, int Bp,
                                       const int* inc_ptr, const int* inc, double* work, double* grad, void* stream) {
  if (bad_common(elems, gtab, dim, u, E, e_se, e_sb, n, m, B, Bp, inc_ptr, inc, work, grad) || !vol || !lam)
    return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int LB = group_lanes(B);
  // algorithmic bytes: u and lambda (and f) once per dof and sample, E, the vertex contributions, the gradient
  account(8.0 * B * (double)dim * n * (f ? 3.0 : 2.0) + modulus_bytes(e_se, e_sb, m, B) + pass_bytes(dim, n, m));
  hipStream_t st = (hipStream_t)stream;
  dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(elast_shape_elem_kernel<D()>, element_grid(m, LB), dim3(256), 0, st, elems, gtab, vol, m, B, Bp, LB,
                       lam1, mu1, u, g, lam, f, E, e_se, e_sb, work);
  });
  launch_shape_gather(inc_ptr, inc, work, n, dim, grad, st);
  return check_launch();
}

template <int D>
static void launch_stress_shape(const int* elems, const double* gtab, double lam1, double mu1, double nu_z, const double* u,
                                const double* E, i64 e_se, i64 e_sb, const double* sigma_bar, i64 osc, i64 ose,
                                const double* vm_bar, int m, int B, int Bp, double* work, hipStream_t st) {
  StressAdjointForm<D, false> form;
  StressElement<D, false>& el = form.el_of;
  el.elems = elems, el.gtab = gtab, el.lam1 = lam1, el.mu1 = mu1, el.nu_z = D == 2 ? nu_z : 0.0;
  el.u = u, el.E = E, el.ese = e_se, el.esb = e_sb, el.m = m;
  form.sigma_bar = sigma_bar, form.osc = osc, form.ose = ose, form.vm_bar = vm_bar, form.work = nullptr, form.B = B;
  const int LB = group_lanes(B);
  hipLaunchKernelGGL(stress_shape_elem_kernel<D>, element_grid(m, LB), dim3(256), 0, st, form, m, B, Bp, LB, work);
}

extern "C" int diffhe_stress_shape_grad(const int* elems, const double* gtab, int dim, double lam1, double mu1, double nu_z,
                                        const double* u, const double* E, long long e_se, long long e_sb,
                                        const double* sigma_bar, long long osc, long long ose, const double* vm_bar, int n,
                                        int m, int B, int Bp, const int* inc_ptr, const int* inc, double* work,
                                        double* grad, void* stream) {
  if (bad_common(elems, gtab, dim, u, E, e_se, e_sb, n, m, B, Bp, inc_ptr, inc, work, grad) || (!sigma_bar && !vm_bar) ||
      (sigma_bar && (osc < 1 || ose < 1)))
    return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nc = dim * (dim + 1) / 2;
  // algorithmic bytes: u once per dof and sample, the cotangents, E, the vertex contributions, the gradient
  account(8.0 * B * ((double)dim * n + (sigma_bar ? (double)nc * m : 0.0) + (vm_bar ? (double)m : 0.0)) +
          modulus_bytes(e_se, e_sb, m, B) + pass_bytes(dim, n, m));
  hipStream_t st = (hipStream_t)stream;
  dispatch_dim<2, 3>(dim, [&](auto D) {
    launch_stress_shape<D()>(elems, gtab, lam1, mu1, nu_z, u, E, e_se, e_sb, sigma_bar, osc, ose, vm_bar, m, B, Bp, work, st);
  });
  launch_shape_gather(inc_ptr, inc, work, n, dim, grad, st);
  return check_launch();
}
