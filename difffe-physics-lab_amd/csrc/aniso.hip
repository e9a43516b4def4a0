// Anisotropic conductivity: -div(K grad u) + c u = f with a symmetric positive-definite tensor K per element (ours: the
// reference has a scalar kappa only).  P1 triangles and tetrahedra on the general (ELL) path.
//
// K is given in Voigt components, NC = 3 in 2D ordered (xx, yy, xy), NC = 6 in 3D ordered (xx, yy, zz, yz, xz, xy); an
// off-diagonal component is ONE parameter that fills both symmetric entries.  With the constant gradients g_p = grad phi_p
// of an element of size |e| (area, volume):
//
//   K_e[p, q]   = |e| g_p^T K g_q                = sum_c w_c(p, q) K_c,   w_c = |e| sym_c(g_p (x) g_q)
//   dL/dK_c[e]  = -|e| sym_c(grad lambda (x) grad u),   grad lambda = sum_p lambda_p g_p, grad u likewise
//
// sym_c(a (x) b) = a_i b_i on a diagonal component and a_i b_j + a_j b_i on an off-diagonal one.  Both read the
// gradient-form element table (g_p as (npe*d, m), |e| as (m)) instead of nc tables of npe^2 entries.
//
// Data layout as in ell.h: node-major, batch innermost; lanes run over samples, so table entries and list indices are
// wave-uniform and every tensor / nodal load is one contiguous segment.  The tensor is read through three strides
// (component, element, sample) and the gradient written through two (component, element; sample stride 1), so the
// batch-innermost layouts (nc, m, Bv) and (m, nc, Bv) and the batch-shared (m, nc) and (nc) all go through one kernel.
// No floating-point atomics anywhere: every sum has a fixed order and the results are bitwise reproducible.
//
// The gradient's element loop, its two-stage per-sample total and its batch reduction are the kernels of element_grad.h;
// this unit holds their form, AnisoForm<DIM>, next to the table and the assembly.
#include "common.h"
#include "element_grad.h"
#include "launch.h"

namespace {

using namespace diffhe;

// ---------------------------------------------------------------------------------------
// Gradient table: the cofactor arithmetic and the degenerate-element rules of tri_integrals / tet_integrals (ell_assemble.hip).
// A degenerate element gets zero gradients and zero size: it contributes nothing.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aniso_table_kernel(const double* __restrict__ coords, const int* __restrict__ elems,
                                                           int dim, int n, int m, double* __restrict__ gtab,
                                                           double* __restrict__ vol) {
#pragma clang fp contract(off)
  for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (i64)gridDim.x * blockDim.x) {
    if (dim == 2) {
      const int i = elems[e], j = elems[(i64)m + e], k = elems[2 * (i64)m + e];
      const double xi = coords[i], yi = coords[(i64)n + i];
      const double xj = coords[j], yj = coords[(i64)n + j];
      const double xk = coords[k], yk = coords[(i64)n + k];
      const double area = 0.5 * fabs((xj - xi) * (yk - yi) - (xk - xi) * (yj - yi));
      const double bb[3] = {yj - yk, yk - yi, yi - yj};
      const double cc[3] = {xk - xj, xi - xk, xj - xi};
      const bool keep = !(area < 1e-15);
      // grad phi_p = (b_p, c_p) / det; the sign of det cancels in every product of two gradients
      const double inv = keep ? 1.0 / (2.0 * area) : 0.0;
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        gtab[(i64)(2 * p) * m + e] = bb[p] * inv;
        gtab[(i64)(2 * p + 1) * m + e] = cc[p] * inv;
      }
      vol[e] = keep ? area : 0.0;
    } else {
      const double* X = coords;
      const double* Y = coords + n;
      const double* Z = coords + 2 * (i64)n;
      const int v0 = elems[e], v1 = elems[(i64)m + e], v2 = elems[2 * (i64)m + e], v3 = elems[3 * (i64)m + e];
      const double x0 = X[v0], y0 = Y[v0], z0 = Z[v0];
      const double ax = X[v1] - x0, ay = Y[v1] - y0, az = Z[v1] - z0;
      const double bx = X[v2] - x0, by = Y[v2] - y0, bz = Z[v2] - z0;
      const double cx = X[v3] - x0, cy = Y[v3] - y0, cz = Z[v3] - z0;
      double g[4][3];
      g[1][0] = by * cz - bz * cy; g[1][1] = bz * cx - bx * cz; g[1][2] = bx * cy - by * cx;
      g[2][0] = cy * az - cz * ay; g[2][1] = cz * ax - cx * az; g[2][2] = cx * ay - cy * ax;
      g[3][0] = ay * bz - az * by; g[3][1] = az * bx - ax * bz; g[3][2] = ax * by - ay * bx;
#pragma unroll
      for (int d = 0; d < 3; ++d) g[0][d] = -((g[1][d] + g[2][d]) + g[3][d]);
      const double det = ax * g[1][0] + ay * g[1][1] + az * g[1][2];
      const double la = ax * ax + ay * ay + az * az, lb = bx * bx + by * by + bz * bz, lc = cx * cx + cy * cy + cz * cz;
      const double l2 = fmax(fmax(la, lb), lc);
      const bool keep = fabs(det) > 1e-12 * (l2 * sqrt(l2));
      const double inv = keep ? 1.0 / fabs(det) : 0.0;   // g_p = 6 V grad phi_p up to the sign of det, which cancels
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int d = 0; d < 3; ++d) gtab[(i64)(3 * p + d) * m + e] = g[p][d] * inv;
      vol[e] = keep ? fabs(det) / 6.0 : 0.0;
    }
  }
}

// s * sym_c(a (x) b) for every Voigt component c
template <int DIM>
__device__ __forceinline__ void sym_products(const double* a, const double* b, double s, double* w) {
  if constexpr (DIM == 2) {
    w[0] = s * (a[0] * b[0]);
    w[1] = s * (a[1] * b[1]);
    w[2] = s * (a[0] * b[1] + a[1] * b[0]);
  } else {
    w[0] = s * (a[0] * b[0]);
    w[1] = s * (a[1] * b[1]);
    w[2] = s * (a[2] * b[2]);
    w[3] = s * (a[1] * b[2] + a[2] * b[1]);
    w[4] = s * (a[0] * b[2] + a[2] * b[0]);
    w[5] = s * (a[0] * b[1] + a[1] * b[0]);
  }
}

// ---------------------------------------------------------------------------------------
// Deterministic row-gather assembly over the plan's ent_ptr / contrib / cols lists, with the Dirichlet handling of
// assemble_rows_kernel (ell_assemble.hip): identity rows, lift = sum K[free, bc] g, couplings to Dirichlet columns zeroed.
// The pattern must hold EVERY coupling of the connectivity (a tensor fills the entries a scalar kappa leaves exactly
// zero on axis-aligned tetrahedra: diffhe/plan.py keeps an unpruned plan for tensor solves).
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void aniso_assemble_rows_kernel(
    const double* __restrict__ gtab, const double* __restrict__ vol, const double* __restrict__ K, i64 ksc, i64 kse,
    i64 ksb, const int* __restrict__ ent_ptr, const int* __restrict__ contrib, const int* __restrict__ cols,
    const unsigned char* __restrict__ is_bc, const double* __restrict__ g, double* __restrict__ vals,
    double* __restrict__ lift, int n, int m, int W, int Bv) {
  constexpr int NPE = DIM + 1, NC = DIM * (DIM + 1) / 2;
  const NodeMap nm = node_map(Bv);
  if (nm.b >= Bv) return;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const bool row_bc = is_bc && is_bc[i];
    double lf = 0.0;
    for (int k = 0; k < W; ++k) {
      const i64 ent = (i64)k * n + i;
      const int j = cols[ent];
      const bool col_bc = is_bc && j != i && is_bc[j];
      const int c0 = ent_ptr[ent], c1 = ent_ptr[ent + 1];
      double v = 0.0;
      for (int c = c0; c < c1; ++c) {
        const int code = contrib[c];
        const int e = code >> 6, pq = code & 63;
        const int p = pq / NPE, q = pq % NPE;
        double gp[DIM], gq[DIM], w[NC];
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          gp[d] = gtab[(i64)(p * DIM + d) * m + e];
          gq[d] = gtab[(i64)(q * DIM + d) * m + e];
        }
        sym_products<DIM>(gp, gq, vol[e], w);
        const double* __restrict__ Ke = K + (i64)e * kse + (i64)nm.b * ksb;
#pragma unroll
        for (int t = 0; t < NC; ++t) v = fma(w[t], Ke[(i64)t * ksc], v);
      }
      if (row_bc) {
        v = (k == 0) ? 1.0 : 0.0;
      } else if (col_bc) {
        lf += v * g[j];
        v = 0.0;
      }
      vals[((i64)k * n + i) * Bv + nm.b] = v;
    }
    if (lift) lift[(i64)i * Bv + nm.b] = lf;
  }
}

// ---------------------------------------------------------------------------------------
// dL/dK: the form of element_grad.h.  Per element the nodes, their Dirichlet values (0 without data), the gradients g_p
// and |e|; per sample grad lambda and grad u, then the NC products -|e| sym_c(grad lambda (x) grad u).
// ---------------------------------------------------------------------------------------
template <int DIM>
struct AnisoForm {
  static constexpr int NPE = DIM + 1, NC = DIM * (DIM + 1) / 2;
  const int* __restrict__ elems;
  const double* __restrict__ gtab;
  const double* __restrict__ vol;
  const double* __restrict__ lam;
  const double* __restrict__ u;
  const double* __restrict__ g;
  int m;

  struct Elem {
    int node[NPE];
    double G[NPE][DIM], gq[NPE], ve;
  };

  __device__ __forceinline__ void load(int e, Elem& el) const {
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
      el.node[p] = elems[(i64)p * m + e];
      el.gq[p] = g ? g[el.node[p]] : 0.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d) el.G[p][d] = gtab[(i64)(p * DIM + d) * m + e];
    }
    el.ve = vol[e];
  }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* dk) const {
    double gl[DIM], gu[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) gl[d] = gu[d] = 0.0;
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
      const i64 o = (i64)el.node[p] * Bp + b;
      const double lp = lam[o];
      const double up = u[o] + el.gq[p];   // full u: Dirichlet values included, as KappaForm adds them
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        gl[d] = fma(lp, el.G[p][d], gl[d]);
        gu[d] = fma(up, el.G[p][d], gu[d]);
      }
    }
    sym_products<DIM>(gl, gu, -el.ve, dk);
  }
};

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" int diffhe_aniso_gradient_table(const double* coords, const int* elems, int dim, int n, int m, double* gtab,
                                           double* vol, void* stream) {
  if (!coords || !elems || !gtab || !vol || (dim != 2 && dim != 3) || n < 1 || m < 1) return DIFFHE_E_BADARG;
  int blocks = (m + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(aniso_table_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, coords, elems, dim, n, m, gtab,
                     vol);
  return diffhe::check_launch();
}

extern "C" int diffhe_aniso_assemble_rows(const double* gtab, const double* vol, int dim, const double* K,
                                          long long k_sc, long long k_se, long long k_sb, const int* ent_ptr,
                                          const int* contrib, const int* cols, const unsigned char* is_bc,
                                          const double* g, double* vals, double* lift, int n, int m, int W, int Bv,
                                          void* stream) {
  if (!gtab || !vol || !K || !ent_ptr || !contrib || !cols || !vals || (dim != 2 && dim != 3) || n < 1 || m < 1 || W < 1)
    return DIFFHE_E_BADARG;
  if (is_bc && !g) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  const int nc = dim == 2 ? 3 : 6;
  diffhe::account(8.0 * Bv * ((double)W * n + (lift ? n : 0) + (k_se ? (double)nc * m : 0)));  // values, lift, tensor field
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(aniso_assemble_rows_kernel<D()>, diffhe::node_grid(n, Bv), dim3(256), 0, (hipStream_t)stream, gtab,
                       vol, K, k_sc, k_se, k_sb, ent_ptr, contrib, cols, is_bc, g, vals, lift, n, m, W, Bv);
  });
  return diffhe::check_launch();
}

extern "C" int diffhe_aniso_grad(const int* elems, const double* gtab, const double* vol, int dim, const double* lam,
                                 const double* u, const double* g, int n, int m, int Bp, double* dk_e, long long o_sc,
                                 long long o_se, double* dk_part, double* dk_sum, void* stream) {
  if (!elems || !gtab || !vol || !lam || !u || (dim != 2 && dim != 3) || n < 1 || m < 1) return DIFFHE_E_BADARG;
  if (!dk_e && !dk_part) return DIFFHE_E_BADARG;
  if ((dk_part == nullptr) != (dk_sum == nullptr)) return DIFFHE_E_BADARG;
  const int nc = dim == 2 ? 3 : 6;
  const double bytes = 8.0 * Bp * (2.0 * n + (dk_e ? (double)nc * m : 0));  // lambda and u once per node, dK per element
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return diffhe::launch_element_grad(AnisoForm<D()>{elems, gtab, vol, lam, u, g, m}, m, Bp, dk_e, o_sc, o_se, dk_part,
                                       dk_sum, bytes, stream);
  });
}

extern "C" int diffhe_aniso_grad_shared(const int* elems, const double* gtab, const double* vol, int dim,
                                        const double* lam, const double* u, const double* g, int n, int m, int B, int Bp,
                                        double* dk, long long o_sc, long long o_se, void* stream) {
  if (!elems || !gtab || !vol || !lam || !u || !dk || (dim != 2 && dim != 3) || n < 1 || m < 1 || B < 1 || B > Bp)
    return DIFFHE_E_BADARG;
  const int nc = dim == 2 ? 3 : 6;
  const double bytes = 8.0 * (Bp * 2.0 * n + (double)nc * m);
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return diffhe::launch_element_grad_shared(AnisoForm<D()>{elems, gtab, vol, lam, u, g, m}, m, B, Bp, dk, o_sc, o_se,
                                              bytes, stream);
  });
}
