// Shape derivative of a P1 solve: dL/dX for the node coordinates X (ours: the reference detaches b and c in 2D,
// solver.py:125-134).  With R = K(X) u - F(X) + c M_L(X) u = 0 on the free rows and the adjoint lambda (0 on Dirichlet
// nodes), element e with size A_e (length, area, volume) and constant grad phi_i adds to its vertex i
//
//   g_i += A_e [ (q_e - tr T_e) I + T_e + T_e^T ] grad phi_i,
//   T_e = sum_b kappa_eb grad u_eb (x) grad lambda_eb,
//   q_e = sum_b [ load_eb - c sum_p lambda_pb u_pb / (d+1) ],
//   load_eb = (sum_p lambda_pb)(sum_p f_pb) / (d+1)^2     (2D, 3D: F_p = A_e/(d+1) * mean f, the m0 of ell_assemble.hip)
//           = sum_p lambda_pb f_pb / 2                     (1D: the reference's trapezoid F_i = h/2 f_i).
//
// Two passes, no floating-point atomics (bitwise reproducible):
//   shape_elem_kernel: one group of LB lanes per element reduces its samples (lanes over samples, LB = min(Bp, 64), when
//     the batch is innermost; LB = 1 -- one element per lane and a sample loop -- otherwise or for B = 1) to the d^2 + 1
//     numbers T_e, q_e and writes the (d+1) d vertex contributions to work (m, (d+1) d);
//   shape_gather_kernel (shape_gather.h, shared with elastic_shape.hip): per node, the contributions of its incident
//     (element, vertex) pairs in the fixed order of the incidence list (diffhe/plan.py: SolvePlan.shape_incidence).
#include "shape_gather.h"
#include "launch.h"

namespace {

using namespace diffhe;

// grad phi_p (G[p][k]) and the element size of a P1 simplex; false for a degenerate element, with the thresholds of the
// assembly (ell_assemble.hip: tri_integrals area < 1e-15, tet_integrals |det| <= 1e-12 l^3; a zero-length segment in 1D).
template <int D>
__device__ inline bool simplex_geometry(const double* __restrict__ coords, int n, const int* v, double (*G)[D],
                                        double* size) {
  if constexpr (D == 1) {
    const double h = coords[v[1]] - coords[v[0]];
    if (h == 0.0) return false;
    G[0][0] = -1.0 / h;
    G[1][0] = 1.0 / h;
    *size = fabs(h);
    return true;
  } else if constexpr (D == 2) {
    const double xi = coords[v[0]], yi = coords[(i64)n + v[0]];
    const double xj = coords[v[1]], yj = coords[(i64)n + v[1]];
    const double xk = coords[v[2]], yk = coords[(i64)n + v[2]];
    const double det = (xj - xi) * (yk - yi) - (xk - xi) * (yj - yi);
    const double area = 0.5 * fabs(det);
    if (area < 1e-15) return false;
    const double inv = 1.0 / det;
    const double bb[3] = {yj - yk, yk - yi, yi - yj};
    const double cc[3] = {xk - xj, xi - xk, xj - xi};
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      G[p][0] = bb[p] * inv;
      G[p][1] = cc[p] * inv;
    }
    *size = area;
    return true;
  } else {
    const double* X = coords;
    const double* Y = coords + n;
    const double* Z = coords + 2 * (i64)n;
    const double x0 = X[v[0]], y0 = Y[v[0]], z0 = Z[v[0]];
    const double ax = X[v[1]] - x0, ay = Y[v[1]] - y0, az = Z[v[1]] - z0;
    const double bx = X[v[2]] - x0, by = Y[v[2]] - y0, bz = Z[v[2]] - z0;
    const double cx = X[v[3]] - x0, cy = Y[v[3]] - y0, cz = Z[v[3]] - z0;
    double g[4][3];
    g[1][0] = by * cz - bz * cy; g[1][1] = bz * cx - bx * cz; g[1][2] = bx * cy - by * cx;
    g[2][0] = cy * az - cz * ay; g[2][1] = cz * ax - cx * az; g[2][2] = cx * ay - cy * ax;
    g[3][0] = ay * bz - az * by; g[3][1] = az * bx - ax * bz; g[3][2] = ax * by - ay * bx;
#pragma unroll
    for (int d = 0; d < 3; ++d) g[0][d] = -((g[1][d] + g[2][d]) + g[3][d]);
    const double det = ax * g[1][0] + ay * g[1][1] + az * g[1][2];
    const double la = ax * ax + ay * ay + az * az, lb = bx * bx + by * by + bz * bz, lc = cx * cx + cy * cy + cz * cz;
    const double l2 = fmax(fmax(la, lb), lc);
    if (!(fabs(det) > 1e-12 * (l2 * sqrt(l2)))) return false;
    const double inv = 1.0 / det;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int d = 0; d < 3; ++d) G[p][d] = g[p][d] * inv;
    *size = fabs(det) / 6.0;
    return true;
  }
}

template <int D>
__global__ __launch_bounds__(256) void shape_elem_kernel(const double* __restrict__ coords, const int* __restrict__ elems,
                                                         int n, int m, int B, int LB, const double* __restrict__ u,
                                                         const double* __restrict__ g, const double* __restrict__ lam,
                                                         i64 sn, i64 sb, const double* __restrict__ kappa, i64 kse,
                                                         i64 ksb, const double* __restrict__ f, i64 fsn, i64 fsb,
                                                         double c, double* __restrict__ work) {
  constexpr int NPE = D + 1, NC = NPE * D;
  const GroupMap gm = group_map(LB);               // a group of LB lanes per element
  const int sub = gm.sub;
  for (i64 e = gm.item0; e < m; e += gm.stride) {
    int v[NPE];
#pragma unroll
    for (int p = 0; p < NPE; ++p) v[p] = elems[(i64)p * m + e];
    double G[NPE][D], size;
    double* out = work + e * NC;
    if (!simplex_geometry<D>(coords, n, v, G, &size)) {     // degenerate: contributes nothing
      for (int ci = sub; ci < NC; ci += LB) out[ci] = 0.0;
      continue;
    }
    double gv[NPE];
#pragma unroll
    for (int p = 0; p < NPE; ++p) gv[p] = g ? g[v[p]] : 0.0;
    double T[D][D], q = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int k = 0; k < D; ++k) T[a][k] = 0.0;
    for (int b = sub; b < B; b += LB) {             // padding samples (b >= B) carry no gradient
      double up[NPE], lp[NPE];
#pragma unroll
      for (int p = 0; p < NPE; ++p) {
        const i64 o = (i64)v[p] * sn + (i64)b * sb;
        up[p] = u[o] + gv[p];                        // full u: Dirichlet values included
        lp[p] = lam[o];
      }
      double gu[D], gl[D];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        gu[k] = 0.0;
        gl[k] = 0.0;
#pragma unroll
        for (int p = 0; p < NPE; ++p) {
          gu[k] += up[p] * G[p][k];
          gl[k] += lp[p] * G[p][k];
        }
      }
      const double kap = kappa[e * kse + (i64)b * ksb];
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int k = 0; k < D; ++k) T[a][k] += kap * gu[a] * gl[k];
      double lu = 0.0;
#pragma unroll
      for (int p = 0; p < NPE; ++p) lu += lp[p] * up[p];
      double load = 0.0;
      if (f) {
        double fp[NPE];
#pragma unroll
        for (int p = 0; p < NPE; ++p) fp[p] = f[(i64)v[p] * fsn + (i64)b * fsb];
        if constexpr (D == 1) {
          load = 0.5 * (lp[0] * fp[0] + lp[1] * fp[1]);
        } else {
          double sl = 0.0, sf = 0.0;
#pragma unroll
          for (int p = 0; p < NPE; ++p) {
            sl += lp[p];
            sf += fp[p];
          }
          load = sl * sf / (double)(NPE * NPE);
        }
      }
      q += load - c * lu / (double)NPE;
    }
    group_sum(LB, q, T);
    double tr = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) tr += T[a][a];
#pragma unroll
    for (int ci = 0; ci < NC; ++ci) {                // component ci = p d + k, written by lane ci % LB of the group
      if (ci % LB != sub) continue;
      const int p = ci / D, k = ci % D;
      double s = (q - tr) * G[p][k];
#pragma unroll
      for (int j = 0; j < D; ++j) s += (T[k][j] + T[j][k]) * G[p][j];
      out[ci] = size * s;
    }
  }
}

}  // namespace

extern "C" int diffhe_p1_shape_grad(const double* coords, const int* elems, int dim, int n, int m, int B,
                                    const double* u, const double* g, const double* lam, long long sn, long long sb,
                                    const double* kappa, long long kse, long long ksb, const double* f, long long fsn,
                                    long long fsb, double c, const int* inc_ptr, const int* inc, double* work,
                                    double* grad, void* stream) {
  if (!coords || !elems || !u || !lam || !kappa || !inc_ptr || !inc || !work || !grad || dim < 1 || dim > 3 || n < 1 ||
      m < 1 || B < 1 || sn < 0 || sb < 0 || kse < 0 || ksb < 0 || fsn < 0 || fsb < 0 || (long long)m * (dim + 1) >= (1LL << 31))
    return DIFFHE_E_BADARG;
  // lanes over samples when they are contiguous in memory, one element per lane otherwise
  const int LB = sb == 1 ? group_lanes(B) : 1;
  // algorithmic bytes: u and lambda once, f once (batch-shared: one row), coords, the gradient
  account(8.0 * (2.0 * n * B + (f ? (fsb ? (double)n * B : (double)n) : 0.0) + 2.0 * dim * n));
  hipStream_t st = (hipStream_t)stream;
  dispatch_dim<1, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(shape_elem_kernel<D()>, dim3(group_grid(m, LB, 8192)), dim3(256), 0, st, coords, elems, n, m, B, LB,
                       u, g, lam, sn, sb, kappa, kse, ksb, f, fsn, fsb, c, work);
  });
  launch_shape_gather(inc_ptr, inc, work, n, dim, grad, st);
  return check_launch();
}
