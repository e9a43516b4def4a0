// Sampling of nodal P1 fields at arbitrary points of a mesh, with the exact transpose (ours: the reference compares
// fields at mesh nodes only), include/diffhe_sample.h:
//
//   diffhe_sample_locate:  the element of every point -- the candidate of the 3^dim cells around the point's cell with the
//                          largest smallest barycentric coordinate, ties to the lowest id --, its dim + 1 weights and the
//                          dim x (dim + 1) table of the shape-function gradients of that element;
//   diffhe_sample_apply:   y[p, r, c, b] = sum_k W[p, r, k] u[el[e_p, k], c, b], the values (W the weights, R = 1) or the
//                          piecewise-constant spatial gradient (W the gradient table, R = dim);
//   diffhe_sample_adjoint: the transpose as a gather over a node -> (point, vertex slot) incidence list.
//
// The barycentric coordinates of a candidate are one fixed chain of fma on the edge vectors x_k - x_0 and x - x_0, and the
// choice among candidates is a maximum with a total order (the smallest coordinate, then the id), so the result does not
// depend on the order in which the cells are scanned.  Every sum of the apply and of the adjoint runs in a fixed order
// with explicit fma and every output entry has one writer: every result is a function of the mesh, the points and tol
// alone, bit for bit, whatever the binning, the batch, the layout or the thread mapping.
//
// The apply and the adjoint map lanes over samples (node_map of common.h): from 64 samples on, the point (or node), its
// element, vertex ids and weights are uniform over the wave and the vector work is one contiguous load per vertex.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "diffhe_sample.h"
#include "launch.h"
#include "cell_grid.h"

namespace {

using namespace diffhe;

// G[r][k - 1] = det * d phi_k / d x_r for k = 1 .. DIM (the cofactors of the edge matrix) and det, from the edge vectors
// E[k - 1][r] = x_k[r] - x_0[r]
template <int DIM>
__device__ inline double cofactors(const double (*E)[DIM], double (*G)[DIM]) {
  if constexpr (DIM == 1) {
    G[0][0] = 1.0;
    return E[0][0];
  } else if constexpr (DIM == 2) {
    G[0][0] = E[1][1];
    G[1][0] = -E[1][0];
    G[0][1] = -E[0][1];
    G[1][1] = E[0][0];
    return fma(E[0][0], E[1][1], -(E[0][1] * E[1][0]));
  } else {
    // g_1 = e_2 x e_3, g_2 = e_3 x e_1, g_3 = e_1 x e_2
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double* a = E[(k + 1) % 3];
      const double* b = E[(k + 2) % 3];
      G[0][k] = fma(a[1], b[2], -(a[2] * b[1]));
      G[1][k] = fma(a[2], b[0], -(a[0] * b[2]));
      G[2][k] = fma(a[0], b[1], -(a[1] * b[0]));
    }
    return fma(E[0][2], G[2][0], fma(E[0][1], G[1][0], E[0][0] * G[0][0]));
  }
}

// the candidate e for the point x: lam[0 .. DIM] and, with GRAD, grad[r][k] = d phi_k / d x_r; returns min_k lam[k]
template <int DIM, bool GRAD>
__device__ inline double barycentric(const double* __restrict__ X, const int* __restrict__ el, int e, const double* x,
                                     double* lam, double (*grad)[DIM + 1]) {
  const int* v = el + (i64)e * (DIM + 1);
  double x0[DIM], E[DIM][DIM], G[DIM][DIM], r[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    x0[a] = X[(i64)v[0] * DIM + a];
    r[a] = x[a] - x0[a];
  }
#pragma unroll
  for (int k = 0; k < DIM; ++k)
#pragma unroll
    for (int a = 0; a < DIM; ++a) E[k][a] = X[(i64)v[k + 1] * DIM + a] - x0[a];
  const double det = cofactors<DIM>(E, G);
  double l0 = 1.0, mn = INFINITY;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    double s = r[0] * G[0][k];
#pragma unroll
    for (int a = 1; a < DIM; ++a) s = fma(r[a], G[a][k], s);
    const double l = s / det;
    lam[k + 1] = l;
    l0 -= l;
    mn = l < mn ? l : mn;
  }
  lam[0] = l0;
  mn = l0 < mn ? l0 : mn;
  if constexpr (GRAD) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      double g0 = 0.0;
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        const double g = G[a][k] / det;
        grad[a][k + 1] = g;
        g0 -= g;
      }
      grad[a][0] = g0;
    }
  }
  return mn;                                                   // a degenerate element gives NaN: never chosen below
}

// one thread per point, taken in cell order so that a wave scans the same cells
template <int DIM>
__global__ __launch_bounds__(256) void sample_locate_kernel(const double* __restrict__ X, const int* __restrict__ el,
                                                            const int* __restrict__ order,
                                                            const int* __restrict__ cell_start, Grid g,
                                                            const double* __restrict__ pts, const int* __restrict__ pcell,
                                                            const int* __restrict__ porder, int P, double tol,
                                                            int* __restrict__ element, double* __restrict__ weights,
                                                            double* __restrict__ gtab, int* __restrict__ tested) {
  const int n_cells = g.ncx * g.ncy * g.ncz;
  for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < P; t += (i64)gridDim.x * blockDim.x) {
    const int p = porder[t];
    double x[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) x[a] = pts[(i64)p * DIM + a];
    int c = pcell[p];
    c = c < 0 ? 0 : (c >= n_cells ? n_cells - 1 : c);          // the point's cell, clamped into the grid
    int best = -1, cnt = 0;
    double best_min = -INFINITY;
    for_each_neighbour_row<DIM>(g, c, [&](i64 c0, i64 c1) {
      for (int q = cell_start[c0]; q < cell_start[c1 + 1]; ++q) {
        const int e = order[q];
        double lam[DIM + 1];
        const double mn = barycentric<DIM, false>(X, el, e, x, lam, nullptr);
        ++cnt;
        if (mn > best_min || (mn == best_min && e < best)) {
          best = e;
          best_min = mn;
        }
      }
    });
    const bool in = best >= 0 && best_min >= -tol;
    double best_lam[DIM + 1] = {}, best_grad[DIM][DIM + 1] = {};
    if (in) barycentric<DIM, true>(X, el, best, x, best_lam, best_grad);    // the same chain again: the same bits
    element[p] = in ? best : -1;
    tested[p] = cnt;
#pragma unroll
    for (int k = 0; k <= DIM; ++k) weights[(i64)p * (DIM + 1) + k] = in ? best_lam[k] : 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int k = 0; k <= DIM; ++k) gtab[((i64)p * DIM + a) * (DIM + 1) + k] = in ? best_grad[a][k] : 0.0;
  }
}

// lanes over samples; WAVE (64 lanes per point): the point index is a scalar, and with it the element, its vertex ids and
// the rows of W.  Both forms evaluate the same expressions in the same order: the same bits.
template <int DIM, bool WAVE>
__global__ __launch_bounds__(256) void sample_apply_kernel(const int* __restrict__ el, const int* __restrict__ element,
                                                           const double* __restrict__ W, int R, int P,
                                                           const double* __restrict__ u, i64 usn, i64 usc, i64 usb,
                                                           double* __restrict__ y, i64 ysp, i64 ysr, i64 ysc, i64 ysb,
                                                           int C, int B, int Bp) {
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < B;                                   // guard lanes of the padded batch: no load, no store
  const i64 ub = (i64)nm.b * usb, yb = (i64)nm.b * ysb;
  for (int p0 = nm.node0; p0 < P; p0 += nm.stride) {
    const int p = WAVE ? __builtin_amdgcn_readfirstlane(p0) : p0;
    const int e = element[p];
    i64 v[DIM + 1] = {};
    if (e >= 0) {                                             // an outside point reads no u
#pragma unroll
      for (int k = 0; k <= DIM; ++k) v[k] = (i64)el[(i64)e * (DIM + 1) + k] * usn;
    }
    for (int c = 0; c < C; ++c) {
      double uv[DIM + 1];
#pragma unroll
      for (int k = 0; k <= DIM; ++k) uv[k] = (ok && e >= 0) ? u[v[k] + c * usc + ub] : 0.0;
      for (int r = 0; r < R; ++r) {
        const double* w = W + ((i64)p * R + r) * (DIM + 1);
        double acc = 0.0;
        if (e >= 0) {
          acc = w[0] * uv[0];
#pragma unroll
          for (int k = 1; k <= DIM; ++k) acc = fma(w[k], uv[k], acc);
        }
        if (ok) y[(i64)p * ysp + r * ysr + c * ysc + yb] = acc;
      }
    }
  }
}

// lanes over samples, one node per wave (or per group of Bp lanes): the row of the node in ascending order of its entries,
// and the rows r of W within an entry; up to three components are carried at once so that the row is read once.
// `rows` (count of them) restricts the launch to those nodes; NULL: all count = n nodes
template <int DIM, bool WAVE>
__global__ __launch_bounds__(256) void sample_adjoint_kernel(const i64* __restrict__ row_ptr,
                                                             const int* __restrict__ entries,
                                                             const int* __restrict__ rows, int count,
                                                             const double* __restrict__ W, int R,
                                                             const double* __restrict__ g, i64 gsp, i64 gsr, i64 gsc,
                                                             i64 gsb, double* __restrict__ out, i64 osn, i64 osc, i64 osb,
                                                             int C, int B, int Bp) {
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < B;
  const i64 gb = (i64)nm.b * gsb, ob = (i64)nm.b * osb;
  for (int t0 = nm.node0; t0 < count; t0 += nm.stride) {
    const int t = WAVE ? __builtin_amdgcn_readfirstlane(t0) : t0;
    const int i = rows ? rows[t] : t;
    const i64 q0 = row_ptr[i], q1 = row_ptr[i + 1];
    double acc[3] = {0.0, 0.0, 0.0};
    for (i64 q = q0; q < q1; ++q) {
      const int j = entries[q];
      const int p = j / (DIM + 1), k = j - p * (DIM + 1);
      for (int r = 0; r < R; ++r) {
        const double w = W[((i64)p * R + r) * (DIM + 1) + k];
        const i64 at = (i64)p * gsp + r * gsr + gb;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (c < C && ok) acc[c] = fma(w, g[at + c * gsc], acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c < C && ok) out[(i64)i * osn + c * osc + ob] = acc[c];
  }
}

inline unsigned point_blocks(int P) {
  i64 gx = ((i64)P + 255) / 256;
  return (unsigned)(gx > 65536 ? 65536 : gx);
}

inline bool bad_batch(int dim, int R, int C, int B) {
  return dim < 1 || dim > 3 || (R != 1 && R != dim) || C < 1 || C > 3 || B < 1 || (B + kWave - 1) / kWave > 65535;
}

// whether the spans [a, a + a_last] and [b, b + b_last] of two strided arrays meet (all strides >= 0)
inline bool overlap(const double* a, i64 a_last, const double* b, i64 b_last) {
  return a <= b + b_last && b <= a + a_last;
}

// f(D, WAVE) for the dimension and for whether the padded batch Bp fills whole waves
template <class F>
void dispatch_apply(int dim, int Bp, F&& f) {
  dispatch_dim<1, 3>(dim, [&](auto D) { dispatch_bool(Bp >= kWave, [&](auto WAVE) { f(D, WAVE); }); });
}

}  // namespace

extern "C" int diffhe_sample_locate(const double* X, const int* el, int dim, int n, int m, const int* order,
                                    const int* cell_start, int ncx, int ncy, int ncz, const double* pts, const int* pcell,
                                    const int* porder, int P, double tol, int* element, double* weights, double* gtab,
                                    int* tested, void* stream) {
  if (!X || !el || !order || !cell_start || !pts || !pcell || !porder || !element || !weights || !gtab || !tested ||
      weights == gtab || element == tested || dim < 1 || dim > 3 || n < 2 || m < 1 || P < 1 ||
      bad_grid(dim, ncx, ncy, ncz) || !(tol >= 0.0) || !(tol < INFINITY))
    return DIFFHE_E_BADARG;
  // the points and the three tables of a point; the candidates are shared by the points of a cell
  account((8.0 * dim + 8.0 + 4.0 + 4.0 + 8.0 * (dim + 1) * (dim + 1)) * P);
  dispatch_dim<1, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(sample_locate_kernel<D()>, dim3(point_blocks(P)), dim3(256), 0, (hipStream_t)stream, X, el, order,
                       cell_start, Grid{ncx, ncy, ncz}, pts, pcell, porder, P, tol, element, weights, gtab, tested);
  });
  return check_launch();
}

extern "C" int diffhe_sample_apply(const int* el, int dim, int n, const int* element, const double* W, int R, int P,
                                   const double* u, long long u_sn, long long u_sc, long long u_sb, double* y,
                                   long long y_sp, long long y_sr, long long y_sc, long long y_sb, int C, int B,
                                   void* stream) {
  if (!el || !element || !W || !u || !y || bad_batch(dim, R, C, B) || n < 2 || P < 1 || u_sn < 0 || u_sc < 0 || u_sb < 0 ||
      y_sp < 0 || y_sr < 0 || y_sc < 0 || y_sb < 0 ||
      overlap(u, (n - 1) * u_sn + (C - 1) * u_sc + (B - 1) * u_sb, y,
              (P - 1) * y_sp + (R - 1) * y_sr + (C - 1) * y_sc + (B - 1) * y_sb))
    return DIFFHE_E_BADARG;
  // per point, component and sample: dim + 1 values read, R written
  account(8.0 * P * C * B * (dim + 1 + R));
  const int Bp = batch_pad(B);
  dispatch_apply(dim, Bp, [&](auto D, auto WAVE) {
    hipLaunchKernelGGL((sample_apply_kernel<D(), WAVE()>), node_grid(P, Bp, 65536), dim3(256), 0, (hipStream_t)stream, el,
                       element, W, R, P, u, u_sn, u_sc, u_sb, y, y_sp, y_sr, y_sc, y_sb, C, B, Bp);
  });
  return check_launch();
}

extern "C" int diffhe_sample_adjoint(const long long* row_ptr, const int* entries, const int* rows, int n_rows, int dim,
                                     int n, const double* W, int R, int P, const double* g, long long g_sp,
                                     long long g_sr, long long g_sc, long long g_sb, double* out, long long o_sn,
                                     long long o_sc, long long o_sb, int C, int B, void* stream) {
  if (!row_ptr || !entries || !W || !g || !out || bad_batch(dim, R, C, B) || n < 2 || P < 1 || g_sp < 0 || g_sr < 0 ||
      g_sc < 0 || g_sb < 0 || o_sn < 0 || o_sc < 0 || o_sb < 0 || (rows ? n_rows < 1 || n_rows > n : n_rows != 0) ||
      overlap(g, (P - 1) * g_sp + (R - 1) * g_sr + (C - 1) * g_sc + (B - 1) * g_sb, out,
              (n - 1) * o_sn + (C - 1) * o_sc + (B - 1) * o_sb))
    return DIFFHE_E_BADARG;
  const int count = rows ? n_rows : n;
  // the point data read once per vertex slot, every visited nodal entry written once
  account(8.0 * C * B * ((double)P * R * (dim + 1) + count));
  const int Bp = batch_pad(B);
  dispatch_apply(dim, Bp, [&](auto D, auto WAVE) {
    hipLaunchKernelGGL((sample_adjoint_kernel<D(), WAVE()>), node_grid(count, Bp, 65536), dim3(256), 0,
                       (hipStream_t)stream, row_ptr, entries, rows, count, W, R, g, g_sp, g_sr, g_sc, g_sb, out, o_sn, o_sc,
                       o_sb, C, B, Bp);
  });
  return check_launch();
}
