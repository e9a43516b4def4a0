// Mesh-independent density filter on the elements of any P1 mesh, with its exact adjoint (ours: the reference has no
// design regularisation), include/diffhe_filter.h.  With centroids c, sizes v and a radius R
//
//     N(i) = { j : |c_i - c_j| < R },   w_ij = R - |c_i - c_j| (cone) or 1 (constant),   S_i = sum_j w_ij v_j,
//     forward  y_i = (sum_{j in N(i)} w_ij v_j x_j) / S_i,      adjoint  y_j = v_j sum_{i in N(j)} w_ij x_i / S_i:
//
//   diffhe_filter_count: |N(i)| of every element, searched in the 3^dim cells of a uniform grid around its own;
//   diffhe_filter_fill:  the ids of N(i) in ASCENDING order (a merge of the per-cell runs, each ascending), S_i summed in
//                        that order, and 1 / S_i;
//   diffhe_filter_apply: H x or H^T x for a batch of fields read and written in place through (element, sample) strides.
//
// The table is the ids alone; the weights are recomputed from the two centroids.  |c_i - c_j| is one fma chain over the
// components in a fixed order, bitwise symmetric in (i, j), and N is symmetric, so H^T is a gather over the same rows with
// the same weights: both directions are ONE kernel that scales x_j by pre[j] and the row sum by post[i]
// (forward: pre = v, post = 1 / S; adjoint: pre = 1 / S, post = v).  Every sum runs in ascending j with explicit fma and
// every entry has one writer: every result is a function of the mesh and R alone, bit for bit, whatever the binning, the
// batch, the layout or the thread mapping.
//
// The apply maps lanes over samples (node_map of common.h): with 64 lanes per element the element, its neighbour j, c_j,
// v_j, w_ij and 1 / S_i are uniform over the wave and the vector work is one contiguous load of x[j, :] and one fma per
// neighbour.  A sample-major field is correct through its strides but not coalesced; diffhe/filters.py transposes it.
#include <limits.h>

#include "common.h"
#include "diffhe_filter.h"
#include "launch.h"
#include "cell_grid.h"

namespace {

using namespace diffhe;

template <int DIM>
__device__ inline void load_centroid(const double* __restrict__ cent, int m, i64 e, double* c) {
#pragma unroll
  for (int k = 0; k < DIM; ++k) c[k] = cent[(i64)k * m + e];
}

// |a - b|: (a_k - b_k) = -(b_k - a_k) exactly and the chain runs over k = 0, 1, 2 on both sides: symmetric bit for bit
template <int DIM>
__device__ inline double distance(const double* a, const double* b) {
  double d2 = 0.0;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    const double t = a[k] - b[k];
    d2 = fma(t, t, d2);
  }
  return sqrt(d2);
}

// w_ij of a pair that is in the table
template <int DIM>
__device__ inline double pair_weight(const double* __restrict__ cent, int m, const double* ci, i64 j, double R,
                                     int weight) {
  if (weight) return 1.0;
  double cj[DIM];
  load_centroid<DIM>(cent, m, j, cj);
  return R - distance<DIM>(ci, cj);
}

// one thread per element, taken in cell order so that a wave scans the same cells
template <int DIM>
__global__ __launch_bounds__(256) void filter_count_kernel(const double* __restrict__ cent, int m,
                                                           const int* __restrict__ cell_of, const int* __restrict__ order,
                                                           const int* __restrict__ cell_start, Grid g, double R,
                                                           int* __restrict__ count) {
  for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += (i64)gridDim.x * blockDim.x) {
    const int i = order[t];
    double ci[DIM];
    load_centroid<DIM>(cent, m, i, ci);
    int cnt = 0;
    for_each_neighbour_row<DIM>(g, cell_of[i], [&](i64 c0, i64 c1) {
      for (int p = cell_start[c0]; p < cell_start[c1 + 1]; ++p) {
        double cj[DIM];
        load_centroid<DIM>(cent, m, order[p], cj);
        cnt += distance<DIM>(ci, cj) < R ? 1 : 0;
      }
    });
    count[i] = cnt;
  }
}

// one thread per element: a merge of the (at most 3^DIM) cell runs, each ascending, filtered by the distance
template <int DIM>
__global__ __launch_bounds__(256) void filter_fill_kernel(const double* __restrict__ cent, const double* __restrict__ vol,
                                                          int m, const int* __restrict__ cell_of,
                                                          const int* __restrict__ order, const int* __restrict__ cell_start,
                                                          Grid g, double R, int weight, const i64* __restrict__ row_ptr,
                                                          int* __restrict__ nbr, double* __restrict__ S,
                                                          double* __restrict__ inv_S) {
  constexpr int NR = DIM == 1 ? 3 : (DIM == 2 ? 9 : 27);
  for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += (i64)gridDim.x * blockDim.x) {
    const int i = order[t];
    double ci[DIM];
    load_centroid<DIM>(cent, m, i, ci);
    int pos[NR], end[NR], head[NR], nr = 0;
    for_each_neighbour_cell<DIM>(g, cell_of[i], [&](i64 cc) {
      pos[nr] = cell_start[cc];
      end[nr] = cell_start[cc + 1];
      ++nr;
    });
    // head[r]: the next id of run r that lies inside the radius, INT_MAX once the run is exhausted
    auto advance = [&](int r) {
      int p = pos[r], h = INT_MAX;
      for (; p < end[r]; ++p) {
        const int j = order[p];
        double cj[DIM];
        load_centroid<DIM>(cent, m, j, cj);
        if (distance<DIM>(ci, cj) < R) {
          h = j;
          break;
        }
      }
      pos[r] = p;
      head[r] = h;
    };
    for (int r = 0; r < nr; ++r) advance(r);
    i64 o = row_ptr[i];
    const i64 oe = row_ptr[i + 1];
    double s = 0.0;
    for (;;) {
      int best = INT_MAX, rb = 0;
      for (int r = 0; r < nr; ++r)
        if (head[r] < best) {
          best = head[r];
          rb = r;
        }
      if (best == INT_MAX) break;
      if (o < oe) nbr[o] = best;                              // never past the row the count reserved
      ++o;
      s += pair_weight<DIM>(cent, m, ci, best, R, weight) * (vol ? vol[best] : 1.0);
      ++pos[rb];
      advance(rb);
    }
    S[i] = s;
    inv_S[i] = 1.0 / s;
  }
}

// a double of lane k of the wave (k uniform)
__device__ inline double read_lane(double v, int k) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// lanes over samples: y[e, b] = post[e] sum_{j in N(e)} w_ej pre[j] x[j, b]; a NULL pre / post is all ones.
// WAVE (64 lanes per element): the element index is a scalar and the row is taken 64 neighbours at a time -- lane k
// computes the id and the coefficient w pre[j] of neighbour k, once per wave instead of once per lane, and the sum then
// runs over k in ascending order with both broadcast: per neighbour one contiguous load of x[j, :] and one fma.
// Otherwise (a padded batch Bp below 64: 64 / Bp elements per wave) the Bp lanes of an element do the same among
// themselves, Bp neighbours at a time, broadcast by shuffles.
// Both forms evaluate the same expressions in the same order: the same bits.
template <int DIM, bool WAVE>
__global__ __launch_bounds__(256) void filter_apply_kernel(
    const double* __restrict__ cent, int m, const i64* __restrict__ row_ptr, const int* __restrict__ nbr,
    const double* __restrict__ pre, const double* __restrict__ post, double R, int weight, const double* __restrict__ x,
    i64 xse, i64 xsb, double* __restrict__ y, i64 yse, i64 ysb, int B, int Bp) {
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < B;                                   // guard lanes of the padded batch: no load, no store
  const i64 xb = (i64)nm.b * xsb, yb = (i64)nm.b * ysb;
  const int lane = threadIdx.x & 63;
  for (int e0 = nm.node0; e0 < m; e0 += nm.stride) {
    const int e = WAVE ? __builtin_amdgcn_readfirstlane(e0) : e0;
    double ce[DIM];
    load_centroid<DIM>(cent, m, e, ce);
    const i64 p0 = row_ptr[e], p1 = row_ptr[e + 1];
    double acc = 0.0;
    if constexpr (WAVE) {
      for (i64 base = p0; base < p1; base += kWave) {
        const int cnt = p1 - base < kWave ? (int)(p1 - base) : kWave;
        int jl = 0;
        double cl = 0.0;
        if (lane < cnt) {                                     // every lane, guard lanes included
          jl = nbr[base + lane];
          const double w = pair_weight<DIM>(cent, m, ce, jl, R, weight);
          cl = pre ? w * pre[jl] : w;
        }
        for (int k = 0; k < cnt; k += 4) {                    // four loads in flight; past the end: the last one again, unused
          double coef[4], xv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int kk = k + u < cnt ? k + u : cnt - 1;
            const i64 j = __builtin_amdgcn_readlane(jl, kk);
            coef[u] = read_lane(cl, kk);
            xv[u] = ok ? x[j * xse + xb] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (k + u < cnt) acc = fma(coef[u], xv[u], acc);
        }
      }
    } else {
      // Bp lanes per element: the same scheme inside the group.  All lanes of a group share e, the row and so every
      // trip count, and a shuffle reads lanes of its own group only: it never meets an inactive lane.
      const int sub = lane & (Bp - 1), first = lane - sub;
      for (i64 base = p0; base < p1; base += Bp) {
        const int cnt = p1 - base < Bp ? (int)(p1 - base) : Bp;
        int jl = 0;
        double cl = 0.0;
        if (sub < cnt) {
          jl = nbr[base + sub];
          const double w = pair_weight<DIM>(cent, m, ce, jl, R, weight);
          cl = pre ? w * pre[jl] : w;
        }
        for (int k = 0; k < cnt; ++k) {
          const i64 j = __shfl(jl, first + k);
          const double coef = __shfl(cl, first + k);
          if (ok) acc = fma(coef, x[j * xse + xb], acc);
        }
      }
    }
    if (ok) y[(i64)e * yse + yb] = post ? acc * post[e] : acc;
  }
}

bool bad_search(const double* cent, int dim, int m, const int* cell_of, const int* order, const int* cell_start, int ncx,
                int ncy, int ncz, double R) {
  return !cent || !cell_of || !order || !cell_start || dim < 1 || dim > 3 || m < 1 || bad_grid(dim, ncx, ncy, ncz) ||
         !(R > 0.0) || !(R < INFINITY);
}

inline unsigned element_blocks(int m) {
  i64 gx = ((i64)m + 255) / 256;
  return (unsigned)(gx > 65536 ? 65536 : gx);
}

}  // namespace

extern "C" int diffhe_filter_count(const double* cent, int dim, int m, const int* cell_of, const int* order,
                                   const int* cell_start, int ncx, int ncy, int ncz, double R, int* count, void* stream) {
  if (bad_search(cent, dim, m, cell_of, order, cell_start, ncx, ncy, ncz, R) || !count) return DIFFHE_E_BADARG;
  dispatch_dim<1, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(filter_count_kernel<D()>, dim3(element_blocks(m)), dim3(256), 0, (hipStream_t)stream, cent, m,
                       cell_of, order, cell_start, Grid{ncx, ncy, ncz}, R, count);
  });
  return check_launch();
}

extern "C" int diffhe_filter_fill(const double* cent, const double* vol, int dim, int m, const int* cell_of,
                                  const int* order, const int* cell_start, int ncx, int ncy, int ncz, double R, int weight,
                                  const long long* row_ptr, int* nbr, double* S, double* inv_S, void* stream) {
  if (bad_search(cent, dim, m, cell_of, order, cell_start, ncx, ncy, ncz, R) || !row_ptr || !nbr || !S || !inv_S ||
      (weight != 0 && weight != 1))
    return DIFFHE_E_BADARG;
  dispatch_dim<1, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(filter_fill_kernel<D()>, dim3(element_blocks(m)), dim3(256), 0, (hipStream_t)stream, cent, vol, m,
                       cell_of, order, cell_start, Grid{ncx, ncy, ncz}, R, weight, row_ptr, nbr, S, inv_S);
  });
  return check_launch();
}

extern "C" int diffhe_filter_apply(const double* cent, const double* vol, int dim, int m, const long long* row_ptr,
                                   const int* nbr, const double* inv_S, double R, int weight, int adjoint, const double* x,
                                   long long x_se, long long x_sb, double* y, long long y_se, long long y_sb, int B,
                                   void* stream) {
  if (!cent || !row_ptr || !nbr || !inv_S || !x || !y || x == y || dim < 1 || dim > 3 || m < 1 || !(R > 0.0) ||
      !(R < INFINITY) || (weight != 0 && weight != 1) || (adjoint != 0 && adjoint != 1) || B < 1 || x_se < 0 || x_sb < 0 ||
      y_se < 0 || y_sb < 0 || (B + kWave - 1) / kWave > 65535)
    return DIFFHE_E_BADARG;
  const double* pre = adjoint ? inv_S : vol;
  const double* post = adjoint ? vol : inv_S;
  account(16.0 * m * B);
  const int Bp = batch_pad(B);
  dispatch_dim<1, 3>(dim, [&](auto D) {
    dispatch_bool(Bp >= kWave, [&](auto WAVE) {
      hipLaunchKernelGGL((filter_apply_kernel<D(), WAVE()>), node_grid(m, Bp, 65536), dim3(256), 0, (hipStream_t)stream,
                         cent, m, row_ptr, nbr, pre, post, R, weight, x, x_se, x_sb, y, y_se, y_sb, B, Bp);
    });
  });
  return check_launch();
}
