// The node pass of a stress adjoint whose dL/dH is a symmetric tensor per element, as stress.hip and
// elastic_aniso_stress.hip launch it: the element pass of either unit leaves T in Voigt components in a work array and this
// kernel gathers T g_p over the per-node incidence list (the list of shape.hip's gather).  Stated once, here.
#pragma once
#include "common.h"
#include "eigen_field.h"
#include "launch.h"

namespace diffhe {
namespace {

// ---------------------------------------------------------------------------------------
// Node pass: u_bar[(i, a), b] = sum over the incidence list of node i (codes e * NPE + p, element order) of
// sum_t T_e[a][t] g_p[t], T (NC, m, Bp).  Samples b >= B: 0.
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void stress_node_kernel(const int* __restrict__ inc_ptr, const int* __restrict__ inc,
                                                           const double* __restrict__ gtab,
                                                           const double* __restrict__ work, int n, int m, int B, int Bp,
                                                           double* __restrict__ u_bar) {
  constexpr int NPE = DIM + 1, NC = DIM * (DIM + 1) / 2;
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
        double T[DIM][DIM];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          const double v = work[k * mb + (i64)e * Bp + nm.b];
          T[voigt_row<DIM>(k)][voigt_col<DIM>(k)] = v;
          T[voigt_col<DIM>(k)][voigt_row<DIM>(k)] = v;
        }
#pragma unroll
        for (int t = 0; t < DIM; ++t) {
          const double g = gtab[(i64)(p * DIM + t) * m + e];
#pragma unroll
          for (int a = 0; a < DIM; ++a) acc[a] = fma(T[a][t], g, acc[a]);
        }
      }
#pragma unroll
    for (int a = 0; a < DIM; ++a) u_bar[((i64)i * DIM + a) * Bp + nm.b] = acc[a];
  }
}

}  // namespace
}  // namespace diffhe
