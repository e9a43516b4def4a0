// The deformation of one element for one sample of the finite-strain units (hyperelastic.hip, hyper_stress.hip):
// F = I + H from the displacement, J, ln J and F^-T, with the first Piola-Kirchhoff stress and the energy of E = 1
// (definitions: include/diffhe_hyperelastic.h).
#pragma once
#include "common.h"
#include "launch.h"

namespace diffhe {
namespace {

// The deformation of one element for one sample, carried as H = grad u so that nothing cancels at small strains:
// F = I + H, J - 1 from H alone, ln J = log1p(J - 1) (NaN for J <= 0), F^-T from the cofactors of F.
template <int DIM>
struct Deformation {
  double H[DIM][DIM], Fit[DIM][DIM], J, lnJ;

  __device__ __forceinline__ void finish() {
    double F[DIM][DIM], jm1;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = 0; t < DIM; ++t) F[a][t] = H[a][t] + (a == t ? 1.0 : 0.0);
    if constexpr (DIM == 2) {
      jm1 = (H[0][0] + H[1][1]) + (H[0][0] * H[1][1] - H[0][1] * H[1][0]);
      J = 1.0 + jm1;
      const double r = 1.0 / J;
      Fit[0][0] = F[1][1] * r;
      Fit[0][1] = -F[1][0] * r;
      Fit[1][0] = -F[0][1] * r;
      Fit[1][1] = F[0][0] * r;
    } else {
      double C[3][3], M[3];   // cofactors of F: F^-T = C / J; principal 2 x 2 minors of H
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
          C[i][j] = F[i1][j1] * F[i2][j2] - F[i1][j2] * F[i2][j1];
        }
        M[i] = H[i1][i1] * H[i2][i2] - H[i1][i2] * H[i2][i1];
      }
      const double det = H[0][0] * M[0] + H[0][1] * (H[1][2] * H[2][0] - H[1][0] * H[2][2]) +
                         H[0][2] * (H[1][0] * H[2][1] - H[1][1] * H[2][0]);
      jm1 = ((H[0][0] + H[1][1]) + H[2][2]) + ((M[0] + M[1]) + M[2]) + det;
      J = 1.0 + jm1;
      const double r = 1.0 / J;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Fit[i][j] = C[i][j] * r;
    }
    lnJ = J > 0.0 ? log1p(jm1) : __builtin_nan("");
  }

  // from the element's node ids and gradients held in registers
  __device__ __forceinline__ void from(const int* node, const double (*G)[DIM], const double* __restrict__ u, int Bp,
                                       int b) {
    constexpr int NPE = DIM + 1;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = 0; t < DIM; ++t) H[a][t] = 0.0;
#pragma unroll
    for (int p = 0; p < NPE; ++p)
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const double up = u[((i64)node[p] * DIM + a) * Bp + b];
#pragma unroll
        for (int t = 0; t < DIM; ++t) H[a][t] = fma(up, G[p][t], H[a][t]);
      }
    finish();
  }

  // from the tables
  __device__ __forceinline__ void from(const int* __restrict__ elems, const double* __restrict__ gtab,
                                       const double* __restrict__ u, int m, int e, int Bp, int b) {
    constexpr int NPE = DIM + 1;
    int node[NPE];
    double G[NPE][DIM];
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
      node[p] = elems[(i64)p * m + e];
#pragma unroll
      for (int t = 0; t < DIM; ++t) G[p][t] = gtab[(i64)(p * DIM + t) * m + e];
    }
    from(node, G, u, Bp, b);
  }

  // P1 = mu1 (F - F^-T) + lam1 ln J F^-T with F - F^-T = H + F^-T H^T
  __device__ __forceinline__ void piola(double lam1, double mu1, double (*P)[DIM]) const {
    const double c = lam1 * lnJ;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = 0; t < DIM; ++t) {
        double w = H[a][t];
#pragma unroll
        for (int s = 0; s < DIM; ++s) w = fma(Fit[a][s], H[t][s], w);
        P[a][t] = fma(c, Fit[a][t], mu1 * w);
      }
  }

  // W / E with tr F^T F - d = 2 tr H + |H|^2; the caller has checked J > 0
  __device__ __forceinline__ double energy(double lam1, double mu1) const {
    double tr = 0.0, sq = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      tr += H[a][a];
#pragma unroll
      for (int t = 0; t < DIM; ++t) sq = fma(H[a][t], H[a][t], sq);
    }
    return mu1 * ((tr - lnJ) + 0.5 * sq) + 0.5 * lam1 * (lnJ * lnJ);
  }
};

}  // namespace
}  // namespace diffhe
