// The eigenstrain (initial strain) of an element and a sample as eigenstrain.hip and the eigen variants of stress.hip read
// it, and the Voigt indexing both units share (definitions: include/diffhe_eigenstrain.h).
//
// eps0 holds component c of element e and sample b at c*zc + e*ze + b*zb, so that one tensor for everything (ze = zb = 0),
// a field the batch shares (zb = 0), one tensor per sample (ze = 0) and a field per sample are read where they lie.  With
// zb = 0 the components belong to the element: a form reads them in its load() next to the gradients, wave-uniform, and on
// the batch-summing kernel, whose element index is a scalar, that read is a scalar load.
#pragma once
#include "common.h"

namespace diffhe {
namespace {

// Voigt component k of a symmetric DIM x DIM tensor: (row, column); the first DIM are the diagonal.
template <int DIM>
__device__ __forceinline__ constexpr int voigt_row(int k) {
  return k < DIM ? k : (DIM == 2 ? 0 : (k == 3 ? 1 : 0));
}
template <int DIM>
__device__ __forceinline__ constexpr int voigt_col(int k) {
  return k < DIM ? k : (DIM == 2 ? 1 : (k == 5 ? 1 : 2));
}

template <int DIM>
struct EigenField {
  static constexpr int NC = DIM * (DIM + 1) / 2;
  static constexpr int NZ = DIM == 2 ? 4 : 6;   // components held in registers: (xx, yy, xy, zz) | the six of 3D
  const double* __restrict__ eps0;
  long long zc, ze, zb;
  double lam1, mu1;
  int pstrain;                                  // DIM == 2: component 3 (zz) is stored and constrained; else absent

  __device__ __forceinline__ int count() const { return DIM == 2 && pstrain ? 4 : NC; }

  // z (NZ) of element e and sample b; the zz of plane stress is 0 and not read
  __device__ __forceinline__ void read(int e, int b, double* z) const {
    const double* __restrict__ p = eps0 + (long long)e * ze + (long long)b * zb;
#pragma unroll
    for (int k = 0; k < NC; ++k) z[k] = p[k * zc];
    if (DIM == 2) z[3] = pstrain ? p[3 * zc] : 0.0;
  }

  // the in-plane unit initial stress s0 (NC) = 2 mu1 eps0 + lam1 theta0 I; returns theta0 = tr eps0, zz included
  __device__ __forceinline__ double initial_stress(const double* z, double* s0) const {
    double th = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) th += z[a];
    if (DIM == 2) th += z[3];
#pragma unroll
    for (int k = 0; k < NC; ++k) s0[k] = k < DIM ? fma(2.0 * mu1, z[k], lam1 * th) : 2.0 * mu1 * z[k];
    return th;
  }

  // The transpose of that map, zz row included: for cotangents c (NC) of the in-plane unit stress -- a shear one the
  // derivative with respect to that one number -- and czz of the out-of-plane one, scale * d / d eps0 -> out (NZ).
  __device__ __forceinline__ void transpose(double scale, const double* c, double czz, double* out) const {
    double tr = czz;
#pragma unroll
    for (int a = 0; a < DIM; ++a) tr += c[a];
#pragma unroll
    for (int k = 0; k < NC; ++k) out[k] = scale * (k < DIM ? fma(2.0 * mu1, c[k], lam1 * tr) : 2.0 * mu1 * c[k]);
    if (DIM == 2) out[3] = scale * fma(2.0 * mu1, czz, lam1 * tr);
  }
};

// bytes of eps0 as the kernels read it, nc0 components
inline double eigen_bytes(int nc0, long long ze, long long zb, int m, int Bp) {
  return 8.0 * nc0 * (ze ? (double)m : 1.0) * (zb ? (double)Bp : 1.0);
}

inline bool bad_eigen(const double* eps0, long long zc, long long ze, long long zb) {
  return !eps0 || zc < 1 || ze < 0 || zb < 0;
}

}  // namespace
}  // namespace diffhe
