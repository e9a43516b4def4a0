// The element of a stress evaluation and the element pass of its adjoint, as stress.hip and elastic_shape.hip read them
// (definitions: include/diffhe_stress.h, include/diffhe_eigenstrain.h).  The cotangent chain -- sigma and vm recomputed,
// c = sigma_bar + vm_bar d vm / d sigma, the symmetric tensor T = dL/dH of the displacement gradient H -- is stated here
// once: the adjoint of stress.hip writes T to its work array for the node pass, the node-coordinate gradient of
// elastic_shape.hip contracts it with H in registers.
//
// Every struct takes a compile-time EIG: with it the element carries an eigenstrain (eigen_field.h) and the stress is
// E (s(u) - s0) with an out-of-plane component of its own; without it the instantiations are the ones of diffhe_stress.h.
#pragma once
#include "common.h"
#include "eigen_field.h"

namespace diffhe {
namespace {

// What an element with an eigenstrain carries on top: the field, and its components where the batch shares them (zb == 0).
template <int DIM, bool EIG>
struct EigenOf {};
template <int DIM>
struct EigenOf<DIM, true> {
  EigenField<DIM> ef;
};
template <int DIM, bool EIG>
struct EigenElem {};
template <int DIM>
struct EigenElem<DIM, true> {
  double z[EigenField<DIM>::NZ];
};

// What both directions read of an element and a sample.
template <int DIM, bool EIG = false>
struct StressElement : EigenOf<DIM, EIG> {
  static constexpr int NPE = DIM + 1, NC = DIM * (DIM + 1) / 2;
  const int* __restrict__ elems;
  const double* __restrict__ gtab;
  double lam1, mu1, nu_z;
  const double* __restrict__ u;
  const double* __restrict__ E;
  long long ese, esb;
  int m;

  struct Elem : EigenElem<DIM, EIG> {
    int e;
    int node[NPE];
    double G[NPE][DIM];
  };

  __device__ __forceinline__ void load(int e, Elem& el) const {
    el.e = e;
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
      el.node[p] = elems[(long long)p * m + e];
#pragma unroll
      for (int t = 0; t < DIM; ++t) el.G[p][t] = gtab[(long long)(p * DIM + t) * m + e];
    }
    if constexpr (EIG) {
      if (this->ef.zb == 0) this->ef.read(e, 0, el.z);
    }
  }

  // H[a][t] = sum_p u[(p, a)] g_p[t] of sample b
  __device__ __forceinline__ void displacement_gradient(const Elem& el, int Bp, int b, double (*H)[DIM]) const {
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = 0; t < DIM; ++t) H[a][t] = 0.0;
#pragma unroll
    for (int p = 0; p < NPE; ++p)
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const double up = u[((long long)el.node[p] * DIM + a) * Bp + b];
#pragma unroll
        for (int t = 0; t < DIM; ++t) H[a][t] = fma(up, el.G[p][t], H[a][t]);
      }
  }

  // the unit stress s (NC) from H; returns tr H
  __device__ __forceinline__ double unit_stress_of(const double (*H)[DIM], double* s) const {
    double tr = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) tr += H[a][a];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int a = voigt_row<DIM>(k), t = voigt_col<DIM>(k);
      s[k] = k < DIM ? fma(2.0 * mu1, H[a][a], lam1 * tr) : mu1 * (H[a][t] + H[t][a]);
    }
    return tr;
  }

  // the unit stress s (NC) of sample b; returns tr H
  __device__ __forceinline__ double unit_stress(const Elem& el, int Bp, int b, double* s) const {
    double H[DIM][DIM];
    displacement_gradient(el, Bp, b, H);
    return unit_stress_of(H, s);
  }

  // EIG: s <- s - s0 in plane, tr = tr H; returns the out-of-plane unit stress lam1 (tr - theta0) - 2 mu1 eps0_zz of
  // plane strain (0 otherwise)
  __device__ __forceinline__ double subtract_initial(const Elem& el, int b, double tr, double* s) const {
    double szz = 0.0;
    if constexpr (EIG) {
      constexpr int NZ = EigenField<DIM>::NZ;
      double z[NZ], s0[NC];
      if (this->ef.zb) {
        this->ef.read(el.e, b, z);
      } else {
#pragma unroll
        for (int k = 0; k < NZ; ++k) z[k] = el.z[k];
      }
      const double th = this->ef.initial_stress(z, s0);
#pragma unroll
      for (int k = 0; k < NC; ++k) s[k] -= s0[k];
      if (DIM == 2 && this->ef.pstrain) szz = fma(lam1, tr - th, -2.0 * mu1 * z[3]);
    }
    return szz;
  }

  __device__ __forceinline__ double modulus(int e, int b) const { return E[(long long)e * ese + (long long)b * esb]; }
};

// The three normal stresses of sigma (NC): in 2D the third is nu_z (sigma_xx + sigma_yy), with an eigenstrain sg_zz.
template <int DIM, bool EIG>
__device__ __forceinline__ void normal_stresses(const double* sg, double nu_z, double sg_zz, double* nn) {
  nn[0] = sg[0];
  nn[1] = sg[1];
  nn[2] = DIM == 2 ? (EIG ? sg_zz : nu_z * (sg[0] + sg[1])) : sg[2];
}

template <int DIM>
__device__ __forceinline__ double von_mises(const double* sg, const double* nn) {
  constexpr int NC = DIM * (DIM + 1) / 2;
  const double d0 = nn[0] - nn[1], d1 = nn[1] - nn[2], d2 = nn[2] - nn[0];
  double sh = 0.0;
#pragma unroll
  for (int k = DIM; k < NC; ++k) sh = fma(sg[k], sg[k], sh);
  return sqrt(fma(0.5, fma(d0, d0, fma(d1, d1, d2 * d2)), 3.0 * sh));
}

// ---------------------------------------------------------------------------------------
// The element pass of the adjoint as a form of element_grad.h: out[0] = dE[e, b] = sum_k c_k s_k with the combined
// cotangent c = sigma_bar + vm_bar d vm / d sigma, and, where `work` is given, T = E (2 mu1 sym(C) + lam1 tr(C) I) to
// work (NC, m, Bp).  Samples b >= B: dE = 0, T = 0, no cotangent read.
// ---------------------------------------------------------------------------------------
template <bool EIG>
struct EigenOut {};
template <>
struct EigenOut<true> {
  double* __restrict__ deps;   // d / d eps0 at c*dzc + e*dze + b, or NULL
  long long dzc, dze;
};

template <int DIM, bool EIG = false>
struct StressAdjointForm : EigenOut<EIG> {
  static constexpr int NC = 1;
  static constexpr int NV = DIM * (DIM + 1) / 2;
  typedef typename StressElement<DIM, EIG>::Elem Elem;
  StressElement<DIM, EIG> el_of;
  const double* __restrict__ sigma_bar;
  long long osc, ose;
  const double* __restrict__ vm_bar;
  double* __restrict__ work;
  int B;

  __device__ __forceinline__ void load(int e, Elem& el) const { el_of.load(e, el); }

  // The chain of sample b < B from the displacement gradient H: the unit stress s (NV), the combined cotangent c (NV) of
  // sigma, and (EIG only) the out-of-plane unit stress szz with its cotangent czz; returns the modulus.
  __device__ __forceinline__ double cotangent(const Elem& el, int Bp, int b, const double (*H)[DIM], double* s, double* c,
                                              double& szz, double& czz) const {
    const long long at = (long long)el.e * Bp + b;
    const double tr_h = el_of.unit_stress_of(H, s);
    szz = el_of.subtract_initial(el, b, tr_h, s);                // EIG only
    czz = 0.0;                                                   // EIG only: the cotangent of sigma_zz
    const double Ee = el_of.modulus(el.e, b);
#pragma unroll
    for (int k = 0; k < NV; ++k) c[k] = sigma_bar ? sigma_bar[k * osc + el.e * ose + b] : 0.0;
    if (vm_bar) {
      double sg[NV], nn[3];
#pragma unroll
      for (int k = 0; k < NV; ++k) sg[k] = Ee * s[k];
      normal_stresses<DIM, EIG>(sg, el_of.nu_z, Ee * szz, nn);
      const double vm = von_mises<DIM>(sg, nn);
      if (vm > 0.0) {                                   // d vm / d sigma = 0 where vm == 0
        const double w = vm_bar[at] / vm;
        const double mean = ((nn[0] + nn[1]) + nn[2]) / 3.0;
        double cn[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) cn[i] = 1.5 * (nn[i] - mean) * w;
#pragma unroll
        for (int i = 0; i < DIM; ++i) c[i] += cn[i];
        if (DIM == 2 && !EIG) {                         // sigma_zz = nu_z (sigma_xx + sigma_yy)
          c[0] = fma(el_of.nu_z, cn[2], c[0]);
          c[1] = fma(el_of.nu_z, cn[2], c[1]);
        }
        if constexpr (EIG && DIM == 2) {                // sigma_zz on its own; identically 0 in plane stress
          if (el_of.ef.pstrain) czz = cn[2];
        }
#pragma unroll
        for (int k = DIM; k < NV; ++k) c[k] = fma(3.0 * sg[k], w, c[k]);
      }
    }
    return Ee;
  }

  // T (NV, Voigt) = E (2 mu1 sym(C) + lam1 tr(C) I) = dL/dH, symmetric: T[a][t] is the derivative with respect to H[a][t]
  __device__ __forceinline__ void tensor(const double* c, double czz, double Ee, double* T) const {
    double tr = EIG ? czz : 0.0;                        // sigma_zz = E lam1 tr eps(u) + ... feeds the trace
#pragma unroll
    for (int i = 0; i < DIM; ++i) tr += c[i];
#pragma unroll
    for (int k = 0; k < NV; ++k) T[k] = Ee * (k < DIM ? fma(2.0 * el_of.mu1, c[k], el_of.lam1 * tr) : el_of.mu1 * c[k]);
  }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* out) const {
    const long long mb = (long long)el_of.m * Bp, at = (long long)el.e * Bp + b;
    if (b >= B) {
      out[0] = 0.0;
      if (work) {
#pragma unroll
        for (int k = 0; k < NV; ++k) work[k * mb + at] = 0.0;
      }
      if constexpr (EIG) {
        if (this->deps)
          for (int k = 0; k < el_of.ef.count(); ++k) this->deps[k * this->dzc + el.e * this->dze + b] = 0.0;
      }
      return;
    }
    double H[DIM][DIM], s[NV], c[NV], szz, czz;
    el_of.displacement_gradient(el, Bp, b, H);
    const double Ee = cotangent(el, Bp, b, H, s, c, szz, czz);
    double de = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) de = fma(c[k], s[k], de);
    if (EIG) de = fma(czz, szz, de);
    out[0] = de;
    if constexpr (EIG) {
      if (this->deps) {
        double dz[EigenField<DIM>::NZ];
        el_of.ef.transpose(-Ee, c, czz, dz);
#pragma unroll
        for (int k = 0; k < EigenField<DIM>::NZ; ++k)
          if (k < el_of.ef.count()) this->deps[k * this->dzc + el.e * this->dze + b] = dz[k];
      }
    }
    if (work) {
      double T[NV];
      tensor(c, czz, Ee, T);
#pragma unroll
      for (int k = 0; k < NV; ++k) work[k * mb + at] = T[k];
    }
  }
};

}  // namespace
}  // namespace diffhe
