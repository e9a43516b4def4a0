// Finite-strain compressible Neo-Hookean elasticity on P1 triangles (plane strain) and tetrahedra (ours: the reference
// has linear scalar equations only).  Per element and sample, from the full displacement u (prescribed values included):
//
//   F = I + sum_p u_p (x) g_p,   J = det F,   h_p = F^-T g_p,   g_p = grad phi_p
//   W(F)  = E [ mu1/2 (tr F^T F - d) - mu1 ln J + lam1/2 (ln J)^2 ]
//   P1(F) = mu1 (F - F^-T) + lam1 ln J F^-T
//   R_(p,i)            = sum_e vol_e E_e [P1 g_p]_i
//   K_T[(p,i),(q,k)]   = sum_e vol_e E_e [ mu1 delta_ik g_p.g_q + (mu1 - lam1 ln J) h_q,i h_p,k + lam1 h_p,i h_q,k ]
//   dL/dE_e            = -vol_e P1(F_e(u)) : grad lam_e
//
// definitions: include/diffhe_hyperelastic.h.  F is LINEAR in g_p: gtab is the gradient table with the sign of every
// element's orientation restored (the linear units take it up to that sign, which cancels in their products of two
// gradients).  The tangent is stored in the dof pattern of include/diffhe_elastic.h and
// solved by the generic entries of ell_pcg.hip / ell_amg.hip; at u = 0 it is the plane-strain / 3D operator of elastic.hip.
//
// Data layout as in elastic.hip: dof-major, batch innermost, lanes over samples (node_map) ALWAYS -- the operator is per
// sample even where E is shared, because u is -- so node ids, gradients and list entries are wave-uniform and every
// access is one contiguous segment.  fp64, no atomics anywhere: every sum has a fixed order, results are bitwise
// reproducible.
//
// The assembly RECOMPUTES F, J and F^-T per contribution (npe*d gathered doubles of u, L2 hits after the first touch of an
// element) instead of reading a per-element table a pre-pass would write: (d*d + 1) m Bp doubles written and read back
// against d*d*W*n*Bp doubles of vals stored, and one launch less per Newton iteration.
#include "common.h"
#include "deformation.h"
#include "diffhe_hyperelastic.h"
#include "element_grad.h"
#include "launch.h"

namespace {

using namespace diffhe;

// ---------------------------------------------------------------------------------------
// The tangent: elast_assemble_rows_kernel of elastic.hip with the element block above.  One lane owns node i of sample b,
// walks the node's W slots and builds the d x d block of each from the node-level contribution lists, then writes its d
// rows: identity rows on fixed dofs, zeroed fixed columns, no lift.
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void hyper_assemble_rows_kernel(
    const int* __restrict__ elems, const double* __restrict__ gtab, const double* __restrict__ vol, double lam1,
    double mu1, const double* __restrict__ E, i64 ese, i64 esb, const double* __restrict__ u,
    const int* __restrict__ ent_ptr, const int* __restrict__ contrib, const int* __restrict__ cols,
    const unsigned char* __restrict__ is_bc, double* __restrict__ vals, int n, int m, int W, int Bp) {
  constexpr int NPE = DIM + 1;
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  const i64 nd = (i64)n * DIM;
  for (int i = nm.node0; i < n; i += nm.stride) {
    bool rbc[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) rbc[a] = is_bc && is_bc[(i64)i * DIM + a];
    for (int k = 0; k < W; ++k) {
      const i64 ent = (i64)k * n + i;
      const int j = cols[ent];
      const bool unused = k > 0 && j == i;   // an unused node slot: d unused dof slots, pointing at the row itself
      const int c0 = ent_ptr[ent], c1 = ent_ptr[ent + 1];
      double blk[DIM][DIM];
#pragma unroll
      for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) blk[a][b] = 0.0;
      for (int c = c0; c < c1; ++c) {
        const int code = contrib[c];
        const int e = code >> 6, pq = code & 63;
        const int p = pq / NPE, q = pq % NPE;
        Deformation<DIM> D;
        D.from(elems, gtab, u, m, e, Bp, nm.b);
        double hp[DIM], hq[DIM];
        double dot = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) hp[a] = hq[a] = 0.0;
#pragma unroll
        for (int t = 0; t < DIM; ++t) {
          const double gp = gtab[(i64)(p * DIM + t) * m + e], gq = gtab[(i64)(q * DIM + t) * m + e];
          dot = fma(gp, gq, dot);
#pragma unroll
          for (int a = 0; a < DIM; ++a) {
            hp[a] = fma(D.Fit[a][t], gp, hp[a]);
            hq[a] = fma(D.Fit[a][t], gq, hq[a]);
          }
        }
        // ln J is NaN for J <= 0: so is every entry of the block
        const double s = vol[e] * E[(i64)e * ese + (i64)nm.b * esb] + 0.0 * D.lnJ;
        const double cross = mu1 - lam1 * D.lnJ;
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
          for (int b = 0; b < DIM; ++b) {
            double w = cross * (hq[a] * hp[b]) + lam1 * (hp[a] * hq[b]);
            if (a == b) w += mu1 * dot;
            blk[a][b] = fma(s, w, blk[a][b]);
          }
      }
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const i64 row = (i64)i * DIM + a;
#pragma unroll
        for (int b = 0; b < DIM; ++b) {
          const i64 col = (i64)j * DIM + b;
          const int slot = k == 0 ? (b - a + DIM) % DIM : k * DIM + b;
          double v = unused ? 0.0 : blk[a][b];
          if (rbc[a]) {
            v = slot == 0 ? 1.0 : 0.0;
          } else if (!unused && col != row && is_bc && is_bc[col]) {
            v = 0.0;
          }
          vals[((i64)slot * nd + row) * Bp + nm.b] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// The internal force: a node pass over the incidence list, the shape of eigen_load_kernel (eigenstrain.hip).
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void hyper_residual_kernel(const int* __restrict__ inc_ptr, const int* __restrict__ inc,
                                                              const int* __restrict__ elems,
                                                              const double* __restrict__ gtab,
                                                              const double* __restrict__ vol, double lam1, double mu1,
                                                              const double* __restrict__ E, i64 ese, i64 esb,
                                                              const double* __restrict__ u, int n, int m, int Bp,
                                                              double* __restrict__ R) {
  constexpr int NPE = DIM + 1;
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  for (int i = nm.node0; i < n; i += nm.stride) {
    double acc[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) acc[a] = 0.0;
    for (int j = inc_ptr[i]; j < inc_ptr[i + 1]; ++j) {
      const int code = inc[j];
      const int e = code / NPE, p = code - e * NPE;
      Deformation<DIM> D;
      D.from(elems, gtab, u, m, e, Bp, nm.b);
      double P[DIM][DIM], r[DIM];
      D.piola(lam1, mu1, P);
      const double ve = vol[e] * E[(i64)e * ese + (i64)nm.b * esb];
#pragma unroll
      for (int a = 0; a < DIM; ++a) r[a] = 0.0;
#pragma unroll
      for (int t = 0; t < DIM; ++t) {
        const double g = gtab[(i64)(p * DIM + t) * m + e];
#pragma unroll
        for (int a = 0; a < DIM; ++a) r[a] = fma(P[a][t], g, r[a]);
      }
#pragma unroll
      for (int a = 0; a < DIM; ++a) acc[a] = fma(ve, r[a], acc[a]);
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a) R[((i64)i * DIM + a) * Bp + nm.b] = acc[a];
  }
}

// block_sum_per_sample of common.h with min in place of +
__device__ inline double block_min_per_sample(double v, int Bp, double* lds) {
  const int LB = Bp < kWave ? Bp : kWave;
  for (int off = LB; off < kWave; off <<= 1) v = fmin(v, __shfl_xor(v, off));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  lds[wave * kWave + lane] = v;
  __syncthreads();
  double s = v;
  if (wave == 0) s = fmin(fmin(lds[lane], lds[kWave + lane]), fmin(lds[2 * kWave + lane], lds[3 * kWave + lane]));
  __syncthreads();
  return s;
}

// ---------------------------------------------------------------------------------------
// The strain energy and the smallest J per sample, first stage: an element pass, the block's sums and minima per sample
// in w_part, j_part (nblk, Bp).  An inverted element (J <= 0, or not a number) adds nothing to the sum and leaves a
// non-positive minimum: the second stage turns that into +inf for that sample alone.
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void hyper_energy_kernel(const int* __restrict__ elems, const double* __restrict__ gtab,
                                                            const double* __restrict__ vol, double lam1, double mu1,
                                                            const double* __restrict__ E, i64 ese, i64 esb,
                                                            const double* __restrict__ u, int m, int Bp,
                                                            double* __restrict__ w_part, double* __restrict__ j_part) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);   // "nodes" are elements here
  const bool ok = nm.b < Bp;
  double s = 0.0, jmin = __builtin_inf();
  if (ok)
    for (int e = nm.node0; e < m; e += nm.stride) {
      Deformation<DIM> D;
      D.from(elems, gtab, u, m, e, Bp, nm.b);
      if (D.J > 0.0) {
        s = fma(vol[e] * E[(i64)e * ese + (i64)nm.b * esb], D.energy(lam1, mu1), s);
        jmin = fmin(jmin, D.J);
      } else {
        jmin = fmin(jmin, D.J == D.J ? D.J : 0.0);   // a NaN counts as inverted
      }
    }
  const double ts = block_sum_per_sample(s, Bp, lds);
  const double tj = block_min_per_sample(jmin, Bp, lds);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave == 0 && lane < (Bp < kWave ? Bp : kWave) && ok) {
    w_part[(i64)blockIdx.x * Bp + nm.b] = ts;
    j_part[(i64)blockIdx.x * Bp + nm.b] = tj;
  }
}

// Second stage: one lane per sample walks the blocks in order.
__global__ __launch_bounds__(256) void hyper_energy_sum_kernel(const double* __restrict__ w_part,
                                                                const double* __restrict__ j_part, int nblk, int Bp,
                                                                double* __restrict__ energy, double* __restrict__ min_j) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= Bp) return;
  double s = 0.0, jmin = __builtin_inf();
  for (int k = 0; k < nblk; ++k) {
    s += w_part[(i64)k * Bp + b];
    jmin = fmin(jmin, j_part[(i64)k * Bp + b]);
  }
  energy[b] = jmin > 0.0 ? s : __builtin_inf();
  min_j[b] = jmin;
}

// ---------------------------------------------------------------------------------------
// dL/dE as a form of element_grad.h (NC = 1): out[0] = -vol P1(F(u)) : grad lam.
// ---------------------------------------------------------------------------------------
template <int DIM>
struct HyperGradForm {
  static constexpr int NC = 1;
  static constexpr int NPE = DIM + 1;
  const int* __restrict__ elems;
  const double* __restrict__ gtab;
  const double* __restrict__ vol;
  double lam1, mu1;
  const double* __restrict__ lam;
  const double* __restrict__ u;
  int m;

  struct Elem {
    int node[NPE];
    double G[NPE][DIM];
    double ve;
  };

  __device__ __forceinline__ void load(int e, Elem& el) const {
    el.ve = vol[e];
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
      el.node[p] = elems[(i64)p * m + e];
#pragma unroll
      for (int t = 0; t < DIM; ++t) el.G[p][t] = gtab[(i64)(p * DIM + t) * m + e];
    }
  }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* out) const {
    Deformation<DIM> D;
    D.from(el.node, el.G, u, Bp, b);
    double P[DIM][DIM], Hl[DIM][DIM];
    D.piola(lam1, mu1, P);
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = 0; t < DIM; ++t) Hl[a][t] = 0.0;
#pragma unroll
    for (int p = 0; p < NPE; ++p)
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const double lp = lam[((i64)el.node[p] * DIM + a) * Bp + b];
#pragma unroll
        for (int t = 0; t < DIM; ++t) Hl[a][t] = fma(lp, el.G[p][t], Hl[a][t]);
      }
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = 0; t < DIM; ++t) s = fma(P[a][t], Hl[a][t], s);
    out[0] = -el.ve * s;
  }
};

// what every entry refuses: pointers, dim, sizes, the int32 codes e * npe + p and (e << 6 | pq)
bool bad_common(const int* elems, const double* gtab, const double* vol, int dim, const double* u, int n, int m) {
  return !elems || !gtab || !vol || !u || (dim != 2 && dim != 3) || n < 1 || m < 1 || (i64)m >= (1LL << 25);
}

bool bad_modulus(const double* E, i64 e_se, i64 e_sb) { return !E || e_se < 0 || e_sb < 0; }

double modulus_bytes(i64 e_se, i64 e_sb, int m, int Bp) { return 8.0 * (e_se ? (double)m : 1.0) * (e_sb ? (double)Bp : 1.0); }

}  // namespace

// =========================================================================================
// C ABI (include/diffhe_hyperelastic.h)
// =========================================================================================
extern "C" int diffhe_hyper_assemble_rows(const int* elems, const double* gtab, const double* vol, int dim, double lam1,
                                          double mu1, const double* E, long long e_se, long long e_sb, const double* u,
                                          const int* ent_ptr, const int* contrib, const int* cols,
                                          const unsigned char* is_bc, double* vals, int n, int m, int W, int Bp,
                                          void* stream) {
  if (bad_common(elems, gtab, vol, dim, u, n, m) || bad_modulus(E, e_se, e_sb) || !ent_ptr || !contrib || !cols || !vals ||
      W < 1)
    return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  if ((long long)n * dim > 2147483647LL / ((long long)dim * W)) return DIFFHE_E_TOOBIG;   // dof entries index as int32 in the ell_* units
  // values, u once per dof, the field
  diffhe::account(8.0 * Bp * ((double)dim * dim * W * n + (double)dim * n) + modulus_bytes(e_se, e_sb, m, Bp));
  const dim3 grid = diffhe::node_grid(n, Bp);
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(hyper_assemble_rows_kernel<D()>, grid, dim3(256), 0, (hipStream_t)stream, elems, gtab, vol, lam1,
                       mu1, E, e_se, e_sb, u, ent_ptr, contrib, cols, is_bc, vals, n, m, W, Bp);
  });
  return diffhe::check_launch();
}

extern "C" int diffhe_hyper_residual(const int* inc_ptr, const int* inc, const int* elems, const double* gtab,
                                     const double* vol, int dim, double lam1, double mu1, const double* E, long long e_se,
                                     long long e_sb, const double* u, int n, int m, int Bp, double* R, void* stream) {
  if (bad_common(elems, gtab, vol, dim, u, n, m) || bad_modulus(E, e_se, e_sb) || !inc_ptr || !inc || !R)
    return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  // u and R once per dof, the field
  diffhe::account(8.0 * Bp * 2.0 * dim * n + modulus_bytes(e_se, e_sb, m, Bp));
  const dim3 grid = diffhe::node_grid(n, Bp);
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(hyper_residual_kernel<D()>, grid, dim3(256), 0, (hipStream_t)stream, inc_ptr, inc, elems, gtab,
                       vol, lam1, mu1, E, e_se, e_sb, u, n, m, Bp, R);
  });
  return diffhe::check_launch();
}

extern "C" int diffhe_hyper_energy(const int* elems, const double* gtab, const double* vol, int dim, double lam1,
                                   double mu1, const double* E, long long e_se, long long e_sb, const double* u, int n,
                                   int m, int Bp, double* w_part, double* j_part, double* energy, double* min_j,
                                   void* stream) {
  if (bad_common(elems, gtab, vol, dim, u, n, m) || bad_modulus(E, e_se, e_sb) || !w_part || !j_part || !energy || !min_j)
    return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const dim3 grid = diffhe::node_grid(m, Bp);
  if ((int)grid.x != diffhe_grad_kappa_blocks(m, Bp)) return DIFFHE_E_BADARG;   // the partials are sized by that entry
  // u once per dof, the field
  diffhe::account(8.0 * Bp * (double)dim * n + modulus_bytes(e_se, e_sb, m, Bp));
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(hyper_energy_kernel<D()>, grid, dim3(256), 0, (hipStream_t)stream, elems, gtab, vol, lam1, mu1, E,
                       e_se, e_sb, u, m, Bp, w_part, j_part);
  });
  hipLaunchKernelGGL(hyper_energy_sum_kernel, dim3((Bp + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const double*)w_part, (const double*)j_part, (int)grid.x, Bp, energy, min_j);
  return diffhe::check_launch();
}

extern "C" int diffhe_hyper_grad(const int* elems, const double* gtab, const double* vol, int dim, double lam1, double mu1,
                                 const double* lam, const double* u, int n, int m, int Bp, double* de_e, double* de_part,
                                 double* de_sum, void* stream) {
  if (bad_common(elems, gtab, vol, dim, u, n, m) || !lam) return DIFFHE_E_BADARG;
  if (!de_e && !de_part) return DIFFHE_E_BADARG;
  if ((de_part == nullptr) != (de_sum == nullptr)) return DIFFHE_E_BADARG;
  const double bytes = 8.0 * Bp * (2.0 * dim * n + (de_e ? (double)m : 0));   // lambda and u once per dof, dE per element
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return diffhe::launch_element_grad(HyperGradForm<D()>{elems, gtab, vol, lam1, mu1, lam, u, m}, m, Bp, de_e, 0, Bp,
                                       de_part, de_sum, bytes, stream);
  });
}

extern "C" int diffhe_hyper_grad_shared(const int* elems, const double* gtab, const double* vol, int dim, double lam1,
                                        double mu1, const double* lam, const double* u, int n, int m, int B, int Bp,
                                        double* de, void* stream) {
  if (bad_common(elems, gtab, vol, dim, u, n, m) || !lam || !de || B < 1 || B > Bp) return DIFFHE_E_BADARG;
  const double bytes = 8.0 * (Bp * 2.0 * dim * n + (double)m);
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return diffhe::launch_element_grad_shared(HyperGradForm<D()>{elems, gtab, vol, lam1, mu1, lam, u, m}, m, B, Bp, de, 0,
                                              1, bytes, stream);
  });
}
