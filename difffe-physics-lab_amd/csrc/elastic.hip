// Linear elasticity: -div sigma(u) = f, sigma = 2 mu eps(u) + lambda tr eps(u) I, on P1 triangles and tetrahedra (ours:
// the reference has scalar unknowns only).  d = DIM displacement components per node, dof(i, a) = i*d + a; K(E) is linear
// in the per-element Young's modulus E, so with the Lame numbers lam1, mu1 of E = 1 and g_p = grad phi_p
//
//   K_e[(p,a),(q,b)] = |e| E_e [ lam1 g_pa g_qb + mu1 g_pb g_qa + mu1 delta_ab g_p.g_q ]
//   dL/dE_e          = -|e| [ lam1 (div lam_h)(div u_h) + 2 mu1 eps(lam_h) : eps(u_h) ]
//
// Both read the gradient table of aniso.hip (g_p as (npe*d, m), |e| as (m)).  The operator is stored as ELL rows over
// the n*d dofs in the pattern include/diffhe_elastic.h describes (a node's own d x d block rotated so that slot 0 is the
// diagonal, then d slots per neighbouring node); the solves run on it through the generic entries of ell_pcg.hip / ell_amg.hip.
//
// Data layout as in aniso.hip: dof-major, batch innermost.  With one matrix per sample (Bv = Bp) lanes run over samples,
// so table entries and list indices are wave-uniform and every store is one contiguous segment; with one matrix for the
// batch (Bv = 1) lanes run over nodes.  fp64, no atomics anywhere: every sum has a fixed order, results are bitwise
// reproducible.
//
// dL/dE keeps its own two kernels: on the element loop of element_grad.h they measured slower (2D at Bp = 256, the 3D
// batch-shared kernel at B = 64).  Only the second stage of the per-sample total is the header's.
#include "common.h"
#include "diffhe_elastic.h"
#include "element_grad.h"
#include "launch.h"

namespace {

using namespace diffhe;

// ---------------------------------------------------------------------------------------
// Block row-gather assembly: one lane owns node i of sample b, walks the node's W slots and builds the d x d block of
// each from the node-level contribution lists (assemble_rows_kernel of ell_assemble.hip, aniso_assemble_rows_kernel), then
// writes its d rows with the per-dof Dirichlet handling: identity rows, zeroed columns, lift.
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void elast_assemble_rows_kernel(
    const double* __restrict__ gtab, const double* __restrict__ vol, double lam1, double mu1,
    const double* __restrict__ E, i64 ese, i64 esb, const int* __restrict__ ent_ptr, const int* __restrict__ contrib,
    const int* __restrict__ cols, const unsigned char* __restrict__ is_bc, const double* __restrict__ g,
    double* __restrict__ vals, double* __restrict__ lift, int n, int m, int W, int Bv) {
  constexpr int NPE = DIM + 1;
  const NodeMap nm = node_map(Bv);
  if (nm.b >= Bv) return;
  const i64 nd = (i64)n * DIM;
  for (int i = nm.node0; i < n; i += nm.stride) {
    bool rbc[DIM];
    double lf[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      rbc[a] = is_bc && is_bc[(i64)i * DIM + a];
      lf[a] = 0.0;
    }
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
        double gp[DIM], gq[DIM];
        double dot = 0.0;
#pragma unroll
        for (int t = 0; t < DIM; ++t) {
          gp[t] = gtab[(i64)(p * DIM + t) * m + e];
          gq[t] = gtab[(i64)(q * DIM + t) * m + e];
          dot = fma(gp[t], gq[t], dot);
        }
        const double s = vol[e] * E[(i64)e * ese + (i64)nm.b * esb];
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
          for (int b = 0; b < DIM; ++b) {
            double w = lam1 * (gp[a] * gq[b]) + mu1 * (gp[b] * gq[a]);
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
            lf[a] += v * g[col];
            v = 0.0;
          }
          vals[((i64)slot * nd + row) * Bv + nm.b] = v;
        }
      }
    }
    if (lift) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) lift[((i64)i * DIM + a) * Bv + nm.b] = lf[a];
    }
  }
}

// The element's dofs, gradients and the Dirichlet values of its dofs (0 without data).
template <int DIM>
__device__ __forceinline__ void load_element(const int* __restrict__ elems, const double* __restrict__ gtab,
                                             const double* __restrict__ g, int m, int e, int* node, double (*G)[DIM],
                                             double (*gq)[DIM]) {
  constexpr int NPE = DIM + 1;
#pragma unroll
  for (int p = 0; p < NPE; ++p) {
    node[p] = elems[(i64)p * m + e];
#pragma unroll
    for (int t = 0; t < DIM; ++t) {
      G[p][t] = gtab[(i64)(p * DIM + t) * m + e];
      gq[p][t] = g ? g[(i64)node[p] * DIM + t] : 0.0;
    }
  }
}

// dE of element e for the sample of this lane, from the element-constant displacement gradients
// H[a][t] = d u_a / d x_t = sum_p u[(p, a)] g_p[t] of lam and u:
//   -|e| [ lam1 tr(Hl) tr(Hu) + mu1 sum_{a,t} Hl[a][t] (Hu[a][t] + Hu[t][a]) ]      (2 eps(l) : eps(u) = the last sum)
template <int DIM>
__device__ __forceinline__ double element_grad(const int* node, const double (*G)[DIM], const double (*gq)[DIM],
                                               double ve, double lam1, double mu1, const double* __restrict__ lam,
                                               const double* __restrict__ u, int Bp, int b) {
  constexpr int NPE = DIM + 1;
  double Hl[DIM][DIM], Hu[DIM][DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a)
#pragma unroll
    for (int t = 0; t < DIM; ++t) Hl[a][t] = Hu[a][t] = 0.0;
#pragma unroll
  for (int p = 0; p < NPE; ++p) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const i64 o = ((i64)node[p] * DIM + a) * Bp + b;
      const double lp = lam[o];
      const double up = u[o] + gq[p][a];   // full u: prescribed displacements included
#pragma unroll
      for (int t = 0; t < DIM; ++t) {
        Hl[a][t] = fma(lp, G[p][t], Hl[a][t]);
        Hu[a][t] = fma(up, G[p][t], Hu[a][t]);
      }
    }
  }
  double trl = 0.0, tru = 0.0, ee = 0.0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    trl += Hl[a][a];
    tru += Hu[a][a];
#pragma unroll
    for (int t = 0; t < DIM; ++t) ee = fma(Hl[a][t], Hu[a][t] + Hu[t][a], ee);
  }
  return -ve * (lam1 * (trl * tru) + mu1 * ee);
}

// ---------------------------------------------------------------------------------------
// dL/dE per element and sample, de_e (m, Bp) (optional), and its block partial sums over the elements per sample,
// de_part (nblk, Bp) (optional): first stage of the per-sample total (second stage: element_grad.h).
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void elast_grad_kernel(const int* __restrict__ elems, const double* __restrict__ gtab,
                                                          const double* __restrict__ vol, double lam1, double mu1,
                                                          const double* __restrict__ lam, const double* __restrict__ u,
                                                          const double* __restrict__ g, int m, int Bp,
                                                          double* __restrict__ de_e, double* __restrict__ de_part) {
  constexpr int NPE = DIM + 1;
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);  // "nodes" are elements here
  const bool ok = nm.b < Bp;
  double s = 0.0;
  if (ok)
    for (int e = nm.node0; e < m; e += nm.stride) {
      int node[NPE];
      double G[NPE][DIM], gq[NPE][DIM];
      load_element<DIM>(elems, gtab, g, m, e, node, G, gq);
      const double d = element_grad<DIM>(node, G, gq, vol[e], lam1, mu1, lam, u, Bp, nm.b);
      if (de_e) de_e[(i64)e * Bp + nm.b] = d;
      s += d;
    }
  if (!de_part) return;   // kernel argument: the whole block leaves together
  store_block_partial(s, de_part, Bp, nm.b, ok, lds);
}

// ---------------------------------------------------------------------------------------
// The same gradient SUMMED OVER THE BATCH, de (m): one wave per element at a time, its lanes walk the samples b < B in a
// fixed order and meet in a fixed-order wave reduction (as element_grad_shared_kernel of element_grad.h).
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void elast_grad_shared_kernel(const int* __restrict__ elems,
                                                                 const double* __restrict__ gtab,
                                                                 const double* __restrict__ vol, double lam1, double mu1,
                                                                 const double* __restrict__ lam,
                                                                 const double* __restrict__ u,
                                                                 const double* __restrict__ g, int m, int B, int Bp,
                                                                 double* __restrict__ de) {
  constexpr int NPE = DIM + 1;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int e = blockIdx.x * 4 + wave; e < m; e += gridDim.x * 4) {
    int node[NPE];
    double G[NPE][DIM], gq[NPE][DIM];
    load_element<DIM>(elems, gtab, g, m, e, node, G, gq);
    const double ve = vol[e];
    double s = 0.0;
    for (int b = lane; b < B; b += kWave)   // padding samples (b >= B) carry no gradient
      s += element_grad<DIM>(node, G, gq, ve, lam1, mu1, lam, u, Bp, b);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) de[e] = s;
  }
}

}  // namespace

// =========================================================================================
// C ABI (include/diffhe_elastic.h)
// =========================================================================================
extern "C" int diffhe_elast_assemble_rows(const double* gtab, const double* vol, int dim, double lam1, double mu1,
                                          const double* E, long long e_se, long long e_sb, const int* ent_ptr,
                                          const int* contrib, const int* cols, const unsigned char* is_bc,
                                          const double* g, double* vals, double* lift, int n, int m, int W, int Bv,
                                          void* stream) {
  if (!gtab || !vol || !E || !ent_ptr || !contrib || !cols || !vals || (dim != 2 && dim != 3) || n < 1 || m < 1 || W < 1)
    return DIFFHE_E_BADARG;
  if ((is_bc == nullptr) != (g == nullptr)) return DIFFHE_E_BADARG;
  if (e_se < 0 || e_sb < 0 || (Bv == 1 && e_sb != 0)) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  if ((long long)n * dim > 2147483647LL / ((long long)dim * W)) return DIFFHE_E_TOOBIG;   // dof entries index as int32 in the ell_* units
  // values, lift, the field
  diffhe::account(8.0 * Bv * ((double)dim * dim * W * n + (lift ? (double)dim * n : 0) + (e_se ? (double)m : 0)));
  const dim3 grid = diffhe::node_grid(n, Bv);
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(elast_assemble_rows_kernel<D()>, grid, dim3(256), 0, (hipStream_t)stream, gtab, vol, lam1, mu1, E,
                       e_se, e_sb, ent_ptr, contrib, cols, is_bc, g, vals, lift, n, m, W, Bv);
  });
  return diffhe::check_launch();
}

extern "C" int diffhe_elast_grad(const int* elems, const double* gtab, const double* vol, int dim, double lam1,
                                 double mu1, const double* lam, const double* u, const double* g, int n, int m, int Bp,
                                 double* de_e, double* de_part, double* de_sum, void* stream) {
  if (!elems || !gtab || !vol || !lam || !u || (dim != 2 && dim != 3) || n < 1 || m < 1) return DIFFHE_E_BADARG;
  if (!de_e && !de_part) return DIFFHE_E_BADARG;
  if ((de_part == nullptr) != (de_sum == nullptr)) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const dim3 grid = diffhe::node_grid(m, Bp);
  if ((int)grid.x != diffhe_grad_kappa_blocks(m, Bp)) return DIFFHE_E_BADARG;   // de_part is sized by that entry
  diffhe::account(8.0 * Bp * (2.0 * dim * n + (de_e ? (double)m : 0)));  // lambda and u once per dof, dE per element
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(elast_grad_kernel<D()>, grid, dim3(256), 0, (hipStream_t)stream, elems, gtab, vol, lam1, mu1, lam,
                       u, g, m, Bp, de_e, de_part);
  });
  if (de_part)
    hipLaunchKernelGGL(diffhe::element_sum_partials_kernel, dim3((Bp + 63) / 64), dim3(256), 0, (hipStream_t)stream,
                       (const double*)de_part, (int)grid.x, Bp, de_sum);
  return diffhe::check_launch();
}

extern "C" int diffhe_elast_grad_shared(const int* elems, const double* gtab, const double* vol, int dim, double lam1,
                                        double mu1, const double* lam, const double* u, const double* g, int n, int m,
                                        int B, int Bp, double* de, void* stream) {
  if (!elems || !gtab || !vol || !lam || !u || !de || (dim != 2 && dim != 3) || n < 1 || m < 1 || B < 1 || B > Bp)
    return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  long long blocks = ((long long)m + 3) / 4;
  if (blocks > 16384) blocks = 16384;
  diffhe::account(8.0 * (Bp * 2.0 * dim * n + (double)m));
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(elast_grad_shared_kernel<D()>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, elems,
                       gtab, vol, lam1, mu1, lam, u, g, m, B, Bp, de);
  });
  return diffhe::check_launch();
}
