// Anisotropic linear elasticity: -div sigma(u) = f, sigma = C eps(u) with a symmetric positive-definite stiffness matrix C
// per element and sample, on P1 triangles and tetrahedra (ours: the reference has scalar unknowns only).  elastic.hip with
// a tensor in place of (lam1, mu1, E): the same dofs, dof(i, a) = i*d + a, the same ELL pattern (include/diffhe_elastic.h),
// the same gradient table (g_p as (npe*d, m), |e| as (m)).
//
// Voigt order (xx, yy, xy) / (xx, yy, zz, yz, xz, xy), NV = 3 / 6, ENGINEERING shear strains: with V(a, t) the Voigt index
// of the unordered pair, eps_V(a,t)(u) collects g_p[t] u_(p,a) from both orders of an off-diagonal pair, so no factor of 2
// appears anywhere:
//
//   K_e[(p,a),(q,b)] = |e| sum_{t,s} g_p[t] C_e[V(a,t)][V(b,s)] g_q[s]
//   dL/dC_IJ[e]      = -|e| (eps_I(lam_h) eps_J(u_h) + [I != J] eps_J(lam_h) eps_I(u_h)),   I <= J
//
// C is stored as its upper triangle, row-major (NT = 6 / 21 components), read through three strides (component, element,
// sample) like the tensor of aniso.hip; an off-diagonal component is ONE parameter that fills both symmetric entries.
//
// Data layout as in elastic.hip: dof-major, batch innermost; lanes over samples with one matrix per sample (Bv = Bp), over
// nodes with one matrix for the batch (Bv = 1).  fp64, no atomics anywhere: every sum has a fixed order, results are
// bitwise reproducible.  The gradient's element loop, its two-stage per-sample total and its batch reduction are the
// kernels of element_grad.h; this unit holds their form, ElastcForm<DIM>.
//
// Last, the row bound of lambda_max(D^-1 A) the solver takes for the Jacobi weights of every level of a hierarchy that
// was built for another operator (diffhe/elastic_aniso.py).
#include "common.h"
#include "diffhe_elastic_aniso.h"
#include "element_grad.h"
#include "launch.h"

namespace {

using namespace diffhe;

// Voigt index of the unordered pair (a, t): the diagonal first, then (0, 1) in 2D and (1, 2), (0, 2), (0, 1) in 3D
template <int DIM>
__host__ __device__ constexpr int voigt(int a, int t) {
  return a == t ? a : DIM * (DIM + 1) / 2 - a - t;
}

// position of entry (I, J) of the symmetric NV x NV matrix in its row-major upper triangle
template <int NV>
__host__ __device__ constexpr int tri(int I, int J) {
  return I <= J ? I * NV - I * (I - 1) / 2 + (J - I) : J * NV - J * (J - 1) / 2 + (I - J);
}

// ---------------------------------------------------------------------------------------
// Block row-gather assembly: elast_assemble_rows_kernel of elastic.hip with the element block above.  Per contribution
// (e, p, q) the lane loads the NT components of C_e, forms Y = C B_q (NV x d: Y[I][b] = sum_s C[I][V(b,s)] g_q[s]) and
// adds |e| B_p^T Y: blk[a][b] += |e| sum_t g_p[t] Y[V(a,t)][b].  Every index below is a compile-time constant after
// unrolling: C, Y and the block live in registers.
// ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void elastc_assemble_rows_kernel(
    const double* __restrict__ gtab, const double* __restrict__ vol, const double* __restrict__ C, i64 csc, i64 cse,
    i64 csb, const int* __restrict__ ent_ptr, const int* __restrict__ contrib, const int* __restrict__ cols,
    const unsigned char* __restrict__ is_bc, const double* __restrict__ g, double* __restrict__ vals,
    double* __restrict__ lift, int n, int m, int W, int Bv) {
  constexpr int NPE = DIM + 1, NV = DIM * (DIM + 1) / 2, NT = NV * (NV + 1) / 2;
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
        double gp[DIM], gq[DIM], Ce[NT], Y[NV][DIM];
        const double ve = vol[e];
#pragma unroll
        for (int t = 0; t < DIM; ++t) {
          gp[t] = ve * gtab[(i64)(p * DIM + t) * m + e];
          gq[t] = gtab[(i64)(q * DIM + t) * m + e];
        }
        const double* __restrict__ Cp = C + (i64)e * cse + (i64)nm.b * csb;
#pragma unroll
        for (int t = 0; t < NT; ++t) Ce[t] = Cp[(i64)t * csc];
#pragma unroll
        for (int I = 0; I < NV; ++I)
#pragma unroll
          for (int b = 0; b < DIM; ++b) {
            double y = 0.0;
#pragma unroll
            for (int s = 0; s < DIM; ++s) y = fma(Ce[tri<NV>(I, voigt<DIM>(b, s))], gq[s], y);
            Y[I][b] = y;
          }
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
          for (int b = 0; b < DIM; ++b)
#pragma unroll
            for (int t = 0; t < DIM; ++t) blk[a][b] = fma(gp[t], Y[voigt<DIM>(a, t)][b], blk[a][b]);
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

// ---------------------------------------------------------------------------------------
// dL/dC: the form of element_grad.h.  Per element the nodes, the Dirichlet values of their dofs (0 without data), the
// gradients g_p and |e|; per sample the displacement gradients H[a][t] = sum_p w[(p, a)] g_p[t] of lam and u, their
// engineering Voigt strains (H[a][a]; H[a][t] + H[t][a]) and the NT products.
// ---------------------------------------------------------------------------------------
template <int DIM>
struct ElastcForm {
  static constexpr int NPE = DIM + 1, NV = DIM * (DIM + 1) / 2, NC = NV * (NV + 1) / 2;
  const int* __restrict__ elems;
  const double* __restrict__ gtab;
  const double* __restrict__ vol;
  const double* __restrict__ lam;
  const double* __restrict__ u;
  const double* __restrict__ g;
  int m;

  struct Elem {
    int node[NPE];
    double G[NPE][DIM], gq[NPE][DIM], ve;
  };

  __device__ __forceinline__ void load(int e, Elem& el) const {
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
      el.node[p] = elems[(i64)p * m + e];
#pragma unroll
      for (int t = 0; t < DIM; ++t) {
        el.G[p][t] = gtab[(i64)(p * DIM + t) * m + e];
        el.gq[p][t] = g ? g[(i64)el.node[p] * DIM + t] : 0.0;
      }
    }
    el.ve = vol[e];
  }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* dc) const {
    double Hl[DIM][DIM], Hu[DIM][DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = 0; t < DIM; ++t) Hl[a][t] = Hu[a][t] = 0.0;
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const i64 o = ((i64)el.node[p] * DIM + a) * Bp + b;
        const double lp = lam[o];
        const double up = u[o] + el.gq[p][a];   // full u: prescribed displacements included
#pragma unroll
        for (int t = 0; t < DIM; ++t) {
          Hl[a][t] = fma(lp, el.G[p][t], Hl[a][t]);
          Hu[a][t] = fma(up, el.G[p][t], Hu[a][t]);
        }
      }
    }
    double sl[NV], su[NV];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int t = a; t < DIM; ++t) {
        sl[voigt<DIM>(a, t)] = a == t ? Hl[a][a] : Hl[a][t] + Hl[t][a];
        su[voigt<DIM>(a, t)] = a == t ? Hu[a][a] : Hu[a][t] + Hu[t][a];
      }
#pragma unroll
    for (int I = 0; I < NV; ++I) {
      const double wl = -el.ve * sl[I], wu = -el.ve * su[I];
      dc[tri<NV>(I, I)] = wl * su[I];
#pragma unroll
      for (int J = I + 1; J < NV; ++J) dc[tri<NV>(I, J)] = fma(wl, su[J], wu * sl[J]);
    }
  }
};

// ---------------------------------------------------------------------------------------
// Row bound.  One lane per (row i, matrix b), b innermost as the values are stored: entry idx = i*Bv + b of slot k sits at
// k*n*Bv + idx.  First stage: the block maxima, part[block]; second stage: one block takes their maximum.  A maximum does
// not depend on the order; NaN and a diagonal that is not positive are turned into +inf before they meet it.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double block_max(double r, double* lds /* 4 doubles */) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) r = fmax(r, __shfl_xor(r, d));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = r;
  __syncthreads();
  return fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
}

__global__ __launch_bounds__(256) void row_bound_kernel(const double* __restrict__ vals, const int* __restrict__ cols,
                                                         int n, int W, int Bv, double* __restrict__ part) {
  __shared__ double lds[4];
  const i64 total = (i64)n * Bv;
  double r = 0.0;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    const int i = (int)(idx / Bv), b = (int)(idx % Bv);
    const double di = vals[idx];
    double s = 0.0;
    for (int k = 0; k < W; ++k) {
      const double v = vals[(i64)k * total + idx];
      const double dj = vals[(i64)cols[(i64)k * n + i] * Bv + b];
      s += fabs(v) / sqrt(di * dj);
    }
    if (!(di > 0.0) || !(s < INFINITY)) s = INFINITY;   // also NaN: neither comparison holds for it
    r = fmax(r, s);
  }
  r = block_max(r, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

__global__ __launch_bounds__(256) void row_bound_final_kernel(const double* __restrict__ part, int nblk,
                                                               double* __restrict__ out) {
  __shared__ double lds[4];
  double r = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) r = fmax(r, part[k]);
  r = block_max(r, lds);
  if (threadIdx.x == 0) out[0] = r;
}

}  // namespace

// =========================================================================================
// C ABI (include/diffhe_elastic_aniso.h)
// =========================================================================================
extern "C" int diffhe_elastc_assemble_rows(const double* gtab, const double* vol, int dim, const double* C,
                                           long long c_sc, long long c_se, long long c_sb, const int* ent_ptr,
                                           const int* contrib, const int* cols, const unsigned char* is_bc,
                                           const double* g, double* vals, double* lift, int n, int m, int W, int Bv,
                                           void* stream) {
  if (!gtab || !vol || !C || !ent_ptr || !contrib || !cols || !vals || (dim != 2 && dim != 3) || n < 1 || m < 1 || W < 1)
    return DIFFHE_E_BADARG;
  if ((is_bc == nullptr) != (g == nullptr)) return DIFFHE_E_BADARG;
  if (c_sc < 0 || c_se < 0 || c_sb < 0 || (Bv == 1 && c_sb != 0)) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  if ((long long)n * dim > 2147483647LL / ((long long)dim * W)) return DIFFHE_E_TOOBIG;   // dof entries index as int32 in the ell_* units
  const int nt = dim == 2 ? 6 : 21;
  // values, lift, the tensor field
  diffhe::account(8.0 * Bv * ((double)dim * dim * W * n + (lift ? (double)dim * n : 0) + (c_se ? (double)nt * m : 0)));
  const dim3 grid = diffhe::node_grid(n, Bv);
  diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(elastc_assemble_rows_kernel<D()>, grid, dim3(256), 0, (hipStream_t)stream, gtab, vol, C, c_sc, c_se,
                       c_sb, ent_ptr, contrib, cols, is_bc, g, vals, lift, n, m, W, Bv);
  });
  return diffhe::check_launch();
}

extern "C" int diffhe_elastc_grad(const int* elems, const double* gtab, const double* vol, int dim, const double* lam,
                                  const double* u, const double* g, int n, int m, int Bp, double* dc_e, long long o_sc,
                                  long long o_se, double* dc_part, double* dc_sum, void* stream) {
  if (!elems || !gtab || !vol || !lam || !u || (dim != 2 && dim != 3) || n < 1 || m < 1) return DIFFHE_E_BADARG;
  if (!dc_e && !dc_part) return DIFFHE_E_BADARG;
  if ((dc_part == nullptr) != (dc_sum == nullptr)) return DIFFHE_E_BADARG;
  const int nt = dim == 2 ? 6 : 21;
  const double bytes = 8.0 * Bp * (2.0 * dim * n + (dc_e ? (double)nt * m : 0));  // lambda and u once per dof, dC per element
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return diffhe::launch_element_grad(ElastcForm<D()>{elems, gtab, vol, lam, u, g, m}, m, Bp, dc_e, o_sc, o_se, dc_part,
                                       dc_sum, bytes, stream);
  });
}

extern "C" int diffhe_elastc_grad_shared(const int* elems, const double* gtab, const double* vol, int dim,
                                         const double* lam, const double* u, const double* g, int n, int m, int B,
                                         int Bp, double* dc, long long o_sc, long long o_se, void* stream) {
  if (!elems || !gtab || !vol || !lam || !u || !dc || (dim != 2 && dim != 3) || n < 1 || m < 1 || B < 1 || B > Bp)
    return DIFFHE_E_BADARG;
  const int nt = dim == 2 ? 6 : 21;
  const double bytes = 8.0 * (Bp * 2.0 * dim * n + (double)nt * m);
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return diffhe::launch_element_grad_shared(ElastcForm<D()>{elems, gtab, vol, lam, u, g, m}, m, B, Bp, dc, o_sc, o_se,
                                              bytes, stream);
  });
}

extern "C" int diffhe_ell_jacobi_row_bound(const double* vals, const int* cols, int n, int W, int Bv, double* part,
                                           double* out, void* stream) {
  if (!vals || !cols || !part || !out || n < 1 || W < 1 || Bv < 1) return DIFFHE_E_BADARG;
  const long long total = (long long)n * Bv;
  if (total > 2147483647LL / W) return DIFFHE_E_TOOBIG;   // the entries of the other ell_* units index as int32 too
  long long blocks = (total + 255) / 256;
  if (blocks > DIFFHE_ROW_BOUND_BLOCKS) blocks = DIFFHE_ROW_BOUND_BLOCKS;
  diffhe::account(8.0 * (double)W * (double)total);
  hipLaunchKernelGGL(row_bound_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, vals, cols, n, W, Bv,
                     part);
  hipLaunchKernelGGL(row_bound_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)part, (int)blocks,
                     out);
  return diffhe::check_launch();
}
