// Lattice fast path: meshes with the connectivity of FEMesh.rectangle (reference mesh.py:79-121;
// node positions may be arbitrary).  The assembled operator is a 7-point stencil, stored as
// SYMMETRIC DIAGONALS (DIA-sym): D0[i] = K[i,i], D1[i] = K[i,i+1], D2[i] = K[i,i+W] (W = nx+1),
// D3[i] = K[i,i+nx] (the quad diagonal b-d; dropped when all triangles are right-angled, where
// it is exactly 0).  No column indices at all; batch-innermost (n, Bp) vectors as in ell.h.
//
// Solver: batched CG preconditioned by one geometric-multigrid V-cycle (P1 interpolation on the
// nested triangulations, R = P^T, re-discretised coarse operators = Galerkin for nested P1,
// damped-Jacobi smoothing, nu_pre = nu_post so the preconditioner is symmetric).  Replaces
// torch.linalg.solve of reference solver.py:174 (forward) and of its autograd backward (adjoint).
//
// Matrix sharing: Bv = Bp (one matrix per sample) or Bv = 1 (one matrix for the batch) with an
// optional per-sample scale s_b on the free rows, K_b = s_b * K_1 -- the exact form of the
// assembled operator when kappa is one scalar per sample (solver.py:88,139: k_e = kappa * k0_e).
//
// This unit is the PRECONDITIONER: the node-loop kernels of the V-cycle, the hierarchy, the operator dispatch, the cycle and
// the full-multigrid start.  The CG around it is lattice_pcg.hip, which reaches this unit through the plain functions
// declared in lattice.h (cycle_*).
#include <stdlib.h>
#include <type_traits>
#include <string.h>

#include "lattice.h"

namespace diffhe_lattice __attribute__((visibility("hidden"))) {
namespace {

// y = A x ; part = per-sample partial of x.y
__global__ __launch_bounds__(256) void dia_apply_dot_kernel(Level L, int Bv, const double* __restrict__ scale,
                                                             const double* __restrict__ x, double* __restrict__ y,
                                                             double* __restrict__ part, int Bp) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const int vb = Bv == 1 ? 0 : nm.b;
  double s = 0.0;
  for (int i = nm.node0; i < L.n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    const double acc = row_scale(L, scale, i, nm.b) * dia_row(L, Bv, vb, x, i, nm.b, Bp) + shift_at(L, i) * x[o];
    y[o] = acc;
    s += acc * x[o];
  }
  STORE_PARTIAL(part, s);
}

// r = b - A x ; optional part = per-sample partial of r.r
template <typename TV>
__global__ __launch_bounds__(256) void dia_residual_kernel(Level L, int Bv, const double* __restrict__ scale,
                                                            const TV* __restrict__ bvec, const TV* __restrict__ x,
                                                            TV* __restrict__ r, double* __restrict__ part, int Bp,
                                                            int dot_bx = 0, double* __restrict__ part2 = nullptr) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const int vb = Bv == 1 ? 0 : nm.b;
  double s = 0.0, s2 = 0.0;
  for (int i = nm.node0; i < L.n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    const double bi = (double)bvec[o];
    const double ri = bi - (row_scale(L, scale, i, nm.b) * dia_row(L, Bv, vb, x, i, nm.b, Bp) + shift_at(L, i) * (double)x[o]);
    if (r) r[o] = (TV)ri;
    s += dot_bx ? bi * (double)x[o] : ri * ri;   // dot_bx: b.x ...
    if (dot_bx) s2 += (double)x[o] * (bi - ri);  // ... and x.(A x): together a lower bound of the solution's energy
  }
  if (part) STORE_PARTIAL(part, s);
  if (part2) STORE_PARTIAL(part2, s2);
}

// damped Jacobi: xout = xin + omega (b - A xin) / D   (xin == NULL: xin = 0)
// optional part = per-sample partial of b.xout  (the r.z dot of the CG, fused into the last sweep)
template <typename TV>
__global__ __launch_bounds__(256) void dia_jacobi_kernel(Level L, int Bv, const double* __restrict__ scale,
                                                          const TV* __restrict__ bvec, const TV* __restrict__ xin,
                                                          TV* __restrict__ xout, double omega,
                                                          double* __restrict__ part, int Bp) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const int vb = Bv == 1 ? 0 : nm.b;
  double s = 0.0;
  for (int i = nm.node0; i < L.n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    const double sc = row_scale(L, scale, i, nm.b);
    const double sh = shift_at(L, i);
    const double dinv = fast_rcp(sc * L.v[(i64)i * Bv + vb] + sh);  // same reciprocal as the strip kernels
    const double bi = (double)bvec[o];
    double xo;
    if (xin)
      xo = (double)xin[o] + omega * (bi - (sc * dia_row(L, Bv, vb, xin, i, nm.b, Bp) + sh * (double)xin[o])) * dinv;
    else
      xo = omega * bi * dinv;
    xout[o] = (TV)xo;
    s += bi * xo;
  }
  if (part) STORE_PARTIAL(part, s);
}

// One step of the Chebyshev semi-iteration (three-term form) on the coarsest level:
//   d_out = c1 d_in + c2 D^-1 (b - A x_in) ;  x_out = x_in + d_out        (d_in == NULL: c1 = 0)
// part (optional): per-sample partial of b.x_out, as in dia_jacobi_kernel.
template <typename TV>
__global__ __launch_bounds__(256) void dia_cheby_kernel(Level L, int Bv, const double* __restrict__ scale,
                                                         const TV* __restrict__ bvec, const TV* __restrict__ xin,
                                                         const TV* __restrict__ din, TV* __restrict__ xout,
                                                         TV* __restrict__ dout, double c1, double c2,
                                                         double* __restrict__ part, int Bp) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const int vb = Bv == 1 ? 0 : nm.b;
  double s = 0.0;
  for (int i = nm.node0; i < L.n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    const double sc = row_scale(L, scale, i, nm.b);
    const double sh = shift_at(L, i);
    const double dinv = fast_rcp(sc * L.v[(i64)i * Bv + vb] + sh);
    const double bi = (double)bvec[o];
    const double xi = xin ? (double)xin[o] : 0.0;
    const double res = xin ? bi - (sc * dia_row(L, Bv, vb, xin, i, nm.b, Bp) + sh * xi) : bi;
    const double dn = (din ? c1 * (double)din[o] : 0.0) + c2 * res * dinv;
    dout[o] = (TV)dn;
    const double xo = xi + dn;
    xout[o] = (TV)xo;
    s += bi * xo;
  }
  if (part) STORE_PARTIAL(part, s);
}

// Coarsening of a level pair: both directions (2:1 nested triangulations, P = P1 interpolation with the
// quad-diagonal midpoints) or ONE direction only (semi-coarsening, used while the mesh is anisotropic:
// P = 1D linear interpolation along the coarsened direction).
__device__ inline int coarsen_x(const Level& F, const Level& C) { return F.nx == 2 * C.nx ? 2 : 1; }
__device__ inline int coarsen_y(const Level& F, const Level& C) { return F.ny == 2 * C.ny ? 2 : 1; }

// coarse rhs = P^T r, 0 on coarse Dirichlet rows
template <typename TV>
__global__ __launch_bounds__(256) void mg_restrict_kernel(Level F, Level C, const TV* __restrict__ r,
                                                           TV* __restrict__ rc, int Bp) {
  const NodeMap nm = node_map(Bp);
  const int sx = coarsen_x(F, C), sy = coarsen_y(F, C);
  for (int I = nm.node0; I < C.n; I += nm.stride) {
    double out = 0.0;
    if (!C.bc[I]) {
      const int ci = I / C.W, cj = I - ci * C.W;
      const int fi = sy * ci, fj = sx * cj;
      const i64 c = (i64)fi * F.W + fj;
      double h = 0.0;
      if (sx == 2) {
        if (fj > 0) h += (double)r[(c - 1) * Bp + nm.b];
        if (fj < F.nx) h += (double)r[(c + 1) * Bp + nm.b];
      }
      if (sy == 2) {
        if (fi > 0) h += (double)r[(c - F.W) * Bp + nm.b];
        if (fi < F.ny) h += (double)r[(c + F.W) * Bp + nm.b];
      }
      if (sx == 2 && sy == 2) {  // midpoints of the quad diagonals b-d
        if (fi > 0 && fj < F.nx) h += (double)r[(c - F.W + 1) * Bp + nm.b];
        if (fi < F.ny && fj > 0) h += (double)r[(c + F.W - 1) * Bp + nm.b];
      }
      out = (double)r[c * Bp + nm.b] + 0.5 * h;
    }
    rc[(i64)I * Bp + nm.b] = (TV)out;
  }
}

// x += P e  (0 on fine Dirichlet rows)
template <typename TV>
__global__ __launch_bounds__(256) void mg_prolong_add_kernel(Level F, Level C, const TV* __restrict__ e,
                                                              TV* __restrict__ x, int Bp, int set = 0) {
  const NodeMap nm = node_map(Bp);
  for (int i = nm.node0; i < F.n; i += nm.stride) {
    if (F.bc[i]) {
      if (set) x[(i64)i * Bp + nm.b] = (TV)0.0;
      continue;
    }
    const int fi = i / F.W, fj = i - fi * F.W;
    const int sx = coarsen_x(F, C), sy = coarsen_y(F, C);
    const bool oi = sy == 2 && (fi & 1), oj = sx == 2 && (fj & 1);  // between two coarse rows / columns
    const int ci = sy == 2 ? fi >> 1 : fi, cj = sx == 2 ? fj >> 1 : fj;
    const i64 c = (i64)ci * C.W + cj;
    double v;
    if (!oi && !oj)
      v = (double)e[c * Bp + nm.b];
    else if (!oi)
      v = 0.5 * ((double)e[c * Bp + nm.b] + (double)e[(c + 1) * Bp + nm.b]);
    else if (!oj)
      v = 0.5 * ((double)e[c * Bp + nm.b] + (double)e[(c + C.W) * Bp + nm.b]);
    else  // midpoint of the quad diagonal b-d (full coarsening only)
      v = 0.5 * ((double)e[(c + 1) * Bp + nm.b] + (double)e[(c + C.W) * Bp + nm.b]);
    x[(i64)i * Bp + nm.b] = set ? (TV)v : (TV)((double)x[(i64)i * Bp + nm.b] + v);
  }
}

// The two transfers for fp32 vectors, full coarsening and batches that are multiples of 128: a wave owns ONE node and 128
// samples (8-byte accesses), the node index and everything derived from it (row / column, parities, Dirichlet flag,
// coarse index) is wave-uniform scalar arithmetic instead of one integer division per lane.  Same fp64 arithmetic per
// sample as mg_prolong_add_kernel / mg_restrict_kernel: bitwise the same values.
__global__ __launch_bounds__(256) void mg_prolong2_kernel(Level F, Level C, const float* __restrict__ e,
                                                           float* __restrict__ x, int Bp, int set) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lb = blockIdx.y * (2 * kWave) + 2 * lane;
  for (int i = blockIdx.x * 4 + wave; i < F.n; i += gridDim.x * 4) {
    float* __restrict__ px = x + (i64)i * Bp + lb;
    if (F.bc[i]) {
      if (set) *(v2f*)px = v2f{0.0f, 0.0f};
      continue;
    }
    const int fi = i / F.W, fj = i - fi * F.W;
    const bool oi = fi & 1, oj = fj & 1;
    const float* __restrict__ pe = e + ((i64)(fi >> 1) * C.W + (fj >> 1)) * Bp + lb;
    double v0, v1;
    if (!oi && !oj) {
      const v2f a = *(const v2f*)pe;
      v0 = (double)a.x; v1 = (double)a.y;
    } else {
      const v2f a = *(const v2f*)(pe + ((oi && oj) ? (i64)Bp : 0));                       // c (or c + 1 on a quad diagonal)
      const v2f b = *(const v2f*)(pe + (!oi ? (i64)Bp : (i64)C.W * Bp));                  // c + 1 (odd column only) or c + C.W
      v0 = 0.5 * ((double)a.x + (double)b.x);
      v1 = 0.5 * ((double)a.y + (double)b.y);
    }
    if (set) {
      *(v2f*)px = v2f{(float)v0, (float)v1};
    } else {
      const v2f o = *(const v2f*)px;
      *(v2f*)px = v2f{(float)((double)o.x + v0), (float)((double)o.y + v1)};
    }
  }
}

__global__ __launch_bounds__(256) void mg_restrict2_kernel(Level F, Level C, const float* __restrict__ r,
                                                            float* __restrict__ rc, int Bp) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lb = blockIdx.y * (2 * kWave) + 2 * lane;
  for (int I = blockIdx.x * 4 + wave; I < C.n; I += gridDim.x * 4) {
    float* __restrict__ po = rc + (i64)I * Bp + lb;
    if (C.bc[I]) {
      *(v2f*)po = v2f{0.0f, 0.0f};
      continue;
    }
    const int ci = I / C.W, cj = I - ci * C.W;
    const int fi = 2 * ci, fj = 2 * cj;
    const float* __restrict__ pc = r + ((i64)fi * F.W + fj) * Bp + lb;
    const i64 row = (i64)F.W * Bp;
    double h0 = 0.0, h1 = 0.0;
    auto acc = [&](const float* q) { const v2f t = *(const v2f*)q; h0 += (double)t.x; h1 += (double)t.y; };
    if (fj > 0) acc(pc - Bp);
    if (fj < F.nx) acc(pc + Bp);
    if (fi > 0) acc(pc - row);
    if (fi < F.ny) acc(pc + row);
    if (fi > 0 && fj < F.nx) acc(pc - row + Bp);
    if (fi < F.ny && fj > 0) acc(pc + row - Bp);
    const v2f cc = *(const v2f*)pc;
    *(v2f*)po = v2f{(float)((double)cc.x + 0.5 * h0), (float)((double)cc.y + 0.5 * h1)};
  }
}

// The right-hand side of a cold full-multigrid start in ONE pass: r32 = (float)(rs b), what pcg_cvt_kernel stores, and the
// level-1 right-hand side R r32, what mg_restrict2_kernel / mg_restrict_kernel form from it -- the same per-sample
// expression on the ROUNDED values in the same order of additions (W, E, S, N, SE-of-the-row-above, SW-of-the-row-below;
// centre + h / 2), so both vectors are bit for bit theirs.  Strip-shaped like the F_RESTRICT passes: a wave owns two coarse
// columns x 64 samples and marches down the coarse rows of its tile holding the fine rows 2 I - 1, 2 I, 2 I + 1 at the five
// fine columns 2 J0 - 1 .. 2 J0 + 3; it stores r32 on the rows 2 I, 2 I + 1 and the columns 2 J0 .. 2 J0 + 3 (each fine
// node has exactly one owner; the halo column and row are read again: L2).  Full coarsening only.
__global__ __launch_bounds__(256) void cvt_restrict_kernel(Level F, Level C, const double* __restrict__ b,
                                                            const double* __restrict__ rs, float* __restrict__ r32,
                                                            float* __restrict__ rc, int Bp, int ncb, int TR) {
  constexpr int CW = 2, NC = 2 * CW + 1;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lb = blockIdx.y * kWave + lane;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int tr = tile / ncb, cb = tile - tr * ncb;
  const int J0 = (cb * 4 + wave) * CW, I0 = tr * TR;
  const int I1 = (I0 + TR < C.ny + 1) ? I0 + TR : C.ny + 1;
  if (J0 >= C.W || I0 >= I1) return;
  const double sc = rs ? rs[lb] : 1.0;
  const int c0 = 2 * J0 - 1;   // fine column of window index 0
  // fine row `row` at the window's columns, rounded; `own`: this wave stores its columns 1 .. NC - 1
  auto load_row = [&](int row, float* dst, bool own) {
    const bool rok = row >= 0 && row <= F.ny;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int c = c0 + k;
      float v = 0.0f;
      if (rok && c >= 0 && c < F.W) {
        const i64 o = ((i64)row * F.W + c) * Bp + lb;
        v = (float)(b[o] * sc);
        if (own && k > 0) r32[o] = v;
      }
      dst[k] = v;
    }
  };
  float pm[NC], cu[NC], nx[NC];
  load_row(2 * I0 - 1, pm, false);   // the tile above owns it (row -1: zeros, never used)
  for (int I = I0; I < I1; ++I) {
    const int fi = 2 * I;
    load_row(fi, cu, true);
    load_row(fi + 1, nx, true);
#pragma unroll
    for (int j = 0; j < CW; ++j) {
      const int J = J0 + j, fj = 2 * J, k = 2 * j + 1;
      if (J >= C.W) continue;
      const i64 Ic = (i64)I * C.W + J;
      double out = 0.0;
      if (!C.bc[Ic]) {
        double h = 0.0;
        if (fj > 0) h += (double)cu[k - 1];
        if (fj < F.nx) h += (double)cu[k + 1];
        if (fi > 0) h += (double)pm[k];
        if (fi < F.ny) h += (double)nx[k];
        if (fi > 0 && fj < F.nx) h += (double)pm[k + 1];
        if (fi < F.ny && fj > 0) h += (double)nx[k - 1];
        out = (double)cu[k] + 0.5 * h;
      }
      rc[Ic * Bp + lb] = (float)out;
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) pm[k] = nx[k];
  }
}

inline bool transfers2_ok(const Level& F, const Level& C, int Bp, size_t esz) {
  return esz == 4 && F.nx == 2 * C.nx && F.ny == 2 * C.ny && Bp % (2 * kWave) == 0;
}
inline dim3 transfer2_grid(int n, int Bp) { return dim3((unsigned)(((i64)n + 3) / 4 < 4096 ? ((i64)n + 3) / 4 : 4096), Bp / (2 * kWave)); }


// Gershgorin bound of D^-1 A: max over rows (and samples) of sum_j |a_ij| / a_ii, as the bit pattern of a
// non-negative double (ordered like an unsigned integer, so atomicMax gives a deterministic result).
// Meshes with obtuse triangles have positive off-diagonal entries and a spectrum that reaches beyond 2.
__global__ __launch_bounds__(256) void dia_gershgorin_kernel(Level L, int Bv, unsigned long long* __restrict__ out) {
  const NodeMap nm = node_map(Bv);
  const i64 n = L.n;
  double m = 0.0;
  if (nm.b < Bv) {
    for (int i = nm.node0; i < L.n; i += nm.stride) {
      double sum = 0.0;
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        if (k < L.nd) {
          const int off = dia_off(L, k);
          if (i + off < L.n) sum += fabs(L.v[((i64)k * n + i) * Bv + nm.b]);
          if (i - off >= 0) sum += fabs(L.v[((i64)k * n + (i - off)) * Bv + nm.b]);
        }
      }
      const double r = 1.0 + sum / L.v[(i64)i * Bv + nm.b];
      m = r > m ? r : m;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double o = __shfl_xor(m, d);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(out, (unsigned long long)__double_as_longlong(m));
}

// y += x (TV)
template <typename TV>
__global__ __launch_bounds__(256) void mg_add_kernel(const TV* __restrict__ x, TV* __restrict__ y, int n, int Bp) {
  const NodeMap nm = node_map(Bp);
  for (int i = nm.node0; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    y[o] = (TV)((double)y[o] + (double)x[o]);
  }
}

// Per-sample max of the matrix diagonal (bit pattern of a non-negative double, atomicMax: deterministic).
// out has Bv entries, zeroed by the caller.
__global__ __launch_bounds__(256) void dia_maxdiag_kernel(Level L, int Bv, unsigned long long* __restrict__ out) {
  const NodeMap nm = node_map(Bv);
  double m = 0.0;
  if (nm.b < Bv)
    for (int i = nm.node0; i < L.n; i += nm.stride) {
      const double d = L.v[(i64)i * Bv + nm.b];
      m = d > m ? d : m;
    }
  const int LB = Bv < kWave ? Bv : kWave;
  for (int off = LB; off < kWave; off <<= 1) {  // lanes that hold the same sample
    const double o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  if ((int)(threadIdx.x & 63) < LB && nm.b < Bv) atomicMax(out + nm.b, (unsigned long long)__double_as_longlong(m));
}

// ---- operator dispatch: strip kernels on big levels, simple kernels on small ones ----------------
// Each returns the number of partial blocks it wrote (when `part` != NULL).  TV is the storage
// type of the vectors (double, or float inside a single-precision preconditioner); arithmetic is
// always fp64 in registers.
template <typename TV>
int op_jacobi(const Hier& H, int l, const TV* rhs, const TV* xin, TV* xout, double omega, double* part,
              hipStream_t st) {
  const Level& L = H.lev[l];
  // the plain sweep runs at the HBM rate of its real traffic either way (0.69 ms one sample per lane, 0.70-0.72 two):
  // it keeps the one-sample kernel
  const StripGeom g = strip_geom(L, H.Bp, strip_cols<TV>());
  if (g.use && xin) {
    if (l == 0) kp_begin(KP_SWEEP, st);
    launch_strip<TV, M_JACOBI, false, F_NONE, TV, strip_cols<TV>()>(L, H.Bv, H.scale, xin, rhs, xout, omega, 0.0, part,
                                                                   H.Bp, g, st);
    if (l == 0) kp_end(KP_SWEEP, st);
    return g.ncb * g.nrc;
  }
  launch_nodes(H, st, (xin ? 3 : 2) * sizeof(TV) + mat_bytes(H, L), dia_jacobi_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, xin, xout, omega, part, H.Bp);
  return lgrid(L.n, H.Bp).x;
}

// two sweeps from a zero guess in one pass over rhs: x1 = w0 D^-1 rhs is formed on the fly
template <typename TV>
int op_jacobi_first2(const Hier& H, int l, const TV* rhs, TV* xa, TV* xb, double w0, double w1, double* part,
                     TV** result, hipStream_t st) {
  const Level& L = H.lev[l];
  StripGeom g;
  const bool two = strip2_pick<TV>(L, H.Bv, H.Bp, strip_cols<TV>(), &g);
  if (g.use) {
    if (l == 0) kp_begin(KP_FIRST2, st);
    if (two)
      launch_strip2<M_JACOBI, true, F_NONE, 4>(L, H.scale, (const float*)nullptr, (const float*)rhs, (float*)xa, w1, w0,
                                               part, H.Bp, g, st);
    else
      launch_strip<TV, M_JACOBI, true, F_NONE, TV, strip_cols<TV>()>(L, H.Bv, H.scale, (const TV*)nullptr, rhs, xa, w1, w0,
                                                                    part, H.Bp, g, st);
    if (l == 0) kp_end(KP_FIRST2, st);
    *result = xa;
    return g.ncb * g.nrc;
  }
  launch_nodes(H, st, 2 * sizeof(TV) + mat_bytes(H, L) / L.nd, dia_jacobi_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, (const TV*)nullptr, xa, w0, (double*)nullptr, H.Bp);
  launch_nodes(H, st, 3 * sizeof(TV) + mat_bytes(H, L), dia_jacobi_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, (const TV*)xa, xb, w1, part, H.Bp);
  *result = xb;
  return lgrid(L.n, H.Bp).x;
}

template <typename TV>
int op_residual(const Hier& H, int l, const TV* rhs, const TV* x, TV* res, double* part, hipStream_t st,
                int dot_bx = 0, double* part2 = nullptr) {
  const Level& L = H.lev[l];
  const StripGeom g = strip_geom(L, H.Bp);
  if (g.use) {
    Extra ex{};
    ex.dot_bx = dot_bx;
    ex.part2 = part2;
    launch_strip<TV, M_RESID, false>(L, H.Bv, H.scale, x, rhs, res, 0.0, 0.0, part, H.Bp, g, st, ex);
    return g.ncb * g.nrc;
  }
  launch_nodes(H, st, (res ? 3 : 2) * sizeof(TV) + mat_bytes(H, L), dia_residual_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, x, res, part, H.Bp,
         dot_bx, part2);
  return lgrid(L.n, H.Bp).x;
}

int op_apply_dot(const Hier& H, const double* x, double* y, double* part, hipStream_t st) {
  const Level& L = H.lev[0];
  const StripGeom g = strip_geom(L, H.Bp);
  if (g.use) {
    launch_strip<double, M_APPLY, false>(L, H.Bv, H.scale, x, (const double*)nullptr, y, 0.0, 0.0, part, H.Bp, g, st);
    return g.ncb * g.nrc;
  }
  launch_nodes(H, st, 16.0 + mat_bytes(H, L), dia_apply_dot_kernel, L.n, L, H.Bv, H.scale, x, y, part, H.Bp);
  return lgrid(L.n, H.Bp).x;
}

// Coarsest-level solve with a precomputed dense inverse of the batch-shared level matrix (K_1 of a factored
// operator, plan-constant): x[i, b] = (1 / s_b) sum_j inv[i, j] rhs[j, b].  A wave owns RPW rows x 64 samples: rhs is
// read once per wave (lanes over samples, 256-512 B per load, L2-resident at these sizes), the inverse arrives as
// wave-uniform scalar loads.  33^2 nodes x 256 samples: 3e8 multiply-adds in ONE launch instead of the ~45 launches
// (5 levels of sweeps, transfers and the Chebyshev solve of the 3 x 3 grid) it replaces -- those were
// launch-latency-bound at ~5 us each.  Exact (to fp32/fp64 rounding) and symmetric, so the cycle stays an SPD
// preconditioner.
template <typename TV, int RPB>
__global__ __launch_bounds__(256) void mg_dense_solve_kernel(int n, const TV* __restrict__ inv,
                                                              const double* __restrict__ scale,
                                                              const TV* __restrict__ rhs, TV* __restrict__ x,
                                                              double* __restrict__ part, int Bp) {
  // block = RPB rows x 64 samples; its 4 waves split the sum over j (a quarter each, 4 loads in flight per wave:
  // one wave per SIMD with one dependent L2 load per step ran 260 us), partial rows meet in LDS
  __shared__ double red[4 * RPB * kWave];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y * kWave + lane;
  const int i0 = blockIdx.x * RPB;
  const int nq = (n + 3) / 4;
  const int j0 = wave * nq, j1 = (j0 + nq < n) ? j0 + nq : n;
  double acc[RPB];
#pragma unroll
  for (int r = 0; r < RPB; ++r) acc[r] = 0.0;
  const TV* __restrict__ row[RPB];
#pragma unroll
  for (int r = 0; r < RPB; ++r) row[r] = inv + (i64)(i0 + r < n ? i0 + r : n - 1) * n;
  const TV* __restrict__ rb = rhs + b;
  int j = j0;
  for (; j + 4 <= j1; j += 4) {
    const double v0 = (double)rb[(i64)j * Bp], v1 = (double)rb[(i64)(j + 1) * Bp];
    const double v2 = (double)rb[(i64)(j + 2) * Bp], v3 = (double)rb[(i64)(j + 3) * Bp];
#pragma unroll
    for (int r = 0; r < RPB; ++r)
      acc[r] += ((double)row[r][j] * v0 + (double)row[r][j + 1] * v1) + ((double)row[r][j + 2] * v2 + (double)row[r][j + 3] * v3);
  }
  for (; j < j1; ++j) {
    const double v = (double)rb[(i64)j * Bp];
#pragma unroll
    for (int r = 0; r < RPB; ++r) acc[r] += (double)row[r][j] * v;
  }
#pragma unroll
  for (int r = 0; r < RPB; ++r) red[(wave * RPB + r) * kWave + lane] = acc[r];
  __syncthreads();
  double s = 0.0;
  if (wave == 0) {
    const double si = scale ? 1.0 / scale[b] : 1.0;
#pragma unroll
    for (int r = 0; r < RPB; ++r) {
      if (i0 + r < n) {
        const double t = (red[r * kWave + lane] + red[(RPB + r) * kWave + lane]) +
                         (red[(2 * RPB + r) * kWave + lane] + red[(3 * RPB + r) * kWave + lane]);
        const double xo = si * t;
        x[(i64)(i0 + r) * Bp + b] = (TV)xo;
        s += (double)rb[(i64)(i0 + r) * Bp] * xo;
      }
    }
    if (part) part[(i64)blockIdx.x * Bp + b] = s;  // rhs . x partials (only when this level is the whole cycle)
  }
}

// The same product on the matrix cores (fp32 storage only): X (n x Bp) = inv (n x n) . R (n x Bp) is a plain GEMM, the one
// GEMM-shaped piece of the path.  v_mfma_f32_32x32x2_f32: a block owns 32 rows x 32 samples, its 4 waves split the sum
// over j and meet in LDS.  A-operand: lane l supplies inv[i0 + l % 32][j + l / 32] -- read as inv[j + l / 32][i0 + l % 32]
// (the inverse of a symmetric matrix is symmetric), so the 32 lanes of a half-wave read 128 contiguous bytes;
// B-operand: rhs[j + l / 32][b0 + l % 32], contiguous as well.  Accumulates in fp32 where the scalar kernel above
// accumulates in fp64: inside an fp32-stored preconditioner the 1e-6 this costs on the coarsest-level solve is immaterial
// (same iteration counts, tests/test_robustness.py).  D layout: lane l holds column l % 32, rows 8 (v / 4) + 4 (l / 32) + v % 4.
typedef float f16v __attribute__((ext_vector_type(16)));
template <int NW>
__global__ __launch_bounds__(64 * NW) void mg_dense_mfma_kernel(int n, const float* __restrict__ inv,
                                                             const double* __restrict__ scale,
                                                             const float* __restrict__ rhs, float* __restrict__ x, int Bp) {
  __shared__ float red[NW - 1][16][kWave];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int il = lane & 31, kh = lane >> 5;
  const int i0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int ia = (i0 + il < n) ? i0 + il : n - 1;
  const float* __restrict__ pa = inv + ia;
  const float* __restrict__ pb = rhs + b0 + il;
  const int nkp = (n + 1) >> 1, q = (nkp + NW - 1) / NW;
  const int kp0 = wave * q, kp1 = (kp0 + q < nkp) ? kp0 + q : nkp;
  f16v acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
  int kp = kp0;
  for (; kp + 4 <= kp1; kp += 4) {
    float a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = 2 * (kp + u) + kh;
      const bool ok = j < n;
      const int jj = ok ? j : 0;
      a[u] = ok ? pa[(i64)jj * n] : 0.0f;
      b[u] = ok ? pb[(i64)jj * Bp] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
  }
  for (; kp < kp1; ++kp) {
    const int j = 2 * kp + kh;
    const bool ok = j < n;
    const int jj = ok ? j : 0;
    const float a = ok ? pa[(i64)jj * n] : 0.0f;
    const float b = ok ? pb[(i64)jj * Bp] : 0.0f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  if (wave > 0) {
#pragma unroll
    for (int v = 0; v < 16; ++v) red[wave - 1][v][lane] = acc[v];
  }
  __syncthreads();
  if (wave == 0) {
    const float si = scale ? (float)(1.0 / scale[b0 + il]) : 1.0f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int i = i0 + 8 * (v >> 2) + 4 * kh + (v & 3);
      float t = acc[v];
#pragma unroll
      for (int w = 0; w < NW - 1; ++w) t += red[w][v][lane];
      if (i < n) x[(i64)i * Bp + b0 + il] = si * t;
    }
  }
}

// The same product for batches below a wave (Bp = 1 .. 32, the unbatched call shape of the reference): one wave per
// row, lanes over the columns j, a wave reduction per sample.
template <typename TV>
__global__ __launch_bounds__(64) void mg_dense_small_kernel(int n, const TV* __restrict__ inv,
                                                             const double* __restrict__ scale,
                                                             const TV* __restrict__ rhs, TV* __restrict__ x,
                                                             double* __restrict__ part, int Bp) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const TV* __restrict__ row = inv + (i64)i * n;
  for (int b = 0; b < Bp; ++b) {
    double s = 0.0;
    for (int j = lane; j < n; j += kWave) s += (double)row[j] * (double)rhs[(i64)j * Bp + b];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) {
      const double xo = (scale ? 1.0 / scale[b] : 1.0) * s;
      x[(i64)i * Bp + b] = (TV)xo;
      if (part) part[(i64)i * Bp + b] = (double)rhs[(i64)i * Bp + b] * xo;   // one partial row per matrix row
    }
  }
}

// Coarsest-level solve: Chebyshev semi-iteration for D^-1 A with the spectrum bounds of the P1 Laplacian
// on an nx x ny lattice, lambda in [ (1 - cos(pi/nx))/2 + (1 - cos(pi/ny))/2 , 2 ]; the lower bound is halved
// for safety (below it the polynomial stays < 1, it only damps less).  The degree follows from the size, so a
// 3 x 3 coarsest grid costs ~5 steps and a 125 x 125 one (sizes that cannot be halved further) ~170 --
// a fixed polynomial in A, hence still a symmetric preconditioner.  Returns the solution buffer.
template <typename TV>
TV* coarse_solve(const Hier& H, int l, const TV* rhs, double* part, int* nblocks, hipStream_t st) {
  const Level& L = H.lev[l];
  if (L.inv && H.Bv == 1 && L.n <= kPartBlocks) {  // dense inverse of the shared level matrix: one launch
    diffhe::account(2.0 * sizeof(TV) * (double)L.n * H.Bp);
    if (H.dense_mfma && sizeof(TV) == 4 && H.Bp >= kWave && !part) {
      // 8 waves per 32 x 32 tile split the sum over j: 1089 nodes x 256 samples = 280 blocks, a chain of 17 dependent
      // 4-step groups per wave (4 waves: 28 us, the scalar fp64-accumulating kernel: 51 us)
      hipLaunchKernelGGL(mg_dense_mfma_kernel<8>, dim3((L.n + 31) / 32, H.Bp / 32), dim3(512), 0, st, L.n, (const float*)L.inv,
                         H.scale, (const float*)rhs, (float*)H.xa[l], H.Bp);
      if (nblocks) *nblocks = 0;
    } else if (H.Bp >= kWave) {
      constexpr int RPB = 4;
      const dim3 grid((L.n + RPB - 1) / RPB, H.Bp / kWave);
      hipLaunchKernelGGL((mg_dense_solve_kernel<TV, RPB>), grid, dim3(256), 0, st, L.n, (const TV*)L.inv, H.scale, rhs,
                         (TV*)H.xa[l], part, H.Bp);
      if (nblocks) *nblocks = grid.x;
    } else {
      hipLaunchKernelGGL(mg_dense_small_kernel<TV>, dim3(L.n), dim3(64), 0, st, L.n, (const TV*)L.inv, H.scale, rhs,
                         (TV*)H.xa[l], part, H.Bp);
      if (nblocks) *nblocks = L.n;
    }
    return (TV*)H.xa[l];
  }
  const double pi = 3.14159265358979323846;
  const double lmin = 0.5 * (0.5 * (1.0 - cos(pi / L.nx)) + 0.5 * (1.0 - cos(pi / L.ny)));
  const double lmax = H.coarse_lmax;
  int deg = (int)ceil(1.5 * sqrt(lmax / lmin));
  if (deg < H.n_coarse) deg = H.n_coarse;
  if (deg > 400) deg = 400;
  const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
  TV* xa = (TV*)H.xa[l];
  TV* xb = (TV*)H.xb[l];
  TV* d = (TV*)H.res[l];  // the coarsest level never restricts: its residual buffer holds d
  double rho = 1.0 / sigma;
  launch_nodes(H, st, 3 * sizeof(TV) + mat_bytes(H, L) / L.nd, dia_cheby_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, (const TV*)nullptr, (const TV*)nullptr, xa, d, 0.0,
         1.0 / theta, (deg == 1) ? part : (double*)nullptr, H.Bp);
  for (int k = 1; k < deg; ++k) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    launch_nodes(H, st, 5 * sizeof(TV) + mat_bytes(H, L), dia_cheby_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, (const TV*)xa, (const TV*)d, xb, d, rho_new * rho,
           2.0 * rho_new / delta, (k == deg - 1) ? part : (double*)nullptr, H.Bp);
    rho = rho_new;
    TV* t = xa; xa = xb; xb = t;
  }
  if (nblocks) *nblocks = lgrid(L.n, H.Bp).x;
  return xa;
}

template <typename TV>
void launch_restrict(const Hier& H, const Level& F, const Level& C, const TV* r, TV* rc, hipStream_t st) {
  if (transfers2_ok(F, C, H.Bp, sizeof(TV))) {
    diffhe::account(((double)F.n / C.n + 1.0) * sizeof(TV) * (double)C.n * H.Bp);
    hipLaunchKernelGGL(mg_restrict2_kernel, transfer2_grid(C.n, H.Bp), dim3(256), 0, st, F, C, (const float*)r, (float*)rc, H.Bp);
  } else {
    launch_nodes(H, st, ((double)F.n / C.n + 1.0) * sizeof(TV), mg_restrict_kernel<TV>, C.n, F, C, r, rc, H.Bp);
  }
}

template <typename TV>
void launch_prolong(const Hier& H, const Level& F, const Level& C, const TV* e, TV* x, int set, hipStream_t st) {
  if (transfers2_ok(F, C, H.Bp, sizeof(TV))) {
    diffhe::account(((set ? 1.0 : 2.0) + (double)C.n / F.n) * sizeof(TV) * (double)F.n * H.Bp);
    hipLaunchKernelGGL(mg_prolong2_kernel, transfer2_grid(F.n, H.Bp), dim3(256), 0, st, F, C, (const float*)e, (float*)x, H.Bp, set);
  } else {
    launch_nodes(H, st, ((set ? 1.0 : 2.0) + (double)C.n / F.n) * sizeof(TV), mg_prolong_add_kernel<TV>, F.n, F, C, e, x, H.Bp, set);
  }
}

// residual + full-weighting restriction of level l in one pass (the residual is never stored): H.rhs[l + 1] = R (rhs - A x)
template <typename TV>
void resid_restrict(const Hier& H, int l, const TV* x, const TV* rhs_l, hipStream_t st) {
  const Level& L = H.lev[l];
  const Level& C = H.lev[l + 1];
  constexpr int CW = kRestrictCols;
  bool two = sizeof(TV) == 4 && strip2_ok(L, H.Bv, H.Bp);
  StripGeom g;
  for (int pass = 0; pass < 2; ++pass) {
    // tiles of coarse rows, at least 4 in the mean; no partial sums
    g = tile_geom(C.ny + 1, (C.W + 4 * CW - 1) / (4 * CW), H.Bp / (two ? 2 * kWave : kWave), kStripBlocks, 4, 0);
    if (!two || strip2_tile_fits(L, H.Bp, 2 * g.TR + 1)) break;
    two = false;                         // tiles beyond 32-bit offsets: the one-sample-per-lane kernel
  }
  Extra ex{};
  ex.cW = C.W;
  ex.bc = C.bc;
  if (l == 0) kp_begin(KP_RESTRICT, st);
  if (two)
    launch_strip2<M_RESID, false, F_RESTRICT, 2 * CW + 1>(L, H.scale, (const float*)x, (const float*)rhs_l,
                                                          (float*)H.rhs[l + 1], 0.0, 0.0, nullptr, H.Bp, g, st, ex);
  else
    launch_strip<TV, M_RESID, false, F_RESTRICT, TV, 2 * CW + 1>(L, H.Bv, H.scale, x, rhs_l, (TV*)H.rhs[l + 1], 0.0, 0.0,
                                                                   nullptr, H.Bp, g, st, ex);
  if (l == 0) kp_end(KP_RESTRICT, st);
}

// samples per lane of the fused passes on level L: per-sample matrices always two; a batch-shared matrix what the batch
// allows (H.fuse), the four-sample form for 3-diagonal levels only
// The PRE pass of a 3-diagonal batch-shared level takes FOUR samples per lane where the batch has whole waves of 256:
// half the vector-memory instructions per byte at half the waves (219 VGPRs, 2 waves per SIMD).  Measured on the
// 1024^2 x 256 bench, same box (gpurun_out/r4k): PRE 0.707 -> 0.659 ms; the POST pass (240 VGPRs) 0.998 -> 1.042 ms:
// it keeps two.
inline int fused_spl(const Hier& H, const Level& L, bool pre) {
  const int spl = H.Bv == 1 ? H.fuse : 2;
  if (pre && H.pre4 && H.Bv == 1 && spl == 2 && H.Bp % (4 * kWave) == 0 && L.nd == 3) return 4;
  return spl;
}

// Can level l of the fp32 cycle run the fused POST pass (and with it the initial-guess form of the cycle)?  Fills the
// tile geometries of the fused PRE (gpre) and POST (gpost) passes; returns the fused_ok mask (0: no fused pass here).
template <typename TV>
int fused_level(const Hier& H, int l, StripGeom* gpre, StripGeom* gpost) {
  if (l >= H.nl - 1) return 0;
  const Level& L = H.lev[l];
  const Level& C = H.lev[l + 1];
  const int fmask = (sizeof(TV) == 4 && H.fuse && H.nu == 2) ? fused_ok(L, H.Bv, H.Bp, H.scale) : 0;
  if (!fmask || !(L.nx == 2 * C.nx && L.ny == 2 * C.ny && strip_geom(L, H.Bp).use)) return 0;
  const int spl = fused_spl(H, L, false), spl_pre = fused_spl(H, L, true);
  const int nw = 4;   // waves per block (fused_pre_kernel: wider blocks measured slower)
  constexpr int CW = kRestrictCols;
  // ~6144 blocks whatever the samples per lane: the four-sample form gets tiles of half the height (6 instead of 11 coarse
  // rows at 1024^2 x 256).  Measured (gpurun_out/r4l, same box): 6 rows 0.660 ms, 11 rows 0.681, 16 rows 0.778 -- the
  // number of independent marches matters more than the halo rows
  // Levels of <= 300 columns cannot fill the GPU with 4-coarse-row tiles: shorter tiles (2 coarse rows going down, ~5 fine
  // rows going up) double the independent marches; -1.4 ms per 1024^2 step, neutral on the 513^2 level (gpurun_out/r5j, r5k)
  const bool small = L.W <= 300;
  // tiles of coarse rows; no partial sums
  const StripGeom g = tile_geom(C.ny + 1, (C.W + nw * CW - 1) / (nw * CW), H.Bp / (spl_pre * kWave), kStripBlocks * 4 / nw,
                                small ? 2 : 4, 0);
  *gpre = g;
  *gpost = strip_geom(L, H.Bp, 4, spl, nw);
  if (small) {
    const int nyp = L.ny + 1;
    int tr = 4;
    while (gpost->ncb * ((nyp + tr - 1) / tr) > kPartBlocks) ++tr;
    gpost->TR = tr;
    gpost->nrc = (nyp + tr - 1) / tr;
  }
  const bool fits = strip2_tile_fits(L, H.Bp, 2 * g.TR + 6) && strip2_tile_fits(L, H.Bp, gpost->TR + 5);
  return fits ? fmask : 0;
}

// z = V(rhs0): returns the buffer holding the result at level 0.  If rz_part != NULL the last
// fine sweep also leaves the partials of rhs0.z there (*rz_blocks of them).
// guess != NULL (only where fused_level(H, l0) & 2): the cycle starts from the initial guess P guess instead of 0 and
// returns the new ITERATE for the right-hand side rhs0 -- in exact arithmetic P guess + V(rhs0 - A P guess), without the
// prolongation, residual and addition passes of that form (full-multigrid start).
// dest != NULL (l0 == 0 only): the last pass of level 0 writes z there where that pass is the fused POST pass or a plain
// sweep (the other forms return their own buffer: the caller tells by the pointer).
template <typename TV>
TV* vcycle(const Hier& H, const TV* rhs0, double* rz_part, int* rz_blocks, hipStream_t st, int l0 = 0,
           const TV* guess = nullptr, TV* dest = nullptr) {
  const TV* rhs[kMaxLevels];
  TV* cur[kMaxLevels];
  bool fused[kMaxLevels];
  StripGeom gpost[kMaxLevels];
  rhs[l0] = rhs0;  // the cycle runs on levels l0 .. last (l0 > 0: inside full multigrid)
  const int last = H.nl - 1;
  for (int l = l0; l <= last; ++l) {  // downward leg
    const Level& L = H.lev[l];
    if (l == last) {  // coarsest level: Chebyshev solve (also the whole cycle when there is one level)
      int nb = 0;
      cur[l] = coarse_solve<TV>(H, l, rhs[l], (l0 == last) ? rz_part : nullptr, &nb, st);
      if (l0 == last && rz_part && rz_blocks) *rz_blocks = nb;
      break;
    }
    const int sweeps = H.nu;
    TV* a = (TV*)H.xa[l];
    TV* b2 = (TV*)H.xb[l];
    fused[l] = false;
    StripGeom gpre;
    const int fmask = fused_level<TV>(H, l, &gpre, &gpost[l]);
    if (fmask) {
      const Level& C = H.lev[l + 1];
      const int spl = fused_spl(H, L, false);
      fused[l] = (fmask & 2) != 0;             // the way up: fused POST pass
      if (l == l0 && guess && fused[l]) {
        // two sweeps from the prolonged guess (the POST kernel with x = 0), then residual + restriction
        launch_fused_post(L, C, H.Bv, H.scale, (const float*)nullptr, (const float*)rhs[l], (const float*)guess, (float*)a,
                          H.omega[0], H.omega[1], nullptr, H.Bp, gpost[l], spl, st);
        resid_restrict<TV>(H, l, a, rhs[l], st);
        cur[l] = a;
        rhs[l + 1] = (const TV*)H.rhs[l + 1];
        continue;
      }
      if (fmask & 1) {
        // both sweeps + residual + restriction in ONE pass (fused_pre_kernel)
        if (l == 0) kp_begin(KP_FIRST2, st);
        launch_fused_pre(L, C, H.Bv, H.scale, (const float*)rhs[l], (float*)a, (float*)H.rhs[l + 1], H.omega[0],
                         H.omega[1], H.Bp, gpre, fused_spl(H, L, true), st);
        if (l == 0) kp_end(KP_FIRST2, st);
        cur[l] = a;
        rhs[l + 1] = (const TV*)H.rhs[l + 1];
        continue;
      }
    }
    int done;
    if (sweeps >= 2) {
      TV* resu;
      op_jacobi_first2<TV>(H, l, rhs[l], a, b2, H.omega[0], H.omega[1 % H.nu], nullptr, &resu, st);
      if (resu != a) { TV* t = a; a = b2; b2 = t; }
      done = 2;
    } else {
      op_jacobi<TV>(H, l, rhs[l], nullptr, a, H.omega[0], nullptr, st);
      done = 1;
    }
    for (int s = done; s < sweeps; ++s) {
      op_jacobi<TV>(H, l, rhs[l], a, b2, H.omega[s % H.nu], nullptr, st);
      TV* t = a; a = b2; b2 = t;
    }
    cur[l] = a;
    if (l < last) {
      const Level& C = H.lev[l + 1];
      if (strip_geom(L, H.Bp).use && L.nx == 2 * C.nx && L.ny == 2 * C.ny) {
        resid_restrict<TV>(H, l, a, rhs[l], st);
      } else {
        op_residual<TV>(H, l, rhs[l], a, (TV*)H.res[l], nullptr, st);
        launch_restrict<TV>(H, L, C, (const TV*)H.res[l], (TV*)H.rhs[l + 1], st);
      }
      rhs[l + 1] = (const TV*)H.rhs[l + 1];
    }
  }
  for (int l = last - 1; l >= l0; --l) {  // upward leg
    const Level& L = H.lev[l];
    const Level& C = H.lev[l + 1];
    TV* a = cur[l];
    TV* b2 = (a == (TV*)H.xa[l]) ? (TV*)H.xb[l] : (TV*)H.xa[l];
    if (fused[l]) {   // prolongation + correction + both post-sweeps (+ the partials of rhs . z) in ONE pass
      const bool dot = (l == l0) && rz_part;
      if (l == 0 && dest) b2 = dest;
      if (l == 0) kp_begin(KP_PROLONG, st);
      launch_fused_post(L, C, H.Bv, H.scale, (const float*)a, (const float*)rhs[l], (const float*)cur[l + 1], (float*)b2,
                        H.omega[1], H.omega[0], dot ? rz_part : nullptr, H.Bp, gpost[l], fused_spl(H, L, false), st);
      if (l == 0) kp_end(KP_PROLONG, st);
      if (dot && rz_blocks) *rz_blocks = gpost[l].ncb * gpost[l].nrc;
      cur[l] = b2;
      continue;
    }
    int s0 = 0;
    StripGeom g;
    const bool two = strip2_pick<TV>(L, H.Bv, H.Bp, strip_cols<TV>(), &g);
    if (g.use && L.nx == 2 * C.nx && L.ny == 2 * C.ny) {  // prolongate + correct + first post-sweep in one pass
      const bool lastsweep = (l == l0 && H.nu == 1);
      Extra ex{};
      ex.a0 = cur[l + 1]; ex.cW = C.W; ex.bc = L.bc;
      if (l == 0) kp_begin(KP_PROLONG, st);
      if (two)
        launch_strip2<M_JACOBI, false, F_PROLONG, 4>(L, H.scale, (const float*)a, (const float*)rhs[l], (float*)b2,
                                                     H.omega[H.nu - 1], 0.0, lastsweep ? rz_part : nullptr, H.Bp, g, st, ex);
      else
        launch_strip<TV, M_JACOBI, false, F_PROLONG, TV, strip_cols<TV>()>(L, H.Bv, H.scale, (const TV*)a, rhs[l], b2,
                                                                            H.omega[H.nu - 1], 0.0,
                                                                            lastsweep ? rz_part : nullptr, H.Bp, g, st, ex);
      if (l == 0) kp_end(KP_PROLONG, st);
      if (lastsweep && rz_blocks) *rz_blocks = g.ncb * g.nrc;
      TV* t = a; a = b2; b2 = t;
      s0 = 1;
    } else {
      launch_prolong<TV>(H, L, C, (const TV*)cur[l + 1], a, 0, st);
    }
    for (int s = s0; s < H.nu; ++s) {
      const bool lastsweep = (l == l0 && s == H.nu - 1);
      if (lastsweep && l == 0 && dest && s > 0) b2 = dest;   // s > 0: a sweep before it has filled `a` (never dest itself)
      const int nb = op_jacobi<TV>(H, l, rhs[l], a, b2, H.omega[H.nu - 1 - s], lastsweep ? rz_part : nullptr, st);
      if (lastsweep && rz_blocks) *rz_blocks = nb;
      TV* t = a; a = b2; b2 = t;
    }
    cur[l] = a;
  }
  return cur[l0];
}

// The fine level of the full-multigrid start takes prolongation and residual as ONE strip pass (M_RESID, F_PROLONG without
// x, lattice.h) where the vectors are fp32, the matrix is batch-shared, the level runs the strip kernels and its
// coarsening halves both directions; DIFFHE_PCG_SPLIT_START keeps the two passes.
template <typename TV>
bool prolong_resid_ok(const Hier& H, int l) {
  if (l != 0 || H.split_start || sizeof(TV) != 4 || H.Bv != 1 || H.lev[0].shift) return false;
  const Level& L = H.lev[0];
  const Level& C = H.lev[1];
  return L.nx == 2 * C.nx && L.ny == 2 * C.ny && strip_geom(L, H.Bp).use;
}

// Full multigrid start: solve on the coarsest level, then per level interpolate, take the residual
// and apply one V-cycle.  Gives the CG an iterate whose error is already smooth (about 3-4 CG
// iterations ahead of a zero guess) for ~0.8 of an iteration.  b0 = right-hand side in TV storage.
// *pending (optional): the fine level's last correction is NOT added to the returned iterate but handed back -- the
// caller's conversion pass (pcg_setx_kernel) adds the two in fp64, one pass over x less.
// have_b1: the level-1 right-hand side is in H.bF[1] already (cycle_cvt_restrict).
template <typename TV>
TV* fmg_start(const Hier& H, const TV* b0, hipStream_t st, const TV** pending = nullptr, bool have_b1 = false) {
  const int last = H.nl - 1;
  const TV* bl[kMaxLevels];
  bl[0] = b0;
  for (int l = 0; l < last; ++l) {
    if (l > 0 || !have_b1) launch_restrict<TV>(H, H.lev[l], H.lev[l + 1], bl[l], (TV*)H.bF[l + 1], st);
    bl[l + 1] = (const TV*)H.bF[l + 1];
  }
  {  // coarsest level: the V-cycle from `last` is n_coarse Jacobi sweeps
    TV* e = vcycle<TV>(H, bl[last], nullptr, nullptr, st, last);
    if (diffhe::check(hipMemcpyAsync(H.xF[last], e, (size_t)H.lev[last].n * H.Bp * sizeof(TV), hipMemcpyDeviceToDevice, st)))
      return nullptr;  // error text recorded for diffhe_last_hip_error()
  }
  const TV* coarse = (const TV*)H.xF[last];      // the iterate of level l + 1
  if (pending) *pending = nullptr;
  // The initial-guess form of the cycle runs below the fine level only.  On the fine level it stores the full ITERATE in
  // fp32 between its passes where the correction form stores a correction ~1e-3 of it: rounding noise of 6e-8 |u|, rough,
  // ~3e-5 of the solution's energy -- measured one PCG iteration more (6 + 6 against 5 + 5 at 1024^2; gpurun_out/r4m)
  for (int l = last - 1; l >= 0; --l) {
    const Level& L = H.lev[l];
    const int cycles = (l == 0) ? 1 : H.fmg_coarse_cycles;  // extra cycles on the cheap coarse levels
    StripGeom g1, g2;
    TV* x = (TV*)H.xF[l];
    int c0 = 0;
    bool have_resid = false;   // H.rhs[l] already holds the residual of x (the fused pass of the fine level)
    if (l > 0 && (fused_level<TV>(H, l, &g1, &g2) & 2)) {
      // levels with the fused passes: ONE cycle from the prolonged guess -- no prolongation, residual or addition pass
      TV* it = vcycle<TV>(H, bl[l], nullptr, nullptr, st, l, coarse);
      if (cycles == 1) {
        coarse = it;          // consumed by the first launch of the next level, before that level's cycle reuses the buffer
        continue;
      }
      if (diffhe::check(hipMemcpyAsync(x, it, (size_t)L.n * H.Bp * sizeof(TV), hipMemcpyDeviceToDevice, st))) return nullptr;
      c0 = 1;
    } else if (prolong_resid_ok<TV>(H, l)) {
      // x = P coarse and rhs - A x in ONE strip pass: the window is the prolonged iterate as the transfer kernel would
      // have stored it, so x and the residual are bit for bit those of the two passes below
      Extra ex{};
      ex.a0 = coarse; ex.cW = H.lev[l + 1].W; ex.bc = L.bc; ex.p_out = x;
      launch_strip<TV, M_RESID, false, F_PROLONG, TV, kStripCols, 5, MAT_SHARED>(
          L, H.Bv, H.scale, (const TV*)nullptr, bl[l], (TV*)H.rhs[l], 0.0, 0.0, nullptr, H.Bp, strip_geom(L, H.Bp), st, ex);
      have_resid = true;
    } else {
      launch_prolong<TV>(H, L, H.lev[l + 1], coarse, x, 1, st);
    }
    for (int c = c0; c < cycles; ++c) {
      if (!have_resid) op_residual<TV>(H, l, bl[l], (const TV*)x, (TV*)H.rhs[l], nullptr, st);
      have_resid = false;
      TV* e = vcycle<TV>(H, (const TV*)H.rhs[l], nullptr, nullptr, st, l);
      if (l == 0 && c == cycles - 1 && pending) {
        *pending = e;
        break;
      }
      launch_nodes(H, st, 3 * sizeof(TV), mg_add_kernel<TV>, L.n, (const TV*)e, x, L.n, H.Bp);
    }
    coarse = x;
  }
  return (TV*)coarse;
}

}  // namespace

// ---- host-side hierarchy --------------------------------------------------------------------
int fill_hier(Hier& H, const diffhe_mg_level* levels, int n_levels, int Bv, int Bp, const double* scale, const double* omegas,
              int nu, int n_coarse) {
  if (!levels || n_levels < 1 || n_levels > kMaxLevels) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  if (Bv != 1 && Bv != Bp) return DIFFHE_E_BADARG;
  if (nu < 1 || nu > 8 || n_coarse < 1 || !omegas) return DIFFHE_E_BADARG;
  for (int l = 0; l < n_levels; ++l) {
    const diffhe_mg_level& s = levels[l];
    if (s.nx < 2 || s.ny < 2 || (s.nd != 3 && s.nd != 4) || !s.vals || !s.is_bc) return DIFFHE_E_BADARG;
    if (l > 0) {  // each level halves the previous one in x, in y, or in both
      const bool hx = levels[l - 1].nx == 2 * s.nx, hy = levels[l - 1].ny == 2 * s.ny;
      const bool kx = levels[l - 1].nx == s.nx, ky = levels[l - 1].ny == s.ny;
      if (!((hx && hy) || (hx && ky) || (kx && hy))) return DIFFHE_E_BADARG;
    }
    if ((long long)(s.nx + 1) * (s.ny + 1) > 0x7fffffffLL) return DIFFHE_E_TOOBIG;
    Level& L = H.lev[l];
    L.nx = s.nx; L.ny = s.ny; L.W = s.nx + 1; L.n = (s.nx + 1) * (s.ny + 1); L.nd = s.nd;
    L.v = s.vals; L.v32 = s.vals32; L.bc = s.is_bc; L.inv = s.dense_inv; L.shift = s.shift; L.rd32 = s.rdiag32; L.mk32 = s.mask32; L.o16 = (Bv == Bp && Bp > 1 && s.offdiag_scales) ? (const _Float16*)s.offdiag16 : nullptr;
    L.osc = s.offdiag_scales;
  }
  H.nl = n_levels; H.Bv = Bv; H.Bp = Bp; H.scale = scale; H.nu = nu; H.n_coarse = n_coarse;
  H.coarse_lmax = 2.0;
  H.fmg_coarse_cycles = 1;
  H.fuse = Bp % (2 * kWave) == 0 ? 2 : 1;   // one sample per lane where the batch is no multiple of 128
  H.pre4 = 1;
  H.dense_mfma = 1;
  H.split_start = 0;
  for (int k = 0; k < 8; ++k) H.omega[k] = omegas[k < nu ? k : nu - 1];
  return DIFFHE_OK;
}

int single_level(Hier& H, const diffhe_mg_level* level, int Bv, int Bp, const double* scale) {
  const double w1 = 0.8;
  return fill_hier(H, level, 1, Bv, Bp, scale, &w1, 1, 1);
}

i64 carve_cycle(Hier& H, double* work, bool fp32) {
  int n_nodes[kMaxLevels];
  for (int l = 0; l < H.nl; ++l) n_nodes[l] = H.lev[l].n;
  return cycle_carve(H, work, n_nodes, H.nl, H.Bp, fp32);
}

// ---- what the driver calls: the storage type is resolved here, once ---------------------------------------------------
const void* cycle_precondition(const Hier& H, bool fp32, const void* r, double* part, int* nblocks, hipStream_t st, void* dest) {
  if (fp32) return vcycle<float>(H, (const float*)r, part, nblocks, st, 0, nullptr, (float*)dest);
  return vcycle<double>(H, (const double*)r, part, nblocks, st);
}

void cycle_cvt_restrict(const Hier& H, const double* b, const double* rs, float* r32, hipStream_t st) {
  const Level& F = H.lev[0];
  const Level& C = H.lev[1];
  // tiles of coarse rows, as the fused residual + restriction (resid_restrict)
  const StripGeom g = tile_geom(C.ny + 1, (C.W + 4 * 2 - 1) / (4 * 2), H.Bp / kWave, kStripBlocks, 4, 0);
  diffhe::account((12.0 * F.n + 4.0 * C.n) * H.Bp);   // b read, r32 and the coarse vector written
  hipLaunchKernelGGL(cvt_restrict_kernel, dim3(g.ncb * g.nrc, H.Bp / kWave), dim3(256), 0, st, F, C, b, rs, r32,
                     (float*)H.bF[1], H.Bp, g.ncb, g.TR);
}

const void* cycle_fmg_start(const Hier& H, bool fp32, const void* b0, hipStream_t st, const void** pending, bool have_b1) {
  if (fp32) {
    const float* e0 = nullptr;
    const float* x0 = fmg_start<float>(H, (const float*)b0, st, &e0, have_b1);
    *pending = e0;
    return x0;
  }
  const double* e0 = nullptr;
  const double* x0 = fmg_start<double>(H, (const double*)b0, st, &e0);
  *pending = e0;
  return x0;
}

int cycle_residual(const Hier& H, const double* rhs, const double* x, double* res, double* part, hipStream_t st, int dot_bx,
                   double* part2) {
  return op_residual<double>(H, 0, rhs, x, res, part, st, dot_bx, part2);
}

int cycle_apply_dot(const Hier& H, const double* x, double* y, double* part, hipStream_t st) {
  return op_apply_dot(H, x, y, part, st);
}

// DIRECT solve: the whole system is small enough for the dense inverse of its (batch-shared) matrix -- the
// reference's own regime (2D meshes up to 32 x 32).  x = (1 / s_b) K_1^{-1} b in one launch.
bool direct_ok(const Hier& H, bool fp32) {
  const Level& L0 = H.lev[0];
  return H.nl == 1 && L0.inv && H.Bv == 1 && !fp32 && L0.n <= kPartBlocks;
}

void cycle_direct_solve(const Hier& H, const double* b, double* x, hipStream_t st) {
  const Level& L0 = H.lev[0];
  const int n = L0.n, Bp = H.Bp;
  diffhe::account(16.0 * (double)n * Bp);
  if (Bp >= kWave)
    hipLaunchKernelGGL((mg_dense_solve_kernel<double, 4>), dim3((n + 3) / 4, Bp / kWave), dim3(256), 0, st, n,
                       (const double*)L0.inv, H.scale, b, x, (double*)nullptr, Bp);
  else
    hipLaunchKernelGGL(mg_dense_small_kernel<double>, dim3(n), dim3(64), 0, st, n, (const double*)L0.inv, H.scale, b, x,
                       (double*)nullptr, Bp);
}

int cycle_maxdiag(const Hier& H, double* out, hipStream_t st) {
  const Level& L0 = H.lev[0];
  const int rc = diffhe::check(hipMemsetAsync((void*)out, 0, sizeof(double) * H.Bv, st));
  if (rc) return rc;
  hipLaunchKernelGGL(dia_maxdiag_kernel, node_grid(L0.n, H.Bv, 512), dim3(256), 0, st, L0, H.Bv, (unsigned long long*)out);
  return DIFFHE_OK;
}

int cycle_coarse_bound(Hier& H, unsigned long long* gb, hipStream_t st) {
  const Level& Lc = H.lev[H.nl - 1];
  if (Lc.nd != 4) return DIFFHE_OK;
  int rc = diffhe::check(hipMemsetAsync(gb, 0, sizeof(unsigned long long), st));
  if (rc) return rc;
  hipLaunchKernelGGL(dia_gershgorin_kernel, node_grid(Lc.n, H.Bv, 256), dim3(256), 0, st, Lc, H.Bv, gb);
  double bound = 0.0;
  rc = diffhe::check(hipMemcpyAsync(&bound, gb, sizeof(double), hipMemcpyDeviceToHost, st));
  if (!rc) rc = diffhe::check(hipStreamSynchronize(st));
  if (rc) return rc;
  if (bound > 2.0 && bound < 1e3) H.coarse_lmax = bound * (1.0 + 1e-9);
  return DIFFHE_OK;
}

}  // namespace diffhe_lattice

using namespace diffhe_lattice;

// =========================================================================================
// C ABI: the single-level entries of this unit's kernels
// =========================================================================================
extern "C" int diffhe_lattice_apply(const diffhe_mg_level* level, int Bv, const double* scale, const double* x,
                                    double* y, double* part, int Bp, void* stream) {
  if (!x || !y || !part) return DIFFHE_E_BADARG;
  Hier H;
  int rc = single_level(H, level, Bv, Bp, scale);
  if (rc) return rc;
  cycle_apply_dot(H, x, y, part, (hipStream_t)stream);
  return diffhe::check_launch();
}

extern "C" int diffhe_lattice_smooth(const diffhe_mg_level* level, int Bv, const double* scale, const double* rhs,
                                     const double* xin, double* xout, double omega, int Bp, void* stream) {
  if (!rhs || !xout) return DIFFHE_E_BADARG;
  Hier H;
  int rc = single_level(H, level, Bv, Bp, scale);
  if (rc) return rc;
  op_jacobi<double>(H, 0, rhs, xin, xout, omega, nullptr, (hipStream_t)stream);
  return diffhe::check_launch();
}
