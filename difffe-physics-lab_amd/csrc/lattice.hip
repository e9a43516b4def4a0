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

// ---- CG vector kernels ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void pcg_init_kernel(const double* __restrict__ bvec, double* __restrict__ x,
                                                        double* __restrict__ r, double* __restrict__ part, int n,
                                                        int Bp) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  double s = 0.0;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    const double bi = bvec[o];
    if (x) {  // x == NULL (full-multigrid start): x and r are set after the start, only b.b is due here
      x[o] = 0.0;
      r[o] = bi;
    }
    s += bi * bi;
  }
  STORE_PARTIAL(part, s);
}

__global__ __launch_bounds__(256) void pcg_update_kernel(const double* __restrict__ p, const double* __restrict__ Ap,
                                                          const double* __restrict__ alpha, double* __restrict__ x,
                                                          double* __restrict__ r, float* __restrict__ r32,
                                                          const double* __restrict__ rs, double* __restrict__ part,
                                                          int n, int Bp) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const double a = alpha[nm.b];
  const double sc = (r32 && rs) ? rs[nm.b] : 1.0;
  double s = 0.0;
  int i = nm.node0;
  // four nodes per trip (the loads of all four in flight together; one node per trip left a wave with two loads
  // outstanding: 4.8 TB/s); same nodes, same order of the partial sum
  if (!x)
    for (; (i64)i + 3LL * nm.stride < n; i += 4 * nm.stride) {
      double rv[4], av[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const i64 o = (i64)(i + u * nm.stride) * Bp + nm.b;
        rv[u] = __builtin_nontemporal_load(r + o);
        av[u] = __builtin_nontemporal_load(Ap + o);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const i64 o = (i64)(i + u * nm.stride) * Bp + nm.b;
        const double ri = rv[u] - a * av[u];
        __builtin_nontemporal_store(ri, r + o);
        if (r32) r32[o] = (float)(ri * sc);
        s += ri * ri;
      }
    }
  for (; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    if (x) x[o] += a * p[o];  // x == NULL: the iterate update is fused into the next operator apply
    const double ri = __builtin_nontemporal_load(r + o) - a * __builtin_nontemporal_load(Ap + o);
    __builtin_nontemporal_store(ri, r + o);
    if (r32) r32[o] = (float)(ri * sc);  // read again right away by the V-cycle: left cacheable
    s += ri * ri;
  }
  STORE_PARTIAL(part, s);
}

// (Two samples per lane -- 16-byte loads and stores, a wave moving 1 KB per instruction -- were measured for this kernel
// and for pcg_finish_kernel: 212.9 / 213.8 -> 214.6 / 214.2 ms per step of the per-element-field variant, headline step
// unchanged, gpurun_out/r4an.  At 4.9 TB/s these passes run at the rate of the box's own device-to-device copy.)
// y += x (TV) ; and the start of the CG from a full-multigrid iterate: x64 = (double) x0
template <typename TV>
__global__ __launch_bounds__(256) void mg_add_kernel(const TV* __restrict__ x, TV* __restrict__ y, int n, int Bp) {
  const NodeMap nm = node_map(Bp);
  for (int i = nm.node0; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    y[o] = (TV)((double)y[o] + (double)x[o]);
  }
}

template <typename TV>
__global__ __launch_bounds__(256) void pcg_setx_kernel(const TV* __restrict__ x0, const double* __restrict__ rs,
                                                        double* __restrict__ x, double* __restrict__ part, int n,
                                                        int Bp, int add = 0, const TV* __restrict__ e0 = nullptr) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const double inv = rs ? 1.0 / rs[nm.b] : 1.0;  // the start was computed from the scaled right-hand side
  double s = 0.0;
  int i = nm.node0;
  if (!add)   // four nodes per trip (see pcg_update_kernel)
    for (; (i64)i + 3LL * nm.stride < n; i += 4 * nm.stride) {
      TV xv[4], ev[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const i64 o = (i64)(i + u * nm.stride) * Bp + nm.b;
        xv[u] = x0[o];
        ev[u] = e0 ? e0[o] : (TV)0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const i64 o = (i64)(i + u * nm.stride) * Bp + nm.b;
        const double v = ((double)xv[u] + (e0 ? (double)ev[u] : 0.0)) * inv + 0.0;
        x[o] = v;
        s += v * v;
      }
    }
  for (; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    // add: x0 is a correction of the caller's iterate;  e0: the last cycle's correction of x0, not yet added (fmg_start)
    const double v = ((double)x0[o] + (e0 ? (double)e0[o] : 0.0)) * inv + (add ? x[o] : 0.0);
    x[o] = v;
    s += v * v;
  }
  if (part) STORE_PARTIAL(part, s);  // |x0|^2: scale of the attainable residual (S_FLOOR)
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

// r32 = fp32(rs * r): the fp32 copies that feed the preconditioner are taken of the residual scaled by a per-sample
// power of two rs ~ 1 / |b| (S_INIT), so they stay inside the fp32 range whatever the magnitude of the data
// (forcing of amplitude 1e-35 used to underflow them); powers of two make the scaling exact, so nothing else changes.
// rlo (optional): the low parts of the pair as well, r32 + rlo = rs * r to 2^-48 (F_RPAIR; a zero start without the
// full-multigrid iterate, where no residual pass opens the loop).
__global__ __launch_bounds__(256) void pcg_cvt_kernel(const double* __restrict__ r, const double* __restrict__ rs,
                                                       float* __restrict__ r32, int n, int Bp,
                                                       float* __restrict__ rlo = nullptr) {
  const NodeMap nm = node_map(Bp);
  const double sc = rs ? rs[nm.b] : 1.0;
  int i = nm.node0;
  if (rlo) {
    for (; i < n; i += nm.stride) {
      const i64 o = (i64)i * Bp + nm.b;
      float hi, lo;
      split(r[o] * sc, hi, lo);
      r32[o] = hi;
      rlo[o] = lo;
    }
    return;
  }
  for (; (i64)i + 3LL * nm.stride < n; i += 4 * nm.stride) {   // four nodes per trip: four loads in flight per wave
    double rv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) rv[u] = r[(i64)(i + u * nm.stride) * Bp + nm.b];
#pragma unroll
    for (int u = 0; u < 4; ++u) r32[(i64)(i + u * nm.stride) * Bp + nm.b] = (float)(rv[u] * sc);
  }
  for (; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    r32[o] = (float)(r[o] * sc);
  }
}

// x += alpha p  (flush of the pending iterate update of the fused CG loop)
template <typename TP>
__global__ __launch_bounds__(256) void pcg_axpy_kernel(const double* __restrict__ alpha, const TP* __restrict__ p,
                                                        double* __restrict__ x, int n, int Bp) {
  const NodeMap nm = node_map(Bp);
  const double a = alpha[nm.b];
  for (int i = nm.node0; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    x[o] += a * (double)p[o];
  }
}

// Directions kept before the iterate is touched: 10 fp32 slots (5 fp64) -- solves of up to 10 iterations (the 9 + 9 of a
// per-element field per sample) form x ONCE, in pcg_finish_kernel; round 3's 6 slots flushed such a solve twice
constexpr int kRingSlots = 10;

// End of the solve: x += alpha p (the pending iterate update of the fused loop; p == NULL: none) + z / rs, where
// z = V(r) is the preconditioned residual of the FINAL iterate -- every iteration ends with that V-cycle (its r.z is
// the error estimate the stop is decided on), and samples that stopped earlier kept r, hence z, unchanged since.
// Adding it is one step of the stationary multigrid iteration: e <- (I - M^-1 A) e, a further reduction by the
// V-cycle's own convergence factor (< 0.3) for no extra pass.
template <typename TP>
__global__ __launch_bounds__(256) void pcg_finish_kernel(const double* __restrict__ alpha, const TP* __restrict__ p,
                                                          long long slot_stride, int j0, int count, int n_slots,
                                                          const TP* __restrict__ z, const double* __restrict__ rs,
                                                          double* __restrict__ x, int n, int Bp) {
  // x += sum_{j = j0 .. j0 + count - 1} alpha_j p_j (+ z / rs): direction j lives in slot j % n_slots of `p`, its
  // step lengths in row j % n_slots of `alpha` (0 for samples that had stopped)
  const NodeMap nm = node_map(Bp);
  const double zi = z ? (rs ? 1.0 / rs[nm.b] : 1.0) : 0.0;   // rs is a power of two: exact
  double a[kRingSlots];
#pragma unroll
  for (int k = 0; k < kRingSlots; ++k) a[k] = k < count ? alpha[(long long)((j0 + k) % n_slots) * Bp + nm.b] : 0.0;
  int i = nm.node0;
  // two nodes per trip: twice the loads in flight per wave (same operations per node)
  for (; (i64)i + nm.stride < n; i += 2 * nm.stride) {
    const i64 o0 = (i64)i * Bp + nm.b, o1 = (i64)(i + nm.stride) * Bp + nm.b;
    double v0 = x[o0], v1 = x[o1];
    TP z0 = z ? z[o0] : (TP)0, z1 = z ? z[o1] : (TP)0;
    TP p0[kRingSlots], p1[kRingSlots];
#pragma unroll
    for (int k = 0; k < kRingSlots; ++k)
      if (k < count) {
        const long long so = (long long)((j0 + k) % n_slots) * slot_stride;
        p0[k] = p[so + o0];
        p1[k] = p[so + o1];
      }
    if (z) { v0 += zi * (double)z0; v1 += zi * (double)z1; }
#pragma unroll
    for (int k = 0; k < kRingSlots; ++k)
      if (k < count) { v0 += a[k] * (double)p0[k]; v1 += a[k] * (double)p1[k]; }
    x[o0] = v0;
    x[o1] = v1;
  }
  for (; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    double v = x[o];
    if (z) v += zi * (double)z[o];
#pragma unroll
    for (int k = 0; k < kRingSlots; ++k)
      if (k < count) v += a[k] * (double)p[(long long)((j0 + k) % n_slots) * slot_stride + o];
    x[o] = v;
  }
}

// p = z + beta p   (first: p = z)
template <typename TV>
__global__ __launch_bounds__(256) void pcg_update_p_kernel(const TV* __restrict__ z, const double* __restrict__ beta,
                                                            double* __restrict__ p, int first, int n, int Bp) {
  const NodeMap nm = node_map(Bp);
  const double be = first ? 0.0 : beta[nm.b];
  for (int i = nm.node0; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    p[o] = first ? (double)z[o] : (double)z[o] + be * p[o];
  }
}

// ---- per-sample scalars -----------------------------------------------------------------------
struct PcgScalars {
  double *rz, *alpha, *beta, *bb, *tol2;
  double* rs;             // per-sample power of two ~ 1 / |b| applied to the fp32 copies of the residual (NULL: none)
  const double* maxdiag;  // S_FLOOR: per-sample (Bv entries) max diagonal of the unscaled level-0 matrix
  const double* scale;    // S_FLOOR: per-sample operator scale (may be NULL)
  int Bv;
  int *active, *iters, *n_active;
  // Energy-norm stop.  With a multigrid preconditioner M ~ A the dot r.z = r^T M^-1 r the CG computes anyway is the
  // squared ENERGY norm of the error e^T A e (to the spectral equivalence of M and A, ~20 %), and b.x that of the
  // solution: sample b stops once r.z <= tol_e2 * energy[b].
  double* energy;         // u^T A u >= (b.x0)^2 / (x0^T A x0) (Cauchy-Schwarz in the A inner product: a LOWER bound for
                          // any x0, tight for the full-multigrid start), or r0.z0 = b^T M^-1 b from a zero start
  double* rr;             // last r.r per sample (guard of the energy stop)
  double* est;            // out: last estimate sqrt(r.z / energy) per sample
  double tol_e2;          // 0: residual criterion only
  int e_max_it;           // the energy rule is trusted within this many iterations (10 at tol_energy 1e-11, one more per decade)
  int have_energy;        // energy[] was set from the full-multigrid start (S_ENERGY)
  int* rule;              // out: which rule ended each sample: 0 none (iteration cap), 1 residual, 2 energy-norm estimate
  // The residual pair's low half is dropped near the end of an energy-rule solve (F_RDROP / F_RSINGLE, lattice.h).
  // S_BETA counts in n_active[1] the samples still active that are NOT yet within 2^16 of the level the energy rule stops
  // them at (est_b^2 <= 2^32 tol_e2), or for which that rule is not in force: the host drops once n_active[1] == 0.
  // Each dropped update rounds an entry of r by <= 2^-25 relative and r shrinks >= 10x per iteration, so what
  // accumulates is <= 2^-24 |r| of the transition, 2^-8 of the exit level: inside the estimate's own accuracy.
  double* gap;            // per sample g_b = 2^-24 sqrt(r_b.r_b) of the transition update: bound of that accumulated rounding
  int lo_state;           // S_CONV: 0 the pair is whole; 1 this update was the transition (sets gap); 2 after it.  From
                          // the transition on the residual rule tests (sqrt(rr_b) + g_b)^2: the rounding can delay a
                          // residual-rule stop, never fake one
};
enum { S_INIT = 0, S_RZ0 = 1, S_ALPHA = 2, S_CONV = 3, S_BETA = 4, S_RELRES = 5, S_SUM = 6, S_FLOOR = 7, S_ENERGY = 8,
       S_ENERGY2 = 9 };

// First stage of a long partial list: block (x, y) sums the rows k = y, y + S, y + 2 S, ... of `part` for the samples of
// chunk x into row y of `slice` (S = gridDim.y rows).  One block of pcg_scalar_kernel summing 1500-2000 rows reads ~1 MB
// through ONE CU (23 us per phase at 1024^2 x 256, 43 phases per step); 16 blocks + the final phase over 16 rows take ~8.
// Fixed assignment and fixed order of additions: bitwise reproducible.
constexpr int kScalarSlices = 16;
__global__ __launch_bounds__(256) void pcg_slice_kernel(const double* __restrict__ part, int nblk, int Bp,
                                                         double* __restrict__ slice) {
  __shared__ double lds[4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kWave + lane;
  const int S = gridDim.y, y = blockIdx.y;
  double s0 = 0.0, s1 = 0.0;
  if (b < Bp) {
    int k = y + S * wave;
    for (; k + 4 * S < nblk; k += 8 * S) {     // two independent chains per wave, four waves: eight loads in flight
      s0 += part[(i64)k * Bp + b];
      s1 += part[(i64)(k + 4 * S) * Bp + b];
    }
    if (k < nblk) s0 += part[(i64)k * Bp + b];
  }
  lds[wave * kWave + lane] = s0 + s1;
  __syncthreads();
  if (wave == 0 && b < Bp)
    slice[(i64)y * Bp + b] = (lds[lane] + lds[kWave + lane]) + (lds[2 * kWave + lane] + lds[3 * kWave + lane]);
}

// 1024 threads: lanes over samples, 16 waves over slices of the partial list (fixed order)
__global__ __launch_bounds__(1024) void pcg_scalar_kernel(int phase, const double* __restrict__ part, int nblk, int Bp,
                                                           double tol, PcgScalars S, double* __restrict__ relres) {
  __shared__ double lds[16 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kWave + lane;
  double s = 0.0;
  if (b < Bp) {  // 4 independent chains keep several loads in flight (fixed order: still deterministic)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int k = wave;
    for (; k + 48 < nblk; k += 64) {
      s0 += part[(i64)k * Bp + b];
      s1 += part[(i64)(k + 16) * Bp + b];
      s2 += part[(i64)(k + 32) * Bp + b];
      s3 += part[(i64)(k + 48) * Bp + b];
    }
    for (; k < nblk; k += 16) s0 += part[(i64)k * Bp + b];
    s = (s0 + s1) + (s2 + s3);
  }
  lds[wave * kWave + lane] = s;
  __syncthreads();
  if (wave != 0 || b >= Bp) return;
  double a = 0.0;
#pragma unroll
  for (int w = 0; w < 16; ++w) a += lds[w * kWave + lane];
  switch (phase) {
    case S_INIT:  // a = b.b
      S.bb[b] = a;
      if (S.rs) S.rs[b] = a > 0.0 ? ldexp(1.0, -ilogb(sqrt(a))) : 1.0;  // rs |b| in [1, 2)
      S.tol2[b] = tol * tol * a;
      S.active[b] = a > 0.0 ? 1 : 0;
      S.rule[b] = a > 0.0 ? 0 : 1;   // a zero right-hand side is solved by x = 0
      S.iters[b] = 0;
      S.alpha[b] = 0.0;
      S.beta[b] = 0.0;
      S.rz[b] = 0.0;
      S.rr[b] = a;
      break;
    case S_RZ0: {  // a = r.z
      S.rz[b] = a;
      const double rs2 = S.rs ? S.rs[b] * S.rs[b] : 1.0;   // z carries rs, so does the copy of r it is dotted with
      if (!S.have_energy) S.energy[b] = a / rs2;           // zero start: r0.z0 = b^T M^-1 b ~ u^T A u
      S.est[b] = S.energy[b] > 0.0 ? sqrt(a / rs2 / S.energy[b]) : 0.0;
      break;
    }
    case S_ENERGY:  // a = b.x0
      S.energy[b] = a;
      break;
    case S_ENERGY2:  // a = x0^T A x0: energy of the solution >= (b.x0)^2 / (x0^T A x0), whatever x0 is
      S.energy[b] = (a > 0.0 && S.energy[b] > 0.0) ? S.energy[b] * (S.energy[b] / a) : 0.0;  // no squares: any data magnitude
      break;
    case S_ALPHA:  // a = p.Ap
      // with scaled fp32 copies z, p and Ap carry the factor rs and both dots rs^2: alpha is unchanged, and the
      // updates x += alpha p, r -= alpha Ap take alpha / rs
      S.alpha[b] = (S.active[b] && a > 0.0) ? (S.rz[b] / a) / (S.rs ? S.rs[b] : 1.0) : 0.0;
      if (b == 0) S.n_active[0] = S.n_active[1] = 0;
      break;
    case S_CONV:  // a = r.r after the update
      if (S.lo_state == 1) S.gap[b] = 5.9604644775390625e-08 * sqrt(a);   // 2^-24 |r_b|
      if (S.active[b]) {
        S.iters[b] += 1;
        S.rr[b] = a;
        double seen = a;   // what the residual rule is shown
        if (S.lo_state) {
          const double up = sqrt(a) + S.gap[b];
          seen = up * up;
        }
        if (seen <= S.tol2[b]) {
          S.active[b] = 0;
          S.rule[b] = 1;
        }
      }
      break;
    case S_BETA: {  // a = r.z (new)
      bool far = false;   // still active and too far from the energy rule's stop to drop the residual's low half
      if (S.active[b]) {
        S.beta[b] = a / S.rz[b];
        S.rz[b] = a;
        const double rs2 = S.rs ? S.rs[b] * S.rs[b] : 1.0;
        const double e2 = a / rs2;                                   // ~ e^T A e of the current iterate
        S.est[b] = S.energy[b] > 0.0 ? sqrt(fmax(e2, 0.0) / S.energy[b]) : 0.0;
        // The estimate stands on M ~ A.  It is trusted only where the iteration is visibly healthy: a positive r.z
        // (a V-cycle that lost definiteness -- obtuse meshes, fp32 overflow -- can return anything), a positive
        // energy bound, and a residual already within 1e4 x the target (|r|/|b| is 6e-9 .. 2e-10 at the iterations
        // where the bench workload stops); otherwise the residual criterion decides alone.
        // ... and only within the first 10 iterations (at tol_energy = 1e-11; one more per decade asked beyond that --
        // a healthy cycle gains a decade per iteration): r.z equals e^T A e up to lambda_min(M^-1 A), and a CG that needs
        // more than that to get here is telling that this constant is small (skewed lattices with pinned interior
        // nodes: 12 and 35 iterations, error 8e-11 at an estimate of 1e-11).
        if (S.tol_e2 > 0.0 && a > 0.0 && S.energy[b] > 0.0 && e2 <= S.tol_e2 * S.energy[b] &&
            S.rr[b] <= 1e8 * S.tol_e2 * S.bb[b] && S.iters[b] <= S.e_max_it) {
          S.active[b] = 0;
          S.rule[b] = 2;
        }
        far = S.active[b] && !(S.tol_e2 > 0.0 && a > 0.0 && S.energy[b] > 0.0 && S.iters[b] < S.e_max_it &&
                               e2 <= 4294967296.0 * S.tol_e2 * S.energy[b]);   // est_b <= 2^16 x the stop level
      } else {
        S.beta[b] = 0.0;
      }
      if (S.active[b]) atomicAdd(S.n_active, 1);                      // both read by the host after this phase
      if (far) atomicAdd(S.n_active + 1, 1);
      break;
    }
    case S_SUM:  // plain per-sample total
      relres[b] = a;
      break;
    case S_FLOOR: {  // a = |x0|^2.  fp64 cannot bring |b - A x| below ~ u |A| |x| (u = 2^-53): the recurrence
      // residual keeps falling past that level but the iterate no longer improves, so the stop is floored at
      // HALF of it -- the backward-stability level a direct fp64 solve (the reference's LU) reaches too.
      const double anorm = 2.0 * S.maxdiag[S.Bv == 1 ? 0 : b] * (S.scale ? S.scale[b] : 1.0);  // >= |A|_inf
      const double fl = 0.5 * 1.1102230246251565e-16 * anorm;
      const double floor2 = fl * fl * a;
      if (floor2 > S.tol2[b]) S.tol2[b] = floor2;
      break;
    }
    default:  // S_RELRES: a = |b - A x|^2
      relres[b] = S.bb[b] > 0.0 ? sqrt(a / S.bb[b]) : 0.0;
  }
}

// ---- opt-in timing of the step's main kernels INSIDE the solver loop (bench.py's roofline entries) ----------
// HIP events on the solve's stream around the fine-level launch of each kernel family, read after the per-iteration
// stream synchronisation the loop performs anyway.  Per calling thread (the adjoint solves run on autograd's thread
// and are not sampled); the only hidden state of the library, and only while enabled.
enum { KP_CGSTEP = 0, KP_UPDATE = 1, KP_FIRST2 = 2, KP_RESTRICT = 3, KP_PROLONG = 4, KP_SWEEP = 5, KP_COUNT = 6 };
struct KernelProfile {
  bool on = false;
  hipEvent_t e0[KP_COUNT] = {}, e1[KP_COUNT] = {};
  bool have[KP_COUNT] = {};
  double ms[KP_COUNT] = {};
  long long n[KP_COUNT] = {};
};
thread_local KernelProfile g_kp;
inline void kp_begin(int id, hipStream_t st) {
  if (g_kp.on) (void)hipEventRecord(g_kp.e0[id], st);
}
inline void kp_end(int id, hipStream_t st) {
  if (g_kp.on) {
    (void)hipEventRecord(g_kp.e1[id], st);
    g_kp.have[id] = true;
  }
}
inline void kp_collect() {  // call with the stream idle: every recorded event has completed
  if (!g_kp.on) return;
  for (int id = 0; id < KP_COUNT; ++id) {
    if (!g_kp.have[id]) continue;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, g_kp.e0[id], g_kp.e1[id]) == hipSuccess) {
      g_kp.ms[id] += ms;
      g_kp.n[id] += 1;
    }
    g_kp.have[id] = false;
  }
}

// ---- host-side hierarchy --------------------------------------------------------------------
constexpr int kMaxLevels = 16;

struct Hier {
  Level lev[kMaxLevels];
  int nl, Bv, Bp;
  const double* scale;
  double omega[8];  // per-sweep damping (Chebyshev-weighted Jacobi); post-smoothing runs them in reverse
  int nu, n_coarse, fmg_coarse_cycles;
  int fuse;  // 0: four single-stage strip passes per level; 1 / 2: fused two-stage passes, samples per lane
  int pre4;  // the fused PRE pass may take four samples per lane (fused_spl)
  int dense_mfma;  // coarsest-level dense solve of an fp32 cycle on the matrix cores (0: scalar-load kernel)
  double coarse_lmax;  // upper bound of the spectrum of D^-1 A on the coarsest level (2 for an M-matrix)
  // per-level work vectors
  void *xa[kMaxLevels], *xb[kMaxLevels], *res[kMaxLevels], *rhs[kMaxLevels];  // TV vectors of the V-cycle
  void *bF[kMaxLevels], *xF[kMaxLevels];  // full-multigrid start: restricted right-hand sides, iterates
};

// bpn = algorithmic bytes per (node, sample) of the launch, for diffhe_traffic_account
#define LAUNCH(bpn, kernel, n, ...)                                                  \
  do {                                                                               \
    diffhe::account((double)(bpn) * (double)(n) * H.Bp);                             \
    hipLaunchKernelGGL(kernel, lgrid((n), H.Bp), dim3(256), 0, st, __VA_ARGS__);     \
  } while (0)
// per-sample matrices: bytes of the nd stored diagonals (fp64) per node; a batch-shared matrix is amortised to 0
#define MATB(L) (H.Bv == 1 ? 0.0 : 8.0 * (L).nd)

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
  LAUNCH((xin ? 3 : 2) * sizeof(TV) + MATB(L), dia_jacobi_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, xin, xout, omega, part, H.Bp);
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
  LAUNCH(2 * sizeof(TV) + MATB(L) / L.nd, dia_jacobi_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, (const TV*)nullptr, xa, w0, (double*)nullptr, H.Bp);
  LAUNCH(3 * sizeof(TV) + MATB(L), dia_jacobi_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, (const TV*)xa, xb, w1, part, H.Bp);
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
  LAUNCH((res ? 3 : 2) * sizeof(TV) + MATB(L), dia_residual_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, x, res, part, H.Bp,
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
  LAUNCH(16.0 + MATB(L), dia_apply_dot_kernel, L.n, L, H.Bv, H.scale, x, y, part, H.Bp);
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
  LAUNCH(3 * sizeof(TV) + MATB(L) / L.nd, dia_cheby_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, (const TV*)nullptr, (const TV*)nullptr, xa, d, 0.0,
         1.0 / theta, (deg == 1) ? part : (double*)nullptr, H.Bp);
  for (int k = 1; k < deg; ++k) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    LAUNCH(5 * sizeof(TV) + MATB(L), dia_cheby_kernel<TV>, L.n, L, H.Bv, H.scale, rhs, (const TV*)xa, (const TV*)d, xb, d, rho_new * rho,
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
    LAUNCH(((double)F.n / C.n + 1.0) * sizeof(TV), mg_restrict_kernel<TV>, C.n, F, C, r, rc, H.Bp);
  }
}

template <typename TV>
void launch_prolong(const Hier& H, const Level& F, const Level& C, const TV* e, TV* x, int set, hipStream_t st) {
  if (transfers2_ok(F, C, H.Bp, sizeof(TV))) {
    diffhe::account(((set ? 1.0 : 2.0) + (double)C.n / F.n) * sizeof(TV) * (double)F.n * H.Bp);
    hipLaunchKernelGGL(mg_prolong2_kernel, transfer2_grid(F.n, H.Bp), dim3(256), 0, st, F, C, (const float*)e, (float*)x, H.Bp, set);
  } else {
    LAUNCH(((set ? 1.0 : 2.0) + (double)C.n / F.n) * sizeof(TV), mg_prolong_add_kernel<TV>, F.n, F, C, e, x, H.Bp, set);
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
template <typename TV>
TV* vcycle(const Hier& H, const TV* rhs0, double* rz_part, int* rz_blocks, hipStream_t st, int l0 = 0,
           const TV* guess = nullptr) {
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
      const int nb = op_jacobi<TV>(H, l, rhs[l], a, b2, H.omega[H.nu - 1 - s], lastsweep ? rz_part : nullptr, st);
      if (lastsweep && rz_blocks) *rz_blocks = nb;
      TV* t = a; a = b2; b2 = t;
    }
    cur[l] = a;
  }
  return cur[l0];
}

// Full multigrid start: solve on the coarsest level, then per level interpolate, take the residual
// and apply one V-cycle.  Gives the CG an iterate whose error is already smooth (about 3-4 CG
// iterations ahead of a zero guess) for ~0.8 of an iteration.  b0 = right-hand side in TV storage.
// *pending (optional): the fine level's last correction is NOT added to the returned iterate but handed back -- the
// caller's conversion pass (pcg_setx_kernel) adds the two in fp64, one pass over x less.
template <typename TV>
TV* fmg_start(const Hier& H, const TV* b0, hipStream_t st, const TV** pending = nullptr) {
  const int last = H.nl - 1;
  const TV* bl[kMaxLevels];
  bl[0] = b0;
  for (int l = 0; l < last; ++l) {
    launch_restrict<TV>(H, H.lev[l], H.lev[l + 1], bl[l], (TV*)H.bF[l + 1], st);
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
    if (l > 0 && (fused_level<TV>(H, l, &g1, &g2) & 2)) {
      // levels with the fused passes: ONE cycle from the prolonged guess -- no prolongation, residual or addition pass
      TV* it = vcycle<TV>(H, bl[l], nullptr, nullptr, st, l, coarse);
      if (cycles == 1) {
        coarse = it;          // consumed by the first launch of the next level, before that level's cycle reuses the buffer
        continue;
      }
      if (diffhe::check(hipMemcpyAsync(x, it, (size_t)L.n * H.Bp * sizeof(TV), hipMemcpyDeviceToDevice, st))) return nullptr;
      c0 = 1;
    } else {
      launch_prolong<TV>(H, L, H.lev[l + 1], coarse, x, 1, st);
    }
    for (int c = c0; c < cycles; ++c) {
      op_residual<TV>(H, l, bl[l], (const TV*)x, (TV*)H.rhs[l], nullptr, st);
      TV* e = vcycle<TV>(H, (const TV*)H.rhs[l], nullptr, nullptr, st, l);
      if (l == 0 && c == cycles - 1 && pending) {
        *pending = e;
        break;
      }
      LAUNCH(3 * sizeof(TV), mg_add_kernel<TV>, L.n, (const TV*)e, x, L.n, H.Bp);
    }
    coarse = x;
  }
  return (TV*)coarse;
}


}  // namespace
}  // namespace diffhe_lattice

using namespace diffhe_lattice;

extern "C" int diffhe_lattice_pcg_profile(int enable, double* total_ms, long long* launches) {
  if (total_ms) *total_ms = g_kp.ms[KP_CGSTEP];
  if (launches) *launches = g_kp.n[KP_CGSTEP];
  if (enable >= 0) {
    if (enable && !g_kp.e0[0]) {
      for (int id = 0; id < KP_COUNT; ++id)
        if (hipEventCreate(&g_kp.e0[id]) != hipSuccess || hipEventCreate(&g_kp.e1[id]) != hipSuccess) return DIFFHE_E_LAUNCH;
    }
    g_kp.on = enable != 0;
    for (int id = 0; id < KP_COUNT; ++id) {
      g_kp.ms[id] = 0.0;
      g_kp.n[id] = 0;
      g_kp.have[id] = false;
    }
  }
  return DIFFHE_OK;
}

extern "C" int diffhe_lattice_kernel_profile(int id, double* total_ms, long long* launches) {
  if (id < 0 || id >= KP_COUNT) return DIFFHE_E_BADARG;
  if (total_ms) *total_ms = g_kp.ms[id];
  if (launches) *launches = g_kp.n[id];
  return DIFFHE_OK;
}

// =========================================================================================
// C ABI
// =========================================================================================
static int fill_hier(Hier& H, const diffhe_mg_level* levels, int n_levels, int Bv, int Bp, const double* scale,
                     const double* omegas, int nu, int n_coarse) {
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
  for (int k = 0; k < 8; ++k) H.omega[k] = omegas[k < nu ? k : nu - 1];
  return DIFFHE_OK;
}

// V-cycle vectors, carved in units of doubles (fp32 vectors take half, rounded up to 64 B)
static long long carve(Hier& H, double* work, bool fp32) {
  long long off = 0;
  auto take = [&](long long cnt) {
    if (fp32) cnt = (cnt + 1) / 2;
    cnt = (cnt + 7) & ~7LL;
    double* p = work ? work + off : nullptr;
    off += cnt;
    return (void*)p;
  };
  for (int l = 0; l < H.nl; ++l) {
    const long long nb = (long long)H.lev[l].n * H.Bp;
    H.xa[l] = take(nb);
    H.xb[l] = take(nb);
    H.res[l] = take(nb);
    H.rhs[l] = take(nb);  // level 0: fp32 copy of the CG residual / FMG residual
    H.bF[l] = l > 0 ? take(nb) : nullptr;
    H.xF[l] = take(nb);
  }
  return off;
}

extern "C" long long diffhe_lattice_pcg_workspace_doubles(const diffhe_mg_level* levels, int n_levels, int Bp) {
  Hier H;
  const double w1 = 0.8;
  if (fill_hier(H, levels, n_levels, 1, Bp, nullptr, &w1, 1, 1)) return -1;
  const long long nb = (long long)H.lev[0].n * Bp;
  // r, the direction ring (kRingSlots fp32 = kRingSlots / 2 fp64 vectors), A p; the fp64 layout of the cycle is the larger
  return carve(H, nullptr, false) + (2 + kRingSlots / 2) * nb + 2LL * kPartBlocks * Bp + (32LL + kScalarSlices) * Bp + 64;
}

extern "C" int diffhe_lattice_pcg_solve(const diffhe_mg_level* levels, int n_levels, int Bv, const double* scale,
                                        const double* b, double* x, int Bp, double tol, double tol_energy, int max_iter,
                                        int nu, int n_coarse, const double* omegas_host, int flags, double* work,
                                        double* relres, double* err_est, int* iters, int* stop_rule, int* status_host,
                                        void* stream) {
  if (!b || !x || !work || !relres || !iters || !status_host || max_iter < 0) return DIFFHE_E_BADARG;
  Hier H;
  int rc = fill_hier(H, levels, n_levels, Bv, Bp, scale, omegas_host, nu, n_coarse);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const Level& L0 = H.lev[0];
  const int n = L0.n;
  const long long nb = (long long)n * Bp;
  const int nblk = lgrid(n, Bp).x;
  const bool f32 = (flags & DIFFHE_PCG_FP32) != 0;
  const bool use_fmg = (flags & DIFFHE_PCG_FMG) != 0 && H.nl > 1;
  const bool warm = (flags & DIFFHE_PCG_WARM) != 0;   // x holds an initial guess (e.g. the previous step of an optimisation)
  H.fmg_coarse_cycles = 1 + ((flags >> DIFFHE_PCG_FMG_CYCLES_SHIFT) & 3);
  if (flags & DIFFHE_PCG_UNFUSED) H.fuse = 0;             // keep the four single-stage passes (A/B runs, tests)
  if (flags & DIFFHE_PCG_DENSE_SCALAR) H.dense_mfma = 0;  // scalar-load dense coarse solve
  if (flags & DIFFHE_PCG_PRE2) H.pre4 = 0;                // fused PRE pass with two samples per lane as well (A/B runs, tests)
  const bool resid64 = (flags & DIFFHE_PCG_RESID_FP64) != 0;  // keep the fp64 residual where the pair would apply (A/B runs, tests)
  const bool keep_lo = (flags & DIFFHE_PCG_RESID_KEEP_LO) != 0;   // ... and the pair whole to the end of the solve (the same)
  const int trust_its = (flags >> DIFFHE_PCG_TRUST_ITS_SHIFT) & 15;   // development, tests: the energy rule's trusted iterations
  double* w = work + carve(H, work, f32);
  float* r32 = f32 ? (float*)H.rhs[0] : nullptr;
  double* r = w;
  float* rlo = (float*)(void*)r;   // `rpair`: the residual's low parts live in the first half of r's region, r itself is unused
  // Search directions.  Fused loop: the iterate is NOT touched inside the loop (that cost 16 of the fused step's 36
  // bytes per node); the directions p_j stay in a ring of slots (10 fp32 / 5 fp64 vectors in these 5 nb doubles) with
  // their step lengths alpha_j, and x += sum_j alpha_j p_j is formed when the ring is full or the solve ends.
  // Unfused loop (small meshes / batches): one fp64 p in the same region, x updated every iteration.
  double* p = r + nb;
  const int n_slots = f32 ? kRingSlots : kRingSlots / 2;
  const long long slot_stride = nb;              // in elements of the stored type: fp32 slots are nb floats apart
  double* Ap = p + (kRingSlots / 2) * nb;
  double* partA = Ap + nb;
  double* partB = partA + (long long)kPartBlocks * Bp;
  double* sc = partB + (long long)kPartBlocks * Bp;
  PcgScalars S;
  S.rz = sc; S.alpha = sc + Bp; S.beta = sc + 2 * Bp; S.bb = sc + 3 * Bp; S.tol2 = sc + 4 * Bp;
  S.active = (int*)(sc + 5 * Bp);
  S.iters = iters;
  S.n_active = (int*)(sc + 6 * Bp);   // two ints: [0] active samples, [1] those of them too far to drop the low half
  const bool use_floor = (flags & DIFFHE_PCG_NO_FLOOR) == 0;  // set: stop on `tol` alone
  S.maxdiag = sc + 9 * Bp;  // Bv entries (Bv <= Bp)
  S.rs = f32 ? sc + 11 * Bp : nullptr;
  S.scale = scale;
  S.Bv = Bv;
  S.energy = sc + 12 * Bp;
  S.est = err_est ? err_est : sc + 13 * Bp;
  S.rr = sc + 14 * Bp;
  S.gap = sc + 15 * Bp;
  S.lo_state = 0;
  S.rule = stop_rule ? stop_rule : (int*)(sc + 7 * Bp);
  double* alpha_ring = sc + 16 * Bp;              // n_slots (<= 10) rows of Bp step lengths (the scalar block has 32 rows)
  double* const alpha_single = S.alpha;
  // tol_energy is asked of the FINAL iterate, which receives one more multigrid correction after the decision
  // (pcg_finish_kernel): the CG iterate's own estimate may be 1 / 0.3 of it (0.3: a cautious bound of the V(2,2)
  // cycle's convergence factor; measured reductions of the nodal error by that step: 5-8x)
  S.tol_e2 = tol_energy > 0.0 ? (tol_energy / 0.3) * (tol_energy / 0.3) : 0.0;
  S.e_max_it = 10 + ((tol_energy > 0.0 && tol_energy < 1e-11) ? (int)ceil(log10(1e-11 / tol_energy) - 1e-9) : 0);
  if (trust_its) S.e_max_it = trust_its;
  S.have_energy = 0;
  if (use_floor && use_fmg) {
    rc = diffhe::check(hipMemsetAsync((void*)S.maxdiag, 0, sizeof(double) * Bv, st));
    if (rc) return rc;
    hipLaunchKernelGGL(dia_maxdiag_kernel, node_grid(L0.n, Bv, 512), dim3(256), 0, st, L0, Bv,
                       (unsigned long long*)S.maxdiag);
  }
  {  // spectrum bound for the coarsest-level Chebyshev solve: 2 unless the mesh has obtuse triangles
    const Level& Lc = H.lev[H.nl - 1];
    if (Lc.nd == 4) {
      unsigned long long* gb = (unsigned long long*)(sc + 8 * Bp);
      rc = diffhe::check(hipMemsetAsync(gb, 0, sizeof(unsigned long long), st));
      if (rc) return rc;
      hipLaunchKernelGGL(dia_gershgorin_kernel, node_grid(Lc.n, Bv, 256), dim3(256), 0, st, Lc, Bv, gb);
      double bound = 0.0;
      rc = diffhe::check(hipMemcpyAsync(&bound, gb, sizeof(double), hipMemcpyDeviceToHost, st));
      if (!rc) rc = diffhe::check(hipStreamSynchronize(st));
      if (rc) return rc;
      if (bound > 2.0 && bound < 1e3) H.coarse_lmax = bound * (1.0 + 1e-9);
    }
  }
  const dim3 sgrid((Bp + 63) / 64);
  double* const slices = sc + 32LL * Bp;          // kScalarSlices rows: first stage of long partial lists
#define SCALAR(phase, part, nb_)                                                                                           \
  do {                                                                                                                     \
    if ((int)(nb_) >= 256) {                                                                                               \
      hipLaunchKernelGGL(pcg_slice_kernel, dim3(sgrid.x, kScalarSlices), dim3(256), 0, st, (const double*)(part), (int)(nb_), \
                         Bp, slices);                                                                                      \
      hipLaunchKernelGGL(pcg_scalar_kernel, sgrid, dim3(1024), 0, st, (int)(phase), (const double*)slices, kScalarSlices, Bp, \
                         tol, S, relres);                                                                                  \
    } else {                                                                                                               \
      hipLaunchKernelGGL(pcg_scalar_kernel, sgrid, dim3(1024), 0, st, (int)(phase), (const double*)(part), (int)(nb_), Bp,   \
                         tol, S, relres);                                                                                  \
    }                                                                                                                      \
  } while (0)

  for (int l = 0; l < H.nl; ++l)
    if (H.lev[l].shift && (H.lev[l].inv || Bv != 1)) return DIFFHE_E_BADARG;  // a shift belongs to a factored operator
  if (H.nl == 1 && L0.inv && Bv == 1 && !f32 && L0.n <= kPartBlocks) {
    // DIRECT solve: the whole system is small enough for the dense inverse of its (batch-shared) matrix -- the
    // reference's own regime (2D meshes up to 32 x 32).  x = (1 / s_b) K_1^{-1} b in one launch, then the true residual.
    diffhe::account(16.0 * (double)n * Bp);
    if (Bp >= kWave)
      hipLaunchKernelGGL((mg_dense_solve_kernel<double, 4>), dim3((n + 3) / 4, Bp / kWave), dim3(256), 0, st, n,
                         (const double*)L0.inv, scale, b, x, (double*)nullptr, Bp);
    else
      hipLaunchKernelGGL(mg_dense_small_kernel<double>, dim3(n), dim3(64), 0, st, n, (const double*)L0.inv, scale, b, x,
                         (double*)nullptr, Bp);
    LAUNCH(8.0, pcg_init_kernel, n, b, (double*)nullptr, (double*)nullptr, partA, n, Bp);
    SCALAR(S_INIT, partA, nblk);                                 // b.b (and the bookkeeping S_RELRES reads)
    const int nbr = op_residual<double>(H, 0, b, (const double*)x, (double*)nullptr, partA, st);
    SCALAR(S_RELRES, partA, nbr);
    rc = diffhe::check(hipMemsetAsync(S.est, 0, sizeof(double) * Bp, st));
    if (rc) return rc;
    if (stop_rule) {  // direct solve: nothing iterated, nothing stopped
      rc = diffhe::check(hipMemsetAsync(stop_rule, 0, sizeof(int) * Bp, st));
      if (rc) return rc;
    }
    rc = diffhe::check_launch();
    if (rc) return rc;
    status_host[0] = 0;
    status_host[1] = 0;
    status_host[3] = 0;
    return DIFFHE_OK;
  }

  int nbz = 0, nba = 0;
  // Fused loop (fine level runs the strip kernels): per iteration
  //   [p = z + beta p ; x += alpha_prev p_old ; Ap = A p ; p.Ap]  ->  alpha  ->  [r -= alpha Ap ; r.r]
  //   -> convergence flags  ->  z = V(r) (last sweep leaves r.z)  ->  beta
  // Unfused fallback (small meshes / batches): separate p-update, apply and x/r update kernels.
  const StripGeom g0 = strip_geom(L0, Bp, kPupdCols);
  const bool fused = g0.use;
  // batch-shared matrix, fp32-stored directions: A p is never stored -- the residual update recomputes it from p (F_RUPD)
  const bool rupd = fused && f32 && Bv == 1;
  // ... and there the residual is carried as a pair of fp32 vectors, r32 (what the V-cycle reads) + rlo, not as fp64 r
  // plus r32 (F_RPAIR, lattice.h): nothing but the residual update and the pass that opens the loop touches it
  // (the pass that opens the loop must be the strip one too: it is what writes the pair -- residual_pass; today the two
  // geometries' `use` cannot differ, the condition keeps the pair from ever depending on that)
  const bool rpair = rupd && !resid64 && strip_geom(L0, Bp).use;
  const bool light_init = (use_fmg && f32) || warm;  // the start overwrites x and r (cold) / x is the caller's guess (warm)
  LAUNCH(light_init ? 8.0 : 24.0, pcg_init_kernel, n, b, light_init ? (double*)nullptr : x, r, partA, n, Bp);
  SCALAR(S_INIT, partA, nblk);
  // fp32 copy of rs * b (rs from S_INIT): the full-multigrid start's right-hand side, or r0 of a zero start -- of which
  // the pair path needs the low parts too (they go where pcg_init_kernel has just put the fp64 r0, unused on that path)
  if (f32 && !warm) {
    const bool lo_too = rpair && !use_fmg;
    LAUNCH(lo_too ? 16.0 : 12.0, pcg_cvt_kernel, n, b, (const double*)S.rs, r32, n, Bp, lo_too ? rlo : (float*)nullptr);
  }
  // cgstep2_kernel: two samples per lane for batches that are multiples of 128, else one
  // (four samples per lane -- what pays in the fused PRE pass -- measured here too: 0.699 -> 0.711 ms at 4 waves per SIMD
  // instead of 8, gpurun_out/r4n; not kept)
  const int cspl = (Bp % (2 * kWave) == 0) ? 2 : 1;
  const StripGeom g2 = (Bp % kWave == 0) ? strip_geom(L0, Bp, 4, cspl) : StripGeom{false, 0, 0, 0};
  const void* z = nullptr;
  int it = 0, flushed = 0;       // iterations done / directions already folded into x (fused loop)
  // x += sum_{j = flushed .. it-1} alpha_j p_j  (+ z / rs at the end of the solve: pcg_finish_kernel)
  auto flush_directions = [&](bool with_z) {
    const int count = it - flushed;
    if (count == 0 && !with_z) return;
    const double bytes = 16.0 + (f32 ? 4.0 : 8.0) * (count + (with_z ? 1 : 0));
    if (f32)
      LAUNCH(bytes, pcg_finish_kernel<float>, n, (const double*)alpha_ring, (const float*)(const void*)p, slot_stride,
             flushed, count, n_slots, with_z ? (const float*)z : (const float*)nullptr, (const double*)S.rs, x, n, Bp);
    else
      LAUNCH(bytes, pcg_finish_kernel<double>, n, (const double*)alpha_ring, (const double*)p, slot_stride, flushed, count,
             n_slots, with_z ? (const double*)z : (const double*)nullptr, (const double*)nullptr, x, n, Bp);
    flushed = it;
  };
  auto precondition = [&](int first) {
    if (f32) z = vcycle<float>(H, (const float*)r32, partB, &nbz, st);
    else z = vcycle<double>(H, (const double*)r, partB, &nbz, st);
    SCALAR(first ? S_RZ0 : S_BETA, partB, nbz);
  };
  auto apply_step = [&](int first) {
    if (fused) {
      if (!first) kp_begin(KP_CGSTEP, st);  // the first step of a solve (p = z) moves fewer bytes: not timed
      if (it - flushed == n_slots) flush_directions(false);   // ring full: fold everything so far into x
      const size_t esz = f32 ? sizeof(float) : sizeof(double);
      char* ring = (char*)p;
      Extra ex{};
      ex.a0 = z;
      ex.p_in = ring + (size_t)((it + n_slots - 1) % n_slots) * slot_stride * esz;
      ex.p_out = ring + (size_t)(it % n_slots) * slot_stride * esz;
      ex.x = nullptr;            // deferred (flush_directions)
      ex.alpha = nullptr; ex.beta = S.beta; ex.first = first;
#define NXV(MINW_, MATS_)                                                                                             \
  launch_strip<double, M_APPLY, false, F_PUPD_NX, float, kPupdCols, MINW_, MATS_>(                                         \
      L0, Bv, scale, (const double*)nullptr, (const double*)nullptr, rupd ? (double*)nullptr : Ap, 0.0, 0.0, partA, Bp, g0, \
      st, ex)
      // DIFFHE_PCG_CLOSED_FP32_STEP: the caller vouches for a lattice closed by Dirichlet data (lambda_min of the scaled operator bounded
      // away from 0).  With large Neumann parts the search directions are dominated by near-null modes, for which the
      // fp32 stencil cancels to noise: measured 13 / 11 instead of 12 / 9 iterations to 1e-14 there (gpurun_out/r6g)
      // (the host also asks for near-square cells and a hierarchy that reaches the dense coarsest level: on a 382 x 259
      // lattice, which coarsens once, 36 iterations to 1e-14 became 38 -- tools/stress.py seed 6301 case 39)
      if (f32 && rupd && (flags & DIFFHE_PCG_CLOSED_FP32_STEP) && g2.use && shared32_ok(L0, Bv, Bp) &&
          strip2_tile_fits(L0, Bp, g2.TR + 3)) {
        // fp32 stencil for p.Ap (cgstep2_kernel; packed, two samples per lane, where the batch allows): the step length only
        launch_cgstep2(L0, scale, (const double*)S.beta, first, (const float*)z, (const float*)ex.p_in, (float*)ex.p_out,
                       partA, Bp, g2, cspl, st);
        S.alpha = alpha_ring + (long long)(it % n_slots) * Bp;
        nba = g2.ncb * g2.nrc;
        if (!first) kp_end(KP_CGSTEP, st);
        return;
      }
      if (f32) {
        // 72 VGPRs (18 spilled), 7 waves per SIMD: 1.16 ms against 1.28 at the compiler's own 85 / 5; 8-column strips
        // (142 VGPRs) 1.96, 2-column strips at 8 waves 1.27, 6 or 8 waves 1.25 / 1.18 (same box, gpurun_out/r2l/variants*.txt).
        // The same cap on the V-cycle's strip kernels (already 6-7 waves) made them slower: -2...-6 % end to end.
        // per-sample matrices (coefficients in VGPRs): 4 waves per SIMD, 245.2 ms per step of the per-element-field variant
        // against 249.5 at 7 (gpurun_out/r4w)
        if (Bv != 1) NXV(4, MAT_PER_SAMPLE); else NXV(7, MAT_ANY);
      }
#undef NXV
      else
        launch_strip<double, M_APPLY, false, F_PUPD_NX, double, kPupdCols>(L0, Bv, scale, (const double*)nullptr,
                                                                (const double*)nullptr, Ap, 0.0, 0.0, partA, Bp, g0, st, ex);
      S.alpha = alpha_ring + (long long)(it % n_slots) * Bp;   // alpha_it goes next to p_it
      nba = g0.ncb * g0.nrc;
      if (!first) kp_end(KP_CGSTEP, st);
    } else {
      if (f32) LAUNCH(first ? 12.0 : 20.0, pcg_update_p_kernel<float>, n, (const float*)z, (const double*)S.beta, p, first, n, Bp);
      else LAUNCH(first ? 16.0 : 24.0, pcg_update_p_kernel<double>, n, (const double*)z, (const double*)S.beta, p, first, n, Bp);
      nba = op_apply_dot(H, p, Ap, partA, st);
    }
  };
  // r = b - A x (+ its fp32 copy, + the partials b.x and x.(A x) of the energy bound when asked for)
  auto residual_pass = [&](bool energy) {
    const StripGeom gr = strip_geom(L0, Bp);
    if (gr.use && f32) {  // r and its fp32 copy in one pass (rpair: the two halves of the pair)
      Extra ex{};
      ex.r32 = r32;
      ex.rscale = S.rs;
      ex.dot_bx = energy ? 1 : 0;   // partial sums of this pass: b.x0 and x0.(A x0) (S_ENERGY / S_ENERGY2)
      ex.part2 = energy ? partB : nullptr;
      if (rpair) {
        ex.rlo = rlo;
        launch_strip<double, M_RESID, false, F_RPAIR, double, kStripCols, 1, MAT_SHARED>(
            L0, Bv, scale, (const double*)x, b, (double*)nullptr, 0.0, 0.0, energy ? partA : (double*)nullptr, Bp, gr, st, ex);
      } else {
        launch_strip<double, M_RESID, false>(L0, Bv, scale, (const double*)x, b, r, 0.0, 0.0, energy ? partA : (double*)nullptr,
                                             Bp, gr, st, ex);
      }
      nba = gr.ncb * gr.nrc;
    } else {
      nba = op_residual<double>(H, 0, b, (const double*)x, r, energy ? partA : (double*)nullptr, st, energy ? 1 : 0,
                                energy ? partB : (double*)nullptr);
      if (f32) LAUNCH(12.0, pcg_cvt_kernel, n, (const double*)r, (const double*)S.rs, r32, n, Bp);
    }
    if (energy) {
      SCALAR(S_ENERGY, partA, nba);
      SCALAR(S_ENERGY2, partB, nba);
      S.have_energy = 1;
    }
  };
  if (use_fmg) {
    // cold: x0 = FMG(b).  warm: x0 = x + FMG(b - A x) -- the full-multigrid start applied to the residual equation of
    // the caller's guess (an optimisation loop's previous solution): the start is then as accurate as the guess is
    // close, times the ~1e-3 of the full-multigrid step itself.
    if (warm) residual_pass(false);
    if (f32) {
      const float* e0 = nullptr;
      const float* x0 = fmg_start<float>(H, (const float*)r32, st, &e0);
      if (!x0) return DIFFHE_E_LAUNCH;
      LAUNCH((warm ? 20.0 : 12.0) + (e0 ? 4.0 : 0.0), pcg_setx_kernel<float>, n, x0, (const double*)S.rs, x,
             use_floor ? partA : (double*)nullptr, n, Bp, warm ? 1 : 0, e0);
    } else {
      const double* e0 = nullptr;
      const double* x0 = fmg_start<double>(H, warm ? (const double*)r : b, st, &e0);
      if (!x0) return DIFFHE_E_LAUNCH;
      LAUNCH((warm ? 24.0 : 16.0) + (e0 ? 8.0 : 0.0), pcg_setx_kernel<double>, n, x0, (const double*)nullptr, x,
             use_floor ? partA : (double*)nullptr, n, Bp, warm ? 1 : 0, e0);
    }
    if (use_floor) SCALAR(S_FLOOR, partA, nblk);
    residual_pass(true);
  } else if (warm) {
    residual_pass(true);
  }
  precondition(1);
  rc = diffhe::check_launch();
  if (rc) return rc;

  int n_active = -1;
  // The pair's low half (PcgScalars::gap has the argument): whole until the batch is near its energy-rule stop, then ONE
  // update that reads the pair and stores hi alone (F_RDROP), then hi alone (F_RSINGLE).  Only where that rule is in force.
  bool may_drop = rpair && !keep_lo && S.tol_e2 > 0.0;
  int lo_state = 0;      // form of the next update: 0 F_RPAIR, 1 F_RDROP, 2 F_RSINGLE
  int n_single = 0;      // updates that wrote no low half (status_host[3])
  while (it < max_iter) {
    apply_step(it == 0);
    SCALAR(S_ALPHA, partA, nba);
    kp_begin(KP_UPDATE, st);
    if (rupd) {
      Extra ex{};
      ex.p_in = (char*)p + (size_t)(it % n_slots) * slot_stride * sizeof(float);   // the direction apply_step just stored
      ex.x = r;
      ex.r32 = r32;
      ex.rscale = S.rs;
      ex.alpha = S.alpha;
      ex.rlo = rlo;
      // 5 waves per SIMD: 1.30 ms at 1024^2 x 256 (compiler's own choice 1.30, 7 waves 2.31 with spills; gpurun_out/r4q)
      // the pair form: 1.13 ms; the compiler's own choice measured 0.8 ms per step slower
#define RUPD_PAIR(FUSE_)                                                                                   \
  launch_strip<double, M_APPLY, false, FUSE_, float, kPupdCols, 5, MAT_SHARED>(   /* rupd: Bv == 1 */        \
      L0, Bv, scale, (const double*)nullptr, (const double*)nullptr, (double*)nullptr, 0.0, 0.0, partA, Bp, g0, st, ex)
      if (rpair && lo_state == 0) RUPD_PAIR(F_RPAIR);
      else if (rpair && lo_state == 1) RUPD_PAIR(F_RDROP);
      else if (rpair) RUPD_PAIR(F_RSINGLE);
#undef RUPD_PAIR
      else
        launch_strip<double, M_APPLY, false, F_RUPD, float, kPupdCols, 5, MAT_SHARED>(
            L0, Bv, scale, (const double*)nullptr, (const double*)nullptr, (double*)nullptr, 0.0, 0.0, partA, Bp, g0, st, ex);
    } else {
      LAUNCH(24.0 + (r32 ? 4.0 : 0.0) + (fused ? 0.0 : 24.0), pcg_update_kernel, n, (const double*)p, (const double*)Ap, (const double*)S.alpha, fused ? (double*)nullptr : x,
             r, r32, (const double*)S.rs, partA, n, Bp);
    }
    kp_end(KP_UPDATE, st);
    S.lo_state = lo_state;
    SCALAR(S_CONV, partA, rupd ? g0.ncb * g0.nrc : nblk);
    ++it;
    if (lo_state) {
      ++n_single;
      lo_state = 2;
      if (it >= S.e_max_it) {
        // the energy rule is no longer trusted from here on, and with it the argument that let the low half go: replace
        // the residual ONCE by b - A x of the iterate (which rewrites the pair) and keep it whole for the rest of the solve
        flush_directions(false);
        residual_pass(false);
        lo_state = 0;
        may_drop = false;
      }
    }
    // z = V(r) and r.z: the new search direction's ingredients AND the energy-norm error estimate of the iterate;
    // the samples still active are counted in the scalar phase behind it (S_BETA)
    precondition(0);
    // [2] the active samples, [3] those of them that still need the low half: one copy, as before
    rc = diffhe::check(hipMemcpyAsync(&status_host[2], S.n_active, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (rc) return rc;
    rc = diffhe::check(hipStreamSynchronize(st));
    if (rc) return rc;
    n_active = status_host[2];
    kp_collect();  // the stream is idle here
    if (n_active == 0) break;
    if (may_drop && lo_state == 0 && status_host[3] == 0) lo_state = 1;   // sticky: only the replacement above undoes it
  }
  // fold the directions still in the ring into x and add the final V-cycle's correction z (pcg_finish_kernel);
  // the unfused loop kept x current: only z is due there
  if (!fused) flushed = it;
  flush_directions(true);
  S.alpha = alpha_single;
  nba = op_residual<double>(H, 0, b, (const double*)x, (double*)nullptr, partA, st);
  SCALAR(S_RELRES, partA, nba);
  rc = diffhe::check_launch();
  if (rc) return rc;
  status_host[0] = it;
  status_host[1] = n_active < 0 ? 0 : n_active;
  status_host[3] = n_single;
  return DIFFHE_OK;
}

// kept in the ABI for bench.py: the fp32 CG recomputes A p in the residual update (F_RUPD); the fused passes take two
// samples per lane
extern "C" int diffhe_lattice_recompute_ap(void) { return 1; }

extern "C" int diffhe_lattice_blocks(int n, int Bp) { (void)n; (void)Bp; return kPartBlocks; }

extern "C" int diffhe_lattice_fused_passes(void) { return 2; }

extern "C" int diffhe_lattice_apply(const diffhe_mg_level* level, int Bv, const double* scale, const double* x,
                                    double* y, double* part, int Bp, void* stream) {
  if (!x || !y || !part) return DIFFHE_E_BADARG;
  Hier H;
  const double w1 = 0.8;
  int rc = fill_hier(H, level, 1, Bv, Bp, scale, &w1, 1, 1);
  if (rc) return rc;
  op_apply_dot(H, x, y, part, (hipStream_t)stream);
  return diffhe::check_launch();
}

extern "C" int diffhe_lattice_bilinear(const diffhe_mg_level* level, int Bv, const double* scale, const double* x,
                                       const double* lam, const double* add, double* part, double* out, int Bp,
                                       void* stream) {
  if (!x || !lam || !part || !out) return DIFFHE_E_BADARG;
  Hier H;
  const double w1 = 0.8;
  int rc = fill_hier(H, level, 1, Bv, Bp, scale, &w1, 1, 1);
  if (rc) return rc;
  const StripGeom g = strip_geom(H.lev[0], Bp);
  if (!g.use) return DIFFHE_E_TOOBIG;  // small problems: use diffhe_p1_grad_kappa
  hipStream_t st = (hipStream_t)stream;
  Extra ex{};
  ex.dotv = lam;
  ex.addv = add;
  launch_strip<double, M_APPLY, false>(H.lev[0], Bv, scale, x, (const double*)nullptr, (double*)nullptr, 0.0, 0.0, part,
                                       Bp, g, st, ex);
  PcgScalars S{};
  hipLaunchKernelGGL(pcg_scalar_kernel, dim3((Bp + 63) / 64), dim3(1024), 0, st, (int)S_SUM, (const double*)part,
                     g.ncb * g.nrc, Bp, 0.0, S, out);
  return diffhe::check_launch();
}

extern "C" int diffhe_lattice_cg_step(const diffhe_mg_level* level, int Bv, const double* scale, const void* z,
                                      int z_fp32, const void* p_in, void* p_out, double* x, const double* alpha,
                                      const double* beta, int first, double* Ap, double* part, int Bp, void* stream) {
  if (!z || !p_out || !Ap || !part || (!first && (!p_in || !beta || (x && !alpha)))) return DIFFHE_E_BADARG;
  Hier H;
  const double w1 = 0.8;
  int rc = fill_hier(H, level, 1, Bv, Bp, scale, &w1, 1, 1);
  if (rc) return rc;
  const StripGeom g = strip_geom(H.lev[0], Bp, kPupdCols);
  if (!g.use) return DIFFHE_E_TOOBIG;
  Extra ex{};
  ex.a0 = z; ex.p_in = p_in; ex.p_out = p_out; ex.x = x; ex.alpha = alpha; ex.beta = beta; ex.first = first;
  hipStream_t st = (hipStream_t)stream;
#define CGSTEP(FUSE_, TA_)                                                                                          \
  launch_strip<double, M_APPLY, false, FUSE_, TA_, kPupdCols>(H.lev[0], Bv, scale, (const double*)nullptr,              \
                                                              (const double*)nullptr, Ap, 0.0, 0.0, part, Bp, g, st, ex)
  if (x) {
    if (z_fp32) CGSTEP(F_PUPD, float); else CGSTEP(F_PUPD, double);
  } else {
    if (z_fp32)   // the solver's instantiation (7 waves per SIMD)
      launch_strip<double, M_APPLY, false, F_PUPD_NX, float, kPupdCols, 7>(H.lev[0], Bv, scale, (const double*)nullptr,
                                                                          (const double*)nullptr, Ap, 0.0, 0.0, part, Bp, g, st, ex);
    else
      CGSTEP(F_PUPD_NX, double);
  }
#undef CGSTEP
  return diffhe::check_launch();
}

extern "C" int diffhe_lattice_smooth(const diffhe_mg_level* level, int Bv, const double* scale, const double* rhs,
                                     const double* xin, double* xout, double omega, int Bp, void* stream) {
  if (!rhs || !xout) return DIFFHE_E_BADARG;
  Hier H;
  int rc = fill_hier(H, level, 1, Bv, Bp, scale, &omega, 1, 1);
  if (rc) return rc;
  op_jacobi<double>(H, 0, rhs, xin, xout, omega, nullptr, (hipStream_t)stream);
  return diffhe::check_launch();
}
