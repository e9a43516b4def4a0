// General path, assembly: element integrals, assembly into a batch-shared ELL pattern, Dirichlet elimination, the
// batch-shared product, Galerkin coarse values, gradient contraction (batch-shared: KappaForm, the scalar form of element_grad.h),
// layout changes.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "element_grad.h"
#include "ell.h"

namespace {
using namespace diffhe_ell;

// ---------------------------------------------------------------------------------------
// Element integrals (reference solver.py:84-88 1D, solver.py:119-139 2D)
// ---------------------------------------------------------------------------------------
__device__ inline void tri_integrals(double xi, double yi, double xj, double yj, double xk, double yk, double* k0,
                                     double* area_out) {
  const double area = 0.5 * fabs((xj - xi) * (yk - yi) - (xk - xi) * (yj - yi));  // solver.py:119
  const double bb[3] = {yj - yk, yk - yi, yi - yj};                               // solver.py:125-129
  const double cc[3] = {xk - xj, xi - xk, xj - xi};                               // solver.py:130-134
  const bool keep = !(area < 1e-15);                                              // solver.py:120-121
  const double inv = keep ? 1.0 / (4.0 * area) : 0.0;
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < 3; ++q) k0[p * 3 + q] = keep ? (bb[p] * bb[q] + cc[p] * cc[q]) * inv : 0.0;
  *area_out = keep ? area : 0.0;
}

// P1 tetrahedron [v0, v1, v2, v3] (ours: the reference stops at 2D, solver.py:67).  Edge vectors a, b, c from v0; the
// cofactor vectors g_1 = b x c, g_2 = c x a, g_3 = a x b, g_0 = -(g_1 + g_2 + g_3) are 6 V grad phi_p, det = a . g_1 =
// +-6 V, so k0[pq] = (g_p . g_q) / (36 V) with 36 V = 6 |det|.  Every operation is rounded on its own (no contraction): a
// product that cancels exactly (hx hy - hy hx on an axis-aligned box) stays an exact zero, which is what lets the plan
// drop structurally zero couplings (diffhe/plan.py: build_ell_pattern) -- and what reference_order_integrals restates
// on the host bit for bit.  Degenerate: |det| <= 1e-12 l^3, l the longest of a, b, c (relative to the element's size,
// unlike the triangles' absolute 1e-15); such a tetrahedron contributes nothing, *vol_out = 0.
__device__ inline void tet_integrals(const double* __restrict__ coords, int n, int v0, int v1, int v2, int v3, double* k0,
                                     double* vol_out) {
#pragma clang fp contract(off)
  const double* X = coords;
  const double* Y = coords + n;
  const double* Z = coords + 2 * (i64)n;
  const double x0 = X[v0], y0 = Y[v0], z0 = Z[v0];
  const double ax = X[v1] - x0, ay = Y[v1] - y0, az = Z[v1] - z0;
  const double bx = X[v2] - x0, by = Y[v2] - y0, bz = Z[v2] - z0;
  const double cx = X[v3] - x0, cy = Y[v3] - y0, cz = Z[v3] - z0;
  double g[4][3];
  g[1][0] = by * cz - bz * cy; g[1][1] = bz * cx - bx * cz; g[1][2] = bx * cy - by * cx;
  g[2][0] = cy * az - cz * ay; g[2][1] = cz * ax - cx * az; g[2][2] = cx * ay - cy * ax;
  g[3][0] = ay * bz - az * by; g[3][1] = az * bx - ax * bz; g[3][2] = ax * by - ay * bx;
#pragma unroll
  for (int d = 0; d < 3; ++d) g[0][d] = -((g[1][d] + g[2][d]) + g[3][d]);
  const double det = ax * g[1][0] + ay * g[1][1] + az * g[1][2];
  const double la = ax * ax + ay * ay + az * az, lb = bx * bx + by * by + bz * bz, lc = cx * cx + cy * cy + cz * cz;
  const double l2 = fmax(fmax(la, lb), lc);
  const bool keep = fabs(det) > 1e-12 * (l2 * sqrt(l2));
  const double den = keep ? 6.0 * fabs(det) : 1.0;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      k0[p * 4 + q] = keep ? (g[p][0] * g[q][0] + g[p][1] * g[q][1] + g[p][2] * g[q][2]) / den : 0.0;
  *vol_out = keep ? fabs(det) / 6.0 : 0.0;
}

__global__ __launch_bounds__(256) void element_integrals_kernel(const double* __restrict__ coords,
                                                                 const int* __restrict__ elems, int dim, int n, int m,
                                                                 double* __restrict__ k0, double* __restrict__ m0) {
  for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (i64)gridDim.x * blockDim.x) {
    if (dim == 1) {
      const int i = elems[e], j = elems[(i64)m + e];
      const double h = coords[j] - coords[i];
      const double k = 1.0 / h;
      k0[e] = k; k0[(i64)m + e] = -k; k0[2 * (i64)m + e] = -k; k0[3 * (i64)m + e] = k;
      m0[e] = 0.5 * h; m0[(i64)m + e] = 0.0; m0[2 * (i64)m + e] = 0.0; m0[3 * (i64)m + e] = 0.5 * h;
    } else if (dim == 3) {
      double loc[16], vol;
      tet_integrals(coords, n, elems[e], elems[(i64)m + e], elems[2 * (i64)m + e], elems[3 * (i64)m + e], loc, &vol);
#pragma unroll
      for (int pq = 0; pq < 16; ++pq) {
        k0[(i64)pq * m + e] = loc[pq];
        // F_p += V/4 * (f_0+f_1+f_2+f_3)/4: the 2D rule above lifted to tetrahedra (no reference rule to copy)
        m0[(i64)pq * m + e] = vol / 16.0;
      }
    } else {
      const int i = elems[e], j = elems[(i64)m + e], k = elems[2 * (i64)m + e];
      double loc[9], area;
      tri_integrals(coords[i], coords[(i64)n + i], coords[j], coords[(i64)n + j], coords[k], coords[(i64)n + k], loc,
                    &area);
#pragma unroll
      for (int pq = 0; pq < 9; ++pq) {
        k0[(i64)pq * m + e] = loc[pq];
        m0[(i64)pq * m + e] = area / 9.0;  // F_p += area/3 * (f_i+f_j+f_k)/3, solver.py:143-145
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Deterministic row-gather assembly + Dirichlet elimination
// ---------------------------------------------------------------------------------------
// REF = true: `local` holds t = b_p b_q + c_p c_q (2D) or 1 / -1 (1D) and `den` holds 4 area (2D) or h (1D); every
// contribution is formed as (kappa * t) / den with each operation rounded on its own and added in element order --
// the operation order of the reference's loops (solver.py:88-92, :139-140), so the stored values (and the lifting
// terms) are bit-identical to the reference's K.  REF = false: kappa * k0 with contracted multiply-adds.
template <bool REF>
__global__ __launch_bounds__(256) void assemble_rows_kernel(
    const double* __restrict__ local, const double* __restrict__ den, const double* __restrict__ kappa, i64 kse,
    i64 ksb, const int* __restrict__ ent_ptr, const int* __restrict__ contrib, const int* __restrict__ cols,
    const int* __restrict__ store_slot, const unsigned char* __restrict__ is_bc, const double* __restrict__ g,
    double* __restrict__ vals, double* __restrict__ lift, int n, int m, int W, int Bv) {
#pragma clang fp contract(off)
  const NodeMap nm = node_map(Bv);
  if (nm.b >= Bv) return;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const bool row_bc = is_bc && is_bc[i];
    double lf = 0.0;
    for (int k = 0; k < W; ++k) {
      const i64 ent = (i64)k * n + i;
      const int store = store_slot ? store_slot[k] : k;
      const int j = cols[ent];
      const bool col_bc = is_bc && j != i && is_bc[j];
      // entries that are not stored (lower triangle of a symmetric format) only matter for the lift
      if (store < 0 && (row_bc || !col_bc)) continue;
      const int c0 = ent_ptr[ent], c1 = ent_ptr[ent + 1];
      double v = 0.0;
      for (int c = c0; c < c1; ++c) {
        const int code = contrib[c];
        const int e = code >> 6, pq = code & 63;   // local entry p * npe + q: < 9 for P1 triangles, < 36 for P2
        const double kap = kappa ? kappa[(i64)e * kse + (i64)nm.b * ksb] : 1.0;
        if (REF) {
          const double num = kap * local[(i64)pq * m + e];
          v = v + num / den[e];  // K[p,q] = K[p,q] + kappa * t / (4 area), solver.py:139-140
        } else {
          v = fma(kap, local[(i64)pq * m + e], v);  // K[p,q] += kappa * k0[p,q], solver.py:89-92/:137-140
        }
      }
      if (row_bc) {
        v = (k == 0) ? 1.0 : 0.0;
      } else if (col_bc) {
        lf += v * g[j];  // F_free -= K[free,bc] g, solver.py:166-169
        v = 0.0;
      }
      if (store >= 0) vals[((i64)store * n + i) * Bv + nm.b] = v;
    }
    if (lift) lift[(i64)i * Bv + nm.b] = lf;
  }
}

// ---------------------------------------------------------------------------------------
// The same gather for FEMesh.rectangle connectivity, lists written into the code (diffhe/plan.py: build_dia_pattern):
// quad (r, c), q = r nx + c, holds T0 = [a, b, d] = element 2q and T1 = [b, c, d] = element 2q + 1; node (r, c) sees the
// six triangles A = T1(r-1,c-1), B = T0(r-1,c), C = T1(r-1,c), D = T0(r,c-1), E = T1(r,c-1), F = T0(r,c).  Same
// contributions, same element order, same fma chain as assemble_rows_kernel<false> -- bitwise the same values -- but
// no index lists to read, each kappa_e loaded once per node (six loads, wave-uniform addresses + lane = sample) instead
// of once per contribution (up to 18), local integrals as scalar loads.  One wave per node, lanes over samples.
// Seven entry kinds per row in the order (0, +1, +W, +nx, -1, -W, -nx); the first nd are stored, the others only feed
// the Dirichlet lift.
// ---------------------------------------------------------------------------------------
// The seven entries of node i's row (and its Dirichlet lift) from the kappa of its six triangles: shared by the
// node-per-wave kernel and the strip kernel below, so that both produce bitwise the same values.
__device__ __forceinline__ void lattice_node_entries(const double* __restrict__ local, i64 lm, i64 emask, double kA,
                                                     double kB, double kC, double kD, double kE, double kF, i64 eA, i64 eB,
                                                     i64 eC, i64 eD, i64 eE, i64 eF, bool up, bool dn, bool lf, bool rt,
                                                     int i, int W, int nx, i64 n, int nd,
                                                     const unsigned char* __restrict__ is_bc,
                                                     const double* __restrict__ g, double* __restrict__ vals,
                                                     double* __restrict__ lift, int Bv, int b) {
#pragma clang fp contract(off)
    const bool hA = dn && lf, hBC = dn && rt, hDE = up && lf, hF = up && rt;
    auto loc = [&](int pq, i64 e) -> double { return local[(i64)pq * lm + (e & emask)]; };
    const bool row_bc = is_bc && is_bc[i];
    double lfv = 0.0;
    // entry kinds: offsets and contribution lists (mask, element, kappa, local entry), increasing element id
#define CONTRIB(mask_, k_, pq_, e_) if (mask_) v = fma((k_), loc((pq_), (e_)), v)
#define ENTRY(kind_, off_, any_, BODY)                                                        \
    {                                                                                         \
      const int store = (kind_) < nd ? (kind_) : -1;                                          \
      const i64 j = (any_) ? (i64)i + (off_) : (i64)i;                                        \
      const bool col_bc = is_bc && j != i && is_bc[j];                                        \
      if (!(store < 0 && (row_bc || !col_bc))) {                                              \
        double v = 0.0;                                                                       \
        BODY                                                                                  \
        if (row_bc) v = ((kind_) == 0) ? 1.0 : 0.0;                                           \
        else if (col_bc) { lfv += v * g[j]; v = 0.0; }                                        \
        if (store >= 0) vals[((i64)store * n + i) * Bv + b] = v;                           \
      }                                                                                       \
    }
    ENTRY(0, 0, true, CONTRIB(hA, kA, 4, eA); CONTRIB(hBC, kB, 8, eB); CONTRIB(hBC, kC, 8, eC); CONTRIB(hDE, kD, 4, eD);
          CONTRIB(hDE, kE, 0, eE); CONTRIB(hF, kF, 0, eF);)
    ENTRY(1, 1, rt, CONTRIB(rt && dn, kC, 7, eC); CONTRIB(rt && up, kF, 1, eF);)
    ENTRY(2, W, up, CONTRIB(up && lf, kE, 1, eE); CONTRIB(up && rt, kF, 2, eF);)
    ENTRY(3, nx, up && lf, CONTRIB(up && lf, kD, 5, eD); CONTRIB(up && lf, kE, 2, eE);)
    ENTRY(4, -1, lf, CONTRIB(lf && dn, kA, 5, eA); CONTRIB(lf && up, kD, 3, eD);)
    ENTRY(5, -W, dn, CONTRIB(dn && lf, kA, 3, eA); CONTRIB(dn && rt, kB, 6, eB);)
    ENTRY(6, -nx, dn && rt, CONTRIB(dn && rt, kB, 7, eB); CONTRIB(dn && rt, kC, 6, eC);)
#undef ENTRY
#undef CONTRIB
    if (lift) lift[(i64)i * Bv + b] = lfv;
}

// `local` is (9, m), or -- compact form, emask = 1, lm = 2 -- (9, 2): one unit matrix per triangle ORIENTATION (element
// parity) of a lattice whose triangles are congruent bit for bit (FEMesh.rectangle with exactly representable spacing:
// the bench mesh).  Same values, same order; the 18 wave-uniform loads per node then hit a 144-byte table instead of a
// (9, m) array (151 MB at 1024^2, which lives in the Infinity Cache at best): 6.7 -> see DESIGN section 6, round 4.
__global__ __launch_bounds__(256) void lattice_assemble_kernel(const double* __restrict__ local, i64 lm, i64 emask,
                                                                const double* __restrict__ kappa, i64 kse, i64 ksb,
                                                                const unsigned char* __restrict__ is_bc,
                                                                const double* __restrict__ g, double* __restrict__ vals,
                                                                double* __restrict__ lift, int nx, int ny, int nd,
                                                                int Bv) {
#pragma clang fp contract(off)
  const NodeMap nm = node_map(Bv);
  if (nm.b >= Bv) return;
  const int W = nx + 1;
  const i64 n = (i64)W * (ny + 1);
  const i64 kb = (i64)nm.b * ksb;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const int r = i / W, c = i - r * W;
    const bool up = r < ny, dn = r >= 1, lf = c >= 1, rt = c < nx;
    // element ids (valid only under their masks)
    const i64 eA = 2 * ((i64)(r - 1) * nx + (c - 1)) + 1, eB = 2 * ((i64)(r - 1) * nx + c), eC = eB + 1;
    const i64 eD = 2 * ((i64)r * nx + (c - 1)), eE = eD + 1, eF = 2 * ((i64)r * nx + c);
    const bool hA = dn && lf, hBC = dn && rt, hDE = up && lf, hF = up && rt;
    const double kA = hA ? (kappa ? kappa[eA * kse + kb] : 1.0) : 0.0;
    const double kB = hBC ? (kappa ? kappa[eB * kse + kb] : 1.0) : 0.0;
    const double kC = hBC ? (kappa ? kappa[eC * kse + kb] : 1.0) : 0.0;
    const double kD = hDE ? (kappa ? kappa[eD * kse + kb] : 1.0) : 0.0;
    const double kE = hDE ? (kappa ? kappa[eE * kse + kb] : 1.0) : 0.0;
    const double kF = hF ? (kappa ? kappa[eF * kse + kb] : 1.0) : 0.0;
    lattice_node_entries(local, lm, emask, kA, kB, kC, kD, kE, kF, eA, eB, eC, eD, eE, eF, up, dn, lf, rt, i, W, nx, n, nd,
                         is_bc, g, vals, lift, Bv, nm.b);
  }
}

// The same assembly as a STRIP pass (per-sample kappa fields on big levels): a wave owns RW node columns x 64 samples
// and marches down the node rows with the kappa of two quad rows in registers -- every kappa_e is loaded once per wave
// and quad row (2 (RW + 1) loads per RW nodes) instead of once per incident node (6 per node).  Same per-node arithmetic
// (lattice_node_entries): bitwise the values of lattice_assemble_kernel.
constexpr int kAsmCols = 4;
__global__ __launch_bounds__(256) void lattice_assemble_strip_kernel(const double* __restrict__ local, i64 lm, i64 emask,
                                                                      const double* __restrict__ kappa, i64 kse, i64 ksb,
                                                                      const unsigned char* __restrict__ is_bc,
                                                                      const double* __restrict__ g,
                                                                      double* __restrict__ vals, double* __restrict__ lift,
                                                                      int nx, int ny, int nd, int Bv, int ncb, int TR) {
  constexpr int RW = kAsmCols;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y * kWave + lane;
  const int rc = blockIdx.x / ncb, cb = blockIdx.x - rc * ncb;
  const int c0 = (cb * 4 + wave) * RW;              // first node column
  const int r0 = rc * TR;
  const int r1 = (r0 + TR < ny + 1) ? r0 + TR : ny + 1;
  if (c0 > nx || r0 >= r1) return;
  const int W = nx + 1;
  const i64 n = (i64)W * (ny + 1);
  const i64 kb = (i64)b * ksb;
  // kappa of quad row qr on the quad columns c0 - 1 + j, both triangles; 0 outside the grid (never used there: masks)
  double lo[RW + 1][2], hi[RW + 1][2];
  auto load_quads = [&](int qr, double (*dst)[2]) {
#pragma unroll
    for (int j = 0; j < RW + 1; ++j) {
      const int qc = c0 - 1 + j;
      const bool ok = qr >= 0 && qr < ny && qc >= 0 && qc < nx;
      const i64 e = 2 * ((i64)qr * nx + qc);
      dst[j][0] = ok ? kappa[e * kse + kb] : 0.0;
      dst[j][1] = ok ? kappa[(e + 1) * kse + kb] : 0.0;
    }
  };
  load_quads(r0 - 1, lo);
  for (int r = r0; r < r1; ++r) {
    load_quads(r, hi);
    const bool up = r < ny, dn = r >= 1;
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      const int c = c0 + k;
      if (c > nx) continue;
      const bool lf = c >= 1, rt = c < nx;
      const i64 eA = 2 * ((i64)(r - 1) * nx + (c - 1)) + 1, eB = 2 * ((i64)(r - 1) * nx + c), eC = eB + 1;
      const i64 eD = 2 * ((i64)r * nx + (c - 1)), eE = eD + 1, eF = 2 * ((i64)r * nx + c);
      // node (r, c): A = T1(r-1, c-1), B = T0(r-1, c), C = T1(r-1, c), D = T0(r, c-1), E = T1(r, c-1), F = T0(r, c)
      lattice_node_entries(local, lm, emask, lo[k][1], lo[k + 1][0], lo[k + 1][1], hi[k][0], hi[k][1], hi[k + 1][0], eA, eB,
                           eC, eD, eE, eF, up, dn, lf, rt, r * W + c, W, nx, n, nd, is_bc, g, vals, lift, Bv, b);
    }
#pragma unroll
    for (int j = 0; j < RW + 1; ++j) { lo[j][0] = hi[j][0]; lo[j][1] = hi[j][1]; }
  }
}

// ---------------------------------------------------------------------------------------
// Element-parallel assembly with fp64 atomics; element integrals staged in LDS
// ---------------------------------------------------------------------------------------
constexpr int kElemTile = 64;

// NPE: the largest element the instance handles (3: intervals and triangles; 4: tetrahedra, whose pruned stiffness
// pattern has no slot for a structurally zero coupling: slot_of < 0, skipped)
template <int NPE>
__global__ __launch_bounds__(256) void assemble_atomic_kernel(const double* __restrict__ coords,
                                                               const int* __restrict__ elems, int dim,
                                                               const double* __restrict__ kappa, i64 kse, i64 ksb,
                                                               const int* __restrict__ slot_of,
                                                               double* __restrict__ vals, int n, int m, int Bp) {
  __shared__ double k0s[NPE * NPE][kElemTile];
  __shared__ int rows[NPE][kElemTile];
  const int npe = dim + 1, nloc = npe * npe;
  const int LB = Bp < kWave ? Bp : kWave;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y * kWave + (lane % LB);
  const int sub = lane / LB, nsub = kWave / LB;
  for (i64 base = (i64)blockIdx.x * kElemTile; base < m; base += (i64)gridDim.x * kElemTile) {
    __syncthreads();
    if (threadIdx.x < kElemTile && base + threadIdx.x < m) {
      const i64 e = base + threadIdx.x;
      const int t = threadIdx.x;
      if (dim == 1) {
        const int i = elems[e], j = elems[(i64)m + e];
        const double k = 1.0 / (coords[j] - coords[i]);
        k0s[0][t] = k; k0s[1][t] = -k; k0s[2][t] = -k; k0s[3][t] = k;
        rows[0][t] = i; rows[1][t] = j;
      } else if (NPE == 4 && dim == 3) {
        double loc[16], vol;
        int v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = elems[(i64)p * m + e];
        tet_integrals(coords, n, v[0], v[1], v[2], v[3], loc, &vol);
#pragma unroll
        for (int pq = 0; pq < 16; ++pq) k0s[pq % (NPE * NPE)][t] = loc[pq];
#pragma unroll
        for (int p = 0; p < 4; ++p) rows[p % NPE][t] = v[p];
      } else {
        const int i = elems[e], j = elems[(i64)m + e], k = elems[2 * (i64)m + e];
        double loc[9], area;
        tri_integrals(coords[i], coords[(i64)n + i], coords[j], coords[(i64)n + j], coords[k], coords[(i64)n + k],
                      loc, &area);
#pragma unroll
        for (int pq = 0; pq < 9; ++pq) k0s[pq][t] = loc[pq];
        rows[0][t] = i; rows[1][t] = j; rows[2][t] = k;
      }
    }
    __syncthreads();
    if (b >= Bp) continue;
    for (int el = wave * nsub + sub; el < kElemTile && base + el < m; el += 4 * nsub) {
      const i64 e = base + el;
      const double kap = kappa ? kappa[e * kse + (i64)b * ksb] : 1.0;
      for (int pq = 0; pq < nloc; ++pq) {
        const int slot = slot_of[(i64)pq * m + e];
        if (NPE == 4 && slot < 0) continue;
        const int row = rows[pq / npe][el];
        unsafeAtomicAdd(&vals[((i64)slot * n + row) * Bp + b], kap * k0s[pq][el]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void apply_dirichlet_kernel(const int* __restrict__ cols,
                                                               const unsigned char* __restrict__ is_bc,
                                                               const double* __restrict__ g, double* __restrict__ vals,
                                                               double* __restrict__ F, int n, int W, int Bp) {
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const bool row_bc = is_bc[i];
    double lf = 0.0;
    for (int k = 0; k < W; ++k) {
      const i64 ent = (i64)k * n + i;
      const int j = cols[ent];
      if (row_bc) {
        vals[ent * Bp + nm.b] = (k == 0) ? 1.0 : 0.0;
      } else if (j != i && is_bc[j]) {
        lf += vals[ent * Bp + nm.b] * g[j];
        vals[ent * Bp + nm.b] = 0.0;
      }
    }
    if (F) F[(i64)i * Bp + nm.b] = row_bc ? 0.0 : F[(i64)i * Bp + nm.b] - lf;
  }
}

// ---------------------------------------------------------------------------------------
// y = (is_bc ? 0 : M x - sub), M batch-shared ELL.  Load vector and df = M^T lambda.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 8) void spmv_shared_kernel(const double* __restrict__ vals,
                                                           const int* __restrict__ cols, const double* __restrict__ x,
                                                           const double* __restrict__ sub, int sub_B,
                                                           const double* __restrict__ sub_scale,
                                                           const unsigned char* __restrict__ is_bc,
                                                           double* __restrict__ y, int n, int W, int Bp) {
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  FOR_EACH_NODE(nm, n, Bp, 1, {
    double acc = ell_row<false, kUni, kShared>(0.0, vals, cols, x, i, n, W, Bp, 1, nm.b);
    if (sub) acc -= (sub_scale ? sub_scale[nm.b] : 1.0) * sub[(i64)i * sub_B + (sub_B == 1 ? 0 : nm.b)];
    if (is_bc && is_bc[i]) acc = 0.0;
    y[(i64)i * Bp + nm.b] = acc;
  });
}

// ---------------------------------------------------------------------------------------
// dL/dkappa contraction
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_kappa_kernel(const int* __restrict__ elems, const double* __restrict__ k0,
                                                          const double* __restrict__ lam, const double* __restrict__ u,
                                                          const double* __restrict__ g, int npe, int m, int Bp,
                                                          double* __restrict__ dk_e,
                                                          double* __restrict__ dk_part) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);  // "nodes" are elements here
  const bool ok = nm.b < Bp;
  double s = 0.0;
  if (ok)
    for (int e = nm.node0; e < m; e += nm.stride) {
      double le[6], ue[6];   // npe <= 6 (P2 triangles)
      for (int p = 0; p < npe; ++p) {
        const int node = elems[(i64)p * m + e];
        const i64 o = (i64)node * Bp + nm.b;
        le[p] = lam[o];
        ue[p] = u[o] + (g ? g[node] : 0.0);  // full u: Dirichlet values included (Appendix A step 2)
      }
      double acc = 0.0;
      for (int p = 0; p < npe; ++p)
        for (int q = 0; q < npe; ++q) acc += le[p] * k0[(i64)(p * npe + q) * m + e] * ue[q];
      const double dk = -acc;
      if (dk_e) dk_e[(i64)e * Bp + nm.b] = dk;
      s += dk;
    }
  store_block_partial(s, dk_part, Bp, nm.b, ok, lds);
}

// The same contraction summed over the batch, for a kappa field SHARED by all samples (kappa (m,)): the batch-shared
// kernel of element_grad.h with this form, dk[e, b] = -lam_e^T k0_e u_e.  npe is a runtime 2, 3, 4 or 6, so nothing indexed
// by it is carried across the call: eval reads the element's nodes and k0 itself -- wave-uniform loads there -- and no array
// spills to scratch.  (The per-sample kernel above stays as it is: on the header's element loop it measured 1 % slower
// at Bp = 256.)
struct KappaForm {
  static constexpr int NC = 1;
  const int* __restrict__ elems;
  const double* __restrict__ k0;
  const double* __restrict__ lam;
  const double* __restrict__ u;
  const double* __restrict__ g;
  int npe, m;

  struct Elem {
    int e;
  };

  __device__ __forceinline__ void load(int e, Elem& el) const { el.e = e; }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* dk) const {
    const int e = el.e;
    double le[6], ue[6];   // npe <= 6 (P2 triangles)
    for (int p = 0; p < npe; ++p) {
      const int node = elems[(i64)p * m + e];
      const i64 o = (i64)node * Bp + b;
      le[p] = lam[o];
      ue[p] = u[o] + (g ? g[node] : 0.0);  // full u: Dirichlet values included (Appendix A step 2)
    }
    double acc = 0.0;
    for (int p = 0; p < npe; ++p)
      for (int q = 0; q < npe; ++q) acc += le[p] * k0[(i64)(p * npe + q) * m + e] * ue[q];
    dk[0] = -acc;
  }
};

__global__ __launch_bounds__(256) void sum_partials_kernel(const double* __restrict__ part, int nblk, int Bp,
                                                            double* __restrict__ out) {
  __shared__ double lds[4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kWave + lane;
  const double a = sum_partials(part, nblk, Bp, b, lds);
  if (wave == 0 && b < Bp) out[b] = a;
}

// ---------------------------------------------------------------------------------------
// (B, n) <-> (n, Bp) through a padded LDS tile
// ---------------------------------------------------------------------------------------
constexpr int kT = 64;

__global__ __launch_bounds__(256) void to_node_major_kernel(const double* __restrict__ src, i64 ld,
                                                             const unsigned char* __restrict__ zero_mask,
                                                             double* __restrict__ dst, int n, int B, int Bp) {
  __shared__ double tile[kT][kT + 1];
  const int i0 = blockIdx.x * kT, b0 = blockIdx.y * kT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the 16 rows of a wave are loaded into registers first (16 loads in flight; a load-store loop had one), then staged
  double v[kT / 4];
#pragma unroll
  for (int k = 0; k < kT / 4; ++k) {  // lanes along i: coalesced reads of a sample row
    const int b = b0 + wave + 4 * k, i = i0 + lane;
    v[k] = (b < B && i < n) ? src[(i64)b * ld + i] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < kT / 4; ++k) tile[wave + 4 * k][lane] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kT / 4; ++k) {  // lanes along b: coalesced writes of a node row
    const int ii = wave + 4 * k;
    const int i = i0 + ii, b = b0 + lane;
    if (i < n && b < Bp) {
      double w = tile[lane][ii];
      if (zero_mask && zero_mask[i]) w = 0.0;
      dst[(i64)i * Bp + b] = w;
    }
  }
}

__global__ __launch_bounds__(256) void to_sample_major_kernel(const double* __restrict__ src,
                                                               const double* __restrict__ add, double* __restrict__ dst,
                                                               i64 ld, int n, int B, int Bp) {
  __shared__ double tile[kT][kT + 1];
  const int i0 = blockIdx.x * kT, b0 = blockIdx.y * kT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double v[kT / 4];
#pragma unroll
  for (int k = 0; k < kT / 4; ++k) {   // 16 node rows per wave, all requested before the first is staged
    const int i = i0 + wave + 4 * k, b = b0 + lane;
    v[k] = (i < n && b < Bp) ? src[(i64)i * Bp + b] + (add ? add[i] : 0.0) : 0.0;
  }
#pragma unroll
  for (int k = 0; k < kT / 4; ++k) tile[wave + 4 * k][lane] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kT / 4; ++k) {
    const int bb = wave + 4 * k;
    const int b = b0 + bb, i = i0 + lane;
    if (b < B && i < n) dst[(i64)b * ld + i] = tile[lane][bb];
  }
}

// ---------------------------------------------------------------------------------------
// Aggregation multigrid for the general path (diffhe/amg.py builds the batch-shared hierarchy)
// ---------------------------------------------------------------------------------------
// coarse values = P^T A P (per sample) from gather lists: plain sums of fine entries for piecewise-constant P
// (weights == NULL), weighted sums w_c = P_iI P_jJ for a smoothed P.  The lists and weights are batch-shared
// (wave-uniform loads), the fine values arrive as one contiguous row of samples per contribution.
__global__ __launch_bounds__(256) void ell_galerkin_kernel(const double* __restrict__ vals_f,
                                                            const int* __restrict__ ent_ptr,
                                                            const int* __restrict__ contrib,
                                                            const double* __restrict__ weights,
                                                            double* __restrict__ vals_c, int nc, int Wc, int Bv) {
  const NodeMap nm = node_map(Bv);
  if (nm.b >= Bv) return;
  for (int I = nm.node0; I < nc; I += nm.stride)
    for (int k = 0; k < Wc; ++k) {
      const i64 ent = (i64)k * nc + I;
      double v = 0.0;
      if (weights)
        for (int c = ent_ptr[ent]; c < ent_ptr[ent + 1]; ++c) v = fma(weights[c], vals_f[(i64)contrib[c] * Bv + nm.b], v);
      else
        for (int c = ent_ptr[ent]; c < ent_ptr[ent + 1]; ++c) v += vals_f[(i64)contrib[c] * Bv + nm.b];
      vals_c[ent * Bv + nm.b] = v;
    }
}
}  // namespace

extern "C" int diffhe_p1_element_integrals(const double* coords, const int* elems, int dim, int n, int m,
                                           double* k0, double* m0, void* stream) {
  if (!coords || !elems || !k0 || !m0 || dim < 1 || dim > 3 || n < 1 || m < 1) return DIFFHE_E_BADARG;
  int blocks = (m + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(element_integrals_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, coords, elems, dim, n,
                     m, k0, m0);
  return diffhe::check_launch();
}

extern "C" int diffhe_ell_assemble_rows(const double* local, const double* kappa, long long kappa_se,
                                        long long kappa_sb, const int* ent_ptr, const int* contrib, const int* cols,
                                        const int* store_slot, const unsigned char* is_bc, const double* g,
                                        double* vals, double* lift, int n, int m, int W, int Bv, void* stream) {
  if (!local || !ent_ptr || !contrib || !cols || !vals || n < 1 || m < 1 || W < 1) return DIFFHE_E_BADARG;
  if (is_bc && !g) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  diffhe::account(8.0 * Bv * ((double)W * n + (lift ? n : 0) + ((kappa && kappa_se) ? m : 0)));  // stored values, lift, kappa field
  hipLaunchKernelGGL(assemble_rows_kernel<false>, diffhe::node_grid(n, Bv), dim3(256), 0, (hipStream_t)stream, local,
                     (const double*)nullptr, kappa, kappa_se, kappa_sb, ent_ptr, contrib, cols, store_slot, is_bc, g,
                     vals, lift, n, m, W, Bv);
  return diffhe::check_launch();
}

extern "C" int diffhe_lattice_assemble_rows(const double* local, int local_compact, const double* kappa,
                                            long long kappa_se, long long kappa_sb, const unsigned char* is_bc,
                                            const double* g, double* vals, double* lift, int nx, int ny, int nd, int Bv,
                                            void* stream) {
  if (!local || !vals || nx < 1 || ny < 1 || nd < 3 || nd > 4) return DIFFHE_E_BADARG;
  if (is_bc && !g) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  const long long n = (long long)(nx + 1) * (ny + 1), m = 2LL * nx * ny;
  if (n > 2147483647LL) return DIFFHE_E_BADARG;
  diffhe::account(8.0 * Bv * ((double)nd * n + (lift ? n : 0) + ((kappa && kappa_se) ? m : 0)));
  const int strip_on = getenv("DIFFHE_ASM_STRIP") ? atoi(getenv("DIFFHE_ASM_STRIP")) : 1;
  if (strip_on && kappa && kappa_se && Bv >= kWave && Bv % kWave == 0 && nx >= 128 && ny >= 64) {
    // per-sample kappa fields on a strip-sized level: every kappa_e loaded once per wave and quad row
    constexpr int TR = 8;   // lattice rows per tile
    const int ncb = (nx + 1 + 4 * kAsmCols - 1) / (4 * kAsmCols), nrc = (ny + 1 + TR - 1) / TR;
    hipLaunchKernelGGL(lattice_assemble_strip_kernel, dim3(ncb * nrc, Bv / kWave), dim3(256), 0, (hipStream_t)stream, local,
                       (i64)(local_compact ? 2 : m), (i64)(local_compact ? 1 : -1), kappa, (i64)kappa_se, (i64)kappa_sb,
                       is_bc, g, vals, lift, nx, ny, nd, Bv, ncb, TR);
    return diffhe::check_launch();
  }
  hipLaunchKernelGGL(lattice_assemble_kernel, diffhe::node_grid((int)n, Bv), dim3(256), 0, (hipStream_t)stream, local,
                     (i64)(local_compact ? 2 : m), (i64)(local_compact ? 1 : -1), kappa, kappa_se, kappa_sb, is_bc, g, vals,
                     lift, nx, ny, nd, Bv);
  return diffhe::check_launch();
}

extern "C" int diffhe_ell_assemble_rows_ref(const double* tnum, const double* den, const double* kappa,
                                            long long kappa_se, long long kappa_sb, const int* ent_ptr,
                                            const int* contrib, const int* cols, const int* store_slot,
                                            const unsigned char* is_bc, const double* g, double* vals, double* lift,
                                            int n, int m, int W, int Bv, void* stream) {
  if (!tnum || !den || !ent_ptr || !contrib || !cols || !vals || n < 1 || m < 1 || W < 1) return DIFFHE_E_BADARG;
  if (is_bc && !g) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  diffhe::account(8.0 * Bv * ((double)W * n + (lift ? n : 0) + ((kappa && kappa_se) ? m : 0)));
  hipLaunchKernelGGL(assemble_rows_kernel<true>, diffhe::node_grid(n, Bv), dim3(256), 0, (hipStream_t)stream, tnum, den,
                     kappa, kappa_se, kappa_sb, ent_ptr, contrib, cols, store_slot, is_bc, g, vals, lift, n, m, W, Bv);
  return diffhe::check_launch();
}

extern "C" int diffhe_ell_assemble_atomic(const double* coords, const int* elems, int dim, const double* kappa,
                                          long long kappa_se, long long kappa_sb, const int* slot_of, double* vals,
                                          int n, int m, int W, int Bp, void* stream) {
  (void)W;
  if (!coords || !elems || !slot_of || !vals || dim < 1 || dim > 3 || n < 1 || m < 1) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  int gx = (m + kElemTile - 1) / kElemTile;
  if (gx > 4096) gx = 4096;
  dim3 grid(gx, (Bp + 63) / 64);
  if (dim == 3)
    hipLaunchKernelGGL(assemble_atomic_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, coords, elems, dim, kappa,
                       kappa_se, kappa_sb, slot_of, vals, n, m, Bp);
  else
    hipLaunchKernelGGL(assemble_atomic_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, coords, elems, dim, kappa,
                       kappa_se, kappa_sb, slot_of, vals, n, m, Bp);
  return diffhe::check_launch();
}

extern "C" int diffhe_ell_apply_dirichlet(const int* cols, const unsigned char* is_bc, const double* g, double* vals,
                                          double* F, int n, int W, int Bp, void* stream) {
  if (!cols || !is_bc || !g || !vals || n < 1 || W < 1) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  hipLaunchKernelGGL(apply_dirichlet_kernel, diffhe::node_grid(n, Bp), dim3(256), 0, (hipStream_t)stream, cols, is_bc,
                     g, vals, F, n, W, Bp);
  return diffhe::check_launch();
}

extern "C" int diffhe_ell_spmv_shared(const double* vals, const int* cols, const double* x, const double* sub,
                                      int sub_B, const double* sub_scale, const unsigned char* is_bc, double* y,
                                      int n, int W, int Bp, void* stream) {
  if (!vals || !cols || !x || !y || n < 1 || W < 1) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  if (sub && sub_B != 1 && sub_B != Bp) return DIFFHE_E_BADARG;
  diffhe::account(16.0 * n * Bp);
  hipLaunchKernelGGL(spmv_shared_kernel, diffhe::node_grid(n, Bp), dim3(256), 0, (hipStream_t)stream, vals, cols, x,
                     sub, sub_B, sub_scale, is_bc, y, n, W, Bp);
  return diffhe::check_launch();
}

extern "C" int diffhe_ell_galerkin(const double* vals_fine, const int* ent_ptr, const int* contrib, const double* weights,
                                   double* vals_coarse, int n_coarse, int W_coarse, int Bv, void* stream) {
  if (!vals_fine || !ent_ptr || !contrib || !vals_coarse || n_coarse < 1 || W_coarse < 1) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  diffhe::account(8.0 * Bv * (double)n_coarse * W_coarse);   // the coarse values written; fine values re-read from cache
  hipLaunchKernelGGL(ell_galerkin_kernel, diffhe::node_grid(n_coarse, Bv), dim3(256), 0, (hipStream_t)stream, vals_fine,
                     ent_ptr, contrib, weights, vals_coarse, n_coarse, W_coarse, Bv);
  return diffhe::check_launch();
}

extern "C" int diffhe_grad_kappa_blocks(int m, int Bp) { return (int)diffhe::node_grid(m, Bp).x; }

extern "C" int diffhe_p1_grad_kappa(const int* elems, const double* k0, const double* lam, const double* u,
                                    const double* g, int npe, int m, int Bp, double* dk_e, double* dk_part,
                                    double* dk_sum, void* stream) {
  if (!elems || !k0 || !lam || !u || !dk_part || !dk_sum || (npe != 2 && npe != 3 && npe != 4 && npe != 6) || m < 1) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const dim3 grid = diffhe::node_grid(m, Bp);
  diffhe::account(8.0 * Bp * (2.0 * m * (npe == 3 ? 0.5 : 1.0) + (dk_e ? m : 0)));  // lambda and u once per node, dk per element
  hipLaunchKernelGGL(grad_kappa_kernel, grid, dim3(256), 0, (hipStream_t)stream, elems, k0, lam, u, g, npe, m, Bp,
                     dk_e, dk_part);
  hipLaunchKernelGGL(sum_partials_kernel, dim3((Bp + 63) / 64), dim3(256), 0, (hipStream_t)stream,
                     (const double*)dk_part, (int)grid.x, Bp, dk_sum);
  return diffhe::check_launch();
}

extern "C" int diffhe_p1_grad_kappa_shared(const int* elems, const double* k0, const double* lam, const double* u,
                                           const double* g, int npe, int m, int B, int Bp, double* dk, void* stream) {
  if (!elems || !k0 || !lam || !u || !dk || (npe != 2 && npe != 3 && npe != 4 && npe != 6) || m < 1 || B < 1 || B > Bp) return DIFFHE_E_BADARG;
  // lambda and u once per node, dk once per element
  const double bytes = 8.0 * (Bp * 2.0 * m * (npe == 3 ? 0.5 : 1.0) + m);
  return diffhe::launch_element_grad_shared(KappaForm{elems, k0, lam, u, g, npe, m}, m, B, Bp, dk, 0, 1, bytes, stream);
}

extern "C" int diffhe_to_node_major(const double* src, long long ld, const unsigned char* zero_mask, double* dst, int n,
                                    int B, int Bp, void* stream) {
  if (!src || !dst || n < 1 || B < 1 || Bp < B) return DIFFHE_E_BADARG;
  dim3 grid((n + kT - 1) / kT, (Bp + kT - 1) / kT);
  diffhe::account(8.0 * n * ((ld ? (double)B : 1.0) + Bp));
  hipLaunchKernelGGL(to_node_major_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, ld, zero_mask, dst, n, B, Bp);
  return diffhe::check_launch();
}

extern "C" int diffhe_to_sample_major(const double* src, const double* add, double* dst, long long ld, int n, int B,
                                      int Bp, void* stream) {
  if (!src || !dst || n < 1 || B < 1 || Bp < B) return DIFFHE_E_BADARG;
  dim3 grid((n + kT - 1) / kT, (Bp + kT - 1) / kT);
  diffhe::account(8.0 * n * ((double)B + Bp));
  hipLaunchKernelGGL(to_sample_major_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, add, dst, ld, n, B, Bp);
  return diffhe::check_launch();
}
