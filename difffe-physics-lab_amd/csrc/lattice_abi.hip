// C-ABI entries of the lattice path that stand apart from the solver: apply_shared, grad_kappa, pack_h16, max_diag and
// restrict_kappa, with the kernels only they use.
#include "lattice.h"

using namespace diffhe_lattice;

namespace {
// per-element kappa of the coarse triangulation.  Full coarsening (sx = sy = 2): mean of the 4 children
// (Galerkin for nested P1).  Semi-coarsening: both coarse triangles of a cell take the mean of the 4 fine
// triangles of the 2 fine cells it covers.
__global__ __launch_bounds__(256) void mg_restrict_kappa_kernel(const double* __restrict__ kf, double* __restrict__ kc,
                                                                 int nxc, int nyc, int sx, int sy, int Bv) {
  const NodeMap nm = node_map(Bv);
  const int mc = 2 * nxc * nyc, nxf = sx * nxc;
  for (int E = nm.node0; E < mc; E += nm.stride) {
    const int q = E >> 1, up = E & 1;
    const int I = q / nxc, J = q - I * nxc;
    // fine element id = 2*(row*nxf + col) + upper
    auto fe = [&](int r, int c, int u) { return (i64)(2 * ((i64)r * nxf + c) + u) * Bv + nm.b; };
    double s;
    if (sx == 2 && sy == 2) {
      if (!up)
        s = kf[fe(2 * I, 2 * J, 0)] + kf[fe(2 * I, 2 * J, 1)] + kf[fe(2 * I, 2 * J + 1, 0)] + kf[fe(2 * I + 1, 2 * J, 0)];
      else
        s = kf[fe(2 * I + 1, 2 * J + 1, 1)] + kf[fe(2 * I + 1, 2 * J + 1, 0)] + kf[fe(2 * I, 2 * J + 1, 1)] +
            kf[fe(2 * I + 1, 2 * J, 1)];
    } else if (sx == 2) {
      s = kf[fe(I, 2 * J, 0)] + kf[fe(I, 2 * J, 1)] + kf[fe(I, 2 * J + 1, 0)] + kf[fe(I, 2 * J + 1, 1)];
    } else {
      s = kf[fe(2 * I, J, 0)] + kf[fe(2 * I, J, 1)] + kf[fe(2 * I + 1, J, 0)] + kf[fe(2 * I + 1, J, 1)];
    }
    kc[(i64)E * Bv + nm.b] = 0.25 * s;
  }
}
}  // namespace

namespace {
// y = is_bc ? 0 : (M x - sub_scale[b] * sub) for a batch-shared symmetric-diagonal matrix M (the load
// matrix of a lattice mesh): F = M f - lift and df = M^T lambda without the general ELL pattern.
__global__ __launch_bounds__(256) void dia_shared_apply_kernel(Level L, const double* __restrict__ x,
                                                                const double* __restrict__ sub, int sub_B,
                                                                const double* __restrict__ sub_scale,
                                                                const unsigned char* __restrict__ mask,
                                                                double* __restrict__ y, int Bp) {
  const NodeMap nm = node_map(Bp);
  for (int i = nm.node0; i < L.n; i += nm.stride) {
    double acc = dia_row(L, 1, 0, x, i, nm.b, Bp);
    if (sub) acc -= (sub_scale ? sub_scale[nm.b] : 1.0) * sub[(i64)i * sub_B + (sub_B == 1 ? 0 : nm.b)];
    if (mask && mask[i]) acc = 0.0;
    y[(i64)i * Bp + nm.b] = acc;
  }
}
}  // namespace

extern "C" int diffhe_lattice_apply_shared(int nx, int ny, int nd, const double* vals, const double* x,
                                           const double* sub, int sub_B, const double* sub_scale,
                                           const unsigned char* mask, double* y, int Bp, void* stream) {
  if (!vals || !x || !y || nx < 2 || ny < 2 || (nd != 3 && nd != 4)) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  if (sub && sub_B != 1 && sub_B != Bp) return DIFFHE_E_BADARG;
  Level L{};   // inv, shift: none
  L.nx = nx; L.ny = ny; L.W = nx + 1; L.n = (nx + 1) * (ny + 1); L.nd = nd; L.v = vals; L.v32 = nullptr; L.bc = nullptr;
  L.rd32 = nullptr; L.mk32 = nullptr; L.o16 = nullptr; L.osc = nullptr;
  const StripGeom g = strip_geom(L, Bp);
  if (g.use) {
    Extra ex{};
    ex.sub = sub; ex.sub_scale = sub_scale; ex.mask = mask;
    ex.sub_pb = (sub && sub_B != 1) ? 1 : 0;   // per-sample lift: read in the strip pass too (it used to fall to the
                                               // gather kernel below: 2.67 instead of ~1.4 ms at 1024^2 x 256)
    if (ex.sub_pb) diffhe::account(8.0 * (double)L.n * Bp);
    launch_strip<double, M_APPLY, false>(L, 1, nullptr, x, (const double*)nullptr, y, 0.0, 0.0, nullptr, Bp, g,
                                         (hipStream_t)stream, ex);
    return diffhe::check_launch();
  }
  diffhe::account((16.0 + (sub && sub_B != 1 ? 8.0 : 0.0)) * (double)L.n * Bp);
  hipLaunchKernelGGL(dia_shared_apply_kernel, lgrid(L.n, Bp), dim3(256), 0, (hipStream_t)stream, L, x, sub, sub_B,
                     sub_scale, mask, y, Bp);
  return diffhe::check_launch();
}

// dL/dkappa per element and sample on a lattice mesh (reverse of solver.py:137-140; Appendix A step 2):
//   dk[e, b] = - sum_{p,q} lambda[node_p, b] k0[p*3+q, e] (u[node_q, b] + g[node_q])
// Quad (r, c) = nodes a (r, c), b (r, c+1), c (r+1, c+1), d (r+1, c) carries T0 = [a, b, d] = element 2q and
// T1 = [b, c, d] = element 2q + 1 (mesh.py:100-105).  A wave owns GW quad columns x 64 samples and marches down the quad
// rows with a two-row window of lambda and u in registers: every nodal value is loaded once per wave (+ one halo
// column) instead of once per incident element (6x), k0 arrives as scalar loads, dk leaves as 512 B rows.
// 32 B per node and sample of algorithmic traffic (lambda, u, two dk): the element-loop kernel ran it at 1.2 TB/s.
constexpr int kGradCols = 4;
__global__ __launch_bounds__(256) void lattice_grad_kappa_kernel(int nx, int ny, const double* __restrict__ k0, i64 lm,
                                                                  i64 emask, const double* __restrict__ lam,
                                                                  const double* __restrict__ u,
                                                                  const double* __restrict__ g, double* __restrict__ dk,
                                                                  int Bp, int ncb, int TR) {
  constexpr int GW = kGradCols;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lb = blockIdx.y * kWave + lane;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int rc = tile / ncb, cb = tile - rc * ncb;
  const int c0 = (cb * 4 + wave) * GW;                 // first quad column
  const int r0 = rc * TR;
  const int r1 = (r0 + TR < ny) ? r0 + TR : ny;        // quad rows r0 .. r1 - 1
  if (c0 >= nx || r0 >= r1) return;
  const int W = nx + 1;
  int dc[GW + 1];                                       // node columns c0 .. c0 + GW, clamped at the right edge
#pragma unroll
  for (int j = 0; j < GW + 1; ++j) dc[j] = (c0 + j < W) ? j : W - 1 - c0;
  double la[GW + 1], ua[GW + 1], lbn[GW + 1], ubn[GW + 1];   // node rows r (a, b) and r + 1 (d, c)
  const double* __restrict__ pl = lam + ((i64)r0 * W + c0) * Bp;
  const double* __restrict__ pu = u + ((i64)r0 * W + c0) * Bp;
  const double* __restrict__ pg = g ? g + (i64)r0 * W + c0 : nullptr;
  const i64 rowX = (i64)W * Bp;
#pragma unroll
  for (int j = 0; j < GW + 1; ++j) {
    la[j] = (pl + (i64)dc[j] * Bp)[lb];
    ua[j] = (pu + (i64)dc[j] * Bp)[lb] + (pg ? pg[dc[j]] : 0.0);
  }
  for (int r = r0; r < r1; ++r) {
#pragma unroll
    for (int j = 0; j < GW + 1; ++j) {
      lbn[j] = (pl + rowX + (i64)dc[j] * Bp)[lb];
      ubn[j] = (pu + rowX + (i64)dc[j] * Bp)[lb] + (pg ? pg[W + dc[j]] : 0.0);
    }
    const i64 e0 = 2 * ((i64)r * nx + c0);               // element 2 q of quad (r, c0)
#pragma unroll
    for (int j = 0; j < GW; ++j) {
      if (c0 + j >= nx) continue;
      const i64 e = e0 + 2 * j;
      // T0 = [a, b, d]: a = (r, c), b = (r, c + 1), d = (r + 1, c)
      {
        const double lp[3] = {la[j], la[j + 1], lbn[j]}, uq[3] = {ua[j], ua[j + 1], ubn[j]};
        double acc = 0.0;
#pragma unroll
        for (int p_ = 0; p_ < 3; ++p_)
#pragma unroll
          for (int q = 0; q < 3; ++q) acc += lp[p_] * k0[(i64)(p_ * 3 + q) * lm + (e & emask)] * uq[q];
        (dk + e * Bp)[lb] = -acc;
      }
      // T1 = [b, c, d]: b = (r, c + 1), c = (r + 1, c + 1), d = (r + 1, c)
      {
        const double lp[3] = {la[j + 1], lbn[j + 1], lbn[j]}, uq[3] = {ua[j + 1], ubn[j + 1], ubn[j]};
        double acc = 0.0;
#pragma unroll
        for (int p_ = 0; p_ < 3; ++p_)
#pragma unroll
          for (int q = 0; q < 3; ++q) acc += lp[p_] * k0[(i64)(p_ * 3 + q) * lm + ((e + 1) & emask)] * uq[q];
        (dk + (e + 1) * Bp)[lb] = -acc;
      }
    }
#pragma unroll
    for (int j = 0; j < GW + 1; ++j) {
      la[j] = lbn[j];
      ua[j] = ubn[j];
    }
    pl += rowX;
    pu += rowX;
    if (pg) pg += W;
  }
}

extern "C" int diffhe_lattice_grad_kappa(int nx, int ny, const double* k0, int k0_compact, const double* lam,
                                         const double* u, const double* g, double* dk, int Bp, void* stream) {
  if (!k0 || !lam || !u || !dk || nx < 2 || ny < 2) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  if (Bp < kWave) return DIFFHE_E_TOOBIG;              // small batches: diffhe_p1_grad_kappa
  const int ncb = (nx + 4 * kGradCols - 1) / (4 * kGradCols);
  const int gy = Bp / kWave;
  int nrc = (kStripBlocks + ncb * gy - 1) / (ncb * gy);
  if (nrc > ny / 8) nrc = ny / 8;
  if (nrc < 1) nrc = 1;
  const int TR = (ny + nrc - 1) / nrc;
  nrc = (ny + TR - 1) / TR;
  diffhe::account(32.0 * (double)(nx + 1) * (ny + 1) * Bp);   // lambda, u once per node; two dk per node
  const i64 mm = 2LL * nx * ny;
  hipLaunchKernelGGL(lattice_grad_kappa_kernel, dim3(ncb * nrc, gy), dim3(256), 0, (hipStream_t)stream, nx, ny, k0,
                     (i64)(k0_compact ? 2 : mm), (i64)(k0_compact ? 1 : -1), lam, u, g, dk, Bp, ncb, TR);
  return diffhe::check_launch();
}

namespace {
// fp32 diagonal + fp16 off-diagonals of a per-sample symmetric-diagonal matrix (h16m above): the off-diagonals of sample b
// divided by `oscale[b]` and rounded to fp16, the diagonal moved by the sum of the rounding differences of the row's
// 2 (nd - 1) couplings so that the row sum is the fp64 matrix's (to the fp32 rounding of the diagonal itself, 6e-8
// relative).  flags[0] is set when a non-zero coupling falls below 2^-19 of its sample's scale: fp16 subnormals keep fewer
// than 5 bits there (and flush to 0 from 2^-25 on: the row-sum rule would then leave a row with a vanishing diagonal), so
// the caller must not use the packed copies of that matrix (high contrast INSIDE a sample; the fp32 copies have no such limit).
__global__ __launch_bounds__(256) void dia_pack_h16_kernel(Level L, int Bv, const double* __restrict__ oscale,
                                                            float* __restrict__ d32, _Float16* __restrict__ o16,
                                                            int* __restrict__ flags) {
  const NodeMap nm = node_map(Bv);
  if (nm.b >= Bv) return;
  const i64 n = L.n;
  const double osc = oscale[nm.b];
  const double inv = 1.0 / osc;   // power of two: exact
  const double tiny = 1.9073486328125e-06;   // 2^-19
  bool under = false;
  for (int i = nm.node0; i < L.n; i += nm.stride) {
    double d = L.v[(i64)i * Bv + nm.b];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (k < L.nd) {
        const int off = dia_off(L, k);
        const double up = L.v[((i64)k * n + i) * Bv + nm.b];            // coupling (i, i + off): stored here
        const _Float16 h = (_Float16)(float)(up * inv);
        o16[((i64)(k - 1) * n + i) * Bv + nm.b] = h;
        if (i + off < L.n) {
          d += up - osc * (double)(float)h;
          under = under || (up != 0.0 && fabs(up * inv) < tiny);
        }
        if (i - off >= 0) {                                             // coupling (i - off, i): stored at the other end
          const double lo = L.v[((i64)k * n + (i - off)) * Bv + nm.b];
          d += lo - osc * (double)(float)(_Float16)(float)(lo * inv);
        }
      }
    }
    d32[(i64)i * Bv + nm.b] = (float)d;
  }
  if (flags && __any(under) && (threadIdx.x & 63) == 0) atomicOr(flags, 1);
}
}  // namespace

extern "C" int diffhe_lattice_pack_h16(const diffhe_mg_level* level, int Bv, const double* offdiag_scales, float* diag32,
                                       void* offdiag16, int* flags, void* stream) {
  if (!level || !diag32 || !offdiag16 || !level->vals || (level->nd != 3 && level->nd != 4) || !offdiag_scales)
    return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  Level L{};
  L.nx = level->nx; L.ny = level->ny; L.W = level->nx + 1; L.n = (level->nx + 1) * (level->ny + 1); L.nd = level->nd;
  L.v = level->vals;
  diffhe::account((8.0 * L.nd + 4.0 + 2.0 * (L.nd - 1)) * (double)L.n * Bv);
  hipLaunchKernelGGL(dia_pack_h16_kernel, node_grid(L.n, Bv), dim3(256), 0, (hipStream_t)stream, L, Bv, offdiag_scales,
                     diag32, (_Float16*)offdiag16, flags);
  return diffhe::check_launch();
}

namespace {
// Per-sample maximum of the main diagonal over the FREE rows (identity rows of Dirichlet nodes carry 1.0 whatever the
// magnitude of kappa and are skipped): the quantity the per-sample fp16 scale is derived from.  out: Bv doubles.
__global__ __launch_bounds__(256) void dia_maxdiag_free_kernel(Level L, int Bv, unsigned long long* __restrict__ out) {
  const NodeMap nm = node_map(Bv);
  double m = 0.0;
  if (nm.b < Bv)
    for (int i = nm.node0; i < L.n; i += nm.stride) {
      const double d = L.bc[i] ? 0.0 : L.v[(i64)i * Bv + nm.b];
      m = d > m ? d : m;
    }
  const int LB = Bv < kWave ? Bv : kWave;
  for (int off = LB; off < kWave; off <<= 1) {  // lanes that hold the same sample
    const double o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  if ((int)(threadIdx.x & 63) < LB && nm.b < Bv) atomicMax(out + nm.b, (unsigned long long)__double_as_longlong(m));
}
}  // namespace

extern "C" int diffhe_lattice_max_diag(const diffhe_mg_level* level, int Bv, double* out, void* stream) {
  if (!level || !out || !level->vals || !level->is_bc || (level->nd != 3 && level->nd != 4)) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  Level L{};
  L.nx = level->nx; L.ny = level->ny; L.W = level->nx + 1; L.n = (level->nx + 1) * (level->ny + 1); L.nd = level->nd;
  L.v = level->vals; L.bc = level->is_bc;
  int rc = diffhe::check(hipMemsetAsync(out, 0, sizeof(double) * Bv, (hipStream_t)stream));
  if (rc) return rc;
  diffhe::account(8.0 * (double)L.n * Bv);
  hipLaunchKernelGGL(dia_maxdiag_free_kernel, node_grid(L.n, Bv, 512), dim3(256), 0, (hipStream_t)stream, L, Bv,
                     (unsigned long long*)out);
  return diffhe::check_launch();
}

extern "C" int diffhe_lattice_restrict_kappa(const double* kappa_fine, double* kappa_coarse, int nx_coarse,
                                             int ny_coarse, int sx, int sy, int Bv, void* stream) {
  if (!kappa_fine || !kappa_coarse || nx_coarse < 1 || ny_coarse < 1) return DIFFHE_E_BADARG;
  if ((sx != 1 && sx != 2) || (sy != 1 && sy != 2) || (sx == 1 && sy == 1)) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  diffhe::account(8.0 * Bv * (2.0 * nx_coarse * ny_coarse) * (1.0 + sx * sy));
  hipLaunchKernelGGL(mg_restrict_kappa_kernel, node_grid(2 * nx_coarse * ny_coarse, Bv), dim3(256), 0,
                     (hipStream_t)stream, kappa_fine, kappa_coarse, nx_coarse, ny_coarse, sx, sy, Bv);
  return diffhe::check_launch();
}
