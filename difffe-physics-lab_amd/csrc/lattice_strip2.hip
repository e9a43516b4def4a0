// The packed-fp32 strip kernels of a batch-shared matrix, two samples per lane: dia_strip2_kernel (sweeps, residual +
// restriction, prolongation + sweep of the fp32 V-cycle) and cgstep2_kernel (the CG step with fp32 directions).
#include "lattice.h"

namespace diffhe_lattice __attribute__((visibility("hidden"))) {
namespace {

// ---------------------------------------------------------------------------------------------
// Two samples per lane: the strip kernels of the fp32-stored V-cycle for a batch-SHARED matrix
// (factored operator K_b = s_b K_1, or one per-element field for the whole batch).
//
// A lane owns TWO adjacent samples, a wave 128: every vector access is 8 B per lane / 512 B per wave
// instead of 4 / 256 (this GPU streams 4 B-per-lane accesses at ~4.8 TB/s, 8 B at 5.3-5.5:
// profiles/r02_stream_bench.txt), and the arithmetic is PACKED fp32 (v_pk_fma_f32: both samples per
// instruction) on fp32 coefficient copies that arrive as scalar loads -- about a fifth of the
// instructions per sample of the fp64-in-registers form.  The vectors of this cycle are stored
// fp32 anyway: a stored x carries a 2^-24 relative rounding that enters A x with weight |A||x|, and
// fp32 accumulation of the seven stencil terms adds the same order (measured: same iteration
// counts, same parity).  Written in "unit" form: with ib = 1 / s_b,
//     Jacobi   x' = x + omega rd0 (b ib - K_1 x)          (rd0 = 1 / diag K_1, batch-shared)
//     residual r  = b - s_b (K_1 x)
// so a sweep needs no division at all.  Same strips, tiles, window and fusions as strip_body.
// ---------------------------------------------------------------------------------------------
template <int MODE, int FUSE, int ND, bool XFROMB, int RW, bool TAIL, bool DOT, bool BST>
__device__ __forceinline__ void strip2_body(const Level& L, v2f ib, v2f sb, const float* __restrict__ src,
                                            const float* __restrict__ bvec, float* __restrict__ out, float omega,
                                            float omega_in, const Extra& ex, int Bp, unsigned lb, int c0w, int r0,
                                            int r1, double& s0, double& s1) {
  const int W = L.W, nyp = L.ny + 1;
  const i64 n = L.n;
  const v2f zero2 = {0.0f, 0.0f};
  // Bases sit at window row r0 - 1, one column LEFT of the strip: window column q (grid column c0w - 1 + q) has the
  // non-negative lane offset (dq[q] + 1) * Bp, row `row` the uniform offset (row - r0 + 1) * W * Bp.
  int dq[RW + 2];
  bool okq[RW + 2];
  unsigned offq[RW + 2];
#pragma unroll
  for (int q = 0; q < RW + 2; ++q) {
    int c = c0w - 1 + q;
    okq[q] = !TAIL || (c >= 0 && c < W);   // interior strips (TAIL = false) have every window column inside the grid
    if (TAIL && c < 0) c = 0;
    if (TAIL && c > W - 1) c = W - 1;
    dq[q] = c - c0w;
    offq[q] = 4u * ((unsigned)((dq[q] + 1) * Bp) + lb);   // bytes
  }
  const i64 i0 = (i64)r0 * W + c0w;          // node (r0, c0w)
  const float* __restrict__ p0 = L.v32 + i0;
  const float* __restrict__ p1 = p0 + n;
  const float* __restrict__ p2 = p1 + n;
  const float* __restrict__ p3 = p2 + n;
  const float* __restrict__ prd = L.rd32 + i0;
  const float* __restrict__ pmk = (FUSE == F_PROLONG) ? L.mk32 + i0 : nullptr;
  const i64 tile0 = (i0 - W - 1) * Bp;                                     // element (r0 - 1, c0w - 1)
  const rsrc_t rx = make_rsrc(src + tile0);
  const rsrc_t rb = make_rsrc(bvec ? bvec + tile0 : nullptr);
  const rsrc_t ro = make_rsrc((out && FUSE != F_RESTRICT) ? out + tile0 : nullptr);
  float* __restrict__ po = (out && FUSE != F_RESTRICT) ? out + tile0 + (i64)W * Bp : nullptr;   // row r0, column c0w - 1
  const unsigned rowB = 4u * (unsigned)W * (unsigned)Bp;                   // bytes per grid row
  const float inv_omega_in = XFROMB ? 1.0f / omega_in : 0.0f;
  const float* __restrict__ aux = (const float*)ex.a0;
  unsigned offc[RW / 2 + 2];   // F_PROLONG: coarse columns c0w/2 - 1 + j (clamped), as offsets into a coarse row
#pragma unroll
  for (int j = 0; j < RW / 2 + 2; ++j) {
    int cj = (c0w >> 1) - 1 + j;
    cj = cj < 0 ? 0 : (cj > ex.cW - 1 ? ex.cW - 1 : cj);
    offc[j] = (FUSE == F_PROLONG) ? 4u * ((unsigned)(cj * Bp) + lb) : 0u;
  }
  const int cr0 = (r0 > 0 ? r0 - 1 : 0) >> 1;                              // first coarse row this tile reads
  const rsrc_t rc = make_rsrc(FUSE == F_PROLONG ? aux + (i64)cr0 * ex.cW * Bp : nullptr);
  const unsigned rowCB = 4u * (unsigned)ex.cW * (unsigned)Bp;

  // sx = byte offset of window row `row` in the tile
  auto load_window = [&](int row, unsigned sx, const float* __restrict__ rdrow, const float* __restrict__ mkrow,
                         v2f* dst) {
    v2f ce[RW / 2 + 2], ce2[RW / 2 + 2];
    if (FUSE == F_PROLONG) {  // coarse values around this strip
      const unsigned sc = (unsigned)((row >> 1) - cr0) * rowCB;
#pragma unroll
      for (int j = 0; j < RW / 2 + 2; ++j) {
        ce[j] = bld(rc, offc[j], sc);
        ce2[j] = (row & 1) ? bld(rc, offc[j], sc + rowCB) : zero2;
      }
    }
#pragma unroll
    for (int q = 0; q < RW + 2; ++q) {
      v2f v = bld(rx, offq[q], sx);
      if (XFROMB) v = (v * ib) * (omega_in * rdrow[dq[q]]);   // x1 = omega_in D^-1 rhs, formed on the fly
      if (FUSE == F_PROLONG) {
        v2f corr;  // c0w is even: window column q has the parity of q + 1
        if (q & 1)
          corr = (row & 1) ? 0.5f * (ce[(q - 1) / 2 + 1] + ce2[(q - 1) / 2 + 1]) : ce[(q - 1) / 2 + 1];
        else
          corr = (row & 1) ? 0.5f * (ce[q / 2 + 1] + ce2[q / 2]) : 0.5f * (ce[q / 2] + ce[q / 2 + 1]);
        v += mkrow[dq[q]] * corr;   // mask: 0 on Dirichlet rows (no correction there), 1 elsewhere
      }
      dst[q] = okq[q] ? v : zero2;
    }
  };

  v2f xm[RW + 2], xc[RW + 2], xp[RW + 2];
  float n2p[RW], d3p[RW + 1];
#pragma unroll
  for (int q = 0; q < RW + 2; ++q) xm[q] = zero2;
  if (r0 > 0) load_window(r0 - 1, 0u, prd - W, pmk ? pmk - W : nullptr, xm);
  load_window(r0, rowB, prd, pmk, xc);
  unsigned sx = rowB;                                                      // byte offset of the current row
#pragma unroll
  for (int k = 0; k < RW; ++k) n2p[k] = (p2 - W)[dq[k + 1]];
#pragma unroll
  for (int k = 0; k < RW + 1; ++k) d3p[k] = (ND == 4) ? (p3 - W)[dq[k + 1]] : 0.0f;

  constexpr int CWR = (FUSE == F_RESTRICT) ? (RW - 1) / 2 : 1;  // coarse columns of an F_RESTRICT strip
  v2f racc[CWR], rnext[CWR];
#pragma unroll
  for (int j = 0; j < CWR; ++j) racc[j] = rnext[j] = zero2;
  const int cI0 = (r0 + 1) >> 1, cJ0 = (c0w + 1) >> 1;          // F_RESTRICT: first coarse row / column

  for (int row = r0; row < r1; ++row) {
    if (row + 1 < nyp) {
      load_window(row + 1, sx + rowB, prd + W, pmk ? pmk + W : nullptr, xp);
    } else {
#pragma unroll
      for (int q = 0; q < RW + 2; ++q) xp[q] = zero2;
    }
    float d0[RW], e1[RW + 1], n2c[RW], d3c[RW + 1];
    v2f resrow[(FUSE == F_RESTRICT) ? RW : 1];
    if (FUSE == F_RESTRICT) {
#pragma unroll
      for (int k = 0; k < RW; ++k) resrow[k] = zero2;
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      d0[k] = p0[dq[k + 1]];
      n2c[k] = p2[dq[k + 1]];
    }
#pragma unroll
    for (int k = 0; k < RW + 1; ++k) {
      const int dc = TAIL ? dq[k] : k - 1;  // east coupling of column c0w - 1 + k (TAIL covers c0w < 1: clamped)
      e1[k] = p1[dc];
      d3c[k] = (ND == 4) ? p3[dq[k + 1]] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      const int q = k + 1;
      if (TAIL && (c0w + k >= W || c0w + k < 0)) continue;
      if (MODE == M_JACOBI) {
        // unit form: bu = b / s_b; XFROMB: the window holds x1 = omega_in rd0 bu, so bu = x1 d0 / omega_in
        v2f braw = zero2, res;
        if (XFROMB) {
          res = xc[q] * (d0[k] * inv_omega_in);
          if (DOT) braw = res * sb;
        } else {
          braw = bld(rb, offq[q], sx);
          res = braw * ib;
        }
        res -= d0[k] * xc[q];
        res -= e1[k + 1] * xc[q + 1];
        res -= e1[k] * xc[q - 1];
        res -= n2c[k] * xp[q];
        res -= n2p[k] * xm[q];
        if (ND == 4) {
          res -= d3c[k] * xp[q - 1];
          res -= d3p[k + 1] * xm[q + 1];
        }
        const v2f xo = xc[q] + (omega * prd[dq[q]]) * res;
        if (BST) bst(ro, offq[q], sx, xo);
        else *(v2f*)((char*)po + offq[q]) = xo;
        if (DOT) {
          const v2f pr = braw * xo;
          s0 += (double)pr.x;
          s1 += (double)pr.y;
        }
      } else {  // M_RESID (+ F_RESTRICT): r = b - s_b (K_1 x)
        v2f acc = d0[k] * xc[q];
        acc += e1[k + 1] * xc[q + 1];
        acc += e1[k] * xc[q - 1];
        acc += n2c[k] * xp[q];
        acc += n2p[k] * xm[q];
        if (ND == 4) {
          acc += d3c[k] * xp[q - 1];
          acc += d3p[k + 1] * xm[q + 1];
        }
        const v2f res = bld(rb, offq[q], sx) - sb * acc;
        if (FUSE == F_RESTRICT) resrow[k] = res;
        else if (BST) bst(ro, offq[q], sx, res);
        else *(v2f*)((char*)po + offq[q]) = res;
      }
    }
    if (FUSE == F_RESTRICT) {
      // strip column k <-> fine column 2 cJ0 - 1 + k, so coarse column cJ0 + j sits at k = 2 j + 1.
      // Full weighting of the P1 lattice: centre 1; W, E, N, S, NE-of-the-row-above, SW-of-the-row-below 1/2.
      const bool store = (row & 1) || row + 1 >= nyp;  // coarse row complete after its odd row (or at the last row)
      if (!(row & 1)) {
#pragma unroll
        for (int j = 0; j < CWR; ++j) racc[j] += resrow[2 * j + 1] + 0.5f * (resrow[2 * j] + resrow[2 * j + 2]);
      } else {
#pragma unroll
        for (int j = 0; j < CWR; ++j) {
          racc[j] += 0.5f * (resrow[2 * j + 1] + resrow[2 * j]);
          rnext[j] = 0.5f * (resrow[2 * j + 1] + resrow[2 * j + 2]);
        }
      }
      if (store) {
        const int I = row >> 1;
        if (I >= cI0) {
#pragma unroll
          for (int j = 0; j < CWR; ++j) {
            const int J = cJ0 + j;
            if (J < ex.cW) {
              const i64 Ic = (i64)I * ex.cW + J;
              st2(out + Ic * Bp, lb, ex.bc[Ic] ? zero2 : racc[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < CWR; ++j) {
          racc[j] = rnext[j];
          rnext[j] = zero2;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RW + 2; ++q) {
      xm[q] = xc[q];
      xc[q] = xp[q];
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) n2p[k] = n2c[k];
#pragma unroll
    for (int k = 0; k < RW + 1; ++k) d3p[k] = d3c[k];
    p0 += W; p1 += W; p2 += W; p3 += W; prd += W;
    if (FUSE == F_PROLONG) pmk += W;
    sx += rowB;
    if (!BST && po) po += (i64)W * Bp;
  }
}

template <int MODE, int FUSE, int ND, bool XFROMB, int RW, bool DOT, bool BST>
__global__ __launch_bounds__(256) void dia_strip2_kernel(Level L, const double* __restrict__ scale,
                                                          const float* __restrict__ xin, const float* __restrict__ bvec,
                                                          float* __restrict__ out, float omega, float omega_in, Extra ex,
                                                          double* __restrict__ part, int Bp, int ncb, int TR) {
  __shared__ double lds[4 * kWave];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lb = blockIdx.y * (2 * kWave) + 2 * lane;   // first of this lane's two samples
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int rc = tile / ncb, cb = tile - rc * ncb;
  const int nyp = L.ny + 1;
  int c0w, r0, r1;
  bool active;
  if (FUSE == F_RESTRICT) {  // TR counts COARSE rows, the wave owns (RW - 1) / 2 coarse columns
    const int J0 = (cb * 4 + wave) * ((RW - 1) / 2), I0 = rc * TR;
    const int cnyp = (nyp + 1) >> 1;
    const int I1 = (I0 + TR < cnyp) ? I0 + TR : cnyp;
    c0w = 2 * J0 - 1;
    r0 = I0 > 0 ? 2 * I0 - 1 : 0;
    r1 = (2 * I1 < nyp) ? 2 * I1 : nyp;
    active = J0 < ex.cW && I0 < I1;
  } else {
    c0w = (cb * 4 + wave) * RW;
    r0 = rc * TR;
    r1 = (r0 + TR < nyp) ? r0 + TR : nyp;
    active = c0w < L.W && r0 < r1;
  }
  v2f sb = {1.0f, 1.0f};
  if (scale) {
    sb.x = (float)scale[lb];
    sb.y = (float)scale[lb + 1];
  }
  const v2f ib = 1.0f / sb;
  const float* __restrict__ src = XFROMB ? bvec : xin;
  double s0 = 0.0, s1 = 0.0;
  if (active) {
    if (c0w + RW + 1 > L.W || c0w < 1)    // strips that touch the left or right edge: clamped window columns
      strip2_body<MODE, FUSE, ND, XFROMB, RW, true, DOT, BST>(L, ib, sb, src, bvec, out, omega, omega_in, ex, Bp, lb, c0w, r0, r1,
                                                         s0, s1);
    else
      strip2_body<MODE, FUSE, ND, XFROMB, RW, false, DOT, BST>(L, ib, sb, src, bvec, out, omega, omega_in, ex, Bp, lb, c0w, r0,
                                                          r1, s0, s1);
  }
  if (DOT) {
    const double t0 = block_sum_per_sample(s0, Bp, lds);
    const double t1 = block_sum_per_sample(s1, Bp, lds);
    if (wave == 0) {
      part[(i64)blockIdx.x * Bp + lb] = t0;
      part[(i64)blockIdx.x * Bp + lb + 1] = t1;
    }
  }
}

// ---- CG step of a batch-shared matrix with fp32-stored directions, two samples per lane -------------------------------
// p = z + beta p_old (fp32 fused multiply-add: the stored value), p . (K_1 p) with the stencil in packed fp32 on the fp32
// coefficient copies, accumulated per sample in fp64; A p itself is never stored (the residual update recomputes it in
// fp64 from the stored p, F_RUPD).  The fp32 stencil only enters the STEP LENGTH alpha = r.z / p.Ap: x += alpha p and
// r -= alpha A p use the same alpha and the exact (fp64) A p, so r = b - A x holds to fp64 whatever alpha is, and an
// error delta in alpha costs delta^2 of the energy reduction of the step (the minimum of a parabola).
// STORE = false (first step only): z already lives in p's ring slot, the direction is read in place and not stored.
template <typename VT, int ND, int RW, bool EDGE, bool STORE>
__device__ __forceinline__ void cgstep2_body(const Level& L, VT beta, bool first, const float* __restrict__ z,
                                             const float* __restrict__ pin, float* __restrict__ pout, int Bp, unsigned lb,
                                             int c0w, int r0, int r1, Acc& acc) {
  constexpr int N = RW + 2;                  // window columns c0w - 1 + j
  const int W = L.W, nyp = L.ny + 1;
  const i64 n = L.n;
  const VT Z = VLane<VT>::zero();
  const Coef<VT, true> cf(L, 0, lb, Bp);
  bool ok[N];
  unsigned off[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    int c = c0w - 1 + j;
    ok[j] = !EDGE || (c >= 0 && c < W);
    if (EDGE) c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
    off[j] = 4u * ((unsigned)(c - (c0w - 1) + 1) * (unsigned)Bp + lb);      // base sits one column further left
  }
  const i64 tile0 = ((i64)(r0 - 1) * W + (c0w - 2)) * Bp;                  // element (r0 - 1, c0w - 2)
  const Src rz = make_src(z + tile0);
  const Src rp = make_src(first ? z + tile0 : pin + tile0);
  const unsigned rowB = 4u * (unsigned)W * (unsigned)Bp;
  auto p_row = [&](int R, VT* dst) {
    if (EDGE && (R < 0 || R >= nyp)) {
#pragma unroll
      for (int j = 0; j < N; ++j) dst[j] = Z;
      return;
    }
    const unsigned sx = (unsigned)(R - (r0 - 1)) * rowB;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      VT v = ldsrc<VT>(rz, off[j], sx);
      if (!first) v += beta * ldsrc<VT>(rp, off[j], sx);
      dst[j] = ok[j] ? v : Z;
    }
  };
  VT a0[N], a1[N], a2[N];
  p_row(r0 - 1, a0);
  p_row(r0, a1);
  float* __restrict__ pp = pout + ((i64)r0 * W + c0w) * Bp;
  for (int row = r0; row < r1; ++row) {
    p_row(row + 1, a2);
    k1_row<VT, RW, ND, EDGE>(cf, n, W, row, c0w, a0, a1, a2, [&](int k, VT kx, float, float) {
      if (!EDGE || c0w + k < W) {
        if (STORE) __builtin_nontemporal_store(a1[k + 1], (VT*)(pp + (i64)k * Bp + lb));
        VLane<VT>::dot(acc, a1[k + 1], kx);
      }
    });
    pp += (i64)W * Bp;
#pragma unroll
    for (int j = 0; j < N; ++j) { a0[j] = a1[j]; a1[j] = a2[j]; }
  }
}

template <typename VT, int ND, int RW, int MW, bool STORE = true>
__global__ __launch_bounds__(256, MW) void cgstep2_kernel(Level L, const double* __restrict__ scale,
                                                           const double* __restrict__ beta, int first,
                                                           const float* __restrict__ z, const float* __restrict__ pin,
                                                           float* __restrict__ pout, double* __restrict__ part, int Bp,
                                                           int ncb, int TR) {
  __shared__ double lds[4 * kWave];
  constexpr int SPL = VLane<VT>::kSpl;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lb = blockIdx.y * (SPL * kWave) + SPL * lane;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int rc = tile / ncb, cb = tile - rc * ncb;
  const int nyp = L.ny + 1;
  const int c0w = (cb * 4 + wave) * RW;
  const int r0 = rc * TR;
  const int r1 = (r0 + TR < nyp) ? r0 + TR : nyp;
  Acc acc;
  if (c0w < L.W && r0 < r1) {
    const VT bt = first ? VLane<VT>::zero() : VLane<VT>::from_scale(beta, lb);
    const bool edge = c0w - 1 < 0 || c0w + RW > L.W - 1 || r0 - 1 < 0 || r1 > nyp - 1;
    if (edge) cgstep2_body<VT, ND, RW, true, STORE>(L, bt, first != 0, z, pin, pout, Bp, lb, c0w, r0, r1, acc);
    else cgstep2_body<VT, ND, RW, false, STORE>(L, bt, first != 0, z, pin, pout, Bp, lb, c0w, r0, r1, acc);
  }
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    const double f = scale ? scale[lb + q] : 1.0;
    const double t = block_sum_per_sample(acc.v[q] * f, Bp, lds);
    if (wave == 0) part[(i64)blockIdx.x * Bp + lb + q] = t;
  }
}

}  // namespace

// p = z + beta p_old, part = partials of p . (K_1 p) in packed fp32, spl (1 or 2) samples per lane (cgstep2_kernel)
void launch_cgstep2(const Level& L, const double* scale, const double* beta, int first, const float* z, const float* pin,
                    float* pout, double* part, int Bp, const StripGeom& g, int spl, hipStream_t st) {
  const dim3 grid(g.ncb * g.nrc, Bp / (spl * kWave));
  const bool in_place = first && pout == z;   // p0 = z0 is in its slot already: read only
  diffhe::account((in_place ? 4.0 : first ? 8.0 : 12.0) * (double)L.n * Bp);
#define CG2(VT_, ND_, MW_)                                                                                             \
  do {                                                                                                                 \
    if (in_place)                                                                                                      \
      hipLaunchKernelGGL((cgstep2_kernel<VT_, ND_, 4, MW_, false>), grid, dim3(256), 0, st, L, scale, beta, first, z, pin, \
                         pout, part, Bp, g.ncb, g.TR);                                                                 \
    else                                                                                                               \
      hipLaunchKernelGGL((cgstep2_kernel<VT_, ND_, 4, MW_>), grid, dim3(256), 0, st, L, scale, beta, first, z, pin, pout, \
                         part, Bp, g.ncb, g.TR);                                                                       \
  } while (0)
  // 8 waves per SIMD: 0.70 ms at 1024^2 x 256 (6: 0.75, 4: 0.75; the one-sample fp64 strip: 0.87; gpurun_out/r6e)
  if (spl == 2) { if (L.nd == 3) CG2(v2f, 3, 8); else CG2(v2f, 4, 8); }
  else { if (L.nd == 3) CG2(float, 3, 8); else CG2(float, 4, 8); }
#undef CG2
}

template <int MODE, bool XFROMB, int FUSE, int RW>
void launch_strip2(const Level& L, const double* scale, const float* xin, const float* bvec, float* out, double omega,
                   double omega_in, double* part, int Bp, const StripGeom& g, hipStream_t st, const Extra& ex) {
  dim3 grid(g.ncb * g.nrc, Bp / (2 * kWave));
  double bpn;  // algorithmic bytes per (node, sample), as launch_strip
  if (MODE == M_JACOBI) bpn = (XFROMB ? 2.0 : 3.0) * 4.0 + (FUSE == F_PROLONG ? 1.0 : 0.0);
  else bpn = 8.0 + (FUSE == F_RESTRICT ? 1.0 : 4.0);
  diffhe::account(bpn * (double)L.n * Bp);
  // 40 000 B of dynamic LDS per block cap the residency at 4 blocks (16 waves) per CU: measured best for these kernels
  // (sweep over 3 .. 7 blocks per CU on one box, gpurun_out/r3d: first two sweeps 0.506 / prolongation 0.803 / restriction
  // 0.582 ms at 4 against 0.514-0.523 / 0.815-0.818 / 0.589-0.590 unrestricted)
  constexpr unsigned dyn_lds = 40000u;
#define STRIP2(ND_, DOT_)                                                                                                  \
  hipLaunchKernelGGL((dia_strip2_kernel<MODE, FUSE, ND_, XFROMB, RW, DOT_, false>), grid, dim3(256), dyn_lds, st, L, scale, xin, \
                     bvec, out, (float)omega, (float)omega_in, ex, part, Bp, g.ncb, g.TR)
  if (MODE == M_JACOBI && part) {   // the sweep that leaves the partials of rhs . x (the CG's r.z)
    if (L.nd == 3) STRIP2(3, MODE == M_JACOBI); else STRIP2(4, MODE == M_JACOBI);
  } else {
    if (L.nd == 3) STRIP2(3, false); else STRIP2(4, false);
  }
#undef STRIP2
}

// Every launch_strip2 the cycle (lattice_cycle.hip) calls, once: with cgstep2_kernel (the driver's, lattice_pcg.hip) the
// kernel inventory of this unit.  Each line instantiates the kernels for 3 and 4 diagonals (M_JACOBI: with and without the partials of rhs . x).
#define INST(...)                                                                                                      \
  template void launch_strip2<__VA_ARGS__>(const Level&, const double*, const float*, const float*, float*, double, double, \
                                           double*, int, const StripGeom&, hipStream_t, const Extra&)
INST(M_JACOBI, true, F_NONE, 4);                        // op_jacobi_first2
INST(M_RESID, false, F_RESTRICT, 2 * kRestrictCols + 1);  // resid_restrict
INST(M_JACOBI, false, F_PROLONG, 4);                    // vcycle way up, unfused
#undef INST

}  // namespace diffhe_lattice
