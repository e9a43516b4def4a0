// The fused two-stage passes of the fp32 V-cycle: fused_pre_kernel (two sweeps + residual + restriction) and
// fused_post_kernel (prolongation + correction + two sweeps), with their launchers.
#include "lattice.h"

namespace diffhe_lattice __attribute__((visibility("hidden"))) {
namespace {

// ---------------------------------------------------------------------------------------------
// FUSED two-stage passes of the fp32 V-cycle (batch-shared matrix), round 3.
//
// The four strip passes of a level -- first two sweeps, residual + restriction, prolongation + sweep, sweep -- read the
// right-hand side four times and write / re-read two intermediate iterates: 42 B per node and sample, all of it HBM
// traffic, at the HBM rate (section 6 of DESIGN.md: these kernels run at 4.4-5.2 TB/s of REAL traffic; their inner
// loops are not the limit).  The packed-fp32 form leaves most of the issue slots idle, so they are spent on
// RECOMPUTATION instead: two chained stencil stages per pass, the intermediate iterate kept in registers on a
// one-column / one-row wider window and never stored.
//   PRE : x2 = two sweeps from 0, coarse rhs = R (r - A x2)       reads r; writes x2 and the coarse rhs:     9 B  (was 17)
//   POST: z  = two sweeps on (x2 + P e)                           reads x2, r, e; writes z:                 13 B  (was 25)
// 22 instead of 42 B per node and sample and cycle.  Same arithmetic per node as the unfused kernels (unit form, packed
// fp32), evaluated once more on the halo ring; results agree with them to fp32 rounding (different association only).
// A wave owns its columns for both stages; VT = v2f (two samples per lane) or float (one).
// ---------------------------------------------------------------------------------------------
// ---- PRE: first two sweeps from a zero guess + residual + full-weighting restriction -------------------------------
// Geometry of the F_RESTRICT strips: the wave owns CW coarse columns J0 .. J0 + CW - 1, i.e. the RW = 2 CW + 1 fine
// residual columns c0w = 2 J0 - 1 .. 2 J0 + 2 CW - 1 (the last one shared with -- and recomputed by -- the next strip),
// and stores x2 on the first 2 CW of them; tile rows: coarse I0 .. I1 - 1 = fine residual rows r0 .. r1 - 1
// (r0 = 2 I0 - 1, r1 = 2 I1), x2 stored on rows r0 .. r1 - 2 (all the way up on the last tile).
template <typename VT, int ND, int CW, bool EDGE, bool SHARED>
__device__ __forceinline__ void fused_pre_body(const Level& L, VT ib, VT sb, const float* __restrict__ rhs,
                                               float* __restrict__ x2out, float* __restrict__ crhs, float w0, float w1,
                                               int cW, const unsigned char* __restrict__ cbc, int Bp, unsigned lb, int c0w,
                                               int r0, int r1) {
  constexpr int RW = 2 * CW + 1;
  constexpr int N1 = RW + 4, N2 = RW + 2;    // columns of the x1 / x2 windows: c0w - 2 + j / c0w - 1 + j
  const int W = L.W, nyp = L.ny + 1;
  const i64 n = L.n;
  const VT Z = VLane<VT>::zero();
  typedef Coef<VT, SHARED> CF;
  i64 cbase = (i64)(r0 - 3) * W;             // coefficient resources: based below everything the tile touches
  if (cbase < 0) cbase = 0;
  const CF cf(L, cbase, lb, Bp);
  bool ok1[N1];
  unsigned off1[N1];
#pragma unroll
  for (int j = 0; j < N1; ++j) {
    int c = c0w - 2 + j;
    ok1[j] = !EDGE || (c >= 0 && c < W);
    if (EDGE) c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
    off1[j] = 4u * ((unsigned)(c - (c0w - 2) + 2) * (unsigned)Bp + lb);   // base sits two columns further left
  }
  // base: element (r0 - 2, c0w - 4): every offset below is non-negative
  const i64 tile0 = ((i64)(r0 - 2) * W + (c0w - 4)) * Bp;
  const Src rr = make_src(rhs + tile0);
  const unsigned rowB = 4u * (unsigned)W * (unsigned)Bp;
  const float inv_w0 = 1.0f / w0;

  // x1 on grid row R (window N1): w0 rd (r ib); 0 outside the grid
  auto x1_row = [&](int R, VT* dst) {
    if (EDGE && (R < 0 || R >= nyp)) {
#pragma unroll
      for (int j = 0; j < N1; ++j) dst[j] = Z;
      return;
    }
    const unsigned sx = (unsigned)(R - (r0 - 2)) * rowB;
    const i64 rb = (i64)R * W + (c0w - 2);
#pragma unroll
    for (int j = 0; j < N1; ++j) {
      const VT v = ldsrc<VT>(rr, off1[j], sx);
      i64 i = rb + j;
      if (EDGE) i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
      const typename CF::T dv = SHARED ? typename CF::T{} : cf.d(i);
      dst[j] = ok1[j] ? (v * ib) * (w0 * cf.rd(i, dv)) : Z;
    }
  };
  // x2 on grid row R (window N2) from x1 rows R - 1, R, R + 1
  auto x2_row = [&](int R, const VT* am, const VT* ac, const VT* ap, VT* dst) {
    if (EDGE && (R < 0 || R >= nyp)) {
#pragma unroll
      for (int j = 0; j < N2; ++j) dst[j] = Z;
      return;
    }
    k1_row<VT, N2, ND, EDGE>(cf, n, W, R, c0w - 1, am, ac, ap, [&](int j, VT kx, typename CF::T d0, typename CF::T rd) {
      const VT bu = ac[j + 1] * (d0 * inv_w0);              // x1 = w0 rd bu  ->  bu = x1 d0 / w0
      const VT v = ac[j + 1] + (w1 * rd) * (bu - kx);
      dst[j] = ok1[j + 1] ? v : Z;
    });
  };

  VT a0[N1], a1[N1], a2[N1];   // x1 rows R - 1, R, R + 1 of the x2 row being formed
  VT b0[N2], b1[N2], b2[N2];   // x2 rows row - 1, row, row + 1
  if constexpr (!SHARED && ND == 3) {
    // Per-sample coefficients: every coefficient row loaded ONCE into a register window (as in fused_post_body): the
    // diagonal when the row's x1 is formed (9 columns), its couplings one iteration later for the x2 stage (raw fp16
    // words), both kept one more iteration for the residual stage; the row below contributes its north couplings.
    struct CR { VT d[N2]; unsigned e[N2 + 1]; unsigned n[N2]; };   // columns c0w - 1 + j; e[t] = east coupling of column c0w - 2 + t
    auto at = [&](i64 i) -> i64 { return EDGE ? (i < 0 ? 0 : (i > n - 1 ? n - 1 : i)) : i; };
    auto load_d = [&](int R, VT* D) {          // diagonal of row R on the N1 columns c0w - 2 + j
      const i64 base = (i64)R * W + (c0w - 2);
#pragma unroll
      for (int j = 0; j < N1; ++j) D[j] = cf.d(at(base + j));
    };
    auto load_en = [&](int R, const VT* D, CR& c) {
      const i64 base = (i64)R * W + (c0w - 2);
#pragma unroll
      for (int t = 0; t < N2 + 1; ++t) c.e[t] = cf.e_raw(at(base + t));
#pragma unroll
      for (int j = 0; j < N2; ++j) {
        c.n[j] = cf.n2_raw(at(base + 1 + j));
        c.d[j] = D[j + 1];
      }
    };
    auto x1c = [&](int R, const VT* D, VT* dst) {
      if (EDGE && (R < 0 || R >= nyp)) {
#pragma unroll
        for (int j = 0; j < N1; ++j) dst[j] = Z;
        return;
      }
      const unsigned sx = (unsigned)(R - (r0 - 2)) * rowB;
#pragma unroll
      for (int j = 0; j < N1; ++j) {
        const VT v = ldsrc<VT>(rr, off1[j], sx);
        dst[j] = ok1[j] ? (v * ib) * (w0 * (1.0f / D[j])) : Z;
      }
    };
    auto k1c = [&](auto nc_tag, auto off_tag, const CR& c, const unsigned* sn, const VT* xm, const VT* xc, const VT* xq,
                   auto&& use) {
      constexpr int NC = decltype(nc_tag)::value, OFF = decltype(off_tag)::value;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int j = k + OFF;
        const VT d0 = c.d[j];
        VT acc = d0 * xc[k + 1];
        acc += cf.cvt(c.e[j + 1]) * xc[k + 2];
        acc += cf.cvt(c.e[j]) * xc[k];
        acc += cf.cvt(c.n[j]) * xq[k + 1];
        acc += cf.cvt(sn[j]) * xm[k + 1];
        use(k, acc, d0, 1.0f / d0);
      }
    };
    typedef std::integral_constant<int, N2> tN2;
    typedef std::integral_constant<int, RW> tRW;
    typedef std::integral_constant<int, 0> t0;
    typedef std::integral_constant<int, 1> t1;
    auto x2c = [&](int R, const CR& c, const unsigned* sn, const VT* am, const VT* ac, const VT* ap, VT* dst) {
      if (EDGE && (R < 0 || R >= nyp)) {
#pragma unroll
        for (int j = 0; j < N2; ++j) dst[j] = Z;
        return;
      }
      k1c(tN2{}, t0{}, c, sn, am, ac, ap, [&](int j, VT kx, VT d0, VT rd) {
        const VT bu = ac[j + 1] * (d0 * inv_w0);
        const VT v = ac[j + 1] + (w1 * rd) * (bu - kx);
        dst[j] = ok1[j + 1] ? v : Z;
      });
    };
    VT Dq[N1], Dn[N1];           // diagonals of the newest two x1 rows
    CR cA, cB;                   // coefficient rows of the x2 row being formed / of the residual row
    unsigned sS[N2];             // north couplings of the row below the residual row
    load_d(r0 - 2, Dq);
    x1c(r0 - 2, Dq, a0);
    load_en(r0 - 2, Dq, cB);     // only its n is used: south of row r0 - 1
    load_d(r0 - 1, Dq);
    x1c(r0 - 1, Dq, a1);
    load_en(r0 - 1, Dq, cA);
    load_d(r0, Dn);
    x1c(r0, Dn, a2);
    x2c(r0 - 1, cA, cB.n, a0, a1, a2, b0);
#pragma unroll
    for (int j = 0; j < N2; ++j) sS[j] = cA.n[j];      // n of row r0 - 1
#pragma unroll
    for (int j = 0; j < N1; ++j) { a0[j] = a1[j]; a1[j] = a2[j]; }
    load_d(r0 + 1, Dq);
    x1c(r0 + 1, Dq, a2);
    load_en(r0, Dn, cB);         // coefficient row r0
    x2c(r0, cB, sS, a0, a1, a2, b1);
    // loop invariant at the top of iteration `row`: cB = coefficient row `row`, sS = n of row - 1, Dq = diagonal of row + 1

    VT racc[CW], rnext[CW];
#pragma unroll
    for (int j = 0; j < CW; ++j) racc[j] = rnext[j] = Z;
    const int cI0 = (r0 + 1) >> 1, cJ0 = (c0w + 1) >> 1;
    const int last_store = (r1 >= nyp) ? nyp - 1 : r1 - 2;
    float* __restrict__ px2 = x2out + ((i64)r0 * W + c0w) * Bp;
    for (int row = r0; row < r1; ++row) {
#pragma unroll
      for (int j = 0; j < N1; ++j) { a0[j] = a1[j]; a1[j] = a2[j]; }
      load_d(row + 2, Dn);
      x1c(row + 2, Dn, a2);
      load_en(row + 1, Dq, cA);
      x2c(row + 1, cA, cB.n, a0, a1, a2, b2);
      VT res[RW];
      k1c(tRW{}, t1{}, cB, sS, b0, b1, b2, [&](int k, VT kx, VT d0, VT) {
        const VT bu = a0[k + 2] * (d0 * inv_w0);
        res[k] = (!EDGE || (c0w + k >= 0 && c0w + k < W)) ? bu - kx : Z;
      });
      if (row <= last_store) {
#pragma unroll
        for (int k = 0; k < RW - 1; ++k) {
          if (!EDGE || (c0w + k >= 0 && c0w + k < W)) *(VT*)(px2 + (i64)k * Bp + lb) = b1[k + 1];
        }
      }
      px2 += (i64)W * Bp;
      const bool store = (row & 1) || row + 1 >= nyp;
      if (!(row & 1)) {
#pragma unroll
        for (int j = 0; j < CW; ++j) racc[j] += res[2 * j + 1] + 0.5f * (res[2 * j] + res[2 * j + 2]);
      } else {
#pragma unroll
        for (int j = 0; j < CW; ++j) {
          racc[j] += 0.5f * (res[2 * j + 1] + res[2 * j]);
          rnext[j] = 0.5f * (res[2 * j + 1] + res[2 * j + 2]);
        }
      }
      if (store) {
        const int I = row >> 1;
        if (I >= cI0) {
#pragma unroll
          for (int j = 0; j < CW; ++j) {
            const int J = cJ0 + j;
            if (J < cW) {
              const i64 Ic = (i64)I * cW + J;
              *(VT*)(crhs + Ic * Bp + lb) = cbc[Ic] ? Z : sb * racc[j];
            }
          }
        }
#pragma unroll
        for (int j = 0; j < CW; ++j) { racc[j] = rnext[j]; rnext[j] = Z; }
      }
#pragma unroll
      for (int j = 0; j < N2; ++j) { b0[j] = b1[j]; b1[j] = b2[j]; sS[j] = cB.n[j]; }
      cB = cA;
#pragma unroll
      for (int j = 0; j < N1; ++j) Dq[j] = Dn[j];
    }
    return;
  }
  x1_row(r0 - 2, a0);
  x1_row(r0 - 1, a1);
  x1_row(r0, a2);
  x2_row(r0 - 1, a0, a1, a2, b0);
#pragma unroll
  for (int j = 0; j < N1; ++j) { a0[j] = a1[j]; a1[j] = a2[j]; }
  x1_row(r0 + 1, a2);
  x2_row(r0, a0, a1, a2, b1);

  VT racc[CW], rnext[CW];
#pragma unroll
  for (int j = 0; j < CW; ++j) racc[j] = rnext[j] = Z;
  const int cI0 = (r0 + 1) >> 1, cJ0 = (c0w + 1) >> 1;
  const int last_store = (r1 >= nyp) ? nyp - 1 : r1 - 2;
  float* __restrict__ px2 = x2out + ((i64)r0 * W + c0w) * Bp;

  for (int row = r0; row < r1; ++row) {
    // x1 row + 2 -> x2 row + 1
#pragma unroll
    for (int j = 0; j < N1; ++j) { a0[j] = a1[j]; a1[j] = a2[j]; }
    x1_row(row + 2, a2);
    x2_row(row + 1, a0, a1, a2, b2);
    // residual of row `row` on the RW columns c0w .. c0w + RW - 1 (unit form, times s_b at the store)
    VT res[RW];
    k1_row<VT, RW, ND, EDGE>(cf, n, W, row, c0w, b0, b1, b2, [&](int k, VT kx, typename CF::T d0, typename CF::T) {
      // bu at (row, c0w + k) from the x1 window kept for this row (a0 after the shift above = x1 row `row`)
      const VT bu = a0[k + 2] * (d0 * inv_w0);
      res[k] = (!EDGE || (c0w + k >= 0 && c0w + k < W)) ? bu - kx : Z;
    });
    // store x2 of this row on the owned columns
    if (row <= last_store) {
#pragma unroll
      for (int k = 0; k < RW - 1; ++k) {
        if (!EDGE || (c0w + k >= 0 && c0w + k < W)) *(VT*)(px2 + (i64)k * Bp + lb) = b1[k + 1];
      }
    }
    px2 += (i64)W * Bp;
    // full weighting, as in strip2_body
    const bool store = (row & 1) || row + 1 >= nyp;
    if (!(row & 1)) {
#pragma unroll
      for (int j = 0; j < CW; ++j) racc[j] += res[2 * j + 1] + 0.5f * (res[2 * j] + res[2 * j + 2]);
    } else {
#pragma unroll
      for (int j = 0; j < CW; ++j) {
        racc[j] += 0.5f * (res[2 * j + 1] + res[2 * j]);
        rnext[j] = 0.5f * (res[2 * j + 1] + res[2 * j + 2]);
      }
    }
    if (store) {
      const int I = row >> 1;
      if (I >= cI0) {
#pragma unroll
        for (int j = 0; j < CW; ++j) {
          const int J = cJ0 + j;
          if (J < cW) {
            const i64 Ic = (i64)I * cW + J;
            *(VT*)(crhs + Ic * Bp + lb) = cbc[Ic] ? Z : sb * racc[j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < CW; ++j) { racc[j] = rnext[j]; rnext[j] = Z; }
    }
#pragma unroll
    for (int j = 0; j < N2; ++j) { b0[j] = b1[j]; b1[j] = b2[j]; }
  }
}

// NW = waves per block (a block owns NW * CW adjacent coarse columns).  Round 4 measured 8 and 16 against 4 on the
// 1024^2 x 256 bench (gpurun_out/r4c): WIDER blocks read MORE from the fabric, not less (POST 1.56 -> 1.65 / 1.66 read
// passes: the waves of a larger block drift apart and miss each other's halo lines) and run slower (PRE 0.708 -> 0.740 /
// 0.818 ms, POST 1.000 -> 0.978 / 1.101 ms, step 81.7 -> 82.6 / 86.6 ms).  4 stays; the parameter documents the experiment.
template <typename VT, int ND, int CW, bool SHARED, int NW = 4, int MW = (SHARED ? 4 : 1)>
__global__ __launch_bounds__(64 * NW, MW) void fused_pre_kernel(Level L, const double* __restrict__ scale,
                                                         const float* __restrict__ rhs, float* __restrict__ x2out,
                                                         float* __restrict__ crhs, float w0, float w1, int cW,
                                                         const unsigned char* __restrict__ cbc, int Bp, int ncb, int TR) {
  constexpr int SPL = VLane<VT>::kSpl;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lb = blockIdx.y * (SPL * kWave) + SPL * lane;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int rc = tile / ncb, cb = tile - rc * ncb;
  const int nyp = L.ny + 1;
  const int J0 = (cb * NW + wave) * CW, I0 = rc * TR;
  const int cnyp = (nyp + 1) >> 1;
  const int I1 = (I0 + TR < cnyp) ? I0 + TR : cnyp;
  if (!(J0 < cW && I0 < I1)) return;
  const int c0w = 2 * J0 - 1;
  const int r0 = I0 > 0 ? 2 * I0 - 1 : 0;
  const int r1 = (2 * I1 < nyp) ? 2 * I1 : nyp;
  const VT sb = VLane<VT>::from_scale(scale, lb);
  const VT ib = 1.0f / sb;
  constexpr int RW = 2 * CW + 1;
  // interior tiles: every window column (c0w - 2 .. c0w + RW + 1) and row (r0 - 2 .. r1 + 1) lies inside the grid
  const bool edge = c0w - 2 < 0 || c0w + RW + 1 > L.W - 1 || r0 - 2 < 0 || r1 + 1 > nyp - 1;
  if (edge) fused_pre_body<VT, ND, CW, true, SHARED>(L, ib, sb, rhs, x2out, crhs, w0, w1, cW, cbc, Bp, lb, c0w, r0, r1);
  else fused_pre_body<VT, ND, CW, false, SHARED>(L, ib, sb, rhs, x2out, crhs, w0, w1, cW, cbc, Bp, lb, c0w, r0, r1);
}

// ---- POST: prolongation + correction + both post-smoothing sweeps (+ the partials of rhs . z) ------------------------
// The wave owns the RW columns c0w .. c0w + RW - 1 (c0w a multiple of RW, even); rows r0 .. r1 - 1.
// Round 4 built and measured a variant in which the 4 waves of a block EXCHANGE their halo columns through LDS instead of
// each loading (and prolongating) them again: 12 instead of 23 vector-memory loads per wave and fine row, x' and r / s_b
// written to a two-slot exchange area, ONE workgroup barrier per row.  Correct (28 GPU tests, same iteration counts) and
// TWICE as slow: 0.999 -> 2.035 ms per fine-level launch at 1024^2 x 256 (gpurun_out/r4o).  The barrier puts the block's
// waves in lockstep, and these passes live on their waves being at DIFFERENT points of the row loop (one wave's loads in
// flight under another's arithmetic); any block-cooperative staging of rows pays the same price.  Removed.
template <typename VT, int ND, int RW, bool EDGE, bool DOT, bool SHARED, bool XZ>
__device__ __forceinline__ void fused_post_body(const Level& L, VT ib, const float* __restrict__ xin,
                                                const float* __restrict__ rhs, const float* __restrict__ ec,
                                                float* __restrict__ zout, float wA, float wB, int cW, int Bp, unsigned lb,
                                                int c0w, int r0, int r1, Acc& acc) {
  constexpr int N1 = RW + 4, N2 = RW + 2;    // x' window: columns c0w - 2 + j; x3 window: c0w - 1 + j
  constexpr int NCE = RW / 2 + 3;            // coarse columns (c0w - 2) / 2 .. (c0w + RW + 1 + 1) / 2
  const int W = L.W, nyp = L.ny + 1;
  const i64 n = L.n;
  const VT Z = VLane<VT>::zero();
  typedef Coef<VT, SHARED> CF;
  i64 cbase = (i64)(r0 - 3) * W;
  if (cbase < 0) cbase = 0;
  const CF cf(L, cbase, lb, Bp);
  bool ok1[N1];
  unsigned off1[N1];
#pragma unroll
  for (int j = 0; j < N1; ++j) {
    int c = c0w - 2 + j;
    ok1[j] = !EDGE || (c >= 0 && c < W);
    if (EDGE) c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
    off1[j] = 4u * ((unsigned)(c - (c0w - 2) + 2) * (unsigned)Bp + lb);
  }
  const int cj0 = (c0w >> 1) - 1;            // first coarse column of the window (c0w is even)
  unsigned offc[NCE];
#pragma unroll
  for (int j = 0; j < NCE; ++j) {
    int cj = cj0 + j;
    cj = cj < 0 ? 0 : (cj > cW - 1 ? cW - 1 : cj);
    offc[j] = 4u * ((unsigned)cj * (unsigned)Bp + lb);
  }
  const i64 tile0 = ((i64)(r0 - 2) * W + (c0w - 4)) * Bp;
  const Src rx = make_src(XZ ? rhs + tile0 : xin + tile0);   // XZ: x = 0, never loaded
  const Src rr = make_src(rhs + tile0);
  const int cr0 = (r0 - 2 > 0 ? r0 - 2 : 0) >> 1;
  const Src rc = make_src(ec + (i64)cr0 * cW * Bp);
  const unsigned rowB = 4u * (unsigned)W * (unsigned)Bp, rowCB = 4u * (unsigned)cW * (unsigned)Bp;

  // x' = x + mask (P e) on grid row R
  auto xp_row = [&](int R, VT* dst) {
    if (EDGE && (R < 0 || R >= nyp)) {
#pragma unroll
      for (int j = 0; j < N1; ++j) dst[j] = Z;
      return;
    }
    const unsigned sx = (unsigned)(R - (r0 - 2)) * rowB;
    const unsigned sc = (unsigned)((R >> 1) - cr0) * rowCB;
    // (Keeping the coarse row in registers between fine rows -- it is loaded three times, 7.5 of a row's 23 loads -- was
    // built and measured in round 4: + 10 live VGPRs spill (100 B of scratch at the 128-VGPR cap of the shared form, 16-100 B
    // at the 168 cap of the per-sample one): POST 1.000 -> 1.034 ms, per-element-field step 213.5 -> 232.0 ms; gpurun_out/r4i.)
    // ... and kept in a lane-private LDS ring instead (no barrier, no cross-lane traffic: LDS as a second register file
    // that bypasses the texture addresser; 2.5 instead of 7.5 memory loads per fine row): correct and 1.002 -> 1.417 ms --
    // LDS and scalar loads share one counter (lgkmcnt), and the waits for the ring serialise the coefficient loads of
    // both stages (gpurun_out/r4r).  Removed as well.
    VT ce[NCE], ce2[NCE];
#pragma unroll
    for (int j = 0; j < NCE; ++j) {
      ce[j] = ldsrc<VT>(rc, offc[j], sc);
      ce2[j] = (R & 1) ? ldsrc<VT>(rc, offc[j], sc + rowCB) : Z;
    }
    const i64 rb = (i64)R * W + (c0w - 2);
#pragma unroll
    for (int j = 0; j < N1; ++j) {
      VT corr;
      if (!(j & 1))                      // even window column <-> coarse column cj0 + j / 2
        corr = (R & 1) ? 0.5f * (ce[j / 2] + ce2[j / 2]) : ce[j / 2];
      else                               // between coarse columns cj0 + (j - 1) / 2 and + 1
        corr = (R & 1) ? 0.5f * (ce[(j + 1) / 2] + ce2[(j - 1) / 2]) : 0.5f * (ce[(j - 1) / 2] + ce[(j + 1) / 2]);
      i64 i = rb + j;
      if (EDGE) i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
      const VT v = XZ ? L.mk32[i] * corr : ldsrc<VT>(rx, off1[j], sx) + L.mk32[i] * corr;
      dst[j] = ok1[j] ? v : Z;
    }
  };
  // bu = r / s_b on grid row R at the N2 columns c0w - 1 + j
  auto bu_row = [&](int R, VT* dst) {
    if (EDGE && (R < 0 || R >= nyp)) {
#pragma unroll
      for (int j = 0; j < N2; ++j) dst[j] = Z;
      return;
    }
    const unsigned sx = (unsigned)(R - (r0 - 2)) * rowB;
#pragma unroll
    for (int j = 0; j < N2; ++j) dst[j] = ok1[j + 1] ? ldsrc<VT>(rr, off1[j + 1], sx) * ib : Z;
  };
  // x3 on grid row R (window N2) from x' rows R - 1, R, R + 1 and bu row R
  auto x3_row = [&](int R, const VT* am, const VT* ac, const VT* ap, const VT* bu, VT* dst) {
    if (EDGE && (R < 0 || R >= nyp)) {
#pragma unroll
      for (int j = 0; j < N2; ++j) dst[j] = Z;
      return;
    }
    k1_row<VT, N2, ND, EDGE>(cf, n, W, R, c0w - 1, am, ac, ap, [&](int j, VT kx, typename CF::T, typename CF::T rd) {
      const VT v = ac[j + 1] + (wA * rd) * (bu[j] - kx);
      dst[j] = ok1[j + 1] ? v : Z;
    });
  };

  VT a0[N1], a1[N1], a2[N1];   // x' rows
  VT b0[N2], b1[N2], b2[N2];   // x3 rows row - 1, row, row + 1
  VT u1[N2], u2[N2];           // bu rows row, row + 1
  if constexpr (!SHARED && ND == 3) {
    // Per-sample coefficients (fp32 diagonal + fp16 couplings, one value per lane and sample): every coefficient row is
    // needed four times -- by the x3 stage and the z stage, as the row's own couplings and as the south couplings of the
    // row above -- and re-loading it each time missed the caches about half the time (PMC: 4.54 passes of traffic for
    // 2.6 algorithmic, 5.4 TB/s: bandwidth-bound on wasted re-reads).  Rows are loaded ONCE into a register window, the
    // couplings kept as raw fp16 words (one VGPR per pair of samples).
    struct CRow { VT d[N2]; unsigned e[N2 + 1]; unsigned n[N2]; };   // columns c0w - 1 + j; e[j + 1] = east coupling of column j
    auto load_crow = [&](int R, CRow& c) {
      const i64 base = (i64)R * W + (c0w - 1);
      auto at = [&](i64 i) -> i64 { return EDGE ? (i < 0 ? 0 : (i > n - 1 ? n - 1 : i)) : i; };
      c.e[0] = cf.e_raw(at(base - 1));
#pragma unroll
      for (int j = 0; j < N2; ++j) {
        const i64 i = at(base + j);
        c.d[j] = cf.d(i);
        c.e[j + 1] = cf.e_raw(i);
        c.n[j] = cf.n2_raw(i);
      }
    };
    // K_1 x on NC columns starting at cached column OFF, row couplings c, south couplings sn (the n of the row below)
    auto k1c = [&](auto nc_tag, auto off_tag, const CRow& c, const unsigned* sn, const VT* xm, const VT* xc, const VT* xq,
                   auto&& use) {
      constexpr int NC = decltype(nc_tag)::value, OFF = decltype(off_tag)::value;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int j = k + OFF;
        const VT d0 = c.d[j];
        VT acc = d0 * xc[k + 1];
        acc += cf.cvt(c.e[j + 1]) * xc[k + 2];
        acc += cf.cvt(c.e[j]) * xc[k];
        acc += cf.cvt(c.n[j]) * xq[k + 1];
        acc += cf.cvt(sn[j]) * xm[k + 1];
        use(k, acc, d0, 1.0f / d0);
      }
    };
    typedef std::integral_constant<int, N2> tN2;
    typedef std::integral_constant<int, RW> tRW;
    typedef std::integral_constant<int, 0> t0;
    typedef std::integral_constant<int, 1> t1;
    auto x3c = [&](int R, const CRow& c, const unsigned* sn, const VT* am, const VT* ac, const VT* ap, const VT* bu, VT* dst) {
      if (EDGE && (R < 0 || R >= nyp)) {
#pragma unroll
        for (int j = 0; j < N2; ++j) dst[j] = Z;
        return;
      }
      k1c(tN2{}, t0{}, c, sn, am, ac, ap, [&](int j, VT kx, VT, VT rd) {
        const VT v = ac[j + 1] + (wA * rd) * (bu[j] - kx);
        dst[j] = ok1[j + 1] ? v : Z;
      });
    };
    CRow cS, cC, cN;             // coefficient rows R - 1, R, R + 1 of the x3 row being formed
    load_crow(r0 - 2, cS);
    load_crow(r0 - 1, cC);
    xp_row(r0 - 2, a0);
    xp_row(r0 - 1, a1);
    xp_row(r0, a2);
    bu_row(r0 - 1, u1);
    x3c(r0 - 1, cC, cS.n, a0, a1, a2, u1, b0);
#pragma unroll
    for (int j = 0; j < N1; ++j) { a0[j] = a1[j]; a1[j] = a2[j]; }
    xp_row(r0 + 1, a2);
    bu_row(r0, u1);
    load_crow(r0, cN);
    x3c(r0, cN, cC.n, a0, a1, a2, u1, b1);
    // from here on: cS = row - 1 (only its n is used), cC = row, cN = row + 1
#pragma unroll
    for (int j = 0; j < N2; ++j) cS.n[j] = cC.n[j];
    cC = cN;
    float* __restrict__ pz = zout + ((i64)r0 * W + c0w) * Bp;
    for (int row = r0; row < r1; ++row) {
#pragma unroll
      for (int j = 0; j < N1; ++j) { a0[j] = a1[j]; a1[j] = a2[j]; }
      xp_row(row + 2, a2);
      bu_row(row + 1, u2);
      load_crow(row + 1, cN);
      x3c(row + 1, cN, cC.n, a0, a1, a2, u2, b2);
      k1c(tRW{}, t1{}, cC, cS.n, b0, b1, b2, [&](int k, VT kx, VT, VT rd) {
        if (!EDGE || c0w + k < W) {
          const VT z = b1[k + 1] + (wB * rd) * (u1[k + 1] - kx);
          *(VT*)(pz + (i64)k * Bp + lb) = z;
          if (DOT) VLane<VT>::dot(acc, u1[k + 1], z);
        }
      });
      pz += (i64)W * Bp;
#pragma unroll
      for (int j = 0; j < N2; ++j) { b0[j] = b1[j]; b1[j] = b2[j]; u1[j] = u2[j]; cS.n[j] = cC.n[j]; }
      cC = cN;
    }
    return;
  }
  xp_row(r0 - 2, a0);
  xp_row(r0 - 1, a1);
  xp_row(r0, a2);
  bu_row(r0 - 1, u1);
  x3_row(r0 - 1, a0, a1, a2, u1, b0);
#pragma unroll
  for (int j = 0; j < N1; ++j) { a0[j] = a1[j]; a1[j] = a2[j]; }
  xp_row(r0 + 1, a2);
  bu_row(r0, u1);
  x3_row(r0, a0, a1, a2, u1, b1);
  float* __restrict__ pz = zout + ((i64)r0 * W + c0w) * Bp;

  // (A software-pipelined form of this loop -- the raw loads of the next row requested before this row's two stencil stages,
  // 48 more live VGPRs, 3 instead of 4 waves per SIMD -- was built and measured at the end of round 4: correct, 168 VGPRs with
  // 80 B of scratch, 0.999 -> 1.321 ms per fine-level launch, step 80.8 -> 87.5 ms, gpurun_out/r4bj.  Independent waves hide the
  // row's load latency better than one wave overlapping its own rows.)
  for (int row = r0; row < r1; ++row) {
#pragma unroll
    for (int j = 0; j < N1; ++j) { a0[j] = a1[j]; a1[j] = a2[j]; }
    xp_row(row + 2, a2);
    bu_row(row + 1, u2);
    x3_row(row + 1, a0, a1, a2, u2, b2);
    k1_row<VT, RW, ND, EDGE>(cf, n, W, row, c0w, b0, b1, b2, [&](int k, VT kx, typename CF::T, typename CF::T rd) {
      if (!EDGE || c0w + k < W) {
        const VT z = b1[k + 1] + (wB * rd) * (u1[k + 1] - kx);
        *(VT*)(pz + (i64)k * Bp + lb) = z;
        if (DOT) VLane<VT>::dot(acc, u1[k + 1], z);     // (r / s_b) . z; times s_b after the loop
      }
    });
    pz += (i64)W * Bp;
#pragma unroll
    for (int j = 0; j < N2; ++j) { b0[j] = b1[j]; b1[j] = b2[j]; u1[j] = u2[j]; }
  }
}

// XZ: the operand is P e alone (x = 0 is not read): two sweeps from a prolonged initial guess, the first stage of a
// full-multigrid level (vcycle with `guess`)
template <typename VT, int ND, int RW, bool DOT, bool SHARED, bool XZ = false, int NW = 4, int MW = (SHARED ? 4 : 1)>
__global__ __launch_bounds__(64 * NW, MW) void fused_post_kernel(Level L, const double* __restrict__ scale,
                                                          const float* __restrict__ xin, const float* __restrict__ rhs,
                                                          const float* __restrict__ ec, float* __restrict__ zout, float wA,
                                                          float wB, int cW, double* __restrict__ part, int Bp, int ncb,
                                                          int TR) {
  __shared__ double lds[NW * kWave];
  constexpr int SPL = VLane<VT>::kSpl;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lb = blockIdx.y * (SPL * kWave) + SPL * lane;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int rc = tile / ncb, cb = tile - rc * ncb;
  const int nyp = L.ny + 1;
  const int c0w = (cb * NW + wave) * RW;
  const int r0 = rc * TR;
  const int r1 = (r0 + TR < nyp) ? r0 + TR : nyp;
  const bool active = c0w < L.W && r0 < r1;
  const VT sb = VLane<VT>::from_scale(scale, lb);
  const VT ib = 1.0f / sb;
  Acc acc;
  if (active) {
    const bool edge = c0w - 2 < 0 || c0w + RW + 1 > L.W - 1 || r0 - 2 < 0 || r1 + 1 > nyp - 1;
    if (edge)
      fused_post_body<VT, ND, RW, true, DOT, SHARED, XZ>(L, ib, xin, rhs, ec, zout, wA, wB, cW, Bp, lb, c0w, r0, r1, acc);
    else
      fused_post_body<VT, ND, RW, false, DOT, SHARED, XZ>(L, ib, xin, rhs, ec, zout, wA, wB, cW, Bp, lb, c0w, r0, r1, acc);
  }
  if (DOT) {
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      const double f = scale ? scale[lb + q] : 1.0;
      const double t = block_sum_waves<NW>(acc.v[q] * f, lds);
      if (wave == 0) part[(i64)blockIdx.x * Bp + lb + q] = t;
    }
  }
}

}  // namespace

// Fused two-stage passes (fused_pre_kernel / fused_post_kernel), two samples per lane where the batch allows (fill_hier).
// They run without dynamic LDS: a cap on the blocks resident per CU only slowed them (118-125 VGPRs: 4 waves per SIMD
// anyway; run r3w: 93.9 ms per step uncapped, 94.4 at 40 000 B per block, 103.8 at 54 000).
void launch_fused_pre(const Level& L, const Level& C, int Bv, const double* scale, const float* rhs, float* x2, float* crhs,
                      double w0, double w1, int Bp, const StripGeom& g, int spl, hipStream_t st) {
  constexpr int CW = kRestrictCols;
  // r read, x2 and the coarse rhs written; per-sample matrices: + the compact coefficients (read by both stages)
  diffhe::account((9.0 + (Bv == 1 ? 0.0 : 4.0 + 2.0 * (L.nd - 1))) * (double)L.n * Bp);
  const dim3 grid(g.ncb * g.nrc, Bp / (spl * kWave));
#define FPRE(VT_, ND_, SH_)                                                                                               \
  hipLaunchKernelGGL((fused_pre_kernel<VT_, ND_, CW, SH_>), grid, dim3(256), 0, st, L, scale, rhs, x2, crhs,              \
                     (float)w0, (float)w1, C.W, C.bc, Bp, g.ncb, g.TR)
  // per-sample coefficients: 206 VGPRs = 2 waves per SIMD; capped at 168 (3 waves) it spills and loses (launch_fused_post)
  if (Bv != 1) { if (L.nd == 3) FPRE(v2f, 3, false); else FPRE(v2f, 4, false); }
  else if (spl == 4 && L.nd == 3)
    hipLaunchKernelGGL((fused_pre_kernel<v4f, 3, CW, true, 4, 2>), grid, dim3(256), 0, st, L, scale, rhs, x2, crhs,
                       (float)w0, (float)w1, C.W, C.bc, Bp, g.ncb, g.TR);
  else if (spl >= 2) { if (L.nd == 3) FPRE(v2f, 3, true); else FPRE(v2f, 4, true); }
  else { if (L.nd == 3) FPRE(float, 3, true); else FPRE(float, 4, true); }
#undef FPRE
}

void launch_fused_post(const Level& L, const Level& C, int Bv, const double* scale, const float* xin, const float* rhs,
                       const float* ec, float* z, double wA, double wB, double* part, int Bp, const StripGeom& g, int spl,
                       hipStream_t st) {
  // x2, r, a quarter of e read; z written (+ compact coefficients of a per-sample matrix); xin == NULL: x2 = 0, not read
  diffhe::account(((xin ? 13.0 : 9.0) + (Bv == 1 ? 0.0 : 4.0 + 2.0 * (L.nd - 1))) * (double)L.n * Bp);
  const dim3 grid(g.ncb * g.nrc, Bp / (spl * kWave));
#define FPOST(VT_, ND_, DOT_, SH_, XZ_)                                                                                      \
  hipLaunchKernelGGL((fused_post_kernel<VT_, ND_, 4, DOT_, SH_, XZ_>), grid, dim3(256), 0, st, L, scale, xin, rhs, ec,         \
                     z, (float)wA, (float)wB, C.W, part, Bp, g.ncb, g.TR)
#define FPOSTD(VT_, ND_, SH_)                                                                                              \
  do {                                                                                                                     \
    if (!xin) FPOST(VT_, ND_, false, SH_, true);                                                                          \
    else if (part) FPOST(VT_, ND_, true, SH_, false);                                                                     \
    else FPOST(VT_, ND_, false, SH_, false);                                                                              \
  } while (0)
  // per-sample coefficients: the POST pass needs 173 VGPRs uncapped (176 allocated: 2 waves per SIMD); capped at 168 it runs
  // 3 waves per SIMD without spills: 218.1 -> 213.5 ms per 1024^2 x 256 step of the per-element-field workload; the PRE pass
  // (206 VGPRs) spills under the same cap: 248.9 ms (run r4e)
  if (Bv != 1 && L.nd == 3) {
#define FPOSTM(DOT_, XZ_)                                                                                                  \
  hipLaunchKernelGGL((fused_post_kernel<v2f, 3, 4, DOT_, false, XZ_, 4, 3>), grid, dim3(256), 0, st, L, scale, xin,         \
                     rhs, ec, z, (float)wA, (float)wB, C.W, part, Bp, g.ncb, g.TR)
    if (!xin) FPOSTM(false, true); else if (part) FPOSTM(true, false); else FPOSTM(false, false);
#undef FPOSTM
  }
  else if (Bv != 1) FPOSTD(v2f, 4, false);
  else if (spl >= 2) { if (L.nd == 3) FPOSTD(v2f, 3, true); else FPOSTD(v2f, 4, true); }
  else { if (L.nd == 3) FPOSTD(float, 3, true); else FPOSTD(float, 4, true); }
#undef FPOSTD
#undef FPOST
}

}  // namespace diffhe_lattice
