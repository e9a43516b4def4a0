// Lattice strip kernels, one sample per lane, any storage type: strip_body, dia_strip_kernel, dia_strip_shift_kernel and
// the definition of their launcher (lattice.h has the strip / window / fusion vocabulary).  Included by the two units
// that instantiate it, lattice_strip_f32.hip (fp32-stored vectors) and lattice_strip_f64.hip (fp64), and by nothing else.
#pragma once
#include <stdlib.h>

#include "lattice.h"

// ---------------------------------------------------------------------------------------------
// Strip kernels: the same three stencil operations with register-level reuse.
//
// A wave owns RW consecutive grid COLUMNS x 64 samples (lanes) and marches down the rows of its
// tile keeping a 3-row window of x in registers: every x value is loaded once per wave (plus
// the 2 halo columns per strip, (RW+2)/RW loads per output) instead of once per stencil leg;
// the 4 waves of a block own 4 adjacent strips, so halo columns hit L1/L2.  Along a row the
// coefficients of a strip are CONTIGUOUS, so with a batch-shared matrix (Bv == 1) they arrive
// as scalar loads off one SGPR base per diagonal -- no per-lane traffic at all.
//
// Invariant relied upon (and kept by every kernel of the solver): all vectors vanish on
// Dirichlet rows, whose matrix rows are identity rows.  It lets the per-sample scale s_b be
// applied to every row without looking up the Dirichlet flag (0 * s_b == 0).
// ---------------------------------------------------------------------------------------------

namespace diffhe_lattice __attribute__((visibility("hidden"))) {
namespace {

template <bool STORED, typename TV> struct WindowType { typedef double type; };
template <typename TV> struct WindowType<true, TV> { typedef TV type; };

template <typename TV, typename TA, typename TM, int MODE, int FUSE, int ND, bool SHARED, bool XFROMB, int RW,
          bool TAIL, bool SHIFT = false>
__device__ __forceinline__ double strip_body(const Level& L, double sb, const TV* __restrict__ src,
                                             const TV* __restrict__ bvec, TV* __restrict__ out, double omega,
                                             double omega_in, const Extra& ex, int Bp, int b, int c0w, int r0,
                                             int r1, double& s2) {
  const int W = L.W, nyp = L.ny + 1;
  const i64 n = L.n;
  const i64 Bv = SHARED ? 1 : Bp;
  // Addressing discipline: every pointer below is WAVE-UNIFORM (lives in SGPRs) and the lane's
  // sample index is added last as a 32-bit offset, so loads/stores use the "SGPR base + VGPR
  // offset" form and the kernel needs one address VGPR instead of one 64-bit pair per stream.
  const unsigned lb = (unsigned)b;            // lane offset into (.., Bp) vectors
  const unsigned lv = SHARED ? 0u : (unsigned)b;  // lane offset into the matrix values
  double s = 0.0;

  // Column offsets of the window (q <-> grid column c0w - 1 + q) and of the strip (k <-> c0w + k),
  // relative to column c0w.  The first strip's left halo and the columns past the right edge are clamped (both
  // only in the TAIL instantiation, which every edge strip takes); their window values are forced to 0.
  int dq[RW + 2];
  bool okq[RW + 2];
#pragma unroll
  for (int q = 0; q < RW + 2; ++q) {
    int c = c0w - 1 + q;
    okq[q] = c >= 0 && (!TAIL || c < W);
    if (c < 0) c = 0;
    if (TAIL && c > W - 1) c = W - 1;
    dq[q] = c - c0w;
  }
  // D_k[i] lives at V[(k*n + i)*Bv + vb].  Row r0 - 1 of D_2 / D_3 is read for the south couplings also when r0 == 0:
  // that is the tail of the previous diagonal in the same array (finite, multiplied by a window value of 0).  Nothing is
  // read in front of an array: the east coupling of column c0w - 1 is an in-grid entry for every non-TAIL strip.
  const i64 i0 = (i64)r0 * W + c0w;          // node (r0, c0w)
  typedef typename MatTypes<TM>::diag TD;
  typedef typename MatTypes<TM>::off TO;
  constexpr bool kSplit = sizeof(TO) == 2;   // h16m: diagonal in L.v32, off-diagonals in L.o16 (times 1 / L.osc[b])
  const double osc = kSplit ? L.osc[b] : 1.0;
  const TD* __restrict__ p0 = (sizeof(TD) == 4 ? (const TD*)L.v32 : (const TD*)L.v) + i0 * Bv;
  const TO* __restrict__ p1 = kSplit ? (const TO*)L.o16 + i0 * Bv : (const TO*)(const void*)(p0 + n * Bv);
  const TO* __restrict__ p2 = p1 + n * Bv;
  const TO* __restrict__ p3 = p2 + n * Bv;
  const double* __restrict__ psh = SHIFT ? L.shift + i0 : nullptr;   // diagonal shift at (row, c0w): wave-uniform loads
  // M_RESID, F_PROLONG: the residual of the prolonged coarse iterate itself -- there is no x operand (lattice.h)
  constexpr bool kProlongOnly = MODE == M_RESID && FUSE == F_PROLONG;
  const TV* __restrict__ px = kProlongOnly ? nullptr : src + i0 * Bp;
  TV* __restrict__ pxo = kProlongOnly ? (TV*)ex.p_out + i0 * Bp : nullptr;   // ... and the strip stores that iterate
  const TV* __restrict__ pb = bvec ? bvec + i0 * Bp : nullptr;
  TV* __restrict__ po = (out && FUSE != F_RESTRICT) ? out + i0 * Bp : nullptr;
  const i64 rowV = (i64)W * Bv, rowX = (i64)W * Bp;

  const double inv_omega_in = XFROMB ? 1.0 / omega_in : 0.0;
  const double sub_fac = (MODE == M_APPLY && FUSE == F_NONE && ex.sub && ex.sub_scale) ? ex.sub_scale[b] : 1.0;
  const double rsc = (plain_resid(MODE, FUSE) && ex.r32 && ex.rscale) ? ex.rscale[b] : 1.0;
  const double beta = (is_pupd(FUSE) && !ex.first) ? ex.beta[b] : 0.0;
  const double alpha_prev = (FUSE == F_PUPD && !ex.first && ex.x) ? ex.alpha[b] : 0.0;  // alpha is NULL when x is
  const TA* __restrict__ aux = (const TA*)ex.a0;
  // F_PUPD row pointers at (row, c0w), advanced with the others
  const TA* __restrict__ pz = (is_pupd(FUSE)) ? aux + i0 * Bp : nullptr;
  constexpr bool kRupd = MODE == M_APPLY && is_rupd(FUSE);   // residual update: fp64 r (F_RUPD) or the pair's forms (is_rpair)
  constexpr bool kRdLo = rupd_reads_lo(FUSE), kWrLo = rupd_writes_lo(FUSE);
  const TA* __restrict__ ppi = (is_pupd(FUSE) || kRupd) ? (const TA*)ex.p_in + i0 * Bp : nullptr;
  double* __restrict__ pr = (FUSE == F_RUPD) ? ex.x + i0 * Bp : nullptr;          // F_RUPD: ex.x is the residual r
  float* __restrict__ pr32 = (kRupd && ex.r32) ? ex.r32 + i0 * Bp : nullptr;     // is_rpair: the high parts (never NULL)
  float* __restrict__ plo = (kRupd && kRdLo) ? ex.rlo + i0 * Bp : nullptr;
  const double alpha_cur = kRupd ? ex.alpha[b] : 0.0;
  const double rsc_u = (kRupd && ex.r32 && ex.rscale) ? ex.rscale[b] : 1.0;
  const double ralpha = rsc_u * alpha_cur, inv_rsc_u = 1.0 / rsc_u;   // is_rpair; rsc_u is a power of two: both exact
  TA* __restrict__ ppo = (is_pupd(FUSE)) ? (TA*)ex.p_out + i0 * Bp : nullptr;
  double* __restrict__ pxx = (FUSE == F_PUPD && ex.x) ? ex.x + i0 * Bp : nullptr;  // NULL: the iterate is not touched

  // The prolongation + residual pass of the full-multigrid start (kProlongOnly) CARRIES the coarse rows under its window
  // from one window row to the next (the rows arrive in order, rw0 first).  cea is coarse row `row >> 1`; an odd row
  // 2k + 1 loads coarse row k + 1 into ceb, and the even row after it takes that over as its cea: every coarse row is
  // loaded once per tile (plus the one the tile starts on), as stored (TA; widened at use, which is exact).  Coarse
  // columns c0w/2 - 1 + j, clamped to the coarse row.  The M_JACOBI form keeps the per-row loads: carrying costs it a
  // wave per SIMD (78 -> 89, 87 -> 108 VGPRs).
  constexpr int NC = RW / 2 + 2;
  // window values: fp64, except where they ARE stored values (kProlongOnly: the prolonged iterate as TV) -- held as such
  // and widened at use, which is exact and leaves the registers to the carried rows
  typedef typename WindowType<kProlongOnly, TV>::type WT;
  TA cea[NC], ceb[NC];
  int cjq[NC];
  const int rw0 = r0 > 0 ? r0 - 1 : r0;      // first row the window loads
  // ... and fetches the Dirichlet flags of a window row once: lane q < RW + 2 loads the flag of window column q (clamped
  // as dq), a ballot turns them into a wave-uniform bit mask -- one byte load per row instead of one per window value
  const int lane = (int)(lb & 63u);
  int bcol = c0w - 1 + (lane < RW + 2 ? lane : RW + 1);
  bcol = bcol < 0 ? 0 : (bcol > W - 1 ? W - 1 : bcol);
  if (FUSE == F_PROLONG) {
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      int cj = (c0w >> 1) - 1 + j;
      cjq[j] = cj < 0 ? 0 : (cj > ex.cW - 1 ? ex.cW - 1 : cj);
      if (kProlongOnly) cea[j] = ceb[j] = (aux + ((i64)(rw0 >> 1) * ex.cW + cjq[j]) * Bp)[lb];
    }
  }

  // `row` is the grid row being loaded; xrow / d0row point at (row, c0w); roff = offset of that
  // row from the current one in vector elements
  auto load_window = [&](int row, i64 roff, const TV* __restrict__ xrow, const TD* __restrict__ d0row,
                         WT* dst, const double* __restrict__ shrow = nullptr) __attribute__((always_inline)) {
    double ce[NC], ce2[NC];
    unsigned long long dir = 0;   // kProlongOnly, bit q: window column q is a Dirichlet node of this row
    if (kProlongOnly) {
      dir = __ballot(ex.bc[(i64)row * W + bcol] != 0);
      const bool odd = row & 1;
      if (odd) {
#pragma unroll
        for (int j = 0; j < NC; ++j) ceb[j] = (aux + ((i64)((row >> 1) + 1) * ex.cW + cjq[j]) * Bp)[lb];
      }
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        cea[j] = odd ? cea[j] : ceb[j];   // even row: the row its predecessor loaded (rw0 even: the primed one)
        ce[j] = (double)cea[j];
        ce2[j] = odd ? (double)ceb[j] : 0.0;
      }
    } else if (FUSE == F_PROLONG) {  // coarse values around this strip
      const int cr = row >> 1;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        ce[j] = (double)(aux + ((i64)cr * ex.cW + cjq[j]) * Bp)[lb];
        ce2[j] = (row & 1) ? (double)(aux + ((i64)(cr + 1) * ex.cW + cjq[j]) * Bp)[lb] : 0.0;
      }
    }
#pragma unroll
    for (int q = 0; q < RW + 2; ++q) {
      double v;
      if (is_pupd(FUSE)) {
        const i64 o = roff + (i64)dq[q] * Bp;
        v = (double)(pz + o)[lb];
        if (!ex.first) v += beta * (double)(ppi + o)[lb];
        // the direction is STORED as TA: use the stored (rounded) value everywhere, so that Ap = A p,
        // x += alpha p and r -= alpha Ap stay exactly consistent (r == b - A x is independent of p)
        v = (double)(TA)v;
      } else if (kRupd) {
        v = (double)(ppi + roff + (i64)dq[q] * Bp)[lb];
      } else if (kProlongOnly) {
        v = 0.0;
      } else {
        v = (double)(xrow + (i64)dq[q] * Bp)[lb];
      }
      if (XFROMB) v = omega_in * v * fast_rcp(sb * ldc(d0row + (i64)dq[q] * Bv, lv) + (SHIFT ? shrow[dq[q]] : 0.0));
      if (FUSE == F_PROLONG) {
        double corr;  // c0w is even: window column q has the parity of q + 1
        if (q & 1)
          corr = (row & 1) ? 0.5 * (ce[(q - 1) / 2 + 1] + ce2[(q - 1) / 2 + 1]) : ce[(q - 1) / 2 + 1];
        else
          corr = (row & 1) ? 0.5 * (ce[q / 2 + 1] + ce2[q / 2]) : 0.5 * (ce[q / 2] + ce[q / 2 + 1]);
        if (kProlongOnly ? (bool)((dir >> q) & 1) : (bool)ex.bc[(i64)row * W + c0w + dq[q]]) corr = 0.0;
        if (kProlongOnly) v = (double)(TV)corr;   // the STORED value of the transfer kernels: the pass reads what they wrote
        else v += corr;
      }
      dst[q] = (WT)(okq[q] ? v : 0.0);
    }
  };

  WT xm[RW + 2], xc[RW + 2], xp[RW + 2];
  double n2p[RW], d3p[RW + 1];
#pragma unroll
  for (int q = 0; q < RW + 2; ++q) xm[q] = 0.0;
  if (r0 > 0) load_window(r0 - 1, -rowX, px - rowX, p0 - rowV, xm, SHIFT ? psh - W : nullptr);
  load_window(r0, 0, px, p0, xc, psh);
#pragma unroll
  for (int k = 0; k < RW; ++k) n2p[k] = kSplit ? osc * ldc(p2 - rowV + (i64)dq[k + 1] * Bv, lv) : ldc(p2 - rowV + (i64)dq[k + 1] * Bv, lv);
#pragma unroll
  for (int k = 0; k < RW + 1; ++k)
    d3p[k] = (ND == 4) ? (kSplit ? osc * ldc(p3 - rowV + (i64)dq[k + 1] * Bv, lv) : ldc(p3 - rowV + (i64)dq[k + 1] * Bv, lv)) : 0.0;

  constexpr int CWR = (FUSE == F_RESTRICT) ? (RW - 1) / 2 : 1;  // coarse columns of an F_RESTRICT strip
  double racc[CWR], rnext[CWR];
#pragma unroll
  for (int j = 0; j < CWR; ++j) racc[j] = rnext[j] = 0.0;
  const int cI0 = (r0 + 1) >> 1, cJ0 = (c0w + 1) >> 1;          // F_RESTRICT: first coarse row / column

  for (int row = r0; row < r1; ++row) {
    if (row + 1 < nyp) {
      load_window(row + 1, rowX, px + rowX, p0 + rowV, xp, SHIFT ? psh + W : nullptr);
    } else {
#pragma unroll
      for (int q = 0; q < RW + 2; ++q) xp[q] = 0.0;
    }
    double d0[RW], e1[RW + 1], n2c[RW], d3c[RW + 1];
    double resrow[(FUSE == F_RESTRICT) ? RW : 1];
    if (FUSE == F_RESTRICT) {
#pragma unroll
      for (int k = 0; k < RW; ++k) resrow[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      d0[k] = ldc(p0 + (i64)dq[k + 1] * Bv, lv);
      n2c[k] = kSplit ? osc * ldc(p2 + (i64)dq[k + 1] * Bv, lv) : ldc(p2 + (i64)dq[k + 1] * Bv, lv);
    }
#pragma unroll
    for (int k = 0; k < RW + 1; ++k) {
      // east coupling of column c0w - 1 + k (interior strips: c0w >= RW, the column exists; edge strips: clamped)
      const int dc = TAIL ? dq[k] : k - 1;
      e1[k] = kSplit ? osc * ldc(p1 + (i64)dc * Bv, lv) : ldc(p1 + (i64)dc * Bv, lv);
      d3c[k] = (ND == 4) ? (kSplit ? osc * ldc(p3 + (i64)dq[k + 1] * Bv, lv) : ldc(p3 + (i64)dq[k + 1] * Bv, lv)) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      const int q = k + 1;
      if (TAIL && (c0w + k >= W || c0w + k < 0)) continue;
      double acc = d0[k] * xc[q];
      acc += e1[k + 1] * xc[q + 1] + e1[k] * xc[q - 1];
      acc += n2c[k] * xp[q] + n2p[k] * xm[q];
      if (ND == 4) acc += d3c[k] * xp[q - 1] + d3p[k + 1] * xm[q + 1];
      const i64 o = (i64)k * Bp;
      const double sh = SHIFT ? psh[dq[k + 1]] : 0.0;   // A = sb K + diag(shift)
      const double diag = SHIFT ? sb * d0[k] + sh : sb * d0[k];
      const double Ax = SHIFT ? sb * acc + sh * xc[q] : sb * acc;
      if (MODE == M_APPLY && is_rpair(FUSE)) {
        // R = rs r as hi + lo: hi is the V-cycle's input (left cacheable), lo is touched here only (nontemporal, as
        // the fp64 r of F_RUPD) -- read by F_RPAIR and F_RDROP, written by F_RPAIR alone.  r.r is taken from what is
        // STORED, pair or hi: S_CONV judges the residual the solver carries.
        float* ha = &(pr32 + o)[lb];
        float hi = *ha, lo = 0.0f;
        if (kRdLo) lo = __builtin_nontemporal_load(&(plo + o)[lb]);
        const double ri = pair_update<kRdLo, kWrLo>(hi, lo, ralpha * Ax) * inv_rsc_u;
        *ha = hi;
        if (kWrLo) __builtin_nontemporal_store(lo, &(plo + o)[lb]);
        s += ri * ri;
      } else if (MODE == M_APPLY && FUSE == F_RUPD) {
        double* ra = &(pr + o)[lb];
        const double ri = __builtin_nontemporal_load(ra) - alpha_cur * Ax;
        __builtin_nontemporal_store(ri, ra);
        if (pr32) (pr32 + o)[lb] = (float)(ri * rsc_u);   // read again right away by the V-cycle: left cacheable
        s += ri * ri;
      } else if (MODE == M_APPLY) {
        double y = Ax;
        if (FUSE == F_NONE && (ex.sub || ex.mask)) {  // load vector of a lattice mesh: F = M f - lift, 0 on Dirichlet rows
          const i64 ig = (i64)row * W + c0w + k;
          if (ex.sub) y -= sub_fac * (ex.sub_pb ? (ex.sub + ig * Bp)[lb] : ex.sub[ig]);
          if (ex.mask && ex.mask[ig]) y = 0.0;
        }
        if (po) {
          // CG-step streams (Ap, p, x) are touched once per iteration, 1-2 GB each: nontemporal accesses keep them
          // from evicting the halo columns and the V-cycle's vectors from L2 / Infinity Cache (fused step -4 %)
          if (is_pupd(FUSE)) __builtin_nontemporal_store((TV)y, &(po + o)[lb]);
          else (po + o)[lb] = (TV)y;
        }
        if (FUSE == F_NONE && ex.dotv) {  // bilinear form lam^T (A x + add): dL/dkappa of a factored operator
          const i64 ig = (i64)row * W + c0w + k;
          s += (y + (ex.addv ? ex.addv[ig] : 0.0)) * (ex.dotv + ig * Bp)[lb];
        } else {
          s += y * xc[q];
        }
        if (is_pupd(FUSE)) {  // store the new direction; apply the pending x += alpha_prev * p_old
          __builtin_nontemporal_store((TA)xc[q], &(ppo + o)[lb]);
          if (FUSE == F_PUPD && !ex.first && pxx) {
            double* xa_ = &(pxx + o)[lb];
            __builtin_nontemporal_store(__builtin_nontemporal_load(xa_) + alpha_prev * (double)(ppi + o)[lb], xa_);
          }
        }
      } else {
        const double dinv = (MODE == M_JACOBI) ? fast_rcp(diag) : 0.0;
        // XFROMB: the window holds x1 = omega_in * rhs * dinv, so rhs = x1 / (omega_in * dinv)
        const double bi = XFROMB ? xc[q] * diag * inv_omega_in : (double)(pb + o)[lb];
        const double res = bi - Ax;
        if (MODE == M_RESID && FUSE == F_RESTRICT) {
          resrow[k] = res;
        } else if (MODE == M_RESID) {
          if (FUSE == F_RPAIR) {   // the residual as a pair only (po is NULL)
            const i64 ig = ((i64)row * W + c0w + k) * Bp;
            float hi, lo;
            split(res * rsc, hi, lo);
            (ex.r32 + ig)[lb] = hi;
            __builtin_nontemporal_store(lo, &(ex.rlo + ig)[lb]);
          }
          if (kProlongOnly) (pxo + o)[lb] = (TV)xc[q];
          if (po) (po + o)[lb] = (TV)res;
          if (FUSE == F_NONE && sizeof(TV) == 8 && ex.r32) (ex.r32 + ((i64)row * W + c0w + k) * Bp)[lb] = (float)(res * rsc);
          if (plain_resid(MODE, FUSE) && ex.dot_bx) {
            s += bi * xc[q];
            s2 += xc[q] * (bi - res);   // x.(A x)
          } else {
            s += res * res;
          }
        } else {
          const double xo = xc[q] + omega * res * dinv;
          (po + o)[lb] = (TV)xo;
          s += bi * xo;
        }
      }
    }
    if (FUSE == F_RESTRICT) {
      // strip column k <-> fine column 2 cJ0 - 1 + k, so coarse column cJ0 + j sits at k = 2 j + 1.
      // Full weighting of the P1 lattice: centre 1; W, E, N, S, NE-of-the-row-above, SW-of-the-row-below 1/2.
      const bool store = (row & 1) || row + 1 >= nyp;  // coarse row complete after its odd row (or at the last row)
      if (!(row & 1)) {
#pragma unroll
        for (int j = 0; j < CWR; ++j) racc[j] += resrow[2 * j + 1] + 0.5 * (resrow[2 * j] + resrow[2 * j + 2]);
      } else {
#pragma unroll
        for (int j = 0; j < CWR; ++j) {
          racc[j] += 0.5 * (resrow[2 * j + 1] + resrow[2 * j]);
          rnext[j] = 0.5 * (resrow[2 * j + 1] + resrow[2 * j + 2]);
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
              (out + Ic * Bp)[lb] = (TV)(ex.bc[Ic] ? 0.0 : racc[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < CWR; ++j) {
          racc[j] = rnext[j];
          rnext[j] = 0.0;
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
    p0 += rowV; p1 += rowV; p2 += rowV; p3 += rowV;
    if (SHIFT) psh += W;
    if (!kProlongOnly) px += rowX;
    else pxo += rowX;
    if (pb) pb += rowX;
    if (po) po += rowX;
    if (is_pupd(FUSE)) { pz += rowX; ppi += rowX; ppo += rowX; if (FUSE == F_PUPD && pxx) pxx += rowX; }
    if (kRupd) { ppi += rowX; if (pr) pr += rowX; if (pr32) pr32 += rowX; if (plo) plo += rowX; }
  }
  return s;
}

// Body of the strip kernels: tile -> (column strip, row chunk) of this wave, the strip march, the per-sample partials.
// One call level below the __global__ functions on purpose: written directly into the kernel the same code gets a
// different register allocation for the batch-shared (SHARED) fp64 variants -- 72 VGPRs + 60 B of scratch instead of
// 62 for the fused CG step, 141-148 instead of 75-95 for the fp64 residual / apply strips -- and the step measures
// 2 % slower that way (A/B on one MI355X, 1024^2 x 256: 116.1 vs 113.9 ms; fused CG step 1.20 vs 1.17 ms; only the
// fp64-stored Jacobi sweep of mg fp32=0 prefers the direct form, 1.27 vs 1.31 ms).
template <typename TV, typename TA, typename TM, int MODE, int FUSE, int ND, bool SHARED, bool XFROMB, int RW, bool SHIFT>
__device__ __forceinline__ void strip_kernel_body(Level L, const double* __restrict__ scale,
                                                  const TV* __restrict__ xin, const TV* __restrict__ bvec,
                                                  TV* __restrict__ out, double omega, double omega_in, Extra ex,
                                                  double* __restrict__ part, int Bp, int ncb, int TR) {
  __shared__ double lds[4 * kWave];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y * kWave + lane;
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
  const double sb = scale ? scale[b] : 1.0;
  const TV* __restrict__ src = XFROMB ? bvec : xin;
  double s = 0.0, s2 = 0.0;
  if (active) {
    // strips that touch the left or right edge take the clamped body -- the first strip (c0w == 0) too: its window column
    // -1 would otherwise read the east coupling one element BEFORE the row, which for row 0 lies in front of the array
    if (c0w + RW + 1 > L.W || c0w <= 0)
      s = strip_body<TV, TA, TM, MODE, FUSE, ND, SHARED, XFROMB, RW, true, SHIFT>(L, sb, src, bvec, out, omega, omega_in, ex,
                                                                              Bp, b, c0w, r0, r1, s2);
    else
      s = strip_body<TV, TA, TM, MODE, FUSE, ND, SHARED, XFROMB, RW, false, SHIFT>(L, sb, src, bvec, out, omega, omega_in, ex,
                                                                               Bp, b, c0w, r0, r1, s2);
  }
  if (part) {
    const double t = block_sum_per_sample(s, Bp, lds);
    if (wave == 0) part[(i64)blockIdx.x * Bp + b] = t;
  }
  if (plain_resid(MODE, FUSE) && ex.part2) {
    const double t = block_sum_per_sample(s2, Bp, lds);
    if (wave == 0) ex.part2[(i64)blockIdx.x * Bp + b] = t;
  }
}

template <typename TV, typename TA, typename TM, int MODE, int FUSE, int ND, bool SHARED, bool XFROMB, int RW,
          int MINW = 1>
__global__ __launch_bounds__(256, MINW) void dia_strip_kernel(Level L, const double* __restrict__ scale,
                                                         const TV* __restrict__ xin, const TV* __restrict__ bvec,
                                                         TV* __restrict__ out, double omega, double omega_in,
                                                         Extra ex, double* __restrict__ part, int Bp, int ncb,
                                                         int TR) {
  strip_kernel_body<TV, TA, TM, MODE, FUSE, ND, SHARED, XFROMB, RW, false>(L, scale, xin, bvec, out, omega, omega_in, ex, part,
                                                                          Bp, ncb, TR);
}

// The same strips for a FACTORED operator with a batch-shared diagonal shift, A_b = scale_b K_1 + diag(L.shift)
// (reaction term / heat-equation steps with one scalar kappa per sample): coefficients stay scalar loads.
template <typename TV, typename TA, int MODE, int FUSE, int ND, bool XFROMB, int RW, int MINW = 1>
__global__ __launch_bounds__(256, MINW) void dia_strip_shift_kernel(Level L, const double* __restrict__ scale,
                                                               const TV* __restrict__ xin, const TV* __restrict__ bvec,
                                                               TV* __restrict__ out, double omega, double omega_in,
                                                               Extra ex, double* __restrict__ part, int Bp, int ncb,
                                                               int TR) {
  strip_kernel_body<TV, TA, double, MODE, FUSE, ND, true, XFROMB, RW, true>(L, scale, xin, bvec, out, omega, omega_in, ex, part,
                                                                           Bp, ncb, TR);
}


}  // namespace

template <typename TV, int MODE, bool XFROMB, int FUSE, typename TA, int RW, int MINW, int MATS>
void launch_strip(const Level& L, int Bv, const double* scale, const TV* xin, const TV* bvec, TV* out,
                  double omega, double omega_in, double* part, int Bp, const StripGeom& g, hipStream_t st,
                  const Extra& ex) {
  dim3 grid(g.ncb * g.nrc, Bp / kWave);
  // per-sample matrices inside the fp32 V-cycle read the fp32 copy of the coefficients
  const bool m32 = (sizeof(TV) == 4) && Bv != 1 && L.v32 != nullptr;
  const bool m16 = m32 && L.o16 != nullptr;   // fp32 diagonal + fp16 off-diagonals
  {  // algorithmic bytes per (node, sample) of this launch (diffhe_traffic_account)
    const double tv = sizeof(TV), ta = sizeof(TA);
    double bpn;
    if (MODE == M_JACOBI) bpn = (XFROMB ? 2.0 : 3.0) * tv + (FUSE == F_PROLONG ? 0.25 * tv : 0.0);
    else if (MODE == M_RESID && FUSE == F_PROLONG) {   // rhs read, P e and the residual written; the coarse vector read once
      bpn = 2.0 * tv + (out ? tv : 0.0);
      diffhe::account(tv * (double)ex.cW * (L.ny / 2 + 1) * Bp);
    }
    else if (MODE == M_RESID) bpn = 2.0 * tv + (FUSE == F_RESTRICT ? 0.25 * tv : (out ? tv : 0.0) + (ex.r32 ? 4.0 : 0.0) + (FUSE == F_RPAIR ? 4.0 : 0.0));
    else if (is_pupd(FUSE)) bpn = (ex.first ? 2.0 * ta : 3.0 * ta) + (out ? 8.0 : 0.0) + ((FUSE == F_PUPD && ex.x) ? 16.0 : 0.0);
    else if (FUSE == F_RUPD) bpn = ta + 16.0 + (ex.r32 ? 4.0 : 0.0);   // p; r read and written; its fp32 copy
    else if (is_rpair(FUSE))   // p; hi read and written; lo read (F_RPAIR, F_RDROP) and written (F_RPAIR): 20, 16, 12 B
      bpn = ta + 8.0 + (rupd_reads_lo(FUSE) ? 4.0 : 0.0) + (rupd_writes_lo(FUSE) ? 4.0 : 0.0);
    else bpn = tv + (out ? tv : 0.0) + (ex.dotv ? 8.0 : 0.0);
    if (Bv != 1) bpn += m16 ? 4.0 + 2.0 * (L.nd - 1) : L.nd * (m32 ? 4.0 : 8.0);
    diffhe::account(bpn * (double)L.n * Bp);
  }
#define STRIP(ND_, SH_, TM_)                                                                                       \
  hipLaunchKernelGGL((dia_strip_kernel<TV, TA, TM_, MODE, FUSE, ND_, SH_, XFROMB, RW, MINW>), grid, dim3(256), 0, st, L,   \
                     scale, xin, bvec, out, omega, omega_in, ex, part, Bp, g.ncb, g.TR)
#define STRIP_SHIFT(ND_)                                                                                           \
  hipLaunchKernelGGL((dia_strip_shift_kernel<TV, TA, MODE, FUSE, ND_, XFROMB, RW, MINW>), grid, dim3(256), 0, st, L, scale, \
                     xin, bvec, out, omega, omega_in, ex, part, Bp, g.ncb, g.TR)
  // fp32 / fp16 coefficient copies only in a cycle with fp32 vectors (m32): other instantiations could never launch
#define STRIP_ND(ND_)                                                                                              \
  do {                                                                                                             \
    if constexpr (sizeof(TV) == 4) {                                                                               \
      if (m16) STRIP(ND_, false, h16m); else if (m32) STRIP(ND_, false, float); else STRIP(ND_, false, double);   \
    } else STRIP(ND_, false, double);                                                                              \
  } while (0)
  if (Bv == 1) {
    if constexpr (MATS != MAT_PER_SAMPLE) {
      if (L.shift) {
        if (L.nd == 3) STRIP_SHIFT(3); else STRIP_SHIFT(4);
      } else {
        if (L.nd == 3) STRIP(3, true, double); else STRIP(4, true, double);
      }
    } else abort();   // a call site narrowed to per-sample matrices met a batch-shared one
  } else if constexpr (MATS != MAT_SHARED) {
    if (L.nd == 3) STRIP_ND(3); else STRIP_ND(4);
  } else abort();     // a call site narrowed to batch-shared matrices met per-sample ones
#undef STRIP_ND
#undef STRIP
#undef STRIP_SHIFT
}

}  // namespace diffhe_lattice
