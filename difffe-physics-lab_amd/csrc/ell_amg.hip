// General path, aggregation multigrid (diffhe/amg.py builds the batch-shared hierarchy): the sweep kernels, restriction
// and prolongation, the dense last level, the cycle, and the multigrid-PCG entries (the PCG itself: ell_pcg.hip).
#include "ell.h"

namespace {
using namespace diffhe_ell;

// weighted Jacobi: xout = xin + omega (b - A xin) / D (xin == NULL: from zero); optional partial of b.xout.
// TV = storage type of the cycle's vectors, TM = storage type of the matrix values (fp32 copies inside a
// single-precision preconditioner); arithmetic is fp64 in registers.
template <typename TV, typename TM>
__global__ __launch_bounds__(256, 8) void ell_jacobi_kernel(const TM* __restrict__ vals, const int* __restrict__ cols,
                                                          const TV* __restrict__ bvec, const TV* __restrict__ xin,
                                                          TV* __restrict__ xout, double omega,
                                                          double* __restrict__ part, int n, int W, int Bp, int Bv) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < Bp;
  const int vb = Bv == 1 ? 0 : nm.b;
  double s = 0.0;
  if (ok)
    FOR_EACH_NODE(nm, n, Bp, Bv, {
      const i64 o = (i64)i * Bp + nm.b;
      const double d = (double)vals[(i64)i * Bv + vb];
      const double bi = (double)bvec[o];
      double xo;
      if (xin) {
        const double xs = (double)xin[o];    // issued with the row's first loads, not behind its last product
        const double acc = ell_row<true, kUni, kShared>(bi, vals, cols, xin, i, n, W, Bp, Bv, nm.b);
        xo = xs + omega * acc / d;
      } else {
        xo = omega * bi / d;
      }
      xout[o] = (TV)xo;
      s += bi * xo;
    });
  if (part) store_block_partial(s, part, Bp, nm.b, ok, lds);
}

template <typename TV, typename TM>
__global__ __launch_bounds__(256, 8) void ell_residual_out_kernel(const TM* __restrict__ vals, const int* __restrict__ cols,
                                                                const TV* __restrict__ bvec, const TV* __restrict__ x,
                                                                TV* __restrict__ r, int n, int W, int Bp, int Bv) {
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  FOR_EACH_NODE(nm, n, Bp, Bv, {
    r[(i64)i * Bp + nm.b] = (TV)ell_row<true, kUni, kShared>((double)bvec[(i64)i * Bp + nm.b], vals, cols, x, i, n, W, Bp, Bv, nm.b);
  });
}

// rc = P^T r: rc[I] = sum over the members c of coarse node I (fixed order) of w_c r[member_c]; w == NULL: 1
// (piecewise-constant aggregation: the plain sum over the aggregate)
template <typename TV>
__global__ __launch_bounds__(256) void agg_restrict_kernel(const TV* __restrict__ r, const int* __restrict__ agg_ptr,
                                                            const int* __restrict__ members,
                                                            const double* __restrict__ w, TV* __restrict__ rc,
                                                            int nc, int Bp) {
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  if (Bp >= kWave) {
    // a wave = one coarse node: 64 member indices (and weights) per vector load, handed out by v_readlane, the gathers
    // of 8 members in flight together -- the plain loop below waited twice per member (33-40 us on levels of a few
    // hundred coarse nodes, whose rows of P^T have 30-40 entries).  Same members, same order, same operations.
    const int lane = threadIdx.x & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int I = (int)blockIdx.x * 4 + wave_u; I < nc; I += (int)gridDim.x * 4) {
      const int beg = agg_ptr[I], end = agg_ptr[I + 1];
      double s = 0.0;
      for (int c0 = beg; c0 < end; c0 += kWave) {
        const int nk = end - c0 < kWave ? end - c0 : kWave;
        const int cl = c0 + (lane < nk ? lane : 0);
        const int mv = members[cl];
        const double wv = w ? w[cl] : 1.0;
        for (int u0 = 0; u0 < nk; u0 += 8) {
          double ww[8];
          TV rv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int k = u0 + u < nk ? u0 + u : 0;
            const TV* __restrict__ rr = r + (i64)__builtin_amdgcn_readlane(mv, k) * Bp;
            rv[u] = rr[nm.b];
            ww[u] = w ? readlane_f64(wv, k) : 1.0;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (u0 + u < nk) {
              if (w) s = fma(ww[u], (double)rv[u], s);
              else s += (double)rv[u];
            }
        }
      }
      rc[(i64)I * Bp + nm.b] = (TV)s;
    }
    return;
  }
  for (int I = nm.node0; I < nc; I += nm.stride) {
    double s = 0.0;
    if (w)
      for (int c = agg_ptr[I]; c < agg_ptr[I + 1]; ++c) s = fma(w[c], (double)r[(i64)members[c] * Bp + nm.b], s);
    else
      for (int c = agg_ptr[I]; c < agg_ptr[I + 1]; ++c) s += (double)r[(i64)members[c] * Bp + nm.b];
    rc[(i64)I * Bp + nm.b] = (TV)s;
  }
}

// x += scale * P e for a smoothed prolongation stored as ELL rows: p_cols / p_vals (pw, n), -1 = no entry
template <typename TV>
__global__ __launch_bounds__(256) void sa_prolong_add_kernel(const TV* __restrict__ e, const int* __restrict__ p_cols,
                                                              const double* __restrict__ p_vals, int pw,
                                                              TV* __restrict__ x, double scale, int n, int Bp) {
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  if (Bp >= kWave && pw <= 8) {
    // a wave = one fine node: its row of P in one vector load (lane k: entry k), entries handed out by v_readlane, the
    // gathers of e in flight together with the node's own x.  Same entries, same order, same operations.
    const int lane = threadIdx.x & 63;
    int first, hi, step;
    wave_node_range(n, first, hi, step);
    for (int i = first; i < hi; i += step) {
      const i64 entl = (i64)(lane < pw ? lane : 0) * n + i;
      const int cv = p_cols[entl];
      const double pv = p_vals[entl];
      const i64 o = (i64)i * Bp + nm.b;
      const TV xs = x[o];
      TV ev[8];
      double pp[8];
      int II[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        II[u] = u < pw ? __builtin_amdgcn_readlane(cv, u) : -1;
        pp[u] = readlane_f64(pv, u);
        ev[u] = (TV)0;
        if (II[u] >= 0) {    // wave-uniform: no load for an absent entry
          const TV* __restrict__ er = e + (i64)II[u] * Bp;
          ev[u] = er[nm.b];
        }
      }
      double s = 0.0;
      bool any = false;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (II[u] >= 0) {
          s = fma(pp[u], (double)ev[u], s);
          any = true;
        }
      if (any) x[o] = (TV)((double)xs + scale * s);
    }
    return;
  }
  for (int i = nm.node0; i < n; i += nm.stride) {
    double s = 0.0;
    bool any = false;
    for (int k = 0; k < pw; ++k) {
      const int I = p_cols[(i64)k * n + i];
      if (I >= 0) {
        s = fma(p_vals[(i64)k * n + i], (double)e[(i64)I * Bp + nm.b], s);
        any = true;
      }
    }
    if (any) x[(i64)i * Bp + nm.b] = (TV)((double)x[(i64)i * Bp + nm.b] + scale * s);
  }
}

// x[i] += scale * e[agg[i]]
template <typename TV>
__global__ __launch_bounds__(256) void agg_prolong_add_kernel(const TV* __restrict__ e, const int* __restrict__ agg,
                                                               TV* __restrict__ x, double scale, int n, int Bp) {
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const int I = agg[i];
    if (I >= 0) x[(i64)i * Bp + nm.b] = (TV)((double)x[(i64)i * Bp + nm.b] + scale * (double)e[(i64)I * Bp + nm.b]);
  }
}

// x += alpha p ; r -= alpha Ap ; partial r.r
__global__ __launch_bounds__(256) void amg_update_kernel(const double* __restrict__ p, const double* __restrict__ Ap,
                                                          const double* __restrict__ alpha, double* __restrict__ x,
                                                          double* __restrict__ r, float* __restrict__ r32,
                                                          const double* __restrict__ rs, double* __restrict__ part_rr,
                                                          double* __restrict__ part_xx, int n, int Bp) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < Bp;
  double s = 0.0, sx = 0.0;
  if (ok) {
    const double a = alpha[nm.b];
    const double sc = (r32 && rs) ? rs[nm.b] : 1.0;
    for (int i = nm.node0; i < n; i += nm.stride) {
      const i64 o = (i64)i * Bp + nm.b;
      const double xi = x[o] + a * p[o];
      x[o] = xi;
      const double ri = r[o] - a * Ap[o];
      r[o] = ri;
      if (r32) r32[o] = (float)(ri * sc);
      s += ri * ri;
      sx += xi * xi;
    }
  }
  store_block_partial(s, part_rr, Bp, nm.b, ok, lds);
  if (part_xx) store_block_partial(sx, part_xx, Bp, nm.b, ok, lds);
}

// Per-sample max of the ELL diagonal (slot 0), as the bit pattern of a non-negative double (atomicMax: deterministic)
__global__ __launch_bounds__(256) void ell_maxdiag_kernel(const double* __restrict__ vals, int n, int Bv,
                                                           unsigned long long* __restrict__ out) {
  const NodeMap nm = node_map(Bv);
  double m = 0.0;
  if (nm.b < Bv)
    for (int i = nm.node0; i < n; i += nm.stride) {
      const double d = vals[(i64)i * Bv + nm.b];
      m = d > m ? d : m;
    }
  const int LB = Bv < kWave ? Bv : kWave;
  for (int off = LB; off < kWave; off <<= 1) {
    const double o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  if ((int)(threadIdx.x & 63) < LB && nm.b < Bv) atomicMax(out + nm.b, (unsigned long long)__double_as_longlong(m));
}

// x = 0 ; r = b ; partial b.b
__global__ __launch_bounds__(256) void amg_init_kernel(const double* __restrict__ bvec, double* __restrict__ x,
                                                        double* __restrict__ r, float* __restrict__ r32,
                                                        double* __restrict__ p, double* __restrict__ part_bb, int n,
                                                        int Bp) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < Bp;
  double s = 0.0;
  if (ok)
    for (int i = nm.node0; i < n; i += nm.stride) {
      const i64 o = (i64)i * Bp + nm.b;
      const double bi = bvec[o];
      x[o] = 0.0; r[o] = bi; p[o] = 0.0;
      s += bi * bi;
    }
  store_block_partial(s, part_bb, Bp, nm.b, ok, lds);
}

__global__ __launch_bounds__(256) void amg_cvt_kernel(const double* __restrict__ r, const double* __restrict__ rs,
                                                       float* __restrict__ r32, int n, int Bp) {
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  const double sc = rs[nm.b];
  for (int i = nm.node0; i < n; i += nm.stride) r32[(i64)i * Bp + nm.b] = (float)(r[(i64)i * Bp + nm.b] * sc);
}

// ---------------------------------------------------------------------------------------
// Wave-per-node sweep kernels of the solvers (batches of >= 64), SOFTWARE-PIPELINED: with ell_row_uniform inside a plain
// node loop a wave still paid two dependent memory latencies per node (row meta data -> gathers) for each of its 32
// nodes, which is what the fine-level sweep's 72-87 us were (32 x 2 x ~1.2 us).  Here the next node's meta data
// (column indices, shared values, b_i, own x_i) are requested right behind the current node's gathers, so a node costs
// ONE exposed latency.  Same entries, order and operations as ell_jacobi_kernel / ell_residual_out_kernel /
// cg_spmv_kernel; same node -> (block, wave) assignment, so the block partials are the same sums.
//   W_JACOBI: out = x + omega (b - A x) / D, partial of b.out;  W_RESID: out = b - A x;  W_SPMV: out = A x, partial x.out
// ---------------------------------------------------------------------------------------
enum { W_JACOBI = 0, W_RESID = 1, W_SPMV = 2 };
template <int OP, typename TV, typename TM, bool SHARED>
__global__ __launch_bounds__(256, 8) void ellw_kernel(const TM* __restrict__ vals, const int* __restrict__ cols,
                                                      const TV* __restrict__ bvec, const TV* __restrict__ xin,
                                                      TV* __restrict__ out, double omega, double* __restrict__ part,
                                                      int n, int W, int Bp) {
  __shared__ double lds[4 * kWave];
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.y * kWave + lane;
  int i, hi, step;
  wave_node_range(n, i, hi, step);
  constexpr int NU = SHARED ? 8 : 4;   // per-sample values are vector loads of their own: shorter chunks fit 64 VGPRs
  const int nk0 = W < kWave ? W : kWave;           // entries of the first (normally the only) 64-entry chunk
  const i64 lane_ent = (i64)(lane < nk0 ? lane : 0) * n;
  double s = 0.0;
  int cv = 0;
  double av = 0.0;
  TV bi = (TV)0, xs = (TV)0;
  if (i < hi) {
    cv = cols[lane_ent + i];
    if (SHARED) av = (double)vals[lane_ent + i];
    if (OP != W_SPMV) bi = bvec[(i64)i * Bp + b];
    if (OP != W_RESID) xs = xin[(i64)i * Bp + b];
  }
  while (i < hi) {
    const int inext = i + step;
    double acc = OP == W_SPMV ? 0.0 : (double)bi;
    double d = 1.0;
    int cvn = 0;
    double avn = 0.0;
    TV bin = (TV)0, xsn = (TV)0;
    for (int k0 = 0; k0 < W; k0 += kWave) {
      const int nk = W - k0 < kWave ? W - k0 : kWave;
      if (k0 > 0) {   // rows wider than 64 entries: not pipelined
        const i64 e2 = (i64)(k0 + (lane < nk ? lane : 0)) * n + i;
        cv = cols[e2];
        if (SHARED) av = (double)vals[e2];
      }
      for (int u0 = 0; u0 < nk; u0 += NU) {
        int c[NU];
        double a[NU];
        TV xv[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const bool in = u0 + u < nk;
          const int k = in ? u0 + u : 0;
          c[u] = __builtin_amdgcn_readlane(cv, k);
          if (SHARED) a[u] = in ? readlane_f64(av, k) : 0.0;
        }
        // (no branches around the loads: a wave-uniform `if` per entry made the compiler wait after every gather;
        // an absent entry re-reads entry 0 and gets the value 0)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const TV* __restrict__ xr = xin + (i64)c[u] * Bp;
          xv[u] = xr[b];
        }
        if (!SHARED) {
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            const bool in = u0 + u < nk;
            const TM* __restrict__ vr = vals + ((i64)(k0 + (in ? u0 + u : 0)) * n + i) * Bp;
            const double t = (double)vr[b];
            a[u] = in ? t : 0.0;
          }
        }
        if (k0 == 0 && u0 == 0 && inext < hi) {   // the next node's meta data, behind this node's gathers
          cvn = cols[lane_ent + inext];
          if (SHARED) avn = (double)vals[lane_ent + inext];
          if (OP != W_SPMV) bin = bvec[(i64)inext * Bp + b];
          if (OP != W_RESID) xsn = xin[(i64)inext * Bp + b];
        }
        if (OP == W_JACOBI && k0 == 0 && u0 == 0) d = a[0];   // entry 0 of a row is its diagonal
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          if (OP == W_SPMV) acc += a[u] * (double)xv[u];
          else acc -= a[u] * (double)xv[u];
        }
      }
    }
    const i64 o = (i64)i * Bp + b;
    if (OP == W_JACOBI) {
      const double xo = (double)xs + omega * acc / d;
      out[o] = (TV)xo;
      s += (double)bi * xo;
    } else if (OP == W_RESID) {
      out[o] = (TV)acc;
    } else {
      out[o] = (TV)acc;
      s += acc * (double)xs;
    }
    i = inext;
    cv = cvn; av = avn; bi = bin; xs = xsn;
  }
  if (OP != W_RESID && part) {
    const int wave = threadIdx.x >> 6;
    const double t = block_sum_per_sample(s, Bp, lds);
    if (wave == 0) part[(i64)blockIdx.x * Bp + b] = t;
  }
}
// (A two-samples-per-lane form of ellw_kernel for batch-shared matrices and batches of 128 k -- 8 / 16-byte gathers, the
// node's scalar work paid once per 128 samples -- was built and measured: bitwise the same values, 117.0 -> 116.0 ms per
// solve at jittered 512^2 x 256, gpurun_out/r4bn.  The sweeps are not instruction-bound; removed.)
// The first sweep of a cycle starts from zero: x = omega b / D, an elementwise pass -- four nodes per trip (one node per
// trip left a wave with a single load outstanding: 55 us for 134 MB on the fine level of 512^2 x 64).
template <typename TV, typename TM>
__global__ __launch_bounds__(256) void ellw_jacobi0_kernel(const TM* __restrict__ vals, const TV* __restrict__ bvec,
                                                           TV* __restrict__ xout, double omega, int n, int Bp, int Bv) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.y * kWave + lane;
  const int vb = Bv == 1 ? 0 : b;
  int i, hi, step;
  wave_node_range(n, i, hi, step);
  for (; (i64)i + 3LL * step < hi; i += 4 * step) {
    TV bv[4];
    double d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      bv[u] = bvec[(i64)(i + u * step) * Bp + b];
      d[u] = (double)vals[(i64)(i + u * step) * Bv + vb];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) xout[(i64)(i + u * step) * Bp + b] = (TV)(omega * (double)bv[u] / d[u]);
  }
  for (; i < hi; i += step)
    xout[(i64)i * Bp + b] = (TV)(omega * (double)bvec[(i64)i * Bp + b] / (double)vals[(i64)i * Bv + vb]);
}
// the wave-per-node kernels apply: whole waves of samples, DIFFHE_ELL_PIPE != 0
bool ellw_on(int Bp) {
  const char* env = getenv("DIFFHE_ELL_PIPE");   // read per launch: a test compares both forms in one process
  const int on = env ? atoi(env) : 1;
  return on && Bp >= kWave && Bp % kWave == 0;
}
template <typename TV, typename TM>
int launch_ellw_jacobi0(const TM* vals, const TV* bvec, TV* xout, double omega, int n, int Bp, int Bv, hipStream_t st) {
  if (!ellw_on(Bp)) return 0;
  hipLaunchKernelGGL((ellw_jacobi0_kernel<TV, TM>), diffhe::node_grid(n, Bp), dim3(256), 0, st, vals, bvec, xout, omega, n, Bp, Bv);
  return 1;
}
// launch helper: 1 = launched (ellw_on), 0 = caller takes the plain kernel
template <int OP, typename TV, typename TM>
int launch_ellw(const TM* vals, const int* cols, const TV* bvec, const TV* xin, TV* out, double omega, double* part, int n,
                int W, int Bp, int Bv, hipStream_t st) {
  if (!ellw_on(Bp)) return 0;
  const dim3 grid = diffhe::node_grid(n, Bp);
  if (Bv == 1)
    hipLaunchKernelGGL((ellw_kernel<OP, TV, TM, true>), grid, dim3(256), 0, st, vals, cols, bvec, xin, out, omega, part, n, W, Bp);
  else
    hipLaunchKernelGGL((ellw_kernel<OP, TV, TM, false>), grid, dim3(256), 0, st, vals, cols, bvec, xin, out, omega, part, n, W, Bp);
  return 1;
}

// Last level of a batch-shared hierarchy: x = A^-1 rhs as ONE dense product with the cached inverse (n <= 128; the 16
// Jacobi sweeps it replaces were 16 launch-bound launches per cycle and only an approximate solve).  A block = 64
// samples x 4 rows (one per wave): rhs staged in LDS, a row of the inverse is one vector load.
template <typename TV>
__global__ __launch_bounds__(256) void amg_dense_solve_kernel(const double* __restrict__ inv, const TV* __restrict__ rhs,
                                                               TV* __restrict__ x, int n, int Bp) {
  extern __shared__ double sm[];   // (n, 64)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int b = blockIdx.x * kWave + lane;
  const bool ok = b < Bp;
  for (int j = wave; j < n; j += 4) sm[j * kWave + lane] = ok ? (double)rhs[(i64)j * Bp + b] : 0.0;
  __syncthreads();
  const int i = (int)blockIdx.y * 4 + wave;   // one row per wave, four rows per block: the level spreads over n / 4 CUs
  if (i >= n) return;
  const double* __restrict__ row = inv + (i64)i * n;
  double acc = 0.0;
  for (int j0 = 0; j0 < n; j0 += kWave) {   // 64 entries of the row per vector load, handed out by v_readlane
    const int nj = n - j0 < kWave ? n - j0 : kWave;
    const double rv = row[j0 + (lane < nj ? lane : 0)];
    for (int j = 0; j < nj; j += 8) {   // 8 LDS reads in flight (entries beyond nj: coefficient 0)
      double sv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) sv[u] = sm[(j0 + (j + u < nj ? j + u : 0)) * kWave + lane];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = fma(j + u < nj ? readlane_f64(rv, j + u) : 0.0, sv[u], acc);
    }
  }
  if (ok) x[(i64)i * Bp + b] = (TV)acc;
}

// x ~= A_l^{-1} rhs from a zero guess: V(2,2) weighted Jacobi, `gamma` coarse corrections per level
// (gamma = 2: W-cycle -- affordable because aggregation coarsens by ~10x -- compensates the weak
// piecewise-constant interpolation).  Returns the buffer holding the result.
template <typename TV>
TV* amg_cycle(const AmgHier& H, int l, const TV* rhs, double* rz_part, hipStream_t st) {
  const diffhe_amg_level& L = H.lev[l];
  TV* a = (TV*)H.xa[l];
  TV* b2 = (TV*)H.xb[l];
  const bool last = (l == H.nl - 1);
  if (last && l > 0 && L.dense_inv && H.Bv == 1 && L.n <= 128) {
    hipLaunchKernelGGL(amg_dense_solve_kernel<TV>, dim3((H.Bp + kWave - 1) / kWave, (L.n + 3) / 4), dim3(256),
                       sizeof(double) * L.n * kWave, st, L.dense_inv, rhs, a, L.n, H.Bp);
    return a;
  }
  auto launch = [&](auto kernel, int n, auto... args) {
    hipLaunchKernelGGL(kernel, node_grid(n, H.Bp), dim3(256), 0, st, args...);
  };
  auto level = [&](auto vals) {   // the level's matrix values: fp64, or their fp32 copy
    typedef std::remove_const_t<std::remove_pointer_t<decltype(vals)>> TM;
    // one sweep: pipelined with an xin, the elementwise pass from zero when no partial is wanted, else the plain kernel
    auto sweep = [&](const TV* xin, TV* xout, double w, double* part) {
      if (xin && launch_ellw<W_JACOBI>(vals, L.cols, rhs, xin, xout, w, part, L.n, L.W, H.Bp, H.Bv, st)) return;
      if (!xin && !part && launch_ellw_jacobi0(vals, rhs, xout, w, L.n, H.Bp, H.Bv, st)) return;
      launch(ell_jacobi_kernel<TV, TM>, L.n, vals, L.cols, rhs, xin, xout, w, part, L.n, L.W, H.Bp, H.Bv);
    };
    const int pre = last ? H.n_coarse : 2;
    for (int s = 0; s < pre; ++s) {
      const double w = (s & 1) ? H.wl1[l] : H.wl0[l];
      double* const part = (last && s == pre - 1) ? rz_part : nullptr;
      if (s == 0) {
        sweep(nullptr, a, w, part);
      } else {
        sweep(a, b2, w, part);
        TV* t = a; a = b2; b2 = t;
      }
    }
    if (last) return;
    const diffhe_amg_level& C = H.lev[l + 1];
    const int cycles = (l + 1 == H.nl - 1) ? 1 : H.gamma;  // the last level is "solved": one visit is enough
    for (int g = 0; g < cycles; ++g) {
      TV* const r = (TV*)H.res[l];
      if (!launch_ellw<W_RESID>(vals, L.cols, rhs, (const TV*)a, r, 0.0, (double*)nullptr, L.n, L.W, H.Bp, H.Bv, st))
        launch(ell_residual_out_kernel<TV, TM>, L.n, vals, L.cols, rhs, (const TV*)a, r, L.n, L.W, H.Bp, H.Bv);
      launch(agg_restrict_kernel<TV>, C.n, (const TV*)r, L.agg_ptr, L.agg_members, L.agg_weights, (TV*)H.rhs[l + 1], C.n, H.Bp);
      const TV* ec = amg_cycle<TV>(H, l + 1, (const TV*)H.rhs[l + 1], nullptr, st);
      if (L.p_cols)   // smoothed aggregation: P as ELL rows
        launch(sa_prolong_add_kernel<TV>, L.n, ec, L.p_cols, L.p_vals, L.p_width, a, H.scale, L.n, H.Bp);
      else
        launch(agg_prolong_add_kernel<TV>, L.n, ec, L.agg, a, H.scale, L.n, H.Bp);
    }
    for (int s = 0; s < 2; ++s) {
      const double w = (s & 1) ? H.wl0[l] : H.wl1[l];  // reverse order: symmetric cycle
      sweep(a, b2, w, (l == 0 && s == 1) ? rz_part : nullptr);
      TV* t = a; a = b2; b2 = t;
    }
  };
  // per-sample matrices inside the fp32 cycle read the fp32 copy of the values
  if (sizeof(TV) == 4 && H.Bv != 1 && L.vals32 != nullptr) level(L.vals32);
  else level(L.vals);
  return a;
}

int amg_fill(AmgHier& H, const diffhe_amg_level* levels, int n_levels, int Bv, int Bp) {
  if (!levels || n_levels < 1 || n_levels > kAmgMaxLevels) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  if (Bv != 1 && Bv != Bp) return DIFFHE_E_BADARG;
  for (int l = 0; l < n_levels; ++l) {
    const diffhe_amg_level& s = levels[l];
    if (s.n < 1 || s.W < 1 || !s.vals || !s.cols) return DIFFHE_E_BADARG;
    if (l < n_levels - 1 && (!s.agg || !s.agg_ptr || !s.agg_members)) return DIFFHE_E_BADARG;
    if (s.p_cols && (!s.p_vals || !s.agg_weights || s.p_width < 1)) return DIFFHE_E_BADARG;
    H.lev[l] = s;
  }
  H.nl = n_levels; H.Bv = Bv; H.Bp = Bp;
  return DIFFHE_OK;
}

// Multigrid preconditioner of the PCG (ell.h PcgHooks): z = one cycle on r.  fp32 cycle: the preconditioner STORES its
// vectors (and, for per-sample matrices, reads copies of the values) in fp32; the CG, its residual, the iterate and every
// dot product stay fp64 (as in diffhe_lattice_pcg_solve)
struct AmgPrecond {
  AmgHier H;
  int flags;
  float* r32;   // fp32 cycle: the copy of rs * r it reads, rs ~ 1 / |b| a power of two (keeps the cycle inside the fp32 range)
};
void amg_precondition(const AmgPrecond& M, Pcg& P) {
  P.z32 = M.r32 != nullptr;
  if (P.z32) P.z = amg_cycle<float>(M.H, 0, (const float*)M.r32, P.w.part[1], P.st);
  else P.z = amg_cycle<double>(M.H, 0, (const double*)P.w.r, P.w.part[1], P.st);
}
int amg_start(void* self, Pcg& P) {
  AmgPrecond& M = *(AmgPrecond*)self;
  const PcgWork& w = P.w;
  CgScalars& S = P.S;
  S.rs = (M.flags & DIFFHE_PCG_FP32) ? P.slot(SL_RS) : nullptr;
  S.xx = (M.flags & DIFFHE_PCG_NO_FLOOR) ? nullptr : P.slot(SL_XX);  // stop on `tol` alone
  S.maxdiag = P.slot(SL_MAXDIAG);
  int rc = check(hipMemsetAsync((void*)S.maxdiag, 0, sizeof(double) * P.Bv, P.st));
  if (rc) return rc;
  if (S.xx) {
    rc = check(hipMemsetAsync((void*)S.xx, 0, sizeof(double) * P.Bp, P.st));
    if (rc) return rc;
  }
  hipLaunchKernelGGL(ell_maxdiag_kernel, node_grid(P.n, P.Bv, 512), dim3(256), 0, P.st, P.vals, P.n, P.Bv,
                     (unsigned long long*)S.maxdiag);
  M.r32 = (M.flags & DIFFHE_PCG_FP32) ? (float*)M.H.rhs[0] : nullptr;
  hipLaunchKernelGGL(amg_init_kernel, P.grid, dim3(256), 0, P.st, P.b, P.x, w.r, M.r32, w.p, w.part[2], P.n, P.Bp);
  if (M.r32) {
    P.scalar(PH_SCALE, w.part[2], nullptr);
    hipLaunchKernelGGL(amg_cvt_kernel, P.grid, dim3(256), 0, P.st, (const double*)w.r, (const double*)S.rs, M.r32, P.n, P.Bp);
  }
  amg_precondition(M, P);
  P.scalar(PH_INIT, w.part[1], w.part[2]);
  P.update_p();  // beta = 0: p = z
  return DIFFHE_OK;
}
int amg_apply(void*, Pcg& P) {
  return launch_ellw<W_SPMV>(P.vals, P.cols, (const double*)nullptr, (const double*)P.w.p, P.w.Ap, 0.0, P.w.part[0], P.n, P.W,
                             P.Bp, P.Bv, P.st);
}
void amg_step(void* self, Pcg& P) {
  const AmgPrecond& M = *(const AmgPrecond*)self;
  const PcgWork& w = P.w;
  const CgScalars& S = P.S;
  hipLaunchKernelGGL(amg_update_kernel, P.grid, dim3(256), 0, P.st, (const double*)w.p, (const double*)w.Ap,
                     (const double*)S.alpha, P.x, w.r, M.r32, (const double*)S.rs, w.part[2], S.xx ? w.part[3] : (double*)nullptr,
                     P.n, P.Bp);
  if (S.xx) P.scalar(PH_XX, w.part[3], nullptr);
  amg_precondition(M, P);
}

}  // namespace

extern "C" long long diffhe_ell_amg_workspace_doubles(const diffhe_amg_level* levels, int n_levels, int Bp) {
  AmgHier H;
  if (amg_fill(H, levels, n_levels, 1, Bp)) return -1;
  PcgWork w;
  return amg_carve(H, nullptr) + pcg_carve(w, nullptr, H.lev[0].n, Bp, false, 4);
}

extern "C" int diffhe_ell_amg_pcg_solve(const diffhe_amg_level* levels, int n_levels, int Bv, const double* b, double* x,
                                        int Bp, double tol, int max_iter, int n_coarse, int gamma, double scale,
                                        int flags, double* work, double* relres, int* iters, int* status_host, void* stream) {
  if (!b || !x || !work || !relres || !iters || !status_host || max_iter < 0 || n_coarse < 1 || gamma < 1)
    return DIFFHE_E_BADARG;
  AmgPrecond M;
  AmgHier& H = M.H;
  int rc = amg_fill(H, levels, n_levels, Bv, Bp);
  if (rc) return rc;
  M.flags = flags;
  H.n_coarse = n_coarse; H.gamma = gamma; H.scale = scale;
  H.w0 = 0.56; H.w1 = 1.39;  // Chebyshev weights for the interval [0.5, 2] of D^-1 A
  // ... which holds for scalar kappa on reasonable meshes (lambda_max ~ 2.05).  A level that comes with a bound of its
  // own above 2 (diffhe_amg_level.reserved, in thousandths: the coefficient-aware hierarchy records it; positive
  // off-diagonals of an anisotropic tensor push lambda_max to 2.6 and the pair of sweeps would AMPLIFY the top modes)
  // gets the same weights for [lambda / 4, lambda].  reserved == 0: the weights above, bit for bit.
  for (int l = 0; l < H.nl; ++l) {
    H.wl0[l] = H.w0; H.wl1[l] = H.w1;
    if (H.lev[l].reserved > 2000) {
      const double f = 2000.0 / (double)H.lev[l].reserved;
      H.wl0[l] = H.w0 * f; H.wl1[l] = H.w1 * f;
    }
  }
  const diffhe_amg_level& L0 = H.lev[0];
  Pcg P{L0.vals, L0.cols, b, x, L0.n, L0.W, Bp, Bv, tol, relres, (hipStream_t)stream};
  const PcgHooks hooks{&M, false, 4, amg_start, amg_apply, amg_step};
  return pcg_solve(P, hooks, work + amg_carve(H, work), max_iter, 1, iters, status_host);   // polls every iteration
}
