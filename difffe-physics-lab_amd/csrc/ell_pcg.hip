// General path, PCG: the CG kernels, the scalar phase, the PCG driver of both general-path solves (Jacobi here,
// aggregation multigrid in ell_amg.hip) and the Jacobi-PCG entries.
#include "ell.h"

namespace {
using namespace diffhe_ell;

__global__ __launch_bounds__(256) void cg_init_kernel(const double* __restrict__ vals, const double* __restrict__ bvec,
                                                       double* __restrict__ x, double* __restrict__ r,
                                                       double* __restrict__ z, double* __restrict__ p,
                                                       double* __restrict__ part_rz, double* __restrict__ part_bb, int n,
                                                       int Bp, int Bv) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < Bp;
  const int vb = Bv == 1 ? 0 : nm.b;
  double s_rz = 0.0, s_bb = 0.0;
  if (ok)
    for (int i = nm.node0; i < n; i += nm.stride) {
      const i64 o = (i64)i * Bp + nm.b;
      const double bi = bvec[o];
      const double zi = bi / vals[(i64)i * Bv + vb];  // slot 0 = diagonal
      x[o] = 0.0; r[o] = bi; z[o] = zi; p[o] = zi;
      s_rz += bi * zi;
      s_bb += bi * bi;
    }
  store_block_partial(s_rz, part_rz, Bp, nm.b, ok, lds);
  store_block_partial(s_bb, part_bb, Bp, nm.b, ok, lds);
}

__global__ __launch_bounds__(256, 8) void cg_spmv_kernel(const double* __restrict__ vals, const int* __restrict__ cols,
                                                       const double* __restrict__ p, double* __restrict__ Ap,
                                                       double* __restrict__ part_pAp, int n, int W, int Bp, int Bv) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < Bp;
  double s = 0.0;
  if (ok)
    FOR_EACH_NODE(nm, n, Bp, Bv, {
      const i64 o = (i64)i * Bp + nm.b;
      const double ps = p[o];    // issued with the row's first loads
      const double acc = ell_row<false, kUni, kShared>(0.0, vals, cols, p, i, n, W, Bp, Bv, nm.b);
      Ap[o] = acc;
      s += acc * ps;
    });
  store_block_partial(s, part_pAp, Bp, nm.b, ok, lds);
}

__global__ __launch_bounds__(256) void cg_update_kernel(const double* __restrict__ vals, const double* __restrict__ p,
                                                         const double* __restrict__ Ap, const double* __restrict__ alpha,
                                                         double* __restrict__ x, double* __restrict__ r,
                                                         double* __restrict__ z, double* __restrict__ part_rz,
                                                         double* __restrict__ part_rr, int n, int Bp, int Bv) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < Bp;
  const int vb = Bv == 1 ? 0 : nm.b;
  double s_rz = 0.0, s_rr = 0.0;
  if (ok) {
    const double a = alpha[nm.b];
    for (int i = nm.node0; i < n; i += nm.stride) {
      const i64 o = (i64)i * Bp + nm.b;
      x[o] += a * p[o];
      const double ri = r[o] - a * Ap[o];
      const double zi = ri / vals[(i64)i * Bv + vb];
      r[o] = ri; z[o] = zi;
      s_rz += ri * zi;
      s_rr += ri * ri;
    }
  }
  store_block_partial(s_rz, part_rz, Bp, nm.b, ok, lds);
  store_block_partial(s_rr, part_rr, Bp, nm.b, ok, lds);
}

template <typename TZ>
__global__ __launch_bounds__(256) void cg_update_p_kernel(const TZ* __restrict__ z, const double* __restrict__ beta,
                                                           double* __restrict__ p, int n, int Bp) {
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  const double be = beta[nm.b];
  for (int i = nm.node0; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    p[o] = (double)z[o] + be * p[o];
  }
}

// true residual |b - A x|^2 partials
__global__ __launch_bounds__(256, 8) void residual_kernel(const double* __restrict__ vals, const int* __restrict__ cols,
                                                        const double* __restrict__ bvec, const double* __restrict__ x,
                                                        double* __restrict__ part, int n, int W, int Bp, int Bv) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < Bp;
  double s = 0.0;
  if (ok)
    FOR_EACH_NODE(nm, n, Bp, Bv, {
      const double acc = ell_row<true, kUni, kShared>(bvec[(i64)i * Bp + nm.b], vals, cols, x, i, n, W, Bp, Bv, nm.b);
      s += acc * acc;
    });
  store_block_partial(s, part, Bp, nm.b, ok, lds);
}

// First stage of a long partial list (2048 rows on big meshes: ONE block of cg_scalar_kernel summing them took 68 us per
// phase at 512^2 x 64, three phases per iteration): block (x, y, z) sums the rows y, y + S, ... of list z for the samples
// of chunk x into row y of that list's slice table (S = kEllSlices rows); cg_scalar_kernel then sums S rows.  Fixed
// assignment and order of additions: bitwise reproducible (the lattice solver's pcg_slice_kernel, for two lists at once).
__global__ __launch_bounds__(256) void cg_slice_kernel(const double* __restrict__ partA, const double* __restrict__ partB,
                                                        int nblk, int Bp, double* __restrict__ slice) {
  __shared__ double lds[4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kWave + lane;
  const int S = gridDim.y, y = blockIdx.y;
  const double* __restrict__ part = blockIdx.z ? partB : partA;
  double s0 = 0.0, s1 = 0.0;
  if (b < Bp) {
    int k = y + S * wave;
    for (; k + 4 * S < nblk; k += 8 * S) {
      s0 += part[(i64)k * Bp + b];
      s1 += part[(i64)(k + 4 * S) * Bp + b];
    }
    if (k < nblk) s0 += part[(i64)k * Bp + b];
  }
  lds[wave * kWave + lane] = s0 + s1;
  __syncthreads();
  if (wave == 0 && b < Bp)
    slice[((i64)blockIdx.z * S + y) * Bp + b] = (lds[lane] + lds[kWave + lane]) + (lds[2 * kWave + lane] + lds[3 * kWave + lane]);
}

__global__ __launch_bounds__(256) void cg_scalar_kernel(int phase, const double* __restrict__ partA,
                                                         const double* __restrict__ partB, int nblk, int Bp,
                                                         double tol, CgScalars S, double* __restrict__ relres) {
  __shared__ double lds[4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kWave + lane;
  const double a = sum_partials(partA, nblk, Bp, b, lds);
  const double c = partB ? sum_partials(partB, nblk, Bp, b, lds) : 0.0;
  if (wave != 0 || b >= Bp) return;
  if (phase == PH_INIT) {  // a = r.z, c = b.b
    S.rz[b] = a;
    S.bb[b] = c;
    S.tol2[b] = tol * tol * c;
    S.active[b] = c > 0.0 ? 1 : 0;
    S.iters[b] = 0;
    S.alpha[b] = 0.0;
    S.beta[b] = 0.0;
  } else if (phase == PH_ALPHA) {  // a = p.Ap
    // scaled fp32 copies: z, p, Ap carry rs and both dots rs^2; the updates of x and r take alpha / rs
    S.alpha[b] = (S.active[b] && a > 0.0) ? (S.rz[b] / a) / (S.rs ? S.rs[b] : 1.0) : 0.0;
    if (b == 0) *S.n_active = 0;
  } else if (phase == PH_BETA) {  // a = r.z (new), c = r.r
    if (S.active[b]) {
      S.iters[b] += 1;
      S.rr[b] = c;
      double thr = S.tol2[b];
      if (S.xx) {  // fp64 cannot bring |b - A x| below ~ u |A| |x|: stop at half of that level (see diffhe_hip.h)
        const double fl = 0.5 * 1.1102230246251565e-16 * 2.0 * S.maxdiag[S.Bv == 1 ? 0 : b];
        const double floor2 = fl * fl * S.xx[b];
        if (floor2 > thr) thr = floor2;
      }
      if (c <= thr) {
        S.active[b] = 0;
        S.beta[b] = 0.0;
      } else {
        S.beta[b] = a / S.rz[b];
        S.rz[b] = a;
        atomicAdd(S.n_active, 1);
      }
    } else {
      S.beta[b] = 0.0;
    }
  } else if (phase == PH_XX) {  // a = x.x
    S.xx[b] = a;
  } else if (phase == PH_SCALE) {  // a = b.b: power of two rs with rs |b| in [1, 2) (see pcg_cvt_kernel in lattice_pcg.hip)
    S.rs[b] = a > 0.0 ? ldexp(1.0, -ilogb(sqrt(a))) : 1.0;
  } else {  // PH_RELRES: a = |b - A x|^2
    relres[b] = S.bb[b] > 0.0 ? sqrt(a / S.bb[b]) : 0.0;
  }
}

}  // namespace

namespace diffhe_ell {

void Pcg::scalar(int phase, const double* pa, const double* pb) const {
  int nblk = grid.x;
  const dim3 sgrid((Bp + 63) / 64);
  if (nblk >= 256) {   // the scalar kernel then sums the kEllSlices rows per list of the slice table
    hipLaunchKernelGGL(cg_slice_kernel, dim3(sgrid.x, kEllSlices, pb ? 2 : 1), dim3(256), 0, st, pa, pb, nblk, Bp, w.slices);
    pa = w.slices;
    if (pb) pb = w.slices + (i64)kEllSlices * Bp;
    nblk = kEllSlices;
  }
  hipLaunchKernelGGL(cg_scalar_kernel, sgrid, dim3(256), 0, st, phase, pa, pb, nblk, Bp, tol, S, relres);
}

void Pcg::update_p() const {
  if (z32) hipLaunchKernelGGL(cg_update_p_kernel<float>, grid, dim3(256), 0, st, (const float*)z, (const double*)S.beta, w.p, n, Bp);
  else hipLaunchKernelGGL(cg_update_p_kernel<double>, grid, dim3(256), 0, st, (const double*)z, (const double*)S.beta, w.p, n, Bp);
}

int pcg_solve(Pcg& P, const PcgHooks& M, double* work, int max_iter, int check_every, int* iters, int* status_host) {
  P.grid = node_grid(P.n, P.Bp);
  pcg_carve(P.w, work, P.n, P.Bp, M.own_z, M.npart);
  CgScalars& S = P.S;
  S.rz = P.slot(SL_RZ); S.pAp = P.slot(SL_PAP); S.alpha = P.slot(SL_ALPHA); S.beta = P.slot(SL_BETA);
  S.bb = P.slot(SL_BB); S.tol2 = P.slot(SL_TOL2); S.rr = P.slot(SL_RR);
  S.active = (int*)P.slot(SL_ACTIVE); S.iters = iters; S.n_active = (int*)P.slot(SL_N_ACTIVE); S.Bv = P.Bv;
  S.rs = S.xx = nullptr; S.maxdiag = nullptr;   // plain `tol` stop unless the start hook sets these
  const double* const* part = P.w.part;

  int rc = M.start(M.self, P);
  if (rc) return rc;
  rc = check_launch();
  if (rc) return rc;
  int it = 0, n_active = -1;
  while (it < max_iter) {
    if (!M.apply || !M.apply(M.self, P))
      hipLaunchKernelGGL(cg_spmv_kernel, P.grid, dim3(256), 0, P.st, P.vals, P.cols, (const double*)P.w.p, P.w.Ap, P.w.part[0],
                         P.n, P.W, P.Bp, P.Bv);
    P.scalar(PH_ALPHA, part[0], nullptr);
    M.step(M.self, P);
    P.scalar(PH_BETA, part[1], part[2]);
    P.update_p();
    ++it;
    if (it % check_every == 0 || it == max_iter) {
      rc = check(hipMemcpyAsync(&status_host[2], S.n_active, sizeof(int), hipMemcpyDeviceToHost, P.st));
      if (!rc) rc = check(hipStreamSynchronize(P.st));
      if (rc) return rc;
      n_active = status_host[2];
      if (n_active == 0) break;
    }
  }
  hipLaunchKernelGGL(residual_kernel, P.grid, dim3(256), 0, P.st, P.vals, P.cols, P.b, (const double*)P.x, P.w.part[0], P.n,
                     P.W, P.Bp, P.Bv);
  P.scalar(PH_RELRES, part[0], nullptr);
  rc = check_launch();
  if (rc) return rc;
  status_host[0] = it;
  status_host[1] = n_active < 0 ? 0 : n_active;
  return DIFFHE_OK;
}

}  // namespace diffhe_ell

namespace {

// Jacobi preconditioner: z = r / D lives in the workspace and is formed inside the fused update
int jacobi_start(void*, Pcg& P) {
  const PcgWork& w = P.w;
  P.z = w.z; P.z32 = false;
  hipLaunchKernelGGL(cg_init_kernel, P.grid, dim3(256), 0, P.st, P.vals, P.b, P.x, w.r, w.z, w.p, w.part[0], w.part[1], P.n,
                     P.Bp, P.Bv);
  P.scalar(PH_INIT, w.part[0], w.part[1]);
  return DIFFHE_OK;
}
void jacobi_step(void*, Pcg& P) {
  const PcgWork& w = P.w;
  hipLaunchKernelGGL(cg_update_kernel, P.grid, dim3(256), 0, P.st, P.vals, (const double*)w.p, (const double*)w.Ap,
                     (const double*)P.S.alpha, P.x, w.r, w.z, w.part[1], w.part[2], P.n, P.Bp, P.Bv);
}
constexpr PcgHooks kJacobi{nullptr, true, 3, jacobi_start, nullptr, jacobi_step};

}  // namespace

extern "C" long long diffhe_cg_workspace_doubles(int n, int Bp) {
  PcgWork w;
  return pcg_carve(w, nullptr, n, Bp, kJacobi.own_z, kJacobi.npart);
}

extern "C" int diffhe_ell_cg_solve(const double* vals, const int* cols, const double* b, double* x, int n, int W,
                                   int Bp, int Bv, double tol, int max_iter, int check_every, double* work,
                                   double* relres, int* iters, int* status_host, void* stream) {
  if (!vals || !cols || !b || !x || !work || !relres || !iters || !status_host || n < 1 || W < 1 || max_iter < 0)
    return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  if (Bv != 1 && Bv != Bp) return DIFFHE_E_BADARG;
  if (check_every < 1) check_every = 1;
  Pcg P{vals, cols, b, x, n, W, Bp, Bv, tol, relres, (hipStream_t)stream};
  return pcg_solve(P, kJacobi, work, max_iter, check_every, iters, status_host);
}

extern "C" int diffhe_ell_apply(const double* vals, const int* cols, const double* x, double* y, double* part, int n,
                                int W, int Bp, int Bv, void* stream) {
  if (!vals || !cols || !x || !y || !part || n < 1 || W < 1) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  if (Bv != 1 && Bv != Bp) return DIFFHE_E_BADARG;
  hipLaunchKernelGGL(cg_spmv_kernel, diffhe::node_grid(n, Bp), dim3(256), 0, (hipStream_t)stream, vals, cols, x, y,
                     part, n, W, Bp, Bv);
  return diffhe::check_launch();
}
