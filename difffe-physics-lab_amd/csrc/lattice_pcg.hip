// Lattice fast path, the SOLVER: batched CG preconditioned by one V-cycle of lattice_cycle.hip (whose head describes the
// operator storage and the cycle).  The CG's vector kernels, its per-sample scalar block, the kernel profile, the driver
// (diffhe_lattice_pcg_solve) and the single-level entries of these kernels.  The workspace layout and the low-half policy of
// the residual pair are lattice_layout.h's.
#include <stdlib.h>
#include <type_traits>
#include <string.h>

#include "lattice.h"

namespace diffhe_lattice __attribute__((visibility("hidden"))) {
namespace {

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

// the start of the CG from a full-multigrid iterate: x64 = (double) x0
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
struct KernelProfile {
  bool on = false;
  hipEvent_t e0[KP_COUNT] = {}, e1[KP_COUNT] = {};
  bool have[KP_COUNT] = {};
  double ms[KP_COUNT] = {};
  long long n[KP_COUNT] = {};
};
thread_local KernelProfile g_kp;

}  // namespace

void kp_begin(int id, hipStream_t st) {
  if (g_kp.on) (void)hipEventRecord(g_kp.e0[id], st);
}
void kp_end(int id, hipStream_t st) {
  if (g_kp.on) {
    (void)hipEventRecord(g_kp.e1[id], st);
    g_kp.have[id] = true;
  }
}
void kp_collect() {  // call with the stream idle: every recorded event has completed
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

namespace {

// ---- the solve ------------------------------------------------------------------------------------------------------
// `flags` of diffhe_lattice_pcg_solve, decoded once
struct PcgOptions {
  bool f32;
  bool use_fmg;
  bool warm;              // x holds an initial guess (e.g. the previous step of an optimisation)
  bool resid64;           // keep the fp64 residual where the pair would apply (A/B runs, tests)
  bool keep_lo;           // ... and the pair whole to the end of the solve (the same)
  int trust_its;          // development, tests: the energy rule's trusted iterations (0: the default)
  bool use_floor;         // false (DIFFHE_PCG_NO_FLOOR): stop on `tol` alone
  bool closed_fp32_step;  // the caller vouches for a lattice closed by Dirichlet data (apply_step)
  int fmg_coarse_cycles;
  bool unfused;           // keep the four single-stage passes (A/B runs, tests)
  bool dense_scalar;      // scalar-load dense coarse solve
  bool pre2;              // fused PRE pass with two samples per lane as well (A/B runs, tests)
  bool split_start;       // keep the separate passes around the full-multigrid start (A/B runs, tests)

  PcgOptions(int flags, int n_levels)
      : f32((flags & DIFFHE_PCG_FP32) != 0),
        use_fmg((flags & DIFFHE_PCG_FMG) != 0 && n_levels > 1),
        warm((flags & DIFFHE_PCG_WARM) != 0),
        resid64((flags & DIFFHE_PCG_RESID_FP64) != 0),
        keep_lo((flags & DIFFHE_PCG_RESID_KEEP_LO) != 0),
        trust_its((flags >> DIFFHE_PCG_TRUST_ITS_SHIFT) & 15),
        use_floor((flags & DIFFHE_PCG_NO_FLOOR) == 0),
        closed_fp32_step((flags & DIFFHE_PCG_CLOSED_FP32_STEP) != 0),
        fmg_coarse_cycles(1 + ((flags >> DIFFHE_PCG_FMG_CYCLES_SHIFT) & 3)),
        unfused((flags & DIFFHE_PCG_UNFUSED) != 0),
        dense_scalar((flags & DIFFHE_PCG_DENSE_SCALAR) != 0),
        pre2((flags & DIFFHE_PCG_PRE2) != 0),
        split_start((flags & DIFFHE_PCG_SPLIT_START) != 0) {}

  void override_hier(Hier& H) const {
    H.fmg_coarse_cycles = fmg_coarse_cycles;
    if (unfused) H.fuse = 0;
    if (dense_scalar) H.dense_mfma = 0;
    if (pre2) H.pre4 = 0;
    if (split_start || warm) H.split_start = 1;   // the fused start passes belong to the cold start
  }
};

// One solve: the carved workspace, the scalar block, the geometry of the fine-level launches and the loop's state; the
// phases of the CG are its methods.
//   Fused loop (fine level runs the strip kernels): per iteration
//     [p = z + beta p ; x += alpha_prev p_old ; Ap = A p ; p.Ap]  ->  alpha  ->  [r -= alpha Ap ; r.r]
//     -> convergence flags  ->  z = V(r) (last sweep leaves r.z)  ->  beta
//   Unfused fallback (small meshes / batches): separate p-update, apply and x/r update kernels.
struct Solve {
  Hier& H;
  const PcgOptions& o;
  const hipStream_t st;
  const Level& L0;
  const int Bv, Bp, n, nblk;
  const double* const scale;
  const double* const b;
  double* const x;
  const double tol;
  double* const relres;

  PcgWork W;
  PcgScalars S;
  float* r32;                  // fp32 copy of rs * r, what an fp32 V-cycle reads (the high half of the pair)
  double* alpha_ring;          // n_slots (<= kRingSlots) rows of Bp step lengths
  double* alpha_single;
  int n_slots;
  i64 slot_stride;             // in elements of the stored type: fp32 slots are nb floats apart

  StripGeom g0, g2;
  bool fused;
  bool rupd;    // batch-shared matrix, fp32-stored directions: A p is never stored -- the residual update recomputes it from p (F_RUPD)
  bool rpair;   // ... and there the residual is carried as a pair of fp32 vectors, r32 (what the V-cycle reads) + rlo, not as
                // fp64 r plus r32 (F_RPAIR, lattice.h): nothing but the residual update and the pass that opens the loop touches it
  int cspl;
  bool step2;        // the CG step is cgstep2_kernel (p.Ap in packed fp32)
  bool fused_start;  // cold full-multigrid start of an fp32 solve with a batch-shared matrix whose fine level takes the strip
                     // kernels and halves in both directions: the passes around the start are fused (DIFFHE_PCG_SPLIT_START
                     // keeps them apart)

  const void* z = nullptr;
  int it = 0, flushed = 0;     // iterations done / directions already folded into x (fused loop)
  int nbz = 0, nba = 0;        // partial blocks of the last r.z / of the last apply or update
  int n_active = -1;
  LowHalf lo;

  Solve(Hier& H_, const PcgOptions& o_, double* work, const double* scale_, const double* b_, double* x_, double tol_,
        double tol_energy, double* relres_, double* err_est, int* iters, int* stop_rule, hipStream_t st_)
      : H(H_), o(o_), st(st_), L0(H_.lev[0]), Bv(H_.Bv), Bp(H_.Bp), n(H_.lev[0].n), nblk(lgrid(H_.lev[0].n, H_.Bp).x),
        scale(scale_), b(b_), x(x_), tol(tol_), relres(relres_), lo(false) {
    pcg_carve(W, work + carve_cycle(H, work, o.f32), n, Bp);
    r32 = o.f32 ? (float*)H.rhs[0] : nullptr;
    n_slots = o.f32 ? kRingSlots : kRingSlots / 2;
    slot_stride = (i64)n * Bp;
    S.rz = W.row(ROW_RZ, Bp); S.alpha = W.row(ROW_ALPHA, Bp); S.beta = W.row(ROW_BETA, Bp); S.bb = W.row(ROW_BB, Bp);
    S.tol2 = W.row(ROW_TOL2, Bp);
    S.active = (int*)W.row(ROW_ACTIVE, Bp);
    S.iters = iters;
    S.n_active = (int*)W.row(ROW_N_ACTIVE, Bp);   // two ints: [0] active samples, [1] those of them too far to drop the low half
    S.maxdiag = W.row(ROW_MAXDIAG, Bp);  // Bv entries (Bv <= Bp)
    S.rs = o.f32 ? W.row(ROW_RS, Bp) : nullptr;
    S.scale = scale;
    S.Bv = Bv;
    S.energy = W.row(ROW_ENERGY, Bp);
    S.est = err_est ? err_est : W.row(ROW_EST_FALLBACK, Bp);
    S.rr = W.row(ROW_RR, Bp);
    S.gap = W.row(ROW_GAP, Bp);
    S.lo_state = 0;
    S.rule = stop_rule ? stop_rule : (int*)W.row(ROW_RULE_FALLBACK, Bp);
    alpha_ring = W.row(ROW_ALPHA_RING, Bp);
    alpha_single = S.alpha;
    // tol_energy is asked of the FINAL iterate, which receives one more multigrid correction after the decision
    // (pcg_finish_kernel): the CG iterate's own estimate may be 1 / 0.3 of it (0.3: a cautious bound of the V(2,2)
    // cycle's convergence factor; measured reductions of the nodal error by that step: 5-8x)
    S.tol_e2 = tol_energy > 0.0 ? (tol_energy / 0.3) * (tol_energy / 0.3) : 0.0;
    S.e_max_it = 10 + ((tol_energy > 0.0 && tol_energy < 1e-11) ? (int)ceil(log10(1e-11 / tol_energy) - 1e-9) : 0);
    if (o.trust_its) S.e_max_it = o.trust_its;
    S.have_energy = 0;

    g0 = strip_geom(L0, Bp, kPupdCols);
    fused = g0.use;
    rupd = fused && o.f32 && Bv == 1;
    // (the pass that opens the loop must be the strip one too: it is what writes the pair -- residual_pass; today the two
    // geometries' `use` cannot differ, the condition keeps the pair from ever depending on that)
    rpair = rupd && !o.resid64 && strip_geom(L0, Bp).use;
    // cgstep2_kernel: two samples per lane for batches that are multiples of 128, else one
    // (four samples per lane -- what pays in the fused PRE pass -- measured here too: 0.699 -> 0.711 ms at 4 waves per SIMD
    // instead of 8, gpurun_out/r4n; not kept)
    cspl = (Bp % (2 * kWave) == 0) ? 2 : 1;
    g2 = (Bp % kWave == 0) ? strip_geom(L0, Bp, 4, cspl) : StripGeom{false, 0, 0, 0};
    lo = LowHalf(rpair && !o.keep_lo && S.tol_e2 > 0.0);
    // DIFFHE_PCG_CLOSED_FP32_STEP: the caller vouches for a lattice closed by Dirichlet data (lambda_min of the scaled operator bounded
    // away from 0).  With large Neumann parts the search directions are dominated by near-null modes, for which the
    // fp32 stencil cancels to noise: measured 13 / 11 instead of 12 / 9 iterations to 1e-14 there (gpurun_out/r6g)
    // (the host also asks for near-square cells and a hierarchy that reaches the dense coarsest level: on a 382 x 259
    // lattice, which coarsens once, 36 iterations to 1e-14 became 38 -- tools/stress.py seed 6301 case 39)
    step2 = o.f32 && rupd && o.closed_fp32_step && g2.use && shared32_ok(L0, Bv, Bp) && strip2_tile_fits(L0, Bp, g2.TR + 3);
    fused_start = !o.split_start && o.f32 && o.use_fmg && !o.warm && Bv == 1 && H.nl > 1 && strip_geom(L0, Bp).use &&
                  L0.nx == 2 * H.lev[1].nx && L0.ny == 2 * H.lev[1].ny;
  }

  // One phase of the per-sample scalars over a list of nb_ partial rows (pcg_scalar_kernel; long lists in two stages)
  void scalar(int phase, const double* part, int nb_) {
    const dim3 sgrid((Bp + 63) / 64);
    if (nb_ >= 256) {
      hipLaunchKernelGGL(pcg_slice_kernel, dim3(sgrid.x, kScalarSlices), dim3(256), 0, st, part, nb_, Bp, W.slices);
      hipLaunchKernelGGL(pcg_scalar_kernel, sgrid, dim3(1024), 0, st, phase, (const double*)W.slices, kScalarSlices, Bp, tol, S,
                         relres);
    } else {
      hipLaunchKernelGGL(pcg_scalar_kernel, sgrid, dim3(1024), 0, st, phase, part, nb_, Bp, tol, S, relres);
    }
  }

  // What the solve needs to know of the matrix before it starts: the per-sample max diagonal (S_FLOOR) and the spectrum
  // bound of the coarsest level.  Runs ahead of the direct solve too.
  int bounds() {
    if (o.use_floor && o.use_fmg) {
      const int rc = cycle_maxdiag(H, (double*)S.maxdiag, st);
      if (rc) return rc;
    }
    return cycle_coarse_bound(H, (unsigned long long*)W.row(ROW_GERSHGORIN, Bp), st);
  }

  // The dense inverse of the whole system (direct_ok), then the true residual.
  int direct(int* stop_rule) {
    cycle_direct_solve(H, b, x, st);
    launch_nodes(H, st, 8.0, pcg_init_kernel, n, b, (double*)nullptr, (double*)nullptr, W.partA, n, Bp);
    scalar(S_INIT, W.partA, nblk);                                 // b.b (and the bookkeeping S_RELRES reads)
    const int nbr = cycle_residual(H, b, x, nullptr, W.partA, st);
    scalar(S_RELRES, W.partA, nbr);
    int rc = diffhe::check(hipMemsetAsync(S.est, 0, sizeof(double) * Bp, st));
    if (rc) return rc;
    if (stop_rule) {  // direct solve: nothing iterated, nothing stopped
      rc = diffhe::check(hipMemsetAsync(stop_rule, 0, sizeof(int) * Bp, st));
      if (rc) return rc;
    }
    return diffhe::check_launch();
  }

  // z = V(r) and r.z, then the scalar phase behind it
  // The first z of a fused start goes straight into ring slot 0, where p0 = z0 lives: the first cgstep2 reads it in place
  // instead of copying it (4 B per node and sample instead of 8).  finish() finds z there when nothing iterates.
  void precondition(int first) {
    void* dest = (first && fused_start && step2) ? (void*)W.p : nullptr;
    z = cycle_precondition(H, o.f32, o.f32 ? (const void*)r32 : (const void*)W.r, W.partB, &nbz, st, dest);
    scalar(first ? S_RZ0 : S_BETA, W.partB, nbz);
  }

  template <typename TP>
  void finish_launch(int count, bool with_z) {
    launch_nodes(H, st, 16.0 + sizeof(TP) * (double)(count + (with_z ? 1 : 0)), pcg_finish_kernel<TP>, n,
                 (const double*)alpha_ring, (const TP*)(const void*)W.p, slot_stride, flushed, count, n_slots,
                 with_z ? (const TP*)z : (const TP*)nullptr, (const double*)S.rs /* NULL unless fp32 */, x, n, Bp);
  }
  // x += sum_{j = flushed .. it-1} alpha_j p_j  (+ z / rs at the end of the solve: pcg_finish_kernel)
  void flush_directions(bool with_z) {
    const int count = it - flushed;
    if (count == 0 && !with_z) return;
    if (o.f32) finish_launch<float>(count, with_z);
    else finish_launch<double>(count, with_z);
    flushed = it;
  }

  // the fused CG step with the iterate update deferred (F_PUPD_NX), fp32-stored directions
  template <int MINW, int MATS>
  void step_nx(const Extra& ex) {
    launch_strip<double, M_APPLY, false, F_PUPD_NX, float, kPupdCols, MINW, MATS>(
        L0, Bv, scale, (const double*)nullptr, (const double*)nullptr, rupd ? (double*)nullptr : W.Ap, 0.0, 0.0, W.partA, Bp, g0,
        st, ex);
  }
  template <typename TV>
  void update_p(int first) {
    launch_nodes(H, st, 8.0 + sizeof(TV) + (first ? 0.0 : 8.0), pcg_update_p_kernel<TV>, n, (const TV*)z, (const double*)S.beta,
                 W.p, first, n, Bp);
  }
  // p = z + beta p, A p and p.Ap
  void apply_step(int first) {
    if (!fused) {
      if (o.f32) update_p<float>(first);
      else update_p<double>(first);
      nba = cycle_apply_dot(H, W.p, W.Ap, W.partA, st);
      return;
    }
    if (!first) kp_begin(KP_CGSTEP, st);  // the first step of a solve (p = z) moves fewer bytes: not timed
    if (it - flushed == n_slots) flush_directions(false);   // ring full: fold everything so far into x
    const size_t esz = o.f32 ? sizeof(float) : sizeof(double);
    char* ring = (char*)W.p;
    Extra ex{};
    ex.a0 = z;
    ex.p_in = ring + (size_t)((it + n_slots - 1) % n_slots) * slot_stride * esz;
    ex.p_out = ring + (size_t)(it % n_slots) * slot_stride * esz;
    ex.x = nullptr;            // deferred (flush_directions)
    ex.alpha = nullptr; ex.beta = S.beta; ex.first = first;
    S.alpha = alpha_ring + (long long)(it % n_slots) * Bp;   // alpha_it goes next to p_it
    if (step2) {
      // fp32 stencil for p.Ap (cgstep2_kernel; packed, two samples per lane, where the batch allows): the step length only
      // (first step of a fused start: z already IS ring slot 0, p_out == z, nothing is stored)
      launch_cgstep2(L0, scale, (const double*)S.beta, first, (const float*)z, (const float*)ex.p_in, (float*)ex.p_out,
                     W.partA, Bp, g2, cspl, st);
      nba = g2.ncb * g2.nrc;
    } else {
      if (o.f32) {
        // 72 VGPRs (18 spilled), 7 waves per SIMD: 1.16 ms against 1.28 at the compiler's own 85 / 5; 8-column strips
        // (142 VGPRs) 1.96, 2-column strips at 8 waves 1.27, 6 or 8 waves 1.25 / 1.18 (same box, gpurun_out/r2l/variants*.txt).
        // The same cap on the V-cycle's strip kernels (already 6-7 waves) made them slower: -2...-6 % end to end.
        // per-sample matrices (coefficients in VGPRs): 4 waves per SIMD, 245.2 ms per step of the per-element-field variant
        // against 249.5 at 7 (gpurun_out/r4w)
        if (Bv != 1) step_nx<4, MAT_PER_SAMPLE>(ex);
        else step_nx<7, MAT_ANY>(ex);
      } else {
        launch_strip<double, M_APPLY, false, F_PUPD_NX, double, kPupdCols>(L0, Bv, scale, (const double*)nullptr,
                                                                (const double*)nullptr, W.Ap, 0.0, 0.0, W.partA, Bp, g0, st, ex);
      }
      nba = g0.ncb * g0.nrc;
    }
    if (!first) kp_end(KP_CGSTEP, st);
  }

  // the residual update of the fp32 CG with A p recomputed from the stored direction, in one of its forms
  // 5 waves per SIMD: 1.30 ms at 1024^2 x 256 (compiler's own choice 1.30, 7 waves 2.31 with spills; gpurun_out/r4q)
  // the pair form: 1.13 ms; the compiler's own choice measured 0.8 ms per step slower
  template <int FUSE>
  void rupd_launch(const Extra& ex) {
    launch_strip<double, M_APPLY, false, FUSE, float, kPupdCols, 5, MAT_SHARED>(   /* rupd: Bv == 1 */
        L0, Bv, scale, (const double*)nullptr, (const double*)nullptr, (double*)nullptr, 0.0, 0.0, W.partA, Bp, g0, st, ex);
  }
  // r -= alpha A p and r.r (of iteration `it`, not yet counted), then the convergence flags
  void update_residual() {
    kp_begin(KP_UPDATE, st);
    if (rupd) {
      Extra ex{};
      ex.p_in = (char*)W.p + (size_t)(it % n_slots) * slot_stride * sizeof(float);   // the direction apply_step just stored
      ex.x = W.r;
      ex.r32 = r32;
      ex.rscale = S.rs;
      ex.alpha = S.alpha;
      ex.rlo = W.rlo;
      if (!rpair) rupd_launch<F_RUPD>(ex);
      else if (lo.form == LowHalf::PAIR) rupd_launch<F_RPAIR>(ex);
      else if (lo.form == LowHalf::DROP) rupd_launch<F_RDROP>(ex);
      else rupd_launch<F_RSINGLE>(ex);
    } else {
      launch_nodes(H, st, 24.0 + (r32 ? 4.0 : 0.0) + (fused ? 0.0 : 24.0), pcg_update_kernel, n, (const double*)W.p,
                   (const double*)W.Ap, (const double*)S.alpha, fused ? (double*)nullptr : x, W.r, r32, (const double*)S.rs,
                   W.partA, n, Bp);
    }
    kp_end(KP_UPDATE, st);
    S.lo_state = lo.form;
    scalar(S_CONV, W.partA, rupd ? g0.ncb * g0.nrc : nblk);
  }

  // r = b - A x (+ its fp32 copy, + the partials b.x and x.(A x) of the energy bound when asked for)
  void residual_pass(bool energy) {
    const StripGeom gr = strip_geom(L0, Bp);
    if (gr.use && o.f32) {  // r and its fp32 copy in one pass (rpair: the two halves of the pair)
      Extra ex{};
      ex.r32 = r32;
      ex.rscale = S.rs;
      ex.dot_bx = energy ? 1 : 0;   // partial sums of this pass: b.x0 and x0.(A x0) (S_ENERGY / S_ENERGY2)
      ex.part2 = energy ? W.partB : nullptr;
      if (rpair) {
        ex.rlo = W.rlo;
        launch_strip<double, M_RESID, false, F_RPAIR, double, kStripCols, 1, MAT_SHARED>(
            L0, Bv, scale, (const double*)x, b, (double*)nullptr, 0.0, 0.0, energy ? W.partA : (double*)nullptr, Bp, gr, st, ex);
      } else {
        launch_strip<double, M_RESID, false>(L0, Bv, scale, (const double*)x, b, W.r, 0.0, 0.0,
                                             energy ? W.partA : (double*)nullptr, Bp, gr, st, ex);
      }
      nba = gr.ncb * gr.nrc;
    } else {
      nba = cycle_residual(H, b, x, W.r, energy ? W.partA : nullptr, st, energy ? 1 : 0, energy ? W.partB : nullptr);
      if (o.f32)
        launch_nodes(H, st, 12.0, pcg_cvt_kernel, n, (const double*)W.r, (const double*)S.rs, r32, n, Bp, (float*)nullptr);
    }
    if (energy) {
      scalar(S_ENERGY, W.partA, nba);
      scalar(S_ENERGY2, W.partB, nba);
      S.have_energy = 1;
    }
  }

  // x = (double) x0 [+ e0] / rs [+ x]: the iterate of the full-multigrid start, and |x|^2 for the floor
  template <typename TV>
  void set_iterate(const void* x0, const void* e0) {
    launch_nodes(H, st, 8.0 + sizeof(TV) + (o.warm ? 8.0 : 0.0) + (e0 ? (double)sizeof(TV) : 0.0), pcg_setx_kernel<TV>, n,
                 (const TV*)x0, (const double*)S.rs /* NULL unless fp32 */, x, o.use_floor ? W.partA : (double*)nullptr, n, Bp,
                 o.warm ? 1 : 0, (const TV*)e0);
  }

  // b.b and the per-sample bookkeeping, the starting iterate, its residual, and the first z = V(r)
  int start() {
    const bool light_init = (o.use_fmg && o.f32) || o.warm;  // the start overwrites x and r (cold) / x is the caller's guess (warm)
    launch_nodes(H, st, light_init ? 8.0 : 24.0, pcg_init_kernel, n, b, light_init ? (double*)nullptr : x, W.r, W.partA, n, Bp);
    scalar(S_INIT, W.partA, nblk);
    // fp32 copy of rs * b (rs from S_INIT): the full-multigrid start's right-hand side, or r0 of a zero start -- of which
    // the pair path needs the low parts too (they go where pcg_init_kernel has just put the fp64 r0, unused on that path)
    const bool start_rhs_fused = fused_start && Bp % kWave == 0;   // conversion and first restriction in one pass
    if (start_rhs_fused) {
      cycle_cvt_restrict(H, b, S.rs, r32, st);
    } else if (o.f32 && !o.warm) {
      const bool lo_too = rpair && !o.use_fmg;
      launch_nodes(H, st, lo_too ? 16.0 : 12.0, pcg_cvt_kernel, n, b, (const double*)S.rs, r32, n, Bp,
                   lo_too ? W.rlo : (float*)nullptr);
    }
    if (o.use_fmg) {
      // cold: x0 = FMG(b).  warm: x0 = x + FMG(b - A x) -- the full-multigrid start applied to the residual equation of
      // the caller's guess (an optimisation loop's previous solution): the start is then as accurate as the guess is
      // close, times the ~1e-3 of the full-multigrid step itself.
      if (o.warm) residual_pass(false);
      const void* rhs0 = o.f32 ? (const void*)r32 : (o.warm ? (const void*)W.r : (const void*)b);
      const void* e0 = nullptr;
      const void* x0 = cycle_fmg_start(H, o.f32, rhs0, st, &e0, start_rhs_fused);
      if (!x0) return DIFFHE_E_LAUNCH;
      if (o.f32) set_iterate<float>(x0, e0);
      else set_iterate<double>(x0, e0);
      if (o.use_floor) scalar(S_FLOOR, W.partA, nblk);
      residual_pass(true);
    } else if (o.warm) {
      residual_pass(true);
    }
    precondition(1);
    return diffhe::check_launch();
  }

  // status_host[2], [3]: where the poll of each iteration lands (the active samples, those of them that still need the
  // low half)
  int iterate(int max_iter, int* status_host) {
    while (it < max_iter) {
      apply_step(it == 0);
      scalar(S_ALPHA, W.partA, nba);
      update_residual();
      ++it;
      if (lo.after_update(it, S.e_max_it)) {
        flush_directions(false);
        residual_pass(false);
      }
      // z = V(r) and r.z: the new search direction's ingredients AND the energy-norm error estimate of the iterate;
      // the samples still active are counted in the scalar phase behind it (S_BETA)
      precondition(0);
      // [2] the active samples, [3] those of them that still need the low half: one copy, as before
      int rc = diffhe::check(hipMemcpyAsync(&status_host[2], S.n_active, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
      if (rc) return rc;
      rc = diffhe::check(hipStreamSynchronize(st));
      if (rc) return rc;
      n_active = status_host[2];
      kp_collect();  // the stream is idle here
      if (n_active == 0) break;
      lo.after_poll(status_host[3]);
    }
    return DIFFHE_OK;
  }

  // fold the directions still in the ring into x and add the final V-cycle's correction z (pcg_finish_kernel);
  // the unfused loop kept x current: only z is due there.  Then the true residual of what is returned.
  int finish() {
    if (!fused) flushed = it;
    flush_directions(true);
    S.alpha = alpha_single;
    nba = cycle_residual(H, b, x, nullptr, W.partA, st);
    scalar(S_RELRES, W.partA, nba);
    return diffhe::check_launch();
  }
};

// the fused CG step of diffhe_lattice_cg_step in one of its forms
template <int FUSE, typename TA, int MINW = 1>
void cg_step_launch(const Level& L, int Bv, const double* scale, double* Ap, double* part, int Bp, const StripGeom& g,
                    hipStream_t st, const Extra& ex) {
  launch_strip<double, M_APPLY, false, FUSE, TA, kPupdCols, MINW>(L, Bv, scale, (const double*)nullptr, (const double*)nullptr,
                                                                  Ap, 0.0, 0.0, part, Bp, g, st, ex);
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
extern "C" long long diffhe_lattice_pcg_workspace_doubles(const diffhe_mg_level* levels, int n_levels, int Bp) {
  Hier H;
  const double w1 = 0.8;
  if (fill_hier(H, levels, n_levels, 1, Bp, nullptr, &w1, 1, 1)) return -1;
  PcgWork W;
  return carve_cycle(H, nullptr, false) + pcg_carve(W, nullptr, H.lev[0].n, Bp);   // the fp64 layout of the cycle is the larger
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
  for (int l = 0; l < H.nl; ++l)
    if (H.lev[l].shift && (H.lev[l].inv || Bv != 1)) return DIFFHE_E_BADARG;  // a shift belongs to a factored operator
  const PcgOptions o(flags, H.nl);
  o.override_hier(H);
  Solve s(H, o, work, scale, b, x, tol, tol_energy, relres, err_est, iters, stop_rule, (hipStream_t)stream);
  rc = s.bounds();
  if (rc) return rc;
  if (direct_ok(H, o.f32)) {
    rc = s.direct(stop_rule);
    if (rc) return rc;
    status_host[0] = 0;
    status_host[1] = 0;
    status_host[3] = 0;
    return DIFFHE_OK;
  }
  rc = s.start();
  if (!rc) rc = s.iterate(max_iter, status_host);
  if (!rc) rc = s.finish();
  if (rc) return rc;
  status_host[0] = s.it;
  status_host[1] = s.n_active < 0 ? 0 : s.n_active;
  status_host[3] = s.lo.n_single;
  return DIFFHE_OK;
}

extern "C" int diffhe_lattice_bilinear(const diffhe_mg_level* level, int Bv, const double* scale, const double* x,
                                       const double* lam, const double* add, double* part, double* out, int Bp,
                                       void* stream) {
  if (!x || !lam || !part || !out) return DIFFHE_E_BADARG;
  Hier H;
  int rc = single_level(H, level, Bv, Bp, scale);
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
  int rc = single_level(H, level, Bv, Bp, scale);
  if (rc) return rc;
  const Level& L = H.lev[0];
  const StripGeom g = strip_geom(L, Bp, kPupdCols);
  if (!g.use) return DIFFHE_E_TOOBIG;
  Extra ex{};
  ex.a0 = z; ex.p_in = p_in; ex.p_out = p_out; ex.x = x; ex.alpha = alpha; ex.beta = beta; ex.first = first;
  hipStream_t st = (hipStream_t)stream;
  if (x) {
    if (z_fp32) cg_step_launch<F_PUPD, float>(L, Bv, scale, Ap, part, Bp, g, st, ex);
    else cg_step_launch<F_PUPD, double>(L, Bv, scale, Ap, part, Bp, g, st, ex);
  } else {
    if (z_fp32) cg_step_launch<F_PUPD_NX, float, 7>(L, Bv, scale, Ap, part, Bp, g, st, ex);   // the solver's instantiation (7 waves per SIMD)
    else cg_step_launch<F_PUPD_NX, double>(L, Bv, scale, Ap, part, Bp, g, st, ex);
  }
  return diffhe::check_launch();
}

// kept in the ABI for bench.py: the fp32 CG recomputes A p in the residual update (F_RUPD); the fused passes take two
// samples per lane
extern "C" int diffhe_lattice_recompute_ap(void) { return 1; }

extern "C" int diffhe_lattice_blocks(int n, int Bp) { (void)n; (void)Bp; return kPartBlocks; }

extern "C" int diffhe_lattice_fused_passes(void) { return 2; }
