// Internal header of the general path (any 1D/2D mesh, P1 tetrahedra in 3D: batch-shared ELL pattern): what its units
// share -- the workspace layout of its two PCG solves, the ELL row product and the node walk of its kernels, the
// scalar block of the CG, the multigrid hierarchy, and the declarations of the launchers each unit defines.
//
// Data layout: node-major, batch-innermost (n, Bp): entry (i, b) at i*Bp + b.  A wave's 64
// lanes are 64 samples of one node (Bp >= 64), so every load -- including the ELL "gather"
// p[col] -- is one contiguous 512 B segment, column indices are wave-uniform and amortised
// over the batch, and per-sample dot products are per-lane sums with no cross-lane traffic.
#pragma once
#include "common.h"
#include "diffhe_hip.h"

// One internal namespace for all general-path units; nothing in it is exported from the library.  Kernels sit in an
// anonymous namespace inside their unit.
namespace diffhe_ell __attribute__((visibility("hidden"))) {

typedef long long i64;

// Workspace layout.  Plain C++ up to the HIP-only part: a host compiler may include this header for the carves alone.
constexpr int kEllSlices = 16;   // rows per list of the slice table (cg_slice_kernel)
constexpr int kAmgMaxLevels = 16;

struct AmgHier {
  diffhe_amg_level lev[kAmgMaxLevels];
  int nl, Bv, Bp, n_coarse, gamma;
  double w0, w1, scale;
  double wl0[kAmgMaxLevels], wl1[kAmgMaxLevels];   // the Jacobi weights of each level (amg_weights)
  void *xa[kAmgMaxLevels], *xb[kAmgMaxLevels], *res[kAmgMaxLevels], *rhs[kAmgMaxLevels];  // TV vectors
};

// The cycle's vectors, four per level, each rounded up to 8 doubles.  work == NULL: the size alone.
inline i64 amg_carve(AmgHier& H, double* work) {
  i64 off = 0;
  auto take = [&](i64 cnt) { double* q = work ? work + off : nullptr; off += (cnt + 7) & ~7LL; return q; };
  for (int l = 0; l < H.nl; ++l) {
    const i64 nb = (i64)H.lev[l].n * H.Bp;
    H.xa[l] = take(nb);
    H.xb[l] = take(nb);
    H.res[l] = take(nb);
    H.rhs[l] = take(nb);  // level 0: the fp32 copy of the CG residual (fp32 cycle)
  }
  return off;
}

// What a PCG solve keeps in `work`: r, [z,] p, A p (n, Bp); npart lists of block partials (nblk, Bp); the scalar block
// (16 rows of Bp, CgScalars below); the slice table (2 x kEllSlices rows of Bp).  The Jacobi solve has a z of its own
// and 3 lists, the multigrid solve (whose z is a vector of the cycle) 4 lists.
struct PcgWork {
  double *r, *z, *p, *Ap, *part[4], *sc, *slices;
};
// work == NULL: the size in doubles alone (64 spare at the end), which is what the *_workspace_doubles entries return
inline i64 pcg_carve(PcgWork& w, double* work, int n, int Bp, bool own_z, int npart) {
  i64 off = 0;
  auto take = [&](i64 cnt) { double* q = work ? work + off : nullptr; off += cnt; return q; };
  const i64 nb = (i64)n * Bp, pb = (i64)diffhe::node_blocks(n, Bp) * Bp;
  w.r = take(nb);
  w.z = own_z ? take(nb) : nullptr;
  w.p = take(nb);
  w.Ap = take(nb);
  for (int k = 0; k < 4; ++k) w.part[k] = k < npart ? take(pb) : nullptr;
  w.sc = take(16LL * Bp);
  w.slices = take(2LL * kEllSlices * Bp);
  return off + 64;
}

#if defined(__HIPCC__)
using namespace diffhe;

// ---------------------------------------------------------------------------------------
// Row i of an ELL matrix against x for this lane's sample: acc -/+= a_k x[col_k], k = 0 .. W-1 in that order (the order
// and the operations of the plain loop: bitwise the same sums).  The loads of NU entries are issued before the first
// product (the plain loop waited for col_k, then for x[col_k], entry by entry: two exposed latencies per entry, 0.2 of
// the HBM rate at 512^2 x 64); entries beyond W repeat entry 0 with the value 0.  With batches of >= 64 a wave works on
// ONE node (FOR_EACH_NODE below) and takes ell_row_uniform instead.
// ---------------------------------------------------------------------------------------
template <bool SUB, int NU, typename TV, typename TM>
__device__ __forceinline__ double ell_row_chunks(double acc, const TM* __restrict__ vals, const int* __restrict__ cols,
                                                 const TV* __restrict__ x, int i, int n, int W, int Bp, int Bv, int b) {
  const int vb = Bv == 1 ? 0 : b;
  for (int k0 = 0; k0 < W; k0 += NU) {
    int c[NU];
    double a[NU];
    TV xv[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const bool in = k0 + u < W;
      const i64 ent = (i64)(in ? k0 + u : 0) * n + i;
      c[u] = cols[ent];
      a[u] = in ? (double)vals[ent * Bv + vb] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) xv[u] = x[(i64)c[u] * Bp + b];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      if (SUB) acc -= a[u] * (double)xv[u];
      else acc += a[u] * (double)xv[u];
    }
  }
  return acc;
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// The wave-uniform form (a wave = one node, all 64 lanes active): ONE vector load brings the node's column indices
// (lane k: entry k; scalar loads came out one after the other, each waited for) and, for a batch-shared matrix
// (SHARED), ONE its values; v_readlane hands them out as scalars BEFORE the gathers are issued, so the NU gathers of a
// chunk are in flight together, each through a scalar row base + the lane's offset.  FULL: W == NU, one chunk, no
// padding (P1 triangulations of lattice connectivity: 7 entries per row).  Same entries, same order, same operations.
template <bool SUB, bool SHARED, int NU, bool FULL, typename TV, typename TM>
__device__ __forceinline__ double ell_row_uniform(double acc, const TM* __restrict__ vals, const int* __restrict__ cols,
                                                  const TV* __restrict__ x, int i, int n, int W, int Bp, int b) {
  const int lane = threadIdx.x & 63;
  for (int k0 = 0; k0 < W; k0 += kWave) {
    const int nk = FULL ? NU : (W - k0 < kWave ? W - k0 : kWave);
    const i64 entl = (i64)(k0 + (lane < nk ? lane : 0)) * n + i;
    const int cv = cols[entl];
    double av = 0.0;
    if (SHARED) av = (double)vals[entl];
    for (int u0 = 0; u0 < nk; u0 += NU) {
      int c[NU];
      double a[NU];
      TV xv[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const bool in = FULL || u0 + u < nk;
        const int k = in ? u0 + u : 0;
        c[u] = __builtin_amdgcn_readlane(cv, k);
        if (SHARED) a[u] = in ? readlane_f64(av, k) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const TV* __restrict__ xr = x + (i64)c[u] * Bp;   // scalar row base
        xv[u] = xr[b];
      }
      if (!SHARED) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const bool in = FULL || u0 + u < nk;
          const TM* __restrict__ vr = vals + ((i64)(k0 + (in ? u0 + u : 0)) * n + i) * Bp;
          a[u] = in ? (double)vr[b] : 0.0;
        }
      }
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        if (SUB) acc -= a[u] * (double)xv[u];
        else acc += a[u] * (double)xv[u];
      }
    }
  }
  return acc;
}
template <bool SUB, bool UNI, bool SHARED, typename TV, typename TM>
__device__ __forceinline__ double ell_row(double acc, const TM* __restrict__ vals, const int* __restrict__ cols,
                                          const TV* __restrict__ x, int i, int n, int W, int Bp, int Bv, int b) {
  if (UNI)
    return W == 7 ? ell_row_uniform<SUB, SHARED, 7, true>(acc, vals, cols, x, i, n, W, Bp, b)
                  : ell_row_uniform<SUB, SHARED, 8, false>(acc, vals, cols, x, i, n, W, Bp, b);
  return ell_row_chunks<SUB, 8>(acc, vals, cols, x, i, n, W, Bp, Bv, b);
}
// for (i over this lane's nodes) BODY -- with batches of >= 64 through wave-uniform indices (see ell_row_uniform), and
// with the nodes dealt to the XCDs in CONTIGUOUS ranges: workgroups go round-robin to the 8 XCDs (block b -> XCD b % 8),
// each with its own L2, and a row's neighbours sit close to it in any sensible numbering.  With the plain grid-stride
// walk every XCD saw every 8th group of 4 nodes, so each L2 fetched nearly ALL of x (the gathers of the fine-level Jacobi
// sweep at 512^2 x 64 moved ~8x the vector through the fabric); now the blocks of one XCD sweep one eighth of the nodes
// together and the gathers hit their own L2.  Which nodes a block sums changes, not the fixed order: still reproducible.
// nodes first, first + step, ... < hi of this wave in the wave-per-node walk (XCD-contiguous ranges when the grid allows)
__device__ __forceinline__ void wave_node_range(int n, int& first, int& hi, int& step) {
  const int wave_u = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  first = (int)blockIdx.x * 4 + wave_u;
  hi = n;
  step = (int)gridDim.x * 4;
  if ((gridDim.x & 7) == 0) {   // else the plain grid-stride walk
    const int chunk = (n + 7) >> 3, lo = ((int)blockIdx.x & 7) * chunk;
    hi = lo + chunk < n ? lo + chunk : n;
    first = lo + ((int)blockIdx.x >> 3) * 4 + wave_u;
    step = ((int)gridDim.x >> 3) * 4;
  }
}
#define FOR_EACH_NODE(nm_, n_, Bp_, Bv_, ...)                                                     \
  do {                                                                                            \
    if ((Bp_) >= kWave) {                                                                         \
      constexpr bool kUni = true;                                                                 \
      int first_, hi_, step_;                                                                     \
      wave_node_range((n_), first_, hi_, step_);                                                  \
      if ((Bv_) == 1) {                                                                           \
        constexpr bool kShared = true;                                                            \
        for (int i = first_; i < hi_; i += step_) __VA_ARGS__                                     \
      } else {                                                                                    \
        constexpr bool kShared = false;                                                           \
        for (int i = first_; i < hi_; i += step_) __VA_ARGS__                                     \
      }                                                                                           \
    } else {                                                                                      \
      constexpr bool kUni = false;                                                                \
      constexpr bool kShared = false;                                                             \
      for (int i = (nm_).node0; i < (n_); i += (nm_).stride) __VA_ARGS__                          \
    }                                                                                             \
  } while (0)

// ---------------------------------------------------------------------------------------
// Batched Jacobi-PCG
// ---------------------------------------------------------------------------------------
struct CgScalars {  // each (Bp) doubles, in `work` after the vectors and partials
  double *rz, *pAp, *alpha, *beta, *bb, *tol2, *rr;
  double* rs;             // per-sample power of two ~ 1 / |b| applied to the fp32 residual copies (NULL: none)
  double* xx;             // |x|^2 of the current iterate (AMG path: attainable-accuracy floor), may be NULL
  const double* maxdiag;  // per-sample (Bv entries) max diagonal entry, with xx
  int Bv;
  int* active;    // (Bp)
  int* iters;     // (Bp)
  int* n_active;  // (1)
};

// Sum the block partials of one quantity for sample b (fixed order: deterministic).
// Block = 4 waves: lanes over samples, waves over quarters of the partial list.
__device__ inline double sum_partials(const double* __restrict__ part, int nblk, int Bp, int b, double* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double s = 0.0;
  if (b < Bp) {  // 4 independent chains keep several loads in flight (fixed order: still deterministic)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int k = wave;
    for (; k + 12 < nblk; k += 16) {
      s0 += part[(i64)k * Bp + b];
      s1 += part[(i64)(k + 4) * Bp + b];
      s2 += part[(i64)(k + 8) * Bp + b];
      s3 += part[(i64)(k + 12) * Bp + b];
    }
    for (; k < nblk; k += 4) s0 += part[(i64)k * Bp + b];
    s = (s0 + s1) + (s2 + s3);
  }
  lds[wave * kWave + lane] = s;
  __syncthreads();
  const double t = (lds[lane] + lds[kWave + lane]) + (lds[2 * kWave + lane] + lds[3 * kWave + lane]);
  __syncthreads();
  return t;
}

enum { PH_INIT = 0, PH_ALPHA = 1, PH_BETA = 2, PH_RELRES = 3, PH_XX = 4, PH_SCALE = 5 };

// The PCG of both general-path solves (ell_pcg.hip).  A solve fills the system part of Pcg and its hooks and calls
// pcg_solve, which carves `work`, fills the scalar block and runs the loop, the poll and the closing true residual.
enum { SL_RZ = 0, SL_PAP, SL_ALPHA, SL_BETA, SL_BB, SL_TOL2, SL_RR, SL_ACTIVE, SL_N_ACTIVE, SL_XX, SL_MAXDIAG, SL_RS };
struct Pcg {
  const double* vals;   // the system, set by the caller
  const int* cols;
  const double* b;
  double* x;
  int n, W, Bp, Bv;
  double tol;
  double* relres;
  hipStream_t st;
  dim3 grid;            // the solve's state, set by pcg_solve: node_grid(n, Bp), ...
  PcgWork w;
  CgScalars S;
  const void* z;        // the preconditioned residual the next p-update reads, stored as float (z32) or double
  bool z32;
  double* slot(int k) const { return w.sc + (i64)k * Bp; }   // row SL_* of the scalar block
  // per-sample scalar phase on one or two partial lists; long lists go through cg_slice_kernel first
  void scalar(int phase, const double* pa, const double* pb) const;
  void update_p() const;   // p = z + beta p
};
// What tells the two solves apart: the workspace (4 vectors + 3 partial lists for Jacobi, 3 + 4 for multigrid), three hooks
struct PcgHooks {
  void* self;
  bool own_z;
  int npart;
  int (*start)(void* self, Pcg& P);    // x = 0, r = b, z, the scalars of PH_INIT, p = z
  int (*apply)(void* self, Pcg& P);    // Ap = A p, partials of p.Ap in part[0]; NULL or returns 0: cg_spmv_kernel does it
  void (*step)(void* self, Pcg& P);    // x += alpha p, r -= alpha Ap, z = M^-1 r; partials of r.z in part[1], r.r in part[2]
};
// polls n_active every check_every iterations and at max_iter; status_host as in diffhe_ell_cg_solve
int pcg_solve(Pcg& P, const PcgHooks& M, double* work, int max_iter, int check_every, int* iters, int* status_host);

#endif  // __HIPCC__

}  // namespace diffhe_ell
