// Set-up passes of the coefficient-aware aggregation hierarchy (ours; diffhe/amg.py builds the levels on the host from
// what these leave).  The aggregates and the prolongation of the general path are shared by the batch, so they are built
// from ONE matrix in the plan's ELL pattern, the representative operator
//
//     abar(k, i) = (1 / B) sum_{b < B} a_b(k, i) / s_b,      s_b = mean free-row diagonal of sample b
//
// -- the stiffness matrix of the mean scaled coefficient: SPD, constants in its near-null space, every sample weighing
// the same whatever the magnitude of its conductivity.
//
//   diffhe_ell_sample_scales:   sum of the free-row diagonals per sample, two fixed-order stages;
//   diffhe_ell_mean_operator:   abar from vals (W, n, Bv): one wave per node, lanes over samples (512 B loads, batch
//                               innermost), fixed-order wave reduction, lane k writes slot k;
//   diffhe_ell_strength_filter: on abar, one wave per node, lane k = slot k of the row:
//                               c_ij = max(-a_ij, 0) / sqrt(a_ii a_jj), slot k STRONG when c_ij >= theta max_k c_ik in row i
//                               AND c_ji >= theta max_l c_jl in row j (looked up through row j: the plan keeps no
//                               transposed-slot table, W compares do it); weak off-diagonals are lumped to the diagonal.
//
// No floating-point atomics: every result is bitwise reproducible.  Division and square root are the IEEE operations
// and no multiply-add is contracted, so diffhe.amg.strength_filter (numpy) restates the filter decision for decision.
#include "common.h"

namespace {

using namespace diffhe;
typedef long long i64;

constexpr int kChunk = DIFFHE_ELL_SCALE_CHUNK;   // rows per block of the first summation stage

// dst[blk, b] = sum over the rows r of chunk blk with mask[r] == 0 of src[r * B + b], in row order; thread -> sample.
// Four loads in flight, added in row order.
__global__ __launch_bounds__(64) void sum_free_rows_kernel(const double* __restrict__ src,
                                                           const unsigned char* __restrict__ mask, int rows, int chunk,
                                                           int B, double* __restrict__ dst) {
  const int b = blockIdx.y * kWave + threadIdx.x;
  if (b >= B) return;
  const i64 r0 = (i64)blockIdx.x * chunk;
  const i64 r1 = r0 + chunk < rows ? r0 + chunk : rows;
  double s = 0.0;
  i64 r = r0;
  for (; r + 3 < r1; r += 4) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = src[(r + u) * B + b];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (!mask || !mask[r + u]) s += v[u];
  }
  for (; r < r1; ++r)
    if (!mask || !mask[r]) s += src[r * B + b];
  dst[(i64)blockIdx.x * B + b] = s;
}

// out[k * n + i] = (sum_{b < B} vals[(k * n + i) * Bv + b] * weight[b]) / B; one wave per node at a time, four slots of
// the row in flight.  Lane l sums its samples l, l + 64, ... in that order, then the fixed butterfly; lane k keeps slot k.
__global__ __launch_bounds__(256) void mean_operator_kernel(const double* __restrict__ vals,
                                                            const double* __restrict__ weight, int n, int W, int Bv,
                                                            int B, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double denom = (double)B;
  for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
    for (int k0 = 0; k0 < W; k0 += kWave) {      // rows wider than a wave: one store per 64 slots
      const int nk = W - k0 < kWave ? W - k0 : kWave;
      double mine = 0.0;
      for (int u0 = 0; u0 < nk; u0 += 4) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = lane; b < B; b += kWave) {
          const double wb = weight[b];
          double v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = k0 + (u0 + u < nk ? u0 + u : 0);     // an absent slot re-reads the first one and is not kept
            v[u] = vals[((i64)k * n + i) * Bv + b];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) s[u] += v[u] * wb;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          double t = s[u];
#pragma unroll
          for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d);
          if (lane == u0 + u) mine = t / denom;
        }
      }
      if (lane < nk) out[(i64)(k0 + lane) * n + i] = mine;
    }
  }
}

// c = max(-a, 0) / sqrt(d_i d_j), 0 where the product of the diagonals is not positive
__device__ __forceinline__ double coupling(double a, double di, double dj) {
  const double p = di * dj;
  const double m = a < 0.0 ? -a : 0.0;
  return p > 0.0 ? m / sqrt(p) : 0.0;
}

// One wave per row i, lane k < W = slot k.  W <= 64.
__global__ __launch_bounds__(256) void strength_filter_kernel(const double* __restrict__ abar,
                                                              const int* __restrict__ cols, int n, int W, double theta,
                                                              int* __restrict__ strong_cols,
                                                              double* __restrict__ filt) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
    const bool in = lane < W;
    const i64 ent = (i64)(in ? lane : 0) * n + i;
    const int j = cols[ent];
    const double a = abar[ent];
    const double dii = __shfl(a, 0);
    const bool real = in && lane > 0 && j != i;          // padding slots point at the row itself
    const double djj = real ? abar[j] : dii;
    const double c = real ? coupling(a, dii, djj) : 0.0;
    double rmax = c;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, d));
    bool strong = real && c > 0.0 && c >= theta * rmax;
    // the column's own row must agree: its coupling to i against its own row maximum, computed as its wave computes them
    double cji = 0.0, jmax = 0.0;
    if (real) {
      for (int kk = 1; kk < W; ++kk) {
        const i64 e2 = (i64)kk * n + j;
        const int l = cols[e2];
        if (l == j) continue;
        const double cjl = coupling(abar[e2], djj, abar[l]);
        jmax = fmax(jmax, cjl);
        if (l == i) cji = cjl;
      }
    }
    strong = strong && cji > 0.0 && cji >= theta * jmax;
    // weak and positive off-diagonals go to the diagonal, in slot order: the row sum is kept
    const double weak = (real && !strong) ? a : 0.0;
    double diag = dii;
    for (int k = 1; k < W; ++k) diag += __shfl(weak, k);
    if (in) {
      strong_cols[ent] = strong ? j : i;
      filt[ent] = lane == 0 ? diag : (strong ? a : 0.0);
    }
  }
}

inline unsigned wave_grid(int n) {
  i64 gx = ((i64)n + 3) / 4;
  if (gx > 16384) gx = 16384;
  return (unsigned)(gx < 1 ? 1 : gx);
}

}  // namespace

extern "C" int diffhe_ell_sample_scales(const double* vals, const unsigned char* is_bc, int n, int Bv, double* part,
                                        double* out, void* stream) {
  if (!vals || !part || !out || n < 1) return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  const int nblk = (n + kChunk - 1) / kChunk;
  const unsigned gy = (unsigned)((Bv + kWave - 1) / kWave);
  account(8.0 * Bv * ((double)n + 2.0 * nblk + 1.0));
  // slot 0 of the ELL values is the diagonal: rows (n, Bv)
  hipLaunchKernelGGL(sum_free_rows_kernel, dim3((unsigned)nblk, gy), dim3(64), 0, (hipStream_t)stream, vals, is_bc, n,
                     kChunk, Bv, part);
  hipLaunchKernelGGL(sum_free_rows_kernel, dim3(1, gy), dim3(64), 0, (hipStream_t)stream, (const double*)part,
                     (const unsigned char*)nullptr, nblk, nblk, Bv, out);
  return check_launch();
}

extern "C" int diffhe_ell_mean_operator(const double* vals, const double* weight, int n, int W, int Bv, int B,
                                        double* out, void* stream) {
  if (!vals || !weight || !out || n < 1 || W < 1 || B < 1 || B > Bv) return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bv)) return DIFFHE_E_BATCHPAD;
  account(8.0 * (double)W * n * ((double)B + 1.0));
  hipLaunchKernelGGL(mean_operator_kernel, dim3(wave_grid(n)), dim3(256), 0, (hipStream_t)stream, vals, weight, n, W, Bv,
                     B, out);
  return check_launch();
}

extern "C" int diffhe_ell_strength_filter(const double* abar, const int* cols, int n, int W, double theta,
                                          int* strong_cols, double* filt, void* stream) {
  if (!abar || !cols || !strong_cols || !filt || n < 1 || W < 1 || W > kWave || !(theta >= 0.0)) return DIFFHE_E_BADARG;
  account(8.0 * (double)W * n * 3.5);
  hipLaunchKernelGGL(strength_filter_kernel, dim3(wave_grid(n)), dim3(256), 0, (hipStream_t)stream, abar, cols, n, W,
                     theta, strong_cols, filt);
  return check_launch();
}
