// Block machinery of the batched eigensolver (diffhe.eigen): per-sample Gram matrices of a block of vectors, a small dense
// Rayleigh-Ritz per sample, the block rotation and the residual norms.  fp64, gfx950.
//
// A block of p <= 16 vectors is stored (p, n, Bp): column c is the ready (n, Bp) right-hand side at c * n * Bp, batch
// innermost, lanes over samples (common.h, node_map).  Every reduction over the nodes runs in two stages -- block
// partials in a fixed order, then a sum over the blocks in block order -- and nothing uses atomics: results are bitwise
// reproducible.  Small per-sample matrices are (rows, cols, Bp), entry (r, c) of sample b at (r * p + c) * Bp + b; the
// symmetric Gram matrices are packed by rows of their upper triangle, q(i, j) = i p - i (i - 1) / 2 + (j - i), i <= j.
//
// The passes that weigh rows by the mass read it through an accessor, a template argument: NodalMass is one (n,) vector
// the batch shares, mass[row] -- the diffhe_eig_* entries (diffhe.eigen) -- and SampleMass<D> a nodal mass per sample
// under D unknowns per node, mass[(row / D) * ms + b * mb] with row = node * D + component -- the diffhe_modal_* entries
// (diffhe.modal, include/diffhe_modal.h).  D is a compile-time constant: no integer division runs in the row loops.
#include "common.h"
#include "diffhe_modal.h"
#include "launch.h"

#include <math.h>

namespace {

using namespace diffhe;

constexpr int kMaxP = 16;       // largest block
constexpr int kTile = 4;        // column tile of the Gram pass: 2 x 16 accumulators next to 12 loads per node
constexpr int kLdsEntries = 128;  // p x (output columns per pass) of the rotation: 128 x 64 lanes x 8 B = 64 KiB of LDS

__host__ __device__ inline int packed(int i, int j, int p) { return i * p - i * (i - 1) / 2 + (j - i); }

struct NodalMass {
  const double* __restrict__ m;
  __device__ __forceinline__ double operator()(int row, int) const { return m[row]; }
};

template <int D>
struct SampleMass {
  const double* __restrict__ m;
  i64 ms, mb;
  __device__ __forceinline__ double operator()(int row, int b) const { return m[(i64)(row / D) * ms + (i64)b * mb]; }
};

inline int lanes_of(int Bp) { return Bp < kWave ? Bp : kWave; }

inline int reduce_blocks(int n, int Bp) {
  const int gy = (Bp + kWave - 1) / kWave;
  int cap = 512 / gy;
  if (cap < 32) cap = 32;
  return (int)node_grid(n, Bp, cap).x;
}

// ---------------------------------------------------------------------------------------------------------------------
// Gram: GA[q(i, j)] = y_i . (A y)_j, GM[q(i, j)] = y_i . M y_j over the free rows.  blockIdx.z names a pair (I, J), I <= J,
// of column tiles of kTile; a diagonal pair reads 2 kTile columns per node, an off-diagonal one 3 kTile.
// part: (blocks, 2, nq, Bp) block partials, GA first.
// ---------------------------------------------------------------------------------------------------------------------
template <class Mass>
__global__ __launch_bounds__(256) void gram_kernel(const double* __restrict__ Y, const double* __restrict__ AY,
                                                   const Mass mass,
                                                   const unsigned char* __restrict__ is_bc, int p, int n, int Bp, int nt,
                                                   double* __restrict__ part) {
  __shared__ double lds[4 * kWave];
  int I = 0, rem = blockIdx.z;
  for (int row = nt; rem >= row; --row) {
    rem -= row;
    ++I;
  }
  const int J = I + rem;
  const NodeMap nm = node_map(Bp);
  const i64 cs = (i64)n * Bp;
  double ga[kTile][kTile], gm[kTile][kTile];
#pragma unroll
  for (int s = 0; s < kTile; ++s)
#pragma unroll
    for (int t = 0; t < kTile; ++t) ga[s][t] = gm[s][t] = 0.0;
  for (int i = nm.node0; i < n; i += nm.stride) {
    if (is_bc && is_bc[i]) continue;
    const i64 o = (i64)i * Bp + nm.b;
    const double mi = mass(i, nm.b);
    double yi[kTile], yj[kTile], aj[kTile];
#pragma unroll
    for (int t = 0; t < kTile; ++t) {
      const int ci = I * kTile + t, cj = J * kTile + t;
      yi[t] = ci < p ? Y[ci * cs + o] : 0.0;
      aj[t] = cj < p ? AY[cj * cs + o] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < kTile; ++t) {
      const int cj = J * kTile + t;
      yj[t] = I == J ? yi[t] : (cj < p ? Y[cj * cs + o] : 0.0);
    }
#pragma unroll
    for (int s = 0; s < kTile; ++s) {
      const double ms = mi * yi[s];
#pragma unroll
      for (int t = 0; t < kTile; ++t) {
        ga[s][t] += yi[s] * aj[t];
        gm[s][t] += ms * yj[t];
      }
    }
  }
  const int nq = p * (p + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int LB = Bp < kWave ? Bp : kWave;
  double* dst = part + (i64)blockIdx.x * 2 * nq * Bp;
#pragma unroll
  for (int s = 0; s < kTile; ++s)
#pragma unroll
    for (int t = 0; t < kTile; ++t) {
      const int ci = I * kTile + s, cj = J * kTile + t;
      if (ci >= p || cj >= p || ci > cj) continue;      // block-uniform
      const double ra = block_sum_per_sample(ga[s][t], Bp, lds);
      const double rm = block_sum_per_sample(gm[s][t], Bp, lds);
      if (wave == 0 && lane < LB) {
        const int q = packed(ci, cj, p);
        dst[(i64)q * Bp + nm.b] = ra;
        dst[(i64)(nq + q) * Bp + nm.b] = rm;
      }
    }
}

// out[row, b] = sum over blk (in order) of part[blk, row, b]; rows = blockIdx.y, thread -> sample
__global__ __launch_bounds__(64) void sum_blocks_kernel(const double* __restrict__ part, int nblk, int rows, int Bp,
                                                        double* __restrict__ out0, double* __restrict__ out1, int split) {
  const int b = blockIdx.x * kWave + threadIdx.x;
  const int row = blockIdx.y;
  if (b >= Bp) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += part[((i64)k * rows + row) * Bp + b];
  if (row < split)
    out0[(i64)row * Bp + b] = s;
  else
    out1[(i64)(row - split) * Bp + b] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Ritz: one sample per lane.  GM = L L^T (Cholesky), At = L^-1 GA L^-T, cyclic Jacobi At = V diag(theta) V^T, eigenvalues
// sorted ascending, C = L^-T V: C^T GA C = diag(theta), C^T GM C = I.  The lane's matrices live in caller-owned global
// memory (work: At then L, p p Bp doubles each; C holds V), every access coalesced over the samples.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ritz_kernel(const double* __restrict__ GA, const double* __restrict__ GM, int p,
                                                  int Bp, int sweeps, double* __restrict__ work, double* __restrict__ C,
                                                  double* __restrict__ theta, int* __restrict__ flag) {
  const int b = blockIdx.x * kWave + threadIdx.x;
  if (b >= Bp) return;
  const i64 B = Bp;
  double* At = work;
  double* Lw = work + (i64)p * p * B;
#define AT(r, c) At[((i64)(r) * p + (c)) * B + b]
#define LL(r, c) Lw[((i64)(r) * p + (c)) * B + b]
#define VV(r, c) C[((i64)(r) * p + (c)) * B + b]
#define SYM(G, r, c) G[(i64)((r) <= (c) ? packed((r), (c), p) : packed((c), (r), p)) * B + b]
  bool ok = true;
  for (int j = 0; j < p && ok; ++j) {
    const double gjj = SYM(GM, j, j);
    double d = gjj;
    for (int k = 0; k < j; ++k) d -= LL(j, k) * LL(j, k);
    if (!(gjj > 0.0) || !(d > 1e-14 * gjj) || !isfinite(d)) {
      ok = false;
      break;
    }
    const double l = sqrt(d);
    LL(j, j) = l;
    for (int i = j + 1; i < p; ++i) {
      double s = SYM(GM, j, i);
      for (int k = 0; k < j; ++k) s -= LL(i, k) * LL(j, k);
      LL(i, j) = s / l;
    }
  }
  if (ok)
    for (int q = 0; q < p * (p + 1) / 2; ++q) ok = ok && isfinite(GA[(i64)q * B + b]);
  if (!ok) {      // GM not positive definite (or non-finite input): identity rotation, nothing non-finite leaves
    flag[b] = 1;
    for (int r = 0; r < p; ++r) {
      theta[(i64)r * B + b] = 0.0;
      for (int c = 0; c < p; ++c) VV(r, c) = r == c ? 1.0 : 0.0;
    }
    return;
  }
  flag[b] = 0;
  // W = L^-1 GA, column by column
  for (int c = 0; c < p; ++c)
    for (int r = 0; r < p; ++r) {
      double s = SYM(GA, r, c);
      for (int k = 0; k < r; ++k) s -= LL(r, k) * AT(k, c);
      AT(r, c) = s / LL(r, r);
    }
  // At = W L^-T, row by row
  for (int r = 0; r < p; ++r)
    for (int c = 0; c < p; ++c) {
      double s = AT(r, c);
      for (int k = 0; k < c; ++k) s -= AT(r, k) * LL(c, k);
      AT(r, c) = s / LL(c, c);
    }
  for (int r = 0; r < p; ++r)
    for (int c = 0; c < p; ++c) {
      if (c > r) {
        const double a = 0.5 * (AT(r, c) + AT(c, r));
        AT(r, c) = a;
        AT(c, r) = a;
      }
      VV(r, c) = r == c ? 1.0 : 0.0;
    }
  for (int sw = 0; sw < sweeps; ++sw) {
    double off = 0.0, dg = 0.0;
    for (int r = 0; r < p; ++r) {
      dg += AT(r, r) * AT(r, r);
      for (int c = r + 1; c < p; ++c) off += AT(r, c) * AT(r, c);
    }
    if (off <= 1e-34 * dg) break;
    for (int r = 0; r < p - 1; ++r)
      for (int c = r + 1; c < p; ++c) {
        const double apq = AT(r, c);
        if (apq == 0.0) continue;
        const double tau = (AT(c, c) - AT(r, r)) / (2.0 * apq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
        for (int k = 0; k < p; ++k) {      // A <- A P, V <- V P
          const double akp = AT(k, r), akq = AT(k, c);
          AT(k, r) = cs * akp - sn * akq;
          AT(k, c) = sn * akp + cs * akq;
          const double vkp = VV(k, r), vkq = VV(k, c);
          VV(k, r) = cs * vkp - sn * vkq;
          VV(k, c) = sn * vkp + cs * vkq;
        }
        for (int k = 0; k < p; ++k) {      // A <- P^T A
          const double apk = AT(r, k), aqk = AT(c, k);
          AT(r, k) = cs * apk - sn * aqk;
          AT(c, k) = sn * apk + cs * aqk;
        }
        AT(r, c) = 0.0;
        AT(c, r) = 0.0;
      }
  }
  for (int i = 0; i < p - 1; ++i) {      // ascending: selection sort of the diagonal, columns of V follow
    int m = i;
    double vm = AT(i, i);
    for (int j = i + 1; j < p; ++j) {
      const double v = AT(j, j);
      if (v < vm) {
        vm = v;
        m = j;
      }
    }
    if (m != i) {
      AT(m, m) = AT(i, i);
      AT(i, i) = vm;
      for (int k = 0; k < p; ++k) {
        const double v = VV(k, i);
        VV(k, i) = VV(k, m);
        VV(k, m) = v;
      }
    }
  }
  for (int c = 0; c < p; ++c) {          // C = L^-T V, in place
    theta[(i64)c * B + b] = AT(c, c);
    for (int j = p - 1; j >= 0; --j) {
      double s = VV(j, c);
      for (int l = j + 1; l < p; ++l) s -= LL(l, j) * VV(l, c);
      VV(j, c) = s / LL(j, j);
    }
  }
#undef AT
#undef LL
#undef VV
#undef SYM
}

// ---------------------------------------------------------------------------------------------------------------------
// Rotate: X = Y C, AX = AY C and, from the same registers, MX = M X and R = theta M X - A X (each optional).  The block's
// 64 samples share `oc` columns of C in LDS (p * oc <= kLdsEntries); blockIdx.z walks the output-column chunks.
// ---------------------------------------------------------------------------------------------------------------------
template <int PT, class Mass>
__global__ __launch_bounds__(256) void rotate_kernel(const double* __restrict__ Y, const double* __restrict__ AY,
                                                     const double* __restrict__ C, const double* __restrict__ theta,
                                                     const Mass mass, int p, int n, int Bp, int oc,
                                                     double* __restrict__ X, double* __restrict__ AX,
                                                     double* __restrict__ MX, double* __restrict__ R) {
  extern __shared__ double Cs[];
  const int LB = Bp < kWave ? Bp : kWave;
  const int c0 = blockIdx.z * oc;
  const int ocz = (p - c0) < oc ? (p - c0) : oc;
  const int b0 = blockIdx.y * kWave;
  for (int idx = threadIdx.x; idx < p * ocz * LB; idx += 256) {
    const int lb = idx % LB, ji = idx / LB;
    const int j = ji / ocz, ii = ji % ocz;
    Cs[idx] = C[((i64)j * p + c0 + ii) * Bp + b0 + lb];
  }
  __syncthreads();
  const NodeMap nm = node_map(Bp);
  const int lb = (threadIdx.x & 63) % LB;
  const i64 cs = (i64)n * Bp;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    const double mi = mass(i, nm.b);
    double y[PT], a[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      y[j] = j < p ? Y[j * cs + o] : 0.0;
      a[j] = j < p ? AY[j * cs + o] : 0.0;
    }
    for (int ii = 0; ii < ocz; ++ii) {
      double x = 0.0, ax = 0.0;
#pragma unroll
      for (int j = 0; j < PT; ++j)
        if (j < p) {
          const double c = Cs[(j * ocz + ii) * LB + lb];
          x += y[j] * c;
          ax += a[j] * c;
        }
      const i64 w = (i64)(c0 + ii) * cs + o;
      X[w] = x;
      AX[w] = ax;
      if (MX) MX[w] = mi * x;
      if (R) R[w] = theta[(i64)(c0 + ii) * Bp + nm.b] * (mi * x) - ax;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Residual: part[blk, c, b] = sum over the nodes of the block of R[c, i, b]^2 / m_i; blockIdx.z = column.
// ---------------------------------------------------------------------------------------------------------------------
template <class Mass>
__global__ __launch_bounds__(256) void resid_kernel(const double* __restrict__ R, const Mass mass, int p,
                                                    int n, int Bp, double* __restrict__ part) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const int c = blockIdx.z;
  const double* r = R + (i64)c * n * Bp;
  double acc = 0.0;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const double v = r[(i64)i * Bp + nm.b];
    const double mi = mass(i, nm.b);
    if (mi > 0.0) acc += v * v / mi;
  }
  const double s = block_sum_per_sample(acc, Bp, lds);
  const int LB = Bp < kWave ? Bp : kWave;
  if ((threadIdx.x >> 6) == 0 && (threadIdx.x & 63) < LB) part[((i64)blockIdx.x * p + c) * Bp + nm.b] = s;
}

__global__ __launch_bounds__(64) void resid_final_kernel(const double* __restrict__ part, const double* __restrict__ theta,
                                                         int nblk, int p, int Bp, double* __restrict__ rho) {
  const int b = blockIdx.x * kWave + threadIdx.x;
  const int c = blockIdx.y;
  if (b >= Bp) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += part[((i64)k * p + c) * Bp + b];
  const double th = fabs(theta[(i64)c * Bp + b]);
  rho[(i64)c * Bp + b] = th > 0.0 ? sqrt(s) / th : 1e300;
}

// ---------------------------------------------------------------------------------------------------------------------
// Sign convention of the returned vectors: sum_i m_i x_i > 0; where that sum is below 1e-8 in magnitude, the entry of
// largest magnitude is positive.  part[blk, c, {sum, entry}, b]; comparisons are strict and run in a fixed order.
// ---------------------------------------------------------------------------------------------------------------------
__device__ inline double larger_mag(double a, double b) { return fabs(b) > fabs(a) ? b : a; }

template <class Mass>
__global__ __launch_bounds__(256) void sign_kernel(const double* __restrict__ X, const Mass mass, int k,
                                                   int n, int Bp, double* __restrict__ part) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const int c = blockIdx.z;
  const double* x = X + (i64)c * n * Bp;
  double acc = 0.0, e = 0.0;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const double v = x[(i64)i * Bp + nm.b];
    acc += mass(i, nm.b) * v;
    e = larger_mag(e, v);
  }
  const int LB = Bp < kWave ? Bp : kWave;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int off = LB; off < kWave; off <<= 1) e = larger_mag(e, __shfl_xor(e, off));
  lds[wave * kWave + lane] = e;
  __syncthreads();
  if (wave == 0) e = larger_mag(larger_mag(lds[lane], lds[kWave + lane]), larger_mag(lds[2 * kWave + lane], lds[3 * kWave + lane]));
  __syncthreads();
  const double s = block_sum_per_sample(acc, Bp, lds);
  if (wave == 0 && lane < LB) {
    double* dst = part + ((i64)blockIdx.x * k + c) * 2 * Bp;
    dst[nm.b] = s;
    dst[Bp + nm.b] = e;
  }
}

__global__ __launch_bounds__(64) void sign_final_kernel(const double* __restrict__ part, int nblk, int k, int Bp,
                                                        double* __restrict__ sgn) {
  const int b = blockIdx.x * kWave + threadIdx.x;
  const int c = blockIdx.y;
  if (b >= Bp) return;
  double s = 0.0, e = 0.0;
  for (int j = 0; j < nblk; ++j) {
    const double* src = part + ((i64)j * k + c) * 2 * Bp;
    s += src[b];
    e = larger_mag(e, src[Bp + b]);
  }
  sgn[(i64)c * Bp + b] = fabs(s) >= 1e-8 ? (s < 0.0 ? -1.0 : 1.0) : (e < 0.0 ? -1.0 : 1.0);
}

__global__ __launch_bounds__(256) void flip_kernel(double* __restrict__ X, const double* __restrict__ sgn, int n, int Bp) {
  const NodeMap nm = node_map(Bp);
  const int c = blockIdx.z;
  if (sgn[(i64)c * Bp + nm.b] >= 0.0) return;
  double* x = X + (i64)c * n * Bp;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    x[o] = -x[o];
  }
}

bool bad_block(int p, int n, int Bp) { return p < 1 || p > kMaxP || n < 1 || (i64)p * n * Bp >= (1LL << 40); }

// ---------------------------------------------------------------------------------------------------------------------
// Host side of the four mass-weighted passes, once for both accessors.  mass_bytes: the algorithmic bytes of the mass, read once (0 for
// a vector the batch shares, as everywhere in account()).
// ---------------------------------------------------------------------------------------------------------------------
template <class Mass>
int launch_gram(const double* Y, const double* AY, const Mass mass, double mass_bytes, const unsigned char* is_bc, int p,
                int n, int Bp, double* part, double* GA, double* GM, void* stream) {
  if (!Y || !AY || !mass.m || !part || !GA || !GM || bad_block(p, n, Bp)) return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nblk = reduce_blocks(n, Bp);
  const int nt = (p + kTile - 1) / kTile, nq = p * (p + 1) / 2;
  const unsigned gy = (unsigned)((Bp + kWave - 1) / kWave);
  account(8.0 * Bp * (2.0 * p * n + 2.0 * nq * (2.0 * nblk + 1.0)) + mass_bytes);
  hipLaunchKernelGGL(gram_kernel<Mass>, dim3((unsigned)nblk, gy, (unsigned)(nt * (nt + 1) / 2)), dim3(256), 0,
                     (hipStream_t)stream, Y, AY, mass, is_bc, p, n, Bp, nt, part);
  hipLaunchKernelGGL(sum_blocks_kernel, dim3(gy, (unsigned)(2 * nq)), dim3(64), 0, (hipStream_t)stream,
                     (const double*)part, nblk, 2 * nq, Bp, GA, GM, nq);
  return check_launch();
}

template <class Mass>
int launch_rotate(const double* Y, const double* AY, const double* C, const double* theta, const Mass mass,
                  double mass_bytes, int p, int n, int Bp, double* X, double* AX, double* MX, double* R, void* stream) {
  if (!Y || !AY || !C || !mass.m || !X || !AX || (R && !theta) || bad_block(p, n, Bp) || X == Y || AX == AY || X == AY ||
      AX == Y)
    return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  int oc = kLdsEntries / p;
  if (oc > p) oc = p;
  const int passes = (p + oc - 1) / oc;
  const dim3 g = node_grid(n, Bp, 1024);
  const dim3 grid(g.x, g.y, (unsigned)passes);
  const size_t lds = sizeof(double) * (size_t)p * oc * lanes_of(Bp);
  account(8.0 * Bp * (double)n * p * (2.0 + 2.0 + (MX ? 1.0 : 0.0) + (R ? 1.0 : 0.0)) + mass_bytes);
  hipStream_t st = (hipStream_t)stream;
#define DIFFHE_ROTATE(PT)                                                                                            \
  hipLaunchKernelGGL((rotate_kernel<PT, Mass>), grid, dim3(256), lds, st, Y, AY, C, theta, mass, p, n, Bp, oc, X, AX, MX, \
                     R)
  if (p <= 4)
    DIFFHE_ROTATE(4);
  else if (p <= 8)
    DIFFHE_ROTATE(8);
  else if (p <= 12)
    DIFFHE_ROTATE(12);
  else
    DIFFHE_ROTATE(16);
#undef DIFFHE_ROTATE
  return check_launch();
}

template <class Mass>
int launch_residual(const double* R, const double* theta, const Mass mass, double mass_bytes, int p, int n, int Bp,
                    double* part, double* rho, void* stream) {
  if (!R || !theta || !mass.m || !part || !rho || bad_block(p, n, Bp)) return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nblk = reduce_blocks(n, Bp);
  const unsigned gy = (unsigned)((Bp + kWave - 1) / kWave);
  account(8.0 * Bp * ((double)p * n + p * (2.0 * nblk + 1.0)) + mass_bytes);
  hipLaunchKernelGGL(resid_kernel<Mass>, dim3((unsigned)nblk, gy, (unsigned)p), dim3(256), 0, (hipStream_t)stream, R, mass,
                     p, n, Bp, part);
  hipLaunchKernelGGL(resid_final_kernel, dim3(gy, (unsigned)p), dim3(64), 0, (hipStream_t)stream, (const double*)part,
                     theta, nblk, p, Bp, rho);
  return check_launch();
}

template <class Mass>
int launch_fix_sign(double* X, const Mass mass, double mass_bytes, int k, int n, int Bp, double* part, double* sgn,
                    void* stream) {
  if (!X || !mass.m || !part || !sgn || bad_block(k, n, Bp)) return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nblk = reduce_blocks(n, Bp);
  const unsigned gy = (unsigned)((Bp + kWave - 1) / kWave);
  account(8.0 * Bp * (double)k * n * 3.0 + mass_bytes);
  hipLaunchKernelGGL(sign_kernel<Mass>, dim3((unsigned)nblk, gy, (unsigned)k), dim3(256), 0, (hipStream_t)stream,
                     (const double*)X, mass, k, n, Bp, part);
  hipLaunchKernelGGL(sign_final_kernel, dim3(gy, (unsigned)k), dim3(64), 0, (hipStream_t)stream, (const double*)part, nblk,
                     k, Bp, sgn);
  const dim3 g = node_grid(n, Bp, 1024);
  hipLaunchKernelGGL(flip_kernel, dim3(g.x, g.y, (unsigned)k), dim3(256), 0, (hipStream_t)stream, X, (const double*)sgn, n,
                     Bp);
  return check_launch();
}

// f(SampleMass<d>, bytes of one read of the mass) for the d of a diffhe_modal_* call; n counts rows, node * d + component
template <class F>
int with_sample_mass(const double* mass, i64 ms, i64 mb, int d, int n, int Bp, F&& f) {
  if (d < 1 || d > 3 || n % d != 0 || ms < 0 || mb < 0) return DIFFHE_E_BADARG;
  const double bytes = mb ? 8.0 * Bp * (double)(n / d) : 0.0;
  return dispatch_dim<1, 3>(d, [&](auto D) { return f(SampleMass<D()>{mass, ms, mb}, bytes); });
}

}  // namespace

extern "C" int diffhe_eig_gram_blocks(int n, int Bp) {
  if (n < 1 || !valid_batch_pad(Bp)) return 0;
  return reduce_blocks(n, Bp);
}

extern "C" int diffhe_eig_gram(const double* Y, const double* AY, const double* mass, const unsigned char* is_bc, int p,
                               int n, int Bp, double* part, double* GA, double* GM, void* stream) {
  return launch_gram(Y, AY, NodalMass{mass}, 0.0, is_bc, p, n, Bp, part, GA, GM, stream);
}

extern "C" int diffhe_eig_ritz(const double* GA, const double* GM, int p, int Bp, int sweeps, double* work, double* C,
                               double* theta, int* flag, void* stream) {
  if (!GA || !GM || !work || !C || !theta || !flag || p < 1 || p > kMaxP || Bp < 1 || sweeps < 1) return DIFFHE_E_BADARG;
  hipLaunchKernelGGL(ritz_kernel, dim3((unsigned)((Bp + kWave - 1) / kWave)), dim3(64), 0, (hipStream_t)stream, GA, GM, p,
                     Bp, sweeps, work, C, theta, flag);
  return check_launch();
}

extern "C" int diffhe_eig_rotate(const double* Y, const double* AY, const double* C, const double* theta,
                                 const double* mass, int p, int n, int Bp, double* X, double* AX, double* MX, double* R,
                                 void* stream) {
  return launch_rotate(Y, AY, C, theta, NodalMass{mass}, 0.0, p, n, Bp, X, AX, MX, R, stream);
}

extern "C" int diffhe_eig_residual(const double* R, const double* theta, const double* mass, int p, int n, int Bp,
                                   double* part, double* rho, void* stream) {
  return launch_residual(R, theta, NodalMass{mass}, 0.0, p, n, Bp, part, rho, stream);
}

extern "C" int diffhe_eig_fix_sign(double* X, const double* mass, int k, int n, int Bp, double* part, double* sgn,
                                   void* stream) {
  return launch_fix_sign(X, NodalMass{mass}, 0.0, k, n, Bp, part, sgn, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// The same four passes with a nodal mass per sample under d unknowns per node (include/diffhe_modal.h).
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int diffhe_modal_gram(const double* Y, const double* AY, const double* mass, long long ms, long long mb, int d,
                                 const unsigned char* is_bc, int p, int n, int Bp, double* part, double* GA, double* GM,
                                 void* stream) {
  return with_sample_mass(mass, ms, mb, d, n, Bp, [&](auto acc, double bytes) {
    return launch_gram(Y, AY, acc, bytes, is_bc, p, n, Bp, part, GA, GM, stream);
  });
}

extern "C" int diffhe_modal_rotate(const double* Y, const double* AY, const double* C, const double* theta,
                                   const double* mass, long long ms, long long mb, int d, int p, int n, int Bp, double* X,
                                   double* AX, double* MX, double* R, void* stream) {
  return with_sample_mass(mass, ms, mb, d, n, Bp, [&](auto acc, double bytes) {
    return launch_rotate(Y, AY, C, theta, acc, bytes, p, n, Bp, X, AX, MX, R, stream);
  });
}

extern "C" int diffhe_modal_residual(const double* R, const double* theta, const double* mass, long long ms, long long mb,
                                     int d, int p, int n, int Bp, double* part, double* rho, void* stream) {
  return with_sample_mass(mass, ms, mb, d, n, Bp, [&](auto acc, double bytes) {
    return launch_residual(R, theta, acc, bytes, p, n, Bp, part, rho, stream);
  });
}

extern "C" int diffhe_modal_fix_sign(double* X, const double* mass, long long ms, long long mb, int d, int k, int n,
                                     int Bp, double* part, double* sgn, void* stream) {
  return with_sample_mass(mass, ms, mb, d, n, Bp, [&](auto acc, double bytes) {
    return launch_fix_sign(X, acc, bytes, k, n, Bp, part, sgn, stream);
  });
}
