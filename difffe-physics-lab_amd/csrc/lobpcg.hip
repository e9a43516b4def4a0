// Block passes of the LOBPCG outer iteration (diffhe.eigen._BlockRun, iteration="lobpcg"; definitions:
// include/diffhe_lobpcg.h): the Gram matrices of the basis S = [X | W | P] against the carried blocks A S and B S, the dense
// Ritz step per sample with its fallback to a smaller basis, and the rotation that leaves X', P' and R'.  fp64, gfx950.
//
// Data layout as in eigen.hip and buckling.hip: a basis of q <= 48 vectors is (q, rows, Bp), batch innermost, lanes over
// samples (common.h, node_map) in the Gram and rotation passes; the Ritz step runs one wave per sample with its matrices in
// LDS.  Every reduction over the rows runs in two stages -- block partials in a fixed order, then a sum over the blocks in
// block order -- and nothing uses atomics: results are bitwise reproducible.  The packed Gram matrices are those of
// eigen.hip with q in the place of p: q(i, j) = i q - i (i - 1) / 2 + (j - i), i <= j.
#include "common.h"
#include "diffhe_lobpcg.h"
#include "launch.h"

#include <math.h>

namespace {

using namespace diffhe;

constexpr int kMaxP = 16;         // largest block (eigen.hip)
constexpr int kMaxQ = 3 * kMaxP;  // largest basis
constexpr int kTile = 4;          // column tile of the Gram pass
constexpr int kBlockCap = 32;     // row blocks of the Gram pass: 32 x 2 x 1176 x 64 x 8 B = 38.5 MB of partials at q = 48, Bp = 64
constexpr int kLdsEntries = 128;  // q x (output columns per pass) of the rotation: 128 x 64 lanes x 8 B = 64 KiB of LDS
constexpr int kLd = kMaxQ + 1;    // row stride of the Ritz matrices in LDS: odd, so a column walk meets every bank once
constexpr double kPivot = 1e-8;   // relative pivot test of the Cholesky factorisation: eigen.hip's, but stricter than its 1e-14,
                                  // because here it decides when P is given up ("LOBPCG")

__host__ __device__ inline int packed(int i, int j, int q) { return i * q - i * (i - 1) / 2 + (j - i); }

__host__ __device__ inline int lanes_of(int Bp) { return Bp < kWave ? Bp : kWave; }

bool bad_basis(int q, int rows, int Bp) { return q < 1 || q > kMaxQ || rows < 1 || (i64)q * rows * Bp >= (1LL << 40); }

// ---------------------------------------------------------------------------------------------------------------------
// Gram: GA[q(i, j)] = s_i . (A s)_j, GB[q(i, j)] = s_i . (B s)_j over the free rows.  blockIdx.z names a pair (I, J),
// I <= J, of column tiles of kTile, as in eigen.hip; 3 kTile loads per row.  part: (blocks, 2, nq, Bp), GA first.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lobpcg_gram_kernel(const double* __restrict__ S, const double* __restrict__ AS,
                                                           const double* __restrict__ BS,
                                                           const unsigned char* __restrict__ is_bc, int q, int n, int Bp,
                                                           int nt, double* __restrict__ part) {
  __shared__ double lds[4 * kWave];
  int I = 0, rem = blockIdx.z;
  for (int row = nt; rem >= row; --row) {
    rem -= row;
    ++I;
  }
  const int J = I + rem;
  const NodeMap nm = node_map(Bp);
  const i64 cs = (i64)n * Bp;
  double ga[kTile][kTile], gb[kTile][kTile];
#pragma unroll
  for (int s = 0; s < kTile; ++s)
#pragma unroll
    for (int t = 0; t < kTile; ++t) ga[s][t] = gb[s][t] = 0.0;
  for (int i = nm.node0; i < n; i += nm.stride) {
    if (is_bc && is_bc[i]) continue;
    const i64 o = (i64)i * Bp + nm.b;
    double si[kTile], aj[kTile], bj[kTile];
#pragma unroll
    for (int t = 0; t < kTile; ++t) {
      const int ci = I * kTile + t, cj = J * kTile + t;
      si[t] = ci < q ? S[ci * cs + o] : 0.0;
      aj[t] = cj < q ? AS[cj * cs + o] : 0.0;
      bj[t] = cj < q ? BS[cj * cs + o] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < kTile; ++s)
#pragma unroll
      for (int t = 0; t < kTile; ++t) {
        ga[s][t] += si[s] * aj[t];
        gb[s][t] += si[s] * bj[t];
      }
  }
  const int nq = q * (q + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int LB = lanes_of(Bp);
  double* dst = part + (i64)blockIdx.x * 2 * nq * Bp;
#pragma unroll
  for (int s = 0; s < kTile; ++s)
#pragma unroll
    for (int t = 0; t < kTile; ++t) {
      const int ci = I * kTile + s, cj = J * kTile + t;
      if (ci >= q || cj >= q || ci > cj) continue;      // block-uniform
      const double ra = block_sum_per_sample(ga[s][t], Bp, lds);
      const double rb = block_sum_per_sample(gb[s][t], Bp, lds);
      if (wave == 0 && lane < LB) {
        const int e = packed(ci, cj, q);
        dst[(i64)e * Bp + nm.b] = ra;
        dst[(i64)(nq + e) * Bp + nm.b] = rb;
      }
    }
}

// out[row, b] = sum over blk (in order) of part[blk, row, b]; rows = blockIdx.y, thread -> sample; rows below `split` go
// to out0, the others to out1
__global__ __launch_bounds__(64) void lobpcg_sum_blocks_kernel(const double* __restrict__ part, int nblk, int rows, int Bp,
                                                                double* __restrict__ out0, double* __restrict__ out1,
                                                                int split) {
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
// Ritz: one wave per sample, the matrices in LDS (three of 48 x 49 doubles, 55 KiB).  Both Gram matrices are scaled by
// diag(GB)^-1/2 from either side; GB = L L^T (right-looking Cholesky, the trailing update spread over the rows), At =
// L^-1 GA L^-T (lanes over columns, then over rows), cyclic Jacobi At = V diag(theta) V^T with the row and column updates
// of a rotation spread over the lanes, the p smallest theta ascending, C = diag(GB)^-1/2 L^-T V: C^T GA C = diag(theta),
// C^T GB C = I.  A factorisation that fails on the leading m x m block is tried again on m - p, down to p; `used` is read as
// well as written: a sample whose last step ran on fewer than q columns starts at max(that, 2p) -- P stays given up until
// the caller clears `used`.  The sweep, pair and lane orders are fixed, so the result is a function of the input alone.  Every
// branch below is wave-uniform.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 1; off < kWave; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(64) void lobpcg_ritz_kernel(const double* __restrict__ GA, const double* __restrict__ GB, int q,
                                                          int p, int Bp, int sweeps, double* __restrict__ C,
                                                          double* __restrict__ theta, int* __restrict__ used,
                                                          int* __restrict__ flag) {
  __shared__ double As[kMaxQ * kLd], Vs[kMaxQ * kLd], Ls[kMaxQ * kLd], sc[kMaxQ], dg[kMaxQ];
  __shared__ int perm[kMaxQ];
  const int b = blockIdx.x, lane = threadIdx.x;
  const i64 B = Bp;
  bool fin = true;
  for (int idx = lane; idx < q * q; idx += kWave) {      // the raw matrices: GA in As, GB in Vs
    const int r = idx / q, c = idx % q;
    const i64 e = (i64)(r <= c ? packed(r, c, q) : packed(c, r, q)) * B + b;
    const double a = GA[e], g = GB[e];
    As[r * kLd + c] = a;
    Vs[r * kLd + c] = g;
    fin = fin && isfinite(a) && isfinite(g);
  }
  fin = __all(fin);
  __syncthreads();
  int m = 0, top = q;
  const int cap = used[b];
  if (cap > 0 && cap < q && q > p) top = cap > 2 * p ? cap / p * p : 2 * p;      // a multiple of p, whatever `used` held
  for (int mm = top; fin && mm >= p && m == 0; mm -= p) {
    bool ok = true;
    for (int j = lane; j < mm; j += kWave) {
      const double d = Vs[j * kLd + j];
      ok = ok && d > 0.0;
      sc[j] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
    }
    ok = __all(ok);
    __syncthreads();
    if (!ok) continue;
    for (int idx = lane; idx < mm * mm; idx += kWave) {
      const int r = idx / mm, c = idx % mm;
      Ls[r * kLd + c] = Vs[r * kLd + c] * sc[r] * sc[c];
    }
    __syncthreads();
    for (int j = 0; j < mm; ++j) {
      const double d = Ls[j * kLd + j];      // one address: every lane reads the same pivot
      if (!(d > kPivot) || !isfinite(d)) {
        ok = false;
        break;
      }
      const double l = sqrt(d);
      __syncthreads();
      for (int i = j + lane; i < mm; i += kWave) Ls[i * kLd + j] = i == j ? l : Ls[i * kLd + j] / l;
      __syncthreads();
      for (int i = j + 1 + lane; i < mm; i += kWave) {      // row i of the trailing block, columns j + 1 .. i
        const double lij = Ls[i * kLd + j];
        for (int k = j + 1; k <= i; ++k) Ls[i * kLd + k] -= lij * Ls[k * kLd + j];
      }
      __syncthreads();
    }
    if (ok) m = mm;
  }
  if (m == 0) {      // not positive definite even on [X], or non-finite input: identity rotation, nothing non-finite leaves
    for (int idx = lane; idx < q * p; idx += kWave) C[(i64)idx * B + b] = idx / p == idx % p ? 1.0 : 0.0;
    if (lane < p) theta[(i64)lane * B + b] = 0.0;
    if (lane == 0) {
      used[b] = p;
      flag[b] = 1;
    }
    return;
  }
  for (int idx = lane; idx < m * m; idx += kWave) {
    const int r = idx / m, c = idx % m;
    As[r * kLd + c] *= sc[r] * sc[c];
  }
  __syncthreads();
  if (lane < m) {      // W = L^-1 GA: lane = column
    const int c = lane;
    for (int r = 0; r < m; ++r) {
      double s = As[r * kLd + c];
      for (int k = 0; k < r; ++k) s -= Ls[r * kLd + k] * As[k * kLd + c];
      As[r * kLd + c] = s / Ls[r * kLd + r];
    }
  }
  __syncthreads();
  if (lane < m) {      // At = W L^-T: lane = row
    const int r = lane;
    for (int c = 0; c < m; ++c) {
      double s = As[r * kLd + c];
      for (int k = 0; k < c; ++k) s -= As[r * kLd + k] * Ls[c * kLd + k];
      As[r * kLd + c] = s / Ls[c * kLd + c];
    }
  }
  __syncthreads();
  for (int idx = lane; idx < m * m; idx += kWave) {
    const int r = idx / m, c = idx % m;
    if (c > r) {
      const double a = 0.5 * (As[r * kLd + c] + As[c * kLd + r]);
      As[r * kLd + c] = a;
      As[c * kLd + r] = a;
    }
    Vs[r * kLd + c] = r == c ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int sw = 0; sw < sweeps; ++sw) {
    double off = 0.0, dd = 0.0;
    if (lane < m) {
      dd = As[lane * kLd + lane] * As[lane * kLd + lane];
      for (int c = lane + 1; c < m; ++c) off += As[lane * kLd + c] * As[lane * kLd + c];
    }
    off = wave_sum(off);
    dd = wave_sum(dd);
    if (off <= 1e-34 * dd) break;
    for (int r = 0; r < m - 1; ++r)
      for (int c = r + 1; c < m; ++c) {
        const double apq = As[r * kLd + c];
        if (apq == 0.0) continue;
        const double tau = (As[c * kLd + c] - As[r * kLd + r]) / (2.0 * apq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
        __syncthreads();
        if (lane < m) {      // A <- A P, V <- V P: lane = row
          const int k = lane;
          const double akp = As[k * kLd + r], akq = As[k * kLd + c];
          As[k * kLd + r] = cs * akp - sn * akq;
          As[k * kLd + c] = sn * akp + cs * akq;
          const double vkp = Vs[k * kLd + r], vkq = Vs[k * kLd + c];
          Vs[k * kLd + r] = cs * vkp - sn * vkq;
          Vs[k * kLd + c] = sn * vkp + cs * vkq;
        }
        __syncthreads();
        if (lane < m) {      // A <- P^T A: lane = column; the rotated pair itself becomes 0
          const int k = lane;
          const double apk = As[r * kLd + k], aqk = As[c * kLd + k];
          As[r * kLd + k] = k == c ? 0.0 : cs * apk - sn * aqk;
          As[c * kLd + k] = k == r ? 0.0 : sn * apk + cs * aqk;
        }
        __syncthreads();
      }
  }
  // ascending: the rank of every diagonal entry (ties by index); column perm[i] of V is the i-th Ritz vector
  if (lane < m) {
    dg[lane] = As[lane * kLd + lane];
    perm[lane] = lane;
  }
  __syncthreads();
  if (lane < m) {
    const double dj = dg[lane];
    int rank = 0;
    for (int i = 0; i < m; ++i) rank += (dg[i] < dj || (dg[i] == dj && i < lane)) ? 1 : 0;
    perm[rank] = lane;
    if (rank < p) theta[(i64)rank * B + b] = dj;
  }
  __syncthreads();
  if (lane < p) {      // C = diag(sc) L^-T V, in place: lane = output column
    const int pc = perm[lane];
    for (int j = m - 1; j >= 0; --j) {
      double s = Vs[j * kLd + pc];
      for (int l = j + 1; l < m; ++l) s -= Ls[l * kLd + j] * Vs[l * kLd + pc];
      Vs[j * kLd + pc] = s / Ls[j * kLd + j];
    }
    for (int j = 0; j < q; ++j) C[((i64)j * p + lane) * B + b] = j < m ? sc[j] * Vs[j * kLd + pc] : 0.0;
  }
  if (lane == 0) {
    used[b] = m;
    flag[b] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Rotate: X' = S C and P' = S C_P (C_P = C with its first p rows zeroed), the same combinations of A S and B S, and R' =
// A X' - theta B X' from the same registers.  The block's 64 samples share OC columns of C in LDS (q * OC <= kLdsEntries);
// blockIdx.z walks the output-column chunks.  The input columns are streamed: a lane holds 6 OC accumulators -- the sums
// over the X rows and over the other rows of C, for the three blocks -- and three loaded values at a time.  X' goes to
// column c and P' to column 2 p + c of the output basis; P' is written when q > p.
// ---------------------------------------------------------------------------------------------------------------------
template <int OC>
__global__ __launch_bounds__(256) void lobpcg_rotate_kernel(const double* __restrict__ S, const double* __restrict__ AS,
                                                             const double* __restrict__ BS, const double* __restrict__ C,
                                                             const double* __restrict__ theta, int q, int p, int n, int Bp,
                                                             double* __restrict__ S2, double* __restrict__ AS2,
                                                             double* __restrict__ BS2, double* __restrict__ R) {
  extern __shared__ double Cs[];
  const int LB = lanes_of(Bp);
  const int c0 = blockIdx.z * OC;
  const int b0 = blockIdx.y * kWave;
  for (int idx = threadIdx.x; idx < q * OC * LB; idx += 256) {
    const int lb = idx % LB, ji = idx / LB;
    const int j = ji / OC, ii = ji % OC;
    Cs[idx] = c0 + ii < p ? C[((i64)j * p + c0 + ii) * Bp + b0 + lb] : 0.0;
  }
  __syncthreads();
  const NodeMap nm = node_map(Bp);
  const int lb = (threadIdx.x & 63) % LB;
  const i64 cs = (i64)n * Bp;
  for (int i = nm.node0; i < n; i += nm.stride) {
    const i64 o = (i64)i * Bp + nm.b;
    double x[OC], ax[OC], bx[OC], px[OC], pa[OC], pb[OC];
#pragma unroll
    for (int ii = 0; ii < OC; ++ii) x[ii] = ax[ii] = bx[ii] = px[ii] = pa[ii] = pb[ii] = 0.0;
    for (int j = 0; j < p; ++j) {
      const double s = S[j * cs + o], a = AS[j * cs + o], bb = BS[j * cs + o];
#pragma unroll
      for (int ii = 0; ii < OC; ++ii) {
        const double c = Cs[(j * OC + ii) * LB + lb];
        x[ii] += s * c;
        ax[ii] += a * c;
        bx[ii] += bb * c;
      }
    }
    for (int j = p; j < q; ++j) {
      const double s = S[j * cs + o], a = AS[j * cs + o], bb = BS[j * cs + o];
#pragma unroll
      for (int ii = 0; ii < OC; ++ii) {
        const double c = Cs[(j * OC + ii) * LB + lb];
        px[ii] += s * c;
        pa[ii] += a * c;
        pb[ii] += bb * c;
      }
    }
#pragma unroll
    for (int ii = 0; ii < OC; ++ii) {
      if (c0 + ii >= p) continue;      // block-uniform
      const i64 w = (i64)(c0 + ii) * cs + o;
      const double xs = x[ii] + px[ii], as = ax[ii] + pa[ii], bs = bx[ii] + pb[ii];
      S2[w] = xs;
      AS2[w] = as;
      BS2[w] = bs;
      if (R) R[w] = as - theta[(i64)(c0 + ii) * Bp + nm.b] * bs;
      if (q > p) {
        const i64 wp = w + 2 * p * cs;
        S2[wp] = px[ii];
        AS2[wp] = pa[ii];
        BS2[wp] = pb[ii];
      }
    }
  }
}

}  // namespace

extern "C" int diffhe_lobpcg_gram_blocks(int rows, int Bp) {
  if (rows < 1 || !valid_batch_pad(Bp)) return 0;
  return (int)node_grid(rows, Bp, kBlockCap).x;
}

extern "C" int diffhe_lobpcg_gram(const double* S, const double* AS, const double* BS, const unsigned char* is_bc, int q,
                                  int rows, int Bp, double* part, double* GA, double* GB, void* stream) {
  if (!S || !AS || !BS || !part || !GA || !GB || bad_basis(q, rows, Bp)) return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nblk = diffhe_lobpcg_gram_blocks(rows, Bp);
  const int nt = (q + kTile - 1) / kTile, nq = q * (q + 1) / 2;
  const unsigned gy = (unsigned)((Bp + kWave - 1) / kWave);
  account(8.0 * Bp * (3.0 * q * rows + 2.0 * nq * (2.0 * nblk + 1.0)));
  hipLaunchKernelGGL(lobpcg_gram_kernel, dim3((unsigned)nblk, gy, (unsigned)(nt * (nt + 1) / 2)), dim3(256), 0,
                     (hipStream_t)stream, S, AS, BS, is_bc, q, rows, Bp, nt, part);
  hipLaunchKernelGGL(lobpcg_sum_blocks_kernel, dim3(gy, (unsigned)(2 * nq)), dim3(64), 0, (hipStream_t)stream,
                     (const double*)part, nblk, 2 * nq, Bp, GA, GB, nq);
  return check_launch();
}

extern "C" int diffhe_lobpcg_ritz(const double* GA, const double* GB, int q, int p, int Bp, int sweeps, double* C,
                                  double* theta, int* used, int* flag, void* stream) {
  if (!GA || !GB || !C || !theta || !used || !flag || p < 1 || p > kMaxP || Bp < 1 || sweeps < 1 ||
      (q != p && q != 2 * p && q != 3 * p))
    return DIFFHE_E_BADARG;
  const double nq = 0.5 * q * (q + 1);
  account(8.0 * Bp * (2.0 * nq + (double)q * p + p + 1.0));
  hipLaunchKernelGGL(lobpcg_ritz_kernel, dim3((unsigned)Bp), dim3(64), 0, (hipStream_t)stream, GA, GB, q, p, Bp, sweeps, C,
                     theta, used, flag);
  return check_launch();
}

extern "C" int diffhe_lobpcg_rotate(const double* S, const double* AS, const double* BS, const double* C,
                                    const double* theta, int q, int p, int rows, int Bp, double* S2, double* AS2,
                                    double* BS2, double* R, void* stream) {
  if (!S || !AS || !BS || !C || !S2 || !AS2 || !BS2 || (R && !theta) || p < 1 || p > kMaxP ||
      (q != p && q != 2 * p && q != 3 * p) || bad_basis(3 * p, rows, Bp))
    return DIFFHE_E_BADARG;
  const double* in[3] = {S, AS, BS};
  const double* out[4] = {S2, AS2, BS2, R};
  for (const double* a : in)
    for (const double* b : out)
      if (a == b) return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  int want = kLdsEntries / q;
  if (want > p) want = p;
  const int oc = want >= 8 ? 8 : want >= 4 ? 4 : want >= 2 ? 2 : 1;
  const int passes = (p + oc - 1) / oc;
  const dim3 g = node_grid(rows, Bp, 1024);
  const dim3 grid(g.x, g.y, (unsigned)passes);
  const size_t lds = sizeof(double) * (size_t)q * oc * lanes_of(Bp);
  // each pass streams the q input columns of the three blocks; 3 (X') + 3 (P') + 1 (R') output columns per column of C
  account(8.0 * Bp * (double)rows * (3.0 * q * passes + p * (3.0 + (q > p ? 3.0 : 0.0) + (R ? 1.0 : 0.0))));
  hipStream_t st = (hipStream_t)stream;
#define DIFFHE_LOBPCG_ROTATE(OC)                                                                                      \
  hipLaunchKernelGGL((lobpcg_rotate_kernel<OC>), grid, dim3(256), lds, st, S, AS, BS, C, theta, q, p, rows, Bp, S2, AS2, \
                     BS2, R)
  if (oc == 8)
    DIFFHE_LOBPCG_ROTATE(8);
  else if (oc == 4)
    DIFFHE_LOBPCG_ROTATE(4);
  else if (oc == 2)
    DIFFHE_LOBPCG_ROTATE(2);
  else
    DIFFHE_LOBPCG_ROTATE(1);
#undef DIFFHE_LOBPCG_ROTATE
  return check_launch();
}
