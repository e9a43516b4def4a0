// Linear buckling of elastic bodies (diffhe.buckling): the geometric stiffness K_G = G (x) I_d applied from the NODE
// pattern, the block passes of the iteration on the pencil N phi = mu K phi, whose right-hand matrix is a block K Y and not
// a diagonal mass, and the cotangent of the prestress (definitions: include/diffhe_buckling.h).  G itself is assembled by
// diffhe_aniso_assemble_rows (aniso.hip) with the stress in the conductivity's place.
//
// Data layout as in elastic.hip and eigen.hip: batch innermost, lanes over samples (node_map), so node ids, element sizes
// and list entries are wave-uniform and every access is one contiguous segment; a block of p <= 16 vectors is
// (p, rows, Bp).  fp64, no atomics: every reduction runs in two stages -- block partials in a fixed order, then a sum over
// the blocks in block order -- and results are bitwise reproducible.
#include "common.h"
#include "diffhe_buckling.h"
#include "element_grad.h"
#include "launch.h"

namespace {

using namespace diffhe;

constexpr int kMaxP = 16;         // largest block (eigen.hip)
constexpr int kTile = 4;          // column tile of the Gram pass
constexpr int kLdsEntries = 128;  // p x (output columns per pass) of the rotation: 128 x 64 lanes x 8 B = 64 KiB of LDS

__host__ __device__ inline int packed(int i, int j, int p) { return i * p - i * (i - 1) / 2 + (j - i); }

__host__ __device__ inline int lanes_of(int Bp) { return Bp < kWave ? Bp : kWave; }

bool bad_block(int p, int n, int Bp) { return p < 1 || p > kMaxP || n < 1 || (i64)p * n * Bp >= (1LL << 40); }

// ---------------------------------------------------------------------------------------------------------------------
// Apply: one lane per (node, sample) walks the node's W entries of G; each value meets the D components of its column
// node, D contiguous segments of x.  The operator bytes are those of the node pattern, 1 / D^2 of the dof operator's.
// ---------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void buckling_apply_kernel(const double* __restrict__ G, const int* __restrict__ cols,
                                                              const unsigned char* __restrict__ is_bc,
                                                              const double* __restrict__ x, double* __restrict__ y,
                                                              double scale, int n, int W, int Bp, int Bv) {
  const NodeMap nm = node_map(Bp);
  if (nm.b >= Bp) return;
  const int vb = Bv == 1 ? 0 : nm.b;
  for (int i = nm.node0; i < n; i += nm.stride) {
    double acc[D];
#pragma unroll
    for (int a = 0; a < D; ++a) acc[a] = 0.0;
    auto entry = [&](int k) {
      const i64 ent = (i64)k * n + i;
      const int j = cols[ent];
      const double g = G[ent * Bv + vb];
      const double* __restrict__ xj = x + (i64)j * D * Bp + nm.b;
#pragma unroll
      for (int a = 0; a < D; ++a) acc[a] = fma(g, xj[(i64)a * Bp], acc[a]);
    };
    // tetrahedral patterns are wide (W = 15 and more): four entries in flight measured 0.78x the plain loop at
    // box(32, 32, 32) x 16; on triangles (W = 7) the same unrolling measured 1.28x at 512^2 x 64, its remainder loop
    if constexpr (D == 3) {
#pragma unroll 4
      for (int k = 0; k < W; ++k) entry(k);
    } else {
      for (int k = 0; k < W; ++k) entry(k);
    }
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const i64 row = (i64)i * D + a;
      y[row * Bp + nm.b] = (is_bc && is_bc[row]) ? 0.0 : scale * acc[a];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Step: y = coef x + dx with the block partials of dx . r per sample.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void buckling_step_kernel(const double* __restrict__ x, const double* __restrict__ dx,
                                                             const double* __restrict__ r, const double* __restrict__ coef,
                                                             int rows, int Bp, double* __restrict__ y,
                                                             double* __restrict__ part) {
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);
  const bool ok = nm.b < Bp;
  double s = 0.0;
  if (ok) {
    const double c = coef[nm.b];
    for (int i = nm.node0; i < rows; i += nm.stride) {
      const i64 o = (i64)i * Bp + nm.b;
      const double di = dx[o];
      y[o] = fma(c, x[o], di);
      s = fma(di, r[o], s);
    }
  }
  store_block_partial(s, part, Bp, nm.b, ok, lds);
}

// out[row, b] = sum over blk (in order) of part[blk, row, b]; rows = blockIdx.y, thread -> sample; rows below `split` go
// to out0, the others to out1
__global__ __launch_bounds__(64) void buckling_sum_blocks_kernel(const double* __restrict__ part, int nblk, int rows,
                                                                  int Bp, double* __restrict__ out0,
                                                                  double* __restrict__ out1, int split) {
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
// Gram: GK[q(i, j)] = y_i . (K y)_j, GN[q(i, j)] = y_i . (N y)_j over the free rows.  blockIdx.z names a pair (I, J),
// I <= J, of column tiles of kTile, as in eigen.hip; 3 kTile loads per row.  part: (blocks, 2, nq, Bp), GK first.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void buckling_gram_kernel(const double* __restrict__ Y, const double* __restrict__ KY,
                                                             const double* __restrict__ NY,
                                                             const unsigned char* __restrict__ is_bc, int p, int n, int Bp,
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
  double gk[kTile][kTile], gn[kTile][kTile];
#pragma unroll
  for (int s = 0; s < kTile; ++s)
#pragma unroll
    for (int t = 0; t < kTile; ++t) gk[s][t] = gn[s][t] = 0.0;
  for (int i = nm.node0; i < n; i += nm.stride) {
    if (is_bc && is_bc[i]) continue;
    const i64 o = (i64)i * Bp + nm.b;
    double yi[kTile], kj[kTile], nj[kTile];
#pragma unroll
    for (int t = 0; t < kTile; ++t) {
      const int ci = I * kTile + t, cj = J * kTile + t;
      yi[t] = ci < p ? Y[ci * cs + o] : 0.0;
      kj[t] = cj < p ? KY[cj * cs + o] : 0.0;
      nj[t] = cj < p ? NY[cj * cs + o] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < kTile; ++s)
#pragma unroll
      for (int t = 0; t < kTile; ++t) {
        gk[s][t] += yi[s] * kj[t];
        gn[s][t] += yi[s] * nj[t];
      }
  }
  const int nq = p * (p + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int LB = lanes_of(Bp);
  double* dst = part + (i64)blockIdx.x * 2 * nq * Bp;
#pragma unroll
  for (int s = 0; s < kTile; ++s)
#pragma unroll
    for (int t = 0; t < kTile; ++t) {
      const int ci = I * kTile + s, cj = J * kTile + t;
      if (ci >= p || cj >= p || ci > cj) continue;      // block-uniform
      const double rk = block_sum_per_sample(gk[s][t], Bp, lds);
      const double rn = block_sum_per_sample(gn[s][t], Bp, lds);
      if (wave == 0 && lane < LB) {
        const int q = packed(ci, cj, p);
        dst[(i64)q * Bp + nm.b] = rk;
        dst[(i64)(nq + q) * Bp + nm.b] = rn;
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Rotate: X = Y C, KX = KY C, NX = NY C and R = NX - mu KX from the same registers.  The block's 64 samples share `oc`
// columns of C in LDS (p * oc <= kLdsEntries); blockIdx.z walks the output-column chunks.
// ---------------------------------------------------------------------------------------------------------------------
template <int PT>
__global__ __launch_bounds__(256) void buckling_rotate_kernel(const double* __restrict__ Y, const double* __restrict__ KY,
                                                               const double* __restrict__ NY, const double* __restrict__ C,
                                                               const double* __restrict__ mu, int p, int n, int Bp, int oc,
                                                               double* __restrict__ X, double* __restrict__ KX,
                                                               double* __restrict__ NX, double* __restrict__ R) {
  extern __shared__ double Cs[];
  const int LB = lanes_of(Bp);
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
    double y[PT], ky[PT], ny[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      y[j] = j < p ? Y[j * cs + o] : 0.0;
      ky[j] = j < p ? KY[j * cs + o] : 0.0;
      ny[j] = j < p ? NY[j * cs + o] : 0.0;
    }
    for (int ii = 0; ii < ocz; ++ii) {
      double x = 0.0, kx = 0.0, nx = 0.0;
#pragma unroll
      for (int j = 0; j < PT; ++j)
        if (j < p) {
          const double c = Cs[(j * ocz + ii) * LB + lb];
          x += y[j] * c;
          kx += ky[j] * c;
          nx += ny[j] * c;
        }
      const i64 w = (i64)(c0 + ii) * cs + o;
      X[w] = x;
      KX[w] = kx;
      NX[w] = nx;
      R[w] = nx - mu[(i64)(c0 + ii) * Bp + nm.b] * kx;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// d lambda / d sigma0 as a form of element_grad.h (NC = Voigt components): vol_e sum_i w[i, b] sum_a g_{i,a} g_{i,a}^T with
// g_{i,a} = sum_p X[i, (el_p, a), b] grad N_p, the off-diagonal components doubled (one parameter fills two entries).
// ---------------------------------------------------------------------------------------------------------------------
template <int DIM>
struct GradSigmaForm {
  static constexpr int NC = DIM * (DIM + 1) / 2;
  static constexpr int NPE = DIM + 1;
  const int* __restrict__ elems;
  const double* __restrict__ gtab;
  const double* __restrict__ vol;
  const double* __restrict__ X;
  const double* __restrict__ w;
  int k, n, m, B;

  struct Elem {
    int node[NPE];
    double G[NPE][DIM], ve;
  };

  __device__ __forceinline__ void load(int e, Elem& el) const {
#pragma unroll
    for (int p = 0; p < NPE; ++p) {
      el.node[p] = elems[(i64)p * m + e];
#pragma unroll
      for (int t = 0; t < DIM; ++t) el.G[p][t] = gtab[(i64)(p * DIM + t) * m + e];
    }
    el.ve = vol[e];
  }

  __device__ __forceinline__ void eval(const Elem& el, int Bp, int b, double* out) const {
#pragma unroll
    for (int c = 0; c < NC; ++c) out[c] = 0.0;
    if (b >= B) return;
    const i64 cs = (i64)n * DIM * Bp;
    double S[DIM][DIM];      // upper triangle used
#pragma unroll
    for (int s = 0; s < DIM; ++s)
#pragma unroll
      for (int t = 0; t < DIM; ++t) S[s][t] = 0.0;
    for (int i = 0; i < k; ++i) {
      const double* __restrict__ x = X + i * cs + b;
      const double wi = w[(i64)i * Bp + b];
      double q[DIM][DIM];
#pragma unroll
      for (int s = 0; s < DIM; ++s)
#pragma unroll
        for (int t = 0; t < DIM; ++t) q[s][t] = 0.0;
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        double g[DIM];
#pragma unroll
        for (int t = 0; t < DIM; ++t) g[t] = 0.0;
#pragma unroll
        for (int p = 0; p < NPE; ++p) {
          const double v = x[((i64)el.node[p] * DIM + a) * Bp];
#pragma unroll
          for (int t = 0; t < DIM; ++t) g[t] = fma(v, el.G[p][t], g[t]);
        }
#pragma unroll
        for (int s = 0; s < DIM; ++s)
#pragma unroll
          for (int t = s; t < DIM; ++t) q[s][t] = fma(g[s], g[t], q[s][t]);
      }
#pragma unroll
      for (int s = 0; s < DIM; ++s)
#pragma unroll
        for (int t = s; t < DIM; ++t) S[s][t] = fma(wi, q[s][t], S[s][t]);
    }
    if constexpr (DIM == 2) {
      out[0] = el.ve * S[0][0];
      out[1] = el.ve * S[1][1];
      out[2] = 2.0 * el.ve * S[0][1];
    } else {
      out[0] = el.ve * S[0][0];
      out[1] = el.ve * S[1][1];
      out[2] = el.ve * S[2][2];
      out[3] = 2.0 * el.ve * S[1][2];
      out[4] = 2.0 * el.ve * S[0][2];
      out[5] = 2.0 * el.ve * S[0][1];
    }
  }
};

bool bad_grad(const int* elems, const double* gtab, const double* vol, int dim, const double* X, const double* w, int k,
              int n, int m, int B, int Bp) {
  return !elems || !gtab || !vol || !X || !w || (dim != 2 && dim != 3) || k < 1 || k > kMaxP || n < 1 || m < 1 || B < 1 ||
         B > Bp;
}

}  // namespace

extern "C" int diffhe_buckling_apply(const double* G, const int* cols, const unsigned char* is_bc, const double* x,
                                     double* y, double scale, int n, int W, int d, int Bp, int Bv, void* stream) {
  if (!G || !cols || !x || !y || x == y || (d != 2 && d != 3) || n < 1 || W < 1 || (Bv != 1 && Bv != Bp))
    return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  account(8.0 * ((Bv > 1 ? (double)Bv * W * n : 0.0) + 2.0 * (double)Bp * d * n));   // G once (shared: 0), x and y
  dispatch_dim<2, 3>(d, [&](auto D) {
    hipLaunchKernelGGL(buckling_apply_kernel<D()>, node_grid(n, Bp), dim3(256), 0, (hipStream_t)stream, G, cols, is_bc, x, y,
                       scale, n, W, Bp, Bv);
  });
  return check_launch();
}

extern "C" int diffhe_buckling_step(const double* x, const double* dx, const double* r, const double* coef, int rows,
                                    int Bp, double* y, double* part, double* dot, void* stream) {
  if (!x || !dx || !r || !coef || !y || !part || !dot || rows < 1) return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const dim3 grid = node_grid(rows, Bp);
  if ((int)grid.x != diffhe_grad_kappa_blocks(rows, Bp)) return DIFFHE_E_BADARG;   // part is sized by that entry
  account(8.0 * Bp * (4.0 * rows + 2.0 * grid.x + 2.0));
  hipLaunchKernelGGL(buckling_step_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, dx, r, coef, rows, Bp, y, part);
  hipLaunchKernelGGL(buckling_sum_blocks_kernel, dim3(grid.y, 1), dim3(64), 0, (hipStream_t)stream, (const double*)part,
                     (int)grid.x, 1, Bp, dot, dot, 1);
  return check_launch();
}

extern "C" int diffhe_buckling_gram(const double* Y, const double* KY, const double* NY, const unsigned char* is_bc, int p,
                                    int rows, int Bp, double* part, double* GK, double* GN, void* stream) {
  if (!Y || !KY || !NY || !part || !GK || !GN || bad_block(p, rows, Bp)) return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nblk = diffhe_eig_gram_blocks(rows, Bp);
  const int nt = (p + kTile - 1) / kTile, nq = p * (p + 1) / 2;
  const unsigned gy = (unsigned)((Bp + kWave - 1) / kWave);
  account(8.0 * Bp * (3.0 * p * rows + 2.0 * nq * (2.0 * nblk + 1.0)));
  hipLaunchKernelGGL(buckling_gram_kernel, dim3((unsigned)nblk, gy, (unsigned)(nt * (nt + 1) / 2)), dim3(256), 0,
                     (hipStream_t)stream, Y, KY, NY, is_bc, p, rows, Bp, nt, part);
  hipLaunchKernelGGL(buckling_sum_blocks_kernel, dim3(gy, (unsigned)(2 * nq)), dim3(64), 0, (hipStream_t)stream,
                     (const double*)part, nblk, 2 * nq, Bp, GK, GN, nq);
  return check_launch();
}

extern "C" int diffhe_buckling_rotate(const double* Y, const double* KY, const double* NY, const double* C,
                                      const double* mu, int p, int rows, int Bp, double* X, double* KX, double* NX,
                                      double* R, void* stream) {
  if (!Y || !KY || !NY || !C || !mu || !X || !KX || !NX || !R || bad_block(p, rows, Bp)) return DIFFHE_E_BADARG;
  const double* in[3] = {Y, KY, NY};
  const double* out[4] = {X, KX, NX, R};
  for (const double* a : in)
    for (const double* b : out)
      if (a == b) return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  int oc = kLdsEntries / p;
  if (oc > p) oc = p;
  const int passes = (p + oc - 1) / oc;
  const dim3 g = node_grid(rows, Bp, 1024);
  const dim3 grid(g.x, g.y, (unsigned)passes);
  const size_t lds = sizeof(double) * (size_t)p * oc * lanes_of(Bp);
  account(8.0 * Bp * (double)rows * p * 7.0);
  hipStream_t st = (hipStream_t)stream;
#define DIFFHE_BUCKLING_ROTATE(PT)                                                                                       \
  hipLaunchKernelGGL((buckling_rotate_kernel<PT>), grid, dim3(256), lds, st, Y, KY, NY, C, mu, p, rows, Bp, oc, X, KX, NX, R)
  if (p <= 4)
    DIFFHE_BUCKLING_ROTATE(4);
  else if (p <= 8)
    DIFFHE_BUCKLING_ROTATE(8);
  else if (p <= 12)
    DIFFHE_BUCKLING_ROTATE(12);
  else
    DIFFHE_BUCKLING_ROTATE(16);
#undef DIFFHE_BUCKLING_ROTATE
  return check_launch();
}

extern "C" int diffhe_buckling_grad_sigma(const int* elems, const double* gtab, const double* vol, int dim, const double* X,
                                          const double* w, int k, int n, int m, int B, int Bp, double* ds_e, long long o_sc,
                                          long long o_se, double* ds_part, double* ds_sum, void* stream) {
  if (bad_grad(elems, gtab, vol, dim, X, w, k, n, m, B, Bp)) return DIFFHE_E_BADARG;
  if (!ds_e && !ds_part) return DIFFHE_E_BADARG;
  if ((ds_part == nullptr) != (ds_sum == nullptr)) return DIFFHE_E_BADARG;
  if (ds_e && (o_sc < 1 || o_se < 1)) return DIFFHE_E_BADARG;
  const int nc = dim == 2 ? 3 : 6;
  const double bytes = 8.0 * Bp * ((double)k * dim * n + k + (ds_e ? (double)nc * m : 0));
  return dispatch_dim<2, 3>(dim, [&](auto D) {
    return launch_element_grad(GradSigmaForm<D()>{elems, gtab, vol, X, w, k, n, m, B}, m, Bp, ds_e, o_sc, o_se, ds_part,
                               ds_sum, bytes, stream);
  });
}

extern "C" int diffhe_buckling_grad_sigma_shared(const int* elems, const double* gtab, const double* vol, int dim,
                                                 const double* X, const double* w, int k, int n, int m, int B, int Bp,
                                                 double* ds, long long o_sc, long long o_se, void* stream) {
  if (bad_grad(elems, gtab, vol, dim, X, w, k, n, m, B, Bp) || !ds || o_sc < 1 || o_se < 1) return DIFFHE_E_BADARG;
  const int nc = dim == 2 ? 3 : 6;
  const double bytes = 8.0 * (Bp * ((double)k * dim * n + k) + (double)nc * m);
  return dispatch_dim<2, 3>(dim, [&](auto D) {
    return launch_element_grad_shared(GradSigmaForm<D()>{elems, gtab, vol, X, w, k, n, m, B}, m, B, Bp, ds, o_sc, o_se,
                                      bytes, stream);
  });
}
