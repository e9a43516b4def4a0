// Robin (convective) and flux boundary conditions (ours: the reference knows Dirichlet nodes and the natural zero-flux
// boundary only).  On a set of boundary facets F (end points of a chain, edges of triangles, faces of tetrahedra; d = 1,
// 2, 3 nodes)
//
//     kappa du/dn + h_F (u - uinf_F) = q_F,
//
// discretised with the consistent P1 facet mass M_F[p, q] = |F| (1 + delta_pq) / (d (d + 1)):
//
//   diffhe_robin_facet_table: |F| of every facet (1 for an end point), 0 for a degenerate one;
//   diffhe_robin_assemble:    vals += sum_F h_F M_F on the free rows (a Dirichlet column goes to the right-hand side with
//                             the Dirichlet value), rhs_p += (h_F uinf_F + q_F) |F| / d;
//   diffhe_robin_grad:        per facet and sample, from the adjoint lambda (0 on Dirichlet nodes) and u:
//                               s = (|F| / d) sum_p lambda_p,   dL/dq = s,   dL/duinf = h s,
//                               dL/dh = -lambda_F^T M_F u_F + uinf s   -- or their sums over the batch;
//   diffhe_robin_sum_facets:  the sum of such per-facet products over the facets, per sample, in two fixed-order stages.
//
// Only the boundary band is touched: O(n^((d-1)/d) B) work.  The gathers run over per-plan lists (diffhe/plan.py:
// SolvePlan.robin_table) in a fixed order, one group of lanes per band row / facet, lanes over samples; no
// floating-point atomics, so every result is bitwise reproducible.  h, uinf and q are read in place through a stride per
// facet and a stride per sample (0: shared), so every layout of the Python API -- (), (B,), (n_F,), (B, n_F), (n_F, B) --
// is one base pointer and two strides.
#include "common.h"
#include "launch.h"

namespace {

using namespace diffhe;
using Datum = Strided<const double>;   // h, uinf or q as the kernels read it
using Grad = Strided<double>;          // dL/dh, dL/duinf or dL/dq: a zero sample stride is the sum over the batch

constexpr int kSumChunk = 128;   // facets per block of the first summation stage

// |F| of a facet with nodes v[0 .. d-1]; coords (dim, n), dim = d
__device__ inline double facet_size(const double* __restrict__ coords, i64 n, int d, const int* v) {
  if (d == 1) return 1.0;
  if (d == 2) {
    const double dx = coords[v[1]] - coords[v[0]], dy = coords[n + v[1]] - coords[n + v[0]];
    const double len = sqrt(dx * dx + dy * dy);
    return len >= 1e-15 ? len : 0.0;                         // the absolute threshold of the triangle tables
  }
  double a[3], b[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = coords[k * n + v[1]] - coords[k * n + v[0]];
    b[k] = coords[k * n + v[2]] - coords[k * n + v[0]];
  }
  const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
  const double nrm = sqrt(cx * cx + cy * cy + cz * cz);
  const double l2 = fmax(a[0] * a[0] + a[1] * a[1] + a[2] * a[2], b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  return nrm > 1e-12 * l2 ? 0.5 * nrm : 0.0;                 // the relative threshold of the tetrahedron tables
}

__global__ __launch_bounds__(256) void facet_table_kernel(const double* __restrict__ coords,
                                                          const int* __restrict__ fac, int d, int n, int nF,
                                                          double* __restrict__ area) {
  for (i64 F = (i64)blockIdx.x * blockDim.x + threadIdx.x; F < nF; F += (i64)gridDim.x * blockDim.x) {
    int v[3];
    for (int p = 0; p < d; ++p) v[p] = fac[(i64)p * nF + F];
    area[F] = facet_size(coords, n, d, v);
  }
}

// one group of LB lanes per band row; lane -> sample b < Bp (padding samples b >= B: h = 1 where h comes per sample,
// uinf = q = 0 -- a well-posed dummy system with a zero right-hand side)
__global__ __launch_bounds__(256) void robin_assemble_kernel(
    const int* __restrict__ fac, int d, int nF, const double* __restrict__ area, const int* __restrict__ rows,
    const int* __restrict__ row_ptr, const int* __restrict__ ent_code, const int* __restrict__ ent_slot, int n_rows,
    const double* __restrict__ g, Datum h, Datum uinf, Datum q, double* __restrict__ vals, double* __restrict__ rhs,
    int n, int Bv, int B, int Bp) {
  const NodeMap nm = node_map(Bp);
  const int b = nm.b;
  if (b >= Bp) return;
  const bool real = b < B;
  const double inv_dd = 1.0 / (double)(d * (d + 1)), inv_d = 1.0 / (double)d;
  for (int r = nm.node0; r < n_rows; r += nm.stride) {
    const i64 i = rows[r];
    double load = 0.0;
    for (int t = row_ptr[r]; t < row_ptr[r + 1]; ++t) {
      const int code = ent_code[t], slot = ent_slot[t];
      const i64 F = code >> 4;
      const int p = (code >> 2) & 3, c = code & 3;
      const double a = area[F];
      const double hv = h.v ? ((real || h.sb == 0) ? h.at(F, b) : 1.0) : 0.0;
      const double mv = hv * (a * (p == c ? 2.0 : 1.0) * inv_dd);
      if (slot < 0) {                                        // Dirichlet column: lifted with its value (padding: rhs stays 0)
        if (real) load -= mv * g[fac[(i64)c * nF + F]];
      } else if (b < Bv)
        vals[((i64)slot * n + i) * Bv + b] += mv;
      if (p == c && real) {                                  // once per (facet, row): the facet load
        const double uv = uinf.v ? uinf.at(F, b) : 0.0;
        const double qv = q.v ? q.at(F, b) : 0.0;
        load += (hv * uv + qv) * (a * inv_d);
      }
    }
    rhs[i * Bp + b] += load;
  }
}

// one group of LB lanes per facet (group_map of launch.h), each lane loops over its samples b = sub, sub + LB, ...; an
// output with a zero sample stride is the sum over the batch: group_sum, lane 0 writes
__global__ __launch_bounds__(256) void robin_grad_kernel(
    const int* __restrict__ fac, int d, int nF, const double* __restrict__ area, const double* __restrict__ lam,
    const double* __restrict__ u, const double* __restrict__ g, int B, int Bp, Datum h, Datum uinf, Grad dh, Grad du,
    Grad dq, int LB) {
  const GroupMap gm = group_map(LB);
  const double inv_dd = 1.0 / (double)(d * (d + 1)), inv_d = 1.0 / (double)d;
  for (i64 F = gm.item0; F < nF; F += gm.stride) {
    int v[3];
    double gv[3];
    for (int p = 0; p < d; ++p) {
      v[p] = fac[(i64)p * nF + F];
      gv[p] = g ? g[v[p]] : 0.0;
    }
    const double a = area[F];
    double th = 0.0, tu = 0.0, tq = 0.0;
    for (int b = gm.sub; b < B; b += LB) {
      double le[3], ue[3], sl = 0.0, su = 0.0, lu = 0.0;
      for (int p = 0; p < d; ++p) {
        const i64 o = (i64)v[p] * Bp + b;
        le[p] = lam[o];
        ue[p] = u[o] + gv[p];
        sl += le[p];
        su += ue[p];
        lu += le[p] * ue[p];
      }
      const double s = sl * (a * inv_d);
      const double lmu = (sl * su + lu) * (a * inv_dd);       // lambda^T M_F u, M_F = |F| (1 1^T + I) / (d (d + 1))
      const double hv = h.v ? h.at(F, b) : 0.0;
      const double uv = uinf.v ? uinf.at(F, b) : 0.0;
      const double vh = uv * s - lmu, vu = hv * s;
      if (dh.v) { if (dh.sb) dh.at(F, b) = vh; else th += vh; }
      if (du.v) { if (du.sb) du.at(F, b) = vu; else tu += vu; }
      if (dq.v) { if (dq.sb) dq.at(F, b) = s; else tq += s; }
    }
    group_sum(LB, th, tu, tq);
    if (gm.sub == 0) {
      if (dh.v && !dh.sb) dh.at(F, 0) = th;
      if (du.v && !du.sb) du.at(F, 0) = tu;
      if (dq.v && !dq.sb) dq.at(F, 0) = tq;
    }
  }
}

// dst[blk, b] = sum of src[r, b] over the rows r of chunk blk, in row order; thread -> sample
__global__ __launch_bounds__(64) void sum_rows_kernel(const double* __restrict__ src, int rows, int chunk, int B,
                                                      double* __restrict__ dst) {
  const int b = blockIdx.y * kWave + threadIdx.x;
  if (b >= B) return;
  const i64 r0 = (i64)blockIdx.x * chunk;
  const i64 r1 = r0 + chunk < rows ? r0 + chunk : rows;
  double s = 0.0;
  for (i64 r = r0; r < r1; ++r) s += src[r * B + b];
  dst[(i64)blockIdx.x * B + b] = s;
}

bool bad_facets(const int* fac, int d, int nF, const double* area) {
  return !fac || !area || d < 1 || d > 3 || nF < 1 || nF >= (1 << 27);
}

}  // namespace

extern "C" int diffhe_robin_facet_table(const double* coords, const int* fac, int dim, int n, int nF, double* area,
                                        void* stream) {
  if (bad_facets(fac, dim, nF, area) || !coords || n < 1) return DIFFHE_E_BADARG;
  int gx = (nF + 255) / 256;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(facet_table_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, coords, fac, dim, n, nF, area);
  return check_launch();
}

extern "C" int diffhe_robin_assemble(const int* fac, int d, int nF, const double* area, const int* rows,
                                     const int* row_ptr, const int* ent_code, const int* ent_slot, int n_rows,
                                     const double* g, const double* h, long long hsf, long long hsb, const double* uinf,
                                     long long usf, long long usb, const double* q, long long qsf, long long qsb,
                                     double* vals, double* rhs, int n, int Bv, int B, int Bp, void* stream) {
  if (bad_facets(fac, d, nF, area) || !g || !vals || !rhs || n < 1 || n_rows < 0 || B < 1 || Bp < B ||
      (Bv != 1 && Bv != Bp) || hsf < 0 || hsb < 0 || usf < 0 || usb < 0 || qsf < 0 || qsb < 0 ||
      (h && hsb != 0 && Bv == 1 && Bp > 1) || (n_rows > 0 && (!rows || !row_ptr || !ent_code || !ent_slot)))
    return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  if (n_rows == 0) return DIFFHE_OK;
  account(8.0 * n_rows * ((double)d * Bv + 2.0 * Bp));
  hipLaunchKernelGGL(robin_assemble_kernel, node_grid(n_rows, Bp), dim3(256), 0, (hipStream_t)stream, fac, d, nF, area,
                     rows, row_ptr, ent_code, ent_slot, n_rows, g, Datum{h, hsf, hsb}, Datum{uinf, usf, usb},
                     Datum{q, qsf, qsb}, vals, rhs, n, Bv, B, Bp);
  return check_launch();
}

extern "C" int diffhe_robin_grad(const int* fac, int d, int nF, const double* area, const double* lam, const double* u,
                                 const double* g, int B, int Bp, const double* h, long long hsf, long long hsb,
                                 const double* uinf, long long usf, long long usb, double* dh, long long dhf,
                                 long long dhb, double* du, long long duf, long long dub, double* dq, long long dqf,
                                 long long dqb, void* stream) {
  if (bad_facets(fac, d, nF, area) || !lam || !u || B < 1 || Bp < B || hsf < 0 || hsb < 0 || usf < 0 || usb < 0 ||
      dhf < 0 || dhb < 0 || duf < 0 || dub < 0 || dqf < 0 || dqb < 0)
    return DIFFHE_E_BADARG;
  if (!dh && !du && !dq) return DIFFHE_OK;
  const int LB = group_lanes(B);
  account(8.0 * nF * (2.0 * d * B + 3.0 * B));
  hipLaunchKernelGGL(robin_grad_kernel, dim3(group_grid(nF, LB, 8192)), dim3(256), 0, (hipStream_t)stream, fac, d, nF,
                     area, lam, u, g, B, Bp, Datum{h, hsf, hsb}, Datum{uinf, usf, usb}, Grad{dh, dhf, dhb},
                     Grad{du, duf, dub}, Grad{dq, dqf, dqb}, LB);
  return check_launch();
}

extern "C" int diffhe_robin_sum_blocks(int nF) { return nF < 1 ? 0 : (nF + kSumChunk - 1) / kSumChunk; }

extern "C" int diffhe_robin_sum_facets(const double* src, int nF, int B, double* part, double* out, void* stream) {
  if (!src || !part || !out || nF < 1 || B < 1) return DIFFHE_E_BADARG;
  const int nblk = diffhe_robin_sum_blocks(nF);
  const unsigned gy = (unsigned)((B + kWave - 1) / kWave);
  account(8.0 * B * ((double)nF + 2.0 * nblk + 1.0));
  hipLaunchKernelGGL(sum_rows_kernel, dim3((unsigned)nblk, gy), dim3(64), 0, (hipStream_t)stream, src, nF, kSumChunk, B,
                     part);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1, gy), dim3(64), 0, (hipStream_t)stream, (const double*)part, nblk, nblk, B,
                     out);
  return check_launch();
}
