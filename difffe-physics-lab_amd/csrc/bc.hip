// Per-sample Dirichlet data (ours: the reference keeps one Python dict of boundary values per mesh).  A solve with
// `dirichlet=` runs the path kernels with HOMOGENEOUS Dirichlet data; the kernels below add what G_b changes.  They
// touch only the boundary band -- the free nodes with a Dirichlet neighbour, the Dirichlet nodes, the elements that
// touch one -- so their cost is O(n^((d-1)/d) B), not O(n B):
//
//   diffhe_bc_lift:       rhs_b[i] -= (K_b[F, D] G_b)_i                 on the free band rows;
//   diffhe_bc_grad:       out_b[j] = gbar_b[j] - (K_b lambda_b)_j        on the Dirichlet nodes (dL/dG_b),
//                         optionally dots_b[j] = G_b[j] (K_1 lambda_b)_j  (unit kappa: the lift term of dL/dkappa_b);
//   diffhe_bc_scatter:    u_b[j] = G_b[j]                                 on the Dirichlet rows of the returned u;
//   diffhe_bc_grad_kappa: dk_eb -= lambda_b^T k0_e G_b                     on the elements that touch a Dirichlet node
//                         (the G part of -lambda^T k0_e u_e, per sample or summed over the batch).
//
// K_b[i, j] = sum_{e ni i, j} kappa_eb k0_e[p, q] is the UNREDUCED stiffness, gathered over per-plan incidence lists
// restricted to the band (diffhe/plan.py: SolvePlan.dirichlet_band) in a fixed order.  One wave per band row, lanes
// over samples; no floating-point atomics, so every result is bitwise reproducible.
#include "common.h"
#include "launch.h"

namespace {

using namespace diffhe;

constexpr int kMaxBlocks = 8192;   // grid.x cap of every kernel here

// sum_q [node q of e is (not) Dirichlet] k0_e[p, q] * v(q): the row p of an element matrix against nodal data
template <bool DIRICHLET_COLS>
__device__ inline double row_dot(const int* __restrict__ elems, int npe, int m, const double* __restrict__ k0,
                                 const int* __restrict__ d_slot, i64 e, int p, const double* __restrict__ v,
                                 i64 vsn, i64 vsb, int b) {
  double s = 0.0;
  for (int q = 0; q < npe; ++q) {
    const int node = elems[(i64)q * m + e];
    const int j = d_slot[node];
    if (DIRICHLET_COLS ? j < 0 : j >= 0) continue;
    const double val = DIRICHLET_COLS ? v[(i64)j * vsn + (i64)b * vsb] : v[(i64)node * vsn + (i64)b * vsb];
    s += k0[(i64)(p * npe + q) * m + e] * val;
  }
  return s;
}

__global__ __launch_bounds__(256) void bc_lift_kernel(const int* __restrict__ elems, int npe, int m,
                                                      const double* __restrict__ k0, const double* __restrict__ kappa,
                                                      i64 kse, i64 ksb, const int* __restrict__ d_slot,
                                                      const double* __restrict__ G, i64 gsj, i64 gsb,
                                                      const int* __restrict__ rows, const int* __restrict__ row_ptr,
                                                      const int* __restrict__ row_inc, int n_rows,
                                                      double* __restrict__ rhs, i64 rsn, i64 rsb, int B, int Bp) {
  const NodeMap nm = node_map(Bp);
  const int b = nm.b;
  if (b >= B) return;
  for (i64 r = nm.node0; r < n_rows; r += nm.stride) {
    double acc = 0.0;
    for (int t = row_ptr[r]; t < row_ptr[r + 1]; ++t) {
      const int code = row_inc[t];
      const i64 e = code / npe;
      const int p = code - (int)e * npe;
      const double kap = kappa ? kappa[e * kse + (i64)b * ksb] : 1.0;
      acc += kap * row_dot<true>(elems, npe, m, k0, d_slot, e, p, G, gsj, gsb, b);
    }
    rhs[(i64)rows[r] * rsn + (i64)b * rsb] -= acc;
  }
}

__global__ __launch_bounds__(256) void bc_grad_kernel(const int* __restrict__ elems, int npe, int m,
                                                      const double* __restrict__ k0, const double* __restrict__ kappa,
                                                      i64 kse, i64 ksb, const int* __restrict__ d_slot,
                                                      const int* __restrict__ d_idx, const int* __restrict__ d_ptr,
                                                      const int* __restrict__ d_inc, int n_d,
                                                      const double* __restrict__ lam, i64 lsn, i64 lsb,
                                                      const double* __restrict__ gbar, i64 gsn, i64 gsb,
                                                      double* __restrict__ out, i64 osj, i64 osb,
                                                      const double* __restrict__ G, i64 Gsj, i64 Gsb,
                                                      double* __restrict__ dots, int B, int Bp) {
  const NodeMap nm = node_map(Bp);
  const int b = nm.b;
  if (b >= B) return;
  for (i64 j = nm.node0; j < n_d; j += nm.stride) {
    double acc = 0.0, unit = 0.0;
    for (int t = d_ptr[j]; t < d_ptr[j + 1]; ++t) {
      const int code = d_inc[t];
      const i64 e = code / npe;
      const int p = code - (int)e * npe;
      const double s = row_dot<false>(elems, npe, m, k0, d_slot, e, p, lam, lsn, lsb, b);   // lambda = 0 on D
      acc += (kappa ? kappa[e * kse + (i64)b * ksb] : 1.0) * s;
      unit += s;
    }
    const double gb = gbar ? gbar[(i64)d_idx[j] * gsn + (i64)b * gsb] : 0.0;
    out[j * osj + (i64)b * osb] = gb - acc;
    if (dots) dots[j * B + b] = G[j * Gsj + (i64)b * Gsb] * unit;
  }
}

__global__ __launch_bounds__(256) void bc_scatter_kernel(const int* __restrict__ d_idx, int n_d,
                                                         const double* __restrict__ G, i64 gsj, i64 gsb,
                                                         double* __restrict__ u, i64 usn, i64 usb, int B, int Bp) {
  const NodeMap nm = node_map(Bp);
  const int b = nm.b;
  if (b >= B) return;
  for (i64 j = nm.node0; j < n_d; j += nm.stride)
    u[(i64)d_idx[j] * usn + (i64)b * usb] = G[j * gsj + (i64)b * gsb];
}

// one group of LB lanes per band element (group_map of launch.h); each lane loops over its samples b = sub, sub + LB, ...
// SHARED: the group reduces over the batch (group_sum) and lane 0 writes
template <bool SHARED>
__global__ __launch_bounds__(256) void bc_grad_kappa_kernel(const int* __restrict__ elems, int npe, int m,
                                                            const double* __restrict__ k0,
                                                            const int* __restrict__ d_slot,
                                                            const int* __restrict__ band_elems, int n_be,
                                                            const double* __restrict__ lam, i64 lsn, i64 lsb,
                                                            const double* __restrict__ G, i64 gsj, i64 gsb,
                                                            double* __restrict__ dk, i64 dse, i64 dsb, int B, int LB) {
  const GroupMap gm = group_map(LB);
  for (i64 r = gm.item0; r < n_be; r += gm.stride) {
    const i64 e = band_elems[r];
    double total = 0.0;
    for (int b = gm.sub; b < B; b += LB) {
      double s = 0.0;
      for (int p = 0; p < npe; ++p) {
        const int node = elems[(i64)p * m + e];
        if (d_slot[node] >= 0) continue;                          // lambda = 0 on D
        s += lam[(i64)node * lsn + (i64)b * lsb] * row_dot<true>(elems, npe, m, k0, d_slot, e, p, G, gsj, gsb, b);
      }
      if (SHARED)
        total += s;
      else
        dk[e * dse + (i64)b * dsb] -= s;
    }
    if (SHARED) {
      group_sum(LB, total);
      if (gm.sub == 0) dk[e * dse] -= total;
    }
  }
}

bool bad_mesh(const int* elems, int npe, int m, const double* k0, const int* d_slot) {
  return !elems || !k0 || !d_slot || npe < 2 || npe > 6 || m < 1 || (i64)m * npe >= (1LL << 31);
}

}  // namespace

extern "C" int diffhe_bc_lift(const int* elems, int npe, int m, const double* k0, const double* kappa, long long kse,
                              long long ksb, const int* d_slot, const double* G, long long gsj, long long gsb,
                              const int* rows, const int* row_ptr, const int* row_inc, int n_rows, double* rhs,
                              long long rsn, long long rsb, int B, void* stream) {
  if (bad_mesh(elems, npe, m, k0, d_slot) || !G || !rhs || B < 1 || n_rows < 0 || kse < 0 || ksb < 0 || gsj < 0 ||
      gsb < 0 || rsn < 0 || rsb < 0 || (n_rows > 0 && (!rows || !row_ptr || !row_inc)))
    return DIFFHE_E_BADARG;
  if (n_rows == 0) return DIFFHE_OK;
  const int Bp = batch_pad(B);
  account(8.0 * (2.0 * n_rows * B));
  hipLaunchKernelGGL(bc_lift_kernel, node_grid(n_rows, Bp, kMaxBlocks), dim3(256), 0, (hipStream_t)stream, elems, npe, m,
                     k0, kappa, kse, ksb, d_slot, G, gsj, gsb, rows, row_ptr, row_inc, n_rows, rhs, rsn, rsb, B, Bp);
  return check_launch();
}

extern "C" int diffhe_bc_grad(const int* elems, int npe, int m, const double* k0, const double* kappa, long long kse,
                              long long ksb, const int* d_slot, const int* d_idx, const int* d_ptr, const int* d_inc,
                              int n_d, const double* lam, long long lsn, long long lsb, const double* gbar,
                              long long gsn, long long gsb, double* out, long long osj, long long osb, const double* G,
                              long long Gsj, long long Gsb, double* dots, int B, void* stream) {
  if (bad_mesh(elems, npe, m, k0, d_slot) || !lam || !out || B < 1 || n_d < 0 || kse < 0 || ksb < 0 || lsn < 0 ||
      lsb < 0 || gsn < 0 || gsb < 0 || osj < 0 || osb < 0 || (dots && (!G || Gsj < 0 || Gsb < 0)) ||
      (n_d > 0 && (!d_idx || !d_ptr || !d_inc)))
    return DIFFHE_E_BADARG;
  if (n_d == 0) return DIFFHE_OK;
  const int Bp = batch_pad(B);
  account(8.0 * ((dots ? 3.0 : 2.0) * n_d * B));
  hipLaunchKernelGGL(bc_grad_kernel, node_grid(n_d, Bp, kMaxBlocks), dim3(256), 0, (hipStream_t)stream, elems, npe, m, k0,
                     kappa, kse, ksb, d_slot, d_idx, d_ptr, d_inc, n_d, lam, lsn, lsb, gbar, gsn, gsb, out, osj, osb, G,
                     Gsj, Gsb, dots, B, Bp);
  return check_launch();
}

extern "C" int diffhe_bc_scatter(const int* d_idx, int n_d, const double* G, long long gsj, long long gsb, double* u,
                                 long long usn, long long usb, int B, void* stream) {
  if (!G || !u || B < 1 || n_d < 0 || gsj < 0 || gsb < 0 || usn < 0 || usb < 0 || (n_d > 0 && !d_idx))
    return DIFFHE_E_BADARG;
  if (n_d == 0) return DIFFHE_OK;
  const int Bp = batch_pad(B);
  account(8.0 * (2.0 * n_d * B));
  hipLaunchKernelGGL(bc_scatter_kernel, node_grid(n_d, Bp, kMaxBlocks), dim3(256), 0, (hipStream_t)stream, d_idx, n_d, G,
                     gsj, gsb, u, usn, usb, B, Bp);
  return check_launch();
}

extern "C" int diffhe_bc_grad_kappa(const int* elems, int npe, int m, const double* k0, const int* d_slot,
                                    const int* band_elems, int n_be, const double* lam, long long lsn, long long lsb,
                                    const double* G, long long gsj, long long gsb, double* dk, long long dse,
                                    long long dsb, int shared, int B, void* stream) {
  if (bad_mesh(elems, npe, m, k0, d_slot) || !lam || !G || !dk || B < 1 || n_be < 0 || lsn < 0 || lsb < 0 ||
      gsj < 0 || gsb < 0 || dse < 0 || dsb < 0 || (n_be > 0 && !band_elems))
    return DIFFHE_E_BADARG;
  if (n_be == 0) return DIFFHE_OK;
  const int LB = group_lanes(B);
  account(8.0 * ((double)n_be * npe * B * 2.0 + (shared ? (double)n_be : 2.0 * n_be * B)));
  dispatch_bool(shared != 0, [&](auto SHARED) {
    hipLaunchKernelGGL(bc_grad_kappa_kernel<SHARED()>, dim3(group_grid(n_be, LB, kMaxBlocks)), dim3(256), 0,
                       (hipStream_t)stream, elems, npe, m, k0, d_slot, band_elems, n_be, lam, lsn, lsb, G, gsj, gsb, dk,
                       dse, dsb, B, LB);
  });
  return check_launch();
}
