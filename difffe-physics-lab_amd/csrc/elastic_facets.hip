// Tractions, pressure and elastic (Winkler) foundations on boundary facets of elastic bodies (ours: the reference solves
// scalar equations only), include/diffhe_elastic_facets.h.  On facets F (edges of triangles, faces of tetrahedra; d = 2,
// 3 nodes) with the OUTWARD unit normal n_F
//
//     sigma(u) n = t_F - p_F n_F - S_F u,      S_F = kn_F n_F n_F^T + kt_F (I - n_F n_F^T),
//
// discretised with the consistent P1 facet mass M_F[p, q] = |F| (1 + delta_pq) / (d (d + 1)) of csrc/robin.hip:
//
//   diffhe_elastf_facet_table: |F| and n_F of every facet, oriented away from the owner's opposite node; 0 and 0 for a
//                              degenerate facet;
//   diffhe_elastf_assemble:    vals += sum_F M_F[p,c] S_F as d x d blocks of the dof ELL rows (slots: diffhe_elastic.h) on
//                              the free rows, a fixed column goes to the right-hand side with its value;
//                              rhs[(p,a)] += (t_F[a] - p_F n_F[a]) |F| / d;
//   diffhe_elastf_grad:        per facet and sample, from the adjoint lambda (0 on fixed dofs) and u:
//                                s = (|F| / d) sum_p lambda_p,  dL/dt = s,  dL/dp = -s . n,
//                                dL/dkn = -sum M_F[p,q] (lambda_p . n)(u_q . n),
//                                dL/dkt = -sum M_F[p,q] lambda_p . u_q - dL/dkn   -- or their sums over the batch.
//
// Only the boundary band is touched: O(n^((d-1)/d) B) work.  The gathers run over per-plan lists (diffhe/plan.py:
// SolvePlan.elastic_facet_table) in a fixed order, one group of lanes per band node / facet, lanes over samples, batch
// innermost: the (., Bp) vectors are read and written coalesced.  Every sum has a fixed order and every entry one writer,
// so every result is bitwise reproducible.  t, p, kn, kt are read in place through a stride per facet, per component and
// per sample (0: shared): every layout of the Python API is one base pointer and its strides.
#include "common.h"
#include "diffhe_elastic_facets.h"
#include "launch.h"

namespace {

using namespace diffhe;
using Datum = Strided<const double>;   // a scalar facet datum as the kernels read it
using Grad = Strided<double>;          // a scalar facet gradient: a zero sample stride is the sum over the batch

template <int DIM>
__global__ __launch_bounds__(256) void elastf_table_kernel(const double* __restrict__ coords, const int* __restrict__ fac,
                                                            const int* __restrict__ opp, int n, int nF,
                                                            double* __restrict__ area, double* __restrict__ normal) {
  for (i64 F = (i64)blockIdx.x * blockDim.x + threadIdx.x; F < nF; F += (i64)gridDim.x * blockDim.x) {
    double X[DIM][DIM], xo[DIM], nv[DIM];
#pragma unroll
    for (int p = 0; p < DIM; ++p) {
      const i64 v = fac[(i64)p * nF + F];
#pragma unroll
      for (int k = 0; k < DIM; ++k) X[p][k] = coords[(i64)k * n + v];
    }
#pragma unroll
    for (int k = 0; k < DIM; ++k) xo[k] = coords[(i64)k * n + opp[F]];
    double size = 0.0, nrm = 0.0;
    if constexpr (DIM == 2) {
      const double dx = X[1][0] - X[0][0], dy = X[1][1] - X[0][1];
      nrm = sqrt(dx * dx + dy * dy);
      nv[0] = dy;
      nv[1] = -dx;
      size = nrm >= 1e-15 ? nrm : 0.0;                       // the absolute threshold of the triangle tables
    } else {
      double a[3], b[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a[k] = X[1][k] - X[0][k];
        b[k] = X[2][k] - X[0][k];
      }
      nv[0] = a[1] * b[2] - a[2] * b[1];
      nv[1] = a[2] * b[0] - a[0] * b[2];
      nv[2] = a[0] * b[1] - a[1] * b[0];
      nrm = sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
      const double l2 = fmax(a[0] * a[0] + a[1] * a[1] + a[2] * a[2], b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
      size = nrm > 1e-12 * l2 ? 0.5 * nrm : 0.0;             // the relative threshold of the tetrahedron tables
    }
    double out = 0.0;                                        // (x_0 - x_opp) . nv > 0: nv points away from the owner
#pragma unroll
    for (int k = 0; k < DIM; ++k) out += (X[0][k] - xo[k]) * nv[k];
    const double sc = size > 0.0 ? (out >= 0.0 ? 1.0 : -1.0) / nrm : 0.0;
    area[F] = size;
#pragma unroll
    for (int k = 0; k < DIM; ++k) normal[(i64)k * nF + F] = size > 0.0 ? sc * nv[k] : 0.0;
  }
}

// one group of LB lanes per band node; lane -> sample b < Bp
template <int DIM>
__global__ __launch_bounds__(256) void elastf_assemble_kernel(
    const int* __restrict__ fac, int nF, const double* __restrict__ area, const double* __restrict__ normal,
    const int* __restrict__ rows, const int* __restrict__ row_ptr, const int* __restrict__ ent_code,
    const int* __restrict__ ent_slot, int n_rows, const unsigned char* __restrict__ is_bc, const double* __restrict__ g,
    const double* __restrict__ t, i64 tsf, i64 tsc, i64 tsb, Datum pr, Datum kn, Datum kt, double* __restrict__ vals,
    double* __restrict__ rhs, int n, int Bv, int B, int Bp) {
  const NodeMap nm = node_map(Bp);
  const int b = nm.b;
  if (b >= Bp) return;
  const bool real = b < B;
  const bool stiff = kn.v || kt.v;
  const bool unit_pad = !real && (kn.sb != 0 || kt.sb != 0);   // padding sample of per-sample stiffness: kn = kt = 1
  const double inv_dd = 1.0 / (double)(DIM * (DIM + 1)), inv_d = 1.0 / (double)DIM;
  const i64 nd = (i64)n * DIM;
  for (int r = nm.node0; r < n_rows; r += nm.stride) {
    const i64 i = rows[r];
    bool rbc[DIM];
    double load[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      rbc[a] = is_bc[i * DIM + a] != 0;
      load[a] = 0.0;
    }
    i64 Fc = -1;                                             // the facet S, nv and ar belong to
    double S[DIM][DIM], nv[DIM], ar = 0.0;
    for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
      const int code = ent_code[e], k = ent_slot[e];
      const i64 F = code >> 4;
      const int p = (code >> 2) & 3, c = code & 3;
      if (F != Fc) {                                         // entries come in facet order: once per (facet, sample)
        Fc = F;
        ar = area[F];
#pragma unroll
        for (int a = 0; a < DIM; ++a) nv[a] = normal[(i64)a * nF + F];
        if (stiff) {
          const double knv = unit_pad ? 1.0 : (kn.v ? kn.at(F, b) : 0.0);
          const double ktv = unit_pad ? 1.0 : (kt.v ? kt.at(F, b) : 0.0);
#pragma unroll
          for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int q = 0; q < DIM; ++q) S[a][q] = (knv - ktv) * (nv[a] * nv[q]) + (a == q ? ktv : 0.0);
        }
      }
      if (stiff) {
        const double mv = ar * (p == c ? 2.0 : 1.0) * inv_dd;
        const i64 j = fac[(i64)c * nF + F];
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
          if (rbc[a]) continue;
          const i64 row = i * DIM + a;
#pragma unroll
          for (int q = 0; q < DIM; ++q) {
            const i64 col = j * DIM + q;
            const double v = mv * S[a][q];
            if (is_bc[col]) {                                // a fixed column: lifted with its value (padding: rhs stays 0)
              if (real) load[a] -= v * g[col];
            } else if (b < Bv) {
              const int slot = k == 0 ? (q - a + DIM) % DIM : k * DIM + q;
              vals[((i64)slot * nd + row) * Bv + b] += v;
            }
          }
        }
      }
      if (p == c && real) {                                  // once per (facet, row): the facet load
        const double pv = pr.v ? pr.at(F, b) : 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
          const double tv = t ? t[F * tsf + (i64)a * tsc + (i64)b * tsb] : 0.0;
          load[a] += (tv - pv * nv[a]) * (ar * inv_d);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a)
      if (!rbc[a]) rhs[(i * DIM + a) * Bp + b] += load[a];
  }
}

// one group of LB lanes per facet (group_map of launch.h), each lane loops over its samples b = sub, sub + LB, ...; an
// output with a zero sample stride is the sum over the batch: group_sum, lane 0 writes
template <int DIM>
__global__ __launch_bounds__(256) void elastf_grad_kernel(
    const int* __restrict__ fac, int nF, const double* __restrict__ area, const double* __restrict__ normal,
    const double* __restrict__ lam, const double* __restrict__ x, const double* __restrict__ g, int B, int Bp,
    double* __restrict__ dt, i64 dtf, i64 dtc, i64 dtb, Grad dp, Grad dkn, Grad dkt, int LB) {
  const GroupMap gm = group_map(LB);
  const double inv_dd = 1.0 / (double)(DIM * (DIM + 1)), inv_d = 1.0 / (double)DIM;
  for (i64 F = gm.item0; F < nF; F += gm.stride) {
    i64 v[DIM];
    double gv[DIM][DIM], nv[DIM];
#pragma unroll
    for (int p = 0; p < DIM; ++p) {
      v[p] = fac[(i64)p * nF + F];
      nv[p] = normal[(i64)p * nF + F];
#pragma unroll
      for (int a = 0; a < DIM; ++a) gv[p][a] = g ? g[v[p] * DIM + a] : 0.0;
    }
    const double ar = area[F];
    double tt[DIM], tp = 0.0, tn = 0.0, tk = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) tt[a] = 0.0;
    for (int b = gm.sub; b < B; b += LB) {
      double sl[DIM], su[DIM], lu = 0.0, sln = 0.0, sun = 0.0, lnun = 0.0;
#pragma unroll
      for (int a = 0; a < DIM; ++a) sl[a] = su[a] = 0.0;
#pragma unroll
      for (int p = 0; p < DIM; ++p) {
        double ln = 0.0, un = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
          const i64 o = (v[p] * DIM + a) * Bp + b;
          const double le = lam[o], ue = x[o] + gv[p][a];
          sl[a] += le;
          su[a] += ue;
          lu += le * ue;
          ln += le * nv[a];
          un += ue * nv[a];
        }
        sln += ln;
        sun += un;
        lnun += ln * un;
      }
      double slsu = 0.0, sn = 0.0;
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        slsu += sl[a] * su[a];
        sn += sl[a] * nv[a];
      }
      // lambda^T (M_F (x) I) u and lambda^T (M_F (x) n n^T) u, M_F = |F| (1 1^T + I) / (d (d + 1))
      const double full = (slsu + lu) * (ar * inv_dd), nn = (sln * sun + lnun) * (ar * inv_dd);
      const double vp = -sn * (ar * inv_d), vn = -nn, vk = nn - full;
      if (dt) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
          const double s = sl[a] * (ar * inv_d);
          if (dtb) dt[F * dtf + (i64)a * dtc + (i64)b * dtb] = s; else tt[a] += s;
        }
      }
      if (dp.v) { if (dp.sb) dp.at(F, b) = vp; else tp += vp; }
      if (dkn.v) { if (dkn.sb) dkn.at(F, b) = vn; else tn += vn; }
      if (dkt.v) { if (dkt.sb) dkt.at(F, b) = vk; else tk += vk; }
    }
    group_sum(LB, tt, tp, tn, tk);
    if (gm.sub == 0) {
      if (dt && !dtb) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) dt[F * dtf + (i64)a * dtc] = tt[a];
      }
      if (dp.v && !dp.sb) dp.at(F, 0) = tp;
      if (dkn.v && !dkn.sb) dkn.at(F, 0) = tn;
      if (dkt.v && !dkt.sb) dkt.at(F, 0) = tk;
    }
  }
}

bool bad_facets(const int* fac, int d, int nF, const double* area, const double* normal) {
  return !fac || !area || !normal || (d != 2 && d != 3) || nF < 1 || nF >= (1 << 27);
}

}  // namespace

extern "C" int diffhe_elastf_facet_table(const double* coords, const int* fac, const int* opp, int dim, int n, int nF,
                                         double* area, double* normal, void* stream) {
  if (bad_facets(fac, dim, nF, area, normal) || !coords || !opp || n < 1) return DIFFHE_E_BADARG;
  int gx = (nF + 255) / 256;
  if (gx > 1024) gx = 1024;
  dispatch_dim<2, 3>(dim, [&](auto D) {
    hipLaunchKernelGGL(elastf_table_kernel<D()>, dim3(gx), dim3(256), 0, (hipStream_t)stream, coords, fac, opp, n, nF,
                       area, normal);
  });
  return check_launch();
}

extern "C" int diffhe_elastf_assemble(const int* fac, int d, int nF, const double* area, const double* normal,
                                      const int* rows, const int* row_ptr, const int* ent_code, const int* ent_slot,
                                      int n_rows, const unsigned char* is_bc, const double* g, const double* t,
                                      long long t_sf, long long t_sc, long long t_sb, const double* p, long long p_sf,
                                      long long p_sb, const double* kn, long long kn_sf, long long kn_sb,
                                      const double* kt, long long kt_sf, long long kt_sb, double* vals, double* rhs, int n,
                                      int Bv, int B, int Bp, void* stream) {
  const bool stiff = kn || kt;
  if (bad_facets(fac, d, nF, area, normal) || !is_bc || !g || !rhs || (stiff && !vals) || n < 1 || n_rows < 0 || B < 1 ||
      Bp < B || (Bv != 1 && Bv != Bp) || t_sf < 0 || t_sc < 0 || t_sb < 0 || p_sf < 0 || p_sb < 0 || kn_sf < 0 ||
      kn_sb < 0 || kt_sf < 0 || kt_sb < 0 || (Bv == 1 && Bp > 1 && ((kn && kn_sb != 0) || (kt && kt_sb != 0))) ||
      (n_rows > 0 && (!rows || !row_ptr || !ent_code || !ent_slot)))
    return DIFFHE_E_BADARG;
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  if (n_rows == 0 || (!stiff && !t && !p)) return DIFFHE_OK;
  // per band node: its d rows of the right-hand side (read + write) and, with a foundation, d x d entries per facet node
  account(8.0 * n_rows * (2.0 * d * Bp + (stiff ? 2.0 * d * d * d * Bv : 0.0)));
  const Datum pd{p, p_sf, p_sb}, nd{kn, kn ? kn_sf : 0, kn ? kn_sb : 0}, td{kt, kt ? kt_sf : 0, kt ? kt_sb : 0};
  dispatch_dim<2, 3>(d, [&](auto D) {
    hipLaunchKernelGGL(elastf_assemble_kernel<D()>, node_grid(n_rows, Bp), dim3(256), 0, (hipStream_t)stream, fac, nF,
                       area, normal, rows, row_ptr, ent_code, ent_slot, n_rows, is_bc, g, t, t_sf, t_sc, t_sb, pd, nd, td,
                       vals, rhs, n, Bv, B, Bp);
  });
  return check_launch();
}

extern "C" int diffhe_elastf_grad(const int* fac, int d, int nF, const double* area, const double* normal,
                                  const double* lam, const double* x, const double* g, int B, int Bp, double* dt,
                                  long long dt_of, long long dt_oc, long long dt_ob, double* dp, long long dp_of,
                                  long long dp_ob, double* dkn, long long dkn_of, long long dkn_ob, double* dkt,
                                  long long dkt_of, long long dkt_ob, void* stream) {
  if (bad_facets(fac, d, nF, area, normal) || !lam || !x || B < 1 || Bp < B || dt_of < 0 || dt_oc < 0 || dt_ob < 0 ||
      dp_of < 0 || dp_ob < 0 || dkn_of < 0 || dkn_ob < 0 || dkt_of < 0 || dkt_ob < 0)
    return DIFFHE_E_BADARG;
  if (!dt && !dp && !dkn && !dkt) return DIFFHE_OK;
  const int LB = group_lanes(B);
  account(8.0 * nF * (2.0 * d * d * B + (double)(d + 3) * B));
  dispatch_dim<2, 3>(d, [&](auto D) {
    hipLaunchKernelGGL(elastf_grad_kernel<D()>, dim3(group_grid(nF, LB, 8192)), dim3(256), 0, (hipStream_t)stream, fac, nF,
                       area, normal, lam, x, g, B, Bp, dt, dt_of, dt_oc, dt_ob, Grad{dp, dp_of, dp_ob},
                       Grad{dkn, dkn_of, dkn_ob}, Grad{dkt, dkt_of, dkt_ob}, LB);
  });
  return check_launch();
}
