/* Tractions, pressure and elastic foundations on boundary facets of elastic bodies: the eighth public header of
 * libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes) and of diffhe_elastic.h (the unknowns dof(i, a) = i*d + a, the dof pattern and its slots): every array
 * is a device pointer, vectors are batch innermost, `stream` is a hipStream_t, the return value is DIFFHE_OK or a
 * DIFFHE_E_* status.  diffhe_hip.h, the other six headers and DIFFHE_ABI_VERSION are unchanged by them; the Python binding
 * keeps them in a table of their own (diffhe/_hip.py, ELASTIC_FACET_SIGNATURES).
 *
 * On boundary facets F with d = dim nodes (edges of triangles, faces of tetrahedra), outward unit normal n_F and size |F|
 *
 *   sigma(u) n = t_F - p_F n_F - S_F u,     S_F = kn_F n_F n_F^T + kt_F (I - n_F n_F^T),
 *
 * discretised with the consistent P1 facet mass M_F[p, q] = |F| (1 + delta_pq) / (d (d + 1)) of diffhe_robin_assemble:
 *
 *   A[(p,a),(q,b)] += sum_F M_F[p,q] S_F[a,b],        F[(p,a)] += sum_F (|F| / d) (t_F[a] - p_F n_F[a]).
 *
 * Facet data.  t, p, kn, kt are read in place: a scalar datum of facet F and sample b at F*sf + b*sb, component a of the
 * traction at F*sf + a*sc + b*sb; a zero stride shares the value, a NULL pointer is a datum of zeros.
 * Facet lists (diffhe/plan.py, SolvePlan.elastic_facet_table): fac (d, nF) the facet nodes, area (nF), normal (d, nF);
 * rows (n_rows) the nodes on a facet and, per row, row_ptr / ent_code / ent_slot: its entries (facet F, local row p,
 * local column c) in facet order, ent_code = F*16 + p*4 + c, ent_slot = the NODE slot k of the coupling (row, node c of
 * F) in the node pattern cols (W, n) the dof pattern derives from.  Fixed dofs are handled per dof inside the kernels. */
#ifndef DIFFHE_ELASTIC_FACETS_H
#define DIFFHE_ELASTIC_FACETS_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* area[F] = |F| and normal[a, F] = the unit normal of facet F that points away from the node opp[F] (the node of the
 * owning element opposite the facet), from coords (dim, n).  A degenerate facet (the thresholds of
 * diffhe_robin_facet_table) gets area 0 and normal 0. */
int diffhe_elastf_facet_table(const double* coords, const int* fac, const int* opp, int dim, int n, int nF, double* area,
                              double* normal, void* stream);

/* In place, after diffhe_elast_assemble_rows: vals (d*W, n*d, Bv) += the foundation blocks M_F[p,c] S_F on the free rows,
 * rhs (n*d, Bp) += the facet loads; the coupling of a free row to a fixed column dof goes to rhs with its value g (n*d),
 * a fixed row (is_bc (n*d)) is left untouched.  Bv = 1 or Bp; Bv = 1 with Bp > 1 needs kn_sb = kt_sb = 0.  kn, kt both
 * NULL: vals is not touched and may be NULL.  Samples B <= b < Bp (padding) get zero loads, and kn = kt = 1 where a
 * stiffness comes per sample: a well-posed dummy system with a zero right-hand side.  No atomics: bitwise reproducible. */
int diffhe_elastf_assemble(const int* fac, int d, int nF, const double* area, const double* normal, const int* rows,
                           const int* row_ptr, const int* ent_code, const int* ent_slot, int n_rows,
                           const unsigned char* is_bc, const double* g, const double* t, long long t_sf, long long t_sc,
                           long long t_sb, const double* p, long long p_sf, long long p_sb, const double* kn,
                           long long kn_sf, long long kn_sb, const double* kt, long long kt_sf, long long kt_sb,
                           double* vals, double* rhs, int n, int Bv, int B, int Bp, void* stream);

/* Per facet F and sample b < B, from the adjoint lam (0 on fixed dofs) and the iterate x, both (n*d, Bp); g (n*d, may be
 * NULL) is added to x: u = x + g.  With s = (|F| / d) sum_p lam_p (d components):
 *   dt[a] = s[a],   dp = -s . n_F,   dkn = -sum_{p,q} M_F[p,q] (lam_p . n_F)(u_q . n_F),
 *   dkt = -sum_{p,q} M_F[p,q] [lam_p . u_q - (lam_p . n_F)(u_q . n_F)].
 * Each output is optional (NULL) and written at F*of + b*ob (dt: + a*oc); an output with ob = 0 is the sum over the
 * batch, in a fixed order. */
int diffhe_elastf_grad(const int* fac, int d, int nF, const double* area, const double* normal, const double* lam,
                       const double* x, const double* g, int B, int Bp, double* dt, long long dt_of, long long dt_oc,
                       long long dt_ob, double* dp, long long dp_of, long long dp_ob, double* dkn, long long dkn_of,
                       long long dkn_ob, double* dkt, long long dkt_of, long long dkt_ob, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_ELASTIC_FACETS_H */
