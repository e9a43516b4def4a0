/* Linear elasticity on P1 triangles and tetrahedra: the second public header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes): every array is a device pointer, vectors are batch innermost, `stream` is a hipStream_t, the
 * return value is DIFFHE_OK or a DIFFHE_E_* status.  diffhe_hip.h and DIFFHE_ABI_VERSION are unchanged by them; the
 * Python binding keeps them in a table of their own (diffhe/_hip.py, ELASTIC_SIGNATURES).
 *
 * Unknowns.  d = dim displacement components per node, dof(i, a) = i*d + a.  A dof vector is (n*d, Bp): the contiguous
 * node-major (n, d, Bp).  gtab (npe*d, m) and vol (m) are the gradient table of diffhe_aniso_gradient_table.
 *
 * Material.  sigma = 2 mu eps(u) + lambda tr eps(u) I with mu = E mu1, lambda = E lam1: lam1, mu1 are the Lame numbers
 * of E = 1 (they carry Poisson's ratio and the plane-stress / plane-strain choice), E is per element and sample at
 * e*e_se + b*e_sb.  The element block of the node pair (p, q) is
 *
 *   K_e[(p,a),(q,b)] = vol_e E_e [ lam1 g_pa g_qb + mu1 g_pb g_qa + mu1 delta_ab g_p.g_q ],   g_p = grad phi_p.
 *
 * Pattern.  The operator is stored as ELL rows of width d*W over n*d rows, derived from the node pattern cols (W, n)
 * (slot 0 = the node itself, unused slots point at the node itself; it must hold every coupling of the connectivity).
 * Row (i, a), dof slot s:
 *   s <  d            column (i, (a + s) mod d)            -- the node's own block, rotated so that slot 0 is the diagonal
 *   s >= d, s = k*d+b column (cols[k, i], b)               -- node slot k >= 1, component b
 *   an unused node slot k >= 1 gives d unused dof slots: they point at the row itself and hold 0.
 * This is what diffhe_ell_cg_solve, diffhe_ell_amg_pcg_solve and diffhe_ell_galerkin assume of a pattern. */
#ifndef DIFFHE_ELASTIC_H
#define DIFFHE_ELASTIC_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Block row-gather assembly over the NODE-level lists ent_ptr / contrib / cols of diffhe_ell_assemble_rows:
 * vals (d*W, n*d, Bv) in the pattern above and lift (n*d, Bv) = sum over fixed columns of K[row, col] g[col].
 * Dirichlet handling per dof as diffhe_ell_assemble_rows: a fixed row is an identity row, couplings of a free row to
 * fixed columns are zeroed and go to the lift.  is_bc, g: (n*d) per dof, both or neither.  Bv = 1 (e_sb = 0): one matrix
 * for the batch.  No atomics: bitwise reproducible. */
int diffhe_elast_assemble_rows(const double* gtab, const double* vol, int dim, double lam1, double mu1, const double* E,
                               long long e_se, long long e_sb, const int* ent_ptr, const int* contrib, const int* cols,
                               const unsigned char* is_bc, const double* g, double* vals, double* lift, int n, int m,
                               int W, int Bv, void* stream);

/* dE[e, b] = -vol_e [ lam1 (div lam_h)(div u_h) + 2 mu1 eps(lam_h) : eps(u_h) ] from the element-constant gradients of
 * the adjoint lam and the displacement u, both (n*d, Bp); g (n*d, may be NULL) is added to u on fixed dofs.
 * de_e (m, Bp) optional; de_part (diffhe_grad_kappa_blocks(m, Bp), Bp) and de_sum (Bp), both or neither: the sums over
 * the elements per sample, two stages in a fixed order. */
int diffhe_elast_grad(const int* elems, const double* gtab, const double* vol, int dim, double lam1, double mu1,
                      const double* lam, const double* u, const double* g, int n, int m, int Bp, double* de_e,
                      double* de_part, double* de_sum, void* stream);

/* The same gradient summed over the samples b < B in a fixed order, de (m): the gradient of a field the batch shares.
 * The (m, Bp) array is never formed. */
int diffhe_elast_grad_shared(const int* elems, const double* gtab, const double* vol, int dim, double lam1, double mu1,
                             const double* lam, const double* u, const double* g, int n, int m, int B, int Bp,
                             double* de, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_ELASTIC_H */
