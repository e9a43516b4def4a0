/* Finite-strain compressible Neo-Hookean elasticity on P1 triangles (plane strain) and tetrahedra: the eleventh public
 * header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes) and of diffhe_elastic.h (the unknowns, the dof pattern, the gradient table): every array is a device
 * pointer, vectors are batch innermost, `stream` is a hipStream_t, the return value is DIFFHE_OK or a DIFFHE_E_* status.
 * diffhe_hip.h, the other ten headers and DIFFHE_ABI_VERSION are unchanged by them; the Python binding keeps them in a
 * table of their own (diffhe/_hip.py, HYPERELASTIC_SIGNATURES).
 *
 * Kinematics and material.  u (n*d, Bp) is the FULL displacement, prescribed values included.  Per element and sample
 *
 *   F = I + sum_p u_p (x) g_p,   J = det F,   g_p = grad phi_p,   h_p = F^-T g_p
 *   W(F)  = E [ mu1/2 (tr F^T F - d) - mu1 ln J + lam1/2 (ln J)^2 ]
 *   P1(F) = mu1 (F - F^-T) + lam1 ln J F^-T                                   (first Piola-Kirchhoff stress of E = 1)
 *
 * gtab (npe*d, m) holds g_p WITH its sign (F is linear in it): the table of diffhe_aniso_gradient_table, which is defined up
 * to the sign of the element's orientation, with that sign restored.  vol (m) is that table's.
 * lam1, mu1 are the 3D Lame numbers of E = 1 (plane strain in 2D); E is per element and sample at e*e_se + b*e_sb.
 * The operator is per sample, because u is: every entry takes the padded batch Bp and runs lanes over samples.
 * fp64, no atomics: every sum has a fixed order, results are bitwise reproducible. */
#ifndef DIFFHE_HYPERELASTIC_H
#define DIFFHE_HYPERELASTIC_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tangent K_T(u, E) by the block row-gather assembly of diffhe_elast_assemble_rows: the same NODE-level lists
 * ent_ptr / contrib / cols and the same dof pattern vals (d*W, n*d, Bp), with the element block
 *
 *   K_e[(p,i),(q,k)] = vol_e E_e [ mu1 delta_ik g_p.g_q + (mu1 - lam1 ln J) h_q,i h_p,k + lam1 h_p,i h_q,k ]
 *
 * evaluated from u; elems (npe, m) names the element's nodes.  Fixed rows (is_bc (n*d), may be NULL) are identity rows,
 * columns of fixed dofs are zeroed and there is NO lift: a Newton increment vanishes there.  An element with J <= 0
 * writes NaN into the rows it touches. */
int diffhe_hyper_assemble_rows(const int* elems, const double* gtab, const double* vol, int dim, double lam1, double mu1,
                               const double* E, long long e_se, long long e_sb, const double* u, const int* ent_ptr,
                               const int* contrib, const int* cols, const unsigned char* is_bc, double* vals, int n,
                               int m, int W, int Bp, void* stream);

/* The internal force R[(i, a), b] = sum over the incidence list of node i (inc_ptr (n+1), inc: codes e*npe + p, element
 * order) of vol_e E_e [P1(F_e) g_p]_a, R (n*d, Bp): a node pass, every row is written. */
int diffhe_hyper_residual(const int* inc_ptr, const int* inc, const int* elems, const double* gtab, const double* vol,
                          int dim, double lam1, double mu1, const double* E, long long e_se, long long e_sb,
                          const double* u, int n, int m, int Bp, double* R, void* stream);

/* energy[b] = sum_e vol_e W(F_e) and min_j[b] = min_e J_e per sample, both (Bp), in two stages of a fixed order through
 * w_part and j_part, each (diffhe_grad_kappa_blocks(m, Bp), Bp).  A sample with any J <= 0 gets energy = +inf (its
 * inverted elements add nothing to the sum); the other samples are unaffected. */
int diffhe_hyper_energy(const int* elems, const double* gtab, const double* vol, int dim, double lam1, double mu1,
                        const double* E, long long e_se, long long e_sb, const double* u, int n, int m, int Bp,
                        double* w_part, double* j_part, double* energy, double* min_j, void* stream);

/* dE[e, b] = -vol_e P1(F_e(u)) : grad lam_e from the adjoint lam and the displacement u, both (n*d, Bp).  de_e (m, Bp)
 * optional; de_part (diffhe_grad_kappa_blocks(m, Bp), Bp) and de_sum (Bp), both or neither: the sums over the elements
 * per sample, two stages in a fixed order. */
int diffhe_hyper_grad(const int* elems, const double* gtab, const double* vol, int dim, double lam1, double mu1,
                      const double* lam, const double* u, int n, int m, int Bp, double* de_e, double* de_part,
                      double* de_sum, void* stream);

/* The same gradient summed over the samples b < B in a fixed order, de (m): the gradient of a field the batch shares.
 * The (m, Bp) array is never formed. */
int diffhe_hyper_grad_shared(const int* elems, const double* gtab, const double* vol, int dim, double lam1, double mu1,
                             const double* lam, const double* u, int n, int m, int B, int Bp, double* de, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_HYPERELASTIC_H */
