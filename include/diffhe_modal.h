/* Vibration modes of linear-elastic bodies, K(E) phi = lambda M(rho) phi per sample, on P1 triangles and tetrahedra: the
 * fifth public header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes): every array is a device pointer, vectors are batch innermost, `stream` is a hipStream_t, the return
 * value is DIFFHE_OK or a DIFFHE_E_* status.  The four other headers and DIFFHE_ABI_VERSION are unchanged by them; the
 * Python binding keeps them in a table of their own (diffhe/_hip.py, MODAL_SIGNATURES).
 *
 * Definitions.  d = dim unknowns per node, row (i, a) = i*d + a.  The mass is LUMPED and nodal: every component a of node
 * i carries m[i, b] = sum over the (e, p) at i of rho[e, b] vol_e / (d + 1), stored (n_nodes, Bv) with Bv = Bp, or Bv = 1
 * for a density the batch shares.  The block entries read the mass of row r and sample b at (r / d)*ms + b*mb -- (ms, mb)
 * = (Bp, 1) per sample, (1, 0) shared -- with d = 1, 2 or 3 a compile-time constant of their kernels; `n` counts ROWS there
 * and must be a multiple of d.  They are the diffhe_eig_* passes of diffhe_hip.h (same kernels, same block layout
 * (p, n, Bp), same `part` sizes from diffhe_eig_gram_blocks(n, Bp)); diffhe_eig_ritz is mass-free and serves both.
 * fp64, no atomics, two-stage reductions in a fixed order: results are bitwise reproducible. */
#ifndef DIFFHE_MODAL_H
#define DIFFHE_MODAL_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mass (n, Bv): a node pass over the incidence list inc_ptr (n+1), inc (codes e*npe + p, diffhe_p1_shape_grad's), in list
 * order.  rho of element e and sample b at e*r_se + b*r_sb (with Bv = 1 the one sample is b = 0 and r_sb is not used: a
 * per-sample field of a batch of one is taken like a shared one); samples b >= B get rho = 1 and rho is not read for
 * them. */
int diffhe_modal_mass(const int* inc_ptr, const int* inc, const double* vol, int dim, const double* rho, long long r_se,
                      long long r_sb, int n, int m, int B, int Bv, double* mass, void* stream);

/* diffhe_eig_gram with that mass: GA = Y^T (A Y), GM = Y^T M Y over the rows with is_bc[row] == 0 (a mask per ROW). */
int diffhe_modal_gram(const double* Y, const double* AY, const double* mass, long long ms, long long mb, int d,
                      const unsigned char* is_bc, int p, int n, int Bp, double* part, double* GA, double* GM,
                      void* stream);

/* diffhe_eig_rotate with that mass: X = Y C, AX = AY C, MX = M X and R = theta M X - A X (each of the two optional). */
int diffhe_modal_rotate(const double* Y, const double* AY, const double* C, const double* theta, const double* mass,
                        long long ms, long long mb, int d, int p, int n, int Bp, double* X, double* AX, double* MX,
                        double* R, void* stream);

/* diffhe_eig_residual with that mass: rho[c, b] = |R_c|_{M^-1} / |theta_c|. */
int diffhe_modal_residual(const double* R, const double* theta, const double* mass, long long ms, long long mb, int d,
                          int p, int n, int Bp, double* part, double* rho, void* stream);

/* diffhe_eig_fix_sign with that mass: sum_r m_r x_r > 0, else the entry of largest magnitude positive. */
int diffhe_modal_fix_sign(double* X, const double* mass, long long ms, long long mb, int d, int k, int n, int Bp,
                          double* part, double* sgn, void* stream);

/* The Hellmann-Feynman gradient with respect to the density for M-normalised columns X (k, n*d, Bp) and weights
 * w (k, Bp) (w[i, b] = -lambda_bar[b, i] lambda[b, i]):
 *   dr[e, b] = vol_e / (d + 1) sum_i w[i, b] sum_{p in e} sum_a X[i, (el_p, a), b]^2,   0 for b >= B,
 * in one element pass.  dr_e (m, Bp), dr_part (diffhe_grad_kappa_blocks(m, Bp), Bp) and dr_sum (Bp) are those of
 * diffhe_elast_grad: dr_e or dr_part must be given, dr_part and dr_sum both or neither. */
int diffhe_modal_grad_rho(const int* elems, const double* vol, int dim, const double* X, const double* w, int k, int n,
                          int m, int B, int Bp, double* dr_e, double* dr_part, double* dr_sum, void* stream);

/* The same gradient summed over the samples b < B in a fixed order, dr (m): the gradient of a density the batch shares. */
int diffhe_modal_grad_rho_shared(const int* elems, const double* vol, int dim, const double* X, const double* w, int k,
                                 int n, int m, int B, int Bp, double* dr, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_MODAL_H */
