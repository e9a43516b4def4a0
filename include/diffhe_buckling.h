/* Linear buckling of elastic bodies, (K(E) + lambda K_G(sigma0)) phi = 0 per sample, on P1 triangles and tetrahedra: the
 * fourteenth public header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes): every array is a device pointer, vectors are batch innermost, `stream` is a hipStream_t, the return
 * value is DIFFHE_OK or a DIFFHE_E_* status.  The thirteen other headers and DIFFHE_ABI_VERSION are unchanged by them; the
 * Python binding keeps them in a table of their own (diffhe/_hip.py, BUCKLING_SIGNATURES).
 *
 * Definitions.  d = dim unknowns per node, row (i, a) = i*d + a.  For P1 elements the geometric stiffness is
 * K_G = G (x) I_d with the scalar operator G[a, b] = sum_e vol_e grad N_a . sigma0_e grad N_b on the NODE pattern
 * (cols (W, n), values (W, n, Bv), Bv = Bp or 1 for a prestress the batch shares): the stiffness of a conductivity tensor
 * with the stress in its place, so diffhe_aniso_assemble_rows (diffhe_hip.h) assembles it -- called without Dirichlet data
 * (is_bc = g = lift = NULL); its arithmetic asks nothing of the tensor's sign.  sigma0 is in the Voigt order of that entry,
 * shear components are tensor components.  The pencil of the iteration is N phi = mu K phi with N = -K_G, mu = 1 / lambda.
 *
 * Blocks of p <= 16 vectors are (p, n*d, Bp) as in diffhe_eig_*; the packed Gram matrices and the block partials have the
 * layout of diffhe_eig_gram (`part`: diffhe_eig_gram_blocks(rows, Bp) * 2 * nq * Bp doubles, nq = p (p + 1) / 2), so they
 * feed diffhe_eig_ritz.  fp64, no atomics, two-stage reductions in a fixed order: results are bitwise reproducible. */
#ifndef DIFFHE_BUCKLING_H
#define DIFFHE_BUCKLING_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y = scale (G (x) I_d) x for one column: y[(i, a), b] = scale sum_k G[k, i, b] x[(cols[k, i], a), b]; every entry of G is
 * read once and applied to the d components of its column node.  x, y (n*d, Bp); n counts NODES.  Rows with
 * is_bc[row] != 0 (a mask per dof, may be NULL) give 0; x must be 0 there.  scale = -1 applies N. */
int diffhe_buckling_apply(const double* G, const int* cols, const unsigned char* is_bc, const double* x, double* y,
                          double scale, int n, int W, int d, int Bp, int Bv, void* stream);

/* y = coef[b] x + dx and dot[b] = sum over the rows of dx[row, b] r[row, b]: the next block column (A + s) x and the
 * squared K-norm of the column's residual from the correction dx = K^-1 r, in one pass.  rows = n*d; part:
 * diffhe_grad_kappa_blocks(rows, Bp) * Bp doubles; coef, dot (Bp). */
int diffhe_buckling_step(const double* x, const double* dx, const double* r, const double* coef, int rows, int Bp,
                         double* y, double* part, double* dot, void* stream);

/* GK[q(i, j)] = y_i . (K y)_j and GN[q(i, j)] = y_i . (N y)_j, i <= j, over the rows with is_bc[row] == 0 (may be NULL). */
int diffhe_buckling_gram(const double* Y, const double* KY, const double* NY, const unsigned char* is_bc, int p, int rows,
                         int Bp, double* part, double* GK, double* GN, void* stream);

/* X = Y C, KX = KY C, NX = NY C and R = NX - mu KX (mu (p, Bp)) in one pass; C (p, p, Bp) as diffhe_eig_ritz leaves it. */
int diffhe_buckling_rotate(const double* Y, const double* KY, const double* NY, const double* C, const double* mu, int p,
                           int rows, int Bp, double* X, double* KX, double* NX, double* R, void* stream);

/* The cotangent of the prestress for K-normalised columns X (k, n*d, Bp) and weights w (k, Bp)
 * (w[i, b] = lambda_bar[b, i] lambda[b, i]^2):
 *   ds_c[e, b] = vol_e sum_i w[i, b] sum_a sym_c(grad phi_{i,a} (x) grad phi_{i,a}),  grad phi_{i,a} = sum_p X[i, (el_p, a), b] g_p,
 * in Voigt tensor components: an off-diagonal component carries the factor 2 of its two symmetric entries; 0 for b >= B.
 * ds_e optional: component c of (e, b) at c*o_sc + e*o_se + b.  ds_part (diffhe_grad_kappa_blocks(m, Bp), nc, Bp) and
 * ds_sum (nc, Bp), both or neither: the sums over the elements per sample.  gtab, vol: diffhe_aniso_gradient_table's. */
int diffhe_buckling_grad_sigma(const int* elems, const double* gtab, const double* vol, int dim, const double* X,
                               const double* w, int k, int n, int m, int B, int Bp, double* ds_e, long long o_sc,
                               long long o_se, double* ds_part, double* ds_sum, void* stream);

/* The same cotangent summed over the samples b < B in a fixed order, component c of element e at c*o_sc + e*o_se: the
 * gradient of a prestress the batch shares. */
int diffhe_buckling_grad_sigma_shared(const int* elems, const double* gtab, const double* vol, int dim, const double* X,
                                      const double* w, int k, int n, int m, int B, int Bp, double* ds, long long o_sc,
                                      long long o_se, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_BUCKLING_H */
