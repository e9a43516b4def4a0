/* Anisotropic linear elasticity on P1 triangles and tetrahedra: the seventh public header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes) and of diffhe_elastic.h (the unknowns, the dof pattern, the gradient table): every array is a device
 * pointer, vectors are batch innermost, `stream` is a hipStream_t, the return value is DIFFHE_OK or a DIFFHE_E_* status.
 * diffhe_hip.h, the other five headers and DIFFHE_ABI_VERSION are unchanged by them; the Python binding keeps them in a
 * table of their own (diffhe/_hip.py, ELASTIC_ANISO_SIGNATURES).
 *
 * Material.  sigma = C eps(u) with a symmetric positive-definite stiffness matrix C per element and sample, nv x nv with
 * nv = 3 in 2D and 6 in 3D.  Strains are in the Voigt order (xx, yy, xy) / (xx, yy, zz, yz, xz, xy), shear strains are
 * ENGINEERING strains gamma = 2 eps: C is the ordinary engineering stiffness matrix.  C is stored as its upper triangle,
 * row-major: nt = 6 components in 2D (11, 12, 13, 22, 23, 33), nt = 21 in 3D; component c of element e and sample b sits
 * at c*c_sc + e*c_se + b*c_sb.  An off-diagonal component is ONE parameter that fills both symmetric entries.  With
 * V(a, t) the Voigt index of the unordered pair (a, t) and g_p = grad phi_p the element block of the node pair (p, q) is
 *
 *   K_e[(p,a),(q,b)] = vol_e sum_{t,s} g_p[t] C_e[V(a,t)][V(b,s)] g_q[s]          (no factors of 2). */
#ifndef DIFFHE_ELASTIC_ANISO_H
#define DIFFHE_ELASTIC_ANISO_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Block row-gather assembly, diffhe_elast_assemble_rows with the stiffness matrix above in place of (lam1, mu1, E): the
 * same NODE-level lists ent_ptr / contrib / cols, the same dof pattern vals (d*W, n*d, Bv) and lift (n*d, Bv), the same
 * Dirichlet handling per dof (identity rows, zeroed columns, lift; is_bc, g: (n*d), both or neither).  Bv = 1
 * (c_sb = 0): one matrix for the batch, lanes over nodes; otherwise lanes over samples.  No atomics: bitwise reproducible. */
int diffhe_elastc_assemble_rows(const double* gtab, const double* vol, int dim, const double* C, long long c_sc,
                                long long c_se, long long c_sb, const int* ent_ptr, const int* contrib, const int* cols,
                                const unsigned char* is_bc, const double* g, double* vals, double* lift, int n, int m,
                                int W, int Bv, void* stream);

/* dC_IJ[e, b] = -vol_e (eps_I(lam) eps_J(u) + [I != J] eps_J(lam) eps_I(u)), I <= J, from the element-constant engineering
 * Voigt strains of the adjoint lam and the displacement u, both (n*d, Bp); g (n*d, may be NULL) is added to u on fixed
 * dofs.  dc_e optional: component c of element e and sample b at c*o_sc + e*o_se + b.  dc_part
 * (diffhe_grad_kappa_blocks(m, Bp), nt, Bp) and dc_sum (nt, Bp), both or neither: the sums over the elements per sample,
 * two stages in a fixed order. */
int diffhe_elastc_grad(const int* elems, const double* gtab, const double* vol, int dim, const double* lam,
                       const double* u, const double* g, int n, int m, int Bp, double* dc_e, long long o_sc,
                       long long o_se, double* dc_part, double* dc_sum, void* stream);

/* The same gradient summed over the samples b < B in a fixed order, component c of element e at c*o_sc + e*o_se: the
 * gradient of a field the batch shares.  The (nt, m, Bp) array is never formed. */
int diffhe_elastc_grad_shared(const int* elems, const double* gtab, const double* vol, int dim, const double* lam,
                              const double* u, const double* g, int n, int m, int B, int Bp, double* dc, long long o_sc,
                              long long o_se, void* stream);

/* out[0] = max over the rows i < n and the stored matrices b < Bv of
 *   sum_k |v[k, i, b]| / sqrt(v[0, i, b] * v[0, cols[k, i], b])
 * for ELL values vals (W, n, Bv) in the pattern cols (W, n) (slot 0 = the diagonal, padding slots hold 0): the
 * infinity norm of the symmetric matrix D^-1/2 A D^-1/2, hence an upper bound of lambda_max(D^-1 A).  An identity row
 * gives 1; a diagonal that is not positive and finite gives +inf.  part: DIFFHE_ROW_BOUND_BLOCKS doubles of scratch (the
 * block maxima: two stages, fixed order). */
#define DIFFHE_ROW_BOUND_BLOCKS 1024
int diffhe_ell_jacobi_row_bound(const double* vals, const int* cols, int n, int W, int Bv, double* part, double* out,
                                void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_ELASTIC_ANISO_H */
