/* Node-coordinate (shape) gradients of linear-elastic solves and stress evaluations on P1 triangles and tetrahedra: the
 * sixth public header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes), diffhe_elastic.h and diffhe_stress.h: every array is a device pointer, vectors are (n*d, Bp) with
 * dof(i, a) = i*d + a and the batch innermost, `stream` is a hipStream_t, the return value is DIFFHE_OK or a DIFFHE_E_*
 * status.  The other five headers and DIFFHE_ABI_VERSION are unchanged by them; the Python binding keeps them in a table
 * of their own (diffhe/_hip.py, ELASTIC_SHAPE_SIGNATURES).
 *
 * Definitions.  gtab (npe*d, m) holds g_p = grad phi_p in the layout of diffhe_aniso_gradient_table WITH the sign of
 * every element's orientation restored, as diffhe_stress.h takes it: the expressions below are odd in g.  vol (m) is the
 * element size A_e.  Per element e and sample b, for a dof vector w,
 *
 *   H_w[a][t] = sum_p w[(p, a)] g_p[t],        S(H) = 2 mu1 sym(H) + lam1 tr(H) I      (lam1, mu1: the Lame numbers of E = 1).
 *
 * Both entries run two passes without floating-point atomics, so that results are bitwise reproducible.  The element
 * pass gives one group of LB = min(next power of two >= B, 64) lanes to an element; the lanes run over the samples
 * b < B (padding samples b >= B are skipped) and meet in a fixed-order butterfly, and the (d+1) d vertex contributions of
 * the element go to work (m, (d+1) d).  The node pass sums them over the incidence list inc_ptr (n+1), inc (codes
 * e*npe + p, diffhe_p1_shape_grad's) in list order into grad (n, d): dL/dX summed over the batch.  An element whose row
 * of gtab is zero (a degenerate one) contributes nothing. */
#ifndef DIFFHE_ELASTIC_SHAPE_H
#define DIFFHE_ELASTIC_SHAPE_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dL/dX of a solve K(X, E) u = M(X) f + load from its adjoint lam (zero on fixed dofs).  u is the solve's iterate and g
 * (n*d, may be NULL) the prescribed values, so that u + g is the full displacement; f (n*d, Bp) is the body-force density
 * in the dof layout, NULL for none; E per element and sample at e*e_se + b*e_sb.  Element e adds to its vertex p
 *
 *   A_e [ sum_b E_eb ( H_u^T S(H_lam) + H_lam^T S(H_u) - (S(H_u) : H_lam) I ) + q_e I ] g_p,
 *   q_e = sum_b sum_a (sum_p lam[(p, a)]) (sum_p f[(p, a)]) / (d+1)^2. */
int diffhe_elast_shape_grad(const int* elems, const double* gtab, const double* vol, int dim, double lam1, double mu1,
                            const double* u, const double* g, const double* lam, const double* f, const double* E,
                            long long e_se, long long e_sb, int n, int m, int B, int Bp, const int* inc_ptr,
                            const int* inc, double* work, double* grad, void* stream);

/* dL/dX of diffhe_stress_eval at fixed u for the cotangents sigma_bar and vm_bar, which are addressed as in
 * diffhe_stress_adjoint (either may be NULL, not both).  With T = dL/dH_u, the symmetric tensor of that entry's element
 * pass, element e adds to its vertex p
 *
 *   - ( sum_b H_u^T T_b ) g_p.
 *
 * The stress has no size factor, so vol is not read.  T is 0 where vm == 0: no NaN or Inf leaves the kernel for finite
 * inputs. */
int diffhe_stress_shape_grad(const int* elems, const double* gtab, int dim, double lam1, double mu1, double nu_z,
                             const double* u, const double* E, long long e_se, long long e_sb, const double* sigma_bar,
                             long long osc, long long ose, const double* vm_bar, int n, int m, int B, int Bp,
                             const int* inc_ptr, const int* inc, double* work, double* grad, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_ELASTIC_SHAPE_H */
