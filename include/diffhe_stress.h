/* Stress recovery of linear-elastic solves on P1 triangles and tetrahedra: the third public header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes) and diffhe_elastic.h: every array is a device pointer, vectors are batch innermost, `stream` is a
 * hipStream_t, the return value is DIFFHE_OK or a DIFFHE_E_* status.  diffhe_hip.h, diffhe_elastic.h and
 * DIFFHE_ABI_VERSION are unchanged by them; the Python binding keeps them in a table of their own (diffhe/_hip.py,
 * STRESS_SIGNATURES).
 *
 * Definitions.  u (n*d, Bp) is the FULL displacement, prescribed values included, dof(i, a) = i*d + a; gtab (npe*d, m)
 * holds g_p = grad phi_p in the layout of diffhe_aniso_gradient_table.  That entry leaves the gradients of a negatively
 * oriented element negated (the sign cancels in the products it is made for); the stress is linear in them, so the
 * caller restores it here.  Per element e and sample b
 *
 *   H[a][t] = sum_p u[(p, a)] g_p[t],   eps = (H + H^T) / 2,
 *   s       = 2 mu1 eps + lam1 tr(eps) I          the unit stress (lam1, mu1: the Lame numbers of E = 1),
 *   sigma   = E s,                                 E per element and sample at e*e_se + b*e_sb,
 *   vm^2    = 1/2 [(s_xx - s_yy)^2 + (s_yy - s_zz)^2 + (s_zz - s_xx)^2] + 3 (s_xy^2 + s_yz^2 + s_xz^2)   of sigma.
 *
 * Voigt order: nc = 3, (xx, yy, xy) for dim = 2; nc = 6, (xx, yy, zz, yz, xz, xy) for dim = 3.  A shear component is the
 * tensor component itself (not doubled); its cotangent is the derivative with respect to that one number.  For dim = 2
 * the out-of-plane stress is sigma_zz = nu_z (sigma_xx + sigma_yy): nu_z = nu in plane strain, 0 in plane stress (it is
 * ignored for dim = 3).  sigma_zz enters vm and is never stored.  d vm / d sigma = (3/2) dev(sigma) / vm, and 0 where
 * vm == 0: no NaN or Inf leaves these kernels for finite inputs.
 *
 * A stress array or its cotangent holds component c of element e and sample b at c*osc + e*ose + b: (nc, m, Bp) is
 * osc = m*Bp, ose = Bp; (m, nc, Bp) is osc = Bp, ose = nc*Bp.  vm and its cotangent are (m, Bp).
 * fp64, no floating-point atomics: every sum has a fixed order, results are bitwise reproducible. */
#ifndef DIFFHE_STRESS_H
#define DIFFHE_STRESS_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sigma and / or vm of every element and sample.  A NULL output is neither computed nor stored (at least one is given);
 * with sigma NULL, osc and ose are ignored and no stress array is touched. */
int diffhe_stress_eval(const int* elems, const double* gtab, int dim, double lam1, double mu1, double nu_z,
                       const double* u, const double* E, long long e_se, long long e_sb, int n, int m, int Bp,
                       double* sigma, long long osc, long long ose, double* vm, void* stream);

/* Adjoint of diffhe_stress_eval for the cotangents sigma_bar (addressed as sigma, may be NULL) and vm_bar (m, Bp) (may be
 * NULL, not both).  Element pass: sigma and vm are recomputed, c = sigma_bar + vm_bar d vm / d sigma (sigma_zz chained
 * through nu_z), dE[e, b] = sum_k c_k s_k, and the symmetric tensor T = E (2 mu1 sym(C) + lam1 tr(C) I), C the tensor of
 * c with each shear cotangent split evenly over its two entries, goes to work (nc, m, Bp).  Node pass over the incidence
 * list inc_ptr (n+1), inc (codes e*npe + p, diffhe_p1_shape_grad's): u_bar[(i, a), b] = sum_{(e, p) at i} sum_t
 * T_e[a][t] g_p[t], in list order.
 * u_bar (n*d, Bp), work, inc_ptr, inc: all four or none (none: no node pass).  de_e (m, Bp), de_part
 * (diffhe_grad_kappa_blocks(m, Bp), Bp) and de_sum (Bp) are those of diffhe_elast_grad (de_part and de_sum both or
 * neither); all three may be NULL when u_bar is given.  Padding samples b >= B get u_bar = 0 and dE = 0 and their
 * cotangents are not read. */
int diffhe_stress_adjoint(const int* elems, const double* gtab, int dim, double lam1, double mu1, double nu_z,
                          const double* u, const double* E, long long e_se, long long e_sb, const double* sigma_bar,
                          long long osc, long long ose, const double* vm_bar, const int* inc_ptr, const int* inc, int n,
                          int m, int B, int Bp, double* work, double* u_bar, double* de_e, double* de_part,
                          double* de_sum, void* stream);

/* dE of the element pass summed over the samples b < B in a fixed order, de (m): the gradient of a field the batch
 * shares.  The (m, Bp) array is never formed. */
int diffhe_stress_adjoint_shared(const int* elems, const double* gtab, int dim, double lam1, double mu1, double nu_z,
                                 const double* u, const double* E, long long e_se, long long e_sb,
                                 const double* sigma_bar, long long osc, long long ose, const double* vm_bar, int n,
                                 int m, int B, int Bp, double* de, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_STRESS_H */
