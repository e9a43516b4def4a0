/* Stress recovery of finite-strain Neo-Hookean solves on P1 triangles (plane strain) and tetrahedra: the twelfth public
 * header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes), of diffhe_hyperelastic.h (kinematics, material, the oriented gradient table) and of diffhe_stress.h
 * (Voigt order, storage of a stress array, the von Mises formula): every array is a device pointer, vectors are batch
 * innermost, `stream` is a hipStream_t, the return value is DIFFHE_OK or a DIFFHE_E_* status.  diffhe_hip.h, the other
 * eleven headers and DIFFHE_ABI_VERSION are unchanged by them; the Python binding keeps them in a table of their own
 * (diffhe/_hip.py, HYPER_STRESS_SIGNATURES).
 *
 * Definitions.  u (n*d, Bp) is the FULL displacement, prescribed values included; gtab (npe*d, m) holds g_p = grad phi_p
 * WITH its sign.  Per element e and sample b, with H[a][t] = sum_p u[(p, a)] g_p[t], F = I + H, J = det F:
 *
 *   s        = (1/J) [ mu1 (H + H^T + H H^T) + lam1 ln J I ]     the unit Cauchy stress, = P1(F) F^T / J; b - I = F F^T - I
 *                                                                is formed from H, so nothing cancels at small strains
 *   sigma    = E s                                               symmetric; E per element and sample at e*e_se + b*e_sb
 *   sigma_zz = E lam1 ln J / J                                   dim = 2 (plane strain, F33 = 1): never stored, enters vm
 *   vm                                                           the formula of diffhe_stress.h on sigma with sigma_zz;
 *                                                                d vm / d sigma = (3/2) dev(sigma) / vm, 0 where vm == 0
 *   w        = E W1(F),  W1 = mu1/2 (tr F^T F - d) - mu1 ln J + lam1/2 (ln J)^2        the strain energy per REFERENCE volume
 *
 * Voigt order: nc = 3, (xx, yy, xy) for dim = 2; nc = 6, (xx, yy, zz, yz, xz, xy) for dim = 3; a shear component is the
 * tensor component itself, and its cotangent is the derivative with respect to that one number.  A stress array or its
 * cotangent holds component c of element e and sample b at c*osc + e*ose + b; vm, w and their cotangents are (m, Bp).
 * An element with J <= 0 gets NaN in its own (e, b) entries of sigma, vm and w -- the convention of
 * diffhe_hyper_assemble_rows -- and every other element and sample is unaffected to the bit.
 * The kernels run lanes over samples.  fp64, no atomics: every sum has a fixed order, results are bitwise reproducible. */
#ifndef DIFFHE_HYPER_STRESS_H
#define DIFFHE_HYPER_STRESS_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sigma and / or vm and / or w of every element and sample.  A NULL output is neither computed nor stored (at least one
 * is given); with sigma NULL, osc and ose are ignored and no stress array is touched. */
int diffhe_hyper_stress_eval(const int* elems, const double* gtab, int dim, double lam1, double mu1, const double* u,
                             const double* E, long long e_se, long long e_sb, int n, int m, int Bp, double* sigma,
                             long long osc, long long ose, double* vm, double* w, void* stream);

/* Adjoint of diffhe_hyper_stress_eval for the cotangents sigma_bar (addressed as sigma), vm_bar (m, Bp) and w_bar (m, Bp);
 * each may be NULL, not all three.  Element pass: the state is recomputed; C is the symmetric tensor of sigma_bar +
 * vm_bar d vm / d sigma, each shear cotangent split evenly over its two entries, c_zz (dim = 2) the out-of-plane cotangent
 * of the von Mises chain; with tr3 C = tr C + c_zz and C:s = sum_at C[a][t] s[a][t] + c_zz s_zz
 *
 *   dE[e, b] = C:s + w_bar W1
 *   T        = E { (1/J) [ 2 mu1 C F + lam1 (tr3 C) F^-T ] - (C:s) F^-T } + w_bar E P1(F)        = dL/dH, d x d, NOT symmetric
 *
 * and T goes to work (d*d, m, Bp), T[a][t] at (a*d + t)*m*Bp + e*Bp + b.  Node pass over the incidence list inc_ptr
 * (n+1), inc (codes e*npe + p, diffhe_p1_shape_grad's): u_bar[(i, a), b] = sum_{(e, p) at i} sum_t T_e[a][t] g_p[t], in
 * list order.
 * u_bar (n*d, Bp), work, inc_ptr, inc: all four or none (none: no node pass).  de_e (m, Bp), de_part
 * (diffhe_grad_kappa_blocks(m, Bp), Bp) and de_sum (Bp) are those of diffhe_elast_grad (de_part and de_sum both or
 * neither); all three may be NULL when u_bar is given.  Padding samples b >= B get u_bar = 0 and dE = 0 and their
 * cotangents are not read. */
int diffhe_hyper_stress_adjoint(const int* elems, const double* gtab, int dim, double lam1, double mu1, const double* u,
                                const double* E, long long e_se, long long e_sb, const double* sigma_bar, long long osc,
                                long long ose, const double* vm_bar, const double* w_bar, const int* inc_ptr,
                                const int* inc, int n, int m, int B, int Bp, double* work, double* u_bar, double* de_e,
                                double* de_part, double* de_sum, void* stream);

/* dE of the element pass summed over the samples b < B in a fixed order, de (m): the gradient of a field the batch
 * shares.  The (m, Bp) array is never formed. */
int diffhe_hyper_stress_adjoint_shared(const int* elems, const double* gtab, int dim, double lam1, double mu1,
                                       const double* u, const double* E, long long e_se, long long e_sb,
                                       const double* sigma_bar, long long osc, long long ose, const double* vm_bar,
                                       const double* w_bar, int n, int m, int B, int Bp, double* de, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_HYPER_STRESS_H */
