/* Stress recovery and quadratic failure criteria of anisotropic elastic solves on P1 triangles and tetrahedra: the
 * thirteenth public header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes), of diffhe_elastic_aniso.h (Voigt order, engineering shear strains, the stiffness as the upper triangle
 * of its matrix read through three strides) and of diffhe_stress.h (storage of a stress array, the oriented gradient
 * table): every array is a device pointer, vectors are batch innermost, `stream` is a hipStream_t, the return value is
 * DIFFHE_OK or a DIFFHE_E_* status.  diffhe_hip.h, the other twelve headers and DIFFHE_ABI_VERSION are unchanged by them;
 * the Python binding keeps them in a table of their own (diffhe/_hip.py, ELASTIC_ANISO_STRESS_SIGNATURES).
 *
 * Definitions.  u (n*d, Bp) is the FULL displacement, prescribed values included; gtab (npe*d, m) holds g_p = grad phi_p
 * WITH its sign.  nv = 3 / 6 Voigt components, nt = nv (nv + 1) / 2 = 6 / 21, nk = nv + nt = 9 / 27.  Per element e and
 * sample b, with H[a][t] = sum_p u[(p, a)] g_p[t]:
 *
 *   eps_I    = H[a][a] on the normal components, H[a][t] + H[t][a] on the shears         engineering Voigt strain
 *   sigma_I  = sum_J C_IJ eps_J                                                          a shear entry is the tensor component
 *   phi      = sum_I q_I sigma_I + sum_IJ Q_IJ sigma_I sigma_J                            the failure index
 *
 * C holds component t of its row-major upper triangle at t*c_sc + e*c_se + b*c_sb; an off-diagonal component is ONE
 * parameter that fills both symmetric entries.  The criterion `crit` holds nk components at k*k_sc + e*k_se + b*k_sb: q
 * first (nv), then the row-major upper triangle of the symmetric Q (nt), under the same rule.  Strides are >= 0; a zero
 * stride shares the datum over elements or samples.  A stress array or its cotangent holds component c of element e and
 * sample b at c*osc + e*ose + b; phi and its cotangent are (m, Bp).
 * The kernels run lanes over samples.  fp64, no atomics: every sum has a fixed order, results are bitwise reproducible. */
#ifndef DIFFHE_ELASTIC_ANISO_STRESS_H
#define DIFFHE_ELASTIC_ANISO_STRESS_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sigma and / or phi of every element and sample.  A NULL output is neither computed nor stored (at least one is given):
 * phi alone never stores sigma; with sigma NULL, osc and ose are ignored.  crit is required with phi and ignored without. */
int diffhe_elastc_stress_eval(const int* elems, const double* gtab, int dim, const double* u, const double* C,
                              long long c_sc, long long c_se, long long c_sb, const double* crit, long long k_sc,
                              long long k_se, long long k_sb, int n, int m, int Bp, double* sigma, long long osc,
                              long long ose, double* phi, void* stream);

/* Adjoint of diffhe_elastc_stress_eval for the cotangents sigma_bar (addressed as sigma) and phi_bar (m, Bp); either may be
 * NULL, not both; crit is required with phi_bar.  Element passes: the state is recomputed and, with the combined cotangent
 * c = sigma_bar + phi_bar (q + 2 Q sigma),
 *
 *   dC_IJ = c_I eps_J + [I != J] c_J eps_I        I <= J, nt components
 *   dq_I  = phi_bar sigma_I                        dQ_IJ = (1 + [I != J]) phi_bar sigma_I sigma_J, I <= J: nk components
 *   T     = dL/dH: the symmetric tensor with the Voigt components t = C c
 *
 * T goes to work (nv, m, Bp).  Node pass over the incidence list inc_ptr (n+1), inc (codes e*npe + p,
 * diffhe_p1_shape_grad's): u_bar[(i, a), b] = sum_{(e, p) at i} sum_t T_e[a][t] g_p[t], in list order -- the node pass of
 * diffhe_stress_adjoint.
 * u_bar (n*d, Bp), work, inc_ptr, inc: all four or none (none: no node pass).  dc_e holds component t of element e and
 * sample b at t*dc_sc + e*dc_se + b; dc_part (diffhe_grad_kappa_blocks(m, Bp), nt, Bp) and dc_sum (nt, Bp) are those of
 * diffhe_elastc_grad (both or neither).  dk_e, dk_sc, dk_se, dk_part (.., nk, Bp), dk_sum (nk, Bp): the same for the
 * criterion (phi_bar required).  The gradients of C and of the criterion are separate kernel instantiations; any of the
 * three groups may be absent, not all.  Padding samples b >= B get zeros everywhere and their cotangents are not read. */
int diffhe_elastc_stress_adjoint(const int* elems, const double* gtab, int dim, const double* u, const double* C,
                                 long long c_sc, long long c_se, long long c_sb, const double* crit, long long k_sc,
                                 long long k_se, long long k_sb, const double* sigma_bar, long long osc, long long ose,
                                 const double* phi_bar, const int* inc_ptr, const int* inc, int n, int m, int B, int Bp,
                                 double* work, double* u_bar, double* dc_e, long long dc_sc, long long dc_se,
                                 double* dc_part, double* dc_sum, double* dk_e, long long dk_sc, long long dk_se,
                                 double* dk_part, double* dk_sum, void* stream);

/* dC and / or the criterion's gradient of the element passes summed over the samples b < B in a fixed order: dc holds
 * component t of element e at t*dc_sc + e*dc_se, dk component k at k*dk_sc + e*dk_se; at least one is given (dk: phi_bar
 * required).  The gradient of a field the batch shares; the per-sample arrays are never formed.  The two are separate
 * launches, so a per-sample C with a shared criterion takes dk here and dC from diffhe_elastc_stress_adjoint. */
int diffhe_elastc_stress_adjoint_shared(const int* elems, const double* gtab, int dim, const double* u, const double* C,
                                        long long c_sc, long long c_se, long long c_sb, const double* crit,
                                        long long k_sc, long long k_se, long long k_sb, const double* sigma_bar,
                                        long long osc, long long ose, const double* phi_bar, int n, int m, int B, int Bp,
                                        double* dc, long long dc_sc, long long dc_se, double* dk, long long dk_sc,
                                        long long dk_se, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_ELASTIC_ANISO_STRESS_H */
