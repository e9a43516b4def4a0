/* Eigenstrain (initial strain) loads and stresses of linear-elastic solves on P1 triangles and tetrahedra: the fourth
 * public header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes), diffhe_elastic.h and diffhe_stress.h: every array is a device pointer, vectors are batch innermost,
 * `stream` is a hipStream_t, the return value is DIFFHE_OK or a DIFFHE_E_* status.  The three other headers and
 * DIFFHE_ABI_VERSION are unchanged by them; the Python binding keeps them in a table of their own (diffhe/_hip.py,
 * EIGENSTRAIN_SIGNATURES).
 *
 * Definitions.  Voigt order, shear components and their cotangents as in diffhe_stress.h.  The eigenstrain eps0 has
 * nc0 = 3 components (xx, yy, xy) in plane stress (dim = 2, plane_strain = 0), nc0 = 4, (xx, yy, xy, zz), in plane strain
 * (dim = 2, plane_strain = 1: the total eps_zz is 0, so an eps0_zz is constrained and loads the body in plane), and
 * nc0 = 6 for dim = 3 (plane_strain ignored).  Component c of element e and sample b lies at c*zc + e*ze + b*zb; ze = 0
 * and / or zb = 0 read one tensor for all elements and / or samples in place.  E per element and sample at e*e_se + b*e_sb.
 * gtab (npe*d, m) holds g_p = grad phi_p with its TRUE sign in every element (the load and the stress are linear in it),
 * vol (m) the element sizes.  Per element and sample
 *
 *   s0[a][t] = 2 mu1 eps0[a][t] + lam1 theta0 delta_at,  theta0 = tr eps0 over all stored normal components,
 *   s0_zz    = 2 mu1 eps0_zz + lam1 theta0                                       (plane strain),
 *   F0[(i, a), b] = sum_{(e, p) at i} vol_e E_e sum_t s0_e[a][t] g_p[t]          the eigenstrain load,
 *   sigma    = E (s(u) - s0) in plane,  s(u) the unit stress of diffhe_stress.h,
 *   sigma_zz = E [lam1 (tr_in-plane eps(u) - theta0) - 2 mu1 eps0_zz]            in plane strain, 0 in plane stress,
 *
 * and vm from the full tensor.  d vm / d sigma = 0 where vm == 0: no NaN or Inf leaves these kernels for finite inputs.
 * fp64, no floating-point atomics: every sum has a fixed order, results are bitwise reproducible.  Padding samples
 * b >= B get zeros and their cotangents are not read. */
#ifndef DIFFHE_EIGENSTRAIN_H
#define DIFFHE_EIGENSTRAIN_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* F0 (n*d, Bp): a node pass over the incidence list inc_ptr (n+1), inc (codes e*npe + p, diffhe_p1_shape_grad's), in list
 * order; s0 is recomputed per incident (e, p).  Every row is written, rows of fixed dofs included. */
int diffhe_eigenstrain_load(const int* inc_ptr, const int* inc, const double* gtab, const double* vol, int dim,
                            double lam1, double mu1, int plane_strain, const double* E, long long e_se, long long e_sb,
                            const double* eps0, long long zc, long long ze, long long zb, int n, int m, int B, int Bp,
                            double* F0, void* stream);

/* Adjoint of the load for a cotangent w (n*d, Bp).  Element pass: W[a][t] = sum_p w[(p, a)] g_p[t];
 *   d/d eps0_aa = vol E (2 mu1 W_aa + lam1 tr W),  d/d eps0_at = vol E 2 mu1 (W_at + W_ta) for a != t,
 *   d/d eps0_zz = vol E lam1 tr W (plane strain),  d/d E = vol s0 : sym(W).
 * deps gets component c of element e and sample b at c*osc + e*ose + b (may be NULL).  de_e (m, Bp), de_part
 * (diffhe_grad_kappa_blocks(m, Bp), Bp) and de_sum (Bp) are those of diffhe_elast_grad (de_part and de_sum both or neither);
 * all three may be NULL when deps is given. */
int diffhe_eigenstrain_load_adjoint(const int* elems, const double* gtab, const double* vol, int dim, double lam1,
                                    double mu1, int plane_strain, const double* E, long long e_se, long long e_sb,
                                    const double* eps0, long long zc, long long ze, long long zb, const double* w, int n,
                                    int m, int B, int Bp, double* deps, long long osc, long long ose, double* de_e,
                                    double* de_part, double* de_sum, void* stream);

/* d/d E of the load summed over the samples b < B in a fixed order, de (m): the gradient of a field the batch shares. */
int diffhe_eigenstrain_load_adjoint_shared(const int* elems, const double* gtab, const double* vol, int dim, double lam1,
                                           double mu1, int plane_strain, const double* E, long long e_se, long long e_sb,
                                           const double* eps0, long long zc, long long ze, long long zb, const double* w,
                                           int n, int m, int B, int Bp, double* de, void* stream);

/* diffhe_stress_eval with an eigenstrain: sigma = E (s(u) - s0) and / or vm, arguments as there. */
int diffhe_stress_eval_eigen(const int* elems, const double* gtab, int dim, double lam1, double mu1, int plane_strain,
                             const double* u, const double* E, long long e_se, long long e_sb, const double* eps0,
                             long long zc, long long ze, long long zb, int n, int m, int Bp, double* sigma, long long osc,
                             long long ose, double* vm, void* stream);

/* diffhe_stress_adjoint with an eigenstrain.  With c = sigma_bar + vm_bar d vm / d sigma, c_zz included: u_bar as there,
 * dE[e, b] = sum_k c_k (s - s0)_k over the in-plane components and zz, and d / d eps0 = -E times the unit-stress map applied
 * to the tensor of c (each shear cotangent split evenly, zz through the formula above), to deps at c*dzc + e*dze + b (may be
 * NULL).  The dE outputs may all be NULL when u_bar or deps is given. */
int diffhe_stress_adjoint_eigen(const int* elems, const double* gtab, int dim, double lam1, double mu1, int plane_strain,
                                const double* u, const double* E, long long e_se, long long e_sb, const double* eps0,
                                long long zc, long long ze, long long zb, const double* sigma_bar, long long osc,
                                long long ose, const double* vm_bar, const int* inc_ptr, const int* inc, int n, int m,
                                int B, int Bp, double* work, double* u_bar, double* de_e, double* de_part, double* de_sum,
                                double* deps, long long dzc, long long dze, void* stream);

/* dE of that element pass summed over the samples b < B in a fixed order, de (m). */
int diffhe_stress_adjoint_eigen_shared(const int* elems, const double* gtab, int dim, double lam1, double mu1,
                                       int plane_strain, const double* u, const double* E, long long e_se, long long e_sb,
                                       const double* eps0, long long zc, long long ze, long long zb,
                                       const double* sigma_bar, long long osc, long long ose, const double* vm_bar, int n,
                                       int m, int B, int Bp, double* de, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_EIGENSTRAIN_H */
