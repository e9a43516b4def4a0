// Stress recovery of a linear-elastic solve (ours: the reference has scalar unknowns only): element stresses
// sigma = E (2 mu1 eps + lam1 tr(eps) I) in Voigt components, the von Mises stress, and their adjoint with respect to the
// displacement u and the Young's modulus E (definitions: include/diffhe_stress.h).  u is the full displacement, so no
// Dirichlet data is read; the gradient table has aniso.hip's layout and, unlike that table, the true sign of grad phi_p
// in every element: everything here is linear in it.
//
// Data layout as in elastic.hip: dof-major, batch innermost, lanes over samples (node_map), so element data -- node
// ids, gradients, list entries -- is wave-uniform and every access is one contiguous segment; Bp = 1 spreads elements
// over lanes.  fp64, no atomics anywhere: every sum has a fixed order, results are bitwise reproducible.
//
// The adjoint is an element pass and a node pass.  The element pass runs on the element loop of element_grad.h with the
// form below (NC = 1: dE); the form writes the tensor T of the element, nc numbers per element and sample, as a side
// product, and the node pass (stress_node.h, shared with elastic_aniso_stress.hip) gathers T g_p over the per-node
// incidence list (the list of shape.hip's gather).  T costs nc m values per sample where the (d+1) d vertex contributions
// of shape.hip's form would cost (d+1) d m.
//
// Every kernel takes a compile-time EIG: with it the element carries an eigenstrain (eigen_field.h) and the stress is
// E (s(u) - s0) with an out-of-plane component of its own (include/diffhe_eigenstrain.h, whose three stress entries are at
// the end of this unit); without it the instantiations are the ones of diffhe_stress.h, unchanged.  The element and the
// adjoint form live in stress_form.h, which elastic_shape.hip shares for the node-coordinate gradient of the stress.
#include "common.h"
#include "diffhe_eigenstrain.h"
#include "diffhe_stress.h"
#include "eigen_field.h"
#include "element_grad.h"
#include "stress_form.h"
#include "stress_node.h"
#include "launch.h"

namespace {

using namespace diffhe;

// ---------------------------------------------------------------------------------------
// sigma at c*osc + e*ose + b and / or vm (m, Bp); a NULL output is neither computed nor stored.
// ---------------------------------------------------------------------------------------
template <int DIM, bool EIG>
__global__ __launch_bounds__(256) void stress_eval_kernel(const StressElement<DIM, EIG> el_of, int Bp,
                                                           double* __restrict__ sigma, i64 osc, i64 ose,
                                                           double* __restrict__ vm) {
  constexpr int NC = DIM * (DIM + 1) / 2;
  const NodeMap nm = node_map(Bp);  // "nodes" are elements here
  if (nm.b >= Bp) return;
  for (int e = nm.node0; e < el_of.m; e += nm.stride) {
    typename StressElement<DIM, EIG>::Elem el;
    double sg[NC];
    el_of.load(e, el);
    const double tr = el_of.unit_stress(el, Bp, nm.b, sg);
    const double szz = el_of.subtract_initial(el, nm.b, tr, sg);   // EIG only
    const double Ee = el_of.modulus(e, nm.b);
#pragma unroll
    for (int k = 0; k < NC; ++k) sg[k] *= Ee;
    if (sigma) {
#pragma unroll
      for (int k = 0; k < NC; ++k) sigma[k * osc + e * ose + nm.b] = sg[k];
    }
    if (vm) {
      double nn[3];
      normal_stresses<DIM, EIG>(sg, el_of.nu_z, Ee * szz, nn);
      vm[(i64)e * Bp + nm.b] = von_mises<DIM>(sg, nn);
    }
  }
}

// the eigenstrain of one call, as the eigen entries get it (absent: the entries of diffhe_stress.h)
struct EigenArgs {
  const double* eps0;
  i64 zc, ze, zb;
  int plane_strain;
};
const EigenArgs kNoEigen = {nullptr, 0, 0, 0, 0};

template <int DIM, bool EIG>
StressElement<DIM, EIG> element_of(const int* elems, const double* gtab, double lam1, double mu1, double nu_z,
                                   const double* u, const double* E, i64 e_se, i64 e_sb, int m, const EigenArgs& z) {
  StressElement<DIM, EIG> el;
  el.elems = elems, el.gtab = gtab, el.lam1 = lam1, el.mu1 = mu1, el.nu_z = DIM == 2 ? nu_z : 0.0;
  el.u = u, el.E = E, el.ese = e_se, el.esb = e_sb, el.m = m;
  if constexpr (EIG) el.ef = EigenField<DIM>{z.eps0, z.zc, z.ze, z.zb, lam1, mu1, DIM == 2 && z.plane_strain ? 1 : 0};
  return el;
}

template <int DIM, bool EIG>
StressAdjointForm<DIM, EIG> form_of(const StressElement<DIM, EIG>& el, const double* sigma_bar, i64 osc, i64 ose,
                                    const double* vm_bar, double* work, int B, double* deps, i64 dzc, i64 dze) {
  StressAdjointForm<DIM, EIG> f;
  f.el_of = el, f.sigma_bar = sigma_bar, f.osc = osc, f.ose = ose, f.vm_bar = vm_bar, f.work = work, f.B = B;
  if constexpr (EIG) f.deps = deps, f.dzc = dzc, f.dze = dze;
  return f;
}

// what every entry refuses: pointers, dim, sizes, the E strides, the int32 codes e * npe + p
bool bad_common(const int* elems, const double* gtab, int dim, const double* u, const double* E, i64 e_se, i64 e_sb, int n,
                int m) {
  return !elems || !gtab || !u || !E || (dim != 2 && dim != 3) || n < 1 || m < 1 || e_se < 0 || e_sb < 0 ||
         (i64)m * (dim + 1) >= (1LL << 31);
}

// bytes of E as the kernels read it: a field per sample, one field, one number per sample, one number
double modulus_bytes(i64 e_se, i64 e_sb, int m, int Bp) { return 8.0 * (e_se ? (double)m : 1.0) * (e_sb ? (double)Bp : 1.0); }

// bytes of an eps0-shaped array (EIG) with the strides ze, zb
template <bool EIG>
double eigen_array_bytes(int dim, int plane_strain, i64 ze, i64 zb, int m, int Bp) {
  return EIG ? eigen_bytes(dim == 3 ? 6 : (plane_strain ? 4 : 3), ze, zb, m, Bp) : 0.0;
}

// ---------------------------------------------------------------------------------------
// The three entries of either header.
// ---------------------------------------------------------------------------------------
template <int DIM, bool EIG>
int eval_of(const StressElement<DIM, EIG>& el, int Bp, double* sigma, i64 osc, i64 ose, double* vm, void* stream) {
  hipLaunchKernelGGL((stress_eval_kernel<DIM, EIG>), diffhe::node_grid(el.m, Bp), dim3(256), 0, (hipStream_t)stream, el,
                     Bp, sigma, osc, ose, vm);
  return diffhe::check_launch();
}

template <bool EIG>
int stress_eval(const int* elems, const double* gtab, int dim, double lam1, double mu1, double nu_z, const double* u,
                const double* E, i64 e_se, i64 e_sb, const EigenArgs& z, int n, int m, int Bp, double* sigma, i64 osc,
                i64 ose, double* vm, void* stream) {
  if (bad_common(elems, gtab, dim, u, E, e_se, e_sb, n, m) || (!sigma && !vm) || (sigma && (osc < 1 || ose < 1)))
    return DIFFHE_E_BADARG;
  if (EIG && bad_eigen(z.eps0, z.zc, z.ze, z.zb)) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nc = dim * (dim + 1) / 2;
  // u once per dof, E, the outputs (EIG: eps0)
  diffhe::account(8.0 * Bp * ((double)dim * n + (sigma ? (double)nc * m : 0.0) + (vm ? (double)m : 0.0)) +
                  modulus_bytes(e_se, e_sb, m, Bp) + eigen_array_bytes<EIG>(dim, z.plane_strain, z.ze, z.zb, m, Bp));
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return eval_of(element_of<D(), EIG>(elems, gtab, lam1, mu1, nu_z, u, E, e_se, e_sb, m, z), Bp, sigma, osc, ose, vm,
                   stream);
  });
}

template <int DIM, bool EIG>
int adjoint_of(const StressAdjointForm<DIM, EIG>& form, const double* gtab, const int* inc_ptr, const int* inc, int n,
               int m, int B, int Bp, double* u_bar, double* de_e, double* de_part, double* de_sum, double bytes,
               void* stream) {
  constexpr int NC = DIM * (DIM + 1) / 2;
  const int status = diffhe::launch_element_grad(form, m, Bp, de_e, 0, Bp, de_part, de_sum, bytes, stream);
  if (status != DIFFHE_OK || !u_bar) return status;
  diffhe::account(8.0 * Bp * ((double)NC * m + (double)DIM * n));   // node pass: T once, u_bar once per dof
  hipLaunchKernelGGL(stress_node_kernel<DIM>, diffhe::node_grid(n, Bp), dim3(256), 0, (hipStream_t)stream, inc_ptr, inc,
                     gtab, (const double*)form.work, n, m, B, Bp, u_bar);
  return diffhe::check_launch();
}

template <bool EIG>
int stress_adjoint(const int* elems, const double* gtab, int dim, double lam1, double mu1, double nu_z, const double* u,
                   const double* E, i64 e_se, i64 e_sb, const EigenArgs& z, const double* sigma_bar, i64 osc, i64 ose,
                   const double* vm_bar, const int* inc_ptr, const int* inc, int n, int m, int B, int Bp, double* work,
                   double* u_bar, double* de_e, double* de_part, double* de_sum, double* deps, i64 dzc, i64 dze,
                   void* stream) {
  if (bad_common(elems, gtab, dim, u, E, e_se, e_sb, n, m) || (!sigma_bar && !vm_bar) ||
      (sigma_bar && (osc < 1 || ose < 1)) || B < 1 || B > Bp)
    return DIFFHE_E_BADARG;
  if (EIG && (bad_eigen(z.eps0, z.zc, z.ze, z.zb) || (deps && (dzc < 1 || dze < 1)))) return DIFFHE_E_BADARG;
  const bool nodes = u_bar != nullptr;
  if ((work != nullptr) != nodes || (inc_ptr != nullptr) != nodes || (inc != nullptr) != nodes) return DIFFHE_E_BADARG;
  if ((de_part == nullptr) != (de_sum == nullptr) || (!nodes && !deps && !de_e && !de_part)) return DIFFHE_E_BADARG;
  if (!diffhe::valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const int nc = dim * (dim + 1) / 2;
  // element pass: u once per dof, E, the cotangents, T and dE per element (EIG: eps0, and d eps0 per element)
  const double bytes = 8.0 * Bp * ((double)dim * n + (sigma_bar ? (double)nc * m : 0.0) + (vm_bar ? (double)m : 0.0) +
                                   (nodes ? (double)nc * m : 0.0) + (de_e ? (double)m : 0.0)) +
                       modulus_bytes(e_se, e_sb, m, Bp) + eigen_array_bytes<EIG>(dim, z.plane_strain, z.ze, z.zb, m, Bp) +
                       (deps ? eigen_array_bytes<EIG>(dim, z.plane_strain, 1, 1, m, Bp) : 0.0);
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return adjoint_of(form_of(element_of<D(), EIG>(elems, gtab, lam1, mu1, nu_z, u, E, e_se, e_sb, m, z), sigma_bar, osc,
                              ose, vm_bar, work, B, deps, dzc, dze),
                      gtab, inc_ptr, inc, n, m, B, Bp, u_bar, de_e, de_part, de_sum, bytes, stream);
  });
}

template <bool EIG>
int stress_adjoint_shared(const int* elems, const double* gtab, int dim, double lam1, double mu1, double nu_z,
                          const double* u, const double* E, i64 e_se, i64 e_sb, const EigenArgs& z,
                          const double* sigma_bar, i64 osc, i64 ose, const double* vm_bar, int n, int m, int B, int Bp,
                          double* de, void* stream) {
  if (bad_common(elems, gtab, dim, u, E, e_se, e_sb, n, m) || (!sigma_bar && !vm_bar) ||
      (sigma_bar && (osc < 1 || ose < 1)) || !de || B < 1 || B > Bp)
    return DIFFHE_E_BADARG;
  if (EIG && bad_eigen(z.eps0, z.zc, z.ze, z.zb)) return DIFFHE_E_BADARG;
  const int nc = dim * (dim + 1) / 2;
  const double bytes = 8.0 * (Bp * ((double)dim * n + (sigma_bar ? (double)nc * m : 0.0) + (vm_bar ? (double)m : 0.0)) +
                              (double)m) + modulus_bytes(e_se, e_sb, m, Bp) +
                       eigen_array_bytes<EIG>(dim, z.plane_strain, z.ze, z.zb, m, Bp);
  return diffhe::dispatch_dim<2, 3>(dim, [&](auto D) {
    return diffhe::launch_element_grad_shared(
        form_of(element_of<D(), EIG>(elems, gtab, lam1, mu1, nu_z, u, E, e_se, e_sb, m, z), sigma_bar, osc, ose, vm_bar,
                nullptr, B, nullptr, 0, 0),
        m, B, Bp, de, 0, 1, bytes, stream);
  });
}

}  // namespace

// =========================================================================================
// C ABI (include/diffhe_stress.h)
// =========================================================================================
extern "C" int diffhe_stress_eval(const int* elems, const double* gtab, int dim, double lam1, double mu1, double nu_z,
                                  const double* u, const double* E, long long e_se, long long e_sb, int n, int m, int Bp,
                                  double* sigma, long long osc, long long ose, double* vm, void* stream) {
  return stress_eval<false>(elems, gtab, dim, lam1, mu1, nu_z, u, E, e_se, e_sb, kNoEigen, n, m, Bp, sigma, osc, ose, vm,
                            stream);
}

extern "C" int diffhe_stress_adjoint(const int* elems, const double* gtab, int dim, double lam1, double mu1, double nu_z,
                                     const double* u, const double* E, long long e_se, long long e_sb,
                                     const double* sigma_bar, long long osc, long long ose, const double* vm_bar,
                                     const int* inc_ptr, const int* inc, int n, int m, int B, int Bp, double* work,
                                     double* u_bar, double* de_e, double* de_part, double* de_sum, void* stream) {
  return stress_adjoint<false>(elems, gtab, dim, lam1, mu1, nu_z, u, E, e_se, e_sb, kNoEigen, sigma_bar, osc, ose, vm_bar,
                               inc_ptr, inc, n, m, B, Bp, work, u_bar, de_e, de_part, de_sum, nullptr, 0, 0, stream);
}

extern "C" int diffhe_stress_adjoint_shared(const int* elems, const double* gtab, int dim, double lam1, double mu1,
                                            double nu_z, const double* u, const double* E, long long e_se, long long e_sb,
                                            const double* sigma_bar, long long osc, long long ose, const double* vm_bar,
                                            int n, int m, int B, int Bp, double* de, void* stream) {
  return stress_adjoint_shared<false>(elems, gtab, dim, lam1, mu1, nu_z, u, E, e_se, e_sb, kNoEigen, sigma_bar, osc, ose,
                                      vm_bar, n, m, B, Bp, de, stream);
}

// =========================================================================================
// C ABI (include/diffhe_eigenstrain.h): the same three with an eigenstrain
// =========================================================================================
extern "C" int diffhe_stress_eval_eigen(const int* elems, const double* gtab, int dim, double lam1, double mu1,
                                        int plane_strain, const double* u, const double* E, long long e_se,
                                        long long e_sb, const double* eps0, long long zc, long long ze, long long zb,
                                        int n, int m, int Bp, double* sigma, long long osc, long long ose, double* vm,
                                        void* stream) {
  return stress_eval<true>(elems, gtab, dim, lam1, mu1, 0.0, u, E, e_se, e_sb, EigenArgs{eps0, zc, ze, zb, plane_strain},
                           n, m, Bp, sigma, osc, ose, vm, stream);
}

extern "C" int diffhe_stress_adjoint_eigen(const int* elems, const double* gtab, int dim, double lam1, double mu1,
                                           int plane_strain, const double* u, const double* E, long long e_se,
                                           long long e_sb, const double* eps0, long long zc, long long ze, long long zb,
                                           const double* sigma_bar, long long osc, long long ose, const double* vm_bar,
                                           const int* inc_ptr, const int* inc, int n, int m, int B, int Bp, double* work,
                                           double* u_bar, double* de_e, double* de_part, double* de_sum, double* deps,
                                           long long dzc, long long dze, void* stream) {
  return stress_adjoint<true>(elems, gtab, dim, lam1, mu1, 0.0, u, E, e_se, e_sb,
                              EigenArgs{eps0, zc, ze, zb, plane_strain}, sigma_bar, osc, ose, vm_bar, inc_ptr, inc, n, m, B,
                              Bp, work, u_bar, de_e, de_part, de_sum, deps, dzc, dze, stream);
}

extern "C" int diffhe_stress_adjoint_eigen_shared(const int* elems, const double* gtab, int dim, double lam1, double mu1,
                                                  int plane_strain, const double* u, const double* E, long long e_se,
                                                  long long e_sb, const double* eps0, long long zc, long long ze,
                                                  long long zb, const double* sigma_bar, long long osc, long long ose,
                                                  const double* vm_bar, int n, int m, int B, int Bp, double* de,
                                                  void* stream) {
  return stress_adjoint_shared<true>(elems, gtab, dim, lam1, mu1, 0.0, u, E, e_se, e_sb,
                                     EigenArgs{eps0, zc, ze, zb, plane_strain}, sigma_bar, osc, ose, vm_bar, n, m, B, Bp, de,
                                     stream);
}
