// The strip kernels of fp64 vectors (fp64 V-cycle, CG step, residuals, applies): dia_strip_kernel<double, ...> /
// dia_strip_shift_kernel<double, ...>.
#include "lattice_strip.h"

namespace diffhe_lattice __attribute__((visibility("hidden"))) {

// Every launch_strip of this vector type the cycle, the driver and the ABI entries (lattice_cycle.hip, lattice_pcg.hip,
// lattice_abi.hip) call, once:
// the kernel inventory of this unit (lattice_strip_f32.hip has the other type).  Each line instantiates the batch-shared,
// shifted and per-sample coefficient variants for 3 and 4 diagonals that its MATS admits.
#define INST(TV_, ...)                                                                                              \
  template void launch_strip<TV_, __VA_ARGS__>(const Level&, int, const double*, const TV_*, const TV_*, TV_*, double, \
                                               double, double*, int, const StripGeom&, hipStream_t, const Extra&)
INST(double, M_JACOBI, false, F_NONE, double, 8, 1, MAT_ANY);         // op_jacobi, fp64 cycle; diffhe_lattice_smooth
INST(double, M_JACOBI, true, F_NONE, double, 8, 1, MAT_ANY);          // op_jacobi_first2, fp64 cycle
INST(double, M_JACOBI, false, F_PROLONG, double, 8, 1, MAT_ANY);      // vcycle way up, fp64 cycle
INST(double, M_RESID, false, F_NONE, double, 8, 1, MAT_ANY);          // op_residual, fp64; residual_pass (r and its fp32 copy)
INST(double, M_RESID, false, F_RESTRICT, double, 5, 1, MAT_ANY);      // resid_restrict, fp64 cycle
INST(double, M_APPLY, false, F_NONE, double, 8, 1, MAT_ANY);          // op_apply_dot, diffhe_lattice_bilinear / _apply_shared
INST(double, M_APPLY, false, F_PUPD_NX, double, 4, 1, MAT_ANY);       // CG step, fp64 directions; diffhe_lattice_cg_step
INST(double, M_APPLY, false, F_PUPD_NX, float, 4, 7, MAT_ANY);        // solve: Bv == 1; diffhe_lattice_cg_step: any Bv
INST(double, M_APPLY, false, F_PUPD_NX, float, 4, 4, MAT_PER_SAMPLE); // CG step, fp32 directions, Bv != 1
INST(double, M_APPLY, false, F_RUPD, float, 4, 5, MAT_SHARED);        // residual update with A p recomputed (rupd: Bv == 1)
INST(double, M_APPLY, false, F_RPAIR, float, 4, 5, MAT_SHARED);       // ... on the fp32 pair (the default of that path)
INST(double, M_APPLY, false, F_RDROP, float, 4, 5, MAT_SHARED);       // ... reading the pair, storing hi alone (the transition)
INST(double, M_APPLY, false, F_RSINGLE, float, 4, 5, MAT_SHARED);     // ... on hi alone (after it)
INST(double, M_RESID, false, F_RPAIR, double, 8, 1, MAT_SHARED);      // residual_pass writing the pair
INST(double, M_APPLY, false, F_PUPD, float, 4, 1, MAT_ANY);           // diffhe_lattice_cg_step with the iterate update, fp32 z
INST(double, M_APPLY, false, F_PUPD, double, 4, 1, MAT_ANY);          // diffhe_lattice_cg_step with the iterate update, fp64 z
#undef INST

}  // namespace diffhe_lattice
