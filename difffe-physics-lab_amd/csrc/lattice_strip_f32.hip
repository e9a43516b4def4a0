// The strip kernels of fp32-stored vectors (the fp32 V-cycle): dia_strip_kernel<float, ...> / dia_strip_shift_kernel<float, ...>.
#include "lattice_strip.h"

namespace diffhe_lattice __attribute__((visibility("hidden"))) {

// Every launch_strip of this vector type the cycle, the driver and the ABI entries (lattice_cycle.hip, lattice_pcg.hip,
// lattice_abi.hip) call, once:
// the kernel inventory of this unit (lattice_strip_f64.hip has the other type).  Each line instantiates the batch-shared,
// shifted and per-sample coefficient variants for 3 and 4 diagonals that its MATS admits.
#define INST(TV_, ...)                                                                                              \
  template void launch_strip<TV_, __VA_ARGS__>(const Level&, int, const double*, const TV_*, const TV_*, TV_*, double, \
                                               double, double*, int, const StripGeom&, hipStream_t, const Extra&)
INST(float, M_JACOBI, false, F_NONE, float, 4, 1, MAT_ANY);           // op_jacobi, fp32 cycle
INST(float, M_JACOBI, true, F_NONE, float, 4, 1, MAT_ANY);            // op_jacobi_first2, fp32 cycle
INST(float, M_JACOBI, false, F_PROLONG, float, 4, 1, MAT_ANY);        // vcycle way up, fp32 cycle, unfused
INST(float, M_RESID, false, F_NONE, float, 8, 1, MAT_ANY);            // op_residual, fp32 cycle (fmg_start)
INST(float, M_RESID, false, F_RESTRICT, float, 5, 1, MAT_ANY);        // resid_restrict, fp32 cycle, one sample per lane
INST(float, M_RESID, false, F_PROLONG, float, 8, 5, MAT_SHARED);      // fmg_start, fine level: prolongation + residual in one pass
#undef INST

}  // namespace diffhe_lattice
