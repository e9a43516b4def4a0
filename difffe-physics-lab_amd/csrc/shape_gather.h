// The node pass of a node-coordinate gradient, shared by shape.hip and elastic_shape.hip: the vertex contributions an
// element pass left in work (m, (d+1) d) are summed per node in the fixed order of the incidence list
// (diffhe/plan.py: SolvePlan.shape_incidence).  No floating-point atomics: bitwise reproducible.
#pragma once
#include "common.h"

namespace diffhe {
namespace {

// grad[i, k] = sum over the incidence list of node i (codes e * (d+1) + p, element order) of work[code * d + k]
__global__ __launch_bounds__(256) void shape_gather_kernel(const int* __restrict__ inc_ptr, const int* __restrict__ inc,
                                                           const double* __restrict__ work, int n, int dim,
                                                           double* __restrict__ grad) {
  typedef long long i64;
  for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < (i64)n * dim; t += (i64)gridDim.x * blockDim.x) {
    const i64 i = t / dim;
    const int k = (int)(t - i * dim);
    double s = 0.0;
    for (int j = inc_ptr[i]; j < inc_ptr[i + 1]; ++j) s += work[(i64)inc[j] * dim + k];
    grad[t] = s;
  }
}

// the node pass on `stream`, after the element pass that wrote `work`
inline void launch_shape_gather(const int* inc_ptr, const int* inc, const double* work, int n, int dim, double* grad,
                                hipStream_t stream) {
  long long gb = ((long long)n * dim + 255) / 256;
  if (gb > 8192) gb = 8192;
  hipLaunchKernelGGL(shape_gather_kernel, dim3((unsigned)gb), dim3(256), 0, stream, inc_ptr, inc, work, n, dim, grad);
}

}  // namespace
}  // namespace diffhe
