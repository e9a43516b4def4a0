// The element loop of a coefficient gradient: dL/dc[e, b] for a coefficient c the operator is linear in (scalar kappa,
// conductivity tensor, Young's modulus), per element and sample or summed over the batch.  A family supplies the element
// formula as a form struct that travels to the kernel by value:
//
//   struct Form {
//     static constexpr int NC;                                  // values per element and sample
//     struct Elem;                                              // what is wave-uniform per element
//     __device__ void load(int e, Elem&) const;
//     __device__ void eval(const Elem&, int Bp, int b, double* out /* NC */) const;   // sample b of the (.., Bp) fields
//   };
//
// AnisoForm<DIM> lives in aniso.hip; KappaForm in ell_assemble.hip drives the batch-shared kernel only, and elastic.hip
// takes the second stage alone (their other kernels measured slower on this loop and keep their own).  Everything else --
// thread mapping, output strides, the two-stage per-sample total, the batch reduction, grid sizing -- is here, once.
// No floating-point atomics: every sum has a fixed order and the results are bitwise reproducible.
#pragma once
#include "common.h"

namespace diffhe {
namespace {

// ---------------------------------------------------------------------------------------
// Per sample: lanes run over samples, a grid-stride loop walks the elements.  dk_e (c, e, b) at c*osc + e*ose + b
// (optional), and the block partial sums over the elements per sample, dk_part (nblk, NC, Bp) (optional): first stage of
// the per-sample total.
// ---------------------------------------------------------------------------------------
template <class Form>
__global__ __launch_bounds__(256) void element_grad_kernel(const Form form, int m, int Bp, double* __restrict__ dk_e,
                                                            long long osc, long long ose,
                                                            double* __restrict__ dk_part) {
  constexpr int NC = Form::NC;
  __shared__ double lds[4 * kWave];
  const NodeMap nm = node_map(Bp);  // "nodes" are elements here
  const bool ok = nm.b < Bp;
  double s[NC];
#pragma unroll
  for (int t = 0; t < NC; ++t) s[t] = 0.0;
  if (ok)
    for (int e = nm.node0; e < m; e += nm.stride) {
      typename Form::Elem el;
      double dk[NC];
      form.load(e, el);
      form.eval(el, Bp, nm.b, dk);
#pragma unroll
      for (int t = 0; t < NC; ++t) {
        if (dk_e) dk_e[t * osc + e * ose + nm.b] = dk[t];
        s[t] += dk[t];
      }
    }
  if (!dk_part) return;   // kernel argument: the whole block leaves together
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < NC; ++t) {
    const double r = block_sum_per_sample(s[t], Bp, lds);
    if (wave == 0 && lane < (Bp < kWave ? Bp : kWave) && ok) dk_part[((long long)blockIdx.x * NC + t) * Bp + nm.b] = r;
  }
}

// Second stage: out[j] = sum over the blocks of part[k, j], j < width (= NC * Bp), one chain per wave, in a fixed order.
__global__ __launch_bounds__(256) void element_sum_partials_kernel(const double* __restrict__ part, int nblk, int width,
                                                                    double* __restrict__ out) {
  __shared__ double lds[4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * kWave + lane;
  double s = 0.0;
  if (j < width)
    for (int k = wave; k < nblk; k += 4) s += part[(long long)k * width + j];
  lds[wave * kWave + lane] = s;
  __syncthreads();
  if (wave == 0 && j < width) out[j] = (lds[lane] + lds[kWave + lane]) + (lds[2 * kWave + lane] + lds[3 * kWave + lane]);
}

// ---------------------------------------------------------------------------------------
// Summed over the batch, dk (c, e) at c*osc + e*ose, for a field all samples share: one wave per element at a time, its
// lanes walk the samples b < B in a fixed order and meet in a fixed-order wave reduction, so the (m, Bp) per-sample
// gradient (4.3 GB at 1024^2 x 256) is never written.
// ---------------------------------------------------------------------------------------
template <class Form>
__global__ __launch_bounds__(256) void element_grad_shared_kernel(const Form form, int m, int B, int Bp,
                                                                   double* __restrict__ dk, long long osc,
                                                                   long long ose) {
  constexpr int NC = Form::NC;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int e = blockIdx.x * 4 + wave; e < m; e += gridDim.x * 4) {
    typename Form::Elem el;
    double s[NC];
    form.load(e, el);
#pragma unroll
    for (int t = 0; t < NC; ++t) s[t] = 0.0;
    for (int b = lane; b < B; b += kWave) {   // padding samples (b >= B) carry no gradient
      double d[NC];
      form.eval(el, Bp, b, d);
#pragma unroll
      for (int t = 0; t < NC; ++t) s[t] += d[t];
    }
#pragma unroll
    for (int t = 0; t < NC; ++t) {
      double r = s[t];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) r += __shfl_xor(r, d);
      if (lane == 0) dk[t * osc + e * ose] = r;
    }
  }
}

// ---------------------------------------------------------------------------------------
// Host side.  `bytes` is the family's algorithmic traffic (account()).  dk_part is sized by diffhe_grad_kappa_blocks and
// summed into dk_sum (NC, Bp) by the second stage.
// ---------------------------------------------------------------------------------------
template <class Form>
inline int launch_element_grad(const Form& form, int m, int Bp, double* dk_e, long long osc, long long ose,
                               double* dk_part, double* dk_sum, double bytes, void* stream) {
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  const dim3 grid = node_grid(m, Bp);
  if ((int)grid.x != diffhe_grad_kappa_blocks(m, Bp)) return DIFFHE_E_BADARG;
  account(bytes);
  hipLaunchKernelGGL(element_grad_kernel<Form>, grid, dim3(256), 0, (hipStream_t)stream, form, m, Bp, dk_e, osc, ose,
                     dk_part);
  if (dk_part) {
    const int width = Form::NC * Bp;
    hipLaunchKernelGGL(element_sum_partials_kernel, dim3((width + 63) / 64), dim3(256), 0, (hipStream_t)stream,
                       (const double*)dk_part, (int)grid.x, width, dk_sum);
  }
  return check_launch();
}

template <class Form>
inline int launch_element_grad_shared(const Form& form, int m, int B, int Bp, double* dk, long long osc, long long ose,
                                      double bytes, void* stream) {
  if (!valid_batch_pad(Bp)) return DIFFHE_E_BATCHPAD;
  long long blocks = ((long long)m + 3) / 4;
  if (blocks > 16384) blocks = 16384;
  account(bytes);
  hipLaunchKernelGGL(element_grad_shared_kernel<Form>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, form, m,
                     B, Bp, dk, osc, ose);
  return check_launch();
}

}  // namespace
}  // namespace diffhe
