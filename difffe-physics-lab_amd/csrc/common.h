// Shared device/host helpers for libdiffhe_hip (gfx950 only, wave = 64).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DIFFHE_HD __host__ __device__
#else
#define DIFFHE_HD
#endif

namespace diffhe {

// A double carried as the unevaluated sum of two floats (the CG residual of the lattice solver, lattice_strip.h F_RPAIR):
// hi is exactly (float)R -- what a plain fp32 copy of R would hold -- and lo the float nearest to the remainder R - hi
// (exact in fp64: hi has 24 of R's 53 bits).  hi + lo keeps 48 bits of R, |join(split(R)) - R| <= 2^-48 |R|, as long as
// lo is a normal float; a remainder below the fp32 range flushes towards 0 and costs nothing but those bits.
// Plain C++ below this line up to the HIP-only part: a host compiler may include this header for these functions alone.
DIFFHE_HD inline void split(double R, float& hi, float& lo) {
  hi = (float)R;
  lo = (float)(R - (double)hi);
}
DIFFHE_HD inline double join(float hi, float lo) { return (double)hi + (double)lo; }

// One residual update R <- R - t on that pair (t = rs alpha (A p), fp64), in the three forms of lattice.h:
//   READ_LO, WRITE_LO  (F_RPAIR)    R = hi + lo - t, stored as split(R): 2^-48 relative;
//   READ_LO only       (F_RDROP)    R = hi + lo - t, stored as hi = (float)R alone: lo is dead afterwards;
//   neither            (F_RSINGLE)  R = hi - t,      stored as hi = (float)R: a plain fp32 residual, 2^-25 relative.
// hi (and lo where written) are updated in place; returns the value actually STORED, what r.r is taken from.
template <bool READ_LO, bool WRITE_LO>
DIFFHE_HD inline double pair_update(float& hi, float& lo, double t) {
  static_assert(READ_LO || !WRITE_LO, "a pair that is written is read by the next update");
  const double R = (READ_LO ? join(hi, lo) : (double)hi) - t;
  if (WRITE_LO) {
    split(R, hi, lo);
    return join(hi, lo);
  }
  hi = (float)R;
  return (double)hi;
}

constexpr int kWave = 64;

// Bp must be a power of two <= 64 or a multiple of 64 (see diffhe_hip.h).
inline bool valid_batch_pad(int Bp) {
  if (Bp <= 0) return false;
  if (Bp <= 64) return (Bp & (Bp - 1)) == 0;
  return (Bp % 64) == 0;
}

// grid.x of node_grid below: blocks of 4 waves over the nodes, each wave holding kWave / min(Bp, kWave) nodes
inline int node_blocks(int n, int Bp, int max_blocks_x = 2048) {
  const int LB = Bp < kWave ? Bp : kWave;
  const int npw = kWave / LB;
  long long groups = ((long long)n + 4 * npw - 1) / (4 * npw);
  int gx = (int)(groups < max_blocks_x ? groups : max_blocks_x);
  return gx < 1 ? 1 : gx;
}

}  // namespace diffhe

#if defined(__HIPCC__)
#include <stdint.h>

#include "diffhe_hip.h"

namespace diffhe {

void set_last_error(hipError_t e);

// Algorithmic-byte accounting (diffhe_traffic_account): every launch on the solve path adds the unique bytes it
// must read + write once (batch-shared data counts 0).  Process-wide: the adjoint solve runs on
// autograd's thread.  bench.py divides the total of a step by the step's duration for the step-level roofline.
void account(double bytes);

// Post-launch check: records the HIP error text and maps to DIFFHE_E_LAUNCH.
inline int check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(e);
    return DIFFHE_E_LAUNCH;
  }
  return DIFFHE_OK;
}

inline int check(hipError_t e) {
  if (e != hipSuccess) {
    set_last_error(e);
    return DIFFHE_E_LAUNCH;
  }
  return DIFFHE_OK;
}

// Node-major thread mapping shared by every (n, Bp) kernel.
//   lanes over samples: LB = min(Bp, 64); nodes per wave: NPW = 64 / LB
//   block = 256 threads = 4 waves; grid.y = sample chunks of 64; grid.x strides nodes
struct NodeMap {
  int b;       // sample index of this lane
  int node0;   // first node of this lane
  int stride;  // node stride of the grid-stride loop
};

__device__ inline NodeMap node_map(int Bp) {
  const int LB = Bp < kWave ? Bp : kWave;
  const int npw = kWave / LB;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  NodeMap m;
  m.b = blockIdx.y * kWave + (lane % LB);
  m.node0 = (blockIdx.x * 4 + wave) * npw + lane / LB;
  m.stride = gridDim.x * 4 * npw;
  return m;
}

// Sum `v` over the lanes that hold the same sample (lane % LB equal), then over
// the block's 4 waves; the result is valid in wave 0, lanes < LB.
__device__ inline double block_sum_per_sample(double v, int Bp, double* lds /* >= 4*64 doubles */) {
  const int LB = Bp < kWave ? Bp : kWave;
  for (int off = LB; off < kWave; off <<= 1) v += __shfl_xor(v, off);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  lds[wave * kWave + lane] = v;
  __syncthreads();
  double s = 0.0;
  if (wave == 0) s = (lds[lane] + lds[kWave + lane]) + (lds[2 * kWave + lane] + lds[3 * kWave + lane]);
  __syncthreads();
  return s;
}

// The epilogue of a kernel that leaves one partial sum per block and sample: row blockIdx.x of `part` gets the block's sum
// of `s` for sample b (ok: this lane holds a sample).  Every thread of the block must call it (two barriers inside).
__device__ inline void store_block_partial(double s, double* __restrict__ part, int Bp, int b, bool ok, double* lds) {
  const double t = block_sum_per_sample(s, Bp, lds);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave == 0 && lane < (Bp < kWave ? Bp : kWave) && ok) part[(long long)blockIdx.x * Bp + b] = t;
}

inline dim3 node_grid(int n, int Bp, int max_blocks_x = 2048) {
  return dim3(node_blocks(n, Bp, max_blocks_x), (Bp + kWave - 1) / kWave, 1);
}

}  // namespace diffhe

#endif  // __HIPCC__
