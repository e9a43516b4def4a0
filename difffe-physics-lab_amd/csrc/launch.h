// Launch plumbing shared by the feature units, on top of common.h: the 64-bit index type, the dispatch of a runtime
// dimension to a template argument, the padded batch, and the "group of LB lanes per item" mapping with its fixed-order
// reduction.  The host half is plain C++ (DIFFHE_HD, as common.h): a host compiler may include this header for it alone.
#pragma once
#include <type_traits>

#include "common.h"

namespace diffhe {

using i64 = long long;

// f(std::integral_constant<int, D>{}) for D = dim, one of LO .. HI; returns what f returns.  The caller has refused a dim
// outside the range: such a dim would run f with HI.
template <int LO, int HI, class F>
inline auto dispatch_dim(int dim, F&& f) {
  static_assert(LO <= HI, "empty range");
  if constexpr (LO < HI) {
    if (dim == LO) return f(std::integral_constant<int, LO>{});
    return dispatch_dim<LO + 1, HI>(dim, f);
  } else {
    return f(std::integral_constant<int, HI>{});
  }
}

// f(std::true_type{}) or f(std::false_type{})
template <class F>
inline auto dispatch_bool(bool v, F&& f) {
  if (v) return f(std::true_type{});
  return f(std::false_type{});
}

// the padded batch node_map takes (valid_batch_pad of common.h): a power of two below a wave, whole waves above
DIFFHE_HD inline int batch_pad(int B) {
  if (B >= kWave) return (B + kWave - 1) / kWave * kWave;
  int Bp = 1;
  while (Bp < B) Bp <<= 1;
  return Bp;
}

// LB lanes per item: the batch rounded up to a power of two, at most a wave; items per wave = 64 / LB
DIFFHE_HD inline int group_lanes(int B) {
  const int Bp = batch_pad(B);
  return Bp < kWave ? Bp : kWave;
}

// grid.x of a group_map kernel: 256-thread blocks of 4 * (64 / LB) items over `count` items, at most `cap`, at least 1
DIFFHE_HD inline unsigned group_grid(i64 count, int LB, i64 cap) {
  const int ipb = 4 * (kWave / LB);
  i64 gx = (count + ipb - 1) / ipb;
  if (gx > cap) gx = cap;
  return (unsigned)(gx < 1 ? 1 : gx);
}

#if defined(__HIPCC__)

// A group of LB lanes per item (a band row, a facet, an element), LB a power of two <= 64; block = 256 threads = 4 waves,
// grid.x strides the items.  Lane `sub` of a group takes the samples b = sub, sub + LB, ...  All lanes of a group share
// the item and so every trip count: the xor shuffles of group_sum never leave the group.
struct GroupMap {
  int sub;     // lane inside the group
  i64 item0;   // first item of this lane
  i64 stride;  // item stride of the grid-stride loop
};

__device__ inline GroupMap group_map(int LB) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ipw = kWave / LB;
  GroupMap m;
  m.sub = lane % LB;
  m.item0 = ((i64)blockIdx.x * 4 + wave) * ipw + lane / LB;
  m.stride = (i64)gridDim.x * 4 * ipw;
  return m;
}

// one butterfly step on a double or on every entry of an array of them
__device__ __forceinline__ void xor_add(double& v, int off) { v += __shfl_xor(v, off); }
template <class T, int N>
__device__ __forceinline__ void xor_add(T (&v)[N], int off) {
#pragma unroll
  for (int k = 0; k < N; ++k) xor_add(v[k], off);
}

// Sum each argument (doubles, arrays of them) over the LB lanes of a group: a fixed-order xor butterfly, offsets
// ascending from 1 (LB = 1: nothing to do).  Every lane of the group gets the sums.
template <class... T>
__device__ __forceinline__ void group_sum(int LB, T&... v) {
  for (int off = 1; off < LB; off <<= 1) (xor_add(v, off), ...);
}

// A scalar datum per item and sample, read or written in place: a base pointer (NULL: absent), a stride per item and a
// stride per sample (0: shared by the batch, or summed over it)
template <class T>
struct Strided {
  T* v;
  i64 si, sb;
  __device__ T& at(i64 item, int b) const { return v[item * si + (i64)b * sb]; }
};

#endif  // __HIPCC__

}  // namespace diffhe
