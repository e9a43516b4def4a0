// Internal header of the lattice fast path: what its units share -- level and fusion types, constants, the device
// helpers more than one kernel family uses, the predicates and tile geometry of the dispatch, and the declarations of
// the launchers each unit defines.  The workspace layout of the solve is lattice_layout.h's.
#pragma once
#include "common.h"
#include "lattice_layout.h"

// One internal namespace for all lattice units; nothing in it is exported from the library.  Kernels sit in an
// anonymous namespace inside their unit.
namespace diffhe_lattice __attribute__((visibility("hidden"))) {

using namespace diffhe;

struct Level {
  int nx, ny, n, W, nd;
  const double* v;          // (nd, n, Bv)
  const float* v32;         // optional fp32 copy of v, used by the fp32 V-cycle's strip kernels
  const _Float16* o16;      // optional fp16 off-diagonals (nd - 1, n, Bv), times 1 / osc[b], of a per-sample matrix (Bv == Bp):
                            // with it v32 holds ONLY the main diagonal (n, Bv), adjusted so that every row sum equals
                            // the fp64 matrix's
  const double* osc;        // (Bv) per-sample powers of two >= the sample's largest free-row diagonal entry: stored
                            // off-diagonals lie in [-1, 1] whatever the magnitude of that sample's kappa
  const float* rd32;        // optional (n) fp32 reciprocal of the main diagonal of a batch-SHARED level matrix (Bv == 1):
                            // with v32 and mk32 it switches the fp32 V-cycle to the two-samples-per-lane strip kernels
  const float* mk32;        // (n) 0.0f on Dirichlet rows, 1.0f elsewhere (scalar-loadable form of bc)
  const unsigned char* bc;  // (n)
  const void* inv;          // optional dense inverse (n, n) of a batch-shared level matrix, in the V-cycle's storage type
  const double* shift;      // optional (n) batch-shared diagonal shift: A_b = scale_b * K + diag(shift) (reaction term
                            // c M_L on a FACTORED operator; 0 on Dirichlet rows); NULL = none
};

// Matrix-value storage of the strip kernels: fp64; fp32 copies (fp32 V-cycle, per-sample matrices); or `h16m`: fp32 main
// diagonal + fp16 off-diagonals (8 instead of 12 B per node and sample for 3 diagonals).  The preconditioner only has to
// be spectrally close to A: rounding an edge weight to fp16 (2^-11 relative) while the diagonal keeps every ROW SUM of
// the fp64 matrix perturbs A by a graph Laplacian with edge weights 2^-11 |a_ij| -- spectrally equivalent within 0.1 %,
// the null-space behaviour of the smooth modes untouched (a rounded diagonal would shift them by 2^-11 |a_ii| >>
// lambda_min).  Range: the off-diagonals of sample b are stored divided by a power of two >= that sample's largest
// free-row diagonal entry (|a_ij| <= max a_ii for an SPD matrix), so kappa of any magnitude -- and samples of very
// different magnitudes in one batch -- fit; what fp16 cannot hold is contrast INSIDE a sample: couplings below
// 2^-19 of the scale keep fewer than 5 bits (subnormals) and flush to 0 below 2^-25, so the packing kernel reports them and
// the host falls back to plain fp32 copies for that solve (dia_pack_h16_kernel).  bf16 (no scaling needed) was measured
// one PCG iteration worse on the bench workload (10 + 10 against 9 + 9).
struct h16m {};   // tag type
template <typename TM> struct MatTypes { typedef TM diag; typedef TM off; };
template <> struct MatTypes<h16m> { typedef float diag; typedef _Float16 off; };
__device__ __forceinline__ double ldc(const double* __restrict__ p, unsigned lv) { return p[lv]; }
__device__ __forceinline__ double ldc(const float* __restrict__ p, unsigned lv) { return (double)p[lv]; }
__device__ __forceinline__ double ldc(const _Float16* __restrict__ p, unsigned lv) { return (double)(float)p[lv]; }

// 1/d for the smoother: hardware v_rcp_f64 (~2^-23 relative) + one Newton step (~1e-14) -- 4 instructions
// instead of the ~30 of an IEEE fp64 division.  D^-1 only has to be the same positive diagonal everywhere in
// the preconditioner, so the remaining 1e-14 is immaterial.
__device__ inline double fast_rcp(double d) {
  const double r0 = __builtin_amdgcn_rcp(d);
  return fma(r0, fma(-d, r0, 1.0), r0);
}

enum { M_APPLY = 0, M_RESID = 1, M_JACOBI = 2 };
// Fusions folded into the window load:
//   F_PROLONG: the operand is x + P e (coarse-grid correction added on the fly; with M_JACOBI this
//              is "prolongate, correct and post-smooth" in one pass);
//   F_PUPD:    the operand is the NEW search direction p = z + beta p_old of the CG (with M_APPLY
//              this is "update p, apply A, dot p.Ap" in one pass); the kernel also stores p and
//              applies the pending iterate update x += alpha_prev p_old.
//   F_RESTRICT (with M_RESID): the residual is not stored; it is restricted on the fly (P1 full
//              weighting) into the coarse right-hand side.  The strip then covers the 2 CW + 1 fine
//              columns 2 J0 - 1 .. 2 J0 + 2 CW - 1 that feed the wave's CW coarse columns (one fine
//              column is shared with -- and recomputed by -- each neighbour strip) and the tile the
//              fine rows 2 I0 - 1 .. 2 I1 - 1 of the coarse rows I0 .. I1 - 1.
//   F_PROLONG with M_RESID and NO x operand (xin == NULL; the full-multigrid start's fine level): the operand IS the
//              prolonged coarse iterate rounded to the storage type -- the very values mg_prolong2_kernel /
//              mg_prolong_add_kernel (set) store, 0 on fine Dirichlet nodes.  The strip stores them for its own
//              columns (ex.p_out) and the residual rhs - A (P e) as the plain residual pass does: one pass for two.
enum { F_NONE = 0, F_PROLONG = 1, F_PUPD = 2, F_RESTRICT = 3, F_PUPD_NX = 4, F_RUPD = 5, F_RPAIR = 6, F_RDROP = 7, F_RSINGLE = 8 };
// F_RUPD (with M_APPLY): the CG's residual update with A p RECOMPUTED from the stored direction p (TA, ex.p_in) instead of
// read back: r -= alpha (A p), the fp32 copy of r and the partials of r.r in one pass -- for a batch-shared matrix (scalar
// loads, no coefficient traffic) reading p's window (4 B + halo) is cheaper than writing and re-reading A p (8 + 8 B).
// F_PUPD_NX: F_PUPD without the iterate update (the solver's form: x is assembled from the kept directions at the
// end); a compile-time variant so that the x stream costs neither registers nor instructions
// F_RPAIR: the residual is carried as a PAIR of fp32 vectors instead of one fp64 and its fp32 copy: R = rs r (rs the
// per-sample power of two of ex.rscale, so R is exact) as hi + lo with hi = (float)R -- the very vector the V-cycle
// reads, ex.r32 -- and lo = (float)(R - hi) in ex.rlo (common.h split / join; 2^-48 relative per update).  With M_APPLY
// it is F_RUPD on the pair (p 4 B, hi and lo read and written: 20 B per node and sample instead of 24), with M_RESID
// the residual pass that opens the CG loop (x, b read, hi and lo written: 24 B instead of 28; the partials are those
// of F_NONE).  The solver's default on the path where F_RUPD applies; DIFFHE_PCG_RESID_FP64 keeps the fp64 residual.
// F_RDROP, F_RSINGLE (with M_APPLY): the same update once the solve is within 2^16 of the level its energy rule stops at
// (pcg_scalar_kernel, S_BETA), where the low half no longer buys anything the stop rules can see.  F_RDROP is the
// transition: it reads the pair and stores hi = (float)R alone (16 B), rlo is dead afterwards; F_RSINGLE reads and
// writes hi only (12 B).  One template, told apart by rupd_reads_lo / rupd_writes_lo (common.h pair_update); r.r is
// taken from the value stored in every form.  DIFFHE_PCG_RESID_KEEP_LO keeps F_RPAIR throughout.
constexpr int kPcgKnownBits = DIFFHE_PCG_FP32 | DIFFHE_PCG_FMG | (3 << DIFFHE_PCG_FMG_CYCLES_SHIFT) | DIFFHE_PCG_NO_FLOOR |
                              DIFFHE_PCG_WARM | DIFFHE_PCG_UNFUSED | DIFFHE_PCG_DENSE_SCALAR | DIFFHE_PCG_CLOSED_FP32_STEP |
                              DIFFHE_PCG_PRE2;
static_assert((DIFFHE_PCG_RESID_FP64 & kPcgKnownBits) == 0, "DIFFHE_PCG_RESID_FP64 must be a bit of its own");
static_assert((DIFFHE_PCG_RESID_KEEP_LO & (kPcgKnownBits | DIFFHE_PCG_RESID_FP64)) == 0,
              "DIFFHE_PCG_RESID_KEEP_LO must be a bit of its own");
static_assert(((15 << DIFFHE_PCG_TRUST_ITS_SHIFT) & (kPcgKnownBits | DIFFHE_PCG_RESID_FP64 | DIFFHE_PCG_RESID_KEEP_LO)) == 0,
              "the four bits at DIFFHE_PCG_TRUST_ITS_SHIFT must be their own");
static_assert((DIFFHE_PCG_SPLIT_START & (kPcgKnownBits | DIFFHE_PCG_RESID_FP64 | DIFFHE_PCG_RESID_KEEP_LO |
                                         (15 << DIFFHE_PCG_TRUST_ITS_SHIFT))) == 0,
              "DIFFHE_PCG_SPLIT_START must be a bit of its own");
constexpr bool is_pupd(int fuse) { return fuse == F_PUPD || fuse == F_PUPD_NX; }
constexpr bool is_rpair(int fuse) { return fuse == F_RPAIR || fuse == F_RDROP || fuse == F_RSINGLE; }   // hi (+ lo) forms
constexpr bool rupd_reads_lo(int fuse) { return fuse == F_RPAIR || fuse == F_RDROP; }
constexpr bool rupd_writes_lo(int fuse) { return fuse == F_RPAIR; }
constexpr bool is_rupd(int fuse) { return fuse == F_RUPD || is_rpair(fuse); }
// M_RESID, F_RPAIR differs from M_RESID, F_NONE in what it stores only
constexpr bool plain_resid(int mode, int fuse) { return mode == M_RESID && (fuse == F_NONE || fuse == F_RPAIR); }

struct Extra {
  const void* a0;           // F_PROLONG: coarse correction e (TA);  F_PUPD: z (TA)
  const void* p_in;         // F_PUPD: previous search direction, stored as TA (the type of z)
  void* p_out;              // F_PUPD: new search direction, stored as TA;  M_RESID, F_PROLONG without x: the prolonged
                            //   iterate, stored as TV
  double* x;                // F_PUPD: iterate, updated in place (NULL: left alone -- the solver keeps its directions
                            //   and forms x once at the end, pcg_finish_kernel)
  const double* alpha;      // F_PUPD: per-sample alpha of the previous iteration
  const double* beta;       // F_PUPD
  int first;                // F_PUPD: first iteration (p = z, nothing pending)
  int cW;                   // F_PROLONG, F_RESTRICT: row width of the coarse level
  const unsigned char* bc;  // F_PROLONG: fine Dirichlet flags (no correction there); F_RESTRICT: coarse flags
  const double* dotv;       // M_APPLY, F_NONE: dot (A x + addv) against this vector instead of x
  const double* addv;       // M_APPLY, F_NONE: batch-shared (n) vector added to A x (may be NULL)
  float* r32;               // M_RESID, F_NONE, fp64 vectors: also store the residual rounded to fp32 (may be NULL)
  const double* rscale;     //   ... multiplied by this per-sample power of two first (may be NULL: 1)
  const double* sub;        // M_APPLY, F_NONE: y = A x - sub_scale[b] * sub[i], sub batch-shared (n) (may be NULL) ...
  const double* sub_scale;  //   per-sample factor of `sub` (NULL: 1)
  int sub_pb;               //   ... or, sub_pb != 0, one value per sample: sub is (n, Bp) (the Dirichlet lift of per-sample matrices)
  const unsigned char* mask;  // M_APPLY, F_NONE: rows with mask[i] != 0 are stored as 0 (may be NULL)
  int dot_bx;               // M_RESID, F_NONE: the partial sums hold b.x (energy of the iterate) instead of r.r ...
  double* part2;            //   ... and these (same layout as `part`) x.(A x)
  float* rlo;               // F_RPAIR, F_RDROP: low parts of the residual pair (the high parts are r32; rscale applies)
};

// Workgroups are handed to the 8 XCDs round-robin by linear id, so blocks x = k (mod 8) share one L2.
// Give each such class a contiguous range of tiles: spatially adjacent strips (which read each other's
// halo columns / rows) then run on the same XCD at about the same time and the halo hits its L2.
__device__ inline int xcd_tile(int x, int gx) {
  const int q = gx >> 3, rem = gx & 7;
  const int k = x & 7, j = x >> 3;
  return k * q + (k < rem ? k : rem) + j;
}

constexpr int kStripCols = 8;
// fp32-stored V-cycle vectors run best on 4-column strips (kernel trace, same box: prolongation + sweep -7 %,
// first two sweeps -5 % against 8 columns); fp64 vectors keep 8 (half the register footprint per column there)
template <typename TV>
constexpr int strip_cols() { return sizeof(TV) == 4 ? 4 : kStripCols; }
constexpr int kRestrictCols = 2;  // coarse columns per wave of the fused residual + restriction (5 fine columns; 3, 4, 6: slower)
constexpr int kPupdCols = 4;  // narrower strips for the 3-stream fused CG kernel: fewer VGPRs, more waves
// blocks (of 4 waves) a strip-kernel launch aims at; the tile height follows from it
constexpr int kStripBlocks = 6144;
// small levels: one wave marching down a strip is latency-bound; the simple kernels win below ~200^2
// 128: the 129^2 level of a 1024^2 hierarchy takes the strip / fused kernels too (-0.7 ms per step; 64: slower again)
constexpr int kStripMinW = 128;

struct StripGeom {
  bool use;
  int ncb, nrc, TR;
};

// The tile-height rule of every strip-shaped launch: `rows` rows are cut into tiles so that the ncb column blocks x gy
// batch rows of the grid come to about `target` blocks, with no fewer than cap_div rows per tile (in the mean) and -- for
// launches that leave one partial sum per block -- no more than part_cap blocks per batch row (0: no partials, no cap).
inline StripGeom tile_geom(int rows, int ncb, int gy, int target, int cap_div, int part_cap) {
  StripGeom g{true, ncb, 0, 0};
  int nrc = (target + ncb * gy - 1) / (ncb * gy);
  if (nrc > rows / cap_div) nrc = rows / cap_div;
  if (nrc < 1) nrc = 1;
  while (part_cap && ncb * nrc > part_cap) --nrc;
  g.TR = (rows + nrc - 1) / nrc;
  g.nrc = (rows + g.TR - 1) / g.TR;
  return g;
}

inline StripGeom strip_geom(const Level& L, int Bp, int rw = kStripCols, int spl = 1, int nw = 4) {
  const StripGeom none{false, 0, 0, 0};
  if (Bp < kWave || L.W < kStripMinW || L.ny + 1 < 64) return none;
  const int ncb = (L.W + nw * rw - 1) / (nw * rw);   // nw = waves (strips) per block
  const int gy = Bp / (kWave * spl);   // spl = samples per lane (2: dia_strip2_kernel)
  if (gy < 1) return none;   // fewer samples than one wave of that form holds
  // target: the same number of WAVES (and tile height) whatever the block width
  return tile_geom(L.ny + 1, ncb, gy, kStripBlocks * 4 / nw, 8, kPartBlocks);
}

inline dim3 lgrid(int n, int Bp) { return node_grid(n, Bp, 2048); }  // <= kPartBlocks partial rows

__device__ inline double shift_at(const Level& L, int i) { return L.shift ? L.shift[i] : 0.0; }

__device__ inline int dia_off(const Level& L, int k) { return k == 1 ? 1 : (k == 2 ? L.W : L.nx); }

// sum_j K[i,j] x[j] for sample b (unscaled)
template <typename TV>
__device__ inline double dia_row(const Level& L, int Bv, int vb, const TV* __restrict__ x, int i, int b, int Bp) {
  const i64 n = L.n;
  double acc = L.v[(i64)i * Bv + vb] * (double)x[(i64)i * Bp + b];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    if (k < L.nd) {
      const int off = dia_off(L, k);
      if (i + off < L.n) acc += L.v[((i64)k * n + i) * Bv + vb] * (double)x[(i64)(i + off) * Bp + b];
      if (i - off >= 0) acc += L.v[((i64)k * n + (i - off)) * Bv + vb] * (double)x[(i64)(i - off) * Bp + b];
    }
  }
  return acc;
}

__device__ inline double row_scale(const Level& L, const double* __restrict__ scale, int i, int b) {
  return (scale && !L.bc[i]) ? scale[b] : 1.0;
}

#define STORE_PARTIAL(part, val)                                                          \
  do {                                                                                    \
    const double t__ = block_sum_per_sample((val), Bp, lds);                              \
    if ((threadIdx.x >> 6) == 0 && (threadIdx.x & 63) < (Bp < kWave ? Bp : kWave))        \
      (part)[(i64)blockIdx.x * Bp + nm.b] = t__;                                          \
  } while (0)

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f ld2(const float* __restrict__ p, unsigned lb) { return *(const v2f*)(p + lb); }
__device__ __forceinline__ void st2(float* __restrict__ p, unsigned lb, v2f v) { *(v2f*)(p + lb) = v; }
// Buffer addressing: one resource descriptor per stream (base = the tile's first window row, one column left of the
// strip), a loop-invariant 32-bit per-lane byte offset per column (VGPR) and a wave-uniform 32-bit byte offset per
// row (SGPR, one s_add per iteration): "buffer_load_dwordx2 v, v_off, s[rsrc], s_row offen" -- no 64-bit address
// arithmetic per access (the flat-pointer form cost a v_lshl_add_u64 per load and ~50 scalar adds per row).
// Offsets are relative to the TILE, so they stay far below 2^32 whatever the size of the vector (checked on the host).
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, -1, 0x00020000);
}
__device__ __forceinline__ v2f bld(rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
__device__ __forceinline__ void bst(rsrc_t r, unsigned voff, unsigned soff, v2f v) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), r, voff, soff, 0);
}

// per-sample sum over the NW waves of a block (lanes hold distinct samples); valid in wave 0.  NW == 4: the same order
// of additions as block_sum_per_sample (results of the default geometry stay bitwise what they were)
template <int NW>
__device__ __forceinline__ double block_sum_waves(double v, double* lds /* >= NW * 64 doubles */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  lds[wave * kWave + lane] = v;
  __syncthreads();
  double s = 0.0;
  if (wave == 0) {
    if (NW == 4) {
      s = (lds[lane] + lds[kWave + lane]) + (lds[2 * kWave + lane] + lds[3 * kWave + lane]);
    } else {
#pragma unroll
      for (int w = 0; w < NW; ++w) s += lds[w * kWave + lane];
    }
  }
  __syncthreads();
  return s;
}

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
struct Acc { double v[4] = {0.0, 0.0, 0.0, 0.0}; };   // per-sample dot-product accumulators of one lane (kSpl used)

template <typename VT> struct VLane;
template <> struct VLane<float> {
  static constexpr int kSpl = 1;
  static __device__ __forceinline__ float zero() { return 0.0f; }
  static __device__ __forceinline__ float ld(rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
  }
  static __device__ __forceinline__ float from_scale(const double* __restrict__ s, unsigned lb) { return s ? (float)s[lb] : 1.0f; }
  static __device__ __forceinline__ void dot(Acc& s, float a, float b) { s.v[0] += (double)(a * b); }
};
template <> struct VLane<v2f> {
  static constexpr int kSpl = 2;
  static __device__ __forceinline__ v2f zero() { return v2f{0.0f, 0.0f}; }
  static __device__ __forceinline__ v2f ld(rsrc_t r, unsigned voff, unsigned soff) { return bld(r, voff, soff); }
  static __device__ __forceinline__ v2f from_scale(const double* __restrict__ s, unsigned lb) {
    return s ? v2f{(float)s[lb], (float)s[lb + 1]} : v2f{1.0f, 1.0f};
  }
  static __device__ __forceinline__ void dot(Acc& s, v2f a, v2f b) {
    const v2f p = a * b;
    s.v[0] += (double)p.x;
    s.v[1] += (double)p.y;
  }
};
// FOUR samples per lane, 256 per wave: one 16-byte access per lane and node -- half the vector-memory instructions per
// byte of the two-sample form (the fused passes are bound by the NUMBER of those instructions),
// twice the registers per lane (2 waves per SIMD instead of 4: the same bytes in flight per SIMD).
template <> struct VLane<v4f> {
  static constexpr int kSpl = 4;
  static __device__ __forceinline__ v4f zero() { return v4f{0.0f, 0.0f, 0.0f, 0.0f}; }
  static __device__ __forceinline__ v4f ld(rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
  }
  static __device__ __forceinline__ v4f from_scale(const double* __restrict__ s, unsigned lb) {
    return s ? v4f{(float)s[lb], (float)s[lb + 1], (float)s[lb + 2], (float)s[lb + 3]} : v4f{1.0f, 1.0f, 1.0f, 1.0f};
  }
  static __device__ __forceinline__ void dot(Acc& s, v4f a, v4f b) {
    const v4f p = a * b;
    s.v[0] += (double)p.x;
    s.v[1] += (double)p.y;
    s.v[2] += (double)p.z;
    s.v[3] += (double)p.w;
  }
};

// A vector stream of the fused kernels: buffer-resource addressing (raw_buffer_load, 32-bit per-lane offset + uniform
// SGPR row offset).  Global loads off a wave-uniform 64-bit base (the form strip_body uses) spilled and ran slower
// (DESIGN.md section 6, round 4), although the PMC counters show the texture-addresser FIFOs full 28-35 % of the time in
// the buffer-load kernels and never in strip_body's.
struct Src {
  rsrc_t r;
};
__device__ __forceinline__ Src make_src(const void* p) { return Src{make_rsrc(p)}; }
template <typename VT>
__device__ __forceinline__ VT ldsrc(const Src& s, unsigned voff, unsigned soff) { return VLane<VT>::ld(s.r, voff, soff); }

// Where the matrix coefficients of the fused passes come from.
//   SHARED: batch-shared fp32 copies + reciprocal diagonal, wave-uniform scalar loads (values are plain floats);
//   per sample: fp32 diagonal + scaled fp16 off-diagonals (Level.v32 / o16 / osc), one value per sample and lane,
//   buffer loads with tile-relative offsets; the reciprocal diagonal is v_rcp_f32 of the loaded diagonal.
template <typename VT, bool SHARED> struct Coef;
template <typename VT> struct Coef<VT, true> {
  typedef float T;
  const float *v0, *v1, *v2, *v3, *rdp;
  __device__ __forceinline__ Coef(const Level& L, i64, unsigned, int) : v0(L.v32), v1(L.v32 + L.n), v2(L.v32 + 2 * (i64)L.n),
                                                                        v3(L.v32 + 3 * (i64)L.n), rdp(L.rd32) {}
  __device__ __forceinline__ T d(i64 i) const { return v0[i]; }
  __device__ __forceinline__ T e(i64 i) const { return v1[i]; }
  __device__ __forceinline__ T n2(i64 i) const { return v2[i]; }
  __device__ __forceinline__ T q3(i64 i) const { return v3[i]; }
  __device__ __forceinline__ T rd(i64 i, T) const { return rdp[i]; }
};
__device__ __forceinline__ float ldh(rsrc_t r, unsigned voff, float) {
  return (float)__builtin_bit_cast(_Float16, __builtin_amdgcn_raw_buffer_load_b16(r, voff, 0, 0));
}
__device__ __forceinline__ v2f ldh(rsrc_t r, unsigned voff, v2f) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const h2 h = __builtin_bit_cast(h2, __builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0));
  return v2f{(float)h.x, (float)h.y};
}
__device__ __forceinline__ unsigned ldraw(rsrc_t r, unsigned voff, float) {
  return (unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(r, voff, 0, 0);
}
__device__ __forceinline__ unsigned ldraw(rsrc_t r, unsigned voff, v2f) {
  return (unsigned)__builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0);
}
__device__ __forceinline__ float unraw(unsigned raw, float) { return (float)__builtin_bit_cast(_Float16, (unsigned short)raw); }
__device__ __forceinline__ v2f unraw(unsigned raw, v2f) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const h2 h = __builtin_bit_cast(h2, raw);
  return v2f{(float)h.x, (float)h.y};
}
template <typename VT> struct Coef<VT, false> {
  typedef VT T;
  rsrc_t r0, r1, r2, r3;
  i64 base;       // node index the resources are based at (<= every index the tile touches)
  unsigned lb, Bp;
  VT osc;         // this lane's sample scale(s) of the fp16 couplings
  __device__ __forceinline__ Coef(const Level& L, i64 base_, unsigned lb_, int Bp_)
      : base(base_), lb(lb_), Bp((unsigned)Bp_), osc(VLane<VT>::from_scale(L.osc, lb_)) {
    const i64 n = L.n;
    r0 = make_rsrc(L.v32 + base * Bp_);
    r1 = make_rsrc(L.o16 + base * Bp_);
    r2 = make_rsrc(L.o16 + (n + base) * Bp_);
    r3 = make_rsrc(L.o16 + (2 * n + base) * Bp_);
  }
  __device__ __forceinline__ unsigned off(i64 i) const { return (unsigned)(i - base) * Bp + lb; }
  __device__ __forceinline__ T d(i64 i) const { return VLane<VT>::ld(r0, 4u * off(i), 0u); }
  __device__ __forceinline__ T e(i64 i) const { return osc * ldh(r1, 2u * off(i), VT{}); }
  __device__ __forceinline__ T n2(i64 i) const { return osc * ldh(r2, 2u * off(i), VT{}); }
  __device__ __forceinline__ T q3(i64 i) const { return osc * ldh(r3, 2u * off(i), VT{}); }
  __device__ __forceinline__ T rd(i64, T dv) const { return 1.0f / dv; }
  // raw fp16 storage words (one per sample of the lane), for the register-cached coefficient rows of the fused POST pass
  __device__ __forceinline__ unsigned e_raw(i64 i) const { return ldraw(r1, 2u * off(i), VT{}); }
  __device__ __forceinline__ unsigned n2_raw(i64 i) const { return ldraw(r2, 2u * off(i), VT{}); }
  __device__ __forceinline__ T cvt(unsigned raw) const { return osc * unraw(raw, VT{}); }
};

// K_1 x at the NC columns col0 .. col0 + NC - 1 of grid row R, handed column by column to `use(k, K1x, d0, rd)`.
// xm / xc / xp hold x on rows R - 1 / R / R + 1 at the NC + 2 columns col0 - 1 .. col0 + NC (index j <-> column
// col0 - 1 + j); out-of-grid positions must hold 0.  EDGE: the strip / tile touches a grid edge, so the coefficient
// indices of non-existent couplings are clamped into the arrays (their values meet a zero x).
template <typename VT, int NC, int ND, bool EDGE, typename CF, typename F>
__device__ __forceinline__ void k1_row(const CF& cf, i64 n, int W, int R, int col0, const VT* xm, const VT* xc,
                                       const VT* xp, F&& use) {
  const i64 base = (i64)R * W + col0;
  auto at = [&](i64 i) -> i64 { return EDGE ? (i < 0 ? 0 : (i > n - 1 ? n - 1 : i)) : i; };
  typename CF::T ew = cf.e(at(base - 1));       // west coupling of the first column; then carried along the row
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const i64 i = base + k;
    const typename CF::T d0 = cf.d(at(i));
    const typename CF::T ee = cf.e(at(i));
    VT acc = d0 * xc[k + 1];
    acc += ee * xc[k + 2];                       // east  (R, c) - (R, c + 1)
    acc += ew * xc[k];                           // west
    acc += cf.n2(at(i)) * xp[k + 1];             // north (R, c) - (R + 1, c)
    acc += cf.n2(at(i - W)) * xm[k + 1];         // south
    if (ND == 4) {
      acc += cf.q3(at(i)) * xp[k];               // (R, c) - (R + 1, c - 1)
      acc += cf.q3(at(i - W + 1)) * xm[k + 2];   // (R - 1, c + 1) - (R, c)
    }
    use(k, acc, d0, cf.rd(at(i), d0));
    ew = ee;
  }
}

// fp32 V-cycle, batch-shared matrix with fp32 coefficient copies and reciprocal diagonal, batch a multiple of 128,
// no diagonal shift: the two-samples-per-lane kernels apply
inline bool shared32_ok(const Level& L, int Bv, int Bp) {   // the fp32 copies of a batch-shared matrix are there, whole waves
  return Bv == 1 && L.v32 && L.rd32 && L.mk32 && !L.shift && Bp % kWave == 0;
}
inline bool strip2_ok(const Level& L, int Bv, int Bp) { return shared32_ok(L, Bv, Bp) && Bp % (2 * kWave) == 0; }
// the kernels address their tile (`rows` fine rows + the window's two halo rows) with 32-bit byte offsets
inline bool strip2_tile_fits(const Level& L, int Bp, int rows) { return 4LL * (rows + 3) * L.W * Bp < (1LL << 31); }
// geometry for the two-samples-per-lane kernels if they apply to this level (and its tiles fit), else the usual one
template <typename TV>
inline bool strip2_pick(const Level& L, int Bv, int Bp, int rw, StripGeom* g) {
  if (sizeof(TV) == 4 && strip2_ok(L, Bv, Bp)) {
    *g = strip_geom(L, Bp, rw, 2);
    if (!g->use || strip2_tile_fits(L, Bp, g->TR)) return g->use;
  }
  *g = strip_geom(L, Bp, rw, 1);
  return false;
}

// The fused two-stage passes (lattice_fused.hip) apply to: a batch-shared matrix with its fp32 copy, reciprocal diagonal and mask (strip2_ok), or a
// per-sample matrix with the compact copies (fp32 diagonal + scaled fp16 off-diagonals) and the mask, no per-sample scale
// returns a bit mask: 1 = the PRE pass may be fused, 2 = the POST pass
inline int fused_ok(const Level& L, int Bv, int Bp, const double* scale) {
  // batch-shared matrix: two samples per lane for multiples of 128, else ONE per lane (batches of 64 or 192 per GPU --
  // BASELINE config 5's shard: same fused passes, fp32 arithmetic, 4-byte accesses)
  if (shared32_ok(L, Bv, Bp)) return 3;
  // per-sample matrices: both passes fused, with the coefficient rows cached in registers (fp16 couplings as raw words:
  // 174 / 206 VGPRs, 2 waves per SIMD, no spills).  Without the cache the PRE pass needed 256 VGPRs and measured slower
  // than its two single passes (forward solve 153 ms against 140), and the POST pass re-read every coefficient row four
  // times (PMC 4.5 passes of traffic for 2.6 algorithmic); 1024^2 x 256 step: 245 (POST only, uncached) -> 236 (POST
  // cached) -> 219 ms (both, cached; runs r5b, r5d).
  return (Bv == Bp && Bp % (2 * kWave) == 0 && L.v32 && L.o16 && L.mk32 && !L.shift && !scale) ? 3 : 0;
}

// ---- lattice_strip.h, instantiated in lattice_strip_f32.hip / _f64.hip: dia_strip_kernel / dia_strip_shift_kernel -------
// MATS narrows the coefficient variants a call site can reach (its own condition on Bv says which): any, the batch-shared
// ones (Bv == 1, with or without a diagonal shift) or the per-sample ones (Bv == Bp).
enum { MAT_ANY = 0, MAT_SHARED = 1, MAT_PER_SAMPLE = 2 };
template <typename TV, int MODE, bool XFROMB, int FUSE = F_NONE, typename TA = TV, int RW = kStripCols, int MINW = 1,
          int MATS = MAT_ANY>
void launch_strip(const Level& L, int Bv, const double* scale, const TV* xin, const TV* bvec, TV* out,
                  double omega, double omega_in, double* part, int Bp, const StripGeom& g, hipStream_t st,
                  const Extra& ex = Extra{});

// ---- lattice_strip2.hip: dia_strip2_kernel, cgstep2_kernel ------------------------------------------------------------
template <int MODE, bool XFROMB, int FUSE, int RW>
void launch_strip2(const Level& L, const double* scale, const float* xin, const float* bvec, float* out, double omega,
                   double omega_in, double* part, int Bp, const StripGeom& g, hipStream_t st, const Extra& ex = Extra{});
// pout == z (first step only): p0 = z0 already lives in its ring slot -- read in place, nothing stored
void launch_cgstep2(const Level& L, const double* scale, const double* beta, int first, const float* z, const float* pin,
                    float* pout, double* part, int Bp, const StripGeom& g, int spl, hipStream_t st);

// ---- lattice_fused.hip: fused_pre_kernel, fused_post_kernel -----------------------------------------------------------
void launch_fused_pre(const Level& L, const Level& C, int Bv, const double* scale, const float* rhs, float* x2, float* crhs,
                      double w0, double w1, int Bp, const StripGeom& g, int spl, hipStream_t st);
void launch_fused_post(const Level& L, const Level& C, int Bv, const double* scale, const float* xin, const float* rhs,
                       const float* ec, float* z, double wA, double wB, double* part, int Bp, const StripGeom& g, int spl,
                       hipStream_t st);

// ---- host-side hierarchy (lattice_cycle.hip) ----------------------------------------------------------------------------
struct Hier : CycleWork {   // + the per-level work vectors (cycle_carve)
  Level lev[kMaxLevels];
  int nl, Bv, Bp;
  const double* scale;
  double omega[8];  // per-sweep damping (Chebyshev-weighted Jacobi); post-smoothing runs them in reverse
  int nu, n_coarse, fmg_coarse_cycles;
  int fuse;  // 0: four single-stage strip passes per level; 1 / 2: fused two-stage passes, samples per lane
  int pre4;  // the fused PRE pass may take four samples per lane (fused_spl)
  int dense_mfma;  // coarsest-level dense solve of an fp32 cycle on the matrix cores (0: scalar-load kernel)
  int split_start; // full-multigrid start: separate prolongation and residual passes on the fine level (DIFFHE_PCG_SPLIT_START)
  double coarse_lmax;  // upper bound of the spectrum of D^-1 A on the coarsest level (2 for an M-matrix)
};

// bpn = algorithmic bytes per (node, sample) of the launch, for diffhe_traffic_account.  The kernel's arguments are
// passed in full (a kernel's default arguments do not travel through a function pointer).
template <typename K, typename... Args>
inline void launch_nodes(const Hier& H, hipStream_t st, double bpn, K kernel, int n, Args... args) {
  diffhe::account(bpn * (double)n * H.Bp);
  hipLaunchKernelGGL(kernel, lgrid(n, H.Bp), dim3(256), 0, st, args...);
}
// per-sample matrices: bytes of the nd stored diagonals (fp64) per node; a batch-shared matrix is amortised to 0
inline double mat_bytes(const Hier& H, const Level& L) { return H.Bv == 1 ? 0.0 : 8.0 * L.nd; }

int fill_hier(Hier& H, const diffhe_mg_level* levels, int n_levels, int Bv, int Bp, const double* scale,
              const double* omegas, int nu, int n_coarse);
// the one-level hierarchy of the entries that run a single kernel family on one level (apply, bilinear, cg_step; smooth
// sets its own weight afterwards)
int single_level(Hier& H, const diffhe_mg_level* level, int Bv, int Bp, const double* scale);
i64 carve_cycle(Hier& H, double* work, bool fp32);   // cycle_carve over H's levels

// What the driver (lattice_pcg.hip) asks of the cycle unit.  fp32 = storage type of the cycle's vectors; the branch on it
// is taken once, inside.  Those that leave partial sums return the number of partial blocks they wrote.
// z = V(r): the buffer holding z; the last fine sweep leaves the partials of r.z in `part` (*nblocks of them)
// dest (optional, fp32 cycles): where the finest level's last pass should put z; honoured where that pass is the fused POST
// pass or a plain sweep -- the caller tells by the pointer that comes back
const void* cycle_precondition(const Hier& H, bool fp32, const void* r, double* part, int* nblocks, hipStream_t st,
                               void* dest = nullptr);
// full-multigrid start from the right-hand side b0: the iterate (NULL: error recorded), *pending = the fine level's last
// correction, not yet added (may come back NULL)
// have_b1 (fp32 only): the level-1 right-hand side is there already (cycle_cvt_restrict)
const void* cycle_fmg_start(const Hier& H, bool fp32, const void* b0, hipStream_t st, const void** pending,
                            bool have_b1 = false);
// r32 = (float)(rs b) and the level-1 right-hand side of the full-multigrid start, R r32, in one pass: fp32 cycle, level 0
// halves in both directions, Bp a multiple of 64 (the caller's condition: Solve::fused_start)
void cycle_cvt_restrict(const Hier& H, const double* b, const double* rs, float* r32, hipStream_t st);
// level 0, fp64: res = rhs - A x (res may be NULL), partials of r.r -- or, dot_bx, of b.x and (part2) x.(A x)
int cycle_residual(const Hier& H, const double* rhs, const double* x, double* res, double* part, hipStream_t st,
                   int dot_bx = 0, double* part2 = nullptr);
int cycle_apply_dot(const Hier& H, const double* x, double* y, double* part, hipStream_t st);   // level 0: y = A x, x.y
bool direct_ok(const Hier& H, bool fp32);   // one level with the dense inverse of its batch-shared matrix, fp64
void cycle_direct_solve(const Hier& H, const double* b, double* x, hipStream_t st);   // x = (1 / s_b) K_1^{-1} b
int cycle_maxdiag(const Hier& H, double* out /* Bv */, hipStream_t st);   // per-sample max diagonal of level 0
// spectrum bound for the coarsest-level Chebyshev solve (H.coarse_lmax): 2 unless the mesh has obtuse triangles, where
// the Gershgorin bound is taken on the device (`scratch`: one word) and read back (synchronises the stream)
int cycle_coarse_bound(Hier& H, unsigned long long* scratch, hipStream_t st);

// ---- opt-in timing of the step's main kernels INSIDE the solver loop (bench.py's roofline entries; lattice_pcg.hip) -------
enum { KP_CGSTEP = 0, KP_UPDATE = 1, KP_FIRST2 = 2, KP_RESTRICT = 3, KP_PROLONG = 4, KP_SWEEP = 5, KP_COUNT = 6 };
void kp_begin(int id, hipStream_t st);
void kp_end(int id, hipStream_t st);
void kp_collect();  // call with the stream idle: every recorded event has completed

}  // namespace diffhe_lattice
