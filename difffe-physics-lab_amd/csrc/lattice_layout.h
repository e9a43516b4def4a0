// Workspace layout of the lattice solve and the low-half policy of its residual pair.  Plain C++: lattice.h includes it
// for the units, and a host compiler may include it alone (tests/test_lattice_workspace_host.py).  The solve and
// diffhe_lattice_pcg_workspace_doubles both go through the two carves below; no offset of `work` is written anywhere else.
#pragma once

namespace diffhe_lattice __attribute__((visibility("hidden"))) {

typedef long long i64;

constexpr int kMaxLevels = 16;
constexpr int kPartBlocks = 2048;  // capacity (in blocks) of every partial-sum buffer
// Directions kept before the iterate is touched: 10 fp32 slots (5 fp64) -- solves of up to 10 iterations (the 9 + 9 of a
// per-element field per sample) form x ONCE, in pcg_finish_kernel; round 3's 6 slots flushed such a solve twice
constexpr int kRingSlots = 10;
constexpr int kScalarSlices = 16;  // rows of the slice table (pcg_slice_kernel)

// ---- the V-cycle's vectors ------------------------------------------------------------------------------------------
struct CycleWork {
  void *xa[kMaxLevels], *xb[kMaxLevels], *res[kMaxLevels], *rhs[kMaxLevels];  // TV vectors of the V-cycle
  void *bF[kMaxLevels], *xF[kMaxLevels];  // full-multigrid start: restricted right-hand sides, iterates
};

// Carved in units of doubles (fp32 vectors take half, rounded up to 64 B): xa, xb, res, rhs, [bF below level 0,] xF per
// level, n_nodes[l] * Bp elements each.  work == NULL: the size alone, no pointers.
inline i64 cycle_carve(CycleWork& w, double* work, const int* n_nodes, int nl, int Bp, bool fp32) {
  i64 off = 0;
  auto take = [&](i64 cnt) {
    if (fp32) cnt = (cnt + 1) / 2;
    cnt = (cnt + 7) & ~7LL;
    double* p = work ? work + off : nullptr;
    off += cnt;
    return (void*)p;
  };
  for (int l = 0; l < nl; ++l) {
    const i64 nb = (i64)n_nodes[l] * Bp;
    w.xa[l] = take(nb);
    w.xb[l] = take(nb);
    w.res[l] = take(nb);
    w.rhs[l] = take(nb);  // level 0: fp32 copy of the CG residual / FMG residual
    w.bF[l] = l > 0 ? take(nb) : nullptr;
    w.xF[l] = take(nb);
  }
  return off;
}

// ---- what the CG keeps behind the cycle's vectors -------------------------------------------------------------------
// Rows (Bp doubles each) of the scalar block.  PcgScalars is filled from these; rows 7 and 13 stand in where the caller
// passes no stop_rule / err_est; row 8 holds one word (the Gershgorin bound of the coarsest level), row 9 the Bv <= Bp
// entries of maxdiag; row 6 two ints; row 10 is free.
enum ScalarRow {
  ROW_RZ = 0, ROW_ALPHA = 1, ROW_BETA = 2, ROW_BB = 3, ROW_TOL2 = 4, ROW_ACTIVE = 5, ROW_N_ACTIVE = 6,
  ROW_RULE_FALLBACK = 7, ROW_GERSHGORIN = 8, ROW_MAXDIAG = 9,
  ROW_RS = 11, ROW_ENERGY = 12, ROW_EST_FALLBACK = 13, ROW_RR = 14, ROW_GAP = 15,
  ROW_ALPHA_RING = 16,   // kRingSlots rows of step lengths, alpha_j next to direction j's slot
  kScalarRows = 32
};
static_assert(ROW_ALPHA_RING + kRingSlots <= kScalarRows, "the alpha ring must fit the scalar block");

struct PcgWork {
  double* r;      // fp64 residual
  float* rlo;     // `rpair`: the residual's low parts live in the first half of r's region, r itself is unused
  // Search directions.  Fused loop: the iterate is NOT touched inside the loop (that cost 16 of the fused step's 36
  // bytes per node); the directions p_j stay in a ring of slots (10 fp32 / 5 fp64 vectors in these 5 nb doubles) with
  // their step lengths alpha_j, and x += sum_j alpha_j p_j is formed when the ring is full or the solve ends.
  // Unfused loop (small meshes / batches): one fp64 p in the same region, x updated every iteration.
  double* p;
  double* Ap;
  double *partA, *partB;   // kPartBlocks rows each
  double* sc;              // kScalarRows rows
  double* slices;          // kScalarSlices rows: first stage of long partial lists
  double* row(int k, int Bp) const { return sc + (i64)k * Bp; }
};

// n = fine-level nodes.  work == NULL: the size in doubles alone (64 spare at the end), no pointers.
inline i64 pcg_carve(PcgWork& w, double* work, i64 n, int Bp) {
  i64 off = 0;
  auto take = [&](i64 cnt) { double* q = work ? work + off : nullptr; off += cnt; return q; };
  const i64 nb = n * Bp;
  w.r = take(nb);
  w.rlo = (float*)(void*)w.r;
  w.p = take((kRingSlots / 2) * nb);
  w.Ap = take(nb);
  w.partA = take((i64)kPartBlocks * Bp);
  w.partB = take((i64)kPartBlocks * Bp);
  w.sc = take((i64)kScalarRows * Bp);
  w.slices = take((i64)kScalarSlices * Bp);
  return off + 64;
}

// ---- the low half of the residual pair ------------------------------------------------------------------------------
// (PcgScalars::gap has the argument): whole until the batch is near its energy-rule stop, then ONE update that reads the
// pair and stores hi alone (F_RDROP), then hi alone (F_RSINGLE).  Only where that rule is in force.
struct LowHalf {
  enum Form { PAIR = 0, DROP = 1, SINGLE = 2 };   // the values PcgScalars::lo_state takes
  bool may_drop;        // the pair is carried, the caller did not ask to keep it whole, the energy rule is in force
  int form = PAIR;      // form of the next update
  int n_single = 0;     // updates that wrote no low half (status_host[3])
  explicit LowHalf(bool may_drop_) : may_drop(may_drop_) {}

  // After the update that completed iteration `it` (1-based), in the form `form` had.  True: the energy rule is no longer
  // trusted from here on, and with it the argument that let the low half go -- the caller replaces the residual ONCE by
  // b - A x of the iterate (which rewrites the pair); it is kept whole for the rest of the solve.
  bool after_update(int it, int e_max_it) {
    if (form == PAIR) return false;
    ++n_single;
    form = SINGLE;
    if (it < e_max_it) return false;
    form = PAIR;
    may_drop = false;
    return true;
  }
  // After the poll of an iteration that left samples active: `far` of them still need the low half (S_BETA).
  // Sticky: only the replacement above undoes it.
  void after_poll(int far) {
    if (may_drop && form == PAIR && far == 0) form = DROP;
  }
};

}  // namespace diffhe_lattice
