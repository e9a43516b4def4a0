"""The workspace layout of the lattice solve (csrc/lattice_layout.h: cycle_carve / pcg_carve, the rows of the scalar block)
and the low-half policy of its residual pair (LowHalf) on the HOST: a stand-alone C++ program, built with the host compiler
from the very header the solver units include (through lattice.h), run once.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "difffe-physics-lab_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "lattice_layout.h"

using namespace diffhe_lattice;
static int bad = 0;
static void expect(bool ok, const char* what, long long n, int Bp, int nl, int fp32) {
  if (!ok && bad++ < 20) std::printf("FAIL %s: n=%lld Bp=%d levels=%d fp32=%d\n", what, n, Bp, nl, fp32);
}

// Runs the loop's two transitions as the driver does: update (in the form the policy names), ++it, after_update, poll.
// far[k] = the "far" count of poll k (the last entry repeats).  Returns the forms of the updates as a string of P / D / S
// and the iterations at which a refresh was asked for.
struct Trace { std::string forms; std::vector<int> refresh; int n_single; };
static Trace run(bool may_drop, const std::vector<int>& far, int iters, int e_max_it) {
  LowHalf lo(may_drop);
  Trace t;
  for (int it = 0; it < iters;) {
    t.forms += "PDS"[lo.form];
    ++it;
    if (lo.after_update(it, e_max_it)) t.refresh.push_back(it);
    lo.after_poll(far[(size_t)(it - 1) < far.size() ? it - 1 : far.size() - 1]);
  }
  t.n_single = lo.n_single;
  return t;
}
static void expect_trace(const Trace& t, const char* forms, std::vector<int> refresh, int n_single, const char* what) {
  if ((t.forms != forms || t.refresh != refresh || t.n_single != n_single) && bad++ < 20)
    std::printf("FAIL low half, %s: forms %s (want %s) n_single %d (want %d) refreshes %zu\n", what, t.forms.c_str(), forms,
                t.n_single, n_single, t.refresh.size());
}

int main() {
  const long long n0s[] = {5, 8385, 1050625};
  const int Bps[] = {1, 8, 64, 192}, nls[] = {1, 2, 5};
  double* const base = (double*)(uintptr_t)4096;   // never dereferenced
  int checked = 0;
  for (long long n0 : n0s) for (int Bp : Bps) for (int nl : nls) for (int fp32 = 0; fp32 < 2; ++fp32) {
    int nodes[kMaxLevels];
    long long n_l = n0;
    for (int l = 0; l < nl; ++l, n_l = n_l / 4 + 1) nodes[l] = (int)n_l;
    // the cycle: 5 (level 0) or 6 vectors per level, each rounded up to 8 doubles
    auto vec = [&](int l) { const long long e = (long long)nodes[l] * Bp; return ((fp32 ? (e + 1) / 2 : e) + 7) & ~7LL; };
    long long want = 0;
    for (int l = 0; l < nl; ++l) want += (l ? 6 : 5) * vec(l);
    CycleWork c;
    expect(cycle_carve(c, nullptr, nodes, nl, Bp, fp32 != 0) == want, "cycle size", n0, Bp, nl, fp32);
    bool none = true;
    for (int l = 0; l < nl; ++l) none = none && !c.xa[l] && !c.xb[l] && !c.res[l] && !c.rhs[l] && !c.bF[l] && !c.xF[l];
    expect(none, "size-only cycle carve hands out pointers", n0, Bp, nl, fp32);
    expect(cycle_carve(c, base, nodes, nl, Bp, fp32 != 0) == want, "cycle size (carved)", n0, Bp, nl, fp32);
    long long off = 0;
    for (int l = 0; l < nl; ++l) {
      const long long s = vec(l);
      bool ok = c.xa[l] == base + off && c.xb[l] == base + off + s && c.res[l] == base + off + 2 * s &&
                c.rhs[l] == base + off + 3 * s;
      if (l == 0) ok = ok && !c.bF[l] && c.xF[l] == base + off + 4 * s;
      else ok = ok && c.bF[l] == base + off + 4 * s && c.xF[l] == base + off + 5 * s;
      expect(ok, "cycle vectors", n0, Bp, l, fp32);
      off += (l ? 6 : 5) * s;
    }
    // the CG's part, behind the cycle's: the closed form diffhe_lattice_pcg_workspace_doubles used to state
    const long long NB = n0 * Bp, PB = (long long)kPartBlocks * Bp;
    const long long size = (2 + kRingSlots / 2) * NB + 2 * PB + (32LL + kScalarSlices) * Bp + 64;
    PcgWork w;
    expect(pcg_carve(w, nullptr, n0, Bp) == size, "pcg size", n0, Bp, nl, fp32);
    expect(!w.r && !w.rlo && !w.p && !w.Ap && !w.partA && !w.partB && !w.sc && !w.slices, "size-only pcg carve hands out pointers",
           n0, Bp, nl, fp32);
    double* const t = base + want;
    expect(pcg_carve(w, t, n0, Bp) == size, "pcg size (carved)", n0, Bp, nl, fp32);
    expect(w.r == t && (void*)w.rlo == (void*)t && w.p == t + NB && w.Ap == w.p + (kRingSlots / 2) * NB, "pcg vectors", n0, Bp, nl,
           fp32);
    expect(w.partA == w.Ap + NB && w.partB == w.partA + PB && w.sc == w.partB + PB, "pcg partial lists", n0, Bp, nl, fp32);
    expect(w.slices == w.sc + 32LL * Bp && w.slices + (long long)kScalarSlices * Bp + 64 == t + size, "slice table / spare", n0,
           Bp, nl, fp32);
    expect(w.row(ROW_ENERGY, Bp) == w.sc + 12LL * Bp && w.row(kScalarRows, Bp) == w.slices, "scalar rows", n0, Bp, nl, fp32);
    ++checked;
  }

  // the rows of the scalar block, at the offsets the solver has always used
  const int rows[] = {ROW_RZ, ROW_ALPHA, ROW_BETA, ROW_BB, ROW_TOL2, ROW_ACTIVE, ROW_N_ACTIVE, ROW_RULE_FALLBACK, ROW_GERSHGORIN,
                      ROW_MAXDIAG, ROW_RS, ROW_ENERGY, ROW_EST_FALLBACK, ROW_RR, ROW_GAP};
  const int at[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15};
  const int nrows = (int)(sizeof(rows) / sizeof(rows[0]));
  for (int i = 0; i < nrows; ++i) {
    if (rows[i] != at[i] && bad++ < 20) std::printf("FAIL row %d sits at %d, not %d\n", i, rows[i], at[i]);
    if ((rows[i] < 0 || rows[i] >= 32) && bad++ < 20) std::printf("FAIL row %d outside the block\n", rows[i]);
    for (int j = 0; j < i; ++j)
      if (rows[i] == rows[j] && bad++ < 20) std::printf("FAIL rows %d and %d coincide\n", i, j);
    if (rows[i] >= ROW_ALPHA_RING && rows[i] < ROW_ALPHA_RING + kRingSlots && bad++ < 20)
      std::printf("FAIL row %d lies in the alpha ring\n", rows[i]);
  }
  if ((ROW_ALPHA_RING != 16 || ROW_ALPHA_RING + kRingSlots > 32 || kScalarRows != 32) && bad++ < 20)
    std::printf("FAIL alpha ring %d .. %d of %d rows\n", (int)ROW_ALPHA_RING, ROW_ALPHA_RING + kRingSlots - 1, (int)kScalarRows);

  // the low half of the residual pair, e_max_it = 10
  expect_trace(run(true, {3, 1, 0, 0, 0}, 6, 10), "PPPDSS", {}, 3, "far 3 1 0 0 0");
  expect_trace(run(true, {0}, 6, 10), "PDSSSS", {}, 5, "far 0 from the first poll");
  // far reaches 0 at poll 9: the drop is first used in the update that makes it == 10 -> refreshed in that very iteration
  expect_trace(run(true, {5, 5, 5, 5, 5, 5, 5, 5, 0}, 16, 10), "PPPPPPPPPDPPPPPP", {10}, 1, "drop first used at it == 10");
  // far reaches 0 at poll 3: dropped in update 4, still running at 10
  expect_trace(run(true, {5, 5, 0}, 16, 10), "PPPDSSSSSSPPPPPP", {10}, 7, "drop at 4, running at 10");
  // keep_lo / tol_energy == 0 / no pair: each makes may_drop false
  for (int k = 0; k < 3; ++k) expect_trace(run(false, {0}, 14, 10), "PPPPPPPPPPPPPP", {}, 0, "may_drop false");

  std::printf("checked %d bad %d\n", checked, bad);
  return bad ? 1 : 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_carves_scalar_rows_and_low_half_policy(tmp_path):
    """For fine levels of 5, 8 385 (129 x 65) and 1 050 625 nodes, hierarchies of 1, 2 and 5 levels, Bp in {1, 8, 64, 192} and
    both storages: the cycle carve returns 5 (level 0) or 6 vectors per level of ((fp32 ? (n_l Bp + 1) / 2 : n_l Bp) + 7) & ~7
    doubles, in the order xa, xb, res, rhs, [bF,] xF without gaps; pcg_carve returns (2 + kRingSlots / 2) n Bp +
    2 kPartBlocks Bp + (32 + kScalarSlices) Bp + 64 with r (= rlo), the ring, A p, the two partial lists, the scalar block and
    the slice table at those offsets; a carve without a base returns the same size and no pointers.  The named rows of the
    scalar block are distinct, below 32, at their historical offsets and outside the alpha ring (16 .. 25).  LowHalf gives
    the sequences of update forms, single-update counts and refresh requests of the driver's loop."""
    cxx = _compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++ / clang++) on PATH")
    src = tmp_path / "lattice_workspace_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "lattice_workspace_host"
    base = [cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)]
    # the sanitizers belong on this stand-alone host program only; a toolchain without their runtimes builds it plain
    built = subprocess.run(base[:3] + ["-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"] + base[3:],
                           capture_output=True, text=True)
    if built.returncode != 0:
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1].split() == ["checked", "72", "bad", "0"]
