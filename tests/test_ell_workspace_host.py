"""The workspace layout of the general path's two PCG solves (csrc/ell.h: amg_carve / pcg_carve) on the HOST: a stand-alone
C++ program, built with the host compiler from the very header the solver units include, run once.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "difffe-physics-lab_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include "ell.h"

using namespace diffhe_ell;
static int bad = 0;
static void expect(bool ok, const char* what, long long n, int Bp, int nl) {
  if (!ok && bad++ < 20) std::printf("FAIL %s: n=%lld Bp=%d levels=%d\n", what, n, Bp, nl);
}

int main() {
  const int ns[] = {5, 4099, 1050625}, Bps[] = {1, 8, 64, 192}, nls[] = {1, 2, 4};
  double* const base = (double*)(uintptr_t)4096;   // never dereferenced
  int checked = 0;
  for (int n : ns) for (int Bp : Bps) for (int nl : nls) {
    // the x of node_grid(n, Bp), restated: blocks of 4 waves, 64 / min(Bp, 64) nodes per wave, at most 2048
    const int npw = 64 / (Bp < 64 ? Bp : 64);
    long long nblk = ((long long)n + 4 * npw - 1) / (4 * npw);
    if (nblk > 2048) nblk = 2048;
    const long long NB = (long long)n * Bp, PB = nblk * Bp, tail = (16 + 2 * 16) * (long long)Bp + 64;

    PcgWork w;
    expect(pcg_carve(w, nullptr, n, Bp, true, 3) == 4 * NB + 3 * PB + tail, "Jacobi size", n, Bp, nl);
    expect(!w.r && !w.z && !w.p && !w.Ap && !w.part[0] && !w.sc && !w.slices, "size-only carve hands out pointers", n, Bp, nl);
    expect(pcg_carve(w, base, n, Bp, true, 3) == 4 * NB + 3 * PB + tail, "Jacobi size (carved)", n, Bp, nl);
    expect(w.r == base && w.z == base + NB && w.p == base + 2 * NB && w.Ap == base + 3 * NB, "Jacobi vectors", n, Bp, nl);
    expect(w.part[0] == base + 4 * NB && w.part[1] == w.part[0] + PB && w.part[2] == w.part[1] + PB && !w.part[3],
           "Jacobi partial lists", n, Bp, nl);
    expect(w.sc == w.part[2] + PB && w.slices == w.sc + 16LL * Bp, "Jacobi scalar block / slice table", n, Bp, nl);

    AmgHier H;
    H.nl = nl; H.Bp = Bp;
    long long hier = 0, n_l = n;
    for (int l = 0; l < nl; ++l, n_l = n_l / 9 + 1) {
      H.lev[l].n = (int)n_l;
      hier += 4 * ((n_l * Bp + 7) & ~7LL);
    }
    expect(amg_carve(H, nullptr) == hier, "hierarchy size", n, Bp, nl);
    expect(amg_carve(H, base) == hier, "hierarchy size (carved)", n, Bp, nl);
    long long off = 0;
    for (int l = 0; l < nl; ++l) {
      const long long step = ((long long)H.lev[l].n * Bp + 7) & ~7LL;
      expect(H.xa[l] == base + off && H.xb[l] == base + off + step && H.res[l] == base + off + 2 * step &&
                 H.rhs[l] == base + off + 3 * step, "hierarchy vectors", n, Bp, l);
      off += 4 * step;
    }
    double* const t = base + hier;
    expect(hier + pcg_carve(w, t, n, Bp, false, 4) == hier + 3 * NB + 4 * PB + tail, "AMG size", n, Bp, nl);
    expect(w.r == t && !w.z && w.p == t + NB && w.Ap == t + 2 * NB, "AMG vectors", n, Bp, nl);
    expect(w.part[0] == t + 3 * NB && w.part[1] == w.part[0] + PB && w.part[2] == w.part[1] + PB && w.part[3] == w.part[2] + PB,
           "AMG partial lists", n, Bp, nl);
    expect(w.sc == w.part[3] + PB && w.slices == w.sc + 16LL * Bp, "AMG scalar block / slice table", n, Bp, nl);
    ++checked;
  }
  std::printf("checked %d bad %d\n", checked, bad);
  return bad ? 1 : 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_carves_return_the_closed_form_sizes_and_offsets(tmp_path):
    """For n in {5, 4 099, 1 050 625}, Bp in {1, 8, 64, 192} and hierarchies of 1, 2 and 4 levels: the Jacobi solve's
    workspace is 4 n Bp + 3 nblk Bp + (16 + 2 * 16) Bp + 64 doubles, the multigrid solve's the hierarchy (four vectors per
    level, each rounded up to 8 doubles) + 3 n Bp + 4 nblk Bp + (16 + 2 * 16) Bp + 64, nblk the x of node_grid(n, Bp); r,
    [z,] p, A p, the partial lists, the scalar block and the slice table follow one another without gaps in that order;
    a carve without a base returns the same size and no pointers."""
    cxx = _compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++ / clang++) on PATH")
    src = tmp_path / "ell_workspace_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "ell_workspace_host"
    base = [cxx, "-std=c++17", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    # the sanitizers belong on this stand-alone host program only; a toolchain without their runtimes builds it plain
    built = subprocess.run(base[:3] + ["-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"] + base[3:],
                           capture_output=True, text=True)
    if built.returncode != 0:
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1].split() == ["checked", "36", "bad", "0"]
