"""The fp32-pair arithmetic of the lattice CG residual (csrc/common.h: split / join) on the HOST: a stand-alone C++
program, built with the host compiler from the very header the kernels include, run once.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

from diffhe import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "difffe-physics-lab_amd", "csrc")

PROGRAM = r"""
#include <cfenv>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include "common.h"

static int bad = 0;
static void fail(const char* what, double R, float hi, float lo) {
  if (bad++ < 10) std::printf("FAIL %s: R=%a hi=%a lo=%a\n", what, R, (double)hi, (double)lo);
}

int main() {
  std::mt19937_64 gen(20240611);
  std::uniform_real_distribution<double> mant(1.0, 2.0);
  std::uniform_int_distribution<int> expo(-60, 0);   // |R| in [2^-60, 2)
  const double bound = std::ldexp(1.0, -47);
  double worst = 0.0;
  long normal_lo = 0;
  const int N = 1000000;
  for (int i = 0; i < N; ++i) {
    double R = std::ldexp(mant(gen), expo(gen));
    if (gen() & 1) R = -R;
    float hi, lo;
    diffhe::split(R, hi, lo);
    if (hi != (float)R) fail("hi != (float)R", R, hi, lo);
    const double back = diffhe::join(hi, lo);
    if (std::isnan(back)) fail("NaN", R, hi, lo);
    if (std::fpclassify(lo) == FP_NORMAL) {
      ++normal_lo;
      const double rel = std::fabs(back - R) / std::fabs(R);
      if (rel > worst) worst = rel;
      if (!(std::fabs(back - R) <= bound * std::fabs(R))) fail("|join(split(R)) - R| > 2^-47 |R|", R, hi, lo);
    }
  }
  // zeros, both signs, a remainder below the fp32 range (lo subnormal or flushed), hi itself subnormal, and values a
  // float holds exactly (lo == 0): nothing traps (the run is under -fsanitize=undefined where available, and with the
  // invalid / divide-by-zero / overflow exceptions checked below), nothing turns into NaN, the sign of hi is R's
  const double specials[] = {0.0, -0.0, 1.0, -1.0, 0.5, 1.5, std::ldexp(1.0, -60), -std::ldexp(1.0, -60),
                             std::ldexp(1.0 + std::ldexp(1.0, -30), -126), -std::ldexp(1.0 + std::ldexp(1.0, -30), -126),
                             std::ldexp(1.0 + std::ldexp(1.0, -40), -110), 1e-40, -1e-40, 1e-46, -1e-46, DBL_MIN, -DBL_MIN,
                             std::ldexp(1.0 + std::ldexp(1.0, -52), -100), 1.9999999999999998, -1.9999999999999998};
  std::feclearexcept(FE_ALL_EXCEPT);
  for (double R : specials) {
    float hi, lo;
    diffhe::split(R, hi, lo);
    const double back = diffhe::join(hi, lo);
    if (hi != (float)R) fail("special: hi != (float)R", R, hi, lo);
    if (std::isnan(hi) || std::isnan(lo) || std::isnan(back)) fail("special: NaN", R, hi, lo);
    if (std::signbit(hi) != std::signbit(R)) fail("special: sign of hi", R, hi, lo);
    if (std::fabs(back - R) > std::fabs(R)) fail("special: join further from R than 0 is", R, hi, lo);
    if (std::fpclassify(lo) == FP_NORMAL && !(std::fabs(back - R) <= bound * std::fabs(R))) fail("special: bound", R, hi, lo);
  }
  if (std::fetestexcept(FE_INVALID | FE_DIVBYZERO | FE_OVERFLOW)) { std::printf("FAIL floating-point exception raised\n"); ++bad; }
  std::printf("checked %d normal_lo %ld worst_rel %.3e bad %d\n", N, normal_lo, worst, bad);
  return bad ? 1 : 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_split_join_over_a_million_doubles(tmp_path):
    """hi == (float)R exactly (the V-cycle's input is formed as before), |join(split(R)) - R| <= 2^-47 |R| wherever lo is a
    normal float, over 10^6 random doubles of magnitude 2^-60 .. 2 and both signs; zeros, signed values and remainders
    that underflow neither trap nor produce NaN."""
    cxx = _compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++ / clang++) on PATH")
    src = tmp_path / "pair_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "pair_host"
    # -ffp-contract=off: the arithmetic under test is two conversions and a subtraction, nothing to contract -- but the
    # checks around it must not be fused differently from how they read
    base = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)]
    # the sanitizers belong on this stand-alone host program only; a toolchain without their runtimes builds it plain
    built = subprocess.run(base[:3] + ["-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"] + base[3:],
                           capture_output=True, text=True)
    if built.returncode != 0:
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.strip().splitlines()[-1].split()
    assert last[0] == "checked" and int(last[1]) == 1000000 and int(last[-1]) == 0
    # the bound is not vacuous: nearly every draw has a normal lo (lo == 0 or subnormal needs 24+ zero bits / |R| < 2^-78)
    assert int(last[3]) > 990000


def test_the_flag_that_keeps_the_fp64_residual_is_one_bit_of_its_own():
    """DIFFHE_PCG_RESID_FP64 of the public header equals the binding's constant and shares no bit with another option."""
    header = open(os.path.join(ROOT, "include", "diffhe_hip.h")).read()
    m = re.search(r"#define\s+DIFFHE_PCG_RESID_FP64\s+\(1 << (\d+)\)", header)
    assert m and 1 << int(m.group(1)) == _hip.PCG_RESID_FP64
    others = {n: int(v) for n, v in re.findall(r"#define\s+DIFFHE_(PCG_\w+)\s+(\d+)", header)}
    assert "PCG_RESID_FP64" not in others and len(others) >= 9
    for name, value in others.items():
        mask = 3 << value if name == "PCG_FMG_CYCLES_SHIFT" else value
        assert mask & _hip.PCG_RESID_FP64 == 0, name
