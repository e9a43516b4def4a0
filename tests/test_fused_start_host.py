"""DIFFHE_PCG_SPLIT_START on the host: the bit of the public header is the binding's, shares nothing with another option,
is known to the solver's flag check and travels from mg={'split_start': 1} into the flags word.  No GPU."""
import os
import re

from diffhe import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "diffhe_hip.h")).read()


def test_the_split_start_flag_is_one_bit_of_its_own():
    header = _header()
    m = re.search(r"#define\s+DIFFHE_PCG_SPLIT_START\s+\(1 << (\d+)\)", header)
    assert m and int(m.group(1)) == 16 and 1 << 16 == _hip.PCG_SPLIT_START
    plain = {n: int(v) for n, v in re.findall(r"#define\s+DIFFHE_(PCG_\w+)\s+(\d+)", header)}
    shifted = {n: 1 << int(v) for n, v in re.findall(r"#define\s+DIFFHE_(PCG_\w+)\s+\(1 << (\d+)\)", header)}
    trust = int(re.search(r"#define\s+DIFFHE_PCG_TRUST_ITS_SHIFT\s+\((\d+)\)", header).group(1))
    assert trust == _hip.PCG_TRUST_ITS_SHIFT and len(plain) >= 9 and "PCG_SPLIT_START" in shifted
    for name, value in plain.items():
        mask = 3 << value if name == "PCG_FMG_CYCLES_SHIFT" else value
        assert mask & _hip.PCG_SPLIT_START == 0, name
    for name, value in shifted.items():
        assert name == "PCG_SPLIT_START" or value & _hip.PCG_SPLIT_START == 0, name
    assert (15 << trust) & _hip.PCG_SPLIT_START == 0


def test_the_lattice_units_know_the_bit():
    """csrc/lattice.h asserts at compile time that the bit is disjoint from every other option; the driver decodes it."""
    csrc = os.path.join(ROOT, "difffe-physics-lab_amd", "csrc")
    assert re.search(r"static_assert\(\(DIFFHE_PCG_SPLIT_START &", open(os.path.join(csrc, "lattice.h")).read())
    assert "flags & DIFFHE_PCG_SPLIT_START" in open(os.path.join(csrc, "lattice_pcg.hip")).read()


def test_split_start_round_trips_through_the_solver_options():
    """mg['split_start'] sets exactly that bit of the word lattice_pcg hands to the library; the default leaves it clear."""
    src = open(os.path.join(ROOT, "difffe-physics-lab_amd", "diffhe", "solver.py")).read()
    m = re.search(r'\(_hip\.PCG_SPLIT_START if int\(mg\.get\("split_start", (\d)\)\) else 0\)', src)
    assert m and m.group(1) == "0"
    flags_expr = src[src.index("flags = (int(mg.get(\"fp32\", 0))"):src.index("# a multigrid-preconditioned CG that has not")]
    assert flags_expr.count("PCG_SPLIT_START") == 1     # OR-ed into the word once, next to the other A/B bits
