"""The C-ABI library loads and exports every symbol include/diffhe_hip.h declares
(no compute call: this runs without a GPU)."""
import ctypes
import os
import re

import pytest
import torch

from diffhe import _hip

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffhe_hip.h")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(diffhe_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert _declared() == sorted(_hip.SIGNATURES)


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libdiffhe_hip.so not built (run __graft_entry__.build())")
def test_library_exports_every_declared_symbol():
    handle = ctypes.CDLL(_hip.LIB_PATH)
    for name in _declared():
        assert hasattr(handle, name), name
    L = _hip.lib()
    assert L.diffhe_abi_version() == _hip.ABI_VERSION
    assert L.diffhe_status_string(0) == b"ok"
    assert b"batch" in L.diffhe_status_string(-4)
    assert L.diffhe_cg_workspace_doubles(1000, 64) > 4 * 1000 * 64


def test_binding_and_header_agree_on_the_abi_version():
    import re
    m = re.search(r"#define\s+DIFFHE_ABI_VERSION\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == _hip.ABI_VERSION


def test_pcg_option_bits_match_the_header():
    """Every DIFFHE_PCG_* value of the header equals the binding's constant of the same name, and the names are pairwise
    disjoint bit sets (the two-bit cycle count enters as the field its shift places)."""
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+DIFFHE_(PCG_\w+)\s+(\d+)", open(HEADER).read())}
    assert len(defs) == 9, defs
    for name, value in defs.items():
        assert getattr(_hip, name) == value, name
    masks = {n: (3 << v if n == "PCG_FMG_CYCLES_SHIFT" else v) for n, v in defs.items()}
    names = sorted(masks)
    for i, a in enumerate(names):
        assert masks[a] > 0
        for b in names[i + 1:]:
            assert masks[a] & masks[b] == 0, (a, b)
    assert sum(masks.values()) == (1 << 10) - 1   # nine names cover the ten bits of the word, no gap


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the two structs that cross the boundary, as a C compiler sees the header, against the ctypes
    mirrors in diffhe/_hip.py (the header is plain C: gcc compiles it without HIP)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = {"diffhe_mg_level": [f for f, _ in _hip.MgLevel._fields_], "diffhe_amg_level": [f for f, _ in _hip.AmgLevel._fields_]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for struct, names in fields.items():
        lines.append(f'  printf("{struct} %zu", sizeof({struct}));')
        for f in names:
            lines.append(f'  printf(" %zu", offsetof({struct}, {f}));')
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for line, (struct, cls) in zip(out, (("diffhe_mg_level", _hip.MgLevel), ("diffhe_amg_level", _hip.AmgLevel))):
        nums = [int(v) for v in line.split()[1:]]
        assert line.split()[0] == struct
        assert nums[0] == ctypes.sizeof(cls)
        assert nums[1:] == [getattr(cls, f).offset for f, _ in cls._fields_]


# the int-returning entries whose result is a VALUE, not a DIFFHE_OK / DIFFHE_E_* status ...
VALUE_ENTRIES = {"diffhe_abi_version", "diffhe_lattice_blocks", "diffhe_lattice_fused_passes", "diffhe_lattice_recompute_ap",
                 "diffhe_grad_kappa_blocks", "diffhe_robin_sum_blocks", "diffhe_eig_gram_blocks"}
# ... and the statuses bound as plain ints all the same: the caller of diffhe_lattice_bilinear reads DIFFHE_E_TOOBIG as an
# answer, and callers of the profile / traffic accessors have always been free to ignore theirs
UNCHECKED_STATUS = {"diffhe_lattice_bilinear", "diffhe_traffic_account", "diffhe_lattice_pcg_profile",
                    "diffhe_lattice_kernel_profile"}
BY_VALUE = {"int": _hip._I, "long long": _hip._L, "double": _hip._D}
ELEMENT = {ctypes.c_double: "double", ctypes.c_longlong: "long long", _hip.MgLevel: "diffhe_mg_level",
           _hip.AmgLevel: "diffhe_amg_level"}
PTR_CLASSES = [(_hip._PD, torch.float64), (_hip._PF, torch.float32), (_hip._PI, torch.int32), (_hip._PL, torch.int64),
               (_hip._PB, torch.uint8), (_hip._PV, None)]


def _declarations():
    """name -> (return type, [(type, is pointer)]) of every diffhe_* function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"typedef struct.*?\}\s*\w+;", "", text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][A-Za-z_ ]*?\**)\s*\b(diffhe_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = []
        for a in ([] if args.strip() == "void" else args.split(",")):
            m = re.match(r"(.+?)\s*(\*?)\s*\w+$", re.sub(r"\bconst\b", "", a).strip())
            params.append((m.group(1).strip(), bool(m.group(2))))
        out[name] = (" ".join(ret.split()), params)
    return out


def test_every_signature_matches_the_header():
    """Arity, every argument type -- int / long long / double by value, pointers by the element type they point to -- and
    the return type of all 64 entries, binding against header."""
    decls = _declarations()
    assert sorted(decls) == sorted(_hip.SIGNATURES) and len(decls) == 64
    for name, (ret, params) in decls.items():
        res, argtypes = _hip.SIGNATURES[name]
        assert len(argtypes) == len(params), name
        for i, ((ctype, is_ptr), t) in enumerate(zip(params, argtypes)):
            if not is_ptr:
                assert t is BY_VALUE[ctype], (name, i, ctype, t)
            elif isinstance(t, type) and issubclass(t, _hip._Ptr):
                assert t.elem == ctype, (name, i, ctype, t)
            else:       # a ctypes POINTER(...): level descriptors and host out-parameters
                assert ELEMENT[t._type_] == ctype, (name, i, ctype, t)
        if ret == "int":
            plain = name in VALUE_ENTRIES or name in UNCHECKED_STATUS
            assert res is (_hip._I if plain else _hip._S), name
        else:
            assert res is {"long long": _hip._L, "const char*": ctypes.c_char_p}[ret], name
    assert VALUE_ENTRIES | UNCHECKED_STATUS <= set(decls)


@pytest.mark.parametrize("cls,dtype", PTR_CLASSES, ids=[c.elem for c, _ in PTR_CLASSES])
def test_pointer_argtypes_convert_and_refuse(cls, dtype):
    assert cls.from_param(None) is None                                         # NULL
    t = torch.zeros(6, dtype=dtype or torch.float16)
    assert cls.from_param(t).value == t.data_ptr()
    assert cls.from_param(t[1::2]).value == t[1::2].data_ptr()                  # strided views stay legal
    passed = ctypes.c_void_p(123)
    assert cls.from_param(passed) is passed and cls.from_param(123).value == 123
    assert cls.from_param(1 << 40).value == 1 << 40                             # an address, not a C int
    with pytest.raises(TypeError):
        cls.from_param("not a pointer")
    others = [d for _, d in PTR_CLASSES if d is not None and d is not dtype] + [torch.float16, torch.bool]
    for other in others:
        wrong = torch.zeros(2, dtype=other)
        if dtype is None:                                                       # void*: any dtype
            assert cls.from_param(wrong).value == wrong.data_ptr()
        else:
            with pytest.raises(TypeError):
                cls.from_param(wrong)


def test_wrong_dtype_is_an_argument_error_before_the_call():
    """Through a ctypes function: the refusal of `from_param` surfaces as ctypes.ArgumentError and the callee never runs."""
    calls = []
    proto = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
    fn = proto(lambda a, b: calls.append((a, b)) or 0)
    fn.argtypes = [_hip._PI, _hip._PD]
    idx, val = torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.float64)
    assert fn(idx, val) == 0 and calls == [(idx.data_ptr(), val.data_ptr())]
    with pytest.raises(ctypes.ArgumentError):
        fn(idx.long(), val)                     # int64 where int* is declared
    with pytest.raises(ctypes.ArgumentError):
        fn(idx, val.float())                    # float32 where double* is declared
    assert len(calls) == 1


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libdiffhe_hip.so not built (run __graft_entry__.build())")
def test_a_failed_status_raises_under_the_entry_name():
    """diffhe_to_node_major refuses NULL arrays before it touches the HIP runtime: the bound function raises by itself,
    with the entry's name and the status string; entries bound as plain ints hand their value back."""
    L = _hip.lib()
    with pytest.raises(_hip.HipExtensionError) as err:
        L.diffhe_to_node_major(None, 0, None, None, 4, 2, 2, None)
    assert "diffhe_to_node_major" in str(err.value) and L.diffhe_status_string(-1).decode() in str(err.value)
    assert L.diffhe_to_node_major.restype is _hip._I and L.diffhe_abi_version.errcheck is not L.diffhe_to_node_major.errcheck
    with pytest.raises(_hip.HipExtensionError, match="some name failed"):
        _hip.check(-1, "some name")             # the explicit form stays for callers that read a status themselves
    _hip.check(0, "some name")


# ------------------------------------------------------------------------------------------------
# GPU: the binding in front of real entries (every failure below is raised on the host, before any launch)
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wrong_dtype_source_is_refused_before_any_launch():
    from diffhe import FEMesh
    from diffhe.plan import get_plan, padded_batch
    from diffhe.solver import _Engine
    mesh = FEMesh.rectangle(4, 4)
    plan = get_plan(mesh, torch.device("cuda:0"))
    eng = _Engine(plan, 1e-12, 100, 1, "gather")
    n, B = mesh.n_nodes, 2
    Bp = padded_batch(B)
    src = torch.arange(B * n, dtype=torch.float64, device="cuda:0").reshape(B, n)
    assert torch.equal(eng.to_node_major(src, B, Bp, n)[:, :B], src.t())
    L = _hip.lib()
    before = ctypes.c_longlong()
    L.diffhe_traffic_account(0, ctypes.byref(ctypes.c_double()), ctypes.byref(before))
    with pytest.raises(ctypes.ArgumentError):
        eng.to_node_major(src.long(), B, Bp, n)
    after = ctypes.c_longlong()
    L.diffhe_traffic_account(0, ctypes.byref(ctypes.c_double()), ctypes.byref(after))
    assert after.value == before.value          # the library counted no launch
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("mg", [None, dict(dense_coarse=0)], ids=["direct", "mgpcg"])
def test_adjoint_info_comes_from_the_adjoint_solve(mg, monkeypatch):
    """Forward and backward each read the record their own lattice solve returned: nothing travels through the engine.
    mg = None is the dense direct product of so small a mesh (no rule fires: {}), dense_coarse = 0 makes the PCG iterate."""
    from diffhe import DifferentiableFESolver, FEMesh
    from diffhe.solver import _Engine
    records = []
    solve = _Engine.lattice_pcg

    def spy(self, *args, **kw):
        records.append(solve(self, *args, **kw))
        return records[-1]
    monkeypatch.setattr(_Engine, "lattice_pcg", spy)
    mesh, B = FEMesh.rectangle(8, 8), 3
    kappa = torch.tensor([0.7, 1.0, 1.9], dtype=torch.float64, device="cuda:0", requires_grad=True)
    solver = DifferentiableFESolver(mesh, kappa, device="cuda:0", mg=mg)
    u = solver(torch.ones(B, mesh.n_nodes, dtype=torch.float64, device="cuda:0"))
    fwd_info = solver.last_info
    assert fwd_info.adj_stop_rules is None and len(records) == 1
    (u ** 2).sum().backward()
    info = solver.last_info
    fwd, adj = records
    assert adj.est is not fwd.est and adj.rule is not fwd.rule and adj.x is not fwd.x
    assert info.adj_stop_rules is not None and info.adj_stop_rules is not info.stop_rules
    assert info.err_est == float(fwd.est[:B].max()) and info.adj_err_est == float(adj.est[:B].max())
    assert info.adj_iterations == adj.iterations and info.iterations == fwd.iterations and info.flags == fwd.flags
    if mg is None:
        assert info.path == "lattice-direct" and info.stop_rules == {} and info.adj_stop_rules == {}
    else:
        assert info.path == "lattice-mgpcg"
        for rules, rec in ((info.stop_rules, fwd), (info.adj_stop_rules, adj)):
            counts = torch.bincount(rec.rule[:B].long(), minlength=3).tolist()
            assert rules == {"cap": counts[0], "residual": counts[1], "energy": counts[2]} and sum(rules.values()) == B
    assert kappa.grad is not None and bool(torch.isfinite(kappa.grad).all())
