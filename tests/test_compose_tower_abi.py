"""Tower-typed expressions and the compute plan at the boundary (CPU only): include/binius_amd.h declares bn_expr_compile_tower and
bn_compute_composite_counters, libbinius_amd.so exports them, the ctypes binding lists and exposes them, the Rust shim declares them and
the constants agree; include/binius_amd_host.h declares bnh_witness_compute and bnh_witness_compute_scratch_elems, libbinius_amd_host.so
exports them and binius_amd._host binds them in WitnessCompute, whose kinds are a strict superset of WitnessBuild's; the scratch formula
matches a hand count for a small plan and answers 0 for every rejected one.  The expression compiler and the packed-subfield arithmetic
of the kernel run here too, on the CPU: tests/cpp/compose_tower_check (binius_amd/csrc/compose_tower.hpp against value-by-value B128)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_expr_compile_tower": "expr_compile_tower", "bn_compute_composite_counters": "compute_composite_counters"}
HOST_SYMBOLS = ("bnh_witness_compute", "bnh_witness_compute_scratch_elems")
CAPS = {"BN_TOWER_EXPR_MAX_STEPS": 1024, "BN_TOWER_EXPR_MAX_INPUTS": 256, "BN_TOWER_EXPR_MAX_LIVE": 16}
COUNTERS = ("CALLS", "LAUNCHES", "BITWISE", "VALUES")
SELECT = [("var", 0), ("var", 1), ("var", 2), ("add", 0, 1), ("mul", 2, 3), ("add", 0, 4)]  # a + s (a + b), mul.rs:466-489


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g

    g.build()
    import binius_amd._ffi as f

    return f


def _decls(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_both_sides_declare_export_and_bind(ffi, symbol):
    assert re.search(r"\bint\s+%s\s*\(" % symbol, _decls("binius_amd.h"))
    assert hasattr(ffi.lib(), symbol)
    assert symbol in ffi.ABI_SYMBOLS
    assert callable(getattr(ffi.Context, DEVICE_SYMBOLS[symbol], None))
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % symbol, src)
    lib_rs = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "lib.rs")).read()
    assert "pub fn compile_expr_tower" in lib_rs and "ffi::bn_expr_compile_tower" in lib_rs
    layer = open(os.path.join(ROOT, "binius_amd", "host", "compute_layer.hpp")).read()
    assert "compile_expr_tower" in layer and "bn_expr_compile_tower(" in layer


def test_the_new_entry_points_take_no_device_memory(ffi):
    """(tests/test_gpu_deferred_visibility.py lists every entry point that does; these two must not be among them)"""
    h = _decls("binius_amd.h")
    for symbol in DEVICE_SYMBOLS:
        args = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % symbol, h, flags=re.S).group(1)
        assert not re.search(r"\bd_\w+", args) and "void" not in args, args


def test_constants_agree(ffi):
    h = open(os.path.join(ROOT, "include", "binius_amd.h")).read()
    rust = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    for name, val in CAPS.items():
        assert re.search(r"#define %s %d\b" % (name, val), h) and getattr(ffi, name) == val
        assert re.search(r"pub const %s: usize = %d;" % (name, val), rust)
    for i, name in enumerate(COUNTERS):
        assert re.search(r"\bBN_CC_TOWER_%s\s*=\s*%d\b" % (name, i), h) and getattr(ffi, "BN_CC_TOWER_" + name) == i
        assert re.search(r"pub const BN_CC_TOWER_%s: usize = %d;" % (name, i), rust)
    assert re.search(r"\bBN_CC_N\s*=\s*4\b", h) and ffi.BN_CC_N == 4 and re.search(r"pub const BN_CC_N: usize = 4;", rust)
    # the slots are the kernel's LDS: 16 slots x 16 B x 256 threads = 64 KiB
    assert CAPS["BN_TOWER_EXPR_MAX_LIVE"] * 16 * 256 == 64 << 10


@pytest.mark.parametrize("symbol", HOST_SYMBOLS)
def test_host_library_exports_and_python_binds_the_plan(ffi, symbol):
    import binius_amd._host as h

    ffi.lib()
    assert re.search(r"\b(int|uint64_t)\s+%s\s*\(" % symbol, _decls("binius_amd_host.h"))
    fn = getattr(h.host_lib(), symbol)
    hm = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % symbol, _decls("binius_amd_host.h"), flags=re.S)
    assert len(fn.argtypes) == len([a for a in hm.group(1).split(",") if a.strip()])
    # bnh_witness_build's parameter list, followed by the expressions
    bm = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % symbol.replace("compute", "build"), _decls("binius_amd_host.h"), flags=re.S)
    tail = "const bn_step *steps, const uint32_t *step_off, const uint32_t *expr_inputs, const uint32_t *expr_input_off, uint32_t n_exprs"
    assert " ".join(hm.group(1).split()) == " ".join(bm.group(1).split()) + ", " + tail


def test_compute_kinds_are_a_strict_superset_of_the_build_plans(ffi):
    import binius_amd._host as h

    old, new = h.WitnessBuild.KINDS, h.WitnessCompute.KINDS
    assert set(old.items()) < set(new.items())
    assert {k: v for k, v in new.items() if k not in old} == {"computed": 13}
    assert re.search(r"\bBNH_WIT_COMPUTED\s*=\s*13\b", _decls("binius_amd_host.h"))


def test_scratch_formula_on_a_small_plan(ffi):
    import binius_amd._host as h

    class Col:
        def __init__(self, ptr):
            self.ptr = ptr

    a = Col(0x1000)
    W = h.WitnessCompute
    bits = [("given", a, 0, 10)] * 32                                                # 0 .. 31: B1, 2^10 bits = 8 elements each (given: no scratch)
    plan = bits + [
        ("lincomb", [(i, 1 << i) for i in range(32)], 0, 10),                        # 32: pack_fp at B32: 2^10 x 32 bits = 256 elements
        ("computed", SELECT, [0, 1, 2], 10, 0),                                      # 33: a B1 composite: 8 elements
        ("given", a, 0, 4), ("given", a, 3, 3),                                      # 34, 35: 16 bits, 8 bytes
        ("computed", [("var", 0), ("var", 0), ("mul", 0, 1)], [34], 4, 0),           # 36: 16 bits, below one element: one element, host work
    ]
    assert W.scratch_elems(plan) == 256 + 8 + 1
    assert W.scratch_elems(plan[:33]) == 256 and W.scratch_elems(plan[:32]) == 0
    assert h.WitnessBuild.scratch_elems(plan[:33]) == 0 and h.WitnessBuild.scratch_elems(bits[:3] + [(13, 0, 10, 0)]) == 0  # the build plan rejects both
    assert h.WitnessPlan.scratch_elems(plan[:33]) == 0
    # the XOR form and the B128 form are what they were
    xor = bits[:2] + [("lincomb", [(0, 1), (1, 1)], 1, 10)]
    assert W.scratch_elems(xor) == h.WitnessBuild.scratch_elems(xor) == 8
    wide = [("given", a, 7, 3), ("lincomb", [(0, 1 << 100)], 5, 3)]
    assert W.scratch_elems(wide) == h.WitnessBuild.scratch_elems(wide) == 8 + 1
    # mixed levels with unit coefficients (B1 + B8 at B8) is an expression now
    mixed = [("given", a, 0, 10), ("given", a, 3, 10), ("lincomb", [(0, 1), (1, 1)], 0, 10)]
    assert W.scratch_elems(mixed) == 64 and h.WitnessBuild.scratch_elems(mixed) == 0
    # ---- what the compute plan rejects answers 0
    g0 = ("given", a, 0, 10)
    assert W.scratch_elems([g0, ("lincomb", [(0, 4)], 0, 10)]) == 0                                  # the combination's level would be 2
    assert W.scratch_elems([g0, ("lincomb", [(0, 1)], 2, 10)]) == 0                                  # ... its offset's level is 1
    assert W.scratch_elems([g0, ("computed", SELECT, [0, 0, 1], 10, 0)]) == 0                        # an input that is not an earlier column
    assert W.scratch_elems([g0, ("given", a, 0, 9), ("computed", SELECT, [0, 0, 1], 10, 0)]) == 0     # an input of another n_vars
    assert W.scratch_elems([g0, ("computed", SELECT, [0, 0], 10, 0)]) == 0                           # a variable without an input
    assert W.scratch_elems([g0, ("computed", [("var", 0), ("const", 2), ("mul", 0, 1)], [0], 10, 0)]) == 0  # a step above the column's level
    assert W.scratch_elems([g0, ("computed", [("var", 0)], [0], 10, 2)]) == 0                        # level 2
    assert W.scratch_elems([("given", a, 3, 10), ("computed", [("var", 0)], [0], 10, 0)]) == 0       # an input above the column's level
    assert W.scratch_elems([g0, ("computed", [], [0], 10, 0)]) == 0                                  # no steps
    assert W.scratch_elems([g0, ("computed", [("var", 0), ("add", 0, 1)], [0], 10, 0)]) == 0         # an operand that is not an earlier step
    assert W.scratch_elems([g0, (14, 0, 0)]) == 0                                                     # an unknown kind
    seventeen = [("var", i) for i in range(34)] + [("mul", 2 * i, 2 * i + 1) for i in range(17)]
    acc = 34
    for i in range(1, 17):
        seventeen.append(("add", acc, 34 + i))
        acc = len(seventeen) - 1
    assert W.scratch_elems([g0, ("computed", seventeen, [0] * 34, 10, 0)]) == 0                      # 17 live slots
    assert W.scratch_elems([g0, ("computed", seventeen[:-2] , [0] * 34, 10, 0)]) == 8                 # (dropping the last sums drops a product: it fits)


def test_compiler_and_packed_arithmetic_on_the_cpu(ffi):
    """binius_amd/csrc/compose_tower.hpp -- what bn_expr_compile_tower and the kernel run -- against value-by-value B128 arithmetic:
    every pair of levels, extreme data, powers, the gadget shapes, 200 random DAGs, the invalid tables (tests/cpp/compose_tower_check.cpp)."""
    exe = os.path.join(ROOT, "tests", "cpp", "compose_tower_check")
    assert os.path.exists(exe), "tests/cpp/compose_tower_check missing -- run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "compose_tower_check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
