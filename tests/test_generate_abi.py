"""The generate op and the build plan at the boundary (CPU only): include/binius_amd.h declares bn_generate_columns_batch and
bn_generate_counters with bn_generate_job, libbinius_amd.so exports them, the ctypes binding lists and exposes them with a struct of the
header's size, offsets and field order, the Rust shim declares them; include/binius_amd_host.h declares bnh_witness_build and
bnh_witness_build_scratch_elems, libbinius_amd_host.so exports them and binius_amd._host binds them in WitnessBuild, whose kinds are a
strict superset of WitnessPlan's; the scratch formula matches a hand count for a small plan."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_generate_columns_batch": "generate_columns_batch", "bn_generate_counters": "generate_counters"}
HOST_SYMBOLS = ("bnh_witness_build", "bnh_witness_build_scratch_elems")
C_TYPES = {"const void *": C.c_void_p, "void *": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "bn_f128": None}
# bn_generate_job on an LP64 target: (field, offset); 72 bytes, no padding
LAYOUT = [("kind", 0), ("tower_level", 4), ("n_vars", 8), ("start_index", 12), ("d_inner", 16), ("d_out", 24), ("query_size", 32), ("reserved", 36),
          ("query_bits", 40), ("index", 48), ("value", 56)]
GEN_KINDS = ("PROJECTED_BITS", "CONSTANT", "STEP_DOWN", "STEP_UP", "SELECT_ROW", "INCREMENTING", "POWERS")


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g

    g.build()
    import binius_amd._ffi as f

    return f


def _decls(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _header_struct(name):
    """[(field, C type)] of `typedef struct { ... } name;` in include/binius_amd.h."""
    m = re.search(r"typedef struct\s*\{([^}]*)\}\s*%s\s*;" % name, _decls("binius_amd.h"), flags=re.S)
    assert m, name
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if decl:
            ty, field = re.match(r"(.*?)(\w+)$", decl).groups()
            fields.append((field, ty.strip()))
    return fields


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_both_sides_declare_export_and_bind_the_op(ffi, symbol):
    assert re.search(r"\bint\s+%s\s*\(" % symbol, _decls("binius_amd.h"))
    assert hasattr(ffi.lib(), symbol)
    assert symbol in ffi.ABI_SYMBOLS
    assert callable(getattr(ffi.Context, DEVICE_SYMBOLS[symbol], None))
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % symbol, src)
    lib_rs = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "lib.rs")).read()
    assert "ffi::bn_generate_columns_batch" in lib_rs


@pytest.mark.parametrize("symbol", HOST_SYMBOLS)
def test_host_library_exports_and_python_binds_the_plan(ffi, symbol):
    import binius_amd._host as h

    ffi.lib()
    assert re.search(r"\b(int|uint64_t)\s+%s\s*\(" % symbol, _decls("binius_amd_host.h"))
    fn = getattr(h.host_lib(), symbol)
    hm = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % symbol, _decls("binius_amd_host.h"), flags=re.S)
    assert len(fn.argtypes) == len([a for a in hm.group(1).split(",") if a.strip()])
    # the encoding is bnh_witness_derive's: the same parameter list
    dm = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % symbol.replace("build", "derive"), _decls("binius_amd_host.h"), flags=re.S)
    assert " ".join(hm.group(1).split()) == " ".join(dm.group(1).split())


def test_build_kinds_are_a_strict_superset_of_the_plans(ffi):
    import binius_amd._host as h

    old, new = h.WitnessPlan.KINDS, h.WitnessBuild.KINDS
    assert old == {"given": 0, "shifted": 1, "repeating": 2, "zero_padded": 3, "packed": 4, "lincomb": 5}
    assert set(old.items()) < set(new.items())
    assert {k: v for k, v in new.items() if k not in old} == {name.lower(): 6 + i for i, name in enumerate(GEN_KINDS)}
    for name, val in new.items():
        c_name = {"lincomb": "LINCOMB"}.get(name, name.upper())
        assert re.search(r"\bBNH_WIT_%s\s*=\s*%d\b" % (c_name, val), _decls("binius_amd_host.h")), name


def test_python_struct_has_the_headers_layout(ffi):
    want = _header_struct("bn_generate_job")
    struct = ffi.GenerateJob
    assert [f[0] for f in struct._fields_] == [f[0] for f in want] == [f[0] for f in LAYOUT]
    for (name, ctype), (_, c_ty) in zip(struct._fields_, want):
        assert c_ty in C_TYPES, c_ty
        assert ctype is (ffi.F128 if c_ty == "bn_f128" else C_TYPES[c_ty]), name
    assert C.sizeof(struct) == 72
    assert [(name, getattr(struct, name).offset) for name, _ in LAYOUT] == LAYOUT
    rust = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    m = re.search(r"pub struct bn_generate_job\s*\{(.*?)\}", rust, flags=re.S)
    assert m and re.findall(r"pub (\w+):", m.group(1)) == [f[0] for f in want]


def test_constants_agree(ffi):
    h = _decls("binius_amd.h")
    rust = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    for i, name in enumerate(GEN_KINDS):
        assert re.search(r"\bBN_GEN_%s\s*=\s*%d\b" % (name, i), h) and getattr(ffi, "GEN_" + name) == i
        assert re.search(r"pub const BN_GEN_%s: u32 = %d;" % (name, i), rust)
        assert ffi.GEN_KINDS[name.lower()] == i
    for i, name in enumerate(("CALLS", "LAUNCHES", "JOBS")):
        assert re.search(r"\bBN_GENERATE_%s\s*=\s*%d\b" % (name, i), h)
    assert re.search(r"\bBN_GENERATE_N\s*=\s*3\b", h) and re.search(r"pub const BN_GENERATE_N: usize = 3;", rust)


def test_scratch_formula_on_a_small_plan(ffi):
    import binius_amd._host as h

    class Col:
        def __init__(self, ptr):
            self.ptr = ptr

    a = Col(0x1000)
    plan = [
        ("given", a, 0, 12),                      # 0: B1, 2^12 bits = 32 elements
        ("shifted", 0, 5, 1, "logical_left"),     # 1: 32 elements
        ("projected_bits", 1, 0, 5, 7),           # 2: bit 7 of every 32-bit word: 2^7 bits = 1 element
        ("projected_bits", 2, 3, 2, 1),           # 3: 2^5 bits, below one element: one element, host work
        ("repeating", 2, 3),                      # 4: 2^10 bits = 8 elements
        ("step_down", 12, 3000),                  # 5: 32 elements
        ("incrementing", 5, 12),                  # 6: B32, 2^12 values = 1024 elements
        ("constant", 3, 4, 0xA5),                 # 7: 16 bytes = 1 element
        ("zero_padded", 7, 2, 0, 1),              # 8: 64 bytes = 4 elements
        ("powers", 6, 3, 0x1234),                 # 9: B64, 8 values = 4 elements
        ("select_row", 3, 5),                     # 10: 8 bits: one element, host work
    ]
    assert h.WitnessBuild.scratch_elems(plan) == 32 + 1 + 1 + 8 + 32 + 1024 + 1 + 4 + 4 + 1
    assert h.WitnessBuild.scratch_elems(plan[:2]) == h.WitnessPlan.scratch_elems(plan[:2]) == 32
    assert h.WitnessPlan.scratch_elems(plan[:2] + [(6, 1, 0, 5)]) == 0  # the derive plan rejects the new kinds: its formula answers 0
    # what the build plan rejects answers 0 too
    assert h.WitnessBuild.scratch_elems([("given", a, 0, 12), ("projected_bits", 0, 8, 5, 0)]) == 0   # start_index + query_size > inner n_vars
    assert h.WitnessBuild.scratch_elems([("given", a, 0, 12), ("projected_bits", 0, 0, 5, 32)]) == 0  # query_bits = 2^query_size
    assert h.WitnessBuild.scratch_elems([("select_row", 12, 1 << 12)]) == 0                            # the strict bound
    assert h.WitnessBuild.scratch_elems([("step_down", 12, 1 << 12)]) == 32                            # ... which a step does not have
    assert h.WitnessBuild.scratch_elems([("incrementing", 3, 9)]) == 0                                 # n_vars > 2^level
    assert h.WitnessBuild.scratch_elems([("powers", 3, 9, 0x100)]) == 0                                # a base above the level
    assert h.WitnessBuild.scratch_elems([("constant", 2, 9, 1)]) == 0                                  # level 2
    assert h.WitnessBuild.scratch_elems([(13, 0, 0)]) == 0                                             # an unknown kind
