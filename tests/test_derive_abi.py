"""The derive op and the witness plan at the boundary (CPU only): include/binius_amd.h declares bn_derive_columns_batch and
bn_derive_counters with bn_derive_job, libbinius_amd.so exports them, the ctypes binding lists and exposes them with a struct of the
header's size, offsets and field order, the Rust shim declares them; include/binius_amd_host.h declares bnh_witness_derive and
bnh_witness_derive_scratch_elems, libbinius_amd_host.so exports them and binius_amd._host binds them; the scratch formula matches a
hand count for a small plan."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_derive_columns_batch": "derive_columns_batch", "bn_derive_counters": "derive_counters"}
HOST_SYMBOLS = ("bnh_witness_derive", "bnh_witness_derive_scratch_elems")
C_TYPES = {"const void *": C.c_void_p, "void *": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "bn_f128": None}
# bn_derive_job on an LP64 target: (field, offset); 88 bytes, no padding
LAYOUT = [("kind", 0), ("tower_level", 4), ("n_vars", 8), ("inner_n_vars", 12), ("d_inner", 16), ("d_out", 24), ("block_size", 32), ("shift_variant", 36),
          ("shift_offset", 40), ("start_index", 48), ("reserved", 52), ("nonzero_index", 56), ("first_term", 64), ("n_terms", 68), ("offset", 72)]


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


@pytest.mark.parametrize("symbol", HOST_SYMBOLS)
def test_host_library_exports_and_python_binds_the_plan(ffi, symbol):
    import binius_amd._host as h

    ffi.lib()
    assert re.search(r"\b(int|uint64_t)\s+%s\s*\(" % symbol, _decls("binius_amd_host.h"))
    fn = getattr(h.host_lib(), symbol)
    hm = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % symbol, _decls("binius_amd_host.h"), flags=re.S)
    assert len(fn.argtypes) == len([a for a in hm.group(1).split(",") if a.strip()])
    assert h.WitnessPlan.KINDS == {"given": 0, "shifted": 1, "repeating": 2, "zero_padded": 3, "packed": 4, "lincomb": 5}
    for name, val in h.WitnessPlan.KINDS.items():
        c_name = {"lincomb": "LINCOMB"}.get(name, name.upper())
        assert re.search(r"\bBNH_WIT_%s\s*=\s*%d\b" % (c_name, val), _decls("binius_amd_host.h"))


def test_python_struct_has_the_headers_layout(ffi):
    want = _header_struct("bn_derive_job")
    struct = ffi.DeriveJob
    assert [f[0] for f in struct._fields_] == [f[0] for f in want] == [f[0] for f in LAYOUT]
    for (name, ctype), (_, c_ty) in zip(struct._fields_, want):
        assert c_ty in C_TYPES, c_ty
        assert ctype is (ffi.F128 if c_ty == "bn_f128" else C_TYPES[c_ty]), name
    assert C.sizeof(struct) == 88
    assert [(name, getattr(struct, name).offset) for name, _ in LAYOUT] == LAYOUT
    rust = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    m = re.search(r"pub struct bn_derive_job\s*\{(.*?)\}", rust, flags=re.S)
    assert m and re.findall(r"pub (\w+):", m.group(1)) == [f[0] for f in want]


def test_constants_agree(ffi):
    h = _decls("binius_amd.h")
    rust = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    for i, name in enumerate(("SHIFTED", "REPEATING", "ZERO_PADDED", "XOR_COMBINATION")):
        assert re.search(r"\bBN_DERIVE_%s\s*=\s*%d\b" % (name, i), h) and getattr(ffi, "DERIVE_" + name) == i
        assert re.search(r"pub const BN_DERIVE_%s: u32 = %d;" % (name, i), rust)
    for i, name in enumerate(("CIRCULAR_LEFT", "LOGICAL_LEFT", "LOGICAL_RIGHT")):
        assert re.search(r"\bBN_SHIFT_%s\s*=\s*%d\b" % (name, i), h) and getattr(ffi, "SHIFT_" + name) == i
        assert re.search(r"pub const BN_SHIFT_%s: u32 = %d;" % (name, i), rust)
    assert re.search(r"\bBN_DERIVE_N\s*=\s*3\b", h) and re.search(r"pub const BN_DERIVE_N: usize = 3;", rust)


def test_scratch_formula_on_a_small_plan(ffi):
    import binius_amd._host as h

    class Col:
        def __init__(self, ptr):
            self.ptr = ptr

    a, b, c, small = Col(0x1000), Col(0x2000), Col(0x3000), Col(0x4000)
    plan = [
        ("given", a, 0, 10),                      # 0: B1, 2^10 bits = 8 elements
        ("given", b, 0, 10),                      # 1
        ("given", c, 7, 3),                       # 2: B128, 8 elements
        ("given", small, 3, 0),                   # 3: one byte, below one element
        ("lincomb", [(0, 1), (1, 1)], 0, 10),     # 4: XOR form at B1: 8 elements
        ("shifted", 4, 6, 1, "circular_left"),    # 5: 8 elements
        ("packed", 5, 3),                         # 6: an alias of 5 at B8, n_vars 7: nothing
        ("repeating", 3, 9),                      # 7: B8, 2^9 bytes: 32 elements
        ("zero_padded", 0, 2, 3, 1),              # 8: B1, 2^12 bits: 32 elements
        ("repeating", 3, 2),                      # 9: B8, 4 bytes, below one element: one element, host work
        ("lincomb", [(2, 0x1234), (2, 1)], 5, 3),  # 10: a B128 combination outside the XOR form: 8 elements + the query ONE
    ]
    assert h.WitnessPlan.scratch_elems(plan) == 8 + 8 + 32 + 32 + 1 + 8 + 1
    assert h.WitnessPlan.scratch_elems(plan[:10]) == 8 + 8 + 32 + 32 + 1  # no lincomb call: no ONE
    assert h.WitnessPlan.scratch_elems(plan[:4]) == 0
    # a B32 combination with a non-unit coefficient has no route: the plan is rejected (the formula answers 0)
    assert h.WitnessPlan.scratch_elems(plan + [("given", a, 5, 5), ("lincomb", [(11, 3)], 0, 5)]) == 0
    # an inner index is smaller than the column's own
    assert h.WitnessPlan.scratch_elems([("given", a, 0, 10), ("shifted", 1, 3, 1, 0)]) == 0
