"""The linear-combination projection at the boundary (CPU only): include/binius_amd.h declares bn_partial_eval_high_lincomb_batch and
bn_partial_eval_lincomb_counters with their two structs, libbinius_amd.so exports them, the ctypes binding lists and exposes them with
structs of the header's sizes and field order, the Rust shim declares them; include/binius_amd_host.h declares
bnh_evalcheck_bivariate_prove_lc, libbinius_amd_host.so exports it and binius_amd._host binds it; the scratch formula counts a distinct
(terms, offset, suffix) once."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_partial_eval_high_lincomb_batch": "partial_eval_high_lincomb_batch", "bn_partial_eval_lincomb_counters": "partial_eval_lincomb_counters"}
HOST_SYMBOL = "bnh_evalcheck_bivariate_prove_lc"
C_TYPES = {"const void *": C.c_void_p, "uint32_t": C.c_uint32, "bn_f128": None}


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


def test_host_library_exports_and_python_binds_the_prover(ffi):
    import binius_amd._host as h

    ffi.lib()
    assert re.search(r"\bint\s+%s\s*\(" % HOST_SYMBOL, _decls("binius_amd_host.h"))
    assert re.search(r"\bBNH_EC_LINCOMB\s*=\s*3\b", _decls("binius_amd_host.h"))
    fn = getattr(h.host_lib(), HOST_SYMBOL)
    assert len(fn.argtypes) == 15 + 5  # bnh_evalcheck_bivariate_prove's arguments, n_terms, three term arrays, the offsets
    assert h.EvalcheckPlan.KINDS["lincomb"] == 3


@pytest.mark.parametrize("c_name,py_name,size", [("bn_pel_term", "PelTerm", 32), ("bn_pel_job", "PelJob", 32)])
def test_python_structs_have_the_headers_layout(ffi, c_name, py_name, size):
    want = _header_struct(c_name)
    struct = getattr(ffi, py_name)
    assert [f[0] for f in struct._fields_] == [f[0] for f in want]
    for (name, ctype), (_, c_ty) in zip(struct._fields_, want):
        assert c_ty in C_TYPES, c_ty
        assert ctype is (ffi.F128 if c_ty == "bn_f128" else C_TYPES[c_ty]), name
    assert C.sizeof(struct) == size  # 8 + 4 + 4 + 16 and 4 * 4 + 16: no padding on an LP64 target
    rust = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    m = re.search(r"pub struct %s\s*\{(.*?)\}" % c_name, rust, flags=re.S)
    assert m and re.findall(r"pub (\w+):", m.group(1)) == [f[0] for f in want]


def test_constants_agree(ffi):
    h = _decls("binius_amd.h")
    rust = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"#define BN_PEL_MAX_TERMS 64\b", h) and ffi.PEL_MAX_TERMS == 64 and re.search(r"pub const BN_PEL_MAX_TERMS: u32 = 64;", rust)
    assert re.search(r"\bBN_PEL_N\s*=\s*7\b", h) and re.search(r"pub const BN_PEL_N: usize = 7;", rust)


def test_scratch_formula_on_a_two_prover_example(ffi):
    import binius_amd._host as h

    class Col:
        def __init__(self, ptr):
            self.ptr = ptr

    a, b, c = Col(0x1000), Col(0x2000), Col(0x3000)
    sum_ab = [(a, 0, 1), (b, 0, 1)]
    provers = [
        # b = 3: a lincomb at the empty suffix and a shift indicator
        (3, [("lincomb", [(c, 6, 2)], 5, 3, 0, 0), ("shift", 3, 1, 2, 0, 3)], [(0, 1)], [0]),
        # b = 6: a + b at suffix [6:10) twice (an equal term list written again: once), the same terms with another offset, a + b at a second
        # suffix, a plain projection at the first suffix (shares its expansion), a shift indicator
        (6, [("lincomb", sum_ab, 0, 10, 6, 4), ("lincomb", list(sum_ab), 0, 10, 6, 4), ("lincomb", sum_ab, 1, 10, 6, 4), ("lincomb", sum_ab, 0, 11, 10, 5),
             ("proj", a, 0, 10, 6, 4), ("shift", 6, 1, 0, 0, 6)], [(0, 5)], [0]),
    ]
    # suffixes: 2^0 + 2^4 + 2^5; tables: (1 + 1) * 8 and (3 + 1 + 1) * 64; fold buffers: 2 * 4 + 6 * 32
    assert h.EvalcheckPlan.scratch_elems(provers) == (1 + 16 + 32) + (16 + 320) + (8 + 192)
    # without the lincombs the formula is the parent's
    plain = [(6, [("proj", a, 0, 10, 6, 4), ("shift", 6, 1, 0, 0, 6)], [(0, 1)], [0])]
    assert h.EvalcheckPlan.scratch_elems(plain) == 16 + 64 + 64 + 2 * 32
