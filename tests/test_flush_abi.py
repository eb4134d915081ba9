"""The flush witnesses at the boundary (CPU only): include/binius_amd.h declares bn_flush_witness_batch and bn_flush_counters,
libbinius_amd.so exports them, the ctypes binding lists and exposes them, the Rust shim declares them; include/binius_amd_host.h
declares bnh_flush_prodcheck_prove, libbinius_amd_host.so exports it and binius_amd._host binds it as FlushProdcheckPlan."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_flush_witness_batch": "flush_witness_batch", "bn_flush_counters": "flush_counters"}
HOST_SYMBOL = "bnh_flush_prodcheck_prove"


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g

    g.build()
    import binius_amd._ffi as f

    return f


def _decls(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_header_declares_the_op(symbol):
    assert re.search(r"\bint\s+%s\s*\(" % symbol, _decls("binius_amd.h"))


def test_the_prototype_uses_known_type_names_only():
    """No new struct in the prototype: the checked FFI declarations know a closed set of type names."""
    m = re.search(r"\bint\s+bn_flush_witness_batch\s*\(([^;]*?)\)\s*;", _decls("binius_amd.h"), flags=re.S)
    assert m
    words = set(re.findall(r"[A-Za-z_]\w*", m.group(1)))
    types = {w for w in words if w.startswith("bn_") or w in ("void", "const", "uint32_t", "uint64_t", "int")}
    assert {w for w in types if w.startswith("bn_")} == {"bn_ctx", "bn_f128"}


def test_host_header_declares_the_prover():
    assert re.search(r"\bint\s+%s\s*\(" % HOST_SYMBOL, _decls("binius_amd_host.h"))


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_library_exports_and_python_binds_the_op(ffi, symbol):
    L = ffi.lib()
    assert hasattr(L, symbol)
    assert symbol in ffi.ABI_SYMBOLS
    assert callable(getattr(ffi.Context, DEVICE_SYMBOLS[symbol], None))


def test_host_library_exports_and_python_binds_the_prover(ffi):
    import binius_amd._host as h

    assert hasattr(h.host_lib(), HOST_SYMBOL)
    assert callable(getattr(h.FlushProdcheckPlan, "run", None))
    flushes = [
        {"channel": 0, "n_vars": 4, "selectors": [(7, None)], "entries": [("oracle", 3, None, 5), ("const", 9), ("oracle", 7, None, 0)]},
        {"channel": 1, "n_vars": 4, "selectors": [], "entries": [("oracle", 3, None, 5)]},
        {"channel": 1, "n_vars": 2, "selectors": [(1, None), (2, None)], "entries": [("oracle", 5, None, 3)]},
    ]
    nonzero = [(11, None, 7, 3)]
    # groups: n_vars 4 over the ids {3, 7} (the selector is also a column: one multilinear), n_vars 2 over {1, 2, 5}
    assert h.FlushProdcheckPlan.groups(flushes) == [(4, [0], [3, 7]), (2, [2], [1, 2, 5])]
    # one query element; witness + arena per oracle: 2 * (16 + 16 + 4 + 8); the grand-product prover's scratch: the padded copies
    # 16 + 16 + 4 + 8 and the indicator's table 2^3; the largest reduction: two multilinears of 16 elements and a table of 8
    assert h.FlushProdcheckPlan.scratch_elems(flushes, nonzero) == 1 + 2 * 44 + (44 + 8) + (2 * 16 + 8)
    # without variables there is no arena and no table
    zero = [{"channel": 0, "n_vars": 0, "selectors": [(1, None)], "entries": [("oracle", 2, None, 7)]}]
    assert h.FlushProdcheckPlan.scratch_elems(zero, []) == 1 + 1 + 0 + 2


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_rust_shim_declares_the_op(symbol):
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % symbol, src)
