"""Evalcheck's column projection and bivariate prover at the boundary (CPU only): include/binius_amd.h declares
bn_partial_eval_high_batch and bn_partial_eval_counters, libbinius_amd.so exports them, the ctypes binding lists and exposes them, the
Rust shim declares them; include/binius_amd_host.h declares bnh_evalcheck_bivariate_prove, libbinius_amd_host.so exports it and
binius_amd._host binds it as EvalcheckPlan."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_partial_eval_high_batch": "partial_eval_high_batch", "bn_partial_eval_counters": "partial_eval_counters"}
HOST_SYMBOL = "bnh_evalcheck_bivariate_prove"


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


def test_header_declares_the_column_and_the_counters():
    h = _decls("binius_amd.h")
    assert re.search(r"typedef struct\s*\{[^}]*d_evals[^}]*tower_level[^}]*n_vars[^}]*\}\s*bn_pe_column\s*;", h, flags=re.S)
    assert re.search(r"\bBN_PE_N\s*=\s*6\b", h)


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
    assert callable(getattr(h.EvalcheckPlan, "run", None))

    class Col:
        def __init__(self, ptr):
            self.ptr = ptr

    a, b = Col(0x1000), Col(0x2000)
    # one 6-variable prover: two projections of column a at the same suffix (projected once), one of column b at it, one of a at a
    # second suffix, a shift indicator and a tower basis; one 3-variable prover with an empty suffix
    provers = [
        (3, [("proj", b, 6, 3, 0, 0), ("shift", 3, 1, 2, 0, 3)], [(0, 1)], [0]),
        (6, [("proj", a, 0, 10, 6, 4), ("proj", a, 0, 10, 6, 4), ("proj", b, 0, 10, 6, 4), ("proj", a, 0, 11, 10, 5), ("shift", 6, 1, 0, 0, 6), ("basis", 6, 0)],
         [(0, 4)], [0]),
    ]
    # suffixes: 2^0 + 2^4 + 2^5; tables: (1 + 1) * 8 and (3 + 2) * 64; fold buffers: 2 * 4 + 6 * 32
    assert h.EvalcheckPlan.scratch_elems(provers) == (1 + 16 + 32) + (16 + 320) + (8 + 192)


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_rust_shim_declares_the_op(symbol):
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % symbol, src)
