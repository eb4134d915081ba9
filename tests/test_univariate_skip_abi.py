"""The univariate round of the univariate-skip zerocheck at the boundary (CPU only): include/binius_amd.h declares
bn_zerocheck_univariate_evals, libbinius_amd.so exports it, the ctypes binding lists and exposes it, and the Rust shim declares it."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "bn_zerocheck_univariate_evals"


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g

    g.build()
    import binius_amd._ffi as f

    return f


def test_header_declares_the_op():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "binius_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, hdr)


def test_library_exports_and_python_binds_the_op(ffi):
    L = ffi.lib()
    assert hasattr(L, SYMBOL)
    assert SYMBOL in ffi.ABI_SYMBOLS
    assert callable(getattr(ffi.Context, "zerocheck_univariate_evals", None))


def test_rust_shim_declares_the_op():
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % SYMBOL, src)
