"""The GKR grand-product argument at the boundary (CPU only): include/binius_amd.h declares bn_product_tree_layers (and its
companion bn_pad_with_ones), libbinius_amd.so exports them, the ctypes binding lists and exposes them, the Rust shim declares them;
include/binius_amd_host.h declares bnh_gkr_gpa_prove, libbinius_amd_host.so exports it and binius_amd._host binds it as GkrGpaPlan."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_product_tree_layers": "product_tree_layers", "bn_pad_with_ones": "pad_with_ones"}
HOST_SYMBOL = "bnh_gkr_gpa_prove"


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
    assert callable(getattr(h.GkrGpaPlan, "run", None))
    assert h.GkrGpaPlan.scratch_elems([3, 0, 5, 1]) == 8 + 32 + 2 + 16


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_rust_shim_declares_the_op(symbol):
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % symbol, src)
