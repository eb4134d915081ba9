"""The GKR exponentiation argument at the boundary (CPU only): include/binius_amd.h declares bn_exp_circuit_layers (and its companion
bn_bits_to_b128), libbinius_amd.so exports them, the ctypes binding lists and exposes them, the Rust shim declares them;
include/binius_amd_host.h declares bnh_gkr_exp_prove, libbinius_amd_host.so exports it and binius_amd._host binds it as GkrExpPlan."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_exp_circuit_layers": "exp_circuit_layers", "bn_bits_to_b128": "bits_to_b128", "bn_exp_counters": "exp_counters"}
HOST_SYMBOL = "bnh_gkr_exp_prove"


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
    assert callable(getattr(h.GkrExpPlan, "run", None))
    # per claim: one column (two for a dynamic base) plus half a column for the indicator's table, none of the latter at n_vars = 0
    assert h.GkrExpPlan.scratch_elems([5, 3, 1, 0, 0], [True, False, True, False, True]) == (64 + 16) + (8 + 4) + (4 + 1) + 1 + 2


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_rust_shim_declares_the_op(symbol):
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % symbol, src)
