"""The univariate-skip zerocheck at the boundary (CPU only): include/binius_amd.h declares bn_univariate_fold_batch and
bn_univariate_fold_counters, libbinius_amd.so exports them, the ctypes binding lists and exposes them, the Rust shim declares them;
include/binius_amd_host.h declares bnh_zerocheck_batch_prove and its scratch formula, libbinius_amd_host.so exports them and
binius_amd._host binds them as ZerocheckBatchPlan; the validation that needs no device rejects."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_univariate_fold_batch": "univariate_fold_batch", "bn_univariate_fold_counters": "univariate_fold_counters"}
HOST_SYMBOLS = ("bnh_zerocheck_batch_prove", "bnh_zerocheck_batch_scratch_elems")


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


def test_header_declares_the_limits_and_the_counters():
    h = _decls("binius_amd.h")
    assert re.search(r"#define\s+BN_UNIVARIATE_FOLD_MAX_SKIP\s+8\b", h)
    assert re.search(r"\bBN_UF_CALLS\s*=\s*0\b.*\bBN_UF_LAUNCHES\s*=\s*1\b.*\bBN_UF_COLS\s*=\s*2\b.*\bBN_UF_N\s*=\s*3\b", h)
    # the columns travel as untyped memory (the layout of bn_pe_column), the coefficients from the host
    assert re.search(r"bn_univariate_fold_batch\s*\(\s*bn_ctx \*ctx,\s*const void \*cols,\s*uint32_t n_cols,\s*uint32_t skip_rounds,\s*const bn_f128 \*h_coeffs,\s*"
                     r"void \*const \*d_outs\s*\)", h)


@pytest.mark.parametrize("symbol", HOST_SYMBOLS)
def test_host_header_declares_the_prover(symbol):
    assert re.search(r"\b(int|uint64_t)\s+%s\s*\(" % symbol, _decls("binius_amd_host.h"))


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_library_exports_and_python_binds_the_op(ffi, symbol):
    L = ffi.lib()
    assert hasattr(L, symbol)
    assert symbol in ffi.ABI_SYMBOLS
    assert callable(getattr(ffi.Context, DEVICE_SYMBOLS[symbol], None))


def test_host_library_exports_and_python_binds_the_prover(ffi):
    import binius_amd._host as h

    for s in HOST_SYMBOLS:
        assert hasattr(h.host_lib(), s)
    assert callable(getattr(h.ZerocheckBatchPlan, "run", None))
    assert h.ZerocheckBatchPlan.PHASES == ("univariate", "fold", "multilinear", "projection", "reduction")
    # a 5-variable table of 2 columns, padded to k = 7: 2 * 16 padded elements, 1 indicator element, 2 folded values; a 9-variable table
    # of 3 columns: 4 + 3 * 4 + 2 (the indicator tables and the folded columns), 4 + 3 * 128 (the projection's query and outputs)
    tables = [(5, [None, None], []), (9, [None, None, None], [])]
    assert h.ZerocheckBatchPlan.scratch_elems(tables, 7) == (32 + 1 + 2) + (4 + 12 + 2) + (4 + 384)
    # n = k: no multilinear round, no indicator table for the prover
    assert h.ZerocheckBatchPlan.scratch_elems([(7, [None], [])], 7) == (1 + 1) + (1 + 128)


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_rust_shim_declares_the_op(symbol):
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % symbol, src)
    assert re.search(r"pub const BN_UF_N: usize = 3;", src)


def test_validation_without_a_device(ffi):
    """A null context is rejected by both entry points before anything else is looked at; so is a prover call without tables."""
    import binius_amd._host as h

    L = ffi.lib()
    one = (ffi.F128 * 2)()
    outs = (C.c_void_p * 1)()
    assert L.bn_univariate_fold_batch(None, None, 1, 1, one, outs) == ffi.BN_ERR_INPUT_VALIDATION
    assert b"null ctx" in L.bn_last_error()
    assert L.bn_univariate_fold_counters(None, (C.c_uint64 * 3)()) == ffi.BN_ERR_INPUT_VALIDATION
    H = h.host_lib()
    u32, f = (C.c_uint32 * 1)(9), (ffi.F128 * 16)()
    args = [None, 1, 7, u32, u32, None, None, u32, None, None, None, None, None, f, f, f, f, f, f, None, 0, f, f, f, f, f, f, f, f, None, None]
    assert H.bnh_zerocheck_batch_prove(*args) == ffi.BN_ERR_INPUT_VALIDATION
    assert b"null argument" in H.bnh_last_error()


def test_binding_checks_the_shapes_it_can(ffi):
    class Ctx:  # (no device: the checks below run before the library is entered)
        _h = None

    with pytest.raises(ffi.BnError) as e:
        ffi.Context.univariate_fold_batch(Ctx(), [(ffi.DevSlice(0x1000, 2), 0, 8)], 7, [0] * 127, [ffi.DevSlice(0x2000, 2)])
    assert e.value.kind == "InputValidation"
    with pytest.raises(ffi.BnError) as e:
        ffi.Context.univariate_fold_batch(Ctx(), [(ffi.DevSlice(0x1000, 2), 0, 8)], 7, [0] * 128, [ffi.DevSlice(0x2000, 4)])
    assert e.value.kind == "InputValidation"
    with pytest.raises(ffi.BnError) as e:
        ffi.Context.univariate_fold_batch(Ctx(), [(ffi.DevSlice(0x1000, 2), 0, 8)], 7, [0] * 128, [])
    assert e.value.kind == "InputValidation"
