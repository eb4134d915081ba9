"""The univariate-skip zerocheck for tables over B16 .. B128 at the boundary (CPU only): include/binius_amd.h declares
bn_zerocheck_univariate_evals_base, libbinius_amd.so exports it, the ctypes binding lists and exposes it, the Rust shim declares it;
include/binius_amd_host.h declares bnh_zerocheck_batch_prove_tower and its scratch formula, libbinius_amd_host.so exports them and
binius_amd._host binds them as ZerocheckBatchPlan(..., tower=True); the validation that needs no device rejects."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "bn_zerocheck_univariate_evals_base"
HOST_SYMBOLS = ("bnh_zerocheck_batch_prove_tower", "bnh_zerocheck_batch_scratch_elems_tower")


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g

    g.build()
    import binius_amd._ffi as f

    return f


def _decls(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_declares_the_op_with_the_base_level_after_the_context():
    h = _decls("binius_amd.h")
    old = re.search(r"\bint\s+bn_zerocheck_univariate_evals\s*\((.*?)\)\s*;", h, flags=re.S).group(1)
    new = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % SYMBOL, h, flags=re.S).group(1)
    norm = lambda s: [re.sub(r"\s+", " ", a).strip() for a in s.split(",")]  # noqa: E731
    old, new = norm(old), norm(new)
    assert new == [old[0], "uint32_t base_level"] + old[1:]


@pytest.mark.parametrize("symbol", HOST_SYMBOLS)
def test_host_header_declares_the_prover(symbol):
    assert re.search(r"\b(int|uint64_t)\s+%s\s*\(" % symbol, _decls("binius_amd_host.h"))


def test_host_prover_takes_the_argument_list_of_the_old_one():
    h = _decls("binius_amd_host.h")
    args = lambda name: re.sub(r"\s+", " ", re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, h, flags=re.S).group(1))  # noqa: E731
    assert args("bnh_zerocheck_batch_prove_tower") == args("bnh_zerocheck_batch_prove")


def test_library_exports_and_python_binds_the_op(ffi):
    assert hasattr(ffi.lib(), SYMBOL)
    assert SYMBOL in ffi.ABI_SYMBOLS
    assert callable(getattr(ffi.Context, "zerocheck_univariate_evals_base", None))


def test_rust_shim_declares_the_op():
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    m = re.search(r"pub fn %s\s*\((.*?)\)\s*->\s*c_int;" % SYMBOL, src, flags=re.S)
    assert m
    names = [a.split(":")[0].strip() for a in m.group(1).split(",") if a.strip()]
    assert names[:4] == ["ctx", "base_level", "n_vars", "skip_rounds"] and len(names) == 15


def test_host_library_exports_and_python_binds_the_prover(ffi):
    import binius_amd._host as h

    for s in HOST_SYMBOLS:
        assert hasattr(h.host_lib(), s)
    col = lambda level: (None, level)  # noqa: E731
    scratch = h.ZerocheckBatchPlan.scratch_elems
    # b32_mul at n = 9, k = 7: 4 + 3 * 4 + 2 (the indicator tables and the folded columns), 4 + 3 * 128 (the projection's query and
    # outputs), 128 Lagrange coefficients for the wide folds
    assert scratch([(9, [col(5)] * 3, [])], 7, tower=True) == (4 + 12 + 2) + (4 + 384) + 128
    # a 2-variable table of a level-7 and a B1 column, padded to k = 7: 128 + 1 padded elements, 1 indicator element, 2 folded values;
    # an 8-variable table of one B8 column: 2 + 2 + 1, then 2 + 128; the 128 coefficients
    assert scratch([(2, [col(7), col(0)], []), (8, [col(3)], [])], 7, tower=True) == (129 + 1 + 2) + (2 + 2 + 1) + (2 + 128) + 128
    # without a wide column: no coefficients, a padded B1 column of 128 bits is 1 element and a B8 one 8; the old formula (16 elements
    # per padded column) is what it was
    assert scratch([(5, [col(0), col(3)], []), (9, [col(0)] * 3, [])], 7, tower=True) == (1 + 8 + 1 + 2) + (4 + 12 + 2) + (4 + 384)
    assert scratch([(5, [col(0), col(3)], []), (9, [col(0)] * 3, [])], 7) == (32 + 1 + 2) + (4 + 12 + 2) + (4 + 384)
    # a level above 7: out of range
    assert scratch([(9, [col(8)], [])], 7, tower=True) == 0


def test_validation_without_a_device(ffi):
    """A null context is rejected by both entry points before anything else is looked at."""
    import binius_amd._host as h

    L = ffi.lib()
    one = (ffi.F128 * 2)()
    u32 = (C.c_uint32 * 2)(0, 3)
    assert L.bn_zerocheck_univariate_evals_base(None, 5, 8, 3, None, 0, None, u32, u32, 0, None, 0, 16, None, one) == ffi.BN_ERR_INPUT_VALIDATION
    assert b"null argument" in L.bn_last_error()
    H = h.host_lib()
    u32, f = (C.c_uint32 * 1)(9), (ffi.F128 * 16)()
    args = [None, 1, 7, u32, u32, None, None, u32, None, None, None, None, None, f, f, f, f, f, f, None, 0, f, f, f, f, f, f, f, f, None, None]
    assert H.bnh_zerocheck_batch_prove_tower(*args) == ffi.BN_ERR_INPUT_VALIDATION
    assert b"null argument" in H.bnh_last_error()
