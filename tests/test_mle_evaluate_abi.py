"""The evaluations in front of an evalcheck round at the boundary (CPU only): include/binius_amd.h declares bn_mle_evaluate_batch,
bn_mle_evaluate_counters, the two structs and the limits, libbinius_amd.so exports the functions, the ctypes binding lists and exposes
them, the Rust shim declares them; include/binius_amd_host.h declares bnh_evalcheck_evaluate and its scratch formula,
libbinius_amd_host.so exports them and binius_amd._host binds them as EvalcheckEvaluatePlan."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_mle_evaluate_batch": "mle_evaluate_batch", "bn_mle_evaluate_counters": "mle_evaluate_counters"}
HOST_SYMBOLS = {"bnh_evalcheck_evaluate": "int", "bnh_evalcheck_evaluate_scratch_elems": "uint64_t"}
POINT_FIELDS = ("d_lo", "d_hi", "lo_vars", "hi_vars")
JOB_FIELDS = ("d_evals", "tower_level", "n_vars", "point", "reserved")


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g

    g.build()
    import binius_amd._ffi as f

    return f


def _decls(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _rust():
    return open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_header_declares_the_op(symbol):
    assert re.search(r"\bint\s+%s\s*\(" % symbol, _decls("binius_amd.h"))


def test_header_declares_the_structs_and_the_limits():
    h = _decls("binius_amd.h")
    assert re.search(r"typedef struct\s*\{[^}]*%s[^}]*\}\s*bn_me_point\s*;" % r"[^}]*".join(POINT_FIELDS), h, flags=re.S)
    assert re.search(r"typedef struct\s*\{[^}]*%s[^}]*\}\s*bn_me_job\s*;" % r"[^}]*".join(JOB_FIELDS), h, flags=re.S)
    assert re.search(r"\bBN_ME_N\s*=\s*4\b", h)
    assert re.search(r"#define\s+BN_ME_MAX_LO_VARS\s+10\b", h)
    m = re.search(r"#define\s+BN_ME_MAX_JOBS\s+(\d+)\b", h)
    assert m and int(m.group(1)) >= 1024


@pytest.mark.parametrize("symbol", sorted(HOST_SYMBOLS))
def test_host_header_declares_the_mirror(symbol):
    assert re.search(r"\b%s\s+%s\s*\(" % (HOST_SYMBOLS[symbol], symbol), _decls("binius_amd_host.h"))


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_library_exports_and_python_binds_the_op(ffi, symbol):
    assert hasattr(ffi.lib(), symbol)
    assert symbol in ffi.ABI_SYMBOLS
    assert callable(getattr(ffi.Context, DEVICE_SYMBOLS[symbol], None))


def test_python_structs_match_the_header(ffi):
    assert tuple(n for n, _ in ffi.MePoint._fields_) == POINT_FIELDS
    assert tuple(n for n, _ in ffi.MeJob._fields_) == JOB_FIELDS
    assert C.sizeof(ffi.MePoint) == 24 and C.sizeof(ffi.MeJob) == 24
    h = _decls("binius_amd.h")
    assert ffi.BN_ME_MAX_LO_VARS == 10
    assert ffi.BN_ME_MAX_JOBS == int(re.search(r"#define\s+BN_ME_MAX_JOBS\s+(\d+)", h).group(1))


def test_rust_shim_declares_the_op_the_structs_and_the_limits():
    src = _rust()
    for symbol in DEVICE_SYMBOLS:
        assert re.search(r"pub fn %s\s*\(" % symbol, src)
    for name, fields in (("bn_me_point", POINT_FIELDS), ("bn_me_job", JOB_FIELDS)):
        m = re.search(r"#\[repr\(C\)\][^{]*?pub struct %s\s*\{(.*?)\}" % name, src, flags=re.S)
        assert m and tuple(re.findall(r"pub (\w+)\s*:", m.group(1))) == fields
    h = _decls("binius_amd.h")
    assert re.search(r"pub const BN_ME_N: usize = 4;", src)
    assert re.search(r"pub const BN_ME_MAX_LO_VARS: u32 = 10;", src)
    assert re.search(r"pub const BN_ME_MAX_JOBS: u32 = %s;" % re.search(r"#define\s+BN_ME_MAX_JOBS\s+(\d+)", h).group(1), src)


def test_host_library_exports_and_python_binds_the_mirror(ffi):
    import binius_amd._host as h

    for symbol in HOST_SYMBOLS:
        assert hasattr(h.host_lib(), symbol)
    assert callable(getattr(h.EvalcheckEvaluatePlan, "run", None))
    split = int(re.search(r"#define\s+BNH_EVALCHECK_LO_SPLIT\s+(\d+)", _decls("binius_amd_host.h")).group(1))
    assert h.EvalcheckEvaluatePlan.LO_SPLIT == split <= 10

    class Col:
        def __init__(self, ptr):
            self.ptr = ptr

    a, b = Col(0x1000), Col(0x2000)
    # points over a pool of 40 coordinates, split at min(len // 2, split):
    #   P = [0, 12)   prefix [0, 6),   suffix [6, 12)
    #   Q = [20, 30)  prefix [20, 25), suffix [25, 30)
    #   R = [21, 30)  prefix [21, 25), suffix [25, 30) -- the suffix slice of Q
    #   S = [39, 40)  one coordinate: prefix [39, 39) (one element), suffix [39, 40)
    claims = [(a, 0, 12, 0, 12), (b, 0, 12, 0, 12), (a, 0, 12, 0, 12), (a, 3, 10, 20, 10), (b, 5, 9, 21, 9), (a, 7, 1, 39, 1)]
    assert split >= 6
    want = (64 + 64) + (32 + 32) + 16 + (1 + 2)
    assert h.EvalcheckEvaluatePlan.scratch_elems(claims) == want
    desc = (C.c_uint32 * (4 * len(claims)))(*[w for c in claims for w in c[1:5]])
    assert h.host_lib().bnh_evalcheck_evaluate_scratch_elems(len(claims), desc, 0) == want
    assert h.host_lib().bnh_evalcheck_evaluate_scratch_elems(len(claims), desc, split) == want
    # a smaller bound moves the split of the longer points: P at 4 -> 16 + 256, Q at 4 -> 16 + 64, R at 4 -> 16 + 32, S unchanged
    assert h.EvalcheckEvaluatePlan.scratch_elems(claims, lo_split=4) == (16 + 256) + (16 + 64) + (16 + 32) + (1 + 2)
    assert h.host_lib().bnh_evalcheck_evaluate_scratch_elems(len(claims), desc, 4) == (16 + 256) + (16 + 64) + (16 + 32) + (1 + 2)
    assert h.host_lib().bnh_evalcheck_evaluate_scratch_elems(len(claims), desc, 11) == 0
