"""The ring switch at the boundary (CPU only): include/binius_amd.h declares bn_ring_switch_eq_ind_batch, its job struct and
bn_ring_switch_counters with their enum, libbinius_amd.so exports them, the ctypes binding lists and exposes them, the Rust shim declares
them; include/binius_amd_host.h declares bnh_ring_switch_prove and its scratch formula, libbinius_amd_host.so exports them and
binius_amd._host binds them as RingSwitchPlan; the validation that needs no device rejects."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_ring_switch_eq_ind_batch": "ring_switch_eq_ind_batch", "bn_ring_switch_counters": "ring_switch_counters"}
HOST_SYMBOLS = ("bnh_ring_switch_prove", "bnh_ring_switch_scratch_elems")


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


def test_header_declares_the_job_and_the_counters():
    h = _decls("binius_amd.h")
    assert re.search(r"typedef struct\s*\{\s*const void \*d_query;\s*uint32_t n_vars;\s*uint32_t kappa;\s*bn_f128 mixing_coeff;\s*\}\s*bn_rs_job;", h)
    assert re.search(r"\bBN_RS_CALLS\s*=\s*0\b.*\bBN_RS_LAUNCHES\s*=\s*1\b.*\bBN_RS_JOBS\s*=\s*2\b.*\bBN_RS_QUERIES\s*=\s*3\b.*\bBN_RS_N\s*=\s*4\b", h)
    # the jobs travel as untyped memory (the layout of bn_rs_job), the coefficients from the host
    assert re.search(r"bn_ring_switch_eq_ind_batch\s*\(\s*bn_ctx \*ctx,\s*const void \*jobs,\s*uint32_t n_jobs,\s*const bn_f128 \*h_row_batch_coeffs,\s*"
                     r"uint32_t n_coeffs,\s*void \*const \*d_outs\s*\)", h)


@pytest.mark.parametrize("symbol", HOST_SYMBOLS)
def test_host_header_declares_the_prover(symbol):
    assert re.search(r"\b(int|uint64_t)\s+%s\s*\(" % symbol, _decls("binius_amd_host.h"))


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_library_exports_and_python_binds_the_op(ffi, symbol):
    L = ffi.lib()
    assert hasattr(L, symbol)
    assert symbol in ffi.ABI_SYMBOLS
    assert callable(getattr(ffi.Context, DEVICE_SYMBOLS[symbol], None))


def test_job_struct_layout(ffi):
    assert C.sizeof(ffi.RsJob) == 32
    assert [(n, getattr(ffi.RsJob, n).offset) for n, _t in ffi.RsJob._fields_] == [("d_query", 0), ("n_vars", 8), ("kappa", 12), ("mixing_coeff", 16)]


def test_host_library_exports_and_python_binds_the_prover(ffi):
    import binius_amd._host as h

    H = h.host_lib()
    for s in HOST_SYMBOLS:
        assert hasattr(H, s)
    assert callable(getattr(h.RingSwitchPlan, "run", None))
    assert h.RingSwitchPlan.PHASES == ("partial_evals", "tensor_algebra", "eq_inds")
    # one bit column of 12 variables claimed at one point: the 32-element suffix table, 128 partial evaluations, one 32-element transparent
    suffixes, claims = [(7, 5, 7)], [(0, 0, 0)]
    assert h.RingSwitchPlan.scratch_elems(suffixes, claims) == 32 + 128 + 32
    # four claims: a bit column (11 variables) at two suffixes, a byte column (10 variables) at one, and the bit column a second time at
    # its first suffix: tables 16 + 16 + 64, pairs 128 + 128 + 16 (the repeated pair once), transparents 16 + 16 + 64 + 16
    suffixes = [(7, 4, 7), (18, 4, 7), (4, 6, 4)]
    claims = [(0, 0, 0), (0, 1, 1), (1, 2, 2), (0, 0, 0)]
    want = (16 + 16 + 64) + (128 + 128 + 16) + (16 + 16 + 64 + 16)
    assert h.RingSwitchPlan.scratch_elems(suffixes, claims) == want
    sd = (C.c_uint32 * 9)(*[w for s in suffixes for w in s])
    cd = (C.c_uint32 * 12)(*[w for c in claims for w in c])
    assert H.bnh_ring_switch_scratch_elems(3, sd, 4, cd) == want
    assert H.bnh_ring_switch_scratch_elems(1, (C.c_uint32 * 3)(7, 5, 7), 1, (C.c_uint32 * 3)(0, 0, 0)) == 32 + 128 + 32


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_rust_shim_declares_the_op(symbol):
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % symbol, src)
    assert re.search(r"pub const BN_RS_N: usize = 4;", src)
    assert re.search(r"pub struct bn_rs_job\s*\{\s*pub d_query: \*const c_void,\s*pub n_vars: u32,\s*pub kappa: u32,\s*pub mixing_coeff: bn_f128,\s*\}", src)


def test_validation_without_a_device(ffi):
    """A null context is rejected by both entry points before anything else is looked at; so is a prover call without a context."""
    import binius_amd._host as h

    L = ffi.lib()
    one = (ffi.F128 * 2)()
    outs = (C.c_void_p * 1)()
    assert L.bn_ring_switch_eq_ind_batch(None, None, 1, one, 1, outs) == ffi.BN_ERR_INPUT_VALIDATION
    assert b"null ctx" in L.bn_last_error()
    assert L.bn_ring_switch_counters(None, (C.c_uint64 * 4)()) == ffi.BN_ERR_INPUT_VALIDATION
    H = h.host_lib()
    u32, f, vp = (C.c_uint32 * 4)(0, 12, 0, 0), (ffi.F128 * 16)(), (C.c_void_p * 1)()
    assert H.bnh_ring_switch_prove(None, 1, vp, u32, f, 16, 1, u32, 1, u32, 1, u32, f, 0, f, 7, None, 0, f, f, vp, None) == ffi.BN_ERR_INPUT_VALIDATION
    assert b"null argument" in H.bnh_last_error()


def test_binding_checks_the_shapes_it_can(ffi):
    class Ctx:  # (no device: the checks below run before the library is entered)
        _h = None

    q, o = ffi.DevSlice(0x1000, 16), ffi.DevSlice(0x2000, 16)
    with pytest.raises(ffi.BnError) as e:
        ffi.Context.ring_switch_eq_ind_batch(Ctx(), [(q, 4, 7, 1)], [0] * 128, [])
    assert e.value.kind == "InputValidation"
    with pytest.raises(ffi.BnError) as e:
        ffi.Context.ring_switch_eq_ind_batch(Ctx(), [(q, 4, 7, 1)], [0] * 128, [ffi.DevSlice(0x2000, 8)])
    assert e.value.kind == "InputValidation"
    with pytest.raises(ffi.BnError) as e:
        ffi.Context.ring_switch_eq_ind_batch(Ctx(), [(ffi.DevSlice(0x1000, 8), 4, 7, 1)], [0] * 128, [o])
    assert e.value.kind == "InputValidation"
