"""A batch of tower-typed expressions and the batched compute plan at the boundary (CPU only): include/binius_amd.h declares
bn_expr_compile_tower_batch and bn_compute_composite_batch_counters, libbinius_amd.so exports them, the ctypes binding lists and exposes
them, the Rust shim declares them and the constants agree; neither takes device memory, bn_compute_composite's prototype is what it was
and BN_CC_N is still 4; include/binius_amd_host.h declares bnh_witness_compute_batched with bnh_witness_compute's parameter list,
libbinius_amd_host.so exports it and binius_amd._host binds it in WitnessComputeBatched.  The plan of a batch runs here too, on the CPU:
tests/cpp/compose_batch_check walks every unit of the grid that binius_amd/csrc/compose_batch.hpp lays out."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = {"bn_expr_compile_tower_batch": "expr_compile_tower_batch", "bn_compute_composite_batch_counters": "compute_composite_batch_counters"}
COUNTERS = ("CALLS", "LAUNCHES", "JOBS", "PROGRAMS")
COMPUTE_COMPOSITE = "bn_ctx *ctx, const void *const *d_rows, uint32_t n_rows, uint64_t row_len, void *d_out, uint64_t out_len, const bn_expr *expr"


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g

    g.build()
    import binius_amd._ffi as f

    return f


def _decls(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _params(header, symbol):
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % symbol, _decls(header), flags=re.S)
    assert m, symbol
    return " ".join(m.group(1).split())


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_both_sides_declare_export_and_bind(ffi, symbol):
    assert re.search(r"\bint\s+%s\s*\(" % symbol, _decls("binius_amd.h"))
    assert hasattr(ffi.lib(), symbol)
    assert symbol in ffi.ABI_SYMBOLS
    assert callable(getattr(ffi.Context, DEVICE_SYMBOLS[symbol], None))
    assert callable(getattr(ffi.Context, "compute_composite_tower_batch", None))
    src = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % symbol, src)
    lib_rs = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "lib.rs")).read()
    assert "pub fn compile_expr_tower_batch" in lib_rs and "ffi::bn_expr_compile_tower_batch" in lib_rs
    layer = open(os.path.join(ROOT, "binius_amd", "host", "compute_layer.hpp")).read()
    assert "compile_expr_tower_batch" in layer and "bn_expr_compile_tower_batch(" in layer


def test_the_new_entry_points_take_no_device_memory(ffi):
    """(tests/test_gpu_deferred_visibility.py lists every entry point that does; the batch runs behind bn_compute_composite, which is in
    its table B, so these two must not be among them)"""
    for symbol in DEVICE_SYMBOLS:
        args = _params("binius_amd.h", symbol)
        assert not re.search(r"\bd_\w+", args) and "void" not in args, args


def test_existing_prototypes_and_counters_are_unchanged(ffi):
    assert _params("binius_amd.h", "bn_compute_composite") == COMPUTE_COMPOSITE
    h = open(os.path.join(ROOT, "include", "binius_amd.h")).read()
    rust = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert re.search(r"\bBN_CC_N\s*=\s*4\b", h) and ffi.BN_CC_N == 4 and re.search(r"pub const BN_CC_N: usize = 4;", rust)
    assert _params("binius_amd.h", "bn_expr_compile_tower") == \
        "bn_ctx *ctx, const bn_step *steps, uint64_t n_steps, const uint32_t *input_levels, uint32_t n_inputs, uint32_t out_level, bn_expr **out"


def test_constants_and_the_job_record_agree(ffi):
    h = open(os.path.join(ROOT, "include", "binius_amd.h")).read()
    rust = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    cap = int(re.search(r"#define BN_COMPOSE_BATCH_MAX_JOBS (\d+)\b", h).group(1))
    assert cap >= 1024 and ffi.BN_COMPOSE_BATCH_MAX_JOBS == cap and re.search(r"pub const BN_COMPOSE_BATCH_MAX_JOBS: usize = %d;" % cap, rust)
    for i, name in enumerate(COUNTERS):
        assert re.search(r"\bBN_CCB_%s\s*=\s*%d\b" % (name, i), h) and getattr(ffi, "BN_CCB_" + name) == i
        assert re.search(r"pub const BN_CCB_%s: usize = %d;" % (name, i), rust)
    assert re.search(r"\bBN_CCB_N\s*=\s*4\b", h) and ffi.BN_CCB_N == 4 and re.search(r"pub const BN_CCB_N: usize = 4;", rust)
    assert re.search(r"#define BN_COMPOSE_JOB_DESC_WORDS 4\b", h) and ffi.BN_COMPOSE_JOB_DESC_WORDS == 4 and re.search(r"pub const BN_COMPOSE_JOB_DESC_WORDS: usize = 4;", rust)
    # bn_compose_job (the planner's and the wrappers' record): the header's fields in order, the Rust struct's the same; the first four are
    # job_desc's words, the fifth is out_offsets' entry
    body = re.search(r"typedef struct \{([^}]*)\} bn_compose_job;", _decls("binius_amd.h")).group(1)
    fields = re.findall(r"(uint32_t|uint64_t)\s+(\w+)\s*;", body)
    assert fields == [("uint32_t", "expr"), ("uint32_t", "first_row"), ("uint32_t", "n_vars"), ("uint32_t", "reserved"), ("uint64_t", "out_offset")]
    rs = re.search(r"pub struct bn_compose_job \{([^}]*)\}", rust).group(1)
    assert re.findall(r"pub (\w+): (u32|u64),", rs) == [(n, "u32" if t == "uint32_t" else "u64") for t, n in fields]
    assert _params("binius_amd.h", "bn_expr_compile_tower_batch") == \
        "bn_ctx *ctx, const bn_expr *const *exprs, uint32_t n_exprs, const uint32_t *job_desc, const uint64_t *out_offsets, uint32_t n_jobs, bn_expr **out"


def test_host_library_exports_and_python_binds_the_batched_plan(ffi):
    import binius_amd._host as h

    ffi.lib()
    assert re.search(r"\bint\s+bnh_witness_compute_batched\s*\(", _decls("binius_amd_host.h"))
    fn = h.host_lib().bnh_witness_compute_batched
    assert _params("binius_amd_host.h", "bnh_witness_compute_batched") == _params("binius_amd_host.h", "bnh_witness_compute")
    assert list(fn.argtypes) == list(h.host_lib().bnh_witness_compute.argtypes)
    W, B = h.WitnessCompute, h.WitnessComputeBatched
    assert issubclass(B, W) and B.KINDS == W.KINDS
    assert (W._RUN, B._RUN) == ("bnh_witness_compute", "bnh_witness_compute_batched") and B._SCRATCH == W._SCRATCH == "bnh_witness_compute_scratch_elems"


def test_the_plan_of_a_batch_on_the_cpu(ffi):
    """binius_amd/csrc/compose_batch.hpp -- what bn_expr_compile_tower_batch and the batch route of bn_compute_composite plan -- with every
    unit of the grid walked as the kernel walks it, each job against its program alone, guards between the outputs, and every rejection
    with its reason (tests/cpp/compose_batch_check.cpp)."""
    exe = os.path.join(ROOT, "tests", "cpp", "compose_batch_check")
    assert os.path.exists(exe), "tests/cpp/compose_batch_check missing -- run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and re.search(r"compose_batch_check ok: \d+ cases", r.stdout), r.stdout[-2000:] + r.stderr[-2000:]
